// Network-resolution maps of a batch brought to the ground truth's size (include/unidepth_hip.h, UdMatchGt): the device form of the
// reference's match_gt / match_intrinsics (unidepth/utils/misc.py:596-690), which loop over the images in Python -- slice the padded
// window, F.interpolate(bilinear, align_corners=False) to the target window, F.pad with zeros, torch.cat -- once per map.
//
// ONE launch for up to UD_MATCH_MAX_PLANES maps of a batch whose images carry different paddings:
//   grid.z = image, grid.y = plane, grid.x = tiles of 4 rows x 64 quads over the plane's C * H2 destination rows
//   a thread owns 4 consecutive destination pixels of one row: the row's source rows and weights are computed once, the 4 columns'
//   indices and weights in registers, every tap loaded with a clamped index, the result leaves as one 16-byte store.  The quads are laid
//   over the row from its first 16-byte boundary, so an unaligned row (W2 % 4 != 0, offset views) has a scalar head and tail and a
//   vector body.  The per-image paddings are workgroup-uniform loads; no LDS, no atomics, no workspace, no host synchronisation.
// The arithmetic is ed_load's of csrc/evaldepth.hip applied to the window; built with -ffp-contract=off (csrc/build.sh), so every
// product and sum rounds on its own and a numpy fp32 restatement reproduces the bits (tools/make_golden_match_gt.py).
#include "ud_common.h"

namespace {

#pragma clang fp contract(off)

constexpr int MG_QUADS = 64;                 // quads (of 4 pixels) per tile row
constexpr int MG_ROWS = 4;                   // destination rows per tile
constexpr int MG_THREADS = MG_QUADS * MG_ROWS;

struct MgArgs {
  UdMatchPlane plane[UD_MATCH_MAX_PLANES];
  const int* pads1; const int* pads2;
  const float* K_in; float* K_out;
  int n_planes, h1, w1, H2, W2;
  int qblocks;                               // tiles along x
};

__device__ __forceinline__ int mg_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// source index pair and weights of destination index o (window-relative) along one axis of `n` source samples
__device__ __forceinline__ void mg_axis(int o, float scale, int n, int& i0, int& i1, float& hi, float& lo) {
  float f = scale * ((float)o + 0.5f) - 0.5f;
  f = f < 0.0f ? 0.0f : f;
  i0 = min((int)f, n - 1);
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  lo = fminf(fmaxf(f - (float)i0, 0.0f), 1.0f);
  hi = 1.0f - lo;
}

__global__ __launch_bounds__(MG_THREADS) void mg_kernel(const MgArgs a) {
  const int b = blockIdx.z;
  // paddings of image b, clamped so that both windows lie inside their allocations whatever the arrays hold
  int pl = 0, pr = 0, pt = 0, pb = 0, ql = 0, qr = 0, qt = 0, qb = 0;
  if (a.pads1) {
    const int* p = a.pads1 + (size_t)b * 4;
    pl = p[0]; pr = p[1]; pt = p[2]; pb = p[3];
  }
  if (a.pads2) {
    const int* p = a.pads2 + (size_t)b * 4;
    ql = p[0]; qr = p[1]; qt = p[2]; qb = p[3];
  }
  pl = mg_clampi(pl, 0, a.w1 - 1); pr = mg_clampi(pr, 0, a.w1 - 1 - pl);
  pt = mg_clampi(pt, 0, a.h1 - 1); pb = mg_clampi(pb, 0, a.h1 - 1 - pt);
  ql = mg_clampi(ql, 0, a.W2); qr = mg_clampi(qr, 0, a.W2 - ql);
  qt = mg_clampi(qt, 0, a.H2); qb = mg_clampi(qb, 0, a.H2 - qt);
  const int wu = a.w1 - pl - pr, hu = a.h1 - pt - pb;          // >= 1
  const int w2 = a.W2 - ql - qr, h2 = a.H2 - qt - qb;          // >= 0 (an empty window: the image is all border)

  if (a.K_in && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    const float* Ki = a.K_in + (size_t)b * 9;
    float* Ko = a.K_out + (size_t)b * 9;
    const float sx = (float)((double)w2 / (double)wu), sy = (float)((double)h2 / (double)hu);
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = Ki[i];
    const float cx = (k[2] - (float)pl) * sx, cy = (k[5] - (float)pt) * sy;
    k[0] = k[0] * sx;
    k[4] = k[4] * sy;
    k[2] = cx + (float)ql;
    k[5] = cy + (float)qt;
#pragma unroll
    for (int i = 0; i < 9; ++i) Ko[i] = k[i];
  }
  if ((int)blockIdx.y >= a.n_planes) return;
  const UdMatchPlane& P = a.plane[blockIdx.y];
  const int tx = threadIdx.x & (MG_QUADS - 1), ty = threadIdx.x / MG_QUADS;
  const int bx = blockIdx.x % a.qblocks, by = blockIdx.x / a.qblocks;
  const long long r = (long long)by * MG_ROWS + ty;            // destination row of the plane's [C * H2] rows of image b
  if (r >= (long long)P.C * a.H2) return;
  const int c = (int)(r / a.H2), y = (int)(r - (long long)c * a.H2);
  float* drow = P.dst + (((size_t)b * P.C + c) * a.H2 + y) * (size_t)a.W2;
  const int mis = (int)(((uintptr_t)drow >> 2) & 3);           // elements past the row's last 16-byte boundary
  const int xs = (bx * MG_QUADS + tx) * 4 - mis;                // first pixel of this thread's quad (>= -3)
  if (xs >= a.W2) return;

  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int oy = y - qt;
  if (oy >= 0 && oy < h2 && xs + 3 >= ql && xs < ql + w2) {
    const bool ident = hu == h2 && wu == w2;
    const float sy = (float)hu / (float)h2, sx = (float)wu / (float)w2;
    int y0, y1;
    float hy, ly;
    mg_axis(oy, sy, hu, y0, y1, hy, ly);
    if (ident) y0 = oy;
    const size_t plane_px = (size_t)a.h1 * a.w1;
    const float* S = P.src + (size_t)b * (size_t)P.src_batch_stride + (size_t)c * plane_px;
    const float* M = P.mul ? P.mul + (size_t)b * plane_px : nullptr;
    const size_t o0 = (size_t)(pt + y0) * a.w1 + pl, o1 = (size_t)(pt + y1) * a.w1 + pl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ox = xs + j - ql;
      if (ox < 0 || ox >= w2) continue;
      if (ident) {                                             // a bit copy of the window (of the rounded product with `mul`)
        v[j] = M ? S[o0 + ox] * M[o0 + ox] : S[o0 + ox];
        continue;
      }
      int x0, x1;
      float hx, lx;
      mg_axis(ox, sx, wu, x0, x1, hx, lx);
      float v00 = S[o0 + x0], v01 = S[o0 + x1], v10 = S[o1 + x0], v11 = S[o1 + x1];
      if (M) {
        v00 = v00 * M[o0 + x0]; v01 = v01 * M[o0 + x1]; v10 = v10 * M[o1 + x0]; v11 = v11 * M[o1 + x1];
      }
      const float t0 = v00 * hx + v01 * lx;
      const float t1 = v10 * hx + v11 * lx;
      v[j] = t0 * hy + t1 * ly;
    }
  }
  if (xs >= 0 && xs + 3 < a.W2) {
    *reinterpret_cast<f32x4*>(drow + xs) = (f32x4){v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (xs + j >= 0 && xs + j < a.W2) drow[xs + j] = v[j];
  }
}

}  // namespace

extern "C" int ud_match_gt(const UdMatchGt* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_match_gt: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdMatchGt& d = *desc;
  if (d.n_planes < 0 || d.n_planes > UD_MATCH_MAX_PLANES) {
    ud_set_error("ud_match_gt: 0 <= n_planes <= UD_MATCH_MAX_PLANES (4)");
    return UD_ERR_BAD_ARG;
  }
  if (d.B < 1 || d.B > 65535 || d.h1 < 1 || d.w1 < 1 || d.H2 < 1 || d.W2 < 1) {
    ud_set_error("ud_match_gt: bad sizes (1 <= B <= 65535, h1, w1, H2, W2 >= 1)");
    return UD_ERR_BAD_ARG;
  }
  if ((d.K_in == nullptr) != (d.K_out == nullptr)) {
    ud_set_error("ud_match_gt: K_in and K_out go together (null pointer)");
    return UD_ERR_BAD_ARG;
  }
  if (d.n_planes == 0 && !d.K_in) {
    ud_set_error("ud_match_gt: nothing to do (no planes and no intrinsics)");
    return UD_ERR_BAD_ARG;
  }
  MgArgs a;
  int maxC = 1;
  for (int i = 0; i < UD_MATCH_MAX_PLANES; ++i) a.plane[i] = UdMatchPlane{nullptr, nullptr, nullptr, 0, 0};
  for (int i = 0; i < d.n_planes; ++i) {
    const UdMatchPlane& p = d.planes[i];
    if (!p.src || !p.dst) {
      ud_set_error("ud_match_gt: null pointer (src or dst of a plane)");
      return UD_ERR_BAD_ARG;
    }
    if (p.C < 1 || p.src_batch_stride < 0 || (long long)p.C * d.H2 > 0x7fffffffLL || ((uintptr_t)p.dst & 3)) {
      ud_set_error("ud_match_gt: bad plane (C >= 1, C * H2 < 2^31, src_batch_stride >= 0, dst 4-byte aligned)");
      return UD_ERR_BAD_ARG;
    }
    a.plane[i] = p;
    maxC = p.C > maxC ? p.C : maxC;
  }
  a.pads1 = d.pads1; a.pads2 = d.pads2; a.K_in = d.K_in; a.K_out = d.K_out;
  a.n_planes = d.n_planes; a.h1 = d.h1; a.w1 = d.w1; a.H2 = d.H2; a.W2 = d.W2;
  // a row's quads start at its last 16-byte boundary: up to 3 pixels before the row
  a.qblocks = (int)((((long long)d.W2 + 3 + 3) / 4 + MG_QUADS - 1) / MG_QUADS);
  const long long rblocks = d.n_planes ? ((long long)maxC * d.H2 + MG_ROWS - 1) / MG_ROWS : 1;
  if (rblocks * a.qblocks > 0x7fffffffLL) {
    ud_set_error("ud_match_gt: bad sizes (too many tiles for one launch)");
    return UD_ERR_BAD_ARG;
  }
  const dim3 grid((unsigned)(d.n_planes ? rblocks * a.qblocks : 1), (unsigned)(d.n_planes ? d.n_planes : 1), (unsigned)d.B);
  hipLaunchKernelGGL(mg_kernel, grid, dim3(MG_THREADS), 0, (hipStream_t)stream, a);
  UD_CHECK_LAUNCH("ud_match_gt launch");
  return UD_OK;
}
