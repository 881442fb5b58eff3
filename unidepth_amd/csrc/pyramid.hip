// The depth pyramid of a batch in ONE launch (include/unidepth_hip.h, UdDepthPyramid): the bilateral filter of level 0 and the gated 2 x 2
// means of up to three coarser levels.  The arithmetic of a pixel is csrc/pyramid_point.h, which the host build of the tests runs under the
// sanitizers; the definition is written out there.
//
//   py_kernel<TW, TH>   a workgroup of 256 threads owns the aligned TW x TH tile of level 0 at (blockIdx.x, blockIdx.y) of image
//                       blockIdx.z; TW * TH = 1024, four pixels per thread, consecutive lanes on consecutive x.
//     1. stage: the tile's staged depth (0 where not live or outside the image) with an r-pixel halo into LDS, normals.hip's halo loop;
//        the tile's own weights (0 where not live) beside it; the range table wr (NB floats) into LDS as well.  One barrier.
//     2. level 0: every thread filters its four pixels from LDS (the taps of a wave are 64 consecutive floats of a row: no bank
//        conflict; wr[bin] is the one data-dependent LDS read; ws[tap] is uniform over the wave and comes through the scalar cache),
//        writes them to memory and keeps them in a second LDS tile.  One barrier.
//     3. level l = 1 .. L - 1: (TW >> l) x (TH >> l) blocks, one per thread, read from the LDS tile of level l - 1 and written to memory
//        and to the LDS tile of level l, one barrier per level.
//   Tiles are multiples of 2^(L-1) in both directions (L <= 4, TW, TH >= 16), so a block never crosses a tile and the result does not
//   depend on the tile shape.  A level whose output pointer is null is computed for the next one and not written.
//
// SAFETY RULE: a global index is formed only after 0 <= x < W_l and 0 <= y < H_l were checked for that level; LDS indices are bounded by
// the compile-time tile and the host-checked r <= 4.  H_l = H_{l-1} / 2 drops an odd last row, so every member of a block that is written
// lies inside level l - 1.
//
// No kernel synchronises with the host; the call captures into a graph.  Built with -ffp-contract=off: every operation rounds separately.
#include "ud_common.h"
#include "pyramid_point.h"
#pragma clang fp contract(off)

namespace {

constexpr int PY_THREADS = 256, PY_PIXELS = 1024;

struct PyArgs {
  const float* depth; const unsigned char* mask; const float* weights;
  const float* ws; const float* wr;
  float* out_d[UD_PY_MAX_LEVELS];
  float* out_w[UD_PY_MAX_LEVELS];
  float gate, inv_bin;
  int H, W, L, r;
};

template <int TW, int TH>
__global__ __launch_bounds__(PY_THREADS) void py_kernel(const PyArgs a) {
  static_assert(TW * TH == PY_PIXELS && TW % 16 == 0 && TH % 16 == 0, "tile");
  constexpr int HALO_MAX = (TW + 2 * UD_PY_MAX_R) * (TH + 2 * UD_PY_MAX_R);
  __shared__ float s_raw[HALO_MAX];                      // staged depth, tile + halo
  __shared__ float s_d[PY_PIXELS + PY_PIXELS / 4];       // level l at offset 0 (even l) or PY_PIXELS (odd l): ping-pong, l >= 2 fit in 256
  __shared__ float s_w[PY_PIXELS + PY_PIXELS / 4];
  __shared__ float s_wr[UD_PY_NB];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int H = a.H, W = a.W, r = a.r;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const size_t hw = (size_t)H * (size_t)W;
  const float* depth_b = a.depth + (size_t)b * hw;
  const unsigned char* mask_b = a.mask ? a.mask + (size_t)b * hw : nullptr;
  const float* w_b = a.weights ? a.weights + (size_t)b * hw : nullptr;
  const bool has_w = w_b != nullptr;
  const int hwid = TW + 2 * r, hhei = TH + 2 * r, halo = hwid * hhei;

  for (int j = tid; j < halo; j += PY_THREADS) {
    const int hy = j / hwid, hx = j - hy * hwid;
    const int ty = hy - r, tx = hx - r;
    const int gy = y0 + ty, gx = x0 + tx;
    float d = 0.0f, w = 0.0f;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t i = (size_t)gy * (size_t)W + (size_t)gx;
      w = has_w ? w_b[i] : 0.0f;
      d = ud_py_stage(depth_b[i], mask_b ? mask_b[i] != 0 : true, has_w, w);
    }
    s_raw[j] = d;
    if (has_w && tx >= 0 && tx < TW && ty >= 0 && ty < TH) s_w[ty * TW + tx] = d > 0.0f ? w : 0.0f;
  }
  if (r > 0) s_wr[tid] = a.wr[tid];                      // PY_THREADS == UD_PY_NB
  __syncthreads();

  // level 0
#pragma unroll
  for (int k = 0; k < PY_PIXELS / PY_THREADS; ++k) {
    const int p = k * PY_THREADS + tid;
    const int ty = p / TW, tx = p - ty * TW;
    const int jc = (ty + r) * hwid + tx + r;
    const float dc = s_raw[jc];
    float v = dc;
    if (r > 0 && dc > 0.0f) v = ud_py_filter(s_raw, hwid, jc, r, a.ws, s_wr, a.inv_bin);
    s_d[p] = v;
    const int gy = y0 + ty, gx = x0 + tx;
    if (gx < W && gy < H) {
      const size_t i = (size_t)b * hw + (size_t)gy * (size_t)W + (size_t)gx;
      if (a.out_d[0]) a.out_d[0][i] = v;
      if (has_w && a.out_w[0]) a.out_w[0][i] = s_w[p];
    }
  }

  // levels 1 .. L - 1
  int Hl = H, Wl = W;
  for (int l = 1; l < a.L; ++l) {
    __syncthreads();
    Hl >>= 1; Wl >>= 1;
    const int tw = TW >> l, th = TH >> l, pw = tw * 2;                  // pw: the row stride of level l - 1's tile
    const int src = (l & 1) ? 0 : PY_PIXELS, dst = (l & 1) ? PY_PIXELS : 0;
    const int xl0 = x0 >> l, yl0 = y0 >> l;
    if (tid < tw * th) {                                                // at most 256 blocks per tile
      const int ty = tid / tw, tx = tid - ty * tw;
      const int j = src + (2 * ty) * pw + 2 * tx;
      const float d[4] = {s_d[j], s_d[j + 1], s_d[j + pw], s_d[j + pw + 1]};
      float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (has_w) {
        w[0] = s_w[j]; w[1] = s_w[j + 1]; w[2] = s_w[j + pw]; w[3] = s_w[j + pw + 1];
      }
      float v, wv;
      ud_py_reduce(d, w, has_w, a.gate, &v, &wv);
      s_d[dst + tid] = v;
      if (has_w) s_w[dst + tid] = wv;
      const int gy = yl0 + ty, gx = xl0 + tx;
      if (gx < Wl && gy < Hl) {
        const size_t i = (size_t)b * (size_t)Hl * (size_t)Wl + (size_t)gy * (size_t)Wl + (size_t)gx;
        if (a.out_d[l]) a.out_d[l][i] = v;
        if (has_w && a.out_w[l]) a.out_w[l][i] = wv;
      }
    }
  }
}

}  // namespace

extern "C" int ud_depth_pyramid(const UdDepthPyramid* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_depth_pyramid: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdDepthPyramid& d = *desc;
  if (d.levels < 1 || d.levels > UD_PY_MAX_LEVELS) {
    ud_set_error("ud_depth_pyramid: levels must be 1 .. 4");
    return UD_ERR_BAD_ARG;
  }
  const int min_side = 1 << (d.levels - 1);
  if (d.B < 1 || d.B > UD_RECON_MAX_B || d.H < min_side || d.W < min_side || (long long)d.H * d.W >= UD_MAX_ELEMS) {
    ud_set_error("ud_depth_pyramid: bad sizes (1 <= B <= 256, H, W >= 2^(levels - 1), H * W < 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if (d.radius < 0 || d.radius > UD_PY_MAX_R) {
    ud_set_error("ud_depth_pyramid: radius must be 0 .. 4");
    return UD_ERR_BAD_ARG;
  }
  if (d.tile < 0 || d.tile > 2) {
    ud_set_error("ud_depth_pyramid: tile must be 0 (default), 1 (32 x 32) or 2 (64 x 16)");
    return UD_ERR_BAD_ARG;
  }
  const float gate = ud_f32_from_bits(d.gate_bits), inv_bin = ud_f32_from_bits(d.inv_bin_bits);
  if (!(gate >= 0.0f)) {
    ud_set_error("ud_depth_pyramid: gate must not be negative or a NaN (+inf is allowed)");
    return UD_ERR_BAD_ARG;
  }
  if (d.radius > 0 && !(inv_bin > 0.0f && inv_bin <= 3.402823466e38f)) {
    ud_set_error("ud_depth_pyramid: inv_bin must be finite and positive");
    return UD_ERR_BAD_ARG;
  }
  if (!d.depth || (d.radius > 0 && (!d.ws || !d.wr))) {
    ud_set_error("ud_depth_pyramid: null pointer (depth; ws and wr with a radius)");
    return UD_ERR_BAD_ARG;
  }
  const bool wide = d.tile == 2;
  const int TW = wide ? 64 : 32, TH = wide ? 16 : 32;
  const dim3 grid((unsigned)((d.W + TW - 1) / TW), (unsigned)((d.H + TH - 1) / TH), (unsigned)d.B);
  if (grid.y > 65535u) {
    ud_set_error("ud_depth_pyramid: bad sizes (H exceeds 65535 rows of tiles)");
    return UD_ERR_BAD_ARG;
  }
  PyArgs a;
  a.depth = d.depth; a.mask = d.mask; a.weights = d.weights; a.ws = d.ws; a.wr = d.wr;
  for (int l = 0; l < UD_PY_MAX_LEVELS; ++l) {
    a.out_d[l] = l < d.levels ? d.out_depth[l] : nullptr;
    a.out_w[l] = l < d.levels ? d.out_weights[l] : nullptr;
  }
  a.gate = gate; a.inv_bin = d.radius > 0 ? inv_bin : 0.0f;
  a.H = d.H; a.W = d.W; a.L = d.levels; a.r = d.radius;
  hipStream_t s = (hipStream_t)stream;
  if (wide) hipLaunchKernelGGL((py_kernel<64, 16>), grid, dim3(PY_THREADS), 0, s, a);
  else hipLaunchKernelGGL((py_kernel<32, 32>), grid, dim3(PY_THREADS), 0, s, a);
  UD_CHECK_LAUNCH("ud_depth_pyramid launch");
  return UD_OK;
}
