// Per-point arithmetic of the sampler (include/unidepth_hip.h, UdRemap / UdOverlapMask): coordinate -> tap indices and weights, the
// clamps, the inside test, the combination of the taps and the overlap-mask decision.  Plain float functions with no device intrinsics
// and no kernel: remap.hip compiles them into its two kernels, tests/remap_host/remap_host.cpp compiles the same header for the host,
// under the sanitizers, to check the arithmetic and the indices without a GPU.
//
// SAFETY RULE: a coordinate never becomes an address before it has been made safe.  Every float that is converted to int has passed a
// clamp written as `x >= lo ? (x <= hi ? x : hi) : lo`, which sends NaN to `lo` and +-inf / +-1e30 to the ends, so the conversion is
// always of an in-range value (an out-of-range float-to-int conversion is undefined on the host).  Every operation rounds separately
// (build with -ffp-contract=off), as the numpy fp32 restatement in tools/make_golden_remap.py.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define UD_RM_FN __host__ __device__ __forceinline__
#else
#define UD_RM_FN static inline
#endif
#pragma clang fp contract(off)

#define UD_RM_NEAREST 0
#define UD_RM_BILINEAR 1
#define UD_RM_ZEROS 0
#define UD_RM_BORDER 1

// NaN -> lo
UD_RM_FN float ud_rm_clamp(float x, float lo, float hi) { return x >= lo ? (x <= hi ? x : hi) : lo; }

// One axis: index-space position p = coordinate - 0.5 in an axis of `size` source pixels -> the two taps i0, i0 + 1 (i0 alone for
// nearest: w1 = 0) and their weights.  zeros: p is clamped to [-2, size + 1] first, which changes nothing for a position with a tap
// in range and keeps both taps out of range for the others.  border: p is clamped to [0, size - 1].
UD_RM_FN void ud_rm_axis(float coord, int size, int mode, int padding, int* i0, float* w0, float* w1) {
  const float p = coord - 0.5f;
  const float q = padding == UD_RM_BORDER ? ud_rm_clamp(p, 0.0f, (float)(size - 1)) : ud_rm_clamp(p, -2.0f, (float)(size + 1));
  if (mode == UD_RM_NEAREST) {
    *i0 = (int)rintf(q);                              // round half to even: grid_sample's nearbyint
    *w0 = 1.0f; *w1 = 0.0f;
  } else {
    const float f = floorf(q);
    *i0 = (int)f;
    *w1 = q - f;
    *w0 = 1.0f - *w1;
  }
}

// finite and inside the closed image rectangle: 0 <= u <= Ws and 0 <= v <= Hs (false for NaN and +-inf)
UD_RM_FN bool ud_rm_inside(float u, float v, int Ws, int Hs) { return u >= 0.0f && u <= (float)Ws && v >= 0.0f && v <= (float)Hs; }

UD_RM_FN bool ud_rm_finite(float u, float v) { return fabsf(u) <= 3.402823466e38f && fabsf(v) <= 3.402823466e38f; }

// The taps of one point: off[k] = y * Ws + x of tap k (k = 2 * row + column), or -1 where the tap is out of range (or, later, masked);
// wx / wy the weights of column / row 0 and 1.
struct UdRmTaps {
  int off[4];
  float wx[2], wy[2];
};

UD_RM_FN void ud_rm_taps(float u, float v, int Ws, int Hs, int mode, int padding, UdRmTaps* t) {
  int x0, y0;
  ud_rm_axis(u, Ws, mode, padding, &x0, &t->wx[0], &t->wx[1]);
  ud_rm_axis(v, Hs, mode, padding, &y0, &t->wy[0], &t->wy[1]);
  const int n = mode == UD_RM_NEAREST ? 1 : 2;
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 2; ++c) {
      const int x = x0 + c, y = y0 + r;
      t->off[2 * r + c] = (r < n && c < n && x >= 0 && x < Ws && y >= 0 && y < Hs) ? y * Ws + x : -1;
    }
}

// at least one remaining tap has a non-zero weight
UD_RM_FN bool ud_rm_any(const UdRmTaps& t) {
  bool any = false;
  for (int k = 0; k < 4; ++k) any = any || (t.off[k] >= 0 && t.wx[k & 1] != 0.0f && t.wy[k >> 1] != 0.0f);
  return any;
}

// t0 = v00*hx + v01*lx, t1 = v10*hx + v11*lx, out = t0*hy + t1*ly (mg_kernel's order, csrc/matchgt.hip); val[k] is 0 for a tap that
// does not contribute
UD_RM_FN float ud_rm_blend(const UdRmTaps& t, const float* val) {
  const float t0 = val[0] * t.wx[0] + val[1] * t.wx[1];
  const float t1 = val[2] * t.wx[0] + val[3] * t.wx[1];
  return t0 * t.wy[0] + t1 * t.wy[1];
}

// the same expression on 1 for the contributing taps: the weight sum the normalised form divides by
UD_RM_FN float ud_rm_weight_sum(const UdRmTaps& t) {
  float one[4];
  for (int k = 0; k < 4; ++k) one[k] = t.off[k] >= 0 ? 1.0f : 0.0f;
  return ud_rm_blend(t, one);
}

// value of one channel from its four tap values (0 where off[k] < 0)
UD_RM_FN float ud_rm_value(const UdRmTaps& t, const float* val, int mode, int normalize, float wsum) {
  if (mode == UD_RM_NEAREST) return val[0];           // the source's bits
  const float s = ud_rm_blend(t, val);
  if (!normalize) return s;
  return wsum > 0.0f ? s / wsum : 0.0f;
}

// round half to even, clamp to [0, 255]: torch's .round().clamp(0, 255); NaN -> 0
UD_RM_FN unsigned char ud_rm_to_u8(float x) { return (unsigned char)(int)ud_rm_clamp(rintf(x), 0.0f, 255.0f); }

UD_RM_FN float ud_rm_load(const float* p) { return *p; }
UD_RM_FN float ud_rm_load(const unsigned char* p) { return (float)*p; }
UD_RM_FN void ud_rm_store(float* p, float x) { *p = x; }
UD_RM_FN void ud_rm_store(unsigned char* p, float x) { *p = ud_rm_to_u8(x); }

// What one thread of ud_remap does, for point i of image b.  Strides in elements; src / mask of one image hold C * Hs * Ws / Hs * Ws
// elements, src_bs / mask_bs are 0 for a batch of 1.
template <typename S, typename O>
struct UdRmArgs {
  const S* src; const unsigned char* src_mask; const float* uv; const unsigned char* coord_valid;
  O* out; unsigned char* valid;
  long long bs, ps, cs, n, src_bs, mask_bs;
  int C, Hs, Ws, mode, padding, normalize, out_rows;
};

template <typename S, typename O>
UD_RM_FN void ud_rm_point(const UdRmArgs<S, O>& a, int b, long long i) {
  const float* s = a.uv + b * a.bs + i * a.ps;
  const float u = s[0], v = s[a.cs];
  const size_t n = (size_t)a.n, at = (size_t)b * n + (size_t)i, hw = (size_t)a.Hs * (size_t)a.Ws;
  // a point whose coord_valid is 0 or whose coordinates are not finite samples nothing: value 0, valid 0
  const bool live = (a.coord_valid ? a.coord_valid[at] != 0 : true) && ud_rm_finite(u, v);
  UdRmTaps t;
  ud_rm_taps(u, v, a.Ws, a.Hs, a.mode, a.padding, &t);
  if (a.src_mask) {
    const unsigned char* m = a.src_mask + (size_t)b * (size_t)a.mask_bs;
    for (int k = 0; k < 4; ++k)
      if (t.off[k] >= 0 && m[t.off[k]] == 0) t.off[k] = -1;
  }
  const float wsum = (a.normalize && a.mode == UD_RM_BILINEAR) ? ud_rm_weight_sum(t) : 1.0f;
  const S* img = a.src + (size_t)b * (size_t)a.src_bs;
  O* q = a.out_rows ? a.out + at * (size_t)a.C : a.out + (size_t)b * (size_t)a.C * n + (size_t)i;
  const size_t qs = a.out_rows ? 1 : n;
  for (int c = 0; c < a.C; ++c) {
    float x = 0.0f;
    if (live) {
      float val[4];
      for (int k = 0; k < 4; ++k) val[k] = t.off[k] >= 0 ? ud_rm_load(img + (size_t)c * hw + (size_t)t.off[k]) : 0.0f;
      x = ud_rm_value(t, val, a.mode, a.normalize, wsum);
    }
    ud_rm_store(q + (size_t)c * qs, x);
  }
  if (a.valid) a.valid[at] = (live && ud_rm_inside(u, v, a.Ws, a.Hs) && ud_rm_any(t) && wsum > 0.0f) ? 1 : 0;
}

// ---- the overlap mask: the reference's Camera.mask_overlap_projection (unidepth/utils/camera.py:132-154) at one pixel -----------------

// grid_sample's position along one axis of `size` pixels for the flow f at identity coordinate id, border-clamped: steps 1 - 4
UD_RM_FN float ud_ov_position(float f, float id, int size) {
  const float s = 0.1f * f + id;
  const float g = s / (float)(size - 1) * 2.0f - 1.0f;
  const float ix = ((g + 1.0f) * (float)size - 1.0f) / 2.0f;
  return ud_rm_clamp(ix, 0.0f, (float)(size - 1));      // NaN -> tap 0
}

// uv planar [2, H, W] of one image; pixel (x, y), 0 <= x < W, 0 <= y < H, H, W >= 2
UD_RM_FN bool ud_ov_pixel(const float* uv, int x, int y, int H, int W) {
  const size_t hw = (size_t)H * (size_t)W;
  const float idx = (float)x + 0.5f, idy = (float)y + 0.5f;
  const float fu = uv[(size_t)y * W + x] - idx, fv = uv[hw + (size_t)y * W + x] - idy;
  const float ix = ud_ov_position(fu, idx, W), iy = ud_ov_position(fv, idy, H);
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0;               // in [0, W - 1], [0, H - 1] after the clamp
  const float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
  // nw, ne, sw, se as torch's CPU kernel forms them
  const float w[4] = {(fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0), (ix - fx0) * (iy - fy0)};
  float a = 0.0f, b = 0.0f;
  for (int k = 0; k < 4; ++k) {
    const int tx = x0 + (k & 1), ty = y0 + (k >> 1);
    float tu = 0.0f, tv = 0.0f;                         // a tap past the border (weight 0 there) adds nothing
    if (tx < W && ty < H) {
      tu = uv[(size_t)ty * W + tx] - ((float)tx + 0.5f);
      tv = uv[hw + (size_t)ty * W + tx] - ((float)ty + 0.5f);
    }
    if (k == 0) {
      a = w[0] * tu; b = w[0] * tv;
    } else {
      a = a + w[k] * tu; b = b + w[k] * tv;
    }
  }
  const float nf = sqrtf(fu * fu + fv * fv), ns = sqrtf(a * a + b * b);
  return (0.9f * nf < ns) || (nf < 1.0f);
}
