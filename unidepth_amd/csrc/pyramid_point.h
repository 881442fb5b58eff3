// Per-pixel arithmetic of the depth pyramid (include/unidepth_hip.h, UdDepthPyramid): what one thread of pyramid.hip's kernel does for a
// pixel of level 0 and for a 2 x 2 block of every coarser level.  Plain functions with no device intrinsics, no libm call and no kernel, so
// that tests/pyramid_host/pyramid_host.cpp compiles the same header for the host, under the sanitizers, and a numpy fp32 restatement
// (tests/pyramid_common.py) has its bits.
//
// THE DEFINITION (every operation below is one separately rounded fp32 operation, in the order written; -ffp-contract=off):
//   live(q)   = mask[q] != 0 && 0 < depth[q] < +inf  (with weights: && 0 < w[q] < +inf); every comparison is false for a NaN
//   staged(q) = live(q) ? depth[q] : 0, and 0 outside the image: a tap is used where staged > 0
//   level 0, radius 0:   out = staged(c)
//   level 0, radius r:   0 where the centre is not live, else with dc = staged(c), num = den = 0 and the taps dy = -r..r (outer),
//                        dx = -r..r (inner) that are used, d = staged(c + (dy, dx)):
//                            delta = |d - dc|;  t = delta * inv_bin;  bin = t >= NB ? NB - 1 : (int)t      (compared in float first)
//                            w = ws[(dy + r) * (2 r + 1) + dx + r] * wr[bin];  num = num + w * d;  den = den + w
//                        out = num / den       (den > 0: the centre tap has delta 0, bin 0 and the tables' ws[centre] * wr[0] > 0)
//   level 0 weight:      the centre's weight where live, else 0
//   level l >= 1:        members m0 = (2y, 2x), m1 = (2y, 2x + 1), m2 = (2y + 1, 2x), m3 = (2y + 1, 2x + 1) of level l - 1, live where
//                        their value there is > 0; anchor = the smallest live value (a running `d < anchor`, in member order);
//                        included = live && d - anchor <= gate; sum = the included values added in member order starting from the first
//                        included one, n = their count; value = sum / (float)n, weight = (the same sum of the weights) / (float)n; both
//                        0 when no member is live.
//
// SAFETY RULE: nothing here forms an address from data but wr[bin] with 0 <= bin <= NB - 1; the tile indices come from the caller, who
// keeps the r-pixel halo inside the staged tile.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define UD_PY_FN __host__ __device__ __forceinline__
#else
#define UD_PY_FN static inline
#endif
#pragma clang fp contract(off)

#define UD_PY_NB 256            /* bins of the range table */
#define UD_PY_MAX_R 4
#define UD_PY_MAX_LEVELS 4

// 0 < v < +inf, false for a NaN
UD_PY_FN bool ud_py_pos_finite(float v) { return v > 0.0f && v <= 3.402823466e+38f; }

// the value a pixel is staged with: its depth where live, 0 where not
UD_PY_FN float ud_py_stage(float d, bool masked_in, bool has_w, float w) {
  const bool live = masked_in && ud_py_pos_finite(d) && (!has_w || ud_py_pos_finite(w));
  return live ? d : 0.0f;
}

UD_PY_FN int ud_py_bin(float delta, float inv_bin) {
  const float t = delta * inv_bin;
  return t >= (float)UD_PY_NB ? UD_PY_NB - 1 : (int)t;
}

// Level 0 at a live centre with r >= 1.  tile: staged values, row stride `stride`; jc: the centre's index there, with r staged pixels on
// every side of it.  ws [(2r+1)^2], wr [NB].
UD_PY_FN float ud_py_filter(const float* tile, int stride, int jc, int r, const float* ws, const float* wr, float inv_bin) {
  const float dc = tile[jc];
  const int k = 2 * r + 1;
  float num = 0.0f, den = 0.0f;
  for (int dy = -r; dy <= r; ++dy) {
    for (int dx = -r; dx <= r; ++dx) {
      const float d = tile[jc + dy * stride + dx];
      if (!(d > 0.0f)) continue;
      float delta = d - dc;
      delta = delta < 0.0f ? -delta : delta;
      const float w = ws[(dy + r) * k + (dx + r)] * wr[ud_py_bin(delta, inv_bin)];
      num = num + w * d;
      den = den + w;
    }
  }
  return num / den;
}

// One 2 x 2 block: d[4], w[4] (w read only with has_w) in member order -> value and weight of the coarser pixel.
UD_PY_FN void ud_py_reduce(const float* d, const float* w, bool has_w, float gate, float* value, float* weight) {
  bool any = false;
  float anchor = 0.0f;
  for (int k = 0; k < 4; ++k) {
    if (!(d[k] > 0.0f)) continue;
    if (!any || d[k] < anchor) anchor = d[k];
    any = true;
  }
  *value = 0.0f;
  *weight = 0.0f;
  if (!any) return;
  float sum = 0.0f, wsum = 0.0f;
  int n = 0;
  for (int k = 0; k < 4; ++k) {
    if (!(d[k] > 0.0f) || !(d[k] - anchor <= gate)) continue;
    sum = n ? sum + d[k] : d[k];
    if (has_w) wsum = n ? wsum + w[k] : w[k];
    ++n;
  }
  if (!n) return;                                   // only an infinite anchor with an infinite member: inf - inf is a NaN
  const float fn = (float)n;
  *value = sum / fn;
  if (has_w) *weight = wsum / fn;
}
