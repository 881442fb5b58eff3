// Per-pixel arithmetic of backward warping (include/unidepth_hip.h, UdWarpCamera): what one thread of warp.hip's kernel does for
// destination pixel i of image b -- the point of the pixel (loaded, or unprojected from a depth through the destination camera), the rigid
// motion, the projection through the source camera, the sample of the source and the optional visibility test.  A plain function with no
// device intrinsics and no kernel: it composes the per-point functions of camera_models.h and remap_taps.h and changes none of them, so
// every output has the bits of ud_camera_unproject -> ud_camera_project -> ud_remap run one after the other.  warp.hip compiles it into
// its kernel; tests/warp_host/warp_host.cpp compiles the same header for the host, under the sanitizers.
//
// SAFETY RULE: remap_taps.h's, unchanged -- no float becomes an index before its clamp.  The only indices formed here are the pixel's own
// (i < n, checked by the caller) and the tap offsets ud_rm_taps returned.  Every operation rounds separately (-ffp-contract=off).
#pragma once
#include "camera_models.h"
#include "remap_taps.h"
#pragma clang fp contract(off)

// Strides in elements: src / src_mask / src_depth of one image hold C * Hs * Ws / Hs * Ws / Hs * Ws elements, src_bs / mask_bs / sdepth_bs
// are 0 for a batch of 1.  Exactly one of points (planar [B,3,n]) and depth ([B,n], with params_dst) is set; n = Ho * Wo.
template <typename S, typename O>
struct UdWpArgs {
  const S* src; const unsigned char* src_mask; const float* src_depth;
  const float* points; const float* depth; const float* params_dst; const float* params_src; const float* T;
  const unsigned char* valid_in;
  O* out; unsigned char* valid; unsigned char* visible; float* uv; float* proj_depth;
  long long n, src_bs, mask_bs, sdepth_bs;
  float tol;
  int C, Wo, Hs, Ws, nT, mode, padding, normalize;
};

// model_dst is read in the depth form only and is one of the closed-form models there (Pinhole, EUCM, Spherical, MEI)
template <typename S, typename O>
UD_RM_FN void ud_wp_point(const UdWpArgs<S, O>& a, int model_dst, int model_src, int b, long long i) {
  const size_t n = (size_t)a.n, at = (size_t)b * n + (size_t)i, hw = (size_t)a.Hs * (size_t)a.Ws;
  // a. the point of the pixel in the destination camera's frame
  float x, y, z;
  bool cv = a.valid_in ? a.valid_in[at] != 0 : true;
  if (a.points) {
    const float* s = a.points + (size_t)b * 3 * n + (size_t)i;
    x = s[0]; y = s[n]; z = s[2 * n];
  } else {                                             // the identity grid at pixel centres, as ud_camera_unproject forms it
    const int py = (int)i / a.Wo, px = (int)i - py * a.Wo;
    const float d = a.depth[at];
    float o[3];
    ud_cam_unproject_closed(model_dst, UD_UNPROJ_DEPTH, a.params_dst + (size_t)b * 16, (float)px + 0.5f, (float)py + 0.5f, d, o);
    x = o[0]; y = o[1]; z = o[2];
    cv = cv && d > 0.0f;                               // false for a NaN; the model's unprojection mask is deliberately not part of it
  }
  // b. the rigid motion, ud_camera_project's arithmetic
  if (a.T) ud_cam_move(a.T + (a.nT == 1 ? 0 : (size_t)b * 12), x, y, z);
  // c. the projection through the source camera
  float u, v;
  ud_cam_project(model_src, a.params_src + (size_t)b * 16, x, y, z, &u, &v);
  const float dproj = ud_cam_depth(model_src, x, y, z);
  // d. coordinate validity
  cv = cv && ud_cam_inside(model_src, u, v, z, a.Hs, a.Ws) && dproj > 0.0f;
  if (a.uv) {
    float* q = a.uv + (size_t)b * 2 * n + (size_t)i;
    q[0] = u; q[n] = v;
  }
  if (a.proj_depth) a.proj_depth[at] = dproj;
  // e. the sample of src: ud_rm_point's body with (u, v) and cv in place of the loaded coordinate and coord_valid
  const bool live = cv && ud_rm_finite(u, v);
  UdRmTaps t;
  ud_rm_taps(u, v, a.Ws, a.Hs, a.mode, a.padding, &t);
  if (a.src_mask) {
    const unsigned char* m = a.src_mask + (size_t)b * (size_t)a.mask_bs;
    for (int k = 0; k < 4; ++k)
      if (t.off[k] >= 0 && m[t.off[k]] == 0) t.off[k] = -1;
  }
  const float wsum = (a.normalize && a.mode == UD_RM_BILINEAR) ? ud_rm_weight_sum(t) : 1.0f;
  const S* img = a.src + (size_t)b * (size_t)a.src_bs;
  O* q = a.out + (size_t)b * (size_t)a.C * n + (size_t)i;
  for (int c = 0; c < a.C; ++c) {
    float r = 0.0f;
    if (live) {
      float val[4];
      for (int k = 0; k < 4; ++k) val[k] = t.off[k] >= 0 ? ud_rm_load(img + (size_t)c * hw + (size_t)t.off[k]) : 0.0f;
      r = ud_rm_value(t, val, a.mode, a.normalize, wsum);
    }
    ud_rm_store(q + (size_t)c * n, r);
  }
  const bool in_image = ud_rm_inside(u, v, a.Ws, a.Hs);
  if (a.valid) a.valid[at] = (live && in_image && ud_rm_any(t) && wsum > 0.0f) ? 1 : 0;
  // f. visibility: src_depth at the same taps, those of a depth <= 0 (or NaN) dropped, the normalised form; then the relative test
  if (a.visible) {
    const float* sd = a.src_depth + (size_t)b * (size_t)a.sdepth_bs;
    float val[4];
    for (int k = 0; k < 4; ++k) {
      val[k] = t.off[k] >= 0 ? sd[t.off[k]] : 0.0f;
      if (!(val[k] > 0.0f)) {
        t.off[k] = -1; val[k] = 0.0f;
      }
    }
    const float dsum = a.mode == UD_RM_BILINEAR ? ud_rm_weight_sum(t) : 1.0f;
    const float ds = live ? ud_rm_value(t, val, a.mode, 1, dsum) : 0.0f;
    const bool dvalid = live && in_image && ud_rm_any(t) && dsum > 0.0f;
    const float diff = fabsf(ds - dproj), bar = a.tol * dproj;
    a.visible[at] = (dvalid && diff <= bar) ? 1 : 0;
  }
}
