// Per-pixel arithmetic of the multi-view depth consistency check (include/unidepth_hip.h, UdDepthConsistency): what one thread of
// consistency.hip's kernel does for reference pixel i of image b -- the point of the pixel, computed ONCE, then for every neighbour view the
// forward-backward test: the point moved into the view and projected, the view's depth sampled there, that sample lifted through the view's
// camera, brought home and projected through the reference camera, and the two comparisons (pixels, relative depth); the count of agreeing
// views and the mean of the depths that agree.  A plain function with no device intrinsics and no kernel: it composes the per-point
// functions of camera_models.h and remap_taps.h and changes none of them, so every output has the bits of warp_camera -> unproject_camera
// -> project_camera and the element-wise arithmetic run one after the other.  consistency.hip compiles it into its kernel;
// tests/consistency_host/consistency_host.cpp compiles the same header for the host, under the sanitizers.
//
// SAFETY RULE: remap_taps.h's, unchanged -- no float becomes an index before its clamp.  The only indices formed here are the pixel's own
// (i < n, checked by the caller), the view's (v < V) and the tap offsets ud_rm_taps returned.  Every operation rounds separately
// (-ffp-contract=off).
#pragma once
#include "camera_models.h"
#include "remap_taps.h"
#pragma clang fp contract(off)

// depth [B,n], valid_in [B,n] (optional), params_ref [B,16]; src_depth / src_mask (optional) [B,V,Hs,Ws]; params_src [V,B,16]; T and Tinv
// [nT,V,3,4] with nT = 1 or B; fused [B,n], count / mask [B,n]; consistent / err_px / err_rel (each optional) [B,V,n].  n = H * W.
struct UdCsArgs {
  const float* depth; const float* params_ref; const unsigned char* valid_in;
  const float* src_depth; const unsigned char* src_mask; const float* params_src; const float* T; const float* Tinv;
  float* fused; unsigned char* count; unsigned char* mask; unsigned char* consistent; float* err_px; float* err_rel;
  long long n;
  float tol2, rel_tol;                                 // px_tol * px_tol, formed in fp32 by the caller
  int B, V, H, W, Hs, Ws, nT, min_views;
};

// model_ref and every model_src[v * B + b] are closed-form models (Pinhole, EUCM, Spherical, MEI)
UD_RM_FN void ud_cs_point(const UdCsArgs& a, int model_ref, const unsigned char* model_src, int b, long long i) {
  const size_t n = (size_t)a.n, at = (size_t)b * n + (size_t)i, hw = (size_t)a.Hs * (size_t)a.Ws;
  // a. the reference point, once: the identity grid at pixel centres, as ud_camera_unproject forms it
  const int py = (int)i / a.W, px = (int)i - py * a.W;
  const float cu = (float)px + 0.5f, cw = (float)py + 0.5f;
  const float depth = a.depth[at];
  const float* pr = a.params_ref + (size_t)b * 16;
  float P[3];
  ud_cam_unproject_closed(model_ref, UD_UNPROJ_DEPTH, pr, cu, cw, depth, P);
  const bool ref_ok = (a.valid_in ? a.valid_in[at] != 0 : true) && depth > 0.0f;       // false for a NaN
  float sum = depth;
  int cnt = 0;
  // b. the views, in order
  for (int v = 0; v < a.V; ++v) {
    const size_t tv = (size_t)(a.nT == 1 ? 0 : b) * (size_t)a.V + (size_t)v, bv = (size_t)b * (size_t)a.V + (size_t)v;
    const int ms = model_src[v * a.B + b];
    const float* ps = a.params_src + ((size_t)v * (size_t)a.B + (size_t)b) * 16;
    float x = P[0], y = P[1], z = P[2];
    ud_cam_move(a.T + tv * 12, x, y, z);
    float su, sv;
    ud_cam_project(ms, ps, x, y, z, &su, &sv);
    const float dproj = ud_cam_depth(ms, x, y, z);
    const bool cv = ref_ok && ud_cam_inside(ms, su, sv, z, a.Hs, a.Ws) && dproj > 0.0f;
    // the view's depth at (su, sv): bilinear, zeros padding, a tap dropped when its depth is not > 0 or its mask is 0, the normalised form
    const bool live = cv && ud_rm_finite(su, sv);
    UdRmTaps t;
    ud_rm_taps(su, sv, a.Ws, a.Hs, UD_RM_BILINEAR, UD_RM_ZEROS, &t);
    const float* sd = a.src_depth + bv * hw;
    const unsigned char* m = a.src_mask ? a.src_mask + bv * hw : nullptr;
    float val[4];
    for (int k = 0; k < 4; ++k) {
      val[k] = 0.0f;
      if (t.off[k] >= 0) {
        const float d = sd[t.off[k]];
        if (d > 0.0f && (!m || m[t.off[k]] != 0)) val[k] = d;
        else t.off[k] = -1;
      }
    }
    const float wsum = ud_rm_weight_sum(t);
    const float ds = live ? ud_rm_value(t, val, UD_RM_BILINEAR, 1, wsum) : 0.0f;
    const bool sampled = live && ud_rm_inside(su, sv, a.Ws, a.Hs) && ud_rm_any(t) && wsum > 0.0f;
    bool consistent = false;
    float epx = 0.0f, erel = 0.0f;
    if (sampled) {
      // the sample lifted through the view's camera, brought home, projected through the reference camera
      float Q[3];
      ud_cam_unproject_closed(ms, UD_UNPROJ_DEPTH, ps, su, sv, ds, Q);
      float xb = Q[0], yb = Q[1], zb = Q[2];
      ud_cam_move(a.Tinv + tv * 12, xb, yb, zb);
      float ru, rv;
      ud_cam_project(model_ref, pr, xb, yb, zb, &ru, &rv);
      const float dback = ud_cam_depth(model_ref, xb, yb, zb);
      const bool inside = ud_cam_inside(model_ref, ru, rv, zb, a.H, a.W);
      const float du = ru - cu, dv = rv - cw;
      const float e2 = du * du + dv * dv;
      const float diff = fabsf(dback - depth), bar = a.rel_tol * depth;
      consistent = inside && dback > 0.0f && e2 <= a.tol2 && diff <= bar;              // false whenever anything is a NaN
      epx = sqrtf(e2);
      erel = diff / depth;
      if (consistent) {
        sum = sum + dback;
        ++cnt;
      }
    }
    if (a.consistent) a.consistent[bv * n + (size_t)i] = consistent ? 1 : 0;
    if (a.err_px) a.err_px[bv * n + (size_t)i] = epx;
    if (a.err_rel) a.err_rel[bv * n + (size_t)i] = erel;
  }
  // c. the outputs
  a.fused[at] = ref_ok ? sum / (float)(cnt + 1) : 0.0f;
  a.count[at] = (unsigned char)cnt;
  a.mask[at] = (ref_ok && cnt >= a.min_views) ? 1 : 0;
}
