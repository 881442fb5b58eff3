// Multi-view depth consistency and fusion in ONE launch (include/unidepth_hip.h, UdDepthConsistency): for every pixel of a reference view,
// the forward-backward test of multi-view stereo against V neighbour views -- the pixel's point moved into the view and projected, the
// view's depth sampled there, that sample lifted through the view's camera, brought home and projected through the reference camera, kept
// when it lands within a pixel tolerance and a relative depth tolerance -- with the count of agreeing views and the mean of the depths that
// agree.  It is, per view, ud_warp_camera -> ud_camera_unproject -> ud_camera_project and a dozen element-wise passes fused: the coordinate
// maps, the sampled depth, the validity, the lifted point map, the second coordinate map, the second depth and the inside mask stay in
// registers, and the reference depth is unprojected once for all views.
//
//   cs_consistency_kernel   one thread per reference pixel, blockIdx.y = image, 256 threads, so the reference model and each view's model
//                           are uniform per workgroup and the parameter rows, T and Tinv are addressed by blockIdx.y and the view alone
//                           (scalar loads).  The view loop runs inside the thread: the reference point, the running sum and the count
//                           stay in registers; a view costs one 4-tap gather (and its mask's) and up to three coalesced stores.  No LDS,
//                           no atomics, no workspace, no host synchronisation: captures into a graph.
//
// The arithmetic of a pixel is csrc/consistency_point.h, which only calls csrc/camera_models.h and csrc/remap_taps.h; the host build of the
// tests runs it under the sanitizers.  Not fused: OPENCV / Fisheye624 members, reference or view, whose unprojection ends on a maximum over
// the whole image (the Python wrapper runs the composition of the separate calls for those).  Built with -ffp-contract=off: every operation
// rounds separately, so each output has the bits of the separate launches.
#include <math.h>
#include "ud_common.h"
#include "consistency_point.h"
#pragma clang fp contract(off)

namespace {

constexpr int CS_THREADS = 256;

struct CsKernelArgs {
  UdCsArgs p;
  unsigned char model_ref[UD_RECON_MAX_B], model_src[UD_RECON_MAX_B];      // model_src[v * B + b]
};

__global__ __launch_bounds__(CS_THREADS) void cs_consistency_kernel(const CsKernelArgs a) {
  const long long i = (long long)blockIdx.x * CS_THREADS + threadIdx.x;
  if (i >= a.p.n) return;
  const int b = blockIdx.y;
  ud_cs_point(a.p, a.model_ref[b], a.model_src, b, i);
}

}  // namespace

extern "C" int ud_depth_consistency(const UdDepthConsistency* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_depth_consistency: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdDepthConsistency& d = *desc;
  if (d.B < 1 || d.V < 1 || d.V > 255 || (long long)d.B * d.V > UD_RECON_MAX_B || d.H < 1 || d.W < 1 || d.Hs < 1 || d.Ws < 1) {
    ud_set_error("ud_depth_consistency: bad sizes (B, V >= 1, B * V <= 256, V <= 255, H, W, Hs, Ws >= 1)");
    return UD_ERR_BAD_ARG;
  }
  const long long n = (long long)d.H * d.W, hw = (long long)d.Hs * d.Ws;
  if (n >= UD_MAX_ELEMS || hw >= UD_MAX_ELEMS || d.V * hw >= UD_MAX_ELEMS) {
    ud_set_error("ud_depth_consistency: too large (H * W, Hs * Ws and V * Hs * Ws must stay below 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.depth || !d.params_ref || !d.src_depth || !d.params_src || !d.T || !d.Tinv || !d.fused || !d.count || !d.mask) {
    ud_set_error("ud_depth_consistency: null pointer (depth, params_ref, src_depth, params_src, T, Tinv, fused, count, mask)");
    return UD_ERR_BAD_ARG;
  }
  if (d.nT != 1 && d.nT != d.B) {
    ud_set_error("ud_depth_consistency: nT must be 1 or B (sets of V matrices)");
    return UD_ERR_BAD_ARG;
  }
  const float px_tol = ud_f32_from_bits(d.px_tol_bits), rel_tol = ud_f32_from_bits(d.rel_tol_bits);
  if (!ud_tolerance_ok(px_tol) || !ud_tolerance_ok(rel_tol)) {
    ud_set_error("ud_depth_consistency: px_tol and rel_tol must be finite and not negative");
    return UD_ERR_BAD_ARG;
  }
  if (d.min_views < 0 || d.min_views > d.V) {
    ud_set_error("ud_depth_consistency: min_views must lie in 0 .. V");
    return UD_ERR_BAD_ARG;
  }
  for (int k = 0; k < d.B * d.V; ++k) {
    const int ms = d.model_src[k], mr = k < d.B ? d.model_ref[k] : UD_CAM_PINHOLE;
    if (!ud_cam_model_ok(ms) || !ud_cam_model_ok(mr)) {
      ud_set_error("ud_depth_consistency: model tag outside 1..6");
      return UD_ERR_BAD_ARG;
    }
    if (!ud_cam_closed_form(ms) || !ud_cam_closed_form(mr)) {
      ud_set_error("ud_depth_consistency: iterative model (OPENCV / Fisheye624), reference or view: its unprojection ends on a maximum over the image; compose the separate calls");
      return UD_ERR_UNSUPPORTED;
    }
  }
  CsKernelArgs a;
  a.p.depth = d.depth; a.p.params_ref = d.params_ref; a.p.valid_in = d.valid_in;
  a.p.src_depth = d.src_depth; a.p.src_mask = d.src_mask; a.p.params_src = d.params_src; a.p.T = d.T; a.p.Tinv = d.Tinv;
  a.p.fused = d.fused; a.p.count = d.count; a.p.mask = d.mask; a.p.consistent = d.consistent; a.p.err_px = d.err_px; a.p.err_rel = d.err_rel;
  a.p.n = n;
  a.p.tol2 = px_tol * px_tol;
  a.p.rel_tol = rel_tol;
  a.p.B = d.B; a.p.V = d.V; a.p.H = d.H; a.p.W = d.W; a.p.Hs = d.Hs; a.p.Ws = d.Ws; a.p.nT = d.nT; a.p.min_views = d.min_views;
  ud_copy_models(a.model_ref, d.model_ref, d.B);
  ud_copy_models(a.model_src, d.model_src, d.B * d.V);
  const dim3 grid((unsigned)((n + CS_THREADS - 1) / CS_THREADS), (unsigned)d.B);
  hipLaunchKernelGGL(cs_consistency_kernel, grid, dim3(CS_THREADS), 0, (hipStream_t)stream, a);
  UD_CHECK_LAUNCH("ud_depth_consistency launch");
  return UD_OK;
}
