// Backward warping through the camera models in ONE launch (include/unidepth_hip.h, UdWarpCamera): for every pixel of a destination view,
// its point (given, or its depth unprojected through the destination camera), moved by a rigid transform, projected through the source
// camera, and the source view's maps sampled there, with the validity of the sample and an optional visibility test against the source's
// depth.  It is ud_camera_unproject -> ud_camera_project -> `inside & (depth > 0)` -> ud_remap (-> ud_remap of the source depth and the
// comparison) fused: the point map, the coordinate map, the inside mask and the projected depth stay in registers.
//
//   wp_warp_kernel   one thread per destination pixel, blockIdx.y = image, 256 threads, so both camera models are uniform per workgroup
//                    and the parameter rows and T are addressed by blockIdx.y alone (scalar loads).  Tap offsets and weights stay in
//                    registers across the channel loop; each channel is four gathers and one store, coalesced per channel plane.  No
//                    LDS, no atomics, no workspace, no host synchronisation: captures into a graph.
//
// The arithmetic of a pixel is csrc/warp_point.h, which only calls csrc/camera_models.h and csrc/remap_taps.h; the host build of the tests
// runs it under the sanitizers.  Not fused: OPENCV / Fisheye624 DESTINATIONS, whose radial loop ends on a maximum over the whole image (the
// caller unprojects those with ud_camera_unproject and hands the points over), and any conversion of sampled values between depth
// conventions.  Built with -ffp-contract=off: every operation rounds separately, so each output has the bits of the separate launches.
#include "ud_common.h"
#include "warp_point.h"
#pragma clang fp contract(off)

namespace {

constexpr int WP_THREADS = 256;

template <typename S, typename O>
struct WpKernelArgs {
  UdWpArgs<S, O> p;
  unsigned char model_dst[UD_RECON_MAX_B], model_src[UD_RECON_MAX_B];
};

template <typename S, typename O>
__global__ __launch_bounds__(WP_THREADS) void wp_warp_kernel(const WpKernelArgs<S, O> a) {
  const long long i = (long long)blockIdx.x * WP_THREADS + threadIdx.x;
  if (i >= a.p.n) return;
  const int b = blockIdx.y;
  ud_wp_point(a.p, a.model_dst[b], a.model_src[b], b, i);
}

template <typename S, typename O>
void wp_launch(const UdWarpCamera& d, hipStream_t s) {
  WpKernelArgs<S, O> a;
  const long long n = (long long)d.Ho * d.Wo, hw = (long long)d.Hs * d.Ws;
  a.p.src = (const S*)d.src; a.p.src_mask = d.src_mask; a.p.src_depth = d.src_depth;
  a.p.points = d.points; a.p.depth = d.depth; a.p.params_dst = d.params_dst; a.p.params_src = d.params_src; a.p.T = d.T;
  a.p.valid_in = d.valid_in;
  a.p.out = (O*)d.out; a.p.valid = d.valid; a.p.visible = d.visible; a.p.uv = d.uv; a.p.proj_depth = d.proj_depth;
  a.p.n = n;
  a.p.src_bs = d.src_shared ? 0 : d.C * hw;
  a.p.mask_bs = d.mask_shared ? 0 : hw;
  a.p.sdepth_bs = d.depth_shared ? 0 : hw;
  a.p.tol = ud_f32_from_bits(d.tol_bits);
  a.p.C = d.C; a.p.Wo = d.Wo; a.p.Hs = d.Hs; a.p.Ws = d.Ws; a.p.nT = d.nT; a.p.mode = d.mode; a.p.padding = d.padding;
  a.p.normalize = d.normalize ? 1 : 0;
  ud_copy_models(a.model_dst, d.model_dst, d.B);
  ud_copy_models(a.model_src, d.model_src, d.B);
  const dim3 grid((unsigned)((n + WP_THREADS - 1) / WP_THREADS), (unsigned)d.B);
  hipLaunchKernelGGL((wp_warp_kernel<S, O>), grid, dim3(WP_THREADS), 0, s, a);
}

}  // namespace

extern "C" int ud_warp_camera(const UdWarpCamera* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_warp_camera: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdWarpCamera& d = *desc;
  if (d.B < 1 || d.B > UD_RECON_MAX_B || d.C < 1 || d.Ho < 1 || d.Wo < 1 || d.Hs < 1 || d.Ws < 1) {
    ud_set_error("ud_warp_camera: bad sizes (1 <= B <= 256, C, Ho, Wo, Hs, Ws >= 1)");
    return UD_ERR_BAD_ARG;
  }
  const long long n = (long long)d.Ho * d.Wo, hw = (long long)d.Hs * d.Ws;
  if (n >= UD_MAX_ELEMS || hw >= UD_MAX_ELEMS || d.C * hw >= UD_MAX_ELEMS || d.C * n >= UD_MAX_ELEMS) {
    ud_set_error("ud_warp_camera: too large (Ho * Wo, C * Ho * Wo and C * Hs * Ws must stay below 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if ((d.points != nullptr) == (d.depth != nullptr)) {
    ud_set_error("ud_warp_camera: exactly one of points or depth must be given");
    return UD_ERR_BAD_ARG;
  }
  if (!d.src || !d.params_src || !d.out || (d.depth && !d.params_dst) || (d.visible && !d.src_depth)) {
    ud_set_error("ud_warp_camera: null pointer (src, params_src, out; params_dst with depth; src_depth with visible)");
    return UD_ERR_BAD_ARG;
  }
  if (d.mode != UD_REMAP_NEAREST && d.mode != UD_REMAP_BILINEAR) {
    ud_set_error("ud_warp_camera: unknown mode (UD_REMAP_NEAREST, UD_REMAP_BILINEAR)");
    return UD_ERR_BAD_ARG;
  }
  if (d.padding != UD_REMAP_ZEROS && d.padding != UD_REMAP_BORDER) {
    ud_set_error("ud_warp_camera: unknown padding (UD_REMAP_ZEROS, UD_REMAP_BORDER)");
    return UD_ERR_BAD_ARG;
  }
  if (d.out_u8 && !d.src_u8) {
    ud_set_error("ud_warp_camera: uint8 output needs a uint8 source");
    return UD_ERR_UNSUPPORTED;
  }
  if (d.T && d.nT != 1 && d.nT != d.B) {
    ud_set_error("ud_warp_camera: nT must be 1 or B when T is given");
    return UD_ERR_BAD_ARG;
  }
  for (int b = 0; b < d.B; ++b) {
    const int ms = d.model_src[b], md = d.model_dst[b];
    if (!ud_cam_model_ok(ms) || (d.depth && !ud_cam_model_ok(md))) {
      ud_set_error("ud_warp_camera: model tag outside 1..6");
      return UD_ERR_BAD_ARG;
    }
    if (d.depth && !ud_cam_closed_form(md)) {
      ud_set_error("ud_warp_camera: iterative destination (OPENCV / Fisheye624) with depth: unproject with ud_camera_unproject and pass points");
      return UD_ERR_UNSUPPORTED;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  if (!d.src_u8) wp_launch<float, float>(d, s);
  else if (d.out_u8) wp_launch<unsigned char, unsigned char>(d, s);
  else wp_launch<unsigned char, float>(d, s);
  UD_CHECK_LAUNCH("ud_warp_camera launch");
  return UD_OK;
}
