// Sampling the maps of a batch at arbitrary image coordinates (include/unidepth_hip.h, UdRemap) and the reference's
// Camera.mask_overlap_projection (unidepth/utils/camera.py:132-154; UdOverlapMask).  A sampler and nothing else: no camera arithmetic,
// no solver.  The coordinates come from project_camera(unproject_camera(grid, dst_cam), src_cam) (undistortion, backward warping), from
// keypoints, or from anywhere else.
//
//   rm_remap_kernel    one thread per output point, blockIdx.y = image, 256 threads.  The coordinate is loaded once; tap offsets and
//                      weights stay in registers across the channel loop; each channel is four gathers and one store, coalesced per
//                      channel plane for the planar output.  No workspace, no atomics, no LDS, no host synchronisation.
//   rm_overlap_kernel  one thread per pixel; reads its own uv and the uv of the four taps of its sample position; the flow
//                      uv - (x + 0.5, y + 0.5) is formed where it is read and never stored.
//
// The arithmetic of a point is csrc/remap_taps.h, which the host build of the tests runs under the sanitizers: a coordinate is clamped
// in floating point (NaN to a fixed in-range value) before it is converted to an index, so no tap address depends on an unchecked float.
// Built with -ffp-contract=off: every operation rounds separately, as the numpy fp32 restatement in tools/make_golden_remap.py; there is
// no libm call in either kernel, so the restatement is reproduced bit for bit.
#include "ud_common.h"
#include "remap_taps.h"
#pragma clang fp contract(off)

namespace {

constexpr int RM_THREADS = 256;

template <typename S, typename O>
__global__ __launch_bounds__(RM_THREADS) void rm_remap_kernel(const UdRmArgs<S, O> a) {
  const long long i = (long long)blockIdx.x * RM_THREADS + threadIdx.x;
  if (i >= a.n) return;
  ud_rm_point(a, (int)blockIdx.y, i);
}

__global__ __launch_bounds__(RM_THREADS) void rm_overlap_kernel(const float* uv, unsigned char* mask, int H, int W) {
  const long long i = (long long)blockIdx.x * RM_THREADS + threadIdx.x;
  const long long hw = (long long)H * W;
  if (i >= hw) return;
  const size_t b = blockIdx.y;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  mask[b * (size_t)hw + (size_t)i] = ud_ov_pixel(uv + b * 2 * (size_t)hw, x, y, H, W) ? 1 : 0;
}

template <typename S, typename O>
void rm_launch(const UdRemap& d, hipStream_t s) {
  UdRmArgs<S, O> a;
  a.src = (const S*)d.src; a.src_mask = d.src_mask; a.uv = d.uv; a.coord_valid = d.coord_valid;
  a.out = (O*)d.out; a.valid = d.valid;
  a.bs = d.batch_stride; a.ps = d.point_stride; a.cs = d.comp_stride; a.n = d.n_points;
  a.src_bs = d.src_shared ? 0 : d.C * ((long long)d.Hs * d.Ws);
  a.mask_bs = d.mask_shared ? 0 : (long long)d.Hs * d.Ws;
  a.C = d.C; a.Hs = d.Hs; a.Ws = d.Ws; a.mode = d.mode; a.padding = d.padding; a.normalize = d.normalize ? 1 : 0; a.out_rows = d.out_rows ? 1 : 0;
  const dim3 grid((unsigned)((d.n_points + RM_THREADS - 1) / RM_THREADS), (unsigned)d.B);
  hipLaunchKernelGGL((rm_remap_kernel<S, O>), grid, dim3(RM_THREADS), 0, s, a);
}


}  // namespace

extern "C" int ud_remap(const UdRemap* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_remap: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdRemap& d = *desc;
  if (d.B < 1 || d.B > UD_RECON_MAX_B || d.C < 1 || d.Hs < 1 || d.Ws < 1 || d.n_points < 1) {
    ud_set_error("ud_remap: bad sizes (1 <= B <= 256, C, Hs, Ws, n_points >= 1)");
    return UD_ERR_BAD_ARG;
  }
  if (d.n_points >= UD_MAX_ELEMS || (long long)d.Hs * d.Ws >= UD_MAX_ELEMS || d.C * ((long long)d.Hs * d.Ws) >= UD_MAX_ELEMS ||
      d.C * d.n_points >= UD_MAX_ELEMS) {
    ud_set_error("ud_remap: too large (n_points, C * n_points and C * Hs * Ws must stay below 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.src || !d.uv || !d.out) {
    ud_set_error("ud_remap: null pointer (src, uv, out)");
    return UD_ERR_BAD_ARG;
  }
  if (d.point_stride < 1 || d.comp_stride < 1 || d.batch_stride < 0) {
    ud_set_error("ud_remap: bad strides (point_stride, comp_stride >= 1, batch_stride >= 0)");
    return UD_ERR_BAD_ARG;
  }
  if (d.mode != UD_REMAP_NEAREST && d.mode != UD_REMAP_BILINEAR) {
    ud_set_error("ud_remap: unknown mode (UD_REMAP_NEAREST, UD_REMAP_BILINEAR)");
    return UD_ERR_BAD_ARG;
  }
  if (d.padding != UD_REMAP_ZEROS && d.padding != UD_REMAP_BORDER) {
    ud_set_error("ud_remap: unknown padding (UD_REMAP_ZEROS, UD_REMAP_BORDER)");
    return UD_ERR_BAD_ARG;
  }
  if (d.out_u8 && !d.src_u8) {
    ud_set_error("ud_remap: uint8 output needs a uint8 source");
    return UD_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  if (!d.src_u8) rm_launch<float, float>(d, s);
  else if (d.out_u8) rm_launch<unsigned char, unsigned char>(d, s);
  else rm_launch<unsigned char, float>(d, s);
  UD_CHECK_LAUNCH("ud_remap launch");
  return UD_OK;
}

extern "C" int ud_overlap_mask(const UdOverlapMask* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_overlap_mask: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdOverlapMask& d = *desc;
  if (d.B < 1 || d.B > UD_RECON_MAX_B || d.H < 2 || d.W < 2) {
    ud_set_error("ud_overlap_mask: bad sizes (1 <= B <= 256, H, W >= 2: the sample grid divides by H - 1 and W - 1)");
    return UD_ERR_BAD_ARG;
  }
  if ((long long)d.H * d.W >= UD_MAX_ELEMS) {
    ud_set_error("ud_overlap_mask: too large (H * W must stay below 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.uv || !d.mask) {
    ud_set_error("ud_overlap_mask: null pointer (uv, mask)");
    return UD_ERR_BAD_ARG;
  }
  const long long hw = (long long)d.H * d.W;
  hipLaunchKernelGGL(rm_overlap_kernel, dim3((unsigned)((hw + RM_THREADS - 1) / RM_THREADS), (unsigned)d.B), dim3(RM_THREADS), 0,
                     (hipStream_t)stream, d.uv, d.mask, d.H, d.W);
  UD_CHECK_LAUNCH("ud_overlap_mask launch");
  return UD_OK;
}
