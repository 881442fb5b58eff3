// Points of a batch projected to image coordinates (include/unidepth_hip.h, UdCameraProject): the device form of the reference's
// Camera.project (unidepth/utils/camera.py: Pinhole :239-252, EUCM :281-304, Spherical :359-368, OPENCV :423-493, Fisheye624 :705-775,
// MEI :1084-1142, BatchCamera :1158-1164), one camera model per image.  All six models are closed form: one launch, one thread per
// point, blockIdx.y = image, so the model is uniform per workgroup.  Planar sources are read with coalesced dword loads per plane,
// packed rows with one 12-byte load per lane (as splat.hip); uv goes out the same way (two planes, or one 8-byte store).
// Built with -ffp-contract=off: every operation rounds separately, as the numpy fp32 restatement in tools/make_golden_camera_project.py.
#include "ud_common.h"
#include "camera_models.h"

namespace {

constexpr int PJ_THREADS = 256;

struct PjArgs {
  const float* xyz; const float* params; const float* T;
  float* uv; unsigned char* inside; float* depth;
  long long bs, ps, cs, n;
  int H, W, nT, uv_rows;
  unsigned char model[UD_RECON_MAX_B];
};

template <bool ROWS>
__global__ __launch_bounds__(PJ_THREADS) void pj_project_kernel(const PjArgs a) {
  const long long i = (long long)blockIdx.x * PJ_THREADS + threadIdx.x;
  if (i >= a.n) return;
  const int b = blockIdx.y;
  const int model = a.model[b];
  const float* src = a.xyz + b * a.bs + i * a.ps;
  float x, y, z;
  if (ROWS) {                                              // cs = 1: one 12-byte load
    struct __attribute__((packed, aligned(4))) Row { float v[3]; };
    const Row row = *(const Row*)src;
    x = row.v[0]; y = row.v[1]; z = row.v[2];
  } else {
    x = src[0]; y = src[a.cs]; z = src[2 * a.cs];
  }
  if (a.T) {                                               // ud_cam_move (camera_models.h) written out: the call changes this kernel's instruction schedule
    const float* t = a.T + (a.nT == 1 ? 0 : (size_t)b * 12);
    const float xt = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
    const float yt = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
    const float zt = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
    x = xt; y = yt; z = zt;
  }
  float u, v;
  ud_cam_project(model, a.params + (size_t)b * 16, x, y, z, &u, &v);
  const size_t o = (size_t)b * (size_t)a.n + (size_t)i;
  if (a.uv_rows) {
    *(float2*)(a.uv + 2 * o) = make_float2(u, v);          // hipMalloc'd and 8-byte aligned: checked on the host
  } else {
    float* q = a.uv + (size_t)b * 2 * (size_t)a.n + (size_t)i;
    q[0] = u; q[a.n] = v;
  }
  if (a.inside) a.inside[o] = ud_cam_inside(model, u, v, z, a.H, a.W) ? 1 : 0;
  if (a.depth) a.depth[o] = ud_cam_depth(model, x, y, z);
}

}  // namespace

extern "C" int ud_camera_project(const UdCameraProject* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_camera_project: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdCameraProject& d = *desc;
  if (d.B < 1 || d.B > UD_RECON_MAX_B || d.H < 1 || d.W < 1 || d.n_points < 0 || d.n_points > 0x7fffffffLL) {
    ud_set_error("ud_camera_project: bad sizes (1 <= B <= 256, H, W >= 1, 0 <= n_points < 2^31)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.xyz || !d.params || !d.uv) {
    ud_set_error("ud_camera_project: null pointer (xyz, params, uv)");
    return UD_ERR_BAD_ARG;
  }
  if (d.point_stride < 1 || d.comp_stride < 1 || d.batch_stride < 0) {
    ud_set_error("ud_camera_project: bad strides (point_stride, comp_stride >= 1, batch_stride >= 0)");
    return UD_ERR_BAD_ARG;
  }
  if (d.uv_rows && ((uintptr_t)d.uv & 7)) {
    ud_set_error("ud_camera_project: uv rows must be 8-byte aligned");
    return UD_ERR_BAD_ARG;
  }
  if (d.T && d.nT != 1 && d.nT != d.B) {
    ud_set_error("ud_camera_project: nT must be 1 or B when T is given");
    return UD_ERR_BAD_ARG;
  }
  PjArgs a;
  a.xyz = d.xyz; a.params = d.params; a.T = d.T; a.uv = d.uv; a.inside = d.inside; a.depth = d.depth;
  a.bs = d.batch_stride; a.ps = d.point_stride; a.cs = d.comp_stride; a.n = d.n_points;
  a.H = d.H; a.W = d.W; a.nT = d.nT; a.uv_rows = d.uv_rows;
  for (int b = 0; b < d.B; ++b) {
    if (!ud_cam_model_ok(d.model[b])) {
      ud_set_error("ud_camera_project: model tag outside 1..6");
      return UD_ERR_BAD_ARG;
    }
  }
  ud_copy_models(a.model, d.model, d.B);
  if (d.n_points == 0) return UD_OK;
  const dim3 grid((unsigned)((d.n_points + PJ_THREADS - 1) / PJ_THREADS), (unsigned)d.B);
  if (d.comp_stride == 1) hipLaunchKernelGGL(pj_project_kernel<true>, grid, dim3(PJ_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pj_project_kernel<false>, grid, dim3(PJ_THREADS), 0, (hipStream_t)stream, a);
  UD_CHECK_LAUNCH("ud_camera_project launch");
  return UD_OK;
}
