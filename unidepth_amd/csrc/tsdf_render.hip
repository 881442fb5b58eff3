// A TSDF volume ray-cast to depth, points, normals and colour (include/unidepth_hip.h, UdTsdfRender): the counterpart of ud_tsdf_integrate,
// KinectFusion's surface prediction.
//
//   tr_render_kernel<PATCH>  one thread per output pixel, blockIdx.y = image, 256 threads.  The march runs inside the thread: the direction,
//                            the previous sample and the scan's state stay in registers; a sample costs one rigid motion, three divisions
//                            and eight gathers of the weight volume, and eight of the distance volume only where the weights pass.  The
//                            image's model, parameter row, T and origin are addressed by blockIdx.y alone (scalar loads).
//                            PATCH = false: a wave is 64 consecutive pixels of the row-major image; PATCH = true: a wave is an 8 x 8 pixel
//                            patch, whose rays walk a more compact bundle of cells.  Measured (profiles/tsdf_render_bench.txt): rows are
//                            the faster at 256^3 (the patch takes 13 - 24 % longer), the patch at 128^3 with B = 8 (up to 17 %); the
//                            wrapper's default is rows.  No output bit depends on the mapping.
//                            No LDS, no atomics, no workspace, no host synchronisation: captures into a graph.
//
// The arithmetic of a ray is csrc/tsdf_ray.h, which only calls csrc/camera_models.h and csrc/remap_taps.h; the host build of the tests
// runs it under the sanitizers.  Built with -ffp-contract=off: every operation rounds separately, so the outputs have the bits of the
// numpy restatement of the tests and of tsdf_render_composition.
#include <math.h>
#include "ud_common.h"
#include "tsdf_ray.h"
#pragma clang fp contract(off)

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_PATCH = 8;                            // 8 x 8 pixels = one wave

struct TrKernelArgs {
  UdTsdfRayArgs p;
  unsigned char model[UD_RECON_MAX_B];
};

template <bool PATCH>
__global__ __launch_bounds__(TR_THREADS) void tr_render_kernel(const TrKernelArgs a) {
  const int b = (int)blockIdx.y;
  int px, py;
  if (PATCH) {
    // wave w of the image: patch (w / patches per row, w % patches per row); lane l: (l / 8, l % 8) inside it
    const int pw = (a.p.Wo + TR_PATCH - 1) / TR_PATCH;
    const long long w = (long long)blockIdx.x * (TR_THREADS / UD_WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long pr = w / pw;
    if (pr * TR_PATCH >= a.p.Ho) return;
    py = (int)pr * TR_PATCH + (lane >> 3);
    px = (int)(w - pr * pw) * TR_PATCH + (lane & 7);
    if (py >= a.p.Ho || px >= a.p.Wo) return;
  } else {
    const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
    if (i >= (long long)a.p.Ho * a.p.Wo) return;
    py = (int)(i / a.p.Wo);
    px = (int)(i - (long long)py * a.p.Wo);
  }
  ud_tsdf_ray(a.p, a.model[b], b, py, px);
}

bool tr_positive(float x) { return x > 0.0f && x <= 3.402823466e38f; }     // finite and > 0 (false for a NaN)

}  // namespace

extern "C" int ud_tsdf_render(const UdTsdfRender* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_tsdf_render: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdTsdfRender& d = *desc;
  if (d.B < 1 || d.B > UD_RECON_MAX_B || d.Ho < 1 || d.Wo < 1 || d.Nx < 1 || d.Ny < 1 || d.Nz < 1) {
    ud_set_error("ud_tsdf_render: bad sizes (1 <= B <= 256, Ho, Wo, Nx, Ny, Nz >= 1)");
    return UD_ERR_BAD_ARG;
  }
  const long long hw = (long long)d.Ho * d.Wo, nxy = (long long)d.Nx * d.Ny;
  if (hw >= UD_MAX_ELEMS || 3 * hw >= UD_MAX_ELEMS || nxy >= UD_MAX_ELEMS || nxy * d.Nz >= UD_MAX_ELEMS) {
    ud_set_error("ud_tsdf_render: too large (Nx * Ny * Nz and 3 * Ho * Wo must stay below 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.tsdf || !d.weight || !d.origin || !d.depth || !d.valid) {
    ud_set_error("ud_tsdf_render: null pointer (tsdf, weight, origin, depth, valid)");
    return UD_ERR_BAD_ARG;
  }
  if (d.color_out && !d.color) {
    ud_set_error("ud_tsdf_render: color_out needs a color volume");
    return UD_ERR_BAD_ARG;
  }
  if (d.T && d.nT != 1 && d.nT != d.B) {
    ud_set_error("ud_tsdf_render: nT must be 1 or B");
    return UD_ERR_BAD_ARG;
  }
  if (d.n_origin != 1 && d.n_origin != d.B) {
    ud_set_error("ud_tsdf_render: n_origin must be 1 or B (rows of the origin)");
    return UD_ERR_BAD_ARG;
  }
  const float vs = ud_f32_from_bits(d.voxel_size_bits), near = ud_f32_from_bits(d.near_bits), step = ud_f32_from_bits(d.step_bits);
  const float min_weight = ud_f32_from_bits(d.min_weight_bits);
  if (!tr_positive(vs) || !tr_positive(step)) {
    ud_set_error("ud_tsdf_render: voxel_size and step must be finite and positive");
    return UD_ERR_BAD_ARG;
  }
  if (!ud_tolerance_ok(near)) {
    ud_set_error("ud_tsdf_render: near must be finite and not negative");
    return UD_ERR_BAD_ARG;
  }
  if (min_weight != min_weight) {
    ud_set_error("ud_tsdf_render: min_weight must not be a NaN");
    return UD_ERR_BAD_ARG;
  }
  if (d.K < 1 || d.K > 16384) {
    ud_set_error("ud_tsdf_render: K (the number of samples) must be 1 .. 16384");
    return UD_ERR_BAD_ARG;
  }
  for (int k = 0; k < d.B; ++k) {
    if (!ud_cam_model_ok(d.model[k])) {
      ud_set_error("ud_tsdf_render: model tag outside 1..6");
      return UD_ERR_BAD_ARG;
    }
    if (!d.rays && !ud_cam_closed_form(d.model[k])) {
      ud_set_error("ud_tsdf_render: an OPENCV / Fisheye624 image needs rays (ud_camera_unproject's, normalised)");
      return UD_ERR_BAD_ARG;
    }
  }
  if (!d.rays && !d.params) {
    ud_set_error("ud_tsdf_render: params is needed without rays");
    return UD_ERR_BAD_ARG;
  }
  TrKernelArgs a;
  a.p.tsdf = d.tsdf; a.p.weight = d.weight; a.p.color = d.color; a.p.origin = d.origin; a.p.T = d.T; a.p.params = d.params; a.p.rays = d.rays;
  a.p.depth = d.depth; a.p.valid = d.valid; a.p.points = d.points; a.p.normals = d.normals; a.p.color_out = d.color_out;
  a.p.n = nxy * d.Nz;
  a.p.vs = vs; a.p.near = near; a.p.step = step; a.p.min_weight = min_weight;
  a.p.B = d.B; a.p.Ho = d.Ho; a.p.Wo = d.Wo; a.p.Nx = d.Nx; a.p.Ny = d.Ny; a.p.Nz = d.Nz; a.p.nT = d.nT; a.p.nO = d.n_origin; a.p.K = d.K;
  a.p.color_f32 = d.color_f32 != 0; a.p.full_scan = d.full_scan != 0;
  ud_copy_models(a.model, d.model, d.B);
  hipStream_t s = (hipStream_t)stream;
  if (d.wave_patch) {
    const long long waves = (long long)((d.Wo + TR_PATCH - 1) / TR_PATCH) * ((d.Ho + TR_PATCH - 1) / TR_PATCH);
    const int per = TR_THREADS / UD_WAVE;
    hipLaunchKernelGGL(tr_render_kernel<true>, dim3((unsigned)((waves + per - 1) / per), (unsigned)d.B), dim3(TR_THREADS), 0, s, a);
  } else {
    hipLaunchKernelGGL(tr_render_kernel<false>, dim3((unsigned)((hw + TR_THREADS - 1) / TR_THREADS), (unsigned)d.B), dim3(TR_THREADS), 0, s, a);
  }
  UD_CHECK_LAUNCH("ud_tsdf_render launch");
  return UD_OK;
}
