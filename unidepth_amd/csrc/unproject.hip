// Viewing rays at arbitrary image coordinates (include/unidepth_hip.h, UdCameraUnproject): the device form of the reference's
// Camera.unproject / get_rays / reconstruct (unidepth/utils/camera.py: base :69-92, Pinhole :255-273, EUCM :307-328, Spherical :371-392,
// OPENCV :496-694, Fisheye624 :778-974, MEI :985-1082, BatchCamera :1167-1171), one camera model per image, one thread per point,
// blockIdx.y = image, so the model is uniform per workgroup.  The arithmetic is csrc/camera_models.h (ud_cam_unproject_*).
//
//   no OPENCV / Fisheye624 image:  up_first_kernel alone
//   otherwise:                     up_first_kernel (closed-form images complete; every point of an iterative image runs its own 10
//                                  trust-region steps in registers; the largest |residual| at theta_0 .. theta_10 is reduced over the
//                                  wave, then over the workgroup in LDS, and published with one atomicMax per workgroup and iteration
//                                  on the bit pattern of a non-negative float.  Every workgroup of an image aims at the same 11 words:
//                                  with one atomic per WAVE the call's time went into same-address atomics, see
//                                  profiles/unproject_bench.txt)
//                                  -> up_second_kernel over the iterative images only: reads the iteration k* at which the image's maximum
//                                  first fell below 1e-3 -- where the reference leaves the loop -- redoes k* steps and writes the result.
// The iterates and trust radii of a point depend on that point alone; the only thing that couples the points of an image is that exit, so
// this is the result of an init / 10 step / final launch sequence (reconstruct.hip) bit for bit, with no per-point state in memory.
// The maxima are cleared at the head of the call, so a captured graph replays correctly -- by a small kernel of this file, not by
// hipMemsetAsync: a captured memset node of these 44 n bytes left host-pointer-like words in every other maximum from the second replay
// on (eager calls were clean), which keeps images iterating (profiles/unproject_bench.txt has the record).  No grid barrier.
// Built with -ffp-contract=off: every operation rounds separately, as the numpy fp32 restatement in tools/make_golden_unproject.py.
#include "ud_common.h"
#include "camera_models.h"

namespace {

constexpr int UP_THREADS = 1024;                    // 16 waves: one atomicMax per workgroup and iteration, see up_first_kernel
constexpr int UP_WAVES = UP_THREADS / 64;
constexpr int UP_ITERS = 10;                        // max_iters of the radial loop (camera.py:496, :778)
constexpr int UP_MAXRES = UP_ITERS + 1;             // maxima per iterative image: at theta_0 .. theta_10

struct UpArgs {
  const float* uv; const float* params; const float* depth;
  float* rays; unsigned char* valid; float* maxres;
  long long bs, ps, cs;
  int n, W, form, rays_rows, n_iter;
  unsigned char model[UD_RECON_MAX_B];
  short slot_of_img[UD_RECON_MAX_B];               // image -> its row of maxres (iterative images only)
  short img_of_slot[UD_RECON_MAX_B];               // the index table the second grid runs over
};

size_t up_maxres_bytes(int n_iter) { return (((size_t)n_iter * UP_MAXRES * sizeof(float)) + 15) & ~(size_t)15; }

// i < n only
__device__ __forceinline__ void up_load(const UpArgs& a, int b, long long i, float& u, float& v, float& d) {
  if (a.uv) {
    const float* s = a.uv + b * a.bs + i * a.ps;
    u = s[0]; v = s[a.cs];
  } else {                                           // the identity grid at pixel centres; n = H * W: checked on the host
    const int y = (int)i / a.W, x = (int)i - y * a.W;
    u = (float)x + 0.5f; v = (float)y + 0.5f;
  }
  d = a.depth ? a.depth[(size_t)b * (size_t)a.n + (size_t)i] : 0.0f;
}

__device__ __forceinline__ void up_store(const UpArgs& a, int b, long long i, const float* o, bool valid) {
  const size_t n = (size_t)a.n, at = (size_t)b * n + (size_t)i;
  if (a.rays_rows) {
    float* q = a.rays + 3 * at;
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
  } else {
    float* q = a.rays + (size_t)b * 3 * n + (size_t)i;
    q[0] = o[0]; q[n] = o[1]; q[2 * n] = o[2];
  }
  if (a.valid) a.valid[at] = valid ? 1 : 0;
}

// largest value of the wave; a NaN wins.  Every lane of the wave calls this.
__device__ __forceinline__ float up_wave_max(float r) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r = ud_cam_nanmax(r, __shfl_xor(r, o, 64));
  return r;
}

__global__ __launch_bounds__(256) void up_clear_kernel(float* maxres, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) maxres[i] = 0.0f;
}

__global__ __launch_bounds__(UP_THREADS) void up_first_kernel(const UpArgs a) {
  const int b = blockIdx.y;
  const int model = a.model[b];
  const float* p = a.params + (size_t)b * 16;
  const long long i = (long long)blockIdx.x * UP_THREADS + threadIdx.x;
  const bool in = i < a.n;
  float u = 0.0f, v = 0.0f, d = 0.0f;
  if (in) up_load(a, b, i, u, v, d);
  if (model == UD_CAM_OPENCV || model == UD_CAM_FISHEYE624) {
    // no lane leaves before the barrier: out-of-range lanes carry a residual of 0
    __shared__ float wmax[UP_MAXRES][UP_WAVES];
    const int nk = model == UD_CAM_FISHEYE624 ? 6 : 3;
    float xr, yr, rnorm;
    if (!ud_cam_radial_front(p, u, v, &xr, &yr, &rnorm)) return;  // no radial term (uniform per image): the loop runs 0 times
    float th = rnorm, delta = 0.1f;
    for (int it = 0; it <= UP_ITERS; ++it) {
      const float r = up_wave_max(in ? fabsf(ud_cam_radial_residual(p + 4, nk, th, rnorm)) : 0.0f);
      if ((threadIdx.x & 63) == 0) wmax[it][threadIdx.x >> 6] = r;
      if (it < UP_ITERS) ud_cam_radial_step(p + 4, nk, rnorm, th, delta);
    }
    __syncthreads();
    if (threadIdx.x < UP_MAXRES) {
      float r = wmax[threadIdx.x][0];
#pragma unroll
      for (int w = 1; w < UP_WAVES; ++w) r = ud_cam_nanmax(r, wmax[threadIdx.x][w]);
      atomicMax((unsigned*)(a.maxres + a.slot_of_img[b] * UP_MAXRES + threadIdx.x), __float_as_uint(r));
    }
    return;
  }
  if (!in) return;
  float o[3];
  const bool valid = ud_cam_unproject_closed(model, a.form, p, u, v, d, o);
  up_store(a, b, i, o, valid);
}

__global__ __launch_bounds__(UP_THREADS) void up_second_kernel(const UpArgs a) {
  const int slot = blockIdx.y;
  const int b = a.img_of_slot[slot];
  const long long i = (long long)blockIdx.x * UP_THREADS + threadIdx.x;
  if (i >= a.n) return;
  // all zero when the image has no radial term: 0 steps
  const int steps = ud_cam_radial_exit(a.maxres + slot * UP_MAXRES);
  float u, v, d, o[3];
  up_load(a, b, i, u, v, d);
  ud_cam_unproject_radial(a.model[b], a.form, a.params + (size_t)b * 16, u, v, d, steps, o);
  up_store(a, b, i, o, true);
}

}  // namespace

extern "C" long long ud_camera_unproject_work_bytes(int B, int n_iterative) {
  if (B < 1 || B > UD_RECON_MAX_B || n_iterative < 0 || n_iterative > B) return -1;
  return (long long)up_maxres_bytes(n_iterative);
}

extern "C" int ud_camera_unproject(const UdCameraUnproject* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_camera_unproject: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdCameraUnproject& d = *desc;
  if (d.B < 1 || d.B > UD_RECON_MAX_B || d.H < 1 || d.W < 1 || d.n_points < 0 || d.n_points > UD_MAX_ELEMS) {
    ud_set_error("ud_camera_unproject: bad sizes (1 <= B <= 256, H, W >= 1, 0 <= n_points < 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.params || !d.rays) {
    ud_set_error("ud_camera_unproject: null pointer (params, rays)");
    return UD_ERR_BAD_ARG;
  }
  if (d.uv && (d.point_stride < 1 || d.comp_stride < 1 || d.batch_stride < 0)) {
    ud_set_error("ud_camera_unproject: bad strides (point_stride, comp_stride >= 1, batch_stride >= 0)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.uv && d.n_points != (long long)d.H * d.W) {
    ud_set_error("ud_camera_unproject: the identity grid (uv = NULL) needs n_points = H * W");
    return UD_ERR_BAD_ARG;
  }
  if (d.normalize && d.depth) {
    ud_set_error("ud_camera_unproject: normalize and depth exclude each other");
    return UD_ERR_BAD_ARG;
  }
  UpArgs a;
  a.uv = d.uv; a.params = d.params; a.depth = d.depth; a.rays = d.rays; a.valid = d.valid; a.maxres = nullptr;
  a.bs = d.batch_stride; a.ps = d.point_stride; a.cs = d.comp_stride;
  a.n = (int)d.n_points; a.W = d.W; a.rays_rows = d.rays_rows; a.n_iter = 0;
  a.form = d.depth ? UD_UNPROJ_DEPTH : (d.normalize ? UD_UNPROJ_NORMALIZE : UD_UNPROJ_RAW);
  for (int b = 0; b < UD_RECON_MAX_B; ++b) {
    a.model[b] = 0; a.slot_of_img[b] = 0; a.img_of_slot[b] = 0;
  }
  for (int b = 0; b < d.B; ++b) {
    const int m = d.model[b];
    if (!ud_cam_model_ok(m)) {
      ud_set_error("ud_camera_unproject: model tag outside 1..6");
      return UD_ERR_BAD_ARG;
    }
    a.model[b] = (unsigned char)m;
    if (m == UD_CAM_OPENCV || m == UD_CAM_FISHEYE624) {
      a.slot_of_img[b] = (short)a.n_iter;
      a.img_of_slot[a.n_iter] = (short)b;
      ++a.n_iter;
    }
  }
  if (a.n_iter > 0) {
    if (!d.work) {
      ud_set_error("ud_camera_unproject: null pointer (work, with an OPENCV / Fisheye624 member)");
      return UD_ERR_BAD_ARG;
    }
    if ((uintptr_t)d.work & 15) {
      ud_set_error("ud_camera_unproject: work not 16-byte aligned");
      return UD_ERR_BAD_ARG;
    }
    if (d.work_bytes < (long long)up_maxres_bytes(a.n_iter)) {
      ud_set_error("ud_camera_unproject: workspace smaller than ud_camera_unproject_work_bytes()");
      return UD_ERR_BAD_ARG;
    }
    a.maxres = (float*)d.work;
  }
  if (d.n_points == 0) return UD_OK;
  hipStream_t s = (hipStream_t)stream;
  if (a.n_iter > 0) {
    const int words = a.n_iter * UP_MAXRES;
    hipLaunchKernelGGL(up_clear_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, a.maxres, words);
  }
  const unsigned nblk = (unsigned)((d.n_points + UP_THREADS - 1) / UP_THREADS);
  hipLaunchKernelGGL(up_first_kernel, dim3(nblk, (unsigned)d.B), dim3(UP_THREADS), 0, s, a);
  if (a.n_iter > 0) hipLaunchKernelGGL(up_second_kernel, dim3(nblk, (unsigned)a.n_iter), dim3(UP_THREADS), 0, s, a);
  UD_CHECK_LAUNCH("ud_camera_unproject launch");
  return UD_OK;
}
