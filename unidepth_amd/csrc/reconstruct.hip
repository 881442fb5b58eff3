// Ground-truth point maps of a batch (include/unidepth_hip.h, UdReconstruct): the device form of the reference's
// Camera.reconstruct (unidepth/utils/camera.py: base :69-76, Pinhole :254-273, EUCM :307-328, Spherical :371-392, OPENCV :496-694,
// Fisheye624 :778-974, MEI :985-1082), one camera model per image, as the validation loop's add_points needs it
// (datasets/base_dataset.py:180-216).  Not the ray kernels of pointwise.hip followed by a product: reconstruct does not normalise,
// clamps differently for each model and runs at ground-truth resolution with one camera per image.
//
//   no OPENCV / Fisheye624 image:  rc_first_kernel alone, blockIdx.y = image, the model uniform per workgroup
//   otherwise:                     rc_first_kernel (closed-form images complete; iterative images: tangential / thin-prism Newton,
//                                  theta_0, trust radius, largest residual at theta_0) -> 10 x rc_step_kernel -> rc_final_kernel
//                                  (direction and the depth product), the last two kinds over the iterative images only.
// The method is the one of pointwise.hip's rays_iter_* kernels: step launch `it` looks at maxres[slot][it], the largest |residual| of
// ITS image at theta_it (one atomicMax per wave on the bit pattern of a non-negative float), and returns at once when the reference
// would have left the loop.  Every member of a BatchCamera runs its own loop in the reference, hence one row of maxima per image.
// The maxima are cleared by a memset node at the head of the call, so a captured graph replays correctly.  No grid barrier.
// Built with -ffp-contract=off: every operation rounds separately, as the numpy fp32 restatement in tools/make_golden_gt_points.py.
#include "ud_common.h"
#include "camera_models.h"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_ITERS = 10;                        // max_iters of the radial loop (camera.py:496, :778)
constexpr int RC_MAXRES = RC_ITERS + 1;             // maxima per iterative image: at theta_0 .. theta_10

enum { RC_PINHOLE = 1, RC_EUCM = 2, RC_SPHERICAL = 3, RC_OPENCV = 4, RC_FISHEYE624 = 5, RC_MEI = 6 };

struct RcArgs {
  const float* depth; const float* params; float* points;
  float4* st; unsigned* maxres;
  int B, W, HW, n_iter;
  unsigned char model[UD_RECON_MAX_B];
  short slot_of_img[UD_RECON_MAX_B];               // image -> its row of st / maxres (iterative images only)
  short img_of_slot[UD_RECON_MAX_B];               // the index table the step and final grids run over
};

size_t rc_up16(size_t v) { return (v + 15) & ~(size_t)15; }
size_t rc_maxres_bytes(int n_iter) { return rc_up16((size_t)n_iter * RC_MAXRES * sizeof(unsigned)); }

bool rc_sizes_ok(int B, int H, int W) {
  return B >= 1 && B <= UD_RECON_MAX_B && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL - RC_THREADS;
}

// max(x, m) that lets a NaN through, as torch.clamp(min=m) does (pointwise.hip rays_kernel writes its norm floor the same way)
__device__ __forceinline__ float rc_floor(float x, float m) { return x < m ? m : x; }

__device__ __forceinline__ bool rc_use_radial(const float* p) {
  return fabsf(p[4]) + fabsf(p[5]) + fabsf(p[6]) + fabsf(p[7]) + fabsf(p[8]) + fabsf(p[9]) > 1e-6f;
}

// largest value of the wave -> one atomicMax; a NaN compares above every finite value as a bit pattern as well: the loop then runs
// on, as `nan < eps` is false in the reference.  Every lane of the wave calls this.
__device__ __forceinline__ void rc_publish_max(float r, unsigned* slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float other = __shfl_xor(r, o, 64);
    r = (other > r || other != other) ? other : r;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(slot, __float_as_uint(r));
}

// Camera.reconstruct of the base class (camera.py:69-76): rays / rays.z.clamp(1e-4) * depth.clamp(1e-4)
__device__ __forceinline__ void rc_store_base(float* out, size_t HW, float x, float y, float z, float d) {
  const float zc = rc_floor(z, 1e-4f), dc = rc_floor(d, 1e-4f);
  out[0] = x / zc * dc; out[HW] = y / zc * dc; out[2 * HW] = z / zc * dc;
}

__global__ __launch_bounds__(RC_THREADS) void rc_first_kernel(const RcArgs a) {
  const int b = blockIdx.y;
  const int model = a.model[b];
  const float* p = a.params + (size_t)b * 16;
  const size_t HW = (size_t)a.HW;
  const int pix = blockIdx.x * RC_THREADS + threadIdx.x;          // < H * W + 256 <= 2^31 - 1: checked on the host
  const bool in = pix < a.HW;
  const int v = pix / a.W, u = pix - v * a.W;
  const float uf = (float)u + 0.5f, vf = (float)v + 0.5f;
  if (model == RC_OPENCV || model == RC_FISHEYE624) {
    const int slot = a.slot_of_img[b];
    const bool use_tan = fabsf(p[10]) + fabsf(p[11]) > 1e-6f;
    const bool use_prism = fabsf(p[12]) + fabsf(p[13]) + fabsf(p[14]) + fabsf(p[15]) > 1e-6f;
    const bool use_radial = rc_use_radial(p);
    float r = 0.0f;
    if (in) {
      const float ud = (uf - p[2]) / p[0], vd = (vf - p[3]) / p[1];
      float xr, yr;
      ud_cam_undistort_tanprism(ud, vd, p[10], p[11], p[12], p[13], p[14], p[15], use_tan, use_prism, (use_tan || use_prism) ? RC_ITERS : 0, xr, yr);
      const float rnorm = sqrtf(xr * xr + yr * yr);
      a.st[(size_t)slot * HW + pix] = make_float4(xr, yr, rnorm, 0.1f);
      if (use_radial) r = fabsf(ud_cam_radial_residual(p + 4, model == RC_FISHEYE624 ? 6 : 3, rnorm, rnorm));
    }
    if (use_radial) rc_publish_max(r, a.maxres + slot * RC_MAXRES);
    return;
  }
  if (!in) return;
  const float d = a.depth[(size_t)b * HW + pix];
  float* out = a.points + (size_t)b * 3 * HW + pix;
  if (model == RC_PINHOLE) {
    // K^-1 [u, v, 1] with the closed-form inverse of a skew-free K, as one subtraction and one division per axis: exactly 0 on the
    // principal point and one rounding away from it, where u / fx - cx / fx would cancel; then camera.py:263 and :272
    const float x = (uf - p[2]) / p[0];
    const float y = (vf - p[3]) / p[1];
    // r.z: the last row of K^-1 is [0 0 1] for finite intrinsics only; a NaN intrinsic makes the whole inverse NaN in the reference
    const float z = 0.0f * (p[0] + p[1] + p[2] + p[3]) + 1.0f;
    const float zc = rc_floor(z, 1e-4f), dc = rc_floor(d, 0.0f);
    out[0] = x / zc * dc; out[HW] = y / zc * dc; out[2 * HW] = z / zc * dc;
  } else if (model == RC_EUCM) {
    const float al = p[4], be = p[5];
    const float mx = (uf - p[2]) / p[0], my = (vf - p[3]) / p[1];
    const float r2 = mx * mx + my * my;
    const float sv = 1.0f - (2.0f * al - 1.0f) * be * r2;
    const float mz = (1.0f - be * (al * al) * r2) / (al * sqrtf(rc_floor(sv, 1e-5f)) + (1.0f - al));
    const float cf = 1.0f / sqrtf(mx * mx + my * my + mz * mz + 1e-5f);
    rc_store_base(out, HW, cf * mx, cf * my, rc_floor(cf * mz, 1e-3f), d);
  } else if (model == RC_SPHERICAL) {
    const float lon = (uf - (p[4] - 1.0f) / 2.0f) / (p[4] - 1.0f) * (2.0f * p[6]);
    const float lat = (vf - (p[5] - 1.0f) / 2.0f) / (p[5] - 1.0f) * (2.0f * p[7]);
    const float cl = cosf(lat);
    const float x = cl * sinf(lon), y = sinf(lat), z = cl * cosf(lon);
    const float n = rc_floor(sqrtf(x * x + y * y + z * z), 1e-5f);
    out[0] = x / n * d; out[HW] = y / n * d; out[2 * HW] = z / n * d;
  } else {                                                          // RC_MEI: fully per pixel
    float dx, dy, pz;
    ud_cam_mei_dir(p, uf, vf, dx, dy, pz);
    rc_store_base(out, HW, dx, dy, pz, d);
  }
}

__global__ __launch_bounds__(RC_THREADS) void rc_step_kernel(const RcArgs a, int it) {
  const int slot = blockIdx.y;
  const int b = a.img_of_slot[slot];
  const float* p = a.params + (size_t)b * 16;
  if (!rc_use_radial(p)) return;
  unsigned* mr = a.maxres + slot * RC_MAXRES;
  if (__uint_as_float(mr[it]) < UD_CAM_EPS) return;               // this image left the loop at (or before) this iteration
  const int nk = a.model[b] == RC_FISHEYE624 ? 6 : 3;
  const int pix = blockIdx.x * RC_THREADS + threadIdx.x;
  float r = 0.0f;
  if (pix < a.HW) {
    float4* sp = a.st + (size_t)slot * a.HW + pix;
    float4 s = *sp;
    const float rnorm = sqrtf(s.x * s.x + s.y * s.y);
    ud_cam_radial_step(p + 4, nk, rnorm, s.z, s.w);
    *sp = s;
    r = fabsf(ud_cam_radial_residual(p + 4, nk, s.z, rnorm));
  }
  rc_publish_max(r, mr + it + 1);
}

__global__ __launch_bounds__(RC_THREADS) void rc_final_kernel(const RcArgs a) {
  const int slot = blockIdx.y;
  const int b = a.img_of_slot[slot];
  const int pix = blockIdx.x * RC_THREADS + threadIdx.x;
  if (pix >= a.HW) return;
  const size_t HW = (size_t)a.HW;
  const float4 s = a.st[(size_t)slot * HW + pix];
  float dx, dy;
  ud_cam_finish_radial_dir(s.x, s.y, sqrtf(s.x * s.x + s.y * s.y), s.z, a.model[b] == RC_FISHEYE624, dx, dy);
  rc_store_base(a.points + (size_t)b * 3 * HW + pix, HW, dx, dy, 1.0f, a.depth[(size_t)b * HW + pix]);
}

}  // namespace

extern "C" long long ud_reconstruct_work_bytes(int B, int H, int W, int n_iterative) {
  if (!rc_sizes_ok(B, H, W) || n_iterative < 0 || n_iterative > B) return -1;
  if (n_iterative == 0) return 0;
  return (long long)(rc_maxres_bytes(n_iterative) + (size_t)n_iterative * H * W * sizeof(float4));
}

extern "C" int ud_reconstruct(const UdReconstruct* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_reconstruct: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdReconstruct& d = *desc;
  if (!rc_sizes_ok(d.B, d.H, d.W)) {
    ud_set_error("ud_reconstruct: bad sizes (1 <= B <= 256, H, W >= 1, H*W < 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.depth || !d.params || !d.points) {
    ud_set_error("ud_reconstruct: null pointer");
    return UD_ERR_BAD_ARG;
  }
  RcArgs a;
  a.depth = d.depth; a.params = d.params; a.points = d.points; a.st = nullptr; a.maxres = nullptr;
  a.B = d.B; a.W = d.W; a.HW = d.H * d.W; a.n_iter = 0;
  for (int b = 0; b < UD_RECON_MAX_B; ++b) {
    a.model[b] = 0; a.slot_of_img[b] = 0; a.img_of_slot[b] = 0;
  }
  for (int b = 0; b < d.B; ++b) {
    const int m = d.model[b];
    if (!ud_cam_model_ok(m)) {
      ud_set_error("ud_reconstruct: model tag outside 1..6");
      return UD_ERR_BAD_ARG;
    }
    a.model[b] = (unsigned char)m;
    if (m == RC_OPENCV || m == RC_FISHEYE624) {
      a.slot_of_img[b] = (short)a.n_iter;
      a.img_of_slot[a.n_iter] = (short)b;
      ++a.n_iter;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  if (a.n_iter > 0) {
    if (!d.work) {
      ud_set_error("ud_reconstruct: null pointer");
      return UD_ERR_BAD_ARG;
    }
    if ((uintptr_t)d.work & 15) {
      ud_set_error("ud_reconstruct: work not 16-byte aligned");
      return UD_ERR_BAD_ARG;
    }
    if (d.work_bytes < ud_reconstruct_work_bytes(d.B, d.H, d.W, a.n_iter)) {
      ud_set_error("ud_reconstruct: workspace smaller than ud_reconstruct_work_bytes()");
      return UD_ERR_BAD_ARG;
    }
    a.maxres = (unsigned*)d.work;
    a.st = (float4*)((char*)d.work + rc_maxres_bytes(a.n_iter));
    if (hipMemsetAsync(a.maxres, 0, (size_t)a.n_iter * RC_MAXRES * sizeof(unsigned), s) != hipSuccess) {
      ud_set_error("ud_reconstruct: memset of the residual maxima failed");
      return UD_ERR_LAUNCH;
    }
  }
  const unsigned nblk = (unsigned)(((long long)a.HW + RC_THREADS - 1) / RC_THREADS);
  const dim3 blk(RC_THREADS);
  hipLaunchKernelGGL(rc_first_kernel, dim3(nblk, (unsigned)d.B), blk, 0, s, a);
  if (a.n_iter > 0) {
    const dim3 grid(nblk, (unsigned)a.n_iter);
    for (int it = 0; it < RC_ITERS; ++it) hipLaunchKernelGGL(rc_step_kernel, grid, blk, 0, s, a, it);
    hipLaunchKernelGGL(rc_final_kernel, grid, blk, 0, s, a);
  }
  UD_CHECK_LAUNCH("ud_reconstruct launch");
  return UD_OK;
}
