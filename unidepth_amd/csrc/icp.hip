// Frame-to-model point-to-plane ICP, one Gauss-Newton step in TWO launches (include/unidepth_hip.h, UdIcp): a depth frame (or a point
// map) aligned to the point and normal maps of a model view -- what tsdf_render predicts -- under the current estimate T.  Per frame pixel
// it is ud_reconstruct -> the rigid motion -> ud_camera_project -> ud_remap(nearest) and a dozen element-wise passes fused; the 6 x 6
// normal system is summed in fp64 in a FIXED order, so the result does not depend on scheduling: no floating-point atomics anywhere.
//
//   icp_rows_kernel    blockIdx.y = image, gridDim.x = nblk workgroups of 256 threads per image; a thread walks the pixels
//                      blockIdx.x * 256 + threadIdx.x + k * nblk * 256 in order, calls ud_icp_row and keeps its 30 fp64 sums in
//                      registers.  The wave's 64 threads are then summed by the xor butterfly 32, 16, 8, 4, 2, 1 (lane 0's value:
//                      ((((l0 + l32) + (l16 + l48)) + ...)), the four waves' sums in wave order by threads 0 .. 29 through LDS, and the
//                      workgroup's partial [32] (slots 30, 31 zero) is written to the workspace [B, nblk, 32].  Every workgroup writes
//                      its partial, pixels or not: the workspace is never read before it is written.
//   icp_solve_kernel   one workgroup of 256 threads per image: the partials of 128 workgroups at a time are loaded into LDS by all threads
//                      (16 independent loads each), then threads 0 .. 31 each add one slot's column in block-index order and write
//                      system[b]; thread 0 then runs ud_icp_solve on it, updates T[b] in place and writes x, status and the stats row.
//                      ud_icp_update launches it alone, on a given system.
//
// nblk = min(ceil(H * W / 256), 256) by default: one pixel per thread up to 65,536 pixels (the grid-stride span), then 256 workgroups per
// image, one per compute unit of the device, with B images side by side in blockIdx.y.  UdIcp.blocks replaces the 256 by up to 1024 for
// measurement (tools/bench_icp.py; DESIGN.md has the figures).  The two kernels are NOT folded into one with a last-block counter: two
// launches per iteration is the design.
//
// The arithmetic is csrc/icp_point.h, which only calls csrc/camera_models.h and csrc/remap_taps.h; the host build of the tests runs it
// under the sanitizers.  Built with -ffp-contract=off: every operation rounds separately, in fp32 and in fp64.
#include <math.h>
#include "ud_common.h"
#include "icp_point.h"
#pragma clang fp contract(off)

namespace {

constexpr int ICP_THREADS = 256;
constexpr int ICP_BLOCKS = 256;                        // the default number of workgroups per image, at most
constexpr int ICP_MAX_BLOCKS = 1024;                   // what UdIcp.blocks may ask for, and what the workspace is sized for
constexpr int ICP_SOLVE_THREADS = 256;
constexpr int ICP_CHUNK = 128;

struct IcpKernelArgs {
  UdIcpArgs p;
  double* work;                                        // [B, nblk, 32]
  unsigned char model_frame[UD_RECON_MAX_B], model_model[UD_RECON_MAX_B];
};

struct IcpSolveArgs {
  const double* work; double* system; float* T; double* x; unsigned char* status; double* stats;
  long long stats_stride;
  double damping;
  int nblk, sum, solve, min_count;
};

__device__ __forceinline__ double icp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(ICP_THREADS) void icp_rows_kernel(const IcpKernelArgs a) {
  __shared__ double red[ICP_THREADS / 64][UD_ICP_SLOTS];
  const int b = blockIdx.y;
  const int mf = a.model_frame[b], mm = a.model_model[b];
  double acc[UD_ICP_SUMS];
#pragma unroll
  for (int k = 0; k < UD_ICP_SUMS; ++k) acc[k] = 0.0;
  const long long stride = (long long)gridDim.x * ICP_THREADS;
  for (long long i = (long long)blockIdx.x * ICP_THREADS + threadIdx.x; i < a.p.n; i += stride) {
    UdIcpRow row;
    if (ud_icp_row(a.p, mf, mm, b, i, &row)) ud_icp_accumulate(acc, row);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < UD_ICP_SUMS; ++k) {
    const double s = icp_wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < UD_ICP_SLOTS) {
    double s = 0.0;
    if (threadIdx.x < UD_ICP_SUMS) {
      s = red[0][threadIdx.x];
      for (int w = 1; w < ICP_THREADS / 64; ++w) s = s + red[w][threadIdx.x];
    }
    a.work[((size_t)b * gridDim.x + blockIdx.x) * UD_ICP_SLOTS + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(ICP_SOLVE_THREADS) void icp_solve_kernel(const IcpSolveArgs a) {
  __shared__ double stage[ICP_CHUNK][UD_ICP_SLOTS];
  __shared__ double S[UD_ICP_SLOTS];
  const int b = blockIdx.x, t = threadIdx.x, slot = t & (UD_ICP_SLOTS - 1), row = t / UD_ICP_SLOTS;
  if (a.sum) {
    // the partials of ICP_CHUNK workgroups at a time: all 256 threads load (16 independent loads each, a row of 32 slots coalesced),
    // then threads 0 .. 31 add their slot's column in block-index order
    constexpr int ROWS = ICP_SOLVE_THREADS / UD_ICP_SLOTS;
    const double* src = a.work + (size_t)b * (size_t)a.nblk * UD_ICP_SLOTS;
    double s = 0.0;
    for (int k0 = 0; k0 < a.nblk; k0 += ICP_CHUNK) {
      const int m = a.nblk - k0 < ICP_CHUNK ? a.nblk - k0 : ICP_CHUNK;
      double v[ICP_CHUNK / ROWS];                        // every load issued before the first store waits for one
#pragma unroll
      for (int j = 0; j < ICP_CHUNK / ROWS; ++j) {
        const int r = row + j * ROWS;
        v[j] = r < m ? src[(size_t)(k0 + r) * UD_ICP_SLOTS + slot] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < ICP_CHUNK / ROWS; ++j) stage[row + j * ROWS][slot] = v[j];
      __syncthreads();
      if (t < UD_ICP_SLOTS) {
        int j = 0;
        if (k0 == 0) s = stage[j++][slot];               // the sum starts AT the first partial, not at 0
#pragma unroll 16
        for (; j < m; ++j) s = s + stage[j][slot];       // reads ahead of the adds: only the adds are serial
      }
      __syncthreads();
    }
    if (t < UD_ICP_SLOTS) {
      a.system[(size_t)b * UD_ICP_SLOTS + t] = s;
      S[t] = s;
    }
  } else if (t < UD_ICP_SLOTS) {
    S[t] = a.system[(size_t)b * UD_ICP_SLOTS + t];
  }
  __syncthreads();
  if (t == 0 && a.solve) {
    float T[12];
    double x[6];
    for (int k = 0; k < 12; ++k) T[k] = a.T[(size_t)b * 12 + k];
    const int status = ud_icp_solve(S, a.damping, a.min_count, T, x);
    if (status)
      for (int k = 0; k < 12; ++k) a.T[(size_t)b * 12 + k] = T[k];
    if (a.x)
      for (int k = 0; k < 6; ++k) a.x[(size_t)b * 6 + k] = x[k];
    if (a.status) a.status[b] = (unsigned char)status;
    if (a.stats) {
      double* st = a.stats + (size_t)b * (size_t)a.stats_stride;
      st[0] = S[27]; st[1] = S[28]; st[2] = S[29]; st[3] = (double)status;
    }
  }
}

int icp_blocks(long long n, int cap) {
  const long long k = (n + ICP_THREADS - 1) / ICP_THREADS;
  return (int)(k < cap ? k : cap);
}

double icp_f64_from_bits(long long bits) {
  union { long long i; double f; } u;
  u.i = bits;
  return u.f;
}

// the checks of the second launch, shared by both entry points
int icp_check_solve(const UdIcp& d, const char* fn, double* damping) {
  char msg[200];
  if (!d.T) {
    snprintf(msg, sizeof(msg), "%s: null pointer (T)", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  if (d.nT != d.B) {
    snprintf(msg, sizeof(msg), "%s: the solve updates T in place and needs one matrix per image (nT = B)", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  *damping = icp_f64_from_bits(d.damping_bits);
  if (!(*damping >= 0.0 && *damping <= 1.7976931348623157e308)) {
    snprintf(msg, sizeof(msg), "%s: damping must be finite and not negative", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  if (d.min_count < 0) {
    snprintf(msg, sizeof(msg), "%s: min_count must not be negative", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  if (d.stats && d.stats_stride < 4) {
    snprintf(msg, sizeof(msg), "%s: stats_stride must be at least 4", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  return UD_OK;
}

}  // namespace

extern "C" long long ud_icp_workspace_bytes(int B, int H, int W) {
  if (B < 1 || B > UD_RECON_MAX_B || H < 1 || W < 1 || (long long)H * W >= UD_MAX_ELEMS) return -1;
  return (long long)B * icp_blocks((long long)H * W, ICP_MAX_BLOCKS) * UD_ICP_SLOTS * (long long)sizeof(double);
}

extern "C" int ud_icp_linearize(const UdIcp* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_icp_linearize: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdIcp& d = *desc;
  if (d.B < 1 || d.B > UD_RECON_MAX_B || d.H < 1 || d.W < 1 || d.Hm < 1 || d.Wm < 1) {
    ud_set_error("ud_icp_linearize: bad sizes (1 <= B <= 256, H, W, Hm, Wm >= 1)");
    return UD_ERR_BAD_ARG;
  }
  const long long n = (long long)d.H * d.W, hw = (long long)d.Hm * d.Wm;
  if (6 * n >= UD_MAX_ELEMS || 3 * hw >= UD_MAX_ELEMS) {
    ud_set_error("ud_icp_linearize: too large (6 * H * W and 3 * Hm * Wm must stay below 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if ((d.depth != nullptr) == (d.points != nullptr)) {
    ud_set_error("ud_icp_linearize: exactly one of depth and points");
    return UD_ERR_BAD_ARG;
  }
  if ((d.depth && !d.params) || !d.model_points || !d.model_normals || !d.model_valid || !d.params_model || !d.T || !d.work || !d.system) {
    ud_set_error("ud_icp_linearize: null pointer (params with depth, model_points, model_normals, model_valid, params_model, T, work, system)");
    return UD_ERR_BAD_ARG;
  }
  if (d.nT != 1 && d.nT != d.B) {
    ud_set_error("ud_icp_linearize: nT must be 1 or B");
    return UD_ERR_BAD_ARG;
  }
  const float dist_tol = ud_f32_from_bits(d.dist_tol_bits), cos_tol = ud_f32_from_bits(d.cos_tol_bits);
  if (!ud_tolerance_ok(dist_tol)) {
    ud_set_error("ud_icp_linearize: dist_tol must be finite and not negative");
    return UD_ERR_BAD_ARG;
  }
  if (d.has_cos && !(cos_tol >= -1.0f && cos_tol <= 1.0f)) {
    ud_set_error("ud_icp_linearize: cos_tol must lie in -1 .. 1");
    return UD_ERR_BAD_ARG;
  }
  if (d.has_cos && !d.normals) {
    ud_set_error("ud_icp_linearize: cos_tol needs the frame's normals");
    return UD_ERR_BAD_ARG;
  }
  if (d.blocks < 0 || d.blocks > ICP_MAX_BLOCKS) {
    ud_set_error("ud_icp_linearize: blocks must lie in 0 .. 1024 (0: the default)");
    return UD_ERR_BAD_ARG;
  }
  const int nblk = icp_blocks(n, d.blocks ? d.blocks : ICP_BLOCKS);
  if (d.work_bytes < ud_icp_workspace_bytes(d.B, d.H, d.W)) {
    ud_set_error("ud_icp_linearize: workspace smaller than ud_icp_workspace_bytes(B, H, W)");
    return UD_ERR_BAD_ARG;
  }
  double damping = 0.0;
  if (d.solve) {
    const int rc = icp_check_solve(d, "ud_icp_linearize", &damping);
    if (rc != UD_OK) return rc;
  }
  for (int b = 0; b < d.B; ++b) {
    if (!ud_cam_model_ok(d.model_model[b]) || (d.depth && !ud_cam_model_ok(d.model_frame[b]))) {
      ud_set_error("ud_icp_linearize: model tag outside 1..6");
      return UD_ERR_BAD_ARG;
    }
    if (d.depth && !ud_cam_closed_form(d.model_frame[b])) {
      ud_set_error("ud_icp_linearize: iterative frame model (OPENCV / Fisheye624) in the depth form: its unprojection ends on a maximum over the image; pass the frame's points");
      return UD_ERR_BAD_ARG;
    }
  }
  IcpKernelArgs a;
  a.p.depth = d.depth; a.p.points = d.points; a.p.params = d.params; a.p.mask = d.mask; a.p.weights = d.weights; a.p.normals = d.normals;
  a.p.model_points = d.model_points; a.p.model_normals = d.model_normals; a.p.model_valid = d.model_valid; a.p.params_model = d.params_model;
  a.p.T = d.T; a.p.matched = d.matched; a.p.residual = d.residual; a.p.rows = d.rows;
  a.p.n = n;
  a.p.tol2 = dist_tol * dist_tol;
  a.p.cos_tol = cos_tol;
  a.p.B = d.B; a.p.H = d.H; a.p.W = d.W; a.p.Hm = d.Hm; a.p.Wm = d.Wm; a.p.nT = d.nT; a.p.has_cos = d.has_cos ? 1 : 0;
  a.work = (double*)d.work;
  ud_copy_models(a.model_frame, d.model_frame, d.depth ? d.B : 0);
  ud_copy_models(a.model_model, d.model_model, d.B);
  hipLaunchKernelGGL(icp_rows_kernel, dim3((unsigned)nblk, (unsigned)d.B), dim3(ICP_THREADS), 0, (hipStream_t)stream, a);
  UD_CHECK_LAUNCH("ud_icp_linearize rows launch");
  IcpSolveArgs s;
  s.work = (const double*)d.work; s.system = d.system; s.T = d.T; s.x = d.x; s.status = d.status; s.stats = d.stats;
  s.stats_stride = d.stats_stride; s.damping = damping; s.nblk = nblk; s.sum = 1; s.solve = d.solve ? 1 : 0; s.min_count = d.min_count;
  hipLaunchKernelGGL(icp_solve_kernel, dim3((unsigned)d.B), dim3(ICP_SOLVE_THREADS), 0, (hipStream_t)stream, s);
  UD_CHECK_LAUNCH("ud_icp_linearize solve launch");
  return UD_OK;
}

extern "C" int ud_icp_update(const UdIcp* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_icp_update: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdIcp& d = *desc;
  if (d.B < 1 || d.B > UD_RECON_MAX_B) {
    ud_set_error("ud_icp_update: bad sizes (1 <= B <= 256)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.system) {
    ud_set_error("ud_icp_update: null pointer (system)");
    return UD_ERR_BAD_ARG;
  }
  double damping = 0.0;
  const int rc = icp_check_solve(d, "ud_icp_update", &damping);
  if (rc != UD_OK) return rc;
  IcpSolveArgs s;
  s.work = nullptr; s.system = d.system; s.T = d.T; s.x = d.x; s.status = d.status; s.stats = d.stats;
  s.stats_stride = d.stats_stride; s.damping = damping; s.nblk = 0; s.sum = 0; s.solve = 1; s.min_count = d.min_count;
  hipLaunchKernelGGL(icp_solve_kernel, dim3((unsigned)d.B), dim3(ICP_SOLVE_THREADS), 0, (hipStream_t)stream, s);
  UD_CHECK_LAUNCH("ud_icp_update launch");
  return UD_OK;
}
