// Point clouds of a batch splatted into depth maps (include/unidepth_hip.h, UdSplat), the device form of the reference's project_points
// (unidepth/utils/geometric.py:161-204: a per-image loop of scatter_add_, mean depth per pixel) plus the z-buffer a re-rendered view
// needs, and the reference's hole-aware min-pool `downsample` (geometric.py:208-224; UdDepthMinPool).
//
// Three launches on the caller's stream:
//   1. sp_fill_kernel     every destination pixel's work word: ~0 (nearest: no key yet) or 0 (mean: an empty sum), and its count word
//   2. sp_splat_kernel    one thread per source point: transform, project, pick the cell, ONE 64-bit integer atomic on the cell's word
//                         (+ a 32-bit add on its count word when counts are kept).  A workgroup takes SP_CHUNK = 1024 consecutive points
//                         of one image (256 threads x 4): thread `tid` handles the points c * 1024 + j * 256 + tid, so planar sources are
//                         read with coalesced dword loads per plane and packed rows with one 12-byte load per lane.
//   3. sp_resolve_kernel  one thread per destination pixel (SP_RTILE = 256 consecutive pixels per workgroup): the word -> depth, and the
//                         winner's index / gathered colour / the count.
// Every dependency is a launch boundary: no tickets, no spinning, no host synchronisation, no float atomics.  Nearest mode is an
// atomicMin on (bits(z') << 32 | r): z' > 0, so the integer order of the keys IS the (z', r) lexicographic order and the winner does not
// depend on arrival order.  Mean mode sums llrintf(z' * 2^24) in an int64: integer addition is associative, so neither does the sum.
// ud_splat_camera (UdSplatCamera) is the same three launches with the projector exchanged: sp_splat_kernel takes it as a template parameter,
// SpProjMatrix (UdSplat's 3x3 matrix) or SpProjCamera (the camera model of the point's image, camera_models.h ud_cam_project).
// Built with -ffp-contract=off: the cell a point lands in must be the one a numpy fp32 restatement computes.
#include "ud_common.h"
#include "camera_models.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_STEPS = 4;
constexpr int SP_CHUNK = SP_THREADS * SP_STEPS;      // points per workgroup of the splat pass
constexpr int SP_RTILE = 256;                        // pixels per workgroup of the fill and resolve passes
constexpr unsigned long long SP_EMPTY = ~0ull;       // above every key: bits(z') <= 0x7f800000
constexpr float SP_Q = 16777216.0f;                  // 2^24: the mean mode's fixed point
constexpr float SP_ZMAX = 1048576.0f;                // 2^20: |z'| beyond it is dropped in mean mode
constexpr unsigned SP_CMAX = 1u << 19;               // 2^19 points of |z'| <= 2^20 in Q24 reach 2^63: the accumulator's headroom

struct SpArgs {
  const float* xyz; const long long* offsets; const float* K; const float* T; const void* color;
  float* depth; int* index; void* rgb; int* count;
  unsigned long long* words; unsigned* counts;
  long long bs, ps, cs;                              // element strides of xyz and color: batch, point, component
  long long n;                                       // points per image, or rows of the packed form
  int B, H, W, HW, nK, nT, mode, flags, color_f32;
  float pixel_offset, dmin, dmax;
};

__global__ __launch_bounds__(SP_RTILE) void sp_fill_kernel(SpArgs a) {
  const unsigned p = blockIdx.x * SP_RTILE + threadIdx.x;
  if (p >= (unsigned)a.HW) return;
  const size_t o = (size_t)blockIdx.y * a.HW + p;
  a.words[o] = a.mode == UD_SPLAT_NEAREST ? SP_EMPTY : 0ull;
  if (a.counts) a.counts[o] = 0u;
}

// the image that owns packed row `row`: the last b with offsets[b] <= row, found as upper_bound - 1.  Whatever the offsets hold, the
// result is in [-1, B] and the caller checks the row against the image's own range, so nothing is addressed through an unchecked value.
__device__ __forceinline__ int sp_find_image(const long long* offsets, int B, long long row) {
  int lo = 0, hi = B + 1;                            // first index in [0, B] whose offset is > row, or B + 1
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= row) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// cell of image coordinate u along an axis of n cells, or -1: decided in float (a NaN or an infinity fails every compare), converted after
__device__ __forceinline__ int sp_cell(float u, int n, bool trunc_mode) {
  const float f = trunc_mode ? truncf(u) : floorf(u);
  if (!(f >= 0.0f && f < 2147483648.0f)) return -1;  // -0.0f (trunc of (-1, 0), floor of -0.0f) passes, as the reference's .int() >= 0
  const int c = (int)f;
  return c < n ? c : -1;
}

// The projector of a splat: (x', y', z') of a point of image b -> image coordinates (before pixel_offset) and the point's depth, or
// false when the projector itself drops the point.
// SpProjMatrix: UdSplat's full 3x3 matrix; the depth is z'.
struct SpProjMatrix {
  __device__ __forceinline__ bool operator()(const SpArgs& a, int b, float x, float y, float z, float& u, float& v, float& dep) const {
    const float* k = a.K + (a.nK == 1 ? 0 : (size_t)b * 9);
    const float pa = (k[0] * x + k[1] * y) + k[2] * z;
    const float pb = (k[3] * x + k[4] * y) + k[5] * z;
    const float pw = (k[6] * x + k[7] * y) + k[8] * z;
    u = pa / pw;
    v = pb / pw;
    dep = z;
    return true;
  }
};

// SpProjCamera: UdSplatCamera's camera model of the image (camera_models.h); the depth is the model's (z', or the distance for Spherical)
struct SpProjCamera {
  const float* params;
  float cos_limit;
  unsigned char model[UD_RECON_MAX_B];
  __device__ __forceinline__ bool operator()(const SpArgs& a, int b, float x, float y, float z, float& u, float& v, float& dep) const {
    const int m = model[b];
    const float* p = params + (size_t)b * 16;
    if (m != UD_CAM_SPHERICAL && z <= 0.0f) return false;
    if (m == UD_CAM_MEI || m == UD_CAM_SPHERICAL || (a.flags & UD_SPLAT_FOV)) {
      const float n = sqrtf(x * x + y * y + z * z);
      if (m == UD_CAM_MEI && !(z + p[8] * n > 0.0f)) return false;
      if ((a.flags & UD_SPLAT_FOV) && !(z >= cos_limit * n)) return false;
    }
    ud_cam_project(m, p, x, y, z, &u, &v);
    dep = ud_cam_depth(m, x, y, z);
    return true;
  }
};

template <bool ROWS, class PROJ>
__global__ __launch_bounds__(SP_THREADS) void sp_splat_kernel(SpArgs a, const PROJ proj) {
  const int tid = threadIdx.x;
  const long long first = (long long)blockIdx.x * SP_CHUNK;
  const bool packed = a.offsets != nullptr;
  const bool trunc_mode = (a.flags & UD_SPLAT_TRUNC) != 0;
#pragma unroll
  for (int j = 0; j < SP_STEPS; ++j) {
    const long long i = first + j * SP_THREADS + tid;     // point of its image, or packed row
    if (i >= a.n) continue;
    int b = blockIdx.y;
    long long r = i;
    const float* src;
    if (packed) {
      b = sp_find_image(a.offsets, a.B, i);
      if (b < 0 || b >= a.B) continue;
      const long long o0 = a.offsets[b], o1 = a.offsets[b + 1];
      if (i < o0 || i >= o1) continue;                     // only with offsets that do not ascend
      r = i - o0;
      src = a.xyz + i * a.ps;
    } else {
      src = a.xyz + b * a.bs + i * a.ps;
    }
    float x, y, z;
    if (ROWS) {                                            // cs = 1: one 12-byte load
      struct __attribute__((packed, aligned(4))) Row { float v[3]; };
      const Row row = *(const Row*)src;
      x = row.v[0]; y = row.v[1]; z = row.v[2];
    } else {
      x = src[0]; y = src[a.cs]; z = src[2 * a.cs];
    }
    if (a.T) {                                             // ud_cam_move (camera_models.h) written out: the call changes this kernel's instruction schedule
      const float* t = a.T + (a.nT == 1 ? 0 : (size_t)b * 12);
      const float xt = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
      const float yt = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
      const float zt = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
      x = xt; y = yt; z = zt;
    }
    float u, v, dep;
    if (!proj(a, b, x, y, z, u, v, dep)) continue;
    z = dep;                                               // from here on the point's depth
    u = u + a.pixel_offset;
    v = v + a.pixel_offset;
    const int cx = sp_cell(u, a.W, trunc_mode), cy = sp_cell(v, a.H, trunc_mode);
    if (cx < 0 || cy < 0) continue;
    if ((a.flags & UD_SPLAT_RANGE) && !(z >= a.dmin && z <= a.dmax)) continue;
    const size_t o = (size_t)b * a.HW + (size_t)cy * a.W + cx;
    if (a.mode == UD_SPLAT_NEAREST) {
      if (!(z > 0.0f) || r > 0x7fffffffLL) continue;
      atomicMin(a.words + o, ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)r);
    } else {
      if (!(fabsf(z) <= SP_ZMAX)) continue;
      atomicAdd(a.words + o, (unsigned long long)llrintf(z * SP_Q));      // two's complement: an int64 sum
    }
    if (a.counts) atomicAdd(a.counts + o, 1u);
  }
}

__global__ __launch_bounds__(SP_RTILE) void sp_resolve_kernel(SpArgs a) {
  const unsigned p = blockIdx.x * SP_RTILE + threadIdx.x;
  if (p >= (unsigned)a.HW) return;
  const int b = blockIdx.y;
  const size_t o = (size_t)b * a.HW + p;
  const unsigned long long w = a.words[o];
  const unsigned c = a.counts ? a.counts[o] : 0u;
  if (a.count) a.count[o] = (int)c;
  if (a.mode == UD_SPLAT_MEAN) {
    float d = 0.0f;
    if (c >= SP_CMAX) d = __builtin_nanf("");
    else if (c) d = (float)((double)(long long)w / ((double)c * (double)SP_Q));
    a.depth[o] = d;
    return;
  }
  const bool hit = w != SP_EMPTY;
  a.depth[o] = hit ? __uint_as_float((unsigned)(w >> 32)) : 0.0f;
  const long long r = (long long)(unsigned)w;
  if (a.index) a.index[o] = hit ? (int)r : -1;
  if (a.rgb) {
    const size_t base = a.offsets ? (size_t)((a.offsets[b] + r) * a.ps) : (size_t)(b * a.bs + r * a.ps);
    const size_t q = (size_t)b * 3 * a.HW + p;
    if (a.color_f32) {
      const float* s = (const float*)a.color + base;
      float* t = (float*)a.rgb + q;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) t[(size_t)ch * a.HW] = hit ? s[ch * a.cs] : 0.0f;
    } else {
      const unsigned char* s = (const unsigned char*)a.color + base;
      unsigned char* t = (unsigned char*)a.rgb + q;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) t[(size_t)ch * a.HW] = hit ? s[ch * a.cs] : (unsigned char)0;
    }
  }
}

struct MpArgs {
  const float* src; float* dst;
  int Ho, Wo, W, f;
};

__global__ __launch_bounds__(SP_RTILE) void sp_minpool_kernel(MpArgs a) {
  const unsigned p = blockIdx.x * SP_RTILE + threadIdx.x;
  if (p >= (unsigned)(a.Ho * a.Wo)) return;
  const int yo = p / a.Wo, xo = p - yo * a.Wo;
  const float* s = a.src + (size_t)blockIdx.y * a.Ho * a.f * a.W + (size_t)yo * a.f * a.W + (size_t)xo * a.f;
  float m = __builtin_inff();
  bool nan = false;
  for (int dy = 0; dy < a.f; ++dy)
    for (int dx = 0; dx < a.f; ++dx) {
      float v = s[(size_t)dy * a.W + dx];
      if (v == 0.0f) v = 1e5f;
      nan |= v != v;                                       // torch.min returns NaN when the block holds one
      m = v < m ? v : m;
    }
  a.dst[(size_t)blockIdx.y * a.Ho * a.Wo + p] = nan ? __builtin_nanf("") : (m > 1000.0f ? 0.0f : m);
}

bool sp_sizes_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL; }

}  // namespace

extern "C" long long ud_splat_work_bytes(int B, int H, int W) {
  if (!sp_sizes_ok(B, H, W)) return -1;
  return (long long)B * H * W * 12;
}

namespace {

// the checks ud_splat and ud_splat_camera share, in two halves around the projector's own (sp_check_rest_and_fill also fills the SpArgs of the call).  `fn` names
// the entry point in the message; max_b and allowed_flags are the entry point's.
template <class D>
int sp_check_head(const D& d, const char* fn, int max_b, int allowed_flags) {
  char msg[256];
  if (!sp_sizes_ok(d.B, d.H, d.W) || d.B > max_b || d.n_points < 0 || d.n_points > 0x7fffffffLL) {
    snprintf(msg, sizeof(msg), "%s: bad sizes (1 <= B <= %d, H, W >= 1, H*W < 2^31, 0 <= n_points < 2^31)", fn, max_b);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  if (d.mode != UD_SPLAT_NEAREST && d.mode != UD_SPLAT_MEAN) {
    snprintf(msg, sizeof(msg), "%s: unknown mode (UD_SPLAT_NEAREST or UD_SPLAT_MEAN)", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  if (d.flags & ~allowed_flags) {
    snprintf(msg, sizeof(msg), "%s: unknown flag", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  if (!d.xyz || !d.depth || d.point_stride < 1 || d.comp_stride < 1 || d.batch_stride < 0) {
    snprintf(msg, sizeof(msg), "%s: null pointer (xyz, depth), or bad strides (point_stride, comp_stride >= 1, batch_stride >= 0)", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  return UD_OK;
}

template <class D>
int sp_check_rest_and_fill(const D& d, const char* fn, SpArgs& a) {
  char msg[256];
  if (d.T && d.nT != 1 && d.nT != d.B) {
    snprintf(msg, sizeof(msg), "%s: nT must be 1 or B when T is given", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  if ((d.color != nullptr) != (d.rgb != nullptr)) {
    snprintf(msg, sizeof(msg), "%s: color and rgb go together (a colour source and the image that receives it)", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  if (d.mode == UD_SPLAT_MEAN && (d.index || d.rgb)) {
    snprintf(msg, sizeof(msg), "%s: index and rgb are outputs of UD_SPLAT_NEAREST only", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  const bool counts = d.mode == UD_SPLAT_MEAN || d.count;
  const long long pixels = (long long)d.B * d.H * d.W;
  if (!d.work || ((uintptr_t)d.work & 7) || d.work_bytes < pixels * (counts ? 12 : 8)) {
    snprintf(msg, sizeof(msg), "%s: work is null, not 8-byte aligned, or smaller than 8 B per pixel (12 B with counts; ud_splat_work_bytes() covers both)", fn);
    ud_set_error(msg);
    return UD_ERR_BAD_ARG;
  }
  a.xyz = d.xyz; a.offsets = d.offsets; a.K = nullptr; a.T = d.T; a.color = d.color;
  a.depth = d.depth; a.index = d.index; a.rgb = d.rgb; a.count = d.count;
  a.words = (unsigned long long*)d.work;
  a.counts = counts ? (unsigned*)((char*)d.work + pixels * 8) : nullptr;
  a.bs = d.batch_stride; a.ps = d.point_stride; a.cs = d.comp_stride; a.n = d.n_points;
  a.B = d.B; a.H = d.H; a.W = d.W; a.HW = d.H * d.W; a.nK = 0; a.nT = d.nT; a.mode = d.mode; a.flags = d.flags; a.color_f32 = d.color_f32;
  a.pixel_offset = d.pixel_offset; a.dmin = d.dmin; a.dmax = d.dmax;
  return UD_OK;
}

// fill, splat (one thread per point through `proj`), resolve
template <class PROJ>
int sp_launch(const SpArgs& a, const PROJ& proj, void* stream, const char* what) {
  hipStream_t s = (hipStream_t)stream;
  const dim3 pix((unsigned)(((long long)a.HW + SP_RTILE - 1) / SP_RTILE), (unsigned)a.B);
  hipLaunchKernelGGL(sp_fill_kernel, pix, dim3(SP_RTILE), 0, s, a);
  if (a.n > 0) {
    const dim3 grid((unsigned)((a.n + SP_CHUNK - 1) / SP_CHUNK), a.offsets ? 1u : (unsigned)a.B);
    if (a.cs == 1) hipLaunchKernelGGL((sp_splat_kernel<true, PROJ>), grid, dim3(SP_THREADS), 0, s, a, proj);
    else hipLaunchKernelGGL((sp_splat_kernel<false, PROJ>), grid, dim3(SP_THREADS), 0, s, a, proj);
  }
  hipLaunchKernelGGL(sp_resolve_kernel, pix, dim3(SP_RTILE), 0, s, a);
  UD_CHECK_LAUNCH(what);
  return UD_OK;
}

}  // namespace

extern "C" int ud_splat(const UdSplat* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_splat: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdSplat& d = *desc;
  SpArgs a;
  int rc = sp_check_head(d, "ud_splat", 65535, UD_SPLAT_TRUNC | UD_SPLAT_RANGE);
  if (rc != UD_OK) return rc;
  if (!d.K || (d.nK != 1 && d.nK != d.B)) {
    ud_set_error("ud_splat: K [nK,3,3] is required, nK = 1 or B");
    return UD_ERR_BAD_ARG;
  }
  rc = sp_check_rest_and_fill(d, "ud_splat", a);
  if (rc != UD_OK) return rc;
  a.K = d.K; a.nK = d.nK;
  return sp_launch(a, SpProjMatrix(), stream, "ud_splat launch");
}

extern "C" int ud_splat_camera(const UdSplatCamera* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_splat_camera: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdSplatCamera& d = *desc;
  SpArgs a;
  int rc = sp_check_head(d, "ud_splat_camera", UD_RECON_MAX_B, UD_SPLAT_TRUNC | UD_SPLAT_RANGE | UD_SPLAT_FOV);
  if (rc != UD_OK) return rc;
  if (!d.params) {
    ud_set_error("ud_splat_camera: params [B,16] is required");
    return UD_ERR_BAD_ARG;
  }
  SpProjCamera proj;
  proj.params = d.params; proj.cos_limit = d.cos_limit;
  for (int b = 0; b < d.B; ++b) {
    if (!ud_cam_model_ok(d.model[b])) {
      ud_set_error("ud_splat_camera: model tag outside 1..6");
      return UD_ERR_BAD_ARG;
    }
  }
  ud_copy_models(proj.model, d.model, d.B);
  rc = sp_check_rest_and_fill(d, "ud_splat_camera", a);
  if (rc != UD_OK) return rc;
  return sp_launch(a, proj, stream, "ud_splat_camera launch");
}

extern "C" int ud_depth_minpool(const UdDepthMinPool* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_depth_minpool: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdDepthMinPool& d = *desc;
  if (d.factor < 1 || d.factor > 64) {
    ud_set_error("ud_depth_minpool: factor must be in [1, 64]");
    return UD_ERR_BAD_ARG;
  }
  if (!sp_sizes_ok(d.N, d.H, d.W) || d.H % d.factor || d.W % d.factor) {
    ud_set_error("ud_depth_minpool: bad sizes (1 <= N <= 65535, H, W >= 1 and multiples of factor, H*W < 2^31)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.src || !d.dst) {
    ud_set_error("ud_depth_minpool: null pointer (src, dst)");
    return UD_ERR_BAD_ARG;
  }
  MpArgs a;
  a.src = d.src; a.dst = d.dst; a.Ho = d.H / d.factor; a.Wo = d.W / d.factor; a.W = d.W; a.f = d.factor;
  const dim3 grid((unsigned)(((long long)a.Ho * a.Wo + SP_RTILE - 1) / SP_RTILE), (unsigned)d.N);
  hipLaunchKernelGGL(sp_minpool_kernel, grid, dim3(SP_RTILE), 0, (hipStream_t)stream, a);
  UD_CHECK_LAUNCH("ud_depth_minpool launch");
  return UD_OK;
}
