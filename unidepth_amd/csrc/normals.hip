// Surface normals from a point map or from a depth map through a camera (include/unidepth_hip.h, UdNormals), and the normal-error metrics
// of a batch (UdEvalNormals).  The arithmetic of a pixel is csrc/normals_point.h, which the host build of the tests runs under the
// sanitizers; the definition is written out there.
//
//   nm_points_kernel  one thread per pixel of a 32 x 8 tile, blockIdx.z = image: the pixel's point and its four neighbours are loaded from
//                     the planar point map (the neighbours of a tile hit the cache lines its own rows brought in), no LDS.
//   nm_depth_kernel   the fused depth form, the same tile: the 34 x 10 points of the tile and its one-pixel halo are reconstructed ONCE
//                     (camera_models.h's reconstruct at the pixel centres, 1.33 points per pixel instead of 5) into LDS with their depth
//                     and ok flag, one barrier, then every thread takes its five points from LDS.  The camera model is uniform per
//                     workgroup; the point map never reaches memory.  Closed-form models only: the radial loop of OPENCV / Fisheye624
//                     ends on a maximum over the whole image, the caller unprojects those with ud_camera_unproject and passes points.
//   en_*              the metrics, evaldepth.hip's scheme: a stats pass (fp64 sums of acosf(c) and its square, threshold counts, the top
//                     radix digit of c's key, the optional error map), three digit passes with a select after each, and the last select
//                     writes the rows.  Float sums never meet an atomic: thread, wave, block and chunk order are fixed.
//
// No kernel synchronises with the host; both calls capture into a graph.  Built with -ffp-contract=off: every operation rounds separately,
// so a numpy fp32 restatement reproduces every bit of the normals and every count of the metrics.
#include <math.h>
#include "ud_common.h"
#include "normals_point.h"
#pragma clang fp contract(off)

namespace {

constexpr int NM_TW = 32, NM_TH = 8, NM_THREADS = NM_TW * NM_TH;
constexpr int NM_HW = NM_TW + 2, NM_HH = NM_TH + 2, NM_HALO = NM_HW * NM_HH;

struct NmKernelArgs {
  UdNmArgs p;
  const float* params;
  unsigned char model[UD_RECON_MAX_B];
};

__global__ __launch_bounds__(NM_THREADS) void nm_points_kernel(const NmKernelArgs a) {
  const int x = blockIdx.x * NM_TW + (threadIdx.x & (NM_TW - 1)), y = blockIdx.y * NM_TH + (threadIdx.x / NM_TW);
  if (x >= a.p.W || y >= a.p.H) return;
  ud_nm_pixel(a.p, blockIdx.z, y, x);
}

#ifdef UD_NM_RECOMPUTE
// The alternative the LDS form was measured against (tools/bench_normals.py --alt-lib, profiles/normals_bench.txt): no LDS, every thread
// reconstructs its own point and its four neighbours.  Same functions, same bits.  Not part of the product build.
__global__ __launch_bounds__(NM_THREADS) void nm_depth_kernel(const NmKernelArgs a) {
  const int b = blockIdx.z, W = a.p.W, H = a.p.H;
  const int x = blockIdx.x * NM_TW + (threadIdx.x & (NM_TW - 1)), y = blockIdx.y * NM_TH + (threadIdx.x / NM_TW);
  if (x >= W || y >= H) return;
  const size_t hw = (size_t)H * (size_t)W;
  const int model = a.model[b];
  const float* params = a.params + (size_t)b * 16;
  const float* depth_b = a.p.depth + (size_t)b * hw;
  const unsigned char* mask_b = a.p.mask ? a.p.mask + (size_t)b * (size_t)a.p.mask_bs : nullptr;
  const int qy[5] = {y, y, y, y - 1, y + 1}, qx[5] = {x, x - 1, x + 1, x, x};
  float p[5][3], d[5], n[3];
  bool ok[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    p[k][0] = p[k][1] = p[k][2] = d[k] = 0.0f;
    ok[k] = false;
    if (qx[k] >= 0 && qx[k] < W && qy[k] >= 0 && qy[k] < H) ok[k] = ud_nm_depth_point(model, params, mask_b, depth_b, W, qy[k], qx[k], p[k], &d[k]);
    if (k > 0 && a.p.has_rtol) ok[k] = ok[k] && ud_nm_edge_ok(d[0], d[k], a.p.rtol);
  }
  const bool valid = ud_nm_normal(p[0], p[1], p[2], p[3], p[4], ok[0], ok[1], ok[2], ok[3], ok[4], n);
  ud_nm_store(a.p, b, (size_t)y * (size_t)W + (size_t)x, valid, n);
}
#else
__global__ __launch_bounds__(NM_THREADS) void nm_depth_kernel(const NmKernelArgs a) {
  __shared__ float sp[3][NM_HALO];
  __shared__ float sd[NM_HALO];
  __shared__ unsigned char sok[NM_HALO];
  const int b = blockIdx.z, W = a.p.W, H = a.p.H;
  const int x0 = blockIdx.x * NM_TW, y0 = blockIdx.y * NM_TH;
  const size_t hw = (size_t)H * (size_t)W;
  const int model = a.model[b];
  const float* params = a.params + (size_t)b * 16;
  const float* depth_b = a.p.depth + (size_t)b * hw;
  const unsigned char* mask_b = a.p.mask ? a.p.mask + (size_t)b * (size_t)a.p.mask_bs : nullptr;
  for (int j = threadIdx.x; j < NM_HALO; j += NM_THREADS) {
    const int hy = j / NM_HW, hx = j - hy * NM_HW;
    const int gy = y0 + hy - 1, gx = x0 + hx - 1;
    float p[3] = {0.0f, 0.0f, 0.0f}, d = 0.0f;
    bool ok = false;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) ok = ud_nm_depth_point(model, params, mask_b, depth_b, W, gy, gx, p, &d);
    sp[0][j] = p[0]; sp[1][j] = p[1]; sp[2][j] = p[2];
    sd[j] = d;
    sok[j] = ok ? 1 : 0;
  }
  __syncthreads();
  const int tx = threadIdx.x & (NM_TW - 1), ty = threadIdx.x / NM_TW;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  const int jc = (ty + 1) * NM_HW + tx + 1;
  const int jq[4] = {jc - 1, jc + 1, jc - NM_HW, jc + NM_HW};          // left, right, up, down: all inside the halo
  float c[3] = {sp[0][jc], sp[1][jc], sp[2][jc]}, q[4][3], n[3];
  bool use[4];
  const float dc = sd[jc];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    q[k][0] = sp[0][jq[k]]; q[k][1] = sp[1][jq[k]]; q[k][2] = sp[2][jq[k]];
    use[k] = sok[jq[k]] != 0;                                           // 0 outside the image
    if (a.p.has_rtol) use[k] = use[k] && ud_nm_edge_ok(dc, sd[jq[k]], a.p.rtol);
  }
  const bool valid = ud_nm_normal(c, q[0], q[1], q[2], q[3], sok[jc] != 0, use[0], use[1], use[2], use[3], n);
  ud_nm_store(a.p, b, (size_t)y * (size_t)W + (size_t)x, valid, n);
}
#endif

// ---- the metrics ------------------------------------------------------------------------------------------------------------------------

constexpr int EN_THREADS = 256, EN_PER_THREAD = 16, EN_CHUNK = EN_THREADS * EN_PER_THREAD;
constexpr int EN_MAX_T = UD_EVAL_NORMALS_MAX_T;
constexpr int EN_NCNT = 1 + EN_MAX_T;                  // n, then one count per threshold
constexpr double EN_DEG = 180.0 / 3.14159265358979323846;

struct EnArgs {
  const float* gt; const float* pred; const unsigned char* mask;
  float* out; long long* count; float* err;
  unsigned* cnt;        // [B][EN_NCNT]   (zeroed per call)
  unsigned* rh;         // [B][256]       (zeroed per call; each select re-zeroes what it read)
  unsigned* sel;        // [B][2] prefix, rank
  double* part;         // [B][C][2]
  long long mask_bs;
  float cos_t[EN_MAX_T];
  int B, HW, C, T;
};

struct EnLayout {
  size_t cnt, rh, sel, part, total, zero_words;
};

inline size_t en_align(size_t x) { return (x + 255) & ~(size_t)255; }

EnLayout en_layout(int B, long long HW) {
  const long long C = (HW + EN_CHUNK - 1) / EN_CHUNK;
  EnLayout L;
  size_t o = 0;
  L.cnt = o; o += (size_t)B * EN_NCNT * 4;
  L.rh = o; o += (size_t)B * 256 * 4;
  L.zero_words = o / 4;
  o = en_align(o);
  L.sel = o; o = en_align(o + (size_t)B * 2 * 4);
  L.part = o; o = en_align(o + (size_t)B * (size_t)C * 2 * 8);
  L.total = o;
  return L;
}

bool en_sizes_ok(int B, int H, int W, int T) {
  return B >= 1 && B <= UD_RECON_MAX_B && H >= 1 && W >= 1 && (long long)H * W < 0x7fffffffLL - EN_CHUNK && T >= 1 && T <= EN_MAX_T;
}

// order-preserving float -> uint32 key; -0 and +0 share the key of +0 (acosf gives them the same error)
__device__ __forceinline__ unsigned en_key(float f) {
  if (f == 0.0f) f = 0.0f;
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float en_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the cosine of pixel i of image b; false where the pixel is dropped
__device__ __forceinline__ bool en_load(const EnArgs& a, int b, int i, float& c) {
  if (a.mask && !a.mask[(size_t)b * (size_t)a.mask_bs + i]) return false;
  const size_t hw = (size_t)a.HW;
  const float* g = a.gt + (size_t)b * 3 * hw + i;
  const float* p = a.pred + (size_t)b * 3 * hw + i;
  return ud_nm_cos(g[0], g[hw], g[2 * hw], p[0], p[hw], p[2 * hw], &c);
}

__device__ __forceinline__ double en_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned en_wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one more value in `digit` of the LDS histogram.  The cosines of a good prediction share their leading digits, so a thread counts a run
// of equal digits in a register and adds it once: integer counts, the same histogram in fewer atomics on one address.
__device__ __forceinline__ void en_count(unsigned* rh, unsigned digit, unsigned& bin, unsigned& run) {
  if (digit != bin && run) {
    atomicAdd(&rh[bin], run);
    run = 0u;
  }
  bin = digit;
  ++run;
}

__global__ void en_zero_kernel(unsigned* w, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) w[i] = 0u;
}

// pass 1: sums, counts, the error map, the top radix digit of c
__global__ __launch_bounds__(EN_THREADS) void en_stats_kernel(const EnArgs a) {
  __shared__ unsigned rh[256];
  __shared__ double red[4 * 2];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  rh[tid] = 0u;
  __syncthreads();
  double s0 = 0.0, s1 = 0.0;
  unsigned c[EN_NCNT], bin = 0u, run = 0u;
#pragma unroll
  for (int k = 0; k < EN_NCNT; ++k) c[k] = 0u;
  const int base = chunk * EN_CHUNK;                    // < HW + EN_CHUNK <= 2^31 - 1: checked on the host
  for (int k = 0; k < EN_PER_THREAD; ++k) {
    const int i = base + k * EN_THREADS + tid;
    if (i >= a.HW) break;
    float v;
    const bool ok = en_load(a, b, i, v);
    const float e = ok ? acosf(v) : 0.0f;
    if (a.err) a.err[(size_t)b * (size_t)a.HW + i] = ok ? (float)((double)e * EN_DEG) : __builtin_nanf("");
    if (!ok) continue;
    s0 += (double)e;
    s1 += (double)e * (double)e;
    c[0] += 1u;
#pragma unroll
    for (int t = 0; t < EN_MAX_T; ++t) c[1 + t] += (t < a.T && v > a.cos_t[t]) ? 1u : 0u;
    en_count(rh, en_key(v) >> 24, bin, run);
  }
  if (run) atomicAdd(&rh[bin], run);
#pragma unroll
  for (int k = 0; k < EN_NCNT; ++k) {
    const unsigned s = en_wave_sum_u(c[k]);
    if ((tid & 63) == 0 && s) atomicAdd(a.cnt + (size_t)b * EN_NCNT + k, s);
  }
  s0 = en_wave_sum_d(s0);
  s1 = en_wave_sum_d(s1);
  if ((tid & 63) == 0) {
    red[(tid >> 6) * 2] = s0; red[(tid >> 6) * 2 + 1] = s1;
  }
  __syncthreads();                                      // the LDS histogram is complete after it as well
  if (tid < 2) a.part[((size_t)b * a.C + chunk) * 2 + tid] = ((red[tid] + red[2 + tid]) + red[4 + tid]) + red[6 + tid];
  if (rh[tid]) atomicAdd(a.rh + (size_t)b * 256 + tid, rh[tid]);
}

// digit passes (shift 16, 8, 0): histogram of the next digit of the cosines under the chosen prefix
__global__ __launch_bounds__(EN_THREADS) void en_digit_kernel(const EnArgs a, const int shift) {
  __shared__ unsigned rh[256];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  rh[tid] = 0u;
  __syncthreads();
  const unsigned pre = a.sel[(size_t)b * 2] >> (shift + 8);
  unsigned bin = 0u, run = 0u;
  const int base = chunk * EN_CHUNK;
  for (int k = 0; k < EN_PER_THREAD; ++k) {
    const int i = base + k * EN_THREADS + tid;
    if (i >= a.HW) break;
    float v;
    if (!en_load(a, b, i, v)) continue;
    const unsigned key = en_key(v);
    if ((key >> (shift + 8)) == pre) en_count(rh, (key >> shift) & 255u, bin, run);
  }
  if (run) atomicAdd(&rh[bin], run);
  __syncthreads();
  if (rh[tid]) atomicAdd(a.rh + (size_t)b * 256 + tid, rh[tid]);
}

// one wave per image: the digit that holds the rank floor((n - 1) / 2) counted from the LARGEST cosine (acos is decreasing: the lower
// median of the error); re-zeroes the histogram it read.  Lane l owns the digits 255 - 4 l .. 252 - 4 l, in that order; a wave scan of the
// lanes' sums finds the lane, the lane finds the digit.  shift 0 also reduces the partial sums in chunk order and writes the rows.
__global__ __launch_bounds__(64) void en_select_kernel(const EnArgs a, const int shift) {
  __shared__ unsigned res[2];
  const int b = blockIdx.x, lane = threadIdx.x;
  const unsigned n = a.cnt[(size_t)b * EN_NCNT];
  unsigned* st = a.sel + (size_t)b * 2;
  const unsigned prefix = shift == 24 ? 0u : st[0];
  const unsigned rank0 = shift == 24 ? (n > 0 ? (n - 1) / 2 : 0u) : st[1];
  unsigned* h = a.rh + (size_t)b * 256;
  unsigned v[4], sum = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = 255 - 4 * lane - k;
    v[k] = h[j];
    h[j] = 0u;
    sum += v[k];
  }
  unsigned incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 0) {
    res[0] = 0u; res[1] = rank0;                      // an image without a usable pixel: digit 0, nothing found
  }
  __syncthreads();
  unsigned cum = incl - sum;
  if (rank0 >= cum && rank0 < incl) {                 // at most one lane
    bool found = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!found && rank0 < cum + v[k]) {
        res[0] = (unsigned)(255 - 4 * lane - k);
        res[1] = rank0 - cum;
        found = true;
      }
      cum += v[k];
    }
  }
  __syncthreads();
  if (lane != 0) return;
  const unsigned digit = res[0], rank = res[1];
  const unsigned key = prefix | (digit << shift);
  st[0] = key;
  st[1] = rank;
  if (shift != 0) return;
  a.count[b] = (long long)n;
  float* out = a.out + b;
  if (n == 0) {
    for (int k = 0; k < 3 + a.T; ++k) out[(size_t)k * a.B] = __builtin_nanf("");
    return;
  }
  const double* src = a.part + (size_t)b * a.C * 2;
  double S0 = 0.0, S1 = 0.0;
  for (int c = 0; c < a.C; ++c) {
    S0 += src[(size_t)c * 2]; S1 += src[(size_t)c * 2 + 1];
  }
  const double dn = (double)n;
  const float fn = (float)n;
  out[0] = (float)(S0 / dn * EN_DEG);
  out[(size_t)a.B] = (float)((double)acosf(en_unkey(key)) * EN_DEG);
  out[(size_t)2 * a.B] = (float)(sqrt(S1 / dn) * EN_DEG);
  for (int t = 0; t < a.T; ++t) out[(size_t)(3 + t) * a.B] = (float)a.cnt[(size_t)b * EN_NCNT + 1 + t] / fn;
}

}  // namespace

extern "C" int ud_normals(const UdNormals* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_normals: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdNormals& d = *desc;
  if (d.B < 1 || d.B > UD_RECON_MAX_B || d.H < 1 || d.W < 1 || (long long)d.H * d.W >= UD_MAX_ELEMS) {
    ud_set_error("ud_normals: bad sizes (1 <= B <= 256, H, W >= 1, H * W < 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.normals || (!d.points && (!d.depth || !d.params))) {
    ud_set_error("ud_normals: null pointer (normals; points, or depth with params)");
    return UD_ERR_BAD_ARG;
  }
  const float rtol = ud_f32_from_bits(d.rtol_bits);
  if (d.has_rtol && !ud_tolerance_ok(rtol)) {
    ud_set_error("ud_normals: edge_rtol must be finite and not negative");
    return UD_ERR_BAD_ARG;
  }
  NmKernelArgs a;
  if (!d.points) {
    for (int b = 0; b < d.B; ++b) {
      const int m = d.model[b];
      if (!ud_cam_model_ok(m)) {
        ud_set_error("ud_normals: model tag outside 1..6");
        return UD_ERR_BAD_ARG;
      }
      if (!ud_cam_closed_form(m)) {
        ud_set_error("ud_normals: iterative model (OPENCV / Fisheye624) with depth: unproject with ud_camera_unproject and pass points");
        return UD_ERR_UNSUPPORTED;
      }
    }
  }
  ud_copy_models(a.model, d.model, d.points ? 0 : d.B);
  a.p.points = d.points; a.p.depth = d.depth; a.p.mask = d.mask;
  a.p.normals = d.normals; a.p.valid = d.valid; a.p.rgb = d.rgb;
  a.p.mask_bs = d.mask_shared ? 0 : (long long)d.H * d.W;
  a.p.rtol = d.has_rtol ? rtol : 0.0f;
  a.p.H = d.H; a.p.W = d.W; a.p.has_rtol = d.has_rtol ? 1 : 0;
  a.params = d.params;
  const dim3 grid((unsigned)((d.W + NM_TW - 1) / NM_TW), (unsigned)((d.H + NM_TH - 1) / NM_TH), (unsigned)d.B);
  if (grid.y > 65535u) {
    ud_set_error("ud_normals: bad sizes (H <= 524280)");
    return UD_ERR_BAD_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  if (d.points) hipLaunchKernelGGL(nm_points_kernel, grid, dim3(NM_THREADS), 0, s, a);
  else hipLaunchKernelGGL(nm_depth_kernel, grid, dim3(NM_THREADS), 0, s, a);
  UD_CHECK_LAUNCH("ud_normals launch");
  return UD_OK;
}

extern "C" long long ud_eval_normals_work_bytes(int B, int H, int W, int T) {
  if (!en_sizes_ok(B, H, W, T)) return -1;
  return (long long)en_layout(B, (long long)H * W).total;
}

extern "C" int ud_eval_normals(const UdEvalNormals* desc, void* workspace, long long bytes, void* stream) {
  if (!desc) {
    ud_set_error("ud_eval_normals: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdEvalNormals& d = *desc;
  if (!en_sizes_ok(d.B, d.H, d.W, d.T)) {
    ud_set_error("ud_eval_normals: bad sizes (1 <= B <= 256, H, W >= 1, H * W < 2^31 - 4096, 1 <= T <= 8)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.gt || !d.pred || !d.out || !d.count || !workspace) {
    ud_set_error("ud_eval_normals: null pointer");
    return UD_ERR_BAD_ARG;
  }
  if ((uintptr_t)workspace & 15) {
    ud_set_error("ud_eval_normals: workspace not 16-byte aligned");
    return UD_ERR_BAD_ARG;
  }
  const long long HW = (long long)d.H * d.W;
  const EnLayout L = en_layout(d.B, HW);
  if (bytes < (long long)L.total) {
    ud_set_error("ud_eval_normals: workspace smaller than ud_eval_normals_work_bytes()");
    return UD_ERR_BAD_ARG;
  }
  char* w = (char*)workspace;
  EnArgs a;
  a.gt = d.gt; a.pred = d.pred; a.mask = d.mask; a.out = d.out; a.count = d.count; a.err = d.error;
  a.cnt = (unsigned*)(w + L.cnt); a.rh = (unsigned*)(w + L.rh); a.sel = (unsigned*)(w + L.sel); a.part = (double*)(w + L.part);
  a.mask_bs = d.mask_shared ? 0 : HW;
  for (int t = 0; t < EN_MAX_T; ++t) a.cos_t[t] = t < d.T ? ud_f32_from_bits(d.cos_bits[t]) : 2.0f;
  a.B = d.B; a.HW = (int)HW; a.C = (int)((HW + EN_CHUNK - 1) / EN_CHUNK); a.T = d.T;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)a.C, (unsigned)d.B);
  hipLaunchKernelGGL(en_zero_kernel, dim3((unsigned)((L.zero_words + 255) / 256)), dim3(256), 0, s, a.cnt, L.zero_words);
  hipLaunchKernelGGL(en_stats_kernel, grid, dim3(EN_THREADS), 0, s, a);
  hipLaunchKernelGGL(en_select_kernel, dim3((unsigned)d.B), dim3(64), 0, s, a, 24);
  for (int shift = 16; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(en_digit_kernel, grid, dim3(EN_THREADS), 0, s, a, shift);
    hipLaunchKernelGGL(en_select_kernel, dim3((unsigned)d.B), dim3(64), 0, s, a, shift);
  }
  UD_CHECK_LAUNCH("ud_eval_normals launch");
  return UD_OK;
}
