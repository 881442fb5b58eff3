// The 2-D depth metrics of a batch (eval_ops.eval_depth / DICT_METRICS; reference unidepth/utils/evaluation_depth.py eval_depth), as a
// short chain of stream-ordered gfx950 kernels instead of ~60 small torch ops and ~100 host syncs per image.
//
// Per image b (definitions in include/unidepth_hip.h, UdEvalDepth):
//   p   = bilinear resample of pred to H x W (align_corners=False, source index clamped at 0; identity when the shapes agree)
//   V   = mask && (g <= max_depth when given), n = |V|
//   r   = max(g / p, p / g) (NaN if either quotient is), d = ln p - ln g
//
// Passes (grid = (pixel chunk of 4096, image); the pixel source is re-read and p re-sampled in every pass, nothing is compacted):
//   1. stats      fp64 sums of the mean metrics and of the ssi normal equations, inlier / NaN counts, a 101-bin histogram of r over the
//                 d_auc thresholds (binary search in LDS), and the top radix digit (bits 31..24) of g, p and d
//   2. select     per (image, array): the digit that holds the lower-median rank; the next pass histograms only the values under the
//                 chosen prefix.  Three more digit passes (23..16, 15..8, 7..0) give the exact lower medians of g, p and d
//   3. params     (the last select) medians -> si factor, the 2x2 ssi solve in fp64, the mean of d
//   4. rescale    d1 / tau counts and arel sums on p'' = s p + t (ssi) and p' = p med(g) / med(p) (si); sum (d - mean d)^2 for silog
//   5. final      fixed-order reduction of the per-chunk partials, 18 metrics -> out[18][B]
//
// Reproducibility: float sums never meet an atomic.  Every thread accumulates its pixels in a fixed order in fp64, a block reduces
// its 256 threads in a fixed butterfly / wave order and stores one partial per (image, chunk); the partials are summed in chunk order
// by one thread.  Counts and histograms are integers (order-free global atomics).  Two calls on the same inputs give the same bits.
// Built with -ffp-contract=off (csrc/build.sh): the resample weights, the ratio and the rescales round every operation separately, as
// the reference's CPU torch ops do, so that threshold counts agree.
#include <math.h>
#include "ud_common.h"

namespace {

#pragma clang fp contract(off)

constexpr int ED_THREADS = 256;
constexpr int ED_PER_THREAD = 16;
constexpr int ED_CHUNK = ED_THREADS * ED_PER_THREAD;   // pixels per block
constexpr int ED_NTHR = 100;                            // d_auc thresholds
constexpr int ED_NS1 = 10;                              // fp64 sums of the stats pass
constexpr int ED_NS2 = 3;                               // fp64 sums of the rescale pass
constexpr int ED_NCNT = 8;                              // n, d1, d2, d3, tau, NaN(g), NaN(p), NaN(d)
constexpr int ED_NCNT2 = 4;                             // d1_ssi, tau_ssi, d1_si, tau_si

// stats-pass sums: 0 (g-p)^2, 1 (ln g - ln p)^2, 2 |g-p|/g, 3 (g-p)^2/g, 4 |log10 p - log10 g|, 5 d, 6 p^2, 7 p, 8 p g, 9 g
// rescale-pass sums: 0 |g-p''|/g, 1 |g-p'|/g, 2 (d - mean d)^2

struct EdArgs {
  const float* gt; const float* pred; const unsigned char* mask; const float* thr;
  float* out;
  unsigned* cnt;      // [B][ED_NCNT]          (zeroed per call)
  unsigned* hauc;     // [B][ED_NTHR + 1]      (zeroed per call)
  unsigned* rh;       // [B][3][256]           (zeroed per call; each select re-zeroes what it read)
  unsigned* cnt2;     // [B][ED_NCNT2]         (zeroed per call)
  unsigned* sel;      // [B][3][2] prefix, rank
  float* par;         // [B][8] med g, med p, med d, s, t
  double* sum1;       // [B][ED_NS1 + 1] reduced stats sums, then mean d
  double* part1;      // [B][C][ED_NS1]
  double* part2;      // [B][C][ED_NS2]
  int B, H, W, h, w, HW, C;
  float sy, sx, maxd;
  int hasmax, ident;
};

struct EdLayout {
  size_t cnt, hauc, rh, cnt2, sel, par, sum1, part1, part2, total, zero_words;
};

inline size_t ed_align(size_t x) { return (x + 255) & ~(size_t)255; }

EdLayout ed_layout(int B, int H, int W) {
  const long long HW = (long long)H * W;
  const long long C = HW > 0 ? (HW + ED_CHUNK - 1) / ED_CHUNK : 1;
  EdLayout L;
  size_t o = 0;
  // the four zeroed count regions are contiguous (one fill of zero_words words)
  L.cnt = o; o += (size_t)B * ED_NCNT * 4;
  L.hauc = o; o += (size_t)B * (ED_NTHR + 1) * 4;
  L.rh = o; o += (size_t)B * 3 * 256 * 4;
  L.cnt2 = o; o += (size_t)B * ED_NCNT2 * 4;
  L.zero_words = o / 4;
  o = ed_align(o);
  L.sel = o; o = ed_align(o + (size_t)B * 6 * 4);
  L.par = o; o = ed_align(o + (size_t)B * 8 * 4);
  L.sum1 = o; o = ed_align(o + (size_t)B * (ED_NS1 + 1) * 8);
  L.part1 = o; o = ed_align(o + (size_t)B * C * ED_NS1 * 8);
  L.part2 = o; o = ed_align(o + (size_t)B * C * ED_NS2 * 8);
  L.total = o;
  return L;
}

// order-preserving float -> uint32 key (-0 and +0 share the key of +0; NaNs sort outside +-inf, and a NaN makes the median NaN anyway)
__device__ __forceinline__ unsigned ed_key(float f) {
  if (f == 0.0f) f = 0.0f;
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ed_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// torch.maximum: NaN if either operand is NaN
__device__ __forceinline__ float ed_ratio(float g, float p) {
  const float a = g / p, b = p / g;
  if (a != a || b != b) return __builtin_nanf("");
  return a > b ? a : b;
}

// one pixel of image b: g, resampled p, and whether it is in V
__device__ __forceinline__ bool ed_load(const EdArgs& a, int b, int i, float& g, float& p) {
  const size_t gi = (size_t)b * a.HW + i;
  if (a.mask && !a.mask[gi]) return false;
  g = a.gt[gi];
  if (a.hasmax && !(g <= a.maxd)) return false;
  const float* P = a.pred + (size_t)b * a.h * a.w;
  const int oy = i / a.W, ox = i - oy * a.W;
  if (a.ident) {
    p = P[i];
    return true;
  }
  // F.interpolate(mode="bilinear", align_corners=False) on the CPU: src = scale (dst + 0.5) - 0.5 clamped at 0, index = min(floor, size-1),
  // lambda = clamp(src - index, 0, 1); out = (v00 w0x + v01 w1x) w0y + (v10 w0x + v11 w1x) w1y
  float fy = a.sy * ((float)oy + 0.5f) - 0.5f;
  fy = fy < 0.0f ? 0.0f : fy;
  float fx = a.sx * ((float)ox + 0.5f) - 0.5f;
  fx = fx < 0.0f ? 0.0f : fx;
  const int y0 = min((int)fy, a.h - 1), x0 = min((int)fx, a.w - 1);
  const float ly = fminf(fmaxf(fy - (float)y0, 0.0f), 1.0f), lx = fminf(fmaxf(fx - (float)x0, 0.0f), 1.0f);
  const float hy = 1.0f - ly, hx = 1.0f - lx;
  const int y1 = y0 + (y0 < a.h - 1 ? 1 : 0), x1 = x0 + (x0 < a.w - 1 ? 1 : 0);
  const float* r0 = P + (size_t)y0 * a.w;
  const float* r1 = P + (size_t)y1 * a.w;
  const float t0 = r0[x0] * hx + r0[x1] * lx;
  const float t1 = r1[x0] * hx + r1[x1] * lx;
  p = t0 * hy + t1 * ly;
  return true;
}

__device__ __forceinline__ double ed_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned ed_wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// fixed-order block sum of NS fp64 values -> dst[0..NS)
template <int NS>
__device__ __forceinline__ void ed_block_sum(double (&v)[NS], double* lds, double* dst) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    v[s] = ed_wave_sum_d(v[s]);
    if (lane == 0) lds[wv * NS + s] = v[s];
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int s = threadIdx.x;
    dst[s] = ((lds[s] + lds[NS + s]) + lds[2 * NS + s]) + lds[3 * NS + s];
  }
}

template <int N>
__device__ __forceinline__ void ed_flush_counts(unsigned (&c)[N], unsigned* dst) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const unsigned s = ed_wave_sum_u(c[k]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(dst + k, s);
  }
}

__global__ void ed_zero_kernel(unsigned* w, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) w[i] = 0u;
}

// pass 1: sums, counts, d_auc histogram, top radix digit of g / p / d
__global__ __launch_bounds__(ED_THREADS) void ed_stats_kernel(const EdArgs a) {
  __shared__ float thr[ED_NTHR];
  __shared__ unsigned hauc[ED_NTHR + 1];
  __shared__ unsigned rh[3 * 256];
  __shared__ double red[4 * ED_NS1];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  if (tid < ED_NTHR) thr[tid] = a.thr[tid];
  for (int j = tid; j < ED_NTHR + 1; j += ED_THREADS) hauc[j] = 0u;
  for (int j = tid; j < 3 * 256; j += ED_THREADS) rh[j] = 0u;
  __syncthreads();
  double s[ED_NS1];
#pragma unroll
  for (int k = 0; k < ED_NS1; ++k) s[k] = 0.0;
  unsigned c[ED_NCNT];
#pragma unroll
  for (int k = 0; k < ED_NCNT; ++k) c[k] = 0u;
  const int base = chunk * ED_CHUNK;
  for (int k = 0; k < ED_PER_THREAD; ++k) {
    const int i = base + k * ED_THREADS + tid;
    if (i >= a.HW) break;
    float g, p;
    if (!ed_load(a, b, i, g, p)) continue;
    const float r = ed_ratio(g, p);
    const float e = g - p;
    const float e2 = e * e;
    const float lg = logf(g), lp = logf(p);
    const float dl = lg - lp;
    const float d = lp - lg;
    const float l10 = fabsf(log10f(p) - log10f(g));
    s[0] += (double)e2;
    s[1] += (double)(dl * dl);
    s[2] += (double)(fabsf(e) / g);
    s[3] += (double)(e2 / g);
    s[4] += (double)l10;
    s[5] += (double)d;
    s[6] += (double)p * (double)p;
    s[7] += (double)p;
    s[8] += (double)p * (double)g;
    s[9] += (double)g;
    c[0] += 1u;
    c[1] += r < 1.25f ? 1u : 0u;
    c[2] += r < 1.5625f ? 1u : 0u;
    c[3] += r < 1.953125f ? 1u : 0u;
    c[4] += r < 1.03f ? 1u : 0u;
    c[5] += g != g ? 1u : 0u;
    c[6] += p != p ? 1u : 0u;
    c[7] += d != d ? 1u : 0u;
    // first threshold index j with r < thr[j] (thresholds non-decreasing); ED_NTHR when none (NaN included)
    int lo = 0, hi = ED_NTHR;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (r < thr[mid]) hi = mid;
      else lo = mid + 1;
    }
    if (r != r) lo = ED_NTHR;
    atomicAdd(&hauc[lo], 1u);
    atomicAdd(&rh[ed_key(g) >> 24], 1u);
    atomicAdd(&rh[256 + (ed_key(p) >> 24)], 1u);
    atomicAdd(&rh[512 + (ed_key(d) >> 24)], 1u);
  }
  ed_flush_counts(c, a.cnt + (size_t)b * ED_NCNT);
  ed_block_sum(s, red, a.part1 + ((size_t)b * a.C + chunk) * ED_NS1);   // contains __syncthreads: LDS histograms complete after it
  for (int j = tid; j < ED_NTHR + 1; j += ED_THREADS)
    if (hauc[j]) atomicAdd(a.hauc + (size_t)b * (ED_NTHR + 1) + j, hauc[j]);
  for (int j = tid; j < 3 * 256; j += ED_THREADS)
    if (rh[j]) atomicAdd(a.rh + (size_t)b * 768 + j, rh[j]);
}

// digit passes 2..4 (shift 16, 8, 0): histogram of the next digit of the values under each array's chosen prefix
__global__ __launch_bounds__(ED_THREADS) void ed_digit_kernel(const EdArgs a, const int shift) {
  __shared__ unsigned rh[3 * 256];
  __shared__ unsigned pre[3];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < 3 * 256; j += ED_THREADS) rh[j] = 0u;
  if (tid < 3) pre[tid] = a.sel[(size_t)b * 6 + tid * 2];
  __syncthreads();
  const unsigned pg = pre[0] >> (shift + 8), pp = pre[1] >> (shift + 8), pd = pre[2] >> (shift + 8);
  const int base = chunk * ED_CHUNK;
  for (int k = 0; k < ED_PER_THREAD; ++k) {
    const int i = base + k * ED_THREADS + tid;
    if (i >= a.HW) break;
    float g, p;
    if (!ed_load(a, b, i, g, p)) continue;
    const unsigned kg = ed_key(g), kp = ed_key(p), kd = ed_key(logf(p) - logf(g));
    if ((kg >> (shift + 8)) == pg) atomicAdd(&rh[(kg >> shift) & 255u], 1u);
    if ((kp >> (shift + 8)) == pp) atomicAdd(&rh[256 + ((kp >> shift) & 255u)], 1u);
    if ((kd >> (shift + 8)) == pd) atomicAdd(&rh[512 + ((kd >> shift) & 255u)], 1u);
  }
  __syncthreads();
  for (int j = tid; j < 3 * 256; j += ED_THREADS)
    if (rh[j]) atomicAdd(a.rh + (size_t)b * 768 + j, rh[j]);
}

// one block of 64 per image: picks the digit holding the lower-median rank for g, p, d and re-zeroes the histogram it read.  shift 24
// also reduces the stats partials (fixed chunk order); shift 0 also derives the rescale parameters.
__global__ __launch_bounds__(64) void ed_select_kernel(const EdArgs a, const int shift) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned n = a.cnt[(size_t)b * ED_NCNT];
  if (tid < 3) {
    unsigned* st = a.sel + (size_t)b * 6 + tid * 2;
    unsigned prefix = shift == 24 ? 0u : st[0];
    unsigned rank = shift == 24 ? (n > 0 ? (n - 1) / 2 : 0u) : st[1];
    unsigned* h = a.rh + (size_t)b * 768 + tid * 256;
    unsigned cum = 0, digit = 255;
    bool found = false;
    for (int j = 0; j < 256; ++j) {
      const unsigned hv = h[j];
      if (!found && rank < cum + hv) {
        digit = (unsigned)j;
        rank -= cum;
        found = true;
      }
      cum += hv;
      h[j] = 0u;
    }
    st[0] = prefix | (digit << shift);
    st[1] = rank;
  }
  if (shift == 24 && tid >= 32 && tid < 32 + ED_NS1) {
    const int k = tid - 32;
    const double* src = a.part1 + (size_t)b * a.C * ED_NS1 + k;
    double acc = 0.0;
    for (int c = 0; c < a.C; ++c) acc += src[(size_t)c * ED_NS1];
    a.sum1[(size_t)b * (ED_NS1 + 1) + k] = acc;
  }
  if (shift != 0) return;
  __syncthreads();
  if (tid != 0) return;
  const unsigned* cn = a.cnt + (size_t)b * ED_NCNT;
  const unsigned* st = a.sel + (size_t)b * 6;
  const float qnan = __builtin_nanf("");
  const float mg = (n == 0 || cn[5]) ? qnan : ed_unkey(st[0]);
  const float mp = (n == 0 || cn[6]) ? qnan : ed_unkey(st[2]);
  const float md = (n == 0 || cn[7]) ? qnan : ed_unkey(st[4]);
  double* S = a.sum1 + (size_t)b * (ED_NS1 + 1);
  const double dn = (double)n;
  // ([[sum p^2, sum p], [sum p, n]] + 1e-9 I) [s, t]^T = [sum p g, sum g]^T
  const double a11 = S[6] + 1e-9, a12 = S[7], a22 = dn + 1e-9;
  const double det = a11 * a22 - a12 * a12;
  const double sc = (a22 * S[8] - a12 * S[9]) / det;
  const double sh = (a11 * S[9] - a12 * S[8]) / det;
  float* P = a.par + (size_t)b * 8;
  P[0] = mg; P[1] = mp; P[2] = md; P[3] = (float)sc; P[4] = (float)sh;
  S[ED_NS1] = S[5] / dn;
}

// pass 5: the six rescaled metrics and the centred silog sum
__global__ __launch_bounds__(ED_THREADS) void ed_rescale_kernel(const EdArgs a) {
  __shared__ double red[4 * ED_NS2];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const float* P = a.par + (size_t)b * 8;
  const float mg = P[0], mp = P[1], sc = P[3], sh = P[4];
  const double mean_d = a.sum1[(size_t)b * (ED_NS1 + 1) + ED_NS1];
  double s[ED_NS2] = {0.0, 0.0, 0.0};
  unsigned c[ED_NCNT2] = {0u, 0u, 0u, 0u};
  const int base = chunk * ED_CHUNK;
  for (int k = 0; k < ED_PER_THREAD; ++k) {
    const int i = base + k * ED_THREADS + tid;
    if (i >= a.HW) break;
    float g, p;
    if (!ed_load(a, b, i, g, p)) continue;
    const float pssi = p * sc + sh;
    const float psi = p * mg / mp;
    const float rssi = ed_ratio(g, pssi), rsi = ed_ratio(g, psi);
    c[0] += rssi < 1.25f ? 1u : 0u;
    c[1] += rssi < 1.03f ? 1u : 0u;
    c[2] += rsi < 1.25f ? 1u : 0u;
    c[3] += rsi < 1.03f ? 1u : 0u;
    s[0] += (double)(fabsf(g - pssi) / g);
    s[1] += (double)(fabsf(g - psi) / g);
    const double dv = (double)(logf(p) - logf(g)) - mean_d;
    s[2] += dv * dv;
  }
  ed_flush_counts(c, a.cnt2 + (size_t)b * ED_NCNT2);
  ed_block_sum(s, red, a.part2 + ((size_t)b * a.C + chunk) * ED_NS2);
}

// one block of 64 per image: reduce the rescale partials in chunk order, write the 18 metrics (reference key order) to out[k][b]
__global__ __launch_bounds__(64) void ed_final_kernel(const EdArgs a) {
  __shared__ double s2[ED_NS2];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < ED_NS2) {
    const double* src = a.part2 + (size_t)b * a.C * ED_NS2 + tid;
    double acc = 0.0;
    for (int c = 0; c < a.C; ++c) acc += src[(size_t)c * ED_NS2];
    s2[tid] = acc;
  }
  __syncthreads();
  if (tid != 0) return;
  const unsigned* cn = a.cnt + (size_t)b * ED_NCNT;
  const unsigned* c2 = a.cnt2 + (size_t)b * ED_NCNT2;
  const double* S = a.sum1 + (size_t)b * (ED_NS1 + 1);
  const float* P = a.par + (size_t)b * 8;
  const unsigned n = cn[0];
  const double dn = (double)n;
  const float fn = (float)n;
  float m[18];
  if (n == 0) {
    for (int k = 0; k < 18; ++k) m[k] = __builtin_nanf("");
  } else {
    // d_auc: fraction below threshold j = (# r with first index <= j) / n; trapezoid over the exponents, / 5
    const unsigned* h = a.hauc + (size_t)b * (ED_NTHR + 1);
    unsigned cum = h[0];
    float fprev = (float)cum / fn;
    double area = 0.0;
    for (int j = 1; j < ED_NTHR; ++j) {
      cum += h[j];
      const float f = (float)cum / fn;
      area += ((double)a.thr[ED_NTHR + j] - (double)a.thr[ED_NTHR + j - 1]) * ((double)fprev + (double)f);
      fprev = f;
    }
    m[0] = (float)c2[0] / fn;                         // d1_ssi
    m[1] = (float)c2[2] / fn;                         // d1_si
    m[2] = (float)cn[1] / fn;                         // d1
    m[3] = (float)cn[2] / fn;                         // d2
    m[4] = (float)cn[3] / fn;                         // d3
    m[5] = (float)sqrt(S[0] / dn);                    // rmse
    m[6] = (float)sqrt(S[1] / dn);                    // rmselog
    m[7] = (float)(s2[0] / dn);                       // arel_ssi
    m[8] = (float)(s2[1] / dn);                       // arel_si
    m[9] = (float)(S[2] / dn);                        // arel
    m[10] = (float)(S[3] / dn);                       // sqrel
    m[11] = (float)(S[4] / dn);                       // log10
    m[12] = (float)(100.0 * sqrt(s2[2] / (dn - 1.0)));   // silog (unbiased std; n = 1 gives NaN, as torch.std)
    m[13] = 100.0f * fabsf(P[2]);                     // medianlog
    m[14] = (float)(area * 0.5 / 5.0);                // d_auc
    m[15] = (float)c2[1] / fn;                        // tau_ssi
    m[16] = (float)c2[3] / fn;                        // tau_si
    m[17] = (float)cn[4] / fn;                        // tau
  }
  for (int k = 0; k < 18; ++k) a.out[(size_t)k * a.B + b] = m[k];
}

}  // namespace

extern "C" long long ud_eval_depth_work_bytes(int B, int H, int W) {
  if (B <= 0 || H < 0 || W < 0) return -1;
  return (long long)ed_layout(B, H, W).total;
}

extern "C" int ud_eval_depth(const UdEvalDepth* desc, void* stream) {
  const UdEvalDepth& d = *desc;
  if (d.B <= 0 || d.B > 65535 || d.H < 0 || d.W < 0 || d.h < 0 || d.w < 0 || (long long)d.H * d.W > 0x7fffffffLL ||
      (long long)d.h * d.w > 0x7fffffffLL || ((long long)d.H * d.W > 0 && (d.h == 0 || d.w == 0))) {
    ud_set_error("ud_eval_depth: bad sizes (1 <= B <= 65535, H*W and h*w < 2^31, h, w > 0 when H*W > 0)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.gt || !d.pred || !d.thresholds || !d.out || !d.work) {
    ud_set_error("ud_eval_depth: null pointer");
    return UD_ERR_BAD_ARG;
  }
  const EdLayout L = ed_layout(d.B, d.H, d.W);
  if (d.work_bytes < (long long)L.total) {
    ud_set_error("ud_eval_depth: workspace smaller than ud_eval_depth_work_bytes()");
    return UD_ERR_BAD_ARG;
  }
  char* w = (char*)d.work;
  EdArgs a;
  a.gt = d.gt; a.pred = d.pred; a.mask = d.mask; a.thr = d.thresholds; a.out = d.out;
  a.cnt = (unsigned*)(w + L.cnt); a.hauc = (unsigned*)(w + L.hauc); a.rh = (unsigned*)(w + L.rh); a.cnt2 = (unsigned*)(w + L.cnt2);
  a.sel = (unsigned*)(w + L.sel); a.par = (float*)(w + L.par); a.sum1 = (double*)(w + L.sum1);
  a.part1 = (double*)(w + L.part1); a.part2 = (double*)(w + L.part2);
  a.B = d.B; a.H = d.H; a.W = d.W; a.h = d.h; a.w = d.w; a.HW = d.H * d.W;
  a.C = a.HW > 0 ? (a.HW + ED_CHUNK - 1) / ED_CHUNK : 1;
  a.sy = d.H > 0 ? (float)d.h / (float)d.H : 1.0f;
  a.sx = d.W > 0 ? (float)d.w / (float)d.W : 1.0f;
  a.maxd = d.max_depth; a.hasmax = d.has_max_depth != 0;
  a.ident = d.h == d.H && d.w == d.W;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)a.C, (unsigned)d.B);
  hipLaunchKernelGGL(ed_zero_kernel, dim3((unsigned)((L.zero_words + 255) / 256)), dim3(256), 0, s, a.cnt, L.zero_words);
  hipLaunchKernelGGL(ed_stats_kernel, grid, dim3(ED_THREADS), 0, s, a);
  hipLaunchKernelGGL(ed_select_kernel, dim3((unsigned)d.B), dim3(64), 0, s, a, 24);
  for (int shift = 16; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(ed_digit_kernel, grid, dim3(ED_THREADS), 0, s, a, shift);
    hipLaunchKernelGGL(ed_select_kernel, dim3((unsigned)d.B), dim3(64), 0, s, a, shift);
  }
  hipLaunchKernelGGL(ed_rescale_kernel, grid, dim3(ED_THREADS), 0, s, a);
  hipLaunchKernelGGL(ed_final_kernel, dim3((unsigned)d.B), dim3(64), 0, s, a);
  UD_CHECK_LAUNCH("ud_eval_depth launch");
  return UD_OK;
}
