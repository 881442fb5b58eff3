// 3-D point metrics of a batch (include/unidepth_hip.h, UdEval3d): the device form of the reference's eval_3d
// (unidepth/utils/evaluation_depth.py:160-182 with DICT_METRICS_3D :109-125, chamfer_dist :12-18, f1_score :74-91) as eight
// stream-ordered launches, no host synchronisation, no device-to-host copy.
//
//   1. e3_count_kernel    valid pixels per 4096-byte slab of the mask -> integer partials
//   2. e3_size_kernel     S = sum of the partials; the reference's resample size (h, w) in its fp32 arithmetic -> header, `size`
//   3. e3_flag_kernel     the h x w nearest-exact sample grid of the mask, 1024 samples per tile -> ballot words, tile counts
//                         (csrc/compact.h's cp_flag; steps 3-5 are its ordered compaction)
//   4. e3_scan_kernel     one workgroup per image: exclusive scan of its tile counts (cp_scan_sweep) -> tile offsets, counts[b];
//                         zeroes the image's threshold counters
//   5. e3_pack_kernel     valid samples in row-major order (cp_pack) -> gt / pred point rows (the order of gt[:, mask]);
//                         nearest-neighbour slots = +inf; fp64 partial of |gt - pred| per tile
//   6. e3_knn_kernel      d1 = gt -> pred and d2 = pred -> gt, squared L2, K = 1, each direction once, no indices: work items of
//                         512 queries x 2048 candidates meet in an integer atomicMin on the distance bits (distances are >= 0, so
//                         the unsigned order is the float order).  The per-pair arithmetic is ud_knn_points' (knn_dist.h).
//   7. e3_partial_kernel  per chunk of 1024 points: fp64 partial of (sqrt d1 + sqrt d2) / 2, and the counts d1 < th_t, d2 < th_t
//                         (strict, fp32, against the squared distance) by ballot -> integer atomicAdd
//   8. e3_final_kernel    one workgroup per image: partials summed in a fixed order, F1 from the integer counts, NaN rows for an
//                         image without a valid sample
// The sizes the host cannot know (h, w, the counts) stay on the device: every grid is sized for the bound H * W points per image
// and surplus workgroups exit on their first test.  Float sums are fp64 partials reduced in a fixed order and the only atomics are
// integer ones, so the result is bitwise reproducible.  Built with -ffp-contract=off: |gt - pred| and the distances round every
// multiply and add separately.
#include "compact.h"
#include "knn_dist.h"

namespace {

constexpr int E3_THREADS = CP_THREADS;              // every kernel of this file runs compact.h's workgroup
constexpr int E3_STEPS = CP_STEPS;
constexpr int E3_TILE = CP_TILE;                    // samples per flag / pack tile = points per metric chunk
constexpr int E3_SLAB = E3_THREADS * 16;            // mask bytes per workgroup of the count
constexpr int E3_QBLOCK = 2 * E3_THREADS;           // queries per K-NN work item (two per lane)
constexpr int E3_SPAN = 2 * KNN_TILE;               // candidates per K-NN work item
constexpr int E3_KNN_BLOCKS = 4096;                 // K-NN workgroups in flight over the whole batch, both directions
constexpr unsigned E3_INF_BITS = 0x7f800000u;

struct E3Hdr {
  long long S;
  int h, w, hw, nTe;                                // sample grid, its size and its tiles per image
};

struct E3Layout {
  size_t hdr, part, bits, tile_counts, tile_offs, thr_cnt, mse_part, ch_part, gt_xyz, pr_xyz, dmin, total;
  int nT;
  long long nP;
};

E3Layout e3_layout(int B, int H, int W, int T) {
  E3Layout L;
  const size_t HW = (size_t)H * W;
  L.nT = (int)((HW + E3_TILE - 1) / E3_TILE);
  L.nP = (long long)(((size_t)B * HW + E3_SLAB - 1) / E3_SLAB);
  const size_t tiles = (size_t)B * L.nT;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  L.hdr = 0;
  L.bits = up(sizeof(E3Hdr));
  L.mse_part = L.bits + tiles * CP_WORDS * sizeof(unsigned long long);
  L.ch_part = L.mse_part + tiles * sizeof(double);
  L.part = L.ch_part + tiles * sizeof(double);
  L.tile_counts = up(L.part + (size_t)L.nP * sizeof(int));
  L.tile_offs = L.tile_counts + tiles * sizeof(int);
  L.thr_cnt = L.tile_offs + tiles * sizeof(int);
  L.gt_xyz = up(L.thr_cnt + (size_t)B * 2 * T * sizeof(unsigned));
  L.pr_xyz = L.gt_xyz + (size_t)B * HW * 3 * sizeof(float);
  L.dmin = L.pr_xyz + (size_t)B * HW * 3 * sizeof(float);
  L.total = up(L.dmin + 2 * (size_t)B * HW * sizeof(unsigned));
  return L;
}

struct E3Args {
  const float* gt; const float* pred; const unsigned char* mask; const float* thr;
  float* out; long long* counts; int* size;
  E3Hdr* hdr; int* part; unsigned long long* bits; int* tile_counts; int* tile_offs; unsigned* thr_cnt;
  double* mse_part; double* ch_part; float* gt_xyz; float* pr_xyz; unsigned* dmin;
  long long nP, total;                              // mask slabs, mask bytes
  int B, H, W, HW, T, nT;
};

// Sum over the workgroup in a fixed order (xor tree inside a wave, waves added in index order); the same value in every thread.
template <class V>
__device__ __forceinline__ V e3_block_sum(V v, V* wave_tot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, UD_WAVE);
  __syncthreads();                                  // wave_tot may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = v;
  __syncthreads();
  V s = wave_tot[0];
#pragma unroll
  for (int k = 1; k < E3_THREADS / UD_WAVE; ++k) s += wave_tot[k];
  return s;
}

__global__ __launch_bounds__(E3_THREADS) void e3_count_kernel(E3Args a) {
  __shared__ int wave_tot[E3_THREADS / UD_WAVE];
  const long long base = (long long)blockIdx.x * E3_SLAB;
  int cnt = 0;
#pragma unroll 4
  for (int k = 0; k < E3_SLAB / E3_THREADS; ++k) {
    const long long i = base + k * E3_THREADS + threadIdx.x;
    cnt += (i < a.total && a.mask[i] != 0) ? 1 : 0;
  }
  const int tot = e3_block_sum(cnt, wave_tot);
  if (threadIdx.x == 0) a.part[blockIdx.x] = tot;
}

// The reference's size rule in its own arithmetic: ratio = min(1.0, (240 * 320 / masks.sum()) ** 0.5) is an fp32 tensor and
// int(H * ratio) truncates an fp32 product.  sqrt through fp64 and back is the correctly rounded fp32 square root (53 >= 2 * 24 + 2).
__global__ __launch_bounds__(E3_THREADS) void e3_size_kernel(E3Args a) {
  __shared__ long long wave_tot[E3_THREADS / UD_WAVE];
  long long s = 0;
  for (long long i = threadIdx.x; i < a.nP; i += E3_THREADS) s += a.part[i];
  const long long S = e3_block_sum(s, wave_tot);
  if (threadIdx.x != 0) return;
  int h = a.H, w = a.W;
  if (S > 0) {
    const float q = 76800.0f / (float)S;
    const float r = (float)sqrt((double)q);
    if (!(r >= 1.0f)) {
      h = (int)((float)a.H * r);
      w = (int)((float)a.W * r);
    }
  }
  E3Hdr hd;
  hd.S = S; hd.h = h; hd.w = w;
  hd.hw = (S > 0 && h > 0 && w > 0) ? h * w : 0;    // nothing to sample: every image is empty
  hd.nTe = (hd.hw + E3_TILE - 1) / E3_TILE;
  *a.hdr = hd;
  a.size[0] = h; a.size[1] = w;
}

// Source pixel of sample p of the h x w grid: F.interpolate(mode="nearest-exact"), min(floor((dst + 0.5) * (in / out)), in - 1) with the
// scale in fp32.
__device__ __forceinline__ int e3_source(const E3Args& a, const E3Hdr& hd, int p) {
  const int oy = p / hd.w, ox = p - oy * hd.w;
  const float sh = (float)a.H / (float)hd.h, sw = (float)a.W / (float)hd.w;
  const int sy = min((int)floorf(((float)oy + 0.5f) * sh), a.H - 1);
  const int sx = min((int)floorf(((float)ox + 0.5f) * sw), a.W - 1);
  return sy * a.W + sx;
}

__global__ __launch_bounds__(E3_THREADS) void e3_flag_kernel(E3Args a) {
  const E3Hdr hd = *a.hdr;
  const int t = blockIdx.x, b = blockIdx.y;
  if (t >= hd.nTe) return;                          // surplus tile of the H * W bound: the whole workgroup leaves
  const size_t tile = (size_t)b * a.nT + t;
  const unsigned char* mk = a.mask + (size_t)b * a.HW;
  // a sample index is < hw + E3_TILE <= 2^31 - 1 + 1024: checked on the host
  cp_flag(a.bits + tile * CP_WORDS, a.tile_counts + tile, t, hd.hw, [=](int p) { return mk[e3_source(a, hd, p)] != 0; });
}

// One workgroup per image: exclusive scan of its nTe tile counts (int sums: an image has fewer than 2^31 samples).
__global__ __launch_bounds__(E3_THREADS) void e3_scan_kernel(E3Args a) {
  const E3Hdr hd = *a.hdr;
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int t = tid; t < 2 * a.T; t += E3_THREADS) a.thr_cnt[(size_t)b * 2 * a.T + t] = 0u;
  const int total = cp_scan_sweep<int>(a.tile_counts + (size_t)b * a.nT, a.tile_offs + (size_t)b * a.nT, hd.nTe);
  if (tid == 0) a.counts[b] = total;
}

__global__ __launch_bounds__(E3_THREADS) void e3_pack_kernel(E3Args a) {
  __shared__ double wave_tot[E3_THREADS / UD_WAVE];
  const E3Hdr hd = *a.hdr;
  const int t = blockIdx.x, b = blockIdx.y;
  if (t >= hd.nTe) return;
  const size_t tile = (size_t)b * a.nT + t;
  const int base = a.tile_offs[tile];
  const float* G = a.gt + (size_t)b * 3 * a.HW;
  const float* P = a.pred + (size_t)b * 3 * a.HW;
  const size_t HW = (size_t)a.HW, BHW = (size_t)a.B * HW;
  double acc = 0.0;
  cp_pack(a.bits + tile * CP_WORDS, t, [=, &acc](int p, int row) {
    const size_t r = (size_t)b * HW + (size_t)(base + row);         // row < (b + 1) * HW
    const int src = e3_source(a, hd, p);
    const float gx = G[src], gy = G[HW + src], gz = G[2 * HW + src];
    const float px = P[src], py = P[HW + src], pz = P[2 * HW + src];
    float* og = a.gt_xyz + r * 3;
    float* op = a.pr_xyz + r * 3;
    og[0] = gx; og[1] = gy; og[2] = gz;
    op[0] = px; op[1] = py; op[2] = pz;
    a.dmin[r] = E3_INF_BITS;
    a.dmin[BHW + r] = E3_INF_BITS;
    const float dx = gx - px, dy = gy - py, dz = gz - pz;
    acc += (double)sqrtf((dx * dx + dy * dy) + dz * dz);
  });
  const double tot = e3_block_sum(acc, wave_tot);   // after the helper: every thread reaches its barriers
  if (threadIdx.x == 0) a.mse_part[tile] = tot;
}

// blockIdx.y = direction * B + image; the workgroups of one (direction, image) stride over its work items (512 queries x 2048
// candidates).  Two queries per lane, the running minimum kept without its index (knn1_d3_kernel's first pass, evalops.hip).
__global__ __launch_bounds__(E3_THREADS) void e3_knn_kernel(E3Args a) {
  __shared__ f32x4 tile[KNN_TILE];
  const int tid = threadIdx.x;
  const int b = blockIdx.y % a.B, dir = blockIdx.y / a.B;
  const int n = (int)a.counts[b];
  if (n == 0) return;
  const size_t row0 = (size_t)b * a.HW;
  const float* Q = (dir == 0 ? a.gt_xyz : a.pr_xyz) + row0 * 3;       // d1: gt -> pred, d2: pred -> gt
  const float* C = (dir == 0 ? a.pr_xyz : a.gt_xyz) + row0 * 3;
  unsigned* best = a.dmin + (size_t)dir * a.B * a.HW + row0;
  const int qb = (n + E3_QBLOCK - 1) / E3_QBLOCK, zs = (n + E3_SPAN - 1) / E3_SPAN;
  const long long items = (long long)qb * zs;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int z = (int)(it / qb), qblk = (int)(it - (long long)z * qb);
    const int q0 = qblk * E3_QBLOCK + tid, q1 = q0 + E3_THREADS;
    const bool a0 = q0 < n, a1 = q1 < n;
    float c0[3], c1[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      c0[d] = a0 ? Q[(size_t)q0 * 3 + d] : 0.0f;
      c1[d] = a1 ? Q[(size_t)q1 * 3 + d] : 0.0f;
    }
    const f32x2 qx = {c0[0], c1[0]}, qy = {c0[1], c1[1]}, qz = {c0[2], c1[2]};
    float b0 = __builtin_inff(), b1 = __builtin_inff();
    const int j_begin = z * E3_SPAN, j_end = min(n, j_begin + E3_SPAN);
    for (int base = j_begin; base < j_end; base += KNN_TILE) {
      const int cnt = min(KNN_TILE, j_end - base);
      const int cnt8 = (cnt + KNN1_CHUNK - 1) & ~(KNN1_CHUNK - 1);
      __syncthreads();
      for (int e = tid; e < cnt8; e += E3_THREADS) {
        f32x4 v = {__builtin_inff(), 0.f, 0.f, 0.f};                  // chunk padding: distance +inf, never a winner
        if (e < cnt) {
          const float* src = C + (size_t)(base + e) * 3;
          v[0] = src[0]; v[1] = src[1]; v[2] = src[2];
        }
        tile[e] = v;
      }
      __syncthreads();
      for (int c = 0; c < cnt8; c += KNN1_CHUNK) {
#pragma unroll
        for (int u = 0; u < KNN1_CHUNK; u += 2) {
          const f32x2 da = knn1_dist(qx, qy, qz, tile[c + u], true), db = knn1_dist(qx, qy, qz, tile[c + u + 1], true);
          b0 = fminf(fminf(b0, da[0]), db[0]);
          b1 = fminf(fminf(b1, da[1]), db[1]);
        }
      }
    }
    if (a0) atomicMin(best + q0, __float_as_uint(b0));
    if (a1) atomicMin(best + q1, __float_as_uint(b1));
  }
}

__global__ __launch_bounds__(E3_THREADS) void e3_partial_kernel(E3Args a) {
  extern __shared__ unsigned e3_lds[];              // T thresholds (as bits), then 2 T counters
  __shared__ double wave_tot[E3_THREADS / UD_WAVE];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int n = (int)a.counts[b];
  if ((long long)c * E3_TILE >= n) return;          // surplus chunk of the H * W bound
  float* th = (float*)e3_lds;
  unsigned* lc = e3_lds + a.T;
  for (int t = tid; t < a.T; t += E3_THREADS) th[t] = a.thr[t];
  for (int t = tid; t < 2 * a.T; t += E3_THREADS) lc[t] = 0u;
  __syncthreads();
  const size_t row0 = (size_t)b * a.HW, BHW = (size_t)a.B * a.HW;
  float d1[E3_STEPS], d2[E3_STEPS];
  bool ok[E3_STEPS];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < E3_STEPS; ++j) {
    const int i = c * E3_TILE + j * E3_THREADS + tid;
    ok[j] = i < n;
    d1[j] = ok[j] ? __uint_as_float(a.dmin[row0 + i]) : 0.0f;
    d2[j] = ok[j] ? __uint_as_float(a.dmin[BHW + row0 + i]) : 0.0f;
    if (ok[j]) acc += (double)((sqrtf(d1[j]) + sqrtf(d2[j])) / 2.0f);
  }
  for (int t = 0; t < a.T; ++t) {
    const float v = th[t];
    int c1 = 0, c2 = 0;
#pragma unroll
    for (int j = 0; j < E3_STEPS; ++j) {
      c1 += __popcll(__ballot(ok[j] && d1[j] < v));
      c2 += __popcll(__ballot(ok[j] && d2[j] < v));
    }
    if (lane == 0) {
      if (c1) atomicAdd(lc + t, (unsigned)c1);
      if (c2) atomicAdd(lc + a.T + t, (unsigned)c2);
    }
  }
  const double tot = e3_block_sum(acc, wave_tot);  // its barriers also order the LDS counters
  if (tid == 0) a.ch_part[(size_t)b * a.nT + c] = tot;
  unsigned* gc = a.thr_cnt + (size_t)b * 2 * a.T;
  for (int t = tid; t < 2 * a.T; t += E3_THREADS)
    if (lc[t]) atomicAdd(gc + t, lc[t]);
}

__global__ __launch_bounds__(E3_THREADS) void e3_final_kernel(E3Args a) {
  extern __shared__ unsigned e3_lds[];              // T values of f_t
  __shared__ double wave_tot[E3_THREADS / UD_WAVE];
  const E3Hdr hd = *a.hdr;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = (int)a.counts[b];
  if (n == 0) {
    if (tid < 3) a.out[(size_t)tid * a.B + b] = __builtin_nanf("");
    return;
  }
  double m = 0.0, ch = 0.0;
  for (int t = tid; t < hd.nTe; t += E3_THREADS) m += a.mse_part[(size_t)b * a.nT + t];
  const int chunks = (n + E3_TILE - 1) / E3_TILE;
  for (int c = tid; c < chunks; c += E3_THREADS) ch += a.ch_part[(size_t)b * a.nT + c];
  m = e3_block_sum(m, wave_tot);
  ch = e3_block_sum(ch, wave_tot);
  float* f = (float*)e3_lds;
  const unsigned* gc = a.thr_cnt + (size_t)b * 2 * a.T;
  const float fn = (float)n;
  for (int t = tid; t < a.T; t += E3_THREADS) {
    const float p = (float)gc[t] / fn, r = (float)gc[a.T + t] / fn;
    const float v = 2.0f * p * r / (p + r);
    f[t] = v != v ? 0.0f : v;
  }
  __syncthreads();
  if (tid != 0) return;
  double area = 0.0;                                // trapz(f, dx = 1)
  for (int t = 0; t + 1 < a.T; ++t) area += ((double)f[t] + (double)f[t + 1]) * 0.5;
  a.out[b] = (float)(m / (double)n);
  a.out[(size_t)a.B + b] = (float)(ch / (double)n);
  a.out[2 * (size_t)a.B + b] = (float)(area / (double)a.T);
}

bool e3_sizes_ok(int B, int H, int W, int T) {
  return B >= 1 && B <= UD_EVAL3D_MAX_B && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL - E3_TILE &&
         (long long)B * H * W < (1LL << 36) && T >= 1 && T <= UD_EVAL3D_MAX_T;
}

}  // namespace

extern "C" long long ud_eval_3d_work_bytes(int B, int H, int W, int T) {
  if (!e3_sizes_ok(B, H, W, T)) return -1;
  return (long long)e3_layout(B, H, W, T).total;
}

extern "C" int ud_eval_3d(const UdEval3d* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_eval_3d: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdEval3d& d = *desc;
  if (!e3_sizes_ok(d.B, d.H, d.W, d.T)) {
    ud_set_error("ud_eval_3d: bad sizes (1 <= B <= 32767, H, W >= 1, H*W < 2^31 - 1024, B*H*W < 2^36, 1 <= T <= 1024)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.gt || !d.pred || !d.mask || !d.thresholds || !d.out || !d.counts || !d.size || !d.work) {
    ud_set_error("ud_eval_3d: null pointer");
    return UD_ERR_BAD_ARG;
  }
  if ((uintptr_t)d.work & 15) {
    ud_set_error("ud_eval_3d: work not 16-byte aligned");
    return UD_ERR_BAD_ARG;
  }
  const E3Layout L = e3_layout(d.B, d.H, d.W, d.T);
  if (d.work_bytes < (long long)L.total) {
    ud_set_error("ud_eval_3d: workspace smaller than ud_eval_3d_work_bytes()");
    return UD_ERR_BAD_ARG;
  }
  char* w = (char*)d.work;
  E3Args a;
  a.gt = d.gt; a.pred = d.pred; a.mask = d.mask; a.thr = d.thresholds; a.out = d.out; a.counts = d.counts; a.size = d.size;
  a.hdr = (E3Hdr*)(w + L.hdr); a.part = (int*)(w + L.part); a.bits = (unsigned long long*)(w + L.bits);
  a.tile_counts = (int*)(w + L.tile_counts); a.tile_offs = (int*)(w + L.tile_offs); a.thr_cnt = (unsigned*)(w + L.thr_cnt);
  a.mse_part = (double*)(w + L.mse_part); a.ch_part = (double*)(w + L.ch_part);
  a.gt_xyz = (float*)(w + L.gt_xyz); a.pr_xyz = (float*)(w + L.pr_xyz); a.dmin = (unsigned*)(w + L.dmin);
  a.B = d.B; a.H = d.H; a.W = d.W; a.HW = d.H * d.W; a.T = d.T; a.nT = L.nT;
  a.nP = L.nP; a.total = (long long)d.B * a.HW;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(E3_THREADS), tiles((unsigned)L.nT, (unsigned)d.B);
  // K-NN workgroups per (direction, image): enough to fill the device with the batch's 2 B searches, never more than the items of
  // the largest possible cloud
  const long long max_items = (((long long)a.HW + E3_QBLOCK - 1) / E3_QBLOCK) * (((long long)a.HW + E3_SPAN - 1) / E3_SPAN);
  long long kx = (E3_KNN_BLOCKS + 2 * d.B - 1) / (2 * d.B);
  if (kx > max_items) kx = max_items;
  hipLaunchKernelGGL(e3_count_kernel, dim3((unsigned)L.nP), blk, 0, s, a);
  hipLaunchKernelGGL(e3_size_kernel, dim3(1), blk, 0, s, a);
  hipLaunchKernelGGL(e3_flag_kernel, tiles, blk, 0, s, a);
  hipLaunchKernelGGL(e3_scan_kernel, dim3((unsigned)d.B), blk, 0, s, a);
  hipLaunchKernelGGL(e3_pack_kernel, tiles, blk, 0, s, a);
  hipLaunchKernelGGL(e3_knn_kernel, dim3((unsigned)kx, (unsigned)(2 * d.B)), blk, 0, s, a);
  hipLaunchKernelGGL(e3_partial_kernel, tiles, blk, (size_t)3 * d.T * sizeof(unsigned), s, a);
  hipLaunchKernelGGL(e3_final_kernel, dim3((unsigned)d.B), blk, (size_t)d.T * sizeof(float), s, a);
  UD_CHECK_LAUNCH("ud_eval_3d launch");
  return UD_OK;
}
