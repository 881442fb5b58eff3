// Packed point clouds from dense prediction maps (include/unidepth_hip.h, UdPointCloud): an ordered stream compaction of the valid
// pixels of a batch, the device form of the reference's get_pointcloud_from_rgbd (unidepth/utils/visualization.py:57-104).
//
// A tile is PC_TILE = 1024 consecutive pixels of ONE image (256 threads x 4 pixels); thread `tid` of tile t handles the pixels
// t * 1024 + j * 256 + tid, j = 0..3, so the ballot word of wave w in step j covers the 64 consecutive pixels of word j * 4 + w.
//   1. pc_flag_kernel        predicate per pixel -> one 64-bit ballot word per wave and step (the bitmask, 16 words per tile) and the
//                            tile's popcount -> tile_counts[b][t]; tails are predicate = false, every lane reaches every ballot
//   2. pc_scan_tiles_kernel  one workgroup per image: exclusive scan of its tile counts (swept in chunks of PC_SCAN) -> tile_offs,
//                            counts[b]
//      pc_scan_images_kernel one workgroup: exclusive scan of counts -> offsets[0..B]
//   3. pc_pack_kernel        row = offsets[b] + tile_offs[b][t] + (valid pixels in the tile's earlier words) + (valid lower lanes);
//                            rows below `capacity` are written, only valid pixels read their payload
// Every dependency is a launch boundary: no atomics, no tickets, no spinning, no float reduction; the output order (images in batch
// order, pixels row-major) and every bit of it are fixed.  Built with -ffp-contract=off: (u - cx) * d / fx rounds three times.
#include "ud_common.h"

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_STEPS = 4;
constexpr int PC_TILE = PC_THREADS * PC_STEPS;
constexpr int PC_WORDS = PC_TILE / UD_WAVE;        // 16 ballot words per tile
constexpr int PC_SCAN = 256;

struct PcLayout {
  size_t bits, tile_counts, tile_offs, total;
  int nT;
};

PcLayout pc_layout(int B, int H, int W) {
  PcLayout L;
  L.nT = (int)(((long long)H * W + PC_TILE - 1) / PC_TILE);
  const size_t tiles = (size_t)B * L.nT;
  L.bits = 0;
  L.tile_counts = tiles * PC_WORDS * sizeof(unsigned long long);
  L.tile_offs = L.tile_counts + tiles * sizeof(int);
  L.total = L.tile_offs + tiles * sizeof(int);
  return L;
}

struct PcArgs {
  const float* points; const float* depth; const float* K;
  const unsigned char* image; const float* image_f32; const unsigned char* mask; const float* conf;
  float* xyz; void* rgb; int* index; long long* counts; long long* offsets;
  unsigned long long* bits; int* tile_counts; int* tile_offs;
  long long capacity;
  int B, H, W, HW, nT, nK, flags;
  float min_conf, dmin, dmax, edge_rtol;
};

__device__ __forceinline__ bool pc_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// false for a NaN on either side (every compare with a NaN is false)
__device__ __forceinline__ bool pc_edge_ok(float d, float dn, float rtol) { return fabsf(d - dn) <= rtol * fminf(d, dn); }

__device__ __forceinline__ bool pc_predicate(const PcArgs& a, int b, int p) {
  const size_t img = (size_t)b * a.HW;
  if (a.mask && a.mask[img + p] == 0) return false;
  const float* ds = a.depth ? a.depth + img : a.points + ((size_t)b * 3 + 2) * a.HW;
  const float d = ds[p];
  if (a.points) {
    const float* px = a.points + (size_t)b * 3 * a.HW + p;
    if (!pc_finite(px[0]) || !pc_finite(px[a.HW]) || !pc_finite(px[2 * (size_t)a.HW])) return false;
  } else if (!pc_finite(d)) {
    return false;
  }
  if ((a.flags & UD_PC_MINCONF) && !(a.conf[img + p] >= a.min_conf)) return false;
  if ((a.flags & UD_PC_RANGE) && !(d >= a.dmin && d <= a.dmax)) return false;
  if (a.flags & UD_PC_EDGE) {
    const int y = p / a.W, x = p - y * a.W;
    if (x > 0 && !pc_edge_ok(d, ds[p - 1], a.edge_rtol)) return false;
    if (x < a.W - 1 && !pc_edge_ok(d, ds[p + 1], a.edge_rtol)) return false;
    if (y > 0 && !pc_edge_ok(d, ds[p - a.W], a.edge_rtol)) return false;
    if (y < a.H - 1 && !pc_edge_ok(d, ds[p + a.W], a.edge_rtol)) return false;
  }
  return true;
}

__global__ __launch_bounds__(PC_THREADS) void pc_flag_kernel(PcArgs a) {
  __shared__ int wave_cnt[PC_THREADS / UD_WAVE];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned long long* words = a.bits + ((size_t)b * a.nT + t) * PC_WORDS;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < PC_STEPS; ++j) {
    const unsigned p = (unsigned)t * PC_TILE + j * PC_THREADS + tid;       // < 2^31 + PC_TILE: fits unsigned
    const bool v = p < (unsigned)a.HW && pc_predicate(a, b, (int)p);
    const unsigned long long m = __ballot(v);
    if (lane == 0) words[j * (PC_THREADS / UD_WAVE) + w] = m;
    cnt += __popcll(m);
  }
  if (lane == 0) wave_cnt[w] = cnt;
  __syncthreads();
  if (tid == 0) a.tile_counts[(size_t)b * a.nT + t] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// Exclusive scan of in[0..n) by one workgroup of PC_SCAN threads, swept in chunks of PC_SCAN with a running carry; returns the total
// (the same value in every thread).  Integer sums: the order does not matter for the bits.
template <class TI, class TO>
__device__ long long pc_scan_sweep(const TI* in, TO* out, int n) {
  __shared__ long long wave_tot[PC_SCAN / UD_WAVE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long carry = 0;
  for (int base = 0; base < n; base += PC_SCAN) {
    const int i = base + tid;
    const long long v = i < n ? (long long)in[i] : 0;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < UD_WAVE; o <<= 1) {
      const long long up = __shfl_up(inc, o, UD_WAVE);
      if (lane >= o) inc += up;
    }
    if (lane == UD_WAVE - 1) wave_tot[w] = inc;
    __syncthreads();
    long long before = 0, chunk = 0;
#pragma unroll
    for (int k = 0; k < PC_SCAN / UD_WAVE; ++k) {
      const long long tk = wave_tot[k];
      if (k < w) before += tk;
      chunk += tk;
    }
    if (i < n) out[i] = (TO)(carry + before + inc - v);
    carry += chunk;
    __syncthreads();                                  // wave_tot is rewritten by the next chunk
  }
  return carry;
}

__global__ __launch_bounds__(PC_SCAN) void pc_scan_tiles_kernel(PcArgs a) {
  const int b = blockIdx.x;
  const long long total = pc_scan_sweep(a.tile_counts + (size_t)b * a.nT, a.tile_offs + (size_t)b * a.nT, a.nT);
  if (threadIdx.x == 0) a.counts[b] = total;
}

__global__ __launch_bounds__(PC_SCAN) void pc_scan_images_kernel(PcArgs a) {
  const long long total = pc_scan_sweep(a.counts, a.offsets, a.B);
  if (threadIdx.x == 0) a.offsets[a.B] = total;
}

__global__ __launch_bounds__(PC_THREADS) void pc_pack_kernel(PcArgs a) {
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long base = a.offsets[b] + a.tile_offs[(size_t)b * a.nT + t];
  // lanes 0..15 of every wave hold the tile's 16 words and the count of valid pixels in the words before each
  const unsigned long long my_word = lane < PC_WORDS ? a.bits[((size_t)b * a.nT + t) * PC_WORDS + lane] : 0ull;
  const int my_cnt = __popcll(my_word);
  int inc = my_cnt;
#pragma unroll
  for (int o = 1; o < PC_WORDS; o <<= 1) {
    const int up = __shfl_up(inc, o, UD_WAVE);
    if (lane >= o) inc += up;
  }
  const int my_before = inc - my_cnt;
  const size_t img = (size_t)b * a.HW;
  float fx = 1.0f, fy = 1.0f, cx = 0.0f, cy = 0.0f;
  if (!a.points) {
    const float* K = a.K + (a.nK == 1 ? 0 : (size_t)b * 9);
    fx = K[0]; cx = K[2]; fy = K[4]; cy = K[5];
  }
#pragma unroll
  for (int j = 0; j < PC_STEPS; ++j) {
    const int k = j * (PC_THREADS / UD_WAVE) + w;
    const unsigned long long m = __shfl(my_word, k, UD_WAVE);
    const int before = __shfl(my_before, k, UD_WAVE);
    if (!((m >> lane) & 1ull)) continue;
    const long long r = base + before + __popcll(m & ((1ull << lane) - 1ull));
    if (r >= a.capacity) continue;
    const int p = t * PC_TILE + k * UD_WAVE + lane;    // a set bit: p < HW
    float X, Y, Z;
    if (a.points) {
      const float* px = a.points + (size_t)b * 3 * a.HW + p;
      X = px[0]; Y = px[a.HW]; Z = px[2 * (size_t)a.HW];
    } else {
      const int v = p / a.W, u = p - v * a.W;
      const float d = a.depth[img + p];
      X = ((float)u - cx) * d / fx;
      Y = ((float)v - cy) * d / fy;
      Z = d;
    }
    if (a.flags & UD_PC_FLIP_Y) Y = -Y;
    float* o = a.xyz + r * 3;
    o[0] = X; o[1] = Y; o[2] = Z;
    if (a.image) {
      const unsigned char* c = a.image + (size_t)b * 3 * a.HW + p;
      unsigned char* oc = (unsigned char*)a.rgb + r * 3;
      oc[0] = c[0]; oc[1] = c[a.HW]; oc[2] = c[2 * (size_t)a.HW];
    } else if (a.image_f32) {
      const float* c = a.image_f32 + (size_t)b * 3 * a.HW + p;
      float* oc = (float*)a.rgb + r * 3;
      oc[0] = c[0]; oc[1] = c[a.HW]; oc[2] = c[2 * (size_t)a.HW];
    }
    if (a.index) a.index[r] = p;
  }
}

}  // namespace

extern "C" long long ud_pointcloud_work_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return -1;
  return (long long)pc_layout(B, H, W).total;
}

extern "C" int ud_pointcloud_pack(const UdPointCloud* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_pointcloud_pack: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdPointCloud& d = *desc;
  if (d.B <= 0 || d.B > 65535 || d.H <= 0 || d.W <= 0 || (long long)d.H * d.W > 0x7fffffffLL || d.capacity < 0) {
    ud_set_error("ud_pointcloud_pack: bad sizes (1 <= B <= 65535, H, W >= 1, H*W < 2^31, capacity >= 0)");
    return UD_ERR_BAD_ARG;
  }
  if (d.index && (long long)d.B * d.H * d.W > 0x7fffffffLL) {
    ud_set_error("ud_pointcloud_pack: B*H*W must stay below 2^31 when index is requested");
    return UD_ERR_BAD_ARG;
  }
  if (!d.points && !d.depth) {
    ud_set_error("ud_pointcloud_pack: neither points nor depth given");
    return UD_ERR_BAD_ARG;
  }
  if (!d.points && (!d.K || (d.nK != 1 && d.nK != d.B))) {
    ud_set_error("ud_pointcloud_pack: depth mode needs K [nK,3,3] with nK = 1 or B");
    return UD_ERR_BAD_ARG;
  }
  if (d.K && d.nK != 1 && d.nK != d.B) {
    ud_set_error("ud_pointcloud_pack: nK must be 1 or B");
    return UD_ERR_BAD_ARG;
  }
  if ((d.flags & ~(UD_PC_MINCONF | UD_PC_RANGE | UD_PC_EDGE | UD_PC_FLIP_Y)) || ((d.flags & UD_PC_MINCONF) && !d.confidence)) {
    ud_set_error("ud_pointcloud_pack: unknown flag, or UD_PC_MINCONF without a confidence map");
    return UD_ERR_BAD_ARG;
  }
  if (!d.counts || !d.offsets || !d.work || ((uintptr_t)d.work & 7)) {
    ud_set_error("ud_pointcloud_pack: null pointer (counts, offsets, work), or work not 8-byte aligned");
    return UD_ERR_BAD_ARG;
  }
  if (d.xyz && ((d.image && d.image_f32) || ((d.image || d.image_f32) && !d.rgb))) {
    ud_set_error("ud_pointcloud_pack: one colour input at most (image or image_f32), and rgb to receive it");
    return UD_ERR_BAD_ARG;
  }
  const PcLayout L = pc_layout(d.B, d.H, d.W);
  if (d.work_bytes < (long long)L.total) {
    ud_set_error("ud_pointcloud_pack: workspace smaller than ud_pointcloud_work_bytes()");
    return UD_ERR_BAD_ARG;
  }
  char* w = (char*)d.work;
  PcArgs a;
  a.points = d.points; a.depth = d.depth; a.K = d.K; a.image = d.image; a.image_f32 = d.image_f32; a.mask = d.mask; a.conf = d.confidence;
  a.xyz = d.xyz; a.rgb = d.rgb; a.index = d.index; a.counts = d.counts; a.offsets = d.offsets;
  a.bits = (unsigned long long*)(w + L.bits); a.tile_counts = (int*)(w + L.tile_counts); a.tile_offs = (int*)(w + L.tile_offs);
  a.capacity = d.capacity;
  a.B = d.B; a.H = d.H; a.W = d.W; a.HW = d.H * d.W; a.nT = L.nT; a.nK = d.nK; a.flags = d.flags;
  a.min_conf = d.min_conf; a.dmin = d.dmin; a.dmax = d.dmax; a.edge_rtol = d.edge_rtol;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)L.nT, (unsigned)d.B);
  hipLaunchKernelGGL(pc_flag_kernel, grid, dim3(PC_THREADS), 0, s, a);
  hipLaunchKernelGGL(pc_scan_tiles_kernel, dim3((unsigned)d.B), dim3(PC_SCAN), 0, s, a);
  hipLaunchKernelGGL(pc_scan_images_kernel, dim3(1), dim3(PC_SCAN), 0, s, a);
  if (d.xyz && d.capacity > 0) hipLaunchKernelGGL(pc_pack_kernel, grid, dim3(PC_THREADS), 0, s, a);
  UD_CHECK_LAUNCH("ud_pointcloud_pack launch");
  return UD_OK;
}
