// The ordered stream compaction that pointcloud.hip (pixels), tsdf.hip (slots), tsdf_mesh.hip (cells, slots) and eval3d.hip (samples) share: a mask of items becomes a
// packed list in item order, every bit fixed.  Device and host inline code; each file keeps its predicate, its row writer, its thin
// __global__ wrappers and its entry point.
//
// The index map.  A tile is CP_TILE = 1024 consecutive items of ONE batch member, handled by CP_THREADS = 256 threads in CP_STEPS = 4
// steps: thread `tid` handles the items t * 1024 + j * 256 + tid, j = 0..3, so the ballot word of wave w in step j is word k = j * 4 + w
// of the tile's CP_WORDS = 16 and its bit `lane` is item t * 1024 + k * 64 + lane.
//   cp_flag        predicate per item -> the tile's 16 words and its popcount; items at or beyond n are predicate = false
//   cp_scan_sweep  exclusive scan by one workgroup of CP_SCAN threads, swept in chunks of CP_SCAN with a carry
//   cp_pack        emit(item, row inside the tile) for every set bit: row = popcount of the earlier words + of the lower lanes
//   cp_test / cp_rank   for a second packer that reads the finished mask of a first (tsdf_mesh.hip): the bit of an item, and the item's row
//                  inside its member from tile_offs and popcounts.  Plain per-lane reads, no barrier: callable from a predicate or an emit
// The contract.  Every thread of the workgroup calls the helper, from uniform control flow: cp_flag holds a ballot per step and a
// barrier, cp_scan_sweep two barriers per chunk, cp_pack wave-wide shuffles.  A caller may return BEFORE the call when the whole
// workgroup does (eval3d.hip's surplus tiles), never a single lane; the predicate and emit run divergently and must hold no barrier.
// Every dependency between the three steps is a launch boundary: no atomics, no tickets, no spinning.  Integer arithmetic only, so the
// -ffp-contract rule of the including file is unaffected.  The callers' lambdas capture the kernel's arguments by value ([=]): with [&]
// the compiler computes the uniform addresses again in each of the four steps (profiles/compact_refactor.txt).
#pragma once
#include "ud_common.h"

constexpr int CP_THREADS = 256;
constexpr int CP_STEPS = 4;
constexpr int CP_TILE = CP_THREADS * CP_STEPS;
constexpr int CP_WORDS = CP_TILE / UD_WAVE;        // 16 ballot words per tile
constexpr int CP_SCAN = 256;

// ---- host: the work area of B members of `items` items each, and what the kernels of a packer read from it
struct CpLayout {
  size_t bits, tile_counts, tile_offs, total;
  int nT;
};

static inline CpLayout cp_layout(int B, long long items) {
  CpLayout L;
  L.nT = (int)((items + CP_TILE - 1) / CP_TILE);
  const size_t tiles = (size_t)B * L.nT;
  L.bits = 0;
  L.tile_counts = tiles * CP_WORDS * sizeof(unsigned long long);
  L.tile_offs = L.tile_counts + tiles * sizeof(int);
  L.total = L.tile_offs + tiles * sizeof(int);
  return L;
}

struct CpArgs {
  long long* counts; long long* offsets;             // [B] items kept per member, [B + 1] their exclusive scan
  unsigned long long* bits; int* tile_counts; int* tile_offs;
  int nT, B;
};

static inline CpArgs cp_args(const CpLayout& L, void* work, long long* counts, long long* offsets, int B) {
  char* w = (char*)work;
  return {counts, offsets, (unsigned long long*)(w + L.bits), (int*)(w + L.tile_counts), (int*)(w + L.tile_offs), L.nT, B};
}

// ---- device
// Tile t of a member of n items: words[0..16) and *tile_count.  pred(item) is called for items < n only.
template <class Pred>
__device__ __forceinline__ void cp_flag(unsigned long long* words, int* tile_count, int t, int n, Pred pred) {
  __shared__ int wave_cnt[CP_THREADS / UD_WAVE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < CP_STEPS; ++j) {
    const unsigned p = (unsigned)t * CP_TILE + j * CP_THREADS + tid;       // < 2^31 + CP_TILE: fits unsigned
    const bool v = p < (unsigned)n && pred(p);
    const unsigned long long m = __ballot(v);                              // tails are false: every lane reaches every ballot
    if (lane == 0) words[j * (CP_THREADS / UD_WAVE) + w] = m;
    cnt += __popcll(m);
  }
  if (lane == 0) wave_cnt[w] = cnt;
  __syncthreads();
  if (tid == 0) *tile_count = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// Exclusive scan of in[0..n) by one workgroup of CP_SCAN threads, swept in chunks of CP_SCAN with a running carry; returns the total
// (the same value in every thread).  Integer sums in ACC: the order does not matter for the bits.
template <class ACC, class TI, class TO>
__device__ ACC cp_scan_sweep(const TI* in, TO* out, int n) {
  __shared__ ACC wave_tot[CP_SCAN / UD_WAVE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  ACC carry = 0;
  for (int base = 0; base < n; base += CP_SCAN) {
    const int i = base + tid;
    const ACC v = i < n ? (ACC)in[i] : 0;
    ACC inc = v;
#pragma unroll
    for (int o = 1; o < UD_WAVE; o <<= 1) {
      const ACC up = __shfl_up(inc, o, UD_WAVE);
      if (lane >= o) inc += up;
    }
    if (lane == UD_WAVE - 1) wave_tot[w] = inc;
    __syncthreads();
    ACC before = 0, chunk = 0;
#pragma unroll
    for (int k = 0; k < CP_SCAN / UD_WAVE; ++k) {
      const ACC tk = wave_tot[k];
      if (k < w) before += tk;
      chunk += tk;
    }
    if (i < n) out[i] = (TO)(carry + before + inc - v);
    carry += chunk;
    __syncthreads();                                  // wave_tot is rewritten by the next chunk
  }
  return carry;
}

// Tile t from its words[0..16): emit(item, row) for every set bit, row = the kept items of the tile before it.  A set bit: item < n.
template <class Emit>
__device__ __forceinline__ void cp_pack(const unsigned long long* words, int t, Emit emit) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // lanes 0..15 of every wave hold the tile's 16 words and the count of kept items in the words before each
  const unsigned long long my_word = lane < CP_WORDS ? words[lane] : 0ull;
  const int my_cnt = __popcll(my_word);
  int inc = my_cnt;
#pragma unroll
  for (int o = 1; o < CP_WORDS; o <<= 1) {
    const int up = __shfl_up(inc, o, UD_WAVE);
    if (lane >= o) inc += up;
  }
  const int my_before = inc - my_cnt;
#pragma unroll
  for (int j = 0; j < CP_STEPS; ++j) {
    const int k = j * (CP_THREADS / UD_WAVE) + w;
    const unsigned long long m = __shfl(my_word, k, UD_WAVE);
    const int before = __shfl(my_before, k, UD_WAVE);
    if ((m >> lane) & 1ull) emit(t * CP_TILE + k * UD_WAVE + lane, before + __popcll(m & ((1ull << lane) - 1ull)));
  }
}

// ---- a second packer reading the mask of a first (tsdf_mesh.hip: a face asks for its four vertices), after the first one's flag kernel
// and scans.  words: the 16 * nT words of ONE member, tile_offs: its nT entries; by the index map item p is bit p & 63 of word p >> 6.
__device__ __forceinline__ bool cp_test(const unsigned long long* words, long long item) { return (words[item >> 6] >> (item & 63)) & 1ull; }

// The row of a kept item inside its member: the kept items of the earlier tiles, of the tile's earlier words and of the word's lower bits.
__device__ __forceinline__ int cp_rank(const unsigned long long* words, const int* tile_offs, long long item) {
  const long long t = item / CP_TILE;
  const int k = (int)(item >> 6) & (CP_WORDS - 1);
  const unsigned long long* w = words + t * CP_WORDS;
  int r = tile_offs[t] + __popcll(w[k] & ((1ull << (item & 63)) - 1ull));
  for (int j = 0; j < k; ++j) r += __popcll(w[j]);
  return r;
}

// ---- the two scans of a packer whose result is counts / offsets (pointcloud.hip, tsdf.hip), launched after its flag kernel.  Templates,
// so that a file that does not launch them (eval3d.hip) does not carry them.
namespace {

template <class ACC>
__global__ __launch_bounds__(CP_SCAN) void cp_scan_tiles_kernel(CpArgs c) {     // one workgroup per member: tile_offs, counts[b]
  const int b = blockIdx.x;
  const ACC total = cp_scan_sweep<ACC>(c.tile_counts + (size_t)b * c.nT, c.tile_offs + (size_t)b * c.nT, c.nT);
  if (threadIdx.x == 0) c.counts[b] = total;
}

template <class ACC>
__global__ __launch_bounds__(CP_SCAN) void cp_scan_batch_kernel(CpArgs c) {     // one workgroup: offsets[0..B]
  const ACC total = cp_scan_sweep<ACC>(c.counts, c.offsets, c.B);
  if (threadIdx.x == 0) c.offsets[c.B] = total;
}

template <class ACC = long long>
void cp_launch_scans(const CpArgs& c, hipStream_t s) {
  hipLaunchKernelGGL(cp_scan_tiles_kernel<ACC>, dim3((unsigned)c.B), dim3(CP_SCAN), 0, s, c);
  hipLaunchKernelGGL(cp_scan_batch_kernel<ACC>, dim3(1), dim3(CP_SCAN), 0, s, c);
}

}  // namespace
