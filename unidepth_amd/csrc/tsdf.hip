// Depth views fused into a truncated signed distance (TSDF) volume, and the volume's surface read back as points (include/unidepth_hip.h,
// UdTsdfIntegrate / UdTsdfPoints): what follows ud_depth_consistency when several frames become one scene.
//
//   ts_integrate_kernel     one thread per voxel, x fastest, blockIdx.y = volume, 256 threads: the volume's loads and stores coalesce, and
//                           each view's model, parameter row and T are addressed by blockIdx.y and the view alone (scalar loads).  The view
//                           loop runs inside the thread: the centre, the distance, the weight and the colour stay in registers; a view
//                           costs one projection and one nearest-pixel gather (and its mask's, weight's and colour's).  All six camera
//                           models: projection is closed form for every one of them.  No LDS, no atomics, no workspace, no host
//                           synchronisation: captures into a graph.
//   tp_* kernels            the ordered compaction of pointcloud.hip over slots (3 * voxel + axis) instead of pixels: tiles of 1024
//                           consecutive slots of one volume, ballot words, a scan per volume, a scan over the volumes, a pack.  Every
//                           dependency is a launch boundary: no atomics, no spinning; the order (volumes, then slots) and the bits are fixed.
//
// The arithmetic of a voxel and of a slot is csrc/tsdf_point.h, which only calls csrc/camera_models.h and csrc/remap_taps.h; the host build
// of the tests runs it under the sanitizers.  Built with -ffp-contract=off: every operation rounds separately, so the volume has the bits
// of project_camera, remap and the element-wise arithmetic run one after the other.
#include <math.h>
#include "ud_common.h"
#include "tsdf_point.h"
#pragma clang fp contract(off)

namespace {

constexpr int TS_THREADS = 256;

struct TsKernelArgs {
  UdTsdfArgs p;
  unsigned char model[UD_RECON_MAX_B];                 // model[v * B + b]
};

__global__ __launch_bounds__(TS_THREADS) void ts_integrate_kernel(const TsKernelArgs a) {
  const long long i = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
  if (i >= a.p.n) return;
  ud_tsdf_voxel(a.p, a.model, (int)blockIdx.y, i);
}

// ---- surface extraction: pointcloud.hip's flag / scan / pack over slots ---------------------------------------------------------------
constexpr int TP_THREADS = 256;
constexpr int TP_STEPS = 4;
constexpr int TP_TILE = TP_THREADS * TP_STEPS;
constexpr int TP_WORDS = TP_TILE / UD_WAVE;            // 16 ballot words per tile
constexpr int TP_SCAN = 256;

struct TpLayout {
  size_t bits, tile_counts, tile_offs, total;
  int nT;
};

TpLayout tp_layout(int B, long long slots) {
  TpLayout L;
  L.nT = (int)((slots + TP_TILE - 1) / TP_TILE);
  const size_t tiles = (size_t)B * L.nT;
  L.bits = 0;
  L.tile_counts = tiles * TP_WORDS * sizeof(unsigned long long);
  L.tile_offs = L.tile_counts + tiles * sizeof(int);
  L.total = L.tile_offs + tiles * sizeof(int);
  return L;
}

struct TpArgs {
  UdTsdfSlotArgs p;
  float* xyz; void* rgb; long long* counts; long long* offsets;
  unsigned long long* bits; int* tile_counts; int* tile_offs;
  long long capacity;
  int slots, nT, rgb_f32;
};

__global__ __launch_bounds__(TP_THREADS) void tp_flag_kernel(TpArgs a) {
  __shared__ int wave_cnt[TP_THREADS / UD_WAVE];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned long long* words = a.bits + ((size_t)b * a.nT + t) * TP_WORDS;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < TP_STEPS; ++j) {
    const unsigned s = (unsigned)t * TP_TILE + j * TP_THREADS + tid;       // < 2^31 + TP_TILE: fits unsigned
    const bool v = s < (unsigned)a.slots && ud_tsdf_slot(a.p, b, (long long)s, nullptr, nullptr);
    const unsigned long long m = __ballot(v);                              // tails are false: every lane reaches every ballot
    if (lane == 0) words[j * (TP_THREADS / UD_WAVE) + w] = m;
    cnt += __popcll(m);
  }
  if (lane == 0) wave_cnt[w] = cnt;
  __syncthreads();
  if (tid == 0) a.tile_counts[(size_t)b * a.nT + t] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// Exclusive scan of in[0..n) by one workgroup of TP_SCAN threads, swept in chunks of TP_SCAN with a running carry; returns the total (the
// same value in every thread).  Integer sums: the order does not matter for the bits.  (pointcloud.hip's sweep, which is local to that file.)
template <class TI, class TO>
__device__ long long tp_scan_sweep(const TI* in, TO* out, int n) {
  __shared__ long long wave_tot[TP_SCAN / UD_WAVE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long carry = 0;
  for (int base = 0; base < n; base += TP_SCAN) {
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
    for (int k = 0; k < TP_SCAN / UD_WAVE; ++k) {
      const long long tk = wave_tot[k];
      if (k < w) before += tk;
      chunk += tk;
    }
    if (i < n) out[i] = (TO)(carry + before + inc - v);
    carry += chunk;
    __syncthreads();                                   // wave_tot is rewritten by the next chunk
  }
  return carry;
}

__global__ __launch_bounds__(TP_SCAN) void tp_scan_tiles_kernel(TpArgs a) {
  const int b = blockIdx.x;
  const long long total = tp_scan_sweep(a.tile_counts + (size_t)b * a.nT, a.tile_offs + (size_t)b * a.nT, a.nT);
  if (threadIdx.x == 0) a.counts[b] = total;
}

__global__ __launch_bounds__(TP_SCAN) void tp_scan_volumes_kernel(TpArgs a) {
  const long long total = tp_scan_sweep(a.counts, a.offsets, a.p.B);
  if (threadIdx.x == 0) a.offsets[a.p.B] = total;
}

__global__ __launch_bounds__(TP_THREADS) void tp_pack_kernel(TpArgs a) {
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long base = a.offsets[b] + a.tile_offs[(size_t)b * a.nT + t];
  // lanes 0..15 of every wave hold the tile's 16 words and the count of live slots in the words before each
  const unsigned long long my_word = lane < TP_WORDS ? a.bits[((size_t)b * a.nT + t) * TP_WORDS + lane] : 0ull;
  const int my_cnt = __popcll(my_word);
  int inc = my_cnt;
#pragma unroll
  for (int o = 1; o < TP_WORDS; o <<= 1) {
    const int up = __shfl_up(inc, o, UD_WAVE);
    if (lane >= o) inc += up;
  }
  const int my_before = inc - my_cnt;
#pragma unroll
  for (int j = 0; j < TP_STEPS; ++j) {
    const int k = j * (TP_THREADS / UD_WAVE) + w;
    const unsigned long long m = __shfl(my_word, k, UD_WAVE);
    const int before = __shfl(my_before, k, UD_WAVE);
    if (!((m >> lane) & 1ull)) continue;
    const long long r = base + before + __popcll(m & ((1ull << lane) - 1ull));
    if (r >= a.capacity) continue;
    const long long s = (long long)t * TP_TILE + k * UD_WAVE + lane;        // a set bit: s < slots
    float xyz[3], rgb[3] = {0.0f, 0.0f, 0.0f};
    ud_tsdf_slot(a.p, b, s, xyz, rgb);
    float* o = a.xyz + r * 3;
    o[0] = xyz[0]; o[1] = xyz[1]; o[2] = xyz[2];
    if (a.rgb) {
      if (a.rgb_f32) {
        float* oc = (float*)a.rgb + r * 3;
        oc[0] = rgb[0]; oc[1] = rgb[1]; oc[2] = rgb[2];
      } else {
        unsigned char* oc = (unsigned char*)a.rgb + r * 3;
        oc[0] = ud_rm_to_u8(rgb[0]); oc[1] = ud_rm_to_u8(rgb[1]); oc[2] = ud_rm_to_u8(rgb[2]);
      }
    }
  }
}

bool ts_positive(float x) { return x > 0.0f && x <= 3.402823466e38f; }     // finite and > 0 (false for a NaN)

}  // namespace

extern "C" int ud_tsdf_integrate(const UdTsdfIntegrate* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_tsdf_integrate: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdTsdfIntegrate& d = *desc;
  if (d.B < 1 || d.V < 1 || d.V > 255 || (long long)d.B * d.V > UD_RECON_MAX_B || d.Nx < 1 || d.Ny < 1 || d.Nz < 1 || d.Hs < 1 || d.Ws < 1) {
    ud_set_error("ud_tsdf_integrate: bad sizes (B, V >= 1, B * V <= 256, V <= 255, Nx, Ny, Nz, Hs, Ws >= 1)");
    return UD_ERR_BAD_ARG;
  }
  const long long nxy = (long long)d.Nx * d.Ny, hw = (long long)d.Hs * d.Ws;
  if (nxy >= UD_MAX_ELEMS || nxy * d.Nz >= UD_MAX_ELEMS || hw >= UD_MAX_ELEMS || d.V * 3 * hw >= UD_MAX_ELEMS) {
    ud_set_error("ud_tsdf_integrate: too large (Nx * Ny * Nz, Hs * Ws and V * 3 * Hs * Ws must stay below 2^31 - 256)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.src_depth || !d.params || !d.T || !d.origin || !d.tsdf || !d.weight) {
    ud_set_error("ud_tsdf_integrate: null pointer (src_depth, params, T, origin, tsdf, weight)");
    return UD_ERR_BAD_ARG;
  }
  if ((d.image != nullptr) != (d.color != nullptr)) {
    ud_set_error("ud_tsdf_integrate: image and color go together (both or neither)");
    return UD_ERR_BAD_ARG;
  }
  if (d.nT != 1 && d.nT != d.B) {
    ud_set_error("ud_tsdf_integrate: nT must be 1 or B (sets of V matrices)");
    return UD_ERR_BAD_ARG;
  }
  if (d.n_origin != 1 && d.n_origin != d.B) {
    ud_set_error("ud_tsdf_integrate: n_origin must be 1 or B (rows of the origin)");
    return UD_ERR_BAD_ARG;
  }
  const float vs = ud_f32_from_bits(d.voxel_size_bits), trunc = ud_f32_from_bits(d.trunc_bits), max_weight = ud_f32_from_bits(d.max_weight_bits);
  if (!ts_positive(vs) || !ts_positive(trunc)) {
    ud_set_error("ud_tsdf_integrate: voxel_size and trunc must be finite and positive");
    return UD_ERR_BAD_ARG;
  }
  if (d.has_max_weight && !ts_positive(max_weight)) {
    ud_set_error("ud_tsdf_integrate: max_weight must be finite and positive when given");
    return UD_ERR_BAD_ARG;
  }
  for (int k = 0; k < d.B * d.V; ++k) {
    if (!ud_cam_model_ok(d.model[k])) {
      ud_set_error("ud_tsdf_integrate: model tag outside 1..6");
      return UD_ERR_BAD_ARG;
    }
  }
  TsKernelArgs a;
  a.p.src_depth = d.src_depth; a.p.src_mask = d.src_mask; a.p.src_weight = d.src_weight; a.p.image = d.image;
  a.p.params = d.params; a.p.T = d.T; a.p.origin = d.origin;
  a.p.tsdf = d.tsdf; a.p.weight = d.weight; a.p.color = d.color; a.p.count = d.count;
  a.p.n = nxy * d.Nz;
  a.p.vs = vs; a.p.trunc = trunc; a.p.max_weight = d.has_max_weight ? max_weight : 0.0f;
  a.p.B = d.B; a.p.V = d.V; a.p.Nx = d.Nx; a.p.Ny = d.Ny; a.p.Nz = d.Nz; a.p.Hs = d.Hs; a.p.Ws = d.Ws; a.p.nT = d.nT; a.p.nO = d.n_origin;
  a.p.fresh = d.fresh != 0; a.p.has_max = d.has_max_weight != 0;
  ud_copy_models(a.model, d.model, d.B * d.V);
  const dim3 grid((unsigned)((a.p.n + TS_THREADS - 1) / TS_THREADS), (unsigned)d.B);
  hipLaunchKernelGGL(ts_integrate_kernel, grid, dim3(TS_THREADS), 0, (hipStream_t)stream, a);
  UD_CHECK_LAUNCH("ud_tsdf_integrate launch");
  return UD_OK;
}

// the slots of one volume, or -1 outside the limits
static long long tp_slots(int B, int Nx, int Ny, int Nz) {
  if (B < 1 || B > 65535 || Nx < 1 || Ny < 1 || Nz < 1) return -1;
  const long long nxy = (long long)Nx * Ny;
  if (nxy >= UD_MAX_ELEMS || nxy * Nz >= UD_MAX_ELEMS || 3 * nxy * Nz >= UD_MAX_ELEMS) return -1;
  return 3 * nxy * Nz;
}

extern "C" long long ud_tsdf_points_work_bytes(int B, int Nx, int Ny, int Nz) {
  const long long slots = tp_slots(B, Nx, Ny, Nz);
  return slots < 0 ? -1 : (long long)tp_layout(B, slots).total;
}

extern "C" int ud_tsdf_points(const UdTsdfPoints* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_tsdf_points: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdTsdfPoints& d = *desc;
  const long long slots = tp_slots(d.B, d.Nx, d.Ny, d.Nz);
  if (slots < 0 || d.capacity < 0) {
    ud_set_error("ud_tsdf_points: bad sizes (1 <= B <= 65535, Nx, Ny, Nz >= 1, 3 * Nx * Ny * Nz < 2^31 - 256, capacity >= 0)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.tsdf || !d.weight || !d.origin || !d.counts || !d.offsets || !d.work || ((uintptr_t)d.work & 7)) {
    ud_set_error("ud_tsdf_points: null pointer (tsdf, weight, origin, counts, offsets, work), or work not 8-byte aligned");
    return UD_ERR_BAD_ARG;
  }
  if (d.rgb && (!d.color || !d.xyz)) {
    ud_set_error("ud_tsdf_points: rgb needs a color volume and xyz");
    return UD_ERR_BAD_ARG;
  }
  if (d.n_origin != 1 && d.n_origin != d.B) {
    ud_set_error("ud_tsdf_points: n_origin must be 1 or B (rows of the origin)");
    return UD_ERR_BAD_ARG;
  }
  const float vs = ud_f32_from_bits(d.voxel_size_bits), min_weight = ud_f32_from_bits(d.min_weight_bits);
  if (!ts_positive(vs)) {
    ud_set_error("ud_tsdf_points: voxel_size must be finite and positive");
    return UD_ERR_BAD_ARG;
  }
  if (min_weight != min_weight) {
    ud_set_error("ud_tsdf_points: min_weight must not be a NaN");
    return UD_ERR_BAD_ARG;
  }
  const TpLayout L = tp_layout(d.B, slots);
  if (d.work_bytes < (long long)L.total) {
    ud_set_error("ud_tsdf_points: workspace smaller than ud_tsdf_points_work_bytes()");
    return UD_ERR_BAD_ARG;
  }
  char* w = (char*)d.work;
  TpArgs a;
  a.p.tsdf = d.tsdf; a.p.weight = d.weight; a.p.color = d.color; a.p.origin = d.origin;
  a.p.n = slots / 3;
  a.p.vs = vs; a.p.min_weight = min_weight;
  a.p.B = d.B; a.p.Nx = d.Nx; a.p.Ny = d.Ny; a.p.Nz = d.Nz; a.p.nO = d.n_origin;
  a.xyz = d.xyz; a.rgb = d.rgb; a.counts = d.counts; a.offsets = d.offsets;
  a.bits = (unsigned long long*)(w + L.bits); a.tile_counts = (int*)(w + L.tile_counts); a.tile_offs = (int*)(w + L.tile_offs);
  a.capacity = d.capacity;
  a.slots = (int)slots; a.nT = L.nT; a.rgb_f32 = d.rgb_f32 != 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)L.nT, (unsigned)d.B);
  hipLaunchKernelGGL(tp_flag_kernel, grid, dim3(TP_THREADS), 0, s, a);
  hipLaunchKernelGGL(tp_scan_tiles_kernel, dim3((unsigned)d.B), dim3(TP_SCAN), 0, s, a);
  hipLaunchKernelGGL(tp_scan_volumes_kernel, dim3(1), dim3(TP_SCAN), 0, s, a);
  if (d.xyz && d.capacity > 0) hipLaunchKernelGGL(tp_pack_kernel, grid, dim3(TP_THREADS), 0, s, a);
  UD_CHECK_LAUNCH("ud_tsdf_points launch");
  return UD_OK;
}
