// Packed point clouds from dense prediction maps (include/unidepth_hip.h, UdPointCloud): an ordered stream compaction of the valid
// pixels of a batch, the device form of the reference's get_pointcloud_from_rgbd (unidepth/utils/visualization.py:57-104).
//
// The compaction itself (tiles of 1024 consecutive pixels of ONE image, the lane / word / step map, the scans) is csrc/compact.h; this
// file holds the predicate of a pixel and the writer of a row.
//   1. pc_flag_kernel        cp_flag over pc_predicate -> the bitmask (16 ballot words per tile) and tile_counts[b][t]
//   2. cp_scan_tiles_kernel  one workgroup per image: exclusive scan of its tile counts -> tile_offs, counts[b]
//      cp_scan_batch_kernel  one workgroup: exclusive scan of counts -> offsets[0..B]
//   3. pc_pack_kernel        cp_pack: row = offsets[b] + tile_offs[b][t] + the row inside the tile; rows below `capacity` are written,
//                            only valid pixels read their payload
// Every dependency is a launch boundary: no atomics, no tickets, no spinning, no float reduction; the output order (images in batch
// order, pixels row-major) and every bit of it are fixed.  Built with -ffp-contract=off: (u - cx) * d / fx rounds three times.
#include "compact.h"

namespace {

struct PcArgs {
  const float* points; const float* depth; const float* K;
  const unsigned char* image; const float* image_f32; const unsigned char* mask; const float* conf;
  float* xyz; void* rgb; int* index;
  CpArgs c;
  long long capacity;
  int H, W, HW, nK, flags;
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

__global__ __launch_bounds__(CP_THREADS) void pc_flag_kernel(PcArgs a) {
  const int t = blockIdx.x, b = blockIdx.y;
  const size_t tile = (size_t)b * a.c.nT + t;
  cp_flag(a.c.bits + tile * CP_WORDS, a.c.tile_counts + tile, t, a.HW, [=](int p) { return pc_predicate(a, b, p); });
}

__global__ __launch_bounds__(CP_THREADS) void pc_pack_kernel(PcArgs a) {
  const int t = blockIdx.x, b = blockIdx.y;
  const size_t tile = (size_t)b * a.c.nT + t;
  const long long base = a.c.offsets[b] + a.c.tile_offs[tile];
  const size_t img = (size_t)b * a.HW;
  float fx = 1.0f, fy = 1.0f, cx = 0.0f, cy = 0.0f;
  if (!a.points) {
    const float* K = a.K + (a.nK == 1 ? 0 : (size_t)b * 9);
    fx = K[0]; cx = K[2]; fy = K[4]; cy = K[5];
  }
  cp_pack(a.c.bits + tile * CP_WORDS, t, [=](int p, int row) {
    const long long r = base + row;
    if (r >= a.capacity) return;
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
  });
}

}  // namespace

extern "C" long long ud_pointcloud_work_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return -1;
  return (long long)cp_layout(B, (long long)H * W).total;
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
  const CpLayout L = cp_layout(d.B, (long long)d.H * d.W);
  if (d.work_bytes < (long long)L.total) {
    ud_set_error("ud_pointcloud_pack: workspace smaller than ud_pointcloud_work_bytes()");
    return UD_ERR_BAD_ARG;
  }
  PcArgs a;
  a.points = d.points; a.depth = d.depth; a.K = d.K; a.image = d.image; a.image_f32 = d.image_f32; a.mask = d.mask; a.conf = d.confidence;
  a.xyz = d.xyz; a.rgb = d.rgb; a.index = d.index;
  a.c = cp_args(L, d.work, d.counts, d.offsets, d.B);
  a.capacity = d.capacity;
  a.H = d.H; a.W = d.W; a.HW = d.H * d.W; a.nK = d.nK; a.flags = d.flags;
  a.min_conf = d.min_conf; a.dmin = d.dmin; a.dmax = d.dmax; a.edge_rtol = d.edge_rtol;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)L.nT, (unsigned)d.B);
  hipLaunchKernelGGL(pc_flag_kernel, grid, dim3(CP_THREADS), 0, s, a);
  cp_launch_scans(a.c, s);
  if (d.xyz && d.capacity > 0) hipLaunchKernelGGL(pc_pack_kernel, grid, dim3(CP_THREADS), 0, s, a);
  UD_CHECK_LAUNCH("ud_pointcloud_pack launch");
  return UD_OK;
}
