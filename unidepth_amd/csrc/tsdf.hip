// Depth views fused into a truncated signed distance (TSDF) volume, and the volume's surface read back as points (include/unidepth_hip.h,
// UdTsdfIntegrate / UdTsdfPoints): what follows ud_depth_consistency when several frames become one scene.
//
//   ts_integrate_kernel     one thread per voxel, x fastest, blockIdx.y = volume, 256 threads: the volume's loads and stores coalesce, and
//                           each view's model, parameter row and T are addressed by blockIdx.y and the view alone (scalar loads).  The view
//                           loop runs inside the thread: the centre, the distance, the weight and the colour stay in registers; a view
//                           costs one projection and one nearest-pixel gather (and its mask's, weight's and colour's).  All six camera
//                           models: projection is closed form for every one of them.  No LDS, no atomics, no workspace, no host
//                           synchronisation: captures into a graph.
//   tp_* kernels            the ordered compaction of csrc/compact.h over slots (3 * voxel + axis): tp_flag_kernel (cp_flag over
//                           ud_tsdf_slot), compact.h's scan per volume and scan over the volumes, tp_pack_kernel (cp_pack, the slot's row).
//                           Every dependency is a launch boundary: no atomics, no spinning; the order (volumes, then slots) and the bits
//                           are fixed.
//
// The arithmetic of a voxel and of a slot is csrc/tsdf_point.h, which only calls csrc/camera_models.h and csrc/remap_taps.h; the host build
// of the tests runs it under the sanitizers.  Built with -ffp-contract=off: every operation rounds separately, so the volume has the bits
// of project_camera, remap and the element-wise arithmetic run one after the other.
#include <math.h>
#include "compact.h"
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

// ---- surface extraction: compact.h's flag / scan / pack over slots -------------------------------------------------------------------
struct TpArgs {
  UdTsdfSlotArgs p;
  float* xyz; void* rgb;
  CpArgs c;
  long long capacity;
  int slots, rgb_f32;
};

__global__ __launch_bounds__(CP_THREADS) void tp_flag_kernel(TpArgs a) {
  const int t = blockIdx.x, b = blockIdx.y;
  const size_t tile = (size_t)b * a.c.nT + t;
  cp_flag(a.c.bits + tile * CP_WORDS, a.c.tile_counts + tile, t, a.slots,
          [=](unsigned s) { return ud_tsdf_slot(a.p, b, (long long)s, nullptr, nullptr); });
}

__global__ __launch_bounds__(CP_THREADS) void tp_pack_kernel(TpArgs a) {
  const int t = blockIdx.x, b = blockIdx.y;
  const size_t tile = (size_t)b * a.c.nT + t;
  const long long base = a.c.offsets[b] + a.c.tile_offs[tile];
  cp_pack(a.c.bits + tile * CP_WORDS, t, [=](int s, int row) {
    const long long r = base + row;
    if (r >= a.capacity) return;
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
  });
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
  return slots < 0 ? -1 : (long long)cp_layout(B, slots).total;
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
  const CpLayout L = cp_layout(d.B, slots);
  if (d.work_bytes < (long long)L.total) {
    ud_set_error("ud_tsdf_points: workspace smaller than ud_tsdf_points_work_bytes()");
    return UD_ERR_BAD_ARG;
  }
  TpArgs a;
  a.p.tsdf = d.tsdf; a.p.weight = d.weight; a.p.color = d.color; a.p.origin = d.origin;
  a.p.n = slots / 3;
  a.p.vs = vs; a.p.min_weight = min_weight;
  a.p.B = d.B; a.p.Nx = d.Nx; a.p.Ny = d.Ny; a.p.Nz = d.Nz; a.p.nO = d.n_origin;
  a.xyz = d.xyz; a.rgb = d.rgb;
  a.c = cp_args(L, d.work, d.counts, d.offsets, d.B);
  a.capacity = d.capacity;
  a.slots = (int)slots; a.rgb_f32 = d.rgb_f32 != 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)L.nT, (unsigned)d.B);
  hipLaunchKernelGGL(tp_flag_kernel, grid, dim3(CP_THREADS), 0, s, a);
  cp_launch_scans(a.c, s);
  if (d.xyz && d.capacity > 0) hipLaunchKernelGGL(tp_pack_kernel, grid, dim3(CP_THREADS), 0, s, a);
  UD_CHECK_LAUNCH("ud_tsdf_points launch");
  return UD_OK;
}
