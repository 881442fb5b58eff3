// The surface of a TSDF volume as an indexed triangle mesh (include/unidepth_hip.h, UdTsdfMesh): naive surface nets as two ordered
// compactions of csrc/compact.h, one over CELLS (n items per volume: the vertices) and one over SLOTS (3 * n items: the quads), the
// second reading the first one's mask.
//
//   tm_cell_flag_kernel   cp_flag over ud_tsdf_cell: one thread per cell, x fastest, so the eight corner loads of a wave are eight
//                         coalesced row segments (plain loads, no LDS: neighbouring lanes share corners through the cache)
//   compact.h's scans     vert_counts / vert_offsets and the cell tiles' offsets
//   tm_slot_flag_kernel   cp_flag over ud_tsdf_quad: the slot's own predicate plus four bits of the cell mask (cp_test)
//   tm_scan_faces_kernel  the slot tiles' offsets in quads, face_counts in triangles (2 per quad); compact.h's scan over the volumes
//   tm_vert_pack_kernel   cp_pack over the cell mask: the vertex, its colour and its normal (ud_tsdf_cell again, with outputs)
//   tm_face_pack_kernel   cp_pack over the slot mask: the quad's four cells become vertex rows local to the volume (cp_rank) and two
//                         triangles
// Every dependency is a launch boundary: no atomics, no spinning, no host synchronisation; the order (volumes, then cells / slots) and
// every bit are fixed.  The arithmetic is csrc/tsdf_mesh_point.h over csrc/tsdf_point.h; the host build of the tests runs it under the
// sanitizers.  Built with -ffp-contract=off: a crossing has the bits ud_tsdf_points gives it.
#include <math.h>
#include "compact.h"
#include "tsdf_mesh_point.h"
#pragma clang fp contract(off)

namespace {

struct TmArgs {
  UdTsdfSlotArgs p;
  float* vertices; void* rgb; float* normals; int* faces;
  CpArgs cv, cf;                                       // cells -> vertices, slots -> quads (cf.counts / cf.offsets count triangles)
  long long vert_capacity, face_capacity;
  int cells, slots, rgb_f32;
};

__global__ __launch_bounds__(CP_THREADS) void tm_cell_flag_kernel(TmArgs a) {
  const int t = blockIdx.x, b = blockIdx.y;
  const size_t tile = (size_t)b * a.cv.nT + t;
  cp_flag(a.cv.bits + tile * CP_WORDS, a.cv.tile_counts + tile, t, a.cells,
          [=](unsigned i) { return ud_tsdf_cell(a.p, b, (long long)i, nullptr, nullptr, nullptr); });
}

__global__ __launch_bounds__(CP_THREADS) void tm_slot_flag_kernel(TmArgs a) {
  const int t = blockIdx.x, b = blockIdx.y;
  const size_t tile = (size_t)b * a.cf.nT + t;
  const unsigned long long* cell_bits = a.cv.bits + (size_t)b * a.cv.nT * CP_WORDS;
  cp_flag(a.cf.bits + tile * CP_WORDS, a.cf.tile_counts + tile, t, a.slots, [=](unsigned s) {
    return ud_tsdf_quad(a.p, b, (long long)s, [=](long long i) { return cp_test(cell_bits, i); }, nullptr);
  });
}

__global__ __launch_bounds__(CP_SCAN) void tm_scan_faces_kernel(CpArgs c) {     // one workgroup per volume: tile_offs in quads, counts in triangles
  const int b = blockIdx.x;
  const long long quads = cp_scan_sweep<long long>(c.tile_counts + (size_t)b * c.nT, c.tile_offs + (size_t)b * c.nT, c.nT);
  if (threadIdx.x == 0) c.counts[b] = 2 * quads;
}

__global__ __launch_bounds__(CP_THREADS) void tm_vert_pack_kernel(TmArgs a) {
  const int t = blockIdx.x, b = blockIdx.y;
  const size_t tile = (size_t)b * a.cv.nT + t;
  const long long base = a.cv.offsets[b] + a.cv.tile_offs[tile];
  cp_pack(a.cv.bits + tile * CP_WORDS, t, [=](int i, int row) {
    const long long r = base + row;
    if (r >= a.vert_capacity) return;
    float xyz[3], rgb[3] = {0.0f, 0.0f, 0.0f}, nrm[3];
    ud_tsdf_cell(a.p, b, i, xyz, rgb, nrm);               // every output asked for: a pointer chosen at run time would put the arrays in memory
    float* o = a.vertices + r * 3;
    o[0] = xyz[0]; o[1] = xyz[1]; o[2] = xyz[2];
    if (a.normals) {
      float* on = a.normals + r * 3;
      on[0] = nrm[0]; on[1] = nrm[1]; on[2] = nrm[2];
    }
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

__global__ __launch_bounds__(CP_THREADS) void tm_face_pack_kernel(TmArgs a) {
  const int t = blockIdx.x, b = blockIdx.y;
  const size_t tile = (size_t)b * a.cf.nT + t;
  const long long base = a.cf.offsets[b] / 2 + a.cf.tile_offs[tile];           // in quads
  const unsigned long long* cell_bits = a.cv.bits + (size_t)b * a.cv.nT * CP_WORDS;
  const int* cell_offs = a.cv.tile_offs + (size_t)b * a.cv.nT;
  cp_pack(a.cf.bits + tile * CP_WORDS, t, [=](int s, int row) {
    const long long r = 2 * (base + row);                                      // the quad's first triangle; both fit or neither is written
    if (r + 1 >= a.face_capacity) return;
    int q[4];
    ud_tsdf_quad(a.p, b, s, [=](long long i) { return cp_test(cell_bits, i); }, q);
    const int v0 = cp_rank(cell_bits, cell_offs, q[0]), v1 = cp_rank(cell_bits, cell_offs, q[1]);
    const int v2 = cp_rank(cell_bits, cell_offs, q[2]), v3 = cp_rank(cell_bits, cell_offs, q[3]);
    int* o = a.faces + r * 3;
    o[0] = v0; o[1] = v1; o[2] = v2;
    o[3] = v0; o[4] = v2; o[5] = v3;
  });
}

bool tm_positive(float x) { return x > 0.0f && x <= 3.402823466e38f; }     // finite and > 0 (false for a NaN)

// the voxels of one volume, or -1 outside the limits (ud_tsdf_points': the slots must stay below 2^31 - 256)
long long tm_cells(int B, int Nx, int Ny, int Nz) {
  if (B < 1 || B > 65535 || Nx < 1 || Ny < 1 || Nz < 1) return -1;
  const long long nxy = (long long)Nx * Ny;
  if (nxy >= UD_MAX_ELEMS || nxy * Nz >= UD_MAX_ELEMS || 3 * nxy * Nz >= UD_MAX_ELEMS) return -1;
  return nxy * Nz;
}

// the work area: the cells' cp_layout, then the slots', 8-byte aligned
size_t tm_second(const CpLayout& cells) { return (cells.total + 7) & ~(size_t)7; }

}  // namespace

extern "C" long long ud_tsdf_mesh_work_bytes(int B, int Nx, int Ny, int Nz) {
  const long long n = tm_cells(B, Nx, Ny, Nz);
  return n < 0 ? -1 : (long long)(tm_second(cp_layout(B, n)) + cp_layout(B, 3 * n).total);
}

extern "C" int ud_tsdf_mesh(const UdTsdfMesh* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_tsdf_mesh: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdTsdfMesh& d = *desc;
  const long long n = tm_cells(d.B, d.Nx, d.Ny, d.Nz);
  if (n < 0 || d.vert_capacity < 0 || d.face_capacity < 0) {
    ud_set_error("ud_tsdf_mesh: bad sizes (1 <= B <= 65535, Nx, Ny, Nz >= 1, 3 * Nx * Ny * Nz < 2^31 - 256, vert_capacity, face_capacity >= 0)");
    return UD_ERR_BAD_ARG;
  }
  if (!d.tsdf || !d.weight || !d.origin || !d.vert_counts || !d.vert_offsets || !d.face_counts || !d.face_offsets || !d.work ||
      ((uintptr_t)d.work & 7)) {
    ud_set_error("ud_tsdf_mesh: null pointer (tsdf, weight, origin, vert_counts, vert_offsets, face_counts, face_offsets, work), or work not "
                 "8-byte aligned");
    return UD_ERR_BAD_ARG;
  }
  if (d.rgb && (!d.color || !d.vertices)) {
    ud_set_error("ud_tsdf_mesh: rgb needs a color volume and vertices");
    return UD_ERR_BAD_ARG;
  }
  if (d.normals && !d.vertices) {
    ud_set_error("ud_tsdf_mesh: normals need vertices");
    return UD_ERR_BAD_ARG;
  }
  if (d.n_origin != 1 && d.n_origin != d.B) {
    ud_set_error("ud_tsdf_mesh: n_origin must be 1 or B (rows of the origin)");
    return UD_ERR_BAD_ARG;
  }
  const float vs = ud_f32_from_bits(d.voxel_size_bits), min_weight = ud_f32_from_bits(d.min_weight_bits);
  if (!tm_positive(vs)) {
    ud_set_error("ud_tsdf_mesh: voxel_size must be finite and positive");
    return UD_ERR_BAD_ARG;
  }
  if (min_weight != min_weight) {
    ud_set_error("ud_tsdf_mesh: min_weight must not be a NaN");
    return UD_ERR_BAD_ARG;
  }
  const CpLayout Lv = cp_layout(d.B, n), Lf = cp_layout(d.B, 3 * n);
  const size_t second = tm_second(Lv);
  if (d.work_bytes < (long long)(second + Lf.total)) {
    ud_set_error("ud_tsdf_mesh: workspace smaller than ud_tsdf_mesh_work_bytes()");
    return UD_ERR_BAD_ARG;
  }
  TmArgs a;
  a.p.tsdf = d.tsdf; a.p.weight = d.weight; a.p.color = d.rgb ? d.color : nullptr; a.p.origin = d.origin;     // colours are read for rgb alone
  a.p.n = n;
  a.p.vs = vs; a.p.min_weight = min_weight;
  a.p.B = d.B; a.p.Nx = d.Nx; a.p.Ny = d.Ny; a.p.Nz = d.Nz; a.p.nO = d.n_origin;
  a.vertices = d.vertices; a.rgb = d.rgb; a.normals = d.normals; a.faces = d.faces;
  a.cv = cp_args(Lv, d.work, d.vert_counts, d.vert_offsets, d.B);
  a.cf = cp_args(Lf, (char*)d.work + second, d.face_counts, d.face_offsets, d.B);
  a.vert_capacity = d.vert_capacity; a.face_capacity = d.face_capacity;
  a.cells = (int)n; a.slots = (int)(3 * n); a.rgb_f32 = d.rgb_f32 != 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 cell_grid((unsigned)Lv.nT, (unsigned)d.B), slot_grid((unsigned)Lf.nT, (unsigned)d.B);
  hipLaunchKernelGGL(tm_cell_flag_kernel, cell_grid, dim3(CP_THREADS), 0, s, a);
  cp_launch_scans(a.cv, s);
  hipLaunchKernelGGL(tm_slot_flag_kernel, slot_grid, dim3(CP_THREADS), 0, s, a);
  hipLaunchKernelGGL(tm_scan_faces_kernel, dim3((unsigned)d.B), dim3(CP_SCAN), 0, s, a.cf);
  hipLaunchKernelGGL(cp_scan_batch_kernel<long long>, dim3(1), dim3(CP_SCAN), 0, s, a.cf);
  if (d.vertices && d.vert_capacity > 0) hipLaunchKernelGGL(tm_vert_pack_kernel, cell_grid, dim3(CP_THREADS), 0, s, a);
  if (d.faces && d.face_capacity > 0) hipLaunchKernelGGL(tm_face_pack_kernel, slot_grid, dim3(CP_THREADS), 0, s, a);
  UD_CHECK_LAUNCH("ud_tsdf_mesh launch");
  return UD_OK;
}
