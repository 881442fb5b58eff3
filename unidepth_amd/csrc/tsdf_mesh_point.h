// Per-cell and per-slot arithmetic of the surface mesh of a TSDF volume (include/unidepth_hip.h, UdTsdfMesh): naive surface nets.  A CELL is
// the cube between voxel i and its seven +x / +y / +z neighbours; it is an item of the voxel index space (border voxels have no cell).  A
// live cell carries one vertex, the mean of the crossing points of its edges, and a live slot of tsdf_point.h (an edge with a sign change)
// whose four surrounding cells are live carries one quad between their vertices.  Plain functions with no device intrinsics and no kernel:
// they call ud_tsdf_slot and change nothing of it, so a crossing has the bits tsdf_points gives it.  tsdf_mesh.hip compiles them into its
// kernels; tests/tsdf_mesh_host/tsdf_mesh_host.cpp compiles the same header for the host, under the sanitizers.
//
// SAFETY RULE: tsdf_point.h's, unchanged.  The only indices formed here are the cell's own voxel (i < n, checked by the caller), its seven
// neighbours' (all three coordinates checked against the grid first) and, for a quad, the three cells below the slot's voxel (the two
// coordinates checked to be >= 1 first).  Every operation rounds separately (-ffp-contract=off).
#pragma once
#include <math.h>
#include "tsdf_point.h"
#pragma clang fp contract(off)

// Cell i of volume b, i < n.  Live when the cell exists (ix + 1 < Nx, iy + 1 < Ny, iz + 1 < Nz), all eight weights are >= min_weight, no
// corner distance is a NaN and the corners are not all of one sign (d < 0 is the sign).  For a live cell with xyz given: the edges
// e = 4 * axis + k, k = 0..3, in order -- the lower voxel of edge e is the cell's voxel moved by k & 1 along the lower and by (k >> 1) & 1
// along the higher of the two other axes, and the edge is slot 3 * lower + axis -- and over those with a live slot the crossing points
// summed in that order (the first initialises the sum) and divided by their number; rgb (with a colour volume; may be null) the slots'
// blended colours averaged the same way, not yet rounded.  normal (may be null): g[axis] = the four edges' (d1 - d0) summed in edge order,
// crossing or not, divided by sqrtf(g0 * g0 + g1 * g1 + g2 * g2), or (0, 0, 0) when that length is not finite and positive.
UD_RM_FN bool ud_tsdf_cell(const UdTsdfSlotArgs& a, int b, long long i, float* xyz, float* rgb, float* normal) {
  const size_t n = (size_t)a.n;
  const int row = (int)(i / a.Nx), ix = (int)(i - (long long)row * a.Nx), iz = row / a.Ny, iy = row - iz * a.Ny;
  if (!(ix + 1 < a.Nx && iy + 1 < a.Ny && iz + 1 < a.Nz)) return false;
  const size_t sx = 1, sy = (size_t)a.Nx, sz = (size_t)a.Nx * (size_t)a.Ny, at = (size_t)b * n + (size_t)i;
  float d[8];                                            // corner dx + 2 * dy + 4 * dz
  bool ok = true, any_neg = false, any_pos = false;
  for (int c = 0; c < 8; ++c) {
    const size_t j = at + (c & 1 ? sx : 0) + (c & 2 ? sy : 0) + (c & 4 ? sz : 0);
    const float dc = a.tsdf[j];
    d[c] = dc;
    ok = ok && a.weight[j] >= a.min_weight && dc == dc;
    if (dc < 0.0f) any_neg = true;
    else any_pos = true;
  }
  if (!ok || !(any_neg && any_pos)) return false;
  if (xyz) {
    float acc[3] = {0.0f, 0.0f, 0.0f}, col[3] = {0.0f, 0.0f, 0.0f};
    const bool with_rgb = rgb && a.color;
    int count = 0;
    for (int e = 0; e < 12; ++e) {
      const int axis = e >> 2, k0 = e & 1, k1 = (e >> 1) & 1;
      // the two other axes in ascending order: (y, z) for x, (x, z) for y, (x, y) for z
      const size_t s0 = axis == 0 ? sy : sx, s1 = axis == 2 ? sy : sz;
      const long long lower = i + (long long)(k0 ? s0 : 0) + (long long)(k1 ? s1 : 0);
      float p[3], c[3] = {0.0f, 0.0f, 0.0f};
      if (!ud_tsdf_slot(a, b, 3 * lower + axis, p, c)) continue;      // c always: a pointer chosen at run time would put the array in memory
      if (count == 0) {
        acc[0] = p[0]; acc[1] = p[1]; acc[2] = p[2];
        col[0] = c[0]; col[1] = c[1]; col[2] = c[2];
      } else {
        acc[0] = acc[0] + p[0]; acc[1] = acc[1] + p[1]; acc[2] = acc[2] + p[2];
        col[0] = col[0] + c[0]; col[1] = col[1] + c[1]; col[2] = col[2] + c[2];
      }
      ++count;
    }
    const float cnt = (float)count;                      // >= 1: a cube whose corners differ in sign has an edge whose ends do
    xyz[0] = acc[0] / cnt; xyz[1] = acc[1] / cnt; xyz[2] = acc[2] / cnt;
    if (with_rgb) {
      rgb[0] = col[0] / cnt; rgb[1] = col[1] / cnt; rgb[2] = col[2] / cnt;
    }
  }
  if (normal) {
    // edge k of an axis runs from corner lo to corner lo + the axis' bit; lo moves by the lower, then the higher other axis
    const float g0 = (((d[1] - d[0]) + (d[3] - d[2])) + (d[5] - d[4])) + (d[7] - d[6]);
    const float g1 = (((d[2] - d[0]) + (d[3] - d[1])) + (d[6] - d[4])) + (d[7] - d[5]);
    const float g2 = (((d[4] - d[0]) + (d[5] - d[1])) + (d[6] - d[2])) + (d[7] - d[3]);
    const float len = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
    const bool good = len > 0.0f && len <= FLT_MAX;
    normal[0] = good ? g0 / len : 0.0f;
    normal[1] = good ? g1 / len : 0.0f;
    normal[2] = good ? g2 / len : 0.0f;
  }
  return true;
}

// Slot s = 3 * voxel + axis of volume b, s < 3 * n: true when the slot is live (ud_tsdf_slot) and, with (u, v) = ((axis + 1) % 3,
// (axis + 2) % 3) and c the slot's voxel, the four cells q0 = c - e_u - e_v, q1 = c - e_v, q2 = c, q3 = c - e_u exist and are live.
// cell_live(voxel index) answers for a cell of volume b; it is asked only for indices inside the grid, and a cell that does not exist is
// never live.  q (may be null): the four cells in winding order, (q0, q1, q2, q3) when the slot's own voxel is negative and
// (q0, q3, q2, q1) otherwise, so the quad's geometric normal points to the positive side.
template <class CellLive>
UD_RM_FN bool ud_tsdf_quad(const UdTsdfSlotArgs& a, int b, long long s, CellLive cell_live, int* q) {
  if (!ud_tsdf_slot(a, b, s, nullptr, nullptr)) return false;
  const long long i = s / 3;
  const int axis = (int)(s - i * 3);
  const int row = (int)(i / a.Nx), ix = (int)(i - (long long)row * a.Nx), iz = row / a.Ny, iy = row - iz * a.Ny;
  const int u = axis == 2 ? 0 : axis + 1, v = axis == 0 ? 2 : axis - 1;
  const int cu = u == 0 ? ix : (u == 1 ? iy : iz), cv = v == 0 ? ix : (v == 1 ? iy : iz);
  if (cu < 1 || cv < 1) return false;
  const long long sxy = (long long)a.Nx * a.Ny;
  const long long eu = u == 0 ? 1 : (u == 1 ? (long long)a.Nx : sxy), ev = v == 0 ? 1 : (v == 1 ? (long long)a.Nx : sxy);
  const long long q0 = i - eu - ev, q1 = i - ev, q2 = i, q3 = i - eu;
  if (!(cell_live(q0) && cell_live(q1) && cell_live(q2) && cell_live(q3))) return false;
  if (q) {
    const bool neg = a.tsdf[(size_t)b * (size_t)a.n + (size_t)i] < 0.0f;
    q[0] = (int)q0; q[1] = (int)(neg ? q1 : q3); q[2] = (int)q2; q[3] = (int)(neg ? q3 : q1);
  }
  return true;
}
