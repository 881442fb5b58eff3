// The per-pair arithmetic of the K = 1, D <= 3 nearest-neighbour searches, shared by ud_knn_points (evalops.hip) and ud_eval_3d
// (eval3d.hip) so that both produce the same bits: two queries per lane in packed fp32, (dx*dx + dy*dy) + dz*dz with every multiply
// and add rounded separately.  Files that include this are built with -ffp-contract=off (csrc/build.sh): the in-source pragma does
// not reach ext_vector_type arithmetic.
#pragma once
#include "ud_common.h"

constexpr int KNN_TILE = 1024;         // p2 points staged in LDS per tile, one f32x4 each
constexpr int KNN1_CHUNK = 8;          // points per running-minimum chunk; a tile is padded to a multiple with +inf points

__device__ __forceinline__ f32x2 knn1_dist(const f32x2 qx, const f32x2 qy, const f32x2 qz, const f32x4 v, const bool l2) {
  const f32x2 dx = qx - (f32x2){v[0], v[0]}, dy = qy - (f32x2){v[1], v[1]}, dz = qz - (f32x2){v[2], v[2]};
  if (l2) return (dx * dx + dy * dy) + dz * dz;
  return ((f32x2){fabsf(dx[0]), fabsf(dx[1])} + (f32x2){fabsf(dy[0]), fabsf(dy[1])}) + (f32x2){fabsf(dz[0]), fabsf(dz[1])};
}
