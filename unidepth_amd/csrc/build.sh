#!/bin/bash
# Build libunidepth_hip.so for gfx950 in-tree (cross-compiles without a GPU).  Usage: csrc/build.sh [extra hipcc flags]
# UD_OUT / UD_BUILD_DIR override the output library / object directory (A/B and instrumented builds, tools/).
set -e
cd "$(dirname "$0")"
OUT=${UD_OUT:-../libunidepth_hip.so}
BD=${UD_BUILD_DIR:-build}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast -Wno-unused-result"
mkdir -p $BD
pids=()
for f in gemm.hip gemm_pp.hip calib.hip layernorm.hip pointwise.hip camera_f32.hip convnext.hip v1dec.hip; do
  ( hipcc $FLAGS "$@" -c $f -o $BD/${f%.hip}.o ) &
  pids+=($!)
done
# attention: keep the MFMA accumulators in VGPRs (the softmax VALU works on them every tile; the default AGPR form costs
# ~160 v_accvgpr_read/write per 16 MFMAs); no SLP vectorisation: packed f32 adds (v_pk_add_f32) next to MFMAs are slower than
# the scalar adds they replace (half-rate issue, /opt/skills/guides MI355X_MICROARCH "price of one filler beside MFMAs")
( hipcc $FLAGS -mllvm -amdgpu-mfma-vgpr-form=1 -fno-slp-vectorize "$@" -c attention.hip -o $BD/attention.o ) & pids+=($!)
# evaluation-side kernels: bit-exact fp32 distances (separately rounded multiply and add, like the reference's CPU build), so no FMA
# contraction anywhere in this file (the in-source pragma does not reach ext_vector_type arithmetic)
( hipcc $FLAGS -ffp-contract=off "$@" -c evalops.hip -o $BD/evalops.o ) & pids+=($!)
# 2-D depth metrics: the resample weights, ratios and rescales must round every operation separately (threshold counts), same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c evaldepth.hip -o $BD/evaldepth.o ) & pids+=($!)
# point-cloud compaction: the filter predicate and the unprojection round every operation separately (a numpy fp32 restatement
# reproduces the predicate exactly), same rule.  compact.h, which this file, tsdf.hip and eval3d.hip include, is integer code only
( hipcc $FLAGS -ffp-contract=off "$@" -c pointcloud.hip -o $BD/pointcloud.o ) & pids+=($!)
# match_gt: the resample of ud_eval_depth applied to per-image windows; bit-exact against its numpy fp32 restatement, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c matchgt.hip -o $BD/matchgt.o ) & pids+=($!)
# colorize: (v - lo) / den * 256 picks a LUT bin and |g - p| / g feeds it; byte-exact against its numpy fp32 restatement, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c colorize.hip -o $BD/colorize.o ) & pids+=($!)
# splat: the cell a point lands in (transform, projection, division, floor) must be the one a numpy fp32 restatement computes, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c splat.hip -o $BD/splat.o ) & pids+=($!)
# testprep: the antialiased resize's weights, both passes, the rounding to a byte and the normalisation are defined operation by
# operation in fp32; bit-exact against its numpy fp32 restatement, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c testprep.hip -o $BD/testprep.o ) & pids+=($!)
# eval_3d: |gt - pred| and the nearest-neighbour distances (knn_dist.h, shared with evalops.hip) round every multiply and add
# separately, so the distances are bit-equal to ud_knn_points' and a numpy fp32 restatement reproduces the threshold counts, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c eval3d.hip -o $BD/eval3d.o ) & pids+=($!)
# reconstruct: the ground-truth point maps are defined operation by operation in fp32 (camera_models.h under this flag is what the numpy
# fp32 restatement and the host build of the tests compute), same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c reconstruct.hip -o $BD/reconstruct.o ) & pids+=($!)
# project: the image coordinates of a point are defined operation by operation in fp32 (the forward models of camera_models.h under this
# flag are what the numpy fp32 restatement and the host build of the tests compute), same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c project.hip -o $BD/project.o ) & pids+=($!)
# unproject: the inverse models of camera_models.h at arbitrary coordinates; the identity grid with a depth must give reconstruct's bits, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c unproject.hip -o $BD/unproject.o ) & pids+=($!)
# remap: tap weights, the blend, the rounding to a byte and the overlap-mask decision are defined operation by operation in fp32 (remap_taps.h
# under this flag is what the numpy fp32 restatement and the host build of the tests compute), same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c remap.hip -o $BD/remap.o ) & pids+=($!)
# warp: unproject, project and remap fused per pixel (warp_point.h calls camera_models.h and remap_taps.h); each output must have the bits
# of those launches run one after the other, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c warp.hip -o $BD/warp.o ) & pids+=($!)
# normals: the differences, the cross product, both normalisations, the orientation test and the byte rounding are defined operation by
# operation in fp32 (normals_point.h under this flag is what the numpy fp32 restatement and the host build of the tests compute); the
# depth form must have the bits of ud_reconstruct followed by the points form; the metric's cosine feeds exact threshold counts, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c normals.hip -o $BD/normals.o ) & pids+=($!)
# consistency: warp, unproject, project and the comparisons of the forward-backward depth check fused per pixel over all views
# (consistency_point.h calls camera_models.h and remap_taps.h); each output must have the bits of those launches run one after the other,
# same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c consistency.hip -o $BD/consistency.o ) & pids+=($!)
# tsdf: project, the nearest-pixel remap and the running weighted mean fused per voxel over all views (tsdf_point.h calls camera_models.h
# and remap_taps.h); the volume must have the bits of those launches run one after the other, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c tsdf.hip -o $BD/tsdf.o ) & pids+=($!)
# tsdf_render: the march, the trilinear reads, the crossing, the gradient and the colour of a ray are defined operation by operation in fp32
# (tsdf_ray.h under this flag is what the numpy fp32 restatement and the host build of the tests compute), same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c tsdf_render.hip -o $BD/tsdf_render.o ) & pids+=($!)
# tsdf_mesh: a vertex is the mean of its cell's crossings (tsdf_mesh_point.h calls tsdf_point.h's ud_tsdf_slot), summed in a fixed order,
# and must have the bits of the numpy fp32 restatement and of the host build of the tests, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c tsdf_mesh.hip -o $BD/tsdf_mesh.o ) & pids+=($!)
# icp: unproject, project, the nearest-pixel remap, the residual and the row fused per pixel (icp_point.h calls camera_models.h and
# remap_taps.h), each per-pixel output with the bits of those launches run one after the other; the fp64 sums and the LDL^T / Cayley solve
# round every operation once, so the numpy fp64 restatement and the host build of the tests have the solve's bits, same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c icp.hip -o $BD/icp.o ) & pids+=($!)
# pyramid: the bilateral filter's taps (difference, bin, weight, the two running sums, the division) and the gated 2 x 2 means are defined
# operation by operation in fp32 in a fixed tap order (pyramid_point.h under this flag is what the numpy fp32 restatement and the host build
# of the tests compute), same rule
( hipcc $FLAGS -ffp-contract=off "$@" -c pyramid.hip -o $BD/pyramid.o ) & pids+=($!)
( hipcc $FLAGS -x hip -c api.cpp -o $BD/api.o ) & pids+=($!)
( hipcc $FLAGS -x hip -c program.cpp -o $BD/program.o ) & pids+=($!)
( hipcc $FLAGS -x hip -c rccl.cpp -o $BD/rccl.o ) & pids+=($!)
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC $BD/*.o -ldl -o $OUT
echo "built $(realpath $OUT)"
