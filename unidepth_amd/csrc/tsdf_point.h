// Per-voxel arithmetic of the truncated signed distance (TSDF) volume (include/unidepth_hip.h, UdTsdfIntegrate / UdTsdfPoints): what one
// thread of tsdf.hip's integration kernel does for voxel i of volume b -- the voxel's centre moved into every view and projected, the
// view's depth read at the nearest pixel, the truncated signed distance averaged into the running state, the views in order -- and the
// predicate and payload of the surface extraction, one slot per voxel and axis.  Plain functions with no device intrinsics and no kernel:
// they compose the per-point functions of camera_models.h and remap_taps.h and change none of them, so every output has the bits of
// project_camera -> remap(mode="nearest") and the element-wise arithmetic run one after the other.  tsdf.hip compiles them into its
// kernels; tests/tsdf_host/tsdf_host.cpp compiles the same header for the host, under the sanitizers.
//
// SAFETY RULE: remap_taps.h's, unchanged -- no float becomes an index before its clamp.  The only indices formed here are the voxel's own
// (i < n, checked by the caller), its +x / +y / +z neighbour's (checked against the grid), the view's (v < V) and the tap offset
// ud_rm_taps returned.  Every operation rounds separately (-ffp-contract=off).
#pragma once
#include <float.h>
#include "camera_models.h"
#include "remap_taps.h"
#pragma clang fp contract(off)

// src_depth / src_mask (optional) / src_weight (optional) [B,V,Hs,Ws]; image (optional) uint8 [B,V,3,Hs,Ws]; params [V,B,16]; T [nT,V,3,4]
// with nT = 1 or B: volume (world) to view-camera coordinates; origin [nO,3] with nO = 1 or B.  tsdf / weight [B,n], color (optional)
// [B,3,n], count (optional) [B,n], n = Nx * Ny * Nz with x fastest.
struct UdTsdfArgs {
  const float* src_depth; const unsigned char* src_mask; const float* src_weight; const unsigned char* image;
  const float* params; const float* T; const float* origin;
  float* tsdf; float* weight; float* color; unsigned char* count;
  long long n;
  float vs, trunc, max_weight;                         // max_weight is read only with has_max
  int B, V, Nx, Ny, Nz, Hs, Ws, nT, nO, fresh, has_max;
};

// the centre of voxel (ix, iy, iz) of a grid whose corner is o: o + ((float)index + 0.5f) * vs per axis
UD_RM_FN void ud_tsdf_centre(const float* o, float vs, int ix, int iy, int iz, float* p) {
  p[0] = o[0] + ((float)ix + 0.5f) * vs;
  p[1] = o[1] + ((float)iy + 0.5f) * vs;
  p[2] = o[2] + ((float)iz + 0.5f) * vs;
}

// model[v * B + b]: any of the six models (projection is closed form for all of them)
UD_RM_FN void ud_tsdf_voxel(const UdTsdfArgs& a, const unsigned char* model, int b, long long i) {
  const size_t n = (size_t)a.n, at = (size_t)b * n + (size_t)i, hw = (size_t)a.Hs * (size_t)a.Ws;
  const int row = (int)(i / a.Nx), ix = (int)(i - (long long)row * a.Nx), iz = row / a.Ny, iy = row - iz * a.Ny;
  float p[3];
  ud_tsdf_centre(a.origin + (a.nO == 1 ? 0 : (size_t)b * 3), a.vs, ix, iy, iz, p);
  // a. the running state: a fresh volume starts empty and its memory is not read
  float tsdf = 1.0f, W = 0.0f, c[3] = {0.0f, 0.0f, 0.0f};
  if (!a.fresh) {
    tsdf = a.tsdf[at];
    W = a.weight[at];
    if (a.color)
      for (int k = 0; k < 3; ++k) c[k] = a.color[((size_t)b * 3 + (size_t)k) * n + (size_t)i];
  }
  int cnt = 0;
  // b. the views, in order
  for (int v = 0; v < a.V; ++v) {
    const size_t tv = (size_t)(a.nT == 1 ? 0 : b) * (size_t)a.V + (size_t)v, bv = (size_t)b * (size_t)a.V + (size_t)v;
    const int m = model[v * a.B + b];
    const float* ps = a.params + ((size_t)v * (size_t)a.B + (size_t)b) * 16;
    float x = p[0], y = p[1], z = p[2];
    ud_cam_move(a.T + tv * 12, x, y, z);
    float u, w;
    ud_cam_project(m, ps, x, y, z, &u, &w);
    const float d = ud_cam_depth(m, x, y, z);
    const bool inside = ud_cam_inside(m, u, w, z, a.Hs, a.Ws);
    // one nearest tap, zeros padding; it contributes when the view's depth there is > 0 and its mask is not 0
    UdRmTaps t;
    ud_rm_taps(u, w, a.Ws, a.Hs, UD_RM_NEAREST, UD_RM_ZEROS, &t);
    const int off = t.off[0];
    float ds = 0.0f;
    bool tap = false;
    if (off >= 0) {
      ds = a.src_depth[bv * hw + (size_t)off];
      tap = ds > 0.0f && (!a.src_mask || a.src_mask[bv * hw + (size_t)off] != 0);
    }
    const bool valid = inside && ud_rm_finite(u, w) && ud_rm_inside(u, w, a.Ws, a.Hs) && tap;
    float wv = 1.0f, rgb[3] = {0.0f, 0.0f, 0.0f};
    if (valid) {
      if (a.src_weight) wv = a.src_weight[bv * hw + (size_t)off];
      if (a.image)
        for (int k = 0; k < 3; ++k) rgb[k] = (float)a.image[(bv * 3 + (size_t)k) * hw + (size_t)off];
    }
    const float sdf = ds - d;
    const bool obs = valid && d > 0.0f && sdf >= -a.trunc && wv > 0.0f && wv <= FLT_MAX;      // false whenever a NaN is involved
    const float s = fminf(sdf / a.trunc, 1.0f);
    if (obs) {
      const float Wn = W + wv;
      tsdf = (tsdf * W + s * wv) / Wn;
      if (a.color)
        for (int k = 0; k < 3; ++k) c[k] = (c[k] * W + rgb[k] * wv) / Wn;
      W = a.has_max ? fminf(Wn, a.max_weight) : Wn;
      ++cnt;
    }
  }
  // c. the outputs, written once
  a.tsdf[at] = tsdf;
  a.weight[at] = W;
  if (a.color)
    for (int k = 0; k < 3; ++k) a.color[((size_t)b * 3 + (size_t)k) * n + (size_t)i] = c[k];
  if (a.count) a.count[at] = (unsigned char)cnt;
}

// tsdf / weight [B,n], color (optional) [B,3,n], origin [nO,3]
struct UdTsdfSlotArgs {
  const float* tsdf; const float* weight; const float* color; const float* origin;
  long long n;
  float vs, min_weight;
  int B, Nx, Ny, Nz, nO;
};

// Slot s = 3 * voxel + axis of volume b, s < 3 * n: the edge from the voxel to its +x / +y / +z neighbour.  Live when the neighbour lies
// in the grid, both weights are >= min_weight, neither distance is a NaN and exactly one of them is negative.  For a live slot with xyz
// given: t = a / (a - b), the point is the voxel's centre moved by t * vs along the axis, and rgb (with a colour volume; may be null) the
// colours blended c0 + t * (c1 - c0), not yet rounded.
UD_RM_FN bool ud_tsdf_slot(const UdTsdfSlotArgs& a, int b, long long s, float* xyz, float* rgb) {
  const size_t n = (size_t)a.n;
  const long long i = s / 3;
  const int axis = (int)(s - i * 3);
  const int row = (int)(i / a.Nx), ix = (int)(i - (long long)row * a.Nx), iz = row / a.Ny, iy = row - iz * a.Ny;
  const bool in_grid = axis == 0 ? ix + 1 < a.Nx : (axis == 1 ? iy + 1 < a.Ny : iz + 1 < a.Nz);
  if (!in_grid) return false;
  const size_t i0 = (size_t)b * n + (size_t)i;
  const size_t i1 = i0 + (axis == 0 ? (size_t)1 : (axis == 1 ? (size_t)a.Nx : (size_t)a.Nx * (size_t)a.Ny));
  if (!(a.weight[i0] >= a.min_weight && a.weight[i1] >= a.min_weight)) return false;
  const float d0 = a.tsdf[i0], d1 = a.tsdf[i1];
  if (d0 != d0 || d1 != d1 || (d0 < 0.0f) == (d1 < 0.0f)) return false;
  if (xyz) {
    const float t = d0 / (d0 - d1);
    ud_tsdf_centre(a.origin + (a.nO == 1 ? 0 : (size_t)b * 3), a.vs, ix, iy, iz, xyz);
    const float move = t * a.vs;                         // written per axis: an index that varies by lane would take the array out of registers
    if (axis == 0) xyz[0] = xyz[0] + move;
    else if (axis == 1) xyz[1] = xyz[1] + move;
    else xyz[2] = xyz[2] + move;
    if (rgb && a.color)
      for (int k = 0; k < 3; ++k) {
        const size_t ck = ((size_t)b * 3 + (size_t)k) * n + (size_t)i, step = i1 - i0;
        const float c0 = a.color[ck], c1 = a.color[ck + step];
        rgb[k] = c0 + t * (c1 - c0);
      }
  }
  return true;
}
