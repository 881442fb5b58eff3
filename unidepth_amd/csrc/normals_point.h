// Per-pixel arithmetic of the surface normals (include/unidepth_hip.h, UdNormals) and of the normal metrics (UdEvalNormals): what one
// thread of normals.hip's kernels does for a pixel.  Plain functions with no device intrinsics and no kernel, so that
// tests/normals_host/normals_host.cpp compiles the same header for the host, under the sanitizers.  The points of the depth form come from
// camera_models.h's reconstruct (ud_cam_unproject_closed), which is unchanged.
//
// THE DEFINITION (every operation below is one separately rounded fp32 operation, in the order written; -ffp-contract=off):
//   ok[q]     = mask[q] != 0 && P[q].x, .y, .z all finite                    (depth form: && depth[q] > 0)
//   d[q]      = depth[q] when a depth is given, else P[q].z
//   usable(q) = q inside the image && ok[q] && (no edge_rtol || |d[c] - d[q]| <= edge_rtol * min(d[c], d[q]))     false for a NaN
//   dx        = P[R] - P[L] (both usable) | P[R] - P[c] (right only) | P[c] - P[L] (left only) | none: invalid;  dy likewise with D, U
//   n         = cross(dy, dx);  m = max(max(|nx|, |ny|), |nz|), valid only if m > 0 and finite;  n = n / m;
//   l         = sqrt((nx*nx + ny*ny) + nz*nz);  n = n / l;  s = (nx*P.x + ny*P.y) + nz*P.z at c;  s > 0: n = -n
//   rgb       = clamp(floor((n + 1) * 127.5 + 0.5), 0, 255); normals and rgb are exactly 0 where not valid.
//
// SAFETY RULE: the only indices formed are y * W + x with 0 <= x < W, 0 <= y < H checked before the load.
#pragma once
#include "camera_models.h"
#pragma clang fp contract(off)

#define UD_NM_FN UD_CAM_FN

UD_NM_FN bool ud_nm_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }                 // false for NaN and +-inf
UD_NM_FN bool ud_nm_finite3(float x, float y, float z) { return ud_nm_finite(x) && ud_nm_finite(y) && ud_nm_finite(z); }

// the depth-edge test between the centre and a neighbour: false when either depth is a NaN
UD_NM_FN bool ud_nm_edge_ok(float dc, float dq, float rtol) {
  const float lo = dq < dc ? dq : dc;
  return fabsf(dc - dq) <= rtol * lo;
}

UD_NM_FN unsigned char ud_nm_byte(float n) {
  const float q = (n + 1.0f) * 127.5f;
  float f = floorf(q + 0.5f);
  f = f < 0.0f ? 0.0f : (f > 255.0f ? 255.0f : f);
  return (unsigned char)f;
}

// The normal of a pixel from its own point c and its usable neighbours (l, r, u, d are read only where their flag is set).
// n = 0 and false where the pixel is not valid.
UD_NM_FN bool ud_nm_normal(const float* c, const float* l, const float* r, const float* u, const float* d, bool okc, bool ul, bool ur,
                           bool uu, bool ud, float* n) {
  n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
  if (!okc || !(ul || ur) || !(uu || ud)) return false;
  const float* xa = ur ? r : c;
  const float* xb = ul ? l : c;
  const float* ya = ud ? d : c;
  const float* yb = uu ? u : c;
  const float dxx = xa[0] - xb[0], dxy = xa[1] - xb[1], dxz = xa[2] - xb[2];
  const float dyx = ya[0] - yb[0], dyy = ya[1] - yb[1], dyz = ya[2] - yb[2];
  float nx = dyy * dxz - dyz * dxy;
  float ny = dyz * dxx - dyx * dxz;
  float nz = dyx * dxy - dyy * dxx;
  const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
  if (!ud_nm_finite3(nx, ny, nz)) return false;       // the maximum lets a NaN through (numpy's maximum): m is finite iff all three are
  float m = ax > ay ? ax : ay;
  m = m > az ? m : az;
  if (!(m > 0.0f)) return false;
  nx = nx / m; ny = ny / m; nz = nz / m;
  const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
  nx = nx / len; ny = ny / len; nz = nz / len;
  const float s = (nx * c[0] + ny * c[1]) + nz * c[2];
  if (s > 0.0f) {
    nx = -nx; ny = -ny; nz = -nz;
  }
  n[0] = nx; n[1] = ny; n[2] = nz;
  return true;
}

// Strides in elements.  points planar [B,3,n], depth [B,n] (optional: P.z otherwise), mask [B or 1 (mask_bs == 0), n] (optional),
// normals planar [B,3,n], valid [B,n] (optional), rgb planar [B,3,n] (optional); n = H * W.
struct UdNmArgs {
  const float* points; const float* depth; const unsigned char* mask;
  float* normals; unsigned char* valid; unsigned char* rgb;
  long long mask_bs;
  float rtol;
  int H, W, has_rtol;
};

UD_NM_FN void ud_nm_store(const UdNmArgs& a, int b, size_t i, bool valid, const float* n) {
  const size_t hw = (size_t)a.H * (size_t)a.W;
  float* o = a.normals + (size_t)b * 3 * hw + i;
  o[0] = n[0]; o[hw] = n[1]; o[2 * hw] = n[2];
  if (a.valid) a.valid[(size_t)b * hw + i] = valid ? 1 : 0;
  if (a.rgb) {
    unsigned char* q = a.rgb + (size_t)b * 3 * hw + i;
    q[0] = valid ? ud_nm_byte(n[0]) : 0; q[hw] = valid ? ud_nm_byte(n[1]) : 0; q[2 * hw] = valid ? ud_nm_byte(n[2]) : 0;
  }
}

// ok[q], P[q] and d[q] of pixel (y, x) of image b in the points form; false (and nothing loaded) outside the image
UD_NM_FN bool ud_nm_fetch(const UdNmArgs& a, int b, int y, int x, float* p, float* d) {
  if (x < 0 || x >= a.W || y < 0 || y >= a.H) return false;
  const size_t hw = (size_t)a.H * (size_t)a.W, i = (size_t)y * (size_t)a.W + (size_t)x;
  const float* s = a.points + (size_t)b * 3 * hw + i;
  p[0] = s[0]; p[1] = s[hw]; p[2] = s[2 * hw];
  *d = a.depth ? a.depth[(size_t)b * hw + i] : p[2];
  const bool m = a.mask ? a.mask[(size_t)b * (size_t)a.mask_bs + i] != 0 : true;
  return m && ud_nm_finite3(p[0], p[1], p[2]);
}

// the points form: pixel (y, x) of image b, 0 <= x < W, 0 <= y < H
UD_NM_FN void ud_nm_pixel(const UdNmArgs& a, int b, int y, int x) {
  float c[3], l[3], r[3], u[3], d[3], dc = 0.0f, dl = 0.0f, dr = 0.0f, du = 0.0f, dd = 0.0f, n[3];
  const bool okc = ud_nm_fetch(a, b, y, x, c, &dc);
  bool ul = ud_nm_fetch(a, b, y, x - 1, l, &dl), ur = ud_nm_fetch(a, b, y, x + 1, r, &dr);
  bool uu = ud_nm_fetch(a, b, y - 1, x, u, &du), ud = ud_nm_fetch(a, b, y + 1, x, d, &dd);
  if (a.has_rtol) {
    ul = ul && ud_nm_edge_ok(dc, dl, a.rtol); ur = ur && ud_nm_edge_ok(dc, dr, a.rtol);
    uu = uu && ud_nm_edge_ok(dc, du, a.rtol); ud = ud && ud_nm_edge_ok(dc, dd, a.rtol);
  }
  const bool valid = ud_nm_normal(c, l, r, u, d, okc, ul, ur, uu, ud, n);
  ud_nm_store(a, b, (size_t)y * (size_t)a.W + (size_t)x, valid, n);
}

// the point of pixel (y, x) in the depth form and its ok flag: a closed-form model's reconstruct at the pixel centre
UD_NM_FN bool ud_nm_depth_point(int model, const float* params, const unsigned char* mask_b, const float* depth_b, int W, int y, int x,
                                float* p, float* d) {
  const size_t i = (size_t)y * (size_t)W + (size_t)x;
  *d = depth_b[i];
  ud_cam_unproject_closed(model, UD_UNPROJ_DEPTH, params, (float)x + 0.5f, (float)y + 0.5f, *d, p);
  const bool m = mask_b ? mask_b[i] != 0 : true;
  return m && *d > 0.0f && ud_nm_finite3(p[0], p[1], p[2]);
}

// ---- the normal metrics: the cosine of the angle between two normals; false where the pixel is dropped ---------------------------------
//   lg = sqrt((gx*gx + gy*gy) + gz*gz), lp likewise; dropped unless all six values are finite and both lengths are > 0 and finite;
//   c = ((gx*px + gy*py) + gz*pz) / (lg * lp), clamped to [-1, 1]; a NaN quotient (an overflow of both the dot and the product) is dropped
UD_NM_FN bool ud_nm_cos(float gx, float gy, float gz, float px, float py, float pz, float* c) {
  if (!ud_nm_finite3(gx, gy, gz) || !ud_nm_finite3(px, py, pz)) return false;
  const float lg = sqrtf((gx * gx + gy * gy) + gz * gz), lp = sqrtf((px * px + py * py) + pz * pz);
  if (!(lg > 0.0f) || !(lp > 0.0f) || !ud_nm_finite(lg) || !ud_nm_finite(lp)) return false;
  float v = ((gx * px + gy * py) + gz * pz) / (lg * lp);
  if (v != v) return false;
  v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
  *c = v;
  return true;
}
