// Per-ray arithmetic of the TSDF ray cast (include/unidepth_hip.h, UdTsdfRender): what one thread of tsdf_render.hip's kernel does for
// pixel (py, px) of image b -- the pixel's direction, a march of K samples t_k = near + k * step through the volume with a trilinear read
// of the distance at each, the first front crossing, and there the depth, the point, the normal from the analytic gradient of the
// interpolant and the colour.  Plain functions with no device intrinsics and no kernel: they call camera_models.h (unprojection, the rigid
// motion, the model's depth) and remap_taps.h (the byte rounding) and change neither.  tsdf_render.hip compiles them into its kernel;
// tests/tsdf_render_host/tsdf_render_host.cpp compiles the same header for the host, under the sanitizers.
//
// THE DEFINITION (every operation one separately rounded fp32 operation, in the order written; -ffp-contract=off):
//   d          the three values of `rays` as they are, or ud_cam_unproject_closed(model, NORMALIZE, params, px + 0.5, py + 0.5)
//   sample k   t = near + (float)k * step;  q = (t dx, t dy, t dz);  p = ud_cam_move(T, q) (q itself without T);
//              g_a = (p_a - o_a) / vs - 0.5 per axis.  IN THE GRID when 0 <= g_a <= (float)(N_a - 1) on every axis (false for a NaN);
//              then i_a = max(min((int)floorf(g_a), N_a - 2), 0), the upper corner min(i_a + 1, N_a - 1), f_a = g_a - (float)i_a.
//              VALID when in the grid, all eight corner weights >= min_weight and the value s is not a NaN;
//              s = lerp along x (four times), then y (twice), then z, lerp(a, b, f) = a + f * (b - a).
//   scan       k = 0 .. K-1 in order; with the previous and the current sample both valid: !(s_prev < 0) && s < 0 is the HIT (stop);
//              s_prev < 0 && !(s < 0) stops without a hit (the surface seen from behind).  An invalid sample resets "previous valid".
//   hit        al = s_prev / (s_prev - s);  t* = t_(k-1) + al * (t_k - t_(k-1));  q* = t* d;  depth = ud_cam_depth(model, q*).
//              The pixel is valid when it hit and depth > 0; otherwise every output of the pixel is exactly 0.
//   gradient   at both samples, of the same eight corners: gx = the four x-differences lerped along y then z, gy the y-differences along
//              x then z, gz the z-differences along x then y (not divided by vs);  G = g_prev + al * (g - g_prev);
//              n = T's rotation transposed times G (G itself without T), divided by its largest magnitude, then by its length (as
//              normals_point.h); negated when n . q* > 0.  Not finite or zero: exactly 0, the pixel stays valid.
//   colour     the trilinear colour at both samples, c_prev + al * (c - c_prev); a byte through ud_rm_to_u8, or fp32.
//
// THE CLIP: ud_tsdf_ray_clip may shorten k = 0 .. K-1 to the samples that can lie in the grid.  The result is DEFINED by the full scan
// (args.full_scan); the clip only skips samples that fail the exact in-grid test, which starts and ends the scan in the state "previous
// not valid" either way.  It is conservative: the box is widened, an axis along which the direction is 0, infinite or NaN (or whose
// bounds are not finite) constrains nothing, and the sample numbers are clamped as floats before they become integers.
//
// SAFETY RULE: remap_taps.h's -- no float becomes an index before its clamp.  A voxel index is formed only after the in-grid test.
#pragma once
#include "camera_models.h"
#include "remap_taps.h"
#pragma clang fp contract(off)

// tsdf / weight [B,n], color (optional) [B,3,n], n = Nx * Ny * Nz with x fastest; origin [nO,3]; T (optional) [nT,3,4]: camera to volume;
// params [B,16] (read without rays); rays (optional) planar [B,3,hw], hw = Ho * Wo.  Outputs: depth [B,hw], valid [B,hw] bytes, and
// optional points / normals planar [B,3,hw], color_out planar [B,3,hw] bytes or fp32 (color_f32).
struct UdTsdfRayArgs {
  const float* tsdf; const float* weight; const float* color; const float* origin; const float* T; const float* params; const float* rays;
  float* depth; unsigned char* valid; float* points; float* normals; void* color_out;
  long long n;
  float vs, near, step, min_weight;
  int B, Ho, Wo, Nx, Ny, Nz, nT, nO, K, color_f32, full_scan;
};

// the cell of a sample: the offset of its lower corner in one volume, the steps to the upper corners (0 along an axis of one voxel) and
// the fractions
struct UdTsdfCell {
  size_t at, sx, sy, sz;
  float fx, fy, fz;
};

UD_RM_FN float ud_tsdf_lerp(float a, float b, float f) { return a + f * (b - a); }

UD_RM_FN int ud_tsdf_lower(float g, int N) {
  int i = (int)floorf(g);                              // 0 <= g <= N - 1 was tested: the conversion is defined
  i = i < N - 2 ? i : N - 2;
  return i > 0 ? i : 0;
}

// the sample at t along d: false (and no index formed) unless it lies in the grid
UD_RM_FN bool ud_tsdf_ray_cell(const UdTsdfRayArgs& a, const float* T, const float* o, const float* d, float t, UdTsdfCell* c) {
  float x = t * d[0], y = t * d[1], z = t * d[2];
  if (T) ud_cam_move(T, x, y, z);
  const float gx = (x - o[0]) / a.vs - 0.5f, gy = (y - o[1]) / a.vs - 0.5f, gz = (z - o[2]) / a.vs - 0.5f;
  const bool in = gx >= 0.0f && gx <= (float)(a.Nx - 1) && gy >= 0.0f && gy <= (float)(a.Ny - 1) && gz >= 0.0f && gz <= (float)(a.Nz - 1);
  if (!in) return false;
  const int ix = ud_tsdf_lower(gx, a.Nx), iy = ud_tsdf_lower(gy, a.Ny), iz = ud_tsdf_lower(gz, a.Nz);
  c->fx = gx - (float)ix; c->fy = gy - (float)iy; c->fz = gz - (float)iz;
  c->at = ((size_t)iz * (size_t)a.Ny + (size_t)iy) * (size_t)a.Nx + (size_t)ix;
  c->sx = ix + 1 < a.Nx ? 1 : 0;
  c->sy = iy + 1 < a.Ny ? (size_t)a.Nx : 0;
  c->sz = iz + 1 < a.Nz ? (size_t)a.Nx * (size_t)a.Ny : 0;
  return true;
}

// the eight corners of a cell of one volume, v[4 * z + 2 * y + x]
UD_RM_FN void ud_tsdf_corners(const float* vol, const UdTsdfCell& c, float* v) {
  const float* p = vol + c.at;
  v[0] = p[0]; v[1] = p[c.sx]; v[2] = p[c.sy]; v[3] = p[c.sy + c.sx];
  v[4] = p[c.sz]; v[5] = p[c.sz + c.sx]; v[6] = p[c.sz + c.sy]; v[7] = p[c.sz + c.sy + c.sx];
}

// along x four times, then y twice, then z
UD_RM_FN float ud_tsdf_trilinear(const float* v, const UdTsdfCell& c) {
  const float c00 = ud_tsdf_lerp(v[0], v[1], c.fx), c10 = ud_tsdf_lerp(v[2], v[3], c.fx);
  const float c01 = ud_tsdf_lerp(v[4], v[5], c.fx), c11 = ud_tsdf_lerp(v[6], v[7], c.fx);
  return ud_tsdf_lerp(ud_tsdf_lerp(c00, c10, c.fy), ud_tsdf_lerp(c01, c11, c.fy), c.fz);
}

// the gradient of the interpolant in voxel units: the differences along an axis, lerped along the two others
UD_RM_FN void ud_tsdf_gradient(const float* v, const UdTsdfCell& c, float* g) {
  g[0] = ud_tsdf_lerp(ud_tsdf_lerp(v[1] - v[0], v[3] - v[2], c.fy), ud_tsdf_lerp(v[5] - v[4], v[7] - v[6], c.fy), c.fz);
  g[1] = ud_tsdf_lerp(ud_tsdf_lerp(v[2] - v[0], v[3] - v[1], c.fx), ud_tsdf_lerp(v[6] - v[4], v[7] - v[5], c.fx), c.fz);
  g[2] = ud_tsdf_lerp(ud_tsdf_lerp(v[4] - v[0], v[5] - v[1], c.fx), ud_tsdf_lerp(v[6] - v[2], v[7] - v[3], c.fx), c.fy);
}

// the weights first, the distances only where the cell passes
UD_RM_FN bool ud_tsdf_cell_weights(const UdTsdfRayArgs& a, int b, const UdTsdfCell& c) {
  float w[8];
  ud_tsdf_corners(a.weight + (size_t)b * (size_t)a.n, c, w);
  bool ok = true;
  for (int k = 0; k < 8; ++k) ok = ok && w[k] >= a.min_weight;
  return ok;
}

// sample t of the scan: valid, and then *s its value
UD_RM_FN bool ud_tsdf_ray_sample(const UdTsdfRayArgs& a, int b, const float* T, const float* o, const float* d, float t, float* s) {
  UdTsdfCell c;
  *s = 0.0f;
  if (!ud_tsdf_ray_cell(a, T, o, d, t, &c) || !ud_tsdf_cell_weights(a, b, c)) return false;
  float v[8];
  ud_tsdf_corners(a.tsdf + (size_t)b * (size_t)a.n, c, v);
  *s = ud_tsdf_trilinear(v, c);
  return *s == *s;
}

// the gradient and (with rgb and a colour volume) the colour at a sample of the scan that was valid; zeros otherwise
UD_RM_FN void ud_tsdf_ray_detail(const UdTsdfRayArgs& a, int b, const float* T, const float* o, const float* d, float t, float* g, float* rgb) {
  UdTsdfCell c;
  g[0] = 0.0f; g[1] = 0.0f; g[2] = 0.0f;
  if (rgb) { rgb[0] = 0.0f; rgb[1] = 0.0f; rgb[2] = 0.0f; }
  if (!ud_tsdf_ray_cell(a, T, o, d, t, &c)) return;
  float v[8];
  ud_tsdf_corners(a.tsdf + (size_t)b * (size_t)a.n, c, v);
  ud_tsdf_gradient(v, c, g);
  if (rgb && a.color)
    for (int k = 0; k < 3; ++k) {
      ud_tsdf_corners(a.color + ((size_t)b * 3 + (size_t)k) * (size_t)a.n, c, v);
      rgb[k] = ud_tsdf_trilinear(v, c);
    }
}

UD_RM_FN bool ud_tsdf_usable(float x) { return fabsf(x) <= 3.402823466e38f; }           // false for a NaN and for +-inf

// The samples k0 .. k1 (k0 > k1: none) outside which every sample fails the in-grid test.  In exact arithmetic the sample at t lies at
// C + t * D in the volume's frame (D = R d, C = T's translation); along an axis it can pass only while lo - m <= C + t * D <= hi + m,
// [lo, hi] = o + [0.5, N - 0.5] * vs the centres of the outermost voxels and m a margin of 1e-4 of the magnitudes involved (about a
// thousand times the rounding of the operations of a sample) plus a voxel.  The interval of t is widened by 1e-4 of the largest t, and
// the sample numbers by two on either side.
UD_RM_FN void ud_tsdf_ray_clip(const UdTsdfRayArgs& a, const float* T, const float* o, const float* d, int* k0, int* k1) {
  const float Kf = (float)a.K, tmax = a.near + Kf * a.step;
  float D[3] = {d[0], d[1], d[2]}, C[3] = {0.0f, 0.0f, 0.0f};
  if (T) {
    D[0] = (T[0] * d[0] + T[1] * d[1]) + T[2] * d[2];
    D[1] = (T[4] * d[0] + T[5] * d[1]) + T[6] * d[2];
    D[2] = (T[8] * d[0] + T[9] * d[1]) + T[10] * d[2];
    C[0] = T[3]; C[1] = T[7]; C[2] = T[11];
  }
  const int N[3] = {a.Nx, a.Ny, a.Nz};
  float t_in = a.near, t_out = tmax;
  for (int k = 0; k < 3; ++k) {
    const float lo = o[k] + 0.5f * a.vs, hi = o[k] + ((float)N[k] - 0.5f) * a.vs;
    const float m = 1e-4f * (((fabsf(D[k]) * tmax + fabsf(C[k])) + fabsf(o[k])) + (float)N[k] * a.vs) + a.vs;
    const float ta = ((lo - m) - C[k]) / D[k], tb = ((hi + m) - C[k]) / D[k];
    // an axis constrains only when everything about it is finite and the ray moves along it; otherwise it keeps the full range
    if (!(D[k] != 0.0f) || !ud_tsdf_usable(D[k]) || !ud_tsdf_usable(ta) || !ud_tsdf_usable(tb)) continue;
    const float t0 = ta < tb ? ta : tb, t1 = ta < tb ? tb : ta;
    t_in = t0 > t_in ? t0 : t_in;
    t_out = t1 < t_out ? t1 : t_out;
  }
  const float w = 1e-4f * (fabsf(a.near) + fabsf(tmax));
  const float fa = ((t_in - w) - a.near) / a.step - 2.0f, fb = ((t_out + w) - a.near) / a.step + 2.0f;
  // clamped as floats: !(x > 0) and !(x < K - 1) also catch a NaN
  *k0 = !(fa > 0.0f) ? 0 : (fa >= Kf ? a.K : (int)fa);
  *k1 = !(fb < Kf - 1.0f) ? a.K - 1 : (fb < 0.0f ? -1 : (int)fb);
}

// pixel (py, px) of image b, 0 <= px < Wo, 0 <= py < Ho; model: any tag with rays (it selects the depth), a closed-form one without
UD_RM_FN void ud_tsdf_ray(const UdTsdfRayArgs& a, int model, int b, int py, int px) {
  const size_t hw = (size_t)a.Ho * (size_t)a.Wo, i = (size_t)py * (size_t)a.Wo + (size_t)px;
  float d[3];
  if (a.rays) {
    const float* r = a.rays + (size_t)b * 3 * hw + i;
    d[0] = r[0]; d[1] = r[hw]; d[2] = r[2 * hw];
  } else {
    ud_cam_unproject_closed(model, UD_UNPROJ_NORMALIZE, a.params + (size_t)b * 16, (float)px + 0.5f, (float)py + 0.5f, 0.0f, d);
  }
  const float* T = a.T ? a.T + (a.nT == 1 ? 0 : (size_t)b * 12) : nullptr;
  const float* o = a.origin + (a.nO == 1 ? 0 : (size_t)b * 3);
  int k0 = 0, k1 = a.K - 1;
  if (!a.full_scan) ud_tsdf_ray_clip(a, T, o, d, &k0, &k1);
  // a. the scan
  bool hit = false, have = false;
  float sp = 0.0f, sc = 0.0f;
  int kh = 0;
  for (int k = k0; k <= k1; ++k) {
    float s;
    const bool v = ud_tsdf_ray_sample(a, b, T, o, d, a.near + (float)k * a.step, &s);
    if (v && have) {
      if (!(sp < 0.0f) && s < 0.0f) {
        hit = true; kh = k; sc = s;
        break;
      }
      if (sp < 0.0f && !(s < 0.0f)) break;
    }
    have = v;
    sp = s;
  }
  // b. the crossing
  float depth = 0.0f, q[3] = {0.0f, 0.0f, 0.0f}, nrm[3] = {0.0f, 0.0f, 0.0f}, rgb[3] = {0.0f, 0.0f, 0.0f};
  bool valid = false;
  if (hit) {
    const float al = sp / (sp - sc);
    const float t0 = a.near + (float)(kh - 1) * a.step, t1 = a.near + (float)kh * a.step;
    const float ts = t0 + al * (t1 - t0);
    const float x = ts * d[0], y = ts * d[1], z = ts * d[2];
    const float dep = ud_cam_depth(model, x, y, z);
    valid = dep > 0.0f;
    if (valid) {
      depth = dep; q[0] = x; q[1] = y; q[2] = z;
      if (a.normals || a.color_out) {
        float g0[3], g1[3], c0[3], c1[3];
        ud_tsdf_ray_detail(a, b, T, o, d, t0, g0, a.color_out ? c0 : nullptr);
        ud_tsdf_ray_detail(a, b, T, o, d, t1, g1, a.color_out ? c1 : nullptr);
        if (a.color_out)
          for (int k = 0; k < 3; ++k) rgb[k] = c0[k] + al * (c1[k] - c0[k]);
        const float Gx = g0[0] + al * (g1[0] - g0[0]), Gy = g0[1] + al * (g1[1] - g0[1]), Gz = g0[2] + al * (g1[2] - g0[2]);
        float nx = Gx, ny = Gy, nz = Gz;
        if (T) {
          nx = (T[0] * Gx + T[4] * Gy) + T[8] * Gz;
          ny = (T[1] * Gx + T[5] * Gy) + T[9] * Gz;
          nz = (T[2] * Gx + T[6] * Gy) + T[10] * Gz;
        }
        const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
        float m = ax > ay ? ax : ay;
        m = m > az ? m : az;
        if (ud_tsdf_usable(nx) && ud_tsdf_usable(ny) && ud_tsdf_usable(nz) && m > 0.0f) {
          nx = nx / m; ny = ny / m; nz = nz / m;
          const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
          nx = nx / len; ny = ny / len; nz = nz / len;
          if ((nx * x + ny * y) + nz * z > 0.0f) {
            nx = -nx; ny = -ny; nz = -nz;
          }
          if (ud_tsdf_usable(nx) && ud_tsdf_usable(ny) && ud_tsdf_usable(nz)) {
            nrm[0] = nx; nrm[1] = ny; nrm[2] = nz;
          }
        }
      }
    }
  }
  // c. the outputs, written once: exactly 0 where the pixel is not valid
  a.depth[(size_t)b * hw + i] = depth;
  a.valid[(size_t)b * hw + i] = valid ? 1 : 0;
  const size_t at = (size_t)b * 3 * hw + i;
  if (a.points) {
    a.points[at] = q[0]; a.points[at + hw] = q[1]; a.points[at + 2 * hw] = q[2];
  }
  if (a.normals) {
    a.normals[at] = nrm[0]; a.normals[at + hw] = nrm[1]; a.normals[at + 2 * hw] = nrm[2];
  }
  if (a.color_out) {
    if (a.color_f32) {
      float* c = (float*)a.color_out + at;
      c[0] = rgb[0]; c[hw] = rgb[1]; c[2 * hw] = rgb[2];
    } else {
      unsigned char* c = (unsigned char*)a.color_out + at;
      c[0] = valid ? ud_rm_to_u8(rgb[0]) : 0; c[hw] = valid ? ud_rm_to_u8(rgb[1]) : 0; c[2 * hw] = valid ? ud_rm_to_u8(rgb[2]) : 0;
    }
  }
}
