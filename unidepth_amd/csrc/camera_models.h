// Per-pixel arithmetic of the iterative ground-truth camera models (reference unidepth/utils/camera.py: OPENCV :412-694,
// Fisheye624 :697-974, MEI :977-1082).  Plain float functions with no device intrinsics: pointwise.hip compiles them into the
// ray kernels, tests/test_camera_models_cpu.py compiles the same header for the host to check the arithmetic without a GPU.
//
// Parameter vectors (after the crop/resize bookkeeping of infer(), one camera):
//   OPENCV / Fisheye624 : [fx, fy, cx, cy, k1..k6, p1, p2, s1..s4]  (16 floats; OPENCV uses k1..k3, k4..k6 must be 0)
//   MEI                 : [fx, fy, cx, cy, k1, k2, p1, p2, xi]
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define UD_CAM_FN __host__ __device__ __forceinline__
#else
#define UD_CAM_FN static inline
#endif

#define UD_CAM_EPS 1e-3f          /* convergence / guard threshold of the OPENCV and Fisheye624 solvers (camera.py:497,779) */
#define UD_CAM_EPS_MEI 1e-6f      /* camera.py:986 */

// Newton iterations undoing tangential (p0, p1) and thin-prism (s0..s3) distortion: solves dist(xr, yr) = (ud, vd) starting
// from (ud, vd), a fixed number of iterations (camera.py:517-585 / :799-867 / :1000-1046).  The reference builds the Jacobian
// from a matrix of ONES (`new_ones(B, N, 2, 2)`), so with thin-prism terms but no tangential terms its off-diagonals start
// at 1, not 0 -- reproduced here, since the results are what has to match.
UD_CAM_FN void ud_cam_undistort_tanprism(float ud, float vd, float p0, float p1, float s0, float s1, float s2, float s3,
                                         int use_tan, int use_prism, int iters, float& xr_out, float& yr_out) {
  float xr = ud, yr = vd;
  for (int it = 0; it < iters; ++it) {
    const float xr2 = xr * xr, yr2 = yr * yr;
    const float rd = xr2 + yr2;
    float ex = xr, ey = yr;
    float a = 1.0f, b = 1.0f, c = 1.0f, d = 1.0f;
    if (use_tan) {
      ex = ex + ((2.0f * xr2 + rd) * p0 + 2.0f * xr * yr * p1);
      ey = ey + ((2.0f * yr2 + rd) * p1 + 2.0f * xr * yr * p0);
      a = 1.0f + 6.0f * xr * p0 + 2.0f * yr * p1;
      b = 2.0f * (xr * p1 + yr * p0);
      c = b;
      d = 1.0f + 6.0f * yr * p1 + 2.0f * xr * p0;
    }
    if (use_prism) {
      const float rd4 = rd * rd;
      ex = ex + (s0 * rd + s1 * rd4);
      ey = ey + (s2 * rd + s3 * rd4);
      const float t1 = 2.0f * (s0 + 2.0f * s1 * rd);
      const float t2 = 2.0f * (s2 + 2.0f * s3 * rd);
      a += xr * t1; b += yr * t1;
      c += xr * t2; d += yr * t2;
    }
    const float det = 1.0f / (a * d - b * c);
    const float e = ud - ex, f = vd - ey;
    xr = xr + ((det * d) * e + (det * -b) * f);
    yr = yr + ((det * -c) * e + (det * a) * f);
  }
  xr_out = xr;
  yr_out = yr;
}

// Radial polynomial th * (1 + sum_j k_j th^(2j+2)) and its derivative 1 + sum_j (2j+3) k_j th^(2j+2), j < nk
// (camera.py:603-622: nk = 3 for OPENCV, 6 for Fisheye624).
UD_CAM_FN float ud_cam_radial(const float* k, int nk, float th, float& dth) {
  const float t2 = th * th;
  float pw = t2, s = 0.0f, ds = 0.0f;
  for (int j = 0; j < nk; ++j) {
    s += pw * k[j];
    ds += (2.0f * (float)j + 3.0f) * k[j] * pw;
    pw *= t2;
  }
  dth = 1.0f + ds;
  return (1.0f + s) * th;
}

UD_CAM_FN float ud_cam_radial_residual(const float* k, int nk, float th, float rnorm) {
  float dth;
  return ud_cam_radial(k, nk, th, dth) - rnorm;
}

// One trust-region Newton iteration on theta (camera.py:603-691 / :885-971).  `delta` is the pixel's trust radius.
// The caller decides whether the iteration runs at all: the reference stops ALL pixels as soon as the largest |residual|
// over the image is below UD_CAM_EPS (`if torch.max(torch.abs(residual)) < eps: break`).
UD_CAM_FN void ud_cam_radial_step(const float* k, int nk, float rnorm, float& th, float& delta) {
  float dth;
  const float res = ud_cam_radial(k, nk, th, dth) - rnorm;
  const float safe = fabsf(dth) < UD_CAM_EPS ? UD_CAM_EPS : dth;
  const float step = -res / safe;
  const float pred = -(res * step);
  const float sn = fabsf(step);
  const float step_scaled = sn > delta ? step * (delta / sn) : step;
  const float th_new = th + step_scaled;
  const float res_new = ud_cam_radial_residual(k, nk, th_new, rnorm);
  const float actual = fabsf(res) - fabsf(res_new);
  float rho = actual / pred;
  if (actual == 0.0f && pred == 0.0f) rho = 1.0f;
  if (rho > 0.5f) delta = fminf(2.0f * delta, 1.0f);
  if (rho < 0.2f) delta = 0.25f * delta;
  if (rho > 0.1f) th = th_new;
}

// Final direction of the OPENCV (tan_theta = 0) / Fisheye624 (tan_theta = 1) models, then Camera.get_rays' normalisation
// (camera.py:693-698, :971-976, :88-92).
UD_CAM_FN void ud_cam_finish_radial(float xr, float yr, float rnorm, float th, int tan_theta, float& x, float& y, float& z) {
  const bool close = fabsf(th) < UD_CAM_EPS && fabsf(rnorm) < UD_CAM_EPS;
  const float sc = (tan_theta ? tanf(th) : th) / rnorm;
  const float dx = close ? xr : sc * xr, dy = close ? yr : sc * yr;
  const float inv = 1.0f / fmaxf(sqrtf(dx * dx + dy * dy + 1.0f), 1e-4f);
  x = dx * inv; y = dy * inv; z = inv;
}

// MEI (unified omnidirectional) model, fully per pixel: 20 tangential Newton iterations, 20 radial ones, lifting to the unit
// sphere model with mirror parameter xi (camera.py:985-1082), then get_rays' normalisation.
UD_CAM_FN void ud_cam_mei(const float* p, float u, float v, float& x, float& y, float& z) {
  const float k1 = p[4], k2 = p[5], p0 = p[6], p1 = p[7], xi = p[8];
  const int use_radial = fabsf(k1) + fabsf(k2) > 1e-6f;
  const int use_tan = fabsf(p0) + fabsf(p1) > 1e-6f;
  const float ud = (u - p[2]) / p[0], vd = (v - p[3]) / p[1];
  float xr, yr;
  ud_cam_undistort_tanprism(ud, vd, p0, p1, 0.f, 0.f, 0.f, 0.f, 1, 0, use_tan ? 20 : 0, xr, yr);
  const float rnorm = sqrtf(xr * xr + yr * yr);
  float th = rnorm;
  for (int it = 0; it < (use_radial ? 20 : 0); ++it) {
    const float t2 = th * th, t4 = t2 * t2;
    const float thr = (1.0f + k1 * t2 + k2 * t4) * th;
    const float dth = 1.0f + 3.0f * k1 * t2 + 5.0f * k2 * t4;
    float step = (rnorm - thr) / dth;
    if (!(fabsf(dth) > UD_CAM_EPS_MEI)) step = (step > 0.f ? 1.f : (step < 0.f ? -1.f : 0.f)) * UD_CAM_EPS_MEI * 10.0f;
    th = th + step;
  }
  const bool close = fabsf(th) < UD_CAM_EPS_MEI && fabsf(rnorm) < UD_CAM_EPS_MEI;
  const float dx = close ? xr : th * xr / rnorm, dy = close ? yr : th * yr / rnorm;
  const float rho = sqrtf(dx * dx + dy * dy);
  const float rho2 = rho * rho;
  const float sq = sqrtf(1.0f + (1.0f - xi * xi) * rho2);
  float pz = 1.0f - xi * (rho2 + 1.0f) / (xi + sq);
  if (xi == 1.0f) pz = (1.0f - rho2) / 2.0f;
  const float inv = 1.0f / fmaxf(sqrtf(dx * dx + dy * dy + pz * pz), 1e-4f);
  x = dx * inv; y = dy * inv; z = pz * inv;
}

// ---- the same directions NOT normalised: what Camera.reconstruct (camera.py:69-76) divides by its z and multiplies with the depth
// (reconstruct.hip).  Separate functions, the same operations in the same order: the normalised ones above stay exactly as they
// were, so the ray kernels that inline them compile to the same code.  The solver bodies are therefore duplicated and must be kept in
// step by hand: test_unnormalised_header_functions_on_the_host (tests/test_gt_points_cpu.py, through tests/recon_host) fails when
// normalising one of these no longer reproduces its twin above bit for bit.
// ud_cam_finish_radial without the normalisation: (dx, dy), z = 1, as unproject() returns it (camera.py:687-694, :967-974).
UD_CAM_FN void ud_cam_finish_radial_dir(float xr, float yr, float rnorm, float th, int tan_theta, float& dx, float& dy) {
  const bool close = fabsf(th) < UD_CAM_EPS && fabsf(rnorm) < UD_CAM_EPS;
  const float sc = (tan_theta ? tanf(th) : th) / rnorm;
  dx = close ? xr : sc * xr;
  dy = close ? yr : sc * yr;
}

// ud_cam_mei without the normalisation: (dx, dy, pz) as MEI.unproject returns it (camera.py:1063-1081); pz is <= 0 beyond the
// mirror's horizon.
UD_CAM_FN void ud_cam_mei_dir(const float* p, float u, float v, float& dx, float& dy, float& pz) {
  const float k1 = p[4], k2 = p[5], p0 = p[6], p1 = p[7], xi = p[8];
  const int use_radial = fabsf(k1) + fabsf(k2) > 1e-6f;
  const int use_tan = fabsf(p0) + fabsf(p1) > 1e-6f;
  const float ud = (u - p[2]) / p[0], vd = (v - p[3]) / p[1];
  float xr, yr;
  ud_cam_undistort_tanprism(ud, vd, p0, p1, 0.f, 0.f, 0.f, 0.f, 1, 0, use_tan ? 20 : 0, xr, yr);
  const float rnorm = sqrtf(xr * xr + yr * yr);
  float th = rnorm;
  for (int it = 0; it < (use_radial ? 20 : 0); ++it) {
    const float t2 = th * th, t4 = t2 * t2;
    const float thr = (1.0f + k1 * t2 + k2 * t4) * th;
    const float dth = 1.0f + 3.0f * k1 * t2 + 5.0f * k2 * t4;
    float step = (rnorm - thr) / dth;
    if (!(fabsf(dth) > UD_CAM_EPS_MEI)) step = (step > 0.f ? 1.f : (step < 0.f ? -1.f : 0.f)) * UD_CAM_EPS_MEI * 10.0f;
    th = th + step;
  }
  const bool close = fabsf(th) < UD_CAM_EPS_MEI && fabsf(rnorm) < UD_CAM_EPS_MEI;
  dx = close ? xr : th * xr / rnorm;
  dy = close ? yr : th * yr / rnorm;
  const float rho = sqrtf(dx * dx + dy * dy);
  const float rho2 = rho * rho;
  const float sq = sqrtf(1.0f + (1.0f - xi * xi) * rho2);
  pz = 1.0f - xi * (rho2 + 1.0f) / (xi + sq);
  if (xi == 1.0f) pz = (1.0f - rho2) / 2.0f;
}

// ---- the forward models: Camera.project of every class (camera.py: Pinhole :239-252, EUCM :281-304, Spherical :359-368, OPENCV :423-493,
// Fisheye624 :705-775, MEI :1084-1142), a camera-frame point (x, y, z) -> image coordinates (u, v).  Closed form, operation by operation
// in the reference's order, so that the numpy fp32 restatement of tools/make_golden_camera_project.py reproduces them (project.hip and
// splat.hip are built with -ffp-contract=off; tests/proj_host compiles this header for the host).  `p` is the 16-float parameter row of
// UdReconstruct.  Model tags as UdReconstruct.model.
enum { UD_CAM_PINHOLE = 1, UD_CAM_EUCM = 2, UD_CAM_SPHERICAL = 3, UD_CAM_OPENCV = 4, UD_CAM_FISHEYE624 = 5, UD_CAM_MEI = 6 };

UD_CAM_FN bool ud_cam_model_ok(int m) { return m >= UD_CAM_PINHOLE && m <= UD_CAM_MEI; }
// closed-form unprojection: every model but OPENCV and Fisheye624, whose radial loop ends on a maximum over the whole image
UD_CAM_FN bool ud_cam_closed_form(int m) { return m == UD_CAM_PINHOLE || m == UD_CAM_EUCM || m == UD_CAM_SPHERICAL || m == UD_CAM_MEI; }

// The rigid motion t fp32 [3,4] applied to a point in place: x' = ((t0 x + t1 y) + t2 z) + t3, and the same for y' and z' with rows 1
// and 2.  The association is fixed -- products summed left to right, the translation last, every operation rounded separately: the
// fused kernels (warp, consistency) have the bits of the separate launches only because all of them move points through this function.
UD_CAM_FN void ud_cam_move(const float* t, float& x, float& y, float& z) {
  const float xt = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
  const float yt = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
  const float zt = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
  x = xt; y = yt; z = zt;
}

// max(x, m) that lets a NaN through, as torch.clamp(min=m) does
UD_CAM_FN float ud_cam_floor(float x, float m) { return x < m ? m : x; }

// K (x, y, z) of the skew-free K built from the row, divided by max(w, 0.01) (camera.py:242-243)
UD_CAM_FN void ud_cam_project_pinhole(const float* p, float x, float y, float z, float* u, float* v) {
  const float zc = ud_cam_floor(z, 0.01f);
  *u = (p[0] * x + p[2] * z) / zc;
  *v = (p[1] * y + p[3] * z) / zc;
}

UD_CAM_FN void ud_cam_project_eucm(const float* p, float x, float y, float z, float* u, float* v) {
  const float al = p[4], be = p[5];
  const float d = sqrtf(be * (x * x + y * y) + z * z);
  const float den = ud_cam_floor(al * d + (1.0f - al) * z, 1e-3f);
  *u = p[0] * (x / den) + p[2];
  *v = p[1] * (y / den) + p[3];
}

// equirectangular: W, H are the row's own values (p[4], p[5]), the half fields of view p[6], p[7]
UD_CAM_FN void ud_cam_project_spherical(const float* p, float x, float y, float z, float* u, float* v) {
  const float lon = atan2f(x, z);
  const float lat = asinf(y / ud_cam_floor(sqrtf(x * x + y * y + z * z), 1e-5f));
  *u = lon / (2.0f * p[6]) * (p[4] - 1.0f) + (p[4] - 1.0f) / 2.0f;
  *v = lat / (2.0f * p[7]) * (p[5] - 1.0f) + (p[5] - 1.0f) / 2.0f;
}

// the shared front end of OPENCV and Fisheye624: z replaced by eps * sign(z) when |z| < eps = 1e-9 (sign(0) = 0, so z = 0 divides by
// zero as in the reference), ab = xy / z, r = |ab|
UD_CAM_FN void ud_cam_project_front(float x, float y, float z, float* a, float* b, float* r) {
  const float sg = z > 0.0f ? 1.0f : (z < 0.0f ? -1.0f : 0.0f);
  const float zz = fabsf(z) < 1e-9f ? 1e-9f * sg : z;
  *a = x / zz;
  *b = y / zz;
  *r = sqrtf(*a * *a + *b * *b);
}

// the shared back end: tangential (p0, p1), thin prism (s = s0..s3, or null for MEI), focal lengths and principal point
UD_CAM_FN void ud_cam_project_back(const float* p, float xr, float yr, float p0, float p1, const float* s, float* u, float* v) {
  const float xr2 = xr * xr, yr2 = yr * yr;
  const float rd = xr2 + yr2;
  float ud = xr + ((2.0f * xr2 + rd) * p0 + 2.0f * xr * yr * p1);
  float vd = yr + ((2.0f * yr2 + rd) * p1 + 2.0f * xr * yr * p0);
  if (s) {
    const float rd4 = rd * rd;
    ud = ud + (s[0] * rd + s[1] * rd4);
    vd = vd + (s[2] * rd + s[3] * rd4);
  }
  *u = ud * p[0] + p[2];
  *v = vd * p[1] + p[3];
}

// radial numerator 1 + k1 r^2 + k2 r^4 + k3 r^6; the denominator is 1: k4..k6 are refused when the camera is constructed
UD_CAM_FN void ud_cam_project_opencv(const float* p, float x, float y, float z, float* u, float* v) {
  float a, b, r;
  ud_cam_project_front(x, y, z, &a, &b, &r);
  const float r2 = r * r, r4 = r2 * r2, r6 = r4 * r2;
  const float num = 1.0f + ((r2 * p[4] + r4 * p[5]) + r6 * p[6]);
  ud_cam_project_back(p, a * num, b * num, p[10], p[11], p + 12, u, v);
}

// th = atan(r), th_k = th + sum_j k_j th^(3+2j), along ab / r (1 for BOTH components where r < 1e-9: the reference's ones_like)
UD_CAM_FN void ud_cam_project_fisheye624(const float* p, float x, float y, float z, float* u, float* v) {
  float a, b, r;
  ud_cam_project_front(x, y, z, &a, &b, &r);
  const float th = atanf(r);
  const float dx = r < 1e-9f ? 1.0f : a / r, dy = r < 1e-9f ? 1.0f : b / r;
  const float t2 = th * th;
  float pw = th * t2, s = 0.0f;
  for (int j = 0; j < 6; ++j) {
    s = s + pw * p[4 + j];
    pw = pw * t2;
  }
  const float thk = th + s;
  ud_cam_project_back(p, thk * dx, thk * dy, p[10], p[11], p + 12, u, v);
}

UD_CAM_FN void ud_cam_project_mei(const float* p, float x, float y, float z, float* u, float* v) {
  const float n = sqrtf(x * x + y * y + z * z);
  const float den = z + p[8] * n;
  const float a = x / den, b = y / den;
  const float r = sqrtf(a * a + b * b);
  const float r2 = r * r, r4 = r2 * r2;
  const float f = 1.0f + p[4] * r2 + p[5] * r4;
  ud_cam_project_back(p, a * f, b * f, p[6], p[7], nullptr, u, v);
}

UD_CAM_FN void ud_cam_project(int model, const float* p, float x, float y, float z, float* u, float* v) {
  switch (model) {
    case UD_CAM_PINHOLE: ud_cam_project_pinhole(p, x, y, z, u, v); break;
    case UD_CAM_EUCM: ud_cam_project_eucm(p, x, y, z, u, v); break;
    case UD_CAM_SPHERICAL: ud_cam_project_spherical(p, x, y, z, u, v); break;
    case UD_CAM_OPENCV: ud_cam_project_opencv(p, x, y, z, u, v); break;
    case UD_CAM_FISHEYE624: ud_cam_project_fisheye624(p, x, y, z, u, v); break;
    default: ud_cam_project_mei(p, x, y, z, u, v); break;
  }
}

// the model's depth of a point, the quantity Camera.reconstruct multiplies its direction with: z, or the distance for Spherical
UD_CAM_FN float ud_cam_depth(int model, float x, float y, float z) {
  return model == UD_CAM_SPHERICAL ? sqrtf(x * x + y * y + z * z) : z;
}

// each class's own in-image test with the reference's comparisons taken literally (a NaN coordinate is "inside" for every model but
// Pinhole, as it is there).  Spherical has no test in the reference: the OPENCV form.
UD_CAM_FN bool ud_cam_inside(int model, float u, float v, float z, int H, int W) {
  const float w = (float)W, h = (float)H;
  if (model == UD_CAM_PINHOLE) return u >= 0.0f && u < w && v >= 0.0f && v < h;
  if (model == UD_CAM_EUCM) return !(u < 0.0f || u > w || v < 0.0f || v > h || z < 0.0f);
  return !(u < 0.0f || u > w || v < 0.0f || v > h);
}

// ---- the inverse models at ANY image coordinate: Camera.unproject of every class (camera.py: Pinhole :255-266, EUCM :307-328, Spherical
// :371-386, OPENCV :496-694, Fisheye624 :778-974, MEI :985-1082) and the three forms a caller can ask of the result (unproject.hip; the
// arithmetic of the closed-form models is reconstruct.hip's, expression by expression, so that the identity grid with a depth gives the
// bits of ud_reconstruct).  Every operation rounds separately under -ffp-contract=off; tests/unproj_host compiles these for the host.

// the closed-form inverse of the skew-free K BEFORE the division by max(z, 1e-4): one subtraction and one division per axis; z is 1, or
// NaN when an intrinsic or a coordinate is not finite: the reference inverts the whole matrix and its last row [0 0 1] multiplies
// (u, v, 1), so the division by z turns the whole ray into NaN there as well
UD_CAM_FN void ud_cam_unproject_pinhole(const float* p, float u, float v, float* x, float* y, float* z) {
  *x = (u - p[2]) / p[0];
  *y = (v - p[3]) / p[1];
  *z = ((0.0f * (p[0] + p[1] + p[2] + p[3]) + 0.0f * u) + 0.0f * v) + 1.0f;
}

// (c mx, c my, c mz) with z NOT yet clamped to 1e-3, and the reference's unprojection_mask (taken before the clamp)
UD_CAM_FN bool ud_cam_unproject_eucm(const float* p, float u, float v, float* x, float* y, float* z) {
  const float al = p[4], be = p[5];
  const float mx = (u - p[2]) / p[0], my = (v - p[3]) / p[1];
  const float r2 = mx * mx + my * my;
  const float sv = 1.0f - (2.0f * al - 1.0f) * be * r2;
  const float mz = (1.0f - be * (al * al) * r2) / (al * sqrtf(ud_cam_floor(sv, 1e-5f)) + (1.0f - al));
  const float cf = 1.0f / sqrtf(mx * mx + my * my + mz * mz + 1e-5f);
  *x = cf * mx; *y = cf * my; *z = cf * mz;
  const float lim = al < 0.5f ? 1e6f : 1.0f / (be * (2.0f * al - 1.0f));
  return r2 < lim && *z > 1e-3f;
}

// the unit-sphere direction of an equirectangular pixel, re-normalised with the 1e-5 floor
UD_CAM_FN void ud_cam_unproject_spherical(const float* p, float u, float v, float* x, float* y, float* z) {
  const float lon = (u - (p[4] - 1.0f) / 2.0f) / (p[4] - 1.0f) * (2.0f * p[6]);
  const float lat = (v - (p[5] - 1.0f) / 2.0f) / (p[5] - 1.0f) * (2.0f * p[7]);
  const float cl = cosf(lat);
  const float sx = cl * sinf(lon), sy = sinf(lat), sz = cl * cosf(lon);
  const float n = ud_cam_floor(sqrtf(sx * sx + sy * sy + sz * sz), 1e-5f);
  *x = sx / n; *y = sy / n; *z = sz / n;
}

// OPENCV / Fisheye624, the part before the radial loop: the tangential / thin-prism Newton iterations and |xr, yr|
UD_CAM_FN bool ud_cam_radial_front(const float* p, float u, float v, float* xr, float* yr, float* rnorm) {
  const int use_tan = fabsf(p[10]) + fabsf(p[11]) > 1e-6f;
  const int use_prism = fabsf(p[12]) + fabsf(p[13]) + fabsf(p[14]) + fabsf(p[15]) > 1e-6f;
  const float ud = (u - p[2]) / p[0], vd = (v - p[3]) / p[1];
  ud_cam_undistort_tanprism(ud, vd, p[10], p[11], p[12], p[13], p[14], p[15], use_tan, use_prism, (use_tan || use_prism) ? 10 : 0, *xr, *yr);
  *rnorm = sqrtf(*xr * *xr + *yr * *yr);
  return fabsf(p[4]) + fabsf(p[5]) + fabsf(p[6]) + fabsf(p[7]) + fabsf(p[8]) + fabsf(p[9]) > 1e-6f;      // use_radial
}

// the larger of two non-negative residuals; a NaN wins, so that `max < eps` is false as in the reference
UD_CAM_FN float ud_cam_nanmax(float a, float b) { return (b > a || b != b) ? b : a; }

// the number of trust-region iterations the reference runs on a point set whose largest |residual| at theta_it is maxima[it], it = 0..9:
// it leaves the loop at the first look below UD_CAM_EPS (camera.py:624)
UD_CAM_FN int ud_cam_radial_exit(const float* maxima) {
  int k = 0;
  while (k < 10 && !(maxima[k] < UD_CAM_EPS)) ++k;
  return k;
}

// theta after `steps` trust-region iterations from theta_0 = rnorm with the trust radius 0.1: a point's iterates depend on that point alone
UD_CAM_FN float ud_cam_radial_solve(const float* k, int nk, float rnorm, int steps) {
  float th = rnorm, delta = 0.1f;
  for (int it = 0; it < steps; ++it) ud_cam_radial_step(k, nk, rnorm, th, delta);
  return th;
}

enum { UD_UNPROJ_RAW = 0, UD_UNPROJ_NORMALIZE = 1, UD_UNPROJ_DEPTH = 2 };

// what goes out for a direction r = (x, y, z) of `model` (Pinhole: before its division; EUCM: z before its clamp):
//   RAW        the class's own unproject value: Pinhole r / max(r.z, 1e-4), EUCM (x, y, max(z, 1e-3)), the others r
//   NORMALIZE  that / max(|that|, 1e-4): Camera.get_rays (camera.py:88-92)
//   DEPTH      the class's reconstruct: Pinhole r / max(r.z, 1e-4) * max(d, 0); Spherical r * d; the others (EUCM after its clamp)
//              r / max(r.z, 1e-4) * max(d, 1e-4)
// Returns the reference's unprojection_mask where the class sets one (Pinhole: z of the stored ray > 1e-4), else true; EUCM's comes from
// ud_cam_unproject_eucm.
UD_CAM_FN bool ud_cam_unproject_form(int model, int form, float x, float y, float z, float d, float* o) {
  bool valid = true;
  if (model == UD_CAM_PINHOLE) {
    const float zc = ud_cam_floor(z, 1e-4f);
    valid = z / zc > 1e-4f;
    if (form == UD_UNPROJ_DEPTH) {
      const float dc = ud_cam_floor(d, 0.0f);
      o[0] = x / zc * dc; o[1] = y / zc * dc; o[2] = z / zc * dc;
      return valid;
    }
    x = x / zc; y = y / zc; z = z / zc;
  } else if (model == UD_CAM_EUCM) {
    z = ud_cam_floor(z, 1e-3f);
  }
  if (form == UD_UNPROJ_DEPTH) {
    if (model == UD_CAM_SPHERICAL) {
      o[0] = x * d; o[1] = y * d; o[2] = z * d;
    } else {
      const float zc = ud_cam_floor(z, 1e-4f), dc = ud_cam_floor(d, 1e-4f);
      o[0] = x / zc * dc; o[1] = y / zc * dc; o[2] = z / zc * dc;
    }
  } else if (form == UD_UNPROJ_NORMALIZE) {
    const float n = ud_cam_floor(sqrtf(x * x + y * y + z * z), 1e-4f);
    o[0] = x / n; o[1] = y / n; o[2] = z / n;
  } else {
    o[0] = x; o[1] = y; o[2] = z;
  }
  return valid;
}

// a closed-form image's point, start to end (Pinhole, EUCM, Spherical, MEI)
UD_CAM_FN bool ud_cam_unproject_closed(int model, int form, const float* p, float u, float v, float d, float* o) {
  float x, y, z;
  bool valid = true;
  if (model == UD_CAM_PINHOLE) ud_cam_unproject_pinhole(p, u, v, &x, &y, &z);
  else if (model == UD_CAM_EUCM) valid = ud_cam_unproject_eucm(p, u, v, &x, &y, &z);
  else if (model == UD_CAM_SPHERICAL) ud_cam_unproject_spherical(p, u, v, &x, &y, &z);
  else ud_cam_mei_dir(p, u, v, x, y, z);
  const bool form_valid = ud_cam_unproject_form(model, form, x, y, z, d, o);
  return valid && form_valid;
}

// an OPENCV / Fisheye624 point once the number of iterations of its image is known
UD_CAM_FN void ud_cam_unproject_radial(int model, int form, const float* p, float u, float v, float d, int steps, float* o) {
  float xr, yr, rnorm, dx, dy;
  ud_cam_radial_front(p, u, v, &xr, &yr, &rnorm);
  const float th = ud_cam_radial_solve(p + 4, model == UD_CAM_FISHEYE624 ? 6 : 3, rnorm, steps);
  ud_cam_finish_radial_dir(xr, yr, rnorm, th, model == UD_CAM_FISHEYE624, dx, dy);
  ud_cam_unproject_form(model, form, dx, dy, 1.0f, d, o);
}
