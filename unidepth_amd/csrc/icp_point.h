// Per-pixel arithmetic, the normal system and the solve of frame-to-model point-to-plane ICP (include/unidepth_hip.h, UdIcp): what one
// thread of icp.hip's first kernel does for frame pixel i of image b -- the pixel's point moved by the current estimate T into the model
// camera's frame and projected, the model's point and normal read at the nearest pixel, the gates, the residual and the row of the
// linearised system -- how a row enters the fp64 accumulators, and what the second kernel does with the sums: LDL^T, the Cayley
// retraction, T updated.  Plain functions with no device intrinsics and no kernel: they compose the per-point functions of
// camera_models.h and remap_taps.h and change none of them, so every per-pixel output has the bits of gt_points / unproject_camera ->
// the rigid motion -> project_camera -> remap(mode="nearest") and the element-wise arithmetic run one after the other.  icp.hip compiles
// them into its kernels; tests/icp_host/icp_host.cpp compiles the same header for the host, under the sanitizers.
//
// SAFETY RULE: remap_taps.h's, unchanged -- no float becomes an index before its clamp.  The only indices formed here are the pixel's own
// (i < n, checked by the caller) and the tap offset ud_rm_taps returned.  Every operation rounds separately (-ffp-contract=off), in fp32
// up to the row and in fp64 from there on; the solve uses + - * / only (no libm, no square root), so a numpy fp64 restatement that follows
// the comments below operation by operation has its bits.
#pragma once
#include "camera_models.h"
#include "remap_taps.h"
#pragma clang fp contract(off)

#define UD_ICP_SLOTS 32           /* A upper triangle row-major 0..20, b 21..26, e 27, wsum 28, count 29, 30 and 31 stay 0 */
#define UD_ICP_SUMS 30

// depth [B,n] with params [B,16], or points [B,3,n] in its place (exactly one of the two); mask / weights (each optional) [B,n]; normals
// (optional) [B,3,n]; model_points / model_normals [B,3,hw], model_valid [B,hw], params_model [B,16]; T [nT,3,4] with nT = 1 or B: frame
// camera to model camera.  matched / residual (each optional) [B,n], rows (optional) [B,6,n].  n = H * W, hw = Hm * Wm.
struct UdIcpArgs {
  const float* depth; const float* points; const float* params; const unsigned char* mask; const float* weights; const float* normals;
  const float* model_points; const float* model_normals; const unsigned char* model_valid; const float* params_model; const float* T;
  unsigned char* matched; float* residual; float* rows;
  long long n;
  float tol2, cos_tol;                                 // dist_tol * dist_tol, formed in fp32 by the caller; cos_tol is read only with has_cos
  int B, H, W, Hm, Wm, nT, has_cos;
};

struct UdIcpRow {
  float g[6], r, w;                                    // (c0, c1, c2, n0, n1, n2), the residual, the weight
};

UD_RM_FN bool ud_icp_finite(float x) { return fabsf(x) <= 3.402823466e38f; }      // false for a NaN

// Frame pixel i of image b -> matched, and the row when matched.  model_frame is read only in the depth form and is a closed-form model
// there (Pinhole, EUCM, Spherical, MEI); model_model is any of the six.  Writes the optional per-pixel outputs, exactly 0 where not matched.
UD_RM_FN bool ud_icp_row(const UdIcpArgs& a, int model_frame, int model_model, int b, long long i, UdIcpRow* row) {
  const size_t n = (size_t)a.n, at = (size_t)b * n + (size_t)i, hw = (size_t)a.Hm * (size_t)a.Wm;
  // a. the pixel's point: the identity grid at pixel centres through the frame camera's reconstruct rule (gt_points' bits), or as given
  float p[3];
  bool live;
  if (a.points) {
    const float* s = a.points + (size_t)b * 3 * n + (size_t)i;
    p[0] = s[0]; p[1] = s[n]; p[2] = s[2 * n];
    live = ud_icp_finite(p[0]) && ud_icp_finite(p[1]) && ud_icp_finite(p[2]);
  } else {
    const int py = (int)i / a.W, px = (int)i - py * a.W;
    const float depth = a.depth[at];
    ud_cam_unproject_closed(model_frame, UD_UNPROJ_DEPTH, a.params + (size_t)b * 16, (float)px + 0.5f, (float)py + 0.5f, depth, p);
    live = depth > 0.0f;                               // false for a NaN
  }
  const float w = a.weights ? a.weights[at] : 1.0f;
  live = live && (a.mask ? a.mask[at] != 0 : true) && w > 0.0f && ud_icp_finite(w);
  // b. moved by the estimate and projected through the model camera
  const float* T = a.T + (size_t)(a.nT == 1 ? 0 : b) * 12;
  float q0 = p[0], q1 = p[1], q2 = p[2];
  ud_cam_move(T, q0, q1, q2);
  const float* pm = a.params_model + (size_t)b * 16;
  float u, v;
  ud_cam_project(model_model, pm, q0, q1, q2, &u, &v);
  const float dq = ud_cam_depth(model_model, q0, q1, q2);
  const bool usable = ud_cam_inside(model_model, u, v, q2, a.Hm, a.Wm) && dq > 0.0f && ud_rm_finite(u, v);
  // c. the model at the nearest pixel, zeros padding: read only where the tap is in range and model_valid is not 0
  UdRmTaps t;
  ud_rm_taps(u, v, a.Wm, a.Hm, UD_RM_NEAREST, UD_RM_ZEROS, &t);
  const int off = t.off[0];
  float m[3] = {0.0f, 0.0f, 0.0f}, nn[3] = {0.0f, 0.0f, 0.0f};
  bool tap = false;
  if (off >= 0 && a.model_valid[(size_t)b * hw + (size_t)off] != 0) {
    tap = true;
    for (int k = 0; k < 3; ++k) {
      m[k] = a.model_points[((size_t)b * 3 + (size_t)k) * hw + (size_t)off];
      nn[k] = a.model_normals[((size_t)b * 3 + (size_t)k) * hw + (size_t)off];
    }
  }
  const bool model_ok = tap && ud_rm_inside(u, v, a.Wm, a.Hm);
  // d. the residual and the row
  const float e0 = m[0] - q0, e1 = m[1] - q1, e2 = m[2] - q2;
  const float d2 = (e0 * e0 + e1 * e1) + e2 * e2;
  const float r = (nn[0] * e0 + nn[1] * e1) + nn[2] * e2;
  const float c0 = q1 * nn[2] - q2 * nn[1], c1 = q2 * nn[0] - q0 * nn[2], c2 = q0 * nn[1] - q1 * nn[0];
  bool facing = true;
  if (a.normals && a.has_cos) {
    // the frame normal rotated by T's rotation, products summed left to right, against the model normal
    const float* s = a.normals + (size_t)b * 3 * n + (size_t)i;
    const float f0 = s[0], f1 = s[n], f2 = s[2 * n];
    const float r0 = (T[0] * f0 + T[1] * f1) + T[2] * f2, r1 = (T[4] * f0 + T[5] * f1) + T[6] * f2, r2 = (T[8] * f0 + T[9] * f1) + T[10] * f2;
    facing = (r0 * nn[0] + r1 * nn[1]) + r2 * nn[2] >= a.cos_tol;
  }
  const bool nonzero = nn[0] != 0.0f || nn[1] != 0.0f || nn[2] != 0.0f;
  const bool finite = ud_icp_finite(r) && ud_icp_finite(c0) && ud_icp_finite(c1) && ud_icp_finite(c2) && ud_icp_finite(nn[0]) &&
                      ud_icp_finite(nn[1]) && ud_icp_finite(nn[2]);
  const bool matched = live && usable && model_ok && nonzero && d2 <= a.tol2 && facing && finite;      // every comparison is false for a NaN
  row->g[0] = c0; row->g[1] = c1; row->g[2] = c2; row->g[3] = nn[0]; row->g[4] = nn[1]; row->g[5] = nn[2];
  row->r = r;
  row->w = w;
  if (a.matched) a.matched[at] = matched ? 1 : 0;
  if (a.residual) a.residual[at] = matched ? r : 0.0f;
  if (a.rows)
    for (int k = 0; k < 6; ++k) a.rows[((size_t)b * 6 + (size_t)k) * n + (size_t)i] = matched ? row->g[k] : 0.0f;
  return matched;
}

// A matched pixel's terms added to the 30 running sums: gw_i = (double)w * (double)g_i (exact: 24 x 24 bits); A_ij += gw_i * (double)g_j
// for i <= j, row-major; b_i += gw_i * (double)r; e += ((double)w * (double)r) * (double)r; wsum += (double)w; count += 1.  Each product
// and each addition rounds once.
UD_RM_FN void ud_icp_accumulate(double* acc, const UdIcpRow& row) {
  const double w = (double)row.w, r = (double)row.r;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double gw = w * (double)row.g[i];
#pragma unroll
    for (int j = i; j < 6; ++j) {
      acc[k] = acc[k] + gw * (double)row.g[j];
      ++k;
    }
    acc[21 + i] = acc[21 + i] + gw * r;
  }
  acc[27] = acc[27] + (w * r) * r;
  acc[28] = acc[28] + w;
  acc[29] = acc[29] + 1.0;
}

UD_RM_FN bool ud_icp_finite_d(double x) { return (x < 0.0 ? -x : x) <= 1.7976931348623157e308; }      // false for a NaN

// The update of one image from its system S [32]: x = (omega, v) minimises sum w (r - g . x)^2, so A x = b.  T [3,4] fp32 is updated in
// place when the status is 1 and left as it was otherwise (x = 0 then).  The operations, in this order, all in fp64:
//   1. A is the symmetric 6 x 6 matrix of S[0..20] (row-major upper triangle), A_ii = A_ii + damping; b = S[21..26].
//   2. LDL^T without pivoting, column by column, j = 0 .. 5:
//        s = 0 for j = 0, else s = (L_j0 * L_j0) * d_0, then s = s + (L_jk * L_jk) * d_k for k = 1 .. j-1;   d_j = A_jj - s   (d_0 = A_00)
//        not d_j > 0 (a NaN included): status 0, stop.
//        for i = j+1 .. 5: s likewise from (L_ik * L_jk) * d_k;   L_ij = (A_ij - s) / d_j   (L_i0 = A_i0 / d_0)
//   3. forward, i = 0 .. 5:  s = L_i0 * y_0, s = s + L_ik * y_k for k = 1 .. i-1;  y_i = b_i - s   (y_0 = b_0)
//      diagonal:             z_i = y_i / d_i
//      back, i = 5 .. 0:     s = L_(i+1)i * x_(i+1), s = s + L_ki * x_k for k = i+2 .. 5;  x_i = z_i - s   (x_5 = z_5)
//   4. status = S[29] >= (double)min_count and every d_j > 0 and every x_i finite.
//   5. Cayley: a_i = x_i * 0.5 (i < 3); aa = (a_0 * a_0 + a_1 * a_1) + a_2 * a_2; den = 1 + aa; k = 1 - aa; t_i = 2 * a_i;
//        R = [ (k + t_0 * a_0) / den     (t_0 * a_1 - t_2) / den   (t_0 * a_2 + t_1) / den
//              (t_1 * a_0 + t_2) / den   (k + t_1 * a_1) / den     (t_1 * a_2 - t_0) / den
//              (t_2 * a_0 - t_1) / den   (t_2 * a_1 + t_0) / den   (k + t_2 * a_2) / den ]
//   6. with O the widened fp32 T: N_ij = (R_i0 * O_0j + R_i1 * O_1j) + R_i2 * O_2j for j = 0 .. 3, and N_i3 = N_i3 + x_(3+i);
//      T_ij = (float)N_ij, the one rounding to fp32.
UD_RM_FN int ud_icp_solve(const double* S, double damping, int min_count, float* T, double* x) {
  for (int i = 0; i < 6; ++i) x[i] = 0.0;
  double A[6][6], L[6][6], d[6], y[6], z[6], xs[6];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      A[i][j] = S[k];
      A[j][i] = S[k];
      ++k;
    }
  for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + damping;
  for (int j = 0; j < 6; ++j) {
    double s = 0.0;
    for (int c = 0; c < j; ++c) {
      const double term = (L[j][c] * L[j][c]) * d[c];
      s = c == 0 ? term : s + term;
    }
    d[j] = j == 0 ? A[j][j] : A[j][j] - s;
    if (!(d[j] > 0.0)) return 0;
    for (int i = j + 1; i < 6; ++i) {
      s = 0.0;
      for (int c = 0; c < j; ++c) {
        const double term = (L[i][c] * L[j][c]) * d[c];
        s = c == 0 ? term : s + term;
      }
      L[i][j] = (j == 0 ? A[i][j] : A[i][j] - s) / d[j];
    }
  }
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
    for (int c = 0; c < i; ++c) {
      const double term = L[i][c] * y[c];
      s = c == 0 ? term : s + term;
    }
    y[i] = i == 0 ? S[21 + i] : S[21 + i] - s;
  }
  for (int i = 0; i < 6; ++i) z[i] = y[i] / d[i];
  for (int i = 5; i >= 0; --i) {
    double s = 0.0;
    for (int c = i + 1; c < 6; ++c) {
      const double term = L[c][i] * xs[c];
      s = c == i + 1 ? term : s + term;
    }
    xs[i] = i == 5 ? z[i] : z[i] - s;
  }
  bool ok = S[29] >= (double)min_count;
  for (int i = 0; i < 6; ++i) ok = ok && ud_icp_finite_d(xs[i]);
  if (!ok) return 0;
  const double a0 = xs[0] * 0.5, a1 = xs[1] * 0.5, a2 = xs[2] * 0.5;
  const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
  const double den = 1.0 + aa, kk = 1.0 - aa, t0 = 2.0 * a0, t1 = 2.0 * a1, t2 = 2.0 * a2;
  const double R[3][3] = {{(kk + t0 * a0) / den, (t0 * a1 - t2) / den, (t0 * a2 + t1) / den},
                          {(t1 * a0 + t2) / den, (kk + t1 * a1) / den, (t1 * a2 - t0) / den},
                          {(t2 * a0 - t1) / den, (t2 * a1 + t0) / den, (kk + t2 * a2) / den}};
  double O[3][4], N[3][4];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) O[i][j] = (double)T[4 * i + j];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) N[i][j] = (R[i][0] * O[0][j] + R[i][1] * O[1][j]) + R[i][2] * O[2][j];
    N[i][3] = N[i][3] + xs[3 + i];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) T[4 * i + j] = (float)N[i][j];
  for (int i = 0; i < 6; ++i) x[i] = xs[i];
  return 1;
}
