// TEST INFRASTRUCTURE ONLY: a stand-alone host program around unidepth_amd/csrc/icp_point.h, which runs what the two kernels of icp.hip
// run -- ud_icp_row for every frame pixel in the kernel's addressing, ud_icp_accumulate over the matched pixels (here in pixel order, one
// running sum per slot), ud_icp_solve on the sums -- and, beside the first pass, the CHAIN of the unchanged per-point functions the fused
// one is made of, pass by pass with every intermediate stored in memory as the separate launches store it: ud_cam_unproject_closed
// (reconstruct.hip) on the identity grid, the rigid motion, ud_cam_project + ud_cam_inside + ud_cam_depth (project.hip), ud_rm_point
// (remap.hip) in nearest mode on the six model channels with coord_valid = inside && depth > 0 and src_mask = model_valid, then one loop per
// element-wise operation.  Both must give the same bits in matched, residual and rows; the program exits 3 otherwise.  So
// tests/test_icp_cpu.py can check the fusion, the sums, the solve and the whole loop without a GPU, under the host sanitizers: every array is
// allocated exactly as large as its contents, so an index that escapes is an AddressSanitizer report, and a float-to-int conversion of an
// unsafe coordinate is an UBSan report.
//
//   icp_host run B H W Hm Wm NT FORM HAS_MASK HAS_W HAS_N HAS_COS DIST_BITS COS_BITS ITERS MIN_COUNT DAMP_BITS MF_0..MF_B-1 MM_0..MM_B-1 < input
//       FORM 0: a depth frame, 1: a point map.  The tolerances as fp32 bit patterns, the damping as an fp64 bit pattern (decimal int64).
//       MF_b the frame camera's model tags (closed-form models; ignored with FORM 1), MM_b the model camera's.  ITERS 0: linearise once at
//       T; ITERS > 0 (needs NT = B): that many steps, T updated in place.
//       input, binary: frame [B,H,W] or [B,3,H,W] float32, params [B,16] float32, mask [B,H,W] bytes (HAS_MASK), weights [B,H,W] float32
//       (HAS_W), normals [B,3,H,W] float32 (HAS_N), model_points [B,3,Hm,Wm] float32, model_normals [B,3,Hm,Wm] float32, model_valid
//       [B,Hm,Wm] bytes, params_model [B,16] float32, T [NT,3,4] float32.
//       output: of the first pass matched [B,H,W] bytes, residual [B,H,W] float32, rows [B,6,H,W] float32, and the chain's p [B,3,H,W]
//       float32 and uv [B,2,H,W] float32; then systems [K,B,32] float64 with K = max(ITERS, 1), and with ITERS > 0 x [K,B,6] float64,
//       status [K,B] bytes, T after each step [K,B,3,4] float32.
//   icp_host solve B MIN_COUNT DAMP_BITS < input
//       input: systems [B,32] float64, T [B,3,4] float32.  output: T_new [B,3,4] float32, x [B,6] float64, status [B] bytes.
//
// Never loaded by the product.
#include "../../unidepth_amd/csrc/icp_point.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

template <typename T>
static bool read_all(std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), stdin) == v.size(); }

template <typename T>
static bool write_all(const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size(); }

template <typename T>
static bool same(const char* what, const std::vector<T>& a, const std::vector<T>& b) {
  if (a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)))) return true;
  size_t k = 0;
  while (k < a.size() && k < b.size() && !memcmp(&a[k], &b[k], sizeof(T))) ++k;
  fprintf(stderr, "icp_host: %s differs between the fused function and the chain, first at element %zu\n", what, k);
  return false;
}

static double f64_from_bits(long long bits) {
  double d;
  memcpy(&d, &bits, sizeof(d));
  return d;
}

static int solve_mode(int argc, char** argv) {
  if (argc != 5) return 2;
  const int Bi = atoi(argv[2]), min_count = atoi(argv[3]);
  const double damping = f64_from_bits(atoll(argv[4]));
  if (Bi < 1 || Bi > 4096) return 2;
  const size_t B = (size_t)Bi;
  std::vector<double> S(B * 32), x(B * 6);
  std::vector<float> T(B * 12);
  std::vector<unsigned char> status(B);
  if (!read_all(S) || !read_all(T)) return 2;
  for (size_t b = 0; b < B; ++b) status[b] = (unsigned char)ud_icp_solve(S.data() + b * 32, damping, min_count, T.data() + b * 12, x.data() + b * 6);
  return write_all(T) && write_all(x) && write_all(status) ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "solve")) {
    const int rc = solve_mode(argc, argv);
    if (rc == 2) fprintf(stderr, "usage: icp_host solve B MIN_COUNT DAMP_BITS < input\n");
    return rc;
  }
  const int fixed = 16;
  long long v0[fixed];
  for (int i = 0; i < fixed; ++i) v0[i] = argc > 2 + i ? atoll(argv[2 + i]) : 0;
  const int Bi = (int)v0[0], H = (int)v0[1], W = (int)v0[2], Hm = (int)v0[3], Wm = (int)v0[4], nT = (int)v0[5], form = (int)v0[6];
  const int has_mask = (int)v0[7], has_w = (int)v0[8], has_n = (int)v0[9], has_cos = (int)v0[10], iters = (int)v0[13], min_count = (int)v0[14];
  bool ok = argc > 1 && !strcmp(argv[1], "run") && Bi >= 1 && Bi <= 256 && H >= 1 && W >= 1 && Hm >= 1 && Wm >= 1 && (nT == 1 || nT == Bi) &&
            (long long)Bi * H * W <= (1 << 24) && (long long)Bi * Hm * Wm <= (1 << 24) && (form == 0 || form == 1) && iters >= 0 && iters <= 64 &&
            (iters == 0 || nT == Bi) && (!has_cos || has_n) && argc == 2 + fixed + 2 * Bi;
  if (!ok) {
    fprintf(stderr, "usage: icp_host run B H W Hm Wm NT FORM HAS_MASK HAS_W HAS_N HAS_COS DIST_BITS COS_BITS ITERS MIN_COUNT DAMP_BITS MF_0.. MM_0.. < input\n");
    return 2;
  }
  int mf[256], mm[256];
  for (int b = 0; b < Bi; ++b) {
    mf[b] = atoi(argv[2 + fixed + b]);
    mm[b] = atoi(argv[2 + fixed + Bi + b]);
    ok = ok && ud_cam_model_ok(mm[b]) && (form == 1 || ud_cam_closed_form(mf[b]));
  }
  if (!ok) {
    fprintf(stderr, "icp_host: bad model tags\n");
    return 2;
  }
  union { int i; float f; } dist, cosv;
  dist.i = (int)v0[11]; cosv.i = (int)v0[12];
  const double damping = f64_from_bits(v0[15]);
  const size_t B = (size_t)Bi, n = (size_t)H * W, hw = (size_t)Hm * Wm;
  std::vector<float> frame(B * (form ? 3 : 1) * n), params(B * 16), weights(has_w ? B * n : 0), normals(has_n ? B * 3 * n : 0);
  std::vector<float> mp(B * 3 * hw), mn(B * 3 * hw), pm(B * 16), T((size_t)nT * 12);
  std::vector<unsigned char> mask(has_mask ? B * n : 0), mv(B * hw);
  if (!read_all(frame) || !read_all(params) || !read_all(mask) || !read_all(weights) || !read_all(normals) || !read_all(mp) || !read_all(mn) ||
      !read_all(mv) || !read_all(pm) || !read_all(T)) {
    fprintf(stderr, "icp_host: short input\n");
    return 2;
  }
  const float tol2 = dist.f * dist.f;

  std::vector<unsigned char> matched(B * n);
  std::vector<float> residual(B * n), rows(B * 6 * n);
  UdIcpArgs a;
  a.depth = form ? nullptr : frame.data(); a.points = form ? frame.data() : nullptr; a.params = params.data();
  a.mask = has_mask ? mask.data() : nullptr; a.weights = has_w ? weights.data() : nullptr; a.normals = has_n ? normals.data() : nullptr;
  a.model_points = mp.data(); a.model_normals = mn.data(); a.model_valid = mv.data(); a.params_model = pm.data(); a.T = T.data();
  a.matched = matched.data(); a.residual = residual.data(); a.rows = rows.data();
  a.n = (long long)n; a.tol2 = tol2; a.cos_tol = cosv.f;
  a.B = Bi; a.H = H; a.W = W; a.Hm = Hm; a.Wm = Wm; a.nT = nT; a.has_cos = has_cos;

  const int K = iters > 0 ? iters : 1;
  std::vector<double> systems((size_t)K * B * 32, 0.0), xs(iters > 0 ? (size_t)K * B * 6 : 0);
  std::vector<unsigned char> status(iters > 0 ? (size_t)K * B : 0), matched0;
  std::vector<float> Ts(iters > 0 ? (size_t)K * B * 12 : 0), residual0, rows0, T0(T);
  for (int it = 0; it < K; ++it) {
    // ---- the fused function and the sums, in pixel order -------------------------------------------------------------------------
    for (int b = 0; b < Bi; ++b) {
      double* S = systems.data() + ((size_t)it * B + b) * 32;
      for (long long i = 0; i < a.n; ++i) {
        UdIcpRow row;
        if (ud_icp_row(a, mf[b], mm[b], b, i, &row)) ud_icp_accumulate(S, row);
      }
    }
    if (it == 0) {
      matched0 = matched; residual0 = residual; rows0 = rows;
    }
    if (iters > 0) {
      for (int b = 0; b < Bi; ++b) {
        const double* S = systems.data() + ((size_t)it * B + b) * 32;
        status[(size_t)it * B + b] = (unsigned char)ud_icp_solve(S, damping, min_count, T.data() + (size_t)b * 12, xs.data() + ((size_t)it * B + b) * 6);
      }
      memcpy(Ts.data() + (size_t)it * B * 12, T.data(), B * 12 * sizeof(float));
    }
  }

  // ---- the chain of the separate functions at the starting T, one pass per launch, every intermediate in memory ----------------------
  std::vector<float> P(B * 3 * n), Q(B * 3 * n), uv(B * 2 * n), dq(B * n);
  std::vector<unsigned char> live(B * n), usable(B * n);
  for (size_t b = 0; b < B; ++b)
    for (size_t i = 0; i < n; ++i) {
      float* p = P.data() + b * 3 * n + i;
      if (form) {
        const float* s = frame.data() + b * 3 * n + i;
        p[0] = s[0]; p[n] = s[n]; p[2 * n] = s[2 * n];
        live[b * n + i] = ud_icp_finite(s[0]) && ud_icp_finite(s[n]) && ud_icp_finite(s[2 * n]);
      } else {
        float r[3];
        ud_cam_unproject_closed(mf[b], UD_UNPROJ_DEPTH, params.data() + b * 16, (float)(i % W) + 0.5f, (float)(i / W) + 0.5f, frame[b * n + i], r);
        p[0] = r[0]; p[n] = r[1]; p[2 * n] = r[2];
        live[b * n + i] = frame[b * n + i] > 0.0f;
      }
    }
  for (size_t k = 0; k < B * n; ++k) live[k] = live[k] && (!has_mask || mask[k] != 0);
  if (has_w)
    for (size_t k = 0; k < B * n; ++k) live[k] = live[k] && weights[k] > 0.0f && ud_icp_finite(weights[k]);
  for (size_t b = 0; b < B; ++b)
    for (size_t i = 0; i < n; ++i) {
      const float* s = P.data() + b * 3 * n + i;
      const float x = s[0], y = s[n], z = s[2 * n];
      const float* t = T0.data() + (nT == 1 ? 0 : b * 12);
      float* q = Q.data() + b * 3 * n + i;
      q[0] = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
      q[n] = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
      q[2 * n] = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
    }
  for (size_t b = 0; b < B; ++b)
    for (size_t i = 0; i < n; ++i) {
      const float* q = Q.data() + b * 3 * n + i;
      float u, w;
      ud_cam_project(mm[b], pm.data() + b * 16, q[0], q[n], q[2 * n], &u, &w);
      uv[b * 2 * n + i] = u; uv[b * 2 * n + n + i] = w;
      dq[b * n + i] = ud_cam_depth(mm[b], q[0], q[n], q[2 * n]);
      usable[b * n + i] = ud_cam_inside(mm[b], u, w, q[2 * n], Hm, Wm) ? 1 : 0;
    }
  for (size_t k = 0; k < B * n; ++k) usable[k] = usable[k] && dq[k] > 0.0f;
  std::vector<float> src(B * 6 * hw), mnq(B * 6 * n);
  std::vector<unsigned char> valid(B * n);
  for (size_t b = 0; b < B; ++b) {
    memcpy(src.data() + b * 6 * hw, mp.data() + b * 3 * hw, 3 * hw * sizeof(float));
    memcpy(src.data() + b * 6 * hw + 3 * hw, mn.data() + b * 3 * hw, 3 * hw * sizeof(float));
  }
  {
    UdRmArgs<float, float> r;
    r.src = src.data(); r.src_mask = mv.data(); r.uv = uv.data(); r.coord_valid = usable.data(); r.out = mnq.data(); r.valid = valid.data();
    r.bs = (long long)(2 * n); r.ps = 1; r.cs = (long long)n; r.n = (long long)n; r.src_bs = (long long)(6 * hw); r.mask_bs = (long long)hw;
    r.C = 6; r.Hs = Hm; r.Ws = Wm; r.mode = UD_RM_NEAREST; r.padding = UD_RM_ZEROS; r.normalize = 0; r.out_rows = 0;
    for (int b = 0; b < Bi; ++b)
      for (long long i = 0; i < r.n; ++i) ud_rm_point(r, b, i);
  }
  std::vector<float> e(B * 3 * n), d2(B * n), res(B * n), g(B * 6 * n), cosn(B * n);
  std::vector<unsigned char> m2(B * n);
  std::vector<float> residual2(B * n), rows2(B * 6 * n);
  for (size_t b = 0; b < B; ++b)
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k < 3; ++k) e[(b * 3 + k) * n + i] = mnq[(b * 6 + k) * n + i] - Q[(b * 3 + k) * n + i];
  for (size_t b = 0; b < B; ++b)
    for (size_t i = 0; i < n; ++i) {
      const float* ee = e.data() + b * 3 * n + i;
      const float* nn = mnq.data() + (b * 6 + 3) * n + i;
      const float* q = Q.data() + b * 3 * n + i;
      d2[b * n + i] = (ee[0] * ee[0] + ee[n] * ee[n]) + ee[2 * n] * ee[2 * n];
      res[b * n + i] = (nn[0] * ee[0] + nn[n] * ee[n]) + nn[2 * n] * ee[2 * n];
      float* gg = g.data() + b * 6 * n + i;
      gg[0] = q[n] * nn[2 * n] - q[2 * n] * nn[n];
      gg[n] = q[2 * n] * nn[0] - q[0] * nn[2 * n];
      gg[2 * n] = q[0] * nn[n] - q[n] * nn[0];
      gg[3 * n] = nn[0]; gg[4 * n] = nn[n]; gg[5 * n] = nn[2 * n];
    }
  for (size_t b = 0; b < B; ++b)
    for (size_t i = 0; i < n; ++i) {
      const float* gg = g.data() + b * 6 * n + i;
      bool m = live[b * n + i] && valid[b * n + i] && (gg[3 * n] != 0.0f || gg[4 * n] != 0.0f || gg[5 * n] != 0.0f) && d2[b * n + i] <= tol2;
      if (has_n && has_cos) {
        const float* t = T0.data() + (nT == 1 ? 0 : b * 12);
        const float* s = normals.data() + b * 3 * n + i;
        const float r0 = (t[0] * s[0] + t[1] * s[n]) + t[2] * s[2 * n], r1 = (t[4] * s[0] + t[5] * s[n]) + t[6] * s[2 * n];
        const float r2 = (t[8] * s[0] + t[9] * s[n]) + t[10] * s[2 * n];
        cosn[b * n + i] = (r0 * gg[3 * n] + r1 * gg[4 * n]) + r2 * gg[5 * n];
        m = m && cosn[b * n + i] >= cosv.f;
      }
      m = m && ud_icp_finite(res[b * n + i]);
      for (size_t k = 0; k < 6; ++k) m = m && ud_icp_finite(gg[k * n]);
      m2[b * n + i] = m ? 1 : 0;
    }
  for (size_t k = 0; k < B * n; ++k) residual2[k] = m2[k] ? res[k] : 0.0f;
  for (size_t b = 0; b < B; ++b)
    for (size_t k = 0; k < 6; ++k)
      for (size_t i = 0; i < n; ++i) rows2[(b * 6 + k) * n + i] = m2[b * n + i] ? g[(b * 6 + k) * n + i] : 0.0f;
  const bool eq = same("matched", matched0, m2) & same("residual", residual0, residual2) & same("rows", rows0, rows2);
  if (!eq) return 3;
  return write_all(matched0) && write_all(residual0) && write_all(rows0) && write_all(P) && write_all(uv) && write_all(systems) && write_all(xs) &&
                 write_all(status) && write_all(Ts) ? 0 : 1;
}
