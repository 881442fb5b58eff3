// TEST INFRASTRUCTURE ONLY: a stand-alone host program around unidepth_amd/csrc/consistency_point.h (ud_cs_point), which runs what one
// thread of consistency.hip's kernel runs, for every reference pixel, in the kernel's addressing -- and, beside it, the CHAIN of the
// unchanged per-point functions the fused one is made of, view by view and pass by pass with every intermediate stored in memory as the
// separate launches store it: ud_wp_point (warp.hip) on the view's depth with the mask `depth > 0 [& src_mask]`, normalised, giving the
// sample, its validity and (u, v); ud_cam_unproject_closed (unproject.hip) at (u, v) with the sample; the rigid motion + ud_cam_project +
// ud_cam_inside + ud_cam_depth (project.hip) with the inverse; then one loop per element-wise operation.  Both must give the same bits
// in every output; the program exits 3 otherwise.  So tests/test_consistency_cpu.py can check the fusion without a GPU, under the host
// sanitizers: every array is allocated exactly as large as its contents, so an index that escapes is an AddressSanitizer report, and a
// float-to-int conversion of an unsafe coordinate is an UBSan report.
//
//   consistency_host B V H W Hs Ws NT HAS_VIN HAS_MASK MIN_VIEWS PX_TOL_BITS REL_TOL_BITS REF_0..REF_B-1 SRC_0..SRC_V*B-1 < input
//       NT 1 or B sets of V matrices; the tolerances as fp32 bit patterns; REF_b the reference's model tags, SRC_(v * B + b) the views'.
//       input, binary: depth [B,H,W] float32, params_ref [B,16] float32, src_depth [B,V,Hs,Ws] float32, src_mask [B,V,Hs,Ws] bytes (with
//       HAS_MASK), params_src [V,B,16] float32, T [NT,V,3,4] float32, Tinv [NT,V,3,4] float32, valid_in [B,H,W] bytes (with HAS_VIN).
//       output: fused [B,H,W] float32, count [B,H,W] bytes, mask [B,H,W] bytes, consistent [B,V,H,W] bytes, err_px [B,V,H,W] float32,
//       err_rel [B,V,H,W] float32 -- the fused function's.
//
// Never loaded by the product.
#include "../../unidepth_amd/csrc/consistency_point.h"
#include "../../unidepth_amd/csrc/warp_point.h"
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
  fprintf(stderr, "consistency_host: %s differs between the fused function and the chain, first at element %zu\n", what, k);
  return false;
}

static bool closed(int m) { return m == UD_CAM_PINHOLE || m == UD_CAM_EUCM || m == UD_CAM_SPHERICAL || m == UD_CAM_MEI; }

int main(int argc, char** argv) {
  const int fixed = 12;
  int v0[fixed];
  for (int i = 0; i < fixed; ++i) v0[i] = argc > 1 + i ? atoi(argv[1 + i]) : 0;
  const int Bi = v0[0], V = v0[1], H = v0[2], W = v0[3], Hs = v0[4], Ws = v0[5], nT = v0[6], has_vin = v0[7], has_mask = v0[8], min_views = v0[9];
  bool ok = Bi >= 1 && V >= 1 && V <= 255 && Bi * V <= 256 && H >= 1 && W >= 1 && Hs >= 1 && Ws >= 1 && (nT == 1 || nT == Bi) &&
            (long long)Bi * V * H * W <= (1 << 26) && (long long)Bi * V * Hs * Ws <= (1 << 26) && min_views >= 0 && min_views <= V &&
            argc == 1 + fixed + Bi + V * Bi;
  if (!ok) {
    fprintf(stderr, "usage: consistency_host B V H W Hs Ws NT HAS_VIN HAS_MASK MIN_VIEWS PX_TOL_BITS REL_TOL_BITS REF_0.. SRC_0.. < input\n");
    return 2;
  }
  int model_ref[256];
  unsigned char model_src[256];
  for (int b = 0; b < Bi; ++b) {
    model_ref[b] = atoi(argv[1 + fixed + b]);
    ok = ok && closed(model_ref[b]);
  }
  for (int k = 0; k < V * Bi; ++k) {
    const int m = atoi(argv[1 + fixed + Bi + k]);
    ok = ok && closed(m);                              // the fused function takes the closed-form models only (the entry point refuses the others)
    model_src[k] = (unsigned char)m;
  }
  if (!ok) {
    fprintf(stderr, "consistency_host: bad model tags\n");
    return 2;
  }
  union { int i; float f; } px, rel;
  px.i = v0[10]; rel.i = v0[11];
  const size_t B = (size_t)Bi, n = (size_t)H * W, hw = (size_t)Hs * Ws;
  std::vector<float> depth(B * n), pr(B * 16), sd(B * V * hw), ps((size_t)V * B * 16), T((size_t)nT * V * 12), Tinv((size_t)nT * V * 12);
  std::vector<unsigned char> mask(has_mask ? B * V * hw : 0), vin(has_vin ? B * n : 0);
  if (!read_all(depth) || !read_all(pr) || !read_all(sd) || !read_all(mask) || !read_all(ps) || !read_all(T) || !read_all(Tinv) || !read_all(vin)) {
    fprintf(stderr, "consistency_host: short input\n");
    return 2;
  }
  const float tol2 = px.f * px.f;

  // ---- the fused function --------------------------------------------------------------------------------------------------------
  std::vector<float> fused(B * n), epx(B * V * n), erel(B * V * n);
  std::vector<unsigned char> count(B * n), okmask(B * n), cons(B * V * n);
  UdCsArgs a;
  a.depth = depth.data(); a.params_ref = pr.data(); a.valid_in = has_vin ? vin.data() : nullptr;
  a.src_depth = sd.data(); a.src_mask = has_mask ? mask.data() : nullptr; a.params_src = ps.data(); a.T = T.data(); a.Tinv = Tinv.data();
  a.fused = fused.data(); a.count = count.data(); a.mask = okmask.data(); a.consistent = cons.data(); a.err_px = epx.data(); a.err_rel = erel.data();
  a.n = (long long)n; a.tol2 = tol2; a.rel_tol = rel.f;
  a.B = Bi; a.V = V; a.H = H; a.W = W; a.Hs = Hs; a.Ws = Ws; a.nT = nT; a.min_views = min_views;
  for (int b = 0; b < Bi; ++b)
    for (long long i = 0; i < a.n; ++i) ud_cs_point(a, model_ref[b], model_src, b, i);

  // ---- the chain of the separate functions, one pass per launch, every intermediate in memory -------------------------------------
  std::vector<float> fused2(B * n), epx2(B * V * n), erel2(B * V * n), total(depth), bar(B * n);
  std::vector<unsigned char> count2(B * n, 0), okmask2(B * n), cons2(B * V * n), ref_ok(B * n);
  for (size_t k = 0; k < B * n; ++k) ref_ok[k] = depth[k] > 0.0f && (!has_vin || vin[k] != 0);
  for (size_t k = 0; k < B * n; ++k) bar[k] = depth[k] * rel.f;
  for (int v = 0; v < V; ++v) {
    // the view's own contiguous maps and matrices, as a caller slices them
    std::vector<float> sdv(B * hw), Tv((size_t)nT * 12), Tiv((size_t)nT * 12);
    std::vector<unsigned char> dmask(B * hw);
    for (size_t b = 0; b < B; ++b)
      for (size_t j = 0; j < hw; ++j) {
        sdv[b * hw + j] = sd[(b * V + v) * hw + j];
        dmask[b * hw + j] = sdv[b * hw + j] > 0.0f && (!has_mask || mask[(b * V + v) * hw + j] != 0);
      }
    for (int t = 0; t < nT; ++t)
      for (int e = 0; e < 12; ++e) {
        Tv[(size_t)t * 12 + e] = T[((size_t)t * V + v) * 12 + e];
        Tiv[(size_t)t * 12 + e] = Tinv[((size_t)t * V + v) * 12 + e];
      }
    const float* psv = ps.data() + (size_t)v * B * 16;
    // warp.hip: the view's depth fetched at every reference pixel, normalised, with its validity and (u, v)
    std::vector<float> ds(B * n), uv(B * 2 * n);
    std::vector<unsigned char> sampled(B * n);
    {
      UdWpArgs<float, float> w;
      w.src = sdv.data(); w.src_mask = dmask.data(); w.src_depth = nullptr;
      w.points = nullptr; w.depth = depth.data(); w.params_dst = pr.data(); w.params_src = psv; w.T = Tv.data();
      w.valid_in = has_vin ? vin.data() : nullptr;
      w.out = ds.data(); w.valid = sampled.data(); w.visible = nullptr; w.uv = uv.data(); w.proj_depth = nullptr;
      w.n = (long long)n; w.src_bs = (long long)hw; w.mask_bs = (long long)hw; w.sdepth_bs = 0;
      w.tol = 0.0f;
      w.C = 1; w.Wo = W; w.Hs = Hs; w.Ws = Ws; w.nT = nT; w.mode = UD_RM_BILINEAR; w.padding = UD_RM_ZEROS; w.normalize = 1;
      for (int b = 0; b < Bi; ++b)
        for (long long i = 0; i < w.n; ++i) ud_wp_point(w, model_ref[b], model_src[v * Bi + b], b, i);
    }
    // unproject.hip: the sample lifted through the view's camera at (u, v)
    std::vector<float> lifted(B * 3 * n);
    for (size_t b = 0; b < B; ++b)
      for (size_t i = 0; i < n; ++i) {
        float r[3];
        ud_cam_unproject_closed(model_src[v * Bi + b], UD_UNPROJ_DEPTH, psv + b * 16, uv[b * 2 * n + i], uv[b * 2 * n + n + i], ds[b * n + i], r);
        float* q = lifted.data() + b * 3 * n + i;
        q[0] = r[0]; q[n] = r[1]; q[2 * n] = r[2];
      }
    // project.hip: brought home with the inverse and projected through the reference camera
    std::vector<float> uv2(B * 2 * n), dback(B * n);
    std::vector<unsigned char> inside(B * n);
    for (size_t b = 0; b < B; ++b)
      for (size_t i = 0; i < n; ++i) {
        const float* s = lifted.data() + b * 3 * n + i;
        float x = s[0], y = s[n], z = s[2 * n];
        const float* t = Tiv.data() + (nT == 1 ? 0 : b * 12);
        const float xt = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
        const float yt = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
        const float zt = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
        x = xt; y = yt; z = zt;
        float u, w;
        ud_cam_project(model_ref[b], pr.data() + b * 16, x, y, z, &u, &w);
        uv2[b * 2 * n + i] = u; uv2[b * 2 * n + n + i] = w;
        inside[b * n + i] = ud_cam_inside(model_ref[b], u, w, z, H, W) ? 1 : 0;
        dback[b * n + i] = ud_cam_depth(model_ref[b], x, y, z);
      }
    // the element-wise operations between and after the launches, one loop each
    std::vector<float> du(B * n), dv(B * n), du2(B * n), dv2(B * n), e2(B * n), diff(B * n), root(B * n), quot(B * n), next(B * n);
    std::vector<unsigned char> c(B * n);
    for (size_t b = 0; b < B; ++b)
      for (size_t i = 0; i < n; ++i) du[b * n + i] = uv2[b * 2 * n + i] - ((float)(i % W) + 0.5f);
    for (size_t b = 0; b < B; ++b)
      for (size_t i = 0; i < n; ++i) dv[b * n + i] = uv2[b * 2 * n + n + i] - ((float)(i / W) + 0.5f);
    for (size_t k = 0; k < B * n; ++k) du2[k] = du[k] * du[k];
    for (size_t k = 0; k < B * n; ++k) dv2[k] = dv[k] * dv[k];
    for (size_t k = 0; k < B * n; ++k) e2[k] = du2[k] + dv2[k];
    for (size_t k = 0; k < B * n; ++k) diff[k] = fabsf(dback[k] - depth[k]);
    for (size_t k = 0; k < B * n; ++k) c[k] = sampled[k] && inside[k] && dback[k] > 0.0f && e2[k] <= tol2 && diff[k] <= bar[k];
    for (size_t k = 0; k < B * n; ++k) next[k] = total[k] + dback[k];
    for (size_t k = 0; k < B * n; ++k) total[k] = c[k] ? next[k] : total[k];
    for (size_t k = 0; k < B * n; ++k) count2[k] = (unsigned char)(count2[k] + c[k]);
    for (size_t k = 0; k < B * n; ++k) root[k] = sqrtf(e2[k]);
    for (size_t k = 0; k < B * n; ++k) quot[k] = diff[k] / depth[k];
    for (size_t b = 0; b < B; ++b)
      for (size_t i = 0; i < n; ++i) {
        const size_t k = b * n + i, o = (b * V + v) * n + i;
        cons2[o] = c[k];
        epx2[o] = sampled[k] ? root[k] : 0.0f;
        erel2[o] = sampled[k] ? quot[k] : 0.0f;
      }
  }
  for (size_t k = 0; k < B * n; ++k) fused2[k] = ref_ok[k] ? total[k] / ((float)count2[k] + 1.0f) : 0.0f;
  for (size_t k = 0; k < B * n; ++k) okmask2[k] = ref_ok[k] && count2[k] >= min_views;

  const bool eq = same("fused", fused, fused2) & same("count", count, count2) & same("mask", okmask, okmask2) & same("consistent", cons, cons2) &
                  same("err_px", epx, epx2) & same("err_rel", erel, erel2);
  if (!eq) return 3;
  return write_all(fused) && write_all(count) && write_all(okmask) && write_all(cons) && write_all(epx) && write_all(erel) ? 0 : 1;
}
