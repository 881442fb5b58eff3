// TEST INFRASTRUCTURE ONLY: a stand-alone host program around unidepth_amd/csrc/warp_point.h (ud_wp_point), which runs what one thread of
// warp.hip's kernel runs, for every destination pixel, in the kernel's addressing -- and, beside it, the CHAIN of the separate per-point
// functions the fused one is made of, pass by pass with every intermediate stored in memory as the separate kernels store it:
// ud_cam_unproject_closed (unproject.hip), the rigid motion + ud_cam_project + ud_cam_inside + ud_cam_depth (project.hip), the validity
// `inside & (depth > 0) ...`, ud_rm_point for the source and again for the source's depth (remap.hip), and the visibility comparison.  Both
// must give the same bits in every output; the program exits 3 otherwise.  So tests/test_warp_cpu.py can check the fusion without a GPU,
// under the host sanitizers: every array is allocated exactly as large as its contents, so an index that escapes is an AddressSanitizer
// report, and a float-to-int conversion of an unsafe coordinate is an UBSan report.
//
//   warp_host MODE PADDING NORMALIZE SRC_U8 OUT_U8 FORM B C Ho Wo Hs Ws SRC_B MASK_B SD_B NT HAS_VIN TOL_BITS DST_0..DST_B-1 SRC_0..SRC_B-1 < input
//       MODE 0 nearest, 1 bilinear; PADDING 0 zeros, 1 border; FORM 0 points, 1 depth; SRC_B 1 (shared) or B; MASK_B / SD_B 0 (none), 1
//       or B; NT 0 (no transform), 1 or B; TOL_BITS the bit pattern of the fp32 tolerance; DST_b / SRC_b the model tags (DST_b is not
//       read in the points form).
//       input, binary: src [SRC_B,C,Hs,Ws] (float32 or bytes), mask [MASK_B,Hs,Ws] bytes, src_depth [SD_B,Hs,Ws] float32, points
//       [B,3,Ho,Wo] or depth [B,Ho,Wo] float32, params_dst [B,16] float32 (depth form only), params_src [B,16] float32, T [NT,3,4]
//       float32, valid_in [B,Ho,Wo] bytes.
//       output: out [B,C,Ho,Wo] (float32 or bytes), valid [B,Ho,Wo] bytes, visible [B,Ho,Wo] bytes (with SD_B), uv [B,2,Ho,Wo] float32,
//       proj_depth [B,Ho,Wo] float32 -- the fused function's.
//
// Never loaded by the product.
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
  fprintf(stderr, "warp_host: %s differs between the fused function and the chain, first at element %zu\n", what, k);
  return false;
}

struct Opt {
  int mode, padding, normalize, form, B, C, Ho, Wo, Hs, Ws, src_b, mask_b, sd_b, nT, has_vin, tol_bits;
  int model_dst[256], model_src[256];
};

template <typename S, typename O>
static int run(const Opt& o) {
  const size_t hw = (size_t)o.Hs * o.Ws, n = (size_t)o.Ho * o.Wo, B = (size_t)o.B;
  std::vector<S> src((size_t)o.src_b * o.C * hw);
  std::vector<unsigned char> mask((size_t)o.mask_b * hw), vin(o.has_vin ? B * n : 0);
  std::vector<float> sd((size_t)o.sd_b * hw), geo(B * n * (o.form ? 1 : 3)), pd(o.form ? B * 16 : 0), ps(B * 16), T((size_t)o.nT * 12);
  if (!read_all(src) || !read_all(mask) || !read_all(sd) || !read_all(geo) || !read_all(pd) || !read_all(ps) || !read_all(T) || !read_all(vin)) {
    fprintf(stderr, "warp_host: short input\n");
    return 2;
  }
  union { int i; float f; } tol;
  tol.i = o.tol_bits;

  // ---- the fused function --------------------------------------------------------------------------------------------------------
  std::vector<O> out(B * o.C * n);
  std::vector<unsigned char> valid(B * n), visible(o.sd_b ? B * n : 0);
  std::vector<float> uv(B * 2 * n), dproj(B * n);
  UdWpArgs<S, O> a;
  a.src = src.data(); a.src_mask = o.mask_b ? mask.data() : nullptr; a.src_depth = o.sd_b ? sd.data() : nullptr;
  a.points = o.form ? nullptr : geo.data(); a.depth = o.form ? geo.data() : nullptr;
  a.params_dst = o.form ? pd.data() : nullptr; a.params_src = ps.data(); a.T = o.nT ? T.data() : nullptr;
  a.valid_in = o.has_vin ? vin.data() : nullptr;
  a.out = out.data(); a.valid = valid.data(); a.visible = o.sd_b ? visible.data() : nullptr; a.uv = uv.data(); a.proj_depth = dproj.data();
  a.n = (long long)n; a.src_bs = o.src_b == 1 ? 0 : (long long)o.C * (long long)hw; a.mask_bs = o.mask_b == 1 ? 0 : (long long)hw;
  a.sdepth_bs = o.sd_b == 1 ? 0 : (long long)hw;
  a.tol = tol.f;
  a.C = o.C; a.Wo = o.Wo; a.Hs = o.Hs; a.Ws = o.Ws; a.nT = o.nT; a.mode = o.mode; a.padding = o.padding; a.normalize = o.normalize;
  for (int b = 0; b < o.B; ++b)
    for (long long i = 0; i < a.n; ++i) ud_wp_point(a, o.model_dst[b], o.model_src[b], b, i);

  // ---- the chain of the separate functions, one pass per kernel, every intermediate in memory -------------------------------------
  std::vector<float> pts;
  if (o.form) {                                                             // unproject.hip: up_load + ud_cam_unproject_closed + up_store
    pts.resize(B * 3 * n);
    for (size_t b = 0; b < B; ++b)
      for (size_t i = 0; i < n; ++i) {
        const int y = (int)i / o.Wo, x = (int)i - y * o.Wo;
        float r[3];
        ud_cam_unproject_closed(o.model_dst[b], UD_UNPROJ_DEPTH, pd.data() + b * 16, (float)x + 0.5f, (float)y + 0.5f, geo[b * n + i], r);
        float* q = pts.data() + b * 3 * n + i;
        q[0] = r[0]; q[n] = r[1]; q[2 * n] = r[2];
      }
  }
  const std::vector<float>& xyz = o.form ? pts : geo;
  std::vector<float> uv2(B * 2 * n), dproj2(B * n);
  std::vector<unsigned char> cv(B * n);
  for (size_t b = 0; b < B; ++b)                                             // project.hip: pj_project_kernel<false>
    for (size_t i = 0; i < n; ++i) {
      const float* s = xyz.data() + b * 3 * n + i;
      float x = s[0], y = s[n], z = s[2 * n];
      if (o.nT) {
        const float* t = T.data() + (o.nT == 1 ? 0 : b * 12);
        const float xt = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
        const float yt = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
        const float zt = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
        x = xt; y = yt; z = zt;
      }
      float u, v;
      ud_cam_project(o.model_src[b], ps.data() + b * 16, x, y, z, &u, &v);
      uv2[b * 2 * n + i] = u; uv2[b * 2 * n + n + i] = v;
      const bool inside = ud_cam_inside(o.model_src[b], u, v, z, o.Hs, o.Ws);
      dproj2[b * n + i] = ud_cam_depth(o.model_src[b], x, y, z);
      // inside & (depth > 0) [& valid_in] [& (destination depth > 0)]: the element-wise operations between the launches
      cv[b * n + i] = inside && dproj2[b * n + i] > 0.0f && (!o.has_vin || vin[b * n + i] != 0) && (!o.form || geo[b * n + i] > 0.0f);
    }
  std::vector<O> out2(B * o.C * n);
  std::vector<unsigned char> valid2(B * n), visible2(o.sd_b ? B * n : 0);
  {
    UdRmArgs<S, O> r;                                                       // remap.hip: rm_remap_kernel on the planar coordinate map
    r.src = src.data(); r.src_mask = o.mask_b ? mask.data() : nullptr; r.uv = uv2.data(); r.coord_valid = cv.data();
    r.out = out2.data(); r.valid = valid2.data();
    r.bs = 2 * (long long)n; r.ps = 1; r.cs = (long long)n; r.n = (long long)n; r.src_bs = a.src_bs; r.mask_bs = a.mask_bs;
    r.C = o.C; r.Hs = o.Hs; r.Ws = o.Ws; r.mode = o.mode; r.padding = o.padding; r.normalize = o.normalize; r.out_rows = 0;
    for (int b = 0; b < o.B; ++b)
      for (long long i = 0; i < r.n; ++i) ud_rm_point(r, b, i);
  }
  if (o.sd_b) {                                                             // the same sampler on the source's depth, normalised
    std::vector<unsigned char> dmask(B * hw);
    for (size_t b = 0; b < B; ++b)
      for (size_t j = 0; j < hw; ++j)
        dmask[b * hw + j] = sd[(o.sd_b == 1 ? 0 : b * hw) + j] > 0.0f && (!o.mask_b || mask[(o.mask_b == 1 ? 0 : b * hw) + j] != 0);
    std::vector<float> ds(B * n);
    std::vector<unsigned char> dv(B * n);
    UdRmArgs<float, float> r;
    r.src = sd.data(); r.src_mask = dmask.data(); r.uv = uv2.data(); r.coord_valid = cv.data(); r.out = ds.data(); r.valid = dv.data();
    r.bs = 2 * (long long)n; r.ps = 1; r.cs = (long long)n; r.n = (long long)n; r.src_bs = a.sdepth_bs; r.mask_bs = (long long)hw;
    r.C = 1; r.Hs = o.Hs; r.Ws = o.Ws; r.mode = o.mode; r.padding = o.padding; r.normalize = 1; r.out_rows = 0;
    for (int b = 0; b < o.B; ++b)
      for (long long i = 0; i < r.n; ++i) ud_rm_point(r, b, i);
    for (size_t k = 0; k < B * n; ++k) {
      const float diff = fabsf(ds[k] - dproj2[k]), bar = tol.f * dproj2[k];
      visible2[k] = (dv[k] && diff <= bar) ? 1 : 0;
    }
  }
  const bool ok = same("out", out, out2) & same("valid", valid, valid2) & same("visible", visible, visible2) & same("uv", uv, uv2) &
                  same("proj_depth", dproj, dproj2);
  if (!ok) return 3;
  return write_all(out) && write_all(valid) && write_all(visible) && write_all(uv) && write_all(dproj) ? 0 : 1;
}

int main(int argc, char** argv) {
  Opt o;
  memset(&o, 0, sizeof(o));
  const int fixed = 18;
  int B = argc > 7 ? atoi(argv[7]) : 0;
  if (B < 1 || B > 256 || argc != 1 + fixed + 2 * B) {
    fprintf(stderr, "usage: warp_host MODE PADDING NORMALIZE SRC_U8 OUT_U8 FORM B C Ho Wo Hs Ws SRC_B MASK_B SD_B NT HAS_VIN TOL_BITS DST_0.. SRC_0.. < input\n");
    return 2;
  }
  int v[fixed];
  for (int i = 0; i < fixed; ++i) v[i] = atoi(argv[1 + i]);
  const int src_u8 = v[3], out_u8 = v[4];
  o.mode = v[0]; o.padding = v[1]; o.normalize = v[2]; o.form = v[5]; o.B = v[6]; o.C = v[7]; o.Ho = v[8]; o.Wo = v[9]; o.Hs = v[10]; o.Ws = v[11];
  o.src_b = v[12]; o.mask_b = v[13]; o.sd_b = v[14]; o.nT = v[15]; o.has_vin = v[16]; o.tol_bits = v[17];
  bool ok = (o.mode == UD_RM_NEAREST || o.mode == UD_RM_BILINEAR) && (o.padding == UD_RM_ZEROS || o.padding == UD_RM_BORDER) &&
            (o.form == 0 || o.form == 1) && o.C >= 1 && o.Ho >= 1 && o.Wo >= 1 && o.Hs >= 1 && o.Ws >= 1 &&
            (long long)o.B * o.C * o.Ho * o.Wo <= (1 << 26) && (long long)o.C * o.Hs * o.Ws <= (1 << 26) && (o.src_b == 1 || o.src_b == o.B) &&
            (o.mask_b == 0 || o.mask_b == 1 || o.mask_b == o.B) && (o.sd_b == 0 || o.sd_b == 1 || o.sd_b == o.B) &&
            (o.nT == 0 || o.nT == 1 || o.nT == o.B) && (!out_u8 || src_u8);
  for (int b = 0; b < o.B; ++b) {
    o.model_dst[b] = atoi(argv[1 + fixed + b]);
    o.model_src[b] = atoi(argv[1 + fixed + o.B + b]);
    ok = ok && o.model_src[b] >= UD_CAM_PINHOLE && o.model_src[b] <= UD_CAM_MEI;
    // the fused function takes the closed-form destinations only (the entry point refuses the others)
    if (o.form) ok = ok && (o.model_dst[b] == UD_CAM_PINHOLE || o.model_dst[b] == UD_CAM_EUCM || o.model_dst[b] == UD_CAM_SPHERICAL || o.model_dst[b] == UD_CAM_MEI);
  }
  if (!ok) {
    fprintf(stderr, "warp_host: bad arguments\n");
    return 2;
  }
  if (!src_u8) return run<float, float>(o);
  return out_u8 ? run<unsigned char, unsigned char>(o) : run<unsigned char, float>(o);
}
