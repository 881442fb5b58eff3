// TEST INFRASTRUCTURE ONLY: a stand-alone host program around unidepth_amd/csrc/tsdf_point.h.  It runs ud_tsdf_voxel, what one thread of
// tsdf.hip's integration kernel runs, for every voxel, in the kernel's addressing -- and, beside it, the CHAIN of the unchanged per-point
// functions the fused one is made of, view by view and pass by pass with every intermediate stored in memory as the separate launches store
// it: the voxel centres as rows; the rigid motion + ud_cam_project + ud_cam_inside + ud_cam_depth (project.hip); ud_rm_point (remap.hip),
// nearest, on the view's depth with the mask `depth > 0 [& src_mask]` and coord_valid = inside, and again on the weights and the colours;
// then one loop per element-wise operation.  Both must give the same bits in every output; the program exits 3 otherwise.  Then it runs
// ud_tsdf_slot on the resulting volume for every slot and writes the flags and payloads, which tests/tsdf_common.py compares with its numpy
// restatement.  So tests/test_tsdf_cpu.py can check the fusion without a GPU, under the host sanitizers: every array is allocated exactly
// as large as its contents, so an index that escapes is an AddressSanitizer report, and a float-to-int conversion of an unsafe coordinate
// is an UBSan report.
//
//   tsdf_host B V Nz Ny Nx Hs Ws NT NO HAS_MASK HAS_WEIGHT HAS_IMAGE FRESH HAS_MAX VS_BITS TRUNC_BITS MAXW_BITS MINW_BITS MODEL_0..MODEL_V*B-1
//       NT 1 or B sets of V matrices, NO 1 or B origins; the scalars as fp32 bit patterns; MODEL_(v * B + b) the views' model tags.
//       input, binary: src_depth [B,V,Hs,Ws] float32, src_mask [B,V,Hs,Ws] bytes (HAS_MASK), src_weight [B,V,Hs,Ws] float32 (HAS_WEIGHT),
//       image [B,V,3,Hs,Ws] bytes (HAS_IMAGE), params [V,B,16] float32, T [NT,V,3,4] float32, origin [NO,3] float32, and without FRESH the
//       volume: tsdf [B,n] float32, weight [B,n] float32, color [B,3,n] float32 (HAS_IMAGE).  n = Nz * Ny * Nx.
//       output: tsdf [B,n] float32, weight [B,n] float32, color [B,3,n] float32 (HAS_IMAGE), count [B,n] bytes -- the fused function's --
//       then of that volume at MINW: live [B,3n] bytes, xyz [B,3n,3] float32, and with HAS_IMAGE rgb [B,3n,3] float32 and its rounding to
//       bytes [B,3n,3]; rows of slots that are not live are 0.
//
// Never loaded by the product.
#include "../../unidepth_amd/csrc/tsdf_point.h"
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
  fprintf(stderr, "tsdf_host: %s differs between the fused function and the chain, first at element %zu\n", what, k);
  return false;
}

static float from_bits(int i) {
  float f;
  memcpy(&f, &i, 4);
  return f;
}

int main(int argc, char** argv) {
  const int fixed = 18;
  int v0[fixed];
  for (int i = 0; i < fixed; ++i) v0[i] = argc > 1 + i ? atoi(argv[1 + i]) : 0;
  const int Bi = v0[0], V = v0[1], Nz = v0[2], Ny = v0[3], Nx = v0[4], Hs = v0[5], Ws = v0[6], nT = v0[7], nO = v0[8];
  const int has_mask = v0[9], has_weight = v0[10], has_image = v0[11], fresh = v0[12], has_max = v0[13];
  bool ok = Bi >= 1 && V >= 1 && V <= 255 && Bi * V <= 256 && Nz >= 1 && Ny >= 1 && Nx >= 1 && Hs >= 1 && Ws >= 1 && (nT == 1 || nT == Bi) &&
            (nO == 1 || nO == Bi) && (long long)Bi * Nz * Ny * Nx <= (1 << 24) && (long long)Bi * V * Hs * Ws <= (1 << 24) &&
            argc == 1 + fixed + V * Bi;
  if (!ok) {
    fprintf(stderr, "usage: tsdf_host B V Nz Ny Nx Hs Ws NT NO HAS_MASK HAS_WEIGHT HAS_IMAGE FRESH HAS_MAX VS_BITS TRUNC_BITS MAXW_BITS MINW_BITS MODEL_0.. < input\n");
    return 2;
  }
  unsigned char model[256];
  for (int k = 0; k < V * Bi; ++k) {
    const int m = atoi(argv[1 + fixed + k]);
    ok = ok && ud_cam_model_ok(m);
    model[k] = (unsigned char)m;
  }
  const float vs = from_bits(v0[14]), trunc = from_bits(v0[15]), max_w = from_bits(v0[16]), min_w = from_bits(v0[17]);
  if (!ok || !(vs > 0.0f) || !(trunc > 0.0f) || (has_max && !(max_w > 0.0f))) {
    fprintf(stderr, "tsdf_host: bad model tags or scalars\n");
    return 2;
  }
  const size_t B = (size_t)Bi, n = (size_t)Nz * Ny * Nx, hw = (size_t)Hs * Ws;
  std::vector<float> sd(B * V * hw), sw(has_weight ? B * V * hw : 0), ps((size_t)V * B * 16), T((size_t)nT * V * 12), origin((size_t)nO * 3);
  std::vector<unsigned char> mask(has_mask ? B * V * hw : 0), image(has_image ? B * V * 3 * hw : 0);
  std::vector<float> tsdf0(fresh ? 0 : B * n), w0(fresh ? 0 : B * n), c0((fresh || !has_image) ? 0 : B * 3 * n);
  if (!read_all(sd) || !read_all(mask) || !read_all(sw) || !read_all(image) || !read_all(ps) || !read_all(T) || !read_all(origin) ||
      !read_all(tsdf0) || !read_all(w0) || !read_all(c0)) {
    fprintf(stderr, "tsdf_host: short input\n");
    return 2;
  }

  // ---- the fused function: fresh volumes start from poisoned memory, which must not be read ------------------------------------------
  std::vector<float> tsdf(B * n), W(B * n), color(has_image ? B * 3 * n : 0);
  std::vector<unsigned char> count(B * n);
  if (fresh) {
    for (auto& x : tsdf) x = from_bits(0x7fc00001);
    for (auto& x : W) x = from_bits(0x7fc00002);
    for (auto& x : color) x = from_bits(0x7fc00003);
  } else {
    tsdf = tsdf0; W = w0; color = c0;
  }
  UdTsdfArgs a;
  a.src_depth = sd.data(); a.src_mask = has_mask ? mask.data() : nullptr; a.src_weight = has_weight ? sw.data() : nullptr;
  a.image = has_image ? image.data() : nullptr; a.params = ps.data(); a.T = T.data(); a.origin = origin.data();
  a.tsdf = tsdf.data(); a.weight = W.data(); a.color = has_image ? color.data() : nullptr; a.count = count.data();
  a.n = (long long)n; a.vs = vs; a.trunc = trunc; a.max_weight = max_w;
  a.B = Bi; a.V = V; a.Nx = Nx; a.Ny = Ny; a.Nz = Nz; a.Hs = Hs; a.Ws = Ws; a.nT = nT; a.nO = nO; a.fresh = fresh; a.has_max = has_max;
  for (int b = 0; b < Bi; ++b)
    for (long long i = 0; i < a.n; ++i) ud_tsdf_voxel(a, model, b, i);

  // ---- the chain of the separate functions, one pass per launch, every intermediate in memory -------------------------------------
  std::vector<float> tsdf2(B * n, 1.0f), W2(B * n, 0.0f), color2(has_image ? B * 3 * n : 0, 0.0f);
  std::vector<unsigned char> count2(B * n, 0);
  if (!fresh) {
    tsdf2 = tsdf0; W2 = w0; color2 = c0;
  }
  // the voxel centres as rows [B,n,3]: origin + (index + 0.5) * vs, one operation per pass
  std::vector<float> P(B * n * 3);
  {
    std::vector<float> cx(Nx), cy(Ny), cz(Nz);
    for (int k = 0; k < Nx; ++k) cx[k] = ((float)k + 0.5f) * vs;
    for (int k = 0; k < Ny; ++k) cy[k] = ((float)k + 0.5f) * vs;
    for (int k = 0; k < Nz; ++k) cz[k] = ((float)k + 0.5f) * vs;
    for (size_t b = 0; b < B; ++b) {
      const float* o = origin.data() + (nO == 1 ? 0 : b * 3);
      for (size_t i = 0; i < n; ++i) {
        const size_t ix = i % Nx, iy = (i / Nx) % Ny, iz = i / ((size_t)Nx * Ny);
        float* q = P.data() + (b * n + i) * 3;
        q[0] = o[0] + cx[ix]; q[1] = o[1] + cy[iy]; q[2] = o[2] + cz[iz];
      }
    }
  }
  for (int v = 0; v < V; ++v) {
    // the view's own contiguous maps and matrices, as a caller slices them
    std::vector<float> sdv(B * hw), swv(has_weight ? B * hw : 0), Tv((size_t)nT * 12);
    std::vector<unsigned char> dmask(B * hw), imv(has_image ? B * 3 * hw : 0);
    for (size_t b = 0; b < B; ++b) {
      for (size_t j = 0; j < hw; ++j) {
        sdv[b * hw + j] = sd[(b * V + v) * hw + j];
        dmask[b * hw + j] = sdv[b * hw + j] > 0.0f && (!has_mask || mask[(b * V + v) * hw + j] != 0);
        if (has_weight) swv[b * hw + j] = sw[(b * V + v) * hw + j];
      }
      if (has_image)
        for (size_t j = 0; j < 3 * hw; ++j) imv[b * 3 * hw + j] = image[(b * V + v) * 3 * hw + j];
    }
    for (int t = 0; t < nT; ++t)
      for (int e = 0; e < 12; ++e) Tv[(size_t)t * 12 + e] = T[((size_t)t * V + v) * 12 + e];
    const float* psv = ps.data() + (size_t)v * B * 16;
    // project.hip: the centres moved into the view and projected: uv rows, inside, depth
    std::vector<float> uv(B * n * 2), d(B * n);
    std::vector<unsigned char> inside(B * n);
    for (size_t b = 0; b < B; ++b)
      for (size_t i = 0; i < n; ++i) {
        const float* s = P.data() + (b * n + i) * 3;
        float x = s[0], y = s[1], z = s[2];
        const float* t = Tv.data() + (nT == 1 ? 0 : b * 12);
        const float xt = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
        const float yt = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
        const float zt = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
        x = xt; y = yt; z = zt;
        const int m = model[v * Bi + (int)b];
        float u, w;
        ud_cam_project(m, psv + b * 16, x, y, z, &u, &w);
        uv[(b * n + i) * 2] = u; uv[(b * n + i) * 2 + 1] = w;
        inside[b * n + i] = ud_cam_inside(m, u, w, z, Hs, Ws) ? 1 : 0;
        d[b * n + i] = ud_cam_depth(m, x, y, z);
      }
    // remap.hip, nearest: the depth with its validity, the weights, the colours
    std::vector<float> ds(B * n), wv(B * n, 1.0f), rgb(has_image ? B * n * 3 : 0);
    std::vector<unsigned char> valid(B * n);
    {
      UdRmArgs<float, float> r;
      r.src = sdv.data(); r.src_mask = dmask.data(); r.uv = uv.data(); r.coord_valid = inside.data(); r.out = ds.data(); r.valid = valid.data();
      r.bs = (long long)(2 * n); r.ps = 2; r.cs = 1; r.n = (long long)n; r.src_bs = (long long)hw; r.mask_bs = (long long)hw;
      r.C = 1; r.Hs = Hs; r.Ws = Ws; r.mode = UD_RM_NEAREST; r.padding = UD_RM_ZEROS; r.normalize = 0; r.out_rows = 1;
      for (int b = 0; b < Bi; ++b)
        for (long long i = 0; i < r.n; ++i) ud_rm_point(r, b, i);
      if (has_weight) {
        r.src = swv.data(); r.out = wv.data(); r.valid = nullptr;
        for (int b = 0; b < Bi; ++b)
          for (long long i = 0; i < r.n; ++i) ud_rm_point(r, b, i);
      }
    }
    if (has_image) {
      UdRmArgs<unsigned char, float> r;
      r.src = imv.data(); r.src_mask = dmask.data(); r.uv = uv.data(); r.coord_valid = inside.data(); r.out = rgb.data(); r.valid = nullptr;
      r.bs = (long long)(2 * n); r.ps = 2; r.cs = 1; r.n = (long long)n; r.src_bs = (long long)(3 * hw); r.mask_bs = (long long)hw;
      r.C = 3; r.Hs = Hs; r.Ws = Ws; r.mode = UD_RM_NEAREST; r.padding = UD_RM_ZEROS; r.normalize = 0; r.out_rows = 1;
      for (int b = 0; b < Bi; ++b)
        for (long long i = 0; i < r.n; ++i) ud_rm_point(r, b, i);
    }
    // the element-wise operations after the launches, one loop each
    const size_t N = B * n;
    std::vector<float> sdf(N), q(N), s(N), Wn(N), m1(N), m2(N), num(N), upd(N), cap(N);
    std::vector<unsigned char> obs(N);
    for (size_t k = 0; k < N; ++k) sdf[k] = ds[k] - d[k];
    for (size_t k = 0; k < N; ++k) obs[k] = valid[k] && d[k] > 0.0f && sdf[k] >= -trunc && wv[k] > 0.0f && wv[k] <= FLT_MAX;
    for (size_t k = 0; k < N; ++k) q[k] = sdf[k] / trunc;
    for (size_t k = 0; k < N; ++k) s[k] = fminf(q[k], 1.0f);
    for (size_t k = 0; k < N; ++k) Wn[k] = W2[k] + wv[k];
    for (size_t k = 0; k < N; ++k) m1[k] = tsdf2[k] * W2[k];
    for (size_t k = 0; k < N; ++k) m2[k] = s[k] * wv[k];
    for (size_t k = 0; k < N; ++k) num[k] = m1[k] + m2[k];
    for (size_t k = 0; k < N; ++k) upd[k] = num[k] / Wn[k];
    for (size_t k = 0; k < N; ++k) tsdf2[k] = obs[k] ? upd[k] : tsdf2[k];
    if (has_image)
      for (int c = 0; c < 3; ++c) {
        for (size_t b = 0; b < B; ++b)
          for (size_t i = 0; i < n; ++i) m1[b * n + i] = color2[(b * 3 + c) * n + i] * W2[b * n + i];
        for (size_t k = 0; k < N; ++k) m2[k] = rgb[k * 3 + c] * wv[k];
        for (size_t k = 0; k < N; ++k) num[k] = m1[k] + m2[k];
        for (size_t k = 0; k < N; ++k) upd[k] = num[k] / Wn[k];
        for (size_t b = 0; b < B; ++b)
          for (size_t i = 0; i < n; ++i)
            if (obs[b * n + i]) color2[(b * 3 + c) * n + i] = upd[b * n + i];
      }
    for (size_t k = 0; k < N; ++k) cap[k] = has_max ? fminf(Wn[k], max_w) : Wn[k];
    for (size_t k = 0; k < N; ++k) W2[k] = obs[k] ? cap[k] : W2[k];
    for (size_t k = 0; k < N; ++k) count2[k] = (unsigned char)(count2[k] + obs[k]);
  }
  const bool eq = same("tsdf", tsdf, tsdf2) & same("weight", W, W2) & same("color", color, color2) & same("count", count, count2);
  if (!eq) return 3;

  // ---- the slots of the resulting volume ------------------------------------------------------------------------------------------
  UdTsdfSlotArgs sa;
  sa.tsdf = tsdf.data(); sa.weight = W.data(); sa.color = has_image ? color.data() : nullptr; sa.origin = origin.data();
  sa.n = (long long)n; sa.vs = vs; sa.min_weight = min_w; sa.B = Bi; sa.Nx = Nx; sa.Ny = Ny; sa.Nz = Nz; sa.nO = nO;
  const size_t S = 3 * n;
  std::vector<unsigned char> live(B * S, 0), rgb8(has_image ? B * S * 3 : 0, 0);
  std::vector<float> xyz(B * S * 3, 0.0f), rgbf(has_image ? B * S * 3 : 0, 0.0f);
  for (int b = 0; b < Bi; ++b)
    for (size_t sl = 0; sl < S; ++sl) {
      const size_t at = (size_t)b * S + sl;
      float p[3], c[3] = {0.0f, 0.0f, 0.0f};
      const bool counted = ud_tsdf_slot(sa, b, (long long)sl, nullptr, nullptr);
      const bool full = ud_tsdf_slot(sa, b, (long long)sl, p, c);
      if (counted != full) {
        fprintf(stderr, "tsdf_host: the predicate of slot %zu depends on whether the payload is asked for\n", at);
        return 3;
      }
      if (!full) continue;
      live[at] = 1;
      for (int k = 0; k < 3; ++k) xyz[at * 3 + k] = p[k];
      if (has_image)
        for (int k = 0; k < 3; ++k) {
          rgbf[at * 3 + k] = c[k];
          rgb8[at * 3 + k] = ud_rm_to_u8(c[k]);
        }
    }
  return write_all(tsdf) && write_all(W) && write_all(color) && write_all(count) && write_all(live) && write_all(xyz) && write_all(rgbf) &&
                 write_all(rgb8)
             ? 0
             : 1;
}
