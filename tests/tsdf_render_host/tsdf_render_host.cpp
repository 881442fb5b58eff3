// TEST INFRASTRUCTURE ONLY: a stand-alone host program around unidepth_amd/csrc/tsdf_ray.h.  It runs ud_tsdf_ray, what one thread of
// tsdf_render.hip's kernel runs, for every pixel of every image, in the kernel's addressing -- once with the clip (the samples that cannot
// lie in the grid skipped) and once with the full scan, each with byte and with fp32 colours.  The two must give the same bits in every
// output; the program exits 3 otherwise.  It writes the outputs and the directions it used, which tests/tsdf_render_common.py compares
// with its numpy restatement of the full scan.  So tests/test_tsdf_render_cpu.py can check the ray function without a GPU, under the host
// sanitizers: every array is allocated exactly as large as its contents, so an index that escapes is an AddressSanitizer report, and a
// float-to-int conversion of an unsafe coordinate is an UBSan report.
//
//   tsdf_render_host B Ho Wo Nz Ny Nx NT NO HAS_COLOR HAS_RAYS K VS_BITS NEAR_BITS STEP_BITS MINW_BITS MODEL_0..MODEL_B-1
//       NT 0 (no transform), 1 or B matrices, NO 1 or B origins; the scalars as fp32 bit patterns.
//       input, binary: tsdf [B,n] float32, weight [B,n] float32, color [B,3,n] float32 (HAS_COLOR), origin [NO,3] float32, T [NT,3,4]
//       float32 (camera to volume), params [B,16] float32, rays [B,3,Ho*Wo] float32 (HAS_RAYS).  n = Nz * Ny * Nx.
//       output: dirs [B,3,hw] float32 (the rays, or the model's normalised ray of every pixel centre), depth [B,hw] float32, valid [B,hw]
//       bytes, points [B,3,hw] float32, normals [B,3,hw] float32, and with HAS_COLOR color [B,3,hw] float32 and [B,3,hw] bytes.
//
// Never loaded by the product.
#include "../../unidepth_amd/csrc/tsdf_ray.h"
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
  fprintf(stderr, "tsdf_render_host: %s differs between the clipped and the full scan, first at element %zu\n", what, k);
  return false;
}

static float from_bits(int i) {
  float f;
  memcpy(&f, &i, 4);
  return f;
}

struct Outputs {
  std::vector<float> depth, points, normals, colf;
  std::vector<unsigned char> valid, col8;
};

int main(int argc, char** argv) {
  const int fixed = 15;
  int v0[fixed];
  for (int i = 0; i < fixed; ++i) v0[i] = argc > 1 + i ? atoi(argv[1 + i]) : 0;
  const int Bi = v0[0], Ho = v0[1], Wo = v0[2], Nz = v0[3], Ny = v0[4], Nx = v0[5], nT = v0[6], nO = v0[7], has_color = v0[8], has_rays = v0[9];
  const int K = v0[10];
  bool ok = Bi >= 1 && Bi <= 256 && Ho >= 1 && Wo >= 1 && Nz >= 1 && Ny >= 1 && Nx >= 1 && (nT == 0 || nT == 1 || nT == Bi) && (nO == 1 || nO == Bi) &&
            K >= 1 && K <= 16384 && (long long)Bi * Nz * Ny * Nx <= (1 << 24) && (long long)Bi * Ho * Wo <= (1 << 24) && argc == 1 + fixed + Bi;
  if (!ok) {
    fprintf(stderr, "usage: tsdf_render_host B Ho Wo Nz Ny Nx NT NO HAS_COLOR HAS_RAYS K VS_BITS NEAR_BITS STEP_BITS MINW_BITS MODEL_0.. < input\n");
    return 2;
  }
  unsigned char model[256];
  for (int k = 0; k < Bi; ++k) {
    const int m = atoi(argv[1 + fixed + k]);
    ok = ok && ud_cam_model_ok(m) && (has_rays || ud_cam_closed_form(m));
    model[k] = (unsigned char)m;
  }
  const float vs = from_bits(v0[11]), near = from_bits(v0[12]), step = from_bits(v0[13]), min_w = from_bits(v0[14]);
  if (!ok || !(vs > 0.0f) || !(step > 0.0f) || !(near >= 0.0f) || min_w != min_w) {
    fprintf(stderr, "tsdf_render_host: bad model tags or scalars\n");
    return 2;
  }
  const size_t B = (size_t)Bi, n = (size_t)Nz * Ny * Nx, hw = (size_t)Ho * Wo;
  std::vector<float> tsdf(B * n), weight(B * n), color(has_color ? B * 3 * n : 0), origin((size_t)nO * 3), T((size_t)nT * 12), ps(B * 16);
  std::vector<float> rays(has_rays ? B * 3 * hw : 0);
  if (!read_all(tsdf) || !read_all(weight) || !read_all(color) || !read_all(origin) || !read_all(T) || !read_all(ps) || !read_all(rays)) {
    fprintf(stderr, "tsdf_render_host: short input\n");
    return 2;
  }
  // the directions, for the restatement: the rays as they are, or the model's normalised ray of the pixel centre
  std::vector<float> dirs(B * 3 * hw);
  for (size_t b = 0; b < B; ++b)
    for (int py = 0; py < Ho; ++py)
      for (int px = 0; px < Wo; ++px) {
        const size_t i = (size_t)py * Wo + px;
        float d[3];
        if (has_rays) {
          for (int k = 0; k < 3; ++k) d[k] = rays[(b * 3 + k) * hw + i];
        } else {
          ud_cam_unproject_closed(model[b], UD_UNPROJ_NORMALIZE, ps.data() + b * 16, (float)px + 0.5f, (float)py + 0.5f, 0.0f, d);
        }
        for (int k = 0; k < 3; ++k) dirs[(b * 3 + k) * hw + i] = d[k];
      }

  Outputs out[4];                                          // (clip, full) x (byte colours, fp32 colours)
  for (int r = 0; r < 4; ++r) {
    const int full = r & 1, f32 = r >> 1;
    Outputs& o = out[r];
    // poisoned: every element must be written
    o.depth.assign(B * hw, from_bits(0x7fc00001)); o.points.assign(B * 3 * hw, from_bits(0x7fc00002)); o.normals.assign(B * 3 * hw, from_bits(0x7fc00003));
    o.valid.assign(B * hw, 0xAB);
    if (has_color && f32) o.colf.assign(B * 3 * hw, from_bits(0x7fc00004));
    if (has_color && !f32) o.col8.assign(B * 3 * hw, 0xAB);
    UdTsdfRayArgs a;
    a.tsdf = tsdf.data(); a.weight = weight.data(); a.color = has_color ? color.data() : nullptr; a.origin = origin.data();
    a.T = nT ? T.data() : nullptr; a.params = has_rays ? nullptr : ps.data(); a.rays = has_rays ? rays.data() : nullptr;
    a.depth = o.depth.data(); a.valid = o.valid.data(); a.points = o.points.data(); a.normals = o.normals.data();
    a.color_out = !has_color ? nullptr : (f32 ? (void*)o.colf.data() : (void*)o.col8.data());
    a.n = (long long)n; a.vs = vs; a.near = near; a.step = step; a.min_weight = min_w;
    a.B = Bi; a.Ho = Ho; a.Wo = Wo; a.Nx = Nx; a.Ny = Ny; a.Nz = Nz; a.nT = nT; a.nO = nO; a.K = K; a.color_f32 = f32; a.full_scan = full;
    for (int b = 0; b < Bi; ++b)
      for (int py = 0; py < Ho; ++py)
        for (int px = 0; px < Wo; ++px) ud_tsdf_ray(a, model[b], b, py, px);
  }
  bool eq = true;
  for (int f32 = 0; f32 < 2; ++f32) {
    const Outputs &c = out[2 * f32], &f = out[2 * f32 + 1];
    eq = eq & same("depth", c.depth, f.depth) & same("valid", c.valid, f.valid) & same("points", c.points, f.points) &
         same("normals", c.normals, f.normals) & same("color (fp32)", c.colf, f.colf) & same("color (bytes)", c.col8, f.col8);
  }
  // the colour type changes nothing else
  eq = eq & same("depth", out[1].depth, out[3].depth) & same("valid", out[1].valid, out[3].valid) & same("points", out[1].points, out[3].points) &
       same("normals", out[1].normals, out[3].normals);
  if (!eq) return 3;
  const Outputs& f = out[1];
  return write_all(dirs) && write_all(f.depth) && write_all(f.valid) && write_all(f.points) && write_all(f.normals) && write_all(out[3].colf) &&
                 write_all(f.col8)
             ? 0
             : 1;
}
