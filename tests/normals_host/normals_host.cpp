// TEST INFRASTRUCTURE ONLY: a stand-alone host program around unidepth_amd/csrc/normals_point.h, which runs what one thread of
// normals.hip's kernels runs, for every pixel, in the kernels' addressing.  tests/test_normals_cpu.py compares its output bit for bit with
// the numpy fp32 restatement of tests/normals_common.py, without a GPU and under the host sanitizers: every array is allocated exactly as
// large as its contents, so an index that escapes is an AddressSanitizer report.
//
//   normals_host FORM B H W MASK_B HAS_DEPTH HAS_RTOL RTOL_BITS MODEL_0..MODEL_B-1 < input
//       FORM 0  the points form (ud_nm_pixel).  input, binary: points [B,3,H,W] float32, depth [B,H,W] float32 (HAS_DEPTH), mask
//               [MASK_B,H,W] bytes (MASK_B 0 none, 1 shared, or B).  MODEL_b is not read.
//       FORM 1  the depth form.  input: depth [B,H,W] float32, params [B,16] float32, mask [MASK_B,H,W] bytes.  The CHAIN is run first:
//               the point map of every image by camera_models.h's reconstruct (closed-form: ud_cam_unproject_closed; OPENCV / Fisheye624:
//               the two-pass radial loop of unproject.hip, the exit iteration from the maxima over the image), mask & (depth > 0), then
//               ud_nm_pixel on that point map with the depth.  For the closed-form images the FUSED order of nm_depth_kernel is run beside
//               it -- ud_nm_depth_point for the pixel and its four neighbours, ud_nm_edge_ok, ud_nm_normal -- and must give the same bits:
//               the program exits 3 otherwise.
//       RTOL_BITS the bit pattern of the fp32 edge_rtol (read with HAS_RTOL).
//       output, binary: normals [B,3,H,W] float32, valid [B,H,W] bytes, rgb [B,3,H,W] bytes; FORM 1 appends the points [B,3,H,W] float32.
//
// Never loaded by the product.
#include "../../unidepth_amd/csrc/normals_point.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

template <typename T>
static bool read_all(std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), stdin) == v.size(); }

template <typename T>
static bool write_all(const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size(); }

// camera_models.h's reconstruct of one image at the pixel centres, planar [3,H,W]
static void reconstruct(int model, const float* p, const float* depth, int H, int W, float* out) {
  const size_t hw = (size_t)H * W;
  int steps = 0;
  const bool iterative = model == UD_CAM_OPENCV || model == UD_CAM_FISHEYE624;
  if (iterative) {
    const int nk = model == UD_CAM_FISHEYE624 ? 6 : 3;
    float maxima[11] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (size_t i = 0; i < hw; ++i) {
      float xr, yr, rnorm;
      if (!ud_cam_radial_front(p, (float)(i % W) + 0.5f, (float)(i / W) + 0.5f, &xr, &yr, &rnorm)) break;
      float th = rnorm, delta = 0.1f;
      for (int it = 0; it <= 10; ++it) {
        maxima[it] = ud_cam_nanmax(maxima[it], fabsf(ud_cam_radial_residual(p + 4, nk, th, rnorm)));
        if (it < 10) ud_cam_radial_step(p + 4, nk, rnorm, th, delta);
      }
    }
    steps = ud_cam_radial_exit(maxima);
  }
  for (size_t i = 0; i < hw; ++i) {
    float o[3];
    const float u = (float)(i % W) + 0.5f, v = (float)(i / W) + 0.5f;
    if (iterative) ud_cam_unproject_radial(model, UD_UNPROJ_DEPTH, p, u, v, depth[i], steps, o);
    else ud_cam_unproject_closed(model, UD_UNPROJ_DEPTH, p, u, v, depth[i], o);
    out[i] = o[0]; out[hw + i] = o[1]; out[2 * hw + i] = o[2];
  }
}

int main(int argc, char** argv) {
  if (argc < 9) {
    fprintf(stderr, "usage: normals_host FORM B H W MASK_B HAS_DEPTH HAS_RTOL RTOL_BITS MODEL_0..MODEL_B-1 < input\n");
    return 2;
  }
  const int form = atoi(argv[1]), B = atoi(argv[2]), H = atoi(argv[3]), W = atoi(argv[4]), mask_b = atoi(argv[5]);
  const int has_depth = atoi(argv[6]), has_rtol = atoi(argv[7]);
  union { int32_t i; float f; } rt;
  rt.i = (int32_t)strtol(argv[8], nullptr, 10);
  if (B < 1 || B > 256 || H < 1 || W < 1 || argc != 9 + B || (mask_b != 0 && mask_b != 1 && mask_b != B) || (form == 1 && !has_depth)) {
    fprintf(stderr, "normals_host: bad arguments\n");
    return 2;
  }
  std::vector<int> model((size_t)B);
  for (int b = 0; b < B; ++b) model[b] = atoi(argv[9 + b]);
  const size_t hw = (size_t)H * W, nb = (size_t)B;
  std::vector<float> points(form == 0 ? nb * 3 * hw : 0), depth(has_depth ? nb * hw : 0), params(form == 1 ? nb * 16 : 0);
  std::vector<unsigned char> mask((size_t)mask_b * hw);
  const bool got = form == 0 ? (read_all(points) && read_all(depth) && read_all(mask)) : (read_all(depth) && read_all(params) && read_all(mask));
  if (!got) {
    fprintf(stderr, "normals_host: short input\n");
    return 2;
  }
  std::vector<float> normals(nb * 3 * hw);
  std::vector<unsigned char> valid(nb * hw), rgb(nb * 3 * hw), eff;
  if (form == 1) {                                     // the chain: the point map, then mask & (depth > 0)
    points.resize(nb * 3 * hw);
    eff.resize(nb * hw);
    for (int b = 0; b < B; ++b) {
      reconstruct(model[b], &params[(size_t)b * 16], &depth[(size_t)b * hw], H, W, &points[(size_t)b * 3 * hw]);
      for (size_t i = 0; i < hw; ++i) {
        const bool m = mask_b ? mask[(mask_b == 1 ? 0 : (size_t)b * hw) + i] != 0 : true;
        eff[(size_t)b * hw + i] = (m && depth[(size_t)b * hw + i] > 0.0f) ? 1 : 0;
      }
    }
  }
  UdNmArgs a;
  a.points = points.data(); a.depth = has_depth ? depth.data() : nullptr;
  a.mask = form == 1 ? eff.data() : (mask_b ? mask.data() : nullptr);
  a.normals = normals.data(); a.valid = valid.data(); a.rgb = rgb.data();
  a.mask_bs = (form == 1 || mask_b == B) ? (long long)hw : 0;
  a.rtol = has_rtol ? rt.f : 0.0f;
  a.H = H; a.W = W; a.has_rtol = has_rtol;
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) ud_nm_pixel(a, b, y, x);
  if (form == 1) {                                     // the fused order of nm_depth_kernel, closed-form images
    std::vector<float> n2(3 * hw);
    std::vector<unsigned char> v2(hw), c2(3 * hw);
    UdNmArgs f = a;
    f.normals = n2.data(); f.valid = v2.data(); f.rgb = c2.data();
    for (int b = 0; b < B; ++b) {
      if (model[b] == UD_CAM_OPENCV || model[b] == UD_CAM_FISHEYE624) continue;
      const float* pr = &params[(size_t)b * 16];
      const float* db = &depth[(size_t)b * hw];
      const unsigned char* mb = mask_b ? &mask[mask_b == 1 ? 0 : (size_t)b * hw] : nullptr;
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const int qy[5] = {y, y, y, y - 1, y + 1}, qx[5] = {x, x - 1, x + 1, x, x};
          float p[5][3] = {{0.0f}}, d[5] = {0.0f}, n[3];
          bool ok[5];
          for (int k = 0; k < 5; ++k) {
            ok[k] = false;
            if (qx[k] >= 0 && qx[k] < W && qy[k] >= 0 && qy[k] < H) ok[k] = ud_nm_depth_point(model[b], pr, mb, db, W, qy[k], qx[k], p[k], &d[k]);
            if (k > 0 && has_rtol) ok[k] = ok[k] && ud_nm_edge_ok(d[0], d[k], f.rtol);
          }
          const bool v = ud_nm_normal(p[0], p[1], p[2], p[3], p[4], ok[0], ok[1], ok[2], ok[3], ok[4], n);
          ud_nm_store(f, 0, (size_t)y * W + x, v, n);
        }
      if (memcmp(n2.data(), &normals[(size_t)b * 3 * hw], 3 * hw * sizeof(float)) || memcmp(v2.data(), &valid[(size_t)b * hw], hw) ||
          memcmp(c2.data(), &rgb[(size_t)b * 3 * hw], 3 * hw)) {
        fprintf(stderr, "normals_host: the fused order differs from the chain in image %d\n", b);
        return 3;
      }
    }
  }
  bool ok = write_all(normals) && write_all(valid) && write_all(rgb);
  if (form == 1) ok = ok && write_all(points);
  return ok ? 0 : 1;
}
