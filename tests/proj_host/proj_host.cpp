// TEST INFRASTRUCTURE ONLY: a stand-alone host program around the forward models of unidepth_amd/csrc/camera_models.h
// (ud_cam_project_<model>, ud_cam_inside, ud_cam_depth), so tests/test_camera_project_cpu.py can check the arithmetic without a GPU.
//
//   proj_host MODEL H W N p0 .. p15      (MODEL 1..6; the parameters as hexadecimal floats, "%a")
//
// reads N points from stdin, binary float32 [N][3], and writes to stdout, binary: float32 [N][2] (u, v), float32 [N] the model's depth,
// then N bytes, the in-image test against H, W.
// Never loaded by the product.
#include "../../unidepth_amd/csrc/camera_models.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 21) {
    fprintf(stderr, "usage: proj_host MODEL H W N p0 .. p15\n");
    return 2;
  }
  const int model = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), N = atoi(argv[4]);
  if (model < UD_CAM_PINHOLE || model > UD_CAM_MEI || H < 1 || W < 1 || N < 0 || N > (1 << 24)) {
    fprintf(stderr, "proj_host: bad MODEL / H / W / N\n");
    return 2;
  }
  float p[16];
  for (int i = 0; i < 16; ++i) p[i] = strtof(argv[5 + i], nullptr);
  std::vector<float> xyz(3 * (size_t)N), uv(2 * (size_t)N), depth(N);
  std::vector<unsigned char> inside(N);
  if (fread(xyz.data(), sizeof(float), xyz.size(), stdin) != xyz.size()) {
    fprintf(stderr, "proj_host: short read\n");
    return 2;
  }
  for (int i = 0; i < N; ++i) {
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    ud_cam_project(model, p, x, y, z, &uv[2 * (size_t)i], &uv[2 * (size_t)i + 1]);
    depth[i] = ud_cam_depth(model, x, y, z);
    inside[i] = ud_cam_inside(model, uv[2 * (size_t)i], uv[2 * (size_t)i + 1], z, H, W) ? 1 : 0;
  }
  bool ok = fwrite(uv.data(), sizeof(float), uv.size(), stdout) == uv.size();
  ok = ok && fwrite(depth.data(), sizeof(float), depth.size(), stdout) == depth.size();
  ok = ok && fwrite(inside.data(), 1, inside.size(), stdout) == inside.size();
  return ok ? 0 : 1;
}
