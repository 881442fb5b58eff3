// TEST INFRASTRUCTURE ONLY: a stand-alone host program around the unprojection functions of unidepth_amd/csrc/camera_models.h
// (ud_cam_unproject_closed, ud_cam_radial_front / _exit / _solve, ud_cam_unproject_radial), driven in the two-pass order of unproject.hip:
// pass 1 runs every point's own 10 trust-region steps and collects the largest |residual| at theta_0 .. theta_10 over the point set,
// pass 2 reads the iteration the set leaves the loop at, redoes that many steps per point and writes the result.  So
// tests/test_unproject_cpu.py can check the arithmetic and the iteration counts without a GPU, under the host sanitizers.
//
//   unproj_host MODEL FORM N p0 .. p15 < input      (MODEL 1..6; FORM 0 raw, 1 normalize, 2 depth; the parameters as hexadecimal
//                                                    floats, "%a"; input: N records of three float32 (u, v, depth), binary)
//
// writes to stdout, binary: int32 steps of the radial loop (-1 for the models without one), N x 3 float32 rays, N bytes of mask.
// Never loaded by the product.
#include "../../unidepth_amd/csrc/camera_models.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 20) {
    fprintf(stderr, "usage: unproj_host MODEL FORM N p0 .. p15 < input\n");
    return 2;
  }
  const int model = atoi(argv[1]), form = atoi(argv[2]), N = atoi(argv[3]);
  if (model < UD_CAM_PINHOLE || model > UD_CAM_MEI || form < UD_UNPROJ_RAW || form > UD_UNPROJ_DEPTH || N < 1 || N > (1 << 24)) {
    fprintf(stderr, "unproj_host: bad MODEL / FORM / N\n");
    return 2;
  }
  float p[16];
  for (int i = 0; i < 16; ++i) p[i] = strtof(argv[4 + i], nullptr);
  std::vector<float> in(3 * (size_t)N), rays(3 * (size_t)N);
  std::vector<unsigned char> mask((size_t)N);
  if (fread(in.data(), sizeof(float), in.size(), stdin) != in.size()) {
    fprintf(stderr, "unproj_host: short input\n");
    return 2;
  }
  int32_t steps = -1;
  if (model == UD_CAM_OPENCV || model == UD_CAM_FISHEYE624) {
    const int nk = model == UD_CAM_FISHEYE624 ? 6 : 3;
    float maxima[11] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};      // as the call's memset leaves them
    for (int i = 0; i < N; ++i) {                                  // pass 1
      float xr, yr, rnorm;
      if (!ud_cam_radial_front(p, in[3 * i], in[3 * i + 1], &xr, &yr, &rnorm)) break;      // no radial term: nothing is published
      float th = rnorm, delta = 0.1f;
      for (int it = 0; it <= 10; ++it) {
        maxima[it] = ud_cam_nanmax(maxima[it], fabsf(ud_cam_radial_residual(p + 4, nk, th, rnorm)));
        if (it < 10) ud_cam_radial_step(p + 4, nk, rnorm, th, delta);
      }
    }
    steps = ud_cam_radial_exit(maxima);
    for (int i = 0; i < N; ++i) {                                  // pass 2
      ud_cam_unproject_radial(model, form, p, in[3 * i], in[3 * i + 1], in[3 * i + 2], steps, &rays[3 * i]);
      mask[i] = 1;
    }
  } else {
    for (int i = 0; i < N; ++i) mask[i] = ud_cam_unproject_closed(model, form, p, in[3 * i], in[3 * i + 1], in[3 * i + 2], &rays[3 * i]) ? 1 : 0;
  }
  bool ok = fwrite(&steps, sizeof(steps), 1, stdout) == 1;
  ok = ok && fwrite(rays.data(), sizeof(float), rays.size(), stdout) == rays.size();
  ok = ok && fwrite(mask.data(), 1, mask.size(), stdout) == mask.size();
  return ok ? 0 : 1;
}
