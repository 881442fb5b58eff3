// TEST INFRASTRUCTURE ONLY: a stand-alone host program around the NOT normalised functions of unidepth_amd/csrc/camera_models.h
// (ud_cam_finish_radial_dir, ud_cam_mei_dir), driven the way reconstruct.hip drives them -- init pass, up to 10 step passes gated by
// the image-wide maximum residual, final pass -- so tests/test_gt_points_cpu.py can check the arithmetic without a GPU.
//
//   recon_host MODEL H W p0 .. p15      (MODEL 4 OPENCV, 5 Fisheye624, 6 MEI; the parameters as hexadecimal floats, "%a")
//
// writes to stdout, binary: int32 steps of the radial loop, then three float32 blocks [3][H*W]:
//   the direction (dx, dy, z) not normalised, that direction normalised as Camera.get_rays does (1 / max(norm, 1e-4)), and the
//   result of the existing normalised functions (ud_cam_finish_radial, ud_cam_mei) on the same solver state.
// Never loaded by the product.
#include "../../unidepth_amd/csrc/camera_models.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 20) {
    fprintf(stderr, "usage: recon_host MODEL H W p0 .. p15\n");
    return 2;
  }
  const int model = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]);
  if (model < 4 || model > 6 || H < 1 || W < 1 || (long long)H * W > (1 << 24)) {
    fprintf(stderr, "recon_host: bad MODEL / H / W\n");
    return 2;
  }
  float p[16];
  for (int i = 0; i < 16; ++i) p[i] = strtof(argv[4 + i], nullptr);
  const int HW = H * W;
  std::vector<float> raw(3 * (size_t)HW), nrm(3 * (size_t)HW), old(3 * (size_t)HW);
  int32_t steps = 0;
  auto normalise = [&](int pix) {
    const float dx = raw[pix], dy = raw[HW + pix], dz = raw[2 * HW + pix];
    const float inv = 1.0f / fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-4f);
    nrm[pix] = dx * inv; nrm[HW + pix] = dy * inv;
    nrm[2 * HW + pix] = model == 6 ? dz * inv : inv;               // z = 1 for the radial models: ud_cam_finish_radial stores inv itself
  };
  if (model == 6) {
    for (int pix = 0; pix < HW; ++pix) {
      const int v = pix / W, u = pix - v * W;
      ud_cam_mei_dir(p, (float)u + 0.5f, (float)v + 0.5f, raw[pix], raw[HW + pix], raw[2 * HW + pix]);
      ud_cam_mei(p, (float)u + 0.5f, (float)v + 0.5f, old[pix], old[HW + pix], old[2 * HW + pix]);
      normalise(pix);
    }
  } else {
    const int nk = model == 5 ? 6 : 3;
    const int use_tan = fabsf(p[10]) + fabsf(p[11]) > 1e-6f;
    const int use_prism = fabsf(p[12]) + fabsf(p[13]) + fabsf(p[14]) + fabsf(p[15]) > 1e-6f;
    const int use_radial = fabsf(p[4]) + fabsf(p[5]) + fabsf(p[6]) + fabsf(p[7]) + fabsf(p[8]) + fabsf(p[9]) > 1e-6f;
    std::vector<float> xr(HW), yr(HW), th(HW), delta(HW, 0.1f);
    for (int pix = 0; pix < HW; ++pix) {
      const int v = pix / W, u = pix - v * W;
      const float ud = ((float)u + 0.5f - p[2]) / p[0], vd = ((float)v + 0.5f - p[3]) / p[1];
      ud_cam_undistort_tanprism(ud, vd, p[10], p[11], p[12], p[13], p[14], p[15], use_tan, use_prism, (use_tan || use_prism) ? 10 : 0, xr[pix], yr[pix]);
      th[pix] = sqrtf(xr[pix] * xr[pix] + yr[pix] * yr[pix]);
    }
    for (int it = 0; it < (use_radial ? 10 : 0); ++it) {
      float mx = 0.0f;
      bool nan = false;
      for (int pix = 0; pix < HW; ++pix) {
        const float rn = sqrtf(xr[pix] * xr[pix] + yr[pix] * yr[pix]);
        const float r = fabsf(ud_cam_radial_residual(p + 4, nk, th[pix], rn));
        if (r != r) nan = true;
        if (r > mx) mx = r;
      }
      if (!nan && mx < UD_CAM_EPS) break;
      ++steps;
      for (int pix = 0; pix < HW; ++pix) {
        const float rn = sqrtf(xr[pix] * xr[pix] + yr[pix] * yr[pix]);
        ud_cam_radial_step(p + 4, nk, rn, th[pix], delta[pix]);
      }
    }
    for (int pix = 0; pix < HW; ++pix) {
      const float rn = sqrtf(xr[pix] * xr[pix] + yr[pix] * yr[pix]);
      ud_cam_finish_radial_dir(xr[pix], yr[pix], rn, th[pix], model == 5, raw[pix], raw[HW + pix]);
      raw[2 * HW + pix] = 1.0f;
      ud_cam_finish_radial(xr[pix], yr[pix], rn, th[pix], model == 5, old[pix], old[HW + pix], old[2 * HW + pix]);
      normalise(pix);
    }
  }
  bool ok = fwrite(&steps, sizeof(steps), 1, stdout) == 1;
  ok = ok && fwrite(raw.data(), sizeof(float), raw.size(), stdout) == raw.size();
  ok = ok && fwrite(nrm.data(), sizeof(float), nrm.size(), stdout) == nrm.size();
  ok = ok && fwrite(old.data(), sizeof(float), old.size(), stdout) == old.size();
  return ok ? 0 : 1;
}
