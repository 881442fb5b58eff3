// Host build of csrc/pyramid_point.h for the CPU tests: the per-pixel functions of the depth pyramid, compiled stand-alone under
// AddressSanitizer and UBSan (tests/host_program.py) and driven over a whole batch the way pyramid.hip's kernel drives them -- a staged
// map with an r-pixel border of zeros stands for a tile with its halo.
//
//   pyramid_host B H W levels radius has_mask has_weights gate_bits inv_bin_bits
//   stdin : depth f32 [B,H,W], mask u8 [B,H,W] (has_mask), weights f32 [B,H,W] (has_weights), ws f32 [(2r+1)^2] and wr f32 [256] (radius)
//   stdout: depth of level 0 .. levels - 1, f32 [B,H_l,W_l] each, then (has_weights) the weights of every level likewise
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../unidepth_amd/csrc/pyramid_point.h"

static float from_bits(int bits) {
  float f;
  memcpy(&f, &bits, 4);
  return f;
}

template <class T>
static bool read_all(std::vector<T>& v) {
  return v.empty() || fread(v.data(), sizeof(T), v.size(), stdin) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 10) {
    fprintf(stderr, "usage: pyramid_host B H W levels radius has_mask has_weights gate_bits inv_bin_bits\n");
    return 2;
  }
  const int B = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), L = atoi(argv[4]), r = atoi(argv[5]);
  const bool has_mask = atoi(argv[6]) != 0, has_w = atoi(argv[7]) != 0;
  const float gate = from_bits(atoi(argv[8])), inv_bin = from_bits(atoi(argv[9]));
  if (B < 1 || H < 1 || W < 1 || L < 1 || L > UD_PY_MAX_LEVELS || r < 0 || r > UD_PY_MAX_R || (H >> (L - 1)) < 1 || (W >> (L - 1)) < 1) {
    fprintf(stderr, "pyramid_host: bad sizes\n");
    return 2;
  }
  const size_t n = (size_t)H * W;
  std::vector<float> depth(B * n), weights(has_w ? B * n : 0), ws(r ? (size_t)(2 * r + 1) * (2 * r + 1) : 0), wr(r ? UD_PY_NB : 0);
  std::vector<unsigned char> mask(has_mask ? B * n : 0);
  if (!read_all(depth) || !read_all(mask) || !read_all(weights) || !read_all(ws) || !read_all(wr)) {
    fprintf(stderr, "pyramid_host: short input\n");
    return 2;
  }
  std::vector<std::vector<float>> out_d(L), out_w(L);
  const int stride = W + 2 * r;
  std::vector<float> staged((size_t)(H + 2 * r) * stride);
  int Hl = H, Wl = W;
  for (int l = 0; l < L; ++l) {
    out_d[l].assign((size_t)B * Hl * Wl, 0.0f);
    if (has_w) out_w[l].assign((size_t)B * Hl * Wl, 0.0f);
    Hl >>= 1; Wl >>= 1;
  }
  for (int b = 0; b < B; ++b) {
    std::fill(staged.begin(), staged.end(), 0.0f);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = b * n + (size_t)y * W + x;
        const float w = has_w ? weights[i] : 0.0f;
        const float d = ud_py_stage(depth[i], has_mask ? mask[i] != 0 : true, has_w, w);
        staged[(size_t)(y + r) * stride + x + r] = d;
        if (has_w) out_w[0][i] = d > 0.0f ? w : 0.0f;
      }
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const int jc = (y + r) * stride + x + r;
        float v = staged[jc];
        if (r > 0 && v > 0.0f) v = ud_py_filter(staged.data(), stride, jc, r, ws.data(), wr.data(), inv_bin);
        out_d[0][b * n + (size_t)y * W + x] = v;
      }
    int Hp = H, Wp = W;
    for (int l = 1; l < L; ++l) {
      const int Hc = Hp >> 1, Wc = Wp >> 1;
      const float* pd = out_d[l - 1].data() + (size_t)b * Hp * Wp;
      const float* pw = has_w ? out_w[l - 1].data() + (size_t)b * Hp * Wp : nullptr;
      for (int y = 0; y < Hc; ++y)
        for (int x = 0; x < Wc; ++x) {
          const size_t j = (size_t)(2 * y) * Wp + 2 * x;
          const float d[4] = {pd[j], pd[j + 1], pd[j + Wp], pd[j + Wp + 1]};
          float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          if (has_w) {
            w[0] = pw[j]; w[1] = pw[j + 1]; w[2] = pw[j + Wp]; w[3] = pw[j + Wp + 1];
          }
          float v, wv;
          ud_py_reduce(d, w, has_w, gate, &v, &wv);
          out_d[l][(size_t)b * Hc * Wc + (size_t)y * Wc + x] = v;
          if (has_w) out_w[l][(size_t)b * Hc * Wc + (size_t)y * Wc + x] = wv;
        }
      Hp = Hc; Wp = Wc;
    }
  }
  for (int l = 0; l < L; ++l) fwrite(out_d[l].data(), 4, out_d[l].size(), stdout);
  if (has_w)
    for (int l = 0; l < L; ++l) fwrite(out_w[l].data(), 4, out_w[l].size(), stdout);
  return 0;
}
