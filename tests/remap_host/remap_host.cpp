// TEST INFRASTRUCTURE ONLY: a stand-alone host program around unidepth_amd/csrc/remap_taps.h (ud_rm_point, ud_ov_pixel), which runs
// what one thread of remap.hip's two kernels runs, for every point, in the kernels' addressing.  So tests/test_remap_cpu.py can check the
// arithmetic bit for bit without a GPU, under the host sanitizers: every array is allocated exactly as large as its contents, so a tap
// index that escapes is an AddressSanitizer report, and a float-to-int conversion of an unsafe coordinate is an UBSan report.
//
//   remap_host remap MODE PADDING NORMALIZE SRC_U8 OUT_U8 UV_ROWS OUT_ROWS B C Hs Ws N SRC_B UV_B MASK_B HAS_CV HAS_VALID < input
//       MODE 0 nearest, 1 bilinear; PADDING 0 zeros, 1 border; SRC_B / UV_B 1 (shared) or B; MASK_B 0 (none), 1 or B.
//       input, binary: src [SRC_B,C,Hs,Ws] (float32 or bytes), mask [MASK_B,Hs,Ws] bytes, uv float32 ([UV_B,N,2] rows or [UV_B,2,N]
//       planar), coord_valid [B,N] bytes.  output: out ([B,N,C] rows or [B,C,N] planar; float32 or bytes), then valid [B,N] bytes.
//   remap_host overlap B H W < uv float32 [B,2,H,W]          output: mask [B,H,W] bytes
//
// Never loaded by the product.
#include "../../unidepth_amd/csrc/remap_taps.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

template <typename T>
static bool read_all(std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), stdin) == v.size(); }

template <typename T>
static bool write_all(const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size(); }

struct Opt {
  int mode, padding, normalize, uv_rows, out_rows, B, C, Hs, Ws, N, src_b, uv_b, mask_b, has_cv, has_valid;
};

template <typename S, typename O>
static int run_remap(const Opt& o) {
  const size_t hw = (size_t)o.Hs * o.Ws, n = (size_t)o.N;
  std::vector<S> src((size_t)o.src_b * o.C * hw);
  std::vector<unsigned char> mask((size_t)o.mask_b * hw), cv(o.has_cv ? (size_t)o.B * n : 0), valid(o.has_valid ? (size_t)o.B * n : 0);
  std::vector<float> uv((size_t)o.uv_b * 2 * n);
  std::vector<O> out((size_t)o.B * o.C * n);
  if (!read_all(src) || !read_all(mask) || !read_all(uv) || !read_all(cv)) {
    fprintf(stderr, "remap_host: short input\n");
    return 2;
  }
  UdRmArgs<S, O> a;
  a.src = src.data(); a.src_mask = o.mask_b ? mask.data() : nullptr; a.uv = uv.data(); a.coord_valid = o.has_cv ? cv.data() : nullptr;
  a.out = out.data(); a.valid = o.has_valid ? valid.data() : nullptr;
  a.bs = o.uv_b == 1 ? 0 : 2 * (long long)n; a.ps = o.uv_rows ? 2 : 1; a.cs = o.uv_rows ? 1 : (long long)n; a.n = (long long)n;
  a.src_bs = o.src_b == 1 ? 0 : (long long)o.C * (long long)hw; a.mask_bs = o.mask_b == 1 ? 0 : (long long)hw;
  a.C = o.C; a.Hs = o.Hs; a.Ws = o.Ws; a.mode = o.mode; a.padding = o.padding; a.normalize = o.normalize; a.out_rows = o.out_rows;
  for (int b = 0; b < o.B; ++b)
    for (long long i = 0; i < a.n; ++i) ud_rm_point(a, b, i);
  return write_all(out) && write_all(valid) ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "overlap")) {
    const int B = atoi(argv[2]), H = atoi(argv[3]), W = atoi(argv[4]);
    if (B < 1 || H < 2 || W < 2 || (long long)B * H * W > (1 << 26)) {
      fprintf(stderr, "remap_host: bad B / H / W\n");
      return 2;
    }
    const size_t hw = (size_t)H * W;
    std::vector<float> uv((size_t)B * 2 * hw);
    std::vector<unsigned char> mask((size_t)B * hw);
    if (!read_all(uv)) {
      fprintf(stderr, "remap_host: short input\n");
      return 2;
    }
    for (int b = 0; b < B; ++b)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) mask[b * hw + (size_t)y * W + x] = ud_ov_pixel(uv.data() + (size_t)b * 2 * hw, x, y, H, W) ? 1 : 0;
    return write_all(mask) ? 0 : 1;
  }
  if (argc != 19 || strcmp(argv[1], "remap")) {
    fprintf(stderr, "usage: remap_host remap MODE PADDING NORMALIZE SRC_U8 OUT_U8 UV_ROWS OUT_ROWS B C Hs Ws N SRC_B UV_B MASK_B HAS_CV HAS_VALID < input\n"
                    "       remap_host overlap B H W < uv\n");
    return 2;
  }
  int v[17];
  for (int i = 0; i < 17; ++i) v[i] = atoi(argv[2 + i]);
  const int src_u8 = v[3], out_u8 = v[4];
  Opt o = {v[0], v[1], v[2], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14], v[15], v[16]};
  const bool ok = (o.mode == UD_RM_NEAREST || o.mode == UD_RM_BILINEAR) && (o.padding == UD_RM_ZEROS || o.padding == UD_RM_BORDER) &&
                  o.B >= 1 && o.C >= 1 && o.Hs >= 1 && o.Ws >= 1 && o.N >= 1 && (long long)o.B * o.C * o.N <= (1 << 26) &&
                  (long long)o.C * o.Hs * o.Ws <= (1 << 26) && (o.src_b == 1 || o.src_b == o.B) && (o.uv_b == 1 || o.uv_b == o.B) &&
                  (o.mask_b == 0 || o.mask_b == 1 || o.mask_b == o.B) && (!out_u8 || src_u8);
  if (!ok) {
    fprintf(stderr, "remap_host: bad arguments\n");
    return 2;
  }
  if (!src_u8) return run_remap<float, float>(o);
  return out_u8 ? run_remap<unsigned char, unsigned char>(o) : run_remap<unsigned char, float>(o);
}
