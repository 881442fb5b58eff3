// TEST INFRASTRUCTURE ONLY: a stand-alone host program around unidepth_amd/csrc/tsdf_mesh_point.h.  It runs ud_tsdf_cell for every cell of
// every volume, what one thread of tsdf_mesh.hip's cell kernels runs, and ud_tsdf_quad for every slot with the cell flags of the first pass
// behind its cell_live, as the slot kernels read the cell mask, and writes the flags and payloads, which tests/tsdf_mesh_common.py
// compares with its numpy restatement.  So tests/test_tsdf_mesh_cpu.py can check the arithmetic without a GPU, under the host sanitizers:
// every array is allocated exactly as large as its contents, so an index that escapes is an AddressSanitizer report.
//
//   tsdf_mesh_host B Nz Ny Nx NO HAS_COLOR VS_BITS MINW_BITS
//       NO 1 or B origins; the scalars as fp32 bit patterns.  n = Nz * Ny * Nx.
//       input, binary: tsdf [B,n] float32, weight [B,n] float32, color [B,3,n] float32 (HAS_COLOR), origin [NO,3] float32.
//       output: live [B,n] bytes, xyz [B,n,3] float32, normal [B,n,3] float32, and with HAS_COLOR rgb [B,n,3] float32 and its rounding to
//       bytes [B,n,3]; then quad_live [B,3n] bytes and quad [B,3n,4] int32, the four voxel indices in winding order.  Rows of cells and
//       slots that are not live are 0.
//       exit status 3: a predicate depends on whether the payload is asked for, or cell_live was asked outside the grid.
//
// Never loaded by the product.
#include "../../unidepth_amd/csrc/tsdf_mesh_point.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

template <typename T>
static bool read_all(std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), stdin) == v.size(); }

template <typename T>
static bool write_all(const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size(); }

static float from_bits(int i) {
  float f;
  memcpy(&f, &i, 4);
  return f;
}

int main(int argc, char** argv) {
  const int fixed = 8;
  int v0[fixed];
  for (int i = 0; i < fixed; ++i) v0[i] = argc > 1 + i ? atoi(argv[1 + i]) : 0;
  const int Bi = v0[0], Nz = v0[1], Ny = v0[2], Nx = v0[3], nO = v0[4], has_color = v0[5];
  const float vs = from_bits(v0[6]), min_w = from_bits(v0[7]);
  const bool ok = argc == 1 + fixed && Bi >= 1 && Nz >= 1 && Ny >= 1 && Nx >= 1 && (nO == 1 || nO == Bi) &&
                  (long long)Bi * Nz * Ny * Nx <= (1 << 22) && vs > 0.0f && min_w == min_w;
  if (!ok) {
    fprintf(stderr, "usage: tsdf_mesh_host B Nz Ny Nx NO HAS_COLOR VS_BITS MINW_BITS < input\n");
    return 2;
  }
  const size_t B = (size_t)Bi, n = (size_t)Nz * Ny * Nx, S = 3 * n;
  std::vector<float> tsdf(B * n), W(B * n), color(has_color ? B * 3 * n : 0), origin((size_t)nO * 3);
  if (!read_all(tsdf) || !read_all(W) || !read_all(color) || !read_all(origin)) {
    fprintf(stderr, "tsdf_mesh_host: short input\n");
    return 2;
  }
  UdTsdfSlotArgs a;
  a.tsdf = tsdf.data(); a.weight = W.data(); a.color = has_color ? color.data() : nullptr; a.origin = origin.data();
  a.n = (long long)n; a.vs = vs; a.min_weight = min_w; a.B = Bi; a.Nx = Nx; a.Ny = Ny; a.Nz = Nz; a.nO = nO;

  // ---- the cells -------------------------------------------------------------------------------------------------------------------
  std::vector<unsigned char> live(B * n, 0), rgb8(has_color ? B * n * 3 : 0, 0);
  std::vector<float> xyz(B * n * 3, 0.0f), normal(B * n * 3, 0.0f), rgbf(has_color ? B * n * 3 : 0, 0.0f);
  for (int b = 0; b < Bi; ++b)
    for (size_t i = 0; i < n; ++i) {
      const size_t at = (size_t)b * n + i;
      float p[3], c[3] = {0.0f, 0.0f, 0.0f}, g[3], p2[3];
      const bool counted = ud_tsdf_cell(a, b, (long long)i, nullptr, nullptr, nullptr);
      const bool full = ud_tsdf_cell(a, b, (long long)i, p, c, g);
      const bool plain = ud_tsdf_cell(a, b, (long long)i, p2, nullptr, nullptr);
      if (counted != full || plain != full || (full && memcmp(p, p2, sizeof(p)))) {
        fprintf(stderr, "tsdf_mesh_host: cell %zu depends on which outputs are asked for\n", at);
        return 3;
      }
      if (!full) continue;
      live[at] = 1;
      for (int k = 0; k < 3; ++k) {
        xyz[at * 3 + k] = p[k];
        normal[at * 3 + k] = g[k];
        if (has_color) {
          rgbf[at * 3 + k] = c[k];
          rgb8[at * 3 + k] = ud_rm_to_u8(c[k]);
        }
      }
    }

  // ---- the quads: cell_live reads the flags above, as the slot kernels read the cell mask ----------------------------------------------
  std::vector<unsigned char> quad_live(B * S, 0);
  std::vector<int32_t> quad(B * S * 4, 0);
  bool escaped = false;
  for (int b = 0; b < Bi; ++b) {
    const unsigned char* mine = live.data() + (size_t)b * n;
    auto cell_live = [&](long long i) {
      if (i < 0 || i >= (long long)n) {
        escaped = true;
        return false;
      }
      return mine[i] != 0;
    };
    for (size_t s = 0; s < S; ++s) {
      const size_t at = (size_t)b * S + s;
      int q[4];
      const bool counted = ud_tsdf_quad(a, b, (long long)s, cell_live, (int*)nullptr);
      const bool full = ud_tsdf_quad(a, b, (long long)s, cell_live, q);
      if (counted != full || escaped) {
        fprintf(stderr, "tsdf_mesh_host: quad of slot %zu: the predicate depends on the payload, or a cell outside the grid was asked for\n", at);
        return 3;
      }
      if (!full) continue;
      quad_live[at] = 1;
      for (int k = 0; k < 4; ++k) quad[at * 4 + k] = q[k];
    }
  }
  return write_all(live) && write_all(xyz) && write_all(normal) && write_all(rgbf) && write_all(rgb8) && write_all(quad_live) && write_all(quad)
             ? 0
             : 1;
}
