// Depth maps of a batch rendered as colour images (include/unidepth_hip.h, UdColorize): the device form of the reference's colorize
// (unidepth/utils/visualization.py:17-36: normalise, matplotlib's Colormap.__call__(bytes=True), black where value < 1e-4) and of its
// image_grid of equal-sized panels, for a whole batch and up to UD_COLORIZE_MAX_PANELS cells per image.
//
// At most TWO launches on `stream`:
//   1. cz_partial_kernel  only when a panel is auto-ranged: grid (chunks, cells, B); a workgroup folds CZ_CHUNK = 1024 consecutive
//                         pixels of one image's map (256 threads x 4, coalesced) into (min, max, has-NaN) -> part[b][cell][chunk]
//   2. cz_render_kernel   grid (tiles, cells, B); a workgroup stages its panel's 256-entry LUT in LDS (one packed dword per entry),
//                         reduces its image's partials (swept CZ_SWEEP = 256 at a time; min / max commute, so every workgroup of an
//                         image gets the same bits), then renders a tile of CZ_ROWS = 4 rows x CZ_QUADS = 64 quads.  A thread owns
//                         CZ_PX = 4 consecutive pixels of one row: 12 bytes (HWC) leave as three dword stores, 4 bytes per plane
//                         (CHW) as one.  The quads are laid over a row from the 4-byte boundary at or before the cell's first byte
//                         (3 W and 3 cols W are odd for odd W), so a row has a head and a tail of byte stores that touch the cell's
//                         own bytes only, and a body of aligned dwords.
// The dependency between the two is the launch boundary: no atomics, no tickets, no host synchronisation; every bit is fixed.
// Built with -ffp-contract=off (csrc/build.sh): (v - lo) / den * 256 and |g - p| / g round every operation separately, so a numpy fp32
// restatement reproduces the bytes (tools/make_golden_colorize.py).
#include "ud_common.h"

namespace {

#pragma clang fp contract(off)

constexpr int CZ_PX = 4;                     // pixels per thread
constexpr int CZ_QUADS = 64;                 // quads per tile row: one wave renders CZ_PX * CZ_QUADS = 256 pixels of a row
constexpr int CZ_ROWS = 4;                   // rows per tile
constexpr int CZ_THREADS = CZ_QUADS * CZ_ROWS;
constexpr int CZ_CHUNK = CZ_THREADS * 4;     // pixels per partial (min, max, has-NaN)
constexpr int CZ_SWEEP = CZ_THREADS;         // partials per reduction sweep
constexpr int CZ_WAVES = CZ_THREADS / UD_WAVE;
static_assert(CZ_THREADS == 256, "one thread stages one LUT entry");
static_assert((long long)UD_COLORIZE_MAX_TILES * CZ_THREADS < (1LL << 32), "a launch's x extent in threads stays below 2^32");

struct CzArgs {
  UdColorPanel panel[UD_COLORIZE_MAX_PANELS];
  unsigned char* dst;
  float* part;                               // [B][UD_COLORIZE_MAX_PANELS][nparts][3]
  int B, H, W, rows, cols, chw;
  int qblocks;                               // tiles along x
  int nparts;                                // chunks per image
};

__device__ __forceinline__ float cz_value(const UdColorPanel& P, int b, int idx) {
  const float v = ((const float*)P.src)[(size_t)b * (size_t)P.batch_stride + idx];
  if (P.kind == UD_CZ_MAP) return v;
  const float p = P.src2[(size_t)b * (size_t)P.batch_stride2 + idx];
  return v == 0.0f ? 0.0f : fabsf(v - p) / v;                        // the demo's error map: |g - p| / g, 0 where g == 0
}

// (min, max, has-NaN) over the workgroup; the result is valid in thread 0 .. every thread (read back from LDS)
__device__ __forceinline__ void cz_block_reduce(float& mn, float& mx, float& nn, float (*red)[CZ_WAVES]) {
  const int lane = threadIdx.x & (UD_WAVE - 1), w = threadIdx.x / UD_WAVE;
#pragma unroll
  for (int o = UD_WAVE / 2; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, UD_WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, o, UD_WAVE));
    nn = fmaxf(nn, __shfl_xor(nn, o, UD_WAVE));
  }
  if (lane == 0) {
    red[0][w] = mn; red[1][w] = mx; red[2][w] = nn;
  }
  __syncthreads();
  mn = red[0][0]; mx = red[1][0]; nn = red[2][0];
#pragma unroll
  for (int k = 1; k < CZ_WAVES; ++k) {
    mn = fminf(mn, red[0][k]); mx = fmaxf(mx, red[1][k]); nn = fmaxf(nn, red[2][k]);
  }
}

__global__ __launch_bounds__(CZ_THREADS) void cz_partial_kernel(const CzArgs a) {
  __shared__ float red[3][CZ_WAVES];
  const int i = blockIdx.x, k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const UdColorPanel& P = a.panel[k];
  if (!(P.flags & (UD_CZ_AUTO_LO | UD_CZ_AUTO_HI))) return;          // workgroup-uniform (the host clears the flags of non-map panels)
  const unsigned HW = (unsigned)a.H * (unsigned)a.W;                 // < 2^31
  float mn = __builtin_inff(), mx = -__builtin_inff(), nn = 0.0f;
#pragma unroll
  for (int j = 0; j < CZ_CHUNK / CZ_THREADS; ++j) {
    const unsigned idx = (unsigned)i * CZ_CHUNK + j * CZ_THREADS + tid;   // < 2^31 + CZ_CHUNK: fits unsigned
    if (idx < HW) {
      const float v = cz_value(P, b, (int)idx);
      if (v != v) {
        nn = 1.0f;
      } else {
        mn = fminf(mn, v); mx = fmaxf(mx, v);
      }
    }
  }
  cz_block_reduce(mn, mx, nn, red);
  if (tid == 0) {
    float* o = a.part + (((size_t)b * UD_COLORIZE_MAX_PANELS + k) * a.nparts + i) * 3;
    o[0] = mn; o[1] = mx; o[2] = nn;
  }
}

__global__ __launch_bounds__(CZ_THREADS) void cz_render_kernel(const CzArgs a) {
  __shared__ unsigned lut_s[256];
  __shared__ float red[3][CZ_WAVES];
  const int k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const UdColorPanel& P = a.panel[k];
  if (P.kind == UD_CZ_NONE) return;                                  // workgroup-uniform: the cell keeps its bytes
  const bool is_map = P.kind != UD_CZ_RGB;
  float lo = P.lo, den = P.den;
  if (is_map) {                                                      // workgroup-uniform branch: the barriers inside are reached by all
    const unsigned char* L = P.lut + tid * 3;
    lut_s[tid] = (unsigned)L[0] | ((unsigned)L[1] << 8) | ((unsigned)L[2] << 16);
    if (P.flags & (UD_CZ_AUTO_LO | UD_CZ_AUTO_HI)) {
      const float* pp = a.part + ((size_t)b * UD_COLORIZE_MAX_PANELS + k) * a.nparts * 3;
      float mn = __builtin_inff(), mx = -__builtin_inff(), nn = 0.0f;
      for (int i = tid; i < a.nparts; i += CZ_SWEEP) {
        mn = fminf(mn, pp[(size_t)i * 3]); mx = fmaxf(mx, pp[(size_t)i * 3 + 1]); nn = fmaxf(nn, pp[(size_t)i * 3 + 2]);
      }
      cz_block_reduce(mn, mx, nn, red);                              // its barrier also publishes lut_s
      if (nn > 0.0f) mn = mx = __builtin_nanf("");                   // ndarray.min() / max() of an image with a NaN
      lo = (P.flags & UD_CZ_AUTO_LO) ? mn : P.lo;
      const float hi = (P.flags & UD_CZ_AUTO_HI) ? mx : P.hi;
      den = hi - lo;
    } else {
      __syncthreads();
    }
  }

  const int tx = tid & (CZ_QUADS - 1), ty = tid / CZ_QUADS;
  const int bx = blockIdx.x % a.qblocks, by = blockIdx.x / a.qblocks;
  const int y = by * CZ_ROWS + ty;
  if (y >= a.H) return;
  const int r = k / a.cols, c = k - r * a.cols;
  const size_t CW = (size_t)a.cols * a.W, RH = (size_t)a.rows * a.H;
  const size_t Y = (size_t)r * a.H + y, X0 = (size_t)c * a.W;
  // first byte of this cell's row (channel 0 of it in CHW) and the pixels before the row's quad grid: the quads start where their
  // first byte is 4-byte aligned.  HWC: address + 3 xs = 0 (mod 4) <=> xs = address (mod 4); CHW: address + xs = 0 (mod 4).
  unsigned char* row0 = a.chw ? a.dst + ((size_t)b * 3 * RH + Y) * CW + X0 : a.dst + (((size_t)b * RH + Y) * CW + X0) * 3;
  const int mis = a.chw ? (int)((uintptr_t)row0 & 3) : (int)((4 - ((uintptr_t)row0 & 3)) & 3);
  const int xs = (bx * CZ_QUADS + tx) * CZ_PX - mis;                 // first pixel of this thread's quad (>= -3)
  if (xs >= a.W) return;

  unsigned col[CZ_PX];
  const int HW = a.H * a.W;
#pragma unroll
  for (int j = 0; j < CZ_PX; ++j) {
    const int x = xs + j;
    col[j] = 0;
    if (x < 0 || x >= a.W) continue;
    const int idx = y * a.W + x;
    if (is_map) {
      const float v = cz_value(P, b, idx);
      const float t = (v - lo) / den;
      const float s = t * 256.0f;
      unsigned cc;
      if (s != s) cc = 0u;                                           // matplotlib's "bad" entry: (0, 0, 0, 0)
      else if (s < 0.0f) cc = lut_s[0];
      else if (s >= 256.0f) cc = lut_s[255];
      else cc = lut_s[(int)s];
      col[j] = v < 1e-4f ? 0u : cc;                                  // the reference's invalid mask (false for a NaN)
    } else {
      const unsigned char* s = (const unsigned char*)P.src + (size_t)b * (size_t)P.batch_stride + idx;
      col[j] = (unsigned)s[0] | ((unsigned)s[HW] << 8) | ((unsigned)s[2 * (size_t)HW] << 16);
    }
  }
  const bool full = xs >= 0 && xs + CZ_PX - 1 < a.W;
  if (!a.chw) {
    unsigned char* p = row0 + 3 * (long long)xs;                     // 4-byte aligned by construction
    if (full) {
      unsigned* q = reinterpret_cast<unsigned*>(p);
      q[0] = col[0] | (col[1] << 24);
      q[1] = (col[1] >> 8) | (col[2] << 16);
      q[2] = (col[2] >> 16) | (col[3] << 8);
    } else {
#pragma unroll
      for (int j = 0; j < CZ_PX; ++j)
        if (xs + j >= 0 && xs + j < a.W) {
          p[3 * j] = (unsigned char)col[j]; p[3 * j + 1] = (unsigned char)(col[j] >> 8); p[3 * j + 2] = (unsigned char)(col[j] >> 16);
        }
    }
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      unsigned char* p = row0 + (size_t)ch * RH * CW + (long long)xs;    // planes 1 and 2 are aligned only when rows H cols W % 4 == 0
      if (full && ((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<unsigned*>(p) = ((col[0] >> (8 * ch)) & 255u) | (((col[1] >> (8 * ch)) & 255u) << 8) |
                                          (((col[2] >> (8 * ch)) & 255u) << 16) | (((col[3] >> (8 * ch)) & 255u) << 24);
      } else {
#pragma unroll
        for (int j = 0; j < CZ_PX; ++j)
          if (xs + j >= 0 && xs + j < a.W) p[j] = (unsigned char)(col[j] >> (8 * ch));
      }
    }
  }
}

int cz_nparts(int H, int W) { return (int)(((long long)H * W + CZ_CHUNK - 1) / CZ_CHUNK); }

// a row's quads start at the 4-byte boundary at or before its first byte: up to 3 pixels before the row
int cz_qblocks(int W) { return (int)((((long long)W + 3 + CZ_PX - 1) / CZ_PX + CZ_QUADS - 1) / CZ_QUADS); }
long long cz_rblocks(int H) { return ((long long)H + CZ_ROWS - 1) / CZ_ROWS; }

// sizes one launch can take: H * W indexes in 31 bits, a destination row's bytes too, and the render grid's x extent in THREADS
// (tiles * CZ_THREADS) stays below 2^32, the runtime's limit on a launch (a thin, tall image has one tile per CZ_ROWS rows)
bool cz_sizes_ok(int B, int H, int W, int cols) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || cols < 1) return false;
  if ((long long)H * W > 0x7fffffffLL || 3LL * cols * W > 0x7fffffffLL) return false;
  return cz_rblocks(H) * cz_qblocks(W) <= UD_COLORIZE_MAX_TILES;
}

}  // namespace

extern "C" long long ud_colorize_work_bytes(int B, int H, int W) {
  if (!cz_sizes_ok(B, H, W, 1)) return -1;
  return (long long)B * UD_COLORIZE_MAX_PANELS * cz_nparts(H, W) * 3 * (long long)sizeof(float);
}

extern "C" int ud_colorize(const UdColorize* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_colorize: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdColorize& d = *desc;
  if (d.rows < 1 || d.cols < 1 || d.rows > UD_COLORIZE_MAX_PANELS || d.cols > UD_COLORIZE_MAX_PANELS || d.rows * d.cols > UD_COLORIZE_MAX_PANELS) {
    ud_set_error("ud_colorize: bad grid (rows, cols >= 1, rows * cols <= UD_COLORIZE_MAX_PANELS (4))");
    return UD_ERR_BAD_ARG;
  }
  if (!cz_sizes_ok(d.B, d.H, d.W, d.cols)) {
    ud_set_error("ud_colorize: bad sizes (1 <= B <= 65535, H, W >= 1, H*W < 2^31, 3*cols*W < 2^31, ceil(H/4) * ceil((W+3)/256) < 2^24 tiles)");
    return UD_ERR_BAD_ARG;
  }
  if (d.flags & ~UD_CZ_CHW) {
    ud_set_error("ud_colorize: unknown flag");
    return UD_ERR_BAD_ARG;
  }
  if (!d.dst) {
    ud_set_error("ud_colorize: null pointer (dst)");
    return UD_ERR_BAD_ARG;
  }
  CzArgs a;
  bool any = false, autorange = false;
  const int cells = d.rows * d.cols;
  for (int i = 0; i < UD_COLORIZE_MAX_PANELS; ++i) {
    UdColorPanel p = UdColorPanel{nullptr, nullptr, nullptr, 0, 0, UD_CZ_NONE, 0, 0.0f, 0.0f, 0.0f};
    if (i < cells) p = d.panels[i];
    if (p.kind < UD_CZ_NONE || p.kind > UD_CZ_RGB || (p.flags & ~(UD_CZ_AUTO_LO | UD_CZ_AUTO_HI))) {
      ud_set_error("ud_colorize: bad panel (unknown kind or flag)");
      return UD_ERR_BAD_ARG;
    }
    if (p.kind != UD_CZ_NONE) {
      const bool is_map = p.kind != UD_CZ_RGB;
      if (!p.src || (is_map && !p.lut) || (p.kind == UD_CZ_AREL && !p.src2)) {
        ud_set_error("ud_colorize: null pointer (src, src2 or lut of a panel)");
        return UD_ERR_BAD_ARG;
      }
      if (p.batch_stride < 0 || (p.kind == UD_CZ_AREL && p.batch_stride2 < 0)) {
        ud_set_error("ud_colorize: bad panel (batch_stride >= 0)");
        return UD_ERR_BAD_ARG;
      }
      if (is_map && (((uintptr_t)p.src & 3) || (p.kind == UD_CZ_AREL && ((uintptr_t)p.src2 & 3)))) {
        ud_set_error("ud_colorize: bad panel (fp32 sources must be 4-byte aligned)");
        return UD_ERR_BAD_ARG;
      }
      if (!is_map) p.flags = 0;                                      // an rgb panel has no range
      any = true;
      autorange = autorange || p.flags != 0;
    } else {
      p.flags = 0;
    }
    a.panel[i] = p;
  }
  if (!any) {
    ud_set_error("ud_colorize: nothing to do (every cell is UD_CZ_NONE)");
    return UD_ERR_BAD_ARG;
  }
  a.nparts = cz_nparts(d.H, d.W);
  if (autorange) {
    if (!d.work || ((uintptr_t)d.work & 3)) {
      ud_set_error("ud_colorize: null pointer (work, needed by an auto-ranged panel), or work not 4-byte aligned");
      return UD_ERR_BAD_ARG;
    }
    if (d.work_bytes < ud_colorize_work_bytes(d.B, d.H, d.W)) {
      ud_set_error("ud_colorize: workspace smaller than ud_colorize_work_bytes()");
      return UD_ERR_BAD_ARG;
    }
  }
  a.dst = d.dst; a.part = (float*)d.work;
  a.B = d.B; a.H = d.H; a.W = d.W; a.rows = d.rows; a.cols = d.cols; a.chw = (d.flags & UD_CZ_CHW) ? 1 : 0;
  a.qblocks = cz_qblocks(d.W);
  const long long rblocks = cz_rblocks(d.H);                         // rblocks * qblocks <= UD_COLORIZE_MAX_TILES: checked above
  hipStream_t s = (hipStream_t)stream;
  if (autorange) hipLaunchKernelGGL(cz_partial_kernel, dim3((unsigned)a.nparts, (unsigned)cells, (unsigned)d.B), dim3(CZ_THREADS), 0, s, a);
  hipLaunchKernelGGL(cz_render_kernel, dim3((unsigned)(rblocks * a.qblocks), (unsigned)cells, (unsigned)d.B), dim3(CZ_THREADS), 0, s, a);
  UD_CHECK_LAUNCH("ud_colorize launch");
  return UD_OK;
}
