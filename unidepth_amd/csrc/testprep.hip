// Validation inputs of a batch (include/unidepth_hip.h, UdResizeAA): crop / zero-pad to a window, separable antialiased resize (bicubic
// a = -0.5 or bilinear, ATen's _compute_indices_min_size_weights_aa), round to uint8, /255 and normalise, the validity mask with the
// NEAREST rule and the pinhole intrinsics -- the device form of the reference's test-time ContextCrop + /255 + TF.normalize
// (unidepth/datasets/pipelines/transforms.py:1131-1355, datasets/image_dataset.py:132-159) and of F.interpolate(antialias=True).
//
// ONE launch:  grid.z = image * planes + plane (planes = C image channels + the mask plane), grid.y x grid.x = tiles of
// TP_TH x TP_TW destination pixels.  A workgroup
//   1. computes the weight tables of its TP_TW + 3 columns and TP_TH rows into LDS once (one thread per column / row),
//   2. walks the source rows its tile needs, all at once or in chunks that fit the stage: stages the chunk's span of window columns into LDS as fp32
//      (zeros outside the image; 16-byte loads over the aligned body of every row, scalar head and tail), then runs the horizontal
//      pass from the stage into the intermediate rows, which stay in LDS,
//   3. runs the vertical pass from the intermediate: a thread owns 4 consecutive destination pixels of one row and stores them as one
//      vector (16 bytes fp32, 4 bytes uint8).  The quads are laid over the row from its last 16-byte (4-byte) boundary, which is why a
//      tile carries 3 extra columns on its left; rows that do not start on a boundary get a scalar head and tail.
// The mask plane needs no filter: its workgroups read the nearest source byte directly.
// Tile sizes follow from the compile-time bound UD_RESIZE_MAX_SCALE on in / out per axis (the host refuses a call beyond it): at most
// UD_RESIZE_MAX_TAPS taps, TP_SPAN staged columns and TP_MID intermediate rows.  The LDS is dynamic: the host sizes the tables, the stage
// and the intermediate for the call's own scale factors (upper bounds from the same formulas, never above the compile-time ones), so
// an up-scale or a mild down-scale keeps 8 workgroups per CU in flight and stages all its rows at once, where the largest down-scale
// uses 53 KB.  Every count is clamped to these bounds in the kernel as well, and every source index to the image, so no descriptor
// content reaches outside a buffer.
// Built with -ffp-contract=off (csrc/build.sh): every product and sum rounds on its own and the numpy fp32 restatement
// (tools/make_golden_testprep.py) reproduces the bits.
#include "ud_common.h"

namespace {

#pragma clang fp contract(off)

constexpr int TP_TW = 64;                                       // destination columns per tile (quads start up to 3 pixels earlier)
constexpr int TP_TH = 8;                                        // destination rows per tile
constexpr int TP_COLS = TP_TW + 3;                              // columns with a weight table
constexpr int TP_MIDLD = TP_COLS + 1;
constexpr int TP_THREADS = 256;
constexpr int TP_TAPS = UD_RESIZE_MAX_TAPS;
constexpr int TP_STAGE_BYTES = 16384;                           // stage budget: all of a tile's rows when they fit, else chunks
constexpr int TP_SPAN = (TP_COLS - 1) * UD_RESIZE_MAX_SCALE + TP_TAPS + 3;   // 564: window columns one tile can touch
constexpr int TP_MID = (TP_TH - 1) * UD_RESIZE_MAX_SCALE + TP_TAPS + 3;      // 92: window rows one tile can touch
static_assert(TP_TAPS == 4 * UD_RESIZE_MAX_SCALE + 1, "taps of the bicubic filter at the largest scale");
static_assert(TP_SPAN % 4 == 0, "staged rows keep 16-byte alignment in LDS");
static_assert(TP_STAGE_BYTES + TP_MID * TP_MIDLD * 4 + (TP_COLS + TP_TH) * (TP_TAPS + 2) * 4 <= 65536, "LDS at the largest scale");
static_assert(TP_STAGE_BYTES / (TP_SPAN * 4) >= 4, "a chunk holds at least one row per wave");

struct TpArgs {
  const void* src; void* dst;
  const unsigned char* mask_src; unsigned char* mask_dst;
  const float* K_in; float* K_out;
  int B, C, h, w, top, left, height, width, Ho, Wo, dtop, dleft, Hn, Wn;
  int src_u8, filter, out_form, planes;
  int taps, span, mid, chunk;                                   // LDS strides / bounds of this call: taps per pixel, staged columns
                                                                // (a multiple of 4), intermediate rows, rows staged at once
  float mean[4], inv_std[4];
};

__device__ __forceinline__ int tp_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ float tp_filter(float x, int filter) {
  x = fabsf(x);
  if (filter == UD_RESIZE_BILINEAR) return x < 1.0f ? 1.0f - x : 0.0f;
  const float a = -0.5f;
  if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
  if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * a;
  return 0.0f;
}

// first tap, tap count and normalised weights of virtual destination index i along an axis of n_in window samples and n_out samples
__device__ void tp_axis(int i, int n_in, int n_out, int filter, int max_taps, int& xmin, int& xsize, float* w) {
  if (n_in == n_out) {
    xmin = tp_clampi(i, 0, n_in - 1);
    xsize = 1;
    w[0] = 1.0f;
    return;
  }
  const float scale = (float)n_in / (float)n_out;
  const float big = scale >= 1.0f ? scale : 1.0f;
  const float support = ((filter == UD_RESIZE_BILINEAR ? 2.0f : 4.0f) * 0.5f) * big;
  const float inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
  const float center = scale * ((float)i + 0.5f);
  int lo = (int)(center - support + 0.5f);
  lo = lo > 0 ? lo : 0;
  int hi = (int)(center + support + 0.5f);
  hi = hi < n_in ? hi : n_in;
  lo = tp_clampi(lo, 0, n_in - 1);
  int n = tp_clampi(hi - lo, 1, n_in - lo);
  n = n < max_taps ? n : max_taps;
  float total = 0.0f;
  for (int j = 0; j < n; ++j) {
    const float v = tp_filter(((float)(j + lo) - center + 0.5f) * inv, filter);
    w[j] = v;
    total = j == 0 ? v : total + v;
  }
  for (int j = 0; j < n; ++j) w[j] = w[j] / total;
  xmin = lo;
  xsize = n;
}

__device__ __forceinline__ int tp_nearest(int o, int n_in, int n_out) {
  const float scale = (float)n_in / (float)n_out;
  const int s = (int)floorf((float)o * scale);
  return tp_clampi(s, 0, n_in - 1);
}

// one source row's window columns [c0, c0 + n) as fp32 into st[0 .. n): zeros outside the image, vector loads over the aligned body
template <typename T>
__device__ __forceinline__ void tp_stage_row(const T* row, bool row_inside, int w, int left, int c0, int n, float* st, int lane) {
  constexpr int E = 16 / (int)sizeof(T);                        // elements per 16-byte load
  // image columns [a, b) are the part of the span that exists; st[0 .. za) and st[zb .. n) are padding
  const int lo = left + c0;
  const int a = tp_clampi(lo, 0, w), b = tp_clampi(lo + n, 0, w);
  if (!row_inside || b <= a) {
    for (int k = lane; k < n; k += UD_WAVE) st[k] = 0.0f;
    return;
  }
  const int za = a - lo, zb = b - lo;                           // 0 <= za < zb <= n
  for (int k = lane; k < za; k += UD_WAVE) st[k] = 0.0f;
  for (int k = zb + lane; k < n; k += UD_WAVE) st[k] = 0.0f;
  const int mis = (int)(((uintptr_t)(row + a) / sizeof(T)) & (E - 1));
  int head = (E - mis) & (E - 1);
  head = head < b - a ? head : b - a;
  const int nv = (b - a - head) / E;
  const int tail0 = a + head + nv * E;
  for (int k = a + lane; k < a + head; k += UD_WAVE) st[k - lo] = (float)row[k];
  for (int k = tail0 + lane; k < b; k += UD_WAVE) st[k - lo] = (float)row[k];
  for (int v = lane; v < nv; v += UD_WAVE) {
    const int k = a + head + v * E;
    float* o = st + (k - lo);
    if constexpr (sizeof(T) == 4) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(row + k);
      o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
    } else {
      const uint4 q = *reinterpret_cast<const uint4*>(row + k);
      const unsigned int u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int t = 0; t < 16; ++t) o[t] = (float)((u[t >> 2] >> (8 * (t & 3))) & 0xffu);
    }
  }
}

__device__ __forceinline__ unsigned int tp_byte(float v) {
  const float r = fminf(fmaxf(rintf(v), 0.0f), 255.0f);
  return (unsigned int)r;
}

__global__ __launch_bounds__(TP_THREADS) void ud_resize_aa_kernel(const TpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  float* const s_stage = s_dyn;                                 // [chunk][span]
  float* const s_mid = s_stage + a.chunk * a.span;              // [mid][TP_MIDLD]
  float* const s_cw = s_mid + a.mid * TP_MIDLD;                 // [TP_COLS][taps]
  float* const s_rw = s_cw + TP_COLS * a.taps;                  // [TP_TH][taps]
  int* const s_cmin = reinterpret_cast<int*>(s_rw + TP_TH * a.taps);
  int* const s_cn = s_cmin + TP_COLS;
  int* const s_rmin = s_cn + TP_COLS;
  int* const s_rn = s_rmin + TP_TH;

  const int tid = threadIdx.x;
  const int b = (int)blockIdx.z / a.planes, c = (int)blockIdx.z - b * a.planes;
  const int x_base = (int)blockIdx.x * TP_TW - 3;               // destination column of table entry 0
  const int y_base = (int)blockIdx.y * TP_TH;

  if (a.K_in && blockIdx.x == 0 && blockIdx.y == 0 && c == 0 && tid == 0) {
    const float* Ki = a.K_in + (size_t)b * 9;
    float* Ko = a.K_out + (size_t)b * 9;
    const float zoom = (float)((double)a.Ho / (double)a.height);
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = Ki[i];
    k[2] = k[2] - (float)a.left;
    k[5] = k[5] - (float)a.top;
#pragma unroll
    for (int i = 0; i < 6; ++i) k[i] = k[i] * zoom;
#pragma unroll
    for (int i = 0; i < 9; ++i) Ko[i] = k[i];
  }

  const int ty = tid >> 4, q = tid & 15;                        // vertical pass / mask: 8 rows x 16 quads (threads 0 .. 127)
  const int y = y_base + ty;

  if (c >= a.C) {                                               // ---- the mask plane: nearest source byte, no LDS
    if (!a.mask_dst || tid >= TP_TH * 16 || y >= a.Hn) return;
    unsigned char* drow = a.mask_dst + ((size_t)b * a.Hn + y) * (size_t)a.Wn;
    const int mis = (int)((uintptr_t)drow & 3);
    const int xs = (int)blockIdx.x * TP_TW + q * 4 - mis;
    if (xs >= a.Wn) return;
    const int sy = a.top + tp_nearest(y + a.dtop, a.height, a.Ho);
    const bool yin = sy >= 0 && sy < a.h;
    const unsigned char* srow = a.mask_src ? a.mask_src + ((size_t)b * a.h + tp_clampi(sy, 0, a.h - 1)) * (size_t)a.w : nullptr;
    unsigned int v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = xs + j;
      if (x < 0 || x >= a.Wn) continue;
      const int sx = a.left + tp_nearest(x + a.dleft, a.width, a.Wo);
      if (yin && sx >= 0 && sx < a.w) v[j] = srow ? (unsigned int)srow[sx] : 1u;
    }
    if (xs >= 0 && xs + 3 < a.Wn) {
      *reinterpret_cast<unsigned int*>(drow + xs) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xs + j >= 0 && xs + j < a.Wn) drow[xs + j] = (unsigned char)v[j];
    }
    return;
  }

  // ---- 1. weight tables
  if (tid < TP_COLS) {
    const int ox = tp_clampi(x_base + tid, 0, a.Wn - 1) + a.dleft;
    int lo, n;
    tp_axis(ox, a.width, a.Wo, a.filter, a.taps, lo, n, s_cw + tid * a.taps);
    s_cmin[tid] = lo;
    s_cn[tid] = n;
  } else if (tid >= 128 && tid < 128 + TP_TH) {
    const int r = tid - 128;
    const int oy = tp_clampi(y_base + r, 0, a.Hn - 1) + a.dtop;
    int lo, n;
    tp_axis(oy, a.height, a.Ho, a.filter, a.taps, lo, n, s_rw + r * a.taps);
    s_rmin[r] = lo;
    s_rn[r] = n;
  }
  __syncthreads();
  // the window columns / rows of this tile (the tables are monotone in the destination index)
  const int c0 = s_cmin[0];
  int cspan = s_cmin[TP_COLS - 1] + s_cn[TP_COLS - 1] - c0;
  cspan = tp_clampi(cspan, 1, a.span);
  const int r0 = s_rmin[0];
  int rspan = s_rmin[TP_TH - 1] + s_rn[TP_TH - 1] - r0;
  rspan = tp_clampi(rspan, 1, a.mid);

  // ---- 2. stage a.chunk window rows, horizontal pass into s_mid
  const int wave = tid >> 6, lane = tid & 63;
  const size_t plane_off = ((size_t)b * a.C + c) * (size_t)a.h * (size_t)a.w;
  for (int rc = 0; rc < rspan; rc += a.chunk) {
    const int nr = rspan - rc < a.chunk ? rspan - rc : a.chunk;
    for (int r = wave; r < nr; r += TP_THREADS / UD_WAVE) {
      const int sy = a.top + r0 + rc + r;                       // image row of window row r0 + rc + r
      const bool inside = sy >= 0 && sy < a.h;
      const size_t ro = plane_off + (size_t)tp_clampi(sy, 0, a.h - 1) * (size_t)a.w;
      if (a.src_u8)
        tp_stage_row(reinterpret_cast<const unsigned char*>(a.src) + ro, inside, a.w, a.left, c0, cspan, s_stage + r * a.span, lane);
      else
        tp_stage_row(reinterpret_cast<const float*>(a.src) + ro, inside, a.w, a.left, c0, cspan, s_stage + r * a.span, lane);
    }
    __syncthreads();
    for (int i = tid; i < nr * TP_COLS; i += TP_THREADS) {
      const int r = i / TP_COLS, k = i - r * TP_COLS;
      const float* wk = s_cw + k * a.taps;
      const int n = s_cn[k];
      int o = s_cmin[k] - c0;
      o = tp_clampi(o, 0, cspan - 1);
      const int nn = n < cspan - o ? n : cspan - o;
      const float* sr = s_stage + r * a.span + o;
      float acc = wk[0] * sr[0];
      for (int j = 1; j < nn; ++j) acc = acc + wk[j] * sr[j];
      s_mid[(rc + r) * TP_MIDLD + k] = acc;
    }
    __syncthreads();
  }

  // ---- 3. vertical pass, one quad per thread
  if (tid >= TP_TH * 16 || y >= a.Hn) return;
  const size_t row_off = (((size_t)b * a.C + c) * a.Hn + y) * (size_t)a.Wn;
  const bool f32_out = a.out_form != UD_RESIZE_OUT_U8;
  const uintptr_t daddr = (uintptr_t)a.dst + row_off * (f32_out ? 4 : 1);
  const int mis = f32_out ? (int)((daddr >> 2) & 3) : (int)(daddr & 3);
  const int xs = (int)blockIdx.x * TP_TW + q * 4 - mis;         // first pixel of this thread's quad (>= -3)
  if (xs >= a.Wn) return;
  const float* wr = s_rw + ty * a.taps;
  int ro = s_rmin[ty] - r0;
  ro = tp_clampi(ro, 0, rspan - 1);
  const int rn = s_rn[ty] < rspan - ro ? s_rn[ty] : rspan - ro;
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = xs + j - x_base;                              // table column, 0 .. TP_COLS - 1
    if (xs + j < 0 || xs + j >= a.Wn) continue;
    const float* m = s_mid + ro * TP_MIDLD + k;
    float acc = wr[0] * m[0];
    for (int t = 1; t < rn; ++t) acc = acc + wr[t] * m[t * TP_MIDLD];
    v[j] = acc;
  }
  if (a.out_form == UD_RESIZE_OUT_U8) {
    unsigned char* drow = reinterpret_cast<unsigned char*>(a.dst) + row_off;
    unsigned int u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = tp_byte(v[j]);
    if (xs >= 0 && xs + 3 < a.Wn) {
      *reinterpret_cast<unsigned int*>(drow + xs) = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xs + j >= 0 && xs + j < a.Wn) drow[xs + j] = (unsigned char)u[j];
    }
    return;
  }
  if (a.out_form == UD_RESIZE_OUT_NORM) {
    const float mean = a.mean[c & 3], inv_std = a.inv_std[c & 3];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ((float)tp_byte(v[j]) / 255.0f - mean) * inv_std;
  }
  float* drow = reinterpret_cast<float*>(a.dst) + row_off;
  if (xs >= 0 && xs + 3 < a.Wn) {
    *reinterpret_cast<f32x4*>(drow + xs) = (f32x4){v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (xs + j >= 0 && xs + j < a.Wn) drow[xs + j] = v[j];
  }
}

}  // namespace

extern "C" int ud_resize_aa(const UdResizeAA* desc, void* stream) {
  if (!desc) {
    ud_set_error("ud_resize_aa: null descriptor");
    return UD_ERR_BAD_ARG;
  }
  const UdResizeAA& d = *desc;
  if (!d.src || !d.dst) {
    ud_set_error("ud_resize_aa: null pointer (src or dst)");
    return UD_ERR_BAD_ARG;
  }
  if (d.B < 1 || d.C < 1 || d.h < 1 || d.w < 1 || d.height < 1 || d.width < 1 || d.Ho < 1 || d.Wo < 1 || d.Hn < 1 || d.Wn < 1 ||
      (long long)d.B * (d.C + 1) > 65535) {
    ud_set_error("ud_resize_aa: bad sizes (B, C, h, w, height, width, Ho, Wo, Hn, Wn >= 1, B * (C + 1) <= 65535)");
    return UD_ERR_BAD_ARG;
  }
  const long long lim = 1LL << 29;
  if (d.top < -lim || d.top > lim || d.left < -lim || d.left > lim || d.height > lim || d.width > lim || d.h > lim || d.w > lim) {
    ud_set_error("ud_resize_aa: bad window (|top|, |left|, height, width, h, w <= 2^29)");
    return UD_ERR_BAD_ARG;
  }
  if (d.dtop < 0 || d.dleft < 0 || (long long)d.dtop + d.Hn > d.Ho || (long long)d.dleft + d.Wn > d.Wo) {
    ud_set_error("ud_resize_aa: bad destination window (0 <= dtop, dtop + Hn <= Ho, 0 <= dleft, dleft + Wn <= Wo)");
    return UD_ERR_BAD_ARG;
  }
  if ((long long)d.height > (long long)UD_RESIZE_MAX_SCALE * d.Ho || (long long)d.width > (long long)UD_RESIZE_MAX_SCALE * d.Wo) {
    ud_set_error("ud_resize_aa: down-scaling beyond UD_RESIZE_MAX_SCALE (8) per axis is not supported");
    return UD_ERR_BAD_ARG;
  }
  if (d.filter != UD_RESIZE_BICUBIC && d.filter != UD_RESIZE_BILINEAR) {
    ud_set_error("ud_resize_aa: bad filter (UD_RESIZE_BICUBIC or UD_RESIZE_BILINEAR)");
    return UD_ERR_BAD_ARG;
  }
  if (d.out_form != UD_RESIZE_OUT_F32 && d.out_form != UD_RESIZE_OUT_U8 && d.out_form != UD_RESIZE_OUT_NORM) {
    ud_set_error("ud_resize_aa: bad out_form (UD_RESIZE_OUT_F32, _U8 or _NORM)");
    return UD_ERR_BAD_ARG;
  }
  if (d.out_form == UD_RESIZE_OUT_NORM && d.C > 4) {
    ud_set_error("ud_resize_aa: UD_RESIZE_OUT_NORM needs C <= 4");
    return UD_ERR_BAD_ARG;
  }
  if ((!d.src_u8 && ((uintptr_t)d.src & 3)) || (d.out_form != UD_RESIZE_OUT_U8 && ((uintptr_t)d.dst & 3))) {
    ud_set_error("ud_resize_aa: fp32 src / dst must be 4-byte aligned");
    return UD_ERR_BAD_ARG;
  }
  if (d.mask_src && !d.mask_dst) {
    ud_set_error("ud_resize_aa: mask_src without mask_dst");
    return UD_ERR_BAD_ARG;
  }
  if ((d.K_in == nullptr) != (d.K_out == nullptr)) {
    ud_set_error("ud_resize_aa: K_in and K_out go together (null pointer)");
    return UD_ERR_BAD_ARG;
  }
  TpArgs a;
  a.src = d.src; a.dst = d.dst; a.mask_src = d.mask_src; a.mask_dst = d.mask_dst; a.K_in = d.K_in; a.K_out = d.K_out;
  a.B = d.B; a.C = d.C; a.h = d.h; a.w = d.w; a.top = d.top; a.left = d.left; a.height = d.height; a.width = d.width;
  a.Ho = d.Ho; a.Wo = d.Wo; a.dtop = d.dtop; a.dleft = d.dleft; a.Hn = d.Hn; a.Wn = d.Wn;
  a.src_u8 = d.src_u8 ? 1 : 0; a.filter = d.filter; a.out_form = d.out_form;
  a.planes = d.C + (d.mask_dst ? 1 : 0);
  for (int i = 0; i < 4; ++i) {
    a.mean[i] = d.mean[i];
    a.inv_std[i] = d.inv_std[i];
  }
  // LDS of this call: upper bounds of what one tile touches at the call's own scale factors (an axis that is copied has one tap)
  const int interp = d.filter == UD_RESIZE_BILINEAR ? 2 : 4;
  auto axis_taps = [&](int n_in, int n_out) {
    if (n_in == n_out) return 1;
    const double sc = (double)n_in / (double)n_out;
    const int t = (int)(interp * (sc > 1.0 ? sc : 1.0)) + 3;
    return t < TP_TAPS ? t : TP_TAPS;
  };
  auto axis_span = [&](int n_in, int n_out, int steps, int taps, int cap) {
    const double sc = (double)n_in / (double)n_out;
    const int v = (int)(steps * sc) + taps + 3;
    return v < cap ? v : cap;
  };
  const int taps_x = axis_taps(d.width, d.Wo), taps_y = axis_taps(d.height, d.Ho);
  a.taps = taps_x > taps_y ? taps_x : taps_y;
  a.span = (axis_span(d.width, d.Wo, TP_COLS - 1, taps_x, TP_SPAN) + 3) & ~3;
  a.mid = axis_span(d.height, d.Ho, TP_TH - 1, taps_y, TP_MID);
  a.chunk = TP_STAGE_BYTES / (a.span * 4);
  a.chunk = a.chunk > a.mid ? a.mid : (a.chunk & ~3);          // all rows at once, or a multiple of the four waves (>= 4: span <= 564)
  const int lds = 4 * (a.chunk * a.span + a.mid * TP_MIDLD + (TP_COLS + TP_TH) * a.taps + 2 * (TP_COLS + TP_TH));
  // a row's quads start at its last vector boundary: up to 3 pixels before the row
  const long long gx = ((long long)d.Wn + 3 + TP_TW - 1) / TP_TW, gy = ((long long)d.Hn + TP_TH - 1) / TP_TH;
  if (gx > 0x7fffffffLL || gy > 65535) {
    ud_set_error("ud_resize_aa: bad sizes (too many tiles for one launch: Hn <= 524280)");
    return UD_ERR_BAD_ARG;
  }
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)(d.B * a.planes));
  hipLaunchKernelGGL(ud_resize_aa_kernel, grid, dim3(TP_THREADS), lds, (hipStream_t)stream, a);
  UD_CHECK_LAUNCH("ud_resize_aa launch");
  return UD_OK;
}
