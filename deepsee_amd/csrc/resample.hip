// Load-time geometry of the input pipeline on the device (deepsee_amd/resample.py builds the tables, deepsee_amd/data.py calls):
//   dsee_resample_u8   Pillow's 8-bit separable resize (Image.resize with BICUBIC / BILINEAR / NEAREST on 'RGB' and 'L' images),
//                      bit for bit, with the centre crop as a source box and the random crop as an output window
//   dsee_resample_u8_ragged   the same two passes over a batch whose samples differ in source size: one arena + an item table
//   dsee_interp_down   F.interpolate(hr, (S, S), mode = bilinear | nearest | area) + clamp(-1, 1)  (data/preprocessor.py:29-33)
//   dsee_resize_hw     F.interpolate(x, (OH, OW), mode = bicubic | bilinear | nearest | area) [+ clamp(-1, 1)], down or up: the LR
//                      image of a non-square batch (Preprocessor.downsample_image(hr, shape=(h, w))) and its bicubic 'baseline'
#include "dsee_common.h"
#include "dsee_interp.h"

namespace {

inline int rgrid(long n) { return (int)min(8192L, (n + 255) / 256); }

// One axis of Pillow's ImagingResample for 8-bit pixels: acc = 1 << 21; acc += pixel * k over the taps; clip8(acc >> 22).
// Integer arithmetic only; `>>` of a negative int is an arithmetic shift on this target, as in Pillow's clip8 lookup.
constexpr int RS_BITS = 22;
__device__ __forceinline__ uint8_t rs_clip8(int acc) {
  const int v = acc >> RS_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// A table row is (first source index, tap count, k[0 .. kmax - 1]).  `rows` holds (first source row, row count) per sample: the
// source rows the sample's output window reads through its vertical taps.  tmp[n][r][xo][c] = horizontal pass of source row
// rows[2n] + r, r < rows[2n + 1].  Indices are clamped to the source box: a malformed table cannot read outside it.
template <int C>
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ tmp, int N,
                                                         long n_stride, int row_stride, int box_w, int box_h, int Wo,
                                                         int tmp_rows, const int32_t* __restrict__ xtab, int kx,
                                                         const int32_t* __restrict__ rows) {
  const long total = (long)N * tmp_rows * Wo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wo);
    const long t = i / Wo;
    const int r = (int)(t % tmp_rows), n = (int)(t / tmp_rows);
    const int sr = rows[2 * n] + r;
    if (r >= rows[2 * n + 1] || sr < 0 || sr >= box_h) continue;
    const int32_t* tab = xtab + ((long)n * Wo + xo) * (2 + kx);
    const int first = max(tab[0], 0);
    const int cnt = min(min(tab[1], kx), box_w - first);
    const uint8_t* p = src + n * n_stride + (long)sr * row_stride + (long)first * C;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_BITS - 1);
    for (int k = 0; k < cnt; ++k) {
      const int kk = tab[2 + k];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += (int)p[k * C + c] * kk;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) tmp[i * C + c] = rs_clip8(acc[c]);
  }
}

// dst[n][yo][xo][c] = vertical pass over tmp; the `first` of a ytab row counts from the sample's first tmp row
template <int C>
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ tmp, uint8_t* __restrict__ dst, int N, int Wo,
                                                         int Ho, int tmp_rows, const int32_t* __restrict__ ytab, int ky,
                                                         const int32_t* __restrict__ rows) {
  const long total = (long)N * Ho * Wo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wo);
    const long t = i / Wo;
    const int yo = (int)(t % Ho), n = (int)(t / Ho);
    const int32_t* tab = ytab + ((long)n * Ho + yo) * (2 + ky);
    const int first = max(tab[0], 0);
    const int cnt = min(min(tab[1], ky), min(rows[2 * n + 1], tmp_rows) - first);
    const uint8_t* p = tmp + (((long)n * tmp_rows + first) * Wo + xo) * C;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_BITS - 1);
    for (int k = 0; k < cnt; ++k) {
      const int kk = tab[2 + k];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += (int)p[(long)k * Wo * C + c] * kk;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) dst[i * C + c] = rs_clip8(acc[c]);
  }
}

// ---- the ragged form: every sample has a source of its own inside one arena of src_bytes bytes, described by a row of `items`
// (byte offset of the box's first pixel, row stride in bytes, box_w, box_h).  The two passes and their arithmetic are those above.

// One output pixel of either pass: `cnt` taps over pixels `step` bytes apart, from the coefficients k[0 .. cnt - 1]
template <int C>
__device__ __forceinline__ void rs_taps(const uint8_t* __restrict__ p, long step, const int32_t* __restrict__ k, int cnt,
                                        uint8_t* __restrict__ out) {
  int acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_BITS - 1);
  for (int t = 0; t < cnt; ++t) {
    const int kk = k[t];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += (int)p[t * step + c] * kk;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[c] = rs_clip8(acc[c]);
}

struct rs_item {
  long off, stride;
  int bw, bh;
};

// Sample n's item row; false (the sample is skipped by both passes) unless its whole box lies inside the arena.  The bounds on
// box_h and the stride keep (box_h - 1) * stride inside a long.
template <int C>
__device__ __forceinline__ bool rs_item_load(const int64_t* __restrict__ items, int n, long src_bytes, rs_item& it) {
  const long off = items[4 * n], stride = items[4 * n + 1], bw = items[4 * n + 2], bh = items[4 * n + 3];
  if (off < 0 || bw <= 0 || bh <= 0 || bw > (1L << 24) || bh > (1L << 24) || stride < bw * C || stride > (1L << 38)) return false;
  if (bw * C > src_bytes || off > src_bytes - bw * C || (bh - 1) * stride > src_bytes - bw * C - off) return false;
  it.off = off, it.stride = stride, it.bw = (int)bw, it.bh = (int)bh;
  return true;
}

template <int C>
__global__ __launch_bounds__(256) void resample_h_ragged_kernel(const uint8_t* __restrict__ src, long src_bytes,
                                                                const int64_t* __restrict__ items, uint8_t* __restrict__ tmp, int N,
                                                                int Wo, int tmp_rows, const int32_t* __restrict__ xtab, int kx,
                                                                const int32_t* __restrict__ rows) {
  const long total = (long)N * tmp_rows * Wo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wo);
    const long t = i / Wo;
    const int r = (int)(t % tmp_rows), n = (int)(t / tmp_rows);
    rs_item it;
    if (!rs_item_load<C>(items, n, src_bytes, it)) continue;
    const int sr = rows[2 * n] + r;
    if (r >= rows[2 * n + 1] || sr < 0 || sr >= it.bh) continue;
    const int32_t* tab = xtab + ((long)n * Wo + xo) * (2 + kx);
    const int first = min(max(tab[0], 0), it.bw);
    const int cnt = min(min(tab[1], kx), it.bw - first);
    rs_taps<C>(src + it.off + (long)sr * it.stride + (long)first * C, C, tab + 2, cnt, tmp + i * C);
  }
}

template <int C>
__global__ __launch_bounds__(256) void resample_v_ragged_kernel(const uint8_t* __restrict__ tmp, uint8_t* __restrict__ dst,
                                                                long src_bytes, const int64_t* __restrict__ items, int N, int Wo,
                                                                int Ho, int tmp_rows, const int32_t* __restrict__ ytab, int ky,
                                                                const int32_t* __restrict__ rows) {
  const long total = (long)N * Ho * Wo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wo);
    const long t = i / Wo;
    const int yo = (int)(t % Ho), n = (int)(t / Ho);
    rs_item it;
    if (!rs_item_load<C>(items, n, src_bytes, it)) continue;
    const int32_t* tab = ytab + ((long)n * Ho + yo) * (2 + ky);
    const int avail = min(rows[2 * n + 1], tmp_rows);
    const int first = min(max(tab[0], 0), max(avail, 0));
    const int cnt = min(min(tab[1], ky), avail - first);
    rs_taps<C>(tmp + (((long)n * tmp_rows + first) * Wo + xo) * C, (long)Wo * C, tab + 2, cnt, dst + i * C);
  }
}

// NHWC [N][H][W][cs_in] -> [N][S][S][cs_out], 3 channels (the rest of cs_out zero); sh = (float)H / S, sw = (float)W / S from the
// host (dsee_interp.h: dsee_interp_px)
__global__ __launch_bounds__(256) void interp_down_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W,
                                                          int S, int cs_in, int cs_out, int mode, float sh, float sw) {
  const long total = (long)N * S * S;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ow = (int)(i % S);
    const long t = i / S;
    const int oh = (int)(t % S), n = (int)(t / S);
    const float* img = x + (size_t)n * H * W * cs_in;
    float v[3] = {0.f, 0.f, 0.f};
    dsee_interp_px(img, H, W, S, S, cs_in, mode, sh, sw, oh, ow, v);
    float* o = y + (size_t)i * cs_out;
    for (int c = 0; c < cs_out; ++c) o[c] = c < 3 ? fminf(fmaxf(v[c], -1.f), 1.f) : 0.f;
  }
}

// NHWC [N][H][W][cs_in] -> [N][OH][OW][cs_out], one thread per output pixel, mode = bilinear | nearest | area: interp_down_kernel
// with one output size per axis and an optional clamp (the same dsee_interp_px)
__global__ __launch_bounds__(256) void resize_hw_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W,
                                                        int OH, int OW, int cs_in, int cs_out, int mode, int clamp, float sh,
                                                        float sw) {
  const long total = (long)N * OH * OW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ow = (int)(i % OW);
    const long t = i / OW;
    const int oh = (int)(t % OH), n = (int)(t / OH);
    const float* img = x + (size_t)n * H * W * cs_in;
    float v[3] = {0.f, 0.f, 0.f};
    dsee_interp_px(img, H, W, OH, OW, cs_in, mode, sh, sw, oh, ow, v);
    float* o = y + (size_t)i * cs_out;
    for (int c = 0; c < cs_out; ++c) o[c] = c < 3 ? (clamp ? fminf(fmaxf(v[c], -1.f), 1.f) : v[c]) : 0.f;
  }
}

}  // namespace

extern "C" {

int dsee_resample_u8(const uint8_t* src, uint8_t* tmp, uint8_t* dst, int N, int C, long src_off, long src_n_stride,
                     int src_row_stride, int box_w, int box_h, int Wo, int Ho, int tmp_rows, const int32_t* xtab, int kx,
                     const int32_t* ytab, int ky, const int32_t* rows, hipStream_t st) {
  DSEE_CHECK_ARG(src && tmp && dst && xtab && ytab && rows && (C == 1 || C == 3));
  DSEE_CHECK_ARG(N > 0 && box_w > 0 && box_h > 0 && Wo > 0 && Ho > 0 && tmp_rows > 0 && tmp_rows <= box_h && kx > 0 && ky > 0);
  DSEE_CHECK_ARG(src_off >= 0 && src_row_stride >= box_w * C && src_n_stride >= (long)src_row_stride * (box_h - 1) + box_w * C);
  const long nh = (long)N * tmp_rows * Wo, nv = (long)N * Ho * Wo;
  if (C == 3) {
    resample_h_kernel<3><<<rgrid(nh), 256, 0, st>>>(src + src_off, tmp, N, src_n_stride, src_row_stride, box_w, box_h, Wo,
                                                    tmp_rows, xtab, kx, rows);
    resample_v_kernel<3><<<rgrid(nv), 256, 0, st>>>(tmp, dst, N, Wo, Ho, tmp_rows, ytab, ky, rows);
  } else {
    resample_h_kernel<1><<<rgrid(nh), 256, 0, st>>>(src + src_off, tmp, N, src_n_stride, src_row_stride, box_w, box_h, Wo,
                                                    tmp_rows, xtab, kx, rows);
    resample_v_kernel<1><<<rgrid(nv), 256, 0, st>>>(tmp, dst, N, Wo, Ho, tmp_rows, ytab, ky, rows);
  }
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_resample_u8_ragged(const uint8_t* src, long src_bytes, const int64_t* items, uint8_t* tmp, uint8_t* dst, int N, int C,
                            int Wo, int Ho, int tmp_rows, const int32_t* xtab, int kx, const int32_t* ytab, int ky,
                            const int32_t* rows, hipStream_t st) {
  DSEE_CHECK_ARG(src && items && tmp && dst && xtab && ytab && rows && (C == 1 || C == 3));
  DSEE_CHECK_ARG(src_bytes > 0 && N > 0 && Wo > 0 && Ho > 0 && tmp_rows > 0 && kx > 0 && ky > 0);
  const long nh = (long)N * tmp_rows * Wo, nv = (long)N * Ho * Wo;
  if (C == 3) {
    resample_h_ragged_kernel<3><<<rgrid(nh), 256, 0, st>>>(src, src_bytes, items, tmp, N, Wo, tmp_rows, xtab, kx, rows);
    resample_v_ragged_kernel<3><<<rgrid(nv), 256, 0, st>>>(tmp, dst, src_bytes, items, N, Wo, Ho, tmp_rows, ytab, ky, rows);
  } else {
    resample_h_ragged_kernel<1><<<rgrid(nh), 256, 0, st>>>(src, src_bytes, items, tmp, N, Wo, tmp_rows, xtab, kx, rows);
    resample_v_ragged_kernel<1><<<rgrid(nv), 256, 0, st>>>(tmp, dst, src_bytes, items, N, Wo, Ho, tmp_rows, ytab, ky, rows);
  }
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_interp_down(const float* x, float* y, int N, int H, int W, int S, int cs_in, int cs_out, int mode, hipStream_t st) {
  DSEE_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && S > 0 && cs_in >= 3 && cs_out >= 3);
  DSEE_CHECK_ARG(mode == INTERP_BILINEAR || mode == INTERP_NEAREST || mode == INTERP_AREA);
  interp_down_kernel<<<rgrid((long)N * S * S), 256, 0, st>>>(x, y, N, H, W, S, cs_in, cs_out, mode, (float)H / (float)S,
                                                             (float)W / (float)S);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_resize_hw(const float* x, float* y, int N, int H, int W, int OH, int OW, int cs_in, int cs_out, int mode, int clamp,
                   hipStream_t st) {
  DSEE_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && cs_in >= 3 && cs_out >= 3);
  DSEE_CHECK_ARG(mode == INTERP_BILINEAR || mode == INTERP_NEAREST || mode == INTERP_AREA || mode == INTERP_BICUBIC);
  DSEE_CHECK_ARG(clamp == 0 || clamp == 1);
  if (mode == INTERP_BICUBIC) return dsee::launch_bicubic_hw(x, y, N, H, W, OH, OW, cs_in, cs_out, clamp, st);
  resize_hw_kernel<<<rgrid((long)N * OH * OW), 256, 0, st>>>(x, y, N, H, W, OH, OW, cs_in, cs_out, mode, clamp,
                                                             (float)H / (float)OH, (float)W / (float)OW);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

}  // extern "C"
