// Output side of the device pipeline: what the reference converts on the host after copying fp32 NCHW tensors (and a one-hot label
// map) over PCIe -- util/util.py:72-103 tensor2im, :107-135 tensor2label, :297-311 Colorize, and the side-by-side strip of
// util/visualizer.py:181-215 save_images_only -- happens here, and 3 bytes per pixel leave the card.
//
// Every kernel writes packed RGB pixels into a window of a destination (base, image stride, row stride, x offset): a per-key image
// and one column of the `combined` strip are the same kernel with another destination, nothing is concatenated afterwards.
//
// Streaming kernels.  A thread owns four destination pixels whose first has an ABSOLUTE x (offset + x) that is a multiple of 4, i.e.
// 12 bytes at a 4-byte aligned address when the base and the strides are multiples of 4: three 4-byte stores, adjacent lanes
// adjacent (a wave writes 768 contiguous bytes of a row).  Groups cut by the window's left / right edge, and destinations that are
// not 4-byte aligned, are written pixel by pixel as bytes -- nothing outside the window is touched.  Sources: a native RGB0 pixel
// is one 16-byte load; NCHW planes and uint8 sources are read per element (adjacent lanes adjacent 16 / 4 bytes).
#include "dsee_common.h"

namespace {

struct DstWin {
  uint8_t* base;
  long image_stride, row_stride;   // bytes
  int x_off;                       // pixels
  int g0, groups;                  // first 4-pixel group (absolute x / 4) a row of the window touches, and how many
  int vec;                         // base and strides are multiples of 4: whole groups leave as three 4-byte stores
};

DstWin make_win(uint8_t* dst, long image_stride, long row_stride, int x_off, int W) {
  DstWin d;
  d.base = dst;
  d.image_stride = image_stride;
  d.row_stride = row_stride;
  d.x_off = x_off;
  d.g0 = x_off / 4;
  d.groups = (x_off + W + 3) / 4 - d.g0;
  d.vec = ((uintptr_t)dst % 4 == 0 && image_stride % 4 == 0 && row_stride % 4 == 0) ? 1 : 0;
  return d;
}

bool win_ok(const uint8_t* dst, int N, int H, int W, long image_stride, long row_stride, int x_off) {
  // rows of one image and images of the batch must not overlap; the thread index is 32-bit
  return dst && N > 0 && H > 0 && W > 0 && x_off >= 0 && row_stride >= 3L * (x_off + W) &&
         (N == 1 || image_stride >= (long)(H - 1) * row_stride + 3L * (x_off + W)) &&
         (long)N * H * ((x_off + W + 3) / 4 - x_off / 4) < (1L << 31);
}

// thread i -> (image n, row y, first absolute x of its group)
__device__ __forceinline__ bool win_split(const DstWin& d, int N, int H, unsigned i, int& n, int& y, int& X0) {
  const unsigned t = i / (unsigned)d.groups, g = i - t * (unsigned)d.groups;
  n = (int)(t / (unsigned)H);
  y = (int)(t - (unsigned)n * (unsigned)H);
  X0 = (d.g0 + (int)g) * 4;
  return n < N;
}

// c[j] = 0x00BBGGRR of pixel X0 + j; pixels with x = X0 + j - x_off outside [0, W) are not written
__device__ __forceinline__ void win_store(const DstWin& d, int n, int y, int X0, int W, const uint32_t (&c)[4]) {
  uint8_t* row = d.base + (long)n * d.image_stride + (long)y * d.row_stride;
  const int x0 = X0 - d.x_off;
  if (d.vec && x0 >= 0 && x0 + 4 <= W) {
    uint32_t* p = reinterpret_cast<uint32_t*>(row + 3L * X0);
    p[0] = c[0] | (c[1] << 24);
    p[1] = (c[1] >> 8) | (c[2] << 16);
    p[2] = (c[2] >> 16) | (c[3] << 8);
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (x0 + j < 0 || x0 + j >= W) continue;
    uint8_t* p = row + 3L * (X0 + j);
    p[0] = (uint8_t)(c[j] & 0xFFu);
    p[1] = (uint8_t)((c[j] >> 8) & 0xFFu);
    p[2] = (uint8_t)(c[j] >> 16);
  }
}

// tensor2im's arithmetic, one fp32 rounding per operation (the intrinsics keep the compiler from contracting or reassociating):
// (x + 1) / 2 * 255 resp. x * 255, np.clip(., 0, 255), astype(uint8) = truncation
template <bool NORMALIZE>
__device__ __forceinline__ uint32_t quantise(float x) {
  float v = NORMALIZE ? __fmul_rn(__fdiv_rn(__fadd_rn(x, 1.0f), 2.0f), 255.0f) : __fmul_rn(x, 255.0f);
  v = fminf(fmaxf(v, 0.0f), 255.0f);
  return (uint32_t)(int)v;
}

template <bool NCHW, bool NORMALIZE>
__global__ __launch_bounds__(256) void image_to_u8_kernel(const float* __restrict__ x, DstWin d, int N, int H, int W, int cs,
                                                          int vec_in) {
  int n, y, X0;
  if (!win_split(d, N, H, blockIdx.x * 256u + threadIdx.x, n, y, X0)) return;
  uint32_t c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int xs = X0 + j - d.x_off;
    c[j] = 0;
    if (xs < 0 || xs >= W) continue;
    float r, g, b;
    if (NCHW) {
      const float* p = x + (((long)n * 3) * H + y) * W + xs;
      r = p[0];
      g = p[(long)H * W];
      b = p[2L * H * W];
    } else {
      const float* p = x + (((long)n * H + y) * W + xs) * cs;
      if (vec_in) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        r = v[0]; g = v[1]; b = v[2];
      } else {
        r = p[0]; g = p[1]; b = p[2];
      }
    }
    c[j] = quantise<NORMALIZE>(r) | (quantise<NORMALIZE>(g) << 8) | (quantise<NORMALIZE>(b) << 16);
  }
  win_store(d, n, y, X0, W, c);
}

__global__ __launch_bounds__(256) void label_colorize_kernel(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ table,
                                                             int n_colors, DstWin d, int N, int H, int W) {
  __shared__ uint32_t cmap[256];   // 0x00BBGGRR, 0 from n_colors on
  {
    const int i = threadIdx.x;
    cmap[i] = i < n_colors ? (uint32_t)table[i * 3] | ((uint32_t)table[i * 3 + 1] << 8) | ((uint32_t)table[i * 3 + 2] << 16) : 0u;
  }
  __syncthreads();
  int n, y, X0;
  if (!win_split(d, N, H, blockIdx.x * 256u + threadIdx.x, n, y, X0)) return;
  const uint8_t* row = lab + ((long)n * H + y) * W;
  const int x0 = X0 - d.x_off;
  uint32_t c[4];
  if (x0 >= 0 && x0 + 4 <= W && ((uintptr_t)(row + x0) & 3) == 0) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(row + x0);
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = cmap[(v >> (8 * j)) & 0xFFu];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = (x0 + j >= 0 && x0 + j < W) ? cmap[row[x0 + j]] : 0u;
  }
  win_store(d, n, y, X0, W, c);
}

// one thread per output pixel: 16 source pixels (one 16-byte load each in the native layout), 3 channels
__global__ __launch_bounds__(256) void bicubic_up_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int S, int H,
                                                         int W, int cs_in, int cs_out, int clamp, int vec_in, int vec_out) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const unsigned t = i / (unsigned)W, ow = i - t * (unsigned)W, n = t / (unsigned)H, oh = t - n * (unsigned)H;
  if (n >= (unsigned)N) return;
  const float sh = (float)S / (float)H, sw = (float)S / (float)W;   // area_pixel_compute_scale, align_corners = False
  const float fy = __fsub_rn(__fmul_rn(sh, (float)oh + 0.5f), 0.5f), fx = __fsub_rn(__fmul_rn(sw, (float)ow + 0.5f), 0.5f);
  const int iy = (int)floorf(fy), ix = (int)floorf(fx);
  float wy[4], wx[4];
  cubic_coeffs(fy - iy, wy);
  cubic_coeffs(fx - ix, wx);
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int yy = min(max(iy - 1 + a, 0), S - 1);
    float row[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int xx = min(max(ix - 1 + b, 0), S - 1);
      const float* p = x + (((long)n * S + yy) * S + xx) * cs_in;
      float v[3];
      if (vec_in) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
      } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) row[c] += wx[b] * v[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += wy[a] * row[c];
  }
  if (clamp) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = fminf(fmaxf(acc[c], -1.f), 1.f);
  }
  float* o = y + (long)i * cs_out;
  if (vec_out) {
    *reinterpret_cast<f32x4*>(o) = (f32x4){acc[0], acc[1], acc[2], 0.f};
  } else {
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    for (int c = 3; c < cs_out; ++c) o[c] = 0.f;
  }
}

// source coordinate of destination index d: i0 = floor(f), t = f - i0, neighbours clamped
__device__ __forceinline__ void bilinear_src(int d, float scale, int S, int& i0, int& i1, float& t) {
  const float f = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)d, 0.5f)), 0.5f);
  const float fl = floorf(f);
  t = __fsub_rn(f, fl);
  i0 = min(max((int)fl, 0), S - 1);
  i1 = min(max((int)fl + 1, 0), S - 1);
}

__device__ __forceinline__ float lerp_rn(float a, float b, float t) {
  return __fadd_rn(__fmul_rn(__fsub_rn(1.0f, t), a), __fmul_rn(t, b));
}

__global__ __launch_bounds__(256) void bilinear_up_u8_kernel(const uint8_t* __restrict__ src, long src_image_stride,
                                                             long src_row_stride, int S, DstWin d, int N, int H, int W) {
  int n, y, X0;
  if (!win_split(d, N, H, blockIdx.x * 256u + threadIdx.x, n, y, X0)) return;
  const float sh = (float)S / (float)H, sw = (float)S / (float)W;
  int y0, y1;
  float ty;
  bilinear_src(y, sh, S, y0, y1, ty);
  const uint8_t* r0 = src + (long)n * src_image_stride + (long)y0 * src_row_stride;
  const uint8_t* r1 = src + (long)n * src_image_stride + (long)y1 * src_row_stride;
  uint32_t c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int xd = X0 + j - d.x_off;
    c[j] = 0;
    if (xd < 0 || xd >= W) continue;
    int x0, x1;
    float tx;
    bilinear_src(xd, sw, S, x0, x1, tx);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float top = lerp_rn((float)r0[x0 * 3 + ch], (float)r0[x1 * 3 + ch], tx);
      const float bot = lerp_rn((float)r1[x0 * 3 + ch], (float)r1[x1 * 3 + ch], tx);
      const float v = floorf(__fadd_rn(lerp_rn(top, bot, ty), 0.5f));      // in [0, 255]: a convex combination of bytes
      c[j] |= (uint32_t)(int)fminf(fmaxf(v, 0.f), 255.f) << (8 * ch);
    }
  }
  win_store(d, n, y, X0, W, c);
}

inline unsigned win_grid(const DstWin& d, int N, int H) { return (unsigned)dsee_cdiv((long)N * H * d.groups, 256); }

}  // namespace

extern "C" {

int dsee_image_to_u8(const float* x, uint8_t* dst, int N, int H, int W, int cs, int nchw, int normalize, long dst_image_stride,
                     long dst_row_stride, int dst_x_offset, hipStream_t st) {
  DSEE_CHECK_ARG(x && (nchw || cs >= 3));
  DSEE_CHECK_ARG(win_ok(dst, N, H, W, dst_image_stride, dst_row_stride, dst_x_offset));
  const DstWin d = make_win(dst, dst_image_stride, dst_row_stride, dst_x_offset, W);
  const int vec_in = (!nchw && cs % 4 == 0 && (uintptr_t)x % 16 == 0) ? 1 : 0;
  const unsigned grid = win_grid(d, N, H);
  if (nchw) {
    if (normalize) image_to_u8_kernel<true, true><<<grid, 256, 0, st>>>(x, d, N, H, W, cs, vec_in);
    else image_to_u8_kernel<true, false><<<grid, 256, 0, st>>>(x, d, N, H, W, cs, vec_in);
  } else {
    if (normalize) image_to_u8_kernel<false, true><<<grid, 256, 0, st>>>(x, d, N, H, W, cs, vec_in);
    else image_to_u8_kernel<false, false><<<grid, 256, 0, st>>>(x, d, N, H, W, cs, vec_in);
  }
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_label_colorize(const uint8_t* labels, const uint8_t* table, int n_colors, uint8_t* dst, int N, int H, int W,
                        long dst_image_stride, long dst_row_stride, int dst_x_offset, hipStream_t st) {
  DSEE_CHECK_ARG(labels && table && n_colors > 0 && n_colors <= 256);
  DSEE_CHECK_ARG(win_ok(dst, N, H, W, dst_image_stride, dst_row_stride, dst_x_offset));
  const DstWin d = make_win(dst, dst_image_stride, dst_row_stride, dst_x_offset, W);
  label_colorize_kernel<<<win_grid(d, N, H), 256, 0, st>>>(labels, table, n_colors, d, N, H, W);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_bicubic_up(const float* x, float* y, int N, int S, int H, int W, int cs_in, int cs_out, int clamp, hipStream_t st) {
  DSEE_CHECK_ARG(x && y && N > 0 && S > 0 && H >= S && W >= S && cs_in >= 3 && cs_out >= 3);
  DSEE_CHECK_ARG((long)N * H * W < (1L << 31));
  const int vec_in = (cs_in % 4 == 0 && (uintptr_t)x % 16 == 0) ? 1 : 0;
  const int vec_out = (cs_out == 4 && (uintptr_t)y % 16 == 0) ? 1 : 0;
  bicubic_up_kernel<<<dsee_cdiv((long)N * H * W, 256), 256, 0, st>>>(x, y, N, S, H, W, cs_in, cs_out, clamp, vec_in, vec_out);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_bilinear_up_u8(const uint8_t* src, long src_image_stride, long src_row_stride, int S, uint8_t* dst, int N, int H, int W,
                        long dst_image_stride, long dst_row_stride, int dst_x_offset, hipStream_t st) {
  DSEE_CHECK_ARG(src && S > 0 && H >= S && W >= S && src_row_stride >= 3L * S);
  DSEE_CHECK_ARG(N == 1 || src_image_stride >= (long)(S - 1) * src_row_stride + 3L * S);
  DSEE_CHECK_ARG(win_ok(dst, N, H, W, dst_image_stride, dst_row_stride, dst_x_offset));
  const DstWin d = make_win(dst, dst_image_stride, dst_row_stride, dst_x_offset, W);
  bilinear_up_u8_kernel<<<win_grid(d, N, H), 256, 0, st>>>(src, src_image_stride, src_row_stride, S, d, N, H, W);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

}  // extern "C"
