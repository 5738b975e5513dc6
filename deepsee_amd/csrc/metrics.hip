// PSNR / SSIM / RMSE of generated against ground-truth images on the device (reference:
// evaluator/evaluation.py:88-137 -> evaluator/calculate_PSNR_SSIM.py:71-122 on util/util.py:72-103 `tensor2im` images).
//
// Reference semantics kept to the letter:
//   * both images are first quantised like tensor2im: u = uint8(clip((x + 1) / 2 * 255, 0, 255)) -- fp32 arithmetic in that
//     order, truncation;
//   * PSNR = 20 log10(255 / sqrt(mean((u_f - u_r)^2))) over all H*W*3 values (inf for identical images); the squared
//     differences are summed as integers, i.e. exactly;
//   * SSIM: 11x11 Gaussian window (sigma 1.5, cv2.getGaussianKernel: exp(-(i-5)^2 / (2 sigma^2)) normalised in double),
//     "valid" region only ([5:-5, 5:-5]), C1 = (0.01*255)^2, C2 = (0.03*255)^2, float64, mean of the SSIM map over the valid
//     pixels and the three channels (calculate_ssim's channel loop passes the whole image three times: the mean over
//     positions and channels IS its result);
//   * RMSE = sqrt(mean((x_f - x_r)^2)) on the [-1, 1] tensors (evaluation.py:107-110; fp32 there, float64 sums here).
// Two launches: per-block partial sums into the caller's workspace (blocks = N x 3 channels x 16x16-pixel tiles, no
// atomics), then one block per image adds them in a fixed order: the result does not depend on scheduling.
#include "dsee_common.h"

namespace {

constexpr int TS = 16;            // output tile edge
constexpr int HALO = 5;
constexpr int IN = TS + 2 * HALO; // 26

struct GaussWindow { double w[11]; };

__device__ __forceinline__ float to_u8(float x) {
  // (x + 1) / 2 * 255 with fp32 rounding after every operation (no contraction into an fma), clip, truncate
  float v = __fmul_rn(__fadd_rn(x, 1.0f) * 0.5f, 255.0f);
  v = fminf(fmaxf(v, 0.0f), 255.0f);
  return floorf(v);
}

// partial[block][4] = {sum of SSIM map values, integer sum of squared u8 differences, sum of squared [-1,1] differences,
// unused}; blocks of image n: n * per_image .. + per_image - 1
__global__ __launch_bounds__(256) void psnr_ssim_partial_kernel(const float* __restrict__ fake, const float* __restrict__ real,
                                                               double* __restrict__ partial, int H, int W, int Cs,
                                                               int tiles_x, int tiles_y, GaussWindow g) {
  __shared__ float sf[IN][IN + 1], sr[IN][IN + 1];
  __shared__ double hz[5][IN][TS];   // horizontally filtered x, y, xx, yy, xy
  __shared__ double red[3][4];
  const int tile = blockIdx.x % (tiles_x * tiles_y), c = (blockIdx.x / (tiles_x * tiles_y)) % 3;
  const int n = blockIdx.x / (tiles_x * tiles_y * 3);
  const int ty0 = (tile / tiles_x) * TS, tx0 = (tile % tiles_x) * TS;   // tile origin in VALID coordinates
  const int tid = threadIdx.x;
  const float* pf = fake + (long)n * H * W * Cs + c;
  const float* pr = real + (long)n * H * W * Cs + c;
  // the block's own 16x16 pixels of the full image (for PSNR / RMSE every pixel must be counted exactly once: tile
  // (ty, tx) of the full-image tiling owns pixels [16 ty, 16 ty + 16) x [16 tx, 16 tx + 16); the valid-region tiling has
  // fewer tiles, the launch covers ceil(H/16) x ceil(W/16) tiles and SSIM positions outside the valid region are skipped)
  double se_u8 = 0.0, se_f = 0.0, ss = 0.0;
  {
    const int y = ty0 + tid / TS, x = tx0 + tid % TS;
    if (y < H && x < W) {
      const float a = pf[((long)y * W + x) * Cs], b = pr[((long)y * W + x) * Cs];
      const float d8 = to_u8(a) - to_u8(b);
      se_u8 = (double)(d8 * d8);
      const double df = (double)a - (double)b;
      se_f = df * df;
    }
  }
  // SSIM: valid position (vy, vx) in [0, H-10) x [0, W-10) reads image rows vy .. vy+10
  const int VH = H - 2 * HALO, VW = W - 2 * HALO;
  if (ty0 < VH && tx0 < VW) {
    for (int i = tid; i < IN * IN; i += 256) {
      const int yy = i / IN, xx = i % IN, y = ty0 + yy, x = tx0 + xx;
      float a = 0.f, b = 0.f;
      if (y < H && x < W) {
        a = to_u8(pf[((long)y * W + x) * Cs]);
        b = to_u8(pr[((long)y * W + x) * Cs]);
      }
      sf[yy][xx] = a;
      sr[yy][xx] = b;
    }
    __syncthreads();
    for (int i = tid; i < IN * TS; i += 256) {
      const int yy = i / TS, xo = i % TS;
      double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        const double a = sf[yy][xo + k], b = sr[yy][xo + k], w = g.w[k];
        s0 += w * a; s1 += w * b; s2 += w * a * a; s3 += w * b * b; s4 += w * a * b;
      }
      hz[0][yy][xo] = s0; hz[1][yy][xo] = s1; hz[2][yy][xo] = s2; hz[3][yy][xo] = s3; hz[4][yy][xo] = s4;
    }
    __syncthreads();
    const int yo = tid / TS, xo = tid % TS;
    if (ty0 + yo < VH && tx0 + xo < VW) {
      double m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        const double w = g.w[k];
        m1 += w * hz[0][yo + k][xo]; m2 += w * hz[1][yo + k][xo];
        e11 += w * hz[2][yo + k][xo]; e22 += w * hz[3][yo + k][xo]; e12 += w * hz[4][yo + k][xo];
      }
      const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
      const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
      const double s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
      ss = ((2 * m12 + C1) * (2 * s12 + C2)) / ((m11 + m22 + C1) * (s11 + s22 + C2));
    }
  }
  // block reduction in a fixed order: wave shuffles, then the 4 wave sums
  double v[3] = {ss, se_u8, se_f};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    double x = v[q];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((tid & 63) == 0) red[q][tid >> 6] = x;
  }
  __syncthreads();
  if (tid < 3) partial[(long)blockIdx.x * 4 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// out[n] = {psnr, ssim, rmse}
__global__ __launch_bounds__(256) void psnr_ssim_finalize_kernel(const double* __restrict__ partial, double* __restrict__ out,
                                                                int per_image, int H, int W) {
  __shared__ double red[3][256];
  const int n = blockIdx.x, tid = threadIdx.x;
  double s[3] = {0, 0, 0};
  for (int i = tid; i < per_image; i += 256)
#pragma unroll
    for (int q = 0; q < 3; ++q) s[q] += partial[((long)n * per_image + i) * 4 + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) red[q][tid] = s[q];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
#pragma unroll
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double npix = 3.0 * H * W, nvalid = 3.0 * (H - 2 * HALO) * (W - 2 * HALO);
    const double mse = red[1][0] / npix;
    out[n * 3 + 0] = mse == 0.0 ? (double)INFINITY : 20.0 * log10(255.0 / sqrt(mse));
    out[n * 3 + 1] = red[0][0] / nvalid;
    out[n * 3 + 2] = sqrt(red[2][0] / npix);
  }
}

// ---- MS-SSIM (reference: evaluator/ssim.py:24-118 as evaluation.py:114,125-127 calls it) -------------------------------------
// Five SSIM passes over an average-pooled pyramid.  What is kept to the letter:
//   * input (x + 1) * 127.5, not quantised, not clipped;
//   * the window of a level is k x k, k = min(11, h, w), and is the float64 outer product of the normalised Gaussian ROUNDED TO
//     fp32 (create_window ends in .float()), the Gaussian's own values being fp32 as well (gaussian() builds a torch.Tensor).
//     The rounded window is not rank 1 and its weights do not sum to 1: a separable pass is off by ~1e-7 in cs, two orders
//     above the bound this kernel is held to, so the convolution is the plain 2-D one (k*k taps) with exactly these weights;
//   * output = prod(cs[:4]^w[:4] * sim[4]^w[4]): ssim.py:117 multiplies EACH of the four cs terms by sim_4^w_4 before the
//     product, i.e. sim_4^w_4 enters with the 4th power.  That is what a reference metrics.csv holds, so it is what is computed;
//   * nothing is clamped: a negative base gives NaN.
// Everything after the fp32 load is float64 (the reference convolves in fp32; tests/golden/ms_ssim/ms_ssim.json records both).
// Launches: 4 poolings (level l -> l+1, planar float64 pyramids in the workspace), 5 per-level partial kernels (blocks =
// N x 3 channels x 16x16-position tiles, partial sums to the workspace, no atomics), 1 finalize block per image.
constexpr int MS_LEVELS = 5;
constexpr int MS_KMAX = 11;
constexpr int MS_IN = TS + MS_KMAX - 1;   // 26

struct MsWindow { double w[MS_KMAX * MS_KMAX]; };   // row-major k x k, the fp32 weights widened

__host__ __device__ inline int ms_dim(int d, int l) { return d >> l; }   // floor halving l times
__host__ __device__ inline int ms_k(int h, int w) { return min(MS_KMAX, min(h, w)); }
__host__ __device__ inline long ms_tiles(int h, int w) {
  const int k = ms_k(h, w);
  return (long)((h - k + 1 + TS - 1) / TS) * ((w - k + 1 + TS - 1) / TS);
}
// doubles of the pyramid levels 1..4 of ONE image set (fake or real) before level l
__host__ __device__ inline long ms_pyr_offset(int N, int H, int W, int l) {
  long o = 0;
  for (int i = 1; i < l; ++i) o += (long)N * 3 * ms_dim(H, i) * ms_dim(W, i);
  return o;
}
// partial blocks before level l
__host__ __device__ inline long ms_part_offset(int N, int H, int W, int l) {
  long o = 0;
  for (int i = 0; i < l; ++i) o += (long)N * 3 * ms_tiles(ms_dim(H, i), ms_dim(W, i));
  return o;
}

__device__ __forceinline__ double ms_to255(float x) { return ((double)x + 1.0) * 127.5; }

// level l -> l + 1 of both images: out[n][c][y][x] = mean of the 2x2 block.  FIRST: the source is the fp32 NHWC input.
template <bool FIRST>
__global__ __launch_bounds__(256) void ms_pool_kernel(const float* __restrict__ f32_f, const float* __restrict__ f32_r,
                                                      const double* __restrict__ src_f, const double* __restrict__ src_r,
                                                      double* __restrict__ dst_f, double* __restrict__ dst_r, int N, int h,
                                                      int w, int Cs) {
  const int ho = h >> 1, wo = w >> 1;
  const long total = (long)N * 3 * ho * wo;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % wo), y = (int)((i / wo) % ho), c = (int)((i / ((long)wo * ho)) % 3);
  const long n = i / ((long)wo * ho * 3);
  double a[2][4];
  if (FIRST) {
    const long base = ((n * h + 2 * y) * w + 2 * x) * Cs + c;
    const long o[4] = {0, (long)Cs, (long)w * Cs, (long)(w + 1) * Cs};
#pragma unroll
    for (int q = 0; q < 4; ++q) { a[0][q] = ms_to255(f32_f[base + o[q]]); a[1][q] = ms_to255(f32_r[base + o[q]]); }
  } else {
    const long base = ((n * 3 + c) * h + 2 * y) * w + 2 * x;
    const long o[4] = {0, 1, (long)w, (long)w + 1};
#pragma unroll
    for (int q = 0; q < 4; ++q) { a[0][q] = src_f[base + o[q]]; a[1][q] = src_r[base + o[q]]; }
  }
  dst_f[i] = (((a[0][0] + a[0][1]) + a[0][2]) + a[0][3]) * 0.25;
  dst_r[i] = (((a[1][0] + a[1][1]) + a[1][2]) + a[1][3]) * 0.25;
}

// partial[block][2] = {sum of cs, sum of the SSIM map} over the block's valid positions.  FIRST: level 0, read from the fp32
// NHWC input; otherwise from the planar float64 pyramid.  KT = 11: unrolled taps; KT = 0: k < 11 at run time (levels <= 10 wide).
template <bool FIRST, int KT>
__global__ __launch_bounds__(256) void ms_ssim_partial_kernel(const float* __restrict__ f32_f, const float* __restrict__ f32_r,
                                                              const double* __restrict__ src_f,
                                                              const double* __restrict__ src_r, double* __restrict__ partial,
                                                              int h, int w, int Cs, int k_rt, int tiles_x, int tiles_y,
                                                              MsWindow g) {
  __shared__ double sx[MS_IN][MS_IN + 1], sy[MS_IN][MS_IN + 1];
  __shared__ double red[2][4];
  const int k = KT ? KT : k_rt;
  const int tile = blockIdx.x % (tiles_x * tiles_y), c = (blockIdx.x / (tiles_x * tiles_y)) % 3;
  const long n = blockIdx.x / (tiles_x * tiles_y * 3);
  const int ty0 = (tile / tiles_x) * TS, tx0 = (tile % tiles_x) * TS, tid = threadIdx.x;
  const int in = TS + k - 1;
  for (int i = tid; i < in * in; i += 256) {
    const int yy = i / in, xx = i % in, y = ty0 + yy, x = tx0 + xx;
    double a = 0.0, b = 0.0;
    if (y < h && x < w) {
      if (FIRST) {
        const long o = ((n * h + y) * w + x) * Cs + c;
        a = ms_to255(f32_f[o]);
        b = ms_to255(f32_r[o]);
      } else {
        const long o = ((n * 3 + c) * h + y) * w + x;
        a = src_f[o];
        b = src_r[o];
      }
    }
    sx[yy][xx] = a;
    sy[yy][xx] = b;
  }
  __syncthreads();
  const int yo = tid / TS, xo = tid % TS;
  double cs = 0.0, sim = 0.0;
  if (ty0 + yo < h - k + 1 && tx0 + xo < w - k + 1) {
    double m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
    auto tap = [&](int ky, int kx) {
      const double wt = g.w[ky * k + kx], a = sx[yo + ky][xo + kx], b = sy[yo + ky][xo + kx];
      const double wa = wt * a, wb = wt * b;
      m1 += wa; m2 += wb; e11 += wa * a; e22 += wb * b; e12 += wa * b;
    };
    if constexpr (KT != 0) {
#pragma unroll
      for (int ky = 0; ky < KT; ++ky)
#pragma unroll
        for (int kx = 0; kx < KT; ++kx) tap(ky, kx);
    } else {
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx) tap(ky, kx);
    }
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
    const double s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
    const double v1 = 2.0 * s12 + C2, v2 = s11 + s22 + C2;
    cs = v1 / v2;
    sim = ((2 * m12 + C1) * v1) / ((m11 + m22 + C1) * v2);
  }
  double v[2] = {cs, sim};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    double x = v[q];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((tid & 63) == 0) red[q][tid >> 6] = x;
  }
  __syncthreads();
  if (tid < 2) partial[(long)blockIdx.x * 2 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

struct MsWeights { double w[MS_LEVELS]; };

// out[n] = {ms-ssim, cs_0..cs_4, sim_0..sim_4}
__global__ __launch_bounds__(256) void ms_ssim_finalize_kernel(const double* __restrict__ partial, double* __restrict__ out,
                                                               int N, int H, int W, MsWeights wt) {
  __shared__ double red[2][256];
  __shared__ double term[2][MS_LEVELS];
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int l = 0; l < MS_LEVELS; ++l) {
    const int h = ms_dim(H, l), w = ms_dim(W, l), k = ms_k(h, w);
    const long per_image = 3 * ms_tiles(h, w);
    const double* p = partial + (ms_part_offset(N, H, W, l) + (long)n * per_image) * 2;
    double s0 = 0, s1 = 0;
    for (long i = tid; i < per_image; i += 256) { s0 += p[i * 2]; s1 += p[i * 2 + 1]; }
    red[0][tid] = s0;
    red[1][tid] = s1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
      __syncthreads();
    }
    if (tid == 0) {
      const double cnt = 3.0 * (h - k + 1) * (w - k + 1);
      term[0][l] = red[0][0] / cnt;
      term[1][l] = red[1][0] / cnt;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double last = pow(term[1][MS_LEVELS - 1], wt.w[MS_LEVELS - 1]);
    double prod = 1.0;
    for (int l = 0; l < MS_LEVELS - 1; ++l) prod *= pow(term[0][l], wt.w[l]) * last;
    double* o = out + (long)n * (1 + 2 * MS_LEVELS);
    o[0] = prod;
    for (int l = 0; l < MS_LEVELS; ++l) { o[1 + l] = term[0][l]; o[1 + MS_LEVELS + l] = term[1][l]; }
  }
}

// create_window(k): gaussian() builds an fp32 tensor of exp(-(i - k//2)^2 / (2 sigma^2)), widens it, normalises in float64;
// the float64 outer product is rounded to fp32
void ms_window(int k, MsWindow* g) {
  double g1[MS_KMAX], sum = 0.0;
  for (int i = 0; i < k; ++i) {
    const int d = i - k / 2;
    g1[i] = (double)(float)exp(-(double)(d * d) / (2.0 * 1.5 * 1.5));
    sum += g1[i];
  }
  for (int i = 0; i < k; ++i) g1[i] /= sum;
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) g->w[i * k + j] = (double)(float)(g1[i] * g1[j]);
}

}  // namespace

extern "C" {

size_t dsee_psnr_ssim_workspace(int N, int H, int W) {
  return (size_t)N * 3 * dsee_cdiv(H, TS) * dsee_cdiv(W, TS) * 4 * sizeof(double);
}

int dsee_psnr_ssim(const float* fake, const float* real, int N, int H, int W, int Cs, double* workspace,
                   size_t workspace_bytes, double* out, hipStream_t st) {
  DSEE_CHECK_ARG(fake && real && workspace && out && N > 0 && Cs >= 3 && H > 2 * HALO && W > 2 * HALO);
  DSEE_CHECK_ARG(workspace_bytes >= dsee_psnr_ssim_workspace(N, H, W));
  GaussWindow g;
  double sum = 0.0;
  for (int i = 0; i < 11; ++i) {
    g.w[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
    sum += g.w[i];
  }
  for (int i = 0; i < 11; ++i) g.w[i] /= sum;
  const int tx = dsee_cdiv(W, TS), ty = dsee_cdiv(H, TS), per_image = 3 * tx * ty;
  psnr_ssim_partial_kernel<<<N * per_image, 256, 0, st>>>(fake, real, workspace, H, W, Cs, tx, ty, g);
  DSEE_LAUNCH_CHECK();
  psnr_ssim_finalize_kernel<<<N, 256, 0, st>>>(workspace, out, per_image, H, W);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

size_t dsee_ms_ssim_workspace(int N, int H, int W) {
  if (N <= 0 || H < 16 || W < 16) return 0;
  return (size_t)(2 * ms_pyr_offset(N, H, W, MS_LEVELS) + 2 * ms_part_offset(N, H, W, MS_LEVELS)) * sizeof(double);
}

int dsee_ms_ssim(const float* fake, const float* real, int N, int H, int W, int Cs, double* workspace,
                 size_t workspace_bytes, double* out, hipStream_t st) {
  DSEE_CHECK_ARG(fake && real && workspace && out && N > 0 && Cs >= 3 && H >= 16 && W >= 16);
  DSEE_CHECK_ARG(workspace_bytes >= dsee_ms_ssim_workspace(N, H, W));
  const long pyr = ms_pyr_offset(N, H, W, MS_LEVELS);
  double* pyr_f = workspace;
  double* pyr_r = workspace + pyr;
  double* partial = workspace + 2 * pyr;
  for (int l = 0; l < MS_LEVELS; ++l) {
    const int h = ms_dim(H, l), w = ms_dim(W, l), k = ms_k(h, w);
    const double* src_f = l ? pyr_f + ms_pyr_offset(N, H, W, l) : nullptr;
    const double* src_r = l ? pyr_r + ms_pyr_offset(N, H, W, l) : nullptr;
    MsWindow g;
    ms_window(k, &g);
    const int tx = dsee_cdiv(w - k + 1, TS), ty = dsee_cdiv(h - k + 1, TS);
    const long blocks = (long)N * 3 * tx * ty;
    DSEE_CHECK_ARG(blocks < (1L << 31));
    double* part = partial + ms_part_offset(N, H, W, l) * 2;
    if (l == 0) {
      if (k == MS_KMAX)
        ms_ssim_partial_kernel<true, MS_KMAX><<<(unsigned)blocks, 256, 0, st>>>(fake, real, nullptr, nullptr, part, h, w, Cs, k,
                                                                                 tx, ty, g);
      else
        ms_ssim_partial_kernel<true, 0><<<(unsigned)blocks, 256, 0, st>>>(fake, real, nullptr, nullptr, part, h, w, Cs, k, tx,
                                                                          ty, g);
    } else {
      if (k == MS_KMAX)
        ms_ssim_partial_kernel<false, MS_KMAX><<<(unsigned)blocks, 256, 0, st>>>(nullptr, nullptr, src_f, src_r, part, h, w, Cs,
                                                                                  k, tx, ty, g);
      else
        ms_ssim_partial_kernel<false, 0><<<(unsigned)blocks, 256, 0, st>>>(nullptr, nullptr, src_f, src_r, part, h, w, Cs, k, tx,
                                                                           ty, g);
    }
    DSEE_LAUNCH_CHECK();
    if (l + 1 < MS_LEVELS) {
      const long total = (long)N * 3 * (h >> 1) * (w >> 1);
      double* dst_f = pyr_f + ms_pyr_offset(N, H, W, l + 1);
      double* dst_r = pyr_r + ms_pyr_offset(N, H, W, l + 1);
      if (l == 0)
        ms_pool_kernel<true><<<dsee_cdiv(total, 256), 256, 0, st>>>(fake, real, nullptr, nullptr, dst_f, dst_r, N, h, w, Cs);
      else
        ms_pool_kernel<false><<<dsee_cdiv(total, 256), 256, 0, st>>>(nullptr, nullptr, src_f, src_r, dst_f, dst_r, N, h, w, Cs);
      DSEE_LAUNCH_CHECK();
    }
  }
  MsWeights wt;
  const float wf[MS_LEVELS] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};
  for (int l = 0; l < MS_LEVELS; ++l) wt.w[l] = (double)wf[l];
  ms_ssim_finalize_kernel<<<N, 256, 0, st>>>(partial, out, N, H, W, wt);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

}  // extern "C"
