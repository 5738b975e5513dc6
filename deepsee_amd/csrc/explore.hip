// Explorative inference (sr_model.py:219-444 of the reference): the style matrices of every (image, variant) pair of a batch in
// one launch, and the result tensor -- the variants of an image side by side, or stacked -- straight from the generator's native
// output.  Both are streaming kernels on KB- resp. image-sized data; the generator pass between them is where the time goes.
#include "dsee_common.h"

namespace {

// One thread owns a float4 of one (b, r) style row and walks the variants k = 0 .. n-1 in registers, so that a variant may read
// its predecessor (the reference's aliased style_a of inference_reference_interpolation) without a second launch.  Arithmetic of
// a masked row, one fp32 rounding per step in the reference's order (the intrinsics keep the compiler from contracting a
// multiply and an add into an fma): (alpha * A) + (beta * s1), + gamma, + noise, clamp.  An unmasked row is A, copied.
// Source rows outside [0, B) cannot be told from the host: they are clamped into the batch instead of read out of bounds.
__global__ __launch_bounds__(256) void style_explore_kernel(const float* __restrict__ s0, const float* __restrict__ s1,
                                                            const int* __restrict__ src0, const int* __restrict__ src1,
                                                            const float* __restrict__ alpha, const float* __restrict__ beta,
                                                            const float* __restrict__ gamma, const float* __restrict__ noise,
                                                            const uint8_t* __restrict__ mask, float* __restrict__ out, int B,
                                                            int n, int nc, int S4, int clamp, int recurrent) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const unsigned t = i / (unsigned)S4, q = i - t * (unsigned)S4;
  const unsigned b = t / (unsigned)nc, r = t - b * (unsigned)nc;
  if (b >= (unsigned)B) return;
  const bool masked = mask[r] != 0;
  const size_t row = (size_t)r * S4 + q, mat = (size_t)nc * S4;   // in float4 units
  const f32x4* a0 = reinterpret_cast<const f32x4*>(s0);
  const f32x4* a1 = reinterpret_cast<const f32x4*>(s1);
  const f32x4* nz = reinterpret_cast<const f32x4*>(noise);
  f32x4* o = reinterpret_cast<f32x4*>(out);
  f32x4 prev = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < n; ++k) {
    const size_t pair = (size_t)b * n + k;
    f32x4 A = prev;
    if (!recurrent || k == 0) A = a0[(size_t)min(max(src0[pair], 0), B - 1) * mat + row];
    f32x4 v = A;
    if (masked) {
      const f32x4 s = a1[(size_t)min(max(src1[pair], 0), B - 1) * mat + row];
      const float al = alpha[k], be = beta[k], ga = gamma[k];
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      if (nz) z = nz[pair * mat + row];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float w = __fadd_rn(__fadd_rn(__fmul_rn(al, A[j]), __fmul_rn(be, s[j])), ga);
        if (nz) w = __fadd_rn(w, z[j]);
        if (clamp) w = w < -1.f ? -1.f : (w > 1.f ? 1.f : w);      // (a NaN stays a NaN, as in torch.clamp)
        v[j] = w;
      }
    }
    o[pair * mat + row] = v;
    prev = v;
  }
}

// One thread owns four consecutive pixels of one row of one pair: four 16-byte RGB0 loads (adjacent lanes adjacent 64 bytes),
// then per colour plane one 16-byte store where the four destination floats are whole and 16-byte aligned, single floats
// otherwise (ragged row ends, W or a column offset that is no multiple of 4).
__global__ __launch_bounds__(256) void nhwc_to_nchw_tiled_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int H,
                                                                 int W, int cs, int merge, int pair0, int pairs, int G,
                                                                 int vec_in, int vec_out) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const unsigned t = i / (unsigned)G, g = i - t * (unsigned)G;
  const unsigned p = t / (unsigned)H, h = t - p * (unsigned)H;
  if (p >= (unsigned)pairs) return;
  const int w0 = (int)g * 4, cnt = min(4, W - w0);
  float px[4][3];
  const float* src = x + (((size_t)p * H + h) * W + w0) * cs;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    px[j][0] = px[j][1] = px[j][2] = 0.f;
    if (j >= cnt) continue;
    if (vec_in) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)j * cs);
      px[j][0] = v[0]; px[j][1] = v[1]; px[j][2] = v[2];
    } else {
      px[j][0] = src[(size_t)j * cs]; px[j][1] = src[(size_t)j * cs + 1]; px[j][2] = src[(size_t)j * cs + 2];
    }
  }
  const unsigned pair = (unsigned)pair0 + p, b = pair / (unsigned)n, k = pair - b * (unsigned)n;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t e = merge ? (((size_t)b * 3 + c) * H + h) * ((size_t)n * W) + (size_t)k * W + w0
                           : (((size_t)pair * 3 + c) * H + h) * (size_t)W + w0;
    if (vec_out && cnt == 4 && (e & 3) == 0) {
      *reinterpret_cast<f32x4*>(y + e) = (f32x4){px[0][c], px[1][c], px[2][c], px[3][c]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) y[e + j] = px[j][c];
    }
  }
}

}  // namespace

extern "C" {

int dsee_style_explore(const float* s0, const float* s1, const int32_t* src0, const int32_t* src1, const float* alpha,
                       const float* beta, const float* gamma, const float* noise, const uint8_t* mask, float* out, int B, int n,
                       int nc, int S, int clamp, int recurrent, hipStream_t st) {
  DSEE_CHECK_ARG(s0 && s1 && src0 && src1 && alpha && beta && gamma && mask && out);
  DSEE_CHECK_ARG(B > 0 && n > 0 && nc > 0 && nc <= 32 && S > 0 && S % 4 == 0);
  DSEE_CHECK_ARG((long)B * n * nc * (S / 4) < (1L << 31));
  DSEE_CHECK_ARG((uintptr_t)s0 % 16 == 0 && (uintptr_t)s1 % 16 == 0 && (uintptr_t)noise % 16 == 0 && (uintptr_t)out % 16 == 0);
  DSEE_CHECK_ARG(out != s0 && out != s1);
  style_explore_kernel<<<dsee_cdiv((long)B * nc * (S / 4), 256), 256, 0, st>>>(s0, s1, src0, src1, alpha, beta, gamma, noise, mask,
                                                                              out, B, n, nc, S / 4, clamp, recurrent);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_nhwc_to_nchw_tiled(const float* x, float* y, int B, int n, int H, int W, int cs, int merge, int pair0, int pairs,
                            hipStream_t st) {
  DSEE_CHECK_ARG(x && y && B > 0 && n > 0 && H > 0 && W > 0 && cs >= 3);
  DSEE_CHECK_ARG(pair0 >= 0 && pairs > 0 && (long)pair0 + pairs <= (long)B * n);
  const int G = (W + 3) / 4;
  DSEE_CHECK_ARG((long)pairs * H * G < (1L << 31) && (long)B * n < (1L << 31));
  const int vec_in = (cs % 4 == 0 && (uintptr_t)x % 16 == 0) ? 1 : 0;
  const int vec_out = ((uintptr_t)y % 16 == 0) ? 1 : 0;
  nhwc_to_nchw_tiled_kernel<<<dsee_cdiv((long)pairs * H * G, 256), 256, 0, st>>>(x, y, n, H, W, cs, merge, pair0, pairs, G, vec_in,
                                                                                vec_out);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

}  // extern "C"
