// The per-image style tables of a SEAN norm without a library GEMM: dsee_style_table_fwd = ops._style_gemm + dsee_style_table_layout
// in one kernel,
//   table[n][tap][row][r] = sum_s wst[tap*rows + row][s] * style[n][r][s]     r <  L
//                         = 0                                                 L <= r < 32
// Per image a [32 x S] . [S x 9 rows] product in exact fp32 on v_mfma_f32_16x16x4_f32 with the (padded) label axis as the MFMA rows:
// a wave keeps the image's whole style matrix (two 16-label tiles, K = S <= 128 per pass) in registers and walks 16-column tiles
// q = tap*rows + row of wst; result register j of lane l is table[q0 + (l & 15)][4 (l >> 4) + j], so a lane stores its four labels
// as one 16-byte word and the 64 lanes of a tile two 64-byte halves of sixteen 128-byte table rows.  Operands are read as 16-byte
// words: lane group g = l >> 4 holds k = 16 j + 4 g + c in component c of its j-th word and MFMA step (j, c) reduces those four k,
// for the style tile and the weight tile alike -- a fixed permutation of the summation order, a function of S alone.  One writer
// per element, no atomics on the table; max |T| goes into the 64-line slot by the order-independent atomic maximum every producer
// of an operand bound uses (dsee_common.h).
#include "dsee_common.h"

namespace {

constexpr int KJ = 8;              // 16-byte words of K per lane and pass: 16 KJ = 128 reduction elements
constexpr int QT_PER_WAVE = 4;     // weight tiles a wave walks per block (grid-stride beyond)

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__global__ __launch_bounds__(256) void style_table_kernel(const float* __restrict__ style, const float* __restrict__ wst,
                                                          float* __restrict__ table, int L, int S, int qtiles,
                                                          float* __restrict__ amax) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c16 = lane & 15, g = lane >> 4;
  const int n = blockIdx.y;
  const float* sty = style + (size_t)n * L * S;
  float* out = table + (size_t)n * qtiles * 16 * 32;
  const int passes = (S + 16 * KJ - 1) / (16 * KJ);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 a[2][KJ];      // style[n][16 t + c16][k0 + 16 j + 4 g ..]: the A operand of both label tiles for one pass
  auto load_style = [&](int k0) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int r = 16 * t + c16, k = k0 + 16 * j + 4 * g;
        a[t][j] = (r < L && k < S) ? ld4(sty + (size_t)r * S + k) : zero;
      }
  };
  if (passes == 1) load_style(0);
  float vmax = 0.f;
  for (int qt = blockIdx.x * 4 + wave; qt < qtiles; qt += gridDim.x * 4) {      // (wave-uniform)
    const float* wrow = wst + (size_t)(qt * 16 + c16) * S;
    f32x4 acc[2] = {zero, zero};
    for (int p = 0; p < passes; ++p) {
      const int k0 = p * 16 * KJ;
      if (passes > 1) load_style(k0);
      f32x4 b[KJ];
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int k = k0 + 16 * j + 4 * g;
        b[j] = k < S ? ld4(wrow + k) : zero;
      }
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        if (k0 + 16 * j >= S) break;      // (wave-uniform: words past S hold zeros on both sides)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][j][c], b[j][c], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][j][c], b[j][c], acc[1], 0, 0, 0);
        }
      }
    }
    // acc[t][i] = T[label 16 t + 4 g + i][q = 16 qt + c16]; labels >= L multiplied zeros: exactly 0
    float* orow = out + (size_t)(qt * 16 + c16) * 32 + 4 * g;
    *reinterpret_cast<f32x4*>(orow) = acc[0];
    *reinterpret_cast<f32x4*>(orow + 16) = acc[1];
    vmax = fmaxf(vmax, fmaxf(dsee_absmax4(acc[0]), dsee_absmax4(acc[1])));
  }
  if (amax) dsee_block_atomic_absmax(amax, vmax);      // (block-uniform condition: every thread arrives)
}

}  // namespace

extern "C" {

int dsee_style_table_fwd(const float* style, const float* wst, float* table, int N, int L, int S, int rows, float* amax,
                         hipStream_t st) {
  static const char* who = "dsee_style_table_fwd";
  if (!(style && wst && table)) {
    dsee_set_error("%s: NULL argument", who);
    return DSEE_EINVAL;
  }
  if (N < 1 || N > 65535 || L < 1 || L > 32 || S < 4 || S % 4 != 0 || rows < 64 || rows % 64 != 0) {
    dsee_set_error("%s: 1 <= L <= 32, S %% 4 == 0, rows %% 64 == 0 and 1 <= N <= 65535 required (N = %d, L = %d, S = %d, "
                   "rows = %d): a wave owns 16 table rows of all 32 label columns", who, N, L, S, rows);
    return DSEE_EUNSUPPORTED;
  }
  const int qtiles = 9 * rows / 16;
  const int gx = (qtiles + 4 * QT_PER_WAVE - 1) / (4 * QT_PER_WAVE);
  style_table_kernel<<<dim3(gx, N), 256, 0, st>>>(style, wst, table, L, S, qtiles, amax);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

}  // extern "C"
