// Reflection padding of a 3x3 / stride 1 convolution as a border pass (the pix2pixHD ResnetBlock of the netG
// ablation `nospadenostyle`, reference deepsee_models/networks/ablation.py:13-29):
//
//     conv3x3(reflect_pad(x), w) = conv3x3(zero_pad(x), w) + ring(x, w)
//
// ring is non-zero on output row 0, row H-1, column 0 and column W-1 only.  At a border output p = (i, j) it is the sum over the
// taps (kh, kw) whose padded coordinate (a, b) = (i + kh - 1, j + kw - 1) lies outside the map of w[co][ci][kh][kw] x[r(a)][r(b)][ci],
// r(-1) = 1, r(H) = H - 2: 3 taps on an edge, 5 in a corner, every outside tap once.  The zero-padded layer runs on the existing
// kernels; the three entry points below add the border terms IN PLACE, each element by one writer, without atomics:
//
//   dsee_reflect_ring_fwd    y[p][co]  += sum_{tap outside at p} sum_ci x[r(p, tap)][ci] w[co][ci][tap]
//   dsee_reflect_ring_dgrad  dx[q][ci] += sum_{(p, tap): tap outside at p, r(p, tap) = q} sum_co dy[p][co] w[co][ci][tap]   (gather form:
//                            q runs over rows 1, H-2 and columns 1, W-2)
//   dsee_reflect_ring_wgrad  dw[co][ci][tap] += sum_n sum_{p: tap outside at p} dy[n][p][co] x[n][r(p, tap)][ci]
//
// All three are thin GEMMs in exact fp32 on v_mfma_f32_16x16x4_f32: a 256-thread block owns a 64 x 64 output tile (4 waves, 2 x 2
// MFMA tiles each) and walks K in LDS-staged slabs of 16.  Forward and data gradient share one kernel: a GEMM row is a pixel, and K
// runs over (slot, channel), a slot being one way a tap can reach the row's pixel; a slot no row of the tile uses is skipped, so a
// tile of 64 pixels of one edge multiplies its 3 taps only.  Per K slab the OIHW weights of the tile's columns are staged once for
// all 9 taps, read in whole contiguous runs, and the loads of the next step are in flight during the MFMAs.  The weight gradient is one GEMM per tap over the pixels that tap
// leaves the map at, K split over `splits` blocks whose partial tiles go to the workspace and are folded in split order: the
// reduction order is a function of the shape alone (bit-reproducible under graph replay).
//
// Also here, for the closing `x + InstanceNorm(conv(.))` of that block: dsee_norm_act_res_fwd, the IN + act forward with a residual.
#include "dsee_common.h"

namespace {

constexpr int TM = 64, TN = 64, TK = 16, LDT = 80;   // LDT: tile row stride in floats (16-byte aligned rows, k rows 16 banks apart)

__device__ __forceinline__ int reflect_idx(int a, int n) { return a < 0 ? -a : (a >= n ? 2 * n - 2 - a : a); }

// idx-th border pixel of an H x W map (H, W >= 2): row 0, row H-1, then column 0 and column W-1 of the rows between
__device__ __forceinline__ void border_pixel(int idx, int H, int W, int& i, int& j) {
  if (idx < W) {
    i = 0, j = idx;
  } else if (idx < 2 * W) {
    i = H - 1, j = idx - W;
  } else {
    const int t = idx - 2 * W;
    if (t < H - 2) i = 1 + t, j = 0;
    else i = 1 + t - (H - 2), j = W - 1;
  }
}
__host__ __device__ __forceinline__ int border_count(int H, int W) { return 2 * W + 2 * (H - 2); }

// the pixels a reflected tap can read = the pixels the data gradient writes: rows 1 and H-2 (one row when they coincide), then
// columns 1 and W-2 of the other rows
struct InnerRing {
  int nsr, nsc, orows, lo, hi, count;
};
__host__ __device__ __forceinline__ InnerRing inner_ring(int H, int W) {
  InnerRing r;
  r.nsr = (H - 2 != 1) ? 2 : 1;
  r.nsc = (W - 2 != 1) ? 2 : 1;
  r.orows = H - r.nsr;
  r.lo = H - 2 < 1 ? H - 2 : 1;
  r.hi = H - 2 < 1 ? 1 : H - 2;
  r.count = r.nsr * W + r.nsc * r.orows;
  return r;
}
__device__ __forceinline__ void inner_pixel(int idx, const InnerRing& r, int H, int W, int& i, int& j) {
  if (idx < W) {
    i = 1, j = idx;
  } else if (r.nsr == 2 && idx < 2 * W) {
    i = H - 2, j = idx - W;
  } else {
    const int t = idx - r.nsr * W;
    const int col = t / r.orows;
    i = t - col * r.orows;
    if (i >= r.lo) ++i;
    if (r.nsr == 2 && i >= r.hi) ++i;
    j = col == 0 ? 1 : W - 2;
  }
}

// One way tap `tap` can connect the row pixel (i, j) with another pixel (oi, oj); false: this slot does not exist at (i, j).
//   forward (9 slots = taps): (i, j) is the output pixel, the tap's padded coordinate is outside, (oi, oj) the reflected source.
//   data gradient (81 slots = tap x row candidate x column candidate): (i, j) is the input pixel q; the padded coordinate (a, b) with
//   (r(a), r(b)) = q is a = i | -1 (i == 1) | H (i == H-2), likewise b; it must be outside and the output pixel
//   (oi, oj) = (a - kh + 1, b - kw + 1) inside.  Distinct slots are distinct (output pixel, tap) pairs: each is counted once.
template <bool DGRAD>
__device__ __forceinline__ bool ring_slot(int s, int i, int j, int H, int W, int& oi, int& oj, int& tap) {
  if (!DGRAD) {
    tap = s;
    const int a = i + s / 3 - 1, b = j + s % 3 - 1;
    oi = reflect_idx(a, H);
    oj = reflect_idx(b, W);
    return a < 0 || a >= H || b < 0 || b >= W;
  }
  tap = s / 9;
  const int ca = (s % 9) / 3, cb = s % 3, kh = tap / 3, kw = tap % 3;
  if (ca == 0 && cb == 0) return false;
  if ((ca == 1 && i != 1) || (ca == 2 && i != H - 2) || (cb == 1 && j != 1) || (cb == 2 && j != W - 2)) return false;
  const int a = ca == 0 ? i : (ca == 1 ? -1 : H), b = cb == 0 ? j : (cb == 1 ? -1 : W);
  oi = a - kh + 1;
  oj = b - kw + 1;
  return oi >= 0 && oi < H && oj >= 0 && oj < W;
}

// acc[i][j] += As[k][wm + 16 i + .] Bs[k][wn + 16 j + .] over the 16 k of the staged slab.  v_mfma_f32_16x16x4_f32: lane l holds
// A[l & 15][k = l >> 4], B[k = l >> 4][l & 15]; result register r is C[4 (l >> 4) + r][l & 15].
__device__ __forceinline__ void tile_mma(const float (*As)[LDT], const float (*Bs)[LDT], f32x4 (&acc)[2][2], int wm, int wn, int lane) {
#pragma unroll
  for (int kk = 0; kk < TK / 4; ++kk) {
    const int k = kk * 4 + (lane >> 4), c = lane & 15;
    const float a0 = As[k][wm + c], a1 = As[k][wm + 16 + c], b0 = Bs[k][wn + c], b1 = Bs[k][wn + 16 + c];
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
  }
}

// out[pixel of row m][n0 + .] += sum over (slot, k) src[other pixel of (m, slot)][k] * w[.][.][tap of slot]
//   forward:       rows = border pixels, src = x (csA = stored Cin, K = Ci), columns = co, w[co][k][tap]
//   data gradient: rows = inner-ring pixels, src = dy (csA = stored Cout, K = Co), columns = ci, w[k][ci][tap]
constexpr int SG = 3;                      // slots per step: the 3 outside taps of an edge
constexpr int WCHUNK = TN * TK * 9;        // staged weights per K slab: 64 columns x 16 k x 9 taps
constexpr int WLOADS = WCHUNK / 256;       // ... floats per thread

template <bool DGRAD>
__global__ __launch_bounds__(256) void ring_gemm_kernel(const float* __restrict__ src, const float* __restrict__ w, float* out, int N,
                                                        int H, int W, int rows_per_img, int csA, int csOut, int Co, int Ci) {
  constexpr int NS = DGRAD ? 81 : 9;
  constexpr int WRUN = DGRAD ? TN * 9 : TK * 9;      // one contiguous run of OIHW floats (stored with one float of padding)
  __shared__ int other[NS][TM];
  __shared__ int outpix[TM];
  __shared__ int active[NS];
  __shared__ int act[NS];
  __shared__ int nact_s;
  __shared__ __attribute__((aligned(16))) float As[SG][TK][LDT];
  __shared__ float Wc[WCHUNK + 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN, M = N * rows_per_img;
  const int K = DGRAD ? Co : Ci, NOUT = DGRAD ? Ci : Co;
  const InnerRing ring = inner_ring(H, W);
  for (int s = tid; s < NS; s += 256) active[s] = 0;
  __syncthreads();
  for (int e = tid; e < NS * TM; e += 256) {
    const int row = e & (TM - 1), s = e >> 6, m = m0 + row;
    int val = -1, pix = -1;
    if (m < M) {
      const int n = m / rows_per_img, idx = m - n * rows_per_img;
      int i, j, oi, oj, tap;
      if (DGRAD) inner_pixel(idx, ring, H, W, i, j);
      else border_pixel(idx, H, W, i, j);
      pix = (n * H + i) * W + j;
      if (ring_slot<DGRAD>(s, i, j, H, W, oi, oj, tap)) {
        val = (n * H + oi) * W + oj;
        active[s] = 1;      // (every writer stores the same value)
      }
    }
    other[s][row] = val;
    if (s == 0) outpix[row] = pix;
  }
  __syncthreads();
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int arow = tid >> 2, akq = (tid & 3) * 4;
  if (tid == 0) {      // the slots this tile uses, in slot order
    int n = 0;
    for (int s = 0; s < NS; ++s)
      if (active[s]) act[n++] = s;
    nact_s = n;
  }
  __syncthreads();
  const int nact = nact_s, ng = (nact + SG - 1) / SG, nk = (K + TK - 1) / TK, total = nk * ng;
  // One step = (K slab, group of up to SG slots).  Per K slab the weights of ALL 9 taps of the tile's 64 columns x 16 k are staged
  // once, read from OIHW in whole contiguous runs (forward: 144 floats per column, data gradient: 576 floats per k) -- a tap-
  // strided read would use 4 of every 36 bytes it fetches.  The global loads of the next step are issued into registers before the
  // MFMAs of this one.
  f32x4 va[SG];
  float vw[WLOADS];
  auto load_a = [&](int it) {
    const int kidx = it / ng, g = it - kidx * ng, k0 = kidx * TK;
#pragma unroll
    for (int j = 0; j < SG; ++j) {
      const int si = g * SG + j;
      va[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (si < nact) {
        const int pix = other[act[si]][arow];
        if (pix >= 0 && k0 + akq < csA) va[j] = *reinterpret_cast<const f32x4*>(src + (size_t)pix * csA + k0 + akq);
      }
    }
  };
  const bool w_vec = (Ci & 3) == 0;      // every run starts 16-byte aligned
  auto load_w = [&](int kidx) {
    const int k0 = kidx * TK;
#pragma unroll
    for (int i = 0; i < WLOADS / 4; ++i) {
      const int e = (tid + 256 * i) * 4;      // 4 consecutive floats of one run (run lengths are multiples of 4)
      const int run = e / WRUN, r = e - run * WRUN;
      // forward: run = column, w[n0 + run][k0 .. k0 + 15][9 taps]; data gradient: run = k, w[k0 + run][n0 .. n0 + 63][9 taps]
      const bool run_ok = DGRAD ? (k0 + run < Co) : (n0 + run < Co);
      const int lim = DGRAD ? (Ci - n0) * 9 : (Ci - k0) * 9;      // valid floats of the run
      const float* p = w + (DGRAD ? ((size_t)(k0 + run) * Ci + n0) * 9 : ((size_t)(n0 + run) * Ci + k0) * 9) + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (run_ok && w_vec && r + 3 < lim) {
        v = *reinterpret_cast<const f32x4*>(p);
      } else if (run_ok) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (r + q < lim) v[q] = p[q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) vw[4 * i + q] = v[q];
    }
  };
  if (total > 0) {
    load_a(0);
    load_w(0);
  }
  for (int it = 0; it < total; ++it) {
    const int kidx = it / ng, g = it - kidx * ng;
    __syncthreads();      // the previous step's MFMAs have read As (and, at g == 0, the previous slab's Wc)
    if (g == 0) {
#pragma unroll
      for (int i = 0; i < WLOADS; ++i) {
        const int e = (tid + 256 * (i / 4)) * 4 + (i & 3);
        const int run = e / WRUN, r = e - run * WRUN;
        Wc[run * (WRUN + 1) + r] = vw[i];
      }
    }
#pragma unroll
    for (int j = 0; j < SG; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) As[j][akq + e][arow] = va[j][e];
    __syncthreads();
    if (g == 0 && kidx + 1 < nk) load_w(kidx + 1);
    if (it + 1 < total) load_a(it + 1);
    for (int j = 0; j < SG; ++j) {
      const int si = g * SG + j;
      if (si >= nact) break;      // block-uniform
      const int tap = DGRAD ? act[si] / 9 : act[si];
#pragma unroll
      for (int kk = 0; kk < TK / 4; ++kk) {
        const int k = kk * 4 + (lane >> 4), c = lane & 15;
        const float a0 = As[j][k][wm + c], a1 = As[j][k][wm + 16 + c];
        // forward: Wc[column][k * 9 + tap], rows of 144 + 1; data gradient: Wc[k][column * 9 + tap], rows of 576 + 1
        const float b0 = DGRAD ? Wc[k * (WRUN + 1) + (wn + c) * 9 + tap] : Wc[(wn + c) * (WRUN + 1) + k * 9 + tap];
        const float b1 = DGRAD ? Wc[k * (WRUN + 1) + (wn + 16 + c) * 9 + tap] : Wc[(wn + 16 + c) * (WRUN + 1) + k * 9 + tap];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wm + 16 * i + 4 * (lane >> 4) + r;
      const int pix = outpix[row];
      if (pix < 0) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn + 16 * j + (lane & 15);
        if (col < NOUT) out[(size_t)pix * csOut + col] += acc[i][j][r];
      }
    }
}

// the k-th (image, pixel) pair tap (kh, kw) leaves the map at: the W pixels of row 0 / H-1 (kh != 1), then the pixels of column
// 0 / W-1 (kw != 1) that are not in that row
__host__ __device__ __forceinline__ int tap_pixels(int kh, int kw, int H, int W) {
  return (kh != 1 ? W : 0) + (kw != 1 ? H - (kh != 1 ? 1 : 0) : 0);
}

__global__ __launch_bounds__(256) void ring_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         float* __restrict__ ws, int N, int H, int W, int Ci, int csIn, int Co,
                                                         int csOut, int splits) {
  __shared__ int pdy[TK], px[TK];
  __shared__ __attribute__((aligned(16))) float As[TK][LDT];
  __shared__ __attribute__((aligned(16))) float Bs[TK][LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co0 = blockIdx.x * TM, ci0 = blockIdx.y * TN;
  const int tap8 = blockIdx.z / splits, split = blockIdx.z - tap8 * splits;
  const int tap = tap8 < 4 ? tap8 : tap8 + 1, kh = tap / 3, kw = tap % 3;
  const int cnt = tap_pixels(kh, kw, H, W), ktot = N * cnt;
  const int chunks = (ktot + TK - 1) / TK, cps = (chunks + splits - 1) / splits;
  const int kbeg = split * cps * TK, kend = min(ktot, kbeg + cps * TK);
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int lk = tid >> 4, lq = (tid & 15) * 4;
  for (int k0 = kbeg; k0 < kend; k0 += TK) {
    __syncthreads();      // the previous slab (and its pixel table) has been consumed
    if (tid < TK) {
      const int k = k0 + tid;
      int a = -1, b = -1;
      if (k < kend) {
        const int n = k / cnt;
        int r = k - n * cnt, i, j;
        if (kh != 1 && r < W) {
          i = kh == 0 ? 0 : H - 1, j = r;
        } else {
          if (kh != 1) r -= W;
          j = kw == 0 ? 0 : W - 1;
          i = r + (kh == 0 ? 1 : 0);
        }
        a = (n * H + i) * W + j;
        b = (n * H + reflect_idx(i + kh - 1, H)) * W + reflect_idx(j + kw - 1, W);
      }
      pdy[tid] = a;
      px[tid] = b;
    }
    __syncthreads();
    f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
    if (pdy[lk] >= 0) {
      if (co0 + lq < csOut) va = *reinterpret_cast<const f32x4*>(dy + (size_t)pdy[lk] * csOut + co0 + lq);
      if (ci0 + lq < csIn) vb = *reinterpret_cast<const f32x4*>(x + (size_t)px[lk] * csIn + ci0 + lq);
    }
    *reinterpret_cast<f32x4*>(&As[lk][lq]) = va;
    *reinterpret_cast<f32x4*>(&Bs[lk][lq]) = vb;
    __syncthreads();
    tile_mma(As, Bs, acc, wm, wn, lane);
  }
  // partial tile of this split: ws[split][tap8][co][ci] (written whole, zeros included: the fold reads every split)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + wm + 16 * i + 4 * (lane >> 4) + r;
      if (co >= Co) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ci = ci0 + wn + 16 * j + (lane & 15);
        if (ci < Ci) ws[(((size_t)split * 8 + tap8) * Co + co) * Ci + ci] = acc[i][j][r];
      }
    }
}

// dw[co][ci][tap] += ws[0][tap8][co][ci] + ws[1][tap8][co][ci] + ... in split order
__global__ __launch_bounds__(256) void ring_wgrad_fold_kernel(const float* __restrict__ ws, float* __restrict__ dw, int Co, int Ci,
                                                              int splits) {
  const long total = (long)Co * Ci * 8;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int tap8 = (int)(e & 7);
    const long cc = e >> 3;      // co * Ci + ci
    float sum = 0.f;
    for (int s = 0; s < splits; ++s) sum += ws[((size_t)s * 8 + tap8) * Co * Ci + cc];
    dw[cc * 9 + (tap8 < 4 ? tap8 : tap8 + 1)] += sum;
  }
}

// the number of K splits of the weight gradient: a function of the shape alone
int wgrad_splits(int N, int H, int W, int Ci, int Co) {
  const long tiles = (long)dsee_cdiv(Co, TM) * dsee_cdiv(Ci, TN) * 8;
  const long kmax = (long)N * (W + H - 1);
  long s = 1024 / tiles;
  const long by_k = (kmax + 63) / 64;
  if (s > by_k) s = by_k;
  if (s > 32) s = 32;
  return s < 1 ? 1 : (int)s;
}

int ring_args_ok(const char* who, const void* a, const void* b, const void* c, int N, int H, int W, int Cin, int Cin_stored, int Cout,
                 int Cout_stored) {
  if (!a || !b || !c) {
    dsee_set_error("%s: NULL pointer argument", who);
    return DSEE_EINVAL;
  }
  if (N < 1 || H < 2 || W < 2) {
    dsee_set_error("%s: N = %d, H = %d, W = %d (reflection padding of 1 needs H >= 2 and W >= 2)", who, N, H, W);
    return DSEE_EINVAL;
  }
  if (Cin < 1 || Cout < 1 || Cin_stored != (Cin + 3) / 4 * 4 || Cout_stored != (Cout + 3) / 4 * 4) {
    dsee_set_error("%s: channel storage mismatch: Cin = %d stored as %d, Cout = %d stored as %d (stored = the count padded to a "
                   "multiple of 4)", who, Cin, Cin_stored, Cout, Cout_stored);
    return DSEE_EINVAL;
  }
  const long px = (long)N * H * W;
  if (px >= (1L << 31) || (long)Cin * Cout * 9 >= (1L << 31)) {
    dsee_set_error("%s: N H W = %ld pixels / %ld weights exceed the 32-bit pixel index", who, px, (long)Cin * Cout * 9);
    return DSEE_EINVAL;
  }
  return DSEE_OK;
}

// ---- y = act((x - mean[g][c]) * invstd[g][c] + res)
__global__ __launch_bounds__(256) void norm_act_res_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                               const float* __restrict__ invstd, const float* __restrict__ res,
                                                               float* __restrict__ y, long total4, int C, long group_elems, int act,
                                                               float slope, float* __restrict__ amax) {
  float vmax = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
    const long e = i * 4;
    const unsigned px = (unsigned)i / ((unsigned)C >> 2);       // (32-bit divisions: dsee_common.h)
    const int c = (int)((unsigned)i - px * ((unsigned)C >> 2)) * 4;
    const int grp = (int)(px / (unsigned)(group_elems / C));
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + e);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + (size_t)grp * C + c);
    const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + (size_t)grp * C + c);
    f32x4 r = (v - mu) * is + *reinterpret_cast<const f32x4*>(res + e);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = dsee_act(r[k], act, slope);
    *reinterpret_cast<f32x4*>(y + e) = r;
    vmax = fmaxf(vmax, dsee_absmax4(r));
  }
  if (amax) dsee_block_atomic_absmax(amax, vmax);   // (block-uniform)
}

}  // namespace

extern "C" {

int dsee_reflect_ring_fwd(const float* x, const float* w_oihw, float* y, int N, int H, int W, int Cin, int Cin_stored, int Cout,
                          int Cout_stored, hipStream_t st) {
  const int rc = ring_args_ok("dsee_reflect_ring_fwd", x, w_oihw, y, N, H, W, Cin, Cin_stored, Cout, Cout_stored);
  if (rc != DSEE_OK) return rc;
  const int rows = border_count(H, W);
  ring_gemm_kernel<false><<<dim3(dsee_cdiv((long)N * rows, TM), dsee_cdiv(Cout, TN)), 256, 0, st>>>(
      x, w_oihw, y, N, H, W, rows, Cin_stored, Cout_stored, Cout, Cin);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_reflect_ring_dgrad(const float* dy, const float* w_oihw, float* dx, int N, int H, int W, int Cin, int Cin_stored, int Cout,
                            int Cout_stored, hipStream_t st) {
  const int rc = ring_args_ok("dsee_reflect_ring_dgrad", dy, w_oihw, dx, N, H, W, Cin, Cin_stored, Cout, Cout_stored);
  if (rc != DSEE_OK) return rc;
  const int rows = inner_ring(H, W).count;
  ring_gemm_kernel<true><<<dim3(dsee_cdiv((long)N * rows, TM), dsee_cdiv(Cin, TN)), 256, 0, st>>>(
      dy, w_oihw, dx, N, H, W, rows, Cout_stored, Cin_stored, Cout, Cin);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

size_t dsee_reflect_ring_wgrad_workspace(int N, int H, int W, int Cin, int Cout) {
  if (N < 1 || H < 2 || W < 2 || Cin < 1 || Cout < 1) return 0;
  return (size_t)wgrad_splits(N, H, W, Cin, Cout) * 8 * Cout * Cin * sizeof(float);
}

int dsee_reflect_ring_wgrad(const float* x, const float* dy, float* workspace, size_t workspace_bytes, float* dw_oihw, int N, int H,
                            int W, int Cin, int Cin_stored, int Cout, int Cout_stored, hipStream_t st) {
  const int rc = ring_args_ok("dsee_reflect_ring_wgrad", x, dy, dw_oihw, N, H, W, Cin, Cin_stored, Cout, Cout_stored);
  if (rc != DSEE_OK) return rc;
  const size_t need = dsee_reflect_ring_wgrad_workspace(N, H, W, Cin, Cout);
  if (!workspace || workspace_bytes < need) {
    dsee_set_error("dsee_reflect_ring_wgrad: workspace of %zu bytes at %p, %zu needed (dsee_reflect_ring_wgrad_workspace)",
                   workspace_bytes, (const void*)workspace, need);
    return DSEE_EINVAL;
  }
  const int splits = wgrad_splits(N, H, W, Cin, Cout);
  ring_wgrad_kernel<<<dim3(dsee_cdiv(Cout, TM), dsee_cdiv(Cin, TN), 8 * splits), 256, 0, st>>>(x, dy, workspace, N, H, W, Cin,
                                                                                                 Cin_stored, Cout, Cout_stored, splits);
  DSEE_LAUNCH_CHECK();
  const long total = (long)Cout * Cin * 8;
  ring_wgrad_fold_kernel<<<(int)min(4096L, (total + 255) / 256), 256, 0, st>>>(workspace, dw_oihw, Cout, Cin, splits);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_norm_act_res_fwd(const float* x, const float* mean, const float* invstd, const float* res, float* y, int N, int HW, int C,
                          int groups, int act, float slope, float* amax_y, hipStream_t st) {
  DSEE_CHECK_ARG(x && mean && invstd && res && y);
  DSEE_CHECK_ARG(N >= 1 && HW >= 1 && C >= 4 && C % 4 == 0 && groups >= 1 && N % groups == 0 && (long)N * HW * C / 4 < (1L << 32));
  const long total4 = (long)N * HW * C / 4;
  norm_act_res_fwd_kernel<<<(int)min(8192L, (total4 + 255) / 256), 256, 0, st>>>(x, mean, invstd, res, y, total4, C,
                                                                                (long)(N / groups) * HW * C, act, slope, amax_y);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

}  // extern "C"
