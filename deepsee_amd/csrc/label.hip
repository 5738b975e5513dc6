// Label-map indexed kernels: everything the reference does with the 19-channel one-hot `input_semantics`
// tensor (data/preprocessor.py:35-41) is restated on a uint8 label map [N][H][W] (76x fewer bytes).
//
//  * onehot_conv3x3: mlp_shared = ReLU(conv3x3(one-hot seg)) (normalization.py:98-101,110-114,174-175) is a
//    9-tap gather-sum of weight columns; its weight gradient is a label-segmented sum.
//  * label_gather:   style_map[b,:,h,w] = style[b, label[b,h,w], :]   (normalization.py:179-185), also the
//    backward of style pooling.
//  * label_segsum:   S[b,r,c] = scale * sum_{hw: label=r} f[b,h,w,c]   (encoder.py:36-49 extract_style_matrix,
//    divides by H*W not by region area), also the backward of label_gather.
//  * nearest resize of the label map is index math: src = dst << shift  (F.interpolate 'nearest', SURVEY B-3).
//
// Labels outside [0, L): a pixel whose byte is >= L (the loader's "unknown" 255 -> label_nc without a dontcare class, or any
// stray value) is an ALL-ZERO one-hot vector in every kernel here -- it adds no table row to a gather-sum, gathers a zero
// style row, and is skipped by the segmented sums -- as in build_d_input and the compare-select weight gradient.  (The
// reference raises in scatter_ instead.)  No address is ever formed from such a byte: every table index below sits behind
// `(unsigned)r < (unsigned)L`.  The 32 one-hot columns (dsee_label_onehot, onehot_coff) flag the raw byte when it is < 32;
// their consumers multiply columns >= L by zero table columns.
#include "dsee_common.h"
#include "dsee_rng.h"

namespace {

__device__ __forceinline__ int lab_at(const uint8_t* lab, int n, int H, int W, int shift, int h, int w) {
  return lab[((size_t)n * H + ((size_t)h << shift)) * W + ((size_t)w << shift)];
}

// wt: [9][L][Co] (tap-major table), out[m][out_ld] at channel offset coff, Co % 4 == 0
__global__ __launch_bounds__(256) void onehot_conv_fwd_kernel(const uint8_t* __restrict__ lab,
                                                              const float* __restrict__ wt,
                                                              const float* __restrict__ bias, float* __restrict__ out,
                                                              int N, int H, int W, int shift, int R, int Rw, int L,
                                                              int Co, int out_ld, int coff, int relu, int onehot_coff,
                                                              float* __restrict__ amax, float amax_floor) {
  const int tpp = Co / 4, ppb = 256 / tpp;
  const int q = threadIdx.x % tpp, s = threadIdx.x / tpp;
  const long M = (long)N * R * Rw;
  float vmax = amax_floor;   // max |out| for the fp16 operand scale of the consumer (the one-hot channels contribute 1)
  if (s < ppb) {
    const f32x4 b = bias ? *reinterpret_cast<const f32x4*>(bias + q * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    for (long m = (long)blockIdx.x * ppb + s; m < M; m += (long)gridDim.x * ppb) {
      // (32-bit divisions: M < 2^32 -- the host checks --, and the ISA has no integer divide: dsee_common.h)
      const unsigned mu_ = (unsigned)m, t_ = mu_ / (unsigned)Rw, n_ = t_ / (unsigned)R;
      const int w = (int)(mu_ - t_ * (unsigned)Rw), h = (int)(t_ - n_ * (unsigned)R), n = (int)n_;
      f32x4 acc = b;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int hh = h + dy, ww = w + dx;
          if (hh >= 0 && hh < R && ww >= 0 && ww < Rw) {
            const int r = lab_at(lab, n, H, W, shift, hh, ww);
            const int tap = (dy + 1) * 3 + (dx + 1);
            if (r < L) acc += *reinterpret_cast<const f32x4*>(wt + ((size_t)tap * L + r) * Co + q * 4);
          }
        }
      if (relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaxf(acc[k], 0.f);
      }
      *reinterpret_cast<f32x4*>(out + m * out_ld + coff + q * 4) = acc;
      vmax = fmaxf(vmax, dsee_absmax4(acc));
      if (onehot_coff >= 0 && q < 8) {   // the 32 one-hot label channels of the same pixel (dsee_label_onehot)
        const int r = lab_at(lab, n, H, W, shift, h, w);
        f32x4 oh;
#pragma unroll
        for (int k = 0; k < 4; ++k) oh[k] = (q * 4 + k == r) ? 1.f : 0.f;
        *reinterpret_cast<f32x4*>(out + m * out_ld + onehot_coff + q * 4) = oh;
      }
    }
  }
  if (amax) dsee_block_atomic_absmax(amax, vmax);   // (amax is block-uniform; every thread arrives here)
}

// Same function with the whole tap table [9][L][Co] resident in LDS (<= 150 KB: L = 19..32 classes x 128 channels): the
// global form is a chain of two dependent loads per tap (label byte -> table row in L2) and ran at 1.1 TB/s of output;
// here one 1024-thread block per CU copies the table once, walks the pixels with stride gridDim.x and fetches the NEXT
// pixel's nine labels while it sums the current pixel's rows out of LDS.
__global__ __launch_bounds__(1024) void onehot_conv_fwd_lds_kernel(const uint8_t* __restrict__ lab,
                                                                   const float* __restrict__ wt,
                                                                   const float* __restrict__ bias, float* __restrict__ out,
                                                                   int N, int H, int W, int shift, int R, int Rw, int L,
                                                                   int Co, int out_ld, int coff, int relu, int onehot_coff,
                                                                   float* __restrict__ amax, float amax_floor) {
  extern __shared__ __attribute__((aligned(16))) float tab[];
  for (int i = threadIdx.x; i < 9 * L * Co / 4; i += 1024)
    reinterpret_cast<f32x4*>(tab)[i] = reinterpret_cast<const f32x4*>(wt)[i];
  __syncthreads();
  const int tpp = Co / 4, ppb = 1024 / tpp;
  const int q = threadIdx.x % tpp, s = threadIdx.x / tpp;
  const long M = (long)N * R * Rw, stride = (long)gridDim.x * ppb;
  float vmax = amax_floor;
  auto labels = [&](long m, int (&r)[9]) {
    // (32-bit divisions: M < 2^32 -- the host checks --, and the ISA has no integer divide: dsee_common.h)
    const unsigned mu_ = (unsigned)m, t_ = mu_ / (unsigned)Rw, n_ = t_ / (unsigned)R;
    const int w = (int)(mu_ - t_ * (unsigned)Rw), h = (int)(t_ - n_ * (unsigned)R), n = (int)n_;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
      const bool in = hh >= 0 && hh < R && ww >= 0 && ww < Rw;
      r[tap] = in ? lab_at(lab, n, H, W, shift, hh, ww) : -1;
    }
  };
  if (s < ppb) {
    const f32x4 b = bias ? *reinterpret_cast<const f32x4*>(bias + q * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    long m = (long)blockIdx.x * ppb + s;
    int cur[9], nxt[9];
    if (m < M) labels(m, cur);
    for (; m < M; m += stride) {
      const bool more = m + stride < M;
      if (more) labels(m + stride, nxt);
      f32x4 acc = b;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        if ((unsigned)cur[tap] < (unsigned)L)    // (-1 outside the image, >= L: no row)
          acc += *reinterpret_cast<const f32x4*>(tab + ((size_t)tap * L + cur[tap]) * Co + q * 4);
      if (relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaxf(acc[k], 0.f);
      }
      __builtin_nontemporal_store(acc, reinterpret_cast<f32x4*>(out + m * out_ld + coff + q * 4));
      vmax = fmaxf(vmax, dsee_absmax4(acc));
      if (onehot_coff >= 0 && q < 8) {   // the 32 one-hot label channels of the same pixel (dsee_label_onehot)
        f32x4 oh;
#pragma unroll
        for (int k = 0; k < 4; ++k) oh[k] = (q * 4 + k == cur[4]) ? 1.f : 0.f;
        *reinterpret_cast<f32x4*>(out + m * out_ld + onehot_coff + q * 4) = oh;
      }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) cur[tap] = nxt[tap];
    }
  }
  if (amax) dsee_block_atomic_absmax(amax, vmax);
}

// ... and with 4 consecutive pixels of a row per thread (Rw % 4 == 0): the 32 threads of a pixel all formed the same 9 label
// addresses and bounds checks, ~300 instructions per 16-byte store (1.8 TB/s of output at 256^2, issue-bound); a run of 4 pixels
// shares its 3 x 6 label window (18 loads for 4 pixels instead of 36) and one index decomposition.
__global__ __launch_bounds__(1024) void onehot_conv_fwd_lds4_kernel(const uint8_t* __restrict__ lab,
                                                                    const float* __restrict__ wt,
                                                                    const float* __restrict__ bias, float* __restrict__ out,
                                                                    int N, int H, int W, int shift, int R, int Rw, int L,
                                                                    int Co, int out_ld, int coff, int relu, int onehot_coff,
                                                                    float* __restrict__ amax, float amax_floor) {
  extern __shared__ __attribute__((aligned(16))) float tab[];
  for (int i = threadIdx.x; i < 9 * L * Co / 4; i += 1024)
    reinterpret_cast<f32x4*>(tab)[i] = reinterpret_cast<const f32x4*>(wt)[i];
  __syncthreads();
  const int tpp = Co / 4, gpb = 1024 / tpp;          // pixel runs per block and step
  const int q = threadIdx.x % tpp, s = threadIdx.x / tpp;
  const unsigned Rw4 = (unsigned)Rw >> 2;
  const long G = (long)N * R * Rw4, stride = (long)gridDim.x * gpb;
  float vmax = amax_floor;
  if (s < gpb) {
    const f32x4 b = bias ? *reinterpret_cast<const f32x4*>(bias + q * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* const tq = tab + q * 4;
    for (long g = (long)blockIdx.x * gpb + s; g < G; g += stride) {
      const unsigned gu = (unsigned)g, t_ = gu / Rw4, n_ = t_ / (unsigned)R;
      const int w0 = (int)(gu - t_ * Rw4) * 4, h = (int)(t_ - n_ * (unsigned)R), n = (int)n_;
      int win[3][6];      // labels of rows h-1 .. h+1, columns w0-1 .. w0+4 (-1 outside the image)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int hh = h + a - 1;
        const bool rin = hh >= 0 && hh < R;
        const uint8_t* const row = lab + ((size_t)n * H + ((size_t)(rin ? hh : 0) << shift)) * W;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const int ww = w0 + c - 1;
          win[a][c] = (rin && ww >= 0 && ww < Rw) ? (int)row[(size_t)ww << shift] : -1;
        }
      }
      const size_t m0 = ((size_t)n * R + h) * Rw + w0;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        f32x4 acc = b;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int r = win[tap / 3][p + tap % 3];
          if ((unsigned)r < (unsigned)L) acc += *reinterpret_cast<const f32x4*>(tq + (tap * L + r) * Co);
        }
        if (relu) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = fmaxf(acc[k], 0.f);
        }
        __builtin_nontemporal_store(acc, reinterpret_cast<f32x4*>(out + (m0 + p) * out_ld + coff + q * 4));
        vmax = fmaxf(vmax, dsee_absmax4(acc));
        if (onehot_coff >= 0 && q < 8) {   // the 32 one-hot label channels of the same pixel (dsee_label_onehot)
          f32x4 oh;
#pragma unroll
          for (int k = 0; k < 4; ++k) oh[k] = (q * 4 + k == win[1][p + 1]) ? 1.f : 0.f;
          *reinterpret_cast<f32x4*>(out + (m0 + p) * out_ld + onehot_coff + q * 4) = oh;
        }
      }
    }
  }
  if (amax) dsee_block_atomic_absmax(amax, vmax);
}

__global__ void onehot_pack_kernel(const float* __restrict__ w, float* __restrict__ wt, int Co, int L) {
  // w [Co][L][3][3] -> wt [9][L][Co]
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 9 * L * Co) return;
  const int co = i % Co, r = (i / Co) % L, tap = i / (Co * L);
  wt[i] = w[((size_t)co * L + r) * 9 + tap];
}

// Weight gradient of the one-hot conv.  Block = 128 channels x 8 tap groups (group g owns tap g, group 7 taps 7 and 8, group 0
// also the bias).  A thread keeps the LT label accumulators of its tap(s) and channel in REGISTERS and updates them with a
// compare-select chain (acc[k] += label == k ? g : 0): the LDS form -- one float atomic per pixel, tap and channel -- was
// bound by the LDS atomic unit at 0.45 ms for 0.5 M pixels whatever the number of waves or the load pipelining.  Fixed
// summation order per thread, partial rows [9*L + 1][128] per block as before.
template <int LT>
__global__ __launch_bounds__(1024) void onehot_conv_wgrad_kernel(const uint8_t* __restrict__ lab,
                                                                const float* __restrict__ dact, int dld,
                                                                const float* __restrict__ act, int ald, int N,
                                                                int H, int W, int shift, int R, int Rw, int L,
                                                                int chunk_px, float* __restrict__ part) {
  const int c = threadIdx.x & 127, tg = threadIdx.x >> 7;
  const int rows = 9 * L + 1;
  const long M = (long)N * R * Rw;
  const long m0 = (long)blockIdx.x * chunk_px, m1 = min(M, m0 + chunk_px);
  const int t0 = tg;
  const bool two = tg == 7;        // (wave-uniform: a wave = 64 channels of one tap group)
  float acc0[LT], acc1[LT], accb = 0.f;
#pragma unroll
  for (int k = 0; k < LT; ++k) acc0[k] = acc1[k] = 0.f;
  constexpr int U = 8;   // pixels per trip: their loads are issued together
  for (long mb = m0; mb < m1; mb += U) {
    float gv[U];
    int r0[U], r1[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const long m = mb + j;
      gv[j] = m < m1 ? (act[(size_t)m * ald + c] > 0.f ? dact[(size_t)m * dld + c] : 0.f) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const long m = mb + j;
      // (32-bit divisions: M < 2^32 -- the host checks --, and the ISA has no integer divide: dsee_common.h)
      const unsigned mu_ = (unsigned)m, t_ = mu_ / (unsigned)Rw, n_ = t_ / (unsigned)R;
      const int w = (int)(mu_ - t_ * (unsigned)Rw), h = (int)(t_ - n_ * (unsigned)R), n = (int)n_;
      {
        const int hh = h + t0 / 3 - 1, ww = w + t0 % 3 - 1;
        r0[j] = (m < m1 && hh >= 0 && hh < R && ww >= 0 && ww < Rw) ? lab_at(lab, n, H, W, shift, hh, ww) : -1;
      }
      r1[j] = -1;
      if (two) {
        const int hh = h + 1, ww = w + 1;   // tap 8
        r1[j] = (m < m1 && hh < R && ww < Rw) ? lab_at(lab, n, H, W, shift, hh, ww) : -1;
      }
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const float g = gv[j];
      accb += g;
#pragma unroll
      for (int k = 0; k < LT; ++k) acc0[k] += r0[j] == k ? g : 0.f;
      if (two) {
#pragma unroll
        for (int k = 0; k < LT; ++k) acc1[k] += r1[j] == k ? g : 0.f;
      }
    }
  }
  float* o = part + (size_t)blockIdx.x * rows * 128;
#pragma unroll
  for (int k = 0; k < LT; ++k)
    if (k < L) {
      o[(t0 * L + k) * 128 + c] = acc0[k];
      if (two) o[(8 * L + k) * 128 + c] = acc1[k];
    }
  if (tg == 0) o[(9 * L) * 128 + c] = accb;
}

__global__ void onehot_wgrad_finalize_kernel(const float* __restrict__ part, int nparts, int L, float* __restrict__ dw,
                                             float* __restrict__ db) {
  // dw [128][L][3][3], db [128]
  const int rows = 9 * L + 1;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * 128) return;
  const int c = i % 128, row = i / 128;
  float v = 0.f;
  for (int p = 0; p < nparts; ++p) v += part[(size_t)p * rows * 128 + i];
  if (row == 9 * L) {
    db[c] = v;
  } else {
    const int tap = row / L, r = row % L;
    dw[((size_t)c * L + r) * 9 + tap] = v;
  }
}

// out[m][coff + r] = (lab(m) == r), r in [0,32)
__global__ __launch_bounds__(256) void label_onehot_kernel(const uint8_t* __restrict__ lab, float* __restrict__ out,
                                                           int N, int H, int W, int shift, int R, int Rw, int ld,
                                                           int coff) {
  const int q = threadIdx.x & 7, s = threadIdx.x >> 3;  // 8 float4 per pixel, 32 pixels per block pass
  const long M = (long)N * R * Rw;
  for (long m = (long)blockIdx.x * 32 + s; m < M; m += (long)gridDim.x * 32) {
    // (32-bit divisions: M < 2^32 -- the host checks --, and the ISA has no integer divide: dsee_common.h)
    const unsigned mu_ = (unsigned)m, t_ = mu_ / (unsigned)Rw, n_ = t_ / (unsigned)R;
    const int w = (int)(mu_ - t_ * (unsigned)Rw), h = (int)(t_ - n_ * (unsigned)R), n = (int)n_;
    const int r = lab_at(lab, n, H, W, shift, h, w);
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (q * 4 + k == r) ? 1.f : 0.f;
    *reinterpret_cast<f32x4*>(out + m * ld + coff + q * 4) = v;
  }
}

// out[m][ld] @coff = scale * table[n][lab(m)][:]   (zeros where lab(m) >= L)
__global__ __launch_bounds__(256) void label_gather_kernel(const uint8_t* __restrict__ lab,
                                                           const float* __restrict__ table, float* __restrict__ out,
                                                           int N, int H, int W, int shift, int R, int Rw, int L, int Cs,
                                                           int ld, int coff, float scale) {
  const int tpp = Cs / 4, ppb = 256 / tpp;
  const int q = threadIdx.x % tpp, s = threadIdx.x / tpp;
  if (s >= ppb) return;
  const long M = (long)N * R * Rw;
  for (long m = (long)blockIdx.x * ppb + s; m < M; m += (long)gridDim.x * ppb) {
    // (32-bit divisions: M < 2^32 -- the host checks --, and the ISA has no integer divide: dsee_common.h)
    const unsigned mu_ = (unsigned)m, t_ = mu_ / (unsigned)Rw, n_ = t_ / (unsigned)R;
    const int w = (int)(mu_ - t_ * (unsigned)Rw), h = (int)(t_ - n_ * (unsigned)R), n = (int)n_;
    const int r = lab_at(lab, n, H, W, shift, h, w);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < L) v = *reinterpret_cast<const f32x4*>(table + ((size_t)n * L + r) * Cs + q * 4) * scale;
    *reinterpret_cast<f32x4*>(out + m * ld + coff + q * 4) = v;
  }
}

// part[n][chunk][L][Cs] = sum_{pixels of chunk with label r} in[m][coff + c]   (pixels with a label >= L enter no sum)
__global__ __launch_bounds__(256) void label_segsum_kernel(const uint8_t* __restrict__ lab,
                                                           const float* __restrict__ in, int ld, int coff, int H, int W,
                                                           int shift, int R, int Rw, int L, int Cs, int chunk_px,
                                                           int chunks, float* __restrict__ part) {
  extern __shared__ float accs[];  // [slots][L][Cs]
  const int slots = 256 / Cs > 0 ? 256 / Cs : 1;
  const int c = threadIdx.x % Cs, s = threadIdx.x / Cs;
  const int n = blockIdx.y, chunk = blockIdx.x;
  for (int i = threadIdx.x; i < slots * L * Cs; i += 256) accs[i] = 0.f;
  __syncthreads();
  const int P = R * Rw;
  const int p0 = chunk * chunk_px, p1 = min(P, p0 + chunk_px);
  if (s < slots && threadIdx.x < slots * Cs) {
    for (int p = p0 + s; p < p1; p += slots) {
      const int h = p / Rw, w = p % Rw;
      const int r = lab_at(lab, n, H, W, shift, h, w);
      if (r < L) accs[(s * L + r) * Cs + c] += in[((size_t)n * P + p) * ld + coff + c];
    }
  }
  __syncthreads();
  float* o = part + ((size_t)n * chunks + chunk) * L * Cs;
  for (int i = threadIdx.x; i < L * Cs; i += 256) {
    float v = 0.f;
    for (int k = 0; k < slots; ++k) v += accs[k * L * Cs + i];
    o[i] = v;
  }
}

__global__ void segsum_finalize_kernel(const float* __restrict__ part, int chunks, int LC, int N, float scale,
                                       float* __restrict__ table) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * LC) return;
  const int n = i / LC, j = i % LC;
  float v = 0.f;
  for (int k = 0; k < chunks; ++k) v += part[((size_t)n * chunks + k) * LC + j];
  table[i] = v * scale;
}

// ---- one-hot x noise conv3x3: the first layer of FullStyleEncoder under opt.random_style_matrix (encoder.py:116-120).  Its input
// randn(N, L, H, W) * one-hot(seg) has ONE non-zero channel per pixel -- the pixel's own class, holding the scalar eps(n, y, x)
// -- so the dense L -> Co convolution is the gather-sum of onehot_conv3x3 with one extra factor per tap:
//   out[n,y,x,:] = bias + sum_tap table[tap][lab(q)][:] * eps(q),   q = (n, y + ky - 1, x + kx - 1), zero padding.
// eps comes from a tensor field[N][H][W], or (field == NULL) from the Philox stream (seed, offset): pixel p = (n*H + y)*W + x is
// component p & 3 of philox_normal4(seed, offset + (p >> 2)), i.e. what dsee_rng_fill writes for an [N,H,W,1] normal tensor.
constexpr int NZ_TH = 16, NZ_TW = 32;                    // output tile (rows x columns) of one block pass
constexpr int NZ_HW = NZ_TW + 2, NZ_HALO = (NZ_TH + 2) * NZ_HW;
constexpr int NZ_SLOTS = (NZ_HW + 3) / 4 + 1;            // Philox counters a halo row can touch, whatever its alignment

// Labels (-1: outside the image or >= L: contributes nothing) and eps of the tile at (n, y0, x0) with its one-pixel halo.
// Every Philox counter the tile touches is evaluated once, by one thread.  Ends with a barrier.
__device__ __forceinline__ void noise_tile_stage(const uint8_t* __restrict__ lab, const float* __restrict__ field, uint64_t seed,
                                                 uint64_t offset, int n, int y0, int x0, int H, int W, int L, int* lab_s,
                                                 float* eps_s) {
  for (int i = threadIdx.x; i < NZ_HALO; i += blockDim.x) {
    const int r = i / NZ_HW, c = i - r * NZ_HW;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    const size_t p = ((size_t)n * H + (in ? y : 0)) * W + (in ? x : 0);
    const int v = in ? (int)lab[p] : -1;
    lab_s[i] = v < L ? v : -1;
    if (field) eps_s[i] = in ? field[p] : 0.f;
    else if (!in) eps_s[i] = 0.f;       // (the pixels inside the image are written below, each by exactly one thread)
  }
  if (!field) {
    for (int i = threadIdx.x; i < (NZ_TH + 2) * NZ_SLOTS; i += blockDim.x) {
      const int r = i / NZ_SLOTS, k = i - r * NZ_SLOTS;
      const int y = y0 - 1 + r;
      const int xa = max(x0 - 1, 0), xb = min(x0 + NZ_TW, W - 1);
      if (y < 0 || y >= H || xa > xb) continue;
      const uint64_t pa = ((uint64_t)n * H + y) * W + xa, pb = pa + (uint64_t)(xb - xa);
      const uint64_t ctr = (pa >> 2) + (uint64_t)k;
      if (ctr > (pb >> 2)) continue;
      const f32x4 v = philox_normal4(seed, offset + ctr);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint64_t p = ctr * 4 + j;
        if (p >= pa && p <= pb) eps_s[r * NZ_HW + (xa - (x0 - 1)) + (int)(p - pa)] = v[j];
      }
    }
  }
  __syncthreads();
}

// table [9][L][Co] in LDS next to the staged tile; 256 threads, Co / 4 threads per pixel (256 % (Co / 4) == 0), float4 stores
__global__ __launch_bounds__(256) void onehot_noise_fwd_kernel(const uint8_t* __restrict__ lab, const float* __restrict__ field,
                                                               uint64_t seed, uint64_t offset,
                                                               const uint64_t* __restrict__ epoch,
                                                               const float* __restrict__ wt, const float* __restrict__ bias,
                                                               float* __restrict__ out, int N, int H, int W, int L, int Co,
                                                               int tiles_x, int tiles_y) {
  extern __shared__ __attribute__((aligned(16))) float nz_smem[];
  float* const tab = nz_smem;                            // [9][L][Co]
  float* const eps_s = tab + 9 * L * Co;                 // [NZ_HALO]
  int* const lab_s = reinterpret_cast<int*>(eps_s + NZ_HALO);
  if (epoch) offset += *epoch;
  for (int i = threadIdx.x; i < 9 * L * Co / 4; i += 256)
    reinterpret_cast<f32x4*>(tab)[i] = reinterpret_cast<const f32x4*>(wt)[i];
  const unsigned b = blockIdx.x, tx_ = b % (unsigned)tiles_x, t_ = b / (unsigned)tiles_x;
  const int ty_ = (int)(t_ % (unsigned)tiles_y), n = (int)(t_ / (unsigned)tiles_y);
  const int y0 = ty_ * NZ_TH, x0 = (int)tx_ * NZ_TW;
  noise_tile_stage(lab, field, seed, offset, n, y0, x0, H, W, L, lab_s, eps_s);   // (its barrier covers the table too)
  const int tpp = Co / 4, ppb = 256 / tpp;
  const int q = threadIdx.x % tpp, s = threadIdx.x / tpp;
  const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + q * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* const tq = tab + q * 4;
  for (int pix = s; pix < NZ_TH * NZ_TW; pix += ppb) {
    const int ty = pix / NZ_TW, tx = pix % NZ_TW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int h = (ty + tap / 3) * NZ_HW + tx + tap % 3;
      const int r = lab_s[h];
      if (r >= 0) acc += *reinterpret_cast<const f32x4*>(tq + (tap * L + r) * Co) * eps_s[h];
    }
    acc += bv;       // (last: the bias then enters one rounding, not the nine of the tap sum)
    *reinterpret_cast<f32x4*>(out + (((size_t)n * H + y) * W + x) * Co + q * 4) = acc;
  }
}

// Weight gradient: dw[co][c][tap] = sum_p [lab(p + tap) = c] eps(p + tap) dout[p][co] over the output pixels p.  Thread = (tap,
// co); its L class accumulators are a private column of LDS, accs[c][thread], indexed by the label: one read-add-write per pixel
// and no conflict (a wave's threads hit consecutive words) -- the compare-select chain over registers of onehot_conv_wgrad_kernel
// costs 3 L instructions per pixel.  A block walks the tiles b, b + gridDim.x, ... in that
// order and writes ONE partial [9 L + 1][Co]: fixed summation order, no atomics.  The centre tap's threads also sum dout for the
// bias.
__global__ __launch_bounds__(1024) void onehot_noise_wgrad_kernel(const uint8_t* __restrict__ lab,
                                                                  const float* __restrict__ field, uint64_t seed,
                                                                  uint64_t offset, const uint64_t* __restrict__ epoch,
                                                                  const float* __restrict__ dout, int N, int H, int W, int L,
                                                                  int Co, int tiles_x, int tiles_y, int tiles,
                                                                  float* __restrict__ part) {
  __shared__ float eps_s[NZ_HALO];
  __shared__ int lab_s[NZ_HALO];
  extern __shared__ float nz_accs[];             // [L][blockDim.x]
  if (epoch) offset += *epoch;
  const int T = blockDim.x;
  const int tap = threadIdx.x / Co, co = threadIdx.x - tap * Co;
  const bool live = tap < 9;
  const int hoff = (tap / 3) * NZ_HW + tap % 3;
  float* const mine = nz_accs + threadIdx.x;
  for (int k = 0; k < L; ++k) mine[k * T] = 0.f;
  float accb = 0.f;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const unsigned tu = (unsigned)t, tx_ = tu % (unsigned)tiles_x, t_ = tu / (unsigned)tiles_x;
    const int ty_ = (int)(t_ % (unsigned)tiles_y), n = (int)(t_ / (unsigned)tiles_y);
    const int y0 = ty_ * NZ_TH, x0 = (int)tx_ * NZ_TW;
    __syncthreads();            // (the previous tile's readers are done)
    noise_tile_stage(lab, field, seed, offset, n, y0, x0, H, W, L, lab_s, eps_s);
    if (!live) continue;
    const int th = min(NZ_TH, H - y0), tw = min(NZ_TW, W - x0);
    for (int ty = 0; ty < th; ++ty) {
      const float* const drow = dout + (((size_t)n * H + y0 + ty) * W + x0) * Co + co;
      const int hrow = ty * NZ_HW + hoff;
      if (tw == NZ_TW) {
        // a full row: its 32 loads are in flight together (one at a time, the loop ran at a load latency per pixel: 370 us for
        // 8 x 256^2 x 32); the sums below keep the pixel order of the general loop
        float g[NZ_TW];
#pragma unroll
        for (int tx = 0; tx < NZ_TW; ++tx) g[tx] = drow[(size_t)tx * Co];
#pragma unroll
        for (int tx = 0; tx < NZ_TW; ++tx) {
          const int r = lab_s[hrow + tx];
          const float e = eps_s[hrow + tx];
          accb += g[tx];
          if (r >= 0) mine[r * T] += g[tx] * e;
        }
      } else {
        for (int tx = 0; tx < tw; ++tx) {
          const float g = drow[(size_t)tx * Co];
          const int r = lab_s[hrow + tx];
          const float e = eps_s[hrow + tx];
          accb += g;
          if (r >= 0) mine[r * T] += g * e;
        }
      }
    }
  }
  if (!live) return;
  float* const o = part + (size_t)blockIdx.x * (9 * L + 1) * Co;
  for (int k = 0; k < L; ++k) o[(tap * L + k) * Co + co] = mine[k * T];
  if (tap == 4) o[9 * L * Co + co] = accb;
}

// dw [Co][L][3][3] (+ db [Co]) = the partials summed in index order, four interleaved chains joined in a fixed order
__global__ void onehot_noise_wgrad_finalize_kernel(const float* __restrict__ part, int nparts, int L, int Co,
                                                   float* __restrict__ dw, float* __restrict__ db) {
  const int rows = 9 * L + 1;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * Co) return;
  const int c = i % Co, row = i / Co;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  int p = 0;
  for (; p + 4 <= nparts; p += 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += part[(size_t)(p + j) * rows * Co + i];
  }
  for (int j = 0; p < nparts; ++p, ++j) v[j] += part[(size_t)p * rows * Co + i];
  const float s = (v[0] + v[1]) + (v[2] + v[3]);
  if (row == 9 * L) {
    if (db) db[c] = s;
  } else {
    const int tap = row / L, r = row % L;
    dw[((size_t)c * L + r) * 9 + tap] = s;
  }
}

int noise_tiles(int N, int H, int W, int* tiles_x, int* tiles_y) {
  *tiles_x = (W + NZ_TW - 1) / NZ_TW;
  *tiles_y = (H + NZ_TH - 1) / NZ_TH;
  return N * *tiles_x * *tiles_y;
}

constexpr int NZ_MAX_PARTS = 512;

int seg_chunks(int N, int P, int* chunk_px) {
  int want = 1024 / (N > 0 ? N : 1);
  if (want < 1) want = 1;
  int cp = (P + want - 1) / want;
  if (cp < 256) cp = 256;
  *chunk_px = cp;
  return (P + cp - 1) / cp;
}

int wgrad_parts(long M, int* chunk_px) {
  long cp = (M + 511) / 512;
  if (cp < 256) cp = 256;
  *chunk_px = (int)cp;
  return (int)((M + cp - 1) / cp);
}

}  // namespace

extern "C" {

int dsee_onehot_conv3x3_pack(const float* w_oihw, float* table, int Co, int L, hipStream_t st) {
  DSEE_CHECK_ARG(w_oihw && table && Co > 0 && L > 0);
  onehot_pack_kernel<<<dsee_cdiv((long)9 * L * Co, 256), 256, 0, st>>>(w_oihw, table, Co, L);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_onehot_conv3x3_fwd(const uint8_t* lab, const float* table, const float* bias, float* out, int N, int H, int W,
                            int shift, int L, int Co, int out_ld, int coff, int relu, int onehot_coff, float* amax,
                            float amax_floor, hipStream_t st) {
  DSEE_CHECK_ARG(lab && table && out && Co % 4 == 0 && Co <= 1024 && out_ld % 4 == 0 && coff % 4 == 0);
  DSEE_CHECK_ARG(onehot_coff < 0 || (onehot_coff % 4 == 0 && out_ld >= onehot_coff + 32 && Co >= 32 && L <= 32));
  const int R = H >> shift, Rw = W >> shift;
  const long M = (long)N * R * Rw;
  DSEE_CHECK_ARG(M < (1L << 32));      // (32-bit pixel index in the kernels)
  const size_t lds = (size_t)9 * L * Co * sizeof(float);
  if (lds <= 150 * 1024 && 1024 % (Co / 4) == 0 && M >= 4096) {
    static size_t attr_lds = 0;   // (the block also holds 64 bytes of static LDS: ask for what is needed, not for 160 KB)
    if (lds > attr_lds) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&onehot_conv_fwd_lds_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        DSEE_CHECK_ARG(!"onehot_conv_fwd: cannot reserve the LDS table");
      }
      attr_lds = lds;
    }
    const int ppb1k = 1024 / (Co / 4);
    if (Rw % 4 == 0) {
      static size_t attr_lds4 = 0;
      if (lds > attr_lds4) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&onehot_conv_fwd_lds4_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
          (void)hipGetLastError();
          DSEE_CHECK_ARG(!"onehot_conv_fwd: cannot reserve the LDS table");
        }
        attr_lds4 = lds;
      }
      onehot_conv_fwd_lds4_kernel<<<(int)min(256L, (M / 4 + ppb1k - 1) / ppb1k), 1024, lds, st>>>(
          lab, table, bias, out, N, H, W, shift, R, Rw, L, Co, out_ld, coff, relu, onehot_coff, amax, amax_floor);
      DSEE_LAUNCH_CHECK();
      return DSEE_OK;
    }
    onehot_conv_fwd_lds_kernel<<<(int)min(256L, (M + ppb1k - 1) / ppb1k), 1024, lds, st>>>(
        lab, table, bias, out, N, H, W, shift, R, Rw, L, Co, out_ld, coff, relu, onehot_coff, amax, amax_floor);
    DSEE_LAUNCH_CHECK();
    return DSEE_OK;
  }
  const int ppb = 256 / (Co / 4);
  onehot_conv_fwd_kernel<<<(int)min(4096L, (M + ppb - 1) / ppb), 256, 0, st>>>(lab, table, bias, out, N, H, W, shift, R,
                                                                                Rw, L, Co, out_ld, coff, relu, onehot_coff, amax,
                                                                                amax_floor);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

size_t dsee_onehot_conv3x3_wgrad_workspace(int N, int H, int W, int shift, int L) {
  int cp;
  const long M = (long)N * (H >> shift) * (W >> shift);
  return (size_t)wgrad_parts(M, &cp) * (9 * L + 1) * 128 * sizeof(float);
}

/* dW_sh[:, r, tap] = sum_{p : lab(p+tap)=r} relu'(act[p]) * dact[p]  (SURVEY Appendix E); Co fixed at 128
 * (normalization.py:95 nhidden).  act/dact are [M][ld] with the 128 channels at offset coff. */
int dsee_onehot_conv3x3_wgrad(const uint8_t* lab, const float* dact, int dact_ld, const float* act, int act_ld, int N,
                              int H, int W, int shift, int L, float* dw_oihw, float* dbias, float* workspace,
                              hipStream_t st) {
  DSEE_CHECK_ARG(lab && dact && act && dw_oihw && dbias && workspace && L <= 32);
  const int R = H >> shift, Rw = W >> shift;
  const long M = (long)N * R * Rw;
  int cp;
  const int parts = wgrad_parts(M, &cp);
  if (L <= 20)
    onehot_conv_wgrad_kernel<20><<<parts, 1024, 0, st>>>(lab, dact, dact_ld, act, act_ld, N, H, W, shift, R, Rw, L, cp, workspace);
  else
    onehot_conv_wgrad_kernel<32><<<parts, 1024, 0, st>>>(lab, dact, dact_ld, act, act_ld, N, H, W, shift, R, Rw, L, cp, workspace);
  DSEE_LAUNCH_CHECK();
  onehot_wgrad_finalize_kernel<<<dsee_cdiv((long)(9 * L + 1) * 128, 256), 256, 0, st>>>(workspace, parts, L, dw_oihw,
                                                                                        dbias);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_onehot_noise_conv3x3_fwd(const uint8_t* lab, const float* field, uint64_t seed, uint64_t offset, int use_epoch,
                                  const float* table, const float* bias, float* out, int N, int H, int W, int L, int Co,
                                  hipStream_t st) {
  DSEE_CHECK_ARG(lab && table && out && N > 0 && H > 0 && W > 0 && L > 0 && L <= 32);
  DSEE_CHECK_ARG(Co > 0 && Co % 4 == 0 && 256 % (Co / 4) == 0);
  DSEE_CHECK_ARG((long)N * H * W < (1L << 31));
  const size_t lds = (size_t)9 * L * Co * sizeof(float) + (size_t)NZ_HALO * (sizeof(float) + sizeof(int));
  DSEE_CHECK_ARG(lds <= 64 * 1024);      // (the whole tap table sits in LDS: with Co / 4 dividing 256 that is Co <= 32 at 32 classes, <= 64 at 19)
  int tx, ty;
  const int tiles = noise_tiles(N, H, W, &tx, &ty);
  onehot_noise_fwd_kernel<<<tiles, 256, lds, st>>>(lab, field, seed, offset, (use_epoch && !field) ? dsee_rng_epoch() : nullptr,
                                                   table, bias, out, N, H, W, L, Co, tx, ty);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

size_t dsee_onehot_noise_conv3x3_wgrad_workspace(int N, int H, int W, int L, int Co) {
  if (N <= 0 || H <= 0 || W <= 0 || L <= 0 || Co <= 0) return 0;
  int tx, ty;
  const int tiles = noise_tiles(N, H, W, &tx, &ty);
  return (size_t)min(tiles, NZ_MAX_PARTS) * (9 * L + 1) * Co * sizeof(float);
}

int dsee_onehot_noise_conv3x3_wgrad(const uint8_t* lab, const float* field, uint64_t seed, uint64_t offset, int use_epoch,
                                    const float* dout, int N, int H, int W, int L, int Co, float* dw_oihw, float* dbias,
                                    float* workspace, hipStream_t st) {
  DSEE_CHECK_ARG(lab && dout && dw_oihw && workspace && N > 0 && H > 0 && W > 0 && L > 0 && L <= 32);
  DSEE_CHECK_ARG(Co > 0 && Co % 4 == 0 && 9 * Co <= 1024);
  DSEE_CHECK_ARG((long)N * H * W < (1L << 31));
  int tx, ty;
  const int tiles = noise_tiles(N, H, W, &tx, &ty);
  const int parts = min(tiles, NZ_MAX_PARTS);
  const int threads = max(256, (9 * Co + 63) / 64 * 64);
  const uint64_t* const ep = (use_epoch && !field) ? dsee_rng_epoch() : nullptr;
  const size_t lds = (size_t)L * threads * sizeof(float);
  DSEE_CHECK_ARG(lds + (size_t)NZ_HALO * (sizeof(float) + sizeof(int)) <= 64 * 1024);   // (L accumulators per (tap, co) in LDS)
  onehot_noise_wgrad_kernel<<<parts, threads, lds, st>>>(lab, field, seed, offset, ep, dout, N, H, W, L, Co, tx, ty, tiles,
                                                         workspace);
  DSEE_LAUNCH_CHECK();
  onehot_noise_wgrad_finalize_kernel<<<dsee_cdiv((long)(9 * L + 1) * Co, 256), 256, 0, st>>>(workspace, parts, L, Co, dw_oihw,
                                                                                             dbias);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_label_onehot(const uint8_t* lab, float* out, int N, int H, int W, int shift, int out_ld, int coff,
                      hipStream_t st) {
  DSEE_CHECK_ARG(lab && out && out_ld % 4 == 0 && coff % 4 == 0 && out_ld >= coff + 32);
  const int R = H >> shift, Rw = W >> shift;
  const long M = (long)N * R * Rw;
  label_onehot_kernel<<<(int)min(4096L, (M + 31) / 32), 256, 0, st>>>(lab, out, N, H, W, shift, R, Rw, out_ld, coff);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

int dsee_label_gather(const uint8_t* lab, const float* table, float* out, int N, int H, int W, int shift, int L, int Cs,
                      int out_ld, int coff, float scale, hipStream_t st) {
  DSEE_CHECK_ARG(lab && table && out && Cs % 4 == 0 && Cs <= 1024 && out_ld % 4 == 0 && coff % 4 == 0);
  const int R = H >> shift, Rw = W >> shift;
  const long M = (long)N * R * Rw;
  const int ppb = 256 / (Cs / 4);
  label_gather_kernel<<<(int)min(4096L, (M + ppb - 1) / ppb), 256, 0, st>>>(lab, table, out, N, H, W, shift, R, Rw, L,
                                                                             Cs, out_ld, coff, scale);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

size_t dsee_label_segsum_workspace(int N, int H, int W, int shift, int L, int Cs) {
  int cp;
  const int chunks = seg_chunks(N, (H >> shift) * (W >> shift), &cp);
  return (size_t)N * chunks * L * Cs * sizeof(float);
}

int dsee_label_segsum(const uint8_t* lab, const float* in, int ld, int coff, float* table, int N, int H, int W,
                      int shift, int L, int Cs, float scale, float* workspace, hipStream_t st) {
  DSEE_CHECK_ARG(lab && in && table && workspace && Cs <= 256 && L <= 32);
  const int R = H >> shift, Rw = W >> shift;
  int cp;
  const int chunks = seg_chunks(N, R * Rw, &cp);
  const int slots = 256 / Cs > 0 ? 256 / Cs : 1;
  const size_t lds = (size_t)slots * L * Cs * sizeof(float);
  label_segsum_kernel<<<dim3(chunks, N), 256, lds, st>>>(lab, in, ld, coff, H, W, shift, R, Rw, L, Cs, cp, chunks,
                                                         workspace);
  DSEE_LAUNCH_CHECK();
  segsum_finalize_kernel<<<dsee_cdiv((long)N * L * Cs, 256), 256, 0, st>>>(workspace, chunks, L * Cs, N, scale, table);
  DSEE_LAUNCH_CHECK();
  return DSEE_OK;
}

}  // extern "C"
