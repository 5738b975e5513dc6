// Coarse entry points of the C ABI: whole-block operations for a host without the Python orchestration.  Each one only sequences
// the fine-grained entry points of this library on the caller's stream, inside memory the caller owns, in the order and with the
// operands deepsee_amd/ops.py uses on the pre-split fp32 path -- so the results are bit-identical to the autograd path
// (tests/test_gpu_ops.py):
//   dsee_sean_norm_fwd             one SPADE / SEAN normalisation + LeakyReLU (normalization.py:107-120, :167-213 with the style half
//                                  as per-image tables; architecture.py:92,114) = ops.py::SeanNormTable.forward: norm_forward below
//   dsee_spade_resblock_fwd        SPADEResnetBlock.forward (architecture.py:75-147, fin == fout, no NoiseInjection):
//                                  out = act(x + conv_1(lrelu(norm_1(conv_0(lrelu(norm_0(x))))))) -- two dsee_sean_norm_fwd and two
//                                  Winograd convolutions on pre-split operands (ops.py::Conv2d: wino_conv3x3_product below)
//   dsee_spade_resblock_train_fwd  the same block as it trains: + noise_middle in conv_0's output transform, which also writes the
//                                  BatchNorm rows norm_1 finalises, + the shortcut x + noise_skip(x) in conv_1's; what the backward
//                                  pass needs stays in the caller's `saved` area
//   dsee_spade_resblock_bwd        the whole backward pass from `saved` = Conv2d.backward (ops.py::_wino_wgrad with w_for_dx) and
//                                  SeanNormTable.backward, twice
//   dsee_generator_prepare / _fwd  the whole generator in evaluation mode (sr.py:54-98 = SRModel mode "demo") from one flat parameter
//                                  buffer: what depends on the weights only once per checkpoint; then initial, the blocks through
//                                  block_forward below with the kernels ops.py picks per level, conv_img + tanh
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <vector>

#include "../../include/deepsee_hip.h"

void dsee_set_error(const char* fmt, ...);

namespace {

constexpr int kHidden = 128;          // nhidden of mlp_shared (normalization.py:95)
constexpr long kAmaxFloats = 64 * 32;   // one operand maximum in the 64-line form of dsee_absmax
// Weight gradients of at least this many FLOP take split fp16x2 operands.  Equals the default of KernelPlan.conv_f16x2_min_flop
// (ops.py::wgrad_raw): the bit-identity with ops.py holds under that default only.
constexpr double kWgradF16x2MinFlop = 1e9;

#define DSEE_TRY(call)          \
  do {                          \
    const int rc__ = (call);    \
    if (rc__ != DSEE_OK) return rc__; \
  } while (0)

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// Every workspace and the saved area are laid out by taking 256-byte aligned pieces in a fixed order; base == NULL only sizes.
struct Arena {
  char* base;
  size_t off;
  void* bytes(size_t n) {
    void* p = base ? base + off : nullptr;
    off += up256(n);
    return p;
  }
  template <typename T>
  T* take(size_t n) { return static_cast<T*>(bytes(n * sizeof(T))); }
};

int zero(float* p, size_t n, hipStream_t st, const char* who) {
  if (hipMemsetAsync(p, 0, n * sizeof(float), st) != hipSuccess) {
    dsee_set_error("%s: hipMemsetAsync failed", who);
    return DSEE_ELAUNCH;
  }
  return DSEE_OK;
}

/* ---- one SPADE / SEAN normalisation + LeakyReLU ------------------------------------------------------------------------------- */
struct NormBufs {
  float *tab, *cat, *stats;     // mlp_shared as a [tap][label][128] table; [embedding (128) | one-hot label (32)]; statistics partials
  uint16_t *v2, *u2;            // split transforms of cat and of the packed gamma|beta weights (per image with a table)
  float *amax_cat, *amax_u, *amax_xhat, *amax_h;   // operand maxima, zeroed by the caller (amax_xhat, amax_h: optional)
  float *mean, *invstd, *out_h, *out_scale;
  uint32_t* sign_mask;
  // what dsee_generator_prepare computed ahead (all unset: every step runs here).  tab_ready: `tab` holds mlp_shared's gather table;
  // u_ready: `u2` and `amax_u` hold a SPADE norm's transformed weights and their bound; u_bound_ready: `amax_u` already bounds w2a and
  // the table (written by their producers); wp_direct: the packed w2a of the direct gamma/beta kernel, which then replaces the
  // Winograd-domain product (a SEAN level whose images are not whole 128-tile GEMM tiles: ops.py::_wino_mod_chunk)
  bool tab_ready, u_ready, u_bound_ready;
  const float* wp_direct;
};
enum StatsFrom { kStatsOfX, kStatsOfParts, kStatsRunning };   // a pass over x | rows x's producer wrote (`part`) | evaluation

// The scratch part of NormBufs as dsee_sean_norm_fwd's workspace holds it; amax_cat: three lines, max |cat|, max |U|, max |xhat|.
NormBufs norm_scratch(Arena& a, int N, int H, int W, int C, int nc, int has_t) {
  const int ld = kHidden + (has_t ? 32 : 0), rows = 2 * C;
  const size_t T = (size_t)N * (H / 4) * (W / 4);
  NormBufs b = {};
  b.amax_cat = a.take<float>(3 * kAmaxFloats);
  b.tab = a.take<float>((size_t)9 * nc * kHidden);
  b.cat = a.take<float>((size_t)N * H * W * ld);
  b.stats = static_cast<float*>(a.bytes(dsee_norm_workspace(N, H * W, C, 1)));
  b.v2 = a.take<uint16_t>(36 * T * ld * 2);
  b.u2 = a.take<uint16_t>((size_t)36 * (has_t ? N : 1) * rows * ld * 2);
  return b;
}

int norm_forward(const dsee_norm_layer& nl, const uint8_t* labels, int lab_h, int lab_w, int shift, int label_nc, const float* x,
                 const NormBufs& b, StatsFrom from, const float* part, float eps, float momentum, float slope, int N, int H, int W,
                 int C, hipStream_t stream) {
  const int has_t = nl.table != nullptr, ld = kHidden + (has_t ? 32 : 0), rows = 2 * C;
  // embedding: actv = ReLU(mlp_shared(one-hot labels)) as a 9-tap gather-sum of weight columns, the 32 one-hot channels of the
  // style-table path behind it in the same launch; max |cat| rides along (>= 1 with one-hot channels present)
  if (!b.tab_ready) DSEE_TRY(dsee_onehot_conv3x3_pack(nl.w_shared, b.tab, kHidden, label_nc, stream));
  DSEE_TRY(dsee_onehot_conv3x3_fwd(labels, b.tab, nl.b_shared, b.cat, N, lab_h, lab_w, shift, label_nc, kHidden, ld, 0, 1,
                                   has_t ? kHidden : -1, b.amax_cat, has_t ? 1.0f : 0.0f, stream));
  // param-free BatchNorm statistics of x (sync_batchnorm/batchnorm.py:51-68 single-device branch; running stats updated)
  if (from == kStatsOfX)
    DSEE_TRY(dsee_norm_stats(x, N, H * W, C, 1, eps, momentum, b.mean, b.invstd, nl.running_mean, nl.running_var, b.stats, stream));
  else if (from == kStatsOfParts)
    DSEE_TRY(dsee_norm_stats_finalize_parts(part, dsee_stats_part_rows((long)N * (H / 4) * (W / 4) * (C / 4)), C, eps, momentum,
                                            b.mean, b.invstd, nl.running_mean, nl.running_var, stream));
  else
    DSEE_TRY(dsee_norm_eval_stats(nl.running_mean, nl.running_var, C, eps, b.mean, b.invstd, stream));
  if (b.wp_direct) {
    // gamma/beta as the epilogue of the direct convolution kernel (ops.py::_norm_product_direct)
    const dsee_conv_geom g = {N, H, W, ld, H, W, rows, 3, 3, 1, -1, 1, 0, 0, 1};
    return dsee_conv2d_modulate_fwd(&g, b.cat, b.wp_direct, nl.table, kHidden, nl.bias_packed, x, b.mean, b.invstd, b.out_h,
                                    b.out_scale, C, nl.add_one, slope, stream);
  }
  // operands of the gamma/beta convolution in the Winograd domain, split into two fp16 terms by their producers
  DSEE_TRY(dsee_wino43_input_f16x2(b.cat, b.v2, N, H, W, ld, b.amax_cat, DSEE_WINO_V_BOUND, stream));
  if (!b.u_ready && !b.u_bound_ready) {
    DSEE_TRY(dsee_absmax(nl.w2a, (long)rows * kHidden * 9, b.amax_u, stream));
    if (has_t) DSEE_TRY(dsee_absmax(nl.table, (long)N * 9 * rows * 32, b.amax_u, stream));
  }
  // (with a style table: the embedding columns once, the table's columns per image -- the front of the buffer sized for N copies;
  // the fused kernel takes that layout as groups = -N)
  if (has_t)
    DSEE_TRY(dsee_wino43_weights_table_shared(nl.w2a, nl.table, reinterpret_cast<float*>(b.u2), N, rows, kHidden, 2, b.amax_u,
                                              stream));
  else if (!b.u_ready)
    DSEE_TRY(dsee_wino43_weights(nl.w2a, reinterpret_cast<float*>(b.u2), rows, kHidden, 0, 2, b.amax_u, stream));
  // gamma/beta GEMM + output transform + normalise + modulate + LeakyReLU: one kernel, M never reaches HBM
  return dsee_spade_fused_fwd(b.v2, b.u2, b.amax_cat, DSEE_WINO_V_BOUND, b.amax_u, nl.bias_packed, x, b.mean, b.invstd, b.out_h,
                              b.out_scale, N, H, W, C, rows, ld, has_t ? -N : 1, nl.add_one, slope, b.amax_h, b.amax_xhat, b.sign_mask,
                              stream);
}

/* ---- one 3x3 convolution on pre-split operands, up to the Winograd-domain product m ------------------------------------------- */
int gemm_nt(const void* a2, const void* b2, float* c, long M, int Nn, int K, long rpg, int brows, const float* amax_a, float bound,
            const float* amax_b, hipStream_t st) {
  // (the same choice deepsee_amd/ops.py::_gemm_pre makes: the one-wave-per-SIMD kernel where its shape rules hold)
  if (Nn % 256 == 0 && K % 32 == 0) return dsee_gemm_f16x2_pre_w4(a2, b2, c, M, Nn, K, rpg, brows, amax_a, bound, amax_b, st);
  return dsee_gemm_f16x2_pre(a2, b2, c, M, Nn, K, rpg, brows, amax_a, bound, amax_b, st);
}

// The input transform's scale comes from the max |h| the fused norm kernel wrote: no pass over h.  max |w| accumulates into amax_w,
// which the caller zeroed.  v2 outlives the call where the weight gradient needs it.  choose_gemm: gemm_nt's choice (the training
// pair) or always dsee_gemm_f16x2_pre (the inference block).  The caller's output transform reads m.
int wino_conv3x3_product(const float* h, const float* amax_h, const float* w, float* amax_w, uint16_t* v2, uint16_t* u2, float* m,
                         bool choose_gemm, int N, int H, int W, int C, hipStream_t stream) {
  const long T = (long)N * (H / 4) * (W / 4);
  DSEE_TRY(dsee_absmax(w, (long)C * C * 9, amax_w, stream));
  DSEE_TRY(dsee_wino43_weights(w, reinterpret_cast<float*>(u2), C, C, 0, 2, amax_w, stream));
  DSEE_TRY(dsee_wino43_input_f16x2(h, v2, N, H, W, C, amax_h, DSEE_WINO_V_BOUND, stream));
  return (choose_gemm ? gemm_nt : dsee_gemm_f16x2_pre)(v2, u2, m, 36 * T, C, C, T, C, amax_h, DSEE_WINO_V_BOUND, amax_w, stream);
}

/* ---- layouts of the block entry points ------------------------------------------------------------------------------------------ */
struct InferScratch {
  size_t norm_bytes;     // dsee_sean_norm_fwd's workspace comes first, at offset 0
  float *h, *dx0, *stat, *amax_h, *amax_w, *m;   // h: lrelu(norm(.)) of the layer in flight; dx0: conv_0's output; stat: mean | invstd
  uint16_t *v2, *u2;                              // split transforms of h and of the convolution weights
};
InferScratch infer_scratch(Arena& a, int N, int H, int W, int C, int nc, int has_t) {
  const size_t px = (size_t)N * H * W, T = (size_t)N * (H / 4) * (W / 4);
  InferScratch f;
  norm_scratch(a, N, H, W, C, nc, has_t);
  f.norm_bytes = a.off;
  f.h = a.take<float>(px * C);
  f.dx0 = a.take<float>(px * C);
  f.stat = a.take<float>((size_t)2 * C);
  f.amax_h = a.take<float>(kAmaxFloats);
  f.amax_w = a.take<float>(kAmaxFloats);
  f.v2 = a.take<uint16_t>(36 * T * C * 2);
  f.u2 = a.take<uint16_t>((size_t)36 * C * C * 2);
  f.m = a.take<float>(36 * T * C);
  return f;
}

struct NormSaved {
  float *cat, *scale, *mean, *invstd, *amax;   // amax: [4][2048] = max |cat|, max |U| (w2a, table), max |xhat|, max |h|
  uint32_t* mask;
  uint16_t* v2cat;
};
struct BlockSaved {
  NormSaved n[2];
  float *dx0, *amax_w;   // conv_0's output (norm_1's input); [2][2048] = max |w_conv_0|, max |w_conv_1|
  uint16_t* v2h[2];      // split transforms of the two convolutions' inputs
};
BlockSaved saved_layout(Arena& a, int N, int H, int W, int C, int has_t) {
  const int ld = kHidden + (has_t ? 32 : 0);
  const size_t px = (size_t)N * H * W, T = (size_t)N * (H / 4) * (W / 4);
  BlockSaved s;
  for (int i = 0; i < 2; ++i) {
    s.n[i].cat = a.take<float>(px * ld);
    s.n[i].scale = a.take<float>(px * C);
    s.n[i].mask = a.take<uint32_t>(px * (C / 32));
    s.n[i].mean = a.take<float>(C);
    s.n[i].invstd = a.take<float>(C);
    s.n[i].amax = a.take<float>(4 * kAmaxFloats);
    s.n[i].v2cat = a.take<uint16_t>(36 * T * ld * 2);
    s.v2h[i] = a.take<uint16_t>(36 * T * C * 2);
  }
  s.dx0 = a.take<float>(px * C);
  s.amax_w = a.take<float>(2 * kAmaxFloats);
  return s;
}

struct FwdScratch {
  float *tab, *stats, *h, *m, *part;
  uint16_t *u2n, *u2c;
};
FwdScratch fwd_scratch(Arena& a, int N, int H, int W, int C, int nc, int has_t) {
  const int ld = kHidden + (has_t ? 32 : 0), rows = 2 * C;
  const size_t px = (size_t)N * H * W, T = (size_t)N * (H / 4) * (W / 4);
  FwdScratch f;
  f.tab = a.take<float>((size_t)9 * nc * kHidden);
  f.stats = a.take<float>(dsee_norm_workspace(N, H * W, C, 1) / sizeof(float) + 64);
  f.u2n = a.take<uint16_t>((size_t)36 * (has_t ? N : 1) * rows * ld * 2);
  f.h = a.take<float>(px * C);
  f.u2c = a.take<uint16_t>((size_t)36 * C * C * 2);
  f.m = a.take<float>(36 * T * C);
  f.part = a.take<float>((size_t)dsee_stats_part_rows((long)T * (C / 4)) * 3 * C);
  return f;
}

struct BwdScratch {
  uint16_t *dm2c, *utc, *dm2n, *ute;
  float *wsw, *dv, *dh, *dmid, *sums, *wsmod, *wst, *dve, *dactv, *wse, *amax, *dbias, *chws, *g1, *oh;
  size_t wsw_bytes, wst_bytes, wse_bytes;
};
BwdScratch bwd_scratch(Arena& a, int N, int H, int W, int C, int has_t) {
  const int ld = kHidden + (has_t ? 32 : 0), rows = 2 * C;
  const size_t px = (size_t)N * H * W, T = (size_t)N * (H / 4) * (W / 4);
  BwdScratch b;
  b.dm2c = a.take<uint16_t>(36 * T * C * 2);
  b.utc = a.take<uint16_t>((size_t)36 * dsee_conv_wrows(C) * C * 2);
  b.wsw_bytes = dsee_wino43_wgrad_workspace((long)T, C, C);
  b.wsw = a.take<float>(b.wsw_bytes / sizeof(float) + 64);
  b.dv = a.take<float>(36 * T * C);
  b.dh = a.take<float>(px * C);      // gradient w.r.t. a norm's output
  b.dmid = a.take<float>(px * C);    // gradient w.r.t. conv_0's output
  b.dm2n = a.take<uint16_t>(36 * T * rows * 2);
  b.sums = a.take<float>(4 * C);
  b.wsmod = a.take<float>(dsee_modulate_bwd_wino_workspace(N, H, W, C) / sizeof(float) + 64);
  b.wst_bytes = has_t ? dsee_wino43_wgrad_table_workspace((long)T, N, kHidden, rows) : dsee_wino43_wgrad_workspace((long)T, ld, rows);
  b.wst = a.take<float>(b.wst_bytes / sizeof(float) + 64);
  b.ute = a.take<uint16_t>((size_t)36 * dsee_conv_wrows(kHidden) * rows * 2);
  b.dve = a.take<float>(36 * T * kHidden);
  b.dactv = a.take<float>(px * kHidden);
  // mlp_shared's weight gradient: over `cat` with a table; SPADE-only norms run it on the MFMA kernel over 32 materialised
  // one-hot channels (oh) and the ReLU-masked gradient (g1)
  dsee_conv_geom g = {N, H, W, has_t ? ld : 32, H, W, kHidden, 3, 3, 1, -1, 1, 0, 0, 1};
  b.wse_bytes = dsee_conv2d_wgrad_workspace(&g);
  b.wse = a.take<float>(b.wse_bytes / sizeof(float) + 64);
  b.g1 = has_t ? nullptr : a.take<float>(px * kHidden);
  b.oh = has_t ? nullptr : a.take<float>(px * 32);
  b.amax = a.take<float>(8 * kAmaxFloats);
  b.dbias = a.take<float>(3 * C + 64);
  const size_t c1 = dsee_channel_dot_workspace((long)px, kHidden), c2 = dsee_wino43_dout_f16x2_workspace();
  b.chws = a.take<float>((c1 > c2 ? c1 : c2) / sizeof(float) + 64);
  return b;
}

/* ---- the argument check of the three block entry points, after their own NULL check ------------------------------------------- */
// Reads the scalar arguments and the two host structs only: tests/test_coarse_host.py and tests/test_label_nc_host.py pass device
// addresses that must never be dereferenced.  Order: kinds, shape rule (with the class count), label map, sizes.
enum Entry { kInference, kTrainFwd, kTrainBwd };

int block_args_ok(const char* who, Entry entry, const dsee_norm_layer* norm_0, const dsee_norm_layer* norm_1, int lab_h, int lab_w,
                  int shift, int label_nc, int N, int H, int W, int C, size_t saved_bytes, size_t workspace_bytes) {
  const int has_t = norm_0->table != nullptr;
  if (has_t != (norm_1->table != nullptr)) {
    dsee_set_error("%s: both norm layers of a block are SPADE or both SEAN", who);
    return DSEE_EINVAL;
  }
  const long T = (long)N * (H / 4) * (W / 4);
  if (entry == kInference) {
    if (C % 128 != 0 || H % 4 != 0 || W % 4 != 0 || T % 256 != 0) {
      dsee_set_error("%s: C %% 128 == 0 and N (H/4) (W/4) %% 256 == 0 required (C = %d, %ld tiles): the "
                     "pre-split Winograd GEMM takes whole 256 x 128 tiles", who, C, T);
      return DSEE_EUNSUPPORTED;
    }
  } else if (N <= 0 || H % 4 || W % 4 || ((H / 4) * (W / 4)) % 64 || T % 256 || C % 256 || (C & (C - 1)) ||
             (36 * T / 256) * (C / 256) < 512 || 256 % (C / 4) != 0) {
    dsee_set_error("%s: the pre-split training path takes C a power of two >= 256 (<= 1024), N (H/4) (W/4) %% 256 == 0, (H/4) (W/4) "
                   "%% 64 == 0 and at least 512 GEMM tiles (36 T / 256 x C / 256): N = %d, H = %d, W = %d, C = %d", who, N, H, W, C);
    return DSEE_EUNSUPPORTED;
  }
  if (label_nc < 1 || label_nc > 32) {     // (with and without table: mlp_shared's weight gradient and the 32 one-hot channels)
    dsee_set_error("%s: label_nc = %d (1..32: the one-hot label is stored in 32 channels)", who, label_nc);
    return DSEE_EUNSUPPORTED;
  }
  if (!((lab_h >> shift) == H && (lab_w >> shift) == W)) {
    dsee_set_error("%s: the label map (%d x %d >> %d) does not cover the %d x %d feature map", who, lab_h, lab_w, shift, H, W);
    return DSEE_EINVAL;
  }
  if (entry == kInference) {
    const size_t need = dsee_spade_resblock_fwd_workspace(N, H, W, C, label_nc, has_t);
    if (workspace_bytes < need) {
      dsee_set_error("%s: workspace of %zu bytes, %zu needed (dsee_spade_resblock_fwd_workspace)", who, workspace_bytes, need);
      return DSEE_EINVAL;
    }
    return DSEE_OK;
  }
  const size_t saved_need = dsee_spade_resblock_saved_bytes(N, H, W, C, label_nc, has_t);
  const size_t need = entry == kTrainFwd ? dsee_spade_resblock_train_fwd_workspace(N, H, W, C, label_nc, has_t)
                                         : dsee_spade_resblock_bwd_workspace(N, H, W, C, label_nc, has_t, lab_h, lab_w, shift);
  if (saved_bytes < saved_need || workspace_bytes < need) {
    dsee_set_error("%s: saved area of %zu bytes (%zu needed), workspace of %zu bytes (%zu needed)", who, saved_bytes, saved_need,
                   workspace_bytes, need);
    return DSEE_EINVAL;
  }
  return DSEE_OK;
}

// mlp_shared's weight gradient as a generic 3x3 weight gradient over g->Cin stored input channels (the one-hot label among them,
// cin_first on), on split fp16x2 operands from kWgradF16x2MinFlop on.  measure_in: max |in| is not known yet (amax_in zeroed).
int shared_wgrad(const dsee_conv_geom* g, const float* in, float* amax_in, bool measure_in, const float* dout, const float* amax_dout,
                 const BwdScratch& B, float* dw, int cin_first, int label_nc, hipStream_t stream) {
  const long px = (long)g->N * g->Ho * g->Wo;
  if (2.0 * (double)px * g->Cout * 9.0 * 32.0 < kWgradF16x2MinFlop)
    return dsee_conv2d_wgrad(g, in, dout, B.wse, B.wse_bytes, dw, g->Cout, cin_first, label_nc, stream);
  if (measure_in) DSEE_TRY(dsee_absmax(in, px * g->Cin, amax_in, stream));
  return dsee_conv2d_wgrad_f16x2(g, in, dout, B.wse, B.wse_bytes, dw, g->Cout, cin_first, label_nc, amax_in, amax_dout, stream);
}

/* ---- the inference block: dsee_spade_resblock_fwd as it stands, and as one block of dsee_generator_fwd ---------------------------- */
// What dsee_generator_prepare left for one norm layer / one block, and the kernel choice of the block's level.
struct NormReady {
  const float *tab, *amax_u;     // mlp_shared's gather table; max |w2a| (SPADE: the bound its u2 was scaled with)
  const uint16_t* u2;            // SPADE: Winograd-domain gamma|beta weights
  const float *wst, *wp_direct;  // SEAN: style weights of the table product; w2a packed for the direct kernel
};
struct BlockReady {
  NormReady norm[2];
  const uint16_t* u2conv[2];     // Winograd-domain weights of conv_0 / conv_1 and the maxima they were scaled with
  const float* amax_conv[2];
  const float* style;            // [N][label_nc][S]
  int S;
  float* table;                  // [N][9][2C][32]: the style table of the norm in flight
  bool norm_direct, presplit;    // SEAN norms on the direct kernel; convolutions on the pre-split GEMM (else fp32 V, split in the GEMM)
};

// Prepared weights: V pre-split from max |h| and the pre-split GEMM (gemm_nt's choice), or -- below ops.py's presplit_min_tiles, and
// behind a direct norm, which writes no max |h| -- an fp32 V with its own maximum, split inside dsee_gemm_f16x2_af32.
int wino_conv3x3_ready(const float* h, const float* amax_h, const uint16_t* u2, const float* amax_w, uint16_t* v, float* amax_v,
                       float* m, bool presplit, int N, int H, int W, int C, hipStream_t stream, const char* who) {
  const long T = (long)N * (H / 4) * (W / 4);
  if (presplit) {
    DSEE_TRY(dsee_wino43_input_f16x2(h, v, N, H, W, C, amax_h, DSEE_WINO_V_BOUND, stream));
    return gemm_nt(v, u2, m, 36 * T, C, C, T, C, amax_h, DSEE_WINO_V_BOUND, amax_w, stream);
  }
  DSEE_TRY(zero(amax_v, kAmaxFloats, stream, who));
  DSEE_TRY(dsee_wino43_input(h, reinterpret_cast<float*>(v), N, H, W, C, amax_v, stream));
  return dsee_gemm_f16x2_af32(reinterpret_cast<const float*>(v), u2, m, 36 * T, C, C, T, C, 0, amax_v, amax_w, stream);
}

// out = act(x + conv_1(lrelu(norm_1(conv_0(lrelu(norm_0(x))))))) in `workspace` (infer_scratch).  ready == NULL: every weight form is
// built here from norms[i]->w2a / ->table and convw[i].  Otherwise norms[i]->table is ignored: a SEAN norm's table is formed from
// ready->style right before the norm, and convw is not read.
int block_forward(const char* who, const dsee_norm_layer* const norms[2], const float* const convw[2], const float* const convb[2],
                  const BlockReady* ready, const uint8_t* labels, int lab_h, int lab_w, int shift, int label_nc, const float* x,
                  float* out, int out_act, int training, float eps, float momentum, float slope, int N, int H, int W, int C,
                  void* workspace, hipStream_t stream) {
  const int has_t = ready ? ready->norm[0].wst != nullptr : norms[0]->table != nullptr;
  Arena a = {static_cast<char*>(workspace), 0};
  const InferScratch F = infer_scratch(a, N, H, W, C, label_nc, has_t);
  const float* in = x;
  for (int i = 0; i < 2; ++i) {
    dsee_norm_layer nl = *norms[i];
    if (!training && !(nl.running_mean && nl.running_var)) {
      dsee_set_error("%s: evaluation mode needs the running statistics", who);
      return DSEE_EINVAL;
    }
    Arena na = {static_cast<char*>(workspace), 0};
    NormBufs b = norm_scratch(na, N, H, W, C, label_nc, has_t);
    DSEE_TRY(zero(F.amax_h, kAmaxFloats, stream, who));
    DSEE_TRY(zero(b.amax_cat, 3 * kAmaxFloats, stream, who));
    b.amax_u = b.amax_cat + kAmaxFloats;
    b.amax_h = F.amax_h;
    b.mean = F.stat;
    b.invstd = F.stat + C;
    b.out_h = F.h;
    if (ready) {
      const NormReady& r = ready->norm[i];
      b.tab = const_cast<float*>(r.tab);
      b.tab_ready = true;
      if (has_t) {
        // the slot that bounds the per-image weights: max |w2a| from the pack, max |table| on top of it from the table kernel
        if (hipMemcpyAsync(b.amax_u, r.amax_u, kAmaxFloats * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) {
          dsee_set_error("%s: hipMemcpyAsync of an operand maximum failed", who);
          return DSEE_ELAUNCH;
        }
        DSEE_TRY(dsee_style_table_fwd(ready->style, r.wst, ready->table, N, label_nc, ready->S, 2 * C, b.amax_u, stream));
        nl.table = ready->table;
        b.u_bound_ready = true;
        if (ready->norm_direct) {
          b.wp_direct = r.wp_direct;
          b.out_scale = F.m;      // (the direct kernel always writes the modulation factor: into the product buffer, free until the GEMM)
        }
      } else {
        nl.table = nullptr;
        b.u2 = const_cast<uint16_t*>(r.u2);
        b.amax_u = const_cast<float*>(r.amax_u);
        b.u_ready = true;
      }
    }
    DSEE_TRY(norm_forward(nl, labels, lab_h, lab_w, shift, label_nc, in, b, training ? kStatsOfX : kStatsRunning, nullptr, eps,
                          momentum, slope, N, H, W, C, stream));
    if (ready) {
      DSEE_TRY(wino_conv3x3_ready(F.h, F.amax_h, ready->u2conv[i], ready->amax_conv[i], F.v2, F.amax_w, F.m, ready->presplit, N, H, W,
                                  C, stream, who));
    } else {
      DSEE_TRY(zero(F.amax_w, kAmaxFloats, stream, who));
      DSEE_TRY(wino_conv3x3_product(F.h, F.amax_h, convw[i], F.amax_w, F.v2, F.u2, F.m, false, N, H, W, C, stream));
    }
    // conv_0: + bias into dx0; conv_1: + bias + the shortcut x, the block's activation
    DSEE_TRY(dsee_wino43_output(F.m, convb[i], i == 0 ? nullptr : x, C, i == 0 ? F.dx0 : out, N, H, W, C,
                                i == 0 ? DSEE_ACT_NONE : out_act, slope, nullptr, 0, 0, nullptr, 0, 0, nullptr, stream));
    in = F.dx0;
  }
  return DSEE_OK;
}

/* ---- the whole generator: layouts, kernel choices and checks of dsee_generator_prepare / dsee_generator_fwd ------------------------- */
constexpr float kSnEps = 1e-12f;       // torch.nn.utils.spectral_norm's eps (ops.py::SN_EPS)
constexpr float kBnEps = 1e-5f, kBnMomentum = 0.1f, kSlope = 0.2f;
constexpr double kDirectF16x2MinFlop = 1e9;     // KernelPlan.conv_f16x2_min_flop: `initial` takes split operands from here on

struct NormPrepared {
  float *w2a, *b2, *amax_u, *tab;
  void* forms;      // SPADE: u2 [36][2C][128] fp16x2 | SEAN: wst [9*2C][S], then wp [2C][1152]
};
struct GenPrepared {
  uint16_t* u2conv;           // [2 n_blocks][36][C][C] fp16x2, conv_0 / conv_1 of every block in forward order
  float* amax_conv;           // [2 n_blocks][2048]
  NormPrepared norm[DSEE_GEN_MAX_BLOCKS][2];
  float *wp_init, *amax_init, *wp_img;
  size_t u2_elems;            // int16 elements of one convolution's u2
  // scratch of dsee_generator_prepare behind the part the forward reads
  dsee_sn_layer* sn;
  int *work_k, *work_r, *work_e;
  float *sn_scratch, *sigma, *saved, *w_sn, *w27;
};
GenPrepared prepared_layout(Arena& a, int C, int nc, int S, int n_blocks) {
  const int rows = 2 * C, nl = 2 * n_blocks;
  const size_t K = (size_t)9 * C;
  GenPrepared P = {};
  P.u2_elems = (size_t)36 * dsee_conv_wrows(C) * dsee_conv_kpad(1, 1, C) * 2;
  P.u2conv = a.take<uint16_t>(nl * P.u2_elems);
  P.amax_conv = a.take<float>(nl * kAmaxFloats);
  const size_t spade = (size_t)36 * rows * kHidden * 2 * sizeof(uint16_t);
  const size_t sean = up256((size_t)9 * rows * S * sizeof(float)) +
                      (size_t)dsee_conv_wrows(rows) * dsee_conv_kpad(3, 3, kHidden) * sizeof(float);
  for (int i = 0; i < n_blocks; ++i)
    for (int j = 0; j < 2; ++j) {
      NormPrepared& n = P.norm[i][j];
      n.w2a = a.take<float>((size_t)rows * kHidden * 9);
      n.b2 = a.take<float>(rows);
      n.amax_u = a.take<float>(kAmaxFloats);
      n.tab = a.take<float>((size_t)9 * nc * kHidden);
      n.forms = a.bytes(spade > sean ? spade : sean);
    }
  P.wp_init = a.take<float>((size_t)dsee_conv_wrows(C) * dsee_conv_kpad(3, 3, 4));
  P.amax_init = a.take<float>(kAmaxFloats);
  P.wp_img = a.take<float>((size_t)dsee_conv_wrows(28) * dsee_conv_kpad(1, 1, C));
  P.sn = a.take<dsee_sn_layer>(nl);
  P.work_k = a.take<int>((size_t)2 * nl * ((K + 31) / 32));
  P.work_r = a.take<int>((size_t)2 * nl * C);
  P.work_e = a.take<int>((size_t)2 * nl * ((C * K + 4095) / 4096));
  P.sn_scratch = a.take<float>(nl * (C + K));
  P.sigma = a.take<float>(nl);
  P.saved = a.take<float>(nl * (C + K));
  P.w_sn = a.take<float>(nl * C * K);
  P.w27 = a.take<float>((size_t)27 * C);
  return P;
}
inline const float* sean_wst(const NormPrepared& n) { return static_cast<const float*>(n.forms); }
inline float* sean_wp(const NormPrepared& n, int C, int S) {
  return reinterpret_cast<float*>(static_cast<char*>(n.forms) + up256((size_t)9 * 2 * C * S * sizeof(float)));
}

struct GenScratch {
  float *x_lr, *amax, *feat[2], *table, *z, *rgb;     // amax: max |x_lr|, max |initial's output|
  void* block;                                        // infer_scratch of the level in flight
};
GenScratch gen_scratch(Arena& a, int C, int nc, int levels, int N, int h, int w) {
  const int H = h << levels, W = w << levels;
  const size_t px = (size_t)N * H * W;
  GenScratch G;
  G.x_lr = a.take<float>((size_t)N * h * w * 4);
  G.amax = a.take<float>(2 * kAmaxFloats);
  for (float*& f : G.feat) f = a.take<float>(px * C);
  G.table = a.take<float>((size_t)N * 9 * 2 * C * 32);
  G.z = a.take<float>(px * 28);
  G.rgb = a.take<float>(px * 4);
  G.block = a.base ? a.base + a.off : nullptr;
  infer_scratch(a, N, H, W, C, nc, 1);
  return G;
}

// ops.py::_wino_chunk on the split-operand path: the images per Winograd pass (0: none), whole 128-row GEMM tiles per group
int wino_chunk(int n, int h, int w, int cmax, bool per_image) {
  const long tpi = (long)(h / 4) * (w / 4);
  for (int nb = n; nb > 0; --nb)
    if (n % nb == 0 && 36L * nb * tpi * cmax * 6 < (1L << 34) && (per_image ? tpi : nb * tpi) % 128 == 0) return nb;
  return 0;
}

struct LevelChoice {
  bool norm_direct, presplit;
};
// The shape rules of one block's level (DSEE_EUNSUPPORTED with the level and the rule) and the kernels ops.py takes there.
int level_choice(const char* who, int level, int kind, int N, int H, int W, int C, int max_fm, LevelChoice* out) {
  const long tpi = (long)(H / 4) * (W / 4), T = N * tpi;
  const int sean = kind == DSEE_GEN_SEAN, rows = 2 * C, ld = kHidden + (sean ? 32 : 0);
  if (H % 4 != 0 || W % 4 != 0 || tpi % 64 != 0) {
    dsee_set_error("%s: level %d (%d x %d): H, W %% 4 == 0 and (H/4) (W/4) %% 64 == 0 required (the fused norm kernel owns blocks of "
                   "64 Winograd tiles of one image); the dense path of maps below 32 x 32 is not built", who, level, H, W);
    return DSEE_EUNSUPPORTED;
  }
  if (T % 256 != 0) {
    dsee_set_error("%s: level %d (%d x %d): N (H/4) (W/4) %% 256 == 0 required (N = %d, %ld tiles): the Winograd GEMMs take whole "
                   "256-row tiles", who, level, H, W, N, T);
    return DSEE_EUNSUPPORTED;
  }
  if (sean && (H > max_fm || W > max_fm)) {
    dsee_set_error("%s: level %d (%d x %d): a SEAN level above max_fm_size = %d: the capped path is not built", who, level, H, W,
                   max_fm);
    return DSEE_EUNSUPPORTED;
  }
  const int nb = wino_chunk(N, H, W, rows, sean);
  out->norm_direct = nb == 0;
  if (nb != 0 && !(36L * N * tpi * ld * 4 < 0xFFFFFFF0L && 36L * N * rows * ld * 4 < 0xFFFFFFF0L)) {
    dsee_set_error("%s: level %d (%d x %d): the gamma/beta operands exceed the fused norm kernel's 32-bit offsets (N = %d, C = %d); "
                   "the chunked norm path is not built", who, level, H, W, N, C);
    return DSEE_EUNSUPPORTED;
  }
  if (wino_chunk(N, H, W, C, false) != N) {
    dsee_set_error("%s: level %d (%d x %d): the batch does not fit one Winograd pass (N = %d, C = %d); the chunked convolution is "
                   "not built", who, level, H, W, N, C);
    return DSEE_EUNSUPPORTED;
  }
  // (ops.py::_presplit_ok: max |h| from the fused norm kernel, whole 256 x 256 tiles, at least presplit_min_tiles = 512 of them)
  out->presplit = !out->norm_direct && C % 256 == 0 && (36 * T / 256) * (C / 256) >= 512;
  return DSEE_OK;
}

int desc_levels(const dsee_generator_desc* d) {
  int levels = 0;
  for (int i = 0; i < d->n_blocks && i < DSEE_GEN_MAX_BLOCKS; ++i) levels += d->blocks[i].ups != 0;
  return levels;
}

// kinds and the rules that do not depend on the batch
int desc_supported(const char* who, const dsee_generator_desc* d) {
  if (d->n_blocks < 1 || d->n_blocks > DSEE_GEN_MAX_BLOCKS) {
    dsee_set_error("%s: n_blocks = %d (1..%d)", who, d->n_blocks, DSEE_GEN_MAX_BLOCKS);
    return DSEE_EUNSUPPORTED;
  }
  if (d->precision != DSEE_GEN_FP32) {
    dsee_set_error("%s: the 16-bit mode is not built: precision DSEE_GEN_FP32 only", who);
    return DSEE_EUNSUPPORTED;
  }
  if (d->norm != DSEE_GEN_NORM_BATCH) {
    dsee_set_error("%s: InstanceNorm norm_G is not built: BatchNorm running statistics only", who);
    return DSEE_EUNSUPPORTED;
  }
  for (int i = 0; i < d->n_blocks; ++i) {
    const int k = d->blocks[i].kind;
    if (k != DSEE_GEN_SPADE && k != DSEE_GEN_SEAN) {
      dsee_set_error("%s: block %d is %s: SPADE and SEAN blocks only (the PureSEAN tail of load_size >= 512 and the resnet / "
                     "puresean generators are not built)", who, i,
                     k == DSEE_GEN_PURESEAN ? "a PureSEAN block" : (k == DSEE_GEN_RESNET ? "a pix2pixHD ResnetBlock" : "of unknown kind"));
      return DSEE_EUNSUPPORTED;
    }
  }
  if (d->C < 128 || d->C % 128 != 0) {
    dsee_set_error("%s: C %% 128 == 0 required (C = %d): the Winograd GEMMs take whole 128-column tiles", who, d->C);
    return DSEE_EUNSUPPORTED;
  }
  if (d->label_nc < 1 || d->label_nc > 32) {
    dsee_set_error("%s: label_nc = %d (1..32: the one-hot label is stored in 32 channels)", who, d->label_nc);
    return DSEE_EUNSUPPORTED;
  }
  if (d->S < 4 || d->S % 4 != 0) {
    dsee_set_error("%s: regional_style_size S = %d (S %% 4 == 0: dsee_style_table_fwd reads 16-byte words)", who, d->S);
    return DSEE_EUNSUPPORTED;
  }
  return DSEE_OK;
}

// every offset of the descriptor addresses a whole tensor inside the flat parameter buffer
int desc_offsets_ok(const char* who, const dsee_generator_desc* d) {
  const long C = d->C, nc = d->label_nc, S = d->S, total = d->param_floats;
  bool ok = true;
  auto in = [&](int64_t off, long n) { ok = ok && off >= 0 && off + n <= total; };
  in(d->initial_w, C * 27);
  in(d->initial_b, C);
  in(d->conv_img_w, 27 * C);
  in(d->conv_img_b, 3);
  for (int i = 0; i < d->n_blocks; ++i) {
    const dsee_generator_block& b = d->blocks[i];
    for (const dsee_generator_conv* c : {&b.conv_0, &b.conv_1}) {
      in(c->weight_orig, C * C * 9);
      in(c->bias, C);
      in(c->weight_u, C);
      in(c->weight_v, 9 * C);
    }
    for (const dsee_generator_norm* n : {&b.norm_0, &b.norm_1}) {
      in(n->w_shared, kHidden * nc * 9);
      in(n->b_shared, kHidden);
      in(n->w_gamma, C * kHidden * 9);
      in(n->w_beta, C * kHidden * 9);
      in(n->b_gamma, C);
      in(n->b_beta, C);
      in(n->running_mean, C);
      in(n->running_var, C);
      if (b.kind == DSEE_GEN_SEAN) {
        in(n->ws_gamma, C * S * 9);
        in(n->ws_beta, C * S * 9);
        in(n->bs_gamma, C);
        in(n->bs_beta, C);
        in(n->alpha_gamma, 1);
        in(n->alpha_beta, 1);
      }
    }
  }
  if (!ok) {
    dsee_set_error("%s: an offset of the descriptor lies outside the parameter buffer of %ld floats", who, total);
    return DSEE_EINVAL;
  }
  return DSEE_OK;
}

// w27[(tap * Co + o)][c] = w[o][c][tap]: the to-RGB layer as a 1x1 convolution with 9 Co outputs (ops.py::conv2d, thin path)
__global__ __launch_bounds__(256) void tap_rows_kernel(const float* __restrict__ w, float* __restrict__ w27, int Co, int Ci) {
  const int total = 9 * Co * Ci;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int c = i % Ci, r = i / Ci, o = r % Co, tap = r / Co;
    w27[i] = w[((size_t)o * Ci + c) * 9 + tap];
  }
}

}  // namespace

extern "C" {

size_t dsee_sean_norm_fwd_workspace(int N, int H, int W, int C, int label_nc, int has_table) {
  Arena a = {nullptr, 0};
  norm_scratch(a, N, H, W, C, label_nc, has_table);
  return a.off;
}

int dsee_sean_norm_fwd(const uint8_t* labels, int lab_h, int lab_w, int shift, int label_nc, const float* w_shared,
                       const float* b_shared, const float* w2a, const float* table, const float* bias_packed, const float* x,
                       float* running_mean, float* running_var, int training, float eps, float momentum, float add_one,
                       float slope, float* out_h, float* out_scale, uint32_t* sign_mask, float* mean, float* invstd,
                       float* amax_h, int N, int H, int W, int C, void* workspace, size_t workspace_bytes,
                       hipStream_t stream) {
  static const char* who = "dsee_sean_norm_fwd";
  if (!(labels && w_shared && b_shared && w2a && bias_packed && x && out_h && mean && invstd && workspace)) {
    dsee_set_error("%s: NULL argument", who);
    return DSEE_EINVAL;
  }
  if (!((lab_h >> shift) == H && (lab_w >> shift) == W)) {
    dsee_set_error("%s: the label map (%d x %d >> %d) does not cover the %d x %d feature map", who, lab_h, lab_w, shift, H, W);
    return DSEE_EINVAL;
  }
  if (C % 64 != 0) {     // (dsee_sean_pack_fwd packs gamma|beta in groups of 64 channels: rows == 2 C only then)
    dsee_set_error("%s: C %% 64 == 0 required (C = %d)", who, C);
    return DSEE_EUNSUPPORTED;
  }
  if (N <= 0 || H % 4 != 0 || W % 4 != 0 || ((H / 4) * (W / 4)) % 64 != 0) {
    dsee_set_error("%s: H and W multiples of 4 with (H/4) (W/4) %% 64 == 0 required (the fused kernel owns blocks of "
                   "64 Winograd tiles of one image): N = %d, H = %d, W = %d", who, N, H, W);
    return DSEE_EUNSUPPORTED;
  }
  // (with and without table: the shared layer's weight gradient takes <= 32 classes too.  Like every check above it reads no
  // pointer: tests/test_label_nc_host.py passes addresses that must never be dereferenced.)
  if (label_nc < 1 || label_nc > 32) {
    dsee_set_error("%s: label_nc = %d (1..32: the one-hot label is stored in 32 channels)", who, label_nc);
    return DSEE_EUNSUPPORTED;
  }
  if (!training && !(running_mean && running_var)) {
    dsee_set_error("%s: evaluation mode needs the running statistics", who);
    return DSEE_EINVAL;
  }
  Arena a = {static_cast<char*>(workspace), 0};
  NormBufs b = norm_scratch(a, N, H, W, C, label_nc, table != nullptr);
  if (workspace_bytes < a.off) {
    dsee_set_error("%s: workspace of %zu bytes, %zu needed (dsee_sean_norm_fwd_workspace)", who, workspace_bytes, a.off);
    return DSEE_EINVAL;
  }
  DSEE_TRY(zero(b.amax_cat, 3 * kAmaxFloats, stream, who));
  b.amax_u = b.amax_cat + kAmaxFloats;
  b.amax_xhat = out_scale ? b.amax_cat + 2 * kAmaxFloats : nullptr;     // (serves the backward pass, like the modulation factor)
  b.amax_h = amax_h;
  b.mean = mean;
  b.invstd = invstd;
  b.out_h = out_h;
  b.out_scale = out_scale;
  b.sign_mask = sign_mask;
  const dsee_norm_layer nl = {w_shared, b_shared, w2a, table, bias_packed, running_mean, running_var, add_one};
  return norm_forward(nl, labels, lab_h, lab_w, shift, label_nc, x, b, training ? kStatsOfX : kStatsRunning, nullptr, eps, momentum,
                      slope, N, H, W, C, stream);
}

size_t dsee_spade_resblock_fwd_workspace(int N, int H, int W, int C, int label_nc, int has_table) {
  Arena a = {nullptr, 0};
  infer_scratch(a, N, H, W, C, label_nc, has_table);
  return a.off;
}

int dsee_spade_resblock_fwd(const dsee_norm_layer* norm_0, const float* w_conv_0, const float* b_conv_0,
                            const dsee_norm_layer* norm_1, const float* w_conv_1, const float* b_conv_1,
                            const uint8_t* labels, int lab_h, int lab_w, int shift, int label_nc, const float* x, float* out,
                            int out_act, int training, float eps, float momentum, float slope, int N, int H, int W, int C,
                            void* workspace, size_t workspace_bytes, hipStream_t stream) {
  static const char* who = "dsee_spade_resblock_fwd";
  if (!(norm_0 && norm_1 && w_conv_0 && w_conv_1 && labels && x && out && workspace)) {
    dsee_set_error("%s: NULL argument", who);
    return DSEE_EINVAL;
  }
  DSEE_TRY(block_args_ok(who, kInference, norm_0, norm_1, lab_h, lab_w, shift, label_nc, N, H, W, C, 0, workspace_bytes));
  const dsee_norm_layer* norms[2] = {norm_0, norm_1};
  const float* convw[2] = {w_conv_0, w_conv_1};
  const float* convb[2] = {b_conv_0, b_conv_1};
  return block_forward(who, norms, convw, convb, nullptr, labels, lab_h, lab_w, shift, label_nc, x, out, out_act, training, eps,
                       momentum, slope, N, H, W, C, workspace, stream);
}

size_t dsee_spade_resblock_saved_bytes(int N, int H, int W, int C, int label_nc, int has_table) {
  (void)label_nc;
  Arena a = {nullptr, 0};
  saved_layout(a, N, H, W, C, has_table);
  return a.off;
}

size_t dsee_spade_resblock_train_fwd_workspace(int N, int H, int W, int C, int label_nc, int has_table) {
  Arena a = {nullptr, 0};
  fwd_scratch(a, N, H, W, C, label_nc, has_table);
  return a.off;
}

int dsee_spade_resblock_train_fwd(const dsee_norm_layer* norm_0, const float* w_conv_0, const float* b_conv_0,
                                  const dsee_norm_layer* norm_1, const float* w_conv_1, const float* b_conv_1,
                                  const dsee_block_noise* noise, const uint8_t* labels, int lab_h, int lab_w, int shift,
                                  int label_nc, const float* x, float* out, float eps, float momentum, float slope, int N, int H,
                                  int W, int C, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                                  hipStream_t stream) {
  static const char* who = "dsee_spade_resblock_train_fwd";
  if (!(norm_0 && norm_1 && w_conv_0 && w_conv_1 && labels && x && out && saved && workspace)) {
    dsee_set_error("%s: NULL argument", who);
    return DSEE_EINVAL;
  }
  DSEE_TRY(block_args_ok(who, kTrainFwd, norm_0, norm_1, lab_h, lab_w, shift, label_nc, N, H, W, C, saved_bytes, workspace_bytes));
  const int has_t = norm_0->table != nullptr;
  Arena sa = {static_cast<char*>(saved), 0}, wa = {static_cast<char*>(workspace), 0};
  const BlockSaved S = saved_layout(sa, N, H, W, C, has_t);
  const FwdScratch F = fwd_scratch(wa, N, H, W, C, label_nc, has_t);
  const dsee_norm_layer* norms[2] = {norm_0, norm_1};
  const float* convw[2] = {w_conv_0, w_conv_1};
  DSEE_TRY(zero(S.amax_w, 2 * kAmaxFloats, stream, who));
  const float* in = x;
  for (int i = 0; i < 2; ++i) {
    const NormSaved& ns = S.n[i];
    float* const amax_h = ns.amax + 3 * kAmaxFloats;
    DSEE_TRY(zero(ns.amax, 4 * kAmaxFloats, stream, who));
    // (x comes from outside: a statistics pass; norm_1's rows were written by conv_0's output transform)
    const NormBufs b = {F.tab, ns.cat, F.stats, ns.v2cat, F.u2n, ns.amax, ns.amax + kAmaxFloats, ns.amax + 2 * kAmaxFloats, amax_h,
                        ns.mean, ns.invstd, F.h, ns.scale, ns.mask};
    DSEE_TRY(norm_forward(*norms[i], labels, lab_h, lab_w, shift, label_nc, in, b, i == 0 ? kStatsOfX : kStatsOfParts, F.part, eps,
                          momentum, slope, N, H, W, C, stream));
    // V2 of h is kept for the weight gradient
    DSEE_TRY(wino_conv3x3_product(F.h, amax_h, convw[i], S.amax_w + i * kAmaxFloats, S.v2h[i], F.u2c, F.m, true, N, H, W, C, stream));
    if (i == 0) {
      // conv_0: + bias, + noise_middle (architecture.py:111-112) regenerated in registers, BatchNorm rows of the result for norm_1
      DSEE_TRY(dsee_wino43_output_stats(F.m, b_conv_0, nullptr, C, S.dx0, N, H, W, C, DSEE_ACT_NONE, slope,
                                        noise ? noise->w_middle : nullptr, noise ? noise->seed_middle : 0,
                                        noise ? noise->offset_middle : 0, nullptr, 0, 0, F.part, stream));
      in = S.dx0;
    } else {
      // conv_1: + bias + the shortcut x + w_skip * eps_skip (architecture.py:127,133-134)
      DSEE_TRY(dsee_wino43_output(F.m, b_conv_1, x, C, out, N, H, W, C, DSEE_ACT_NONE, slope, nullptr, 0, 0,
                                  noise ? noise->w_skip : nullptr, noise ? noise->seed_skip : 0, noise ? noise->offset_skip : 0,
                                  nullptr, stream));
    }
  }
  return DSEE_OK;
}

size_t dsee_spade_resblock_bwd_workspace(int N, int H, int W, int C, int label_nc, int has_table, int lab_h, int lab_w, int shift) {
  (void)label_nc, (void)lab_h, (void)lab_w, (void)shift;
  Arena a = {nullptr, 0};
  bwd_scratch(a, N, H, W, C, has_table);
  return a.off;
}

int dsee_spade_resblock_bwd(const dsee_norm_layer* norm_0, const float* w_conv_0, const dsee_norm_layer* norm_1,
                            const float* w_conv_1, const dsee_block_noise* noise, const uint8_t* labels, int lab_h, int lab_w,
                            int shift, int label_nc, const float* x, const float* dout, const float* amax_dout,
                            const dsee_block_grads* grads, float* dx, float* amax_dx, float slope, int N, int H, int W, int C,
                            const void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  static const char* who = "dsee_spade_resblock_bwd";
  if (!(norm_0 && norm_1 && w_conv_0 && w_conv_1 && labels && x && dout && amax_dout && grads && dx && amax_dx && saved && workspace)) {
    dsee_set_error("%s: NULL argument", who);
    return DSEE_EINVAL;
  }
  DSEE_TRY(block_args_ok(who, kTrainBwd, norm_0, norm_1, lab_h, lab_w, shift, label_nc, N, H, W, C, saved_bytes, workspace_bytes));
  const int has_t = norm_0->table != nullptr;
  Arena sa = {const_cast<char*>(static_cast<const char*>(saved)), 0}, wa = {static_cast<char*>(workspace), 0};
  const BlockSaved S = saved_layout(sa, N, H, W, C, has_t);
  const BwdScratch B = bwd_scratch(wa, N, H, W, C, has_t);
  const int ld = kHidden + (has_t ? 32 : 0), rows = 2 * C, rows_tc = dsee_conv_wrows(C), rows_te = dsee_conv_wrows(kHidden);
  const long T = (long)N * (H / 4) * (W / 4);
  const size_t px = (size_t)N * H * W;
  const dsee_norm_layer* norms[2] = {norm_0, norm_1};
  const dsee_norm_grads* ngr[2] = {&grads->norm_0, &grads->norm_1};
  const float* convw[2] = {w_conv_0, w_conv_1};
  float* dwc[2] = {grads->dw_conv_0, grads->dw_conv_1};
  float* dbc[2] = {grads->db_conv_0, grads->db_conv_1};
  DSEE_TRY(zero(B.amax, 8 * kAmaxFloats, stream, who));
  float *amax_dh = B.amax, *amax_g = B.amax + kAmaxFloats, *amax_dmid = B.amax + 2 * kAmaxFloats, *amax_da = B.amax + 3 * kAmaxFloats;

  const float* g = dout;              // gradient w.r.t. the output of the convolution in flight
  const float* amax_gc = amax_dout;
  for (int i = 1; i >= 0; --i) {
    const NormSaved& ns = S.n[i];
    const dsee_norm_grads& ng = *ngr[i];
    float* const amax_cat = ns.amax;
    const float *amax_u = ns.amax + kAmaxFloats, *amax_xhat = ns.amax + 2 * kAmaxFloats, *amax_h = ns.amax + 3 * kAmaxFloats;
    const float* amax_w = S.amax_w + i * kAmaxFloats;
    // ---- Conv2d.backward (ops.py::_wino_wgrad with w_for_dx): ONE A dY A^T, pre-split, carrying the bias / NoiseInjection-weight
    //      sums; weight gradient on the kept V2; data gradient in the adjoint form
    float* dnw0 = (i == 0 && noise && noise->w_middle) ? grads->dw_noise_middle : nullptr;   // conv_0: y += w_middle * eps
    float* dnw1 = (i == 1 && noise && noise->w_skip) ? grads->dw_noise_skip : nullptr;       // conv_1: residual + w_skip * eps
    DSEE_TRY(dsee_wino43_dout_f16x2(g, B.dm2c, N, H, W, C, amax_gc, 1.0f, B.chws, dbc[i] ? B.dbias : nullptr, dnw0 ? B.dbias + C : nullptr,
                                    dnw0 ? noise->seed_middle : 0, dnw0 ? noise->offset_middle : 0, dnw1 ? B.dbias + 2 * C : nullptr,
                                    dnw1 ? noise->seed_skip : 0, dnw1 ? noise->offset_skip : 0, stream));
    if ((dbc[i] && hipMemcpyAsync(dbc[i], B.dbias, C * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) ||
        (dnw0 && hipMemcpyAsync(dnw0, B.dbias + C, C * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) ||
        (dnw1 && hipMemcpyAsync(dnw1, B.dbias + 2 * C, C * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess)) {
      dsee_set_error("%s: hipMemcpyAsync of the channel sums failed", who);
      return DSEE_ELAUNCH;
    }
    if (dwc[i])
      DSEE_TRY(dsee_wino43_wgrad(reinterpret_cast<const float*>(S.v2h[i]), reinterpret_cast<const float*>(B.dm2c), B.wsw, B.wsw_bytes,
                                 dwc[i], T, C, C, C, C, 6, amax_h, amax_gc, stream));
    DSEE_TRY(dsee_wino43_weights(convw[i], reinterpret_cast<float*>(B.utc), C, C, 2, 2, amax_w, stream));
    DSEE_TRY(gemm_nt(B.dm2c, B.utc, B.dv, 36 * T, C, C, T, rows_tc, amax_gc, 1.0f, amax_w, stream));
    DSEE_TRY(zero(amax_dh, kAmaxFloats, stream, who));
    DSEE_TRY(dsee_wino43_input_adjoint_amax(B.dv, B.dh, N, H, W, C, amax_dh, stream));

    // ---- SeanNormTable.backward: BN + modulate + LeakyReLU backward (reduce pass writes dM = A (g xhat | g) A^T pre-split; the
    //      apply pass adds the shortcut's gradient for norm_0), table / gamma-beta weight gradient, embedding gradient (adjoint),
    //      mlp_shared gradients
    const float* xin = i == 0 ? x : S.dx0;
    float* dxo = i == 0 ? dx : B.dmid;
    float* amax_dxo = i == 0 ? amax_dx : amax_dmid;
    DSEE_TRY(zero(amax_g, kAmaxFloats, stream, who));
    DSEE_TRY(dsee_amax_product(amax_dh, amax_xhat, 1.0f, amax_g, stream));
    DSEE_TRY(dsee_modulate_bwd_reduce_wino_f16x2(B.dh, nullptr, xin, ns.scale, ns.mean, ns.invstd, B.dm2n, rows, B.sums, N, H, W, C,
                                                 slope, B.wsmod, amax_g, 1.0f, ns.mask, stream));
    DSEE_TRY(zero(amax_dxo, kAmaxFloats, stream, who));
    DSEE_TRY(dsee_modulate_bwd_apply_amax(B.dh, nullptr, xin, ns.scale, ns.mean, ns.invstd, B.sums, i == 0 ? dout : nullptr, dxo, N,
                                          H * W, C, 1.0f / (float)px, slope, amax_dxo, 0, ns.mask, stream));
    DSEE_TRY(dsee_wino43_weights(norms[i]->w2a, reinterpret_cast<float*>(B.ute), rows, kHidden, 2, 2, amax_u, stream));
    if (has_t)
      DSEE_TRY(dsee_wino43_wgrad_table(reinterpret_cast<const float*>(ns.v2cat), reinterpret_cast<const float*>(B.dm2n), B.wst,
                                       B.wst_bytes, ng.dw2a, ng.dtable, T, N, kHidden, rows, label_nc, 6, amax_cat, amax_g, stream));
    else
      DSEE_TRY(dsee_wino43_wgrad(reinterpret_cast<const float*>(ns.v2cat), reinterpret_cast<const float*>(B.dm2n), B.wst, B.wst_bytes,
                                 ng.dw2a, T, ld, rows, rows, kHidden, 6, amax_cat, amax_g, stream));
    DSEE_TRY(dsee_gemm_f16x2_pre(B.dm2n, B.ute, B.dve, 36 * T, kHidden, rows, T, rows_te, amax_g, 1.0f, amax_u, stream));
    DSEE_TRY(zero(amax_da, kAmaxFloats, stream, who));
    if (has_t) {
      // (the ReLU of the embedding rides in the adjoint transform as a mask on `cat`; mlp_shared -- a convolution over the
      // one-hot label -- takes its weight gradient w.r.t. the one-hot channels already sitting in `cat`)
      DSEE_TRY(dsee_wino43_input_adjoint(B.dve, ns.cat, ld, B.dactv, N, H, W, kHidden, nullptr, amax_da, stream));
      const dsee_conv_geom gs = {N, H, W, ld, H, W, kHidden, 3, 3, 1, -1, 1, 0, 0, 1};
      if (ng.dw_shared)
        DSEE_TRY(shared_wgrad(&gs, ns.cat, amax_cat, false, B.dactv, amax_da, B, ng.dw_shared, kHidden, label_nc, stream));
      if (ng.db_shared) DSEE_TRY(dsee_channel_dot(B.dactv, nullptr, ng.db_shared, (long)px, kHidden, B.chws, stream));
    } else {
      DSEE_TRY(dsee_wino43_input_adjoint_amax(B.dve, B.dactv, N, H, W, kHidden, amax_da, stream));
      if (ng.dw_shared || ng.db_shared) {
        // ReLU backward of the embedding (+ max |g|); for the weight gradient the one-hot label channels materialised; the bias
        // gradient as a channel sum
        float *amax_g1 = B.amax + 4 * kAmaxFloats, *amax_oh = B.amax + 5 * kAmaxFloats;
        DSEE_TRY(zero(amax_g1, 2 * kAmaxFloats, stream, who));
        DSEE_TRY(dsee_act_bwd_amax(B.dactv, ns.cat, B.g1, (long)(px * kHidden), DSEE_ACT_RELU, slope, amax_g1, stream));
        if (ng.dw_shared) {
          DSEE_TRY(dsee_label_onehot(labels, B.oh, N, lab_h, lab_w, shift, 32, 0, stream));
          const dsee_conv_geom gs = {N, H, W, 32, H, W, kHidden, 3, 3, 1, -1, 1, 0, 0, 1};
          DSEE_TRY(shared_wgrad(&gs, B.oh, amax_oh, true, B.g1, amax_g1, B, ng.dw_shared, 0, label_nc, stream));
        }
        if (ng.db_shared) DSEE_TRY(dsee_channel_dot(B.g1, nullptr, ng.db_shared, (long)px, kHidden, B.chws, stream));
      }
    }
    if (ng.dgamma_beta_sums &&
        hipMemcpyAsync(ng.dgamma_beta_sums, B.sums + 2 * C, 2 * C * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) {
      dsee_set_error("%s: hipMemcpyAsync of the gamma / beta sums failed", who);
      return DSEE_ELAUNCH;
    }
    g = B.dmid;
    amax_gc = amax_dmid;
  }
  return DSEE_OK;
}

size_t dsee_generator_prepared_bytes(int C, int label_nc, int S, int n_blocks) {
  if (C < 1 || label_nc < 1 || S < 1 || n_blocks < 1 || n_blocks > DSEE_GEN_MAX_BLOCKS) return 0;
  Arena a = {nullptr, 0};
  prepared_layout(a, C, label_nc, S, n_blocks);
  return a.off;
}

size_t dsee_generator_fwd_workspace(int C, int label_nc, int levels, int N, int h, int w) {
  if (C < 1 || label_nc < 1 || levels < 0 || levels > DSEE_GEN_MAX_BLOCKS || N < 1 || h < 1 || w < 1) return 0;
  Arena a = {nullptr, 0};
  gen_scratch(a, C, label_nc, levels, N, h, w);
  return a.off;
}

int dsee_generator_prepare(const dsee_generator_desc* desc, const float* params, void* prepared, size_t prepared_bytes,
                           hipStream_t stream) {
  static const char* who = "dsee_generator_prepare";
  if (!(desc && params && prepared)) {
    dsee_set_error("%s: NULL argument", who);
    return DSEE_EINVAL;
  }
  DSEE_TRY(desc_supported(who, desc));
  const int C = desc->C, nc = desc->label_nc, S = desc->S, nb = desc->n_blocks, nl = 2 * nb, rows = 2 * C, K = 9 * C;
  const size_t need = dsee_generator_prepared_bytes(C, nc, S, nb);
  if (prepared_bytes < need) {
    dsee_set_error("%s: prepared buffer of %zu bytes, %zu needed (dsee_generator_prepared_bytes)", who, prepared_bytes, need);
    return DSEE_EINVAL;
  }
  DSEE_TRY(desc_offsets_ok(who, desc));
  Arena a = {static_cast<char*>(prepared), 0};
  const GenPrepared P = prepared_layout(a, C, nc, S, nb);

  // ---- eval-mode spectral norm of all 2 n_blocks convolutions as one group (ops.py::SNGroup: sigma from the stored u, v), their
  //      Winograd-domain weights in one launch behind it
  std::vector<dsee_sn_layer> sn(nl);
  std::vector<int> wk, wr, we;
  long out_off = 0, saved_off = 0;
  int sc_off = 0;
  for (int i = 0; i < nl; ++i) {
    const dsee_generator_conv& c = (i & 1) ? desc->blocks[i / 2].conv_1 : desc->blocks[i / 2].conv_0;
    sn[i] = {params + c.weight_orig, const_cast<float*>(params + c.weight_u), const_cast<float*>(params + c.weight_v), out_off,
             saved_off, C, K, sc_off, 0};      // (power_iter = 0: u and v are only read)
    for (int j = 0; j < (K + 31) / 32; ++j) wk.insert(wk.end(), {i, j});
    for (int j = 0; j < C; ++j) wr.insert(wr.end(), {i, j});
    for (int j = 0; j < (int)(((long)C * K + 4095) / 4096); ++j) we.insert(we.end(), {i, j});
    out_off += ((long)C * K + 3) / 4 * 4;
    saved_off += (C + K + 3) / 4 * 4;
    sc_off += C + K;
  }
  if (hipMemcpyAsync(P.sn, sn.data(), sn.size() * sizeof(dsee_sn_layer), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(P.work_k, wk.data(), wk.size() * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(P.work_r, wr.data(), wr.size() * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(P.work_e, we.data(), we.size() * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess) {
    dsee_set_error("%s: copying the spectral-norm tables to the device failed", who);
    return DSEE_ELAUNCH;
  }
  DSEE_TRY(zero(P.amax_conv, nl * kAmaxFloats, stream, who));
  DSEE_TRY(dsee_spectral_norm_group_fwd(P.sn, nl, P.work_k, (int)wk.size() / 2, P.work_r, (int)wr.size() / 2, P.work_e,
                                        (int)we.size() / 2, 0, kSnEps, P.sn_scratch, P.sigma, P.w_sn, P.saved, P.amax_conv, stream));
  DSEE_TRY(dsee_wino43_weights_batch(P.w_sn, reinterpret_cast<float*>(P.u2conv), nl, (long)C * K, (long)(P.u2_elems / 2), C, C, 0, 2,
                                     P.amax_conv, stream));

  // ---- the direct layers at both ends: `initial` packed tap-major over 4 stored channels (with its maximum, for the split-operand
  //      form large batches take), conv_img as a 1x1 layer with 27 outputs
  DSEE_TRY(dsee_pack_weight_fwd(params + desc->initial_w, nullptr, nullptr, P.wp_init, C, 3, 3, 3, 4, 0, stream));
  DSEE_TRY(zero(P.amax_init, kAmaxFloats, stream, who));
  DSEE_TRY(dsee_absmax(P.wp_init, (long)dsee_conv_wrows(C) * dsee_conv_kpad(3, 3, 4), P.amax_init, stream));
  tap_rows_kernel<<<(27 * C + 255) / 256, 256, 0, stream>>>(params + desc->conv_img_w, P.w27, 3, C);
  if (hipGetLastError() != hipSuccess) {
    dsee_set_error("%s: launch failed", who);
    return DSEE_ELAUNCH;
  }
  DSEE_TRY(dsee_pack_weight_fwd(P.w27, nullptr, nullptr, P.wp_img, 27, C, 1, 1, C, 1, stream));

  // ---- per norm layer: the packed, blended weight set with max |w2a|, mlp_shared's gather table, and the form of w2a its kernel reads
  for (int i = 0; i < nb; ++i) {
    const bool sean = desc->blocks[i].kind == DSEE_GEN_SEAN;
    for (int j = 0; j < 2; ++j) {
      const dsee_generator_norm& n = j ? desc->blocks[i].norm_1 : desc->blocks[i].norm_0;
      const NormPrepared& o = P.norm[i][j];
      auto at = [&](int64_t off) { return params + off; };
      DSEE_TRY(zero(o.amax_u, kAmaxFloats, stream, who));
      if (sean) {
        float* wst = static_cast<float*>(o.forms);
        DSEE_TRY(dsee_sean_pack_fwd(at(n.w_gamma), at(n.w_beta), at(n.ws_gamma), at(n.ws_beta), at(n.b_gamma), at(n.b_beta),
                                    at(n.bs_gamma), at(n.bs_beta), at(n.alpha_gamma), at(n.alpha_beta), 1, C, kHidden, S, o.w2a, wst,
                                    o.b2, o.amax_u, stream));
        DSEE_TRY(dsee_pack_weight_fwd(o.w2a, nullptr, nullptr, sean_wp(o, C, S), rows, kHidden, 3, 3, kHidden, 1, stream));
      } else {
        DSEE_TRY(dsee_sean_pack_fwd(at(n.w_gamma), at(n.w_beta), nullptr, nullptr, at(n.b_gamma), at(n.b_beta), nullptr, nullptr,
                                    nullptr, nullptr, 0, C, kHidden, 0, o.w2a, nullptr, o.b2, o.amax_u, stream));
        DSEE_TRY(dsee_wino43_weights(o.w2a, static_cast<float*>(o.forms), rows, kHidden, 0, 2, o.amax_u, stream));
      }
      DSEE_TRY(dsee_onehot_conv3x3_pack(at(n.w_shared), o.tab, kHidden, nc, stream));
    }
  }
  // (the tables above were copied from host vectors that end with this call)
  if (hipStreamSynchronize(stream) != hipSuccess) {
    dsee_set_error("%s: hipStreamSynchronize failed", who);
    return DSEE_ELAUNCH;
  }
  return DSEE_OK;
}

int dsee_generator_fwd(const dsee_generator_desc* desc, const float* params, const void* prepared, size_t prepared_bytes,
                       const float* image_lr, const uint8_t* labels, int lab_h, int lab_w, const float* style, float* out, int N,
                       int h, int w, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  static const char* who = "dsee_generator_fwd";
  if (!(desc && params && prepared && image_lr && labels && style && out && workspace)) {
    dsee_set_error("%s: NULL argument", who);
    return DSEE_EINVAL;
  }
  DSEE_TRY(desc_supported(who, desc));
  if (N < 1 || h < 1 || w < 1) {
    dsee_set_error("%s: N = %d, LR image of %d x %d", who, N, h, w);
    return DSEE_EUNSUPPORTED;
  }
  const int C = desc->C, nc = desc->label_nc, S = desc->S, nb = desc->n_blocks, levels = desc_levels(desc);
  LevelChoice choice[DSEE_GEN_MAX_BLOCKS];
  for (int i = 0, level = 0; i < nb; ++i) {
    level += desc->blocks[i].ups != 0;
    DSEE_TRY(level_choice(who, level, desc->blocks[i].kind, N, h << level, w << level, C, desc->max_fm_size, &choice[i]));
  }
  const int H = h << levels, W = w << levels;
  if (lab_h != H || lab_w != W) {
    dsee_set_error("%s: the label map (%d x %d) does not match the output of %d x %d (LR %d x %d << %d levels)", who, lab_h, lab_w, H,
                   W, h, w, levels);
    return DSEE_EINVAL;
  }
  const size_t pneed = dsee_generator_prepared_bytes(C, nc, S, nb), wneed = dsee_generator_fwd_workspace(C, nc, levels, N, h, w);
  if (prepared_bytes < pneed) {
    dsee_set_error("%s: prepared buffer of %zu bytes, %zu needed (dsee_generator_prepared_bytes)", who, prepared_bytes, pneed);
    return DSEE_EINVAL;
  }
  if (workspace_bytes < wneed) {
    dsee_set_error("%s: workspace of %zu bytes, %zu needed (dsee_generator_fwd_workspace)", who, workspace_bytes, wneed);
    return DSEE_EINVAL;
  }
  DSEE_TRY(desc_offsets_ok(who, desc));
  Arena pa = {const_cast<char*>(static_cast<const char*>(prepared)), 0}, wa = {static_cast<char*>(workspace), 0};
  const GenPrepared P = prepared_layout(pa, C, nc, S, nb);      // (read only from here on)
  const GenScratch G = gen_scratch(wa, C, nc, levels, N, h, w);

  // ---- NCHW -> NHWC (3 channels stored as 4), `initial` on the direct kernel (sr.py:90)
  DSEE_TRY(dsee_nchw_to_nhwc(image_lr, G.x_lr, N, 3, h, w, 4, stream));
  DSEE_TRY(zero(G.amax, 2 * kAmaxFloats, stream, who));
  const dsee_conv_geom gi = {N, h, w, 4, h, w, C, 3, 3, 1, -1, 1, 0, 0, 0};
  int cur = 0;       // feat[cur] holds the feature map; an upsample and a block each write the other buffer
  if (2.0 * N * h * w * C * 36.0 >= kDirectF16x2MinFlop) {
    DSEE_TRY(dsee_absmax(G.x_lr, (long)N * h * w * 4, G.amax, stream));
    DSEE_TRY(dsee_conv2d_fwd_f16x2_amax(&gi, G.x_lr, P.wp_init, params + desc->initial_b, nullptr, 0, G.feat[cur], DSEE_ACT_NONE, kSlope,
                                        G.amax, P.amax_init, G.amax + kAmaxFloats, 0, stream));
  } else {
    DSEE_TRY(dsee_conv2d_fwd_amax(&gi, G.x_lr, P.wp_init, params + desc->initial_b, nullptr, 0, G.feat[cur], DSEE_ACT_NONE, kSlope,
                                  G.amax + kAmaxFloats, stream));
  }

  // ---- the blocks (sr.py:91-93): nearest x2 where the block has `ups`, LeakyReLU of sr.py:94 in the last block's epilogue
  int Hc = h, Wc = w, level = 0;
  for (int i = 0; i < nb; ++i) {
    const dsee_generator_block& blk = desc->blocks[i];
    if (blk.ups) {
      Hc <<= 1, Wc <<= 1, ++level;
      DSEE_TRY(dsee_upsample_noise_fwd(G.feat[cur], nullptr, nullptr, G.feat[cur ^ 1], N, Hc, Wc, C, 1, stream));
      cur ^= 1;
    }
    const bool sean = blk.kind == DSEE_GEN_SEAN;
    dsee_norm_layer nls[2];
    BlockReady R = {};
    for (int j = 0; j < 2; ++j) {
      const dsee_generator_norm& n = j ? blk.norm_1 : blk.norm_0;
      const NormPrepared& p = P.norm[i][j];
      // (evaluation mode: the running statistics are only read)
      nls[j] = {params + n.w_shared, params + n.b_shared, p.w2a, nullptr, p.b2, const_cast<float*>(params + n.running_mean),
                const_cast<float*>(params + n.running_var), 1.0f};
      R.norm[j] = {p.tab, p.amax_u, sean ? nullptr : static_cast<const uint16_t*>(p.forms), sean ? sean_wst(p) : nullptr,
                   sean ? sean_wp(p, C, S) : nullptr};
      R.u2conv[j] = P.u2conv + (size_t)(2 * i + j) * P.u2_elems;
      R.amax_conv[j] = P.amax_conv + (size_t)(2 * i + j) * kAmaxFloats;
    }
    R.style = style;
    R.S = S;
    R.table = G.table;
    R.norm_direct = sean && choice[i].norm_direct;
    R.presplit = choice[i].presplit;
    const dsee_norm_layer* norms[2] = {&nls[0], &nls[1]};
    const float* convb[2] = {params + blk.conv_0.bias, params + blk.conv_1.bias};
    const float* convw[2] = {nullptr, nullptr};
    DSEE_TRY(block_forward(who, norms, convw, convb, &R, labels, lab_h, lab_w, levels - level, nc, G.feat[cur], G.feat[cur ^ 1],
                           i == nb - 1 ? DSEE_ACT_LRELU : DSEE_ACT_NONE, 0, kBnEps, kBnMomentum, kSlope, N, Hc, Wc, C, G.block, stream));
    cur ^= 1;
  }

  // ---- conv_img + tanh (sr.py:95-96) as a 1x1 layer with 27 outputs and a 9-point gather, NHWC -> NCHW
  const dsee_conv_geom go = {N, H, W, C, H, W, 28, 1, 1, 1, 0, 1, 0, 0, 1};
  DSEE_TRY(dsee_conv2d_fwd_amax(&go, G.feat[cur], P.wp_img, nullptr, nullptr, 0, G.z, DSEE_ACT_NONE, kSlope, nullptr, stream));
  DSEE_TRY(dsee_thin_gather_fwd(G.z, params + desc->conv_img_b, G.rgb, N, H, W, 28, 3, DSEE_ACT_TANH, kSlope, stream));
  return dsee_nhwc_to_nchw(G.rgb, out, N, 3, H, W, 4, stream);
}

}  // extern "C"
