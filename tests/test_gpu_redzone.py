"""Existing GPU test bodies re-run inside tests/redzone.py's harness: every device buffer the C ABI receives sits between two
guard bands in an exact-sized arena, every workspace is exact-sized, fresh and poisoned, `ops.new` / `ops._i16` outputs and the
allocator's free blocks start from NaN.  The bodies' own float64 / oracle assertions run unchanged on top of that; the harness
adds: no byte outside a buffer is written, no pointer reaches the library unguarded outside redzone.ALLOWLIST.  The last test
holds the set of entry points that ran guarded against include/deepsee_hip.h.

Cases: the smallest parametrisation of every layer-level test plus every parametrisation whose comment names a ragged, odd,
tail or regression path.  Every scenario names a parametrisation the original test declares (checked at import)."""
import contextlib
import inspect
import random
import re
import time

import pytest
import torch

import redzone
import test_gpu_conv as TC
import test_gpu_explore as TE
import test_gpu_gan_mode as TG
import test_gpu_instance_norm as TI
import test_gpu_label_nc as TK
import test_gpu_loader as TL
import test_gpu_model as TM
import test_gpu_ms_ssim as TS
import test_gpu_nonspade_norm as TN
import test_gpu_ops as TO
import test_gpu_random_style as TR
import test_gpu_rect as TQ
import test_gpu_visuals as TV
from test_gpu_visuals import gold  # noqa: F401  (the module-scoped fixture of the visuals bodies)
from oracle import deepsee_oracle as O

pytestmark = pytest.mark.gpu


_PARAM = type(pytest.param())


def rows_of(func, argnames=None):
    """The parametrize rows of a test function as plain tuples (one mark, or the one whose argnames are given)."""
    for m in getattr(func, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names = [a.strip() for a in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
        if argnames is None or names == [a.strip() for a in argnames.split(",")]:
            rows = []
            for r in m.args[1]:
                vals = r.values if isinstance(r, _PARAM) else (tuple(r) if len(names) > 1 else (r,))
                rows.append(tuple(vals) if len(names) > 1 else vals[0])
            return names, rows
    raise LookupError("%s has no such parametrize mark" % func.__name__)


def _declared(func, kwargs):
    for m in getattr(func, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names, rows = rows_of(func, m.args[0] if isinstance(m.args[0], str) else ",".join(m.args[0]))
        want = tuple(kwargs[n] for n in names) if len(names) > 1 else kwargs[names[0]]
        assert want in rows, "%s: %r is not a declared parametrisation of %s" % (func.__name__, want, names)


SCENARIOS = []


def S(func, _plan=None, _twins=False, **kwargs):
    """One scenario: func(**kwargs) inside the harness; `_plan`: KernelPlan overrides the body runs under (the layer tests
    consult the calling thread's plan, autograd nodes the one their forward recorded); `_twins`: see twin_calls()."""
    _declared(func, kwargs)
    tag = "-".join(re.sub(r"[^A-Za-z0-9.x]+", "_", "x".join(map(str, v)) if isinstance(v, tuple) else str(v)).strip("_")
                   for v in kwargs.values())
    if _plan:
        tag += "-plan_" + "_".join("%s_%s" % kv for kv in _plan.items())
    if _twins:
        tag += "-twins"
    name = func.__name__[5:] if func.__name__.startswith("test_") else func.__name__
    SCENARIOS.append(pytest.param(func, kwargs, dict(plan=_plan, twins=_twins), id=(name + ("-" + tag.strip("-") if tag else ""))[:110]))


def _conv_case(*prefix):
    (row,) = [c for c in TC.CASES if c[:4] == prefix]
    return row


def _smallest(func, argnames, work):
    names, rows = rows_of(func, argnames)
    return dict(zip(names, min(rows, key=work)))


def _with(func, argnames, name, value):
    names, rows = rows_of(func, argnames)
    return [dict(zip(names, r)) for r in rows if r[names.index(name)] == value]


def _prod4(r):
    return r[0] * r[1] * r[2] * r[3]


# ---------------------------------------------------------------------------------------------- direct / implicit-GEMM conv
for _p in [(1, 64, 192, 12), (2, 3, 64, 20), (2, 64, 3, 16), (2, 22, 32, 17), (1, 256, 1, 10), (2, 32, 64, (16, 40)),
           (2, 32, 64, (40, 16)), (8, 3, 64, 50), (6, 128, 128, 64), (16, 64, 128, (64, 16))]:
    for _f in (False, True):
        S(TC.test_conv_fwd_dgrad_wgrad, case=_conv_case(*_p), f16x2=_f)

# ---------------------------------------------------------------------------------------------- Winograd and the 16-bit mode
S(TC.test_winograd_conv_autograd_function, n=2, cin=128, cout=256, h=32, act=1, use_res=True)
S(TC.test_winograd_conv_autograd_function, n=4, cin=128, cout=128, h=(16, 32), act=1, use_res=True)
S(TC.test_winograd_conv_16bit_storage_mode, n=8, cin=128, cout=128, h=(16, 32))
S(TC.test_winograd_conv_16bit_storage_mode, n=2, cin=256, cout=256, h=64)      # 256-row tiles: the adjoint data gradient
S(TC.test_transforms_packed_one_term, n=1, h=32, c=96)
S(TC.test_transforms_packed_one_term, n=2, h=32, c=160)
S(TC.test_dout_transform_pre_split_with_channel_sums, n=2, h=32, c=48)
S(TC.test_dout_transform_pre_split_with_channel_sums, n=1, h=(8, 64), c=48)
S(TC.test_bf16x3_adds_no_error_to_the_winograd_conv)
S(TC.test_small_channel_keeps_its_precision_in_the_winograd_conv, shift=16)
S(TC.test_wino43_weights_lds_staged_form_is_bit_identical, co=64, ci=192, flip=1, split=2)
S(TC.test_wino43_weights_lds_staged_form_is_bit_identical, co=64, ci=192, flip=2, split=4)

# ---------------------------------------------------------------------------------------------- GEMMs: smallest row + the K tail
for _t, _names, _tail in [(TC.test_gemm_bf16x3_is_fp32_accurate, "groups,tg,n,k,tile", "k"),
                          (TC.test_gemm_bf16x3_af32, "groups,tg,n,k,tile", "k"),
                          (TC.test_gemm_f16x2_is_fp32_accurate, "groups,tg,n,k,tile,spread", "k"),
                          (TC.test_gemm_f16x2_tn_matches_float64, "groups,t,rp,rq,splits", "rq"),
                          (TC.test_gemm_f16x2_tn_pre_split_q, "groups,t,rp,rq,splits,bound", "rq"),
                          (TC.test_gemm_f16x2_tn_both_operands_pre_split, "groups,t,rp,rq,splits", "rq"),
                          (TC.test_gemm_f16p_tn_packed_one_term, "groups,t,rp,rq,splits", "rq")]:
    _rows = [_smallest(_t, _names, _prod4)] + _with(_t, _names, _tail, 160)
    for _kw in [r for i, r in enumerate(_rows) if r not in _rows[:i]]:
        S(_t, **_kw)
for _t in (TC.test_gemm_f16x2_pre_split_a, TC.test_gemm_f16p_pre_packed_one_term):
    _rows = [_smallest(_t, "groups,tg,n,k,bound", _prod4)] + _with(_t, "groups,tg,n,k,bound", "k", 160)
    for _kw in [r for i, r in enumerate(_rows) if r not in _rows[:i]]:
        for _k in ("w8", "w4"):
            if _t is TC.test_gemm_f16p_pre_packed_one_term and _k == "w4" and (_kw["n"] % 256 or _kw["k"] % 64):
                continue        # (the body skips: gemm_f16p_pre_w4 takes whole 256-column tiles and an even number of 32-k slabs)
            S(_t, kernel=_k, **_kw)
S(TC.test_gemm_f16p_pre_packed_one_term, kernel="w4", groups=2, tg=512, n=512, k=512, bound=100.0)   # its smallest w4 row
S(TC.test_gemm_f16x2_tn_long_chain_accuracy)
for _m in ("f16x2", "bf16x3", "f16"):
    S(TC.test_pipelined_gemms_with_poisoned_lds, mode=_m)

# ---------------------------------------------------------------------------------------------- thin convolutions
S(TC.test_thin_conv3x3, n=2, cin=128, cout=3, h=32, w=48, act=3, use_bias=True)
S(TC.test_thin_conv3x3, n=1, cin=512, cout=2, h=16, w=16, act=1, use_bias=False)
for _m in [(3 * 17 * 5, 128, 27, 28), (4096 + 3, 640, 32, 32), (77, 256, 5, 8)]:
    S(TC.test_thin_1x1_backward, **dict(zip("mck", _m), ldz=_m[3]))
for _r in [(2, 22, 32, 17, 4, 2, 2, True), (2, 256, 1, 10, 4, 1, 2, True), (2, 256, 1, (10, 13), 4, 1, 2, True)]:
    S(TO.test_discriminator_layer_paths, **dict(zip(("n", "cin", "cout", "h", "k", "stride", "pad", "bias"), _r)))

# ---------------------------------------------------------------------------------------------- norms
for _r in [("spade", 8, 8, 2), ("sean", 64, 16, 2), ("puresean", 32, 8, 2), ("sean", 64, (8, 16), 2), ("spade", 8, (16, 8), 2)]:
    S(TO.test_spade_sean_norm_fwd_bwd, **dict(zip(("kind", "C", "R", "N"), _r)))
S(TO.test_sean_norm_table_path, kind="spade", C=64, R=16, N=2, max_fm=256)
S(TO.test_sean_norm_table_path, kind="sean", C=64, R=16, N=2, max_fm=256)
S(TO.test_sean_norm_table_path, kind="puresean", C=64, R=16, N=2, max_fm=8)
for _pk in (False, True):
    S(TC.test_spade_fused_forward_vs_float64, n=2, h=32, c=64, per_image=True, with_scale=True, packed=_pk, waves=8)
S(TC.test_norm_backward_reduce_writes_pre_split_gradient, n=2, h=32, c=64)
S(TC.test_norm_backward_reduce_writes_pre_split_gradient, n=2, h=(16, 64), c=64)
S(TO.test_instnorm_act, act=1)
S(TO.test_instnorm_act, act=3)
S(TN.test_bn_act_layer_vs_float64, N=2, H=9, W=9, C=64, act="lrelu")
S(TN.test_bn_act_layer_vs_float64, N=2, H=5, W=7, C=256, act="lrelu")
S(TO.test_batchnorm_statistics_from_the_producers, n=2, c=128, h=32)
S(TI.test_instance_layer_vs_float64, **dict(zip(("kind", "N", "C", "R", "fm", "over", "half", "path"), TI.LAYER_CASES[5])))
S(TI.test_instance_layer_vs_float64, **dict(zip(("kind", "N", "C", "R", "fm", "over", "half", "path"), TI.LAYER_CASES[7])))
S(TI.test_instance_layer_vs_float64, **dict(zip(("kind", "N", "C", "R", "fm", "over", "half", "path"), TI.LAYER_CASES[8])))
S(TI.test_instance_layer_vs_float64, **dict(zip(("kind", "N", "C", "R", "fm", "over", "half", "path"), TI.LAYER_CASES[10])))
S(TO.test_syncbn_kernels_two_shards_match_reference_dp_branch)

# ---------------------------------------------------------------------------------------------- small kernels
S(TO.test_pools)
S(TQ.test_avgpool3s2_rect, h=17, w=12)
S(TQ.test_maxpool2_rect)
S(TQ.test_upnoise_rect, c=16, h=5, w=7)
S(TO.test_upsample_noise_and_sumpool)
S(TO.test_style_pool_fwd_bwd)
S(TQ.test_style_pool_rect, lh=32, lw=64, fh=16, fw=32)
S(TQ.test_onehot_conv3x3_fwd, name="plain_12x20", relu=0)
S(TQ.test_onehot_conv3x3_fwd, name="lds_46x50", relu=1)
S(TQ.test_onehot_conv3x3_wgrad, name="plain_12x20", nl=19)
S(TQ.test_onehot_conv3x3_wgrad, name="lds_46x50", nl=27)
S(TQ.test_dinput_rect)
S(TQ.test_layout_round_trip_rect)
S(TQ.test_bicubic_down_rect_source)
S(TR.test_forward_explicit_field_vs_float64, shape=(2, 8, 8, 19, 8), bias=True)
S(TR.test_forward_explicit_field_vs_float64, shape=(1, 5, 7, 19, 32), bias=False)
S(TR.test_wgrad_explicit_field_vs_float64, shape=(2, 8, 8, 19, 8))
S(TR.test_wgrad_explicit_field_vs_float64, shape=(1, 5, 7, 19, 32))
S(TR.test_philox_field_equals_rng_fill, shape=(1, 5, 7, 19, 32), offset=7, steps=2)
S(TO.test_preprocess_bicubic_labels_dinput)
S(TO.test_losses)
S(TO.test_loss_backward_honours_the_upstream_gradient)
S(TG.test_new_modes_vs_float64, shape=(4, 9, 9, 1), valid_c=1, lo=0, hi=2)
S(TG.test_new_modes_vs_float64, shape=(6, 5, 7, 4), valid_c=1, lo=3, hi=6)
S(TO.test_spectral_norm_fwd_bwd_and_buffers)
S(TO.test_device_input_pipeline_kernels_bit_exact)
S(TO.test_flat_adam_matches_torch_adam_incl_skipped_tensors_and_lr_change)
S(TO.test_rng_statistics)
S(TO.test_conv_noise_fused_in_output_transform_rect)
S(TO.test_resblock_fused_noise_shortcut_and_gradient_sink, kind="spade", ups=1)

# ---------------------------------------------------------------------------------------------- class counts 1 and 32
# the two ends of the class count, where 9 L + 1 rows and slots x L x Cs floats size the workspaces, the LDS table of the one-hot
# convolution is smallest / 144 KB, and the 32-column tables have no zero column: the smallest shape of each body
for _l in (1, 32):
    S(TK.test_onehot_conv3x3_fwd, shape="global_16x16", nl=_l, kind="uniform", co=128)
    S(TK.test_onehot_conv3x3_fwd, shape="lds_46x46", nl=_l, kind="uniform", co=128)
    S(TK.test_onehot_conv3x3_fwd, shape="lds4_64x64", nl=_l, kind="uniform", co=128)
    S(TK.test_onehot_conv3x3_wgrad, shape="23x41", nl=_l, kind="uniform", ld=160)
    S(TK.test_label_gather_and_segsum, shape="20x28", nl=_l, kind="uniform", cs=4)
    S(TK.test_label_gather_and_segsum, shape="32x64s2", nl=_l, kind="uniform", cs=256)
    S(TK.test_style_pool_fwd_bwd, nl=_l, kind="uniform")
    S(TK.test_label_onehot, nl=_l, coff=128, pad=0)
    S(TK.test_dinput_fwd_bwd, nl=_l)
    S(TK.test_onehot_noise_conv3x3, shape=(2, 20, 40, _l, 32))
    S(TK.test_style_table_layout_fwd_bwd, nl=_l)
    S(TK.test_style_explore, nl=_l, flags=5)
    S(TK.test_spade_sean_norm_direct_path, nl=_l, kind="uniform")
    S(TK.test_sean_norm_table_path, nl=_l, kind="uniform", R=16)
S(TK.test_onehot_conv3x3_fwd, shape="global_16x16", nl=32, kind="uniform", co=48)
S(TK.test_onehot_noise_conv3x3_widest_at_32_classes)

# ---------------------------------------------------------------------------------------------- metrics, visuals, loader, explore
S(TO.test_psnr_ssim_rmse_kernel_matches_reference_numbers)
S(TS.test_ms_ssim_smallest_size_and_batch_order)
S(TV.test_image_to_u8_is_bit_identical_to_numpy, layout="nhwc", normalize=True, window="ragged")
S(TV.test_image_to_u8_is_bit_identical_to_numpy, layout="nchw", normalize=False, window="aligned")
S(TV.test_label_colorize_matches_fixture_and_blacks_out_of_range, window="ragged")
S(TV.test_bilinear_up_u8_matches_the_stated_formula, window="ragged")
S(TV.test_bicubic_up_matches_interpolate, name="5to12")
for _n in ("resize_23x17_bicubic", "resize_23x17_bilinear", "label_7x13_to_5x9"):
    S(TL.test_resample_u8_equals_the_reference_pixels, name=_n)
S(TL.test_interp_down_against_the_reference_and_float64, name="12x20_to_4")
S(TE.test_style_explore_equals_the_torch_rule, f=TE.FLAGS[3])
S(TE.test_style_explore_equals_the_torch_rule, f=TE.FLAGS[4])
S(TE.test_nhwc_to_nchw_tiled_equals_permute_and_cat, shape=(2, 3, 5, 6, 4), shift=1, merge=True)
S(TE.test_nhwc_to_nchw_tiled_equals_permute_and_cat, shape=(2, 3, 5, 6, 4), shift=1, merge=False)

# ---------------------------------------------------------------------------------------------- coarse entry points
S(TO.test_coarse_sean_norm_fwd_is_the_autograd_path, kind="sean")
S(TO.test_coarse_spade_resblock_fwd_matches_the_module)
S(TO.test_coarse_resblock_training_pair, kind="sean")


# ---------------------------------------------------------------------------------------------- the other side of plan switches
S(TC.test_thin_conv3x3, _plan=dict(thin_gemm=False), n=1, cin=512, cout=2, h=16, w=16, act=1, use_bias=False)
S(TC.test_thin_conv3x3, _plan=dict(thin_gemm=False), n=2, cin=256, cout=3, h=8, w=64, act=3, use_bias=True)
S(TC.test_winograd_conv_autograd_function, _plan=dict(gemm_af32=False), n=2, cin=128, cout=256, h=32, act=1, use_res=True)
S(TO.test_sean_norm_table_path, _plan=dict(fused_norm=False), kind="sean", C=64, R=64, N=2, max_fm=256)
S(TC.test_spade_fused_forward_vs_float64, n=2, h=32, c=64, per_image=True, with_scale=True, packed=False, waves=4)
S(TI.test_instance_layer_vs_float64, **dict(zip(("kind", "N", "C", "R", "fm", "over", "half", "path"), TI.LAYER_CASES[0])))
S(TI.test_instance_layer_vs_float64, **dict(zip(("kind", "N", "C", "R", "fm", "over", "half", "path"), TI.LAYER_CASES[3])))


# ---------------------------------------------------------------------------------------------- entry points without a caller
# Forms of the ABI that deepsee_amd itself no longer calls (it takes their *_amax / *_range / two-call siblings): run next to the
# sibling the body exercises, on the same operands, and held bit-identical to it -- the sibling is what the body's own
# float64 / oracle assertions check.
def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# exercised entry point -> (plain form, positions dropped from the argument list, positions of the tensors it writes)
TWINS = {"conv2d_fwd_amax": ("conv2d_fwd", (9,), (6,)),
         "conv2d_fwd_f16x2_amax": ("conv2d_fwd_f16x2", (11, 12), (6,)),          # (flags = 0 only)
         "norm_act_fwd_amax": ("norm_act_fwd", (10,), (3,)),
         "norm_act_bwd_amax": ("norm_act_bwd", (13,), (5,)),
         "build_d_input_amax": ("build_d_input", (7,), (2,)),
         "adam_step_range": ("adam_step", (6,), (0, 2, 3, 4))}                  # (first_block = 0 only)


@contextlib.contextmanager
def twin_calls():
    from deepsee_amd import lib as L, ops
    inner = L.call
    seen, reduce_ = set(), {}

    def call(name, *a):
        if name == "modulate_bwd_reduce":      # (dh, h, x, scale, mean, invstd, dgb, dgb_ld, sums, N, HW, C, slope, workspace)
            dgb0 = a[6].clone()
            inner(name, *a)
            reduce_.update(args=a, dgb0=dgb0, dgb=a[6].clone(), sums=a[8].clone())
            return
        if (name in ("modulate_bwd_apply", "modulate_bwd_apply_amax") and reduce_ and a[1] is not None
                and reduce_["args"][0].data_ptr() == a[0].data_ptr() and (len(a) == 14 or (a[15] == 0 and a[16] is None))):
            # (dh, h, x, scale, mean, invstd, sums, add, dx, N, HW, C, inv_count, slope[, amax_dx, scale_f16, sign_mask]);
            # dsee_modulate_bwd is the pair in one call
            r = reduce_["args"]
            n, hw, c = a[9], a[10], a[11]
            if abs(a[12] * n * hw - 1.0) < 1e-6:                       # (not a SyncBN shard: the sums are this call's own)
                dx2, dgb2 = a[8].clone(), reduce_["dgb0"]
                cs2 = torch.full((2, c), float("nan"), device="cuda")
                ws = ops.scratch(L.lib().dsee_norm_workspace(n, hw, c, 1), "norm")
                inner(name, *a)
                inner("modulate_bwd", *a[:6], a[7], dx2, dgb2, r[7], cs2, n, hw, c, a[13], ws)
                assert _bits_equal(dx2, a[8]) and _bits_equal(dgb2, reduce_["dgb"]), "dsee_modulate_bwd != reduce + apply"
                assert _bits_equal(cs2.view(-1), reduce_["sums"].view(-1)[2 * c:4 * c]), "dsee_modulate_bwd: col_sums"
                reduce_.clear()
                seen.add("modulate_bwd")
                return
        if name not in TWINS or (name == "conv2d_fwd_f16x2_amax" and a[12] != 0) or (name == "adam_step_range" and a[6] != 0):
            return inner(name, *a)
        plain, drop, outs = TWINS[name]
        before = {i: a[i].clone() for i in outs}
        inner(name, *a)
        inner(plain, *[before.get(i, v) for i, v in enumerate(a) if i not in drop])
        for i in outs:
            assert _bits_equal(before[i], a[i]), "dsee_%s and dsee_%s differ in argument %d" % (plain, name, i)
        seen.add(plain)

    L.call = call
    try:
        yield seen
        assert seen, "no entry point with a twin was called"
    finally:
        L.call = inner


S(TC.test_conv_fwd_dgrad_wgrad, _twins=True, case=_conv_case(2, 22, 32, 17), f16x2=False)
S(TC.test_conv_fwd_dgrad_wgrad, _twins=True, case=_conv_case(2, 22, 32, 17), f16x2=True)
S(TC.test_conv_fwd_dgrad_wgrad, _twins=True, case=_conv_case(1, 64, 192, 12), f16x2=False)
S(TC.test_conv_fwd_dgrad_wgrad, _twins=True, case=_conv_case(8, 3, 64, 50), f16x2=True)
S(TO.test_instnorm_act, _twins=True, act=1)
S(TO.test_instnorm_act, _twins=True, act=3)
S(TQ.test_dinput_rect, _twins=True)
S(TO.test_flat_adam_matches_torch_adam_incl_skipped_tensors_and_lr_change, _twins=True)
S(TO.test_spade_sean_norm_fwd_bwd, _twins=True, kind="spade", C=8, R=8, N=2)
S(TO.test_spade_sean_norm_fwd_bwd, _twins=True, kind="sean", C=64, R=(8, 16), N=2)


def axpby_vs_float64():
    """dsee_axpby: y = alpha a + beta b, at sizes that are no multiple of a wave or a block.  Two roundings at the most (one with a
    fused multiply-add): |y - ref| <= 2^-22 (|alpha a| + |beta b|)."""
    from deepsee_amd import lib as L
    g = torch.Generator().manual_seed(3)
    for n in (4, 12, 1020, 4100, 65536 + 12):        # (n % 4 == 0 is the entry point's contract)
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
        y = torch.full((n,), float("nan"), device="cuda")
        L.call("axpby", a.cuda(), 0.75, b.cuda(), -1.3, y, n)
        ref = 0.75 * a.double() + float(torch.tensor(-1.3, dtype=torch.float32)) * b.double()
        bound = 2.0 ** -22 * (0.75 * a.double().abs() + 1.3 * b.double().abs()) + 1e-30
        assert bool(((y.cpu().double() - ref).abs() <= bound).all()), (n, float((y.cpu().double() - ref).abs().max()))


def act_fwd_vs_float64():
    """dsee_act_fwd (ops.Act) at odd sizes: LeakyReLU / ReLU are one fp32 product at the most (2^-23 relative), tanh is held to the
    suite's 2e-5 of the activations that follow a convolution (tests/test_gpu_conv.py), absolute: its values are O(1)."""
    import torch.nn.functional as F
    from deepsee_amd import lib as L, ops
    g = torch.Generator().manual_seed(4)
    for shape in ((1, 3, 5, 4), (2, 7, 9, 12), (3, 33, 31, 20)):
        x = torch.randn(shape, generator=g) * 2
        slope = float(torch.tensor(ops.LRELU_SLOPE, dtype=torch.float32))
        for act, ref, tol in ((L.ACT_LRELU, F.leaky_relu(x.double(), slope), 2.0 ** -23), (L.ACT_RELU, F.relu(x.double()), 0.0)):
            y = ops.Act.apply(x.cuda(), act).cpu().double()
            assert bool(((y - ref).abs() <= tol * ref.abs()).all()), (shape, act, float((y - ref).abs().max()))
        y = ops.Act.apply(x.cuda(), L.ACT_TANH).cpu().double()
        assert float((y - torch.tanh(x.double())).abs().max()) <= 2e-5, shape


def gemm_bf16x3_tn_vs_float64():
    """dsee_gemm_bf16x3_tn on the transposed bf16x3 operands dsee_wino43_dout_split_t / dsee_wino43_input_split_t write (the
    operand form of dsee_wino43_wgrad split = 1): C[g * splits + s] = dM[g, tiles of s]^T V[g, tiles of s] against float64 on the
    fp32 transforms dsee_wino43_dout / dsee_wino43_input of the same tensors, at test_gemm_bf16x3_is_fp32_accurate's 5e-7; a
    ragged 160-column Q and both tile shapes."""
    from deepsee_amd import lib as L
    g = torch.Generator().manual_seed(6)
    for n, h, w, cin, cout, splits in ((2, 16, 16, 32, 128, 2), (1, 16, 32, 160, 256, 1)):
        t = n * (h // 4) * (w // 4)
        x, dy = torch.randn(n, h, w, cin, generator=g).cuda(), torch.randn(n, h, w, cout, generator=g).cuda()
        v, dm = torch.empty(36, t, cin, device="cuda"), torch.empty(36, t, cout, device="cuda")
        L.call("wino43_input", x, v, n, h, w, cin, None)
        L.call("wino43_dout", dy, dm, n, h, w, cout, None)
        v3 = torch.empty(36 * t * cin * 3, dtype=torch.int16, device="cuda")
        dm3 = torch.empty(36 * t * cout * 3, dtype=torch.int16, device="cuda")
        L.call("wino43_input_split_t", x, v3, n, h, w, cin)
        L.call("wino43_dout_split_t", dy, dm3, n, h, w, cout)
        c = torch.full((36 * splits, cout, cin), float("nan"), device="cuda")
        L.call("gemm_bf16x3_tn", dm3, v3, c, 36, t, cout, cin, cin, splits)
        torch.cuda.synchronize()
        ts = t // splits
        ref = torch.einsum("ztp,ztq->zpq", dm.cpu().double().view(36 * splits, ts, cout), v.cpu().double().view(36 * splits, ts, cin))
        err = float((c.cpu().double() - ref).norm() / ref.norm())
        print("gemm_bf16x3_tn T=%d %dx%d splits=%d: %.2e" % (t, cout, cin, splits, err))
        assert err < 5e-7, err


def half_mode_producer_statistics():
    """tests/test_gpu_ops.py::test_batchnorm_statistics_from_the_producers' Winograd leg in the 16-bit storage mode
    (dsee_wino43_output_stats_f16: the product M arrives as scaled fp16): the statistics rows against float64 statistics of the
    tensor the kernel stored, at the same 2e-6, and the same values with and without the rows."""
    from deepsee_amd import ops
    n, c, h, wdt = 8, 128, 16, 32                     # 256 tiles: whole 256-row GEMM tiles
    g = TO.gen(n * c + h)
    x = (torch.randn(n, c, h, wdt, generator=g) * 2 + torch.randn(1, c, 1, 1, generator=g) * 3)
    nw = torch.randn(c, generator=g).cuda()
    w = (torch.randn(c, c, 3, 3, generator=g) / (c * 9) ** 0.5).cuda()
    b = torch.randn(c, generator=g).cuda()
    eps = ops.PhiloxNormal((n, h, wdt, c), 99, 777)

    def make(st):
        xs = TO.nhwc(x)
        ops.tag_amax(xs, ops.tensor_amax(xs))
        return ops.conv2d(xs, w, b, noise=(nw, eps), stats=st)
    with ops.KernelPlan(half=True).active():
        y, plain = make(True), make(False)
        assert getattr(y, "dsee_stats_rows", None) is not None and getattr(plain, "dsee_stats_rows", None) is None
        assert torch.equal(y, plain)
        rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        mean, inv, _ = ops.bn_stats(y, rm, rv, True)
    torch.cuda.synchronize()
    y64 = y.double().reshape(-1, c)
    mu, var = y64.mean(0), y64.var(0, unbiased=False)
    ref_inv = 1.0 / torch.sqrt(var + ops.BN_EPS)
    assert float((mean.double() - mu).abs().max() / mu.abs().max()) < 2e-6
    assert float(((inv.double() - ref_inv) / ref_inv).abs().max()) < 2e-6


S(axpby_vs_float64)
S(act_fwd_vs_float64)
S(gemm_bf16x3_tn_vs_float64)
S(half_mode_producer_statistics)


# ---------------------------------------------------------------------------------------------- whole steps (eager: a replayed
# oracle tape never takes the captured-graph path, managers.TrainerManager._graphed)
def half_step_vs_oracle():
    """indep_4to32_bs2_ngf8 in the 16-bit mode, one eager G+D step against the fp32 CPU oracle at the forward bounds of
    test_gpu_model.py::test_half_mode_vs_oracle (image 3e-2, losses 5 %)."""
    from deepsee_amd import networks as N
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    over = TM.CASES["indep_4to32_ngf8"]
    oopt = O.make_opt(**over)
    states = O.recipe_state(oopt, gain=1.0)
    batch = O.synthetic_batch(oopt, 2, seed=31)
    ctl = O.RecordingCtl()
    orc = O.Oracle(oopt, states, ctl)
    orc.create_optimizers()
    random.seed(31)
    torch.manual_seed(31)
    gl, fake = orc.run_generator_one_step({k: v.clone() for k, v in batch.items()})
    dl = orc.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
    tm = TrainerManager(make_opt(precision="fp16", hip_graphs=False, **over))
    assert tm.sr_model.plan.half
    tm.sr_model.load_states(states)
    tm.sr_model.noise = N.ReplayNoise(ctl.tape)
    tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
    tm.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
    torch.cuda.synchronize()
    got = {k: float(v) for k, v in tm.get_latest_losses().items()}
    dev = TM.rel(tm.get_latest_generated().detach().cpu(), fake.detach())
    print("fp16 step vs the oracle: |fake| deviation %.2e, losses %s" % (dev, got))
    assert dev < 3e-2, dev
    for k, v in gl.items():
        assert abs(got[k] - float(v.detach())) <= 0.05 * abs(float(v.detach())) + 1e-3, (k, got[k], float(v.detach()))
    for k, v in dl.items():
        assert got[k] == got[k] and abs(got[k]) < 1e4, (k, got[k])


for _n in ("indep_4to32_ngf8", "guided_4to32_ngf8", "puresean_4to128_ngf4"):
    S(TM.test_train_step_matches_oracle, name=_n)
S(half_step_vs_oracle)
S(TI.test_instance_train_step_matches_oracle)
S(TN.test_nonspade_train_step_matches_oracle, name="indep_dbatch_ebatch_4to32_bs2_ngf8")
S(TR.test_random_style_train_step_matches_oracle, name=sorted(TR.GOLD_CASES)[0])
S(TM.test_inference_mode_matches_oracle)


def run_body(func, kwargs, monkeypatch, tmp_path, request):
    extra = {}
    for name in inspect.signature(func).parameters:
        if name not in kwargs:
            extra[name] = {"monkeypatch": monkeypatch, "tmp_path": tmp_path}.get(name) or request.getfixturevalue(name)
    return func(**kwargs, **extra)


@pytest.mark.parametrize("func,kwargs,how", SCENARIOS)
def test_guarded(func, kwargs, how, monkeypatch, tmp_path, request):
    from deepsee_amd import plan as PL
    t0 = time.time()
    with contextlib.ExitStack() as stack:
        rz = stack.enter_context(redzone.guarded())
        if how["twins"]:
            stack.enter_context(twin_calls())
        if how["plan"]:
            stack.enter_context(PL.DEFAULT_PLAN.replace(**how["plan"]).active())
        run_body(func, kwargs, monkeypatch, tmp_path, request)
    print("guarded %s: %.2f s, %d calls in arenas, entry points %s, pass-through %s"
          % (request.node.callspec.id, time.time() - t0, rz.calls, sorted(rz.guarded), rz.passthrough))
    assert rz.calls + sum(rz.passthrough.values()) > 0, "the body made no call through lib.call"
    assert set(rz.passthrough) <= set(redzone.ALLOWLIST)


# ---------------------------------------------------------------------------------------------- coverage condition
# entry points that take a pointer and need not run guarded here, each with its reason
EXEMPT = {
    "comm_unique_id": "RCCL bootstrap (host memory)", "comm_init": "RCCL bootstrap (host memory)",
    "comm_world": "communicator query", "comm_rank": "communicator query", "comm_destroy": "communicator teardown",
    "comm_allreduce_sum": "multi-rank collective", "comm_broadcast": "multi-rank collective",
    "comm_allgather": "multi-rank collective",
    "conv2d_wgrad_workspace": "pure query (host geometry struct)",
    "conv2d_wgrad_table_workspace": "pure query (host geometry struct)",
    "rng_set_epoch": "registers the address of the device-side epoch counter, touches no memory",
}


def test_every_device_pointer_entry_point_ran_guarded(request):
    import ctypes as C
    from deepsee_amd import lib as L
    mine = [i for i in request.session.items if i.module is request.module]
    if len(mine) != len(SCENARIOS) + 1:
        pytest.skip("only part of this module was selected")
    protos = L.header_prototypes()
    hdr = re.sub(r"/\*.*?\*/", "", open(L.HEADER_PATH).read(), flags=re.S)
    streamed = set(re.findall(r"\b(dsee_[a-z0-9_]+)\s*\([^)]*hipStream_t", hdr))
    needs = {n[5:] for n, (_, args) in protos.items() if sum(a is C.c_void_p for a in args) > (n in streamed)}
    ran = redzone.RECORD["guarded"] | set(redzone.RECORD["passthrough"])
    missing = sorted(needs - ran - set(EXEMPT))
    print("guarded entry points: %d of %d that take a pointer; %d calls in arenas; pass-through %s"
          % (len(needs & ran), len(needs), redzone.RECORD["calls"], redzone.RECORD["passthrough"]))
    # every entry point with a *_workspace function, without exception
    with_ws = set()
    for q in protos:
        if "_workspace" in q:
            base = q.replace("_workspace", "")[5:]
            if "dsee_" + base in protos:
                with_ws.add(base)
    assert not sorted(with_ws - redzone.RECORD["guarded"]), sorted(with_ws - redzone.RECORD["guarded"])
    assert not missing, "entry points that never ran guarded: %s" % missing
    assert set(redzone.RECORD["passthrough"]) <= set(redzone.ALLOWLIST)
    stale = sorted(set(EXEMPT) & redzone.RECORD["guarded"])
    assert not stale, "EXEMPT names entry points that did run guarded: %s" % stale
