"""InstanceNorm SPADE / SEAN / PureSEAN (opt.norm_G = ...instance3x3) on the MI355X: every layer path (fused, chunked
Winograd, direct, dense, capped) against float64, per-image independence, the G+D step / inference modes against the
InstanceNorm form of the oracle (tools/gen_golden_instance.py; pinned to the reference by tests/test_instance_norm_host.py),
replayed graphs, the 16-bit mode and the checkpoint layout."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import deepsee_oracle as O
from tools.gen_golden_instance import install_instance_norm

pytestmark = pytest.mark.gpu

INST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance")
NORM_G = "spectrallateseaninstance3x3"
# the geometry of tests/golden/instance/indep_instance_4to32_bs2_ngf8.json
STEP = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8, norm_G=NORM_G)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-20))


def nhwc(x):
    from deepsee_amd import ops
    return ops.to_nhwc(x.cuda())


def nchw(x, c):
    from deepsee_amd import ops
    return ops.to_nchw(x.contiguous(), c).cpu()


def _layer_inputs(kind, N, C, R, seed):
    """Labels, style and an input whose images have clearly different statistics (x[n] = (1 + 3n) x[n] + 2n): BatchNorm
    statistics would be off by O(1)."""
    from deepsee_amd import ops
    g = torch.Generator().manual_seed(seed)
    Lc, S = 19, 128
    label = F.interpolate(torch.randint(0, Lc, (N, 1, 8, 8), generator=g).float(), size=(R, R), mode="nearest")
    style = torch.rand(N, Lc, S, generator=g) * 2 - 1
    k = torch.arange(N, dtype=torch.float32).view(N, 1, 1, 1)
    x = torch.randn(N, C, R, R, generator=g) * (1 + 3 * k) + 2 * k
    gy = torch.randn(N, C, R, R, generator=g)
    return label, style, x, gy, ops.Labels(ops.label_to_u8(label.cuda()), Lc)


def _instance_layer(kind, C, fm):
    from deepsee_amd import networks as Nw
    mod = Nw.SpadeNorm(kind, C, 19, 128, fm, norm="instance")
    assert mod.param_free_norm is None and not any("param_free_norm" in k for k in mod.state_dict())
    st = {"n." + k: O.recipe_tensor("in_" + kind, k, v.shape, 1.0) for k, v in mod.state_dict().items()}
    mod.load_state_dict({k[2:]: v for k, v in st.items()})
    return mod.cuda(), st


def _run_layer(mod, x, style, gy, labels, C, plan, calls=None):
    """Forward + backward of one layer under `plan`; `calls` (a list) receives the C-ABI entry points the layer invoked."""
    from deepsee_amd import lib as L
    call = L.call

    def spy(name, *a):
        calls.append(name)
        return call(name, *a)
    xs = nhwc(x).requires_grad_()
    sty = style.cuda().requires_grad_()
    mod.zero_grad(set_to_none=True)
    if calls is not None:
        L.call = spy
    try:
        with plan.active():
            h = mod(xs, labels, sty, True)
            g = nhwc(gy)
            if plan.half:
                from deepsee_amd import ops
                ops.tag_amax(g, ops.tensor_amax(g))
            h.backward(g)
    finally:
        L.call = call
    torch.cuda.synchronize()
    return (nchw(h.detach(), C), nchw(xs.grad, C), None if sty.grad is None else sty.grad.cpu(),
            {k: p.grad.cpu() for k, p in mod.named_parameters() if p.grad is not None})


# (kind, N, C, R, max_fm_size, plan overrides, half, the forward entry point the layer must take):
#   spade_fused_fwd[_f16p]_sg    the fused kernel (64 tiles of one image per block), also the capped SPADE/PureSEAN path
#   wino43_output_modulate_sg    the chunked Winograd path (fused_norm off; PureSEAN's 32-channel one-hot operand)
#   conv2d_modulate_fwd_sg       the direct GEMM (SPADE below 16^2) and the dense path (SEAN below 16^2, SEAN capped, C % 64 != 0)
LAYER_CASES = [
    ("sean", 3, 128, 64, 256, {}, False, "spade_fused_fwd_sg"),
    ("spade", 3, 128, 64, 256, {}, False, "spade_fused_fwd_sg"),
    ("puresean", 3, 128, 64, 256, {}, False, "wino43_output_modulate_sg"),
    ("sean", 3, 128, 64, 256, dict(fused_norm=False), False, "wino43_output_modulate_sg"),
    ("spade", 3, 128, 64, 256, dict(fused_norm=False), False, "wino43_output_modulate_sg"),
    ("spade", 2, 64, 8, 256, {}, False, "conv2d_modulate_fwd_sg"),
    ("sean", 2, 64, 8, 256, {}, False, "conv2d_modulate_fwd_sg"),
    ("puresean", 2, 64, 32, 16, {}, False, "spade_fused_fwd_sg"),
    ("sean", 2, 32, 16, 8, {}, False, "conv2d_modulate_fwd_sg"),
    ("sean", 3, 128, 64, 256, {}, True, "spade_fused_fwd_f16p_sg"),
    ("puresean", 2, 64, 32, 16, {}, True, "spade_fused_fwd_f16p_sg"),
]
# entry points that take BatchNorm statistics only: an InstanceNorm layer must not reach them
BN_ONLY = {"spade_fused_fwd", "spade_fused_fwd_f16p", "spade_fused_fwd_w4", "wino43_output_modulate", "conv2d_modulate_fwd",
           "modulate_bwd_reduce", "modulate_bwd_reduce_wino", "modulate_bwd_reduce_wino_f16x2", "modulate_bwd_reduce_wino_f16p",
           "modulate_bwd_apply", "modulate_bwd_apply_amax", "norm_eval_stats", "norm_stats_finalize_parts"}


@pytest.mark.parametrize("kind,N,C,R,fm,over,half,path", LAYER_CASES)
def test_instance_layer_vs_float64(kind, N, C, R, fm, over, half, path, monkeypatch):
    """The method of test_gpu_ops.py::test_benchmark_shape_norm_vs_float64 with InstanceNorm: float64 oracle layer, its
    LeakyReLU decisions taken from the HIP output.  fp32: forward < 1e-4, every gradient < 1e-3; 16-bit mode: 2e-3 / 8e-3."""
    from deepsee_amd import ops
    install_instance_norm(monkeypatch.setattr)
    label, style, x, gy, labels = _layer_inputs(kind, N, C, R, 7 + C + R)
    mod, st = _instance_layer(kind, C, fm)
    plan = ops.KernelPlan(half=half, **over)
    calls = []
    h, dx, dsty, grads = _run_layer(mod, x, style, gy, labels, C, plan, calls)
    assert path in calls and "modulate_bwd_apply_amax_sg" in calls and not BN_ONLY & set(calls), sorted(set(calls))
    orc = O.Oracle(O.make_opt(max_fm_size=fm), {"SR": st}, dtype=torch.float64)
    P = orc.S["SR"]
    x6, s6 = x.double().requires_grad_(), style.double().requires_grad_()
    pre = orc._norm(kind, P, "n", x6, O.onehot_labels(label, 19).double(), s6)
    torch.where(h > 0, pre, 0.2 * pre).backward(gy.double())
    errs = {"dx": rel(dx, x6.grad)}
    if kind != "spade" and fm >= R:      # (above max_fm_size the style matrix is ignored: no gradient on either side)
        errs["dstyle"] = rel(dsty, s6.grad)
    for k, gr in grads.items():
        if P["n." + k].grad is not None:
            errs[k] = rel(gr, P["n." + k].grad)
    fwd = rel(h, F.leaky_relu(pre.detach(), 0.2))
    worst = max(errs, key=errs.get)
    print("%s N=%d C=%d %d^2 fm %d %s%s: forward %.1e, gradients worst %.1e (%s)"
          % (kind, N, C, R, fm, over, " 16-bit" if half else "", fwd, errs[worst], worst))
    fb, gb = (2e-3, 8e-3) if half else (1e-4, 1e-3)
    assert fwd < fb and errs[worst] < gb, (fwd, errs)


@pytest.mark.parametrize("kind,N,C,R,fm", [("sean", 3, 128, 64, 256), ("spade", 2, 64, 8, 256), ("puresean", 2, 64, 32, 16),
                                         ("sean", 8, 512, 256, 256), ("spade", 8, 512, 256, 256)])
def test_instance_layer_images_are_independent(kind, N, C, R, fm):
    """Image k of a batch gives the output and dx of the same layer run on image k alone -- also at the benchmark's layer
    geometry (N = 8 images of 256^2 x 512 channels: 8 statistics groups of 256 reduce blocks each)."""
    from deepsee_amd import ops
    label, style, x, gy, labels = _layer_inputs(kind, N, C, R, 3 + C)
    mod, _ = _instance_layer(kind, C, fm)
    h, dx, _, _ = _run_layer(mod, x, style, gy, labels, C, ops.KernelPlan())
    for k in range(N):
        lab1 = ops.Labels(ops.label_to_u8(label[k:k + 1].cuda()), 19)
        h1, dx1, _, _ = _run_layer(mod, x[k:k + 1], style[k:k + 1], gy[k:k + 1], lab1, C, ops.KernelPlan())
        # an output within rounding of zero may take the other LeakyReLU branch in the two runs (at 8 x 512 x 256^2 a handful of
        # the 268M elements do): dx is compared where both runs took the same branch, the branch flips are counted
        same = (h[k:k + 1] > 0) == (h1 > 0)
        flips = 1.0 - float(same.double().mean())
        e_h, e_dx = rel(h[k:k + 1], h1), rel(dx[k:k + 1][same], dx1[same])
        assert e_h <= 1e-5 and e_dx <= 1e-5 and flips <= 1e-6, (k, e_h, e_dx, flips)


def test_instance_train_step_matches_oracle(monkeypatch):
    """G+D step (tape replay, D step from the oracle's post-G state) of the InstanceNorm generator against the
    InstanceNorm oracle: test_gpu_model.py::test_train_step_matches_oracle's bounds and post-step state checks."""
    from tests import test_gpu_model as TGM
    install_instance_norm(monkeypatch.setattr)
    monkeypatch.setitem(TGM.CASES, "instance_4to32_ngf8", STEP)
    TGM.test_train_step_matches_oracle("instance_4to32_ngf8")


def test_instance_inference_modes_match_oracle(monkeypatch):
    """inference / encode_only / demo in eval mode: InstanceNorm normalises with the statistics of the batch there too."""
    from tests import test_gpu_model as TGM
    install_instance_norm(monkeypatch.setattr)
    monkeypatch.setitem(TGM.CASES, "indep_8to64_ngf8", dict(TGM.CASES["indep_8to64_ngf8"], norm_G=NORM_G))
    TGM.test_inference_mode_matches_oracle()


def _steps(over, n_steps, batch):
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    tm = TrainerManager(make_opt(**over))
    out = []
    for _ in range(n_steps):
        tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
        fake = tm.get_latest_generated().detach().cpu()
        tm.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
        out.append((fake, {k: float(v.detach()) for k, v in tm.get_latest_losses().items()}))
    torch.cuda.synchronize()
    return out


def test_instance_graphs_and_half_mode():
    """Two G+D steps replayed from captured graphs equal the same steps run eagerly; one 16-bit step stays within the 16-bit
    model bounds of test_gpu_model.py::test_half_mode_tracks_fp32 (image 3e-2, losses 5 %) of the fp32 InstanceNorm step."""
    over = dict(STEP, seed=11)
    batch = O.synthetic_batch(O.make_opt(**STEP), 2, seed=5)
    eager = _steps(dict(over, hip_graphs=False), 2, batch)
    graph = _steps(dict(over, hip_graphs=True), 2, batch)
    for (fe, le), (fg, lg) in zip(eager, graph):
        assert rel(fg, fe) <= 1e-6, rel(fg, fe)
        for k in le:
            assert abs(lg[k] - le[k]) <= 1e-5 * abs(le[k]) + 1e-7, (k, lg[k], le[k])
    half = _steps(dict(over, precision="fp16"), 1, batch)
    assert rel(half[0][0], eager[0][0]) < 3e-2, rel(half[0][0], eager[0][0])
    for k, v in eager[0][1].items():
        assert abs(half[0][1][k] - v) <= 0.05 * abs(v) + 0.05, (k, half[0][1][k], v)


def test_instance_checkpoint_roundtrip(tmp_path):
    """save / load_weights of an InstanceNorm model: SR keys = the reference InstanceNorm model's (fixture), no
    param_free_norm buffers, and the weights come back."""
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    rec = json.load(open(os.path.join(INST, "indep_instance_4to32_bs2_ngf8.json")))
    assert rec["opt"]["norm_G"] == NORM_G
    ref_keys = {k.split("/", 1)[1] for k in rec["iters"][0]["state_norms"] if k.startswith("SR/")}
    over = dict(STEP, checkpoints_dir=str(tmp_path), name="ck")
    tm = TrainerManager(make_opt(**over))
    tm.save("latest")
    ck = torch.load(str(tmp_path / "ck" / "latest_net_SR.pth"))
    assert set(ck["model"]) == ref_keys and not any("param_free_norm" in k for k in ck["model"])
    tm2 = TrainerManager(make_opt(**dict(over, continue_train=True, seed=5)))
    a, b = tm.sr_model.netSR.state_dict(), tm2.sr_model.netSR.state_dict()
    assert set(a) == set(b) == ref_keys
    assert all(torch.equal(a[k], b[k]) for k in a)
    # load_states (the oracle / recipe layout) takes the same key set
    states = O.recipe_state(O.make_opt(**STEP))
    states["SR"] = {k: v for k, v in states["SR"].items() if ".param_free_norm." not in k}
    tm2.sr_model.load_states(states)
