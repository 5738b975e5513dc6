"""The ablation generators (opt.netG) on the MI355X.

Layer level: the reflect-padded 3x3 convolution of ops.Conv2d (`reflect=True`: the zero-padded layer on its usual path + the border
pass dsee_reflect_ring_fwd / _dgrad / _wgrad) against float64 F.conv2d(F.pad(x, mode='reflect'), w) for y, dx and
dw -- the identity tests/test_ablation_host.py restates term by term -- in fp32 and under precision='fp16', once more with every
buffer fenced by tests/redzone.py; the argument checks; the InstanceNorm forward with a residual operand (dsee_norm_act_res_fwd).

Model level: one G + D step, inference / encode_only / demo of every fixture case of tests/golden/ablation against the substituted
oracle (tools/gen_golden_ablation.py; pinned to the reference by tests/test_ablation_host.py), replayed hipGraphs against eager
steps, and the 16-bit mode."""
import functools
import random

import pytest
import torch
import torch.nn.functional as F

import redzone      # (as tests/test_gpu_redzone.py imports it: one module, one RECORD of what ran guarded)
from oracle import deepsee_oracle as O
from tools.gen_golden_ablation import CASES as GOLD_CASES, install_ablation

pytestmark = pytest.mark.gpu


def rel(a, b):
    """the measure of tests/test_gpu_conv.py"""
    return float((a - b).norm() / b.norm().clamp_min(1e-20))


def nhwc(x):
    n, c, h, w = x.shape
    out = torch.zeros(n, h, w, (c + 3) // 4 * 4)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out.contiguous()


def nchw(x, c):
    return x[..., :c].permute(0, 3, 1, 2).contiguous()


# (N, Cin, Cout, H, W): the smallest shapes at which the border logic can go wrong
LAYER_SHAPES = [
    (1, 128, 128, 4, 4),      # rows 1 and H-2 adjacent, every border pixel next to a corner (direct path)
    (2, 64, 64, 8, 12),       # direct path, H != W, two 64-row tiles of border pixels
    (2, 128, 128, 32, 32),    # the Winograd path
    (2, 20, 36, 8, 8),        # channel counts that are no multiple of 32 (ragged K slab and ragged 64-column tile)
]


@functools.lru_cache(maxsize=None)
def layer_reference(n, cin, cout, h, w):
    """Inputs and the float64 y, dx, dw of conv3x3(reflect_pad(x), w); computed once per shape, shared, never modified."""
    g = torch.Generator().manual_seed(n * 1000 + cin + 7 * h + w)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    gy = torch.randn(n, cout, h, w, generator=g)
    xr, wr = x.double().requires_grad_(), wt.double().requires_grad_()
    y = F.conv2d(F.pad(xr, (1, 1, 1, 1), mode="reflect"), wr)
    dx, dw = torch.autograd.grad(y, (xr, wr), gy.double())
    return x, wt, gy, y.detach(), dx, dw


def run_layer(x, wt, gy):
    from deepsee_amd import ops
    xd, wd = nhwc(x).cuda().requires_grad_(), wt.cuda().requires_grad_()
    y = ops.conv2d(xd, wd, None, reflect=True)
    y.backward(nhwc(gy).cuda())
    torch.cuda.synchronize()
    return y.detach().cpu(), xd.grad.cpu(), wd.grad.cpu()


def layer_errors(shape, got):
    n, cin, cout, h, w = shape
    _, _, _, y, dx, dw = layer_reference(*shape)
    yd, dxd, dwd = got
    assert float(yd[..., cout:].abs().max() if yd.shape[-1] > cout else 0.0) == 0.0      # pad channels stay zero
    return {"y": rel(nchw(yd, cout).double(), y), "dx": rel(nchw(dxd, cin).double(), dx), "dw": rel(dwd.double(), dw)}


@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reflect_conv_vs_float64(shape):
    """y, dx, dw through the autograd node against float64, the 2e-5 bound of tests/test_gpu_conv.py; a second run is bitwise equal
    (the ring weight gradient folds its K splits in a fixed order); the same layer without `reflect` differs on the border only."""
    from deepsee_amd import ops
    n, cin, cout, h, w = shape
    assert ops._wino_ok(n, h, w, (cin + 3) // 4 * 4, (cout + 3) // 4 * 4, 3, 1, 1, 0) == (shape == (2, 128, 128, 32, 32))
    x, wt, gy = layer_reference(*shape)[:3]
    got = run_layer(x, wt, gy)
    errs = layer_errors(shape, got)
    print("reflect conv %s vs float64: %s" % (shape, {k: "%.2e" % v for k, v in errs.items()}))
    again = run_layer(x, wt, gy)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    xd, wd = nhwc(x).cuda(), wt.cuda()
    with torch.no_grad():
        zero = ops.conv2d(xd, wd, None).cpu()
    diff = (got[0] - zero).abs().amax(dim=(0, 3))
    assert float(diff[1:-1, 1:-1].max() if h > 2 and w > 2 else 0.0) == 0.0
    assert float(diff[0].min()) > 0 and float(diff[-1].min()) > 0 and float(diff[:, 0].min()) > 0 and float(diff[:, -1].min()) > 0
    assert errs["y"] < 2e-5 and errs["dx"] < 2e-5 and errs["dw"] < 2e-5, errs


@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reflect_conv_fp16_mode_vs_float64(shape):
    """The same layer under precision='fp16' (the zero-padded layer on one-term fp16 operands, the border pass unchanged in
    fp32) within the 8e-3 of test_gpu_conv.py::test_winograd_conv_16bit_storage_mode."""
    from deepsee_amd.options import make_opt
    from deepsee_amd.plan import from_opt
    plan = from_opt(make_opt(precision="fp16"))
    assert plan.half
    x, wt, gy = layer_reference(*shape)[:3]
    with plan.active():
        errs = layer_errors(shape, run_layer(x, wt, gy))
    print("reflect conv %s, fp16 mode, vs float64: %s" % (shape, {k: "%.2e" % v for k, v in errs.items()}))
    assert errs["y"] < 8e-3 and errs["dx"] < 8e-3 and errs["dw"] < 8e-3, errs


@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reflect_conv_guarded(shape):
    """Once with every buffer the three entry points touch between poisoned guard zones (tests/redzone.py): nothing written
    outside, no poison read back, the same bounds."""
    x, wt, gy = layer_reference(*shape)[:3]
    with redzone.guarded() as rz:
        got = run_layer(x, wt, gy)
    assert {"reflect_ring_fwd", "reflect_ring_dgrad", "reflect_ring_wgrad"} <= rz.guarded and not rz.passthrough
    errs = layer_errors(shape, got)
    assert errs["y"] < 2e-5 and errs["dx"] < 2e-5 and errs["dw"] < 2e-5, errs


@pytest.mark.parametrize("h,w", [(1, 8), (8, 1), (1, 1)])
def test_reflect_ring_refuses_one_pixel_wide_maps(h, w):
    """H < 2 or W < 2 (no pixel to reflect onto): DSEE_EINVAL with the error text set, nothing launched -- the in-place operands
    keep their bits."""
    from deepsee_amd import lib as L, ops
    c = 8
    x, y = torch.randn(2, h, w, c).cuda(), torch.randn(2, h, w, c).cuda()
    wt, dw = torch.randn(c, c, 3, 3).cuda(), torch.randn(c, c, 3, 3).cuda()
    y0, x0, dw0 = y.clone(), x.clone(), dw.clone()
    ws = ops.scratch(1 << 16, "ringw")
    for name, args in (("reflect_ring_fwd", (x, wt, y, 2, h, w, c, c, c, c)), ("reflect_ring_dgrad", (y, wt, x, 2, h, w, c, c, c, c)),
                       ("reflect_ring_wgrad", (x, y, ws, 1 << 16, dw, 2, h, w, c, c, c, c))):
        with pytest.raises(L.DseeError, match="reflection padding"):
            L.call(name, *args)
    assert L.lib().dsee_reflect_ring_wgrad_workspace(2, h, w, c, c) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and torch.equal(x, x0) and torch.equal(dw, dw0)
    # a stored channel count that is not the padded count, a NULL pointer
    x2, y2 = torch.randn(1, 4, 4, c).cuda(), torch.randn(1, 4, 4, c).cuda()
    with pytest.raises(L.DseeError, match="channel storage"):
        L.call("reflect_ring_fwd", x2, wt, y2, 1, 4, 4, c, c + 4, c, c)
    with pytest.raises(L.DseeError, match="NULL"):
        L.call("reflect_ring_fwd", x2, None, y2, 1, 4, 4, c, c, c, c)


@pytest.mark.parametrize("n,h,w,c,act", [(2, 8, 12, 64, "none"), (3, 5, 7, 20, "lrelu"), (2, 32, 32, 128, "none")])
def test_instance_norm_residual_vs_float64(n, h, w, c, act):
    """act(res + InstanceNorm(x)) forward, dx and dres against float64 (LeakyReLU branches taken from the HIP output, as
    tests/test_gpu_nonspade_norm.py does): bounds of that file's layer test, 1e-5 forward and 1e-4 backward."""
    from deepsee_amd import lib as L, ops
    g = torch.Generator().manual_seed(n * 100 + c + h)
    k = torch.arange(c, dtype=torch.float32)
    x = torch.randn(n, h, w, c, generator=g) * (0.5 + k / c) + k / c
    res, gy = torch.randn(n, h, w, c, generator=g), torch.randn(n, h, w, c, generator=g)
    a = L.ACT_LRELU if act == "lrelu" else L.ACT_NONE
    xd, rd = x.cuda().requires_grad_(), res.cuda().requires_grad_()
    y = ops.InstNormRes.apply(xd, rd, a)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    x6, r6 = x.double().permute(0, 3, 1, 2).requires_grad_(), res.double().permute(0, 3, 1, 2).requires_grad_()
    pre = F.instance_norm(x6, eps=1e-5) + r6
    y_hip = y.detach().cpu().permute(0, 3, 1, 2)
    ref = torch.where(y_hip > 0, pre, 0.2 * pre) if act == "lrelu" else pre
    ref.backward(gy.double().permute(0, 3, 1, 2))
    errs = {"y": rel(y_hip.double(), ref.detach()), "dx": rel(xd.grad.cpu().permute(0, 3, 1, 2).double(), x6.grad),
            "dres": rel(rd.grad.cpu().permute(0, 3, 1, 2).double(), r6.grad)}
    print("IN + residual N=%d %dx%d C=%d %s: %s" % (n, h, w, c, act, {k_: "%.1e" % v for k_, v in errs.items()}))
    assert errs["y"] < 1e-5 and errs["dx"] < 1e-4 and errs["dres"] < 1e-5, errs


def test_instance_norm_residual_guarded():
    """dsee_norm_act_res_fwd and the backward behind it with every buffer fenced (tests/redzone.py); same result as unfenced."""
    from deepsee_amd import lib as L, ops
    g = torch.Generator().manual_seed(5)
    x, res, gy = (torch.randn(3, 5, 7, 20, generator=g).cuda() for _ in range(3))

    def run():
        xd, rd = x.clone().requires_grad_(), res.clone().requires_grad_()
        y = ops.InstNormRes.apply(xd, rd, L.ACT_LRELU)
        y.backward(gy)
        torch.cuda.synchronize()
        return y.detach(), xd.grad, rd.grad
    plain = run()
    with redzone.guarded() as rz:
        fenced = run()
    assert "norm_act_res_fwd" in rz.guarded and not rz.passthrough
    assert all(torch.equal(a, b) for a, b in zip(plain, fenced))


# ------------------------------------------------------------------------------------ model level
def _case(name):
    return dict(GOLD_CASES[name]["opt"])


@pytest.mark.parametrize("name", sorted(GOLD_CASES))
def test_ablation_train_step_matches_oracle(name, monkeypatch):
    """G+D step (tape replay, D step from the oracle's post-G state) against the substituted oracle with the bounds and post-step
    state checks of test_gpu_model.py::test_train_step_matches_oracle.  A generator that ignores the style leaves the encoder
    without gradients (the reference: 12 of 12 netE parameters): those parameters come out of the step bit-unchanged."""
    from tests import test_gpu_model as TGM
    install_ablation(monkeypatch.setattr)
    monkeypatch.setitem(TGM.CASES, name, _case(name))
    captured = {}
    run_case = TGM.run_case

    def spy(*a, **kw):
        out = run_case(*a, **kw)
        captured["r"] = out
        return out
    monkeypatch.setattr(TGM, "run_case", spy)
    TGM.test_train_step_matches_oracle(name)
    orc, tm, out = captured["r"]
    r = out[0]
    kinds = {k for _, k in tm.sr_model._block_plan}
    # (nostyle_4to128_ngf4: its PureSEAN tail sits above max_fm_size, where the reference feeds the upsampled SPADE activation
    # in place of the style map, normalization.py:275-277 -- no encoder gradient there either)
    uses_style = _case(name)["netG"] == "puresean"
    assert uses_style == any(k.startswith("E.") for k in r["ggrads"])
    enc_touched = {k for k in r["touched_g"] if k.startswith("E.")}
    assert bool(enc_touched) == uses_style, (kinds, enc_touched)
    if not uses_style:
        start = O.recipe_state(O.make_opt(**_case(name)), gain=1.0)["E"]
        params = [k for k in start if not O.is_buffer(k)]
        assert len(params) == 12
        for k in params:
            assert torch.equal(r["post_g"]["E"][k], start[k]), k
    if _case(name)["netG"] == "nospadenostyle":
        assert kinds == {"resnet"} and len(tm.sr_model.netSR.state_dict()) == 4 + 6 * len(tm.sr_model._block_plan)


@pytest.mark.parametrize("name", ["nostyle_4to32_ngf8", "puresean_abl_4to32_ngf8", "nospadenostyle_8to64_ngf8"])
def test_ablation_inference_modes_match_oracle(name, monkeypatch):
    """inference / encode_only / demo against the substituted oracle, bounds of test_gpu_model.py::test_inference_mode_matches_oracle."""
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    install_ablation(monkeypatch.setattr)
    over = _case(name)
    oopt = O.make_opt(**over)
    states = O.recipe_state(oopt, gain=1.0)
    batch = O.synthetic_batch(oopt, 2, seed=77)
    orc = O.Oracle(oopt, states)
    want = orc.inference({k: v.clone() for k, v in batch.items()})
    tm = TrainerManager(make_opt(**over))
    tm.sr_model.load_states(states)
    tm.sr_model.eval()
    out = tm.sr_model(tm.preprocess_input({k: v.clone() for k, v in batch.items()}), mode="inference")
    assert rel(out["fake_image"].cpu(), want) < 1e-4
    pre = tm.preprocess_input({k: v.clone() for k, v in batch.items()})
    style = tm.sr_model(dict(pre), mode="encode_only")
    want_style = orc.encode_only({k: v.clone() for k, v in batch.items()})
    assert tuple(style.shape) == tuple(want_style.shape) and rel(style.detach().cpu(), want_style) < 1e-4
    given = (want_style * 0.5 + 0.1).clamp(-1, 1)
    pre["encoded_style"] = given
    demo = tm.sr_model(pre, mode="demo")
    tm.sr_model.train()
    want_demo = orc.demo({k: v.clone() for k, v in batch.items()}, given)
    assert rel(demo["fake_image"].cpu(), want_demo) < 1e-4
    if over["netG"] == "nospadenostyle":      # the generator ignores the style: demo == inference
        assert torch.equal(demo["fake_image"], out["fake_image"])
    tm.close()


def test_ablation_replayed_graphs_equal_eager():
    """nospadenostyle_8to64_ngf8 with hip_graphs on (first occurrence of a step variant eager, second captured, later ones
    replayed) against the same model stepped eagerly: at least 3 G and 3 D steps ran from graphs, losses and every parameter of
    G, E and D bit-identical -- the border pass allocates nothing, reads nothing on the host and folds in a fixed order."""
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    over = dict(_case("nospadenostyle_8to64_ngf8"), seed=21, full_style_image=True)
    batch = O.synthetic_batch(O.make_opt(**_case("nospadenostyle_8to64_ngf8")), 2, seed=31)
    iters = 8

    def run(**kw):
        tm = TrainerManager(make_opt(**over, **kw))
        out = []
        for _ in range(iters):
            tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
            tm.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
            out.append({k: float(v) for k, v in tm.get_latest_losses().items()})
        torch.cuda.synchronize()
        flat = (tm.optimizer_G.flat.detach().cpu().clone(), tm.optimizer_D.flat.detach().cpu().clone())
        stats = dict(tm.graph_stats)
        tm.close()
        return out, flat, stats

    eager, graphs = run(hip_graphs=False), run()
    print("graph stats", graphs[2])
    assert eager[2]["replayed"] == 0 and graphs[2]["captured"] + graphs[2]["replayed"] >= 6, graphs[2]
    assert graphs[2]["replayed"] >= 2, graphs[2]
    for it, (a, b) in enumerate(zip(eager[0], graphs[0])):
        assert a == b, (it, a, b)
    for x, y in zip(eager[1], graphs[1]):
        assert torch.equal(x, y), float((x - y).abs().max())


def test_ablation_half_mode_vs_oracle(monkeypatch):
    """nospadenostyle_8to64_ngf8 under precision='fp16' against the CPU oracle: the generated image within the 3e-2 that
    test_gpu_model.py::test_half_mode_vs_oracle applies to `fake`, the generator losses within its 5 %."""
    from deepsee_amd import networks as N
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    install_ablation(monkeypatch.setattr)
    over = _case("nospadenostyle_8to64_ngf8")
    oopt = O.make_opt(**over)
    states = O.recipe_state(oopt, gain=1.0)
    batch = O.synthetic_batch(oopt, 2, seed=31)
    ctl = O.RecordingCtl()
    orc = O.Oracle(oopt, states, ctl)
    orc.create_optimizers()
    random.seed(31)
    torch.manual_seed(31)
    gl, fake = orc.run_generator_one_step({k: v.clone() for k, v in batch.items()})
    tm = TrainerManager(make_opt(precision="fp16", **over))
    assert tm.sr_model.plan.half
    tm.sr_model.load_states(states)
    tm.sr_model.noise = N.ReplayNoise(ctl.tape)
    tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
    torch.cuda.synchronize()
    hgl = {k: float(v) for k, v in tm.g_losses.items()}
    dev = rel(tm.get_latest_generated().detach().cpu(), fake.detach())
    print("fp16 mode, nospadenostyle 8->64: |fake - oracle| / |oracle| = %.2e, losses %s" % (dev, hgl))
    assert dev < 3e-2, dev
    for k, v in gl.items():
        assert abs(hgl[k] - float(v.detach())) <= 0.05 * abs(float(v.detach())) + 1e-3, (k, hgl[k], float(v.detach()))
    tm.close()
