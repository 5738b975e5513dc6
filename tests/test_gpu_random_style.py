"""opt.random_style_matrix on the MI355X: the one-hot x noise convolution (dsee_onehot_noise_conv3x3_fwd / _wgrad) against float64
torch with an explicit field, its Philox form against the explicit form fed dsee_rng_fill's tensor (bit for bit), the G+D step,
`inference` and `encode_only` against the substituted oracle (tools/gen_golden_random_style.py; pinned to the reference by
tests/test_random_style_host.py), replayed graphs, the 16-bit mode, the eval-mode stream (style_seed), refusals and the
checkpoint layout."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from oracle import deepsee_oracle as O
from tools.gen_golden_random_style import CASES as GOLD_CASES, install_random_style

pytestmark = pytest.mark.gpu

SMALL = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)
RANDOM = dict(SMALL, netE="fullstyle", noisy_style_scale=0.05, random_style_matrix=True)

# (N, H, W, L, Co): every pixel near a border; odd, rectangular, smaller than a tile; tile edges with a partial tile; 32 classes
FWD_SHAPES = [(2, 8, 8, 19, 8), (1, 5, 7, 19, 32), (2, 40, 40, 19, 32), (3, 16, 16, 32, 32)]
WGRAD_SHAPES = FWD_SHAPES + [(2, 64, 64, 19, 32)]           # + several partial blocks


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-20))


def _inputs(shape, bias=True):
    """Seeded label map (classes 0 and L - 1 present, class 3 absent, a few pixels of value 255), field, weight, bias and an
    upstream gradient, all on the CPU."""
    n, h, w, nl, co = shape
    g = torch.Generator().manual_seed(1000 * h + 10 * w + nl + co)
    lab = torch.randint(0, nl, (n, h, w), generator=g)
    lab[lab == 3] = 4
    flat = lab.view(-1)
    flat[0], flat[-1] = 0, nl - 1
    flat[torch.randperm(flat.numel(), generator=g)[:max(2, flat.numel() // 40)] + 0] = 255
    flat[1], flat[-2] = 0, nl - 1                       # (whatever the 255s hit)
    eps = torch.randn(n, h, w, generator=g)
    wt = torch.randn(co, nl, 3, 3, generator=g) * 0.1
    b = torch.randn(co, generator=g) * 0.1 if bias else None
    dout = torch.randn(n, h, w, co, generator=g)
    return lab.to(torch.uint8), eps, wt, b, dout


def _masked(lab, eps, nl):
    """onehot(lab) * eps_full in float64, NCHW: the class channel of every pixel holds its eps (255: no channel)."""
    oh = (lab.long()[:, None] == torch.arange(nl)[None, :, None, None]).double()
    return oh * eps.double()[:, None]


def _reference(lab, eps, wt, b, dout, nl):
    """float64 F.conv2d(onehot(lab) * eps, w, b, padding=1) with its weight / bias gradients under `dout`, and the sums of the
    absolute terms of every output and gradient element."""
    x = _masked(lab, eps, nl)
    w64 = wt.double().requires_grad_()
    b64 = b.double().requires_grad_() if b is not None else None
    y = F.conv2d(x, w64, b64, padding=1)
    d64 = dout.double().permute(0, 3, 1, 2)
    (y * d64).sum().backward()
    y_abs = F.conv2d(x.abs(), wt.double().abs(), None, padding=1)
    wa = torch.ones_like(w64).requires_grad_()
    (F.conv2d(x.abs(), wa, None, padding=1) * d64.abs()).sum().backward()
    return (y.detach().permute(0, 2, 3, 1), y_abs.permute(0, 2, 3, 1), w64.grad, wa.grad,
            None if b is None else b64.grad, d64.abs().sum((0, 2, 3)))


def _run(lab, field, wt, b, dout, nl):
    from deepsee_amd import ops
    labels = ops.Labels(lab.cuda(), nl)
    w = wt.cuda().requires_grad_()
    bb = b.cuda().requires_grad_() if b is not None else None
    y = ops.onehot_noise_conv3x3(labels, field, w, bb)
    y.backward(dout.cuda())
    torch.cuda.synchronize()
    return y.detach(), w.grad, None if bb is None else bb.grad


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_forward_explicit_field_vs_float64(shape, bias):
    """|err| <= 1e-6 * sum_taps |w eps| + 1e-30 element by element (nine fp32 FMAs: at most 9 * 2^-24 = 5.4e-7 of that sum)."""
    lab, eps, wt, b, dout = _inputs(shape, bias)
    want, terms, _, _, _, _ = _reference(lab, eps, wt, b, dout, shape[3])
    y, _, _ = _run(lab, eps.cuda(), wt, b, dout, shape[3])
    assert tuple(y.shape) == (shape[0], shape[1], shape[2], shape[4])
    err = (y.double().cpu() - want).abs()
    ratio = float((err / terms.clamp_min(1e-30)).max())
    print("forward %s bias %s: worst |err| / sum|w eps| = %.3g" % (shape, bias, ratio))
    assert bool((err <= 1e-6 * terms + 1e-30).all()), ratio


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad_explicit_field_vs_float64(shape):
    """|err| <= 1e-5 * sum |terms| element by element (the bound of test_gpu_gan_mode.py's reductions: room for ~100 serial fp32
    adds per partial before the tree); the absent class's rows are exactly 0; a second call is bit-identical."""
    lab, eps, wt, b, dout = _inputs(shape, True)
    _, _, dw, dw_terms, db, db_terms = _reference(lab, eps, wt, b, dout, shape[3])
    _, gw, gb = _run(lab, eps.cuda(), wt, b, dout, shape[3])
    ew, eb = (gw.double().cpu() - dw).abs(), (gb.double().cpu() - db).abs()
    ratio = max(float((ew / dw_terms.clamp_min(1e-30)).max()), float((eb / db_terms.clamp_min(1e-30)).max()))
    print("wgrad %s: worst |err| / sum|terms| = %.3g" % (shape, ratio))
    assert bool((ew <= 1e-5 * dw_terms + 1e-30).all()) and bool((eb <= 1e-5 * db_terms + 1e-30).all()), ratio
    assert not bool((lab == 3).any()) and not bool(gw[:, 3].any())
    _, gw2, gb2 = _run(lab, eps.cuda(), wt, b, dout, shape[3])
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
    # without a bias no bias gradient is written, and the weight gradient is the same
    _, gw3, gb3 = _run(lab, eps.cuda(), wt, None, dout, shape[3])
    assert gb3 is None and torch.equal(gw, gw3)


@pytest.mark.parametrize("offset,steps", [(0, 0), (12345, 0), (7, 2)])
@pytest.mark.parametrize("shape", [(1, 5, 7, 19, 32), (2, 40, 40, 19, 32)])
def test_philox_field_equals_rng_fill(shape, offset, steps):
    """field = NULL with (seed, offset): forward and weight gradient are torch.equal to the explicit path fed the tensor
    dsee_rng_fill writes at the same (seed, offset) -- N H W not a multiple of 4, a non-zero offset, a non-zero device epoch."""
    from deepsee_amd import networks as N
    from deepsee_amd import ops
    n, h, w, nl, co = shape
    lab, _, wt, b, dout = _inputs(shape, True)
    noise = N.DeviceNoise(5)
    for _ in range(steps):
        noise.begin_step()
    assert int(noise.epoch.item()) == steps * N.EPOCH_STRIDE
    seed, px = 991, n * h * w
    field = ops.rng_fill(((px + 3) // 4 * 4,), seed, offset, normal=True)[:px].reshape(n, h, w).contiguous()
    y0, gw0, gb0 = _run(lab, field, wt, b, dout, nl)
    y1, gw1, gb1 = _run(lab, ops.PhiloxField((n, h, w), seed, offset, True, noise), wt, b, dout, nl)
    assert torch.equal(y0, y1) and torch.equal(gw0, gw1) and torch.equal(gb0, gb1)
    assert float(field.std()) > 0.5 and float(y1.abs().max()) > 0
    if steps:       # without the epoch the stream is the one of epoch 0: other values
        y2, _, _ = _run(lab, ops.PhiloxField((n, h, w), seed, offset, False), wt, b, dout, nl)
        assert not torch.equal(y1, y2)


def test_entry_points_validate_before_they_launch():
    from deepsee_amd import lib as L
    from deepsee_amd import ops
    lab, eps, wt, b, dout = _inputs((1, 5, 7, 19, 8), True)
    labels = ops.Labels(lab.cuda(), 19)
    table, out = ops.new(9, 19, 8), ops.new(1, 5, 7, 8)
    for co in (6, 36):          # not a multiple of 4; 9 float4 per pixel do not divide the block
        with pytest.raises(L.DseeError, match="argument check failed"):
            L.call("onehot_noise_conv3x3_fwd", labels.t, eps.cuda(), 0, 0, 0, table, None, out, 1, 5, 7, 19, co)
    with pytest.raises(L.DseeError, match="argument check failed"):
        L.call("onehot_noise_conv3x3_fwd", labels.t, eps.cuda(), 0, 0, 0, table, None, out, 1, 5, 7, 33, 8)
    with pytest.raises(L.DseeError, match="argument check failed"):
        L.call("onehot_noise_conv3x3_wgrad", labels.t, eps.cuda(), 0, 0, 0, dout.cuda(), 1, 5, 7, 19, 8, ops.new(8, 19, 3, 3),
               None, None)
    assert L.lib().dsee_onehot_noise_conv3x3_wgrad_workspace(1, 5, 7, 19, 8) == (9 * 19 + 1) * 8 * 4


# ------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("name", sorted(GOLD_CASES))
def test_random_style_train_step_matches_oracle(name, monkeypatch):
    """G+D step (tape replay, D step from the oracle's post-G state) against the substituted oracle with the bounds and
    post-step state checks of test_gpu_model.py::test_train_step_matches_oracle."""
    from tests import test_gpu_model as TGM
    install_random_style(monkeypatch.setattr)
    over = dict(GOLD_CASES[name]["opt"])
    monkeypatch.setitem(TGM.CASES, name, over)
    captured = {}
    run_case = TGM.run_case

    def spy(*a, **kw):
        out = run_case(*a, **kw)
        captured["r"] = out
        return out
    monkeypatch.setattr(TGM, "run_case", spy)
    TGM.test_train_step_matches_oracle(name)
    orc, tm, out = captured["r"]
    assert orc.opt.random_style_matrix and tm.opt.random_style_matrix
    assert tuple(tm.sr_model.netE.state_dict()["initial.0.0.weight_orig"].shape) == (tm.opt.nef, tm.opt.label_nc, 3, 3)
    assert "E.initial.0.0.weight_orig" in out[0]["touched_g"]
    assert sum(1 for k, t, _ in orc.ctl.tape if t == "style_field") == 2      # the G step's field and the D step's own
    tm.close()


def _manager(over):
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return TrainerManager(make_opt(**over))


@pytest.mark.parametrize("guide", [True, False])
def test_inference_and_encode_only_match_oracle(guide, monkeypatch):
    """`inference` and `encode_only` in eval mode on a tape recorded from the substituted oracle."""
    from deepsee_amd import networks as N
    install_random_style(monkeypatch.setattr)
    over = dict(RANDOM, guiding_style_image=guide)
    oopt = O.make_opt(**over)
    states = O.recipe_state(oopt, gain=1.0)
    batch = O.synthetic_batch(oopt, 2, seed=77)
    ctl = O.RecordingCtl()
    orc = O.Oracle(oopt, states, ctl)
    torch.manual_seed(3)
    ofake = orc.inference({k: v.clone() for k, v in batch.items()})
    ostyle = orc.encode_only({k: v.clone() for k, v in batch.items()})
    assert [t for _, t, _ in ctl.tape] == ["style_field", "style_field"]
    tm = _manager(over)
    m = tm.sr_model
    m.load_states(states)
    m.eval()
    m.noise = N.ReplayNoise(ctl.tape)
    fake = m(tm.preprocess_input({k: v.clone() for k, v in batch.items()}), mode="inference")["fake_image"]
    style = m(tm.preprocess_input({k: v.clone() for k, v in batch.items()}), mode="encode_only")
    torch.cuda.synchronize()
    assert m.noise.pos == 2
    print("inference %.3g encode_only %.3g" % (rel(fake.cpu(), ofake), rel(style.cpu(), ostyle)))
    assert rel(fake.cpu(), ofake) < 1e-4 and rel(style.cpu(), ostyle) < 1e-4
    tm.close()


def _steps(over, n_steps, batch):
    """The helper of test_gpu_gan_mode.py, returning the graph statistics as well."""
    tm = _manager(over)
    out = []
    for _ in range(n_steps):
        tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
        fake = tm.get_latest_generated().detach().cpu()
        tm.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
        out.append((fake, {k: float(v.detach()) for k, v in tm.get_latest_losses().items()}))
    torch.cuda.synchronize()
    stats = dict(tm.graph_stats)
    tm.close()
    return out, stats


def test_random_style_graphs_and_half_mode():
    """Four G+D steps replayed from captured graphs equal the same steps run eagerly (a replay draws the field the eager step
    draws: same seed, offset and device epoch), with the bounds of test_gpu_gan_mode.py; the fields differ from step to step;
    the 16-bit mode runs the same steps finitely, its first step within that mode's bounds (image 3e-2, losses 5 %)."""
    over = dict(RANDOM, seed=11)
    batch = O.synthetic_batch(O.make_opt(**RANDOM), 2, seed=5)
    eager, es = _steps(dict(over, hip_graphs=False), 4, batch)
    graph, gs = _steps(dict(over, hip_graphs=True), 4, batch)
    assert gs["replayed"] >= 2 and es.get("replayed", 0) == 0, (gs, es)
    for (fe, le), (fg, lg) in zip(eager, graph):
        assert rel(fg, fe) <= 1e-6, rel(fg, fe)
        assert set(le) == set(lg)
        for k in le:
            assert abs(lg[k] - le[k]) <= 1e-5 * abs(le[k]) + 1e-7, (k, lg[k], le[k])
    assert rel(graph[3][0], graph[2][0]) > 1e-3          # (replays of one graph: fresh fields, stepped weights)
    half, _ = _steps(dict(over, precision="fp16"), 4, batch)
    for fake, losses in half:
        assert bool(torch.isfinite(fake).all()) and all(v == v and abs(v) < 1e4 for v in losses.values()), losses
    assert rel(half[0][0], eager[0][0]) < 3e-2, rel(half[0][0], eager[0][0])
    for k, v in eager[0][1].items():
        assert abs(half[0][1][k] - v) <= 0.05 * abs(v) + 0.05, (k, half[0][1][k], v)


# ------------------------------------------------------------------------------------------------ the eval stream
def test_eval_stream_and_style_seed():
    """`inference` twice without style_seed: different images; twice with the same style_seed: bit-identical; another seed:
    different.  inference_interpolation with style_seed = s: its middle column is `inference` with style_seed = s."""
    tm = _manager(dict(RANDOM, seed=4, hip_graphs=False, noise_delta=0.5, n_interpolation=3))
    m = tm.sr_model
    m.load_states(O.recipe_state(O.make_opt(**RANDOM), gain=1.0))     # (O(1) activations: a fresh init saturates the tanh)
    m.eval()
    batch = O.synthetic_batch(O.make_opt(**RANDOM), 2, seed=9)

    def run(mode="inference", **kw):
        return m(tm.preprocess_input({k: v.clone() for k, v in batch.items()}), mode=mode, **kw)
    a, b = run()["fake_image"].clone(), run()["fake_image"].clone()
    assert bool(torch.isfinite(a).all()) and not torch.equal(a, b)
    c, d, e = run(style_seed=31)["fake_image"].clone(), run(style_seed=31)["fake_image"].clone(), run(style_seed=32)["fake_image"]
    assert torch.equal(c, d) and not torch.equal(c, e) and not torch.equal(c, a)
    strip = run("inference_interpolation", style_seed=31)["fake_image"]
    wd = c.shape[3]
    assert tuple(strip.shape) == (2, 3, c.shape[2], 3 * wd)
    assert torch.equal(strip[:, :, :, wd:2 * wd], c)
    assert not torch.equal(strip[:, :, :, :wd], c)
    s1, s2, s3 = run("encode_only", style_seed=5), run("encode_only", style_seed=5), run("encode_only")
    assert torch.equal(s1, s2) and not torch.equal(s1, s3) and not torch.equal(s3, run("encode_only"))
    tm.close()


def test_eval_forwards_leave_training_bit_identical():
    """train, InferenceManager.run, train == train, train: losses and an encoder parameter, bit for bit."""
    from deepsee_amd.data import DeviceLoader, SyntheticDataset
    from deepsee_amd.managers import InferenceManager
    over = dict(RANDOM, seed=6)
    batch = O.synthetic_batch(O.make_opt(**RANDOM), 2, seed=5)

    def train(validate):
        tm = _manager(over)
        out = []
        for it in range(2):
            tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
            tm.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
            out.append({k: float(v.detach()) for k, v in tm.get_latest_losses().items()})
            if validate and it == 0:
                res = InferenceManager(tm.opt, num_samples=3).run(
                    tm.sr_model, DeviceLoader(SyntheticDataset(tm.opt, length=4), tm.opt, shuffle=False))
                assert res["n_samples"] == 4 and tm.sr_model.training and tm.sr_model.noise.eval_count == 2
        torch.cuda.synchronize()
        p = tm.sr_model.netE.state_dict()["initial.0.0.weight_orig"].detach().cpu().clone()
        state = tm.sr_model.noise.state_dict()
        tm.close()
        return out, p, state
    plain, p0, st0 = train(False)
    mixed, p1, st1 = train(True)
    assert plain == mixed and torch.equal(p0, p1) and st0 == st1 and "eval_count" not in st0


# ------------------------------------------------------------------------------------------------ refusals and layout
def test_combinedstyle_is_refused_at_build():
    from deepsee_amd.options import make_opt
    from deepsee_amd.sr_model import SRModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(ValueError, match="random_style_matrix needs netE='fullstyle'.*encoder.py:197-198"):
            SRModel(make_opt(**dict(SMALL, netE="combinedstyle", random_style_matrix=True)))


def test_reference_layout_state_dict_loads_and_rgb_encoder_is_refused():
    """The oracle's e_spec is the reference's state-dict layout (tools/gen_golden_random_style.py checks it against the
    reference's own state_dict()): a state of the variant loads, key for key and shape for shape; the state of the 3-channel
    encoder is refused with both shapes in the message."""
    oopt = O.make_opt(**RANDOM)
    spec = O.e_spec(oopt)
    assert tuple(spec["initial.0.0.weight_orig"]) == (oopt.nef, oopt.label_nc, 3, 3)
    assert tuple(spec["initial.0.0.weight_v"]) == (oopt.label_nc * 9,)
    states = O.recipe_state(oopt, gain=1.0)
    tm = _manager(dict(RANDOM, hip_graphs=False))
    m = tm.sr_model
    own = m.netE.state_dict()
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(s) for k, s in spec.items()}
    m.load_states(states)
    assert torch.equal(m.netE.state_dict()["initial.0.0.weight_orig"].cpu(), states["E"]["initial.0.0.weight_orig"])
    rgb = O.recipe_state(O.make_opt(**dict(RANDOM, random_style_matrix=False)), gain=1.0)["E"]
    with pytest.raises(RuntimeError, match=r"initial\.0\.0\.weight_orig is \[32, 3, 3, 3\] in the checkpoint, \[32, 19, 3, 3\]"):
        m.load_net_state(m.netE, rgb)
    tm.close()
