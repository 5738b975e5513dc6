"""The GAN objective (opt.gan_mode = ls / original / w) on the MI355X: the new element losses of ops.mean_loss against float64
torch (value and gradient, padded channels, row halves, weights, upstream scales, BCE logits up to 1e4, bitwise
reproducibility), the G+D step against the substituted oracle (tools/gen_golden_gan_mode.py; pinned to the reference by
tests/test_gan_mode_host.py), replayed graphs, the 16-bit mode, and the reference's ValueError for an unknown mode."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from oracle import deepsee_oracle as O
from tools.gen_golden_gan_mode import CASES as GOLD_CASES, install_gan_mode
from tools.gen_golden_nonspade_norm import install_nonspade_norm

pytestmark = pytest.mark.gpu

SMALL = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-20))


def _elem64(mode, x):
    """float64 element loss of a new mode (x: float64 tensor)."""
    from deepsee_amd import ops
    if mode == ops.MODE_W_FAKE:
        return x
    if mode == ops.MODE_LS_REAL:
        return (x - 1) ** 2
    if mode == ops.MODE_LS_FAKE:
        return x ** 2
    t = torch.ones_like(x) if mode == ops.MODE_BCE_REAL else torch.zeros_like(x)
    return F.binary_cross_entropy_with_logits(x, t, reduction="none")


def _new_modes():
    from deepsee_amd import ops
    return [ops.MODE_W_FAKE, ops.MODE_LS_REAL, ops.MODE_LS_FAKE, ops.MODE_BCE_REAL, ops.MODE_BCE_FAKE]


def _run(a, mode, weight, valid_c, lo, hi, upstream):
    """ops.mean_loss on a copy of the device tensor `a`; returns (loss, gradient w.r.t. a) after backward(upstream)."""
    from deepsee_amd import ops
    ad = a.clone().requires_grad_()
    loss = ops.mean_loss(ad, None, mode, weight, valid_c=valid_c, lo=lo, hi=hi)
    (loss * upstream).backward()
    torch.cuda.synchronize()
    return loss.detach(), ad.grad


def _want(a, mode, weight, valid_c, lo, hi, upstream):
    x = a.double().cpu().clone().requires_grad_()
    sub = x[lo:hi][..., :valid_c]
    l = _elem64(mode, sub)
    loss = weight * l.mean()
    (loss * upstream).backward()
    return loss.detach(), x.grad, weight * float(l.detach().abs().mean())


def _check(a, mode, weight, valid_c, lo, hi, upstream):
    loss, grad = _run(a, mode, weight, valid_c, lo, hi, upstream)
    wl, wg, scale = _want(a, mode, weight, valid_c, lo, hi, upstream)
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    g = grad.double().cpu()
    # (relative to the mean |element loss|: W's mean of signed logits may nearly cancel)
    assert abs(float(loss) - float(wl)) <= 1e-5 * scale + 1e-37, (mode, float(loss), float(wl))
    # element by element: relative to the element (the smallest BCE gradients are ~1e-9 / count), floored below fp32's range
    err = (g - wg).abs() - (1e-5 * wg.abs() + 1e-37)
    assert float(err.max()) <= 0.0, (mode, float(err.max()))
    # nothing outside [lo, hi) or in the padded channels
    mask = torch.zeros_like(g, dtype=torch.bool)
    mask[lo:hi, ..., :valid_c] = True
    assert not bool(g[~mask].any())
    return loss, grad


# (shape, valid_c, lo, hi): D predictions [2N, h, w, 1] with the generated / real halves of the G and D steps, a padded
# ld > valid_c tensor, a larger map of the benchmark's size (bs 8: 2N = 16 images of 35 x 35)
SHAPES = [((4, 9, 9, 1), 1, 0, 2), ((4, 9, 9, 1), 1, 2, 4), ((4, 9, 9, 1), 1, 0, 4), ((6, 5, 7, 4), 1, 3, 6),
          ((2, 6, 6, 8), 5, 0, 2), ((16, 35, 35, 1), 1, 8, 16)]


@pytest.mark.parametrize("shape,valid_c,lo,hi", SHAPES)
def test_new_modes_vs_float64(shape, valid_c, lo, hi):
    """Value and gradient of every new mode against float64 torch for weights 1 and 0.37 and upstream gradients 1 and -2.5
    (loss scaling / a re-weighted term); a second identical call is bitwise equal."""
    g = torch.Generator().manual_seed(sum(shape) + 10 * lo)
    a = (torch.randn(shape, generator=g) * 1.5).cuda()
    for mode in _new_modes():
        for weight, upstream in ((1.0, 1.0), (0.37, -2.5)):
            loss, grad = _check(a, mode, weight, valid_c, lo, hi, upstream)
            loss2, grad2 = _run(a, mode, weight, valid_c, lo, hi, upstream)
            assert torch.equal(loss, loss2) and torch.equal(grad, grad2), mode


@pytest.mark.parametrize("mag", [20.0, 100.0, 1e4])
def test_bce_modes_stay_finite_and_accurate_for_large_logits(mag):
    """Logits of +-20, +-100 and +-1e4 (each sign on its own, so the tiny values are not hidden under the large ones, and
    mixed): softplus and sigmoid stay finite and match float64 to 1e-5 relative, element by element."""
    from deepsee_amd import ops
    g = torch.Generator().manual_seed(int(mag))
    base = 1.0 + 0.01 * torch.rand(4, 7, 7, 1, generator=g)
    sign = torch.where(torch.rand(4, 7, 7, 1, generator=g) < 0.5, -1.0, 1.0)
    for a in ((mag * base).cuda(), (-mag * base).cuda(), (mag * base * sign).cuda()):
        for mode in (ops.MODE_BCE_REAL, ops.MODE_BCE_FAKE):
            for lo, hi in ((0, 2), (2, 4)):
                _check(a, mode, 0.5, 1, lo, hi, 3.0)


def test_hinge_modes_unchanged_and_bad_mode_refused():
    """Modes 0-3 keep their element losses; a mode past the last one is refused by the argument check."""
    from deepsee_amd import lib as L
    from deepsee_amd import ops
    g = torch.Generator().manual_seed(5)
    a = torch.randn(4, 9, 9, 1, generator=g).cuda()
    x = a.double().cpu()
    for mode, f in ((ops.MODE_NEG, lambda v: -v), (ops.MODE_HINGE_REAL, lambda v: -torch.clamp(v - 1, max=0)),
                    (ops.MODE_HINGE_FAKE, lambda v: -torch.clamp(-v - 1, max=0))):
        loss = ops.mean_loss(a, None, mode, 1.0, valid_c=1, lo=0, hi=4)
        assert abs(float(loss) - float(f(x).mean())) < 1e-6
    with pytest.raises(L.DseeError, match="argument check failed"):
        ops.mean_loss(a, None, ops.MODE_BCE_FAKE + 1, 1.0, valid_c=1, lo=0, hi=4)


def _install(monkeypatch):
    install_nonspade_norm(monkeypatch.setattr)
    install_gan_mode(monkeypatch.setattr)


@pytest.mark.parametrize("name", sorted(GOLD_CASES))
def test_gan_mode_train_step_matches_oracle(name, monkeypatch):
    """G+D step (tape replay, D step from the oracle's post-G state) against the substituted oracle with the bounds and
    post-step state checks of test_gpu_model.py::test_train_step_matches_oracle; the losses are the selected objective's."""
    from tests import test_gpu_model as TGM
    _install(monkeypatch)
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
    assert orc.opt.gan_mode == tm.opt.gan_mode == over["gan_mode"] != "hinge"
    print("%s: G %s D %s" % (name, out[0]["hgl"], out[0]["hdl"]))


def test_gan_mode_iterations_track_oracle(monkeypatch):
    """The two-iteration fixture case on the HIP model on its own (no oracle state loaded in between): the losses of both
    iterations follow the oracle (the second one within the beta1 = 0 Adam sign noise of the first step)."""
    from tests import test_gpu_model as TGM
    _install(monkeypatch)
    name = "indep_original_two_iters_4to32_ngf8"
    iters = GOLD_CASES[name]["iters"]
    orc, tm, out = TGM.run_case(dict(GOLD_CASES[name]["opt"]), seed=101 + len(name), iters=iters, sync_before_d=False)
    assert len(out) == iters == 2
    for it, r in enumerate(out):
        for k, v in r["gl"].items():
            assert abs(r["hgl"][k] - v) <= (1e-4 if it == 0 else 2e-2) * abs(v) + 1e-6, (it, k, r["hgl"][k], v)
        for k, v in r["dl"].items():
            assert abs(r["hdl"][k] - v) <= 5e-2 * abs(v) + 1e-6, (it, k, r["hdl"][k], v)


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
    flat = (tm.optimizer_G.flat.detach().cpu().clone(), tm.optimizer_D.flat.detach().cpu().clone())
    tm.close()
    return out, flat


@pytest.mark.parametrize("gan_mode,norm_d", [("ls", "spectralinstance"), ("original", "spectralinstance"),
                                             ("w", "spectralinstance"), ("ls", "spectralbatch")])
def test_gan_mode_graphs_and_half_mode(gan_mode, norm_d):
    """Three G+D steps replayed from captured graphs equal the same steps run eagerly (losses, images, G and D weights); one
    16-bit step gives finite losses within the 16-bit bounds of the norm tests (image 3e-2, losses 5 %) of the fp32 step."""
    over = dict(SMALL, seed=11, gan_mode=gan_mode, norm_D=norm_d)
    batch = O.synthetic_batch(O.make_opt(**SMALL), 2, seed=5)
    eager, ew = _steps(dict(over, hip_graphs=False), 3, batch)
    graph, gw = _steps(dict(over, hip_graphs=True), 3, batch)
    for (fe, le), (fg, lg) in zip(eager, graph):
        assert rel(fg, fe) <= 1e-6, rel(fg, fe)
        assert set(le) == set(lg)
        for k in le:
            assert abs(lg[k] - le[k]) <= 1e-5 * abs(le[k]) + 1e-7, (k, lg[k], le[k])
    # (beta1 = 0 Adam: a weight whose gradient is rounding noise may step the other way, by 2 lr_D = 8e-4 per step)
    for a, b in zip(ew, gw):
        assert float((b - a).abs().max()) <= 3 * 8e-4 and rel(b, a) <= 1e-4, (float((b - a).abs().max()), rel(b, a))
    half, _ = _steps(dict(over, precision="fp16"), 1, batch)
    assert rel(half[0][0], eager[0][0]) < 3e-2, rel(half[0][0], eager[0][0])
    for k, v in eager[0][1].items():
        assert half[0][1][k] == half[0][1][k] and abs(half[0][1][k]) < 1e4, (k, half[0][1][k])
        assert abs(half[0][1][k] - v) <= 0.05 * abs(v) + 0.05, (k, half[0][1][k], v)


def test_gan_mode_selects_the_objective():
    """The same model, weights and batch under hinge / w / ls / original: w's generator term is hinge's (both -x), bit for
    bit; the D terms of w, ls and original and the generator terms of ls and original differ from hinge's, and the ls /
    original terms are positive."""
    out = {m: _steps(dict(SMALL, seed=3, gan_mode=m, hip_graphs=False), 1, O.synthetic_batch(O.make_opt(**SMALL), 2,
                                                                                              seed=6))[0][0][1]
           for m in ("hinge", "w", "ls", "original")}
    assert out["w"]["GAN"] == out["hinge"]["GAN"]
    for m in ("ls", "original"):
        assert out[m]["D_Fake"] > 0 and out[m]["D_Real"] > 0 and out[m]["GAN"] > 0
        assert out[m]["D_Fake"] != out["hinge"]["D_Fake"] and out[m]["D_Real"] != out["hinge"]["D_Real"]
        assert out[m]["GAN"] != out["hinge"]["GAN"]
    assert out["w"]["D_Fake"] != out["hinge"]["D_Fake"] and out["w"]["D_Real"] != out["hinge"]["D_Real"]


def test_unknown_gan_mode_raises_for_training_only(tmp_path):
    """A training TrainerManager with gan_mode = 'LS' raises the reference's ValueError; an inference SRModel
    (isTrain = False: no GAN loss, sr_model.py:34-36) with the same value builds and runs."""
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    from deepsee_amd.sr_model import SRModel
    with pytest.raises(ValueError, match="Unexpected gan_mode LS"):
        TrainerManager(make_opt(**dict(SMALL, gan_mode="LS")))
    over = dict(SMALL, checkpoints_dir=str(tmp_path), name="ck", hip_graphs=False)
    tm = TrainerManager(make_opt(**over))
    tm.save("latest")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m = SRModel(make_opt(**dict(over, gan_mode="LS", isTrain=False)))
    assert m.netD is None and m.gan_modes is None
    assert all(torch.equal(a, b) for a, b in zip(m.netSR.state_dict().values(), tm.sr_model.netSR.state_dict().values()))
    batch = O.synthetic_batch(O.make_opt(**SMALL), 2, seed=5)
    m.eval()
    out = m(tm.preprocess_input({k: v.clone() for k, v in batch.items()}), mode="inference")
    assert torch.isfinite(out["fake_image"]).all()
    tm.close()
