"""Non-square (H != W) batches through SRModel and the managers on the MI355X: the G+D step, `inference`, `encode_only`, `demo`
and `baseline` against the oracle with the wrappers of tools/gen_golden_rect.py (pinned to the reference by
tests/test_rect_model_host.py), dsee_resize_hw inside the red-zone harness against float64 F.interpolate and, for square outputs,
bit for bit against dsee_bicubic_down / dsee_interp_down, the 16-bit mode, the device loader feeding replayed hipGraphs, the
validation loop with its image files, inference_interpolation, and the refusal of the max_fm_size cap before any launch."""
import os
import random
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import redzone
from oracle import deepsee_oracle as O
from tools import gen_golden_loader as GL
from tools.gen_golden_rect import CASES as GOLD_CASES, hr_shape, install_rect

pytestmark = pytest.mark.gpu

UP_BOUND = 1e-6       # tests/test_gpu_visuals.py holds dsee_bicubic_up to this against F.interpolate
SHAPES = {"indep_5x4_to_40x32": ((5, 4), (40, 32)), "indep_4x8_to_32x64": ((4, 8), (32, 64)),
          "guided_8x4_to_64x32": ((8, 4), (64, 32))}
_models = {}


def rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-20))


def _manager(over, **kw):
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return TrainerManager(make_opt(**dict(over, **kw)))


def model_of(name):
    """One manager per case for the eval-mode tests of this module (recipe weights; `inference`, `demo`, `encode_only`, `baseline`
    and the explorative modes leave the model unchanged)."""
    if name not in _models:
        over = GOLD_CASES[name]["opt"]
        tm = _manager(over, no_vgg_loss=True, hip_graphs=False)
        tm.sr_model.load_states(O.recipe_state(O.make_opt(**over), gain=1.0))
        _models[name] = tm
    return _models[name]


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    """The cached managers go when the module is done: every live TrainerManager is closed again (with a full garbage collection
    each) behind every later GPU test of the session (tests/conftest.py)."""
    yield
    for tm in _models.values():
        tm.close()
    _models.clear()


def oracle_of(name, seed=None):
    """(oracle, batch) of a case; call with the wrappers installed."""
    spec = GOLD_CASES[name]
    oopt = O.make_opt(**spec["opt"])
    batch = O.synthetic_batch(oopt, spec["n"], seed=1000 + spec["seed"] if seed is None else seed)
    return O.Oracle(oopt, O.recipe_state(oopt, gain=1.0)), batch


def clone(batch):
    return {k: v.clone() for k, v in batch.items()}


# ------------------------------------------------------------------------------------------------ the train step
@pytest.mark.parametrize("name", sorted(GOLD_CASES))
def test_rect_train_step_matches_oracle(name, monkeypatch):
    """One G+D step (tape replay, D step from the oracle's post-G state) on the fixture's batch, with every assertion and bound of
    test_gpu_model.py::test_train_step_matches_oracle (output and losses 1e-4, GRAD_MEDIAN_BOUND / GRAD_MAX_BOUND, D gradients,
    post-step state); the generated image has the HR shape."""
    from tests import test_gpu_model as TGM
    install_rect(monkeypatch.setattr)
    spec = GOLD_CASES[name]
    monkeypatch.setitem(TGM.CASES, name, dict(spec["opt"]))
    captured = {}
    run_case = TGM.run_case

    def on_the_fixture_batch(over, seed, **kw):
        out = run_case(over, seed=1000 + spec["seed"], **kw)
        captured["r"] = out
        return out
    monkeypatch.setattr(TGM, "run_case", on_the_fixture_batch)
    assert TGM.GRAD_MEDIAN_BOUND == 6e-3 and TGM.GRAD_MAX_BOUND == 2.5e-2
    TGM.test_train_step_matches_oracle(name)
    orc, tm, out = captured["r"]
    (lh, lw), (h, w) = SHAPES[name]
    assert hr_shape(tm.opt) == (h, w)
    assert tuple(out[0]["hfake"].shape) == tuple(out[0]["fake"].shape) == (2, 3, h, w)
    assert tuple(tm.sr_model.logs["image/downsized"].shape) == (2, lh, lw, 4)
    tm.close()


# ------------------------------------------------------------------------------------------------ the eval modes
@pytest.mark.parametrize("name", sorted(GOLD_CASES))
def test_rect_inference_encode_only_demo_match_oracle(name, monkeypatch):
    """The three modes of test_gpu_model.py::test_inference_mode_matches_oracle with its bound (test_gpu_explore.BOUND)."""
    from tests.test_gpu_explore import BOUND
    install_rect(monkeypatch.setattr)
    orc, batch = oracle_of(name)
    (lh, lw), (h, w) = SHAPES[name]
    tm = model_of(name)
    model = tm.sr_model.eval()
    try:
        pre = tm.preprocess_input(clone(batch))
        assert tuple(pre["image_lr"].shape) == (2, lh, lw, 4) and tuple(pre["image_hr"].shape) == (2, h, w, 4)
        out = model(dict(pre), mode="inference")
        want = orc.inference(clone(batch))
        assert tuple(out["fake_image"].shape) == tuple(want.shape) == (2, 3, h, w)
        err = {"inference": rel(out["fake_image"], want)}
        style = model(dict(pre), mode="encode_only")
        want_style = orc.encode_only(clone(batch))
        assert tuple(style.shape) == tuple(want_style.shape)
        err["encode_only"] = rel(style.detach(), want_style)
        given = (want_style * 0.5 + 0.1).clamp(-1, 1)
        demo = model(dict(pre, encoded_style=given), mode="demo")
        err["demo"] = rel(demo["fake_image"], orc.demo(clone(batch), given))
    finally:
        model.train()
    print("%s: %s" % (name, {k: "%.2e" % v for k, v in err.items()}))
    assert max(err.values()) < BOUND, err


@pytest.mark.parametrize("name", ["indep_5x4_to_40x32", "indep_4x8_to_32x64"])
def test_rect_baseline_is_the_bicubic_image(name, monkeypatch):
    """`baseline` on a non-square LR image: F.interpolate(lr, (H, W), 'bicubic').clamp(-1, 1) in float64 of the LR image the model
    was given, to the bound dsee_bicubic_up is held to."""
    from deepsee_amd import ops
    install_rect(monkeypatch.setattr)
    _, batch = oracle_of(name)
    (lh, lw), (h, w) = SHAPES[name]
    tm = model_of(name)
    pre = tm.preprocess_input(clone(batch))
    noise = (tm.sr_model.noise.step, tm.sr_model.noise.offset)
    out = tm.sr_model(pre, "baseline")
    lr = ops.to_nchw(pre["image_lr"], 3).cpu()
    assert tuple(lr.shape) == (2, 3, lh, lw)
    err = rel(out["fake_image"], F.interpolate(lr.double(), (h, w), mode="bicubic").clamp(-1, 1))
    print("%s baseline: %.2e" % (name, err))
    assert tuple(out["fake_image"].shape) == (2, 3, h, w) and err < UP_BOUND
    assert float(out["fake_image"].max()) <= 1.0 and float(out["fake_image"].min()) >= -1.0
    assert out["image_full"] is pre["image_hr"] and (tm.sr_model.noise.step, tm.sr_model.noise.offset) == noise


# ------------------------------------------------------------------------------------------------ dsee_resize_hw
def native(x_nchw, cs):
    """Tagged native NHWC [N, H, W, cs]; with cs = 4 the padding channel holds 1e30 (it must never be read as data)."""
    n, _, h, w = x_nchw.shape
    t = torch.full((n, h, w, cs), 1e30, dtype=torch.float32, device="cuda")
    t[..., :3] = x_nchw.cuda().permute(0, 2, 3, 1)
    t.dsee_layout = "nhwc"
    return t


def _image(n, h, w):
    g = torch.Generator().manual_seed(100 * h + w)
    return torch.rand(n, 3, h, w, generator=g) * 2.4 - 1.2                               # the clamp is reached


def float64_resize(x, oh, ow, mode, clamp):
    y = F.interpolate(x.double(), (oh, ow), mode=mode)
    return y.clamp(-1, 1) if clamp else y


RESIZES = [((40, 32), (5, 4)), ((32, 40), (4, 5)), ((12, 20), (3, 5)), ((20, 12), (5, 3)),        # down, both orientations
           ((5, 4), (40, 32)), ((4, 5), (32, 40))]                                                # up


@pytest.mark.parametrize("cs", [3, 4])
@pytest.mark.parametrize("src,dst", RESIZES)
def test_resize_hw_guarded_against_float64(src, dst, cs):
    """All four modes, with and without the clamp, inside the red-zone harness (guards around the source, the destination: no
    byte outside them is written, no poison reaches the result).  Down-sampling to tools.gen_golden_loader.LR_BOUND, up-sampling
    to the bound of dsee_bicubic_up; nearest at these integer ratios is bit for bit F.interpolate's."""
    from deepsee_amd import ops
    x = _image(2, *src)
    xd = native(x, cs)
    bound = GL.LR_BOUND if dst[0] < src[0] else UP_BOUND
    with redzone.guarded() as rz:
        got = {(mode, clamp): ops.resize_hw(xd, dst[0], dst[1], mode, clamp=clamp)
               for mode in ("bicubic", "bilinear", "nearest", "area") for clamp in (True, False)}
    assert rz.guarded == {"resize_hw"} and rz.calls == 8 and not rz.passthrough
    for (mode, clamp), y in got.items():
        assert tuple(y.shape) == (2, dst[0], dst[1], 4) and y.dsee_layout == "nhwc" and float(y[..., 3].abs().max()) == 0.0
        want = float64_resize(x, dst[0], dst[1], mode, clamp)
        err = rel(y[..., :3].permute(0, 3, 1, 2), want)
        print("%s -> %s cs %d %-8s clamp %d: %.2e" % (src, dst, cs, mode, clamp, err))
        assert err < bound, (mode, clamp, err)
        if mode == "nearest":
            assert torch.equal(y[..., :3].permute(0, 3, 1, 2).cpu(), float64_resize(x, dst[0], dst[1], mode, clamp).float())
        if clamp:
            assert float(y.abs().max()) <= 1.0


@pytest.mark.parametrize("cs", [3, 4])
@pytest.mark.parametrize("src,s", [((32, 32), 4), ((48, 80), 8)])
def test_resize_hw_square_output_has_the_bits_of_the_old_downsamplers(src, s, cs):
    from deepsee_amd import ops
    xd = native(_image(2, *src), cs)
    with redzone.guarded():
        assert torch.equal(ops.resize_hw(xd, s, s, "bicubic"), ops.bicubic_down(xd, s))
        for mode in ("bilinear", "nearest", "area"):
            assert torch.equal(ops.resize_hw(xd, s, s, mode), ops.interp_down(xd, s, mode)), mode


def test_resize_hw_refuses_bad_arguments():
    from deepsee_amd import lib as L
    from deepsee_amd import ops
    xd = native(_image(1, 8, 8), 4)
    with pytest.raises(ValueError, match="bicubic, bilinear|bilinear, nearest"):
        ops.resize_hw(xd, 4, 4, "linear")
    for bad in ((0, 4, 3, 1), (4, 4, 7, 1), (4, 4, 3, 2)):
        with pytest.raises(L.DseeError, match="argument check failed"):
            L.call("resize_hw", xd, ops.new(1, 4, 4, 4), 1, 8, 8, bad[0], bad[1], 4, 4, bad[2], bad[3])


# ------------------------------------------------------------------------------------------------ VGG19 on 40 x 32: a 5 x 4 map
@pytest.mark.parametrize("h,w", [(5, 4), (4, 7), (7, 9)])
def test_maxpool2_drops_the_odd_row_and_column(h, w):
    """nn.MaxPool2d(2, 2) floors: the last row / column of an odd map is in no window and gets a zero gradient (the fourth pool of
    the VGG loss on a 40 x 32 image sees 5 x 4).  Bit for bit against torch, inside the red-zone harness."""
    from deepsee_amd import ops
    g = torch.Generator().manual_seed(10 * h + w)
    x = F.relu(torch.randn(2, 8, h, w, generator=g)).requires_grad_()                    # ties at 0 like VGG after ReLU
    y = F.max_pool2d(x, 2, 2)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    with redzone.guarded() as rz:
        xs = ops.to_nhwc(x.detach().cuda()).requires_grad_()
        ys = ops.MaxPool2.apply(xs)
        ys.backward(ops.to_nhwc(gy.cuda()))
    assert {"maxpool2_fwd", "maxpool2_bwd"} <= rz.guarded
    assert tuple(ys.shape) == (2, h // 2, w // 2, 8)
    assert torch.equal(ops.to_nchw(ys.detach(), 8).cpu(), y.detach())
    assert torch.equal(ops.to_nchw(xs.grad, 8).cpu(), x.grad)


# ------------------------------------------------------------------------------------------------ the 16-bit mode
def test_rect_half_mode_vs_oracle(monkeypatch):
    """precision='fp16' on 4 x 8 -> 32 x 64: the generated image of one G step against the oracle (same weights, inputs, noise
    tape and branch decisions) within the 16-bit forward bound of test_gpu_model.py / test_gpu_explore.py."""
    from deepsee_amd import networks as N
    from tests.test_gpu_explore import HALF_BOUND
    install_rect(monkeypatch.setattr)
    name = "indep_4x8_to_32x64"
    spec = GOLD_CASES[name]
    oopt = O.make_opt(**spec["opt"])
    states = O.recipe_state(oopt, gain=1.0)
    batch = O.synthetic_batch(oopt, 2, seed=1000 + spec["seed"])
    ctl = O.RecordingCtl()
    orc = O.Oracle(oopt, states, ctl)
    orc.create_optimizers()
    random.seed(spec["seed"])
    torch.manual_seed(spec["seed"])
    _, fake = orc.run_generator_one_step(clone(batch))
    tm = _manager(spec["opt"], precision="fp16")
    assert tm.sr_model.plan.half
    tm.sr_model.load_states(states)
    tm.sr_model.noise = N.ReplayNoise(ctl.tape)
    tm.run_generator_one_step(clone(batch))
    torch.cuda.synchronize()
    hfake = tm.get_latest_generated().detach().cpu()
    dev = rel(hfake, fake.detach())
    print("fp16 mode on 32 x 64 vs the oracle: |fake - oracle| / |oracle| = %.2e" % dev)
    assert tuple(hfake.shape) == (2, 3, 32, 64) and 0 < dev < HALF_BOUND, dev
    tm.close()


# ------------------------------------------------------------------------------------------------ loader -> model
def _write_pairs(folder, n, hw=(48, 44)):
    from PIL import Image
    os.makedirs(os.path.join(folder, "lab"))
    os.makedirs(os.path.join(folder, "img"))
    rng = np.random.default_rng(3)
    for i in range(n):
        Image.fromarray(rng.integers(0, 19, hw, dtype=np.uint8)).save(os.path.join(folder, "lab", "%03d.png" % i))
        Image.fromarray(rng.integers(0, 256, hw + (3,), dtype=np.uint8)).save(os.path.join(folder, "img", "%03d.png" % i))


FIXED = dict(preprocess_mode="fixed", crop_size=32, aspect_ratio=0.8, start_size=4, batchSize=2, ngf=8, nef=8, ndf=8)


def test_fixed_mode_loader_feeds_replayed_graphs(tmp_path):
    """RawFolderDataset + DeviceLoader with preprocess_mode='fixed', aspect_ratio 0.8: HR 40 x 32, LR 5 x 4.  The guided model
    has one graph key per step kind (no branch coins), so step 1 is eager, step 2 is captured and replayed, step 3 replays; a
    following square batch is a shape of its own: eager again, then its own graphs."""
    from deepsee_amd import data as D
    _write_pairs(str(tmp_path), 6)
    tm = _manager(dict(FIXED, netE="fullstyle", noisy_style_scale=0.05), hip_graphs=True, no_flip=True, seed=5)
    opt = tm.opt
    ds = D.RawFolderDataset(opt, str(tmp_path / "lab"), str(tmp_path / "img"), seed=1)
    batches = list(D.DeviceLoader(ds, opt, shuffle=False))
    assert len(batches) == 3
    stats = []
    for b in batches:
        assert tuple(b["image_hr"].shape) == (2, 40, 32, 4) and tuple(b["image_lr"].shape) == (2, 5, 4, 4)
        assert tuple(b["input_semantics"].t.shape) == (2, 40, 32)
        tm.run_generator_one_step(b)
        tm.run_discriminator_one_step(b)
        losses = {k: float(v) for k, v in tm.get_latest_losses().items()}
        assert all(np.isfinite(v) for v in losses.values()), losses
        assert tuple(tm.get_latest_generated().shape) == (2, 3, 40, 32)
        stats.append(dict(tm.graph_stats))
    assert [(s["eager"], s["captured"], s["replayed"]) for s in stats] == [(2, 0, 0), (2, 2, 0), (2, 2, 2)], stats
    sig_rect = tm._shape_signature(batches[0])
    g = torch.Generator().manual_seed(2)
    square = {"image": torch.randint(0, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8),
              "label": torch.randint(0, 19, (2, 32, 32), generator=g, dtype=torch.uint8)}
    for step in range(2):
        b = D.device_preprocess(opt, square)
        assert tuple(b["image_lr"].shape) == (2, 4, 4, 4)
        assert tm._shape_signature(b) != sig_rect
        tm.run_generator_one_step(b)
        tm.run_discriminator_one_step(b)
        assert tuple(tm.get_latest_generated().shape) == (2, 3, 32, 32)
        assert all(np.isfinite(float(v)) for v in tm.get_latest_losses().values())
    s = tm.graph_stats
    assert (s["eager"], s["captured"], s["replayed"], s["evicted_shapes"]) == (4, 4, 2, 0), s
    assert len({k[-2] for k in tm._graphs}) == 2                                         # two shapes own graphs
    tm.close()


# ------------------------------------------------------------------------------------------------ validation loop, image files
def test_rect_validation_loop_and_image_files(tmp_path, monkeypatch):
    """InferenceManager.run(save_to=) on non-square batches: PSNR / SSIM / RMSE are the oracle's psnr_ssim_rmse of the same images
    (the bounds of test_gpu_ops.py::test_psnr_ssim_rmse_kernel_matches_reference_numbers against the oracle: 1e-11, 1e-9, 1e-9);
    every PNG has the shape save_images_only implies; fake_image/<name>.png is tensor2im of the returned image."""
    from PIL import Image
    from deepsee_amd.managers import InferenceManager
    from deepsee_amd.visuals import tensor2im
    install_rect(monkeypatch.setattr)
    name = "indep_5x4_to_40x32"
    tm = model_of(name)
    opt, model = tm.opt, tm.sr_model
    oopt = O.make_opt(**GOLD_CASES[name]["opt"])
    raw = [O.synthetic_batch(oopt, 2, seed=300 + i) for i in range(2)]
    for i, b in enumerate(raw):       # smooth images: SSIM / MS-SSIM of pure noise say nothing
        b["image"] = F.interpolate(F.interpolate(b["image"], (10, 8), mode="area"), (40, 32), mode="bicubic").clamp(-1, 1)
        b["path"] = ["s%d_%d.png" % (i, k) for k in range(2)]
    folder = str(tmp_path / "val")
    res = InferenceManager(opt, num_samples=3).run(model, [dict(clone({k: v for k, v in b.items() if k != "path"}), path=b["path"])
                                                           for b in raw], save_to=folder)
    assert model.training and res["n_samples"] == 4
    model.eval()
    scores, index = [], 0
    try:
        for b in raw:
            with torch.no_grad():
                out = model(tm.preprocess_input(clone({k: v for k, v in b.items() if k != "path"})), "inference")
            fake = out["fake_image"]
            assert tuple(fake.shape) == (2, 3, 40, 32)
            scores.append(O.psnr_ssim_rmse(fake.cpu(), b["image"]))
            want_u8 = tensor2im(fake)
            for k in range(2):
                stem = b["path"][k]
                shapes = {key: np.asarray(Image.open(os.path.join(folder, key, stem))).shape
                          for key in ("input_semantics", "image_lr", "fake_image", "image_hr", "combined")}
                assert shapes == {"input_semantics": (40, 32, 3), "image_lr": (5, 4, 3), "fake_image": (40, 32, 3),
                                  "image_hr": (40, 32, 3), "combined": (40, 4 * 32, 3)}, shapes
                assert np.array_equal(np.asarray(Image.open(os.path.join(folder, "fake_image", stem))), want_u8[k])
                strip = np.asarray(Image.open(os.path.join(folder, "combined", stem)))
                for col, key in ((0, "input_semantics"), (2, "fake_image"), (3, "image_hr")):
                    assert np.array_equal(strip[:, 32 * col:32 * (col + 1)], np.asarray(Image.open(os.path.join(folder, key, stem))))
                # the LR column: the bilinear upsampling of the LR image, within one level of the float64 result of its fp32 pixels
                lr = out["image_lr"][k:k + 1, ..., :3].permute(0, 3, 1, 2).double().cpu()
                up = (F.interpolate(lr, (40, 32), mode="bilinear") + 1) / 2 * 255
                want_col = up.clamp(0, 255)[0].permute(1, 2, 0).numpy()
                assert np.abs(strip[:, 32:64].astype(np.float64) - want_col).max() <= 1.0
                index += 1
    finally:
        model.train()
    scores = torch.cat(scores).numpy()
    assert index == 4 and np.isfinite(scores).all()
    print("rect validation:", dict(res))
    assert abs(float(res["psnr/mean"]) - scores[:, 0].mean()) <= 1e-11
    assert abs(float(res["ssim/mean"]) - scores[:, 1].mean()) <= 1e-9
    assert abs(float(res["rmse/mean"]) - scores[:, 2].mean()) <= 1e-9


# ------------------------------------------------------------------------------------------------ an explorative mode
def test_rect_inference_interpolation_columns_are_demo_calls(monkeypatch):
    """inference_interpolation on 4 x 8 -> 32 x 64: [B, 3, 32, n * 64]; column k is the `demo` call with the k-th style matrix of
    the mode (deepsee_amd.explore.build_styles), to the bound of test_gpu_explore.py::test_middle_column_is_plain_inference."""
    from deepsee_amd import explore
    from tests.test_gpu_explore import BOUND
    from tools import gen_golden_explore as GE
    install_rect(monkeypatch.setattr)
    name = "indep_4x8_to_32x64"
    _, batch = oracle_of(name)
    tm = model_of(name)
    model = tm.sr_model
    saved = {k: getattr(model.opt, k, None) for k in dict(GE.TEST_DEFAULTS, explore_chunk=0)}
    # (4 of the 6 pairs per pass: a pass straddles images)
    for k, v in dict(GE.TEST_DEFAULTS, n_interpolation=3, noise_delta=1.0, explore_chunk=4).items():
        setattr(model.opt, k, v)
    model.eval()
    try:
        pre = tm.preprocess_input(clone(batch))
        out = model(dict(pre), "inference_interpolation")
        fake = out["fake_image"]
        n = int(model.opt.n_interpolation)
        assert n == 3 and tuple(fake.shape) == (2, 3, 32, n * 64)
        s0 = model.encode_with("mini", pre["image_lr"], pre["input_semantics"])
        styles = explore.build_styles("inference_interpolation", model.opt, s0, rule=explore.style_variants)
        assert tuple(styles.shape[:2]) == (2, n)
        errs = []
        for k in range(n):
            demo = model(dict(pre, encoded_style=styles[:, k].contiguous()), "demo")["fake_image"]
            errs.append(rel(fake[..., 64 * k:64 * (k + 1)], demo))
        plain = model(dict(pre), "inference")["fake_image"]
    finally:
        model.train()
        for k, v in saved.items():
            setattr(model.opt, k, v)
    print("inference_interpolation 32 x 64: column errors %s" % ["%.2e" % e for e in errs])
    assert max(errs) < BOUND, errs
    assert rel(fake[..., :64], fake[..., 64:128]) > 1e-3                                 # the columns do differ
    assert tuple(plain.shape) == (2, 3, 32, 64)


# ------------------------------------------------------------------------------------------------ the refused cap
def test_cap_on_a_non_square_map_is_refused_before_any_launch(monkeypatch):
    """64 x 32 with max_fm_size=16: ValueError from every mode that runs the generator, with no entry point called (lib.CALLS)
    and the noise state (step, offset, device epoch) where it was; the same model runs a square batch, cap and all."""
    from deepsee_amd import lib as L
    install_rect(monkeypatch.setattr)
    over = dict(GOLD_CASES["guided_8x4_to_64x32"]["opt"], max_fm_size=16)
    tm = _manager(over, hip_graphs=False, no_vgg_loss=True)
    model = tm.sr_model
    batch = O.synthetic_batch(O.make_opt(**over), 2, seed=9)
    pre = tm.preprocess_input(clone(batch))
    assert tuple(pre["image_lr"].shape) == (2, 8, 4, 4)
    torch.cuda.synchronize()
    epoch = int(model.noise.epoch.item())
    state = (model.noise.step, model.noise.offset)
    calls = L.CALLS
    for mode in ("generator", "discriminator", "inference", "demo", "inference_reference"):
        with pytest.raises(ValueError, match=r"32 x 16.*max_fm_size=16"):
            model(dict(pre), mode)
    assert L.CALLS == calls and (model.noise.step, model.noise.offset) == state and int(model.noise.epoch.item()) == epoch
    with pytest.raises(ValueError, match="max_fm_size=16"):
        tm.run_generator_one_step(clone(batch))
    assert (model.noise.step, model.noise.offset) == state
    # `baseline` and `encode_only` run no generator level
    assert tuple(model(dict(pre), "baseline")["fake_image"].shape) == (2, 3, 64, 32)
    # a square batch of the same model keeps the reference's cap
    sq = O.make_opt(**dict(over, aspect_ratio=1.0))
    tm.run_generator_one_step(clone(O.synthetic_batch(sq, 2, seed=9)))
    assert tuple(tm.get_latest_generated().shape) == (2, 3, 32, 32)
    assert all(np.isfinite(float(v)) for v in tm.get_latest_losses().values())
    tm.close()
