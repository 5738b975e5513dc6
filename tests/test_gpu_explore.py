"""The explorative inference modes on the MI355X: dsee_style_explore and dsee_nhwc_to_nchw_tiled bit for bit against their torch
restatements, every mode against the fixtures the REAL reference wrote (tests/golden/explore, tools/gen_golden_explore.py) at
the bound of test_gpu_model.py::test_inference_mode_matches_oracle, in one pass and in chunks, the refusals, and that a live
trainer's model is left as it was."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import deepsee_oracle as O
from tools import gen_golden_explore as G

pytestmark = pytest.mark.gpu

CASES = sorted(G.CASES)
BOUND = 1e-4          # test_inference_mode_matches_oracle's
HALF_BOUND = 3e-2     # the 16-bit forward bound of test_gpu_model.py
_models = {}


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64).cpu(), torch.as_tensor(b, dtype=torch.float64).cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-20))


load = G.load


def model_of(over, **kw):
    """One manager per option set for the whole module (recipe weights; its model is only ever run in the explorative modes and
    `inference`, which leave it unchanged)."""
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    key = json.dumps([over, kw], sort_keys=True)
    if key not in _models:
        tm = TrainerManager(make_opt(**dict(over, no_vgg_loss=True, hip_graphs=False, **kw)))
        tm.sr_model.load_states(O.recipe_state(O.make_opt(**over), gain=1.0))
        _models[key] = tm
    return _models[key]


def set_test_options(model, test_opt, chunk):
    for k, v in dict(G.TEST_DEFAULTS, **test_opt).items():
        setattr(model.opt, k, v)
    model.opt.explore_chunk = chunk


def inputs_of(tm, rec):
    batch = O.synthetic_batch(O.make_opt(**rec["opt"]), 2, seed=rec["batch_seed"])
    data = tm.preprocess_input({k: v.clone() for k, v in batch.items()})
    if rec["guiding_image_id"] is not None:
        data["guiding_image_id"] = list(rec["guiding_image_id"])
    if rec["mode"] == "inference_interpolation_style":
        given = G.unpack(rec["encoded"][0])
        data["style_from"], data["style_to"] = given.clone(), given.flip(0).clone()
    return data


def run_case(rec, chunk, **kw):
    tm = model_of(rec["opt"], **kw)
    model = tm.sr_model
    set_test_options(model, rec["test_opt"], chunk)
    model.eval()
    try:
        torch.manual_seed(rec["rng_seed"])
        out = model(inputs_of(tm, rec), rec["mode"])
    finally:
        model.train()
    torch.cuda.synchronize()
    return out


def columns(img, n):
    return [img[:, k] for k in range(n)] if img.dim() == 5 else list(img.chunk(n, dim=-1))


def sample(t, k=64):      # oracle.gen_golden.slice_of
    f = t.detach().reshape(-1)
    return f[torch.linspace(0, f.numel() - 1, min(k, f.numel())).long()]


# ------------------------------------------------------------------------------------------------ the two kernels
FLAGS = [dict(clamp=c, recurrent=r, noise=z, same=s, mask=m)
         for c, r, z, s, m in [(1, 0, 0, 1, "some"), (0, 0, 0, 0, "some"), (1, 1, 0, 0, "some"), (0, 1, 1, 0, "some"),
                               (1, 0, 1, 1, "some"), (1, 1, 1, 0, "all"), (1, 1, 1, 0, "none"), (0, 0, 1, 1, "all")]]


@pytest.mark.parametrize("f", FLAGS, ids=lambda f: "-".join("%s%s" % (k[0], v) for k, v in f.items()))
def test_style_explore_equals_the_torch_rule(f):
    style_explore_equals_the_torch_rule(f)


def style_explore_equals_the_torch_rule(f, nc=19):
    """(the body, with the class count as an argument: tests/test_gpu_label_nc.py runs it at other counts than 19)"""
    from deepsee_amd import explore
    B, n, S = 2, 4, 128
    g = torch.Generator().manual_seed(11)
    s0 = torch.rand(B, nc, S, generator=g) * 3 - 1.5
    s1 = s0 if f["same"] else torch.rand(B, nc, S, generator=g) * 3 - 1.5
    src0, src1 = torch.randint(0, B, (B, n), generator=g), torch.randint(0, B, (B, n), generator=g)
    alpha, beta, gamma = (torch.rand(n, generator=g) * 2 - 1 for _ in range(3))
    noise = torch.randn(B, n, nc, S, generator=g) * 0.3 if f["noise"] else None
    mask = {"some": torch.rand(nc, generator=g) < 0.4, "all": torch.ones(nc, dtype=torch.bool),
            "none": torch.zeros(nc, dtype=torch.bool)}[f["mask"]]
    assert f["mask"] != "some" or 0 < int(mask.sum()) < nc
    want = explore.style_variants_torch(s0, s1, src0, src1, alpha, beta, gamma, noise, mask, f["clamp"], f["recurrent"])
    d0 = s0.cuda()
    d1 = d0 if f["same"] else s1.cuda()
    buf = torch.full((B * n * nc * S + 512,), float("nan"), device="cuda")           # poisoned, with guard bands
    out = buf[256:-256].view(B, n, nc, S)
    got = explore.style_variants(d0, d1, src0, src1, alpha, beta, gamma, None if noise is None else noise.cuda(), mask,
                                 f["clamp"], f["recurrent"], out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    assert bool(torch.isnan(buf[:256]).all()) and bool(torch.isnan(buf[-256:]).all())
    un = ~mask
    for b in range(B):
        for k in range(n):
            assert torch.equal(got[b, k, un].cpu(), s0[src0[b, 0 if f["recurrent"] else k]][un])
    # the same rule evaluated by torch on the device agrees too (no contraction on either side)
    assert torch.equal(explore.style_variants_torch(d0, d1, src0, src1, alpha, beta, gamma,
                                                    None if noise is None else noise.cuda(), mask, f["clamp"],
                                                    f["recurrent"]).cpu(), want)


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("shape,shift", [((2, 3, 32, 32, 4), 0), ((2, 3, 5, 6, 4), 0), ((2, 3, 5, 6, 4), 1), ((2, 3, 8, 8, 4), 3)])
def test_nhwc_to_nchw_tiled_equals_permute_and_cat(shape, shift, merge):
    """`shift`: floats by which source and destination are moved off their 16-byte alignment."""
    from deepsee_amd import explore
    B, n, H, W, cs = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * n, H, W, cs, generator=g)
    nchw = x[..., :3].permute(0, 3, 1, 2).reshape(B, n, 3, H, W)
    want = torch.cat([nchw[:, k] for k in range(n)], -1) if merge else nchw.contiguous()
    xbuf = torch.zeros(x.numel() + 8, device="cuda")
    xd = xbuf[shift:shift + x.numel()].view(x.shape)
    xd.copy_(x)
    guard = 1024
    for splits in ([(0, B * n)], [(0, 4), (4, B * n)], [(p, p + 1) for p in range(B * n)]):
        ybuf = torch.full((want.numel() + 2 * guard + 8,), -7.0, device="cuda")
        y = ybuf[guard + shift:guard + shift + want.numel()].view(want.shape)
        for p0, p1 in splits:
            explore.assemble(xd[p0:p1], B, n, merge, out=y, pair0=p0)
        torch.cuda.synchronize()
        assert torch.equal(y.cpu(), want), (splits, float((y.cpu() - want).abs().max()))
        assert bool((ybuf[:guard + shift] == -7.0).all()) and bool((ybuf[guard + shift + want.numel():] == -7.0).all())
    # one chunk alone writes its own pairs only
    ybuf = torch.full((want.numel(),), -7.0, device="cuda")
    y = ybuf.view(want.shape)
    explore.assemble(xd[2:4], B, n, merge, out=y, pair0=2)
    torch.cuda.synchronize()
    written = (y != -7.0).cpu()
    stacked = written if not merge else torch.stack(list(written.chunk(n, dim=-1)), 1)
    touched = stacked.reshape(B * n, -1).all(1).tolist()
    assert touched == [False, False, True, True, False, False] and not stacked.reshape(B * n, -1)[[0, 1, 4, 5]].any()
    fresh = explore.assemble(xd, B, n, merge)
    assert tuple(fresh.shape) == tuple(want.shape) and torch.equal(fresh.cpu(), want)


# ------------------------------------------------------------------------------------------------ the modes against the reference
@pytest.mark.parametrize("case", CASES)
def test_style_kernel_reproduces_the_references_applied_styles(case):
    """dsee_style_explore on the fixture's encoded styles: the style matrices the reference fed its generator, exactly."""
    from deepsee_amd import explore
    from deepsee_amd.options import make_opt
    rec = load(case)
    opt = make_opt(**dict(rec["opt"], **rec["test_opt"]))
    encoded = [G.unpack(e).cuda() for e in rec["encoded"]]
    s1 = {"inference_interpolation_style": encoded[0].flip(0).contiguous(),
          "inference_particular_full": encoded[-1]}.get(rec["mode"])
    drawn = G.unpack(rec["noise"]).cuda() if "noise" in rec else None
    got = explore.build_styles(rec["mode"], opt, encoded[0], s1, drawn, explore.style_variants)
    assert G.same_styles(rec, got)


@pytest.mark.parametrize("chunk", [64, 1, 4])
@pytest.mark.parametrize("case", CASES)
def test_mode_matches_the_reference(case, chunk):
    """Every fixture case in one pass (chunk >= the pair count), pair by pair, and in passes of 4 (which straddle images at
    n = 3); all three held to the same bound -- they are not bit-identical to each other: operand scales come from per-tensor
    maxima."""
    rec = load(case)
    out = run_case(rec, chunk)
    assert list(out.keys()) == rec["keys"]
    n = rec["n"]
    particular = rec["mode"].startswith("inference_particular")
    for key, want in rec["images"].items():
        img = out[key].detach().cpu()
        assert list(img.shape) == want["shape"], key
        errs = [abs(float(img.norm()) - want["norm"]) / want["norm"], rel(sample(img), want["slice"]), rel(img, G.unpack(want["full"]))]
        errs += [abs(float(c.norm()) - w) / w for c, w in zip(columns(img, 1 if particular else n), want["column_norms"])]
        print("%s chunk %d %s: norm %.2e sample %.2e whole tensor %.2e columns %.2e"
              % (case, chunk, key, errs[0], errs[1], errs[2], max(errs[3:])))
        assert max(errs) < BOUND, (key, errs)
    if rec.get("style_list"):
        applied = G.applied_of(rec)
        assert [list(s.shape) for s in out["style"]] == rec["style_list"]
        for b, s in enumerate(out["style"]):
            assert rel(s, applied[b]) < BOUND
            at = applied[b].abs() == 1
            assert torch.equal(s.cpu()[at], applied[b][at])          # clamped entries are exactly +-1 on both sides
    elif "style" in rec["keys"]:
        assert out["style"] == []
    if rec["guiding_image_id"] is not None:
        assert out["guiding_image_id"] == rec["guiding_image_id"]
        assert out["guiding_image"] is not None and out["guiding_input_label"] is not None


def test_middle_column_is_plain_inference():
    rec = load("indep_interpolation")
    out = run_case(rec, 8)
    tm = model_of(rec["opt"])
    tm.sr_model.eval()
    try:
        plain = tm.sr_model(inputs_of(tm, rec), "inference")["fake_image"]
    finally:
        tm.sr_model.train()
    w = plain.shape[-1]
    mid = out["fake_image"][..., w:2 * w]
    assert rel(mid, plain) < BOUND
    assert rel(out["fake_image"][..., :w], plain) > 0.1 and rel(out["fake_image"][..., 2 * w:], plain) > 0.1   # the others move


def test_style_matrix_input_is_used_instead_of_the_encoder():
    rec = load("indep_interpolation")
    tm = model_of(rec["opt"])
    set_test_options(tm.sr_model, rec["test_opt"], 8)
    data = inputs_of(tm, rec)
    data["style_matrix"] = G.unpack(rec["encoded"][0])
    tm.sr_model.eval()
    try:
        out = tm.sr_model(data, "inference_interpolation")
    finally:
        tm.sr_model.train()
    assert rel(sample(out["fake_image"].cpu()), rec["images"]["fake_image"]["slice"]) < BOUND


def test_half_precision_mode():
    """One case under precision = 'fp16', with the metric and the bound of the 16-bit forward parity of tests/test_gpu_model.py
    (test_half_mode_tracks_fp32): |fake_fp16 - fake_fp32| / |fake_fp32| < 3e-2 between two managers that differ in opt.precision
    only, on freshly initialised weights (seed 11): inference_interpolation at 8 -> 64 with the InstanceNorm generator
    (norm_G = spectrallateseaninstance3x3).
    Why that case and not a fixture case: the explorative modes run in eval mode, and with BatchNorm running statistics that no
    training has fitted -- the recipe weights' as well as a fresh model's -- every pixel of an eval-mode image sits at exactly
    +-1 (tests/golden/explore: saturated_share 1.0).  On such a sign map an L2 distance counts flipped pixels, 2 * sqrt(share
    flipped), instead of measuring precision: measured on the MI355X, fp16 against fp32 reads 5.7e-2 for indep_interpolation
    (15 flipped pixels of 18 432), 5.1e-2 .. 7.4e-2 over five fixture cases, and plain `inference` on the same batches reads
    the same (3.6e-2 .. 7.1e-2).  The test this bound comes from compares training-mode images, which are not saturated;
    InstanceNorm normalises per image in eval mode too, so its eval-mode image is not saturated either (asserted below)."""
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    over = dict(start_size=8, crop_size=64, load_size=64, batchSize=2, ngf=8, seed=11, no_vgg_loss=True, hip_graphs=False,
                norm_G="spectrallateseaninstance3x3", region_idx=[1, 2, 5], n_interpolation=3, noise_delta=1.0)
    batch = O.synthetic_batch(O.make_opt(**{k: over[k] for k in ("start_size", "crop_size", "load_size", "batchSize", "ngf")}), 2,
                              seed=5)
    fakes = {}
    for precision in ("fp32", "fp16"):
        tm = TrainerManager(make_opt(precision=precision, **over))
        assert tm.sr_model.plan.half == (precision == "fp16")
        tm.sr_model.eval()
        fakes[precision] = tm.sr_model(tm.preprocess_input({k: v.clone() for k, v in batch.items()}),
                                       "inference_interpolation")["fake_image"].cpu()
    full, half = fakes["fp32"], fakes["fp16"]
    assert float((full.abs() == 1).float().mean()) < 0.01           # not a sign map
    w = full.shape[-1] // 3
    assert rel(full[..., :w], full[..., w:2 * w]) > 1e-3             # and the variants differ
    dev = rel(half, full)
    print("fp16 vs fp32: %.2e" % dev)
    assert 0 < dev < HALF_BOUND, dev


# ------------------------------------------------------------------------------------------------ refusals
def test_unsupported_combinations_are_refused():
    small = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)
    guided = dict(small, netE="fullstyle", noisy_style_scale=0.05)
    combos = [(dict(guided, guiding_style_image=True), "inference_particular_combined"),
              (dict(guided, guiding_style_image=False), "inference_particular_combined"),
              (small, "inference_particular_full"),
              (dict(guided, guiding_style_image=False), "inference_particular_full"),
              (dict(guided, guiding_style_image=True), "inference_reference_interpolation"),
              (dict(small, guiding_style_image=True), "inference_reference_interpolation")]
    for over, mode in combos:
        tm = model_of(over)
        set_test_options(tm.sr_model, {}, 8)
        batch = O.synthetic_batch(O.make_opt(**over), 2, seed=3)
        data = tm.preprocess_input({k: v.clone() for k, v in batch.items()})
        data["guiding_image_id"] = ["a", "b"]
        with pytest.raises(ValueError, match=mode):
            tm.sr_model(data, mode)


def test_even_n_missing_id_and_unknown_modes():
    small = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)
    tm = model_of(small)
    model = tm.sr_model
    batch = O.synthetic_batch(O.make_opt(**small), 2, seed=3)
    data = tm.preprocess_input({k: v.clone() for k, v in batch.items()})
    set_test_options(model, dict(n_interpolation=4), 8)
    with pytest.raises(AssertionError, match="odd n"):
        model(dict(data), "inference_interpolation")
    style = torch.zeros(2, 19, 128)
    with pytest.raises(AssertionError, match="odd n"):
        model(dict(data, style_from=style, style_to=style), "inference_interpolation_style")
    set_test_options(model, {}, 8)
    for mode in ("inference_noise", "inference_multi_modal", "inference_replace_semantics", "inference_reference_semantics",
                 "bogus"):
        with pytest.raises(ValueError, match=r"\|mode\| is invalid"):
            model(dict(data), mode)
    gover = dict(small, netE="fullstyle", noisy_style_scale=0.05, guiding_style_image=True)
    gtm = model_of(gover)
    set_test_options(gtm.sr_model, dict(n_interpolation=3), 8)
    gbatch = O.synthetic_batch(O.make_opt(**gover), 2, seed=3)
    with pytest.raises(KeyError, match="guiding_image_id"):
        gtm.sr_model(gtm.preprocess_input({k: v.clone() for k, v in gbatch.items()}), "inference_reference")


# ------------------------------------------------------------------------------------------------ a live trainer, files
def test_a_live_trainer_is_left_untouched():
    """In TRAINING mode, between two steps: parameters, running statistics, spectral-norm vectors, the noise source's epoch,
    forward index and coins are what they were, and the model is still in training mode."""
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    over = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)
    tm = TrainerManager(make_opt(**dict(over, hip_graphs=False, no_vgg_loss=True, region_idx=[1, 2, 5], n_interpolation=3,
                                        noise_delta=0.4)))
    batch = O.synthetic_batch(O.make_opt(**over), 2, seed=9)
    tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
    tm.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
    model = tm.sr_model

    def snapshot():
        torch.cuda.synchronize()
        nets = {lab: {k: v.detach().clone() for k, v in net.state_dict().items()}
                for lab, net in (("SR", model.netSR), ("E", model.netE), ("D", model.netD))}
        noise = model.noise
        return nets, (noise.step, noise.offset, int(noise.epoch.item()), noise.coin("enc_full"), noise.coin("enc_noise")), \
            (model.training, model.last_encoded_style_is_full, model.last_encoded_style_is_noisy)

    before = snapshot()
    assert model.training
    for mode in ("inference_interpolation", "inference_reference", "inference_particular_combined"):
        out = model(tm.preprocess_input({k: v.clone() for k, v in batch.items()}), mode)
        assert torch.isfinite(out.get("fake_image", out.get("fake_image_original"))).all()
    after = snapshot()
    assert before[1:] == after[1:]
    for lab in before[0]:
        for k, v in before[0][lab].items():
            assert torch.equal(v, after[0][lab][k]), (lab, k)
    tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})       # and training goes on
    assert all(bool(torch.isfinite(v).all()) for v in tm.g_losses.values())


@pytest.mark.parametrize("stacked", [False, True])
def test_save_strips_round_trip(tmp_path, stacked):
    from PIL import Image
    from deepsee_amd import explore, visuals
    rec = load("indep_interpolation_stacked" if stacked else "indep_interpolation")
    tm = model_of(rec["opt"])
    set_test_options(tm.sr_model, rec["test_opt"], 8)
    tm.sr_model.eval()
    try:
        out = tm.sr_model(inputs_of(tm, rec), rec["mode"], u8=True)
    finally:
        tm.sr_model.train()
    fake = out["fake_image"]
    strip = torch.cat([fake[:, k] for k in range(3)], -1) if stacked else fake
    want = visuals.tensor2im(strip)
    assert want.shape == (2, 32, 96, 3) and np.array_equal(out["fake_image_u8"].cpu().numpy(), want)
    paths = ["/data/val/first.jpg", "synthetic/000002"]
    explore.save_strips(out, paths, str(tmp_path))
    assert sorted(os.listdir(str(tmp_path / "fake_image"))) == ["000002.png", "first.png"]
    for b, name in enumerate(("first.png", "000002.png")):
        back = np.asarray(Image.open(str(tmp_path / "fake_image" / name)))
        assert back.shape == (32, 96, 3) and np.array_equal(back, want[b])
    del out["fake_image_u8"]                                   # without the strips asked for: converted on the way out
    explore.save_strips(out, paths, str(tmp_path / "again"))
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "again" / "fake_image" / "first.png"))), want[0])
