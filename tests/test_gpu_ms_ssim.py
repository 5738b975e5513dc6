"""MS-SSIM (dsee_ms_ssim) and the InferenceManager validation loop on the MI355X: the kernel against tests/golden/ms_ssim/ms_ssim.json
(the float64 restatement to 1e-9, the reference's fp32 value to 2 g + 1e-9 with g the fixture's own gap), NaN where and only
where the reference has NaN, layouts and the padding channel, the argument check through the binding, the evaluator's MSSSIM
column, InferenceManager.run against scoring by hand, and a training run that continues bit-identically after a validation
pass (eager and with replayed hipGraphs)."""
import math
import os
import random
import warnings

import numpy as np
import pytest
import torch

from tools.gen_golden_ms_ssim import CASES as GEN_CASES, checksum, host_test_module, images

pytestmark = pytest.mark.gpu

H = host_test_module()      # msssim64 (the float64 restatement), fixture(), fixture_gap()
SMALL = dict(batchSize=2, ngf=8)
PRESET = "independent_8x_32"


def bits(t):
    return t.contiguous().view(torch.int64)


def native_with_garbage(x_nchw, fill):
    """Tagged native NHWC [N, H, W, 4] of an NCHW image, the padding channel filled with `fill`."""
    n, _, h, w = x_nchw.shape
    t = torch.full((n, h, w, 4), fill, dtype=torch.float32, device="cuda")
    t[..., :3] = x_nchw.cuda().permute(0, 2, 3, 1)
    t.dsee_layout = "nhwc"
    return t


# ---- 4: the kernel against the fixture
@pytest.mark.parametrize("name", sorted(GEN_CASES))
def test_ms_ssim_kernel_matches_fixture(name):
    from deepsee_amd import metrics as M
    cases = H.fixture()
    c, g = cases[name], H.fixture_gap(cases)
    fake, real = images(c)
    assert checksum(fake) == c["checksum"]["fake"] and checksum(real) == c["checksum"]["real"], "the recipe drifted"
    got = M.ms_ssim(fake.cuda(), real.cuda(), detail=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (c["N"], 11) and not got.is_cuda
    for i in range(c["N"]):
        terms = [float(v) for v in got[i, 1:]]
        worst = max(abs(a - b) for a, b in zip(terms, c["cs"][i] + c["sim"][i]))
        print("%s[%d]: value %.15g f64 %.15g ref %.9g  max |term - f64| %.3e  |value - f64| %.3e  g %.3e"
              % (name, i, float(got[i, 0]), c["f64"][i], c["ref"][i], worst, abs(float(got[i, 0]) - c["f64"][i]), g))
        for a, b in zip(terms, c["cs"][i] + c["sim"][i]):
            assert abs(a - b) <= 1e-9, (name, i, a, b)
        if math.isnan(c["ref"][i]):
            assert math.isnan(float(got[i, 0]))
        else:
            assert abs(float(got[i, 0]) - c["f64"][i]) <= 1e-9, (name, i, float(got[i, 0]), c["f64"][i])
            assert abs(float(got[i, 0]) - c["ref"][i]) <= 2 * g + 1e-9, (name, i, float(got[i, 0]), c["ref"][i], g)
    # the plain value; native NHWC in (garbage in the padding channel), same bits
    assert torch.equal(bits(M.ms_ssim(fake.cuda(), real.cuda())), bits(got[:, 0]))
    for fill in (float("nan"), 1e30):
        nat = M.ms_ssim(native_with_garbage(fake, fill), native_with_garbage(real, -fill), detail=True)
        assert torch.equal(bits(nat), bits(got)), (name, fill)
    # CPU tensors in the reference's layout are accepted as well
    assert torch.equal(bits(M.ms_ssim(fake, real, detail=True)), bits(got))


def test_ms_ssim_smallest_size_and_batch_order():
    """16 x 16 (level 4 is one pixel, every window smaller than 11; the reference itself raises below 32 on a pooling whose
    result it never uses) against the restatement alone, and a batch gives what its samples give one by one."""
    from deepsee_amd import metrics as M
    g = torch.Generator().manual_seed(5)
    for h, w in ((16, 16), (16, 40), (23, 37)):
        real = (torch.rand(2, 3, h, w, generator=g) * 1.6 - 0.8)
        fake = (real + 0.1 * torch.randn(2, 3, h, w, generator=g)).clamp(-1, 1)
        got = M.ms_ssim(fake, real, detail=True)
        for i in range(2):
            val, cs, sim = H.msssim64(fake[i], real[i])
            assert min(cs[:4] + [sim[4]]) >= 0.05
            want = [val] + cs + sim
            worst = max(abs(float(a) - b) for a, b in zip(got[i], want))
            print("%dx%d[%d]: max |kernel - f64| %.3e" % (h, w, i, worst))
            assert worst <= 1e-9
            assert torch.equal(bits(M.ms_ssim(fake[i:i + 1], real[i:i + 1], detail=True)), bits(got[i:i + 1]))


# ---- 5: the argument check through the binding
def test_ms_ssim_too_small_raises_before_any_launch():
    from deepsee_amd import lib as L
    from deepsee_amd import metrics as M
    for h, w in ((15, 32), (32, 15)):
        with pytest.raises(L.DseeError, match="argument check failed"):
            M.ms_ssim(torch.zeros(1, 3, h, w), torch.zeros(1, 3, h, w))
    torch.cuda.synchronize()


# ---- 6: the evaluator
def test_metrics_evaluator_ms_ssim_column(tmp_path):
    from deepsee_amd import metrics as M
    c = GEN_CASES["noise0.5_64_n3_s4"]
    fake, real = images(c)
    names = ["/data/val/img_%d.png" % i for i in range(3)]
    base = M.MetricsEvaluator()
    base.collect_samples(fake, real, names)
    d = tmp_path / "out"
    d.mkdir()
    ev = M.MetricsEvaluator(write_details=True, folder_out=str(d), ms_ssim=True)
    ev.collect_samples(fake, real, names)
    assert ev.psnr_buffer == base.psnr_buffer and ev.ssim_buffer == base.ssim_buffer and ev.rmse_buffer == base.rmse_buffer
    assert ev.ms_ssim_buffer == [float(v) for v in M.ms_ssim(fake, real)] and ev.n_samples == 3
    res = ev.get_result()
    assert list(res) == ["psnr/mean", "ssim/mean", "ms_ssim/mean", "rmse/mean", "psnr/std", "ssim/std", "ms_ssim/std",
                         "rmse/std", "n_samples"]
    assert list(base.get_result()) == ["psnr/mean", "ssim/mean", "rmse/mean", "psnr/std", "ssim/std", "rmse/std", "n_samples"]
    assert res["ms_ssim/mean"] == np.mean(ev.ms_ssim_buffer) and res["ms_ssim/std"] == np.std(ev.ms_ssim_buffer)
    for k, v in base.get_result().items():
        assert res[k] == v, k
    rows = open(os.path.join(str(d), "metrics.csv")).read().split()
    assert rows[0] == "ID,PSNR,SSIM,MSSSIM,RMSE" and len(rows) == 4
    for i, row in enumerate(rows[1:]):
        assert row == ",".join(map(str, ["img_%d" % i, ev.psnr_buffer[i], ev.ssim_buffer[i], ev.ms_ssim_buffer[i],
                                         ev.rmse_buffer[i]]))
    ev.clear()
    assert ev.ms_ssim_buffer == [] and ev.psnr_buffer == [] and ev.ssim_buffer == [] and ev.rmse_buffer == []
    assert ev.n_samples == 0


# ---- 7 + 8: the validation loop
def _opt(**over):
    from deepsee_amd.options import make_opt
    return make_opt(PRESET, **dict(SMALL, **over))


def _manager(opt):
    from deepsee_amd.managers import TrainerManager
    random.seed(1)
    torch.manual_seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return TrainerManager(opt)


def _batch(opt, seed, with_path=False):
    import bench
    b = bench.synthetic_batch(opt, opt.batchSize, seed, "cpu")
    if with_path:
        b["path"] = ["/data/val/s%d_%d.png" % (seed, i) for i in range(opt.batchSize)]
    return b


class FlakyLoader:
    """A list-backed loader whose iterator raises ValueError instead of handing out the batches listed in `bad`."""

    def __init__(self, batches, bad=()):
        self.batches, self.bad = batches, set(bad)

    def __iter__(self):
        self.i = -1
        return self

    def __next__(self):
        self.i += 1
        if self.i >= len(self.batches):
            raise StopIteration
        if self.i in self.bad:
            raise ValueError("corrupt sample")
        return self.batches[self.i]


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_inference_manager_run_matches_scoring_by_hand(tmp_path, capsys):
    from deepsee_amd import metrics as M
    from deepsee_amd.managers import InferenceManager
    opt = _opt()
    tm = _manager(opt)
    model = tm.sr_model
    batches = [_batch(opt, 300 + i, with_path=True) for i in range(4)]
    im = InferenceManager(opt, num_samples=20, write_details=True, folder_out=str(tmp_path / "val"))
    # 11 batches asked for, 4 listed, the third one raises ValueError: three scored, one skipped, StopIteration ends the loop
    res = im.run(model, FlakyLoader(batches, bad=(2,)))
    assert model.training and im.skipped_samples == 1
    text = capsys.readouterr().out
    assert "corrupt sample" in text and "Skipping sample" in text and "StopIteration raised" in text
    assert "Total number of samples skipped: 1" in text
    # by hand
    model.eval()
    scores, ms = [], []
    for i in (0, 1, 3):
        out = model(im.preprocess({k: v for k, v in batches[i].items()}, from_dataloader=True), "inference")
        scores.append(M.psnr_ssim_rmse(out["fake_image"], out["image_hr"]))
        ms.append(M.ms_ssim(out["fake_image"], out["image_hr"]))
    model.train()
    scores, ms = torch.cat(scores).numpy(), torch.cat(ms).numpy()
    want = {"psnr/mean": np.mean(scores[:, 0]), "ssim/mean": np.mean(scores[:, 1]), "ms_ssim/mean": np.mean(ms),
            "rmse/mean": np.mean(scores[:, 2]), "psnr/std": np.std(scores[:, 0]), "ssim/std": np.std(scores[:, 1]),
            "ms_ssim/std": np.std(ms), "rmse/std": np.std(scores[:, 2]), "n_samples": 6}
    print("run:", dict(res))
    assert list(res) == list(want) and "FID" not in res
    for k in want:
        assert same(float(res[k]), float(want[k])), (k, res[k], want[k])
    assert np.isfinite(scores).all()
    rows = open(os.path.join(str(tmp_path / "val"), "metrics.csv")).read().split()
    assert rows[0] == "ID,PSNR,SSIM,MSSSIM,RMSE" and [r.split(",")[0] for r in rows[1:]] == [
        "s300_0", "s300_1", "s301_0", "s301_1", "s303_0", "s303_1"]
    # the buffers were cleared; a num_samples below the loader's length stops after num_samples // batchSize + 1 batches
    assert im.metrics.n_samples == 0 and im.metrics.ms_ssim_buffer == []
    res2 = InferenceManager(opt, num_samples=3).run(model, batches)
    assert res2["n_samples"] == 4 and model.training
    # the loop restores train mode and clears the buffers when it raises as well
    im3 = InferenceManager(opt, num_samples=20)
    with pytest.raises(KeyError):
        im3.run(model, [batches[0], {"label": batches[0]["label"]}])
    assert model.training and im3.metrics.n_samples == 0


@pytest.mark.parametrize("hip_graphs,variant", [(False, "independent"), (True, "independent"), (True, "guided")])
def test_validation_does_not_disturb_training(hip_graphs, variant):
    """Two managers from the same seed run 4 G+D steps; one validates after step 2.  Losses and the final state (parameters,
    running statistics, spectral-norm vectors) are bit-identical.  Guided variant: one encoder branch, so steps 3-4 are
    replays of the graphs captured at step 2."""
    from deepsee_amd.managers import InferenceManager
    over = dict(hip_graphs=hip_graphs)
    if variant == "guided":
        over.update(netE="fullstyle", noisy_style_scale=0.05, guiding_style_image=True)
    opt = _opt(**over)
    train = [_batch(opt, 100 + i) for i in range(4)]
    val = [_batch(opt, 200 + i, with_path=True) for i in range(2)]

    def run(validate):
        tm = _manager(opt)
        losses, result = [], None
        for i, b in enumerate(train):
            tm.run_generator_one_step({k: v.clone() for k, v in b.items()})
            tm.run_discriminator_one_step({k: v.clone() for k, v in b.items()})
            losses.append({k: float(v.detach()) for k, v in tm.get_latest_losses().items()})
            if validate and i == 1:
                result = InferenceManager(opt, num_samples=3).run(tm.sr_model, val)
                assert tm.sr_model.training
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in tm.sr_model.state_dict().items()}
        stats = dict(tm.graph_stats)
        tm.close()
        return losses, state, stats, result

    l0, s0, g0, _ = run(False)
    l1, s1, g1, res = run(True)
    assert res["n_samples"] == 4 and math.isfinite(res["psnr/mean"]) and math.isfinite(res["ssim/mean"])
    print("graph stats", g0, g1, "losses of step 4", l0[3])
    assert g0 == g1
    if hip_graphs:
        if variant == "guided":      # (the independent variant's branch coins decide which of its graphs a step replays)
            assert (g0["eager"], g0["captured"], g0["replayed"]) == (2, 2, 4), g0
    else:
        assert g0["captured"] == 0 and g0["replayed"] == 0
    for i in range(4):
        assert l0[i] == l1[i], (i, l0[i], l1[i])
    assert list(s0) == list(s1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
