"""MS-SSIM and the validation loop on the host: the float64 restatement of the reference's msssim (evaluator/ssim.py:24-118)
against tests/golden/ms_ssim/ms_ssim.json (written from the REAL reference by tools/gen_golden_ms_ssim.py), the fixture's own fp32 gap,
the unchanged MetricsEvaluator default, InferenceManager's surface and the argument checks of dsee_ms_ssim.  CPU only."""
import ctypes
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tools.gen_golden_ms_ssim import CASES as GEN_CASES, checksum, images

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ms_ssim", "ms_ssim.json")
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


# ---- the restatement (also loaded by tools/gen_golden_ms_ssim.py, tools/time_ms_ssim.py and tests/test_gpu_ms_ssim.py)
def window64(k, device="cpu"):
    """create_window(k) of the reference, widened: the Gaussian's values are fp32 (gaussian() builds a torch.Tensor), it is
    normalised in float64, and the float64 outer product is rounded to fp32."""
    g = torch.Tensor([math.exp(-(x - k // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(k)]).double()
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().double().to(device)


def ssim64(x, y, dtype=torch.float64):
    """x, y: [3, h, w] on the 0..255 scale.  Returns (sim, cs): the means over positions, then over the three channels."""
    h, w = x.shape[-2:]
    k = min(11, h, w)
    win = window64(k, x.device).to(dtype).view(1, 1, k, k)
    x, y = x.unsqueeze(1), y.unsqueeze(1)                       # channels as the batch of a 1-channel convolution
    mu1, mu2 = F.conv2d(x, win), F.conv2d(y, win)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11 = F.conv2d(x * x, win) - mu1_sq
    s22 = F.conv2d(y * y, win) - mu2_sq
    s12 = F.conv2d(x * y, win) - mu1_mu2
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    v1, v2 = 2.0 * s12 + c2, s11 + s22 + c2
    ssim_map = ((2 * mu1_mu2 + c1) * v1) / ((mu1_sq + mu2_sq + c1) * v2)
    return ssim_map.mean(dim=(1, 2, 3)).mean(), (v1 / v2).mean(dim=(1, 2, 3)).mean()


def msssim64(fake, real, dtype=torch.float64):
    """fake, real: [3, H, W] in [-1, 1] (fp32).  Returns (value, cs[5], sim[5]) as Python floats: msssim(fake255, real255,
    size_average=True, val_range=255) with every operation after the load in `dtype`.  ssim.py:117 is prod(pow1[:-1] *
    pow2[-1]): each of the four cs_l ** w_l is multiplied by sim_4 ** w_4 before the product."""
    x, y = (fake.to(dtype) + 1.0) * 127.5, (real.to(dtype) + 1.0) * 127.5
    weights = torch.FloatTensor(WEIGHTS).to(x.device).to(dtype)
    sims, css = [], []
    for level in range(len(WEIGHTS)):
        sim, cs = ssim64(x, y, dtype)
        sims.append(sim)
        css.append(cs)
        if level + 1 < len(WEIGHTS):      # (the reference pools a sixth, unused level as well: it raises for H or W < 32)
            x, y = F.avg_pool2d(x, (2, 2)), F.avg_pool2d(y, (2, 2))
    sims, css = torch.stack(sims), torch.stack(css)
    pow1, pow2 = css ** weights, sims ** weights
    value = torch.prod(pow1[:-1] * pow2[-1])
    return float(value), [float(v) for v in css], [float(v) for v in sims]


def fixture():
    with open(GOLD) as f:
        return json.load(f)["cases"]


def fixture_gap(cases):
    """g = max |ref - f64| over the finite samples of the fixture: what the reference's fp32 arithmetic costs."""
    return max(abs(r - v) for c in cases.values() for r, v in zip(c["ref"], c["f64"]) if math.isfinite(v))


# ---- 1 + 2: the fixture
def test_fixture_covers_the_generator_cases():
    cases = fixture()
    assert sorted(cases) == sorted(GEN_CASES)
    for name, c in cases.items():
        assert {k: c[k] for k in ("H", "W", "N", "kind", "seed")} == GEN_CASES[name], name
        assert len(c["ref"]) == len(c["f64"]) == len(c["cs"]) == len(c["sim"]) == c["N"]
    nan = [n for n, c in cases.items() if any(math.isnan(v) for v in c["ref"])]
    assert nan == ["indep_32_s2"], nan
    sizes = {(c["H"], c["W"]) for c in cases.values()}
    assert {(32, 32), (256, 256), (512, 512), (48, 80), (80, 48)} <= sizes and any(c["N"] == 3 for c in cases.values())


@pytest.mark.parametrize("name", sorted(GEN_CASES))
def test_float64_restatement_reproduces_the_fixture(name):
    c = fixture()[name]
    fake, real = images(c)
    assert checksum(fake) == c["checksum"]["fake"] and checksum(real) == c["checksum"]["real"], "the recipe drifted"
    for i in range(c["N"]):
        val, cs, sim = msssim64(fake[i], real[i])
        print(name, i, "f64", val, "fixture", c["f64"][i], "ref", c["ref"][i])
        for got, want in zip(cs + sim, c["cs"][i] + c["sim"][i]):
            assert abs(got - want) <= 1e-10, (name, i, got, want)
        if math.isnan(c["f64"][i]):
            assert math.isnan(val) and math.isnan(c["ref"][i])
            assert min(cs[:4] + [sim[4]]) <= -0.05
        else:
            assert abs(val - c["f64"][i]) <= 1e-10, (name, i, val, c["f64"][i])
            assert min(cs[:4] + [sim[4]]) >= 0.05


def test_fixture_gap_between_reference_and_float64():
    g = fixture_gap(fixture())
    print("fixture gap g = max |ref - f64| = %.3e" % g)
    assert g < 1e-5


# ---- 3: defaults, surface, argument checks
def test_metrics_evaluator_default_is_unchanged():
    from deepsee_amd.metrics import MetricsEvaluator
    assert MetricsEvaluator.columns == ["ID", "PSNR", "SSIM", "RMSE"]
    m = MetricsEvaluator()
    assert m.columns == ["ID", "PSNR", "SSIM", "RMSE"] and m.ms_ssim is False
    m.psnr_buffer, m.ssim_buffer, m.rmse_buffer, m.n_samples = [30.0, 32.0], [0.9, 0.8], [0.1, 0.2], 2
    res = m.get_result()
    assert list(res) == ["psnr/mean", "ssim/mean", "rmse/mean", "psnr/std", "ssim/std", "rmse/std", "n_samples"]
    assert res["psnr/mean"] == 31.0 and res["n_samples"] == 2


def test_metrics_evaluator_with_ms_ssim_keys_and_columns(tmp_path):
    from deepsee_amd.metrics import MetricsEvaluator
    m = MetricsEvaluator(write_details=True, folder_out=str(tmp_path), ms_ssim=True)
    assert m.columns == ["ID", "PSNR", "SSIM", "MSSSIM", "RMSE"] and MetricsEvaluator.columns == ["ID", "PSNR", "SSIM", "RMSE"]
    assert m.ms_ssim_buffer == []
    m.psnr_buffer, m.ssim_buffer, m.ms_ssim_buffer, m.rmse_buffer, m.n_samples = [30.0], [0.9], [0.95], [0.1], 1
    assert list(m.get_result()) == ["psnr/mean", "ssim/mean", "ms_ssim/mean", "rmse/mean", "psnr/std", "ssim/std",
                                    "ms_ssim/std", "rmse/std", "n_samples"]
    m.clear()
    assert m.ms_ssim_buffer == [] and m.psnr_buffer == [] and m.n_samples == 0
    assert open(os.path.join(str(tmp_path), "metrics.csv")).read().split() == ["ID,PSNR,SSIM,MSSSIM,RMSE"]


def test_inference_manager_surface():
    from deepsee_amd.managers import BaseManager, InferenceManager
    from deepsee_amd.options import make_opt
    opt = make_opt("independent_8x_32", batchSize=2, ngf=8)
    im = InferenceManager(opt, num_samples=5)
    assert isinstance(im, BaseManager) and not hasattr(im, "sr_model")        # builds no model
    assert im.num_samples == 5 and im.batch_size == 2 and im.metrics.ms_ssim is True
    assert im.metrics.columns == ["ID", "PSNR", "SSIM", "MSSSIM", "RMSE"]
    with pytest.raises(NotImplementedError):
        InferenceManager(opt, num_samples=5, save_images=True)


def test_ms_ssim_entry_points_validate_before_they_launch():
    from deepsee_amd import lib as L
    so = L.lib()
    # pure host function: pyramids of both images (levels 1..4, float64, 3 planes) + 2 doubles per 16x16-position tile
    n, h, w = 2, 32, 48
    pyr = sum(n * 3 * (h >> l) * (w >> l) for l in range(1, 5))
    tiles = 0
    for l in range(5):
        hl, wl = h >> l, w >> l
        k = min(11, hl, wl)
        tiles += n * 3 * (-(-(hl - k + 1) // 16)) * (-(-(wl - k + 1) // 16))
    assert so.dsee_ms_ssim_workspace(n, h, w) == (2 * pyr + 2 * tiles) * 8
    assert so.dsee_ms_ssim_workspace(8, 512, 512) > so.dsee_ms_ssim_workspace(8, 256, 256) > 0
    ws = so.dsee_ms_ssim_workspace(1, 16, 16)
    one = ctypes.c_void_p(64)        # a non-null address that is never dereferenced: the checks come before any launch
    assert so.dsee_ms_ssim(None, None, 1, 16, 16, 3, None, ws, None, None) == -1
    assert b"argument check failed" in so.dsee_last_error()
    for args in [(one, one, 1, 15, 16, 3, one, 1 << 20, one), (one, one, 1, 16, 15, 3, one, 1 << 20, one),
                 (one, one, 1, 16, 16, 2, one, ws, one), (one, one, 0, 16, 16, 3, one, ws, one),
                 (one, one, 1, 16, 16, 3, one, ws - 8, one)]:
        assert so.dsee_ms_ssim(*args, None) == -1, args
        assert b"argument check failed" in so.dsee_last_error()
