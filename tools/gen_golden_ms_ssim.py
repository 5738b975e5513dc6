"""Golden fixture of MS-SSIM (dsee_ms_ssim, deepsee_amd.metrics.ms_ssim), pinned against the real reference:

  * the reference's evaluator/ssim.py is loaded BY FILE PATH (it imports only torch; the evaluator package's __init__ chain,
    with LPIPS / skimage behind it, is never imported) and msssim(fake255[i:i+1], real255[i:i+1], size_average=True,
    val_range=255) is evaluated per sample exactly as MetricsEvaluator.collect_samples does (evaluation.py:114,125-127);
  * the float64 restatement kept in tests/test_ms_ssim_host.py (msssim64) gives the value and the per-level cs / sim terms.

Per case tests/golden/ms_ssim/ms_ssim.json (a directory of its own: tests/test_oracle_golden.py takes every tests/golden/*.json
for a model case) holds the recipe (H, W, N, kind, seed), a float64 checksum of both images (sum and sum of
squares), the reference's fp32 result `ref` and the restatement's `f64`, `cs[5]`, `sim[5]`, one entry per sample.  The images
themselves are not stored: `images(case)` below rebuilds them from seeded torch.Generator draws, nearest upsampling and
elementwise operations only, and the tests assert the checksums before anything else.

The generator refuses to write unless, in every finite case, each of cs_0..cs_3 and sim_4 is >= 0.05 (no rounding can flip a
sign into NaN), and exactly one case ("indep") is NaN in the reference with a negative term <= -0.05.

    python tools/gen_golden_ms_ssim.py        # needs the reference sources (oracle.gen_golden.REF)

`CASES` and `images` are imported by the tests and by tools/time_ms_ssim.py; that needs no reference."""
import importlib.util
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "ms_ssim", "ms_ssim.json")
MARGIN = 0.05

# kind: real = blocky base (uniform draws, nearest-upsampled x8) + 0.05 Gaussian noise, clamped to [-1, 1];
#   noise<s>: fake = clamp(real + s * Gaussian noise);  blur: fake = real 2x2-averaged and nearest-upsampled;
#   indep: fake and real two independent uniform images (the deliberately-NaN case)
CASES = {}
for _size in (32, 256, 512):
    for _kind in ("noise0.1", "noise0.5", "blur"):
        for _seed in (1, 2, 3):
            CASES["%s_%d_s%d" % (_kind, _size, _seed)] = dict(H=_size, W=_size, N=1, kind=_kind, seed=_seed)
CASES["noise0.1_48x80_s1"] = dict(H=48, W=80, N=1, kind="noise0.1", seed=1)
CASES["blur_48x80_s2"] = dict(H=48, W=80, N=1, kind="blur", seed=2)
CASES["noise0.1_80x48_s3"] = dict(H=80, W=48, N=1, kind="noise0.1", seed=3)
CASES["noise0.5_64_n3_s4"] = dict(H=64, W=64, N=3, kind="noise0.5", seed=4)
CASES["blur_128_n3_s5"] = dict(H=128, W=128, N=3, kind="blur", seed=5)
# (no case below 32: the reference pools once more after its fifth level and raises on the empty result for 16 <= H, W < 32,
#  although its value does not depend on that pooling; the GPU test holds 16 x 16 against the restatement alone)
CASES["indep_32_s2"] = dict(H=32, W=32, N=1, kind="indep", seed=2)


def images(case):
    """(fake, real): fp32 NCHW [N, 3, H, W] in [-1, 1] on the CPU, bit-identical wherever torch's CPU generator is."""
    n, h, w, kind = case["N"], case["H"], case["W"], case["kind"]
    g = torch.Generator().manual_seed(1000 + case["seed"])
    if kind == "indep":
        return (torch.rand(n, 3, h, w, generator=g) * 2 - 1), (torch.rand(n, 3, h, w, generator=g) * 2 - 1)
    assert h % 8 == 0 and w % 8 == 0
    low = torch.rand(n, 3, h // 8, w // 8, generator=g) * 1.6 - 0.8
    base = low.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)
    real = (base + 0.05 * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1)
    if kind.startswith("noise"):
        fake = (real + float(kind[5:]) * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1)
    elif kind == "blur":
        small = (((real[..., 0::2, 0::2] + real[..., 0::2, 1::2]) + real[..., 1::2, 0::2]) + real[..., 1::2, 1::2]) * 0.25
        fake = small.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    else:
        raise ValueError(kind)
    return fake.contiguous(), real.contiguous()


def checksum(t):
    """[sum, sum of squares] of an fp32 tensor in float64, correctly rounded (math.fsum; the squares of fp32 values are exact
    in float64): the same bits on every machine, whatever order its reductions run in."""
    d = t.double().flatten()
    return [math.fsum(d.tolist()), math.fsum((d * d).tolist())]


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def host_test_module():
    """tests/test_ms_ssim_host.py, which keeps the float64 restatement (msssim64) and the fixture's readers."""
    return load_by_path("_ms_ssim_host_restatement", os.path.join(ROOT, "tests", "test_ms_ssim_host.py"))


def main():
    from oracle import gen_golden as G
    path = os.path.join(G.REF, "evaluator", "ssim.py")
    assert os.path.isfile(path), "needs the reference sources (%s)" % G.REF
    ref_ssim = load_by_path("_reference_ssim", path)
    msssim64 = host_test_module().msssim64
    torch.set_num_threads(8)
    out, n_nan = {}, 0
    for name, case in CASES.items():
        fake, real = images(case)
        rec = dict(case, checksum={"fake": checksum(fake), "real": checksum(real)}, ref=[], f64=[], cs=[], sim=[])
        f255, r255 = (fake + 1.0) * 127.5, (real + 1.0) * 127.5            # MetricsEvaluator._to255, fp32
        for i in range(case["N"]):
            ref = float(ref_ssim.msssim(f255[i].unsqueeze(0), r255[i].unsqueeze(0), size_average=True, val_range=255))
            val, cs, sim = msssim64(fake[i], real[i])
            terms = cs[:4] + [sim[4]]
            if case["kind"] == "indep":
                assert math.isnan(ref) and math.isnan(val), (name, ref, val)
                assert min(terms) <= -MARGIN, "%s: the negative term %r is not <= -%g; pick another seed" % (name, terms, MARGIN)
                n_nan += 1
            else:
                assert math.isfinite(ref) and math.isfinite(val), (name, ref, val)
                assert min(terms) >= MARGIN, "%s: a term of %r is below %g: drop or change the case" % (name, terms, MARGIN)
            rec["ref"].append(ref)
            rec["f64"].append(val)
            rec["cs"].append(cs)
            rec["sim"].append(sim)
            print("%-22s %d ref %.9f f64 %.12f |d| %.2e min term %.4f" % (name, i, ref, val, abs(ref - val), min(terms)))
        out[name] = rec
    assert n_nan == 1, "exactly one NaN case expected, got %d" % n_nan
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"margin": MARGIN, "cases": out}, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
