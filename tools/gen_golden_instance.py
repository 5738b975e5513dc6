"""Golden fixtures of the InstanceNorm generator (norm_G = spectral{spade,latesean}instance3x3), pinned against the real
reference the way oracle/gen_golden.py pins the BatchNorm cases, without editing the oracle:

  * the oracle's param-free norm (deepsee_oracle.batch_norm_train) is replaced by F.instance_norm (eps 1e-5, no running
    statistics, batch statistics in train and eval alike: normalization.py:84-85 nn.InstanceNorm2d(affine=False));
  * the SR net's `param_free_norm.*` buffers are dropped from deepsee_oracle.net_specs, so that the recipe state and the key
    set run_case asserts against are the reference's InstanceNorm model.

Then gen_golden.run_case drives reference and oracle on each case (inference, encode_only, demo, one G+D step, post-step
state) and writes the reference's numbers; they are kept in tests/golden/instance/<case>.json (a directory of their own: the
BatchNorm oracle of tests/test_oracle_golden.py checks every tests/golden/*.json).  Needs the reference sources (gen_golden.REF), so it
runs where oracle/gen_golden.py runs; the tests read only the written fixtures.

    python tools/gen_golden_instance.py            # all cases
    python tools/gen_golden_instance.py case_name  # one case
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import deepsee_oracle as O  # noqa: E402
from oracle import gen_golden as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "instance")

CASES = {
    # SPADE head + SEAN blocks (the default topology with InstanceNorm), independent 8x
    "indep_instance_4to32_bs2_ngf8": dict(opt=dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8,
                                                   norm_G="spectrallateseaninstance3x3"), n=2, seed=21, iters=1),
    # PureSEAN tail above max_fm_size (the capped path); a seed whose D step stays above the reference's own noise floor
    # (run_case's post-step state bounds)
    "puresean_instance_4to128_bs2_ngf4": dict(opt=dict(start_size=4, crop_size=128, load_size=512, batchSize=2, ngf=4,
                                                       add_noise=False, max_fm_size=64,
                                                       norm_G="spectrallateseaninstance3x3"), n=2, seed=28, iters=1),
    # SPADE-only generator
    "spade_instance_4to32_bs2_ngf8": dict(opt=dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8,
                                                   norm_G="spectralspadeinstance3x3"), n=2, seed=23, iters=1),
}


def instance_norm_train(x, st, prefix, training):
    """nn.InstanceNorm2d(affine=False, track_running_stats=False): per image and channel, biased variance + eps."""
    return F.instance_norm(x, eps=O.BN_EPS)


def install_instance_norm(setattr_=setattr):
    """Substitute the oracle's param-free norm and state layout (setattr_: pytest's monkeypatch.setattr in the tests)."""
    specs = O.net_specs

    def net_specs(opt):
        out = specs(opt)
        out["SR"] = type(out["SR"])((k, v) for k, v in out["SR"].items() if ".param_free_norm." not in k)
        return out

    setattr_(O, "batch_norm_train", instance_norm_train)
    setattr_(O, "net_specs", net_specs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    assert os.path.isdir(G.REF), "needs the reference sources (%s)" % G.REF
    G.install_torchvision_stub()
    sys.path.insert(0, G.REF)
    torch.set_num_threads(8)
    install_instance_norm()
    for name, spec in CASES.items():
        if a.cases and name not in a.cases:
            continue
        G.run_case(name, spec)
        os.makedirs(OUT, exist_ok=True)
        os.replace(os.path.join(ROOT, "tests", "golden", name + ".json"), os.path.join(OUT, name + ".json"))


if __name__ == "__main__":
    main()
