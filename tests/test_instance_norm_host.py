"""InstanceNorm SPADE / SEAN / PureSEAN (opt.norm_G = spectral{spade,sean,latesean}instance3x3) on the host: the norm_G
parser, the module layout it selects, and the InstanceNorm form of the oracle against fixtures written from the REAL
reference by tools/gen_golden_instance.py (tests/golden/instance/*.json).  CPU only."""
import glob
import json
import os

import pytest

from deepsee_amd import networks as N
from deepsee_amd.options import PRESETS, make_opt
from deepsee_amd.sr_model import block_plan
from oracle import deepsee_oracle as O
from tools.gen_golden_instance import install_instance_norm

INST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance")
CASES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(INST, "*.json")))


@pytest.mark.parametrize("norm_G,want", [
    ("spectralspadeinstance3x3", "instance"), ("spectralseaninstance3x3", "instance"),
    ("spectrallateseaninstance3x3", "instance"),
    ("spectralspadebatch3x3", "batch"), ("spectralseanbatch3x3", "batch"), ("spectrallateseanbatch3x3", "batch"),
    ("spectralspadesyncbatch3x3", "batch"), ("spectralseansyncbatch3x3", "batch"),
    ("spectrallateseansyncbatch3x3", "batch")])
def test_norm_G_parses_like_the_reference(norm_G, want):
    assert N.param_free_norm_of(norm_G) == want
    block_plan(make_opt(norm_G=norm_G))      # (block_plan validates norm_G too)


@pytest.mark.parametrize("norm_G", ["spectralspadegroup3x3", "spectrallateseanlayer3x3", "spectralinstance", "spectral",
                                    "spectralspadefoobatch3x3", "spectralspadeinstancebatch3x3", "spectralseanbatchinstance3x3"])
def test_unknown_norm_G_raises_value_error(norm_G):
    with pytest.raises(ValueError):
        N.param_free_norm_of(norm_G)
    with pytest.raises(ValueError):
        block_plan(make_opt(norm_G=norm_G))


@pytest.mark.parametrize("norm_G", ["spectralspadebatch5x5", "spectrallateseaninstance5x5", "spadesyncbatch3x3",
                                    "lateseaninstance3x3"])
def test_unimplemented_norm_G_raises(norm_G):
    """A SPADE kernel size other than 3 and a generator without spectral norm are refused, not silently replaced."""
    with pytest.raises(NotImplementedError):
        N.param_free_norm_of(norm_G)
    with pytest.raises(NotImplementedError):
        block_plan(make_opt(norm_G=norm_G))


@pytest.mark.parametrize("preset", [None] + sorted(PRESETS))
def test_presets_keep_batch_norm(preset):
    opt = make_opt(preset)
    assert N.param_free_norm_of(opt.norm_G) == "batch"
    sr = N.DeepSEESR(opt, block_plan(opt))
    norms = [m for m in sr.modules() if isinstance(m, N.SpadeNorm)]
    assert norms and all(m.norm == "batch" and isinstance(m.param_free_norm, N.BNStats) for m in norms)


@pytest.mark.parametrize("case", CASES)
def test_instance_state_dict_is_the_reference_key_set(case):
    """SR keys/shapes == the reference InstanceNorm model's (the fixture's post-step state was read from it): no
    param_free_norm buffers; D and E unchanged."""
    rec = json.load(open(os.path.join(INST, case + ".json")))
    opt = make_opt(**rec["opt"])
    ref_keys = {k.split("/", 1)[1] for k in rec["iters"][0]["state_norms"] if k.startswith("SR/")}
    sr = N.DeepSEESR(opt, block_plan(opt))
    got = set(sr.state_dict())
    assert got == ref_keys, got ^ ref_keys
    assert not any("param_free_norm" in k for k in got)
    assert all(m.norm == "instance" and m.param_free_norm is None for m in sr.modules() if isinstance(m, N.SpadeNorm))


def test_instance_fixtures_present():
    assert {"indep_instance_4to32_bs2_ngf8", "puresean_instance_4to128_bs2_ngf4"} <= set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_instance_oracle_matches_reference_fixture(case, monkeypatch):
    """The InstanceNorm-substituted oracle (the yardstick of tests/test_gpu_instance_norm.py) reproduces the reference's
    inference / encode_only / demo outputs, G+D step losses, gradients and post-step state, with the bounds of
    tests/test_oracle_golden.py."""
    from tests import test_oracle_golden as TG
    install_instance_norm(monkeypatch.setattr)
    monkeypatch.setattr(TG, "GOLD", INST)
    rec = json.load(open(os.path.join(INST, case + ".json")))
    spec = O.net_specs(O.make_opt(**rec["opt"]))["SR"]
    assert not any("param_free_norm" in k for k in spec)
    TG.test_oracle_matches_reference_fixture(case)
