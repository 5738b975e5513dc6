"""Discriminator / style-encoder norms (opt.norm_D, opt.norm_E = spectral{instance,batch,sync_batch,none}) on the host: the
parser, the module layouts it selects, BatchNorm initialisation, and the substituted oracle against fixtures written from
the REAL reference by tools/gen_golden_nonspade_norm.py (tests/golden/nonspade_norm/*.json).  CPU only."""
import glob
import json
import os

import pytest
import torch

from deepsee_amd import networks as N
from deepsee_amd.options import PRESETS, make_opt
from deepsee_amd.sr_model import init_weights
from oracle import deepsee_oracle as O
from tools.gen_golden_nonspade_norm import install_nonspade_norm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nonspade_norm")
CASES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLD, "*.json")))


@pytest.mark.parametrize("norm_type,want", [
    ("spectralinstance", "instance"), ("spectralbatch", "batch"), ("spectralsync_batch", "sync_batch"),
    ("spectralnone", "none"), ("spectral", "none")])
def test_nonspade_norm_parses_like_the_reference(norm_type, want):
    assert N.nonspade_norm_of(norm_type) == want


@pytest.mark.parametrize("norm_type", ["spectralsyncbatch", "spectralgroup", "spectralinstancebatch", "spectralBatch"])
def test_unknown_subtype_raises_like_the_reference(norm_type):
    with pytest.raises(ValueError, match="normalization layer .* is not recognized"):
        N.nonspade_norm_of(norm_type)


@pytest.mark.parametrize("norm_type", ["batch", "instance", "none", "sync_batch", ""])
def test_value_without_spectral_raises_value_error(norm_type):
    with pytest.raises(ValueError, match=repr(norm_type)):
        N.nonspade_norm_of(norm_type)


@pytest.mark.parametrize("which", ["norm_D", "norm_E"])
def test_models_refuse_an_unknown_norm(which):
    opt = make_opt(**{which: "spectralsyncbatch"})
    with pytest.raises(ValueError):
        (N.MultiscaleDiscriminator if which == "norm_D" else N.StyleEncoder)(opt)


@pytest.mark.parametrize("preset", [None] + sorted(PRESETS))
def test_presets_keep_instance_norm_with_todays_keys(preset):
    opt = make_opt(preset)
    assert opt.norm_D == opt.norm_E == "spectralinstance"
    d, e = N.MultiscaleDiscriminator(opt), N.StyleEncoder(opt)
    assert d.per_sample and e.norm == "instance"
    ospec = O.net_specs(O.make_opt(**{k: getattr(opt, k) for k in PRESETS.get(preset, {})}))
    for net, got in (("D", d.state_dict()), ("E", e.state_dict())):
        assert {k: tuple(v.shape) for k, v in got.items()} == dict(ospec[net])
    assert not any(isinstance(m, N.BatchNormP) for m in list(d.modules()) + list(e.modules()))


def test_fixtures_present():
    assert len(CASES) == 4, CASES


def _ref_state(rec, net):
    return {k.split("/", 1)[1] for k in rec["iters"][0]["state_norms"] if k.startswith(net + "/")}


@pytest.mark.parametrize("case", CASES)
def test_d_and_e_state_dicts_are_the_reference_layout(case, monkeypatch):
    """D / E keys == the reference model's (read from it after the step) and shapes == the reference layout for every
    norm_D / norm_E value of the fixtures."""
    rec = json.load(open(os.path.join(GOLD, case + ".json")))
    opt = make_opt(**rec["opt"])
    d, e = N.MultiscaleDiscriminator(opt), N.StyleEncoder(opt)
    assert set(d.state_dict()) == _ref_state(rec, "D"), set(d.state_dict()) ^ _ref_state(rec, "D")
    assert set(e.state_dict()) == _ref_state(rec, "E"), set(e.state_dict()) ^ _ref_state(rec, "E")
    install_nonspade_norm(monkeypatch.setattr)
    spec = O.net_specs(O.make_opt(**rec["opt"]))
    for net, m in (("D", d), ("E", e)):
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(spec[net])
        assert m.state_dict()[next(k for k in spec[net] if k.endswith("weight_u"))].dtype == torch.float32
    assert d.per_sample == (N.nonspade_norm_of(opt.norm_D) == "none")
    if N.nonspade_norm_of(opt.norm_D) == "batch":
        assert all(v.dtype == torch.long and v.dim() == 0
                   for k, v in d.state_dict().items() if k.endswith("num_batches_tracked"))


def test_batch_norm_init_statistics():
    opt = make_opt(norm_D="spectralbatch", norm_E="spectralsync_batch", init_variance=0.02)
    gen = torch.Generator().manual_seed(0)
    for net in (N.MultiscaleDiscriminator(opt), N.StyleEncoder(opt)):
        init_weights(net, opt.init_type, opt.init_variance, gen)
        bns = [m for m in net.modules() if isinstance(m, N.BatchNormP)]
        assert bns
        w = torch.cat([m.weight.detach() for m in bns])
        assert abs(float(w.mean()) - 1.0) < 0.01 and abs(float(w.std()) - 0.02) < 0.005, (float(w.mean()), float(w.std()))
        for m in bns:
            assert not m.bias.any() and not m.running_mean.any() and bool((m.running_var == 1).all())
            assert int(m.num_batches_tracked) == 0


def test_none_keeps_a_zero_initialised_conv_bias():
    opt = make_opt(norm_D="spectralnone", norm_E="spectralnone")
    gen = torch.Generator().manual_seed(0)
    for net in (N.MultiscaleDiscriminator(opt), N.StyleEncoder(opt)):
        with torch.no_grad():
            for p in net.parameters():
                p.fill_(3.0)
        init_weights(net, opt.init_type, opt.init_variance, gen)
        biases = [m.bias for m in net.modules() if isinstance(m, N.SNConvP)]
        assert biases and all(b is not None and not b.any() for b in biases)


@pytest.mark.parametrize("case", CASES)
def test_nonspade_oracle_matches_reference_fixture(case, monkeypatch):
    """The substituted oracle (the yardstick of tests/test_gpu_nonspade_norm.py) reproduces the reference's inference /
    encode_only / demo outputs, G+D step losses, gradients and post-step state (running statistics included), with the
    bounds of tests/test_oracle_golden.py."""
    from tests import test_oracle_golden as TG
    install_nonspade_norm(monkeypatch.setattr)
    monkeypatch.setattr(TG, "GOLD", GOLD)
    TG.test_oracle_matches_reference_fixture(case)
