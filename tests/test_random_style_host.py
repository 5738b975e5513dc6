"""opt.random_style_matrix on the host: the substituted oracle (tools/gen_golden_random_style.py) against fixtures written from the
REAL reference (tests/golden/random_style/*.json), its refusal of combinedstyle, the encoder's state-dict layout, the eval-stream
keys, and the three new entry points (declared, exported, bound, validating before they launch).  CPU only."""
import ctypes
import glob
import json
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import deepsee_oracle as O
from tools.gen_golden_random_style import CASES as GEN_CASES, ENCODE_ONLY_SEED, install_random_style

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_style")
CASES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLD, "*.json")))
SMALL = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)


def test_fixtures_present():
    assert CASES == sorted(GEN_CASES) and len(CASES) == 2, CASES
    recs = [json.load(open(os.path.join(GOLD, c + ".json"))) for c in CASES]
    assert all(r["opt"]["random_style_matrix"] and r["opt"]["netE"] == "fullstyle" for r in recs)
    assert sorted(bool(r["opt"].get("guiding_style_image", False)) for r in recs) == [False, True]
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLD, c + ".json")) < 128 * 1024


@pytest.mark.parametrize("case", CASES)
def test_random_style_oracle_matches_reference_fixture(case, monkeypatch):
    """The substituted oracle (the yardstick of tests/test_gpu_random_style.py) reproduces the reference's inference /
    encode_only / demo outputs, G+D step losses, gradients and post-step state with the bounds of tests/test_oracle_golden.py;
    encode_only is reseeded as the tool reseeds both sides."""
    from tests import test_oracle_golden as TG
    install_random_style(monkeypatch.setattr)
    monkeypatch.setattr(TG, "GOLD", GOLD)
    TG.test_oracle_matches_reference_fixture(case)


def test_unsubstituted_oracle_misses_the_fixtures():
    """The fixtures pin the label-masked noise input: the plain oracle, which feeds the RGB image to a label_nc-channel
    convolution, cannot even run them."""
    rec = json.load(open(os.path.join(GOLD, CASES[0] + ".json")))
    opt = O.make_opt(**rec["opt"])
    orc = O.Oracle(opt, O.recipe_state(opt, gain=1.0))
    with pytest.raises(RuntimeError):
        orc.inference(O.synthetic_batch(opt, rec["n"], seed=rec["batch_seed"]))


def test_substituted_input_is_the_masked_draw(monkeypatch):
    """The wrapped encoder_forward draws (N, label_nc, crop, crop) under the tag 'style_field' before anything else and feeds
    draw * seg; encode_only restarts torch's generator at ENCODE_ONLY_SEED; without the flag nothing changes."""
    install_random_style(monkeypatch.setattr)
    opt = O.make_opt(**dict(SMALL, netE="fullstyle", noisy_style_scale=0.05, random_style_matrix=True))
    states = O.recipe_state(opt, gain=1.0)
    batch = O.synthetic_batch(opt, 2, seed=3)
    ctl = O.RecordingCtl()
    orc = O.Oracle(opt, states, ctl)
    torch.manual_seed(1)
    s1 = orc.encode_only({k: v.clone() for k, v in batch.items()})
    torch.manual_seed(2)
    s2 = orc.encode_only({k: v.clone() for k, v in batch.items()})
    assert torch.equal(s1, s2)
    assert [(k, t, tuple(v.shape)) for k, t, v in ctl.tape] == [("normal", "style_field", (2, 19, 32, 32))] * 2
    torch.manual_seed(ENCODE_ONLY_SEED)
    assert torch.equal(ctl.tape[0][2], torch.empty(2, 19, 32, 32).normal_())
    # the same numbers from the restated first layer on draw * seg
    data = orc.preprocess({k: v.clone() for k, v in batch.items()})
    seg = data["input_semantics"]
    w = O.spectral_weight(orc.S["E"], "initial.0.0", False)
    x = F.conv2d(ctl.tape[0][2] * seg, w, None, padding=1)
    assert tuple(x.shape) == (2, opt.nef, 32, 32) and bool((ctl.tape[0][2] * seg).ne(0).sum(1).le(1).all())
    plain = O.make_opt(**dict(SMALL, netE="fullstyle", noisy_style_scale=0.05))
    ctl2 = O.RecordingCtl()
    O.Oracle(plain, O.recipe_state(plain, gain=1.0), ctl2).encode_only({k: v.clone() for k, v in batch.items()})
    assert ctl2.tape == []


def test_install_random_style_refuses_combinedstyle(monkeypatch):
    install_random_style(monkeypatch.setattr)
    opt = O.make_opt(**dict(SMALL, netE="combinedstyle", random_style_matrix=True, full_style_image=True))
    orc = O.Oracle(opt, O.recipe_state(opt, gain=1.0))
    with pytest.raises(ValueError, match="random_style_matrix needs netE='fullstyle'.*encoder.py:197-198"):
        orc.inference(O.synthetic_batch(opt, 2, seed=3))


def test_e_spec_of_the_variant():
    opt = O.make_opt(**dict(SMALL, netE="fullstyle", random_style_matrix=True))
    spec = O.e_spec(opt)
    assert tuple(spec["initial.0.0.weight_orig"]) == (opt.nef, opt.label_nc, 3, 3)
    assert tuple(spec["initial.0.0.weight_v"]) == (opt.label_nc * 9,) and tuple(spec["initial.0.0.weight_u"]) == (opt.nef,)
    assert tuple(spec["down0.0.0.weight_orig"]) == (2 * opt.nef, opt.nef, 3, 3)
    rgb = O.e_spec(O.make_opt(**dict(SMALL, netE="fullstyle")))
    assert tuple(rgb["initial.0.0.weight_orig"]) == (opt.nef, 3, 3, 3) and set(rgb) == set(spec)


def test_option_default_and_eval_stream_keys():
    from deepsee_amd import networks as N
    from deepsee_amd.options import DEFAULTS
    assert DEFAULTS["random_style_matrix"] is False
    keys = {N.eval_stream_seed(s, p) for s in range(64) for p in (False, True)}
    assert len(keys) == 128 and all(0 <= k < 1 << 64 for k in keys)
    assert N.eval_stream_seed(17, False) == N.eval_stream_seed(17, False) != 17


def test_entry_points_are_declared_exported_and_bound():
    from deepsee_amd import lib as L
    protos = L.header_prototypes()
    so = L.lib()
    p, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    want = {"dsee_onehot_noise_conv3x3_fwd": (ctypes.c_int, [p, p, u, u, i, p, p, p] + [i] * 5 + [p]),
            "dsee_onehot_noise_conv3x3_wgrad_workspace": (ctypes.c_size_t, [i] * 5),
            "dsee_onehot_noise_conv3x3_wgrad": (ctypes.c_int, [p, p, u, u, i, p] + [i] * 5 + [p, p, p, p])}
    for name, proto in want.items():
        assert protos[name] == proto, name
        fn = getattr(so, name)
        assert fn.restype is proto[0] and list(fn.argtypes) == proto[1]


def test_entry_points_validate_before_they_launch():
    """Bad arguments are refused with DSEE_EINVAL and a message before any HIP call (so this runs without a GPU)."""
    from deepsee_amd import lib as L
    so = L.lib()
    one = ctypes.c_void_p(64)        # a non-null, 16-byte aligned address that is never dereferenced

    def fwd(**kw):
        a = dict(lab=one, field=one, seed=0, offset=0, use_epoch=0, table=one, bias=None, out=one, N=2, H=8, W=8, L=19, Co=32)
        assert set(kw) <= set(a)
        a.update(kw)
        return so.dsee_onehot_noise_conv3x3_fwd(*a.values(), None)

    def wgrad(**kw):
        a = dict(lab=one, field=one, seed=0, offset=0, use_epoch=0, dout=one, N=2, H=8, W=8, L=19, Co=32, dw=one, db=None,
                 ws=one)
        assert set(kw) <= set(a)
        a.update(kw)
        return so.dsee_onehot_noise_conv3x3_wgrad(*a.values(), None)

    for bad in (dict(lab=None), dict(table=None), dict(out=None), dict(Co=30), dict(Co=36), dict(Co=0), dict(L=33), dict(L=0),
                dict(N=0), dict(H=0), dict(W=-1), dict(L=32, Co=64), dict(N=1 << 11, H=1 << 10, W=1 << 10)):
        assert fwd(**bad) != 0, bad
        assert b"argument check failed" in so.dsee_last_error(), bad
    for bad in (dict(lab=None), dict(dout=None), dict(dw=None), dict(ws=None), dict(Co=30), dict(Co=116), dict(L=33),
                dict(N=0), dict(N=1 << 11, H=1 << 10, W=1 << 10)):
        assert wgrad(**bad) != 0, bad
        assert b"argument check failed" in so.dsee_last_error(), bad
    # one partial [9 L + 1][Co] per 16 x 32 tile, at most 512 of them
    ws = so.dsee_onehot_noise_conv3x3_wgrad_workspace
    assert ws(1, 5, 7, 19, 8) == 172 * 8 * 4 and ws(2, 40, 40, 19, 32) == 2 * 3 * 2 * 172 * 32 * 4
    assert ws(8, 256, 256, 19, 32) == 512 * 172 * 32 * 4 and ws(0, 8, 8, 19, 32) == 0
