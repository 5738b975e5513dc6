"""The explorative inference modes on the host (deepsee_amd.explore): the style rule in plain torch ops against the applied
styles the REAL reference fed its generator (tests/golden/explore/*.json, written by tools/gen_golden_explore.py), the two new
C-ABI entry points and their argument checks, the option defaults.  CPU only."""
import ctypes
import glob
import json
import os
from types import SimpleNamespace

import pytest
import torch

from tools import gen_golden_explore as G

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "explore")
CASES = sorted(G.CASES)


load = G.load


def test_a_fixture_per_group_and_none_larger_than_the_largest_before():
    groups = sorted({G.group_of(c) for c in CASES})
    assert sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLD, "*.json"))) == groups
    modes = {load(c)["mode"] for c in CASES}
    from deepsee_amd import explore
    assert modes == set(explore.MODES)
    for g in groups:
        assert os.path.getsize(os.path.join(GOLD, g + ".json")) <= 134859, g      # tests/golden/host_logic.json
        with open(os.path.join(GOLD, g + ".json")) as f:
            assert sorted(json.load(f)["runs"]) == sorted(c for c in CASES if G.group_of(c) == g)


@pytest.mark.parametrize("case", CASES)
def test_torch_rule_reproduces_the_references_applied_styles(case):
    """style_variants_torch on the fixture's encoded styles, the mode's coefficients and the stored noise gives, bit for bit, the
    style matrices the reference handed to its generator."""
    from deepsee_amd import explore
    from deepsee_amd.options import make_opt
    rec = load(case)
    opt = make_opt(**dict(rec["opt"], **rec["test_opt"]))
    encoded = [G.unpack(e) for e in rec["encoded"]]
    s0, s1 = encoded[0], None
    if rec["mode"] == "inference_interpolation_style":
        s1 = s0.flip(0)
    elif rec["mode"] == "inference_particular_full":
        s1 = encoded[1]
    drawn = G.unpack(rec["noise"]) if "noise" in rec else None
    got = explore.build_styles(rec["mode"], opt, s0, s1, drawn, explore.style_variants_torch)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, rec["n"], 19, 128)
    assert G.same_styles(rec, got)
    assert ("applied_xor_encoded" in rec) == (bool(rec["test_opt"].get("dont_merge_fake"))
                                              or rec["mode"] == "inference_reference_interpolation")
    want = got                                  # (bit for bit the reference's, just checked)
    # the fixtures exercise what they are there for
    mask = explore.region_mask(opt.region_idx, 19)
    share = float((want[:, :, mask].abs() == 1).float().mean())
    assert share == pytest.approx(rec["share_at_clamp"])
    if rec["mode"] in ("inference_interpolation", "inference_reference_interpolation"):
        assert 0.05 < share < 0.95
    if rec["mode"] == "inference_reference_interpolation":
        assert rec["n"] == 4 and rec["recurrence_vs_closed_form"] > 1e-2
        v = explore.variants(rec["mode"], opt, 2, 19)
        closed = explore.style_variants_torch(s0, s0 * opt.manipulate_scale, v["src0"], v["src1"], v["alpha"], v["beta"],
                                              v["gamma"], None, v["mask"], True, False)
        assert float((closed - want).abs().max()) > 1e-2            # the aliasing matters at n = 4
    if rec["mode"] == "inference_interpolation":
        assert torch.equal(want[:, rec["n"] // 2], s0)              # the middle variant is the encoded style


def test_variants_refuse_an_even_n_where_the_reference_does():
    from deepsee_amd import explore
    from deepsee_amd.options import make_opt
    opt = make_opt(n_interpolation=4)
    for mode in ("inference_interpolation", "inference_interpolation_style"):
        with pytest.raises(AssertionError, match="odd n"):
            explore.variants(mode, opt, 2, 19)
    assert explore.variants("inference_reference_interpolation", opt, 2, 19)["n"] == 4
    assert explore.region_mask(None, 19).all() and explore.region_mask([], 19).all()
    assert explore.region_mask([1, 2, 5], 19).nonzero().flatten().tolist() == [1, 2, 5]


def test_torch_rule_flags():
    from deepsee_amd import explore
    g = torch.Generator().manual_seed(3)
    s0, s1 = torch.rand(2, 5, 8, generator=g) * 4 - 2, torch.rand(2, 5, 8, generator=g) * 4 - 2
    src0, src1 = torch.tensor([[0, 1, 0], [1, 1, 0]]), torch.tensor([[1, 0, 1], [0, 0, 1]])
    al, be, ga = torch.tensor([0.5, 0.25, 2.0]), torch.tensor([0.5, 1.0, -1.0]), torch.tensor([0.0, 0.125, -0.5])
    mask = torch.tensor([True, False, True, False, False])
    out = explore.style_variants_torch(s0, s1, src0, src1, al, be, ga, None, mask, False, False)
    for b in range(2):
        for k in range(3):
            a = s0[src0[b, k]]
            assert torch.equal(out[b, k, ~mask], a[~mask])
            assert torch.equal(out[b, k, mask], (al[k] * a + be[k] * s1[src1[b, k]] + ga[k])[mask])
    rec = explore.style_variants_torch(s0, s1, src0, src1, al, be, ga, None, mask, True, True)
    assert torch.equal(rec[:, 0], torch.where(mask[None, :, None], out[:, 0].clamp(-1, 1), out[:, 0]))
    for k in (1, 2):
        a = rec[:, k - 1]
        assert torch.equal(rec[:, k, mask], (al[k] * a + be[k] * s1[src1[:, k]] + ga[k]).clamp(-1, 1)[:, mask])
        assert torch.equal(rec[:, k, ~mask], rec[:, 0, ~mask])
    assert float(rec[:, :, mask].abs().max()) <= 1 and float(out[:, :, mask].abs().max()) > 1


# ---- C ABI
def test_entry_points_are_declared_exported_and_bound():
    from deepsee_amd import lib as L
    protos = L.header_prototypes()
    so = L.lib()
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float      # noqa: F841
    want = {"dsee_style_explore": [p] * 10 + [i] * 6 + [p], "dsee_nhwc_to_nchw_tiled": [p, p] + [i] * 8 + [p]}
    for name, args in want.items():
        assert protos[name] == (ctypes.c_int, args), name
        fn = getattr(so, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args


def test_entry_points_validate_before_they_launch():
    from deepsee_amd import lib as L
    so = L.lib()
    one = ctypes.c_void_p(64)        # a non-null, 16-byte aligned address that is never dereferenced

    def explore(**kw):
        a = dict(s0=one, s1=one, src0=one, src1=one, alpha=one, beta=one, gamma=one, noise=None, mask=one,
                 out=ctypes.c_void_p(128), B=2, n=3, nc=19, S=128, clamp=1, recurrent=0)
        assert set(kw) <= set(a)
        a.update(kw)
        return so.dsee_style_explore(*a.values(), None)

    def tiled(**kw):
        a = dict(x=one, y=one, B=2, n=3, H=8, W=8, cs=4, merge=1, pair0=0, pairs=6)
        assert set(kw) <= set(a)
        a.update(kw)
        return so.dsee_nhwc_to_nchw_tiled(*a.values(), None)

    bad = [lambda: explore(S=6), lambda: explore(nc=33), lambda: explore(out=None), lambda: explore(S=0), lambda: explore(n=0),
           lambda: explore(s1=None), lambda: explore(mask=None), lambda: explore(out=one),          # in place
           lambda: explore(noise=ctypes.c_void_p(68)), lambda: explore(B=1 << 20, n=1 << 10),
           lambda: tiled(y=None), lambda: tiled(x=None), lambda: tiled(cs=2), lambda: tiled(pairs=7), lambda: tiled(pair0=-1),
           lambda: tiled(pair0=5, pairs=2), lambda: tiled(pairs=0), lambda: tiled(W=0)]
    for k, call in enumerate(bad):
        assert call() == -1, k
        assert b"argument check failed" in so.dsee_last_error(), k


# ---- options, public surface
def test_option_defaults_are_the_references_test_options():
    from deepsee_amd.options import DEFAULTS, make_opt
    want = dict(region_idx=None, n_interpolation=5, noise_delta=0.0, noise_dist="normal", dont_merge_fake=False,
                manipulate_scale=1.0, explore_chunk=8)
    assert {k: DEFAULTS[k] for k in want} == want
    opt = make_opt("independent_8x_32", n_interpolation=3)
    assert opt.n_interpolation == 3 and opt.explore_chunk == 8 and opt.region_idx is None


def test_the_model_routes_the_six_modes_and_nothing_else():
    import inspect
    from deepsee_amd import explore
    from deepsee_amd.sr_model import SRModel
    assert len(explore.MODES) == 6 and all(m.startswith("inference_") for m in explore.MODES)
    for m in ("inference_noise", "inference_multi_modal", "inference_replace_semantics", "inference_reference_semantics"):
        assert m not in explore.MODES
    src = inspect.getsource(SRModel._forward)
    assert "explore.MODES" in src and "|mode| is invalid" in src
    assert callable(SRModel.get_noise) and callable(SRModel.encode_with)
    for name in ("style_variants", "style_variants_torch", "assemble", "run_pairs", "save_strips"):
        assert callable(getattr(explore, name)), name


def test_get_noise_draws_the_references_numbers():
    from deepsee_amd.sr_model import SRModel
    rec = load("indep_particular_combined_noise")
    torch.manual_seed(rec["rng_seed"])
    drawn = torch.randn(2, 3, 128).clamp(-1, 1) * rec["test_opt"]["noise_delta"]
    assert torch.equal(drawn, G.unpack(rec["noise"]))
    with pytest.raises(ValueError, match="Invalid noise distribution"):
        SRModel.get_noise(SimpleNamespace(opt=SimpleNamespace(noise_dist="cauchy")), (1,), 0.1)
