"""The ablation generators (opt.netG = nostyle | nospadenostyle | puresean; reference deepsee_models/networks/ablation.py) on the
host: the block plan netG selects, the module layout and its checkpoint keys against fixtures written from the REAL reference by
tools/gen_golden_ablation.py (tests/golden/ablation/*.json), the substituted oracle against the same fixtures, the new C entry
points' declarations, and a float64 restatement of the identity the border-pass kernels are held to
(tests/test_gpu_ablation.py):  conv3x3(reflect_pad(x), w) = conv3x3(zero_pad(x), w) + ring(x, w).  CPU only."""
import glob
import json
import os

import pytest
import torch
import torch.nn.functional as F

from deepsee_amd import networks as N
from deepsee_amd.options import make_opt
from deepsee_amd.sr_model import SRModel, block_plan
from oracle import deepsee_oracle as O
from tools.gen_golden_ablation import CASES as GOLD_CASES, install_ablation

ABL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ablation")
CASES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(ABL, "*.json")))
SMALL = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)


def _rec(case):
    return json.load(open(os.path.join(ABL, case + ".json")))


def test_ablation_fixtures_present():
    assert set(CASES) == set(GOLD_CASES) == {"nostyle_4to32_ngf8", "puresean_abl_4to32_ngf8", "nospadenostyle_4to32_ngf8",
                                             "nospadenostyle_8to64_ngf8", "nostyle_4to128_ngf4"}
    for case in CASES:
        assert _rec(case)["opt"] == GOLD_CASES[case]["opt"]


@pytest.mark.parametrize("case", CASES)
def test_ablation_oracle_matches_reference_fixture(case, monkeypatch):
    """The substituted oracle (the yardstick of tests/test_gpu_ablation.py) reproduces the reference's inference / encode_only /
    demo outputs, G+D step losses, gradients and post-step state, with the bounds of tests/test_oracle_golden.py."""
    from tests import test_oracle_golden as TG
    install_ablation(monkeypatch.setattr)
    monkeypatch.setattr(TG, "GOLD", ABL)
    TG.test_oracle_matches_reference_fixture(case)


@pytest.mark.parametrize("case", CASES)
def test_ablation_state_dict_is_the_reference_key_set(case, monkeypatch):
    """SR / D / E keys and shapes == the reference model's (the fixture's post-step state was read from it; shapes from the
    substituted oracle layout, which gen_golden.run_case asserted equal to the reference's when the fixture was written)."""
    rec = _rec(case)
    opt = make_opt(**rec["opt"])
    ref_keys = {net: {k.split("/", 1)[1] for k in rec["iters"][0]["state_norms"] if k.startswith(net + "/")}
                for net in ("SR", "D", "E")}
    nets = {"SR": N.DeepSEESR(opt, block_plan(opt)), "D": N.MultiscaleDiscriminator(opt), "E": N.StyleEncoder(opt)}
    install_ablation(monkeypatch.setattr)
    spec = O.net_specs(O.make_opt(**rec["opt"]))
    for net, m in nets.items():
        got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert set(got) == ref_keys[net], (net, set(got) ^ ref_keys[net])
        assert got == {k: tuple(s) for k, s in spec[net].items()}, net
    want_n = {"nostyle_4to32_ngf8": 149, "nospadenostyle_4to32_ngf8": 34, "puresean_abl_4to32_ngf8": 169}.get(case)
    if want_n is not None:
        assert len(ref_keys["SR"]) == want_n
    if rec["opt"]["netG"] == "nospadenostyle":
        sr = set(nets["SR"].state_dict())
        blocks = [n for n, _ in block_plan(opt)]
        assert sr == {"initial.weight", "initial.bias", "conv_img.weight", "conv_img.bias"} | {
            "%s.conv_block.%d.0.%s" % (b, i, leaf) for b in blocks for i in (1, 4)
            for leaf in ("weight_orig", "weight_u", "weight_v")}


@pytest.mark.parametrize("netG,load_size,crop,want", [
    ("nostyle", 32, 32, ["spade"] * 5),
    ("puresean", 32, 32, ["puresean"] * 5),
    ("nospadenostyle", 32, 32, ["resnet"] * 5),
    ("deepsee", 32, 32, ["spade", "sean", "sean", "sean", "sean"]),
    # load_size >= 512: four full blocks, the tail beyond them PureSEAN (ablation.py:64-74) -- also under nostyle
    ("nostyle", 512, 128, ["spade"] * 6 + ["puresean"]),
    ("puresean", 512, 128, ["puresean"] * 7),
    ("nospadenostyle", 512, 128, ["resnet"] * 7),
    ("deepsee", 512, 128, ["spade"] + ["sean"] * 5 + ["puresean"]),
])
def test_block_plan_of_every_netG(netG, load_size, crop, want, monkeypatch):
    opt = make_opt(start_size=4, crop_size=crop, load_size=load_size, batchSize=2, ngf=4, netG=netG)
    plan = block_plan(opt)
    names = ["head_0", "G_middle_0", "G_middle_1"] + ["up_list.%d" % i for i in range(len(want) - 3)]
    assert plan == list(zip(names, want))
    # ... and it is the plan the substituted oracle runs
    install_ablation(monkeypatch.setattr)
    assert O.block_plan(O.make_opt(start_size=4, crop_size=crop, load_size=load_size, batchSize=2, ngf=4, netG=netG)) == plan


@pytest.mark.parametrize("netG", ["DeepSEE", "ablation", "nostyleablation", "no_style", "", None, 3])
def test_unknown_netG_raises_value_error(netG):
    with pytest.raises(ValueError):
        block_plan(make_opt(netG=netG, **SMALL))


def test_default_netG_is_the_deepsee_generator():
    """netG='deepsee' == an opt without the field: same plan, same keys and shapes."""
    a, b = make_opt(**SMALL), make_opt(netG="deepsee", **SMALL)
    assert a.netG == "deepsee"
    bare = make_opt(**SMALL)
    del bare.netG
    assert block_plan(a) == block_plan(b) == block_plan(bare)
    sds = [{k: tuple(v.shape) for k, v in N.DeepSEESR(o, block_plan(o)).state_dict().items()} for o in (a, b, bare)]
    assert sds[0] == sds[1] == sds[2]
    assert sds[0] == {k: tuple(s) for k, s in O.sr_spec(O.make_opt(**SMALL)).items()}


@pytest.mark.parametrize("netG", ["nostyle", "nospadenostyle", "puresean"])
def test_checkpoint_roundtrip_keeps_the_reference_keys(netG, tmp_path, monkeypatch):
    """{"model": state_dict} as SRModel.save writes it, read back through SRModel.load_net_state: the reference's key names in
    the reference's order, values intact; a DeepSEE checkpoint is refused by name."""
    install_ablation(monkeypatch.setattr)
    opt = make_opt(netG=netG, **SMALL)
    spec = O.sr_spec(O.make_opt(netG=netG, **SMALL))
    src, dst = N.DeepSEESR(opt, block_plan(opt)), N.DeepSEESR(opt, block_plan(opt))
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for v in src.state_dict().values():
            if v.is_floating_point():
                v.copy_(torch.randn(v.shape, generator=g))
    path = str(tmp_path / "latest_net_SR.pth")
    torch.save({"model": {k: v.detach().clone() for k, v in src.state_dict().items()}}, path)
    ck = torch.load(path)["model"]
    assert list(ck) == list(spec)
    SRModel.load_net_state(dst, ck)
    for (ka, a), (kb, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert ka == kb and torch.equal(a, b)
    other = make_opt(**SMALL)
    with pytest.raises(RuntimeError):
        SRModel.load_net_state(N.DeepSEESR(other, block_plan(other)), ck)


def test_resnet_block_has_no_style_noise_or_norm_state():
    opt = make_opt(netG="nospadenostyle", **SMALL)
    sr = N.DeepSEESR(opt, block_plan(opt))
    assert all(isinstance(b, N.ResnetBlock) for b in [sr.head_0, sr.G_middle_0, sr.G_middle_1] + list(sr.up_list))
    assert not any(isinstance(m, (N.SpadeNorm, N.BNStats, N.VecP)) for m in sr.modules())
    assert all(c.bias is None for b in sr.up_list for c in (b.conv_0, b.conv_1))
    assert len(sr.state_dict()) == 34


def test_new_entry_points_are_declared():
    from deepsee_amd import lib as L
    import ctypes as C
    protos = L.header_prototypes()
    for name in ("dsee_reflect_ring_fwd", "dsee_reflect_ring_dgrad", "dsee_reflect_ring_wgrad", "dsee_norm_act_res_fwd"):
        res, args = protos[name]
        assert res is C.c_int and args[-1] is C.c_void_p
    assert protos["dsee_reflect_ring_fwd"][1] == protos["dsee_reflect_ring_dgrad"][1] == [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_void_p]
    assert protos["dsee_reflect_ring_wgrad_workspace"] == (C.c_size_t, [C.c_int] * 5)
    if os.path.exists(L.LIB_PATH):
        lib = L.lib()
        # validated before anything is launched: a NULL pointer, H < 2, W < 2, a stored count that is not the padded count
        bad = [(0, 1, 1, 2, 4, 4, 8, 8, 8, 8), (1, 1, 1, 2, 1, 4, 8, 8, 8, 8), (1, 1, 1, 2, 4, 1, 8, 8, 8, 8),
               (1, 1, 1, 2, 4, 4, 6, 6, 8, 8), (1, 1, 1, 2, 4, 4, 8, 8, 5, 12)]
        for fn in (lib.dsee_reflect_ring_fwd, lib.dsee_reflect_ring_dgrad):
            for x, w, y, *rest in bad:
                assert fn(x, w, y, *rest, None) == -1 and b"dsee_reflect_ring" in lib.dsee_last_error()
        assert lib.dsee_reflect_ring_wgrad(1, 1, 1, 1 << 30, 1, 2, 1, 4, 8, 8, 8, 8, None) == -1
        assert lib.dsee_reflect_ring_wgrad(1, 1, 0, 0, 1, 2, 4, 4, 8, 8, 8, 8, None) == -1      # no workspace
        assert lib.dsee_reflect_ring_wgrad_workspace(2, 1, 4, 8, 8) == 0
        assert lib.dsee_reflect_ring_wgrad_workspace(2, 8, 8, 20, 36) % (8 * 20 * 36 * 4) == 0


# ------------------------------------------------------------------------------------ the identity, restated in float64
def _r(a, n):
    return -a if a < 0 else (2 * n - 2 - a if a >= n else a)


def ring_terms(H, W):
    """[(output pixel, tap, source pixel)]: every tap of a border output whose padded coordinate lies outside the map."""
    out = []
    for i in range(H):
        for j in range(W):
            for kh in range(3):
                for kw in range(3):
                    a, b = i + kh - 1, j + kw - 1
                    if a < 0 or a >= H or b < 0 or b >= W:
                        out.append(((i, j), (kh, kw), (_r(a, H), _r(b, W))))
    return out


@pytest.mark.parametrize("N_,H,W,ci,co", [(1, 8, 12, 5, 7), (2, 4, 4, 3, 4), (1, 2, 2, 2, 3), (1, 3, 5, 2, 2), (1, 2, 7, 3, 2)])
def test_ring_identity_float64(N_, H, W, ci, co):
    """y, dx and dw of the reflect-padded layer = those of the zero-padded layer + the ring terms, term by term: what
    dsee_reflect_ring_fwd / _dgrad / _wgrad add.  Edge pixels have 3 outside taps, corners 5, interior outputs none; dx receives
    ring terms in rows 1, H-2 and columns 1, W-2 only; dw's centre tap none."""
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N_, ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(N_, co, H, W, generator=g, dtype=torch.float64)
    y_ref = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w)
    dx_ref, dw_ref = torch.autograd.grad(y_ref, (x, w), gy)
    y_zero = F.conv2d(x, w, padding=1)
    dx_zero, dw_zero = torch.autograd.grad(y_zero, (x, w), gy)
    terms = ring_terms(H, W)
    per_pixel = {}
    for p, _, _ in terms:
        per_pixel[p] = per_pixel.get(p, 0) + 1
    if H >= 3 and W >= 3:
        corners = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
        assert all(c == (5 if p in corners else 3) for p, c in per_pixel.items())
        assert set(per_pixel) == {(i, j) for i in range(H) for j in range(W) if i in (0, H - 1) or j in (0, W - 1)}
    assert len(terms) == 6 * H + 6 * W - 4
    xd, wd = x.detach(), w.detach()
    ring_y, ring_dx, ring_dw = torch.zeros_like(y_zero), torch.zeros_like(xd), torch.zeros_like(wd)
    for (i, j), (kh, kw), (si, sj) in terms:
        ring_y[:, :, i, j] += xd[:, :, si, sj] @ wd[:, :, kh, kw].t()
        ring_dx[:, :, si, sj] += gy[:, :, i, j] @ wd[:, :, kh, kw]
        ring_dw[:, :, kh, kw] += gy[:, :, i, j].t() @ xd[:, :, si, sj]
    assert float((y_zero + ring_y - y_ref).detach().abs().max()) < 1e-12
    assert float((dx_zero + ring_dx - dx_ref).abs().max()) < 1e-12
    assert float((dw_zero + ring_dw - dw_ref).abs().max()) < 1e-12
    inner = torch.zeros(H, W, dtype=torch.bool)
    inner[1], inner[H - 2], inner[:, 1], inner[:, W - 2] = True, True, True, True
    assert float(ring_dx[:, :, ~inner].abs().max() if (~inner).any() else 0.0) == 0.0
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    assert float(ring_y[:, :, ~border].abs().max() if (~border).any() else 0.0) == 0.0
    assert float(ring_dw[:, :, 1, 1].abs().max()) == 0.0
