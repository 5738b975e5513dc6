"""Non-square batches through the model layer, on the host: the oracle with the wrappers of tools/gen_golden_rect.py against
fixtures written from the REAL reference (tests/golden/rect/*.json), the LR shape rule, the geometry check that runs before any
launch, and the one new entry point (declared, exported, bound, validating before it launches).  CPU only."""
import ctypes
import glob
import json
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import deepsee_oracle as O
from tools.gen_golden_rect import CASES as GEN_CASES, hr_shape, install_rect

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rect")
CASES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLD, "*.json")))
LARGEST_EXISTING = os.path.join(os.path.dirname(GOLD), "host_logic.json")


def test_fixtures_present():
    assert CASES == sorted(GEN_CASES) and len(CASES) == 3, CASES
    recs = {c: json.load(open(os.path.join(GOLD, c + ".json"))) for c in CASES}
    assert {c: (r["opt"]["aspect_ratio"], r["rng_seed"], r["batch_seed"]) for c, r in recs.items()} == {
        "indep_5x4_to_40x32": (0.8, 3, 1003), "indep_4x8_to_32x64": (2.0, 4, 1004), "guided_8x4_to_64x32": (0.5, 8, 1008)}
    assert all(r["opt"]["batchSize"] == 2 and r["opt"]["ngf"] == 8 and r["n"] == 2 for r in recs.values())
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLD, c + ".json")) <= os.path.getsize(LARGEST_EXISTING)


@pytest.mark.parametrize("case", sorted(GEN_CASES))
def test_rect_oracle_matches_reference_fixture(case, monkeypatch):
    """The wrapped oracle (the yardstick of tests/test_gpu_rect_model.py) reproduces the reference's inference / encode_only /
    demo outputs, G+D step losses, gradients and post-step state with the checks and bounds of tests/test_oracle_golden.py."""
    from tests import test_oracle_golden as TG
    install_rect(monkeypatch.setattr)
    monkeypatch.setattr(TG, "GOLD", GOLD)
    TG.test_oracle_matches_reference_fixture(case)


def test_wrappers_make_the_rectangular_batch(monkeypatch):
    plain = O.make_opt(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)
    before = O.synthetic_batch(plain, 2, seed=5)
    install_rect(monkeypatch.setattr)
    after = O.synthetic_batch(plain, 2, seed=5)
    assert all(torch.equal(before[k], after[k]) for k in before)               # aspect_ratio == 1: handed on unchanged
    for name, (h, w, lh, lw) in {"indep_5x4_to_40x32": (40, 32, 5, 4), "indep_4x8_to_32x64": (32, 64, 4, 8),
                                 "guided_8x4_to_64x32": (64, 32, 8, 4)}.items():
        opt = O.make_opt(**GEN_CASES[name]["opt"])
        assert hr_shape(opt) == (h, w)
        batch = O.synthetic_batch(opt, 2, seed=1)
        assert tuple(batch["image"].shape) == (2, 3, h, w) and tuple(batch["label"].shape) == (2, 1, h, w)
        assert ("guiding_image" in batch) == bool(opt.guiding_style_image)
        cells = batch["label"][:, :, ::h // 4, ::w // 4]                       # a 4 x 4 grid of cells, nearest-upsampled
        assert torch.equal(F.interpolate(cells, size=(h, w), mode="nearest"), batch["label"])
        pre = O.Oracle(opt, O.recipe_state(opt, gain=1.0)).preprocess(batch)
        assert tuple(pre["image_lr"].shape) == (2, 3, lh, lw)
        assert torch.equal(pre["image_lr"], F.interpolate(batch["image"], (lh, lw), mode="bicubic").clamp(-1, 1))


# ---- the LR shape rule
@pytest.mark.parametrize("crop,start,h,w,want", [
    (32, 4, 32, 32, (4, 4)), (256, 32, 256, 256, (32, 32)), (64, 8, 64, 64, (8, 8)),       # square: (start_size, start_size)
    (32, 4, 40, 32, (5, 4)), (64, 8, 32, 64, (4, 8)), (32, 4, 64, 32, (8, 4)), (256, 32, 320, 256, (40, 32)),
    (12, 4, 12, 17, (4, 4)),             # f = 3 is no power of two
    (32, 4, 12, 17, (4, 4)),             # neither side a multiple of f = 8
    (32, 4, 36, 32, (4, 4)),             # H % f != 0
    (32, 4, 40, 36, (4, 4)),             # W % f != 0
    (33, 4, 32, 32, (4, 4)),             # start_size * f != crop_size
    (32, 4, 4, 4, (4, 4)),               # smaller than f
    (4, 4, 7, 9, (7, 9)),                # f = 1: the LR image is the image
])
def test_lr_shape_table(crop, start, h, w, want):
    from deepsee_amd import ops
    from deepsee_amd.options import make_opt
    assert ops.lr_shape(make_opt(crop_size=crop, start_size=start), h, w) == want


# ---- the geometry check
def _plan(**over):
    from deepsee_amd.options import make_opt
    from deepsee_amd.sr_model import block_plan
    opt = make_opt(**over)
    return opt, block_plan(opt)


def test_check_geometry_refuses_the_cap_on_non_square_maps():
    from deepsee_amd.sr_model import check_geometry
    opt, plan = _plan(start_size=4, crop_size=32, aspect_ratio=0.5, max_fm_size=16)
    with pytest.raises(ValueError, match=r"level 2 .*32 x 16.*max_fm_size=16") as e:
        check_geometry(opt, plan, 8, 4)                    # 8 x 4 -> 64 x 32: 16 x 8 passes, 32 x 16 is the first above the cap
    assert "64" in str(e.value)                            # ... and the message names the cap that would do
    with pytest.raises(ValueError, match="max_fm_size=16"):
        check_geometry(opt, plan, 4, 8)                    # the other orientation
    opt64, plan64 = _plan(start_size=4, crop_size=32, aspect_ratio=0.5, max_fm_size=64)
    assert check_geometry(opt64, plan64, 8, 4) is None and check_geometry(opt64, plan64, 4, 8) is None
    opt32, plan32 = _plan(start_size=4, crop_size=32, aspect_ratio=0.5, max_fm_size=32)
    with pytest.raises(ValueError, match=r"level 3 .*64 x 32"):
        check_geometry(opt32, plan32, 8, 4)                # the cap bites on one axis only
    for cap in (1, 8, 16, 64, 256):                        # square maps keep the reference's cap, whatever it is
        for over in (dict(start_size=4, crop_size=32), dict(start_size=8, crop_size=64), dict(start_size=32, crop_size=256),
                     dict(start_size=4, crop_size=128, load_size=512)):
            o, p = _plan(max_fm_size=cap, **over)
            assert check_geometry(o, p, o.start_size, o.start_size) is None
    # a SPADE level has no cap in the reference either (head_0 with the default 'late' norm_G)
    assert plan[0] == ("head_0", "spade")
    o, p = _plan(start_size=4, crop_size=4, max_fm_size=2)
    assert [k for _, k in p] == ["spade", "sean", "sean"]
    with pytest.raises(ValueError, match=r"level 1 \(G_middle_0, sean\)"):
        check_geometry(o, p, 3, 2)
    with pytest.raises(ValueError):
        check_geometry(o, p, 0, 4)


def test_forward_checks_the_geometry_first():
    import inspect
    from deepsee_amd.sr_model import SRModel
    src = inspect.getsource(SRModel._forward)
    assert 0 < src.index("check_geometry(") < src.index("self._native(") < src.index("begin_step()")


# ---- C ABI
PROTOTYPES = {   # (result, arguments without the stream) as the parent commit declares them
    "dsee_bicubic_down": "int dsee_bicubic_down(const float* x, float* y, int N, int H, int W, int S, int cs_in, int cs_out, "
                         "hipStream_t stream);",
    "dsee_interp_down": "int dsee_interp_down(const float* x, float* y, int N, int H, int W, int S, int cs_in, int cs_out, int mode, "
                        "hipStream_t stream);",
    "dsee_bicubic_up": "int dsee_bicubic_up(const float* x, float* y, int N, int S, int H, int W, int cs_in, int cs_out, int clamp, "
                       "hipStream_t stream);",
}


def test_resize_hw_is_declared_exported_and_bound():
    from deepsee_amd import lib as L
    protos = L.header_prototypes()
    so = L.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    assert protos["dsee_resize_hw"] == (ctypes.c_int, [p, p] + [i] * 9 + [p])
    fn = so.dsee_resize_hw
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == protos["dsee_resize_hw"][1]
    assert protos["dsee_bicubic_down"] == (ctypes.c_int, [p, p] + [i] * 6 + [p])
    assert protos["dsee_interp_down"] == (ctypes.c_int, [p, p] + [i] * 7 + [p])
    assert protos["dsee_bicubic_up"] == (ctypes.c_int, [p, p] + [i] * 7 + [p])
    header = " ".join(open(L.HEADER_PATH).read().split())
    for name, text in PROTOTYPES.items():
        assert " ".join(text.split()) in header, name


def test_resize_hw_validates_before_it_launches():
    from deepsee_amd import lib as L
    so = L.lib()
    one = ctypes.c_void_p(64)        # a non-null address that is never dereferenced: the checks come before any launch

    def call(**kw):
        a = dict(x=one, y=one, N=1, H=40, W=32, OH=5, OW=4, cs_in=4, cs_out=4, mode=3, clamp=1)
        assert set(kw) <= set(a)
        a.update(kw)
        return so.dsee_resize_hw(*a.values(), None)

    for bad in (dict(x=None), dict(y=None), dict(N=0), dict(H=0), dict(W=-1), dict(OH=0), dict(OW=0), dict(cs_in=2),
                dict(cs_out=2), dict(mode=4), dict(mode=-1), dict(clamp=2)):
        assert call(**bad) == -1, bad
        assert b"argument check failed" in so.dsee_last_error(), bad


def test_python_surface():
    import inspect
    from deepsee_amd import ops
    assert ops.RESIZE_MODES == {"bilinear": 0, "nearest": 1, "area": 2, "bicubic": 3}
    assert list(inspect.signature(ops.lr_shape).parameters) == ["opt", "H", "W"]
    src = inspect.getsource(ops.lr_image)
    assert "resize_hw(" in src and "bicubic_down(" not in src.replace("bits of bicubic_down", "")
    for fn, args in ((ops.bicubic_down, ["img_nhwc", "size"]), (ops.interp_down, ["img_nhwc", "size", "mode"]),
                     (ops.bicubic_up, ["img_nhwc", "h", "w", "clamp"])):
        assert list(inspect.signature(fn).parameters) == args
    with pytest.raises(ValueError, match="bicubic"):
        ops.resize_hw(torch.zeros(1, 4, 4, 4), 2, 2, "linear")
