"""Host half of the on-device load-time geometry (deepsee_amd/resample.py, data.RawFolderDataset, DeviceLoader workers) against the
fixtures tools/gen_golden_loader.py wrote from the reference's own get_transform / get_params / Preprocessor and Pillow
(tests/golden/loader), and against Pillow itself.  CPU only."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from tools import gen_golden_loader as G

GEO = G.load("geometry")["cases"]
LR = G.load("lr")["cases"]


def _emulated(case, key, filt):
    """The numpy emulation of the device arithmetic over resample's tables, for the image or label batch of a geometry case."""
    from deepsee_amd import resample as R
    opt = G.case_opt(case)
    src = G.unpack_u8(case[key + "_src"])
    out = []
    for n in range(src.shape[0]):
        geo = R.load_geometry(opt, (src.shape[2], src.shape[1]), case["crop_pos"][n])
        x0, y0, bw, bh = geo["box"]
        xt, yt = R.axis_tables(geo, filt)
        out.append(R.emulate(src[n, y0:y0 + bh, x0:x0 + bw], xt, yt))
    return np.stack(out)


@pytest.mark.parametrize("name", sorted(GEO))
def test_integer_two_pass_equals_the_reference_fixture(name):
    """Tables + geometry + integer arithmetic == the pixels the reference's get_transform produced with Pillow, bit for bit:
    images with the case's filter, labels with NEAREST, every preprocess_mode."""
    case = dict(GEO[name])
    assert np.array_equal(_emulated(case, "image", case["filter"]), G.unpack_u8(case["image_out"]))
    assert np.array_equal(_emulated(case, "label", "nearest"), G.unpack_u8(case["label_out"]))


def test_fixtures_cover_every_mode_and_hold_what_they_promise():
    from deepsee_amd import resample as R
    assert {c["opt"]["preprocess_mode"] for c in GEO.values()} == set(R.MODES) and len(R.MODES) == 11
    checks = G.load("geometry")["checks"]
    assert min(checks["overshoot_case"]["below_0"], checks["overshoot_case"]["above_255"]) >= 0.01
    assert checks["pixels_changed_by_the_uint8_rounding_between_passes"]
    assert checks["nearest_pairs_of_cases_that_differ"]
    assert any((G.unpack_u8(c["label_src"]) == 255).any() and (G.unpack_u8(c["label_out"]) == 255).any() for c in GEO.values())
    assert sum(os.path.getsize(os.path.join(G.OUT, f)) for f in os.listdir(G.OUT)) < 200 * 1024


def test_emulation_equals_pillow_for_a_sweep_of_sizes():
    from PIL import Image
    from deepsee_amd import resample as R
    rng = np.random.default_rng(3)
    sizes = [(5, 7, 3, 2), (30, 30, 77, 41), (64, 64, 16, 16), (50, 70, 13, 29), (100, 33, 25, 33), (33, 100, 33, 20),
             (31, 9, 8, 8), (16, 16, 17, 15), (128, 96, 32, 24), (11, 11, 4, 4)]
    for h, w, oh, ow in sizes:
        for filt, pf in ((R.BICUBIC, Image.BICUBIC), (R.BILINEAR, Image.BILINEAR)):
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            a[::3] = np.where(rng.random((len(a[::3]), w, 3)) < 0.5, 0, 255)
            want = np.asarray(Image.fromarray(a).resize((ow, oh), pf))
            got = R.emulate(a, R.pil_tables(w, ow, filt), R.pil_tables(h, oh, filt))
            assert np.array_equal(got, want), (h, w, oh, ow, filt)
            gray = np.asarray(Image.fromarray(a[..., 0]).resize((ow, oh), pf))
            assert np.array_equal(R.emulate(a[..., 0], R.pil_tables(w, ow, filt), R.pil_tables(h, oh, filt)), gray)


def test_nearest_table_equals_pillow_below_64():
    from PIL import Image
    from deepsee_amd import resample as R
    for i in range(1, 64):
        row = np.arange(i, dtype=np.uint8)[None, :].repeat(2, 0)
        for o in range(1, 64):
            want = np.asarray(Image.fromarray(row).resize((o, 2), Image.NEAREST))[0]
            assert np.array_equal(R.nearest_table(i, o)[0], want), (i, o)


def test_tables_stay_inside_int32_and_the_source():
    from deepsee_amd import resample as R
    for filt in (R.BICUBIC, R.BILINEAR):
        for i, o in ((1024, 256), (1024, 255), (7, 64), (64, 7), (2, 3)):
            first, count, coef = R.pil_tables(i, o, filt)
            assert first.min() >= 0 and (first + count).max() <= i and count.min() >= 1
            assert 255 * int(np.abs(coef.astype(np.int64)).sum(1).max()) < 2 ** 31
            assert abs(int(coef.astype(np.int64).sum(1).max()) - (1 << 22)) < 64
    first, count, coef = R.pil_tables(9, 9, R.BICUBIC)            # a pass Pillow skips
    assert np.array_equal(first, np.arange(9)) and (count == 1).all() and (coef == 1 << 22).all()


def test_load_geometry_of_every_mode():
    """One box, one resize, one window per mode -- the sizes of every fixture, and the values worked out by hand from
    base_dataset.py:171-245 for the cases whose arithmetic can go wrong."""
    from deepsee_amd import resample as R
    for name, case in GEO.items():
        src = case["image_src"]["shape"]
        for n in range(2):
            geo = R.load_geometry(G.case_opt(case), (src[2], src[1]), case["crop_pos"][n])
            assert [geo["out"][1], geo["out"][0]] == case["image_out"]["shape"][1:3], name
    opt = G.case_opt
    # centre crops with h - s = 1, 3, 5: int(round(0.5)) = 0, int(round(1.5)) = 2, int(round(2.5)) = 2 (halves to even)
    assert R.load_geometry(opt(GEO["center_crop_13x15"]), (15, 13))["box"] == (2, 0, 12, 12)
    assert R.load_geometry(opt(GEO["center_crop_17x13"]), (13, 17))["box"] == (0, 2, 12, 12)
    g = R.load_geometry(opt(GEO["center_crop_and_resize_15x17"]), (17, 15))
    assert g["box"] == (2, 2, 12, 12) and g["resize"] == (8, 8) and g["window"] == (0, 0, 8, 8)
    assert R.load_geometry(opt(GEO["scale_width_23x17"]), (17, 23))["resize"] == (12, 16)
    assert R.load_geometry(opt(GEO["scale_width_9x12_no_resize"]), (12, 9))["resize"] is None
    assert R.load_geometry(opt(GEO["scale_shortside_23x17"]), (17, 23))["resize"] == (17, 16)      # the reference keeps ss
    assert R.load_geometry(opt(GEO["scale_shortside_17x23"]), (23, 17))["resize"] == (16, 17)
    assert R.load_geometry(opt(GEO["fixed_aspect2_23x17"]), (17, 23))["resize"] == (12, 6)
    g = R.load_geometry(opt(GEO["scale_width_and_crop_23x17"]), (17, 23), (4, 8))
    assert g["resize"] == (12, 16) and g["window"] == (4, 8, 8, 8)
    assert R.load_geometry(opt(GEO["none_9x12"]), (12, 9)) == {"box": (0, 0, 12, 9), "resize": None, "window": (0, 0, 12, 9),
                                                              "out": (12, 9)}


def test_crop_params_equal_get_params_under_seeded_random():
    from deepsee_amd import resample as R
    from deepsee_amd.options import make_opt
    cases = G.load("params")["cases"]
    assert {"resize_and_crop", "scale_width_and_crop", "scale_shortside_and_crop"} <= {c["preprocess_mode"] for c in cases}
    for c in cases:
        opt = make_opt(preprocess_mode=c["preprocess_mode"], load_size=c["load_size"], crop_size=c["crop_size"])
        rng = random.Random(c["seed"])
        for want in c["draws"]:
            got = R.crop_params(opt, tuple(c["size"]), rng)
            assert list(got["crop_pos"]) == want["crop_pos"] and bool(got["flip"]) == want["flip"], c


def test_refusals():
    from deepsee_amd import data as D, ops, resample as R
    from deepsee_amd.options import make_opt
    with pytest.raises(ValueError, match="leaves"):                      # PIL pads a crop that leaves the image
        R.load_geometry(make_opt(preprocess_mode="crop", crop_size=8), (17, 23), (10, 0))
    with pytest.raises(ValueError, match="leaves"):
        R.load_geometry(make_opt(preprocess_mode="resize_and_crop", load_size=12, crop_size=8), (17, 23), (0, 5))
    with pytest.raises(ValueError, match="leaves"):                      # torchvision pads a centre crop larger than the image
        R.load_geometry(make_opt(preprocess_mode="center_crop", center_crop_size=20), (17, 23))
    with pytest.raises(ValueError, match="center_crop_size"):
        R.load_geometry(make_opt(preprocess_mode="center_crop"), (17, 23))
    with pytest.raises(ValueError, match="scale_width"):
        R.load_geometry(make_opt(preprocess_mode="scale_height"), (17, 23))
    with pytest.raises(ValueError, match="bicubic, bilinear, nearest, area"):
        ops.lr_image(make_opt(downsampling_method="linear"), None)
    with pytest.raises(ValueError, match="bilinear, nearest, area"):
        ops.interp_down(None, 4, "bicubic")
    with pytest.raises(ValueError, match="a.png.*b.png"):
        D.stack_raw([np.zeros((4, 4, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)], ["a.png", "b.png"])
    opt = make_opt()
    ds = D.SyntheticDataset(opt, length=4)
    with pytest.raises(ValueError, match="workers"):
        D.DeviceLoader(ds, opt, workers=17)
    assert make_opt().center_crop_size is None and D.MAX_WORKERS == 16

    class Sequential:
        def __len__(self):
            return 4
    with pytest.raises(ValueError, match="thread_safe"):
        D.DeviceLoader(Sequential(), opt, workers=2)
    assert not getattr(D.FolderDataset, "thread_safe", False) and D.RawFolderDataset.thread_safe and D.SyntheticDataset.thread_safe


def _write_pairs(tmp_path, n=3, img_hw=(40, 48), lab_hw=(20, 24)):
    from PIL import Image
    (tmp_path / "lab").mkdir()
    (tmp_path / "img").mkdir()
    rng = np.random.default_rng(0)
    for i in range(n):
        Image.fromarray(rng.integers(0, 19, lab_hw, dtype=np.uint8)).save(str(tmp_path / "lab" / ("%03d.png" % i)))
        Image.fromarray(rng.integers(0, 256, img_hw + (3,), dtype=np.uint8)).save(str(tmp_path / "img" / ("%03d.png" % i)))


def test_raw_folder_dataset(tmp_path):
    from deepsee_amd import data as D
    from deepsee_amd.options import make_opt
    _write_pairs(tmp_path)
    lab, img = str(tmp_path / "lab"), str(tmp_path / "img")
    for mode in ("scale_width_and_crop", "center_crop", "none"):          # every mode is accepted: the dataset only decodes
        assert len(D.RawFolderDataset(make_opt(preprocess_mode=mode, center_crop_size=8), lab, img)) == 3
    with pytest.raises(ValueError, match="preprocess_mode"):
        D.RawFolderDataset(make_opt(preprocess_mode="stretch"), lab, img)
    opt = make_opt(preprocess_mode="resize_and_crop", load_size=16, crop_size=8, start_size=4)
    ds = D.RawFolderDataset(opt, lab, img, seed=4)
    s = ds[1]
    assert set(s) == {"image_raw", "label_raw", "crop_pos", "flip", "path"}
    assert s["image_raw"].shape == (40, 48, 3) and s["image_raw"].dtype == np.uint8
    assert s["label_raw"].shape == (20, 24) and s["label_raw"].dtype == np.uint8
    assert s["path"].endswith("001.png") and s["flip"] in (0, 1) and all(0 <= v <= 8 for v in s["crop_pos"])
    # a pure function of (seed, epoch, index): the same whatever was loaded before, different between epochs and seeds
    again = D.RawFolderDataset(opt, lab, img, seed=4)
    _ = again[2], again[0]
    assert again[1]["crop_pos"] == s["crop_pos"] and again[1]["flip"] == s["flip"]
    assert np.array_equal(again[1]["image_raw"], s["image_raw"])

    def draws(d):
        return [(d[i]["crop_pos"], d[i]["flip"]) for i in range(3)]
    first = draws(ds)
    epochs = []
    for e in range(1, 6):
        ds.set_epoch(e)
        epochs.append(draws(ds))
    assert any(e != first for e in epochs)
    ds.set_epoch(0)
    assert draws(ds) == first
    assert any(draws(D.RawFolderDataset(opt, lab, img, seed=k)) != first for k in range(5, 9))
    nf = D.RawFolderDataset(opt, lab, img, seed=4, no_flip=True)
    flips = []
    for e in range(8):
        nf.set_epoch(e)
        ds.set_epoch(e)
        assert all(nf[i]["flip"] == 0 for i in range(3))
        flips += [ds[i]["flip"] for i in range(3)]
    assert 0 < sum(flips) < len(flips)
    # the position is drawn for the LABEL file's size, as get_params(self.opt, label.size) does
    from deepsee_amd import resample as R
    ds.set_epoch(0)
    want = R.crop_params(opt, (24, 20), random.Random((4 * 1000003 + 0) * 1000003 + 1))
    assert ds[1]["crop_pos"] == want["crop_pos"]
    # collate keeps the raw form; a CPU DeviceLoader with workers loads in index order
    ld = D.DeviceLoader(ds, opt, batch_size=3, shuffle=False)
    host = ld.collate([ds[i] for i in range(3)])
    assert tuple(host["image_raw"].shape) == (3, 40, 48, 3) and tuple(host["label_raw"].shape) == (3, 20, 24)
    assert host["crop_pos"] == [ds[i]["crop_pos"] for i in range(3)] and host["image_raw"].dtype == torch.uint8


@pytest.mark.parametrize("name", sorted(LR))
def test_reference_fp32_lr_image_is_within_the_lr_bound(name):
    """The bound the device kernels are held to is attainable: the reference's own fp32 F.interpolate result, against float64 on
    the same input.  Where it misses 1e-6 (non-integer ratios: the fp32 source coordinate), the case's bound is twice its error
    (tools/gen_golden_loader.lr_bound; the values are listed in profiles/loader.md)."""
    rec = LR[name]
    x = G.unpack_f32(rec["input"])
    for mode in G.LR_MODES:
        err = G.rel(G.unpack_f32(rec["output"][mode]), G.lr_float64(x, rec["start_size"], mode))
        bound = G.lr_bound(rec, mode)
        print("%s %-8s reference fp32 vs float64 %.2e, bound %.2e" % (name, mode, err, bound))
        assert err <= bound and G.LR_BOUND <= bound < 5e-6
        if mode in ("nearest", "area") or name in ("32x32_to_4", "12x20_to_4"):
            assert bound == G.LR_BOUND


def test_new_prototypes_parse_and_resolve():
    from deepsee_amd import lib as L
    protos = L.header_prototypes()
    res, args = protos["dsee_resample_u8"]
    assert res is ctypes.c_int and len(args) == 19 and args[:3] == [ctypes.c_void_p] * 3
    assert args[5:7] == [ctypes.c_long, ctypes.c_long] and args[-1] is ctypes.c_void_p
    res, args = protos["dsee_interp_down"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    so = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(so, "dsee_resample_u8") and hasattr(so, "dsee_interp_down")
    # argument checks return an error code + message instead of launching
    so.dsee_last_error.restype = ctypes.c_char_p
    so.dsee_interp_down.argtypes = protos["dsee_interp_down"][1]
    assert so.dsee_interp_down(None, None, 1, 8, 8, 4, 4, 4, 0, None) == -1 and b"argument check failed" in so.dsee_last_error()
    so.dsee_resample_u8.argtypes = protos["dsee_resample_u8"][1]
    assert so.dsee_resample_u8(None, None, None, 1, 3, 0, 0, 0, 1, 1, 1, 1, 1, None, 1, None, 1, None, None) == -1
