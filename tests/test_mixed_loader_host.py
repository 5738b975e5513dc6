"""Host half of the loader over batches of differently sized files: resample.pack_arena / ragged_tables (the arguments of
dsee_resample_u8_ragged) read back by a numpy stand-in of the kernel and held to Pillow's own crop / resize / crop per file, bit
for bit; the fixture the reference wrote (tests/golden/mixed_loader, tools/gen_golden_mixed_loader.py); the refusal of batches
whose outputs differ in size; the host asserts of ops.resample_u8_ragged; DeviceLoader.collate.  CPU only.

CASES (sizes are (w, h)) is shared with tests/test_gpu_mixed_loader.py, which runs the same batches through the entry point."""
import ctypes

import numpy as np
import pytest
import torch

from tools import gen_golden_loader as G
from tools import gen_golden_mixed_loader as M

GOLD = M.load()["cases"]

_RC = dict(preprocess_mode="resize_and_crop", load_size=16, crop_size=8)
_POS4 = [(0, 0), (8, 8), (3, 5), (8, 0)]
# name: options, (w, h) of the files, channels, filter, crop position per file
CASES = {
    "resize_and_crop_bicubic": (_RC, [(37, 29), (64, 48), (23, 41), (9, 40)], 3, "bicubic", _POS4),
    "resize_and_crop_bilinear": (_RC, [(37, 29), (64, 48), (23, 41), (9, 40)], 3, "bilinear", _POS4),
    "label_maps_nearest": (_RC, [(19, 15), (32, 24), (12, 21), (5, 20)], 1, "nearest", _POS4),
    "center_crop_and_resize": (dict(preprocess_mode="center_crop_and_resize", center_crop_size=12, load_size=8),
                               [(13, 15), (17, 13), (40, 12)], 3, "bicubic", [(0, 0)] * 3),
    "fixed": (dict(preprocess_mode="fixed", crop_size=10, aspect_ratio=0.8), [(24, 17), (7, 13), (33, 50)], 3, "bicubic",
              [(0, 0)] * 3),
}


def make_opt(over, filt="bicubic"):
    from deepsee_amd.options import make_opt
    return make_opt(**dict(dict(no_flip=True, start_size=4, label_nc=19, downsampling_method=filt if filt != "nearest" else "bicubic"),
                           **over))


def files(name):
    """The files of a case: noise, every second one with 0 / 255 rows (the overshoot of the bicubic taps is reached)."""
    over, sizes, c, filt, pos = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 40)
    out = []
    for n, (w, h) in enumerate(sizes):
        a = rng.integers(0, 19 if c == 1 else 256, (h, w) if c == 1 else (h, w, 3), dtype=np.uint8)
        if n % 2 and c == 3:
            a[::2] = np.where(rng.random(a[::2].shape) < 0.5, 0, 255)
        if c == 1:
            a[0, 0] = 255
        out.append(a)
    return out


def pillow(name, arrays):
    """Pillow's own crop, resize and crop of every file of a case, written out per mode (not through resample.load_geometry)."""
    from PIL import Image
    over, sizes, c, filt, pos = CASES[name]
    pf = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "nearest": Image.NEAREST}[filt]
    out = []
    for a, (x, y) in zip(arrays, pos):
        im = Image.fromarray(a)
        w, h = im.size
        if over["preprocess_mode"] == "resize_and_crop":
            im = im.resize((over["load_size"],) * 2, pf).crop((x, y, x + over["crop_size"], y + over["crop_size"]))
        elif over["preprocess_mode"] == "center_crop_and_resize":
            s = over["center_crop_size"]
            left, top = int(round((w - s) / 2.0)), int(round((h - s) / 2.0))
            im = im.crop((left, top, left + s, top + s)).resize((over["load_size"],) * 2, pf)
        else:
            im = im.resize((over["crop_size"], int(round(over["crop_size"] / over["aspect_ratio"]))), pf)
        out.append(np.asarray(im, dtype=np.uint8))
    return np.stack(out)


def tables_of(opt, arrays, pos, filt, mode=None):
    """(arena, ragged tables, geometries) of a batch of files."""
    from deepsee_amd import resample as R
    buf, offsets = R.pack_arena(arrays)
    geos = [R.load_geometry(opt, (a.shape[1], a.shape[0]), p, mode) for a, p in zip(arrays, pos)]
    c = 1 if arrays[0].ndim == 2 else 3
    tab = R.ragged_tables(geos, filt, [(a.shape[1], a.shape[0], c) for a in arrays], offsets, ["file%d" % n for n in range(len(arrays))])
    return buf, tab, geos


def stand_in(arena, tab, c):
    """What dsee_resample_u8_ragged computes, in numpy: every sample is read FROM THE ARENA through its item row, its horizontal
    pass runs over the rows `rows` names, with the padded tables as the kernel gets them (resample.emulate is the arithmetic)."""
    from deepsee_amd import resample as R
    arena = np.asarray(arena)
    out = []
    for n, (off, stride, bw, bh) in enumerate(tab["items"].tolist()):
        box = np.stack([arena[off + r * stride:off + r * stride + bw * c].reshape(bw, c) for r in range(bh)])
        r0, nr = tab["rows"][n].tolist()
        assert r0 + nr <= bh and nr <= tab["tmp_rows"]
        xt, yt = [(t[n, :, 0], t[n, :, 1], t[n, :, 2:]) for t in (tab["xtab"], tab["ytab"])]
        res = R.emulate(box[r0:r0 + nr], xt, yt)
        out.append(res[..., 0] if c == 1 else res)
    return np.stack(out)


@pytest.mark.parametrize("name", sorted(CASES))
def test_ragged_tables_read_through_the_arena_equal_pillow(name):
    over, sizes, c, filt, pos = CASES[name]
    arrays = files(name)
    buf, tab, geos = tables_of(make_opt(over, filt), arrays, pos, filt)
    assert np.array_equal(stand_in(buf.numpy(), tab, c), pillow(name, arrays))
    # the padding is exercised: samples of one batch need different numbers of taps, the tables carry the maximum
    from deepsee_amd import resample as R
    own = [R.axis_tables(g, filt)[0][2].shape[1] for g in geos]
    assert tab["xtab"].shape[2] - 2 == max(own), own
    if name in ("resize_and_crop_bicubic", "resize_and_crop_bilinear", "fixed"):       # (boxes of different widths)
        assert len(set(own)) > 1, own
    assert tab["tmp_rows"] == int(tab["rows"][:, 1].max()) and tab["items"].dtype == np.int64 and tab["items"].shape == (len(sizes), 4)


def test_tap_counts_of_the_cases_span_3_to_19():
    from deepsee_amd import resample as R
    counts = set()
    for name, (over, sizes, c, filt, pos) in CASES.items():
        if filt == "nearest":
            continue
        for (w, h), p in zip(sizes, pos):
            xt, yt = R.axis_tables(R.load_geometry(make_opt(over, filt), (w, h), p), filt)
            counts |= {xt[2].shape[1], yt[2].shape[1]}
    assert min(counts) <= 3 and max(counts) >= 19, sorted(counts)


@pytest.mark.parametrize("name", sorted(GOLD))
def test_stand_in_equals_the_reference_fixture(name):
    """The batches the reference's own get_params / get_transform processed file by file (the `not gpu` twin of
    tests/test_gpu_mixed_loader.py::test_entry_point_equals_the_reference_fixture)."""
    case = GOLD[name]
    labs = [G.unpack_u8(r) for r in case["label_src"]]
    imgs = [G.unpack_u8(r) for r in case["image_src"]]
    assert len({a.shape for a in imgs}) > 1 and max(max(a.shape[:2]) for a in imgs + labs) <= 64
    for filt in case["filters"]:
        buf, tab, _ = tables_of(M.case_opt(case, filt), imgs, case["crop_pos"], filt)
        assert np.array_equal(stand_in(buf.numpy(), tab, 3), G.unpack_u8(case["image_out"][filt])), filt
    buf, tab, _ = tables_of(M.case_opt(case), labs, case["crop_pos"], "nearest")
    assert np.array_equal(stand_in(buf.numpy(), tab, 1), G.unpack_u8(case["label_out"]))


def test_outputs_of_different_sizes_are_refused_naming_both_files():
    from deepsee_amd import resample as R
    opt = make_opt(dict(preprocess_mode="scale_width", load_size=12))

    def tables(sizes):
        geos = [R.load_geometry(opt, wh) for wh in sizes]
        return R.ragged_tables(geos, "bicubic", [wh + (3,) for wh in sizes], [0, 4096], ["a/first.png", "b/second.png"])
    with pytest.raises(ValueError) as e:
        tables([(23, 17), (24, 24)])
    msg = str(e.value)
    assert "a/first.png" in msg and "b/second.png" in msg and "12 x 8" in msg and "12 x 12" in msg
    assert "23 x 17" in msg and "24 x 24" in msg
    tab = tables([(23, 17), (46, 34)])                        # outputs that happen to coincide: 12 x 8 from both
    assert tab["xtab"].shape[:2] == (2, 12) and tab["ytab"].shape[:2] == (2, 8)
    assert tab["items"].tolist() == [[0, 69, 23, 17], [4096, 138, 46, 34]]


def test_item_table_asserts_fire_before_any_launch(monkeypatch):
    from deepsee_amd import lib as L, ops
    monkeypatch.setattr(L, "call", lambda *a: pytest.fail("the entry point was called"))
    name = "resize_and_crop_bicubic"
    over, sizes, c, filt, pos = CASES[name]
    buf, tab, geos = tables_of(make_opt(over, filt), files(name), pos, filt)
    dev = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in tab.items()}

    def run(items):
        return ops.resample_u8_ragged(buf, items, dev, geos[0]["out"], c)
    bad = tab["items"].copy()
    bad[3, 0] += 1                                            # the last file ends where the arena ends: one byte further is outside
    with pytest.raises(AssertionError, match="past the arena"):
        run(bad)
    bad = tab["items"].copy()
    bad[2, 0] = buf.numel() + 256
    with pytest.raises(AssertionError, match="past the arena"):
        run(bad)
    bad = tab["items"].copy()
    bad[1, 1] = bad[1, 2] * c - 1
    with pytest.raises(AssertionError, match="row stride"):
        run(bad)
    bad = tab["items"].copy()
    bad[0, 0] = -1
    with pytest.raises(AssertionError, match="negative offset"):
        run(bad)


def test_arena_starts_are_aligned_and_hold_the_files():
    from deepsee_amd import resample as R
    arrays = files("resize_and_crop_bicubic") + files("label_maps_nearest")
    buf, offsets = R.pack_arena(arrays)
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and R.ARENA_ALIGN == 256
    assert all(o % 256 == 0 for o in offsets) and offsets == sorted(offsets) and offsets[0] == 0
    for a, o, nxt in zip(arrays, offsets, offsets[1:] + [None]):
        assert np.array_equal(buf.numpy()[o:o + a.size], a.reshape(-1))
        assert nxt is None or 0 <= nxt - (o + a.size) < 256
    assert buf.numel() == offsets[-1] + arrays[-1].size


def _samples(img_sizes, lab_sizes, guided=False):
    rng = np.random.default_rng(8)
    out = []
    for n, ((w, h), (lw, lh)) in enumerate(zip(img_sizes, lab_sizes)):
        s = {"image_raw": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "label_raw": rng.integers(0, 19, (lh, lw), dtype=np.uint8),
             "crop_pos": (n, 1), "flip": n % 2, "path": "img/%d.png" % n}
        if guided:
            s.update(guiding_image_raw=rng.integers(0, 256, (h + 1, w, 3), dtype=np.uint8), guiding_path="img/g%d.png" % n,
                     guiding_label_raw=rng.integers(0, 19, (lh, lw), dtype=np.uint8))
        out.append(s)
    return out


def test_collate_returns_the_arena_form_for_mixed_sizes_only():
    from deepsee_amd import data as D
    opt = make_opt(_RC)
    ld = D.DeviceLoader(D.SyntheticDataset(opt, length=4), opt, batch_size=3, shuffle=False)
    # uniform: exactly the stacked tensors of before
    uni = _samples([(12, 10)] * 3, [(6, 5)] * 3)
    host = ld.collate(uni)
    assert set(host) == {"flip", "path", "label_raw", "image_raw", "crop_pos"}
    for key in ("image_raw", "label_raw"):
        assert isinstance(host[key], torch.Tensor) and host[key].dtype == torch.uint8
        assert torch.equal(host[key], torch.from_numpy(np.stack([s[key] for s in uni])))
    assert host["crop_pos"] == [(0, 1), (1, 1), (2, 1)] and host["flip"].tolist() == [0, 1, 0]
    # images mixed, label maps of one size: the arena form for the images alone
    mixed = _samples([(12, 10), (9, 14), (12, 10)], [(6, 5)] * 3)
    host = ld.collate(mixed)
    assert isinstance(host["label_raw"], torch.Tensor) and isinstance(host["image_raw"], D.RawArena)
    arena = host["image_raw"]
    assert arena.shapes == [(10, 12, 3), (14, 9, 3), (10, 12, 3)] and arena.paths == host["path"] and len(arena) == 3
    assert all(o % 256 == 0 for o in arena.offsets)
    for s, o in zip(mixed, arena.offsets):
        assert np.array_equal(arena.buf.numpy()[o:o + s["image_raw"].size], s["image_raw"].reshape(-1))
    # guided: samples and guides of a kind share one buffer, the guides' files after the samples'; the label maps (samples and
    # guides of one size each) stay tensors
    host = ld.collate(_samples([(12, 10)] * 3, [(6, 5)] * 3, guided=True))
    assert all(isinstance(host[k], torch.Tensor) for k in ("image_raw", "label_raw", "guiding_image_raw", "guiding_label_raw"))
    g = _samples([(12, 10), (9, 14), (12, 10)], [(6, 5)] * 3, guided=True)
    host = ld.collate(g)
    a, b = host["image_raw"], host["guiding_image_raw"]
    assert isinstance(a, D.RawArena) and isinstance(b, D.RawArena) and a.buf is b.buf and max(a.offsets) < min(b.offsets)
    assert b.shapes == [(11, 12, 3), (15, 9, 3), (11, 12, 3)] and b.paths == host["guiding_path"]
    assert isinstance(host["label_raw"], torch.Tensor) and isinstance(host["guiding_label_raw"], torch.Tensor)
    # stack_raw itself still refuses, as tests/test_loader_host.py pins; so does device_preprocess for a plain list of mixed arrays
    with pytest.raises(ValueError, match="one size"):
        D.stack_raw([s["image_raw"] for s in mixed], host["path"])


def test_ragged_prototype_parses():
    from deepsee_amd import lib as L
    res, args = L.header_prototypes()["dsee_resample_u8_ragged"]
    p, i, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert res is ctypes.c_int and args == [p, lg, p, p, p, i, i, i, i, i, p, i, p, i, p, p]
