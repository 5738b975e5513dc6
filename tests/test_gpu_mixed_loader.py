"""Batches of differently sized files on the device: dsee_resample_u8_ragged against Pillow's own pixels per file and against
the fixture the reference wrote (tests/golden/mixed_loader), bit for bit with dsee_resample_u8 on a uniform batch, and
device_preprocess / DeviceLoader over mixed raw batches, plain and guided, against the per-file results of the uniform path.
The batches are those of tests/test_mixed_loader_host.py."""
import numpy as np
import pytest
import torch

import redzone
import test_mixed_loader_host as TH
from tools import gen_golden_loader as G
from tools import gen_golden_mixed_loader as M

pytestmark = pytest.mark.gpu

IMG_WH = [(37, 29), (64, 48), (23, 41), (9, 40)]
LAB_WH = [(19, 15), (32, 24), (12, 21), (5, 20)]


def ragged(opt, arrays, pos, filt, mode=None):
    """The files of a batch in the arena form through one dsee_resample_u8_ragged call."""
    from deepsee_amd import data as D, resample as R
    buf, offsets = R.pack_arena(arrays)
    arena = D.RawArena(buf, offsets, [a.shape for a in arrays], ["file%d" % n for n in range(len(arrays))])
    return D.resample_ragged(opt, [arena], pos, filt, mode)


@pytest.mark.parametrize("name", sorted(TH.CASES))
def test_entry_point_equals_pillow(name):
    """C = 3 with the case's filter resp. C = 1 with NEAREST, and C = 1 with the case's filter (one channel of every image as a
    map [H, W]: Pillow treats the bands of an image alike)."""
    over, sizes, c, filt, pos = TH.CASES[name]
    arrays, opt = TH.files(name), TH.make_opt(over, filt)
    want = torch.from_numpy(TH.pillow(name, arrays))
    got = ragged(opt, arrays, pos, filt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want)
    if c == 3:
        got = ragged(opt, [np.ascontiguousarray(a[..., 1]) for a in arrays], pos, filt)
        assert torch.equal(got.cpu(), want[..., 1])


def test_uniform_batch_has_the_bits_of_resample_u8():
    """4 x 48 x 48 RGB to 16, crop 8, per-sample crop positions: both entry points, the same bits (and Pillow's)."""
    from deepsee_amd import data as D, lib as L
    opt = TH.make_opt(TH._RC)
    src = np.random.default_rng(21).integers(0, 256, (4, 48, 48, 3), dtype=np.uint8)
    src[1, ::2] = 0
    pos = TH._POS4
    before = L.CALLS
    uniform = D.resample_raw(opt, torch.from_numpy(src), pos, "bicubic")
    mixed = ragged(opt, list(src), pos, "bicubic")
    assert L.CALLS - before == 2 and torch.equal(uniform, mixed) and tuple(mixed.shape) == (4, 8, 8, 3)
    labs = src[..., 0] % 19
    assert torch.equal(D.resample_raw(opt, torch.from_numpy(labs), pos, "nearest"), ragged(opt, list(labs), pos, "nearest"))


def _mixed_samples(seed=5, guided=False, n=4):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        (w, h), (lw, lh) = IMG_WH[k], LAB_WH[k]
        lab = rng.integers(0, 19, (lh, lw), dtype=np.uint8)
        lab[0, :2] = 255
        s = {"image_raw": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "label_raw": lab, "crop_pos": TH._POS4[k],
             "flip": [1, 0, 1, 0][k], "path": "img/%d.png" % k}
        if guided:                         # the guides: the files of the other end of the list, so all 2N sizes differ
            (w, h), (lw, lh) = IMG_WH[3 - k], LAB_WH[3 - k]
            s.update(guiding_image_raw=rng.integers(0, 256, (h, w, 3), dtype=np.uint8), guiding_path="img/g%d.png" % k,
                     guiding_label_raw=rng.integers(0, 19, (lh, lw), dtype=np.uint8))
        out.append(s)
    return out


def _one(opt, s, pre=""):
    """One file pair through the uniform path, N = 1."""
    from deepsee_amd import data as D
    return D.device_preprocess(opt, {"image_raw": torch.from_numpy(s[pre + "image_raw"][None]), "crop_pos": [s["crop_pos"]],
                                     "label_raw": torch.from_numpy(s[pre + "label_raw"][None]),
                                     "flip": torch.tensor([s["flip"]], dtype=torch.uint8)})


def mixed_batch_equals_the_files_one_by_one():
    from deepsee_amd import data as D
    opt = TH.make_opt(TH._RC)
    samples = _mixed_samples()
    ld = D.DeviceLoader(D.SyntheticDataset(opt, length=4), opt, batch_size=4, shuffle=False)
    host = ld.collate(samples)          # (the parent commit refuses here: stack_raw's ValueError)
    assert isinstance(host["image_raw"], D.RawArena) and isinstance(host["label_raw"], D.RawArena)
    got = D.device_preprocess(opt, host)
    single = [_one(opt, s) for s in samples]
    torch.cuda.synchronize()
    assert got["path"] == [s["path"] for s in samples] and got["image_hr"].dsee_layout == "nhwc"
    assert tuple(got["image_hr"].shape) == (4, 8, 8, 4) and tuple(got["image_lr"].shape) == (4, 4, 4, 4)
    for k in ("image_hr", "image_lr"):
        assert torch.equal(got[k], torch.cat([o[k] for o in single])), k
    assert torch.equal(got["input_semantics"].t, torch.cat([o["input_semantics"].t for o in single]))
    assert int(got["input_semantics"].t.max()) == 19
    assert not torch.equal(got["image_hr"][0], got["image_hr"][0].flip(1))          # (a flip that shows)


def test_device_preprocess_on_a_mixed_raw_batch():
    mixed_batch_equals_the_files_one_by_one()


def test_mixed_raw_batch_inside_red_zones():
    """The same batch with every buffer of every call between guard bands (tests/redzone.py): the arena is one guarded buffer, the
    item table holds offsets into it, so dsee_resample_u8_ragged needs no pass-through."""
    with redzone.guarded() as rz:
        mixed_batch_equals_the_files_one_by_one()
    assert "resample_u8_ragged" in rz.guarded and "resample_u8_ragged" not in rz.passthrough
    assert "resample_u8_ragged" not in redzone.ALLOWLIST and not rz.passthrough


@pytest.mark.parametrize("name", sorted(TH.GOLD))
def test_entry_point_equals_the_reference_fixture(name):
    case = TH.GOLD[name]
    imgs, labs = [G.unpack_u8(r) for r in case["image_src"]], [G.unpack_u8(r) for r in case["label_src"]]
    for filt in case["filters"]:
        got = ragged(M.case_opt(case, filt), imgs, case["crop_pos"], filt)
        assert torch.equal(got.cpu(), torch.from_numpy(G.unpack_u8(case["image_out"][filt]))), filt
    got = ragged(M.case_opt(case), labs, case["crop_pos"], "nearest")
    assert torch.equal(got.cpu(), torch.from_numpy(G.unpack_u8(case["label_out"])))


def test_guided_mixed_batch_takes_two_ragged_calls(monkeypatch):
    """N = 2 samples and their guides, all four files of a kind of different sizes: one arena and one call of 4 items per kind."""
    from deepsee_amd import data as D, lib as L
    opt = TH.make_opt(TH._RC)
    samples = _mixed_samples(seed=6, guided=True, n=2)
    ld = D.DeviceLoader(D.SyntheticDataset(opt, length=4), opt, batch_size=2, shuffle=False)
    host = ld.collate(samples)
    assert host["image_raw"].buf is host["guiding_image_raw"].buf and host["label_raw"].buf is host["guiding_label_raw"].buf
    names, real = [], L.call

    def counted(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(L, "call", counted)
    got = D.device_preprocess(opt, host)
    monkeypatch.setattr(L, "call", real)
    assert names.count("resample_u8_ragged") == 2 and "resample_u8" not in names, names
    own = [_one(opt, s) for s in samples]
    guide = [_one(opt, s, "guiding_") for s in samples]
    torch.cuda.synchronize()
    assert got["guiding_path"] == ["img/g0.png", "img/g1.png"]
    assert torch.equal(got["image_hr"], torch.cat([o["image_hr"] for o in own]))
    assert torch.equal(got["image_lr"], torch.cat([o["image_lr"] for o in own]))
    assert torch.equal(got["input_semantics"].t, torch.cat([o["input_semantics"].t for o in own]))
    assert torch.equal(got["guiding_image"], torch.cat([o["image_hr"] for o in guide]))
    assert torch.equal(got["guiding_label"].t, torch.cat([o["input_semantics"].t for o in guide]))


def test_device_loader_over_a_folder_of_three_sizes(tmp_path):
    """Six PNG pairs in three sizes, batches of 3, two epochs, with 2 decoding threads and with none: every item equals Pillow's
    resize + crop of its own files at the crop position and flip of (seed, epoch, index)."""
    import random
    from PIL import Image
    from deepsee_amd import data as D, resample as R
    (tmp_path / "lab").mkdir()
    (tmp_path / "img").mkdir()
    rng = np.random.default_rng(2)
    sizes = [((40, 48), (20, 24)), ((33, 27), (33, 27)), ((21, 50), (10, 25))]            # (h, w) of image and label file
    for i in range(6):
        ihw, lhw = sizes[i % 3]
        Image.fromarray(rng.integers(0, 19, lhw, dtype=np.uint8)).save(str(tmp_path / "lab" / ("%03d.png" % i)))
        Image.fromarray(rng.integers(0, 256, ihw + (3,), dtype=np.uint8)).save(str(tmp_path / "img" / ("%03d.png" % i)))
    opt = TH.make_opt(dict(TH._RC, no_flip=False, batchSize=3))
    runs = []
    for workers in (2, 0):
        ds = D.RawFolderDataset(opt, str(tmp_path / "lab"), str(tmp_path / "img"), seed=6)
        ld = D.DeviceLoader(ds, opt, shuffle=True, seed=2, workers=workers)
        epochs = []
        for _ in range(2):
            batches = list(ld)
            torch.cuda.synchronize()
            assert len(batches) == 2 and tuple(batches[0]["image_hr"].shape) == (3, 8, 8, 4)
            epochs.append(batches)
        assert ld.pool is None
        runs.append(epochs)
    flips = 0
    for e in range(2):
        for a, b in zip(runs[0][e], runs[1][e]):
            assert a["path"] == b["path"] and torch.equal(a["image_hr"], b["image_hr"]) and torch.equal(a["image_lr"], b["image_lr"])
            assert torch.equal(a["input_semantics"].t, b["input_semantics"].t)
            wire = {"image": [], "label": [], "flip": []}
            for p in a["path"]:
                i = int(p[-7:-4])
                lab = Image.open(str(tmp_path / "lab" / ("%03d.png" % i)))
                par = R.crop_params(opt, lab.size, random.Random((6 * 1000003 + e) * 1000003 + i))
                x, y = par["crop_pos"]
                box = (x, y, x + 8, y + 8)
                wire["label"].append(np.asarray(lab.resize((16, 16), Image.NEAREST).crop(box), dtype=np.uint8))
                wire["image"].append(np.asarray(Image.open(p).convert("RGB").resize((16, 16), Image.BICUBIC).crop(box), dtype=np.uint8))
                wire["flip"].append(int(par["flip"]))
            flips += sum(wire["flip"])
            want = D.device_preprocess(opt, {"image": torch.from_numpy(np.stack(wire["image"])),
                                             "label": torch.from_numpy(np.stack(wire["label"])),
                                             "flip": torch.tensor(wire["flip"], dtype=torch.uint8)})
            torch.cuda.synchronize()
            assert torch.equal(a["image_hr"], want["image_hr"]) and torch.equal(a["image_lr"], want["image_lr"])
            assert torch.equal(a["input_semantics"].t, want["input_semantics"].t)
    assert 0 < flips < 12
    assert sorted(p for b in runs[0][0] for p in b["path"]) == sorted(p for b in runs[0][1] for p in b["path"])
