"""Identity-paired guiding images on the host (data.IdentityIndex, the guides of FolderDataset / RawFolderDataset,
data.create_dataloader, the DeviceLoader's iterator) against the fixtures tools/gen_golden_guided_loader.py recorded from the
reference's CelebAMaskHQDataset / CelebADataset (tests/golden/guided_loader).  CPU only: the loader's device half is replaced by
the identity, so a 'batch' here is what collate made."""
import os
import random
import sys

import numpy as np
import pytest
import torch

from tools import gen_golden_guided_loader as GG

DATASET = GG.load("dataset")
CASES = {mode: GG.load(mode) for mode in ("celebamaskhq", "celeba")}
IDS = DATASET["ids"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return GG.write_files(DATASET, str(tmp_path_factory.mktemp("guided")))


@pytest.fixture
def host_only(monkeypatch):
    from deepsee_amd import data as D
    monkeypatch.setattr(D.DeviceLoader, "_upload", lambda self, host: (host, None))
    monkeypatch.setattr(D.DeviceLoader, "_hand_over", lambda self, dev, ev: dev)


def _opt(mode, phase="train", train=True, **over):
    from deepsee_amd.options import make_opt
    d = dict(CASES[mode]["opt"], start_size=4, batchSize=2, guiding_style_image=True, phase=phase, isTrain=train, dataset_mode=mode)
    d.update(over)
    return make_opt(**d)


def _raw(files, mode, phase="train", train=True, **kw):
    from deepsee_amd import data as D
    return D.RawFolderDataset(_opt(mode, phase, train), files["label_dir"], files["image_dir"], seed=DATASET["seed"],
                              identities=files[mode], dataset_mode=mode, **kw)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_both_identity_formats_parse_to_the_same_index(files):
    from deepsee_amd import data as D
    hq, ca = D.IdentityIndex.from_file(files["celebamaskhq"]), D.IdentityIndex.from_file(files["celeba"])
    assert DATASET["identities.csv"].startswith('"","hq_file_id","celeba_file_id","identity","count"')    # every field quoted
    assert len(hq) == 7 and len(ca) == 6 and hq != ca      # the CSV has a row of a file that is not in the folder
    assert hq.restrict(IDS) == ca and hq.restrict(IDS).id2identity == DATASET["identity"]
    assert ca.candidates("000002", False) == ["000002", "000005", "000011"]
    assert ca.candidates("000002", True) == ["000005", "000011"]
    assert hq.candidates("000100", True) == ["000999"] and hq.restrict(IDS).candidates("000100", True) == []
    with pytest.raises(KeyError, match=r"000777.*identities\.txt"):
        ca.candidates("000777", False)
    import deepsee_amd.data as mod
    assert "pandas" not in open(mod.__file__).read()


@pytest.mark.parametrize("mode", sorted(CASES))
def test_candidates_equal_the_references(files, mode):
    from deepsee_amd import data as D
    assert issubclass(D.SkipSampleException, ValueError)
    seen_skip = 0
    for phase in GG.PHASES:
        ds = _raw(files, mode, phase)
        for key in ("train_flips", "no_flips"):
            for i, want in enumerate(CASES[mode]["cases"]["%s/%s" % (phase, key)]):
                if want["raised"]:
                    assert want["id"] == "000100" and want["raised"] in ("ValueError", "SkipSampleException")
                    with pytest.raises(D.SkipSampleException, match="000100"):
                        ds.guide_candidates(i)
                    with pytest.raises(ValueError):
                        ds[i]
                    seen_skip += 1
                else:
                    assert ds.guide_candidates(i) == want["candidates"], (phase, i)
    assert seen_skip == (4 if mode == "celebamaskhq" else 2)
    # C's lone file guides itself in training; in celeba / val the sample stays a candidate
    assert _raw(files, mode, "train").guide_candidates(5) == ["000100"]
    assert ("000002" in _raw(files, mode, "val").guide_candidates(0)) == (mode == "celeba")
    assert "000002" not in _raw(files, mode, "test").guide_candidates(0)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("phase", GG.PHASES)
def test_folder_dataset_item_equals_the_reference(files, phase, train):
    """FolderDataset (PIL on the host, resize_and_crop: the CelebAMask-HQ fixture) with its generator at the item's seed: crop
    position, flip and guide are the reference's, and so is every pixel, the guide's included.  The flip and the 255 -> label_nc
    remap run on the device, so they are applied here to what the dataset returned (the reference does not remap the guide)."""
    from deepsee_amd import data as D
    opt = _opt("celebamaskhq", phase, train)
    ds = D.FolderDataset(opt, files["label_dir"], files["image_dir"], identities=files["celebamaskhq"])
    for i, want in enumerate(CASES["celebamaskhq"]["cases"]["%s/%s" % (phase, "train_flips" if train else "no_flips")]):
        ds.rng = random.Random(GG.item_seed(i))
        if want["raised"]:
            with pytest.raises(D.SkipSampleException):
                ds[i]
            continue
        got = ds[i]
        assert got["flip"] == int(want["flip"]) and got["path"].endswith(want["id"] + ".jpg")

        def flipped(a):
            return a[:, ::-1] if got["flip"] else a
        label = np.where(got["label"] == 255, opt.label_nc, got["label"])
        assert np.array_equal(flipped(got["image"]), GG.unpack_u8(want["image"]))
        assert np.array_equal(flipped(label), GG.unpack_u8(want["label"]))
        assert np.array_equal(flipped(got["guiding_image"]), GG.unpack_u8(want["guiding_image"]))
        assert np.array_equal(flipped(got["guiding_label"]), GG.unpack_u8(want["guiding_label"]))


@pytest.mark.parametrize("mode", sorted(CASES))
def test_raw_folder_dataset_guides(files, mode, host_only):
    from deepsee_amd import data as D
    images, labels = GG.unpack_u8(DATASET["images"]), GG.unpack_u8(DATASET["labels"])
    ds = _raw(files, mode)
    for i, want in enumerate(CASES[mode]["cases"]["train/train_flips"]):
        s = ds[i]
        assert set(s) == {"image_raw", "label_raw", "crop_pos", "flip", "path", "guiding_image_raw", "guiding_label_raw",
                          "guiding_path"}
        g = IDS.index(want["guide"])
        assert s["guiding_path"].endswith(want["guide"] + ".jpg") and s["path"].endswith(want["id"] + ".jpg")
        assert list(s["crop_pos"]) == want["crop_pos"] and s["flip"] == int(want["flip"])
        assert np.array_equal(s["image_raw"], images[i]) and np.array_equal(s["label_raw"], labels[i])
        assert np.array_equal(s["guiding_image_raw"], images[g]) and np.array_equal(s["guiding_label_raw"], labels[g])
        assert s["guiding_image_raw"].dtype == np.uint8 and s["guiding_label_raw"].shape == (12, 12)
    # a pure function of (seed, epoch, index): any call order, any number of threads; another epoch draws again
    assert D.RawFolderDataset.thread_safe
    first = [ds[i] for i in range(6)]
    again = _raw(files, mode)
    for i in (4, 1, 5, 0, 3, 2):
        _same(again[i], first[i])
    opt = _opt(mode)
    runs = []
    for workers in (0, 4):
        ld = D.DeviceLoader(_raw(files, mode), opt, batch_size=2, shuffle=True, seed=3, workers=workers)
        runs.append([list(ld), list(ld)])
        assert ld.pool is None and len(runs[-1][0]) == len(ld) == 3
    for e in range(2):
        for a, b in zip(runs[0][e], runs[1][e]):
            assert a["path"] == b["path"] and a["guiding_path"] == b["guiding_path"] and a["crop_pos"] == b["crop_pos"]
            for k in ("image_raw", "label_raw", "guiding_image_raw", "guiding_label_raw", "flip"):
                assert torch.equal(a[k], b[k]), k
            assert tuple(a["guiding_image_raw"].shape) == (2, 24, 24, 3) and tuple(a["guiding_label_raw"].shape) == (2, 12, 12)
    guides = []
    for e in range(8):
        ds.set_epoch(e)
        guides.append([ds[i]["guiding_path"] for i in range(6)])
    assert len({tuple(g) for g in guides}) > 1
    ds.set_epoch(0)
    assert [s["guiding_path"] for s in first] == guides[0]


def test_unguided_items_do_not_change(files):
    from deepsee_amd import data as D, resample as R
    for cls in (D.RawFolderDataset, D.FolderDataset):
        opt = _opt("celebamaskhq", guiding_style_image=False)
        plain = cls(opt, files["label_dir"], files["image_dir"], seed=5)
        new = cls(opt, files["label_dir"], files["image_dir"], seed=5, identities=files["celeba"], dataset_mode="celeba")
        assert new.identities is None and plain.items == new.items
        for i in range(6):
            a, b = plain[i], new[i]
            _same(a, b)
            assert set(a) == ({"image_raw", "label_raw", "crop_pos", "flip", "path"} if cls is D.RawFolderDataset
                              else {"image", "label", "flip", "path"})
            if cls is D.RawFolderDataset:      # the crop position of today's seeds: three draws of the item's own generator
                want = R.crop_params(opt, (12, 12), random.Random((5 * 1000003 + 0) * 1000003 + i))
                assert a["crop_pos"] == want["crop_pos"] and a["flip"] == int(want["flip"])
    # ... and the guide is drawn after them: a guided item has the unguided item's crop position and flip
    guided, plain = _raw(files, "celebamaskhq"), D.RawFolderDataset(_opt("celebamaskhq", guiding_style_image=False),
                                                                     files["label_dir"], files["image_dir"], seed=DATASET["seed"])
    assert all(guided[i]["crop_pos"] == plain[i]["crop_pos"] and guided[i]["flip"] == plain[i]["flip"] for i in range(6))
    rng = random.Random(7)
    fd = D.FolderDataset(_opt("celebamaskhq"), files["label_dir"], files["image_dir"], seed=7, identities=files["celebamaskhq"])
    x, y, flip = rng.randint(0, 4), rng.randint(0, 4), int(rng.random() > 0.5)
    cands = fd.guide_candidates(0)
    item = fd[0]
    assert item["flip"] == flip and fd.by_id[cands[rng.randrange(len(cands))]][1].endswith(".jpg")
    assert fd.rng.random() == rng.random()      # four draws per guided item, in this order


def _numbered(tmp_path, names):
    from PIL import Image
    (tmp_path / "lab").mkdir()
    (tmp_path / "img").mkdir()
    for k, n in enumerate(names):
        Image.fromarray(np.full((12, 12), k, np.uint8)).save(str(tmp_path / "lab" / (n + ".png")))
        Image.fromarray(np.full((24, 24, 3), 10 * k, np.uint8)).save(str(tmp_path / "img" / (n + ".png")))
    return str(tmp_path / "lab"), str(tmp_path / "img")


def test_create_dataloader_maps_the_options(files, tmp_path):
    from deepsee_amd import data as D
    from deepsee_amd.options import DEFAULTS, make_opt
    want = dict(phase="train", identities_file="", dataset_mode="celebamaskhq", label_dir=None, image_dir=None,
                max_dataset_size=sys.maxsize, serial_batches=False, nThreads=0, label_preprocess_mode=None)
    assert {k: DEFAULTS[k] for k in want} == want
    base = dict(label_dir=files["label_dir"], image_dir=files["image_dir"])
    ld = D.create_dataloader(_opt("celebamaskhq", identities_file=files["celebamaskhq"], batchSize=4, nThreads=3, **base),
                             seed=9, shard=(1, 2))
    assert isinstance(ld.ds, D.RawFolderDataset) and ld.ds.identities is not None and ld.ds.dataset_mode == "celebamaskhq"
    assert (ld.bs, ld.shuffle, ld.drop_last, ld.workers, ld.seed, ld.rank, ld.world, ld.ds.seed) == (4, True, True, 3, 9, 1, 2, 9)
    assert ld.opt.label_preprocess_mode is None and ld.ds.exclude_self is False
    opt = _opt("celeba", "test", train=False, identities_file=files["celeba"], serial_batches=True, nThreads=64,
               max_dataset_size=4, **base)
    ld = D.create_dataloader(opt)
    assert (ld.bs, ld.shuffle, ld.drop_last, ld.workers) == (2, False, False, 16) and len(ld.ds) == 4 and len(ld) == 2
    assert opt.label_preprocess_mode == "resize" and ld.ds.dataset_mode == "celeba" and ld.ds.exclude_self is True
    # celeba: candidates come from the folder (max_dataset_size cuts the items only); celebamaskhq: from the items, like the reference
    assert ld.ds.guide_candidates(2) == ["000023"]
    hq = D.create_dataloader(_opt("celebamaskhq", identities_file=files["celebamaskhq"], max_dataset_size=4, **base))
    assert hq.ds.guide_candidates(2) == ["000010"] and hq.ds.guide_candidates(0) == ["000002", "000005", "000011"]
    assert isinstance(D.create_dataloader(_opt("celebamaskhq", identities_file=files["celebamaskhq"], nThreads=8, **base),
                                          raw=False).ds, D.FolderDataset)
    plain = D.create_dataloader(_opt("celebamaskhq", guiding_style_image=False, **base))
    assert plain.ds.identities is None and set(plain.ds[0]) == {"image_raw", "label_raw", "crop_pos", "flip", "path"}
    # the reference's two assertions, an unknown dataset_mode, missing folders
    with pytest.raises(AssertionError, match="Please provide an identity file."):
        D.create_dataloader(_opt("celebamaskhq", **base))
    with pytest.raises(AssertionError, match=r"Please provide a correct path to the identities file \(invalid path: /no/such\.csv\)"):
        D.create_dataloader(_opt("celeba", identities_file="/no/such.csv", **base))
    with pytest.raises(ValueError, match="dataset_mode"):
        D.create_dataloader(make_opt(dataset_mode="ade20k", **base))
    with pytest.raises(ValueError, match="dataset_mode"):
        D.RawFolderDataset(make_opt(), base["label_dir"], base["image_dir"], dataset_mode="ade20k")
    with pytest.raises(ValueError, match="label_dir"):
        D.create_dataloader(make_opt())
    # natural order (2 before 10) and truncation; the default order of the datasets stays the sorted stems
    lab, img = _numbered(tmp_path, ["10", "2", "1", "a10", "a9"])
    ld = D.create_dataloader(make_opt(label_dir=lab, image_dir=img, load_size=12, crop_size=8, max_dataset_size=4))
    assert [os.path.basename(p) for _, p in ld.ds.items] == ["1.png", "2.png", "10.png", "a9.png"]
    assert [os.path.basename(p) for _, p in D.RawFolderDataset(make_opt(), lab, img).items] == \
        ["1.png", "10.png", "2.png", "a10.png", "a9.png"]
    with pytest.raises(ValueError, match="order"):
        D.RawFolderDataset(make_opt(), lab, img, order="random")


def test_label_preprocess_mode_geometry():
    """CelebA: images centre-cropped and resized, label maps only resized (celeba_dataset.py:53-55), get_params as the image."""
    from deepsee_amd import resample as R
    opt = _opt("celeba")
    assert R.load_geometry(opt, (24, 24)) == {"box": (2, 2, 20, 20), "resize": (12, 12), "window": (0, 0, 12, 12), "out": (12, 12)}
    assert R.load_geometry(opt, (12, 12), mode="resize") == {"box": (0, 0, 12, 12), "resize": (12, 12), "window": (0, 0, 12, 12),
                                                             "out": (12, 12)}
    assert R.load_geometry(opt, (16, 10), (3, 1), mode="resize")["out"] == (12, 12)
    with pytest.raises(ValueError, match="resize"):
        R.load_geometry(opt, (12, 12), mode="stretch")
    with pytest.raises(ValueError, match="preprocess_mode"):          # 'resize' is a label mode, not an opt.preprocess_mode
        R.load_geometry(_opt("celeba", preprocess_mode="resize"), (12, 12))
    # get_params keeps opt.preprocess_mode and the label file's size: a position is drawn (and ignored by both geometries)
    for i, want in enumerate(CASES["celeba"]["cases"]["train/train_flips"]):
        got = R.crop_params(opt, (12, 12), random.Random(GG.item_seed(i)))
        assert want["params_size"] == [12, 12] and list(got["crop_pos"]) == want["crop_pos"] and got["flip"] == want["flip"]
    assert any(want["crop_pos"] != [0, 0] for want in CASES["celeba"]["cases"]["train/train_flips"])


class _Stub:
    thread_safe = True

    def __init__(self, n=5, bad=2, exc=None):
        self.n, self.bad, self.exc, self.epochs = n, bad, exc, []

    def __len__(self):
        return self.n

    def set_epoch(self, e):
        self.epochs.append(e)

    def __getitem__(self, i):
        if i == self.bad:
            raise self.exc
        return {"label": np.full((2, 2), i, np.uint8), "image": np.full((2, 2, 3), i, np.uint8), "flip": 0, "path": "item%d" % i}


@pytest.mark.parametrize("workers", [0, 2])
def test_a_skipped_batch_does_not_end_the_epoch(host_only, workers):
    from deepsee_amd import data as D
    from deepsee_amd.options import make_opt
    opt = make_opt()
    ld = D.DeviceLoader(_Stub(exc=D.SkipSampleException("no guide for item2")), opt, batch_size=1, shuffle=False,
                        drop_last=False, workers=workers)
    assert len(ld) == 5
    it = iter(ld)
    assert iter(it) is it and ld.ds.epochs == []             # nothing runs before the first next()
    assert next(it)["path"] == ["item0"] and next(it)["path"] == ["item1"] and ld.ds.epochs == [0]
    with pytest.raises(D.SkipSampleException, match="item2"):
        next(it)
    assert next(it)["path"] == ["item3"] and next(it)["path"] == ["item4"]
    with pytest.raises(StopIteration):
        next(it)
    with pytest.raises(StopIteration):
        next(it)
    assert ld.pool is None and len(ld) == 5 and ld.epoch == 1
    # a consumer that skips on ValueError (InferenceManager.run) sees every other item; a plain for loop sees the exception
    got, skipped, it = [], 0, iter(ld)
    while True:
        try:
            got += next(it)["path"]
        except ValueError:
            skipped += 1
        except StopIteration:
            break
    assert got == ["item0", "item1", "item3", "item4"] and skipped == 1
    # the first and the last batch of an epoch
    for bad, want in ((0, ["item1", "item2", "item3", "item4"]), (4, ["item0", "item1", "item2", "item3"])):
        ld = D.DeviceLoader(_Stub(bad=bad, exc=D.SkipSampleException("x")), opt, batch_size=1, shuffle=False, drop_last=False,
                            workers=workers)
        got, it = [], iter(ld)
        for _ in range(5):
            try:
                got += next(it)["path"]
            except D.SkipSampleException:
                pass
        assert got == want
        with pytest.raises(StopIteration):
            next(it)
    # any other exception behaves as before: raised by the next() during which the batch was staged (one batch ahead), and the
    # iteration is over
    for exc in (ValueError("broken file"), KeyError("item2")):
        ld = D.DeviceLoader(_Stub(exc=exc), opt, batch_size=1, shuffle=False, drop_last=False, workers=workers)
        it = iter(ld)
        assert next(it)["path"] == ["item0"]
        with pytest.raises(type(exc)):
            next(it)
        with pytest.raises(StopIteration):
            next(it)
        assert ld.pool is None
