"""Identity-paired guiding images through the device loader: DeviceLoader over the guided RawFolderDataset of both dataset modes
against the tensors the reference's CelebAMaskHQDataset / CelebADataset returned (tests/golden/guided_loader,
tools/gen_golden_guided_loader.py) bit for bit, samples and guides in one dsee_resample_u8 call each for images and label maps,
a training step and a validation run of the guided model from files."""
import warnings

import numpy as np
import pytest
import torch

from tools import gen_golden_guided_loader as GG

pytestmark = pytest.mark.gpu

DATASET = GG.load("dataset")
CASES = {mode: GG.load(mode) for mode in ("celebamaskhq", "celeba")}
IDS = DATASET["ids"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return GG.write_files(DATASET, str(tmp_path_factory.mktemp("guided")))


@pytest.fixture(scope="module")
def files40(tmp_path_factory):
    return GG.write_files(DATASET, str(tmp_path_factory.mktemp("guided40")), image_hw=(40, 40))


def _opt(mode, files, phase="train", train=True, **over):
    from deepsee_amd.options import make_opt
    d = dict(CASES[mode]["opt"], start_size=4, batchSize=2, guiding_style_image=True, phase=phase, isTrain=train, dataset_mode=mode,
             label_dir=files["label_dir"], image_dir=files["image_dir"], identities_file=files[mode], serial_batches=True)
    d.update(over)
    return make_opt(**d)


def _wire(items, key):
    return torch.from_numpy(np.stack([GG.unpack_u8(it[key]) for it in items]))


@pytest.mark.parametrize("key", ["train/train_flips", "val/no_flips"])
@pytest.mark.parametrize("mode", sorted(CASES))
def test_loader_reproduces_the_reference_items(files, mode, key):
    """image_hr and guiding_image: the device's normalise of the reference's own (already flipped) uint8 pixels; the label maps:
    the reference's values themselves, with the guide's 255 as label_nc (the reference forgets that remap for the guide)."""
    from deepsee_amd import data as D
    phase, flips = key.split("/")
    opt = _opt(mode, files, phase, flips == "train_flips")
    ld = D.create_dataloader(opt, seed=DATASET["seed"])
    assert ld.drop_last == opt.isTrain and (opt.label_preprocess_mode == "resize") == (mode == "celeba")
    want = CASES[mode]["cases"][key]
    it, seen = iter(ld), {"flip": 0, "guide255": 0, "skipped": 0}
    for k in range(3):
        items = want[2 * k:2 * k + 2]
        if any(w["raised"] for w in items):
            with pytest.raises(D.SkipSampleException, match="000100"):
                next(it)
            seen["skipped"] += 1
            continue
        got = next(it)
        torch.cuda.synchronize()
        assert [p[-10:] for p in got["path"]] == [w["id"] + ".jpg" for w in items]
        assert [p[-10:] for p in got["guiding_path"]] == [w["guide"] + ".jpg" for w in items]
        ref = D.device_preprocess(opt, {"image": _wire(items, "image"), "label": _wire(items, "label"),
                                        "guiding_image": _wire(items, "guiding_image"), "guiding_label": _wire(items, "guiding_label")})
        glab = _wire(items, "guiding_label")
        seen["flip"] += sum(bool(w["flip"]) for w in items)
        seen["guide255"] += int((glab == 255).sum())
        assert torch.equal(got["image_hr"], ref["image_hr"]) and torch.equal(got["image_lr"], ref["image_lr"])
        assert torch.equal(got["guiding_image"], ref["guiding_image"])
        assert torch.equal(got["input_semantics"].t.cpu(), _wire(items, "label"))
        assert torch.equal(got["guiding_label"].t.cpu(), torch.where(glab == 255, torch.full_like(glab, opt.label_nc), glab))
        assert got["guiding_label"].nc == got["input_semantics"].nc == 19 and got["guiding_image"].dsee_layout == "nhwc"
        side = 8 if mode == "celebamaskhq" else 12
        assert tuple(got["image_hr"].shape) == tuple(got["guiding_image"].shape) == (2, side, side, 4)
    with pytest.raises(StopIteration):
        next(it)
    assert seen["guide255"] > 0 and seen["skipped"] == (1 if key == "val/no_flips" and mode == "celebamaskhq" else 0)
    assert (seen["flip"] > 0) == (flips == "train_flips")


@pytest.mark.parametrize("mode", sorted(CASES))
def test_guide_equals_the_unguided_pipeline_on_its_own_file(files, mode):
    from deepsee_amd import data as D
    opt = _opt(mode, files)
    ld = D.create_dataloader(opt, seed=DATASET["seed"])
    images, labels = GG.unpack_u8(DATASET["images"]), GG.unpack_u8(DATASET["labels"])
    plain = _opt(mode, files, guiding_style_image=False, label_preprocess_mode=opt.label_preprocess_mode)
    n = 0
    for got in ld:
        g = [IDS.index(p[-10:-4]) for p in got["guiding_path"]]
        pos = [ld.ds[IDS.index(p[-10:-4])]["crop_pos"] for p in got["path"]]
        flip = torch.tensor([ld.ds[IDS.index(p[-10:-4])]["flip"] for p in got["path"]], dtype=torch.uint8)
        own = D.device_preprocess(plain, {"image_raw": torch.from_numpy(images[g]), "label_raw": torch.from_numpy(labels[g]),
                                          "crop_pos": pos, "flip": flip})
        torch.cuda.synchronize()
        assert "guiding_image" not in own
        assert torch.equal(got["guiding_image"], own["image_hr"]) and torch.equal(got["guiding_label"].t, own["input_semantics"].t)
        n += 1
    assert n == 3


def test_samples_and_guides_share_the_resample_calls(files, monkeypatch):
    from deepsee_amd import data as D, ops
    calls = []
    real = ops.resample_u8

    def counted(src, *a, **kw):
        calls.append(tuple(src.shape))
        return real(src, *a, **kw)
    monkeypatch.setattr(ops, "resample_u8", counted)
    for mode in sorted(CASES):
        for guided in (True, False):
            calls.clear()
            ld = D.create_dataloader(_opt(mode, files, guiding_style_image=guided), seed=DATASET["seed"])
            batches = list(ld)
            n = 4 if guided else 2
            assert len(batches) == 3 and calls == [(n, 24, 24, 3), (n, 12, 12)] * 3, (mode, guided, calls)
            assert ("guiding_image" in batches[0]) == guided
    # guide files of another size: calls of their own, and the same bits as the shared calls give for the same pixels
    opt = _opt("celebamaskhq", files)
    ds = D.RawFolderDataset(opt, files["label_dir"], files["image_dir"], seed=DATASET["seed"])
    host = D.DeviceLoader(ds, opt, shuffle=False).collate([ds[0], ds[1]])
    calls.clear()
    shared = D.device_preprocess(opt, host)
    assert calls == [(4, 24, 24, 3), (4, 12, 12)]
    padded = dict(host)
    for k, rows in (("guiding_image_raw", 3), ("guiding_label_raw", 3)):                      # 27 x 24 images, 15 x 12 label maps
        padded[k] = torch.cat([host[k], torch.zeros_like(host[k][:, :rows])], 1)
    calls.clear()
    apart = D.device_preprocess(opt, padded)
    assert calls == [(2, 24, 24, 3), (2, 12, 12), (2, 27, 24, 3), (2, 15, 12)]
    for k in ("image_hr", "image_lr"):
        assert torch.equal(shared[k], apart[k]), k
    assert torch.equal(shared["input_semantics"].t, apart["input_semantics"].t)
    assert tuple(apart["guiding_image"].shape) == tuple(shared["guiding_image"].shape)
    assert not torch.equal(shared["guiding_image"], apart["guiding_image"])
    # ... and of the same size, passed as a caller's own lists: the shared calls again, the same bits
    calls.clear()
    lists = D.device_preprocess(opt, dict(host, **{k: [a.numpy() for a in host[k]] for k in
                                                   ("image_raw", "label_raw", "guiding_image_raw", "guiding_label_raw")}))
    assert calls == [(4, 24, 24, 3), (4, 12, 12)]
    assert torch.equal(lists["guiding_image"], shared["guiding_image"]) and torch.equal(lists["guiding_label"].t, shared["guiding_label"].t)


MODEL = dict(netE="fullstyle", noisy_style_scale=0.05, ngf=8, batchSize=2, start_size=4, crop_size=32, load_size=36,
             no_vgg_loss=True, preprocess_mode="resize_and_crop", center_crop_size=None, nThreads=2, serial_batches=False)


def _manager(opt):
    from deepsee_amd.managers import TrainerManager
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return TrainerManager(opt)


@pytest.mark.parametrize("graphs", [False, True])
def test_guided_model_trains_from_files(files40, graphs):
    from deepsee_amd import data as D
    opt = _opt("celebamaskhq", files40, hip_graphs=graphs, seed=3, **MODEL)
    ld = D.create_dataloader(opt, seed=4)
    assert ld.workers == 2 and len(ld) == 3
    tm = _manager(opt)
    name, p = next(iter(tm.sr_model.netE.named_parameters()))
    before = p.detach().clone()
    steps = 0
    for b in ld:
        assert tuple(b["guiding_image"].shape) == (2, 32, 32, 4) and tuple(b["guiding_label"].t.shape) == (2, 32, 32)
        tm.run_generator_one_step(b)
        tm.run_discriminator_one_step(b)
        losses = {k: float(v) for k, v in tm.get_latest_losses().items()}
        assert all(np.isfinite(v) for v in losses.values()), losses
        assert tuple(tm.get_latest_generated().shape) == (2, 3, 32, 32)
        steps += 1
        if steps == (2 if graphs else 1):
            break
    torch.cuda.synchronize()
    assert not torch.equal(p.detach(), before), name
    if graphs:
        assert tm.graph_stats["captured"] == 2, tm.graph_stats
    tm.close()


def test_validation_skips_the_sample_without_a_guide(files40):
    from deepsee_amd import data as D
    from deepsee_amd.managers import InferenceManager
    train = _opt("celebamaskhq", files40, hip_graphs=False, **MODEL)
    tm = _manager(train)
    val = _opt("celebamaskhq", files40, phase="val", train=False, **dict(MODEL, batchSize=1, serial_batches=True))
    ld = D.create_dataloader(val)
    assert len(ld) == 6 and not ld.drop_last and not ld.shuffle
    im = InferenceManager(val, num_samples=20)
    res = im.run(tm.sr_model, ld)
    assert im.skipped_samples == 1 and res["n_samples"] == 5 and tm.sr_model.training
    assert ld.pool is None
    tm.close()
