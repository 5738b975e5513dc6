"""The load-time geometry and the LR downsampling on the device: dsee_resample_u8 against the pixels the reference's own
get_transform produced with Pillow (tests/golden/loader, tools/gen_golden_loader.py) bit for bit, the raw path of
device_preprocess per preprocess_mode, dsee_interp_down against the reference's Preprocessor.downsample_image and float64, and
the DeviceLoader over raw files with and without worker threads."""
import numpy as np
import pytest
import torch

from tools import gen_golden_loader as G

pytestmark = pytest.mark.gpu

GEO = G.load("geometry")["cases"]
LR = G.load("lr")["cases"]


def nhwc(x):
    from deepsee_amd import ops
    return ops.to_nhwc(x.cuda())


def nchw(x, c=3):
    from deepsee_amd import ops
    return ops.to_nchw(x.contiguous(), c).cpu()


def _write_pairs(tmp_path, n, img_hw=(40, 48), lab_hw=(20, 24)):
    from PIL import Image
    (tmp_path / "lab").mkdir()
    (tmp_path / "img").mkdir()
    rng = np.random.default_rng(0)
    for i in range(n):
        Image.fromarray(rng.integers(0, 19, lab_hw, dtype=np.uint8)).save(str(tmp_path / "lab" / ("%03d.png" % i)))
        Image.fromarray(rng.integers(0, 256, img_hw + (3,), dtype=np.uint8)).save(str(tmp_path / "img" / ("%03d.png" % i)))


def _opt(case, **over):
    opt = G.case_opt(case)
    for k, v in dict(start_size=4, label_nc=19, **over).items():
        setattr(opt, k, v)
    return opt


@pytest.mark.parametrize("name", sorted(GEO))
def test_resample_u8_equals_the_reference_pixels(name):
    """C = 3 (the image batch, the case's filter), C = 1 (the label batch, NEAREST) and C = 1 with the case's filter (one channel
    of the image batch as a [N, H, W] map: Pillow treats the bands of an image alike)."""
    from deepsee_amd import data as D
    case = GEO[name]
    opt = _opt(case)
    img, lab = torch.from_numpy(G.unpack_u8(case["image_src"])), torch.from_numpy(G.unpack_u8(case["label_src"]))
    want_img, want_lab = torch.from_numpy(G.unpack_u8(case["image_out"])), torch.from_numpy(G.unpack_u8(case["label_out"]))
    got = D.resample_raw(opt, img, case["crop_pos"], case["filter"])
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want_img)
    got = D.resample_raw(opt, lab, case["crop_pos"], "nearest")
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want_lab)
    if lab.shape == img.shape[:3]:
        got = D.resample_raw(opt, img[..., 1].contiguous(), case["crop_pos"], case["filter"])
        assert torch.equal(got.cpu(), want_img[..., 1])


@pytest.mark.parametrize("name", sorted(GEO))
def test_raw_device_preprocess_per_mode(name):
    """Raw batch -> device_preprocess == the existing kernels run on the reference's uint8 crop, in every output, bit for bit."""
    from deepsee_amd import data as D
    case = GEO[name]
    opt = _opt(case)
    flip = torch.tensor([0, 1], dtype=torch.uint8)
    raw = {"image_raw": torch.from_numpy(G.unpack_u8(case["image_src"])), "label_raw": [a for a in G.unpack_u8(case["label_src"])],
           "crop_pos": [tuple(p) for p in case["crop_pos"]], "flip": flip, "path": ["a", "b"]}
    wire = {"image": torch.from_numpy(G.unpack_u8(case["image_out"])), "label": torch.from_numpy(G.unpack_u8(case["label_out"])),
            "flip": flip}
    got, want = D.device_preprocess(opt, raw), D.device_preprocess(opt, wire)
    torch.cuda.synchronize()
    assert got["path"] == ["a", "b"] and got["image_hr"].dsee_layout == "nhwc"
    assert torch.equal(got["image_hr"], want["image_hr"]) and torch.equal(got["image_lr"], want["image_lr"])
    assert torch.equal(got["input_semantics"].t, want["input_semantics"].t)
    assert int(want["input_semantics"].t.max()) == 19                        # the 255 of the label files arrived as label_nc
    # ... which is outside [0, nc) without a dontcare class (an all-zero one-hot vector in every kernel: label.hip,
    # tests/test_gpu_label_nc.py) and class 19 of 20 with one
    assert want["input_semantics"].nc == 19
    from deepsee_amd.options import make_opt
    dc = make_opt(**dict({k: v for k, v in vars(opt).items() if k != "semantic_nc"}, contain_dontcare_label=True))
    with_dc = D.device_preprocess(dc, wire)
    assert with_dc["input_semantics"].nc == 20 and torch.equal(with_dc["input_semantics"].t, want["input_semantics"].t)
    raw.update(guiding_image_raw=raw["image_raw"], guiding_label_raw=raw["label_raw"])
    guided = D.device_preprocess(opt, raw)
    assert torch.equal(guided["guiding_image"], want["image_hr"]) and torch.equal(guided["guiding_label"].t, want["input_semantics"].t)


def test_resample_u8_many_blocks_against_pillow():
    """More than one block, a window that needs a strict subset of the source rows, per-sample crop positions: 200 x 264 files
    resized to 64 x 64 and cropped to 48 x 48, against Pillow run here."""
    from PIL import Image
    from deepsee_amd import data as D, resample as R
    from deepsee_amd.options import make_opt
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, (3, 200, 264, 3), dtype=np.uint8)
    src[1, ::2] = np.where(rng.random((100, 264, 3)) < 0.5, 0, 255)
    pos = [(0, 0), (16, 16), (5, 11)]
    for method, pf in (("bicubic", Image.BICUBIC), ("bilinear", Image.BILINEAR), ("nearest", Image.NEAREST)):
        opt = make_opt(preprocess_mode="resize_and_crop", load_size=64, crop_size=48, downsampling_method=method)
        want = np.stack([np.asarray(Image.fromarray(src[n]).resize((64, 64), pf).crop((x, y, x + 48, y + 48)))
                         for n, (x, y) in enumerate(pos)])
        got = D.resample_raw(opt, torch.from_numpy(src), pos, method)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), method
    tab = R.batch_tables([R.load_geometry(opt, (264, 200), p) for p in pos], "bicubic")
    assert tab["tmp_rows"] < 200 and len({tuple(r) for r in tab["rows"].tolist()}) == 3


def test_raw_batch_equals_pil_prepared_batch(tmp_path):
    """resize_and_crop: device_preprocess of raw samples == device_preprocess of the same samples prepared with PIL the way
    FolderDataset prepares them (resize to load_size, NEAREST / BICUBIC, one crop), in all three outputs."""
    from PIL import Image
    from deepsee_amd import data as D
    from deepsee_amd.options import make_opt
    _write_pairs(tmp_path, n=4)
    opt = make_opt(preprocess_mode="resize_and_crop", load_size=16, crop_size=8, start_size=4)
    ds = D.RawFolderDataset(opt, str(tmp_path / "lab"), str(tmp_path / "img"), seed=3)
    ld = D.DeviceLoader(ds, opt, batch_size=4, shuffle=False)
    samples = [ds[i] for i in range(4)]
    assert len({s["crop_pos"] for s in samples}) > 1
    prepared = []
    for s, (lp, ip) in zip(samples, ds.items):
        x, y = s["crop_pos"]
        box = (x, y, x + 8, y + 8)
        prepared.append({"label": np.asarray(Image.open(lp).resize((16, 16), Image.NEAREST).crop(box), dtype=np.uint8),
                         "image": np.asarray(Image.open(ip).convert("RGB").resize((16, 16), Image.BICUBIC).crop(box), dtype=np.uint8),
                         "flip": s["flip"], "path": s["path"]})
    got, want = D.device_preprocess(opt, ld.collate(samples)), D.device_preprocess(opt, ld.collate(prepared))
    torch.cuda.synchronize()
    assert tuple(got["image_hr"].shape) == (4, 8, 8, 4) and tuple(got["image_lr"].shape) == (4, 4, 4, 4)
    for k in ("image_hr", "image_lr"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["input_semantics"].t, want["input_semantics"].t)
    with pytest.raises(ValueError, match=r"first\.png.*second\.png"):
        D.device_preprocess(opt, {"image_raw": [samples[0]["image_raw"], samples[1]["image_raw"][:-1]],
                                  "label_raw": [samples[0]["label_raw"], samples[1]["label_raw"]],
                                  "crop_pos": [(0, 0), (0, 0)], "path": ["first.png", "second.png"]})


@pytest.mark.parametrize("name", sorted(LR))
def test_interp_down_against_the_reference_and_float64(name):
    """nearest: the reference's own fp32 result, bit for bit.  bilinear, area: within the LR bound of F.interpolate on the float64
    input (1e-6, or twice the reference's own fp32 error where that misses 1e-6: tools/gen_golden_loader.lr_bound)."""
    from deepsee_amd import ops
    rec = LR[name]
    x, s = G.unpack_f32(rec["input"]), rec["start_size"]
    xd = nhwc(x)
    for mode in ("nearest", "bilinear", "area"):
        y = ops.interp_down(xd, s, mode)
        assert tuple(y.shape) == (2, s, s, 4) and y.dsee_layout == "nhwc" and float(y[..., 3].abs().max()) == 0.0
        got = nchw(y)
        err, bound = G.rel(got, G.lr_float64(x, s, mode)), G.lr_bound(rec, mode)
        print("%s %-8s vs float64 %.2e (bound %.2e), vs the reference's fp32 %.2e"
              % (name, mode, err, bound, G.rel(got, G.unpack_f32(rec["output"][mode]))))
        if mode == "nearest":
            assert torch.equal(got, G.unpack_f32(rec["output"][mode]))
        assert err < bound, (mode, err, bound)


def test_interp_down_production_shape():
    """256^2 -> 32^2 (several blocks; an integer ratio, at which fp32 source coordinates are exact: the plain 1e-6 bound) and a
    rectangular 96 x 160 source, against F.interpolate: float64 for bilinear / area, fp32 (bit for bit) for nearest."""
    import torch.nn.functional as F
    from deepsee_amd import ops
    g = torch.Generator().manual_seed(5)
    for n, h, w, s in ((2, 256, 256, 32), (3, 96, 160, 32)):
        x = torch.rand(n, 3, h, w, generator=g) * 2.4 - 1.2                  # the clamp is reached
        xd = nhwc(x)
        for mode in ("bilinear", "area"):
            err = G.rel(nchw(ops.interp_down(xd, s, mode)), G.lr_float64(x, s, mode))
            print("%dx%d -> %d %s %.2e" % (h, w, s, mode, err))
            assert err < G.LR_BOUND
        assert torch.equal(nchw(ops.interp_down(xd, s, "nearest")), F.interpolate(x, (s, s), mode="nearest").clamp(-1, 1))


def test_downsampling_method_selects_the_lr_kernel():
    from deepsee_amd import data as D, ops
    from deepsee_amd.managers import BaseManager
    from deepsee_amd.options import make_opt
    g = torch.Generator().manual_seed(9)
    img = torch.rand(2, 3, 32, 32, generator=g) * 2 - 1
    label = torch.randint(0, 19, (2, 1, 32, 32), generator=g).float()
    u8 = {"image": torch.randint(0, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8),
          "label": torch.randint(0, 19, (2, 32, 32), generator=g, dtype=torch.uint8)}
    lrs = {}
    for method in ("bicubic", "bilinear", "nearest", "area"):
        opt = make_opt(start_size=4, crop_size=32, load_size=32, batchSize=2, downsampling_method=method)
        mgr = BaseManager(opt, create_model=False)
        out = mgr.preprocess({"image": img, "label": label}, from_dataloader=True)
        dev = D.device_preprocess(opt, u8)
        for res in (out, dev):
            hr = res["image_hr"]
            want = ops.bicubic_down(hr, 4) if method == "bicubic" else ops.interp_down(hr, 4, method)
            assert torch.equal(res["image_lr"], want), method
        lrs[method] = out["image_lr"]
    default = BaseManager(make_opt(start_size=4, crop_size=32, load_size=32, batchSize=2), create_model=False)
    assert torch.equal(default.preprocess({"image": img, "label": label}, True)["image_lr"], lrs["bicubic"])
    assert torch.equal(lrs["bicubic"], ops.bicubic_down(nhwc(img), 4))
    assert not torch.equal(lrs["bilinear"], lrs["bicubic"]) and not torch.equal(lrs["bilinear"], lrs["area"])
    assert G.rel(nchw(lrs["bilinear"]), G.lr_float64(img, 4, "bilinear")) < G.LR_BOUND
    bad = make_opt(start_size=4, crop_size=32, load_size=32, batchSize=2, downsampling_method="linear")
    with pytest.raises(ValueError, match="bicubic, bilinear, nearest, area"):
        BaseManager(bad, create_model=False).preprocess({"image": img, "label": label}, from_dataloader=True)
    with pytest.raises(ValueError, match="bicubic, bilinear, nearest, area"):
        D.device_preprocess(bad, u8)


def test_device_loader_over_raw_files_with_workers(tmp_path):
    from deepsee_amd import data as D
    from deepsee_amd.options import make_opt
    _write_pairs(tmp_path, n=4)
    opt = make_opt(preprocess_mode="scale_width_and_crop", load_size=16, crop_size=8, start_size=4, batchSize=2)
    runs = []
    for workers in (0, 2):
        ds = D.RawFolderDataset(opt, str(tmp_path / "lab"), str(tmp_path / "img"), seed=6)
        ld = D.DeviceLoader(ds, opt, shuffle=True, seed=2, workers=workers)
        epochs = []
        for _ in range(2):
            batches = list(ld)
            torch.cuda.synchronize()
            assert len(batches) == 2 and tuple(batches[0]["image_hr"].shape) == (2, 8, 8, 4)
            epochs.append(batches)
        assert ld.pool is None
        runs.append(epochs)
    for e in range(2):
        for a, b in zip(runs[0][e], runs[1][e]):
            assert a["path"] == b["path"] and torch.equal(a["image_hr"], b["image_hr"]) and torch.equal(a["image_lr"], b["image_lr"])
            assert torch.equal(a["input_semantics"].t, b["input_semantics"].t)
    first, second = runs[0]
    assert sorted(p for b in first for p in b["path"]) == sorted(p for b in second for p in b["path"])
