"""The output path on the MI355X: the four conversion kernels of deepsee_amd/csrc/visuals.hip against the numpy restatements of
tools/gen_golden_visuals.py (which tests/test_visuals_host.py holds to the reference's own results in
tests/golden/visuals/visuals.json), SRModel's "baseline" mode, and InferenceManager.run(..., mode=, save_to=) end to end: every
file, byte for byte, against the batch's own tensors."""
import json
import math
import os
import random
import warnings
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tools import gen_golden_visuals as G

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visuals", "visuals.json")
FILL = 0xAB
SMALL = dict(batchSize=2, ngf=8, nef=8, ndf=8)


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-20))


def native(x_nchw, fill=float("nan")):
    """Tagged native NHWC [N, H, W, 4] of an NCHW image; the padding channel holds `fill` (it must never be read as data)."""
    n, _, h, w = x_nchw.shape
    t = torch.full((n, h, w, 4), fill, dtype=torch.float32, device="cuda")
    t[..., :3] = x_nchw.cuda().permute(0, 2, 3, 1)
    t.dsee_layout = "nhwc"
    return t


# a destination larger than the image: (byte offset of the first image, row stride, x offset, gap between images).
#   "aligned": base and strides are multiples of 4 -- whole 4-pixel groups leave as 4-byte stores, the groups cut by the window's
#              edges as bytes (x offset 3, width 7: absolute pixels 3..9 = one pixel of group 0, group 1 whole, two of group 2);
#   "ragged":  nothing is a multiple of 4 -- the byte path alone.
WINDOWS = {"aligned": dict(offset=8, x_offset=3, align=4), "ragged": dict(offset=5, x_offset=2, align=1)}


def window_for(n, h, w, offset, x_offset, align):
    """(buffer filled with FILL, Window, boolean mask of the bytes the window covers)."""
    from deepsee_amd.visuals import Window
    row = 3 * (x_offset + w) + 5
    image = h * row + 7
    if align > 1:
        row = -(-row // align) * align
        image = -(-(h * row + 7) // align) * align
    else:
        row |= 1
        image = (h * row + 7) | 1
    assert (row % 4 == 0 and image % 4 == 0) == (align == 4)
    size = offset + n * image + 13
    buf = torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
    mask = np.zeros(size, dtype=bool)
    for i in range(n):
        for y in range(h):
            start = offset + i * image + y * row + 3 * x_offset
            mask[start:start + 3 * w] = True
    return buf, Window(buf, offset, image, row, x_offset), mask


def read_window(buf, mask, n, h, w):
    host = buf.cpu().numpy()
    assert (host[~mask] == FILL).all(), "bytes outside the window were written"
    return host[mask].reshape(n, h, w, 3)


# ---- dsee_image_to_u8
@pytest.mark.parametrize("window", sorted(WINDOWS))
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_image_to_u8_is_bit_identical_to_numpy(layout, normalize, window):
    """The issue asks for ONE N = 2, 5 x 7 input holding all 256 level centres, their fp32 neighbours on both sides and +-1, +-1.5,
    +-0: 774 values, while 2 x 3 x 5 x 7 holds 210.  The shape is kept and the values are fed as four such inputs
    (tools.gen_golden_visuals.crafted_chunks), each through the same call."""
    from deepsee_amd import visuals as V
    mismatches = total = 0
    for chunk in G.crafted_chunks():
        n, _, h, w = chunk.shape
        assert (n, h, w) == (2, 5, 7)
        want = np.stack([G.np_tensor2im(chunk[b].numpy(), normalize) for b in range(n)])
        buf, win, mask = window_for(n, h, w, **WINDOWS[window])
        assert (buf.data_ptr() + win.offset) % 4 == (0 if window == "aligned" else 1)
        V.image_to_u8(native(chunk) if layout == "nhwc" else chunk.cuda(), win, normalize)
        got = read_window(buf, mask, n, h, w)
        mismatches += int((got != want).sum())
        total += want.size
    print("%s normalize=%s %s: %d mismatches of %d" % (layout, normalize, window, mismatches, total))
    assert mismatches == 0


def test_tensor2im_shapes_and_fixture(gold):
    from deepsee_amd.visuals import tensor2im
    chunks = G.crafted_chunks()
    for i, c in enumerate(chunks):
        assert tensor2im(c).tolist() == gold["tensor2im"]["normalize"][i]               # NCHW batch, host tensor
        assert tensor2im(native(c)).tolist() == gold["tensor2im"]["normalize"][i]       # native batch
        assert tensor2im(c[1], normalize=False).tolist() == gold["tensor2im"]["plain"][i][1]      # one image: [H, W, 3]
    c = chunks[0]
    one = tensor2im(c[0, :1])                                                           # single channel: [H, W]
    assert one.shape == (5, 7) and np.array_equal(one, G.np_tensor2im(c[0].numpy())[..., 0])
    assert np.array_equal(tensor2im(c[0, 0]), one)                                      # 2-D input
    batch = torch.cat([c, c, c[:1]])                                                    # 5 images, tiled 4 per row
    tiled = tensor2im(batch, tile=True)
    assert tiled.shape == (10, 28, 3) and not tiled[5:, 7:].any()
    assert np.array_equal(tiled[:5, 7:14], G.np_tensor2im(c[1].numpy()))
    assert [t.shape for t in tensor2im([c[0], c[1]])] == [(5, 7, 3)] * 2


# ---- dsee_label_colorize
@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_label_colorize_matches_fixture_and_blacks_out_of_range(gold, window):
    from deepsee_amd import visuals as V
    base = G.label_map()
    lab = np.stack([base, base[::-1]]).copy()
    out_of_range = [(0, 0, 0, 21), (0, 5, 7, 255), (0, 15, 15, 21), (1, 3, 2, 255), (1, 9, 13, 22)]
    for n, y, x, v in out_of_range:
        lab[n, y, x] = v
    want = np.array(gold["tensor2label"]["batch"], dtype=np.uint8)                      # the reference, for indices 0..20
    for n, y, x, _ in out_of_range:
        want[n, y, x] = 0                                                               # Colorize leaves unmatched pixels black
    assert np.array_equal(want, G.np_colorize(lab, V.labelcolormap(21)))
    buf, win, mask = window_for(2, 16, 16, **WINDOWS[window])
    V.label_colorize(torch.from_numpy(lab).cuda(), 21, win)
    got = read_window(buf, mask, 2, 16, 16)
    assert np.array_equal(got, want), int((got != want).sum())


def test_tensor2label_inputs_and_tiling(gold):
    from deepsee_amd import ops
    from deepsee_amd.visuals import tensor2label
    base = G.label_map()
    idx = torch.from_numpy(base.astype(np.int64))
    onehot = F.one_hot(idx, 21).permute(2, 0, 1).float()
    single, batch = gold["tensor2label"]["single"], gold["tensor2label"]["batch"]
    assert tensor2label(onehot, 21).tolist() == single                                  # one-hot [C, H, W] -> [H, W, 3]
    assert tensor2label(torch.stack([onehot, onehot.flip(1)]), 21).tolist() == batch
    lab = torch.from_numpy(np.stack([base, base[::-1]]).copy()).cuda()
    assert tensor2label(ops.Labels(lab, 19), 21).tolist() == batch                      # the native label map
    assert tensor2label(lab[0], 21).tolist() == single
    five = torch.cat([lab, lab, lab[:1]])
    tiled = tensor2label(five, 21, tile=True, picturesPerRow=2)                         # 5 maps, 2 per row: 3 rows, 1 zero map
    assert tiled.shape == (48, 32, 3) and not tiled[32:, 16:].any() and tiled[:16, :16].tolist() == single
    assert tensor2label(torch.zeros(3), 21).shape == (64, 64, 3)


# ---- dsee_bicubic_up
@pytest.mark.parametrize("name", sorted(G.BICUBIC))
def test_bicubic_up_matches_interpolate(gold, name):
    from deepsee_amd import ops
    case = G.BICUBIC[name]
    x = G.bicubic_input(case)
    want = G.bicubic_reference(case)
    assert float(F.interpolate(x, (case["H"], case["W"]), mode="bicubic").abs().max()) > 1.0       # the clamp has work to do
    y = ops.bicubic_up(native(x, fill=1e30), case["H"], case["W"], clamp=True)
    assert tuple(y.shape) == (2, case["H"], case["W"], 4) and y.dsee_layout == "nhwc"
    assert float(y[..., 3].abs().max()) == 0.0                                          # the padding channel is written as 0
    got = ops.to_nchw(y, 3).cpu()
    err = rel(got, want)
    fix = torch.tensor(gold["bicubic"][name]["values"], dtype=torch.float64)
    err_fix = rel(got.reshape(-1)[::G.STRIDE], fix)
    print("%s: rel. error %.3e against F.interpolate on the CPU, %.3e against the fixture" % (name, err, err_fix))
    assert err < 1e-6 and err_fix < 1e-6
    assert float(got.max()) <= 1.0 and float(got.min()) >= -1.0


def test_bicubic_up_overshoots_without_the_clamp():
    from deepsee_amd import ops
    x = -torch.ones(2, 3, 4, 4)
    x[..., 2:] = 1.0                                                                    # a step edge
    want = F.interpolate(x, (32, 32), mode="bicubic")
    raw = ops.to_nchw(ops.bicubic_up(native(x), 32, 32, clamp=False), 3).cpu()
    assert rel(raw, want) < 1e-6
    assert float(raw.max()) > 1.05 and float(raw.min()) < -1.05
    clamped = ops.to_nchw(ops.bicubic_up(native(x), 32, 32, clamp=True), 3).cpu()
    assert float(clamped.max()) == 1.0 and float(clamped.min()) == -1.0 and rel(clamped, want.clamp(-1, 1)) < 1e-6


# ---- dsee_bilinear_up_u8
@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_bilinear_up_u8_matches_the_stated_formula(window):
    from deepsee_amd import visuals as V
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, size=(2, 4, 4, 3), dtype=np.uint8)
    src[1, :, 2:] = 255
    src[1, :, :2] = 0                                                                   # a full-range edge as well
    want = np.stack([G.np_bilinear_up(src[b], 32, 32) for b in range(2)])
    sbuf = torch.from_numpy(src.reshape(-1).copy()).cuda()
    buf, win, mask = window_for(2, 32, 32, **WINDOWS[window])
    V.bilinear_up_u8(V.Window(sbuf, 0, 48, 12), 2, 4, win, 32, 32)
    got = read_window(buf, mask, 2, 32, 32)
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    share = float((diff == 0).mean())
    # every operation is rounded as the formula says, so equality is expected; a difference in evaluation order could only move
    # a value across a .5 boundary, i.e. by one level
    assert diff.max() <= 1, "max |difference| %d levels; exact-match share %.4f" % (diff.max(), share)
    print("bilinear 4 -> 32 (%s): exact-match share %.4f" % (window, share))


# ---- the model and the manager
def _opt(variant):
    from deepsee_amd.options import make_opt
    if variant == "guided":
        return make_opt("guided_8x_256", start_size=4, crop_size=32, load_size=32, **SMALL)
    return make_opt("independent_8x_32", **SMALL)


def _manager(opt):
    from deepsee_amd.managers import TrainerManager
    random.seed(1)
    torch.manual_seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return TrainerManager(opt)


def _loader(opt):
    from deepsee_amd.data import DeviceLoader, SyntheticDataset
    return DeviceLoader(SyntheticDataset(opt, length=4), opt, shuffle=False)


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _host_images(t):
    """numpy fp32 [N, 3, H, W] of a native or NCHW device image."""
    if getattr(t, "dsee_layout", None) == "nhwc":
        t = t.detach()[..., :3].permute(0, 3, 1, 2)
    return t.detach().cpu().numpy()


def _expected_files(out, n_label):
    """{key: uint8 [N, h, w, 3]} by the numpy restatements, from the batch's own tensors copied to the host."""
    from deepsee_amd.visuals import labelcolormap
    table = labelcolormap(n_label)
    want = OrderedDict()
    want["input_semantics"] = G.np_colorize(out["input_semantics"].t.cpu().numpy(), table)
    for k in ("image_lr", "fake_image", "image_hr"):
        want[k] = np.stack([G.np_tensor2im(img) for img in _host_images(out[k])])
    if "guiding_image" in out:
        want["guiding_image"] = np.stack([G.np_tensor2im(img) for img in _host_images(out["guiding_image"])])
        want["guiding_input_label"] = G.np_colorize(out["guiding_label"].t.cpu().numpy(), table)
    return want


@pytest.mark.parametrize("variant", ["independent", "guided"])
def test_run_with_save_to_writes_every_file(tmp_path, variant):
    from PIL import Image
    from deepsee_amd.managers import InferenceManager
    opt = _opt(variant)
    tm = _manager(opt)
    model = tm.sr_model
    folder = str(tmp_path / "out")
    res_plain = InferenceManager(opt, num_samples=3).run(model, _loader(opt))
    res_saved = InferenceManager(opt, num_samples=3).run(model, _loader(opt), save_to=folder)
    assert model.training and res_saved["n_samples"] == 4
    assert list(res_plain) == list(res_saved)
    for k in res_plain:
        assert same(float(res_plain[k]), float(res_saved[k])), (k, res_plain[k], res_saved[k])
    keys = ["input_semantics", "image_lr", "fake_image", "image_hr"] + (
        ["guiding_image", "guiding_input_label"] if variant == "guided" else [])
    assert sorted(os.listdir(folder)) == sorted(keys + ["combined"])
    for k in keys + ["combined"]:
        assert sorted(os.listdir(os.path.join(folder, k))) == ["%06d.png" % i for i in range(4)], k
    # the same batches once more, by hand
    model.eval()
    index = 0
    for batch in _loader(opt):
        with torch.no_grad():
            out = model(batch, "inference")
        want = _expected_files(out, opt.label_nc + 2)
        assert list(want) == keys
        for b in range(opt.batchSize):
            name = "%06d.png" % index
            assert os.path.basename(batch["path"][b]) == name[:-4]
            read = {k: np.asarray(Image.open(os.path.join(folder, k, name))) for k in keys + ["combined"]}
            for k in keys:
                assert read[k].shape == want[k][b].shape and np.array_equal(read[k], want[k][b]), (k, name)
            assert read["image_lr"].shape == (4, 4, 3) and read["fake_image"].shape == (32, 32, 3)
            # the strip: its parts side by side; the LR column by the stated bilinear formula (within one level, as the kernel's
            # own test allows), every other column exactly the file of its key
            columns = [read[k] for k in keys]
            columns[1] = G.np_bilinear_up(read["image_lr"], 32, 32)
            strip = np.concatenate(columns, axis=1)
            assert read["combined"].shape == strip.shape == (32, 32 * len(keys), 3)
            diff = np.abs(read["combined"].astype(np.int16) - strip.astype(np.int16))
            diff_lr = diff[:, 32:64].max()
            diff[:, 32:64] = 0
            assert diff.max() == 0 and diff_lr <= 1, (name, diff.max(), diff_lr)
            index += 1
    model.train()
    assert index == 4


def test_save_images_only_and_writer_errors(tmp_path):
    from PIL import Image
    from deepsee_amd import visuals as V
    opt = _opt("independent")
    model = _manager(opt).sr_model.eval()
    batch = next(iter(_loader(opt)))
    with torch.no_grad():
        out = model(batch, "inference")
    model.train()
    folder = str(tmp_path / "once")
    V.save_images_only(out, ["/data/val/a.jpg", "b.png"], folder)                       # returns when the files are there
    want = _expected_files(out, opt.label_nc + 2)
    for k in V.SAVE_KEYS:
        assert sorted(os.listdir(os.path.join(folder, k))) == ["a.png", "b.png"]
        assert np.array_equal(np.asarray(Image.open(os.path.join(folder, k, "b.png"))), want[k][1])
    # more batches than pinned buffers: a buffer is reused only after its files are written, and every batch arrives intact
    with V.ImageWriter(str(tmp_path / "many")) as writer:
        for i in range(5):
            writer.submit(out, ["%d_0" % i, "%d_1" % i])
        assert writer.bytes_copied == 5 * V._Layout(out).nbytes
    for i in range(5):
        got = np.asarray(Image.open(os.path.join(str(tmp_path / "many"), "fake_image", "%d_1.png" % i)))
        assert np.array_equal(got, want["fake_image"][1])
    # an exception of the writer thread surfaces in close()
    blocked = tmp_path / "blocked"
    blocked.write_text("a file where the folder should be")
    writer = V.ImageWriter(str(blocked))
    writer.submit(out, ["x", "y"])
    with pytest.raises(OSError):
        writer.close()
    writer.close()                                                                      # idempotent
    with pytest.raises(RuntimeError):
        writer.submit(out, ["x", "y"])


def _blocky_loader(opt):
    """4 samples whose images have structure below the LR grid: 4 x 4 cells of one colour each (32..223, nearest-upsampled to
    crop_size) + uniform noise of +-8 levels.  MS-SSIM is NaN, here as in the reference, when a level's mean contrast term is
    negative (a negative base under a fractional power); the bicubic image of SyntheticDataset's uniform random pixels against
    those pixels is such a pair (the "indep" case of tests/golden/ms_ssim), so the bicubic row is scored on images that an 8x
    downsampling leaves something of.  For these four the float64 restatement (tests/test_ms_ssim_host.msssim64) of the
    F.interpolate route gives cs_0..cs_3 >= 0.51 and sim_4 >= 0.97, MS-SSIM 0.80..0.84: no rounding moves a term near zero."""
    from deepsee_amd.data import DeviceLoader, SyntheticDataset

    class Blocky(SyntheticDataset):
        def _pair(self, rng):
            label, _ = super()._pair(rng)
            h = self.opt.crop_size
            cells = rng.integers(32, 224, size=(4, 4, 3))
            image = np.repeat(np.repeat(cells, h // 4, 0), h // 4, 1) + rng.integers(-8, 9, size=(h, h, 3))
            return label, image.astype(np.uint8)

    return DeviceLoader(Blocky(opt, length=4), opt, shuffle=False)


def test_baseline_mode_is_the_bicubic_image(tmp_path):
    from deepsee_amd import metrics as M
    from deepsee_amd import ops
    from deepsee_amd.managers import InferenceManager
    opt = _opt("independent")
    model = _manager(opt).sr_model
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    noise = (model.noise.step, model.noise.offset)
    batches = list(_blocky_loader(opt))
    out = model(batches[0], "baseline")
    assert isinstance(out, OrderedDict) and list(out) == ["input_label", "image_downsized", "fake_image", "image_full"]
    assert out["input_label"] is batches[0]["input_semantics"] and out["image_full"] is batches[0]["image_hr"]
    lr = ops.to_nchw(batches[0]["image_lr"], 3).cpu()
    want = F.interpolate(lr, (32, 32), mode="bicubic").clamp(-1, 1)
    assert tuple(out["fake_image"].shape) == (2, 3, 32, 32) and rel(out["fake_image"].cpu(), want) < 1e-6
    # the manager: the same metrics as the same images fed to the evaluator directly; the images are written as well
    res = InferenceManager(opt, num_samples=3).run(model, batches, mode="baseline", save_to=str(tmp_path / "bicubic"))
    ev = M.MetricsEvaluator(ms_ssim=True)
    for b in batches:
        ev.collect_samples(model(b, "baseline")["fake_image"], b["image_hr"])
    direct = ev.get_result()
    print("baseline:", dict(res))
    assert list(res) == list(direct) and res["n_samples"] == 4
    for k in ("psnr/mean", "ssim/mean", "ms_ssim/mean", "rmse/mean"):
        assert math.isfinite(float(res[k])), (k, res[k])
    assert 0.75 < float(res["ms_ssim/mean"]) < 0.9, res["ms_ssim/mean"]                 # (_blocky_loader: 0.80..0.84 per sample)
    for k in res:
        assert float(res[k]) == float(direct[k]), (k, res[k], direct[k])
    assert sorted(os.listdir(str(tmp_path / "bicubic" / "fake_image"))) == ["%06d.png" % i for i in range(4)]
    # no network, noise or coin state was touched
    assert (model.noise.step, model.noise.offset) == noise and model.training
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k


def test_writing_images_does_not_disturb_training(tmp_path):
    """Two managers from the same seed run 3 G+D steps (eager, captured, replayed or eager again, as the branch coins fall); one
    validates with save_to after step 2.  Losses and the final state are bit-identical."""
    from deepsee_amd.managers import InferenceManager
    import bench
    opt = _opt("independent")
    train = [bench.synthetic_batch(opt, opt.batchSize, 100 + i, "cpu") for i in range(3)]

    def run(validate):
        tm = _manager(opt)
        losses = []
        for i, b in enumerate(train):
            tm.run_generator_one_step({k: v.clone() for k, v in b.items()})
            tm.run_discriminator_one_step({k: v.clone() for k, v in b.items()})
            losses.append({k: float(v.detach()) for k, v in tm.get_latest_losses().items()})
            if validate and i == 1:
                res = InferenceManager(opt, num_samples=3).run(tm.sr_model, _loader(opt), save_to=str(tmp_path / "val"))
                assert res["n_samples"] == 4 and tm.sr_model.training
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in tm.sr_model.state_dict().items()}
        stats = dict(tm.graph_stats)
        tm.close()
        return losses, state, stats

    l0, s0, g0 = run(False)
    l1, s1, g1 = run(True)
    assert len(os.listdir(str(tmp_path / "val" / "combined"))) == 4
    assert g0 == g1 and l0 == l1, (g0, g1)
    assert list(s0) == list(s1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
