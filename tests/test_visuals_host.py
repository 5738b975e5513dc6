"""The output path on the host (deepsee_amd.visuals): colour maps, tiling and the file rules against
tests/golden/visuals/visuals.json (written from the REAL reference by tools/gen_golden_visuals.py), the numpy restatements the GPU
tests hold the kernels to against the same fixture, the new C-ABI entry points and their argument checks, and the new arguments of
SRModel / InferenceManager.  CPU only."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tools import gen_golden_visuals as G

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visuals", "visuals.json")
ENTRY_POINTS = ("dsee_image_to_u8", "dsee_label_colorize", "dsee_bicubic_up", "dsee_bilinear_up_u8")


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


# ---- colour maps, tiling
@pytest.mark.parametrize("n", [21, 35])
def test_labelcolormap_equals_the_reference(gold, n):
    from deepsee_amd.visuals import labelcolormap
    cmap = labelcolormap(n)
    assert cmap.dtype == np.uint8 and cmap.shape == (n, 3)
    assert cmap.tolist() == gold["labelcolormap"][str(n)]


def test_tile_images_equals_the_reference(gold):
    from deepsee_amd.visuals import tile_images
    imgs = G.tile_input()
    tiled = tile_images(imgs, picturesPerRow=4)
    want = np.array(gold["tile_images"], dtype=np.uint8)
    assert tiled.dtype == np.uint8 and tiled.shape == want.shape == (4, 12, 3)      # 5 images -> 2 rows of 4, 3 zero images
    assert np.array_equal(tiled, want)
    assert not tiled[2:, 3:].any()
    assert np.array_equal(tile_images(imgs[:4], picturesPerRow=2), np.concatenate(
        [np.concatenate([imgs[0], imgs[1]], 1), np.concatenate([imgs[2], imgs[3]], 1)], 0))       # a multiple: no padding


# ---- the restatements used by tests/test_gpu_visuals.py
def test_numpy_restatements_reproduce_the_fixture(gold):
    chunks = G.crafted_chunks()
    values = G.crafted_values()
    assert len(chunks) == 4 and values.size == 3 * 256 + 6 and not np.isnan(values).any()
    assert set(values.tolist()) <= set(np.concatenate([c.numpy().ravel() for c in chunks]).tolist())   # every value is fed
    for i, c in enumerate(chunks):
        assert tuple(c.shape) == G.CHUNK
        for b in range(c.shape[0]):
            assert G.np_tensor2im(c[b].numpy()).tolist() == gold["tensor2im"]["normalize"][i][b], (i, b)
            assert G.np_tensor2im(c[b].numpy(), normalize=False).tolist() == gold["tensor2im"]["plain"][i][b], (i, b)
    from deepsee_amd.visuals import labelcolormap
    lab = G.label_map()
    assert set(lab.ravel().tolist()) == set(range(21)) and gold["tensor2label"]["n_label"] == G.N_LABEL
    table = labelcolormap(G.N_LABEL)
    assert G.np_colorize(lab, table).tolist() == gold["tensor2label"]["single"]
    assert G.np_colorize(np.stack([lab, lab[::-1]]), table).tolist() == gold["tensor2label"]["batch"]
    assert G.np_colorize(np.array([[21, 255, 20]], dtype=np.uint8), table).tolist() == [[[0, 0, 0], [0, 0, 0], table[20].tolist()]]


def test_bicubic_fixture_is_what_this_torch_computes(gold):
    for name, case in G.BICUBIC.items():
        rec = gold["bicubic"][name]
        assert {k: rec[k] for k in case} == case and rec["stride"] == G.STRIDE and rec["clamped"] > 0
        y = G.bicubic_reference(case).reshape(-1)[::G.STRIDE]
        want = torch.tensor(rec["values"], dtype=torch.float64)
        assert y.numel() == want.numel()
        assert float((y.double() - want).norm() / want.norm()) < 1e-6, name


def test_bilinear_restatement_basics():
    src = np.arange(4 * 4 * 3, dtype=np.uint8).reshape(4, 4, 3) * 5
    assert np.array_equal(G.np_bilinear_up(src, 4, 4), src)                      # same size: every t is 0
    up = G.np_bilinear_up(src, 32, 32)
    assert up.shape == (32, 32, 3) and up.dtype == np.uint8
    assert np.array_equal(up[0, 0], src[0, 0]) and np.array_equal(up[-1, -1], src[-1, -1])      # clamped borders
    assert up.min() >= src.min() and up.max() <= src.max()
    flat = np.full((4, 4, 3), 77, dtype=np.uint8)
    assert (G.np_bilinear_up(flat, 12, 20) == 77).all()


# ---- files
def test_save_image_naming_and_channel_rules(tmp_path):
    from PIL import Image
    from deepsee_amd.visuals import save_image
    rgb = (np.arange(4 * 5 * 3) % 256).astype(np.uint8).reshape(4, 5, 3)
    save_image(rgb, str(tmp_path / "a" / "b" / "x.jpg"), create_dir=True)
    assert os.listdir(str(tmp_path / "a" / "b")) == ["x.png"]                    # .jpg -> .png
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "a" / "b" / "x.png"))), rgb)
    gray = rgb[:, :, 0]
    save_image(gray, str(tmp_path / "g2.png"))                                    # 2-D -> 3 equal channels
    save_image(gray[:, :, None], str(tmp_path / "g1.png"))                        # 1 channel -> 3 equal channels
    for name in ("g2.png", "g1.png"):
        back = np.asarray(Image.open(str(tmp_path / name)))
        assert back.shape == (4, 5, 3) and all(np.array_equal(back[:, :, c], gray) for c in range(3))
    with pytest.raises(OSError):
        save_image(rgb, str(tmp_path / "missing" / "x.png"))                      # create_dir defaults to False


def test_save_style_matrix(tmp_path):
    from deepsee_amd.visuals import save_style_matrix
    style = torch.arange(6, dtype=torch.float32).reshape(2, 3) / 7
    path = str(tmp_path / "styles" / "s.csv")
    save_style_matrix(style, path, create_dir=True)
    back = np.loadtxt(path, delimiter=",")
    assert back.shape == (2, 3) and np.array_equal(back.astype(np.float32), style.numpy())
    np.savetxt(str(tmp_path / "numpy.csv"), style.numpy(), delimiter=",")          # the reference's call: the same bytes
    assert open(path, "rb").read() == open(str(tmp_path / "numpy.csv"), "rb").read()
    with pytest.raises(AssertionError):
        save_style_matrix(style[0], path)
    with pytest.raises(AssertionError):
        save_style_matrix(style, str(tmp_path / "s.txt"))


def test_file_names_of_the_writer():
    from deepsee_amd import visuals as V
    assert V._file_name("/data/val/123.jpg") == "123.png" and V._file_name("synthetic/000004") == "000004.png"
    assert V.SAVE_KEYS == ("input_semantics", "image_lr", "fake_image", "image_hr")
    assert V.GUIDED_KEYS == ("guiding_image", "guiding_input_label")


# ---- C ABI
def test_new_entry_points_are_declared_exported_and_bound():
    from deepsee_amd import lib as L
    protos = L.header_prototypes()
    so = L.lib()
    for name in ENTRY_POINTS:
        assert name in protos, name
        fn = getattr(so, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == protos[name][1] and fn.argtypes[-1] is ctypes.c_void_p
    assert len(protos["dsee_image_to_u8"][1]) == 12 and len(protos["dsee_label_colorize"][1]) == 11
    assert len(protos["dsee_bicubic_up"][1]) == 10 and len(protos["dsee_bilinear_up_u8"][1]) == 12


def test_new_entry_points_validate_before_they_launch():
    from deepsee_amd import lib as L
    so = L.lib()
    one = ctypes.c_void_p(64)        # a non-null address that is never dereferenced: the checks come before any launch
    bad = [
        ("dsee_image_to_u8", (None, one, 1, 4, 4, 4, 0, 1, 48, 12, 0)),
        ("dsee_image_to_u8", (one, None, 1, 4, 4, 4, 0, 1, 48, 12, 0)),
        ("dsee_image_to_u8", (one, one, 1, 4, 4, 2, 0, 1, 48, 12, 0)),              # NHWC with fewer than 3 channels
        ("dsee_image_to_u8", (one, one, 1, 4, 4, 4, 0, 1, 48, 11, 0)),              # rows overlap
        ("dsee_image_to_u8", (one, one, 1, 4, 4, 4, 0, 1, 48, 12, 1)),              # the window leaves the row
        ("dsee_image_to_u8", (one, one, 2, 4, 4, 4, 0, 1, 47, 12, 0)),              # images overlap
        ("dsee_image_to_u8", (one, one, 1, 4, 4, 4, 0, 1, 48, 12, -1)),
        ("dsee_label_colorize", (one, one, 0, one, 1, 4, 4, 48, 12, 0)),
        ("dsee_label_colorize", (one, one, 257, one, 1, 4, 4, 48, 12, 0)),
        ("dsee_label_colorize", (one, None, 21, one, 1, 4, 4, 48, 12, 0)),
        ("dsee_bicubic_up", (one, one, 1, 8, 4, 8, 4, 4, 1)),                       # H < S: this is the upsampler
        ("dsee_bicubic_up", (one, one, 1, 4, 8, 8, 2, 4, 1)),
        ("dsee_bicubic_up", (one, one, 0, 4, 8, 8, 4, 4, 1)),
        ("dsee_bilinear_up_u8", (one, 48, 11, 4, one, 1, 8, 8, 192, 24, 0)),        # source rows overlap
        ("dsee_bilinear_up_u8", (one, 48, 12, 4, one, 1, 8, 8, 192, 23, 0)),
        ("dsee_bilinear_up_u8", (one, 48, 12, 4, one, 1, 2, 8, 192, 24, 0)),
    ]
    for name, args in bad:
        assert getattr(so, name)(*args, None) == -1, (name, args)
        assert b"argument check failed" in so.dsee_last_error()


# ---- public surface
def test_manager_and_model_accept_the_new_arguments():
    from deepsee_amd import ops
    from deepsee_amd.managers import InferenceManager
    from deepsee_amd.options import make_opt
    from deepsee_amd.sr_model import SRModel
    run = inspect.signature(InferenceManager.run).parameters
    assert list(run) == ["self", "model", "dataloader", "mode", "save_to"]
    assert run["mode"].default == "inference" and run["save_to"].default is None
    assert inspect.signature(InferenceManager.run_batch).parameters["mode"].default == "inference"
    assert callable(ops.bicubic_up) and '"baseline"' in inspect.getsource(SRModel._forward)
    im = InferenceManager(make_opt("independent_8x_32", batchSize=2, ngf=8), num_samples=2)
    with pytest.raises(ValueError, match="baseline"):
        im.run(None, [], mode="demo")                  # refused before the model or the loader is touched
    with pytest.raises(NotImplementedError, match="save_to"):
        InferenceManager(make_opt("independent_8x_32", batchSize=2, ngf=8), num_samples=2, save_images=True)
