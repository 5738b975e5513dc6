"""Golden fixture of the output path (deepsee_amd.visuals, deepsee_amd/csrc/visuals.hip), pinned against the real reference:

  * the reference's util/util.py is loaded BY FILE PATH (modules it imports but never uses on this path are stubbed when they are
    not installed) and its labelcolormap, tensor2im, tensor2label and tile_images are evaluated on the recipes below;
  * F.interpolate(x, (H, W), mode='bicubic').clamp(-1, 1) -- the 'baseline' mode of the reference's sr_model.py:109-115 -- on the
    two baseline shapes, every STRIDE-th value.

tests/golden/visuals/visuals.json (a directory of its own: tests/test_oracle_golden.py takes every tests/golden/*.json for a model
case) holds only results; the inputs are rebuilt by the recipe functions below, which the tests import (that needs no reference).

    python tools/gen_golden_visuals.py        # needs the reference sources (oracle.gen_golden.REF)
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "visuals", "visuals.json")

CHUNK = (2, 3, 5, 7)                       # N, C, H, W of one tensor2im input: odd sizes, so that vector tails are exercised
N_LABEL = 21                               # label_nc + 2 for the 19 CelebAMask-HQ classes
BICUBIC = {"4to32": dict(S=4, H=32, W=32, seed=11), "5to12": dict(S=5, H=12, W=12, seed=12)}
STRIDE = 7                                 # of the flattened NCHW result kept in the fixture


def crafted_values():
    """fp32 values at which tensor2im's quantisation can go wrong: every level centre k / 127.5 - 1 (k = 0..255), its fp32
    neighbours on both sides, and +-1, +-1.5, +-0.  No NaN (numpy's cast of NaN to uint8 is undefined)."""
    c = (np.arange(256, dtype=np.float32) / np.float32(127.5) - np.float32(1.0)).astype(np.float32)
    below, above = np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))
    extra = np.array([1.0, -1.0, 1.5, -1.5, 0.0, -0.0], dtype=np.float32)
    return np.concatenate([c, below, above, extra]).astype(np.float32)


def crafted_chunks():
    """The 774 crafted values as NCHW tensors of shape CHUNK (210 values each: 4 tensors, the last one filled up by starting
    over), in an order that spreads neighbouring values over channels and pixels."""
    v = crafted_values()
    per = int(np.prod(CHUNK))
    count = -(-v.size // per)
    v = np.resize(v, count * per)
    return [torch.from_numpy(v[i * per:(i + 1) * per].reshape(CHUNK).copy()) for i in range(count)]


def label_map():
    """uint8 [16, 16]: every index 0..20 (12 or 13 times each)."""
    return (np.arange(256) % N_LABEL).astype(np.uint8).reshape(16, 16)


def tile_input():
    """uint8 [5, 2, 3, 3]: five distinguishable 2 x 3 RGB images."""
    return (np.arange(5 * 2 * 3 * 3) * 3 % 251).astype(np.uint8).reshape(5, 2, 3, 3)


def bicubic_input(case):
    """fp32 NCHW [2, 3, S, S], uniform in [-1, 1]: bicubic overshoot beyond +-1 occurs, so the clamp matters."""
    g = torch.Generator().manual_seed(case["seed"])
    return torch.rand(2, 3, case["S"], case["S"], generator=g) * 2 - 1


def bicubic_reference(case):
    x = bicubic_input(case)
    return F.interpolate(x, (case["H"], case["W"]), mode="bicubic").clamp(-1, 1)


# ---- numpy restatements the tests hold the kernels to (tests/test_visuals_host.py holds THEM to the fixture)
def np_tensor2im(chw, normalize=True):
    """util/util.py:95-103 for one fp32 [3, H, W] array: fp32 arithmetic in this order, clip, truncate."""
    x = np.transpose(np.asarray(chw, dtype=np.float32), (1, 2, 0))
    x = (x + 1) / 2.0 * 255.0 if normalize else x * 255.0
    assert x.dtype == np.float32
    return np.clip(x, 0, 255).astype(np.uint8)


def np_colorize(index_map, table):
    """Colorize: the table row of every index, (0, 0, 0) where no row matches."""
    table = np.concatenate([np.asarray(table, dtype=np.uint8), np.zeros((256 - len(table), 3), dtype=np.uint8)])
    return table[np.asarray(index_map, dtype=np.uint8)]


def np_bilinear_up(src, h, w):
    """The definition dsee_bilinear_up_u8 states, for one uint8 [S, S, 3] image: half-pixel centres, clamped neighbours, every
    operation rounded to fp32, floor(v + 0.5)."""
    f32 = np.float32
    s = src.shape[0]

    def coords(n_out):
        f = f32(s) / f32(n_out) * (np.arange(n_out, dtype=f32) + f32(0.5)) - f32(0.5)
        fl = np.floor(f)
        i = fl.astype(np.int64)
        return np.clip(i, 0, s - 1), np.clip(i + 1, 0, s - 1), (f - fl).astype(f32)

    def lerp(a, b, t):
        return (f32(1) - t) * a + t * b

    y0, y1, ty = coords(h)
    x0, x1, tx = coords(w)
    p = src.astype(f32)
    tx, ty = tx[None, :, None], ty[:, None, None]
    top = lerp(p[y0][:, x0], p[y0][:, x1], tx)
    bot = lerp(p[y1][:, x0], p[y1][:, x1], tx)
    v = np.floor(lerp(top, bot, ty) + f32(0.5))
    assert v.dtype == f32
    return v.astype(np.uint8)


def load_reference_util(ref_root):
    for name in ("dill",):                       # imported at the top of util/util.py, used only by save_obj / load_obj
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    spec = importlib.util.spec_from_file_location("_reference_util", os.path.join(ref_root, "util", "util.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from oracle import gen_golden as G
    assert os.path.isfile(os.path.join(G.REF, "util", "util.py")), "needs the reference sources (%s)" % G.REF
    U = load_reference_util(G.REF)
    torch.set_num_threads(1)
    out = {"labelcolormap": {str(n): U.labelcolormap(n).tolist() for n in (21, 35)}}
    chunks = crafted_chunks()
    out["tensor2im"] = {
        # the batch call (normalize=True; the reference's batch branch has no other) and, image by image, normalize=False
        "normalize": [U.tensor2im(c).tolist() for c in chunks],
        "plain": [[U.tensor2im(c[b], normalize=False).tolist() for b in range(c.shape[0])] for c in chunks],
    }
    idx = torch.from_numpy(label_map().astype(np.int64))
    onehot = F.one_hot(idx, N_LABEL).permute(2, 0, 1).float()
    out["tensor2label"] = {"n_label": N_LABEL, "single": U.tensor2label(onehot, N_LABEL).tolist(),
                           "batch": U.tensor2label(torch.stack([onehot, onehot.flip(1)]), N_LABEL).tolist()}
    out["tile_images"] = U.tile_images(tile_input(), picturesPerRow=4).tolist()
    out["bicubic"] = {}
    for name, case in BICUBIC.items():
        y = bicubic_reference(case)
        out["bicubic"][name] = dict(case, stride=STRIDE, clamped=int(((y == 1) | (y == -1)).sum()),
                                    values=[float(v) for v in y.reshape(-1)[::STRIDE]])
        assert out["bicubic"][name]["clamped"] > 0, "%s: the clamp is never active; pick another seed" % name
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
