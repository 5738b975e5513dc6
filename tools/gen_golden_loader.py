"""Golden fixtures of the loader's load-time geometry and LR downsampling (tests/golden/loader/*.json), written from the real
reference the way tools/gen_golden_explore.py writes its own.

geometry.json   per case the reference's own get_transform(opt, params, method, normalize=False, toTensor=False) of
                data/base_dataset.py applied to PIL images: uint8 pixels written by the reference's function and Pillow, for an
                image batch (BICUBIC or BILINEAR) and a label batch (NEAREST) of N = 2, plus the source bytes (zlib + base85).
                Every preprocess_mode of options/base_options.py:56-63 occurs.
params.json     get_params under seeded `random`, for its three branches and the fall-through.
lr.json         Preprocessor.downsample_image of data/preprocessor.py for bicubic, bilinear, nearest and area: fp32 input and output.

torchvision is not a dependency of this project: the four transforms get_transform uses are restated from their published
definitions (Compose, Lambda, Resize([h, w], interpolation) = img.resize((w, h), interpolation), CenterCrop(size) = crop at
int(round((h - s) / 2.0)), int(round((w - s) / 2.0))), so CenterCrop is pinned to this stub, not to torchvision.  The two
reference files are loaded by path (their package's other imports are not needed for the functions used).

The script asserts what makes the fixtures worth having: in one bicubic case the accumulator of the second pass leaves [0, 255]
before clipping for >= 1 % of the outputs on both sides; a float two-pass WITHOUT the uint8 rounding between the passes
differs from the fixture; and it records for how many size pairs below 64 Pillow's nearest index differs from
floor((x + 0.5) * scale) in fp32 (asserting that a case's own pair is among them if there are any).

    python tools/gen_golden_loader.py
"""
import argparse
import base64
import importlib.util
import json
import os
import random
import re
import sys
import types
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "loader")

_BASE = dict(load_size=12, crop_size=12, center_crop_size=None, aspect_ratio=1.0)
# name: (h, w) of the image files, options, Pillow filter of the image, crop position per sample[, (h, w) of the label files]
GEOMETRY = {
    "resize_23x17_bicubic": dict(src=(23, 17), opt=dict(preprocess_mode="resize_and_crop"), filter="bicubic"),
    "resize_23x17_bilinear": dict(src=(23, 17), opt=dict(preprocess_mode="resize_and_crop"), filter="bilinear"),
    "resize_48x48_ratio4": dict(src=(48, 48), opt=dict(preprocess_mode="resize_and_crop"), filter="bicubic"),
    "resize_48x48_ratio4_bilinear": dict(src=(48, 48), opt=dict(preprocess_mode="resize_and_crop"), filter="bilinear"),
    "resize_9x40_up_and_down": dict(src=(9, 40), opt=dict(preprocess_mode="resize_and_crop", load_size=16, crop_size=16),
                                    filter="bicubic"),
    "fixed_24x17_one_pass_skipped": dict(src=(24, 17), opt=dict(preprocess_mode="fixed", aspect_ratio=0.5), filter="bicubic"),
    "label_24x24_to_10": dict(src=(24, 24), opt=dict(preprocess_mode="resize_and_crop", load_size=10, crop_size=10),
                              filter="bicubic"),
    "label_7x13_to_5x9": dict(src=(7, 13), opt=dict(preprocess_mode="fixed", crop_size=9, aspect_ratio=1.8), filter="bicubic"),
    # both axes are size pairs at which Pillow's accumulated nearest index differs from floor((x + 0.5) * scale) in fp32
    "label_16x14_to_12x5_accumulated_nearest": dict(src=(16, 14), opt=dict(preprocess_mode="fixed", crop_size=5, aspect_ratio=5 / 12),
                                                    filter="bicubic"),
    "pair_48_24_crop_corners": dict(src=(48, 48), label_src=(24, 24), opt=dict(preprocess_mode="resize_and_crop", crop_size=8),
                                    filter="bicubic", crop_pos=[(0, 0), (4, 4)]),
    "center_crop_13x15": dict(src=(13, 15), opt=dict(preprocess_mode="center_crop", center_crop_size=12), filter="bicubic"),
    "center_crop_17x13": dict(src=(17, 13), opt=dict(preprocess_mode="center_crop", center_crop_size=12), filter="bicubic"),
    "center_crop_and_resize_15x17": dict(src=(15, 17), opt=dict(preprocess_mode="center_crop_and_resize", center_crop_size=12,
                                                                load_size=8), filter="bicubic"),
    "scale_width_and_center_crop_13x15": dict(src=(13, 15), opt=dict(preprocess_mode="scale_width_and_center_crop",
                                                                     center_crop_size=12, load_size=8), filter="bilinear"),
    "scale_width_23x17": dict(src=(23, 17), opt=dict(preprocess_mode="scale_width"), filter="bicubic"),
    "scale_width_9x12_no_resize": dict(src=(9, 12), opt=dict(preprocess_mode="scale_width"), filter="bicubic"),
    "scale_width_and_crop_23x17": dict(src=(23, 17), opt=dict(preprocess_mode="scale_width_and_crop", crop_size=8),
                                       filter="bicubic", crop_pos=[(4, 8), (1, 3)]),
    "scale_shortside_23x17": dict(src=(23, 17), opt=dict(preprocess_mode="scale_shortside"), filter="bicubic"),
    "scale_shortside_17x23": dict(src=(17, 23), opt=dict(preprocess_mode="scale_shortside"), filter="bilinear"),
    "scale_shortside_and_crop_17x23": dict(src=(17, 23), opt=dict(preprocess_mode="scale_shortside_and_crop", crop_size=8),
                                           filter="bicubic", crop_pos=[(8, 9), (0, 5)]),
    "fixed_aspect2_23x17": dict(src=(23, 17), opt=dict(preprocess_mode="fixed", aspect_ratio=2.0), filter="bicubic"),
    "crop_23x17": dict(src=(23, 17), opt=dict(preprocess_mode="crop", crop_size=8), filter="bicubic", crop_pos=[(9, 15), (0, 7)]),
    "none_9x12": dict(src=(9, 12), opt=dict(preprocess_mode="none"), filter="bicubic"),
}
PARAMS = [dict(preprocess_mode=m, load_size=ls, crop_size=cs, size=wh, seed=seed)
          for seed, (m, ls, cs, wh) in enumerate([
              ("resize_and_crop", 40, 32, (100, 60)), ("resize_and_crop", 32, 32, (64, 64)),
              ("scale_width_and_crop", 40, 16, (100, 60)), ("scale_width_and_crop", 40, 32, (60, 100)),
              ("scale_shortside_and_crop", 40, 16, (100, 60)), ("scale_shortside_and_crop", 40, 16, (60, 100)),
              ("crop", 40, 16, (100, 60)), ("none", 40, 80, (60, 50))])]
LR_SHAPES = [((20, 20), 6), ((32, 32), 4), ((48, 48), 9), ((12, 20), 4)]
LR_MODES = ("bicubic", "bilinear", "nearest", "area")


def pack_u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return {"shape": list(a.shape), "u8": base64.b85encode(zlib.compress(a.tobytes(), 9)).decode("ascii")}


def unpack_u8(rec):
    return np.frombuffer(zlib.decompress(base64.b85decode(rec["u8"])), dtype=np.uint8).reshape(rec["shape"]).copy()


def pack_f32(t):
    """fp32 tensor -> the little-endian bytes, byte-transposed, zlib-compressed, base85 (as tools/gen_golden_explore.py)."""
    a = np.ascontiguousarray(t.detach().cpu().numpy().astype("<f4"))
    planes = np.ascontiguousarray(a.reshape(-1).view(np.uint8).reshape(-1, 4).T)
    return {"shape": list(a.shape), "f32": base64.b85encode(zlib.compress(planes.tobytes(), 9)).decode("ascii")}


def unpack_f32(rec):
    planes = np.frombuffer(zlib.decompress(base64.b85decode(rec["f32"])), dtype=np.uint8).reshape(4, -1)
    return torch.from_numpy(np.ascontiguousarray(planes.T).view("<f4").reshape(rec["shape"]).copy())


def load(name):
    with open(os.path.join(OUT, name + ".json")) as f:
        return json.load(f)


LR_BOUND = 1e-6      # rel of tests/test_gpu_ops.py for bicubic_down: |got - want| / |want| against float64


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-20))


def lr_float64(x, size, mode):
    """F.interpolate(x.double(), (size, size), mode).clamp(-1, 1): what the LR kernels are held to."""
    import torch.nn.functional as F
    return F.interpolate(x.double(), (size, size), mode=mode).clamp(-1, 1)


def lr_bound(rec, mode):
    """The LR bound of one case: LR_BOUND, or twice the error of the reference's own fp32 result where that misses LR_BOUND
    (the factor 2 allows for a different summation order)."""
    err = rel(unpack_f32(rec["output"][mode]), lr_float64(unpack_f32(rec["input"]), rec["start_size"], mode))
    return LR_BOUND if err < LR_BOUND else 2 * err


def case_opt(spec):
    """The option namespace of a geometry case, as the loader under test gets it."""
    from deepsee_amd.options import make_opt
    return make_opt(**dict(_BASE, no_flip=True, downsampling_method=spec["filter"], **spec["opt"]))


def install_transforms_stub():
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, img):
            for t in self.transforms:
                img = t(img)
            return img

    class Lambda:
        def __init__(self, lambd):
            self.lambd = lambd

        def __call__(self, img):
            return self.lambd(img)

    class Resize:
        def __init__(self, size, interpolation):
            self.size, self.interpolation = size, interpolation

        def __call__(self, img):
            h, w = self.size
            return img.resize((w, h), self.interpolation)

    class CenterCrop:
        def __init__(self, size):
            self.size = (int(size), int(size))

        def __call__(self, img):
            w, h = img.size
            th, tw = self.size
            assert th <= h and tw <= w, "the padding branch of CenterCrop is not restated"
            top, left = int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))
            return img.crop((left, top, left + tw, top + th))

    tr.Compose, tr.Lambda, tr.Resize, tr.CenterCrop = Compose, Lambda, Resize, CenterCrop
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr


def load_reference():
    """(data/base_dataset.py, data/preprocessor.py) of the reference as modules, loaded by path; the modules base_dataset imports
    for its file listing (util.util, data.image_folder: not used here) are empty stand-ins while it loads."""
    from oracle.gen_golden import REF
    assert os.path.isdir(REF), "needs the reference sources (%s)" % REF
    install_transforms_stub()
    stand_ins = {"util": types.ModuleType("util"), "util.util": types.ModuleType("util.util"),
                 "data": types.ModuleType("data"), "data.image_folder": types.ModuleType("data.image_folder")}
    stand_ins["util"].util = stand_ins["util.util"]
    stand_ins["data.image_folder"].make_dataset = None
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    try:
        mods = []
        for name in ("base_dataset", "preprocessor"):
            spec = importlib.util.spec_from_file_location("_ref_" + name, os.path.join(REF, "data", name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mods.append(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mods


def content(rng, n, h, w, label=False):
    """Sample 0: uniform noise; sample 1: 0 / 255 checkerboards and edges (labels: class indices with 255 = unknown in both)."""
    if label:
        a = rng.integers(0, 19, size=(n, h, w), dtype=np.uint8)
        a[rng.random((n, h, w)) < 0.1] = 255
        a[:, 0, 0] = 255
        return a
    a = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for c, period in enumerate((1, 2, 3)):
        a[1::2, :, :, c] = (((yy // period + xx // period) % 2) * 255).astype(np.uint8)
    a[1::2, h // 2:, : max(w // 3, 1)] = 255          # a block edge across the checkerboards
    a[1::2, : h // 3, w // 2:] = 0
    return a


def geometry_cases(BD):
    from PIL import Image
    from deepsee_amd import resample as R
    out, both_sides, unrounded_differs, nearest_cases = {}, [], [], []
    for k, (name, spec) in enumerate(GEOMETRY.items()):
        rng = np.random.default_rng(5000 + k)
        h, w = spec["src"]
        lh, lw = spec.get("label_src", spec["src"])
        img, lab = content(rng, 2, h, w), content(rng, 2, lh, lw, label=True)
        crop_pos = [tuple(p) for p in spec.get("crop_pos", [(0, 0), (0, 0)])]
        ropt = argparse.Namespace(**vars(case_opt(spec)))
        method = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[spec["filter"]]
        img_out, lab_out = [], []
        for n in range(2):
            params = {"crop_pos": crop_pos[n], "flip": False}
            t_img = BD.get_transform(ropt, params, method=method, normalize=False, toTensor=False)
            t_lab = BD.get_transform(ropt, params, method=Image.NEAREST, normalize=False, toTensor=False)
            img_out.append(np.asarray(t_img(Image.fromarray(img[n])), dtype=np.uint8))
            lab_out.append(np.asarray(t_lab(Image.fromarray(lab[n])), dtype=np.uint8))
        img_out, lab_out = np.stack(img_out), np.stack(lab_out)
        assert img_out.shape[1:3] == lab_out.shape[1:3], name
        out[name] = {"opt": dict(_BASE, **spec["opt"]), "filter": spec["filter"], "crop_pos": [list(p) for p in crop_pos],
                     "image_src": pack_u8(img), "image_out": pack_u8(img_out), "label_src": pack_u8(lab),
                     "label_out": pack_u8(lab_out)}
        # ---- what makes the case worth having (computed with the tables under test; the fixture itself is the reference's)
        for n in range(2):
            geo = R.load_geometry(case_opt(spec), (w, h), crop_pos[n])
            if geo["resize"] is None:
                continue
            (xf, xc, xk), (yf, yc, yk) = R.axis_tables(geo, spec["filter"])
            x0, y0, bw, bh = geo["box"]
            src = img[n, y0:y0 + bh, x0:x0 + bw].astype(np.float64)
            X = np.zeros((len(xf), bw))
            Y = np.zeros((len(yf), bh))
            for i in range(len(xf)):
                X[i, xf[i]:xf[i] + xc[i]] = xk[i, :xc[i]]
            for i in range(len(yf)):
                Y[i, yf[i]:yf[i] + yc[i]] = yk[i, :yc[i]]
            hpass = np.clip(np.floor((np.einsum("ow,hwc->hoc", X, src) + 2 ** 21) / 2 ** 22), 0, 255)
            acc = np.floor((np.einsum("oh,hwc->owc", Y, hpass) + 2 ** 21) / 2 ** 22)
            assert np.array_equal(np.clip(acc, 0, 255), img_out[n]), (name, "the tables under test miss the reference")
            if spec["filter"] == "bicubic":
                both_sides.append((name, n, float((acc < 0).mean()), float((acc > 255).mean())))
            smooth = np.einsum("oh,hwc->owc", Y, np.einsum("ow,hwc->hoc", X, src)) / 2.0 ** 44
            unrounded_differs.append((name, n, int((np.clip(np.floor(smooth + 0.5), 0, 255) != img_out[n]).sum())))
            for a, b in ((lw, geo["resize"][0]), (lh, geo["resize"][1])):
                nearest_cases.append((a, b))
    best = max(both_sides, key=lambda r: min(r[2], r[3]))
    assert min(best[2], best[3]) >= 0.01, ("no bicubic case leaves [0, 255] on both sides for 1 % of its outputs", best)
    assert any(r[2] > 0 for r in unrounded_differs), "a float two-pass without the uint8 rounding reproduces every case"
    differing = [(i, o) for i in range(1, 64) for o in range(1, 64) if not np.array_equal(
        R.nearest_table(i, o)[0], np.floor((np.arange(o, dtype=np.float32) + np.float32(0.5)) * (np.float32(i) / np.float32(o))))]
    if differing:
        assert any(p in differing for p in nearest_cases), ("no label case uses a size pair of", differing[:8])
    meta = {"overshoot_case": {"name": best[0], "sample": best[1], "below_0": best[2], "above_255": best[3]},
            "pixels_changed_by_the_uint8_rounding_between_passes": {"%s/%d" % (r[0], r[1]): r[2] for r in unrounded_differs if r[2]},
            "nearest_pairs_below_64_that_differ_from_fp32_floor": len(differing),
            "nearest_pairs_of_cases_that_differ": sorted({list(p).__str__() for p in nearest_cases if p in differing})}
    return out, meta


def params_cases(BD):
    out = []
    for spec in PARAMS:
        opt = argparse.Namespace(preprocess_mode=spec["preprocess_mode"], load_size=spec["load_size"], crop_size=spec["crop_size"])
        random.seed(spec["seed"])
        draws = []
        for _ in range(4):
            p = BD.get_params(opt, tuple(spec["size"]))
            draws.append({"crop_pos": [int(p["crop_pos"][0]), int(p["crop_pos"][1])], "flip": bool(p["flip"])})
        out.append(dict(spec, size=list(spec["size"]), draws=draws))
    return out


def lr_cases(PP):
    out = {}
    for k, ((h, w), s) in enumerate(LR_SHAPES):
        rng = np.random.default_rng(7000 + k)
        x = (torch.from_numpy(content(rng, 2, h, w)).permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5   # ToTensor + Normalize
        rec = {"start_size": s, "input": pack_f32(x), "output": {}}
        for mode in LR_MODES:
            pp = PP.Preprocessor(argparse.Namespace(gpu_ids=[], start_size=s, downsampling_method=mode))
            y = pp.downsample_image(x)
            assert tuple(y.shape) == (2, 3, s, s)
            rec["output"][mode] = pack_f32(y)
        out["%dx%d_to_%d" % (h, w, s)] = rec
    return out


def write(name, obj):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".json")
    text = json.dumps(obj, indent=1)
    text = re.sub(r"\[\s+(-?[\d.][^\[\]{}\"]*?)\s+\]", lambda m: "[" + " ".join(m.group(1).split()) + "]", text)
    with open(path, "w") as f:
        f.write(text + "\n")
    print("%-16s %7d bytes" % (name, os.path.getsize(path)))


def main():
    import PIL
    BD, PP = load_reference()
    cases, meta = geometry_cases(BD)
    write("geometry", {"pillow": PIL.__version__, "checks": meta, "cases": cases})
    write("params", {"cases": params_cases(BD)})
    write("lr", {"torch": torch.__version__, "cases": lr_cases(PP)})
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    assert total < 200 * 1024, total
    print("total %d bytes" % total)


if __name__ == "__main__":
    main()
