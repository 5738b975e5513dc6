"""Golden fixture of the loader's load-time geometry over batches of DIFFERENTLY SIZED files (tests/golden/mixed_loader/
geometry.json), written from the real reference the way tools/gen_golden_loader.py writes its own (the same stubs for the four
torchvision transforms, the reference's data/base_dataset.py loaded by path).

Per case a batch of files of different sizes, image files and label files differing again: the reference's own get_params(opt,
label.size) under seeded `random` per file, then its get_transform(opt, params, method, normalize=False, toTensor=False) per file
-- what its DataLoader does to such a folder, every file on its own -- for the image files (BICUBIC and / or BILINEAR) and the
label files (NEAREST).  Stored: the source bytes per file (zlib + base85), the parameters drawn, and the uint8 pixels the
reference's function and Pillow produced, stacked: every case leaves the geometry with one size.

    python tools/gen_golden_mixed_loader.py
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import gen_golden_loader as G      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mixed_loader")

# name: options, Pillow filters of the images, (w, h) of the image files, (w, h) of the label files, seed of get_params
MIXED = {
    "resize_and_crop": dict(opt=dict(preprocess_mode="resize_and_crop", load_size=16, crop_size=8), filters=["bicubic", "bilinear"],
                            images=[(37, 29), (64, 48), (23, 41), (9, 40)], labels=[(19, 15), (32, 24), (12, 21), (5, 20)], seed=1),
    "center_crop_and_resize": dict(opt=dict(preprocess_mode="center_crop_and_resize", center_crop_size=12, load_size=8),
                                   filters=["bicubic"], images=[(13, 15), (17, 13), (40, 12)], labels=[(15, 13), (12, 40), (17, 17)],
                                   seed=2),
    "fixed": dict(opt=dict(preprocess_mode="fixed", crop_size=10, aspect_ratio=0.8), filters=["bicubic"],
                  images=[(24, 17), (7, 13), (33, 50)], labels=[(12, 9), (33, 50), (7, 13)], seed=3),
    "scale_width_and_crop": dict(opt=dict(preprocess_mode="scale_width_and_crop", load_size=12, crop_size=8), filters=["bilinear"],
                                 images=[(23, 17), (46, 34), (30, 64)], labels=[(23, 17), (46, 34), (30, 64)], seed=4),
    # outputs that happen to coincide: 12 x 8 from both
    "scale_width_coinciding": dict(opt=dict(preprocess_mode="scale_width", load_size=12), filters=["bicubic"],
                                   images=[(23, 17), (46, 34)], labels=[(46, 34), (23, 17)], seed=5),
}


def load():
    with open(os.path.join(OUT, "geometry.json")) as f:
        return json.load(f)


def case_opt(case, filt=None):
    """The option namespace of a case, as the loader under test gets it."""
    return G.case_opt({"opt": case["opt"], "filter": filt or case["filters"][0]})


def cases(BD):
    from PIL import Image
    out = {}
    for k, (name, spec) in enumerate(MIXED.items()):
        rng = np.random.default_rng(9000 + k)
        imgs = [G.content(rng, 2, h, w)[n % 2] for n, (w, h) in enumerate(spec["images"])]
        labs = [G.content(rng, 2, h, w, label=True)[n % 2] for n, (w, h) in enumerate(spec["labels"])]
        opt = argparse.Namespace(**vars(case_opt(spec)))
        random.seed(spec["seed"])
        params = [BD.get_params(opt, (w, h)) for w, h in spec["labels"]]        # (drawn for the label file's size)
        rec = {"opt": dict(G._BASE, **spec["opt"]), "filters": spec["filters"],
               "crop_pos": [[int(v) for v in p["crop_pos"]] for p in params], "flip": [int(bool(p["flip"])) for p in params],
               "image_src": [G.pack_u8(a) for a in imgs], "label_src": [G.pack_u8(a) for a in labs], "image_out": {}}
        plain = [dict(p, flip=False) for p in params]                            # (the flip happens on the device, after this)
        for filt in spec["filters"]:
            method = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[filt]
            done = [np.asarray(BD.get_transform(opt, p, method=method, normalize=False, toTensor=False)(Image.fromarray(a)), np.uint8)
                    for a, p in zip(imgs, plain)]
            rec["image_out"][filt] = G.pack_u8(np.stack(done))
        done = [np.asarray(BD.get_transform(opt, p, method=Image.NEAREST, normalize=False, toTensor=False)(Image.fromarray(a)), np.uint8)
                for a, p in zip(labs, plain)]
        rec["label_out"] = G.pack_u8(np.stack(done))
        assert rec["label_out"]["shape"][1:3] == rec["image_out"][spec["filters"][0]]["shape"][1:3], name
        out[name] = rec
    assert len({tuple(p) for p in out["resize_and_crop"]["crop_pos"]}) > 1
    return out


def main():
    import PIL
    BD, _ = G.load_reference()
    G.OUT, saved = OUT, G.OUT
    try:
        G.write("geometry", {"pillow": PIL.__version__, "cases": cases(BD)})
    finally:
        G.OUT = saved
    size = os.path.getsize(os.path.join(OUT, "geometry.json"))
    assert size < 64 * 1024 and max(max(wh) for s in MIXED.values() for wh in s["images"] + s["labels"]) <= 64, size


if __name__ == "__main__":
    main()
