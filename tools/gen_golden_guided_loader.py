"""Golden fixtures of the identity-paired guiding images (tests/golden/guided_loader/*.json), written from the real reference
the way tools/gen_golden_loader.py writes its own.

dataset.json        the tiny data set: 6 files, images 24 x 24 RGB, label maps 12 x 12 with classes 0..18 and a few 255,
                    identities A = {3 files}, B = {2}, C = {1}; the source pixels (zlib + base85) and the text of both identities
                    files -- CelebAMask-HQ's CSV written by pandas with quoting=csv.QUOTE_ALL exactly as the reference's
                    celebamaskhq_compute_identities_file.py:69-70 writes it, and CelebA's '<filename> <identity>' lines.
celebamaskhq.json   CelebAMaskHQDataset.__getitem__ of the reference (resize_and_crop, load_size 12, crop_size 8) and
celeba.json         CelebADataset.__getitem__ (center_crop_and_resize, center_crop_size 20, load_size 12; labels 'resize'),
                    for the phases train / val / test, each with isTrain and flips and without: per item the candidate list, the
                    chosen guide, crop_pos and flip, 'image', 'label', 'guiding_image', 'guiding_label' as uint8 -- or what the
                    item raised.

Image files are written losslessly under the name <id>.jpg: PNG bytes, because Pillow sniffs the content and not the extension,
so the fixture does not depend on a libjpeg version.  write_files() is what the tests rebuild the folder with.

The reference draws the guide with random.sample(<set>, 1), which depends on string hashing and is gone from Python 3.11.  It is
wrapped by a recorder that returns sorted(population)[random.randrange(len(population))] (an empty population goes to the real
function, which raises the reference's ValueError); `random` is seeded per item with the seed data.RawFolderDataset(seed=SEED)
gives that item in epoch 0, so the draw after get_params' three is the one the loader under test makes.

torchvision is not a dependency of this project: the transforms are the stand-ins of tools/gen_golden_loader.py plus ToTensor
(HWC uint8 -> CHW float / 255) and Normalize ((x - mean) / std), restated from their published definitions.

    python tools/gen_golden_guided_loader.py
"""
import argparse
import csv
import importlib
import io
import json
import os
import random
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import gen_golden_loader as G  # noqa: E402
from tools.gen_golden_loader import pack_u8, unpack_u8  # noqa: E402,F401

OUT = os.path.join(ROOT, "tests", "golden", "guided_loader")
SEED = 0
IDS = ["000002", "000005", "000010", "000011", "000023", "000100"]
IDENTITY = {"000002": "7", "000005": "7", "000010": "31", "000011": "7", "000023": "31", "000100": "4"}   # A = 7, B = 31, C = 4
PHASES = ("train", "val", "test")
OPTS = {
    "celebamaskhq": dict(preprocess_mode="resize_and_crop", load_size=12, crop_size=8, center_crop_size=None),
    "celeba": dict(preprocess_mode="center_crop_and_resize", load_size=12, crop_size=8, center_crop_size=20),
}
LABEL_NC = 19


def load(name):
    with open(os.path.join(OUT, name + ".json")) as f:
        return json.load(f)


def item_seed(i, seed=SEED, epoch=0):
    """The seed of data.RawFolderDataset's generator for item i."""
    return (seed * 1000003 + epoch) * 1000003 + int(i)


def sources():
    rng = np.random.default_rng(4242)
    images = G.content(rng, len(IDS), 24, 24)
    labels = rng.integers(0, LABEL_NC, size=(len(IDS), 12, 12), dtype=np.uint8)
    labels[rng.random(labels.shape) < 0.08] = 255
    return images, labels


def write_files(dataset, folder, image_hw=None):
    """The data set of dataset.json under folder/lab, folder/img + folder/identities.csv, folder/identities.txt.
    image_hw: write the files enlarged to this size (nearest), labels at half of it, for tests that need a larger model."""
    from PIL import Image
    os.makedirs(os.path.join(folder, "lab"))
    os.makedirs(os.path.join(folder, "img"))
    images, labels = unpack_u8(dataset["images"]), unpack_u8(dataset["labels"])
    for k, file_id in enumerate(dataset["ids"]):
        img, lab = Image.fromarray(images[k]), Image.fromarray(labels[k])
        if image_hw is not None:
            h, w = image_hw
            img, lab = img.resize((w, h), Image.NEAREST), lab.resize((w // 2, h // 2), Image.NEAREST)
        img.save(os.path.join(folder, "img", file_id + ".jpg"), format="PNG")
        lab.save(os.path.join(folder, "lab", file_id + ".png"))
    for name in ("identities.csv", "identities.txt"):
        with open(os.path.join(folder, name), "w", newline="") as f:
            f.write(dataset[name])
    return {"label_dir": os.path.join(folder, "lab"), "image_dir": os.path.join(folder, "img"),
            "celebamaskhq": os.path.join(folder, "identities.csv"), "celeba": os.path.join(folder, "identities.txt")}


def identities_texts():
    import pandas as pd
    rows = [{"hq_file_id": k, "celeba_file_id": "%06d.jpg" % (900 + n), "identity": IDENTITY[k],
             "count": sum(v == IDENTITY[k] for v in IDENTITY.values())} for n, k in enumerate(IDS)]
    txt = "".join("%s.jpg %s\n" % (r["hq_file_id"], r["identity"]) for r in rows)
    # the CSV has one more row, of identity C and a file that is not in the folder: the reference's restriction to the folder's
    # ids removes it (its CelebA path has no such restriction and would try to open the file)
    rows.append({"hq_file_id": "000999", "celeba_file_id": "000998.jpg", "identity": "4", "count": 1})
    df = pd.DataFrame(rows, columns=["hq_file_id", "celeba_file_id", "identity", "count"])
    buf = io.StringIO()
    df.to_csv(buf, quoting=csv.QUOTE_ALL)
    return buf.getvalue(), txt


def load_reference():
    """The reference's data package, imported for real (its torchvision.transforms: the stand-ins)."""
    from oracle.gen_golden import REF
    assert os.path.isdir(REF), "needs the reference sources (%s)" % REF
    G.install_transforms_stub()
    tr = sys.modules["torchvision.transforms"]

    class ToTensor:
        def __call__(self, img):
            a = np.asarray(img, dtype=np.uint8)
            a = a[:, :, None] if a.ndim == 2 else a
            return torch.from_numpy(a.transpose(2, 0, 1).copy()).float().div(255)

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = torch.tensor(mean).view(-1, 1, 1), torch.tensor(std).view(-1, 1, 1)

        def __call__(self, t):
            return (t - self.mean) / self.std

    tr.ToTensor, tr.Normalize = ToTensor, Normalize
    sys.path.insert(0, REF)
    try:
        mods = [importlib.import_module(n) for n in ("data.base_dataset", "data.celebamaskhq_dataset", "data.celeba_dataset",
                                                     "data.custom_exception")]
    finally:
        sys.path.remove(REF)
    return mods


def to_u8(t, image):
    if image:
        return ((t * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()
    return t[0].round().clamp(0, 255).to(torch.uint8).numpy()


def record(mods, paths, mode):
    BD, HQ, CA, CE = mods
    cls = {"celebamaskhq": HQ.CelebAMaskHQDataset, "celeba": CA.CelebADataset}[mode]
    trace = {}
    real_sample, real_params = random.sample, BD.get_params

    def sample(population, k):
        assert k == 1
        pop = sorted(population)
        if not pop:
            return real_sample(pop, 1)                 # raises the reference's ValueError
        trace["candidates"], trace["chosen"] = pop, pop[random.randrange(len(pop))]
        return [trace["chosen"]]

    def get_params(opt, size):
        p = real_params(opt, size)
        trace["crop_pos"], trace["flip"], trace["params_size"] = [int(v) for v in p["crop_pos"]], bool(p["flip"]), list(size)
        return p

    out = {}
    random.sample = sample
    BD.get_params = CA.get_params = get_params
    try:
        for phase in PHASES:
            for train in (True, False):
                opt = argparse.Namespace(
                    downsampling_method="bicubic", max_dataset_size=sys.maxsize, no_pairing_check=False, ignore_path_match=False,
                    label_dir=paths["label_dir"], image_dir=paths["image_dir"], guiding_style_image=True,
                    identities_file=paths[mode], phase=phase, isTrain=train, no_flip=False, label_nc=LABEL_NC, aspect_ratio=1.0,
                    **OPTS[mode])
                ds = cls()
                ds.initialize(opt)
                assert [os.path.basename(p)[:-4] for p in ds.image_paths] == IDS
                items = []
                for i in range(len(ds)):
                    trace.clear()
                    random.seed(item_seed(i))
                    try:
                        d = ds[i]
                    except (ValueError, CE.SkipSampleException) as e:
                        items.append({"id": IDS[i], "raised": type(e).__name__, "message": str(e),
                                      "crop_pos": trace["crop_pos"], "flip": trace["flip"]})
                        continue
                    assert os.path.basename(d["path"])[:-4] == IDS[i] and d["guiding_image_id"] == trace["chosen"]
                    items.append({"id": IDS[i], "raised": None, "candidates": trace["candidates"], "guide": trace["chosen"],
                                  "crop_pos": trace["crop_pos"], "flip": trace["flip"] and train,
                                  "params_size": trace["params_size"],
                                  "image": pack_u8(to_u8(d["image"], True)), "label": pack_u8(to_u8(d["label"], False)),
                                  "guiding_image": pack_u8(to_u8(d["guiding_image"], True)),
                                  "guiding_label": pack_u8(to_u8(d["guiding_label"], False))})
                out["%s/%s" % (phase, "train_flips" if train else "no_flips")] = items
    finally:
        random.sample = real_sample
        BD.get_params = CA.get_params = real_params
    return out


def main():
    import PIL
    images, labels = sources()
    csv_text, txt = identities_texts()
    dataset = {"ids": IDS, "identity": IDENTITY, "seed": SEED, "label_nc": LABEL_NC, "images": pack_u8(images),
               "labels": pack_u8(labels), "identities.csv": csv_text, "identities.txt": txt}
    mods = load_reference()
    with tempfile.TemporaryDirectory() as folder:
        paths = write_files(dataset, folder)
        cases = {mode: record(mods, paths, mode) for mode in OPTS}
    # ---- what makes the fixtures worth having
    good = [it for mode in cases for items in cases[mode].values() for it in items if not it["raised"]]
    assert any(it["flip"] for it in good) and any(not it["flip"] for it in good)
    assert any((unpack_u8(it["guiding_label"]) == 255).any() for it in good), "no 255 in a guide's label map"
    assert any((unpack_u8(it["label"]) == LABEL_NC).any() for it in good) and not any((unpack_u8(it["label"]) == 255).any() for it in good)
    assert any(it["guide"] != it["id"] for it in good) and any(it["guide"] == it["id"] for it in good)
    assert len({tuple(it["crop_pos"]) for it in good}) > 2
    for mode, phases in (("celebamaskhq", ("val", "test")), ("celeba", ("test",))):
        for phase in phases:
            for key in ("train_flips", "no_flips"):
                raised = [it for it in cases[mode]["%s/%s" % (phase, key)] if it["raised"]]
                assert [it["id"] for it in raised] == ["000100"], (mode, phase, raised)
    assert cases["celebamaskhq"]["test/no_flips"][5]["raised"] == "ValueError"
    assert cases["celeba"]["test/no_flips"][5]["raised"] == "SkipSampleException"
    assert not any(it["raised"] for it in cases["celeba"]["val/no_flips"])
    G.OUT, saved = OUT, G.OUT
    try:
        G.write("dataset", dict(dataset, pillow=PIL.__version__))
        for mode in OPTS:
            G.write(mode, {"opt": OPTS[mode], "cases": cases[mode]})
    finally:
        G.OUT = saved
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    assert total < 200 * 1024, total
    print("total %d bytes" % total)


if __name__ == "__main__":
    main()
