"""Device input pipeline: replaces the reference's data/base_dataset.py:87-116,171-201 (PIL ->
torchvision transforms -> float CPU tensors -> .cuda()) + data/preprocessor.py on the hot path.

What travels over PCIe is what the files hold: a uint8 label map [H,W] and a uint8 RGB image [H,W,3] per sample
(256 KB at 256x256 instead of 1 MB of fp32 + a 5 MB one-hot map built on the device by the reference).  ToTensor,
Normalize((.5,.5,.5),(.5,.5,.5)), the per-sample horizontal flip, the 255 -> label_nc 'unknown' remap and the bicubic
LR image are HIP kernels (dsee_image_u8_to_nhwc, dsee_label_u8_prepare, dsee_bicubic_down) that write the NHWC RGB0
fp32 / uint8-label layout the networks consume.  Host side: PIL decoding + resize + crop only (get_params /
get_transform semantics of base_dataset.py:171-201, 'resize_and_crop' mode), batches collated into pinned memory and
uploaded asynchronously one batch ahead of the compute stream.

Datasets yield dicts  {'label': uint8 [H,W], 'image': uint8 [H,W,3], 'flip': 0/1, 'path': str}  (+ 'guiding_label',
'guiding_image' for the guided variant); DeviceLoader yields the native batch dict TrainerManager.run_*_one_step
accept: {'input_semantics': ops.Labels, 'image_hr', 'image_lr'[, 'guiding_label', 'guiding_image'], 'path'}.

Raw variant (every preprocess_mode of options/base_options.py:56-63, any opt.downsampling_method): RawFolderDataset only decodes
and yields {'image_raw': uint8 [Hs,Ws,3], 'label_raw': uint8 [Hl,Wl], 'crop_pos': (x, y), 'flip', 'path'}; the files' pixels
are uploaded as they are and dsee_resample_u8 does the centre crop, the resize (Pillow's 8-bit arithmetic, bit for bit) and the
random crop on the device, which gives the wire format above.  The tables that drive it come from deepsee_amd/resample.py.
DeviceLoader(workers=k) decodes the samples of a batch on k threads (PIL releases the GIL while it decodes).
Files of different sizes in one batch (a user's own folder): DeviceLoader.collate packs them into one pinned arena (RawArena),
which travels in one upload and goes through dsee_resample_u8_ragged, the same arithmetic with the source described per sample;
all that is asked is that the samples leave the geometry with one size.

Guided variant (opt.guiding_style_image): FolderDataset and RawFolderDataset add a second file of the same identity to every
item ('guiding_label' / 'guiding_image', resp. 'guiding_label_raw' / 'guiding_image_raw' + 'guiding_path'), chosen through an
IdentityIndex (the identities file of CelebAMask-HQ or CelebA) by the rules of DESIGN 4.3; the guide shares the sample's crop
position and flip and, where the files have one size, its dsee_resample_u8 launches.  create_dataloader(opt) builds the loader
from the reference's option names (data/__init__.py:41-54).
"""
import csv
import os
import random
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import lib as L
from . import ops
from . import resample as R

MAX_WORKERS = 16      # decoding threads of a DeviceLoader: a fixed cap, never derived from the machine's CPU count
IMG_EXT = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".tiff", ".webp")


class SyntheticDataset:
    """Blocky 19-class label maps (16x16 cells, nearest-upsampled: piecewise constant like real masks) + uniform
    random images, as uint8 -- the benchmark's input distribution in the loader's wire format."""
    thread_safe = True     # an item is a pure function of (seed, index)

    def __init__(self, opt, length=64, seed=1234, guided=None):
        self.opt, self.length, self.seed = opt, int(length), int(seed)
        self.guided = bool(opt.guiding_style_image) if guided is None else guided

    def __len__(self):
        return self.length

    def _pair(self, rng):
        h = self.opt.crop_size
        cells = rng.integers(0, self.opt.label_nc, size=(16, 16), dtype=np.uint8)
        label = np.repeat(np.repeat(cells, h // 16, 0), h // 16, 1)
        image = rng.integers(0, 256, size=(h, h, 3), dtype=np.uint8)
        return label, image

    def __getitem__(self, i):
        rng = np.random.default_rng(self.seed * 1000003 + i)
        label, image = self._pair(rng)
        out = {"label": label, "image": image, "flip": int(rng.integers(0, 2)) if self.opt.isTrain else 0,
               "path": "synthetic/%06d" % i}
        if self.guided:
            out["guiding_label"], out["guiding_image"] = self._pair(rng)
        return out


class SkipSampleException(ValueError):
    """A sample that cannot be served (data/custom_exception.py): no guide is left for it.  A ValueError, because that is what
    the reference's CelebAMask-HQ path ends in there (random.sample of an empty set) and what InferenceManager.run skips on."""


DATASET_MODES = ("celebamaskhq", "celeba")


def _stem(path):
    return os.path.splitext(os.path.basename(path))[0]


class IdentityIndex:
    """file id <-> identity, from an identities file of either dataset:
    *.csv       CelebAMask-HQ, as celebamaskhq_compute_identities_file.py:69-70 writes it (every field quoted): an index
                column, then hq_file_id, celeba_file_id, identity, count;
    otherwise   CelebA: one '<filename> <identity>' line per file, id = the filename without its extension."""

    def __init__(self, id2identity, path=""):
        self.path = path
        self.id2identity = dict(id2identity)
        self.identity2ids = {}
        for file_id, identity in self.id2identity.items():
            self.identity2ids.setdefault(identity, set()).add(file_id)

    @classmethod
    def from_file(cls, path):
        path = str(path)
        id2identity = {}
        if path.lower().endswith(".csv"):
            with open(path, newline="") as f:
                rows = csv.reader(f)
                header = next(rows)
                try:
                    fid, ident = header.index("hq_file_id"), header.index("identity")
                except ValueError:
                    raise ValueError("%s: no hq_file_id / identity column in %r" % (path, header))
                for row in rows:
                    if row:
                        id2identity[row[fid]] = row[ident]
        else:
            with open(path) as f:
                for line in f:
                    if line.strip():
                        filename, identity = line.split()
                        id2identity[os.path.splitext(filename)[0]] = identity
        return cls(id2identity, path)

    def __len__(self):
        return len(self.id2identity)

    def __eq__(self, other):
        return isinstance(other, IdentityIndex) and self.id2identity == other.id2identity

    def restrict(self, file_ids):
        """The index of these file ids alone (celebamaskhq_dataset.py:25-27: the rows of the data set's split)."""
        keep = set(file_ids)
        return IdentityIndex({k: v for k, v in self.id2identity.items() if k in keep}, self.path)

    def candidates(self, file_id, exclude_self):
        """The ids of file_id's identity, sorted as strings; without file_id itself if exclude_self."""
        if file_id not in self.id2identity:
            raise KeyError("file id %r has no entry in the identities file %s" % (file_id, self.path))
        ids = self.identity2ids[self.id2identity[file_id]]
        return sorted(k for k in ids if not (exclude_self and k == file_id))


class _FilePairs:
    """What FolderDataset and RawFolderDataset share: the file pairs, and the guide of an item (a second file of the same person,
    base_dataset.py:118-140 + sample_guiding_image of celebamaskhq_dataset.py / celeba_dataset.py)."""

    def _init_files(self, opt, label_dir, image_dir, identities, dataset_mode, order, max_dataset_size):
        if dataset_mode not in DATASET_MODES:
            raise ValueError("dataset_mode must be one of %s, got %r" % (", ".join(DATASET_MODES), dataset_mode))
        pairs = _paired_files(label_dir, image_dir, order)
        self.items = pairs if max_dataset_size is None else pairs[:max_dataset_size]
        self.dataset_mode, self.identities = dataset_mode, None
        if not getattr(opt, "guiding_style_image", False):
            return
        if identities is None:
            identities = getattr(opt, "identities_file", "")
        assert identities, "Please provide an identity file."
        if not isinstance(identities, IdentityIndex):
            assert os.path.exists(identities), \
                "Please provide a correct path to the identities file (invalid path: {})".format(identities)
            identities = IdentityIndex.from_file(identities)
        # CelebAMask-HQ: the rows of this data set (after max_dataset_size, like the reference).  CelebA: the reference does not
        # filter; the ids of the folder, which only removes candidates whose file it would fail to open.
        self.by_id = {_stem(ip): (lp, ip) for lp, ip in (self.items if dataset_mode == "celebamaskhq" else pairs)}
        self.identities = identities.restrict(self.by_id)
        phase = getattr(opt, "phase", "train")
        self.exclude_self = phase != "train" if dataset_mode == "celebamaskhq" else phase == "test"

    def guide_candidates(self, i):
        file_id = _stem(self.items[i][1])
        cands = self.identities.candidates(file_id, self.exclude_self)
        if not cands:
            raise SkipSampleException("There is no other candidate for file id: {}".format(file_id))
        return cands

    def _guide(self, cands, rng):
        """(label path, image path) of the guide: one draw, made after the three of the crop position and the flip."""
        return self.by_id[cands[rng.randrange(len(cands))]]

    def __len__(self):
        return len(self.items)


def _open_label(path):
    from PIL import Image
    lab = Image.open(path)
    if lab.mode not in ("L", "P"):
        raise ValueError("%s: label maps are single-channel class-index images, got mode %r" % (path, lab.mode))
    return lab


class FolderDataset(_FilePairs):
    """label_dir/<id>.png (uint8 class indices, 255 = unknown) + image_dir/<id>.jpg pairs, matched by file stem like
    base_dataset.py:44-62 (paths_match).  'resize_and_crop': both are resized to load_size (NEAREST for the label,
    BICUBIC for the image, base_dataset.py:92,107), cropped to crop_size at one random position and flipped with
    p = 0.5 in training (the flip itself happens on the device).  With opt.guiding_style_image the item also holds
    'guiding_label' / 'guiding_image': a file of the same identity (`identities`: an IdentityIndex or the path of an identities
    file, default opt.identities_file), drawn after the flip, resized and cropped with the sample's box."""

    def __init__(self, opt, label_dir, image_dir, seed=0, no_flip=None, identities=None, dataset_mode="celebamaskhq",
                 order="stem", max_dataset_size=None):
        from PIL import Image  # noqa: F401  (fail here, not in a worker)
        mode = getattr(opt, "preprocess_mode", "resize_and_crop")
        if mode != "resize_and_crop":     # (base_dataset.py:76-104 also knows scale_width*, fixed, none: not restated here)
            raise ValueError("FolderDataset implements preprocess_mode='resize_and_crop' only, got %r" % (mode,))
        self.opt = opt
        self.no_flip = bool(getattr(opt, "no_flip", False)) if no_flip is None else bool(no_flip)
        self.rng = random.Random(seed)
        self._init_files(opt, label_dir, image_dir, identities, dataset_mode, order, max_dataset_size)

    def __getitem__(self, i):
        from PIL import Image
        opt = self.opt
        lp, ip = self.items[i]
        cands = self.guide_candidates(i) if self.identities is not None else None    # (skips before anything is drawn)
        x = self.rng.randint(0, max(0, opt.load_size - opt.crop_size))
        y = self.rng.randint(0, max(0, opt.load_size - opt.crop_size))
        flip = int(self.rng.random() > 0.5) if (opt.isTrain and not self.no_flip) else 0
        if cands is not None and not (opt.isTrain and not self.no_flip):
            self.rng.random()      # get_params draws the flip whether it is used or not: the guide's draw is always the fourth
        box = (x, y, x + opt.crop_size, y + opt.crop_size)

        def load(lp, ip):
            lab = _open_label(lp).resize((opt.load_size, opt.load_size), Image.NEAREST).crop(box)
            img = Image.open(ip).convert("RGB").resize((opt.load_size, opt.load_size), Image.BICUBIC).crop(box)
            return np.asarray(lab, dtype=np.uint8), np.asarray(img, dtype=np.uint8)

        lab, img = load(lp, ip)
        out = {"label": lab, "image": img, "flip": flip, "path": ip}
        if cands is not None:
            out["guiding_label"], out["guiding_image"] = load(*self._guide(cands, self.rng))
        return out


class RawFolderDataset(_FilePairs):
    """The file pairs of FolderDataset, decoded and nothing else: every preprocess_mode is accepted, because the geometry runs on
    the device (device_preprocess).  Image and label file may differ in size (1024^2 and 512^2 in CelebAMask-HQ); the crop
    position is drawn for the LABEL file's size and applied to both, like base_dataset.py:91-106.  Crop position, flip and guide
    are a pure function of (seed, epoch, index) -- set_epoch(e) is called by DeviceLoader at each __iter__ -- so items do not
    depend on the order, or the thread, in which they are loaded.  With opt.guiding_style_image the item also holds
    'guiding_label_raw', 'guiding_image_raw' and 'guiding_path' (see FolderDataset); the guide shares the sample's crop_pos."""
    thread_safe = True

    def __init__(self, opt, label_dir, image_dir, seed=0, no_flip=None, identities=None, dataset_mode="celebamaskhq",
                 order="stem", max_dataset_size=None):
        from PIL import Image  # noqa: F401  (fail here, not in a worker)
        mode = getattr(opt, "preprocess_mode", "resize_and_crop")
        if mode not in R.MODES:
            raise ValueError("preprocess_mode must be one of %s, got %r" % (", ".join(R.MODES), mode))
        self.opt, self.seed, self.epoch = opt, int(seed), 0
        self.no_flip = bool(getattr(opt, "no_flip", False)) if no_flip is None else bool(no_flip)
        self._init_files(opt, label_dir, image_dir, identities, dataset_mode, order, max_dataset_size)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __getitem__(self, i):
        from PIL import Image
        lp, ip = self.items[i]
        cands = self.guide_candidates(i) if self.identities is not None else None    # (skips before anything is decoded)
        lab = _open_label(lp)
        rng = random.Random((self.seed * 1000003 + self.epoch) * 1000003 + int(i))
        params = R.crop_params(self.opt, lab.size, rng)
        flip = int(params["flip"]) if (self.opt.isTrain and not self.no_flip) else 0
        out = {"label_raw": np.asarray(lab, dtype=np.uint8), "image_raw": np.asarray(Image.open(ip).convert("RGB"), dtype=np.uint8),
               "crop_pos": params["crop_pos"], "flip": flip, "path": ip}
        if cands is not None:
            glp, gip = self._guide(cands, rng)
            out["guiding_label_raw"] = np.asarray(_open_label(glp), dtype=np.uint8)
            out["guiding_image_raw"] = np.asarray(Image.open(gip).convert("RGB"), dtype=np.uint8)
            out["guiding_path"] = gip
        return out


def _natural_key(text):
    """util/util.py:174-184 (natural_keys): digit runs compare as numbers, so 2.png sorts before 10.png."""
    return [int(c) if c.isdigit() else c for c in re.split(r"(\d+)", text)]


def _paired_files(label_dir, image_dir, order="stem"):
    """[(label path, image path)] matched by file stem (base_dataset.py:44-62, paths_match).  order: 'stem' (sorted by stem) or
    'natural' (the label files' names in the reference's natural sort, base_dataset.py:51-52)."""
    if order not in ("stem", "natural"):
        raise ValueError("order must be 'stem' or 'natural', got %r" % (order,))
    labels = {os.path.splitext(f)[0]: os.path.join(label_dir, f) for f in sorted(os.listdir(label_dir))
              if f.lower().endswith(IMG_EXT)}
    images = {os.path.splitext(f)[0]: os.path.join(image_dir, f) for f in sorted(os.listdir(image_dir))
              if f.lower().endswith(IMG_EXT)}
    missing = sorted(set(labels) ^ set(images))
    assert not missing, "label/image files without a partner (first: %s)" % missing[:3]
    stems = sorted(labels) if order == "stem" else sorted(labels, key=lambda k: _natural_key(os.path.basename(labels[k])))
    return [(labels[k], images[k]) for k in stems]


def stack_raw(arrays, paths=None):
    """Raw items of one batch as one uint8 tensor; items of different sizes are refused (out of scope: one set of tables and
    one upload per batch)."""
    if isinstance(arrays, torch.Tensor):
        return arrays
    for i, a in enumerate(arrays):
        if a.shape != arrays[0].shape:
            names = (paths[0], paths[i]) if paths else (0, i)
            raise ValueError("raw items of one batch must have one size: %s is %s, %s is %s"
                             % (names[0], tuple(arrays[0].shape), names[1], tuple(a.shape)))
    return torch.from_numpy(np.stack([np.asarray(a, dtype=np.uint8) for a in arrays]))


class RawArena:
    """Raw items of DIFFERENT sizes, as DeviceLoader.collate hands them on: `buf`, one uint8 buffer that holds the files back to
    back, each from a 256-byte boundary (resample.pack_arena), and per item of this key its byte `offsets`, array `shapes`
    ((h, w, 3) or (h, w)) and `paths`.  The samples and the guides of a kind share one buffer (the guides' items after the
    samples'): one upload and one dsee_resample_u8_ragged call serve both."""

    def __init__(self, buf, offsets, shapes, paths):
        self.buf, self.offsets, self.shapes, self.paths = buf, list(offsets), [tuple(s) for s in shapes], list(paths)

    def __len__(self):
        return len(self.offsets)


def _upload_tables(tab, keys):
    """The integer tables `keys` of a table dict in one flat host-to-device transfer (int64 'items' travel as int32 pairs, first,
    so that they stay 8-byte aligned) -> the dict of device views + 'tmp_rows'."""
    flat = torch.from_numpy(np.concatenate([tab[k].reshape(-1).view(np.int32) for k in keys])).cuda(non_blocking=True)
    dev, at = {"tmp_rows": tab["tmp_rows"]}, 0
    for k in keys:
        words = tab[k].size * tab[k].itemsize // 4
        dev[k] = flat[at:at + words].view(torch.int64 if tab[k].itemsize == 8 else torch.int32).view(tab[k].shape)
        at += words
    return dev


def resample_raw(opt, raw, crop_pos, filt, mode=None):
    """Load-time geometry of a raw uint8 batch [N,Hs,Ws(,3)] on the device: centre crop, resize and crop of opt.preprocess_mode
    (resample.load_geometry; `mode` instead, where given) through dsee_resample_u8 with `filt` -> uint8 [N,H,W(,3)], the wire
    format."""
    raw = raw if raw.is_cuda else raw.cuda(non_blocking=True)
    n, hs, ws = raw.shape[:3]
    assert len(crop_pos) == n, "one crop position per sample"
    geos = [R.load_geometry(opt, (ws, hs), tuple(int(v) for v in p), mode) for p in crop_pos]
    dev = _upload_tables(R.batch_tables(geos, filt), ("xtab", "ytab", "rows"))
    return ops.resample_u8(raw, dev, geos[0]["out"], geos[0]["box"])


def resample_ragged(opt, parts, crop_pos, filt, mode=None, uploaded=None):
    """resample_raw for raw items of different sizes: `parts`, RawArenas over ONE buffer (the samples [, the guides]), with one
    crop position per item, through one dsee_resample_u8_ragged call -> uint8 [items,H,W(,3)].  The tables are built, and a
    batch whose items leave the geometry with different sizes is refused (resample.ragged_tables), before anything is uploaded.
    uploaded: {id(host buffer): device buffer} of the arenas already on the device."""
    buf = parts[0].buf
    assert all(p.buf is buf for p in parts), "the RawArenas of one call share one buffer"
    shapes = [s for p in parts for s in p.shapes]
    offsets, paths = [o for p in parts for o in p.offsets], [q for p in parts for q in p.paths]
    assert len(crop_pos) == len(shapes), "one crop position per item"
    c = {2: 1, 3: 3}[len(shapes[0])]
    assert all(len(s) == len(shapes[0]) and (c == 1 or s[2] == 3) for s in shapes), "label maps [H,W] or RGB images [H,W,3]"
    geos = [R.load_geometry(opt, (s[1], s[0]), tuple(int(v) for v in p), mode) for s, p in zip(shapes, crop_pos)]
    tab = R.ragged_tables(geos, filt, [(s[1], s[0], c) for s in shapes], offsets, paths)
    dev = _upload_tables(tab, ("items", "xtab", "ytab", "rows"))
    uploaded = {} if uploaded is None else uploaded
    if id(buf) not in uploaded:
        uploaded[id(buf)] = buf if buf.is_cuda else buf.cuda(non_blocking=True)
    return ops.resample_u8_ragged(uploaded[id(buf)], tab["items"], dev, geos[0]["out"], c)


def collate_raw(arrays, paths, guides=None, guide_paths=None):
    """The raw items of one kind (images or label maps) of a batch, host side -> (samples, guides or None).  Items of one size:
    each a stacked uint8 tensor (stack_raw), as ever.  Samples or guides of different sizes: RawArenas over one buffer that holds
    the samples' files, then the guides'."""
    def uniform(items):
        return items is None or all(a.shape == items[0].shape for a in items)

    if uniform(arrays) and uniform(guides):
        return stack_raw(arrays, paths), None if guides is None else stack_raw(guides, guide_paths)
    n = len(arrays)
    every = list(arrays) + list(guides or [])
    buf, offsets = R.pack_arena(every)
    shapes = [a.shape for a in every]
    return (RawArena(buf, offsets[:n], shapes[:n], paths),
            None if guides is None else RawArena(buf, offsets[n:], shapes[n:], guide_paths))


def device_preprocess(opt, batch, stream=None):
    """uint8 host/device batch -> native batch dict on the device (all kernels on the current stream).
    batch: 'label' uint8 [N,H,W], 'image' uint8 [N,H,W,3], optional 'flip' uint8 [N], 'guiding_*', 'path' -- or the raw form
    'label_raw' uint8 [N,Hl,Wl], 'image_raw' uint8 [N,Hs,Ws,3] (tensors, or lists of arrays of one size) + 'crop_pos' [N] of
    (x, y), which dsee_resample_u8 turns into the former: the image with Pillow's BILINEAR if opt.downsampling_method is
    'bilinear' and BICUBIC otherwise (base_dataset.py:45-47), the label with NEAREST and the geometry of
    opt.label_preprocess_mode (None: opt.preprocess_mode, like the image).  'guiding_label_raw' / 'guiding_image_raw' share the
    samples' crop positions; where they also share their sizes, samples and guides go through dsee_resample_u8 as one batch of
    2N (one call for the images, one for the label maps), otherwise through calls of their own.  A raw key may also be a RawArena
    (DeviceLoader.collate, collate_raw: items of different sizes); it goes through dsee_resample_u8_ragged, samples and guides of
    a kind in one call of 2N items, and the batch is refused only if its items leave the geometry with different sizes."""
    def dev(t):
        return t if t.is_cuda else t.cuda(non_blocking=True)

    if "image_raw" in batch:
        filt = R.BILINEAR if getattr(opt, "downsampling_method", "bicubic") == "bilinear" else R.BICUBIC
        lmode = getattr(opt, "label_preprocess_mode", None)        # celeba_dataset.py:53-55: 'resize' for the label maps
        wire, pos = dict(batch), list(batch["crop_pos"])
        def raw(key, paths):
            return batch[key] if isinstance(batch[key], RawArena) else stack_raw(batch[key], paths)

        raws = {pre: (raw(pre + "image_raw", batch.get(pre + "path", batch.get("path"))),
                      raw(pre + "label_raw", batch.get(pre + "path", batch.get("path"))))
                for pre in ("", "guiding_") if pre + "image_raw" in batch}
        n = len(pos)

        def both(a, b):                      # samples and guides of one size: one device batch of 2N, uploaded in place
            out = torch.empty((2 * n,) + tuple(a.shape[1:]), dtype=torch.uint8, device="cuda")
            out[:n].copy_(a, non_blocking=True)
            out[n:].copy_(b, non_blocking=True)
            return out

        uploaded = {}

        def kind(k, f, mode):                # images (k = 0) or label maps (1) of a batch in which some kind has mixed sizes
            parts = [raws[pre][k] for pre in raws]
            if any(isinstance(p, RawArena) for p in parts):     # (collate_raw: samples and guides are arenas together)
                out = resample_ragged(opt, parts, pos * len(parts), f, mode, uploaded)
            elif len(parts) == 2 and parts[0].shape == parts[1].shape and parts[0].shape[0] == n:
                out = resample_raw(opt, both(*parts), pos * 2, f, mode)
            else:
                return [resample_raw(opt, p, pos, f, mode) for p in parts]
            return [out[i * n:(i + 1) * n] for i in range(len(parts))]

        if any(isinstance(v, RawArena) for pair in raws.values() for v in pair):
            imgs, labs = kind(0, filt, None), kind(1, R.NEAREST, lmode)
            done = {pre: (imgs[i], labs[i]) for i, pre in enumerate(raws)}
        elif len(raws) == 2 and all(raws[""][k].shape == raws["guiding_"][k].shape and raws[""][k].shape[0] == n for k in (0, 1)):
            img = resample_raw(opt, both(raws[""][0], raws["guiding_"][0]), pos * 2, filt)
            lab = resample_raw(opt, both(raws[""][1], raws["guiding_"][1]), pos * 2, R.NEAREST, lmode)
            done = {"": (img[:n], lab[:n]), "guiding_": (img[n:], lab[n:])}
        else:
            done = {pre: (resample_raw(opt, img, pos, filt), resample_raw(opt, lab, pos, R.NEAREST, lmode))
                    for pre, (img, lab) in raws.items()}
        for pre, (img, lab) in done.items():
            if img.shape[1:3] != lab.shape[1:3]:
                raise ValueError("preprocess_mode=%r leaves the image at %s and the label map at %s"
                                 % (opt.preprocess_mode, tuple(img.shape[1:3]), tuple(lab.shape[1:3])))
            wire[pre + "image"], wire[pre + "label"] = img, lab
        batch = wire

    flip = dev(batch["flip"]) if batch.get("flip") is not None else None

    def image(u8):
        u8 = dev(u8).contiguous()
        n, h, w, _ = u8.shape
        out = ops.new(n, h, w, 4)
        L.call("image_u8_to_nhwc", u8, flip, out, n, h, w, 4)
        out.dsee_layout = "nhwc"
        return out

    def labels(u8):
        u8 = dev(u8).contiguous()
        n, h, w = u8.shape
        out = torch.empty_like(u8)
        L.call("label_u8_prepare", u8, flip, out, n, h, w, opt.label_nc)
        return ops.Labels(out, opt.semantic_nc)

    hr = image(batch["image"])
    res = {"input_semantics": labels(batch["label"]), "image_hr": hr, "image_lr": ops.lr_image(opt, hr)}
    if "guiding_image" in batch:
        res["guiding_image"] = image(batch["guiding_image"])
        res["guiding_label"] = labels(batch["guiding_label"])
    for key in ("path", "guiding_path"):
        if key in batch:
            res[key] = batch[key]
    return res


class DeviceLoader:
    """Batches a dataset into pinned uint8 tensors and runs upload + device_preprocess for batch k+1 on a side stream
    while the compute stream works on batch k.  `shard` = (rank, world) gives every data-parallel rank a disjoint,
    equally long slice of every epoch (the reference's DataLoader feeds one process and DataParallel scatters).
    workers = k > 0: the ds[i] of a batch run on k threads (results in index order); the dataset must declare thread_safe."""

    def __init__(self, dataset, opt, batch_size=None, shuffle=True, seed=0, shard=(0, 1), drop_last=True, workers=0):
        self.workers = int(workers)
        if not 0 <= self.workers <= MAX_WORKERS:
            raise ValueError("workers must be 0 ... %d, got %r" % (MAX_WORKERS, workers))
        if self.workers and not getattr(dataset, "thread_safe", False):
            raise ValueError("workers > 0 needs a dataset that declares thread_safe = True (%s draws from one sequential "
                             "generator)" % type(dataset).__name__)
        self.pool = None
        self.ds, self.opt = dataset, opt
        self.bs = int(batch_size or opt.batchSize)
        self.shuffle, self.seed, self.epoch = shuffle, seed, 0
        self.rank, self.world = shard
        self.drop_last = drop_last
        self.side = torch.cuda.Stream() if torch.cuda.is_available() else None

    def __len__(self):
        per_rank = len(self.ds) // self.world
        return per_rank // self.bs if self.drop_last else (per_rank + self.bs - 1) // self.bs

    def indices(self):
        idx = list(range(len(self.ds)))
        if self.shuffle:
            random.Random(self.seed + self.epoch).shuffle(idx)     # same permutation on every rank
        per_rank = len(idx) // self.world
        return idx[self.rank * per_rank:(self.rank + 1) * per_rank]

    def collate(self, samples):
        pin = torch.cuda.is_available()

        def stack(key):
            t = torch.from_numpy(np.stack([s[key] for s in samples]))
            return t.pin_memory() if pin else t

        out = {"flip": torch.tensor([s.get("flip", 0) for s in samples], dtype=torch.uint8),
               "path": [s.get("path", "") for s in samples]}
        if pin:
            out["flip"] = out["flip"].pin_memory()
        if "image_raw" in samples[0]:
            guided = "guiding_image_raw" in samples[0]
            if guided:
                out["guiding_path"] = [s.get("guiding_path", "") for s in samples]
            for key in ("label_raw", "image_raw"):     # one size: stacked and pinned; mixed sizes: the arena form (pinned by pack_arena)
                t, g = collate_raw([s[key] for s in samples], out["path"],
                                   [s["guiding_" + key] for s in samples] if guided else None, out.get("guiding_path"))
                out[key] = t.pin_memory() if pin and isinstance(t, torch.Tensor) else t
                if guided:
                    out["guiding_" + key] = g.pin_memory() if pin and isinstance(g, torch.Tensor) else g
            out["crop_pos"] = [tuple(s["crop_pos"]) for s in samples]
            return out
        out["label"], out["image"] = stack("label"), stack("image")
        if "guiding_image" in samples[0]:
            out["guiding_image"], out["guiding_label"] = stack("guiding_image"), stack("guiding_label")
        return out

    def _stage(self, ids):
        samples = list(self.pool.map(self.ds.__getitem__, ids)) if self.pool else [self.ds[i] for i in ids]
        host = self.collate(samples)
        dev, ev = self._upload(host)
        return dev, ev, host       # `host` is kept alive until the copies that read it have run

    def _upload(self, host):
        with torch.cuda.stream(self.side):
            dev = device_preprocess(self.opt, host)
            ev = torch.cuda.Event()
            ev.record(self.side)
        return dev, ev

    def _hand_over(self, dev, ev):
        torch.cuda.current_stream().wait_event(ev)
        for v in dev.values():                       # tensors made on the side stream, used on the compute stream
            t = v.t if isinstance(v, ops.Labels) else v
            if isinstance(t, torch.Tensor):
                t.record_stream(torch.cuda.current_stream())
        return dev

    def __iter__(self):
        return _Epoch(self)


class _Epoch:
    """The iterator of one epoch of a DeviceLoader (an object, not a generator: an exception ends a generator for good).  Batch
    k + 1 is staged before batch k is handed out.  A batch whose staging raised SkipSampleException is raised from the next()
    that would have yielded it, and the next() after that yields the following batch, so a consumer that skips (InferenceManager.
    run) goes on with the epoch.  Any other exception propagates at once and ends the iteration.  Nothing runs before the first
    next(); the decoding threads live from there until the iteration ends, is closed or is collected."""

    def __init__(self, loader):
        self.ld, self.batches, self.k, self.nxt, self.pool, self.held = loader, None, 0, None, None, None

    def __iter__(self):
        return self

    def _start(self):
        ld = self.ld
        if ld.workers:
            ld.pool = self.pool = ThreadPoolExecutor(ld.workers)
        idx = ld.indices()
        if hasattr(ld.ds, "set_epoch"):
            ld.ds.set_epoch(ld.epoch)
        ld.epoch += 1
        batches = [idx[i:i + ld.bs] for i in range(0, len(idx), ld.bs)]
        if ld.drop_last:
            batches = [b for b in batches if len(b) == ld.bs]
        self.batches = batches
        self.nxt = self._stage(0)

    def _stage(self, k):
        if k >= len(self.batches):
            return None
        try:
            return self.ld._stage(self.batches[k])
        except SkipSampleException as e:
            return e

    def close(self):
        self.batches, self.nxt, self.k, self.held = [], None, 0, None
        if self.pool is not None:
            pool, self.pool = self.pool, None
            if self.ld.pool is pool:
                self.ld.pool = None
            pool.shutdown(wait=True)

    __del__ = close

    def __next__(self):
        try:
            if self.batches is None:
                self._start()
            cur = self.nxt
            if cur is not None:
                self.k += 1
                self.nxt = self._stage(self.k)
        except BaseException:
            self.close()
            raise
        if cur is None:
            self.close()
            raise StopIteration
        if isinstance(cur, SkipSampleException):
            raise cur
        self.held = cur                 # (the pinned host batch lives until the next batch is handed out, as it always did)
        dev, ev, host = cur
        return self.ld._hand_over(dev, ev)


def create_dataloader(opt, seed=0, shard=(0, 1), raw=True):
    """data/__init__.py:41-54 over the device loader: the data set of opt.dataset_mode ('celebamaskhq' | 'celeba') on
    opt.label_dir / opt.image_dir, in the reference's natural order and cut to opt.max_dataset_size, guided if and only if
    opt.guiding_style_image (opt.identities_file), batched like the reference's DataLoader: batch_size = batchSize, shuffle =
    not serial_batches, drop_last = isTrain, nThreads decoding threads (at most MAX_WORKERS).  raw=False: FolderDataset (PIL
    geometry on the host, no threads) instead of RawFolderDataset.  'celeba' resamples its label maps with 'resize'
    (celeba_dataset.py:53-55): opt.label_preprocess_mode is set to it unless the caller chose one."""
    mode = getattr(opt, "dataset_mode", "celebamaskhq")
    if mode not in DATASET_MODES:
        raise ValueError("dataset_mode must be one of %s, got %r" % (", ".join(DATASET_MODES), mode))
    label_dir, image_dir = getattr(opt, "label_dir", None), getattr(opt, "image_dir", None)
    if not label_dir or not image_dir:
        raise ValueError("create_dataloader needs opt.label_dir and opt.image_dir, got %r and %r" % (label_dir, image_dir))
    if mode == "celeba" and getattr(opt, "label_preprocess_mode", None) is None:
        opt.label_preprocess_mode = "resize"
    size = getattr(opt, "max_dataset_size", None)
    cls = RawFolderDataset if raw else FolderDataset
    ds = cls(opt, label_dir, image_dir, seed=seed, dataset_mode=mode, order="natural",
             max_dataset_size=None if size is None else int(size))
    print("dataset [%s, %s] of size %d was created" % (cls.__name__, mode, len(ds)))
    workers = min(int(getattr(opt, "nThreads", 0)), MAX_WORKERS) if raw else 0
    return DeviceLoader(ds, opt, batch_size=opt.batchSize, shuffle=not getattr(opt, "serial_batches", False), seed=seed,
                        shard=shard, drop_last=bool(opt.isTrain), workers=workers)
