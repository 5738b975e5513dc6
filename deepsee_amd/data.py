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
"""
import os
import random
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


class FolderDataset:
    """label_dir/<id>.png (uint8 class indices, 255 = unknown) + image_dir/<id>.jpg pairs, matched by file stem like
    base_dataset.py:44-62 (paths_match).  'resize_and_crop': both are resized to load_size (NEAREST for the label,
    BICUBIC for the image, base_dataset.py:92,107), cropped to crop_size at one random position and flipped with
    p = 0.5 in training (the flip itself happens on the device)."""

    def __init__(self, opt, label_dir, image_dir, seed=0, no_flip=None):
        from PIL import Image  # noqa: F401  (fail here, not in a worker)
        mode = getattr(opt, "preprocess_mode", "resize_and_crop")
        if mode != "resize_and_crop":     # (base_dataset.py:76-104 also knows scale_width*, fixed, none: not restated here)
            raise ValueError("FolderDataset implements preprocess_mode='resize_and_crop' only, got %r" % (mode,))
        self.opt = opt
        self.no_flip = bool(getattr(opt, "no_flip", False)) if no_flip is None else bool(no_flip)
        self.rng = random.Random(seed)
        labels = {os.path.splitext(f)[0]: os.path.join(label_dir, f) for f in sorted(os.listdir(label_dir))
                  if f.lower().endswith(IMG_EXT)}
        images = {os.path.splitext(f)[0]: os.path.join(image_dir, f) for f in sorted(os.listdir(image_dir))
                  if f.lower().endswith(IMG_EXT)}
        missing = sorted(set(labels) ^ set(images))
        assert not missing, "label/image files without a partner (first: %s)" % missing[:3]
        self.items = [(labels[k], images[k]) for k in sorted(labels)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        from PIL import Image
        opt = self.opt
        lp, ip = self.items[i]
        x = self.rng.randint(0, max(0, opt.load_size - opt.crop_size))
        y = self.rng.randint(0, max(0, opt.load_size - opt.crop_size))
        flip = int(self.rng.random() > 0.5) if (opt.isTrain and not self.no_flip) else 0
        box = (x, y, x + opt.crop_size, y + opt.crop_size)
        lab = Image.open(lp)
        if lab.mode not in ("L", "P"):
            raise ValueError("%s: label maps are single-channel class-index images, got mode %r" % (lp, lab.mode))
        lab = lab.resize((opt.load_size, opt.load_size), Image.NEAREST).crop(box)
        img = Image.open(ip).convert("RGB").resize((opt.load_size, opt.load_size), Image.BICUBIC).crop(box)
        return {"label": np.asarray(lab, dtype=np.uint8), "image": np.asarray(img, dtype=np.uint8), "flip": flip,
                "path": ip}


class RawFolderDataset:
    """The file pairs of FolderDataset, decoded and nothing else: every preprocess_mode is accepted, because the geometry runs on
    the device (device_preprocess).  Image and label file may differ in size (1024^2 and 512^2 in CelebAMask-HQ); the crop
    position is drawn for the LABEL file's size and applied to both, like base_dataset.py:91-106.  Crop position and flip are a
    pure function of (seed, epoch, index) -- set_epoch(e) is called by DeviceLoader at each __iter__ -- so items do not depend
    on the order, or the thread, in which they are loaded."""
    thread_safe = True

    def __init__(self, opt, label_dir, image_dir, seed=0, no_flip=None):
        from PIL import Image  # noqa: F401  (fail here, not in a worker)
        mode = getattr(opt, "preprocess_mode", "resize_and_crop")
        if mode not in R.MODES:
            raise ValueError("preprocess_mode must be one of %s, got %r" % (", ".join(R.MODES), mode))
        self.opt, self.seed, self.epoch = opt, int(seed), 0
        self.no_flip = bool(getattr(opt, "no_flip", False)) if no_flip is None else bool(no_flip)
        self.items = _paired_files(label_dir, image_dir)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        from PIL import Image
        lp, ip = self.items[i]
        lab = Image.open(lp)
        if lab.mode not in ("L", "P"):
            raise ValueError("%s: label maps are single-channel class-index images, got mode %r" % (lp, lab.mode))
        params = R.crop_params(self.opt, lab.size, random.Random((self.seed * 1000003 + self.epoch) * 1000003 + int(i)))
        flip = int(params["flip"]) if (self.opt.isTrain and not self.no_flip) else 0
        return {"label_raw": np.asarray(lab, dtype=np.uint8), "image_raw": np.asarray(Image.open(ip).convert("RGB"), dtype=np.uint8),
                "crop_pos": params["crop_pos"], "flip": flip, "path": ip}


def _paired_files(label_dir, image_dir):
    """[(label path, image path)] matched by file stem (base_dataset.py:44-62, paths_match), sorted by stem."""
    labels = {os.path.splitext(f)[0]: os.path.join(label_dir, f) for f in sorted(os.listdir(label_dir))
              if f.lower().endswith(IMG_EXT)}
    images = {os.path.splitext(f)[0]: os.path.join(image_dir, f) for f in sorted(os.listdir(image_dir))
              if f.lower().endswith(IMG_EXT)}
    missing = sorted(set(labels) ^ set(images))
    assert not missing, "label/image files without a partner (first: %s)" % missing[:3]
    return [(labels[k], images[k]) for k in sorted(labels)]


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


def resample_raw(opt, raw, crop_pos, filt):
    """Load-time geometry of a raw uint8 batch [N,Hs,Ws(,3)] on the device: centre crop, resize and crop of opt.preprocess_mode
    (resample.load_geometry) through dsee_resample_u8 with `filt` -> uint8 [N,H,W(,3)], the wire format."""
    raw = raw if raw.is_cuda else raw.cuda(non_blocking=True)
    n, hs, ws = raw.shape[:3]
    assert len(crop_pos) == n, "one crop position per sample"
    geos = [R.load_geometry(opt, (ws, hs), tuple(int(v) for v in p)) for p in crop_pos]
    tab = R.batch_tables(geos, filt)
    flat = torch.from_numpy(np.concatenate([tab[k].reshape(-1) for k in ("xtab", "ytab", "rows")])).cuda(non_blocking=True)
    dev, at = {"tmp_rows": tab["tmp_rows"]}, 0
    for k in ("xtab", "ytab", "rows"):
        dev[k] = flat[at:at + tab[k].size].view(tab[k].shape)
        at += tab[k].size
    return ops.resample_u8(raw, dev, geos[0]["out"], geos[0]["box"])


def device_preprocess(opt, batch, stream=None):
    """uint8 host/device batch -> native batch dict on the device (all kernels on the current stream).
    batch: 'label' uint8 [N,H,W], 'image' uint8 [N,H,W,3], optional 'flip' uint8 [N], 'guiding_*', 'path' -- or the raw form
    'label_raw' uint8 [N,Hl,Wl], 'image_raw' uint8 [N,Hs,Ws,3] (tensors, or lists of arrays of one size) + 'crop_pos' [N] of
    (x, y), which dsee_resample_u8 turns into the former: the image with Pillow's BILINEAR if opt.downsampling_method is
    'bilinear' and BICUBIC otherwise (base_dataset.py:45-47), the label with NEAREST."""
    def dev(t):
        return t if t.is_cuda else t.cuda(non_blocking=True)

    if "image_raw" in batch:
        filt = R.BILINEAR if getattr(opt, "downsampling_method", "bicubic") == "bilinear" else R.BICUBIC
        wire, paths = dict(batch), batch.get("path")
        for pre in ("", "guiding_"):
            if pre + "image_raw" not in batch:
                continue
            img = resample_raw(opt, stack_raw(batch[pre + "image_raw"], paths), batch["crop_pos"], filt)
            lab = resample_raw(opt, stack_raw(batch[pre + "label_raw"], paths), batch["crop_pos"], R.NEAREST)
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
    if "path" in batch:
        res["path"] = batch["path"]
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
            for key in ("label_raw", "image_raw"):
                t = stack_raw([s[key] for s in samples], out["path"])
                out[key] = t.pin_memory() if pin else t
            out["crop_pos"] = [tuple(s["crop_pos"]) for s in samples]
            return out
        out["label"], out["image"] = stack("label"), stack("image")
        if "guiding_image" in samples[0]:
            out["guiding_image"], out["guiding_label"] = stack("guiding_image"), stack("guiding_label")
        return out

    def _stage(self, ids):
        samples = list(self.pool.map(self.ds.__getitem__, ids)) if self.pool else [self.ds[i] for i in ids]
        host = self.collate(samples)
        with torch.cuda.stream(self.side):
            dev = device_preprocess(self.opt, host)
            ev = torch.cuda.Event()
            ev.record(self.side)
        return dev, ev, host       # `host` is kept alive until the copies that read it have run

    def __iter__(self):
        if not self.workers:
            yield from self._batches()
            return
        with ThreadPoolExecutor(self.workers) as self.pool:     # lives as long as the epoch's iterator
            try:
                yield from self._batches()
            finally:
                self.pool = None

    def _batches(self):
        idx = self.indices()
        if hasattr(self.ds, "set_epoch"):
            self.ds.set_epoch(self.epoch)
        self.epoch += 1
        batches = [idx[i:i + self.bs] for i in range(0, len(idx), self.bs)]
        if self.drop_last:
            batches = [b for b in batches if len(b) == self.bs]
        nxt = self._stage(batches[0]) if batches else None
        for k in range(len(batches)):
            dev, ev, host = nxt
            nxt = self._stage(batches[k + 1]) if k + 1 < len(batches) else None
            torch.cuda.current_stream().wait_event(ev)
            for v in dev.values():                       # tensors made on the side stream, used on the compute stream
                t = v.t if isinstance(v, ops.Labels) else v
                if isinstance(t, torch.Tensor):
                    t.record_stream(torch.cuda.current_stream())
            yield dev
