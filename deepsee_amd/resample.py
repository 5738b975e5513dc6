"""Host half of the on-device load-time geometry (numpy, float64): the integer tables dsee_resample_u8 is driven by, and the
reference's get_params / get_transform (data/base_dataset.py:149-201) restated as one source box, one resize and one window.

Tables.  Pillow resizes 8-bit images in two passes (horizontal, then vertical over the uint8 result of the first), each a
convolution with per-output coefficient rows quantised to int32 at 22 fractional bits (src/libImaging/Resample.c:
precompute_coeffs, normalize_coeffs_8bpc).  pil_tables restates that computation, operation for operation in float64, for
BICUBIC (a = -0.5, support 2) and BILINEAR (support 1); nearest_table restates the index walk of Image.resize(NEAREST)
(Geometry.c: ImagingScaleAffine, an accumulated xo += scale).  A table is (first [out], count [out], coef [out, kmax]).

Geometry.  load_geometry returns {'box': (x, y, w, h) in the file, 'resize': (w, h) or None, 'window': (x, y, w, h) in the resized
image, 'out': (w, h)} for every preprocess_mode of options/base_options.py:56-63; where PIL / torchvision would pad (a crop that
leaves the image) it raises ValueError.  batch_tables cuts the tables down to each sample's window, in the layout of
include/deepsee_hip.h.  ragged_tables does the same for files of different sizes (dsee_resample_u8_ragged): per-sample boxes, an
item table that says where each sample's box lies in the arena pack_arena builds, and one output size asked of all.
"""
import functools

import numpy as np

BICUBIC, BILINEAR, NEAREST = "bicubic", "bilinear", "nearest"
FILTERS = (BICUBIC, BILINEAR, NEAREST)
PRECISION_BITS = 22
MODES = ("center_crop_and_resize", "center_crop", "resize_and_crop", "crop", "scale_width", "scale_width_and_crop",
         "scale_shortside", "scale_shortside_and_crop", "fixed", "none", "scale_width_and_center_crop")


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


_SUPPORT = {BICUBIC: (_bicubic, 2.0), BILINEAR: (_bilinear, 1.0)}


def identity_table(size):
    """The table of a pass Pillow skips (size unchanged), also one row per pixel of an image that is not resized at all:
    one tap of weight 1, which the device arithmetic reproduces exactly ((v << 22) + (1 << 21)) >> 22 == v."""
    return (np.arange(size, dtype=np.int32), np.ones(size, np.int32), np.full((size, 1), 1 << PRECISION_BITS, np.int32))


@functools.lru_cache(maxsize=64)
def pil_tables(in_size, out_size, filt):
    """Pillow's coefficient rows of one axis in_size -> out_size for BICUBIC / BILINEAR (an unchanged size: the identity)."""
    in_size, out_size = int(in_size), int(out_size)
    if filt == NEAREST:
        return nearest_table(in_size, out_size)
    if in_size == out_size:
        return identity_table(in_size)
    fn, fsupport = _SUPPORT[filt]
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)             # C's (int): truncation; the operand is > -1
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < xmax[:, None]
    w = np.where(live, fn(((x + xmin[:, None]) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                           # sequential, like the C loop
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    q = w * float(1 << PRECISION_BITS)
    coef = np.where(w < 0, (-0.5 + q), (0.5 + q)).astype(np.int64)              # (int)(+-0.5 + w * 2^22): truncation
    assert int(np.abs(coef).sum(1).max()) * 255 < 2 ** 31
    return xmin.astype(np.int32), xmax.astype(np.int32), np.where(live, coef, 0).astype(np.int32)


@functools.lru_cache(maxsize=64)
def nearest_table(in_size, out_size):
    """Source index per output of Image.resize(NEAREST): xo = scale / 2, then idx = int(xo); xo += scale."""
    in_size, out_size = int(in_size), int(out_size)
    scale = float(in_size) / out_size
    idx = np.empty(out_size, np.int32)
    xo = scale * 0.5
    for i in range(out_size):
        idx[i] = int(xo)
        xo += scale
    assert idx.min() >= 0 and idx.max() < in_size
    return idx, np.ones(out_size, np.int32), np.full((out_size, 1), 1 << PRECISION_BITS, np.int32)


def emulate(src, xt, yt):
    """The device arithmetic in numpy: src uint8 [H, W, C] (or [H, W]) through the tables of the two axes -> uint8.  int32
    accumulation, arithmetic shift, uint8 between the passes."""
    def one(a, tab):                                                            # resamples axis 0
        first, count, coef = tab
        out = np.empty((len(first),) + a.shape[1:], np.uint8)
        for i in range(len(first)):
            acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
            for k in range(int(count[i])):
                acc = acc + a[first[i] + k].astype(np.int32) * np.int32(coef[i, k])
            out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
        return out
    a = np.asarray(src, np.uint8)
    h = one(np.swapaxes(a, 0, 1), xt)                                           # horizontal pass first, rounded to uint8
    return one(np.swapaxes(h, 0, 1), yt)


def crop_params(opt, size, rng):
    """get_params of base_dataset.py:149-168 as it stands (including the scale_shortside_and_crop branch, which scales the
    long side and keeps the short one): size = (w, h) of the label file; rng has random.Random's randint / random."""
    w, h = size
    new_h, new_w = h, w
    if opt.preprocess_mode == "resize_and_crop":
        new_h = new_w = opt.load_size
    elif opt.preprocess_mode == "scale_width_and_crop":
        new_w = opt.load_size
        new_h = opt.load_size * h // w
    elif opt.preprocess_mode == "scale_shortside_and_crop":
        ss, ls = min(w, h), max(w, h)
        width_is_shorter = w == ss
        ls = int(opt.load_size * ls / ss)
        new_w, new_h = (ss, ls) if width_is_shorter else (ls, ss)
    x = rng.randint(0, max(0, new_w - opt.crop_size))
    y = rng.randint(0, max(0, new_h - opt.crop_size))
    flip = rng.random() > 0.5
    return {"crop_pos": (x, y), "flip": flip}


def load_geometry(opt, src_wh, crop_pos=(0, 0), mode=None):
    """get_transform of base_dataset.py:171-201 (with its substring tests on the mode name) for a file of src_wh = (w, h).
    mode: get_transform's own preprocess_mode argument (default opt.preprocess_mode); besides MODES it may be 'resize', which
    celeba_dataset.py:53-55 gives the label maps: resize to load_size and nothing else."""
    valid = MODES if mode is None else MODES + ("resize",)
    mode = opt.preprocess_mode if mode is None else mode
    if mode not in valid:
        raise ValueError("preprocess_mode must be one of %s, got %r" % (", ".join(valid), mode))
    w, h = int(src_wh[0]), int(src_wh[1])
    box = (0, 0, w, h)
    if "center_crop" in mode:
        s = getattr(opt, "center_crop_size", None)
        if s is None:
            raise ValueError("preprocess_mode=%r needs opt.center_crop_size" % (mode,))
        if s > w or s > h:
            raise ValueError("center_crop_size %d leaves the %d x %d image (torchvision pads; not restated)" % (s, w, h))
        box = (int(round((w - s) / 2.0)), int(round((h - s) / 2.0)), s, s)      # Python's round: halves to even
        w = h = s
    resize = None
    if "resize" in mode:
        resize = (opt.load_size, opt.load_size)
    elif "scale_width" in mode:
        if w != opt.load_size:
            resize = (opt.load_size, int(opt.load_size * h / w))
    elif "scale_shortside" in mode:
        ss, ls = min(w, h), max(w, h)
        if ss != opt.load_size:
            ls2 = int(opt.load_size * ls / ss)
            resize = (ss, ls2) if w == ss else (ls2, ss)
    if resize is not None:
        w, h = resize
    window = (0, 0, w, h)
    if "crop" in mode and "center_crop" not in mode:
        x, y = int(crop_pos[0]), int(crop_pos[1])
        c = opt.crop_size
        if x < 0 or y < 0 or x + c > w or y + c > h:
            raise ValueError("crop of %d at (%d, %d) leaves the %d x %d image (PIL pads; not restated)" % (c, x, y, w, h))
        window = (x, y, c, c)
    if mode == "fixed":
        resize = (opt.crop_size, int(round(opt.crop_size / opt.aspect_ratio)))
        window = (0, 0) + resize
    if resize is not None and min(resize) < 1:
        raise ValueError("resize to %s" % (resize,))
    return {"box": box, "resize": resize, "window": window, "out": (window[2], window[3])}


def axis_tables(geo, filt):
    """(xtab, ytab) of one geometry, cut to its window; the source indices count from the box's corner."""
    bw, bh = geo["box"][2:]
    rw, rh = geo["resize"] if geo["resize"] is not None else (bw, bh)
    x, y, w, h = geo["window"]
    if geo["resize"] is None:
        xt, yt = identity_table(bw), identity_table(bh)
    else:
        xt, yt = pil_tables(bw, rw, filt), pil_tables(bh, rh, filt)
    return tuple(t[x:x + w] for t in xt), tuple(t[y:y + h] for t in yt)


def pack(ts, rebase=None):
    """Per-sample tables of one axis -> int32 [N, out, 2 + k], k the largest tap count of the batch (shorter rows zero-padded; the
    count column says how many are read); rebase[n] is subtracted from sample n's first indices."""
    k = max(t[2].shape[1] for t in ts)
    out = np.zeros((len(ts), len(ts[0][0]), 2 + k), np.int32)
    for n, (first, count, coef) in enumerate(ts):
        out[n, :, 0] = first - (rebase[n] if rebase is not None else 0)
        out[n, :, 1] = count
        out[n, :, 2:2 + coef.shape[1]] = coef
    return out


def batch_tables(geos, filt):
    """The int32 arguments of dsee_resample_u8 for a batch of geometries with one box size and one output size:
    {'xtab' [N, Wo, 2 + kx], 'ytab' [N, Ho, 2 + ky], 'rows' [N, 2], 'tmp_rows'} -- the ytab's first indices rebased to the
    first source row each sample reads."""
    tabs = [axis_tables(g, filt) for g in geos]
    bw, bh = geos[0]["box"][2:]

    rows = np.array([[int(yt[0].min()), int((yt[0] + yt[1]).max() - yt[0].min())] for _, yt in tabs], np.int32)
    xtab, ytab = pack([t[0] for t in tabs]), pack([t[1] for t in tabs], rows[:, 0])
    # what the kernel relies on: every tap inside the box resp. inside the rows of the horizontal pass
    assert xtab[..., 0].min() >= 0 and (xtab[..., 0] + xtab[..., 1]).max() <= bw and xtab[..., 1].max() <= xtab.shape[2] - 2
    assert ytab[..., 0].min() >= 0 and ((ytab[..., 0] + ytab[..., 1]).max(1) <= rows[:, 1]).all()
    assert rows[:, 0].min() >= 0 and (rows.sum(1) <= bh).all()
    return {"xtab": xtab, "ytab": ytab, "rows": rows, "tmp_rows": int(rows[:, 1].max())}


ARENA_ALIGN = 256     # every file of an arena starts on a multiple of this many bytes


def pack_arena(arrays):
    """uint8 arrays of any shapes back to back in one uint8 buffer, each start ARENA_ALIGN-byte aligned -> (buffer, [byte offset
    per array]).  The buffer is a torch tensor, pinned when CUDA is available: one upload carries the whole batch."""
    import torch
    arrays = [np.ascontiguousarray(a, dtype=np.uint8) for a in arrays]
    offsets, at = [], 0
    for a in arrays:
        at = (at + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN
        offsets.append(at)
        at += a.size
    buf = torch.empty(max(at, 1), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    view, end = buf.numpy(), 0
    for a, off in zip(arrays, offsets):
        view[end:off] = 0                                                       # (the padding is never read; kept defined)
        view[off:off + a.size] = a.reshape(-1)
        end = off + a.size
    view[end:] = 0
    return buf, offsets


def ragged_tables(geos, filt, files, offsets, paths=None):
    """batch_tables without its one-box assumption: the arguments of dsee_resample_u8_ragged for geometries whose boxes differ,
    as long as all have one output size.  files: (w, h, channels) of every file, offsets: its first byte in the arena
    (pack_arena).  {'xtab', 'ytab', 'rows', 'tmp_rows'} as in batch_tables -- kx, ky padded to the batch maximum, tmp_rows the
    maximum row count -- plus 'items' int64 [N, 4]: (byte offset of the box's first pixel in the arena, row stride in bytes,
    box_w, box_h).  Geometries that differ in their output size are refused (ValueError naming the first two that do)."""
    names = list(paths) if paths is not None else list(range(len(geos)))
    for n, g in enumerate(geos):
        if g["out"] != geos[0]["out"]:
            raise ValueError("the samples of one batch must leave the load-time geometry with one size: %s (%d x %d) becomes "
                             "%d x %d, %s (%d x %d) becomes %d x %d"
                             % ((names[0],) + tuple(files[0][:2]) + tuple(geos[0]["out"])
                                + (names[n],) + tuple(files[n][:2]) + tuple(g["out"])))
    tabs = [axis_tables(g, filt) for g in geos]

    rows = np.array([[int(yt[0].min()), int((yt[0] + yt[1]).max() - yt[0].min())] for _, yt in tabs], np.int32)
    xtab, ytab = pack([t[0] for t in tabs]), pack([t[1] for t in tabs], rows[:, 0])
    items = np.zeros((len(geos), 4), np.int64)
    for n, (g, (w, h, c), off) in enumerate(zip(geos, files, offsets)):
        x0, y0, bw, bh = g["box"]
        # what the kernel relies on, per sample: the box inside its file, every tap inside the box resp. inside the rows of the
        # horizontal pass
        assert 0 <= x0 and 0 <= y0 and x0 + bw <= w and y0 + bh <= h and c in (1, 3) and off >= 0, (g["box"], files[n], off)
        assert xtab[n, :, 0].min() >= 0 and (xtab[n, :, 0] + xtab[n, :, 1]).max() <= bw and xtab[n, :, 1].max() <= xtab.shape[2] - 2
        assert ytab[n, :, 0].min() >= 0 and (ytab[n, :, 0] + ytab[n, :, 1]).max() <= rows[n, 1]
        assert rows[n, 0] >= 0 and rows[n].sum() <= bh
        items[n] = (int(off) + (y0 * w + x0) * c, w * c, bw, bh)
    return {"xtab": xtab, "ytab": ytab, "rows": rows, "tmp_rows": int(rows[:, 1].max()), "items": items}
