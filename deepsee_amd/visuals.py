"""Output side of the device pipeline: tensors -> uint8 images -> PNG files.

Mirror of deepsee_amd.data on the way out.  The reference copies fp32 NCHW tensors (12 bytes per pixel per visual, plus a one-hot
label map) to the host and converts them in numpy (util/util.py:44-158,245-311 tile_images / tensor2im / tensor2label / save_image /
save_style_matrix / labelcolormap / Colorize, util/visualizer.py:181-215 save_images_only).  Here the conversions are HIP kernels
(dsee_image_to_u8, dsee_label_colorize, dsee_bilinear_up_u8; deepsee_amd/csrc/visuals.hip) that write packed RGB bytes where the
files will take them from, and 3 bytes per pixel leave the card.

  * tensor2im / tensor2label / tile_images / labelcolormap / save_image / save_style_matrix: the reference's functions, the first
    two device-backed.  tensor2im's arithmetic is the reference's to the bit ((x + 1) / 2 * 255 in fp32, clip, truncate).
  * save_images_only(visuals, paths, folder_out): <folder>/<key>/<name>.png per visual and <folder>/combined/<name>.png =
    [label colours | LR upsampled | fake | HR (| guiding image | guiding label colours)] side by side.
  * ImageWriter: the same files, asynchronously.  Per batch the kernels fill ONE device arena laid out as the files are (the
    per-key images, then the combined strips, each column written in place), one asynchronous copy brings it into one of two pinned
    buffers, and one host thread encodes the PNGs with PIL and writes them while the device works on the next batch.

The LR column of the combined strip is the one piece that is not pinned to the reference: it resizes with cv2 there; here it is
the bilinear upsampling dsee_bilinear_up_u8 defines (half-pixel centres, clamped borders, fp32, rounded half up).  That entry
point takes one source side; a non-square LR image (a non-square batch, ops.lr_shape) is upsampled by dsee_resize_hw (the same
half-pixel bilinear on the fp32 image) and converted by dsee_image_to_u8 like every other column.  The label columns need no
resize: the label map is kept at the HR size.
"""
import os
import queue
import threading
from collections import OrderedDict

import numpy as np
import torch

from . import lib as L
from . import ops
from .util import save_style_matrix  # noqa: F401  (util/util.py:150-158; writes the bytes of np.savetxt(delimiter=','))

SAVE_KEYS = ("input_semantics", "image_lr", "fake_image", "image_hr")
GUIDED_KEYS = ("guiding_image", "guiding_input_label")

_CITYSCAPES = [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (111, 74, 0), (81, 0, 81), (128, 64, 128), (244, 35, 232),
               (250, 170, 160), (230, 150, 140), (70, 70, 70), (102, 102, 156), (190, 153, 153), (180, 165, 180), (150, 100, 100),
               (150, 120, 90), (153, 153, 153), (153, 153, 153), (250, 170, 30), (220, 220, 0), (107, 142, 35), (152, 251, 152),
               (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70), (0, 60, 100), (0, 0, 90), (0, 0, 110),
               (0, 80, 100), (0, 0, 230), (119, 11, 32), (0, 0, 142)]


# ------------------------------------------------------------------------------------------------ host functions of util/util.py
def labelcolormap(n):
    """util/util.py:250-294: the Cityscapes table for n == 35, otherwise colour i from the bits of i + 1, three at a time into
    (r, g, b) from the top bit down (the COCO overrides of n == 182 need the reference's util.coco and are not restated)."""
    if n == 35:
        return np.array(_CITYSCAPES, dtype=np.uint8)
    cmap = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        ident, rgb = i + 1, [0, 0, 0]
        for j in range(7):
            for c in range(3):
                rgb[c] ^= ((ident >> c) & 1) << (7 - j)
            ident >>= 3
        cmap[i] = rgb
    return cmap


def tile_images(imgs, picturesPerRow=4):
    """util/util.py:44-67: [N, H, W, ...] -> rows of picturesPerRow images side by side, the last row padded with zero images."""
    pad = (-imgs.shape[0]) % picturesPerRow
    if pad:
        imgs = np.concatenate([imgs, np.zeros((pad,) + imgs.shape[1:], dtype=imgs.dtype)], axis=0)
    rows = [np.concatenate(list(imgs[i:i + picturesPerRow]), axis=1) for i in range(0, imgs.shape[0], picturesPerRow)]
    return np.concatenate(rows, axis=0)


def save_image(image_numpy, image_path, create_dir=False):
    """util/util.py:138-147: a 2-D or 1-channel image is repeated to 3 channels; '.jpg' in the path becomes '.png'."""
    from PIL import Image
    if create_dir:
        os.makedirs(os.path.dirname(image_path), exist_ok=True)
    if image_numpy.ndim == 2:
        image_numpy = image_numpy[:, :, None]
    if image_numpy.shape[2] == 1:
        image_numpy = np.repeat(image_numpy, 3, 2)
    Image.fromarray(image_numpy).save(image_path.replace(".jpg", ".png"))



# ------------------------------------------------------------------------------------------------ kernels
class Window:
    """Where a kernel writes: a W-pixel wide window starting x_offset pixels into rows `row_stride` bytes apart, images
    `image_stride` bytes apart, from byte `offset` of the uint8 device tensor `buf`."""

    def __init__(self, buf, offset, image_stride, row_stride, x_offset=0):
        assert buf.dtype == torch.uint8 and buf.is_cuda and buf.is_contiguous() and buf.dim() == 1
        self.buf, self.offset, self.image_stride, self.row_stride, self.x_offset = buf, offset, image_stride, row_stride, x_offset

    def args(self, n, h, w):
        """(address, image stride, row stride, x offset) after checking that the last byte of the window lies inside buf."""
        end = self.offset + (n - 1) * self.image_stride + (h - 1) * self.row_stride + 3 * (self.x_offset + w)
        assert self.offset >= 0 and end <= self.buf.numel(), "window ends at byte %d of a %d-byte buffer" % (end, self.buf.numel())
        return self.buf.data_ptr() + self.offset, self.image_stride, self.row_stride, self.x_offset


def packed(n, h, w, device="cuda"):
    """A fresh [n, h, w, 3] uint8 device tensor and the Window that covers it."""
    out = torch.empty(n * h * w * 3, dtype=torch.uint8, device=device)
    return out, Window(out, 0, h * w * 3, w * 3)


def image_to_u8(x, win, normalize=True):
    """fp32 image batch -> uint8 RGB in `win`.  x: a tagged native NHWC tensor [N,H,W,cs] or plain NCHW [N,3,H,W]."""
    native, x = getattr(x, "dsee_layout", None) == "nhwc", x.detach()      # (detach() drops the layout tag)
    if native:
        n, h, w, cs = x.shape
        nchw = 0
    else:
        assert x.dim() == 4 and x.shape[1] == 3, "NCHW [N,3,H,W] or a tagged native NHWC tensor expected, got %s" % (tuple(x.shape),)
        n, _, h, w = x.shape
        cs, nchw = 0, 1
    assert x.dtype == torch.float32 and x.is_cuda
    dst, d_img, d_row, d_x = win.args(n, h, w)
    L.call("image_to_u8", x.contiguous(), dst, n, h, w, cs, nchw, int(bool(normalize)), d_img, d_row, d_x)


_tables = {}


def color_table(n_label):
    """Device copy of labelcolormap(n_label)[:n_label] (Colorize.__init__)."""
    key = (int(n_label), torch.cuda.current_device())
    if key not in _tables:
        _tables[key] = torch.from_numpy(np.ascontiguousarray(labelcolormap(n_label)[:n_label])).cuda()
    return _tables[key]


def label_colorize(lab_u8, n_label, win):
    """uint8 index map [N,H,W] -> the colours of labelcolormap(n_label) in `win`; indices >= n_label give black."""
    assert lab_u8.dtype == torch.uint8 and lab_u8.is_cuda and lab_u8.dim() == 3
    n, h, w = lab_u8.shape
    table = color_table(n_label)
    dst, d_img, d_row, d_x = win.args(n, h, w)
    L.call("label_colorize", lab_u8.contiguous(), table, table.shape[0], dst, n, h, w, d_img, d_row, d_x)


def bilinear_up_u8(src_win, n, s, win, h, w):
    """uint8 RGB [n, s, s, 3] in the window `src_win` (x_offset 0) -> [n, h, w, 3] in `win`, bilinear (see the module docstring)."""
    assert src_win.x_offset == 0
    src, s_img, s_row, _ = src_win.args(n, s, s)
    dst, d_img, d_row, d_x = win.args(n, h, w)
    L.call("bilinear_up_u8", src, s_img, s_row, s, dst, n, h, w, d_img, d_row, d_x)


# ------------------------------------------------------------------------------------------------ tensor2im / tensor2label
def _index_map(labels):
    """ops.Labels | uint8 index map [N,H,W] / [H,W] | one-hot or 1-channel float map [N,C,H,W] / [C,H,W] -> (uint8 [N,H,W] on the
    device, whether a batch dimension was given).  A multi-channel map is reduced like tensor2label does: max(0)[1]."""
    if isinstance(labels, ops.Labels):
        return labels.t, True
    t = labels.detach()
    if t.dtype == torch.uint8:
        batched = t.dim() == 3
        return (t if batched else t[None]).cuda().contiguous(), batched
    batched = t.dim() == 4
    t = t if batched else t[None]
    t = t.float().max(1, keepdim=True)[1].float() if t.shape[1] > 1 else t.float()
    return ops.label_to_u8(t.cuda()), batched


def tensor2im(image_tensor, normalize=True, tile=False):
    """util/util.py:72-103 on the device.  A tagged native NHWC batch, an NCHW batch [N,C,H,W] (C = 3 or 1), one image [C,H,W] or
    [H,W], or a list of those -> numpy uint8 [N,H,W,3] (tiled 4 per row with tile=True), [H,W,3], or without the channel axis for
    C = 1.  (`normalize` applies to a batch as well; the reference's batch branch drops the argument.)"""
    if isinstance(image_tensor, list):
        return [tensor2im(t, normalize) for t in image_tensor]
    t = image_tensor.detach()
    native = getattr(image_tensor, "dsee_layout", None) == "nhwc"
    batched = t.dim() == 4
    single = False
    if native:
        t.dsee_layout = "nhwc"
    else:
        if t.dim() == 2:
            t = t[None]
        if t.dim() == 3:
            t = t[None]
        single = t.shape[1] == 1
        t = t.float().cuda()
        if single:
            t = t.expand(-1, 3, -1, -1)
        t = t.contiguous()
    n, h, w = (t.shape[0], t.shape[1], t.shape[2]) if native else (t.shape[0], t.shape[2], t.shape[3])
    out, win = packed(n, h, w)
    image_to_u8(t, win, normalize)
    images = out.view(n, h, w, 3).cpu().numpy()
    if single:
        images = images[..., 0]
    if not batched:
        return images[0]
    return tile_images(images) if tile else images


def tensor2label(labels, n_label, tile=False, picturesPerRow=4):
    """util/util.py:107-135 on the device: colours of labelcolormap(n_label) for an index / one-hot map (see _index_map); numpy
    uint8 [N,H,W,3], tiled with tile=True, or [H,W,3] for one map."""
    if isinstance(labels, torch.Tensor) and labels.dim() == 1:
        return np.zeros((64, 64, 3), dtype=np.uint8)
    if n_label == 0:
        return tensor2im(labels)
    lab, batched = _index_map(labels)
    n, h, w = lab.shape
    out, win = packed(n, h, w)
    label_colorize(lab, n_label, win)
    images = out.view(n, h, w, 3).cpu().numpy()
    if not batched:
        return images[0]
    return tile_images(images, picturesPerRow=picturesPerRow) if tile else images


# ------------------------------------------------------------------------------------------------ the writer
def _align(v, a=16):
    return (v + a - 1) // a * a


def _file_name(path):
    """<basename without its extension>.png (visualizer.py:196 takes the basename; save_image turns .jpg into .png)."""
    return os.path.splitext(os.path.basename(path))[0] + ".png"


class _Layout:
    """Byte layout of one batch's arena: region[key] = (offset, h, w) of N packed images, `combined` likewise with
    w = columns * W."""

    def __init__(self, visuals):
        hr = visuals["image_hr"]
        native = getattr(hr, "dsee_layout", None) == "nhwc"
        self.n = hr.shape[0]
        self.h, self.w = (hr.shape[1], hr.shape[2]) if native else (hr.shape[2], hr.shape[3])
        lr = visuals["image_lr"]
        self.sh, self.sw = (lr.shape[1], lr.shape[2]) if getattr(lr, "dsee_layout", None) == "nhwc" else (lr.shape[2], lr.shape[3])
        self.s = self.sw        # (the side of a square LR image, what dsee_bilinear_up_u8 takes)
        self.guided = "guiding_image" in visuals
        self.keys = SAVE_KEYS + (GUIDED_KEYS if self.guided else ())
        self.columns = len(self.keys)
        self.region, off = OrderedDict(), 0
        for k in self.keys:
            h, w = (self.sh, self.sw) if k == "image_lr" else (self.h, self.w)
            self.region[k] = (off, h, w)
            off = _align(off + self.n * h * w * 3)
        self.region["combined"] = (off, self.h, self.columns * self.w)
        self.nbytes = off + self.n * self.h * self.columns * self.w * 3

    def window(self, buf, key):
        off, h, w = self.region[key]
        return Window(buf, off, h * w * 3, w * 3)

    def column(self, buf, index):
        off, h, w = self.region["combined"]
        return Window(buf, off, h * w * 3, w * 3, index * self.w)

    def views(self, host):
        """{key: numpy [N, h, w, 3]} over a host buffer that holds the arena."""
        out = OrderedDict()
        for k, (off, h, w) in self.region.items():
            out[k] = host[off:off + self.n * h * w * 3].reshape(self.n, h, w, 3)
        return out


def _label_nc(sem):
    return sem.nc if isinstance(sem, ops.Labels) else sem.shape[1]


def render(visuals, arena, layout):
    """Run the conversion kernels of one batch into `arena` (current stream): every visual into its own region and into its
    column of the combined strip."""
    n_label = _label_nc(visuals["input_semantics"]) + 2          # (convert_visuals_to_numpy: label_nc + 2)
    guiding_label = visuals.get("guiding_input_label", visuals.get("guiding_label"))
    order = {k: i for i, k in enumerate(layout.keys)}
    for key in layout.keys:
        targets = (layout.window(arena, key), layout.column(arena, order[key]))
        if key in ("input_semantics", "guiding_input_label"):
            lab, _ = _index_map(visuals[key] if key == "input_semantics" else guiding_label)
            assert tuple(lab.shape) == (layout.n, layout.h, layout.w), "label maps are kept at the HR size"
            for win in targets:
                label_colorize(lab, n_label, win)
        elif key == "image_lr":
            lr = _device_image(visuals[key])
            image_to_u8(lr, targets[0])
            if layout.sh == layout.sw:
                bilinear_up_u8(targets[0], layout.n, layout.s, targets[1], layout.h, layout.w)
            else:
                # dsee_bilinear_up_u8 takes ONE source side.  A non-square LR image is upsampled in fp32 (dsee_resize_hw, the
                # same half-pixel bilinear, no clamp needed: a convex combination) and converted like every other column
                if getattr(lr, "dsee_layout", None) != "nhwc":
                    lr = ops.to_nhwc(lr)
                image_to_u8(ops.resize_hw(lr, layout.h, layout.w, "bilinear", clamp=False), targets[1])
        else:
            img = _device_image(visuals[key])
            for win in targets:
                image_to_u8(img, win)


def _device_image(t):
    if getattr(t, "dsee_layout", None) == "nhwc":
        return t
    return t.detach().float().cuda().contiguous()


def _write_files(views, names, folder_out):
    for key, images in views.items():
        os.makedirs(os.path.join(folder_out, key), exist_ok=True)
        for b, name in enumerate(names):
            save_image(images[b], os.path.join(folder_out, key, name))


class ImageWriter:
    """Writes the save_images_only files of every submitted batch from a host thread.

        with ImageWriter(folder) as writer:
            for batch in loader:
                out = model(batch, "inference")
                writer.submit(out, out["path"])

    submit() enqueues the conversion kernels and one asynchronous device-to-host copy on the current stream and returns; it
    blocks only while both pinned buffers still hold batches whose files are not written yet.  close() (or leaving the `with`
    block) waits for the files and re-raises the first exception of the writer thread.  One stream: submit from the stream that
    produced the visuals."""

    SLOTS = 2

    def __init__(self, folder_out):
        self.folder_out = folder_out
        self._arena = [None] * self.SLOTS          # device, uint8
        self._pinned = [None] * self.SLOTS         # host, pinned uint8
        self._free = [threading.Event() for _ in range(self.SLOTS)]
        for e in self._free:
            e.set()
        self._events = [torch.cuda.Event() for _ in range(self.SLOTS)]
        self._queue = queue.Queue(maxsize=self.SLOTS)
        self._error = None
        self._count = 0
        self.bytes_copied = 0                      # device-to-host, all batches
        self._device = torch.cuda.current_device()
        self._thread = threading.Thread(target=self._work, name="dsee-image-writer", daemon=True)
        self._thread.start()

    def _buffers(self, slot, nbytes):
        if self._arena[slot] is None or self._arena[slot].numel() < nbytes:
            self._arena[slot] = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            self._pinned[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return self._arena[slot], self._pinned[slot]

    def submit(self, visuals, paths):
        if self._thread is None:
            raise RuntimeError("ImageWriter.submit() after close()")
        layout = _Layout(visuals)
        assert len(paths) == layout.n, "%d paths for a batch of %d" % (len(paths), layout.n)
        slot = self._count % self.SLOTS
        self._count += 1
        self._free[slot].wait()                    # its previous batch's files are written
        self._free[slot].clear()
        try:
            arena, pinned = self._buffers(slot, layout.nbytes)
            render(visuals, arena, layout)
            pinned[:layout.nbytes].copy_(arena[:layout.nbytes], non_blocking=True)
            self._events[slot].record()
        except BaseException:
            self._free[slot].set()
            raise
        self.bytes_copied += layout.nbytes
        self._queue.put((slot, layout, [_file_name(p) for p in paths]))

    def _work(self):
        torch.cuda.set_device(self._device)
        while True:
            item = self._queue.get()
            if item is None:
                return
            slot, layout, names = item
            try:
                if self._error is None:            # (after a failure the remaining batches are dropped, not written)
                    self._events[slot].synchronize()
                    _write_files(layout.views(self._pinned[slot].numpy()), names, self.folder_out)
            except BaseException as e:
                self._error = e
            finally:
                self._free[slot].set()

    def close(self, reraise=True):
        """Wait for the files of every submitted batch, stop the thread and raise the first exception it met (reraise=False:
        drop it -- for a caller that is already unwinding with an exception of its own).  Idempotent."""
        thread, self._thread = self._thread, None
        if thread is not None:
            self._queue.put(None)
            thread.join()
        error, self._error = self._error, None
        if error is not None and reraise:
            raise error

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close(reraise=exc_type is None)
        return False


def save_images_only(visuals, paths, folder_out):
    """util/visualizer.py:181-215: <folder_out>/<key>/<name>.png for input_semantics, image_lr, fake_image, image_hr (and
    guiding_image, guiding_input_label when visuals has a guiding image) and <folder_out>/combined/<name>.png.  Returns when the
    files are written."""
    with ImageWriter(folder_out) as writer:
        writer.submit(visuals, paths)
