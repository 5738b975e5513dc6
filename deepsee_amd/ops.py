"""torch.autograd.Function wrappers over the C ABI (include/deepsee_hip.h).

Everything here works on fp32 NHWC device tensors whose channel count is padded to a multiple of 4.
PyTorch supplies allocation, the stream and the autograd graph; every activation-sized computation
is a hand-written HIP kernel in libdeepsee_hip.so.  There is no CPU / ATen fallback: without the
library these functions raise.
"""
import os
import ctypes as C

import threading
from collections import namedtuple
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import lib as L
from .lib import GemmKind, WgradMode     # (the integer codes of the Winograd kernels' arithmetic, with what each implies)
from .plan import KernelPlan, DEFAULT_PLAN, current as P   # P(): the active KernelPlan of this thread (deepsee_amd/plan.py)

LRELU_SLOPE = 0.2
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
SN_EPS = 1e-12
NHIDDEN = 128

_scratch = {}

# bench.py sets this to a dict to time every MFMA conv launch with HIP events on the launch stream:
# PROFILE[kernel_name] = [(start_event, end_event, algorithmic_flops), ...]; PROFILE_BYTES[kernel_name] = algorithmic HBM bytes
PROFILE = None
PROFILE_BYTES = {}
PROFILE_OPERAND_GB = 0.0   # operand bytes the fused SPADE kernel pulls through the L2 -> LDS path in the profiled step


def _variant(geom, modulate=False):
    """Name of the kernel the C dispatcher (conv_mfma.hip: launch_conv / halo_ok) picks for this geometry."""
    halo = (geom.korder == 1 and geom.KH == 3 and geom.KW == 3 and geom.mul == 1 and geom.Hi == geom.Ho
            and geom.Wi == geom.Wo and geom.Ho % 8 == 0 and geom.Wo % 16 == 0 and geom.off == -geom.kdir)
    if modulate:
        return "conv_halo_128x128_modulate" if halo else "conv_igemm_128x128_modulate"
    if geom.Cout > 64:
        return "conv_halo_128x128" if halo else "conv_igemm_128x128"
    return "conv_igemm_256x64" if geom.Cout > 32 else "conv_igemm_128x32"


def _flops(geom):
    m = geom.N * geom.Ho * geom.Wo
    return 2.0 * m * geom.Cout * geom.KH * geom.KW * geom.Cin / (4 ** geom.dshift)


class _timed:
    def __init__(self, name, flops, nbytes=0.0):
        self.name, self.flops, self.nbytes = name, flops, nbytes

    def __enter__(self):
        if PROFILE is not None:
            self.s, self.e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.s.record()

    def __exit__(self, *a):
        if PROFILE is not None:
            self.e.record()
            PROFILE.setdefault(self.name, []).append((self.s, self.e, self.flops))
            PROFILE_BYTES[self.name] = PROFILE_BYTES.get(self.name, 0.0) + self.nbytes


def scratch(nbytes, tag="ws"):
    """Grow-only device scratch (fp32).  Safe to share: all kernels run in stream order and every
    workspace is consumed inside the C call that fills it."""
    n = (int(nbytes) + 3) // 4
    key = (tag, torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    t = _scratch.get(key)
    if t is None or t.numel() < n:
        t = torch.empty(max(n, 1024), dtype=torch.float32, device="cuda")
        _scratch[key] = t
    return t


def new(*shape):
    return torch.empty(*shape, dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------------------------ independent branches on side streams
_branch_streams = {}
_branch_tls = threading.local()


def _mark_streams(obj, stream):
    """Tensors a branch hands to the joined stream were allocated on the branch's stream: tell the caching allocator they are
    in use elsewhere too (eager mode; inside a capture the graph's private pool is not recycled across streams)."""
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda:
            obj.record_stream(stream)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _mark_streams(o, stream)
    elif isinstance(obj, dict):
        for o in obj.values():
            _mark_streams(o, stream)


def branches(*fns, inputs=()):
    """Run independent parts of the step -- the two discriminator scales, VGG(fake) / VGG(real) -- on side streams (VERDICT r4
    #4): their small layers fill a fraction of the 256 CUs each, and serialised on one stream every one of their ~600 launches
    waits for the previous one to drain.  fns[0] stays on the calling stream, fns[1:] fork from it (each side stream waits for
    everything the calling stream has enqueued) and are joined before this returns.  Inside a hipGraph capture the forks
    become parallel branches of the graph.  The autograd engine runs every node's backward on the stream of its forward and
    inserts the cross-stream waits itself, so the backward passes of the branches overlap the same way.  Scratch buffers and
    operand-maximum pools are per stream (scratch(), amax_slot()).  plan.branch_streams = False runs them in order.

    `inputs`: tensors (or nests of them) that were allocated on the CALLING stream, are consumed inside a side branch -- forward
    or backward -- and may be FREED before the step ends (activations feeding a branch, per-forward weight tensors such as the
    spectral-normalised W / sigma).  They are marked as in use on every side stream (record_stream): the caching allocator
    would otherwise hand their memory to the next allocation of the calling stream the moment the last Python reference goes --
    e.g. right after the branch's backward node RAN on the host, while its kernel is still queued on the side stream."""
    if len(fns) < 2 or not P().branch_streams:
        return [f() for f in fns]
    main = torch.cuda.current_stream()
    depth = getattr(_branch_tls, "depth", 0)
    dev = torch.cuda.current_device()
    sides = []
    for i in range(len(fns) - 1):
        key = (dev, depth, i)
        if key not in _branch_streams:
            _branch_streams[key] = torch.cuda.Stream()
        sides.append(_branch_streams[key])
    _branch_tls.depth = depth + 1
    try:
        outs = [None] * len(fns)
        for i, sd in enumerate(sides):
            _mark_streams(inputs, sd)
            sd.wait_stream(main)
            with torch.cuda.stream(sd):
                outs[i + 1] = fns[i + 1]()
        outs[0] = fns[0]()
        for i, sd in enumerate(sides):
            main.wait_stream(sd)
            _mark_streams(outs[i + 1], main)
    finally:
        _branch_tls.depth = depth
    return outs


def _under_plan(backward):
    """Run an autograd node's backward under the KernelPlan its forward recorded (ctx.plan): the engine calls it on its own
    thread, possibly while another model with another plan is mid-forward on the caller's."""
    def wrapped(ctx, *grads):
        with ctx.plan.active():
            return backward(ctx, *grads)
    wrapped.__doc__ = backward.__doc__
    return wrapped


def pad_vec(v, n):
    """[c] -> [n] zero padded (bias vectors for padded channel counts)."""
    if v is None or v.numel() == n:
        return v
    out = torch.zeros(n, dtype=torch.float32, device=v.device)
    out[: v.numel()] = v
    return out


# ------------------------------------------------------------------------------------ layout
def to_nhwc(x_nchw, cs=None):
    n, c, h, w = x_nchw.shape
    cs = cs or L.pad4(c)
    y = new(n, h, w, cs)
    L.call("nchw_to_nhwc", x_nchw.contiguous().float(), y, n, c, h, w, cs)
    y.dsee_layout = "nhwc"
    return y


def to_nchw(x_nhwc, c):
    n, h, w, cs = x_nhwc.shape
    y = new(n, c, h, w)
    L.call("nhwc_to_nchw", x_nhwc.contiguous(), y, n, c, h, w, cs)
    return y


class ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c):
        ctx.cs = x.shape[3]
        return to_nchw(x, c)

    @staticmethod
    def backward(ctx, dy):
        return to_nhwc(dy, ctx.cs), None


def label_to_u8(label):
    """float label map [N,1,H,W] -> uint8 [N,H,W]  (.long() of base_manager.py:35-39)."""
    n, _, h, w = label.shape
    out = torch.empty(n, h, w, dtype=torch.uint8, device="cuda")
    L.call("label_to_u8", label.contiguous().float(), out, C.c_long(n * h * w))
    return out


def bicubic_down(img_nhwc, size):
    n, h, w, cs = img_nhwc.shape
    y = new(n, size, size, 4)
    L.call("bicubic_down", img_nhwc, y, n, h, w, size, cs, 4)
    y.dsee_layout = "nhwc"
    return y


INTERP_MODES = {"bilinear": 0, "nearest": 1, "area": 2}


def interp_down(img_nhwc, size, mode):
    """F.interpolate(hr, (size, size), mode) + clamp(-1, 1) for mode = bilinear | nearest | area (data/preprocessor.py:29-33) of a
    native image [N,H,W,cs], H and W independent -> [N,size,size,4]."""
    if mode not in INTERP_MODES:
        raise ValueError("interp_down: mode must be one of %s, got %r" % (", ".join(INTERP_MODES), mode))
    n, h, w, cs = img_nhwc.shape
    y = new(n, size, size, 4)
    L.call("interp_down", img_nhwc.contiguous(), y, n, h, w, size, cs, 4, INTERP_MODES[mode])
    y.dsee_layout = "nhwc"
    return y


RESIZE_MODES = dict(INTERP_MODES, bicubic=3)


def resize_hw(img_nhwc, oh, ow, mode, clamp=True):
    """dsee_resize_hw: F.interpolate(x, (oh, ow), mode)[.clamp(-1, 1)] for mode = bicubic | bilinear | nearest | area of a native image
    [N,H,W,cs] -> [N,oh,ow,4], one scale per axis, down or up.  For oh == ow and clamp=True it has the bits of bicubic_down /
    interp_down (the same device functions)."""
    if mode not in RESIZE_MODES:
        raise ValueError("resize_hw: mode must be one of %s, got %r" % (", ".join(RESIZE_MODES), mode))
    n, h, w, cs = img_nhwc.shape
    y = new(n, int(oh), int(ow), 4)
    L.call("resize_hw", img_nhwc.contiguous(), y, n, h, w, int(oh), int(ow), cs, 4, RESIZE_MODES[mode], int(bool(clamp)))
    y.dsee_layout = "nhwc"
    return y


def lr_shape(opt, H, W):
    """(h, w) of the LR image of an H x W batch.  With f = crop_size // start_size a power of two that divides crop_size, H and W
    exactly: (H // f, W // f) -- Preprocessor.downsample_image(hr, shape=(H / f, W / f)), the shape from which the generator's
    upsampling levels arrive at H x W again.  Anything else (a loader mode whose shape depends on the file): the reference's
    default, a start_size square.  Pure host arithmetic; never raises."""
    s, crop = int(opt.start_size), int(opt.crop_size)
    f = crop // s if s > 0 else 0
    if f >= 1 and f & (f - 1) == 0 and s * f == crop and H % f == 0 and W % f == 0 and H >= f and W >= f:
        return H // f, W // f
    return s, s


def lr_image(opt, hr_nhwc):
    """The LR input of the generator, lr_shape(opt, H, W) in size: opt.downsampling_method selects the F.interpolate mode
    (preprocessor.py:29-30).  One kernel for every shape and mode (dsee_resize_hw); a square output has the bits of bicubic_down /
    interp_down."""
    mode = getattr(opt, "downsampling_method", "bicubic")
    if mode not in RESIZE_MODES:       # the reference's help text offers 'linear', which F.interpolate rejects for 4-D input
        raise ValueError("downsampling_method must be one of bicubic, %s, got %r" % (", ".join(INTERP_MODES), mode))
    oh, ow = lr_shape(opt, hr_nhwc.shape[1], hr_nhwc.shape[2])
    return resize_hw(hr_nhwc, oh, ow, mode, clamp=True)


def resample_u8(src, tables, out_wh, box=None):
    """dsee_resample_u8: uint8 device batch [N,Hs,Ws,C] (or [N,Hs,Ws]) through the tables of resample.batch_tables (already on
    the device: int32 tensors 'xtab', 'ytab', 'rows' + the int 'tmp_rows') -> uint8 [N,Ho,Wo,C] (resp. [N,Ho,Wo]).  box =
    (x, y, w, h) of the source the tables index; default: the whole image."""
    src = src.contiguous()
    c = src.shape[3] if src.dim() == 4 else 1
    n, hs, ws = src.shape[:3]
    x0, y0, bw, bh = box if box is not None else (0, 0, ws, hs)
    assert 0 <= x0 and 0 <= y0 and x0 + bw <= ws and y0 + bh <= hs and src.dtype == torch.uint8, (box, tuple(src.shape))
    wo, ho = out_wh
    xtab, ytab, rows, tmp_rows = tables["xtab"], tables["ytab"], tables["rows"], tables["tmp_rows"]
    assert tuple(xtab.shape[:2]) == (n, wo) and tuple(ytab.shape[:2]) == (n, ho) and tuple(rows.shape) == (n, 2)
    assert xtab.dtype == ytab.dtype == rows.dtype == torch.int32 and 0 < tmp_rows <= bh
    tmp = scratch(n * tmp_rows * wo * c, "resample").view(torch.uint8)
    dst = torch.empty((n, ho, wo, c) if src.dim() == 4 else (n, ho, wo), dtype=torch.uint8, device="cuda")
    L.call("resample_u8", src, tmp, dst, n, c, (y0 * ws + x0) * c, hs * ws * c, ws * c, bw, bh, wo, ho, tmp_rows,
           xtab, xtab.shape[2] - 2, ytab, ytab.shape[2] - 2, rows)
    return dst


def resample_u8_ragged(arena, items_host, tables, out_wh, c):
    """dsee_resample_u8_ragged: the sources of N samples of different sizes in one uint8 device arena (resample.pack_arena) through
    the tables of resample.ragged_tables (on the device: 'xtab', 'ytab', 'rows' int32, 'items' int64 [N,4] + the int 'tmp_rows')
    -> uint8 [N,Ho,Wo,3] for c = 3, [N,Ho,Wo] for c = 1.  items_host is the host copy of 'items': every sample's box is checked
    against the arena here, before the call."""
    items_host = np.asarray(items_host, dtype=np.int64)         # (numpy: a handful of N-element operations, microseconds)
    n, size = items_host.shape[0], arena.numel()
    assert arena.dtype == torch.uint8 and arena.dim() == 1 and arena.is_contiguous() and c in (1, 3)
    assert items_host.shape == (n, 4)
    off, stride, bw, bh = items_host.T
    assert off.min() >= 0 and bw.min() > 0 and bh.min() > 0, "item table: negative offset or empty box"
    assert (stride >= bw * c).all(), "item table: a row stride below box_w * c"
    assert (off + (bh - 1) * stride + bw * c).max() <= size, "item table: a box reaches past the arena's %d bytes" % size
    wo, ho = out_wh
    xtab, ytab, rows, items, tmp_rows = tables["xtab"], tables["ytab"], tables["rows"], tables["items"], tables["tmp_rows"]
    assert tuple(xtab.shape[:2]) == (n, wo) and tuple(ytab.shape[:2]) == (n, ho) and tuple(rows.shape) == (n, 2)
    assert xtab.dtype == ytab.dtype == rows.dtype == torch.int32 and items.dtype == torch.int64 and tuple(items.shape) == (n, 4)
    assert 0 < tmp_rows <= int(bh.max())
    tmp = scratch(n * tmp_rows * wo * c, "resample").view(torch.uint8)
    dst = torch.empty((n, ho, wo, c) if c == 3 else (n, ho, wo), dtype=torch.uint8, device="cuda")
    L.call("resample_u8_ragged", arena, size, items, tmp, dst, n, c, wo, ho, tmp_rows, xtab, xtab.shape[2] - 2,
           ytab, ytab.shape[2] - 2, rows)
    return dst


def bicubic_up(img_nhwc, h, w, clamp=True):
    """F.interpolate(x, (h, w), mode='bicubic')[.clamp(-1, 1)] of a square native image [N,S,S,cs] -> [N,h,w,4] (the 'baseline'
    every SR table is compared against, sr_model.py:109-115)."""
    n, s, s2, cs = img_nhwc.shape
    assert s == s2, "square source expected, got %s" % (tuple(img_nhwc.shape),)
    y = new(n, h, w, 4)
    L.call("bicubic_up", img_nhwc.contiguous(), y, n, s, h, w, cs, 4, int(bool(clamp)))
    y.dsee_layout = "nhwc"
    return y


MAX_LABELS = 32      # one-hot columns of every per-image table and of dsee_label_onehot; L <= 32 in the label kernels


def check_label_count(nc):
    """ValueError unless 1 <= nc <= MAX_LABELS.  Raised where a model or a label map is BUILT, so that no pass can fail
    half-way (a forward that succeeds and a backward that stops after other gradients were written)."""
    if not 1 <= int(nc) <= MAX_LABELS:
        raise ValueError("%d semantic classes: the kernels keep the one-hot label in %d columns (1 <= semantic_nc <= %d)"
                         % (nc, MAX_LABELS, MAX_LABELS))
    return int(nc)


class Labels:
    """uint8 HR label map + the shift for a given resolution (nearest resize as index math)."""

    def __init__(self, lab_u8, nc):
        self.t = lab_u8
        self.n, self.h, self.w = lab_u8.shape
        self.nc = check_label_count(nc)      # (so every consumer below, forward and backward, sees 1..32 classes)

    def shift_for(self, r, rw=None):
        """Shift that maps an r x rw feature map (rw None: the same fraction of the width) onto the label map.  Both axes must be
        the same power-of-two fraction: the label kernels index row h << shift, column w << shift of a [H][W] map."""
        s = 0
        while (self.h >> s) > r:
            s += 1
        assert (self.h >> s) == r, "resolution %d is not a power-of-two fraction of %d" % (r, self.h)
        if rw is not None:
            assert (self.w >> s) == rw, \
                "%d x %d is not the same power-of-two fraction of the %d x %d label map on both axes" % (r, rw, self.h, self.w)
        return s


class PhiloxNormal:
    """A N(0,1) tensor that is never materialised: the Philox stream (seed, offset) of dsee_rng_fill, regenerated in
    registers by the consumers (UpNoise forward and the noise-weight gradient)."""

    def __init__(self, shape, seed, offset, source=None):
        self.shape, self.seed, self.offset = tuple(shape), int(seed), int(offset)
        self.source = source     # the DeviceNoise whose device-side epoch offsets this stream

    def bind(self):
        """Make the library read THIS stream's epoch (one device int64 per DeviceNoise, i.e. per model): with two models
        in a process, a backward pass that regenerates a forward's draws must not pick up the other model's epoch."""
        if self.source is not None:
            self.source.ensure_registered()

    def materialize(self):
        self.bind()
        return rng_fill(self.shape, self.seed, self.offset, True)


class PhiloxField:
    """One N(0,1) scalar per label pixel, [N, H, W], never materialised: the Philox stream (seed, offset) of dsee_rng_fill for an
    [N,H,W,1] tensor, regenerated per tile by onehot_noise_conv3x3 (forward and weight gradient).  `use_epoch`: the device
    epoch of `source` (a networks.DeviceNoise) offsets the stream, as for every training draw; False: (seed, offset) are
    taken as they are -- the eval-mode stream, which must not depend on where training stands."""

    def __init__(self, shape, seed, offset, use_epoch=True, source=None):
        self.shape = tuple(shape)
        self.seed, self.offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
        self.use_epoch, self.source = bool(use_epoch), source

    def bind(self):
        if self.use_epoch and self.source is not None:
            self.source.ensure_registered()


def _bind_rng(*streams):
    for e in streams:
        if isinstance(e, PhiloxNormal):
            e.bind()


def rng_fill(shape, seed, offset, normal=True):
    t = new(*shape)
    assert t.numel() % 4 == 0
    L.call("rng_fill", t, C.c_long(t.numel()), C.c_uint64(seed), C.c_uint64(offset), int(normal))
    return t


# ------------------------------------------------------------------------------------ convolution
def _frozen_cache(w, key, build):
    """Weight-derived tensors of a FROZEN parameter (the VGG19 taps: requires_grad False, never stepped) are built once and
    kept on the parameter, keyed by its version: 13 layers x 2 passes x (pack + max |w|) launches per step otherwise."""
    # (opt-in by the owner -- networks.VGG19Taps marks its parameters `dsee_frozen`: "requires_grad is False" alone also holds for
    # the discriminator's weights during the generator step, and the fused Adam kernel does not bump tensor versions)
    if not getattr(w, "dsee_frozen", False) or w.requires_grad:
        return build()
    cache = w.__dict__.setdefault("_dsee_frozen", {})
    if cache.get("version") != w._version or cache.get("ptr") != w.data_ptr():
        cache.clear()
        cache["version"], cache["ptr"] = w._version, w.data_ptr()
    if key not in cache:
        if torch.cuda.is_current_stream_capturing():
            return build()       # (a tensor allocated inside a capture lives in the graph's pool: not cacheable)
        cache[key] = build()
    return cache[key]


def _pack(kind, w, c_s, korder):
    """Packed weights of a direct kernel with the maximum w carries.  "fwd": one row per output channel, c_s = padded Cin;
    "dgrad": one row per input channel, c_s = padded Cout."""
    def build():
        co, ci, kh, kw = w.shape
        wp = new(L.wrows(L.pad4(co if kind == "fwd" else ci)), L.kpad(kh, kw, c_s))
        L.call("pack_weight_" + kind, w, None, None, wp, co, ci, kh, kw, c_s, korder)
        wp.dsee_amax = getattr(w, "dsee_amax", None)     # (a permutation + zero padding of w: same maximum)
        if wp.dsee_amax is None and getattr(w, "dsee_frozen", False):
            wp.dsee_amax = torch.zeros(AMAX_FLOATS, dtype=torch.float32, device=wp.device)
            L.call("absmax", wp, wp.numel(), wp.dsee_amax)
        return wp
    return _frozen_cache(w, (kind, c_s, korder), build)


def tensor_amax(t, cache=None):
    """Device-side max |t| (2048-float slot).  `cache`: a dict shared by the consumers of the same tensors (the data and
    the weight gradient both read dy, the forward conv and the weight gradient both read x): one pass per tensor."""
    if carried_amax(t) is not None:      # carried by its producer (spectral-norm group launch)
        return t.dsee_amax
    key = (t.data_ptr(), t.numel(), t._version)
    if cache is not None and key in cache:
        return cache[key]
    a = amax_slot()
    L.call("absmax", t, t.numel(), a)
    if cache is not None:
        cache[key] = a
    return a


def _s2_parity_ok(geom, kh, kw):
    return (P().dgrad_s2_parity and geom.mul == 2 and kh == 4 and kw == 4 and geom.off == -2 and geom.ups == 0 and geom.kdir == 1)


def _dgrad_stride2_parity(g, w, geom, ci, amax_cache=None, exact=False):
    """Data gradient of a 4 x 4 / stride 2 / padding 2 convolution (the discriminator's down-sampling layers,
    discriminator.py:78-96) by output parity (round 6).  dx[2a + py] = dy[a + 1] w[py] + dy[a] w[py + 2] per dimension: each of
    the four (py, px) classes of input pixels is a dense 2 x 2 / stride 1 convolution over dy with its own quarter of the taps,
    all four with the SAME source window -- so they run as ONE convolution with 4 Cin output columns (K = 4 Cout instead of 16
    Cout of which three quarters multiplied zeros: the general kernel reached 15-20 TFLOP/s of useful work) followed by a
    depth-to-space copy."""
    co = w.shape[0]
    cin_s, n, h, wd = geom.Cin, geom.N, geom.Hi, geom.Wi
    ha, wa = (h + 1) // 2, (wd + 1) // 2
    wq = w if ci == cin_s else torch.nn.functional.pad(w, (0, 0, 0, 0, 0, cin_s - ci))
    # [co][c][a][py][b][px] -> [co][(py, px, c)][a][b]: tap (a, b) of parity class (py, px) is the forward tap (2 a + py, 2 b + px)
    w4 = wq.reshape(co, cin_s, 2, 2, 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(co, 4 * cin_s, 2, 2)
    if getattr(w, "dsee_amax", None) is not None:
        w4.dsee_amax = w.dsee_amax                    # (a permutation of w: same maximum)
    korder = 1 if geom.Cout % 32 == 0 else 0
    gd = L.ConvGeom(n, geom.Ho, geom.Wo, geom.Cout, ha, wa, 4 * cin_s, 2, 2, 1, 1, -1, 0, 0, korder)
    z = conv_raw(g, _pack("dgrad", w4, geom.Cout, korder), gd, amax_cache=amax_cache, exact=exact)
    dx = z.view(n, ha, wa, 2, 2, cin_s).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * ha, 2 * wa, cin_s)
    dx = dx[:, :h, :wd].contiguous() if (2 * ha != h or 2 * wa != wd) else dx.contiguous()
    if carried_amax(z) is not None:
        tag_amax(dx, z.dsee_amax)         # (a permutation / crop of z: the same bound)
    return dx


def _direct_split_on(exact=False):
    """the direct implicit-GEMM layers run on split fp16 operands (and therefore need operand maxima)"""
    return (not exact) and P().gemm_split and P().gemm_f16x2 and P().conv_f16x2_min_flop > 0


def conv_raw(x, wp, geom, bias=None, res=None, act=L.ACT_NONE, slope=LRELU_SLOPE, res_ld=0, amax_cache=None, exact=False):
    out = new(geom.N, geom.Ho, geom.Wo, geom.Cout)
    # round 6: the epilogue writes max |out| -- the bound the NEXT direct layer's fp16x2 split needs (VGG conv -> conv, the data
    # gradient chain through D / VGG) -- instead of a stand-alone absmax pass over the activation (55 such passes per step before)
    ao = amax_slot() if (_direct_split_on(exact) and P().conv_amax_out) else None
    if _direct_split_on(exact) and _flops(geom) >= P().conv_f16x2_min_flop:
        ax, aw = tensor_amax(x, amax_cache), tensor_amax(wp)
        with _timed(_variant(geom).replace("halo", "igemm") + "_f16x2", _flops(geom)):   # (the halo kernel is fp32-only)
            L.call("conv2d_fwd_f16x2_amax", C.byref(geom), x, wp, bias, res, res_ld, out, act, float(slope), ax, aw, ao,
                   0 if P().conv_halo_f16 else 1)       # (1 = DSEE_CONV_NO_HALO)
    else:
        with _timed(_variant(geom), _flops(geom)):
            L.call("conv2d_fwd_amax", C.byref(geom), x, wp, bias, res, res_ld, out, act, float(slope), ao)
    if ao is not None:
        tag_amax(out, ao)
    return out


def wgrad_raw(x, dout, geom, cout, cin, kh, kw, cin_first=0, amax_cache=None, exact=False):
    nbytes = L.lib().dsee_conv2d_wgrad_workspace(C.byref(geom))
    ws = scratch(nbytes, "wgrad")
    dw = new(cout, cin, kh, kw)
    flops = _flops(geom) * ((cin + 31) // 32 * 32 if geom.korder else geom.Cin) / geom.Cin
    if not exact and P().gemm_split and P().gemm_f16x2 and P().conv_f16x2_min_flop > 0 and flops >= P().conv_f16x2_min_flop:
        ax, ad = tensor_amax(x, amax_cache), tensor_amax(dout, amax_cache)
        with _timed("conv_wgrad_128x128_f16x2(+slab reduce)", flops):
            L.call("conv2d_wgrad_f16x2", C.byref(geom), x, dout, ws, C.c_size_t(nbytes), dw, cout, cin_first, cin, ax, ad)
        return dw
    with _timed("conv_wgrad_128x128(+slab reduce)", flops):
        L.call("conv2d_wgrad", C.byref(geom), x, dout, ws, C.c_size_t(nbytes), dw, cout, cin_first, cin)
    return dw


def channel_dot(a, b, c):
    """[c] = sum over rows of a*b (b None: column sums); a viewed as [M, C]."""
    cs = a.shape[-1]
    m = a.numel() // cs
    ws = scratch(L.lib().dsee_channel_dot_workspace(C.c_long(m), cs), "chdot")
    out = new(cs)
    L.call("channel_dot", a, b, out, C.c_long(m), cs, ws)
    return out[:c]


# ---- Winograd F(4x4,3x3) for the wide 3x3 / stride-1 layers (4x fewer fp32 MACs than the direct form)


def _wino_chunk(n, h, w, cmax, per_image=False):
    """Images per Winograd pass.  A 128-row GEMM tile must not straddle two groups (transform positions; with
    per_image also images).  The fp32-MFMA kernels address the transformed tensors [36][T][C] with 32-bit byte
    offsets; the bf16x3 path (64-bit tile bases) is only bounded to 16 GB per operand."""
    if h % 4 or w % 4:
        return None
    tpi = (h // 4) * (w // 4)
    wide = P().gemm_split and cmax % 32 == 0
    for nb in range(n, 0, -1):
        fits = 36 * nb * tpi * cmax * 6 < (1 << 34) if wide else 36 * nb * tpi * cmax * 4 < 0xF0000000
        if n % nb == 0 and fits and ((tpi if per_image else nb * tpi) % 128 == 0):
            return nb
    return None


def _wino_mod_chunk(n, h, w, c, rows, per_image):
    """Images per pass of the Winograd gamma/beta GEMM (None: use the direct kernel)."""
    if not (P().winograd and P().winograd_mod and c % 64 == 0 and rows == 2 * c and rows % 128 == 0):
        return None
    return _wino_chunk(n, h, w, rows, per_image)


def _wino_ok(n, h, w, cin_s, cout_s, k, stride, pad, ups):
    return (P().winograd and k == 3 and stride == 1 and pad == 1 and ups == 0 and cin_s % 32 == 0 and cout_s % 128 == 0
            and cin_s >= 128 and _wino_chunk(n, h, w, max(cin_s, cout_s)) is not None)


def _u_kind(k_s, r_s, x_pk=False, dm_form=None, f16_only=False):
    """The GemmKind of the weights U of one NT GEMM (k_s reduction, r_s output channels): the plan's for the shape, or packed where the
    A operand is -- a forward V whose layer takes the packed chain (`x_pk`: _pk_ok), an adjoint GEMM whose dM is packed (`dm_form`).
    `f16_only`: the fused norm and the spectral-norm group's batch transform, which exist in the two-term and the packed form only."""
    if f16_only:
        return GemmKind.F16_PACKED if P().half else GemmKind.F16X2_AF32
    if dm_form == F16P:
        return GemmKind.F16_PACKED
    if not (P().gemm_split and k_s % 32 == 0 and r_s % 128 == 0):
        return GemmKind.FP32
    af32 = P().gemm_af32 and k_s * 4 * 256 < 0x7FFFFFFF
    if P().half and af32:
        return GemmKind.F16_PACKED if x_pk else GemmKind.F16_AF32
    return GemmKind.F16X2_AF32 if (P().gemm_f16x2 and af32) else GemmKind.BF16X3


_split_kind = _u_kind       # (k_s, r_s): the kind the plan gives a shape, never F16_PACKED


def _i16(n):
    return torch.empty(n, dtype=torch.int16, device="cuda")


_amax_pools = {}
AMAX_FLOATS = 64 * 32   # DSEE_AMAX_LINES x DSEE_AMAX_STRIDE (dsee_common.h): a maximum lives in 64 separate cache lines


def amax_slot():
    """A zeroed device buffer for the atomic max |x| of one tensor (operand scale of the fp16 GEMMs; also used for the
    one-float output scale of the 16-bit mode).  Slots come from a 4 MB pool that is zero-filled once per 512 uses;
    every slot is used for one tensor only."""
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    st = _amax_pools.get(key)
    if st is None or st[1] + AMAX_FLOATS > st[0].numel():
        st = [torch.zeros(512 * AMAX_FLOATS, dtype=torch.float32, device="cuda"), 0]
        _amax_pools[key] = st
    t = st[0][st[1]:st[1] + AMAX_FLOATS]
    st[1] += AMAX_FLOATS
    return t


def tag_amax(t, slot):
    """Attach the operand bound `slot` (device max |t|, written by t's producer) to an ACTIVATION / GRADIENT tensor together
    with the tensor version it was measured at.  Such a tensor may cross the autograd engine, which sums fan-in gradients
    in place (InputBuffer add_): the sum keeps one addend's Python attributes but not its maximum.  The in-place add bumps
    `_version`, so carried_amax() then ignores the stale bound."""
    t.dsee_amax, t.dsee_amax_ver = slot, t._version
    return slot


def carried_amax(t):
    """The operand bound attached to `t`, or None -- also None when `t` was modified in place after the bound was measured."""
    a = getattr(t, "dsee_amax", None)
    if a is not None and getattr(t, "dsee_amax_ver", t._version) != t._version:
        return None
    return a


def begin_capture():
    """Called right before a hipGraph capture starts: the zero-fill of an operand-maximum pool must be part of the graph
    that uses its slots (a replay has to find them zeroed), so pools handed out earlier are dropped."""
    _amax_pools.clear()


def weight_amax(*tensors):
    """max |w| over the given weight tensors (device scalar): |G g G^T| <= max |g|, so it bounds the Winograd-domain
    weights built from them.  A weight that carries its maximum (`.dsee_amax`, written by the spectral-norm group launch)
    needs no pass of its own."""
    live = [t for t in tensors if t is not None]
    carried = [getattr(t, "dsee_amax", None) for t in live]
    if live and carried[0] is not None and all(c is carried[0] for c in carried):
        return carried[0]                 # every tensor's maximum went into the same slot
    a = amax_slot()
    for t in tensors:
        if t is not None:
            L.call("absmax", t.contiguous(), t.numel(), a)
    return a


def _u_key(transpose_flip, kind, rows, kp):
    return (int(transpose_flip), int(kind), rows, kp)     # key of a U in `dsee_u`: SNGroup.wino_weights writes it, _wino_u reads


def _wino_u(w, co, ci, transpose_flip, rows, kp, kind):
    """Winograd-domain weights U [36][rows][kp] of `kind` (a GemmKind or its integer): fp32, or kind.words int16 words per element.
    Returns (U, amax) with amax = the device scalar the fp16 scale was derived from (None where the kind has none)."""
    kind, key, pre = GemmKind(kind), _u_key(transpose_flip, kind, rows, kp), getattr(w, "dsee_u", None)
    if pre is not None and key in pre:
        return pre[key]       # transformed with its whole network (SNGroup.wino_weights)
    def build():
        if kind.needs_amax and getattr(w, "dsee_frozen", False):
            amax = torch.zeros(AMAX_FLOATS, dtype=torch.float32, device=w.device)     # (kept with the cached U: not a pool slot)
            L.call("absmax", w, w.numel(), amax)
        else:
            amax = weight_amax(w) if kind.needs_amax else None
        u = _i16(36 * rows * kp * kind.words) if kind else new(36, rows, kp)
        L.call("wino43_weights", w, u, co, ci, int(transpose_flip), int(kind), amax)
        return u, amax
    return _frozen_cache(w, ("u",) + key, build)


FUSED_V_BOUND = 100.0       # |B^T d B| <= 100 max|d| for F(4x4,3x3): scale of a pre-split V from max |input|

# the four storage forms of a Winograd-domain operand (V of an input, dM = A dY A^T of an output gradient)
FP32 = "fp32"               # [36][t][c] fp32; amax = its device maximum (None where no fp16 kernel will scale by it)
F16X2 = "f16x2"             # two scaled fp16 terms per element, written by the transform; amax = max |input| it was scaled with
F16P = "f16p"               # ONE scaled fp16 term per element (16-bit storage mode); amax as for F16X2
BF16X3_T = "bf16x3_t"       # transposed, three bf16 terms per element (weight-gradient mode 1); no maximum
WinoOperand = NamedTuple("WinoOperand", [("data", torch.Tensor), ("amax", Optional[torch.Tensor]), ("form", str)])


def save_with_operand(ctx, op, *tensors):
    """ctx.save_for_backward(*tensors) plus one WinoOperand (or None): its tensors are saved with the others, its form on ctx."""
    ctx.operand_form = None if op is None else op.form
    ctx.save_for_backward(*tensors, *((None, None) if op is None else op[:2]))


def saved_with_operand(ctx):
    """(tensors, operand) as save_with_operand() stored them"""
    *tensors, data, amax = ctx.saved_tensors
    return tensors, (None if data is None else WinoOperand(data, amax, ctx.operand_form))


def _presplit_ok(xc, t, t_g, r_s, k_s=0, keep=False):
    """dsee_gemm_f16x2_pre takes 256 x 256 tiles only; below 512 of them the 128 x 128 kernel fills the chip better.
    `keep`: the weight gradient will read the same V2 (dsee_gemm_f16x2_tn_qpre: 160 or a multiple of 128 columns)."""
    return (P().presplit_a and carried_amax(xc) is not None and t_g % 256 == 0 and r_s % 256 == 0
            and (36 * t // 256) * (r_s // 256) >= P().presplit_min_tiles and (not keep or k_s == 160 or k_s % 128 == 0))


def _gemm_pre(name, k_s, r_s):
    """Entry point of a pre-split NT GEMM: the one-wave-per-SIMD kernel (csrc/gemm_w4.hip, round 6) where its shape rules hold --
    whole 256-column tiles and an even number of 64-byte-row slabs -- else the 8-wave ping-pong kernel."""
    slab = 32 if name == "gemm_f16p_pre" else 16
    if P().gemm_w4 and r_s % 256 == 0 and k_s % (2 * slab) == 0:
        return name + "_w4"
    return name


def _pk_ok(xc, t_g, r_s, k_s):
    """16-bit storage mode (plan.half): the layer takes the packed one-term kernels (dsee_wino43_input_f16p ->
    dsee_gemm_f16p_pre -> fp16 product) when the input's maximum was written by its producer, every GEMM group is whole
    256-row tiles, the output width whole 128-column tiles and the reduction whole 32-channel slabs."""
    return (P().half and P().presplit_a and P().gemm_split and P().gemm_af32 and carried_amax(xc) is not None
            and t_g % 256 == 0 and r_s % 128 == 0 and k_s % 32 == 0)


def _wino_vgemm(xc, nb, h, wd, k_s, u, r_s, rows, kp, per_image, kind, keep=None, u_amax=None):
    """(M [36][t][r_s], mscale) = V(xc) x U: input transform of `nb` images + the 36 (x nb with per-image weights) GEMMs.
    mscale: None (M is fp32) or the device scalar that rescales the fp16 M of the half-precision mode.
    `keep` (a list) receives V as a WinoOperand where the weight gradient can read it as its Q operand."""
    tpi = (h // 4) * (wd // 4)
    t = nb * tpi
    groups, t_g = (36 * nb, tpi) if per_image else (36, t)
    m = torch.empty(36, t, r_s, dtype=torch.float16, device="cuda") if kind.f16_product else new(36, t, r_s)
    ms = amax_slot() if kind.f16_product else None
    shape, flops = (36 * t, r_s, k_s, t_g, rows), 2.0 * 36 * t * k_s * r_s
    if kind == GemmKind.BF16X3 and not (P().gemm_af32 and k_s * 4 * 256 < 0x7FFFFFFF):
        v = _i16(36 * t * k_s * 3)
        L.call("wino43_input_split", xc, v, nb, h, wd, k_s)
        with _timed(kind.timer, flops, 6.0 * 36 * t * k_s + 6.0 * groups * rows * k_s + 4.0 * 36 * t * r_s):
            L.call("gemm_bf16x3", v, u, m, *shape, 0)
        return m, ms
    pk = kind == GemmKind.F16_PACKED
    if pk or (kind == GemmKind.F16X2_AF32 and _presplit_ok(xc, t, t_g, r_s, k_s, keep is not None)):
        # the input's maximum is known (written by its producer): the transform writes V already split (two scaled fp16 terms per
        # element; ONE in the 16-bit storage mode) with the scale fixed by |B^T d B| <= 100 max|d|; the GEMM streams it as it is
        v = WinoOperand(_i16(36 * t * k_s * (1 if pk else 2)), xc.dsee_amax, F16P if pk else F16X2)
        L.call("wino43_input_f16p" if pk else "wino43_input_f16x2", xc, v.data, nb, h, wd, k_s, v.amax, FUSED_V_BOUND)
    else:
        v = WinoOperand(new(36, t, k_s), amax_slot() if kind.needs_amax else None, FP32)     # (its maximum: the fp16 GEMMs' scale)
        L.call("wino43_input", xc, v.data, nb, h, wd, k_s, v.amax)
    if kind == GemmKind.FP32:
        g = L.ConvGeom(groups, t_g, 1, k_s, t_g, 1, r_s, 1, 1, 1, 0, 1, 0, 0, 1)
        with _timed(kind.timer, flops):
            L.call("conv2d_fwd_grouped", C.byref(g), v.data, u, rows * kp, m)
        return m, ms
    with _timed(kind.timer, flops, kind.gemm_bytes(t, k_s, r_s, groups, rows)):
        _wino_gemm(v, FUSED_V_BOUND, u, u_amax, m, shape, kind, ms)
    if keep is not None:
        keep.append(v)         # the weight gradient's Q operand as it is
    return m, ms


def _wino_gemm(a, bound, u, u_amax, m, shape, kind, ms):
    """m = a x u, `shape` = (M, N, K, rows per group, weight rows) of the grouped NT GEMM: the kernel by the form of operand
    a (pre-split: scaled by `bound` x a.amax) and, for an fp32 a, by the GemmKind of u; `ms`: slot for an fp16 m's scale."""
    if a.form == F16P:
        L.call(_gemm_pre("gemm_f16p_pre", shape[2], shape[1]), a.data, u, m, *shape, a.amax, bound, u_amax, ms)
    elif a.form == F16X2:
        L.call(_gemm_pre("gemm_f16x2_pre", shape[2], shape[1]), a.data, u, m, *shape, a.amax, bound, u_amax)
    elif kind == GemmKind.F16_AF32:
        L.call("gemm_f16_af32", a.data, u, m, *shape, 0, a.amax, u_amax, 1, ms)
    elif kind == GemmKind.F16X2_AF32:
        L.call("gemm_f16x2_af32", a.data, u, m, *shape, 0, a.amax, u_amax)
    else:
        L.call("gemm_bf16x3_af32", a.data, u, m, *shape, 0)


def _wino_conv(x, w, n, h, wd, cin_s, cout_s, transpose_flip, bias=None, res=None, act=L.ACT_NONE, res_ld=0, keep=None,
               noise=None, res_noise=None, stats=False):
    """y = conv3x3(x, w) (transpose_flip: data gradient of that conv) through 36 Winograd-domain GEMMs.
    `keep`: list that receives the WinoOperand V of the input when the whole batch went through in one pass.
    `noise` = (noise_w [r_s], PhiloxNormal of y's shape): y += noise_w * eps in the output transform;
    `res_noise`: the same on the residual (res + w * eps is what gets added)."""
    co, ci = w.shape[0], w.shape[1]
    r_s, k_s = (cin_s, cout_s) if transpose_flip else (cout_s, cin_s)   # GEMM output / reduction channels
    rows, kp = L.wrows(r_s), L.kpad(1, 1, k_s)
    nb = _wino_chunk(n, h, wd, max(r_s, k_s))
    kind = _u_kind(k_s, r_s, x_pk=nb == n and _pk_ok(x, n * (h // 4) * (wd // 4), r_s, k_s))
    u, ua = _wino_u(w, co, ci, transpose_flip, rows, kp, kind)
    y = new(n, h, wd, r_s)
    for n0 in range(0, n, nb):
        xc = x if nb == n else x[n0:n0 + nb]
        if nb != n and carried_amax(x) is not None:
            tag_amax(xc, x.dsee_amax)           # (the maximum of the whole batch bounds every chunk)
        m, ms = _wino_vgemm(xc, nb, h, wd, k_s, u, r_s, rows, kp, False, kind, keep if nb == n else None, ua)
        nz = (None, 0, 0) if noise is None else (noise[0], noise[1].seed, noise[1].offset + n0 * h * wd * r_s // 4)
        rz = ((None, 0, 0) if res_noise is None else
              (res_noise[0], res_noise[1].seed, res_noise[1].offset + n0 * h * wd * r_s // 4))
        if (stats and P().producer_stats and nb == n and (ms is None or kind == GemmKind.F16_PACKED) and act != L.ACT_MASK
                and _stats_rows_ok(r_s)):
            rows = L.lib().dsee_stats_part_rows(C.c_long(nb * (h // 4) * (wd // 4) * (r_s // 4)))
            part = new(rows, 3, r_s)
            L.call("wino43_output_stats" if ms is None else "wino43_output_stats_f16", m, bias, res, res_ld or r_s, y, nb, h, wd,
                   r_s, act, LRELU_SLOPE, *nz, *rz, *(() if ms is None else (ms,)), part)
            y.dsee_stats_rows = (part, rows)
            continue
        L.call("wino43_output", m, bias, None if res is None else res[n0:n0 + nb], res_ld or r_s, y[n0:n0 + nb], nb, h, wd,
               r_s, act, LRELU_SLOPE, *nz, *rz, ms)
    return y


def _wgrad_mode(cin_s, cout_s):
    """The WgradMode of a layer: AF32 takes 256-row tiles (cout_s % 256 == 0, cin_s == 160 or % 128 == 0)."""
    if not (P().gemm_split and cout_s % 128 == 0 and cin_s % 32 == 0):
        return WgradMode.FP32
    if P().gemm_af32 and cout_s % 256 == 0 and (cin_s == 160 or cin_s % 128 == 0) and max(cin_s, cout_s) * 64 < 0x7FFFFFFF:
        return WgradMode.AF32
    return WgradMode.BF16X3_T


def _wgrad_split(mode):
    """Kernel code of dsee_wino43_wgrad[_table] for a mode on fp32 operands: its value, or in AF32 3 = fp16x2, 4 = one fp16 term."""
    if mode == WgradMode.AF32 and P().half:
        return 4
    return 3 if (mode == WgradMode.AF32 and P().gemm_f16x2) else int(mode)


def _wgrad_name(mode):
    return "winograd_wgrad_" + {0: "128x128(36 groups)", 4: "f16_1term", 3: "f16x2"}.get(_wgrad_split(mode), "bf16x3")


def _dout_sums_ok(n, nb, cout_s, mode):
    """The channel sums over dY (bias / noise-weight gradients) can ride in the A dY A^T transform (dsee_wino43_dout_sums)."""
    return P().dout_sums and nb == n and mode != WgradMode.BF16X3_T and cout_s // 4 <= 256 and 256 % (cout_s // 4) == 0


# Every dM holds f_i f_j (A dY A^T)[i][j], f = (1, 1/4, 1/4, 1/16, 1/16, 1) (include/deepsee_hip.h, "ROW FACTORS": the absolute row
# sums of A are 1, 4, 4, 15, 15, 1), bounded by max|dY| at every position; the consumers of the GEMM results (weight-gradient
# finalize, adjoint input transform) undo the factors
DM_BOUND = 1.0


# kernel code of dsee_wino43_wgrad[_table] per (V form, dM form); None: the weight-gradient mode decides (_wgrad_split)
_WGRAD_CODES = {(FP32, FP32): None, (BF16X3_T, BF16X3_T): None, (F16X2, FP32): 5, (F16X2, F16X2): 6, (F16P, F16P): 7}


def _wgrad_code(v, dm, mode):
    """Kernel code 0..7 of dsee_wino43_wgrad[_table] for the operand forms at hand, the one place that produces it; a pairing no
    kernel takes raises (a packed one-term V needs a packed one-term dM: dsee_gemm_f16p_tn_pqpre)."""
    mode = WgradMode(mode)
    if (v.form, dm.form) not in _WGRAD_CODES or (v.form == BF16X3_T) != (mode == WgradMode.BF16X3_T):
        raise ValueError("no weight-gradient kernel for V %s x dM %s in mode %d" % (v.form, dm.form, mode))
    return _WGRAD_CODES[(v.form, dm.form)] or _wgrad_split(mode)


def _fp16_amax_needed():
    """fp32 operands get their maximum measured: an fp16 GEMM will scale them by it"""
    return P().gemm_split and (P().gemm_f16x2 or P().half)


def _wino_dout(gc, nb, h, wd, cout_s, form, sums=None):
    """dM = A dY A^T of one image chunk as a WinoOperand of `form`: FP32, or F16X2 / F16P scaled by the maximum dY carries.
    `sums`: {"bias": bool, "n0": PhiloxNormal | None, "n1": ...} -- the bias gradient and the NoiseInjection weight gradients
    of the layer, computed by the same pass and returned in the same dict as "dbias" / "dn0" / "dn1"."""
    t = nb * (h // 4) * (wd // 4)
    n0, n1 = (sums.get("n0"), sums.get("n1")) if sums else (None, None)
    db = new(cout_s) if sums and sums.get("bias") else None
    dn0, dn1 = (new(cout_s) if n0 is not None else None), (new(cout_s) if n1 is not None else None)
    if sums:
        sums.update(dbias=db, dn0=dn0, dn1=dn1)
    r0, r1 = ((r.seed, r.offset) if r is not None else (0, 0) for r in (n0, n1))
    tail = (db, dn0, *r0, dn1, *r1)          # the seven trailing arguments of the three kernels that also sum
    if form != FP32:
        dm = WinoOperand(_i16(36 * t * cout_s * (1 if form == F16P else 2)), carried_amax(gc), form)
        any_sum = db is not None or dn0 is not None or dn1 is not None
        ws = scratch(L.lib().dsee_wino43_dout_f16x2_workspace(), "doutsums2") if any_sum else None
        L.call("wino43_dout_f16p" if form == F16P else "wino43_dout_f16x2", gc, dm.data, nb, h, wd, cout_s, dm.amax, DM_BOUND, ws,
               *tail)
        return dm
    dm = WinoOperand(new(36, t, cout_s), amax_slot() if _fp16_amax_needed() else None, FP32)
    if sums:
        ws = scratch(L.lib().dsee_wino43_dout_sums_workspace(cout_s), "doutsums")
        L.call("wino43_dout_sums", gc, dm.data, nb, h, wd, cout_s, dm.amax, ws, *tail)
    else:
        L.call("wino43_dout", gc, dm.data, nb, h, wd, cout_s, dm.amax)
    return dm


def _wino_wgrad_operands(xc, gc, nb, h, wd, cin_s, cout_s, mode, v=None, dm=None, sums=None, pre_dm=False):
    """(V, dM) of one image chunk for the Winograd-domain weight gradient, as WinoOperands: transposed bf16x3 in mode BF16X3_T;
    else `v` may be the V the forward pass kept and `dm` the A dY A^T its producer already wrote.  `pre_dm`: dM may leave
    its transform in the form of a pre-split `v` (when dY carries its maximum).  `sums`: see _wino_dout."""
    t = nb * (h // 4) * (wd // 4)
    if mode == WgradMode.BF16X3_T:
        vt, dmt = _i16(36 * t * cin_s * 3), _i16(36 * t * cout_s * 3)
        L.call("wino43_input_split_t", xc, vt, nb, h, wd, cin_s)
        L.call("wino43_dout_split_t", gc, dmt, nb, h, wd, cout_s)
        return WinoOperand(vt, None, BF16X3_T), WinoOperand(dmt, None, BF16X3_T)
    pre_dm = dm is None and pre_dm and carried_amax(gc) is not None
    if v is not None and v.form == F16P and not pre_dm and not (dm is not None and dm.form == F16P):
        v = None       # a packed one-term V needs a packed one-term dM (dsee_gemm_f16p_tn_pqpre): transform x again in fp32
    if v is None or (v.form == FP32 and v.amax is None and _fp16_amax_needed()):
        v = WinoOperand(new(36, t, cin_s), amax_slot() if _fp16_amax_needed() else None, FP32)
        L.call("wino43_input", xc, v.data, nb, h, wd, cin_s, v.amax)
    if dm is None:
        dm = _wino_dout(gc, nb, h, wd, cout_s, v.form if pre_dm else FP32, sums)
    return v, dm


def _adjoint_ok(k_s, r_s):
    """dV = dM x U^T on the fp32-A split GEMM: k_s = channels of dy (reduction), r_s = channels of dx."""
    return P().adjoint_dgrad and P().gemm_af32 and _split_kind(k_s, r_s) != GemmKind.FP32 and k_s * 4 * 256 < 0x7FFFFFFF


WinoBwd = namedtuple("WinoBwd", "nb mode t whole pk pre_dm u_t as_dm")


def _wino_bwd(n, nb, h, w, cin_s, cout_s, dx_s, v_form, g_amax=False, norm_c=None):
    """The backward decisions of a Winograd layer cin_s -> cout_s that runs `nb` of its n images per pass (0: it does not run), under
    the active plan: no tensors, no launches.  `dx_s`: channels of the data gradient wanted from the weight gradient's dM (adjoint
    form), 0: none; `v_form`: form of the V the forward kept; `g_amax`: the output gradient carries its maximum; `norm_c`: the layer
    is the gamma/beta convolution (ld -> rows) of a norm over norm_c channels.  -> t: tiles per pass; whole: one pass in mode AF32,
    which reads the kept V; pk: the packed one-term chain; pre_dm: dM may leave its transform in the form of a kept pre-split V; u_t:
    GemmKind of the adjoint U^T, None: dx does not come from dM; as_dm: the norm backward writes the dM all its consumers read."""
    t, mode, norm = nb * (h // 4) * (w // 4), _wgrad_mode(cin_s, cout_s), norm_c is not None
    whole = mode == WgradMode.AF32 and nb == n
    adjoint = bool(nb and dx_s and mode != WgradMode.BF16X3_T and _adjoint_ok(cout_s, dx_s))
    served = adjoint or not dx_s      # (a norm without an embedding has no dx; with one, dx must come from dM)
    # 16-bit storage mode: the forward kept a packed one-term V -> A dY A^T packed one-term too, when dY's maximum is known
    pk = bool(not norm and v_form == F16P and P().presplit_dm and whole and g_amax and t % 256 == 0 and cout_s % 32 == 0
              and (not adjoint or cin_s % 128 == 0))
    # ... pre-split when the whole chain can take it: a kept split V for the TN weight gradient, the adjoint GEMM on 256 x 256 tiles
    pre_dm = (bool(v_form in (F16X2, F16P) and mode == WgradMode.AF32 and served) if norm else
              pk or bool(P().presplit_dm and whole and _split_kind(cout_s, cin_s) == GemmKind.F16X2_AF32 and t % 256 == 0
                         and cout_s % 16 == 0 and (not adjoint or (cin_s % 256 == 0 and (36 * t // 256) * (cin_s // 256) >= 512))))
    as_dm = bool(norm and P().fuse_dm and nb == n and mode != WgradMode.BF16X3_T and served and 256 % (norm_c // 4) == 0)
    return WinoBwd(nb, mode, t, whole, pk, pre_dm, _u_kind(cout_s, dx_s, dm_form=F16P if pk else None) if adjoint else None, as_dm)


def _wino_dgrad_from_dm(dm, u_t, nb, h, wd, k_s, r_s, rows, mask=None, mask_ld=0):
    """dx [nb,h,wd,r_s] of a 3x3 convolution from the WinoOperand dm (dM [36][t][k_s] = A dY A^T): one grouped GEMM with the
    transposed forward weights u_t = (U^T [36][rows][k_s], amax, the GemmKind it was built with) and the overlap-add of B dV B^T."""
    t, (u, ua, kind) = nb * (h // 4) * (wd // 4), u_t
    assert (kind == GemmKind.F16_PACKED) == (dm.form == F16P), (kind, dm.form)
    dv = torch.empty(36, t, r_s, dtype=torch.float16, device="cuda") if kind.f16_product else new(36, t, r_s)
    dvs = amax_slot() if kind.f16_product else None
    with _timed(kind.timer, 2.0 * 36 * t * k_s * r_s, kind.gemm_bytes(t, k_s, r_s, 36, rows)):
        _wino_gemm(dm, DM_BOUND, u, ua, dv, (36 * t, r_s, k_s, t, rows), kind, dvs)
    dx = new(nb, h, wd, r_s)
    # max |dx| rides along: dx is the gradient w.r.t. a norm's output (bound of that norm's gamma/beta gradient) or, in the masked
    # form, the embedding's gradient (the dout operand of mlp_shared's weight gradient)
    tag_amax(dx, amax_slot())
    if mask is None and dvs is None and P().presplit_dm:
        L.call("wino43_input_adjoint_amax", dv, dx, nb, h, wd, r_s, dx.dsee_amax)
    elif mask is None and kind == GemmKind.F16_PACKED and P().presplit_dm:
        L.call("wino43_input_adjoint_amax_f16", dv, dx, nb, h, wd, r_s, dvs, dx.dsee_amax)
    else:
        L.call("wino43_input_adjoint", dv, mask, mask_ld, dx, nb, h, wd, r_s, dvs, dx.dsee_amax)
    return dx


def _wino_wgrad(x, g, n, h, wd, cin_s, cout_s, co, ci, v_fwd=None, w_for_dx=None, sums=None):
    """dw OIHW of conv3x3(x, w) given g = dL/dy, reduced over tiles in the Winograd domain.  `v_fwd`: the WinoOperand V of
    x kept by the forward pass (used when the weight gradient takes fp32 operands and runs in one pass).
    `w_for_dx` (the weight): also return dx, computed from the same dM in the adjoint form -> (dw, dx)."""
    with_dx = w_for_dx is not None
    bwd = _wino_bwd(n, _wino_chunk(n, h, wd, max(cin_s, cout_s)), h, wd, cin_s, cout_s, cin_s if with_dx else 0,
                    getattr(v_fwd, "form", None), carried_amax(g) is not None)
    assert not with_dx or bwd.u_t is not None
    (nb, mode, t), total = bwd[:3], None
    nbytes = L.lib().dsee_wino43_wgrad_workspace(C.c_long(t), cin_s, cout_s)
    ws = scratch(nbytes, "wgrad")
    if with_dx:
        rows_t = L.wrows(cin_s)
        u_t = (*_wino_u(w_for_dx, co, ci, 2, rows_t, L.kpad(1, 1, cout_s), bwd.u_t), bwd.u_t)
        dx = new(n, h, wd, cin_s) if nb != n else None
    for n0 in range(0, n, nb):
        gc = g if nb == n else g[n0:n0 + nb]
        v, dm = _wino_wgrad_operands(x[n0:n0 + nb], gc, nb, h, wd, cin_s, cout_s, mode, v_fwd if bwd.whole else None, sums=sums,
                                     pre_dm=bwd.pre_dm)
        dw = new(co, ci, 3, 3)
        with _timed(_wgrad_name(mode), 2.0 * 36 * t * cin_s * cout_s):
            L.call("wino43_wgrad", v.data, dm.data, ws, nbytes, dw, t, cin_s, cout_s, co, ci, _wgrad_code(v, dm, mode), v.amax,
                   dm.amax)
        total = dw if total is None else total.add_(dw)
        if with_dx:
            dxc = _wino_dgrad_from_dm(dm, u_t, nb, h, wd, cout_s, cin_s, rows_t)
            if nb == n:
                dx = dxc
            else:
                dx[n0:n0 + nb].copy_(dxc)
    return (total, dx) if with_dx else total


# ---- the convolution node: its kernel families are chosen once per layer (_conv_path); its backward is the steps below, in order
THIN3, WINO, DIRECT = "thin3", "wino", "direct"     # forward / weight gradient: thin.hip's 3 x 3 kernels | Winograd | implicit GEMM
THIN1, ADJOINT = "thin1", "adjoint"    # both gradients by one dsee_thin1x1_bwd (conv2d's thin path) | dx from the Winograd wgrad dM
S2_PARITY, DIRECT_SUMPOOL = "s2_parity", "direct_sumpool"     # data gradient: _dgrad_stride2_parity | direct + sumpool (ups)
# dgrad / wgrad: None where the gradient is not needed; keep_v: the forward keeps V of x for the weight gradient; g_amax: the
# activation backward attaches max |g|; dout_sums: bias / noise-weight gradients can ride in the weight gradient's A dY A^T pass
ConvPath = namedtuple("ConvPath", "fwd dgrad wgrad keep_v g_amax dout_sums")
# all of a Conv2d call that autograd does not differentiate (Conv2d.forward, conv2d); *_eps: the draws behind the noise weights
ConvSpec = namedtuple("ConvSpec", "stride pad ups act noise_eps res_noise_eps res_sink exact stats in_act defer_act_bwd reflect",
                      defaults=(1, 1, 0, L.ACT_NONE, None, None, None, False, False, 0, False, False))


def _conv_path(n, hi, wi, cin_s, cout_s, co, ci, kh, kw, stride, pad, ups, has_res, exact, need_dx, need_dw):
    """The ConvPath of a layer of this geometry under the active plan: no tensors, no launches.  What depends on run-time tensor
    state (a carried maximum, the form of the kept V: pre_dm / pk) is decided in the backward pass, by _wino_bwd."""
    geom = L.geom_fwd(n, hi, wi, cin_s, cout_s, kh, stride, pad, ups)
    wino = _wino_ok(n, hi, wi, cin_s, cout_s, kh, stride, pad, ups)
    thin3 = (not P().thin_gemm and kh == 3 and stride == 1 and pad == 1 and ups == 0 and co <= 4 and cin_s % 256 == 0
             and cin_s <= 1024 and wi % 64 == 0 and not has_res)
    thin1 = (P().thin_gemm and kh == 1 and kw == 1 and ups == 0 and co <= 32 and ci == cin_s and not has_res
             and geom.Ho == hi and geom.Wo == wi and cin_s >= 128)
    wino_w = wino and P().winograd_wgrad and need_dw
    bwd = _wino_bwd(n, _wino_chunk(n, hi, wi, max(cin_s, cout_s)) if wino_w else 0, hi, wi, cin_s, cout_s, cin_s, None)
    adjoint = bwd.u_t is not None      # one A dY A^T of g serves both gradients
    dgrad = (None if not need_dx else THIN1 if thin1 else ADJOINT if adjoint else WINO if wino
             else S2_PARITY if _s2_parity_ok(geom, kh, kw) else DIRECT_SUMPOOL if ups else DIRECT)
    wgrad = None if not need_dw else THIN1 if thin1 else THIN3 if thin3 else WINO if wino_w else DIRECT
    keep_v = wino and not thin3 and P().keep_v and need_dw and bwd.mode == WgradMode.AF32
    g_amax = P().presplit_dm if wino else (_direct_split_on(exact) and P().conv_amax_out)
    dout_sums = wino_w and _dout_sums_ok(n, bwd.nb, cout_s, bwd.mode)
    return ConvPath(THIN3 if thin3 else WINO if wino else DIRECT, dgrad, wgrad, bool(keep_v), bool(g_amax), bool(dout_sums))


def _act_bwd(dy, out, act, with_amax, deferred=False):
    """g = dy act'(out); `deferred`: the consumer's backward already applied act'(out) and tagged max |g| (Conv2d.forward).
    `with_amax`: max |g| is attached, the bound the kernels that read g scale or split it with."""
    if deferred or act == L.ACT_NONE:
        return dy
    g = torch.empty_like(dy)
    amax = (tag_amax(g, amax_slot()),) if with_amax else ()
    L.call("act_bwd_amax" if with_amax else "act_bwd", dy, out, g, C.c_long(dy.numel()), act, LRELU_SLOPE, *amax)
    return g


def _thin1_grads(x, w, g, geom, need_dx, need_dw, in_act):
    """(dx, dw) of the 1 x 1 layer with <= 32 outputs.  `in_act`: the producer of x = LeakyReLU(.) deferred its activation's
    backward to this kernel, which then also writes max |dx|."""
    co, ci = w.shape[0], w.shape[1]
    dx, dw = (torch.empty_like(x) if need_dx else None), (new(co, ci, 1, 1) if need_dw else None)
    ws = scratch(L.lib().dsee_thin1x1_bwd_workspace(geom.Cin, co), "wgrad") if need_dw else None
    da = tag_amax(dx, amax_slot()) if (need_dx and in_act) else None
    L.call("thin1x1_bwd", g, geom.Cout, w, x, dx, dw, C.c_long(geom.N * geom.Hi * geom.Wi), geom.Cin, co, ws, int(da is not None),
           LRELU_SLOPE, da)
    return dx, dw


def _conv_dgrad(family, x, w, g, geom, direct):
    """dx by the rotated-kernel Winograd convolution | by output parity | by the direct kernel (+ sumpool under an upsampling)"""
    if family == WINO:
        return _wino_conv(g, w, geom.N, geom.Ho, geom.Wo, geom.Cin, geom.Cout, True)
    if family == S2_PARITY:
        return _dgrad_stride2_parity(g, w, geom, w.shape[1], **direct)
    gd = L.geom_dgrad(geom)
    dx = conv_raw(g, _pack("dgrad", w, geom.Cout, gd.korder), gd, **direct)
    if family == DIRECT_SUMPOOL:
        dxl, dx = dx, torch.empty_like(x)
        L.call("sumpool", dxl, dx, geom.N, gd.Ho, gd.Wo, geom.Cin, geom.ups)
    return dx


def _conv_wgrad(family, x, w, g, geom, vkeep, sums, direct):
    co, ci, kh, kw = w.shape
    if family == WINO:
        return _wino_wgrad(x, g, geom.N, geom.Hi, geom.Wi, geom.Cin, geom.Cout, co, ci, vkeep, sums=sums)
    if family == DIRECT:
        return wgrad_raw(x, g, geom, co, ci, kh, kw, **direct)
    ws = scratch(L.lib().dsee_conv3x3_thin_wgrad_workspace(geom.Cin), "wgrad")       # THIN3
    dw = new(co, ci, 3, 3)
    L.call("conv3x3_thin_wgrad", x, g, ws, dw, geom.N, geom.Hi, geom.Wi, geom.Cin, co, ci)
    return dw


def _conv_grads(path, x, w, g, geom, vkeep, sums, in_act, direct):
    """(dx, dw) by the families of `path`, the data gradient first; `direct`: amax_cache / exact of the direct kernels"""
    if THIN1 in (path.dgrad, path.wgrad):
        return _thin1_grads(x, w, g, geom, path.dgrad == THIN1, path.wgrad == THIN1, in_act)
    if path.dgrad == ADJOINT:
        return _wino_wgrad(x, g, geom.N, geom.Hi, geom.Wi, geom.Cin, geom.Cout, *w.shape[:2], vkeep, w_for_dx=w, sums=sums)[::-1]
    dx = _conv_dgrad(path.dgrad, x, w, g, geom, direct) if path.dgrad else None
    dw = _conv_wgrad(path.wgrad, x, w, g, geom, vkeep, sums, direct) if path.wgrad else None
    return dx, dw


def _reflect_border_grads(x, w, g, dx, dw, geom):
    """The border terms of the reflection padding, added in place to what the zero-padded paths produced."""
    dims = (geom.N, geom.Hi, geom.Wi, w.shape[1], geom.Cin, w.shape[0], geom.Cout)
    if dx is not None:
        L.call("reflect_ring_dgrad", g, w, dx, *dims)
        dx.dsee_amax = None
    if dw is not None:
        nbytes = L.lib().dsee_reflect_ring_wgrad_workspace(geom.N, geom.Hi, geom.Wi, w.shape[1], w.shape[0])
        L.call("reflect_ring_wgrad", x, g, scratch(nbytes, "ringw"), C.c_size_t(nbytes), dw, *dims)


def _noise_wgrad(g, eps):
    """gradient [C] of a NoiseInjection weight: sum over pixels of g x the regenerated draw `eps` (a PhiloxNormal)"""
    cn = g.shape[-1]
    m, d = g.numel() // cn, new(cn)
    L.call("channel_dot_rng", g, d, m, cn, scratch(L.lib().dsee_channel_dot_workspace(m, cn), "chdot"), eps.seed, eps.offset)
    return d


def _conv_side_grads(g, co, want, sums, res_sink):
    """(db, dres, dnw, drnw) of the entries of `want` (_wino_dout's, + "res").  Bias and noise weights: what the A dY A^T pass left
    in `sums`, else channel_dot / channel_dot_rng passes over g; the residual's is g itself, returned or put into the GradSink."""
    if want["res"] and res_sink is not None:
        res_sink.put(g)      # picked up as the `add` operand of the norm backward that also feeds on `res`
    dres = g if (want["res"] and res_sink is None) else None
    if sums is not None:
        return (sums["dbias"][:co] if want["bias"] else None), dres, sums["dn0"], sums["dn1"]
    db = channel_dot(g, None, co).clone() if want["bias"] else None
    return db, dres, *(None if eps is None else _noise_wgrad(g, eps) for eps in (want["n0"], want["n1"]))


IN_X, IN_W, IN_BIAS, IN_RES, IN_NOISE_W, IN_RES_NOISE_W, IN_SPEC = range(7)     # Conv2d.apply's inputs in needs_input_grad


class Conv2d(torch.autograd.Function):
    """out = act(conv(x, w) + bias + residual); x stored [N,H,W,pad4(Cin)], w OIHW (real channel counts)."""

    @staticmethod
    def forward(ctx, x, w, bias, res, noise_w, res_noise_w, spec):
        """The fields of `spec` (ConvSpec) -- `reflect`: the padding is nn.ReflectionPad2d(1) instead of zeros (3 x 3, stride 1, no
        epilogue but the bias): the zero-padded layer runs as always and dsee_reflect_ring_* add the border terms in place, here and
        in backward.  `exact`: keep a direct convolution on the fp32 MFMA (no operand-maximum passes over its input).
        `defer_act_bwd` / `in_act` are the two halves of ONE contract set up by the caller (networks.DeepSEESR.forward): this
        layer's output y = LeakyReLU(.) has exactly one consumer, a convolution called with `in_act = ACT_LRELU`, whose backward
        multiplies the gradient it hands back by LeakyReLU'(y) (inside its data-gradient kernel where it can) and attaches its
        maximum; this layer's backward then skips its own pass over (dy, y) -> g."""
        ctx.plan, ctx.spec = P(), spec
        stride, pad, ups, act = spec[:4]
        assert spec.in_act in (0, L.ACT_LRELU) and (not spec.defer_act_bwd or act == L.ACT_LRELU)
        _bind_rng(spec.noise_eps, spec.res_noise_eps)
        (n, hi, wi, cin_s), (co, ci, kh, kw) = x.shape, w.shape
        assert cin_s == L.pad4(ci), (cin_s, ci)
        cout_s = L.pad4(co)
        geom = L.geom_fwd(n, hi, wi, cin_s, cout_s, kh, stride, pad, ups)
        path = _conv_path(n, hi, wi, cin_s, cout_s, co, ci, kh, kw, stride, pad, ups, res is not None, spec.exact,
                          ctx.needs_input_grad[IN_X], ctx.needs_input_grad[IN_W])
        ctx.w_amax, ctx.w_u = getattr(w, "dsee_amax", None), getattr(w, "dsee_u", None)   # carried by a spectral-norm group launch
        w = w.contiguous()
        w.dsee_amax, w.dsee_u = ctx.w_amax, ctx.w_u
        vkeep, ctx.amax_cache = None, None
        if path.fwd == THIN3:
            out = new(n, hi, wi, cout_s)
            L.call("conv3x3_thin_fwd", x, w, bias, out, n, hi, wi, cin_s, co, act, LRELU_SLOPE)
        elif path.fwd == WINO:
            keep = [] if path.keep_v else None
            # bench.py: the whole layer (input transform + GEMMs + output transform) on its algorithmic bytes (x in, y out)
            # and its Winograd-domain FLOPs (2.25 multiplies per output and channel pair instead of 9)
            with _timed("conv_forward@%dx%d %d->%d" % (hi, wi, cin_s, cout_s), 2.0 * 36 * (n * hi * wi // 16) * cin_s * cout_s,
                        4.0 * n * hi * wi * (cin_s + cout_s)):
                out = _wino_conv(x, w, n, hi, wi, cin_s, cout_s, False, pad_vec(bias, cout_s), res, act, keep=keep,
                                 noise=None if noise_w is None else (noise_w, spec.noise_eps),
                                 res_noise=None if res_noise_w is None else (res_noise_w, spec.res_noise_eps), stats=spec.stats)
            vkeep = keep[0] if keep else None
        else:
            ctx.amax_cache = {}   # max |x| found here is reused by the weight gradient
            out = conv_raw(x, _pack("fwd", w, cin_s, geom.korder), geom, pad_vec(bias, cout_s), res, act,
                           amax_cache=ctx.amax_cache, exact=spec.exact)
        assert noise_w is None or (path.fwd == WINO and act == L.ACT_NONE and isinstance(spec.noise_eps, PhiloxNormal))
        assert res_noise_w is None or (path.fwd == WINO and res is not None and isinstance(spec.res_noise_eps, PhiloxNormal))
        ctx.geom, ctx.path, ctx.has_bias, ctx.has_res = geom, path, bias is not None, res is not None
        ctx.noise = spec.noise_eps if noise_w is not None else None
        ctx.res_noise = spec.res_noise_eps if res_noise_w is not None else None
        if spec.reflect:
            assert ((kh, kw, stride, pad, ups) == (3, 3, 1, 1, 0) and path.fwd != THIN3 and act == L.ACT_NONE and res is None
                    and noise_w is None and res_noise_w is None and not spec.stats and not spec.in_act), "reflect: plain 3 x 3"
            L.call("reflect_ring_fwd", x, w, out, n, hi, wi, ci, cin_s, co, cout_s)
            out.dsee_amax = None      # (a bound its producer measured no longer holds on the border)
        save_with_operand(ctx, vkeep, x, w, out if act != L.ACT_NONE else None)
        return out

    @staticmethod
    @_under_plan
    def backward(ctx, dy):
        (x, w, out), vkeep = saved_with_operand(ctx)
        w.dsee_amax, w.dsee_u = ctx.w_amax, ctx.w_u
        _bind_rng(ctx.noise, ctx.res_noise)
        spec, path, geom, need = ctx.spec, ctx.path, ctx.geom, ctx.needs_input_grad
        g = _act_bwd(dy.contiguous(), out, spec.act, path.g_amax, spec.defer_act_bwd)
        want = {"bias": bool(ctx.has_bias and need[IN_BIAS]), "res": bool(ctx.has_res and need[IN_RES]),
                "n0": ctx.noise if need[IN_NOISE_W] else None, "n1": ctx.res_noise if need[IN_RES_NOISE_W] else None}
        sums = want if (path.dout_sums and (want["bias"] or want["n0"] is not None or want["n1"] is not None)) else None
        dx, dw = _conv_grads(path, x, w, g, geom, vkeep, sums, spec.in_act, dict(amax_cache=ctx.amax_cache, exact=spec.exact))
        if spec.reflect:
            _reflect_border_grads(x, w, g, dx, dw, geom)
        db, dres, dnw, drnw = _conv_side_grads(g, w.shape[0], want, sums, spec.res_sink)
        if spec.in_act and dx is not None and path.dgrad != THIN1:
            dx = _act_bwd(dx.contiguous(), x, spec.in_act, True)    # the LeakyReLU backward x's producer deferred, as a pass
        return dx, dw, db, dres, dnw, drnw, None


class GradSink:
    """One-slot mailbox between two autograd nodes of a resblock: the convolution that consumes `x` as its residual puts
    the residual's gradient here instead of returning it, and the backward of the normalisation that ALSO consumes `x`
    (it runs later: its own incoming gradient depends on that convolution's data gradient) adds it to its dx in the
    same pass -- the autograd engine's separate fan-in addition (3 full-tensor passes) never runs.

    A sink lives for ONE forward/backward pair (the resblock creates a new one per forward) and only full backward passes
    are supported: a partial backward that runs the convolution's node but not the norm's (torch.autograd.grad with
    `inputs=` restricted to the convolution's weight) would drop the shortcut gradient -- `put` refuses a second gradient
    instead of silently overwriting the first."""

    def __init__(self):
        self.g = None

    def put(self, g):
        if self.g is not None:
            raise RuntimeError("GradSink holds a gradient nobody took: the previous backward pass did not reach the "
                               "normalisation that consumes it (partial backward passes are not supported)")
        self.g = g

    def take(self):
        g, self.g = self.g, None
        return g


def _fusable_noise(x, w, stride, pad, ups, eps):
    n, hi, wi, cin_s = x.shape
    return (P().fuse_noise and isinstance(eps, PhiloxNormal) and w.shape[2] == 3 and w.shape[0] > 4
            and _wino_ok(n, hi, wi, cin_s, L.pad4(w.shape[0]), 3, stride, pad, ups))


class ThinGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, bias, co, act, kh=3, kw=3, pad=1):
        n, h, w, ldz = z.shape
        ho, wo = h + 2 * pad - kh + 1, w + 2 * pad - kw + 1
        out = new(n, ho, wo, 4)
        if (kh, kw, pad) == (3, 3, 1):
            L.call("thin_gather_fwd", z, bias, out, n, h, w, ldz, co, act, LRELU_SLOPE)
        else:
            L.call("thin_gather_k_fwd", z, bias, out, n, h, w, ldz, co, kh, kw, pad, act, LRELU_SLOPE)
        ctx.save_for_backward(out)
        ctx.meta = (co, act, ldz, bias is not None, kh, kw, pad, h, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        co, act, ldz, has_bias, kh, kw, pad, h, w = ctx.meta
        n = out.shape[0]
        dout = dout.contiguous()
        dz = new(n, h, w, ldz)
        if (kh, kw, pad) == (3, 3, 1):
            L.call("thin_gather_bwd", dout, out, dz, n, h, w, ldz, co, act, LRELU_SLOPE)
        else:
            L.call("thin_gather_k_bwd", dout, out, dz, n, h, w, ldz, co, kh, kw, pad, act, LRELU_SLOPE)
        db = None
        if has_bias and ctx.needs_input_grad[1]:
            g = torch.empty_like(dout)
            L.call("act_bwd", dout, out, g, C.c_long(dout.numel()), act, LRELU_SLOPE)
            db = channel_dot(g, None, co).clone()
        return dz, db, None, None, None, None, None


def _thin_ok(x, w, res, stride, pad, ups, noise, res_noise):
    """Layers with <= 4 output channels as a (KH KW Cout)-output 1x1 GEMM + a gather: the to-RGB layer (3 x 3, padding 1) and --
    round 6 -- the discriminator's last layer (4 x 4, padding 2: 16 outputs, within dsee_thin1x1_bwd's 32 rows)."""
    co, ci, kh, kw = w.shape
    shape_ok = (kh, kw, pad) == (3, 3, 1) or ((kh, kw, pad) == (4, 4, 2) and co * 16 <= 32)
    return (P().thin_gemm and shape_ok and stride == 1 and ups == 0 and co <= 4 and res is None
            and noise is None and res_noise is None and x.shape[3] >= 128 and x.shape[3] % 32 == 0)


def conv2d(x, w, bias=None, res=None, stride=1, pad=1, ups=0, act=L.ACT_NONE, noise=None, res_noise=None, res_sink=None,
           stats=False, in_act=0, defer_act_bwd=False, reflect=False):
    """`noise` = (noise_w, eps): the NoiseInjection that follows the conv; `res_noise` = (noise_w, eps): the
    NoiseInjection on the residual (the shortcut x_s = noise_skip(x)).  PhiloxNormal draws on a Winograd layer ride in
    the output transform; anything else (a replayed tensor, a non-Winograd layer) runs as its own UpNoise pass.
    `res_sink` (GradSink): the residual's gradient is handed to the norm backward instead of the autograd engine.
    `stats`: the output feeds a training-mode BatchNorm -- a Winograd layer then writes the statistics rows in its output
    transform (bn_stats finds them on the tensor).
    `in_act` / `defer_act_bwd` (x is the LeakyReLU output of a layer called with defer_act_bwd), `reflect`: see Conv2d.forward."""
    in_act = int(in_act or 0) if (torch.is_grad_enabled() and x.requires_grad) else 0
    if reflect:
        assert noise is None and res_noise is None and res is None and act == L.ACT_NONE
        return Conv2d.apply(x, w, bias, None, None, None, ConvSpec(stride=stride, pad=pad, ups=ups, act=act, reflect=True))
    if _thin_ok(x, w, res, stride, pad, ups, noise, res_noise):
        co, ci, kh, kw = w.shape
        w27 = w.permute(2, 3, 0, 1).reshape(kh * kw * co, ci, 1, 1)    # row tap*co_n + co (55 KB of parameter glue)
        z = Conv2d.apply(x, w27, None, None, None, None, ConvSpec(stride=1, pad=0, exact=True, in_act=in_act))
        return ThinGather.apply(z, bias, co, act, kh, kw, pad)
    if res_noise is not None and not _fusable_noise(x, w, stride, pad, ups, res_noise[1]):
        # (the shortcut's own node must see its gradient: no sink)
        res, res_noise, res_sink = UpNoise.apply(res, res_noise[0], res_noise[1], 0), None, None
    rn = (None, None) if res_noise is None else res_noise
    spec = ConvSpec(stride=stride, pad=pad, ups=ups, act=act, res_noise_eps=rn[1], res_sink=res_sink, in_act=in_act)
    if noise is None or (_fusable_noise(x, w, stride, pad, ups, noise[1]) and act == L.ACT_NONE):
        nz = (None, None) if noise is None else noise
        spec = spec._replace(noise_eps=nz[1], stats=bool(stats), defer_act_bwd=bool(defer_act_bwd))
        return Conv2d.apply(x, w, bias, res, nz[0], rn[0], spec)
    assert not defer_act_bwd
    return UpNoise.apply(Conv2d.apply(x, w, bias, res, None, rn[0], spec), noise[0], noise[1], 0)


# ------------------------------------------------------------------------------------ spectral norm
class SpectralNorm(torch.autograd.Function):
    """W = W_orig / sigma with one in-place power iteration on (u, v) when `power_iter`
    (torch.nn.utils.spectral_norm hook semantics; SURVEY B-2)."""

    @staticmethod
    def forward(ctx, w_orig, u, v, power_iter):
        r = w_orig.shape[0]
        k = w_orig.numel() // r
        w_orig = w_orig.contiguous()
        sigma = new(1)
        w_sn = torch.empty_like(w_orig)
        L.call("spectral_norm_fwd", w_orig, u, v, sigma, w_sn, r, k, int(power_iter), SN_EPS, scratch((r + k) * 4, "sn"))
        ctx.save_for_backward(w_sn, u.clone(), v.clone(), sigma)
        return w_sn

    @staticmethod
    def backward(ctx, dw):
        w_sn, u, v, sigma = ctx.saved_tensors
        r = w_sn.shape[0]
        k = w_sn.numel() // r
        dwo = torch.empty_like(w_sn)
        L.call("spectral_norm_bwd", dw.contiguous(), w_sn, u, v, sigma, dwo, r, k, scratch(1024, "sn"))
        return dwo, None, None, None


class _SpectralNormPre(torch.autograd.Function):
    """Autograd node of ONE layer of a spectral-norm group: the forward value was computed by the group launch
    (spectral_norm_group), the backward is the per-layer dW_orig = (dW - <dW, W> u v^T) / sigma."""

    @staticmethod
    def forward(ctx, w_orig, w_sn, u, v, sigma):
        ctx.save_for_backward(w_sn, u, v, sigma)
        return w_sn.view_as(w_orig)

    @staticmethod
    def backward(ctx, dw):
        w_sn, u, v, sigma = ctx.saved_tensors
        r = u.numel()
        k = v.numel()
        dwo = torch.empty_like(dw, memory_format=torch.contiguous_format)
        L.call("spectral_norm_bwd", dw.contiguous(), w_sn, u, v, sigma, dwo, r, k, scratch(1024, "sn"))
        return dwo, None, None, None, None


_SN_DT = None


class SNGroup:
    """The spectral-normalised layers one network uses in a forward pass, with the device-resident tables of
    dsee_spectral_norm_group_fwd (built once; rebuilt if a parameter or buffer moved)."""

    def __init__(self, layers):
        self.layers = list(layers)
        self.key = None

    def _build(self):
        import numpy as np
        global _SN_DT
        if _SN_DT is None:
            _SN_DT = np.dtype([("w", "<u8"), ("u", "<u8"), ("v", "<u8"), ("out_off", "<i8"), ("saved_off", "<i8"),
                               ("R", "<i4"), ("K", "<i4"), ("scratch_off", "<i4"), ("pad", "<i4")])
        desc = np.zeros(len(self.layers), dtype=_SN_DT)
        wk, wr, we = [], [], []
        out_off = saved_off = sc_off = 0
        self.slices = []
        for i, m in enumerate(self.layers):
            w = m.weight_orig
            r = w.shape[0]
            k = w.numel() // r
            assert w.is_contiguous() and m.weight_u.numel() == r and m.weight_v.numel() == k
            desc[i] = (w.data_ptr(), m.weight_u.data_ptr(), m.weight_v.data_ptr(), out_off, saved_off, r, k, sc_off, 0)
            wk += [(i, j) for j in range((k + 31) // 32)]
            wr += [(i, j) for j in range(r)]
            we += [(i, j) for j in range((r * k + 4095) // 4096)]
            self.slices.append((out_off, r * k, saved_off, r, k))
            out_off += (r * k + 3) // 4 * 4
            saved_off += (r + k + 3) // 4 * 4
            sc_off += r + k
        dev = self.layers[0].weight_orig.device
        self.desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        self.wk, self.wr, self.we = (torch.tensor(t, dtype=torch.int32, device=dev).reshape(-1) for t in (wk, wr, we))
        self.n = (len(wk), len(wr), len(we))
        self.out_total, self.saved_total, self.scratch_total = out_off, saved_off, sc_off
        self.key = tuple(int(v) for d in desc for v in (d["w"], d["u"], d["v"]))

    def run(self, power_iter):
        key = tuple(p for m in self.layers for p in (m.weight_orig.data_ptr(), m.weight_u.data_ptr(), m.weight_v.data_ptr()))
        if key != self.key:
            self._build()
        nl = len(self.layers)
        out, saved, sigma = new(self.out_total), new(self.saved_total), new(nl)
        amax = torch.zeros(nl, AMAX_FLOATS, dtype=torch.float32, device=out.device)
        with torch.no_grad():
            L.call("spectral_norm_group_fwd", self.desc, nl, self.wk, self.n[0], self.wr, self.n[1], self.we, self.n[2],
                   int(bool(power_iter)), SN_EPS, scratch(self.scratch_total * 4, "sng"), sigma, out, saved, amax)
        for i, (m, (oo, n, so, r, k)) in enumerate(zip(self.layers, self.slices)):
            w = _SpectralNormPre.apply(m.weight_orig, out[oo:oo + n], saved[so:so + r], saved[so + r:so + r + k],
                                       sigma[i:i + 1])
            w.dsee_amax = amax[i]           # max |W_sn| (64-line form): no stand-alone absmax pass over the weight
            m._pre = w
        self.last = (out, amax)

    def wino_weights(self, with_adjoint):
        """Winograd-domain weights U = G g G^T of ALL layers of the group in one launch (forward form; with the adjoint
        form for the backward pass in a second one) when the layers are equally shaped 3x3 convolutions on the fp16x2 split
        path; attached to the normalised weights so that ops._wino_u finds them."""
        w0 = self.layers[0].weight_orig
        co, ci = w0.shape[0], w0.shape[1]
        same = all(tuple(m.weight_orig.shape) == tuple(w0.shape) for m in self.layers) and tuple(w0.shape[2:]) == (3, 3)
        if not (same and P().winograd and P().gemm_split and P().gemm_f16x2 and P().gemm_af32 and co % 128 == 0 and ci % 128 == 0):
            return
        out, amax = self.last
        nl = len(self.layers)
        stride = self.slices[1][0] - self.slices[0][0] if nl > 1 else co * ci * 9
        kind = _u_kind(ci, co, f16_only=True)              # (16-bit storage mode: packed one-term weights)
        for flip in ((0, 2) if with_adjoint else (0,)):
            r_s, k_s = (ci, co) if flip else (co, ci)
            rows, kp = L.wrows(r_s), L.kpad(1, 1, k_s)
            per = 36 * rows * kp * kind.words     # int16 elements per layer (one / two fp16 terms)
            u = _i16(nl * per)
            with torch.no_grad():
                L.call("wino43_weights_batch", out, u, nl, stride, per // 2, co, ci, flip, int(kind), amax)
            for i, m in enumerate(self.layers):
                d = getattr(m._pre, "dsee_u", None) or {}
                d[_u_key(flip, kind, rows, kp)] = (u[i * per:(i + 1) * per], amax[i])
                m._pre.dsee_u = d


# ------------------------------------------------------------------------------------ instance norm + act
class InstNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        n, h, w, c = x.shape
        mean, invstd = new(n, c), new(n, c)
        ws = scratch(L.lib().dsee_norm_workspace(n, h * w, c, n), "norm")
        L.call("norm_stats", x, n, h * w, c, n, BN_EPS, 0.0, mean, invstd, None, None, ws)
        y = torch.empty_like(x)
        ao = amax_slot() if (_direct_split_on() and P().conv_amax_out) else None    # (max |y| for the direct layer that reads y)
        L.call("norm_act_fwd_amax", x, mean, invstd, y, n, h * w, c, n, act, LRELU_SLOPE, ao)
        if ao is not None:
            tag_amax(y, ao)
        ctx.act, ctx.emit_amax = act, ao is not None
        ctx.save_for_backward(x, y, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, invstd = ctx.saved_tensors
        n, h, w, c = x.shape
        dx = torch.empty_like(x)
        ws = scratch(L.lib().dsee_norm_workspace(n, h * w, c, n), "norm")
        ao = amax_slot() if ctx.emit_amax else None    # (max |dx|: dx is a direct layer's output gradient; decided in forward --
        #                                                 the engine's thread has no plan of its own)
        L.call("norm_act_bwd_amax", dy.contiguous(), y, x, mean, invstd, dx, n, h * w, c, n, ctx.act, LRELU_SLOPE, ws, ao)
        if ao is not None:
            tag_amax(dx, ao)
        return dx, None


class InstNormRes(torch.autograd.Function):
    """act(res + InstanceNorm(x)): the closing `x + conv_block(x)` of the pix2pixHD ResnetBlock (ablation.py:26-29) in the norm's own
    pass (dsee_norm_act_res_fwd).  Backward: the IN backward on the saved output; the residual's gradient is g = dy act'(y) itself
    and goes back through the autograd engine (its fan-in add with the gradient of the block's first convolution: DESIGN 3.17)."""

    @staticmethod
    def forward(ctx, x, res, act):
        n, h, w, c = x.shape
        assert res.shape == x.shape
        mean, invstd = new(n, c), new(n, c)
        ws = scratch(L.lib().dsee_norm_workspace(n, h * w, c, n), "norm")
        L.call("norm_stats", x, n, h * w, c, n, BN_EPS, 0.0, mean, invstd, None, None, ws)
        y = torch.empty_like(x)
        L.call("norm_act_res_fwd", x, mean, invstd, res.contiguous(), y, n, h * w, c, n, act, LRELU_SLOPE, None)
        ctx.act = act
        ctx.save_for_backward(x, y, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, invstd = ctx.saved_tensors
        n, h, w, c = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        ws = scratch(L.lib().dsee_norm_workspace(n, h * w, c, n), "norm")
        L.call("norm_act_bwd_amax", dy, y, x, mean, invstd, dx, n, h * w, c, n, ctx.act, LRELU_SLOPE, ws, None)
        dres = None
        if ctx.needs_input_grad[1]:
            dres = dy
            if ctx.act != L.ACT_NONE:
                dres = torch.empty_like(dy)
                L.call("act_bwd", dy, y, dres, C.c_long(dy.numel()), ctx.act, LRELU_SLOPE)
        return dx, dres, None


class BatchNormAct(torch.autograd.Function):
    """act(BatchNorm2d(affine=True)(x)) of the discriminator and the style encoders (opt.norm_D / opt.norm_E = spectralbatch,
    spectralsync_batch; normalization.py:19-56): batch statistics and a running-statistics update in training (bn_stats: sync-
    free per shard, or merged over the ranks under opt.sync_bn), the running statistics in eval.  `counter`: the layer's
    num_batches_tracked, incremented on the device in every training forward (nn.BatchNorm2d; None for SynchronizedBatchNorm2d,
    whose single-device branch goes through F.batch_norm and leaves it at 0)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, counter, training, act):
        n, h, w, c = x.shape
        mean, invstd, cfg = bn_stats(x, running_mean, running_var, training)
        if training and counter is not None:
            L.call("counter_inc", counter)
        y = torch.empty_like(x)
        ao = amax_slot() if (_direct_split_on() and P().conv_amax_out) else None    # (max |y| for the direct layer that reads y)
        L.call("bn_act_fwd", x, mean, invstd, gamma, beta, y, n, h * w, c, act, LRELU_SLOPE, ao)
        if ao is not None:
            tag_amax(y, ao)
        ctx.act, ctx.emit_amax, ctx.cfg, ctx.training = act, ao is not None, cfg, training
        ctx.save_for_backward(x, y, mean, invstd, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        assert ctx.training, "BatchNormAct: backward of an eval-mode forward"
        x, y, mean, invstd, gamma = ctx.saved_tensors
        n, h, w, c = x.shape
        dy = dy.contiguous()
        sums = new(2, c)
        ws = scratch(L.lib().dsee_norm_workspace(n, h * w, c, 1), "norm")
        L.call("bn_act_bwd_reduce", dy, y, x, mean, invstd, n, h * w, c, ctx.act, LRELU_SLOPE, sums, ws)
        count, local, cfg = n * h * w, None, ctx.cfg
        if cfg is not None:        # SyncBN: the two sums over the global batch; the parameter gradients stay rank-local
            from . import parallel
            local = sums.clone()
            parallel.allreduce_sums(sums, cfg.world, cfg.group)
            count *= cfg.world
        dgamma = new(c) if ctx.needs_input_grad[1] else None
        dbeta = new(c) if ctx.needs_input_grad[2] else None
        dx = torch.empty_like(x)
        ao = amax_slot() if ctx.emit_amax else None    # (max |dx|: dx is a direct layer's output gradient)
        L.call("bn_act_bwd_apply", dy, y, x, mean, invstd, gamma, sums, local, 1.0 / count, dx, dgamma, dbeta, n, h * w, c,
               ctx.act, LRELU_SLOPE, ao)
        if ao is not None:
            tag_amax(dx, ao)
        return dx, dgamma, dbeta, None, None, None, None, None


class Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        y = torch.empty_like(x)
        L.call("act_fwd", x, y, C.c_long(x.numel()), act, LRELU_SLOPE)
        ctx.act = act
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        L.call("act_bwd", dy.contiguous(), y, dx, C.c_long(y.numel()), ctx.act, LRELU_SLOPE)
        return dx, None


# ------------------------------------------------------------------------------------ upsample + noise
class UpNoise(torch.autograd.Function):
    """y = nearest_up(x, 2^ups) + w[c] * eps   (eps/w may be None)."""

    @staticmethod
    def forward(ctx, x, noise_w, eps, ups, stats=False):
        """`stats`: y feeds a training-mode BatchNorm: its statistics rows are written in the same pass."""
        ctx.plan = P()
        n, h0, w0, c = x.shape
        y = new(n, h0 << ups, w0 << ups, c)
        ctx.philox = eps if isinstance(eps, PhiloxNormal) else None
        _bind_rng(eps)
        if ctx.philox is not None:
            assert eps.shape == tuple(y.shape)
            if stats and P().producer_stats and _stats_rows_ok(c):
                rows = L.lib().dsee_stats_part_rows(C.c_long(y.numel() // 4))
                part = new(rows, 3, c)
                L.call("upsample_noise_rng_fwd_stats", x, noise_w, y, n, h0 << ups, w0 << ups, c, ups, C.c_uint64(eps.seed),
                       C.c_uint64(eps.offset), part)
                y.dsee_stats_rows = (part, rows)
            else:
                L.call("upsample_noise_rng_fwd", x, noise_w, y, n, h0 << ups, w0 << ups, c, ups, C.c_uint64(eps.seed),
                       C.c_uint64(eps.offset))
            eps = None
        else:
            L.call("upsample_noise_fwd", x, eps, noise_w if eps is not None else None, y, n, h0 << ups, w0 << ups, c, ups)
        ctx.ups = ups
        ctx.save_for_backward(eps)
        ctx.xshape = x.shape
        return y

    @staticmethod
    @_under_plan
    def backward(ctx, dy):
        (eps,) = ctx.saved_tensors
        _bind_rng(ctx.philox)
        dy = dy.contiguous()
        n, h, w, c = dy.shape
        dx = dw = None
        if (ctx.ups and ctx.philox is not None and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and P().fuse_noise
                and 256 % (c // 4) == 0):
            # one pass over dy for both gradients (dsee_sumpool_dot_rng)
            dx, dw = new(*ctx.xshape), new(c)
            tag_amax(dx, amax_slot())      # (dx is the output gradient of the previous block's conv_1)
            ws = scratch(L.lib().dsee_sumpool_dot_rng_workspace(n, h, w, c, ctx.ups), "chdot")
            L.call("sumpool_dot_rng", dy, dx, n, h, w, c, ctx.ups, dx.dsee_amax, dw, ws, C.c_uint64(ctx.philox.seed),
                   C.c_uint64(ctx.philox.offset))
            return dx, dw, None, None, None
        if ctx.needs_input_grad[0]:
            if ctx.ups:
                dx = new(*ctx.xshape)
                tag_amax(dx, amax_slot())      # (dx is the output gradient of the previous block's conv_1)
                L.call("sumpool_amax", dy, dx, n, h, w, c, ctx.ups, dx.dsee_amax)
            else:
                dx = dy
        if ctx.philox is not None and ctx.needs_input_grad[1]:
            dw = _noise_wgrad(dy, ctx.philox)
        elif eps is not None and ctx.needs_input_grad[1]:
            dw = channel_dot(dy, eps, c).clone()
        return dx, dw, None, None, None


# ------------------------------------------------------------------------------------ SPADE/SEAN inputs
class SeanInput(torch.autograd.Function):
    """cat([ReLU(conv3x3(one-hot label; W_sh) + b_sh), style[label]]) at resolution H>>shift, from the uint8
    label map (normalization.py:174-185).  `style` None -> SPADE (128 channels only)."""

    @staticmethod
    def forward(ctx, w_sh, b_sh, style, labels, shift, want_actv, want_style):
        n, h, w, nc = labels.n, labels.h, labels.w, labels.nc
        r, rw = h >> shift, w >> shift
        ld = (NHIDDEN if want_actv else 0) + (style.shape[2] if want_style else 0)
        cat = new(n, r, rw, ld)
        coff = 0
        if want_actv:
            table = new(9, nc, NHIDDEN)
            L.call("onehot_conv3x3_pack", w_sh.contiguous(), table, NHIDDEN, nc)
            L.call("onehot_conv3x3_fwd", labels.t, table, b_sh, cat, n, h, w, shift, nc, NHIDDEN, ld, 0, 1, -1, None, 0.0)
            coff = NHIDDEN
        if want_style:
            L.call("label_gather", labels.t, style.contiguous(), cat, n, h, w, shift, nc, style.shape[2], ld, coff, 1.0)
        ctx.labels, ctx.shift, ctx.want_actv, ctx.want_style, ctx.coff = labels, shift, want_actv, want_style, coff
        ctx.sshape = style.shape if want_style else None
        ctx.save_for_backward(cat)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        (cat,) = ctx.saved_tensors
        lab, shift = ctx.labels, ctx.shift
        dcat = dcat.contiguous()
        n, r, rw, ld = cat.shape
        dw = db = dstyle = None
        if ctx.want_actv and ctx.needs_input_grad[0]:
            dw, db = new(NHIDDEN, lab.nc, 3, 3), new(NHIDDEN)
            ws = scratch(L.lib().dsee_onehot_conv3x3_wgrad_workspace(n, lab.h, lab.w, shift, lab.nc), "ohw")
            L.call("onehot_conv3x3_wgrad", lab.t, dcat, ld, cat, ld, n, lab.h, lab.w, shift, lab.nc, dw, db, ws)
        if ctx.want_style and ctx.needs_input_grad[2]:
            s = ctx.sshape[2]
            dstyle = new(*ctx.sshape)
            ws = scratch(L.lib().dsee_label_segsum_workspace(n, lab.h, lab.w, shift, lab.nc, s), "seg")
            L.call("label_segsum", lab.t, dcat, ld, ctx.coff, dstyle, n, lab.h, lab.w, shift, lab.nc, s, 1.0, ws)
        return dw, db, dstyle, None, None, None, None


def _field_args(field, shape):
    """(tensor or None, seed, offset, use_epoch) of a noise field given as a device tensor [N,H,W] or a PhiloxField."""
    if isinstance(field, PhiloxField):
        assert field.shape == tuple(shape), "field %s for a label map %s" % (field.shape, tuple(shape))
        field.bind()
        return None, field.seed, field.offset, int(field.use_epoch)
    assert isinstance(field, torch.Tensor) and field.is_cuda and field.dtype == torch.float32 \
        and tuple(field.shape) == tuple(shape), "field: a float32 device tensor %s or a PhiloxField" % (tuple(shape),)
    return field.contiguous(), 0, 0, 0


class OnehotNoiseConv3x3(torch.autograd.Function):
    """conv3x3(randn(N, nc, H, W) * one-hot(labels), weight) + bias -> NHWC [N,H,W,Co]: the first layer of FullStyleEncoder
    under opt.random_style_matrix (encoder.py:116-120) as a 9-tap gather-sum over the label map with one noise scalar per
    pixel (`field`: a device tensor [N,H,W] or a PhiloxField).  No data gradient (the input is noise): backward returns the
    gradients of weight and bias only."""

    @staticmethod
    def forward(ctx, labels, field, weight, bias):
        n, h, w, nc = labels.n, labels.h, labels.w, labels.nc
        co = weight.shape[0]
        assert tuple(weight.shape) == (co, nc, 3, 3), "weight %s for %d classes" % (tuple(weight.shape), nc)
        f, seed, offset, use_epoch = _field_args(field, (n, h, w))
        table = new(9, nc, co)
        L.call("onehot_conv3x3_pack", weight.contiguous(), table, co, nc)
        out = new(n, h, w, co)
        L.call("onehot_noise_conv3x3_fwd", labels.t, f, C.c_uint64(seed), C.c_uint64(offset), use_epoch, table, bias, out,
               n, h, w, nc, co)
        out.dsee_layout = "nhwc"
        ctx.labels, ctx.field, ctx.co, ctx.has_bias = labels, field, co, bias is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        lab, co = ctx.labels, ctx.co
        n, h, w, nc = lab.n, lab.h, lab.w, lab.nc
        f, seed, offset, use_epoch = _field_args(ctx.field, (n, h, w))
        dw = new(co, nc, 3, 3)
        db = new(co) if ctx.has_bias else None
        ws = scratch(L.lib().dsee_onehot_noise_conv3x3_wgrad_workspace(n, h, w, nc, co), "ohn")
        L.call("onehot_noise_conv3x3_wgrad", lab.t, f, C.c_uint64(seed), C.c_uint64(offset), use_epoch, dout.contiguous(),
               n, h, w, nc, co, dw, db, ws)
        return None, None, dw, db


def onehot_noise_conv3x3(labels, field_or_stream, weight, bias=None):
    return OnehotNoiseConv3x3.apply(labels, field_or_stream, weight, bias)


class StylePool(torch.autograd.Function):
    """S[b,r,c] = (1/HW) sum_{hw: label=r} f[b,h,w,c]   (encoder.py:36-49; SURVEY B-4)."""

    @staticmethod
    def forward(ctx, feat, labels, shift):
        n, hf, wf, c = feat.shape
        assert hf == labels.h >> shift and wf == labels.w >> shift, "feature map %d x %d vs labels %d x %d >> %d" % (
            hf, wf, labels.h, labels.w, shift)
        out = new(n, labels.nc, c)
        ws = scratch(L.lib().dsee_label_segsum_workspace(n, labels.h, labels.w, shift, labels.nc, c), "seg")
        L.call("label_segsum", labels.t, feat, c, 0, out, n, labels.h, labels.w, shift, labels.nc, c,
               1.0 / (hf * wf), ws)
        ctx.labels, ctx.shift, ctx.fshape = labels, shift, feat.shape
        return out

    @staticmethod
    def backward(ctx, ds):
        lab = ctx.labels
        n, hf, wf, c = ctx.fshape
        df = new(*ctx.fshape)
        L.call("label_gather", lab.t, ds.contiguous(), df, n, lab.h, lab.w, ctx.shift, lab.nc, c, c, 0, 1.0 / (hf * wf))
        return df, None, None


# ------------------------------------------------------------------------------------ fused BN + modulate + lrelu
_perm_cache = {}


def packed_perm(c, device):
    """Row order of the gamma/beta GEMM: packed row b*128 + w*64 + h*32 + cc <-> (h ? beta : gamma)[b*64 + w*32 + cc].
    Returns (index into cat([gamma rows, beta rows, one zero row]), number of packed rows)."""
    key = (c, str(device))
    if key not in _perm_cache:
        rows = (c + 63) // 64 * 128
        idx = torch.full((rows,), 2 * c, dtype=torch.long)
        for p in range(rows):
            b, rem = divmod(p, 128)
            w, rem = divmod(rem, 64)
            h, cc = divmod(rem, 32)
            ch = b * 64 + w * 32 + cc
            if ch < c:
                idx[p] = h * c + ch
        _perm_cache[key] = (idx.to(device), rows)
    return _perm_cache[key]


def pack_gamma_beta(w_gamma, w_beta, b_gamma, b_beta):
    """OIHW [C,K,3,3] x2 (+ biases) -> the row-permuted [rows,K,3,3] / [rows] the modulate kernel expects.
    Parameter-space glue on <= 5 MB tensors (differentiable torch indexing)."""
    c = w_gamma.shape[0]
    idx, rows = packed_perm(c, w_gamma.device)
    zw = torch.zeros((1,) + tuple(w_gamma.shape[1:]), dtype=w_gamma.dtype, device=w_gamma.device)
    zb = torch.zeros(1, dtype=w_gamma.dtype, device=w_gamma.device)
    w2 = torch.cat([w_gamma, w_beta, zw], 0).index_select(0, idx)
    b2 = torch.cat([b_gamma, b_beta, zb], 0).index_select(0, idx)
    return w2, b2


class SeanPack(torch.autograd.Function):
    """(w2a, wst, b2) = the packed, sigmoid-blended weight set of one SPADE / SEAN / PureSEAN norm layer in ONE kernel
    (dsee_sean_pack_fwd; backward: one kernel + a 2-thread finalize), replacing ~30 + ~45 ATen launches of sigmoid,
    blends, cat, index_select, zeros, permute and their autograd backwards per layer and pass.
    mode 0 spade (w2a, b2) | 1 sean (w2a, wst, b2) | 2 puresean (wst, b2) | 3 sean above max_fm_size (folded w2a, b2).
    wst [(tap, row)][S] is the B operand of the style-table GEMM."""

    @staticmethod
    def forward(ctx, mode, wg, wb, wsg, wsb, bg, bb, bsg, bsb, ag, ab, amax=None):
        ref = wg if wg is not None else wsg
        c = ref.shape[0]
        k = wg.shape[1] if wg is not None else 0
        sdim = wsg.shape[1] if wsg is not None else 0
        rows = L.lib().dsee_sean_pack_rows(c)
        w2a = new(rows, k, 3, 3) if mode != 2 else None
        wst = new(9 * rows, sdim) if mode in (1, 2) else None
        b2 = new(rows)
        L.call("sean_pack_fwd", wg, wb, wsg, wsb, bg, bb, bsg, bsb, ag, ab, int(mode), c, k, sdim, w2a, wst, b2, amax)
        ctx.mode, ctx.dims = int(mode), (c, k, sdim, rows)
        ctx.save_for_backward(wg, wb, wsg, wsb, bg, bb, bsg, bsb, ag, ab)
        return w2a, wst, b2

    @staticmethod
    def backward(ctx, dw2a, dwst, db2):
        wg, wb, wsg, wsb, bg, bb, bsg, bsb, ag, ab = ctx.saved_tensors
        c, k, sdim, rows = ctx.dims
        mode = ctx.mode
        if mode != 2 and dw2a is None:
            dw2a = torch.zeros(rows, k, 3, 3, dtype=torch.float32, device=db2.device if db2 is not None else wg.device)
        if mode in (1, 2) and dwst is None:
            dwst = torch.zeros(9 * rows, sdim, dtype=torch.float32, device=wsg.device)
        outs = [torch.empty_like(t) if (t is not None and ctx.needs_input_grad[i + 1]) else None
                for i, t in enumerate((wg, wb, wsg, wsb, bg, bb, bsg, bsb))]
        dalpha = new(2) if (mode in (1, 3) and (ctx.needs_input_grad[9] or ctx.needs_input_grad[10])) else None
        ws = scratch(L.lib().dsee_sean_pack_bwd_workspace(), "seanpack")
        L.call("sean_pack_bwd", wg, wb, wsg, wsb, bg, bb, bsg, bsb, ag, ab, mode, c, k, sdim,
               None if dw2a is None else dw2a.contiguous(), None if dwst is None else dwst.contiguous(),
               None if db2 is None else db2.contiguous(), *outs, dalpha, ws)
        da = (dalpha[0:1], dalpha[1:2]) if dalpha is not None else (None, None)
        return (None, *outs, da[0] if ctx.needs_input_grad[9] else None, da[1] if ctx.needs_input_grad[10] else None, None)


class TableLayout(torch.autograd.Function):
    """[N*L][9*rows] (the style-table GEMM's result) <-> the [N][9][rows][32] per-image table the kernels read."""

    @staticmethod
    def forward(ctx, t, n, nc, rows, amax=None):
        ctx.dims = (n, nc, rows)
        out = new(n, 9, rows, 32)
        L.call("style_table_layout", t.contiguous(), out, n, nc, rows, amax)
        return out

    @staticmethod
    def backward(ctx, dout):
        n, nc, rows = ctx.dims
        dt = new(n * nc, 9 * rows)
        L.call("style_table_layout_bwd", dout.contiguous(), dt, n, nc, rows)
        return dt, None, None, None, None


def style_table_packed(style, wst, rows, amax=None):
    """T[n][tap][row][r(32)] = sum_s wst[tap*rows + row][s] * style[n][r][s]: one GEMM on parameter-sized operands
    (rocBLAS through torch.matmul, see _style_gemm) + the layout kernel.  `amax`: slot that receives max |T| (on top of
    what it holds: max |w2a| from SeanPack) -- the operand bound of the gamma/beta GEMM's weights.
    (Round 4 tried hand-written VALU kernels for this 152 x 128 x 9216 product and its two gradients: 34 / 71 / 225 us against
    20 / 30 / 20 us for the library -- profiles/r04_notes.md -- and kept the library call.)"""
    n, nc, s = style.shape
    t = TableLayout.apply(_style_gemm(style.reshape(n * nc, s), wst), n, nc, rows, amax)
    t.dsee_amax = amax
    return t


class SyncBNConfig:
    """SyncBN-over-RCCL option: BatchNorm statistics over the GLOBAL batch of all data-parallel ranks, the
    reference's DataParallel branch (sync_batchnorm/batchnorm.py:70-145) with its clamp(var, eps).  Off by default:
    north_star's sync-free BN uses the shard's statistics (= the reference's single-device branch per shard)."""

    def __init__(self, world, group=None, clamp=True):
        self.world, self.group, self.clamp = int(world), group, bool(clamp)


def _stats_rows_ok(c):
    return P().sync_bn is None and c % 4 == 0 and c // 4 <= 256 and 256 % (c // 4) == 0


def bn_stats(x, running_mean, running_var, training):
    """(mean, invstd, synced) of the param-free BatchNorm inside SPADE/SEAN."""
    n, h, w, c = x.shape
    mean, invstd = new(c), new(c)
    if not training:
        L.call("norm_eval_stats", running_mean, running_var, c, BN_EPS, mean, invstd)
        return mean, invstd, None
    cfg = P().sync_bn
    if cfg is None:
        # norm_0 and norm_s of a resblock normalise the same tensor: the partial (mean, M2) rows of the pass over x stay
        # attached to it, the second layer only folds them (its own running statistics)
        rows = getattr(x, "dsee_stats_rows", None)
        if rows is not None:       # written by x's producer (UpNoise / the Winograd output transform)
            L.call("norm_stats_finalize_parts", rows[0], rows[1], c, BN_EPS, BN_MOMENTUM, mean, invstd, running_mean,
                   running_var)
            return mean, invstd, None
        part = getattr(x, "dsee_stats_part", None)
        if part is None:
            part = torch.empty(L.lib().dsee_norm_workspace(n, h * w, c, 1) // 4, dtype=torch.float32, device="cuda")
            L.call("norm_stats_partial", x, n, h * w, c, 1, part)
            if P().share_stats:
                x.dsee_stats_part = part
        L.call("norm_stats_finalize", part, n, h * w, c, 1, BN_EPS, BN_MOMENTUM, mean, invstd, running_mean, running_var)
        return mean, invstd, None
    ws = scratch(L.lib().dsee_norm_workspace(n, h * w, c, 1), "norm")
    from . import parallel
    local = new(2, c)
    L.call("norm_stats_local", x, n, h * w, c, local, ws)
    rows = parallel.gather_stats(local, cfg.world, cfg.group)      # [world, 2, C]: 8*C bytes per rank
    L.call("norm_stats_merge", rows, cfg.world, n * h * w, c, BN_EPS, BN_MOMENTUM, int(cfg.clamp), mean, invstd,
           running_mean, running_var)
    return mean, invstd, cfg


def in_stats(x):
    """(mean, invstd) [N][C] of the param-free InstanceNorm2d(affine=False) inside SPADE/SEAN (normalization.py:84-85):
    per image and channel, biased variance + eps, no running statistics -- batch statistics in training and eval alike, and
    never all-reduced.  norm_0 and norm_s of a resblock normalise the same tensor: one partial pass, finalized per layer."""
    n, h, w, c = x.shape
    mean, invstd = new(n, c), new(n, c)
    part = getattr(x, "dsee_in_part", None)
    if part is None:
        part = torch.empty(L.lib().dsee_norm_workspace(n, h * w, c, n) // 4, dtype=torch.float32, device="cuda")
        L.call("norm_stats_partial", x, n, h * w, c, n, part)
        if P().share_stats:
            x.dsee_in_part = part
    L.call("norm_stats_finalize", part, n, h * w, c, n, BN_EPS, BN_MOMENTUM, mean, invstd, None, None)
    return mean, invstd


def norm_stats(x, running_mean, running_var, training):
    """(mean, invstd, synced) of a SPADE/SEAN param-free norm: BatchNorm ([C], bn_stats) for a layer with running statistics,
    InstanceNorm ([N][C], in_stats) for one without (networks.SpadeNorm with norm_G ...instance...)."""
    if running_mean is None:
        mean, invstd = in_stats(x)
        return mean, invstd, None
    return bn_stats(x, running_mean, running_var, training)


def stat_groups(mean):
    """1 for BatchNorm statistics [C], N for InstanceNorm statistics [N][C] (the `stat_groups` of the _sg entry points)."""
    return mean.shape[0] if mean.dim() == 2 else 1


def _call_sg(name, sg, head, tail):
    """dsee_<name>(*head, *tail) for BatchNorm statistics (sg = 1: the entry point and launches of the BatchNorm path as
    they are), dsee_<name>_sg(*head, sg, *tail) for InstanceNorm statistics."""
    if sg == 1:
        L.call(name, *head, *tail)
    else:
        L.call(name + "_sg", *head, sg, *tail)


def _wino_ws(n, h, w, c, sg):
    return (L.lib().dsee_modulate_bwd_wino_workspace(n, h, w, c) if sg == 1
            else L.lib().dsee_modulate_bwd_wino_workspace_sg(n, h, w, c, sg))


def modulate_bwd(dh, out, x, scale, mean, invstd, rows, cfg, as_dm=False, add=None, xhat_amax=None, mask=None):
    """Backward of BN + modulate + LeakyReLU: (dx, dgb, col_sums [2][C], dM).  With SyncBN (`cfg`) the two per-channel
    sums of the BN backward are all-reduced over the ranks between the reduce and the apply pass.  `as_dm`: the
    gamma/beta gradient leaves the reduce pass as dM = A (g*xhat | g) A^T [36][T][rows] (dgb is None).  `mask`: the LeakyReLU
    branch of `out` as bits (written by the fused forward); the passes that take it do not read `out`.
    InstanceNorm statistics (mean [N][C]): the two sums of the norm backward are per image ([2][N][C]), the bias gradients
    col_sums stay per channel."""
    n, h, w, c = x.shape
    sg = stat_groups(mean)
    dx = torch.empty_like(x)
    sums = new(2 * sg + 2, c)
    dgb = dm = None
    t = n * (h // 4) * (w // 4)
    dha = carried_amax(dh)
    # (the pre-split reduce passes take BatchNorm statistics only: an InstanceNorm layer writes an fp32 dM in both precisions)
    pre = (as_dm and P().presplit_dm and P().presplit_gb and xhat_amax is not None and dha is not None and t % 256 == 0
           and sg == 1)
    s16 = scale.dtype == torch.float16       # written by dsee_spade_fused_fwd_f16p (16-bit storage mode)
    if s16 and not (pre and P().half):
        scale, s16 = scale.float(), False    # (a pass the packed kernels do not take: they read fp32)
    if pre:
        # max |dh| (written by the kernel that produced dh) x max(1, max |xhat|) (written by the forward pass) bounds both halves
        # (g * xhat | g) of the gradient: dM leaves the reduce pass pre-split, for the table / embedding weight gradient's P
        # operand and the adjoint data-gradient GEMM's A operand
        ga = amax_slot()
        L.call("amax_product", dha, xhat_amax, 1.0, ga)
        pk = P().half      # 16-bit storage mode: one scaled fp16 term per element (dsee_modulate_bwd_reduce_wino_f16p)
        dm = WinoOperand(_i16(36 * t * rows * (1 if pk else 2)), ga, F16P if pk else F16X2)
        ws = scratch(L.lib().dsee_modulate_bwd_wino_workspace(n, h, w, c), "norm")
        L.call("modulate_bwd_reduce_wino_f16p" if pk else "modulate_bwd_reduce_wino_f16x2", dh.contiguous(),
               None if mask is not None else out, x, scale, mean, invstd, dm.data, rows, sums, n, h, w, c, LRELU_SLOPE, ws, ga,
               DM_BOUND, mask)
    elif as_dm:
        dm = WinoOperand(new(36, t, rows), amax_slot() if _fp16_amax_needed() else None, FP32)
        ws = scratch(_wino_ws(n, h, w, c, sg), "norm")
        _call_sg("modulate_bwd_reduce_wino", sg, (dh.contiguous(), out, x, scale, mean, invstd, dm.data, rows, sums, n, h, w, c),
                 (LRELU_SLOPE, ws, dm.amax))
    else:
        dgb = (torch.zeros if c % 64 else torch.empty)(n, h, w, rows, dtype=torch.float32, device=x.device)
        ws = scratch(L.lib().dsee_norm_workspace(n, h * w, c, sg), "norm")
        _call_sg("modulate_bwd_reduce", sg, (dh.contiguous(), out, x, scale, mean, invstd, dgb, rows, sums, n, h * w, c),
                 (LRELU_SLOPE, ws))
    count = (n // sg) * h * w
    if cfg is not None:        # (BatchNorm only: InstanceNorm statistics are per image, never all-reduced)
        from . import parallel
        parallel.allreduce_sums(sums[0:2], cfg.world, cfg.group)
        count *= cfg.world
    da = amax_slot()             # max |dx|: dx is the output gradient of the convolution in front of this norm
    # dx += add: the gradient of the other consumer of x (the resblock shortcut)
    _call_sg("modulate_bwd_apply_amax", sg,
             (dh.contiguous(), None if mask is not None else out, x, scale, mean, invstd, sums, add, dx, n, h * w, c),
             (1.0 / count, LRELU_SLOPE, da, int(s16), mask))
    tag_amax(dx, da)
    return dx, dgb, sums[2 * sg:2 * sg + 2], dm


def _norm_product_direct(geom, cat, w, table, ca, b2, x, mean, invstd, out, scale, add_one):
    """out = lrelu(norm(x) * (gamma + add_one) + beta), (gamma | beta) = conv3x3(cat, w (+ per-image `table` over the one-hot
    channels behind the first `ca`)) + b2 formed in the epilogue of the direct convolution kernel"""
    wp = _pack("fwd", w, w.shape[1], geom.korder) if w is not None else None
    with _timed(_variant(geom, True), _flops(geom)):
        _call_sg("conv2d_modulate_fwd", stat_groups(mean),
                 (C.byref(geom), cat, wp, table, ca, b2.contiguous(), x, mean, invstd, out, scale, x.shape[3]),
                 (float(add_one), LRELU_SLOPE))


def _packed_bias_grad(cs, c):
    """gradient of the packed (gamma | beta) bias b2 from the two column sums cs [2][C] of the norm backward"""
    idx, _ = packed_perm(c, cs.device)
    return torch.cat([cs.reshape(-1), torch.zeros(1, device=cs.device)]).index_select(0, idx)


class SpadeNormAct(torch.autograd.Function):
    """h = lrelu(BN(x) * (conv_gamma(cat) + add_one) + conv_beta(cat)) with gamma/beta formed inside the GEMM
    epilogue; BN = sync-free batch statistics in training, running statistics in eval.  running_mean None: InstanceNorm
    (per-image batch statistics, norm_stats)."""

    @staticmethod
    def forward(ctx, x, cat, w2, b2, running_mean, running_var, training, add_one, cat_ups, grad_sink=None):
        ctx.plan = P()
        ctx.grad_sink = grad_sink
        n, h, w, c = x.shape
        rows, kin = w2.shape[0], w2.shape[1]
        assert cat.shape[3] == kin and kin % 4 == 0
        mean, invstd, ctx.sync = norm_stats(x, running_mean, running_var, training)
        geom = L.geom_fwd(n, cat.shape[1], cat.shape[2], kin, rows, 3, 1, 1, cat_ups)
        assert geom.Ho == h and geom.Wo == w
        w2 = w2.contiguous()
        out, scale = torch.empty_like(x), torch.empty_like(x)
        _norm_product_direct(geom, cat, w2, None, 0, b2, x, mean, invstd, out, scale, add_one)
        ctx.geom = geom
        ctx.save_for_backward(x, cat, w2, out, scale, mean, invstd)
        return out

    @staticmethod
    @_under_plan
    def backward(ctx, dh):
        x, cat, w2, out, scale, mean, invstd = ctx.saved_tensors
        geom = ctx.geom
        n, h, w, c = x.shape
        rows, kin = w2.shape[0], w2.shape[1]
        add = ctx.grad_sink.take() if ctx.grad_sink is not None else None
        dx, dgb, cs, _ = modulate_bwd(dh, out, x, scale, mean, invstd, rows, ctx.sync, add=add)
        dcat = dw2 = db2 = None
        if ctx.needs_input_grad[1]:
            gd = L.geom_dgrad(geom)
            dcl = conv_raw(dgb, _pack("dgrad", w2, rows, gd.korder), gd)
            if geom.ups:
                dcat = torch.empty_like(cat)
                L.call("sumpool", dcl, dcat, n, gd.Ho, gd.Wo, kin, geom.ups)
            else:
                dcat = dcl
        if ctx.needs_input_grad[2]:
            dw2 = wgrad_raw(cat, dgb, geom, rows, kin, 3, 3)
        if ctx.needs_input_grad[3]:
            db2 = _packed_bias_grad(cs, c)
        return dx, dcat, dw2, db2, None, None, None, None, None, None


def _fused_norm_ok(n, h, w, c, rows, ld):
    tpi = (h // 4) * (w // 4)
    return (P().fused_norm and P().gemm_split and P().gemm_f16x2 and P().gemm_af32 and ld in (128, 160) and rows == 2 * c
            and c % 32 == 0 and h % 4 == 0 and w % 4 == 0 and tpi % 64 == 0
            and 36 * n * tpi * ld * 4 < 0xFFFFFFF0 and 36 * n * rows * ld * 4 < 0xFFFFFFF0)


def _norm_plan(plan):
    """The plan a SPADE/SEAN norm runs under: in the 16-bit mode with plan.half_norms off the norm's own GEMMs stay on the
    two-term kernels of the fp32 path (its output h still carries max |h|, so the convolution behind it runs one-term)."""
    return plan.replace(half=False) if (plan.half and not plan.half_norms) else plan


def _norm_cat(w_sh, b_sh, labels, shift, n, h, w, has_a, has_t, cat_ups):
    """(cat, max |cat| or None, actv_low or None): the gamma/beta convolution's input cat [n,h,w,ld] = [ReLU(mlp_shared(one-hot
    label)) (128, `has_a`) ; one-hot label (32, `has_t`)].  `cat_ups`: the embedding is computed at the capped resolution
    (actv_low) and nearest-upsampled."""
    nc, ca = labels.nc, (NHIDDEN if has_a else 0)
    ld = ca + (32 if has_t else 0)
    cat, actv_low = new(n, h, w, ld), None
    cat_amax = amax_slot()     # max |cat|, written by the kernel that produces the embedding (>= 1: one-hot channels)
    if has_a:
        tab = new(9, nc, NHIDDEN)
        L.call("onehot_conv3x3_pack", w_sh.contiguous(), tab, NHIDDEN, nc)
        if cat_ups:
            assert not has_t and ld == NHIDDEN
            actv_low = new(n, h >> cat_ups, w >> cat_ups, NHIDDEN)
            L.call("onehot_conv3x3_fwd", labels.t, tab, b_sh, actv_low, n, labels.h, labels.w, shift, nc, NHIDDEN,
                   NHIDDEN, 0, 1, -1, cat_amax, 0.0)   # (the nearest upsample below keeps the maximum)
            L.call("upsample_noise_fwd", actv_low, None, None, cat, n, h, w, NHIDDEN, cat_ups)
        else:
            # ... and, with a style table, the 32 one-hot label channels behind the embedding in the same launch
            L.call("onehot_conv3x3_fwd", labels.t, tab, b_sh, cat, n, labels.h, labels.w, shift, nc, NHIDDEN, ld, 0,
                   1, ca if has_t else -1, cat_amax, 1.0 if has_t else 0.0)
    elif has_t:
        L.call("label_onehot", labels.t, cat, n, labels.h, labels.w, shift, ld, ca)
        cat_amax = None
    return cat, cat_amax, actv_low


def _norm_u(w2a, table, nb, rows, ca, kp, kind, shared=False):
    """(U, amax) of the gamma/beta convolution for `nb` images: the shared weights w2a alone, or per image with the rows of
    `table` (the style half over the one-hot channels) behind them.  `shared` (two-term form, what the fused forward reads under
    plan.shared_u): the embedding columns once per position and only the table's 32 columns per image."""
    if table is None:
        return _wino_u(w2a, rows, ca, False, rows, kp, kind)
    ua = weight_amax(w2a, table) if kind.needs_amax else None
    if shared:
        assert kind == GemmKind.F16X2_AF32 and kp == ca + 32
        u = _i16(36 * (ca // 16 + 2 * nb) * rows * 32)
        L.call("wino43_weights_table_shared", w2a, table, u, nb, rows, ca, int(kind), ua)
        return u, ua
    u = _i16(36 * nb * rows * kp * kind.words) if kind else new(36, nb, rows, kp)
    L.call("wino43_weights_table", w2a, table, u, nb, rows, ca, int(kind), ua)
    return u, ua


def _norm_keeps_v(scale, nb, n, ld, rows):
    """The V of `cat` is the Q operand of the weight / table gradient: kept for a backward pass that takes it whole"""
    return P().keep_v and scale is not None and nb == n and _wgrad_mode(ld, rows) == WgradMode.AF32


def _norm_product_fused(cat, cat_amax, w2a, table, ca, b2, x, mean, invstd, out, scale, add_one, rows, nb):
    """round 3: gamma/beta GEMM + output transform + normalise + modulate + LeakyReLU in ONE kernel (spade_fused.hip): the
    Winograd-domain product M never reaches HBM.  Returns (kept V, max |xhat|, sign mask, max |cat|)."""
    (n, h, w, c), ld, sg = x.shape, cat.shape[3], stat_groups(mean)
    kp, t = L.kpad(1, 1, ld), n * (h // 4) * (w // 4)
    ac = cat_amax if cat_amax is not None else tensor_amax(cat)
    kind = _u_kind(ld, rows, f16_only=True)
    pk = kind == GemmKind.F16_PACKED    # 16-bit storage mode: packed one-term operands, one MFMA product (dsee_spade_fused_fwd_f16p)
    v2 = WinoOperand(_i16(36 * t * ld * (1 if pk else 2)), ac, F16P if pk else F16X2)
    L.call("wino43_input_f16p" if pk else "wino43_input_f16x2", cat, v2.data, n, h, w, ld, ac, FUSED_V_BOUND)
    # SEAN norm on BatchNorm statistics: the U with its embedding columns stored once (the entry point takes it as groups = -n)
    su = (P().shared_u and table is not None and not pk and not P().fused_w4 and sg == 1 and ca >= 32 and ca % 32 == 0)
    u, ua = _norm_u(w2a, table, n, rows, ca, kp, kind, su)
    if PROFILE is not None:
        global PROFILE_OPERAND_GB
        PROFILE_OPERAND_GB += (t // 64) * (rows // 64) * 36 * 2 * 64 * ld * 4.0 / 1e9
    with _timed("spade_fused_fwd", 2.0 * 36 * t * ld * rows,
                4.0 * 36 * t * ld + 4.0 * n * h * w * c * (3 if scale is not None else 2)):
        hm = amax_slot()     # max |h|: the convolution that consumes h writes its V pre-split with this bound
        xm = amax_slot() if scale is not None else None     # max |xhat|: bounds the backward pass's gamma/beta gradient
        # the LeakyReLU branch of h as bits: all the backward pass needs of h (1/32 of its bytes, read twice).  (The kernel forms
        # the mask index with a shift: a channel count that is not a power of two -- ngf = 24, 48 -- keeps the backward on `out`)
        smask = (torch.empty(n * h * w * (c // 32), dtype=torch.int32, device=x.device)
                 if (scale is not None and P().sign_mask and (c & (c - 1)) == 0) else None)
        # (the one-wave-per-SIMD kernel takes BatchNorm statistics only: InstanceNorm layers stay on spade_fused_fwd)
        _call_sg("spade_fused_fwd_f16p" if pk else ("spade_fused_fwd_w4" if (P().fused_w4 and sg == 1) else
                                                    "spade_fused_fwd"), sg,
                 (v2.data, u, ac, FUSED_V_BOUND, ua, b2.contiguous(), x, mean, invstd, out, scale, n,
                  h, w, c, rows, ld, (-n if su else n) if table is not None else 1),
                 (float(add_one), LRELU_SLOPE, hm, xm, smask))
        tag_amax(out, hm)
    # the weight / table gradient reads the split V the kernel above consumed, or an fp32 V of its own as its Q operand
    keep = v2 if _norm_keeps_v(scale, nb, n, ld, rows) else None
    if keep is not None and not P().presplit_a:
        keep = WinoOperand(new(36, t, ld), amax_slot(), FP32)
        L.call("wino43_input", cat, keep.data, n, h, w, ld, keep.amax)
    return keep, xm, smask, ac       # (max |cat|: the backward's mlp_shared weight gradient takes `cat` as an operand again)


def _norm_product_wino(cat, w2a, table, ca, b2, x, mean, invstd, out, scale, add_one, rows, nb):
    """The gamma/beta GEMM in the Winograd domain, chunk by chunk, then dsee_wino43_output_modulate.  Returns the kept V."""
    (n, h, w, c), ld, sg = x.shape, cat.shape[3], stat_groups(mean)
    kp, b2c, kind = L.kpad(1, 1, ld), b2.contiguous(), _split_kind(ld, rows)
    keep = [] if _norm_keeps_v(scale, nb, n, ld, rows) else None
    for n0 in range(0, n, nb):
        u, ua = _norm_u(w2a, None if table is None else table[n0:n0 + nb], nb, rows, ca, kp, kind)
        m, ms = _wino_vgemm(cat[n0:n0 + nb], nb, h, w, ld, u, rows, rows, kp, table is not None, kind, keep, ua)
        px = nb * h * w
        with _timed("spade_modulate_fused", 0.0,
                    kind.bytes[2] * 36 * (px // 16) * rows + 4.0 * px * c * (3 if scale is not None else 2)):
            # (InstanceNorm: the statistics rows of this pass's images)
            mc, ic = (mean, invstd) if sg == 1 else (mean[n0:n0 + nb], invstd[n0:n0 + nb])
            _call_sg("wino43_output_modulate", 1 if sg == 1 else nb,
                     (m, b2c, x[n0:n0 + nb], mc, ic, out[n0:n0 + nb], scale[n0:n0 + nb] if scale is not None else None, nb, h,
                      w, c, rows), (float(add_one), LRELU_SLOPE, ms))
    return keep[0] if keep else None


def _norm_product(cat, cat_amax, w2a, table, b2, x, mean, invstd, out, scale, add_one, geom, nb, fused):
    """out (and scale, where the backward pass will want it) on the kernel path the shapes allow.  Returns (kept V of cat, max
    |xhat|, sign mask of out, max |cat|): what the backward pass reads besides the tensors; None where the path has none."""
    rows, ca = geom.Cout, geom.Cin - (32 if table is not None else 0)     # ca: embedding channels in front of the one-hot ones
    if fused:
        return _norm_product_fused(cat, cat_amax, w2a, table, ca, b2, x, mean, invstd, out, scale, add_one, rows, nb)
    if nb:
        return _norm_product_wino(cat, w2a, table, ca, b2, x, mean, invstd, out, scale, add_one, rows, nb), None, None, None
    _norm_product_direct(geom, cat, w2a, table, ca, b2, x, mean, invstd, out, scale, add_one)
    return None, None, None, None


def _norm_wino_wgrad(cat, dgb, dm_all, vcat, w_for_dx, nc, bwd, has_a, has_t, rows):
    """(dw2a, dtable, dactv): weight gradient of the gamma/beta convolution in the Winograd domain -- groups (xi, image), shared
    columns summed over images into dw2a, one-hot columns per image into dtable -- from the gamma/beta gradient dgb or, where the
    norm backward wrote it, its dM `dm_all`.  `w_for_dx` (w2a, where the WinoBwd `bwd` has a u_t): also dactv, from the same dM."""
    n, h, w, ld = cat.shape
    dw2a = dactv = None
    (nb, mode, t), ca, with_dx = bwd[:3], (NHIDDEN if has_a else 0), w_for_dx is not None
    if with_dx:
        rows_t, kind = L.wrows(NHIDDEN), _u_kind(rows, NHIDDEN, dm_form=getattr(dm_all, "form", None))   # (packed where dM is)
        u_t = (*_wino_u(w_for_dx, rows, NHIDDEN, 2, rows_t, L.kpad(1, 1, rows), kind), kind)
        dactv = new(n, h, w, NHIDDEN) if nb != n else None
    nbytes = (L.lib().dsee_wino43_wgrad_table_workspace(C.c_long(t), nb, ca, rows) if has_t else
              L.lib().dsee_wino43_wgrad_workspace(C.c_long(t), ld, rows))
    dtable = new(n, 9, rows, 32) if has_t else None
    wsw = scratch(nbytes, "wgrad")
    for n0 in range(0, n, nb):
        v, dm = _wino_wgrad_operands(cat[n0:n0 + nb], None if dm_all is not None else dgb[n0:n0 + nb], nb, h, w, ld, rows,
                                     mode, vcat if bwd.whole else None, dm_all)
        dwc = new(rows, NHIDDEN, 3, 3) if has_a else None
        tail = (_wgrad_code(v, dm, mode), v.amax, dm.amax)
        with _timed(_wgrad_name(mode), 2.0 * 36 * t * ld * rows):
            if has_t:
                L.call("wino43_wgrad_table", v.data, dm.data, wsw, nbytes, dwc, dtable[n0:n0 + nb], t, nb, ca, rows, nc, *tail)
            else:
                L.call("wino43_wgrad", v.data, dm.data, wsw, nbytes, dwc, t, ld, rows, rows, NHIDDEN, *tail)
        if dwc is not None:
            dw2a = dwc if dw2a is None else dw2a.add_(dwc)
        if with_dx:
            # (the ReLU mask of the embedding rides in the epilogue when the one-hot channels share `cat`)
            dac = _wino_dgrad_from_dm(dm, u_t, nb, h, w, rows, NHIDDEN, rows_t,
                                      cat[n0:n0 + nb] if has_t else None, ld if has_t else 0)
            if nb == n:
                dactv = dac
            else:
                dactv[n0:n0 + nb].copy_(dac)
    return dw2a, dtable, dactv


def _embedding_dgrad(dgb, w2a, cat, rows, has_t, wino):
    """dactv: data gradient w.r.t. the 128 embedding channels only (the one-hot channels need none), by a pass of its own over
    the gamma/beta gradient dgb.  With the one-hot channels in `cat` (`has_t`) the ReLU backward is fused into the epilogue."""
    n, h, w, ld = cat.shape
    res, act, res_ld = (cat, L.ACT_MASK, ld) if has_t else (None, L.ACT_NONE, 0)
    if wino and _wino_chunk(n, h, w, rows) is not None:
        return _wino_conv(dgb, w2a, n, h, w, NHIDDEN, rows, True, None, res, act, res_ld=res_ld)
    ga = L.ConvGeom(n, h, w, rows, h, w, NHIDDEN, 3, 3, 1, 1, -1, 0, 0, 1)
    return conv_raw(dgb, _pack("dgrad", w2a, rows, 1), ga, None, res, act, res_ld=res_ld)


def _mlp_shared_grad(dactv, cat, cat_amax, actv_low, cat_ups, lab, shift, has_t):
    """(dw_sh, db_sh) of mlp_shared, a 3x3 convolution over the one-hot label, from the embedding's gradient dactv."""
    n, h, w, ld = cat.shape
    if has_t:
        # (ReLU backward done in the dgrad epilogue) the weight gradient w.r.t. the one-hot channels already sitting in `cat`
        # (MFMA); known: the operand maximum the forward pass already wrote
        known = {(cat.data_ptr(), cat.numel(), cat._version): cat_amax} if cat_amax is not None else {}
        dw_sh = wgrad_raw(cat, dactv, L.geom_fwd(n, h, w, ld, NHIDDEN, 3, 1, 1, 0), NHIDDEN, lab.nc, 3, 3, cin_first=NHIDDEN,
                          amax_cache=known)
        return dw_sh, channel_dot(dactv, None, NHIDDEN).clone()
    wso = scratch(L.lib().dsee_onehot_conv3x3_wgrad_workspace(n, lab.h, lab.w, shift, lab.nc), "ohw")
    act_lo, ld_lo = cat, ld
    if cat_ups:
        # gradient of the nearest upsample: 2^ups x 2^ups block sums; the ReLU mask is constant per block
        dlow = torch.empty_like(actv_low)
        L.call("sumpool", dactv, dlow, n, h, w, NHIDDEN, cat_ups)
        dactv, act_lo, ld_lo = dlow, actv_low, NHIDDEN
    if P().onehot_wgrad_mfma and ld_lo == NHIDDEN and _direct_split_on():
        # round 6: the compare-select kernel is VALU bound (128 channels x 9 taps x 20 labels per pixel: 0.29 ms at 64^2,
        # N = 8); the MFMA weight gradient over 32 materialised one-hot channels takes 0.07 (profiles/r06_onehot_wgrad.txt)
        g1 = torch.empty_like(dactv)
        tag_amax(g1, amax_slot())
        L.call("act_bwd_amax", dactv.contiguous(), act_lo, g1, C.c_long(g1.numel()), L.ACT_RELU, LRELU_SLOPE, g1.dsee_amax)
        oh = new(*g1.shape[:3], MAX_LABELS)     # (lab.nc <= MAX_LABELS: Labels checks it where the map is built)
        L.call("label_onehot", lab.t, oh, n, lab.h, lab.w, shift, 32, 0)
        dw_sh = wgrad_raw(oh, g1, L.geom_fwd(*g1.shape[:3], 32, NHIDDEN, 3, 1, 1, 0), NHIDDEN, lab.nc, 3, 3)
        return dw_sh, channel_dot(g1, None, NHIDDEN).clone()
    dw_sh, db_sh = new(NHIDDEN, lab.nc, 3, 3), new(NHIDDEN)
    L.call("onehot_conv3x3_wgrad", lab.t, dactv, NHIDDEN, act_lo, ld_lo, n, lab.h, lab.w, shift, lab.nc, dw_sh, db_sh, wso)
    return dw_sh, db_sh


class SeanNormTable(torch.autograd.Function):
    """SPADE / SEAN / PureSEAN norm + LeakyReLU as ONE node, with the SEAN style half as per-image tables.

    The style map is constant per region, so its 3x3 convs are convs over the one-hot label with per-image weights
    T[n][tap][row][r] = sum_s W_s[row][s][tap] * style[n][r][s] (SURVEY B-7).  The GEMM therefore reads
    [ReLU(mlp_shared(seg)) (128) ; one-hot label (19 -> 32)] = 160 channels (K = 1440) instead of
    [actv ; style_map] = 256 (K = 2304), and the style gradient is a label-segmented sum of the gamma/beta
    gradient rows.  `table` None -> SPADE (128 channels); `w2a` None -> PureSEAN (one-hot only)."""
    W2A, B2 = 3, 5      # positions of w2a and b2 in forward's arguments (ctx.needs_input_grad)

    @staticmethod
    def forward(ctx, x, *args):
        ctx.plan = _norm_plan(P())
        n, h, w, c = x.shape
        # bench.py: the whole forward on SURVEY 8(d)'s algorithmic bytes (x twice, out, the 128-channel embedding, labels)
        with _timed("norm_forward@%dx%d" % (h, w), 0.0, 4.0 * n * h * w * (3 * c + NHIDDEN) + n * h * w), ctx.plan.active():
            return SeanNormTable._forward(ctx, x, *args)

    @staticmethod
    def _forward(ctx, x, w_sh, b_sh, w2a, table, b2, running_mean, running_var, labels, shift, training, add_one,
                 grad_sink=None, cat_ups=0):
        """`cat_ups` > 0 (the reference's max_fm_size cap, normalization.py:188-190 / 275-277): the 128-channel
        embedding is computed at the capped resolution (`shift` refers to IT) and nearest-upsampled by 2^cat_ups to x's
        resolution before the gamma/beta convolution; there is no style table then."""
        ctx.grad_sink = grad_sink
        n, h, w, c = x.shape
        has_a, has_t = w2a is not None, table is not None
        rows = w2a.shape[0] if has_a else table.shape[2]
        cat, cat_amax, actv_low = _norm_cat(w_sh, b_sh, labels, shift, n, h, w, has_a, has_t, cat_ups)
        ld = cat.shape[3]
        mean, invstd, ctx.sync = norm_stats(x, running_mean, running_var, training)
        geom = L.geom_fwd(n, h, w, ld, rows, 3, 1, 1, 0)
        assert geom.korder == 1
        w2a, tb = (w2a.contiguous() if has_a else None), (table.contiguous() if has_t else None)
        nb = ctx.wino_nb = _wino_mod_chunk(n, h, w, c, rows, has_t)
        # `scale` is only read by the backward pass: the no-grad generator forward of the D step does not write it
        need_scale = any(ctx.needs_input_grad) or not nb
        fused = nb and _fused_norm_ok(n, h, w, c, rows, ld)
        # (16-bit storage mode: the fused kernel writes the modulation factor as fp16 -- the backward pass is its only reader)
        sdt = torch.float16 if (fused and P().half) else torch.float32
        out, scale = torch.empty_like(x), (torch.empty(x.shape, dtype=sdt, device=x.device) if need_scale else None)
        vcat, ctx.xhat_amax, ctx.sign_mask, ctx.cat_amax = _norm_product(cat, cat_amax, w2a, tb, b2, x, mean, invstd, out, scale,
                                                                          add_one, geom, nb, fused)
        ctx.geom, ctx.labels, ctx.shift, ctx.has_a, ctx.has_t, ctx.rows = geom, labels, shift, has_a, has_t, rows
        ctx.cat_ups, ctx.w_amax = cat_ups, (getattr(w2a, "dsee_amax", None) if has_a else None)
        save_with_operand(ctx, vcat, x, cat, w2a, out, scale, mean, invstd, actv_low)
        return out

    @staticmethod
    @_under_plan
    def backward(ctx, dh):
        (x, cat, w2a, out, scale, mean, invstd, actv_low), vcat = saved_with_operand(ctx)
        if w2a is not None:
            w2a.dsee_amax = ctx.w_amax     # (an upper bound: the slot also holds max |style table|)
        geom, lab, rows, nb = ctx.geom, ctx.labels, ctx.rows, ctx.wino_nb
        (n, h, w, c), ld = x.shape, cat.shape[3]
        dw_sh = db_sh = dw2a = dtable = db2 = dactv = None
        wino_w = bool(nb) and (ctx.has_t or ctx.needs_input_grad[SeanNormTable.W2A])
        bwd = _wino_bwd(n, nb if wino_w else 0, h, w, ld, rows, NHIDDEN if ctx.has_a else 0, getattr(vcat, "form", None), norm_c=c)
        fused_d = bwd.u_t is not None     # the embedding's data gradient from the weight gradient's dM: no second transform of dgb
        add = ctx.grad_sink.take() if ctx.grad_sink is not None else None
        dx, dgb, cs, dm_all = modulate_bwd(dh, out, x, scale, mean, invstd, rows, ctx.sync, bwd.as_dm, add,
                                           ctx.xhat_amax if bwd.pre_dm else None, ctx.sign_mask)
        # (the weight gradient runs before the embedding block when that block takes its dactv, after it otherwise)
        wino_args = (cat, dgb, dm_all, vcat, w2a if fused_d else None, lab.nc, bwd, ctx.has_a, ctx.has_t, rows)
        if fused_d:
            dw2a, dtable, dactv = _norm_wino_wgrad(*wino_args)
        if ctx.has_a:
            if not fused_d:
                dactv = _embedding_dgrad(dgb, w2a, cat, rows, ctx.has_t, bool(nb))
            dw_sh, db_sh = _mlp_shared_grad(dactv, cat, ctx.cat_amax, actv_low, ctx.cat_ups, lab, ctx.shift, ctx.has_t)
        if wino_w:
            if not fused_d:
                dw2a, dtable, _ = _norm_wino_wgrad(*wino_args)
        elif ctx.has_t:
            # one split-K launch (image-aligned splits): shared columns -> dw2a, one-hot columns per image -> dtable
            nbytes = L.lib().dsee_conv2d_wgrad_table_workspace(C.byref(geom))
            wsw = scratch(nbytes, "wgrad")
            dtable = new(n, 9, rows, 32)
            if ctx.has_a:
                dw2a = new(rows, NHIDDEN, 3, 3)
            with _timed("conv_wgrad_128x128(+slab reduce)", _flops(geom)):
                L.call("conv2d_wgrad_table", C.byref(geom), cat, dgb, wsw, C.c_size_t(nbytes), dw2a, ld - 32, dtable,
                       lab.nc)
        elif ctx.has_a and ctx.needs_input_grad[SeanNormTable.W2A]:
            dw2a = wgrad_raw(cat, dgb, geom, rows, NHIDDEN, 3, 3)
        if ctx.needs_input_grad[SeanNormTable.B2]:
            db2 = _packed_bias_grad(cs, c)
        return dx, dw_sh, db_sh, dw2a, dtable, db2, None, None, None, None, None, None, None, None


def _style_gemm(x, wt):
    """t[nr][j] = sum_s style[nr][s] * wt[j][s]  (nr = N*19 style rows, S = 128, j = 9*rows table columns): a plain
    152 x 128 x 9216 GEMM on parameter-sized operands (<= 6 MB) -- rocBLAS through torch.matmul, forward and both
    gradients (round 1 ran it on the 1x1-conv / split-K weight-gradient kernels: 1.9 ms per step at 3-11 TF/s, the
    shapes fill 2 CUs)."""
    return x @ wt.t()


def style_table(style, ws2):
    """T[n][tap][row][r(32)] from the style matrix [N,19,S] and the (row-permuted, blend-scaled) style conv weights
    ws2 [rows,S,3,3]: a 1x1 convolution over the N*19 style rows (HIP conv kernel, differentiable), then a
    parameter-sized transpose/pad (<= 6 MB) into the layout the modulate kernel reads."""
    n, nc, s = style.shape
    rows = ws2.shape[0]
    assert s % 4 == 0 and (9 * rows) % 4 == 0
    wt = ws2.permute(2, 3, 0, 1).reshape(9 * rows, s)                   # [(tap,row)][s]
    t = _style_gemm(style.reshape(n * nc, s), wt)                       # [N*19, 9*rows]
    t = t.reshape(n, nc, 9, rows).permute(0, 2, 3, 1)                   # [N,9,rows,19]
    return torch.nn.functional.pad(t, (0, 32 - nc)).contiguous()


# ------------------------------------------------------------------------------------ pooling
class AvgPool3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n, h, w, c = x.shape
        y = new(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c)
        L.call("avgpool3s2_fwd", x, y, n, h, w, c)
        ctx.shape = x.shape
        if carried_amax(x) is not None:
            tag_amax(y, x.dsee_amax)       # (an average: max |y| <= max |x|)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, h, w, c = ctx.shape
        dx = new(n, h, w, c)
        L.call("avgpool3s2_bwd", dy.contiguous(), dx, n, h, w, c)
        return dx


class MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n, h, w, c = x.shape
        y = new(n, h // 2, w // 2, c)
        L.call("maxpool2_fwd", x, y, n, h, w, c)
        ctx.save_for_backward(x)
        if carried_amax(x) is not None:
            tag_amax(y, x.dsee_amax)       # (max |maxpool(x)| <= max |x|: the producer's bound holds for the pooled tensor)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        n, h, w, c = x.shape
        dx = torch.empty_like(x)
        dy = dy.contiguous()
        L.call("maxpool2_bwd", dy, x, dx, n, h, w, c)
        if carried_amax(dy) is not None:
            tag_amax(dx, dy.dsee_amax)     # (dx routes every dy to one position: max |dx| <= max |dy|)
        return dx


# ------------------------------------------------------------------------------------ discriminator input
class DInput(torch.autograd.Function):
    """cat([one-hot(label), image]) in NHWC (19 + 3 channels, stored 24) for a list of images that share the
    label map, stacked on N like sr_model.py:655-668 (fake first, real second)."""

    @staticmethod
    def forward(ctx, labels, *imgs):
        n, h, w, cs = imgs[0].shape
        ld = L.pad4(labels.nc + 3)
        out = new(n * len(imgs), h, w, ld)
        ao = amax_slot() if (_direct_split_on() and P().conv_amax_out) else None
        for i, img in enumerate(imgs):
            L.call("build_d_input_amax", labels.t, img.contiguous(), out[i * n:(i + 1) * n], C.c_long(n * h * w), labels.nc,
                   ld, cs, ao)
        if ao is not None:
            tag_amax(out, ao)
        ctx.nc, ctx.cs, ctx.k, ctx.n = labels.nc, cs, len(imgs), n
        return out

    @staticmethod
    def backward(ctx, dout):
        _, h, w, ld = dout.shape
        dout = dout.contiguous()
        grads = []
        for i in range(ctx.k):
            if not ctx.needs_input_grad[1 + i]:
                grads.append(None)
                continue
            dimg = new(ctx.n, h, w, ctx.cs)
            L.call("extract_image_grad", dout[i * ctx.n:(i + 1) * ctx.n], dimg, C.c_long(ctx.n * h * w), ctx.nc, ld,
                   ctx.cs)
            grads.append(dimg)
        return (None,) + tuple(grads)


# ------------------------------------------------------------------------------------ losses
MODE_L1, MODE_NEG, MODE_HINGE_REAL, MODE_HINGE_FAKE = 0, 1, 2, 3
# the other gan_mode element losses (real label 1, fake label 0; W real is MODE_NEG): x, (x-1)^2, x^2, softplus(-x),
# softplus(x) -- the last two are binary cross-entropy on logits
MODE_W_FAKE, MODE_LS_REAL, MODE_LS_FAKE, MODE_BCE_REAL, MODE_BCE_FAKE = 4, 5, 6, 7, 8


class MeanLoss(torch.autograd.Function):
    """weight * mean(l(a[lo:hi][, b])); the gradient w.r.t. `a` (zero outside [lo,hi)) is formed in the backward pass
    from the upstream gradient (a device scalar), so re-weighted terms / loss scaling / 1/k accumulation are exact.
    The train step itself backpropagates sum(losses).mean() (trainer_manager.py:36-37,53-54)."""

    @staticmethod
    def forward(ctx, a, b, mode, weight, valid_c, lo, hi):
        a = a.contiguous()
        b = b.contiguous() if b is not None else None
        ld = a.shape[-1]
        sub = a[lo:hi]
        loss = torch.zeros(1, dtype=torch.float32, device=a.device)
        L.call("loss_fwd_bwd", mode, sub, b, None, sub.numel() // ld, ld, valid_c, float(weight), loss,
               scratch(L.lib().dsee_loss_workspace(), "loss"))
        ctx.args = (mode, float(weight), valid_c, lo, hi)
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, dl):
        a, b = ctx.saved_tensors
        mode, weight, valid_c, lo, hi = ctx.args
        ld = a.shape[-1]
        grad = torch.empty_like(a) if (lo == 0 and hi == a.shape[0]) else torch.zeros_like(a)
        sub = grad[lo:hi]
        L.call("loss_bwd", mode, a[lo:hi], b, sub, sub.numel() // ld, ld, valid_c, weight,
               dl.reshape(-1)[:1].contiguous().float())
        return grad, None, None, None, None, None, None


def mean_loss(a, b, mode, weight, valid_c=None, lo=0, hi=None):
    return MeanLoss.apply(a, b, mode, weight, a.shape[-1] if valid_c is None else valid_c, lo,
                          a.shape[0] if hi is None else hi)
