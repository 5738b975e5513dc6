"""Networks of the DeepSEE train-step hot path on the HIP ops.

Module/parameter names reproduce the reference ``state_dict()`` keys exactly so
``{epoch}_net_{SR,D,E}.pth`` checkpoints interchange; the computation is re-designed for MI355X:
NHWC fp32, uint8 label maps instead of one-hot tensors, gamma/beta convolutions fused with the
sync-free BatchNorm + modulation + LeakyReLU in one MFMA kernel, upsample/noise/residual folded
into producers/consumers.

Reference: deepsee_models/networks/{sr,architecture,normalization,encoder,discriminator,loss}.py.
"""
import math
import re

import torch
import torch.nn as nn

from . import lib as L
from . import ops

NHIDDEN = ops.NHIDDEN


# ------------------------------------------------------------------------------------ parameter holders
class Holder(nn.Module):
    """Pure container used to reproduce nn.Sequential-style key paths ('mlp_shared.0.weight')."""


def attach(root, dotted, module):
    parts = dotted.split(".")
    cur = root
    for p in parts[:-1]:
        if not hasattr(cur, p):
            cur.add_module(p, Holder())
        cur = getattr(cur, p)
    cur.add_module(parts[-1], module)
    return module


class ConvP(nn.Module):
    def __init__(self, cout, cin, k, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin, k, k))
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None


class SNConvP(nn.Module):
    """Parameters of spectral_norm(nn.Conv2d): weight_orig (+bias), buffers weight_u / weight_v."""

    def __init__(self, cout, cin, k, bias):
        super().__init__()
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout))
        else:
            self.bias = None
        self.weight_orig = nn.Parameter(torch.zeros(cout, cin, k, k))
        self.register_buffer("weight_u", torch.zeros(cout))
        self.register_buffer("weight_v", torch.zeros(cin * k * k))

    _pre = None   # this forward's normalised weight when the network ran its layers as one group (ops.SNGroup)

    def weight(self, power_iter):
        if self._pre is not None:
            w, self._pre = self._pre, None
            return w
        return ops.SpectralNorm.apply(self.weight_orig, self.weight_u, self.weight_v, bool(power_iter))


class BNStats(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.long))  # never incremented


_NORM_G_RE = re.compile(r"(?:sean|spade)(\D+)(\d)x\d")


def param_free_norm_of(norm_G):
    """The param-free normalisation inside every SPADE / SEAN / PureSEAN layer of the generator, parsed from opt.norm_G as the
    reference does (normalization.py:76-92, 130-143, 223-236: `spade(\\D+)(\\d)x\\d` / `sean(...)` / `latesean(...)` after
    removing 'spectral'): "instance" (nn.InstanceNorm2d(affine=False): per image and channel, batch statistics in eval too)
    or "batch" ('syncbatch' and 'batch': BatchNorm, sync-free per shard unless opt.sync_bn).  The type is compared exactly
    (the reference tests substrings, so it would also take e.g. 'fooinstance'); any other type raises ValueError.  What this
    build does not implement -- a generator without spectral norm, a SPADE kernel size other than 3 -- raises
    NotImplementedError instead of training something else."""
    m = _NORM_G_RE.search(norm_G.replace("spectral", ""))
    if m is None:
        raise ValueError("norm_G %r: expected spectral{spade,sean,latesean}<norm><k>x<k>" % norm_G)
    kind = m.group(1)
    out = {"instance": "instance", "syncbatch": "batch", "batch": "batch"}.get(kind)
    if out is None:
        raise ValueError("%s is not a recognized param-free norm type in SPADE" % kind)
    if int(m.group(2)) != 3:
        raise NotImplementedError("norm_G %r: only 3x3 SPADE / SEAN convolutions are implemented" % norm_G)
    if "spectral" not in norm_G:
        raise NotImplementedError("norm_G %r: only the spectral-norm generator is implemented" % norm_G)
    return out


def nonspade_norm_of(norm_type):
    """The norm of the discriminator's and the style encoders' conv layers, parsed from opt.norm_D / opt.norm_E as the
    reference's get_nonspade_norm_layer does (normalization.py:19-56): "instance" (InstanceNorm2d(affine=False)), "batch"
    (nn.BatchNorm2d(affine=True)), "sync_batch" (SynchronizedBatchNorm2d(affine=True)) or "none" (the spectral-norm conv
    alone, its bias kept).  The subtype after 'spectral' is compared exactly ('syncbatch', valid in norm_G, is not valid
    here); any other value raises ValueError (a value without 'spectral' crashes the reference with UnboundLocalError)."""
    if not norm_type.startswith("spectral"):
        raise ValueError("norm type %r: expected spectral{instance,batch,sync_batch,none}" % norm_type)
    sub = norm_type[len("spectral"):]
    if sub in ("none", ""):
        return "none"
    if sub in ("instance", "batch", "sync_batch"):
        return sub
    raise ValueError("normalization layer %s is not recognized" % sub)


class BatchNormP(nn.Module):
    """Parameters and buffers of nn.BatchNorm2d(affine=True) / SynchronizedBatchNorm2d (the same state-dict entries)."""

    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.long))


class NormConv:
    """One `norm_layer(nn.Conv2d(...))` of get_nonspade_norm_layer (normalization.py:19-56) in the state-dict layout of its
    norm.  `path` is the conv's key path under a normed layout ('model1.0.0', 'initial.0.0'): Sequential(SN conv, norm) there,
    so the norm's entries (batch / sync_batch) sit at '<parent>.1'; with 'none' the SN conv (bias kept) replaces the
    Sequential, one level up ('model1.0')."""

    def __init__(self, root, path, cout, cin, k, norm):
        self.norm = norm
        parent = path.rsplit(".", 1)[0]
        self.conv_path = parent if norm == "none" else path
        self.bn_path = parent + ".1" if norm in ("batch", "sync_batch") else None
        attach(root, self.conv_path, SNConvP(cout, cin, k, norm == "none"))
        if self.bn_path is not None:
            attach(root, self.bn_path, BatchNormP(cout))

    @staticmethod
    def _get(root, dotted):
        m = root
        for p in dotted.split("."):
            m = m._modules[p]
        return m

    def conv(self, root):
        return self._get(root, self.conv_path)

    def apply(self, root, x, w, act, training, conv=None, **conv_kw):
        """act(norm(conv(x, w))): w is the conv's spectral-normalised weight of this forward.  `conv`: conv(w, bias) replaces
        the dense convolution of x (the label-masked noise layer of StyleEncoder; x is then ignored)."""
        if self.norm == "none":
            if conv is not None:
                return ops.Act.apply(conv(w, self.conv(root).bias), act)
            return ops.conv2d(x, w, self.conv(root).bias, act=act, **conv_kw)
        x = conv(w, None) if conv is not None else ops.conv2d(x, w, None, **conv_kw)
        if self.norm == "instance":
            return ops.InstNormAct.apply(x, act)
        bn = self._get(root, self.bn_path)
        return ops.BatchNormAct.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                      bn.num_batches_tracked if self.norm == "batch" else None, training, act)


class VecP(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n))


class Conv1dP(nn.Module):
    """style_conv = nn.Conv1d(19, 19, 1): defined by the reference, never used (normalization.py:156)."""

    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(19, 19, 1))
        self.bias = nn.Parameter(torch.zeros(19))


# ------------------------------------------------------------------------------------ noise / randomness
EPOCH_STRIDE = 1 << 36          # stream positions reserved per forward (a forward draws < 2^31 float4s)
_M64 = (1 << 64) - 1


def eval_stream_seed(seed, pinned):
    """Philox key of the eval-mode style-field stream: a fixed odd-multiplier transform of the model's noise seed (pinned False)
    or of an explicit `style_seed` (pinned True), the two families kept apart by the low bit of the argument."""
    return ((2 * int(seed) + int(bool(pinned))) * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & _M64
_COIN_TAGS = {"enc_full": 0, "enc_noise": 1}
_REGISTERED_EPOCH = None


class DeviceNoise:
    """Production source of the path's random draws: Philox counter RNG on the device for N(0,1)/U(0,1)
    tensors; the two per-forward branch coins (sr_model.py:616,643: python ``random`` in the reference) are a pure
    function of (coin_seed, forward index, tag).  Under data-parallel training every rank must take the same
    encoder branch (the unused branch gets no gradient): `coin_seed` is therefore the same on all ranks
    (it never depends on the rank, unlike `seed`, which parallel.attach offsets per rank for the noise tensors), and
    nothing else in the process -- a dataset drawing from the global ``random``, say -- can desynchronise it.  Being
    stateless, the coins of the NEXT forward can be looked at before it runs (the hipGraph variant to replay is chosen
    by them, managers.TrainerManager)."""

    def __init__(self, seed=0, coin_seed=None):
        self.seed, self.offset, self.step = int(seed), 0, 0
        self.coin_seed = int(seed) if coin_seed is None else int(coin_seed)
        # The device-side epoch every Philox stream drawn through this object is offset by (dsee_rng_set_epoch): one int64
        # in HBM, advanced by a device-side add at the start of every training forward -- so that a captured hipGraph,
        # whose kernel arguments (seed, offset) are frozen, still draws fresh noise on every replay.
        self.epoch = torch.zeros(1, dtype=torch.int64, device="cuda")
        # eval-mode style fields (opt.random_style_matrix) draw from a second stream, positioned by a HOST counter that is not
        # part of state_dict(): an eval forward between two training steps moves neither `offset` nor the device epoch
        self.eval_count = 0
        self._eval = [eval_stream_seed(self.seed, False), 0]
        self._register()

    def _register(self):
        """Tell the library which epoch the kernels launched from now on read (a captured graph keeps the pointer it was
        captured with).  The registered tensor is pinned by a module-level reference: the library must never be left
        with the address of freed memory."""
        import ctypes
        from . import lib as L
        global _REGISTERED_EPOCH
        _REGISTERED_EPOCH = self.epoch
        L.lib().dsee_rng_set_epoch(ctypes.c_void_p(self.epoch.data_ptr()))

    def ensure_registered(self):
        """Re-register this object's epoch if another DeviceNoise (a second model in the process) registered its own since:
        called by every consumer of a Philox stream drawn here (ops.PhiloxNormal.bind), forward and backward."""
        if _REGISTERED_EPOCH is not self.epoch:
            self._register()

    def begin_step(self):
        """Start of a training forward: stream offsets restart at 0 and the device epoch advances."""
        self.step += 1
        self.offset = 0
        self.epoch.add_(EPOCH_STRIDE)
        self._register()

    def begin_eval(self, style_seed=None):
        """Start of an eval-mode forward (SRModel.forward for every mode but generator / discriminator).  Without `style_seed` the
        forward gets the next EPOCH_STRIDE positions of the eval stream; with it, position 0 of the stream keyed by that seed,
        and the counter stays: same seed, same labels -> the same style fields, bit for bit."""
        if style_seed is None:
            self.eval_count += 1
            self._eval = [eval_stream_seed(self.seed, False), self.eval_count * EPOCH_STRIDE]
        else:
            self._eval = [eval_stream_seed(style_seed, True), 0]

    def style_field(self, labels, training):
        """The noise field of FullStyleEncoder under opt.random_style_matrix, one N(0,1) scalar per pixel of `labels`
        (ops.Labels), as a lazily consumed stream (ops.PhiloxField).  Training: the ordinary (seed, offset, device epoch)
        positions, (N H W + 3) // 4 of them -- a captured graph draws a fresh field on every replay.  Eval: the eval stream, its
        (seed, offset) plain kernel arguments without the epoch."""
        shape = (labels.n, labels.h, labels.w)
        count = (labels.n * labels.h * labels.w + 3) // 4
        if training:
            f = ops.PhiloxField(shape, self.seed, self.offset, True, self)
            self.offset += count
        else:
            f = ops.PhiloxField(shape, self._eval[0], self._eval[1], False)
            self._eval[1] += count
        return f

    def state_dict(self):
        """What a resumed run needs to CONTINUE the branch-coin and noise sequences instead of repeating them from the start
        of training (saved next to the checkpoints, SRModel.save)."""
        return {"step": int(self.step), "epoch": int(self.epoch.item())}

    def load_state_dict(self, state):
        self.step = int(state["step"])
        self.epoch.fill_(int(state["epoch"]))

    def coin(self, tag, step=None):
        import random as _r
        s = self.step if step is None else int(step)
        return _r.Random((self.coin_seed * 2654435761 + s) * 4 + _COIN_TAGS[tag]).random()

    def _fill(self, shape_nhwc, normal):
        n = 1
        for s in shape_nhwc:
            n *= s
        t = ops.rng_fill(tuple(shape_nhwc), self.seed, self.offset, normal)
        self.offset += (n + 3) // 4
        return t

    def normal_nhwc(self, shape_nhwc, tag):
        """The noise-injection draws are consumed lazily (ops.PhiloxNormal): same stream positions as _fill."""
        n = 1
        for s in shape_nhwc:
            n *= s
        assert n % 4 == 0
        t = ops.PhiloxNormal(shape_nhwc, self.seed, self.offset, self)
        self.offset += n // 4
        return t

    def uniform(self, shape, tag):
        return self._fill(shape, False)

    def normal(self, shape, tag):
        return self._fill(shape, True)


class ReplayNoise:
    """Test-time source: replays a tape recorded from the oracle (oracle.RecordingCtl) so both sides see the
    same noise tensors and branch decisions."""

    def __init__(self, tape):
        self.tape, self.pos = list(tape), 0

    def begin_step(self):
        pass

    def begin_eval(self, style_seed=None):
        pass

    def style_field(self, labels, training):
        """The reference's randn(N, label_nc, H, W) from the tape, gathered at every pixel's own class -> [N, H, W] (the other
        channels are multiplied by zero)."""
        v = self._next("normal", "style_field")
        assert tuple(v.shape) == (labels.n, labels.nc, labels.h, labels.w), (tuple(v.shape), labels.nc)
        idx = labels.t.long().clamp_(max=labels.nc - 1)[:, None]
        return v.cuda().float().gather(1, idx)[:, 0].contiguous()

    def _next(self, kind, tag):
        k, t, v = self.tape[self.pos]
        assert k == kind and t == tag, "replay mismatch: want %s/%s, tape has %s/%s" % (kind, tag, k, t)
        self.pos += 1
        return v

    def coin(self, tag):
        return self._next("coin", tag)

    def normal_nhwc(self, shape_nhwc, tag):
        v = self._next("normal", tag)  # NCHW cpu
        t = ops.to_nhwc(v.cuda(), shape_nhwc[3])
        assert tuple(t.shape) == tuple(shape_nhwc)
        return t

    def uniform(self, shape, tag):
        v = self._next("uniform", tag)
        assert tuple(v.shape) == tuple(shape)
        return v.cuda()

    def normal(self, shape, tag):
        v = self._next("normal", tag)
        assert tuple(v.shape) == tuple(shape)
        return v.cuda()


# ------------------------------------------------------------------------------------ SPADE / SEAN / PureSEAN
class SpadeNorm(nn.Module):
    """normalization.py: SPADE (:71-120), SEAN_Block (:123-213), PureSEAN_Block (:216-286) followed by the
    resblock's LeakyReLU (architecture.py:92,114)."""

    def __init__(self, kind, c, label_nc, style_size, max_fm_size, norm="batch"):
        super().__init__()
        self.kind, self.c, self.max_fm = kind, c, max_fm_size
        # InstanceNorm keeps no running statistics: no buffers, the reference's state-dict keys (ops.norm_stats)
        self.param_free_norm = BNStats(c) if norm == "batch" else None
        self.norm = norm
        attach(self, "mlp_shared.0", ConvP(NHIDDEN, label_nc, 3))
        if kind in ("spade", "sean"):
            self.mlp_gamma = ConvP(c, NHIDDEN, 3)
            self.mlp_beta = ConvP(c, NHIDDEN, 3)
        if kind in ("sean", "puresean"):
            self.style_conv = Conv1dP()
            self.mlp_style_gamma = ConvP(c, style_size, 3)
            self.mlp_style_beta = ConvP(c, style_size, 3)
        if kind == "sean":
            self.alpha_beta = nn.Parameter(torch.rand(1))
            self.alpha_gamma = nn.Parameter(torch.rand(1))

    def _running(self):
        """(running_mean, running_var) of a BatchNorm layer; (None, None) selects InstanceNorm statistics in ops."""
        st = self.param_free_norm
        return (st.running_mean, st.running_var) if st is not None else (None, None)

    def forward(self, x, labels, style, training, grad_sink=None):
        """`grad_sink` (ops.GradSink): the gradient of the other consumer of x (the resblock shortcut) is added to dx
        inside this norm's backward pass."""
        n, h, w, c = x.shape
        fm = h if self.kind == "spade" else min(h, self.max_fm)  # SPADE.forward has no fm cap
        if h != w and self.kind != "spade":
            # the cap of a non-square map is per axis in the reference (one nearest-neighbour factor each): not built here, and
            # unreachable behind sr_model.check_geometry -- never decided from the height alone
            if max(h, w) > self.max_fm:
                raise ValueError("%s norm on a %d x %d map with max_fm_size=%d: the cap on non-square maps is not built"
                                 % (self.kind, h, w, self.max_fm))
            fm = h
        sh = self.mlp_shared._modules["0"]
        capped = fm != h
        if capped and (h * w) % 128 == 0 and c % 64 == 0:
            return self._forward_capped(x, labels, training, fm, grad_sink)
        if capped or (self.kind != "spade" and (h * w) % 128 != 0):
            return self._forward_dense(x, labels, style, training, fm, grad_sink)
        shift = labels.shift_for(h, w)
        # ---- table path: one fused autograd node per norm; its packed / blended weight set comes from ONE kernel
        P = ops.SeanPack.apply
        am = ops.amax_slot()     # max |packed weights| (and |style table|), written by the producers themselves
        if self.kind == "spade":
            w2a, _, b2 = P(0, self.mlp_gamma.weight, self.mlp_beta.weight, None, None, self.mlp_gamma.bias,
                           self.mlp_beta.bias, None, None, None, None, am)
            w2a.dsee_amax = am
            return ops.SeanNormTable.apply(x, sh.weight, sh.bias, w2a, None, b2, *self._running(),
                                           labels, shift, training, 1.0, grad_sink)
        if self.kind == "sean":
            w2a, wst, b2 = P(1, self.mlp_gamma.weight, self.mlp_beta.weight, self.mlp_style_gamma.weight,
                             self.mlp_style_beta.weight, self.mlp_gamma.bias, self.mlp_beta.bias,
                             self.mlp_style_gamma.bias, self.mlp_style_beta.bias, self.alpha_gamma, self.alpha_beta, am)
            w2a.dsee_amax = am
            table = ops.style_table_packed(style, wst, b2.shape[0], am)
            return ops.SeanNormTable.apply(x, sh.weight, sh.bias, w2a, table, b2, *self._running(),
                                           labels, shift, training, 1.0, grad_sink)
        # puresean: out = xhat * gamma_s + beta_s
        _, wst, b2 = P(2, None, None, self.mlp_style_gamma.weight, self.mlp_style_beta.weight, None, None,
                       self.mlp_style_gamma.bias, self.mlp_style_beta.bias, None, None, None)
        table = ops.style_table_packed(style, wst, b2.shape[0], am)
        return ops.SeanNormTable.apply(x, None, None, None, table, b2, *self._running(), labels, shift,
                                       training, 0.0, grad_sink)

    def _forward_capped(self, x, labels, training, fm, grad_sink=None):
        """The reference's max_fm_size cap (normalization.py:171-190, 258-277) on the fused / Winograd path: above the
        cap BOTH the SPADE embedding and the "style map" are the embedding computed at the capped resolution and
        nearest-upsampled (the style matrix is ignored; it only type-checks because nhidden == style size), so the two
        weight sets act on the same 128 channels and fold into one: gamma/beta = conv(up(actv), W_folded)."""
        n, h, w, c = x.shape
        sh = self.mlp_shared._modules["0"]
        ups = int(round(math.log2(h // fm)))
        am = ops.amax_slot()
        if self.kind == "sean":
            w2a, _, b2 = ops.SeanPack.apply(3, self.mlp_gamma.weight, self.mlp_beta.weight, self.mlp_style_gamma.weight,
                                            self.mlp_style_beta.weight, self.mlp_gamma.bias, self.mlp_beta.bias,
                                            self.mlp_style_gamma.bias, self.mlp_style_beta.bias, self.alpha_gamma,
                                            self.alpha_beta, am)
            add_one = 1.0
        else:  # puresean: out = xhat * gamma_s + beta_s
            w2a, _, b2 = ops.SeanPack.apply(0, self.mlp_style_gamma.weight, self.mlp_style_beta.weight, None, None,
                                            self.mlp_style_gamma.bias, self.mlp_style_beta.bias, None, None, None, None, am)
            add_one = 0.0
        w2a.dsee_amax = am
        return ops.SeanNormTable.apply(x, sh.weight, sh.bias, w2a, None, b2, *self._running(), labels,
                                       labels.shift_for(fm, w * fm // h), training, add_one, grad_sink, ups)

    def _forward_dense(self, x, labels, style, training, fm, grad_sink=None):
        """General path (style map materialised as 128 gathered channels): resolutions below 16x16, and the
        reference's max_fm_size cap where the upsampled embedding replaces the style map."""
        n, h, w, c = x.shape
        shift = labels.shift_for(fm, w * fm // h)
        cat_ups = 0
        sh = self.mlp_shared._modules["0"]
        capped = fm != h
        if capped:
            # normalization.py:188-190 / 275-277: actv AND style_map both become the nearest-upsampled SPADE
            # activation (style is ignored; only type-checks because nhidden == style size).
            cat_ups = int(round(math.log2(h // fm)))
            actv = ops.SeanInput.apply(sh.weight, sh.bias, None, labels, shift, True, False)
        if self.kind == "spade":
            cat = ops.SeanInput.apply(sh.weight, sh.bias, None, labels, shift, True, False)
            w2, b2 = ops.pack_gamma_beta(self.mlp_gamma.weight, self.mlp_beta.weight, self.mlp_gamma.bias,
                                         self.mlp_beta.bias)
            add_one = 1.0
        elif self.kind == "sean":
            wg, wb = torch.sigmoid(self.alpha_gamma), torch.sigmoid(self.alpha_beta)
            if capped:
                # both halves of the concatenated input are `actv`: fold the two weight sets together
                wgam = (1.0 - wg) * self.mlp_gamma.weight + wg * self.mlp_style_gamma.weight
                wbet = (1.0 - wb) * self.mlp_beta.weight + wb * self.mlp_style_beta.weight
                cat = actv
            else:
                cat = ops.SeanInput.apply(sh.weight, sh.bias, style, labels, shift, True, True)
                wgam = torch.cat([(1.0 - wg) * self.mlp_gamma.weight, wg * self.mlp_style_gamma.weight], 1)
                wbet = torch.cat([(1.0 - wb) * self.mlp_beta.weight, wb * self.mlp_style_beta.weight], 1)
            bg = (1.0 - wg) * self.mlp_gamma.bias + wg * self.mlp_style_gamma.bias
            bb = (1.0 - wb) * self.mlp_beta.bias + wb * self.mlp_style_beta.bias
            w2, b2 = ops.pack_gamma_beta(wgam, wbet, bg, bb)
            add_one = 1.0
        else:  # puresean: out = xhat * gamma_s + beta_s
            cat = actv if capped else ops.SeanInput.apply(sh.weight, sh.bias, style, labels, shift, False, True)
            w2, b2 = ops.pack_gamma_beta(self.mlp_style_gamma.weight, self.mlp_style_beta.weight,
                                         self.mlp_style_gamma.bias, self.mlp_style_beta.bias)
            add_one = 0.0
        return ops.SpadeNormAct.apply(x, cat, w2, b2, *self._running(), training, add_one, cat_ups,
                                      grad_sink)


class SPADEResnetBlock(nn.Module):
    """architecture.py:24-147 with fin == fout (identity shortcut)."""

    def __init__(self, c, opt, kind):
        super().__init__()
        self.kind, self.add_noise_cfg = kind, bool(opt.add_noise)
        self.conv_0 = SNConvP(c, c, 3, True)
        self.conv_1 = SNConvP(c, c, 3, True)
        norm = param_free_norm_of(opt.norm_G) if hasattr(opt, "norm_G") else "batch"    # (an opt without norm_G: BatchNorm)
        self.norm_0 = SpadeNorm(kind, c, opt.semantic_nc, opt.regional_style_size, opt.max_fm_size, norm)
        self.norm_1 = SpadeNorm(kind, c, opt.semantic_nc, opt.regional_style_size, opt.max_fm_size, norm)
        if self.add_noise_cfg:
            self.noise_in, self.noise_skip, self.noise_middle = VecP(c), VecP(c), VecP(c)

    def forward(self, x, labels, style, noise, tag, ups, training, out_act=L.ACT_NONE, defer_act_bwd=False):
        """`defer_act_bwd`: the block's only consumer applies the backward of `out_act` (ops.Conv2d.forward)."""
        noisy = self.add_noise_cfg and training
        n, h0, w0, c = x.shape
        shp = (n, h0 << ups, w0 << ups, c)
        res_noise = None
        if noisy:
            x = ops.UpNoise.apply(x, self.noise_in.weight, noise.normal_nhwc(shp, tag + ".noise_in"), ups, training)
            # the shortcut x_s = noise_skip(x) (architecture.py:133-134) is not materialised: conv_1's output transform
            # adds x + w_skip * eps_skip (a replayed noise TENSOR, as in the parity tests, takes the explicit pass)
            res_noise = (self.noise_skip.weight, noise.normal_nhwc(shp, tag + ".noise_skip"))
        elif ups:
            x = ops.UpNoise.apply(x, None, None, ups)
        # x feeds norm_0 and the shortcut: the shortcut's gradient reaches x through norm_0's backward (ops.GradSink)
        sink = ops.GradSink() if (torch.is_grad_enabled() and x.requires_grad) else None
        h = self.norm_0(x, labels, style, training, sink)
        # noise_middle (architecture.py:111-112) rides in conv_0's output transform
        dx = ops.conv2d(h, self.conv_0.weight(training), self.conv_0.bias,
                        noise=(self.noise_middle.weight, noise.normal_nhwc(shp, tag + ".noise_middle")) if noisy else None,
                        stats=training)
        h = self.norm_1(dx, labels, style, training)
        return ops.conv2d(h, self.conv_1.weight(training), self.conv_1.bias, res=x, act=out_act, res_noise=res_noise,
                          res_sink=sink, defer_act_bwd=defer_act_bwd)


class ResnetBlock(nn.Module):
    """The pix2pixHD block of the netG ablation `nospadenostyle` (ablation.py:13-29) with norm_layer = spectralinstance
    (ablation.py:147: the conv's bias removed, InstanceNorm2d(affine=False)):
        ReflectionPad(1) -> SN conv3x3 -> IN -> ReLU -> ReflectionPad(1) -> SN conv3x3 -> IN;  out = x + y
    State-dict keys as the reference's nn.Sequential: conv_block.{1,4}.0.{weight_orig,weight_u,weight_v}.  Labels, style and
    noise are unused.  The reflection padding is the border pass of ops.Conv2d (`reflect`), the closing sum rides in the second
    norm's pass (ops.InstNormRes)."""
    kind = "resnet"
    defers_act = False      # (the LeakyReLU in front of conv_img is applied here, forward and backward: no `in_act` contract)

    def __init__(self, c):
        super().__init__()
        attach(self, "conv_block.1.0", SNConvP(c, c, 3, False))
        attach(self, "conv_block.4.0", SNConvP(c, c, 3, False))

    @property
    def conv_0(self):
        return self.conv_block._modules["1"]._modules["0"]

    @property
    def conv_1(self):
        return self.conv_block._modules["4"]._modules["0"]

    def forward(self, x, labels, style, noise, tag, ups, training, out_act=L.ACT_NONE, defer_act_bwd=False):
        assert not defer_act_bwd
        if ups:
            x = ops.UpNoise.apply(x, None, None, ups)
        h = ops.conv2d(x, self.conv_0.weight(training), None, reflect=True)
        h = ops.InstNormAct.apply(h, L.ACT_RELU)
        h = ops.conv2d(h, self.conv_1.weight(training), None, reflect=True)
        return ops.InstNormRes.apply(h, x, out_act)


def make_block(c, opt, kind):
    """One generator block of a sr_model.block_plan kind: 'resnet' (netG = nospadenostyle) or a SPADE / SEAN / PureSEAN block."""
    return ResnetBlock(c) if kind == "resnet" else SPADEResnetBlock(c, opt, kind)


class DeepSEESR(nn.Module):
    """sr.py:10-98; with the block kinds of sr_model.block_plan also the three generators of ablation.py (opt.netG)."""

    def __init__(self, opt, plan):
        super().__init__()
        c = 16 * opt.ngf
        self.c = c
        self.initial = ConvP(c, 3, 3)
        self.head_0 = make_block(c, opt, plan[0][1])
        self.G_middle_0 = make_block(c, opt, plan[1][1])
        self.G_middle_1 = make_block(c, opt, plan[2][1])
        self.up_list = nn.ModuleList([make_block(c, opt, k) for _, k in plan[3:]])
        self.conv_img = ConvP(3, c, 3)
        self._sn = None

    def forward(self, image_lr, labels, style, noise, training):
        blocks = [("head_0", self.head_0, 0), ("G_middle_0", self.G_middle_0, 1), ("G_middle_1", self.G_middle_1, 0)]
        blocks += [("up_list.%d" % i, b, 1) for i, b in enumerate(self.up_list)]
        if self._sn is None:      # all spectral-normalised convolutions of the generator: one group launch per forward
            self._sn = ops.SNGroup([c for _, b, _ in blocks for c in (b.conv_0, b.conv_1)])
        self._sn.run(training)
        self._sn.wino_weights(torch.is_grad_enabled())
        x = ops.conv2d(image_lr, self.initial.weight, self.initial.bias)
        for i, (tag, blk, ups) in enumerate(blocks):
            # the LeakyReLU in front of conv_img (sr.py:94) rides in the last block's epilogue
            # ... and its BACKWARD in conv_img's data-gradient kernel (x has no other consumer): ops.Conv2d.forward
            last = i == len(blocks) - 1
            defer = last and torch.is_grad_enabled() and x.requires_grad and ops.P().defer_act and getattr(blk, "defers_act", True)
            x = blk(x, labels, style, noise, tag, ups, training, L.ACT_LRELU if last else L.ACT_NONE, defer)
        return ops.conv2d(x, self.conv_img.weight, self.conv_img.bias, act=L.ACT_TANH, in_act=L.ACT_LRELU if defer else 0)


# ------------------------------------------------------------------------------------ style encoders
class EncBranch(nn.Module):
    """conv(SN) + norm (opt.norm_E: InstanceNorm by default) + LeakyReLU stacks of encoder.py:83-99 (full) / :142-158 (mini)."""

    def __init__(self, names, strides, ups, nf, cin, norm="instance"):
        super().__init__()
        chans = [(nf, cin), (2 * nf, nf), (4 * nf, 2 * nf), (8 * nf, 4 * nf)]
        self.names, self.strides, self.ups = names, strides, ups
        self.norm_layers = [NormConv(self, nm, co, ci, 3, norm) for nm, (co, ci) in zip(names, chans)]

    def convs(self):
        return [nl.conv(self) for nl in self.norm_layers]

    def forward_main(self, x, training):
        for nl, s, u in zip(self.norm_layers, self.strides, self.ups):
            x = nl.apply(self, x, nl.conv(self).weight(training), L.ACT_LRELU, training, stride=s, pad=1, ups=u)
        return x


FULL_NAMES = ["initial.0.0", "down0.0.0", "down1.0.0", "up_conv.1.0"]
MINI_NAMES = ["initial.0.0", "conv0.0.0", "conv1.0.0", "conv2.1.0"]


class StyleEncoder(nn.Module):
    """CombinedstyleEncoder (encoder.py:178-210) or FullStyleEncoder (:73-132)."""

    def __init__(self, opt):
        super().__init__()
        nf, s = opt.nef, opt.regional_style_size
        self._sn = {}
        self.combined = opt.netE == "combinedstyle"
        # encoder.py:116-120: FullStyleEncoder.forward replaces its input by randn(N, label_nc, crop, crop) * seg
        self.random_style = bool(getattr(opt, "random_style_matrix", False))
        if self.random_style and opt.netE != "fullstyle":
            raise ValueError("random_style_matrix needs netE='fullstyle', got netE=%r: CombinedstyleEncoder.forward calls "
                             "encoder_full.forward_main(x) directly (encoder.py:197-198), so the replacement of x by "
                             "label-masked noise in FullStyleEncoder.forward (encoder.py:118-120) never runs there and the RGB "
                             "image meets a convolution built for label_nc=%d input channels" % (opt.netE, opt.label_nc))
        self.scale = opt.noisy_style_scale
        self.dist = opt.noisy_style_dist
        if opt.semantic_nc != opt.label_nc and (self.scale > 0 or self.random_style):
            # the reference fails in its first training forward pass here: the style matrix has semantic_nc rows and the corruption
            # indexes the label_nc noise weights with them (encoder.py:54-56, IndexError); the random style field is
            # randn(N, seg.size(1) = semantic_nc, ..) * seg, fed to a first convolution built for label_nc input channels
            # (encoder.py:78, 119).  There is no training behaviour to reproduce: refuse at build (which also rules out the one use
            # the reference could run, inference with the corruption switched off by no_noise).
            raise ValueError("contain_dontcare_label (semantic_nc=%d, label_nc=%d) needs noisy_style_scale=0 and no "
                             "random_style_matrix: the encoder has label_nc noise weights and a label_nc-channel first layer for "
                             "semantic_nc regions / noise channels (the reference raises in encoder.py:56 / :120)"
                             % (opt.semantic_nc, opt.label_nc))
        if self.scale > 0:
            self.noise_weights = nn.Parameter(torch.zeros(opt.label_nc))
        self.norm = norm = nonspade_norm_of(getattr(opt, "norm_E", "spectralinstance"))
        self.final_layer = NormConv(self, "final.0.0", s, 8 * nf, 3, norm)
        if self.combined:
            self.encoder_full = EncBranch(FULL_NAMES, [1, 2, 2, 1], [0, 0, 0, 1], nf, 3, norm)
            NormConv(self.encoder_full, "final.0.0", s, 8 * nf, 3, norm)  # constructed, unused
            self.encoder_mini = EncBranch(MINI_NAMES, [1, 1, 1, 1], [0, 0, 0, 1], nf, 3, norm)
            NormConv(self.encoder_mini, "final.0.0", s, 8 * nf, 3, norm)  # constructed, unused
        elif opt.netE == "fullstyle":
            # FullStyleEncoder keeps its layers at the root of the state dict
            chans = [(nf, opt.label_nc if self.random_style else 3), (2 * nf, nf), (4 * nf, 2 * nf), (8 * nf, 4 * nf)]
            self.norm_layers = [NormConv(self, nm, co, ci, 3, norm) for nm, (co, ci) in zip(FULL_NAMES, chans)]
        else:
            raise NotImplementedError("netE=%s (ministyle crashes in the reference too)" % opt.netE)

    def forward(self, x, labels, mode, no_noise, noise, training):
        # the spectral-normalised layers THIS forward uses (the other branch's u / v must not advance: the reference's
        # hook only runs for modules that are called), as one group launch
        if mode not in self._sn:
            if self.combined:
                br = self.encoder_full if mode == "full" else self.encoder_mini
                layers = br.convs()
            else:
                layers = [nl.conv(self) for nl in self.norm_layers]
            self._sn[mode] = ops.SNGroup(layers + [self.final_layer.conv(self)])
        self._sn[mode].run(training)
        if self.combined:
            x = (self.encoder_full if mode == "full" else self.encoder_mini).forward_main(x, training)
        else:
            first = None
            if self.random_style:
                # the image is ignored: the first layer reads (labels, one noise scalar per pixel) -- ops.OnehotNoiseConv3x3
                field = noise.style_field(labels, training)
                first = lambda w, b: ops.onehot_noise_conv3x3(labels, field, w, b)      # noqa: E731
            for i, (nl, s, u) in enumerate(zip(self.norm_layers, [1, 2, 2, 1], [0, 0, 0, 1])):
                x = nl.apply(self, x, nl.conv(self).weight(training), L.ACT_LRELU, training,
                             conv=first if i == 0 else None, stride=s, pad=1, ups=u)
        x = self.final_layer.apply(self, x, self.final_layer.conv(self).weight(training), L.ACT_TANH, training)
        sm = ops.StylePool.apply(x, labels, labels.shift_for(x.shape[1], x.shape[2]))
        if self.scale > 0 and not no_noise:
            # encoder.py:51-70 on the [N,19,S] style matrix (KB-sized parameter-space glue)
            nw = torch.sigmoid(self.noise_weights)[None, :, None]
            if self.dist == "uniform":
                z = noise.uniform(tuple(sm.shape), "style_noise")
            elif self.dist == "normal":
                z = noise.normal(tuple(sm.shape), "style_noise")
            else:
                raise ValueError("Does not exist: {}".format(self.dist))      # encoder.py:66
            sm = (sm + ((z * 2 - 1) * self.scale) * nw).clamp(-1, 1)
        return sm


# ------------------------------------------------------------------------------------ discriminator
class NLayerD(nn.Module):
    """discriminator.py:67-120."""

    def __init__(self, opt):
        super().__init__()
        nf = opt.ndf
        cin = opt.semantic_nc + opt.output_nc         # (what ops.DInput writes: Labels.nc one-hot channels + the image)
        self.nl = opt.n_layers_D
        self.norm = nonspade_norm_of(getattr(opt, "norm_D", "spectralinstance"))
        attach(self, "model0.0", ConvP(nf, cin, 4))
        self.norm_layers = []
        for n in range(1, self.nl):
            prev, nf = nf, min(nf * 2, 512)
            self.norm_layers.append(NormConv(self, "model%d.0.0" % n, nf, prev, 4, self.norm))
        attach(self, "model%d.0" % self.nl, ConvP(1, nf, 4))

    def convs(self):
        """The spectral-normalised convolutions model1 .. model{n_layers_D - 1}."""
        return [nl.conv(self) for nl in self.norm_layers]

    @property
    def per_sample(self):
        """True when every layer normalises each sample on its own (InstanceNorm or no norm): D's output for one image
        does not depend on the other images of the batch."""
        return self.norm in ("instance", "none")

    def forward(self, x, training, x_detached=None):
        """`x_detached` (round 6): a second batch segment that needs no gradient -- the real images of the GENERATOR step, whose
        features enter the feature-matching loss detached (sr_model.py:547-564).  The reference stacks it on N behind the
        generated images (sr_model.py:655-668); the discriminator has no batch statistics (InstanceNorm is per sample, SURVEY
        B-8), so running it as its own no-grad pass on the SAME weights of this forward (one spectral-norm power iteration) gives
        the same numbers and spares the backward pass the data gradients of a batch half whose upstream gradient is zero."""
        m0 = self.model0._modules["0"]
        mids = [c.weight(training) for c in self.convs()]
        ml = getattr(self, "model%d" % self.nl)._modules["0"]

        def run(x):
            outs = []
            x = ops.conv2d(x, m0.weight, m0.bias, stride=2, pad=2, act=L.ACT_LRELU)
            outs.append(x)
            for n in range(1, self.nl):
                x = self.norm_layers[n - 1].apply(self, x, mids[n - 1], L.ACT_LRELU, training,
                                                  stride=1 if n == self.nl - 1 else 2, pad=2)
                outs.append(x)
            outs.append(ops.conv2d(x, ml.weight, ml.bias, stride=1, pad=2))
            return outs
        if x_detached is None:
            return run(x)
        assert self.per_sample, "norm_D=%s has batch statistics: D must run once over cat([fake; real])" % self.norm
        with torch.no_grad():
            det = run(x_detached)
        return run(x), det


class MultiscaleDiscriminator(nn.Module):
    """discriminator.py:14-63."""

    def __init__(self, opt):
        super().__init__()
        self.num_d = opt.num_D
        self._sn = None
        for i in range(opt.num_D):
            self.add_module("discriminator_%d" % i, NLayerD(opt))

    @property
    def per_sample(self):
        return all(getattr(self, "discriminator_%d" % i).per_sample for i in range(self.num_d))

    def forward(self, x, training, x_detached=None):
        """Returns the per-scale feature lists; with `x_detached` a pair (features of x, features of x_detached): see NLayerD."""
        if self._sn is None:
            self._sn = ops.SNGroup([c for i in range(self.num_d) for c in getattr(self, "discriminator_%d" % i).convs()])
        self._sn.run(training)
        # the scales are independent given x (and its pooled copies): one branch per scale (ops.branches)
        xs, ds = [x], [x_detached]
        for i in range(1, self.num_d):
            xs.append(ops.AvgPool3s2.apply(xs[-1]))
            if x_detached is not None:
                with torch.no_grad():
                    ds.append(ops.AvgPool3s2.apply(ds[-1]))
            else:
                ds.append(None)
        # (tensors made on this stream that the side branches read, forward and backward: the pooled inputs and the
        # spectral-normalised weights W / sigma of this forward)
        shared = xs[1:] + [t for t in ds[1:] if t is not None] + list(self._sn.last)   # (SNGroup.last: the buffer all W / sigma are slices of + their maxima)
        res = ops.branches(*[(lambda i=i: getattr(self, "discriminator_%d" % i)(xs[i], training, ds[i])) for i in range(self.num_d)],
                           inputs=shared)
        if x_detached is None:
            return res
        return [r[0] for r in res], [r[1] for r in res]


# ------------------------------------------------------------------------------------ VGG19 perceptual taps
VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512]
VGG_TAPS = (1, 6, 11, 20, 29)
VGG_WEIGHTS = [1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0]


class VGG19Taps(nn.Module):
    """architecture.py:151-181 (frozen).  Keys follow torchvision's vgg19().features indices."""

    def __init__(self):
        super().__init__()
        self.features = Holder()
        cin, idx = 3, 0
        for v in VGG_CFG:
            if v == "M":
                idx += 1
                continue
            self.features.add_module(str(idx), ConvP(v, cin, 3))
            cin = v
            idx += 2
        for p in self.parameters():
            p.requires_grad = False
            p.dsee_frozen = True     # ops._frozen_cache: packed weights and their maxima are built once, not per forward

    def forward(self, x):
        feats, idx = [], 0
        for v in VGG_CFG:
            if v == "M":
                x = ops.MaxPool2.apply(x)
                idx += 1
                continue
            m = self.features._modules[str(idx)]
            x = ops.conv2d(x, m.weight, m.bias, act=L.ACT_RELU)
            if idx + 1 in VGG_TAPS:
                feats.append(x)
            idx += 2
        return feats
