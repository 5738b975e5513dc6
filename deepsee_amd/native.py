"""The generator forward through the C entry points alone: dsee_generator_prepare / dsee_generator_fwd (include/deepsee_hip.h).

SRModel mode "demo" -- LR image + label map + style matrix -> HR image -- for a host without this package's orchestration.  What
such a host needs from Python is here: the layout of the flat parameter buffer under the reference's state-dict keys (`layout`),
the buffer itself (`pack`), a file form of both (`NativeGenerator.export`: raw little-endian fp32 + JSON), and `NativeGenerator`,
which makes exactly the two calls a C host makes.  Nothing here computes: a configuration the library does not build (PureSEAN or
ResnetBlock kinds, InstanceNorm norm_G, the 16-bit mode, shapes off the tile rules) is described faithfully and refused by the
library with DSEE_EUNSUPPORTED.
"""
import ctypes as C
import json
import os

import torch

from . import lib as L
from . import networks as N

MAX_BLOCKS = 12                                   # DSEE_GEN_MAX_BLOCKS
KINDS = {"spade": 0, "sean": 1, "puresean": 2, "resnet": 3}        # DSEE_GEN_*
ALIGN = 64                                        # floats: every tensor of the flat buffer starts on a 256-byte boundary

_CONV_FIELDS = ("weight_orig", "bias", "weight_u", "weight_v")
# dsee_generator_norm field -> key below '<block>.norm_<i>.'
_NORM_KEYS = (("w_shared", "mlp_shared.0.weight"), ("b_shared", "mlp_shared.0.bias"),
              ("w_gamma", "mlp_gamma.weight"), ("b_gamma", "mlp_gamma.bias"),
              ("w_beta", "mlp_beta.weight"), ("b_beta", "mlp_beta.bias"),
              ("ws_gamma", "mlp_style_gamma.weight"), ("bs_gamma", "mlp_style_gamma.bias"),
              ("ws_beta", "mlp_style_beta.weight"), ("bs_beta", "mlp_style_beta.bias"),
              ("alpha_gamma", "alpha_gamma"), ("alpha_beta", "alpha_beta"),
              ("running_mean", "param_free_norm.running_mean"), ("running_var", "param_free_norm.running_var"))


class ConvDesc(C.Structure):
    _fields_ = [(k, C.c_int64) for k in _CONV_FIELDS]


class NormDesc(C.Structure):
    _fields_ = [(k, C.c_int64) for k, _ in _NORM_KEYS]


class BlockDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("ups", C.c_int32), ("conv_0", ConvDesc), ("conv_1", ConvDesc),
                ("norm_0", NormDesc), ("norm_1", NormDesc)]


class GeneratorDesc(C.Structure):
    """dsee_generator_desc"""
    _fields_ = [("C", C.c_int32), ("label_nc", C.c_int32), ("S", C.c_int32), ("max_fm_size", C.c_int32),
                ("n_blocks", C.c_int32), ("norm", C.c_int32), ("precision", C.c_int32), ("reserved_", C.c_int32),
                ("param_floats", C.c_int64), ("initial_w", C.c_int64), ("initial_b", C.c_int64),
                ("conv_img_w", C.c_int64), ("conv_img_b", C.c_int64), ("blocks", BlockDesc * MAX_BLOCKS)]

    @property
    def levels(self):
        return sum(int(self.blocks[i].ups != 0) for i in range(self.n_blocks))


def meta_of(opt):
    """The scalars and block list of the descriptor, as plain data (the "network" object of the exported JSON)."""
    from .sr_model import block_plan
    plan = block_plan(opt)
    if len(plan) > MAX_BLOCKS:
        raise ValueError("%d generator blocks: dsee_generator_desc holds %d" % (len(plan), MAX_BLOCKS))
    return {"C": 16 * opt.ngf, "label_nc": int(opt.semantic_nc), "S": int(opt.regional_style_size),
            "max_fm_size": int(opt.max_fm_size),
            "norm": {"batch": 0, "instance": 1}[N.param_free_norm_of(opt.norm_G)],
            "precision": 1 if getattr(opt, "precision", "fp32") == "fp16" else 0,
            "blocks": [{"name": nm, "kind": kind, "ups": int(nm == "G_middle_0" or nm.startswith("up_list."))}
                       for nm, kind in plan]}


def _tensors_of(meta):
    """[(state-dict key, shape)] the generator reads, in the order of the flat buffer.  Not read, hence not packed: the
    num_batches_tracked counters, style_conv (defined by the reference, never used), the NoiseInjection weights (training only)."""
    c, nc, s, nh = meta["C"], meta["label_nc"], meta["S"], N.NHIDDEN
    out = [("initial.weight", (c, 3, 3, 3)), ("initial.bias", (c,))]
    for b in meta["blocks"]:
        p, kind = b["name"], b["kind"]
        if kind == "resnet":
            continue              # (conv_block.* keys: described by its kind alone, the library refuses it)
        for cv in ("conv_0", "conv_1"):
            out += [("%s.%s.bias" % (p, cv), (c,)), ("%s.%s.weight_orig" % (p, cv), (c, c, 3, 3)),
                    ("%s.%s.weight_u" % (p, cv), (c,)), ("%s.%s.weight_v" % (p, cv), (9 * c,))]
        for nm in ("norm_0", "norm_1"):
            q = "%s.%s." % (p, nm)
            if meta["norm"] == 0:
                out += [(q + "param_free_norm.running_mean", (c,)), (q + "param_free_norm.running_var", (c,))]
            out += [(q + "mlp_shared.0.weight", (nh, nc, 3, 3)), (q + "mlp_shared.0.bias", (nh,))]
            if kind in ("spade", "sean"):
                out += [(q + "mlp_gamma.weight", (c, nh, 3, 3)), (q + "mlp_gamma.bias", (c,)),
                        (q + "mlp_beta.weight", (c, nh, 3, 3)), (q + "mlp_beta.bias", (c,))]
            if kind in ("sean", "puresean"):
                out += [(q + "mlp_style_gamma.weight", (c, s, 3, 3)), (q + "mlp_style_gamma.bias", (c,)),
                        (q + "mlp_style_beta.weight", (c, s, 3, 3)), (q + "mlp_style_beta.bias", (c,))]
            if kind == "sean":
                out += [(q + "alpha_beta", (1,)), (q + "alpha_gamma", (1,))]
    return out + [("conv_img.weight", (3, c, 3, 3)), ("conv_img.bias", (3,))]


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _desc_of(meta, entries, total):
    """The filled dsee_generator_desc of a block list and an offset table [(key, offset, shape)]."""
    off = {k: o for k, o, _ in entries}
    d = GeneratorDesc()
    d.C, d.label_nc, d.S, d.max_fm_size = meta["C"], meta["label_nc"], meta["S"], meta["max_fm_size"]
    d.n_blocks, d.norm, d.precision, d.param_floats = len(meta["blocks"]), meta["norm"], meta["precision"], total
    d.initial_w, d.initial_b = off["initial.weight"], off["initial.bias"]
    d.conv_img_w, d.conv_img_b = off["conv_img.weight"], off["conv_img.bias"]
    for i, b in enumerate(meta["blocks"]):
        blk = d.blocks[i]
        blk.kind, blk.ups = KINDS[b["kind"]], b["ups"]
        for cv in ("conv_0", "conv_1"):
            for f in _CONV_FIELDS:
                setattr(getattr(blk, cv), f, off.get("%s.%s.%s" % (b["name"], cv, f), -1))
        for nm in ("norm_0", "norm_1"):
            for f, key in _NORM_KEYS:
                setattr(getattr(blk, nm), f, off.get("%s.%s.%s" % (b["name"], nm, key), -1))
    return d


def _layout_of(meta):
    entries, o = [], 0
    for key, shape in _tensors_of(meta):
        entries.append((key, o, tuple(shape)))
        o += (_numel(shape) + ALIGN - 1) // ALIGN * ALIGN
    return entries, _desc_of(meta, entries, o)


def layout(opt):
    """(entries, desc): entries = the ordered [(state-dict key, offset in floats, shape)] of the flat parameter buffer, keys as
    SRModel.save writes them ({epoch}_net_SR.pth); desc = the filled GeneratorDesc (dsee_generator_desc) that goes with it."""
    return _layout_of(meta_of(opt))


def _pack(state_dict, entries, total, device="cuda"):
    flat = torch.zeros(total, dtype=torch.float32)
    for key, o, shape in entries:
        t = state_dict[key].detach().to("cpu", torch.float32)
        if t.numel() != _numel(shape):
            raise ValueError("%s: %s in the state dict, %s in the layout" % (key, list(t.shape), list(shape)))
        flat[o:o + t.numel()] = t.reshape(-1)
    return flat.to(device)


def pack(state_dict, opt, device="cuda"):
    """The flat fp32 device tensor of layout(opt), filled from a state dict of the SR network (reference keys); the gaps between
    the 256-byte aligned tensors are zero."""
    entries, desc = layout(opt)
    return _pack(state_dict, entries, int(desc.param_floats), device)


class NativeGenerator:
    """`demo` through the C ABI: prepare() once per checkpoint, then __call__ per batch.  Calls nothing but dsee_generator_prepare
    and dsee_generator_fwd (through lib.call, on the current stream) and the two host-side size queries."""

    def __init__(self, opt, state_dict, _parts=None):
        if _parts is None:
            self.meta = meta_of(opt)
            self.entries, self.desc = _layout_of(self.meta)
            self.params = _pack(state_dict, self.entries, int(self.desc.param_floats))
        else:
            self.meta, self.entries, self.desc, self.params = _parts
        d = self.desc
        self.prepared_bytes = int(L.lib().dsee_generator_prepared_bytes(d.C, d.label_nc, d.S, d.n_blocks))
        self.prepared = None
        self._ws = {}

    @classmethod
    def from_export(cls, path):
        """The generator of a file pair written by export(): `path` (raw little-endian fp32) and `path`.json."""
        import numpy as np
        with open(path + ".json") as f:
            doc = json.load(f)
        meta = doc["network"]
        entries = [(t["key"], int(t["offset"]), tuple(t["shape"])) for t in doc["tensors"]]
        total = int(doc["param_floats"])
        flat = torch.from_numpy(np.fromfile(path, dtype="<f4").astype("float32"))
        if flat.numel() != total:
            raise ValueError("%s holds %d floats, %s.json says %d" % (path, flat.numel(), path, total))
        return cls(None, None, _parts=(meta, entries, _desc_of(meta, entries, total), flat.cuda()))

    def prepare(self):
        """Everything that depends on the weights only, into a buffer this object owns (again after the parameters changed)."""
        if self.prepared is None:
            self.prepared = torch.empty((self.prepared_bytes + 3) // 4, dtype=torch.float32, device="cuda")
        L.call("generator_prepare", C.byref(self.desc), self.params, self.prepared, self.prepared_bytes)
        return self

    def workspace_bytes(self, n, h, w):
        d = self.desc
        return int(L.lib().dsee_generator_fwd_workspace(d.C, d.label_nc, d.levels, n, h, w))

    def __call__(self, image_lr, labels_u8, style, out=None, workspace=None):
        """image_lr [N,3,h,w] NCHW fp32 in [-1, 1], labels_u8 [N,H,W] uint8 class map at the HR resolution, style [N,label_nc,S]
        -> fake_image [N,3,H,W].  `out` / `workspace` (fp32 tensors): caller-owned buffers, e.g. the static ones of a captured
        graph; by default the output is fresh and the workspace kept per shape."""
        if self.prepared is None:
            self.prepare()
        n, _, h, w = image_lr.shape
        lv = self.desc.levels
        if out is None:
            out = torch.empty(n, 3, h << lv, w << lv, dtype=torch.float32, device="cuda")
        nbytes = self.workspace_bytes(n, h, w)
        if workspace is None:
            workspace = self._ws.get((n, h, w))
            if workspace is None:
                self._ws.clear()
                workspace = self._ws[(n, h, w)] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device="cuda")
        L.call("generator_fwd", C.byref(self.desc), self.params, self.prepared, self.prepared_bytes, image_lr, labels_u8,
               labels_u8.shape[1], labels_u8.shape[2], style, out, n, h, w, workspace, workspace.numel() * 4)
        return out

    def export(self, path):
        """Write the flat buffer as raw little-endian fp32 to `path` and its description to `path`.json: "network" (the scalars of
        dsee_generator_desc and per block name / kind / ups), "tensors" ([{key, offset, shape}], offsets in floats) and
        "param_floats".  A C host maps the file, uploads it in one copy and fills the struct from the JSON."""
        self.params.cpu().numpy().astype("<f4").tofile(path)
        doc = {"network": self.meta, "param_floats": int(self.desc.param_floats),
               "tensors": [{"key": k, "offset": o, "shape": list(s)} for k, o, s in self.entries]}
        tmp = "%s.json.tmp.%d" % (path, os.getpid())
        with open(tmp, "w") as f:
            json.dump(doc, f, indent=1)
        os.replace(tmp, path + ".json")
