"""Explorative inference: the modes of SRModel.forward that vary the regional style matrix of a batch and return the family of
HR images (sr_model.py:219-444 of the reference).

The reference loops over (image b, variant k), edits one style matrix and runs the generator at batch 1, B * n times.  In eval
mode every layer of the generator is per image (running BatchNorm statistics, InstanceNorm, no noise), so one pass over all
pairs computes the same images; here

  * style_variants (dsee_style_explore) writes the B * n style matrices in one launch,
  * run_pairs runs the generator over the pairs i = b * n + k in passes of at most opt.explore_chunk pairs (the LR image and
    the label map of pair i are those of image i // n), and
  * assemble (dsee_nhwc_to_nchw_tiled) puts each pass's native output where the reference's torch.cat(fake_samples, -1) /
    torch.stack(fake_samples, 1) would: [B, 3, H, n * W] or, with opt.dont_merge_fake, [B, n, 3, H, W].

Every mode is one rule  out[b][k][r] = clamp(alpha_k * A + beta_k * s1[src1[b][k]][r] + gamma_k (+ noise))  on the rows r of
opt.region_idx and A elsewhere, with A = s0[src0[b][k]][r] -- or the previous variant's row where the reference aliases its
working copy (`recurrent`).  variants() holds the per-mode coefficients; style_variants_torch is the rule in plain torch ops,
the readable specification the kernel is tested against bit for bit.

The modes the reference cannot run, or runs with an unpinned random draw inside the encoder (inference_noise,
inference_multi_modal, inference_replace_semantics, inference_reference_semantics), are not here: SRModel.forward refuses them.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

MODES = ("inference_interpolation", "inference_interpolation_style", "inference_particular_combined",
         "inference_particular_full", "inference_reference", "inference_reference_interpolation")
ODD_MESSAGE = "Please use an odd n such that the middle image has delta=0"
# inference_particular_combined: after the noise, the rows CONSISTENT_TO take the rows CONSISTENT_FROM (sr_model.py:314-317)
CONSISTENT_TO, CONSISTENT_FROM = (4, 6, 8, 11), (5, 7, 9, 12)


def region_mask(region_idx, nc):
    """opt.region_idx -> bool [nc]; None or empty means every row (sr_model.py:230)."""
    mask = torch.zeros(nc, dtype=torch.bool)
    mask[list(region_idx) if region_idx else list(range(nc))] = True
    return mask


def _f32(values):
    """float64 host values -> fp32, rounded once (what `tensor + np.float64` does with the scalar)."""
    return torch.from_numpy(np.asarray(values, dtype=np.float64)).to(torch.float32)


def variants(mode, opt, B, nc):
    """The coefficients of `mode` for a batch of B: dict(n, src0, src1 [B][n] int64, alpha, beta, gamma [n] fp32, mask bool [nc],
    clamp, recurrent).  Host only."""
    assert mode in MODES, mode
    rows = torch.arange(B)[:, None]
    region = region_mask(getattr(opt, "region_idx", None), nc)
    everything = torch.ones(nc, dtype=torch.bool)
    clamp, recurrent = True, False
    if mode == "inference_interpolation":
        n = int(opt.n_interpolation)
        assert n % 2 == 1, ODD_MESSAGE
        src0 = src1 = rows.expand(B, n)
        alpha, beta, gamma = torch.ones(n), torch.zeros(n), _f32(np.linspace(-opt.noise_delta, opt.noise_delta, num=n))
        mask = region
    elif mode == "inference_interpolation_style":
        n = int(opt.n_interpolation)
        assert n % 2 == 1, ODD_MESSAGE
        t = np.linspace(0, 1, num=n)
        src0 = src1 = rows.expand(B, n)
        alpha, beta, gamma, mask, clamp = _f32(1 - t), _f32(t), torch.zeros(n), everything, False
    elif mode == "inference_particular_combined":
        # s + noise, clamped, on the region rows when noise_delta > 0; the encoded style as it is otherwise
        n = 1
        src0 = src1 = rows.expand(B, n)
        alpha, beta, gamma = torch.ones(n), torch.zeros(n), torch.zeros(n)
        mask = region if opt.noise_delta > 0 else torch.zeros(nc, dtype=torch.bool)
    elif mode == "inference_particular_full":
        # variant 0: the style of the HR image (s0), variant 1: the style of the guiding image (s1)
        n = 2
        src0 = src1 = rows.expand(B, n)
        alpha, beta, gamma, mask, clamp = torch.tensor([1.0, 0.0]), torch.tensor([0.0, 1.0]), torch.zeros(n), everything, False
    elif mode == "inference_reference":
        n = B
        src0, src1 = rows.expand(B, n), torch.arange(n)[None, :].expand(B, n)
        alpha, beta, gamma, mask = torch.zeros(n), torch.ones(n), torch.zeros(n), region
    else:    # inference_reference_interpolation: s1 is the style set times opt.manipulate_scale
        n = int(opt.n_interpolation)
        t = np.linspace(0, 1, num=n)
        src0, src1 = rows.expand(B, n), ((rows + 1) % B).expand(B, n)
        alpha, beta, gamma, mask, recurrent = _f32(1 - t), _f32(t), torch.zeros(n), region, True
    return dict(n=n, src0=src0.contiguous(), src1=src1.contiguous(), alpha=alpha.float(), beta=beta.float(),
                gamma=gamma.float(), mask=mask, clamp=clamp, recurrent=recurrent)


def style_variants_torch(s0, s1, src0, src1, alpha, beta, gamma, noise, mask, clamp, recurrent):
    """The rule of dsee_style_explore in torch ops, one fp32 rounding each (runs wherever its inputs live, the CPU included):
    s0, s1 [B, nc, S]; src0, src1 [B, n] integer rows of the batch; alpha, beta, gamma [n] fp32; noise [B, n, nc, S] or None;
    mask [nc] -> [B, n, nc, S]."""
    n = src0.shape[1]
    src0, src1 = src0.long().to(s0.device), src1.long().to(s0.device)
    alpha, beta, gamma = (c.to(s0.device, torch.float32) for c in (alpha, beta, gamma))
    mask = mask.to(s0.device).bool()[None, :, None]
    out, prev = [], None
    for k in range(n):
        a = prev if (recurrent and k > 0) else s0[src0[:, k]]
        v = alpha[k] * a + beta[k] * s1[src1[:, k]]
        v = v + gamma[k]
        if noise is not None:
            v = v + noise[:, k]
        if clamp:
            v = v.clamp(-1, 1)
        prev = torch.where(mask, v, a)
        out.append(prev)
    return torch.stack(out, 1)


def style_variants(s0, s1, src0, src1, alpha, beta, gamma, noise, mask, clamp, recurrent, out=None):
    """dsee_style_explore: as style_variants_torch, on device tensors s0, s1 (and noise); the index and coefficient tables may
    live on the host.  `out`: a contiguous fp32 [B, n, nc, S] device tensor to write (allocated when not given)."""
    from . import lib as L
    B, nc, S = s0.shape
    n = src0.shape[1]
    assert s0.is_cuda and s0.dtype == torch.float32 and s1.shape == s0.shape and s1.dtype == torch.float32
    assert tuple(src0.shape) == tuple(src1.shape) == (B, n) and all(tuple(c.shape) == (n,) for c in (alpha, beta, gamma))
    assert 0 <= int(src0.min()) and int(src0.max()) < B and 0 <= int(src1.min()) and int(src1.max()) < B, "rows of the batch"
    assert tuple(mask.shape) == (nc,)
    if noise is not None:
        assert tuple(noise.shape) == (B, n, nc, S) and noise.dtype == torch.float32 and noise.is_cuda
        noise = noise.contiguous()
    dev = s0.device
    idx = torch.stack([src0, src1]).to(torch.int32).contiguous().to(dev)
    coef = torch.stack([alpha, beta, gamma]).to(torch.float32).contiguous().to(dev)
    if out is None:
        out = torch.empty(B, n, nc, S, dtype=torch.float32, device=dev)
    assert tuple(out.shape) == (B, n, nc, S) and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    L.call("style_explore", s0.contiguous(), s1.contiguous(), idx[0], idx[1], coef[0], coef[1], coef[2], noise,
           mask.to(torch.uint8).contiguous().to(dev), out, B, n, nc, S, int(bool(clamp)), int(bool(recurrent)))
    return out


def noise_rows(opt, nc):
    """The style rows inference_particular_combined draws noise for, in the order of the drawn tensor's rows."""
    return list(opt.region_idx) if opt.region_idx else list(range(nc))


def build_styles(mode, opt, s0, s1=None, drawn=None, rule=style_variants_torch):
    """The style matrices [B, n, nc, S] of `mode` from its encoded style set(s): s0 (and s1: style_to of
    inference_interpolation_style, the guiding image's styles of inference_particular_full), `drawn` the noise
    [B, len(noise_rows), S] of inference_particular_combined.  `rule`: style_variants_torch or style_variants."""
    B, nc, S = s0.shape
    v = variants(mode, opt, B, nc)
    if mode == "inference_reference_interpolation":
        s1 = s0 * opt.manipulate_scale
    noise = None
    if drawn is not None:
        noise = torch.zeros(B, 1, nc, S, dtype=torch.float32, device=s0.device)
        noise[:, 0, noise_rows(opt, nc)] = drawn.to(s0.device)
    styles = rule(s0, s0 if s1 is None else s1, v["src0"], v["src1"], v["alpha"], v["beta"], v["gamma"], noise, v["mask"],
                  v["clamp"], v["recurrent"])
    if drawn is not None:
        styles[:, :, list(CONSISTENT_TO)] = styles[:, :, list(CONSISTENT_FROM)]
    return styles


def assemble(fake_nhwc, B, n, merge, out=None, pair0=0):
    """dsee_nhwc_to_nchw_tiled: the generator's native output for the pairs pair0 .. pair0 + len(fake_nhwc) - 1 (pair i = image
    i // n, variant i % n) into `out` -- [B, 3, H, n * W] (merge) or [B, n, 3, H, W] -- which is allocated when not given."""
    from . import lib as L
    pairs, h, w, cs = fake_nhwc.shape
    shape = (B, 3, h, n * w) if merge else (B, n, 3, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=fake_nhwc.device)
    assert tuple(out.shape) == shape and out.dtype == torch.float32 and out.is_contiguous() and fake_nhwc.dtype == torch.float32
    L.call("nhwc_to_nchw_tiled", fake_nhwc.contiguous(), out, B, n, h, w, cs, int(bool(merge)), pair0, pairs)
    return out


def run_pairs(model, d, styles, chunk):
    """The generator, in eval mode, over the pairs of styles [B, n, nc, S] in passes of at most `chunk` pairs; yields (first pair,
    native output [pairs, H, W, cs]) per pass.  A pass may straddle images: the LR image and the label map of a pair are
    gathered per pass (LR-sized and uint8 data; nothing of the size of an HR activation is copied)."""
    from . import ops
    B, n = styles.shape[:2]
    flat = styles.reshape(B * n, styles.shape[2], styles.shape[3])
    lr, labels = d["image_lr"], d["labels"]
    chunk = max(1, int(chunk))
    for p0 in range(0, B * n, chunk):
        p1 = min(B * n, p0 + chunk)
        if n == 1 and p0 == 0 and p1 == B:
            x, lab = lr, labels
        else:
            idx = (torch.arange(p0, p1, device=lr.device) // n)
            x, lab = lr.index_select(0, idx), ops.Labels(labels.t.index_select(0, idx), labels.nc)
        yield p0, model.netSR(x, lab, flat[p0:p1].contiguous(), model.noise, False)


def generate(model, d, styles, merge, u8=False):
    """styles [B, n, nc, S] -> the result tensor of assemble() over all pairs (and its uint8 strips [B, H, n * W, 3])."""
    B, n = styles.shape[:2]
    out = None
    for p0, fake in run_pairs(model, d, styles, getattr(model.opt, "explore_chunk", 8)):
        out = assemble(fake, B, n, merge, out, p0)
    return (out, strips_u8(out)) if u8 else (out, None)


def strips_u8(fake):
    """[B, 3, H, n * W] or [B, n, 3, H, W] fp32 -> uint8 [B, H, n * W, 3] on the device, tensor2im's arithmetic."""
    from . import visuals as V
    if fake.dim() == 4:
        B, _, h, wide = fake.shape
        buf, win = V.packed(B, h, wide, fake.device)
        V.image_to_u8(fake, win)
    else:
        B, n, _, h, w = fake.shape
        buf, _ = V.packed(B, h, n * w, fake.device)
        for k in range(n):      # variant k is the k-th column of every strip
            V.image_to_u8(fake[:, k].contiguous(), V.Window(buf, 0, h * n * w * 3, n * w * 3, k * w))
        wide = n * w
    return buf.view(B, h, wide, 3)


def save_strips(out, paths, folder_out):
    """<folder_out>/fake_image/<name>.png per input image: its variants side by side.  `out`: what SRModel.forward returned for
    an explorative mode (its fake_image_u8 if it was asked for with u8=True).  Returns when the files are written."""
    from . import visuals as V
    u8 = out.get("fake_image_u8")
    if u8 is None:
        u8 = strips_u8(out["fake_image"] if "fake_image" in out else out["fake_image_original"])
    assert len(paths) == u8.shape[0], "%d paths for a batch of %d" % (len(paths), u8.shape[0])
    images = u8.cpu().numpy()
    os.makedirs(os.path.join(folder_out, "fake_image"), exist_ok=True)
    for b, path in enumerate(paths):
        V.save_image(images[b], os.path.join(folder_out, "fake_image", V._file_name(path)))


# ------------------------------------------------------------------------------------------------ the modes
def _style_inputs(d, guiding):
    return (d["guiding_image"], d["guiding_labels"]) if guiding else (d["image_hr"], d["labels"])


def forward(model, data, d, mode, u8=False):
    """SRModel.forward for mode in MODES.  data: the caller's dict, d: its native form (SRModel._native)."""
    opt = model.opt
    guided, guiding = model.model_variant == "guided", bool(opt.guiding_style_image)
    if mode == "inference_particular_combined" and guided:
        raise ValueError("%s needs the mini encoder of the independent model" % mode)
    if mode == "inference_particular_full" and not guiding:
        raise ValueError("%s needs opt.guiding_style_image" % mode)
    if mode == "inference_reference_interpolation" and guiding:
        raise ValueError("%s cannot run with opt.guiding_style_image" % mode)
    if mode in ("inference_interpolation", "inference_interpolation_style"):
        assert int(opt.n_interpolation) % 2 == 1, ODD_MESSAGE
    extra = OrderedDict()
    if guiding:     # (read first: a missing id is a KeyError before any kernel runs)
        extra["guiding_image_id"] = data["guiding_image_id"]
        extra["guiding_image"] = data.get("guiding_image")
        extra["guiding_input_label"] = data.get("guiding_label")
    with torch.no_grad():
        # ---- the style sets
        s1 = None
        if mode == "inference_interpolation":
            if "style_matrix" in data:
                s0 = data["style_matrix"].to("cuda", torch.float32).contiguous()
            elif guided:
                s0 = model.encode_with("full", *_style_inputs(d, guiding))
            else:
                s0 = model.encode_with("mini", d["image_lr"], d["labels"])
        elif mode == "inference_interpolation_style":
            s0 = data["style_from"].to("cuda", torch.float32).contiguous()
            s1 = data["style_to"].to("cuda", torch.float32).contiguous()
        elif mode == "inference_particular_combined":
            s0 = model.encode_with("mini", d["image_lr"], d["labels"])
        elif mode == "inference_particular_full":
            s0 = model.encode_with("full", d["image_hr"], d["labels"])
            s1 = model.encode_with("full", d["guiding_image"], d["guiding_labels"])
        else:
            s0 = model.encode_with("full", *_style_inputs(d, guiding))
        B, nc, S = s0.shape
        drawn = None
        if mode == "inference_particular_combined" and opt.noise_delta > 0:
            drawn = model.get_noise((B, len(noise_rows(opt, nc)), S), opt.noise_delta)
        styles = build_styles(mode, opt, s0, s1, drawn, style_variants)
        # ---- the generator over all pairs, and the result tensor
        particular = mode.startswith("inference_particular")
        stacked = particular or (bool(opt.dont_merge_fake) and mode in ("inference_interpolation", "inference_interpolation_style"))
        fake, strips = generate(model, d, styles, not stacked, u8)
    out = OrderedDict([("input_label", data.get("input_semantics")), ("image_downsized", data.get("image_lr"))])
    if particular:
        out["fake_image_original"] = fake[:, 0]
        out["image_full"] = data.get("image_hr")
        if mode == "inference_particular_full":
            out["fake_image_guiding"] = fake[:, 1]
    else:
        out["fake_image"] = fake
        out["image_full"] = data.get("image_hr")
        if mode in ("inference_interpolation", "inference_interpolation_style"):
            out["style"] = [styles[b] for b in range(B)] if stacked else []
    out.update(extra)
    if u8:
        out["fake_image_u8"] = strips
    return out
