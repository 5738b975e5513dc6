"""Rectangular (H != W) shapes for the kernels that had no harness to generalise: the label-map kernels through the C ABI and the
streaming kernels through their autograd functions, against plain float64 torch on the CPU (the StylePool case against the oracle,
which tests/test_rect_host.py pins at these shapes).  Both orientations wherever a swapped index could hide in one of them."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import deepsee_oracle as O

pytestmark = pytest.mark.gpu

TOL = 2e-5
CO = 128      # nhidden of mlp_shared: the only width the one-hot weight gradient is built for


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-20))


def nhwc(x):
    from deepsee_amd import ops
    return ops.to_nhwc(x.cuda())


def nchw(x, c):
    from deepsee_amd import ops
    return ops.to_nchw(x.contiguous(), c).cpu()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------ one-hot 3x3 convolution (label.hip)
# name: (N, label H, label W, shift) -- the three kernels of dsee_onehot_conv3x3_fwd: below 4096 output pixels the plain kernel,
# from 4096 the LDS-table kernels, four pixels of a row per thread when the output width is a multiple of 4, else one
ONEHOT_SHAPES = {"plain_12x20": (2, 24, 40, 1), "lds4_48x96": (2, 48, 96, 0), "lds_46x50": (2, 46, 50, 0)}


@functools.lru_cache(maxsize=None)
def _onehot_case(name, nl):
    """label map, weights and the float64 reference of ReLU-less conv3x3(one-hot) with its autograd through a ReLU; built once per
    (shape, class count) and shared by the forward and the weight-gradient tests (never modified)."""
    n, h, w, shift = ONEHOT_SHAPES[name]
    g = gen(h * w + nl)
    lab = torch.randint(0, nl, (n, 1, h, w), generator=g)
    lab[:, :, : h // 3, : w // 4] = 5                                   # a region: neighbouring taps read equal labels there
    wt = (torch.randn(CO, nl, 3, 3, generator=g) * 0.3).double().requires_grad_()
    b = (torch.randn(CO, generator=g) * 0.2).double().requires_grad_()
    seg = torch.zeros(n, nl, h, w, dtype=torch.float64).scatter_(1, lab, 1.0)
    if shift:
        seg = F.interpolate(seg, size=(h >> shift, w >> shift), mode="nearest")
    pre = F.conv2d(seg, wt, b, padding=1)
    act = F.relu(pre)
    dact = torch.randn(act.shape, generator=g).double()
    act.backward(dact)
    return {"lab": lab.to(torch.uint8)[:, 0].contiguous(), "w": wt.detach().float(), "b": b.detach().float(), "seg": seg,
            "pre": pre.detach(), "act": act.detach(), "dact": dact, "dw": wt.grad, "db": b.grad}


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("name", sorted(ONEHOT_SHAPES))
def test_onehot_conv3x3_fwd(name, relu):
    """dsee_onehot_conv3x3_fwd, all three kernels, on maps with H != W: values against F.conv2d of the scattered one-hot in float64
    (2e-5); with onehot_coff >= 0 the 32 extra columns equal dsee_label_onehot bit for bit (and the float64 one-hot); amax
    equals max(amax_floor, max |stored values|); the 128-column form without the extras writes the same bits."""
    from deepsee_amd import lib as L
    n, h, w, shift = ONEHOT_SHAPES[name]
    nl, r, rw = 19, h >> shift, w >> shift
    m = n * r * rw
    assert {"plain": m < 4096, "lds4": m >= 4096 and rw % 4 == 0, "lds": m >= 4096 and rw % 4 != 0}[name.split("_")[0]]
    ref = _onehot_case(name, nl)
    want = (ref["act"] if relu else ref["pre"]).permute(0, 2, 3, 1)
    lab = ref["lab"].cuda()
    table = torch.empty(9, nl, CO, device="cuda")
    L.call("onehot_conv3x3_pack", ref["w"].cuda(), table, CO, nl)
    bias = ref["b"].cuda()
    ld = CO + 32
    for floor in (0.0, 1000.0):
        out = torch.full((n, r, rw, ld), float("nan"), device="cuda")
        amax = torch.zeros(2048, device="cuda")
        L.call("onehot_conv3x3_fwd", lab, table, bias, out, n, h, w, shift, nl, CO, ld, 0, relu, CO, amax, floor)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        assert float(amax.max()) == max(floor, float(out[..., :CO].abs().max())), (floor, float(amax.max()))
    err = rel(out[..., :CO].cpu(), want)
    print("one-hot conv forward %s relu=%d (%d pixels): %.2e" % (name, relu, m, err))
    assert err < TOL
    oh = torch.full((n, r, rw, 32), float("nan"), device="cuda")
    L.call("label_onehot", lab, oh, n, h, w, shift, 32, 0)
    plain = torch.full((n, r, rw, CO), float("nan"), device="cuda")
    L.call("onehot_conv3x3_fwd", lab, table, bias, plain, n, h, w, shift, nl, CO, CO, 0, relu, -1, None, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(out[..., CO:], oh)
    assert torch.equal(oh[..., :nl].cpu().double(), ref["seg"].permute(0, 2, 3, 1)) and float(oh[..., nl:].abs().max()) == 0.0
    assert torch.equal(plain, out[..., :CO].contiguous())


@pytest.mark.parametrize("nl", [19, 27])
@pytest.mark.parametrize("name", sorted(ONEHOT_SHAPES))
def test_onehot_conv3x3_wgrad(name, nl):
    """dsee_onehot_conv3x3_wgrad (register accumulators for 20 classes, 32 from 21) at the same three shapes against autograd of
    ReLU(conv3x3(one-hot)) in float64; the ReLU mask comes from the reference activation, so no branch decision differs."""
    from deepsee_amd import lib as L
    n, h, w, shift = ONEHOT_SHAPES[name]
    ref = _onehot_case(name, nl)
    lab = ref["lab"].cuda()
    act = ref["act"].permute(0, 2, 3, 1).float().contiguous().cuda()
    assert bool(((act > 0).cpu() == (ref["act"].permute(0, 2, 3, 1) > 0)).all())
    dact = ref["dact"].permute(0, 2, 3, 1).float().contiguous().cuda()
    dw, db = torch.full((CO, nl, 3, 3), float("nan"), device="cuda"), torch.full((CO,), float("nan"), device="cuda")
    ws = torch.empty(L.lib().dsee_onehot_conv3x3_wgrad_workspace(n, h, w, shift, nl) // 4, device="cuda")
    L.call("onehot_conv3x3_wgrad", lab, dact, CO, act, CO, n, h, w, shift, nl, dw, db, ws)
    torch.cuda.synchronize()
    e_w, e_b = rel(dw.cpu(), ref["dw"]), rel(db.cpu(), ref["db"])
    print("one-hot conv weight gradient %s L=%d: dw %.2e db %.2e" % (name, nl, e_w, e_b))
    assert e_w < 5 * TOL and e_b < 5 * TOL


@pytest.mark.parametrize("lh,lw,fh,fw", [(32, 64, 16, 32), (64, 32, 64, 32)])
def test_style_pool_rect(lh, lw, fh, fw):
    """dsee_label_segsum / dsee_label_gather through ops.StylePool (forward / backward) with the label map at 2x and 1x the
    feature map, against the oracle's style_pool."""
    from deepsee_amd import ops
    g = gen(lh + fw)
    n, c = 2, 128
    label = torch.randint(0, 19, (n, 1, lh, lw), generator=g).float()
    seg = O.onehot_labels(label, 19, torch.float64)
    f = torch.randn(n, c, fh, fw, generator=g).double().requires_grad_()
    s = O.style_pool(f, seg)
    gs = torch.randn(s.shape, generator=g)
    s.backward(gs.double())
    labels = ops.Labels(ops.label_to_u8(label.cuda()), 19)
    fs = nhwc(f.detach().float()).requires_grad_()
    sd = ops.StylePool.apply(fs, labels, labels.shift_for(fh, fw))
    sd.backward(gs.cuda())
    torch.cuda.synchronize()
    e_s, e_f = rel(sd.detach().cpu(), s.detach()), rel(nchw(fs.grad, c), f.grad)
    print("style pool labels %dx%d features %dx%d: s %.2e df %.2e" % (lh, lw, fh, fw, e_s, e_f))
    assert e_s < TOL and e_f < TOL
    with pytest.raises(AssertionError):       # a feature map that is not the same fraction on both axes is refused
        labels.shift_for(fh, fh)


# ------------------------------------------------------------------------------------ streaming kernels (elementwise.hip, norm.hip)
@pytest.mark.parametrize("c,h,w", [(16, 5, 7), (24, 7, 5)])
def test_upnoise_rect(c, h, w):
    """ops.UpNoise (nearest x2 + noise): with a materialised eps against the formula in float64, and with the Philox stream
    (indexed in NHWC element order) against its own materialize().  C = 24: C / 4 = 6 does not divide 256, so the backward runs the
    separate dsee_sumpool_amax + dsee_channel_dot_rng passes instead of dsee_sumpool_dot_rng."""
    from deepsee_amd import ops
    g = gen(c + h)
    n = 2
    x = torch.randn(n, c, h, w, generator=g).double().requires_grad_()
    nw = torch.randn(c, generator=g).double().requires_grad_()
    eps = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    y = F.interpolate(x, scale_factor=2, mode="nearest") + nw[None, :, None, None] * eps.double()
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    xs, ws = nhwc(x.detach().float()).requires_grad_(), nw.detach().float().cuda().requires_grad_()
    ys = ops.UpNoise.apply(xs, ws, nhwc(eps), 1)
    ys.backward(nhwc(gy))
    errs = (rel(nchw(ys.detach(), c), y.detach()), rel(nchw(xs.grad, c), x.grad), rel(ws.grad.cpu(), nw.grad))
    print("UpNoise %dx%d C=%d: y %.2e dx %.2e dw %.2e" % ((h, w, c) + errs))
    assert max(errs) < TOL
    tok = ops.PhiloxNormal((n, 2 * h, 2 * w, c), seed=77, offset=1234)
    xa, wa = xs.detach().clone().requires_grad_(), ws.detach().clone().requires_grad_()
    xb, wb = xs.detach().clone().requires_grad_(), ws.detach().clone().requires_grad_()
    ya = ops.UpNoise.apply(xa, wa, tok, 1)
    yb = ops.UpNoise.apply(xb, wb, tok.materialize(), 1)
    ya.backward(nhwc(gy))
    yb.backward(nhwc(gy))
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    print("... Philox stream vs materialised: dw %.2e" % rel(wa.grad.cpu(), wb.grad.cpu()))
    assert rel(wa.grad.cpu(), wb.grad.cpu()) < 1e-6


@pytest.mark.parametrize("h,w", [(17, 12), (12, 17)])
def test_avgpool3s2_rect(h, w):
    """ops.AvgPool3s2 (count_include_pad=False): an odd and an even size, so the border counts differ per axis."""
    from deepsee_amd import ops
    g = gen(h)
    x = torch.randn(2, 24, h, w, generator=g).double().requires_grad_()
    y = F.avg_pool2d(x, 3, 2, [1, 1], count_include_pad=False)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    xs = nhwc(x.detach().float()).requires_grad_()
    ys = ops.AvgPool3s2.apply(xs)
    assert tuple(ys.shape[1:3]) == tuple(y.shape[2:])
    ys.backward(nhwc(gy))
    errs = (rel(nchw(ys.detach(), 24), y.detach()), rel(nchw(xs.grad, 24), x.grad))
    print("AvgPool3s2 %dx%d: y %.2e dx %.2e" % ((h, w) + errs))
    assert max(errs) < TOL


def test_maxpool2_rect():
    from deepsee_amd import ops
    g = gen(23)
    x = F.relu(torch.randn(2, 8, 6, 10, generator=g)).requires_grad_()  # ties at 0 like VGG after ReLU
    y = F.max_pool2d(x, 2, 2)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    xs = nhwc(x.detach()).requires_grad_()
    ys = ops.MaxPool2.apply(xs)
    ys.backward(nhwc(gy))
    assert rel(nchw(ys.detach(), 8), y.detach()) == 0.0
    assert rel(nchw(xs.grad, 8), x.grad) == 0.0


def test_dinput_rect():
    from deepsee_amd import ops
    g = gen(29)
    n, h, w = 2, 24, 40
    label = torch.randint(0, 19, (n, 1, h, w), generator=g).float()
    labels = ops.Labels(ops.label_to_u8(label.cuda()), 19)
    assert torch.equal(labels.t.cpu().long(), label[:, 0].long())
    seg = F.one_hot(label[:, 0].long(), 19).permute(0, 3, 1, 2).float()
    img, fake = torch.rand(n, 3, h, w, generator=g) * 2 - 1, torch.randn(n, 3, h, w, generator=g)
    want = torch.cat([torch.cat([seg, fake], 1), torch.cat([seg, img], 1)], 0)
    fk = nhwc(fake).requires_grad_()
    din = ops.DInput.apply(labels, fk, nhwc(img))
    assert tuple(din.shape) == (2 * n, h, w, 24)
    assert rel(nchw(din.detach(), 22), want) == 0.0
    assert float(din[..., 22:].abs().max()) == 0.0
    assert float(din.dsee_amax.max()) == float(din.detach().abs().max())
    gd = torch.randn(2 * n, 22, h, w, generator=g)
    din.backward(nhwc(gd))
    assert rel(nchw(fk.grad, 3), gd[:n, 19:22]) == 0.0


def test_layout_round_trip_rect():
    from deepsee_amd import ops
    x = torch.randn(2, 5, 6, 9, generator=gen(31))
    xs = ops.to_nhwc(x.cuda())
    assert tuple(xs.shape) == (2, 6, 9, 8)
    assert torch.equal(xs[..., :5].cpu(), x.permute(0, 2, 3, 1)) and float(xs[..., 5:].abs().max()) == 0.0
    assert torch.equal(ops.to_nchw(xs, 5).cpu(), x)


def test_bicubic_down_rect_source():
    """dsee_bicubic_down computes one scale per axis (H / S and W / S): a 48 x 80 source to 8 x 8 against F.interpolate in float64."""
    from deepsee_amd import ops
    img = torch.rand(2, 3, 48, 80, generator=gen(37)) * 2 - 1
    lr = O.bicubic_down(img.double(), 8)
    lr_d = ops.bicubic_down(nhwc(img), 8)
    assert tuple(lr_d.shape) == (2, 8, 8, 4)
    err = rel(nchw(lr_d, 3), lr)
    print("bicubic_down 48x80 -> 8x8: %.2e" % err)
    assert err < 1e-6
