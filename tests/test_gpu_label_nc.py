"""The semantic class count L is a runtime argument of every label-indexed kernel (label.hip, build_d_input, the 32-column style
tables); the rest of the suite runs them at L = 19.  Here each operation runs at L in {1, 2, 20, 21, 32} (+ 19 where no 19-class
test of that body exists) against the plain dense form in float64: O.onehot_labels -> F.conv2d / einsum / indexing, gradients by
autograd.  20 | 21 straddles onehot_conv_wgrad_kernel<20> | <32>, 21 is the D input without a padding channel, 32 fills every
32-column table (and puts the 128-channel tap table at 144 KB of LDS), 1 and 2 are the degenerate ends.

Label maps: i.i.d. uniform, and for L > 2 a constant map and a blocky map (8 x 8 cells) with class 0 absent from every image,
class 1 from image 0 and class L - 1 present: the rows of an absent class must be exactly 0.0, and so must every column r >= L of
a 32-wide table.

Bounds are those of the 19-class tests of the same operations (tests/test_gpu_rect.py, test_gpu_ops.py, test_gpu_random_style.py),
bit equality where they assert bit equality.  The last section pins the defined behaviour for label bytes >= L: an all-zero
one-hot vector in every kernel."""
import functools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_explore as TE
import test_gpu_ops as TO
import test_gpu_random_style as TR
from oracle import deepsee_oracle as O

pytestmark = pytest.mark.gpu

TOL = 2e-5
CO = 128
LS = [1, 2, 20, 21, 32]
MAPS = [(nl, "uniform") for nl in LS] + [(nl, k) for nl in LS if nl > 2 for k in ("constant", "blocky")]
MAP_IDS = ["L%d-%s" % m for m in MAPS]


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


def label_map(kind, nl, n, h, w, seed=0):
    """int64 [n, h, w] with values in [0, nl).  blocky: 8 x 8 cells drawn from [1, nl), those of image 0 from [2, nl) when there
    are more than three classes -- class 0 is absent from every image and class 1 from image 0 by construction --, the first cell
    of every image is class nl - 1.  constant: class nl // 2 only."""
    g = gen(97 * h + 13 * w + nl + seed)
    if kind == "uniform":
        return torch.randint(0, nl, (n, h, w), generator=g)
    if kind == "constant":
        return torch.full((n, h, w), nl // 2, dtype=torch.long)
    assert kind == "blocky" and nl > 2
    cells = torch.randint(1, nl, (n, (h + 7) // 8, (w + 7) // 8), generator=g)
    cells[0] = torch.randint(min(2, nl - 1), nl, cells[0].shape, generator=g)
    cells[:, 0, 0] = nl - 1
    return cells.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :h, :w].contiguous()


def low(lab, shift):
    """the map a kernel sees at shift: row h << shift, column w << shift (F.interpolate 'nearest' by a power of two)"""
    n, h, w = lab.shape
    return lab[:, ::1 << shift, ::1 << shift][:, :h >> shift, :w >> shift].contiguous()


def onehot64(lab, nl):
    """[n, nl, h, w] float64 through the oracle's scatter (in-range maps only: scatter_ raises otherwise, like the reference)"""
    return O.onehot_labels(lab[:, None].float(), nl, torch.float64)


def absent_classes(lab, nl):
    """[n, nl] bool: class r does not occur in image b"""
    return torch.stack([torch.bincount(im.reshape(-1), minlength=nl)[:nl] == 0 for im in lab])


def u8(lab):
    return lab.to(torch.uint8).contiguous().cuda()


# ------------------------------------------------------------------------------------ one-hot 3x3 convolution, forward
# name: (N, label H, label W, shift).  dsee_onehot_conv3x3_fwd takes the LDS kernels when the table 9 L Co floats is <= 150 KB,
# 1024 % (Co / 4) == 0 and M = N (H >> s) (W >> s) >= 4096: lds4 when (W >> s) % 4 == 0, lds otherwise; the global kernel below.
FWD_SHAPES = {"global_16x16": (2, 16, 16, 0), "lds4_64x64": (1, 64, 64, 0), "lds4_128x128s1": (1, 128, 128, 1),
              "lds_46x46": (2, 46, 46, 0), "lds_40x106": (1, 40, 106, 0)}
FWD_CASES = ([(s, nl, "uniform", CO) for s in sorted(FWD_SHAPES) for nl in LS]
             + [(s, nl, k, CO) for s in ("global_16x16", "lds4_64x64", "lds_46x46") for nl in LS if nl > 2
                for k in ("constant", "blocky")]
             # 12 and 20 threads per pixel do not divide 1024: the global kernel whatever M, with idle threads at the block's end
             + [(s, 32, "uniform", 48) for s in ("global_16x16", "lds_46x46")]
             + [(s, 19, "uniform", 80) for s in ("global_16x16", "lds_46x46")])


def expected_fwd_kernel(n, r, rw, nl, co):
    if 9 * nl * co * 4 <= 150 * 1024 and 1024 % (co // 4) == 0 and n * r * rw >= 4096:
        return "lds4" if rw % 4 == 0 else "lds"
    return "global"


@functools.lru_cache(maxsize=None)
def _conv_case(shape, nl, kind, co):
    """label map, weights, float64 reference of conv3x3(one-hot) with its autograd through a ReLU: built once per case, shared by
    the forward and weight-gradient tests, never modified."""
    n, h, w, shift = shape
    g = gen(h * w + nl + co)
    lab = label_map(kind, nl, n, h, w)
    wt = (torch.randn(co, nl, 3, 3, generator=g) * 0.3).double().requires_grad_()
    b = (torch.randn(co, generator=g) * 0.2).double().requires_grad_()
    seg = onehot64(low(lab, shift), nl)
    pre = F.conv2d(seg, wt, b, padding=1)
    act = F.relu(pre)
    dact = torch.randn(act.shape, generator=g).double()
    act.backward(dact)
    return {"lab": lab, "w": wt.detach().float(), "b": b.detach().float(), "seg": seg, "pre": pre.detach(), "act": act.detach(),
            "dact": dact, "dw": wt.grad, "db": b.grad}


def gather_sum_f32(lab_low, w_oihw, bias, nl):
    """The kernels' own arithmetic in float32 on the CPU: bias, then + table[tap][label] for tap = 0 .. 8 in that order, taps
    outside the image and labels >= nl skipped.  Only additions, one rounding each: the kernels must match it bit for bit."""
    n, r, rw = lab_low.shape
    co = w_oihw.shape[0]
    table = w_oihw.permute(2, 3, 1, 0).reshape(9, nl, co)                # [tap][class][co]
    padded = F.pad(lab_low, (1, 1, 1, 1), value=-1)
    acc = bias[None, None, None, :].expand(n, r, rw, co).clone()
    for tap in range(9):
        lt = padded[:, tap // 3:tap // 3 + r, tap % 3:tap % 3 + rw]
        ok = (lt >= 0) & (lt < nl)
        acc = torch.where(ok[..., None], acc + table[tap][lt.clamp(0, nl - 1)], acc)
    return acc


@pytest.mark.parametrize("shape,nl,kind,co", FWD_CASES, ids=["%s-L%d-%s-co%d" % c for c in FWD_CASES])
def test_onehot_conv3x3_fwd(shape, nl, kind, co):
    """pack + forward with and without ReLU, with and without the 32 one-hot columns: against float64 F.conv2d (2e-5, the bound
    of the 19-class test), bit for bit against the float32 gather-sum in the kernels' tap order, amax == max(floor, max |out|),
    one-hot columns == dsee_label_onehot == the float64 one-hot with columns >= L zero, nothing written outside the columns."""
    from deepsee_amd import lib as L
    n, h, w, shift = FWD_SHAPES[shape]
    r, rw = h >> shift, w >> shift
    assert expected_fwd_kernel(n, r, rw, nl, co) == (shape.split("_")[0] if co == CO else "global")
    ref = _conv_case(FWD_SHAPES[shape], nl, kind, co)
    lab = u8(ref["lab"])
    table = torch.full((9, nl, co), float("nan"), device="cuda")
    L.call("onehot_conv3x3_pack", ref["w"].cuda(), table, co, nl)
    assert torch.equal(table.cpu(), ref["w"].permute(2, 3, 1, 0).reshape(9, nl, co))
    bias = ref["b"].cuda()
    oh = torch.full((n, r, rw, 32), float("nan"), device="cuda")
    L.call("label_onehot", lab, oh, n, h, w, shift, 32, 0)
    torch.cuda.synchronize()
    assert torch.equal(oh[..., :nl].cpu().double(), ref["seg"].permute(0, 2, 3, 1))
    assert nl == 32 or float(oh[..., nl:].abs().max()) == 0.0
    for relu in (0, 1):
        want = (ref["act"] if relu else ref["pre"]).permute(0, 2, 3, 1)
        bits = gather_sum_f32(low(ref["lab"], shift), ref["w"], ref["b"], nl)
        bits = bits.clamp_min(0.0) if relu else bits
        ld = co + 32 + 4
        for floor in (0.0, 1000.0):
            out = torch.full((n, r, rw, ld), -7.0, device="cuda")
            amax = torch.zeros(2048, device="cuda")
            L.call("onehot_conv3x3_fwd", lab, table, bias, out, n, h, w, shift, nl, co, ld, 0, relu, co, amax, floor)
            torch.cuda.synchronize()
            assert float(amax.max()) == max(floor, float(out[..., :co].abs().max())), (floor, float(amax.max()))
        err = rel(out[..., :co].cpu(), want)
        print("one-hot conv forward %s L=%d %s Co=%d relu=%d: %.2e" % (shape, nl, kind, co, relu, err))
        assert err < TOL
        assert torch.equal(out[..., :co].cpu(), bits)
        assert torch.equal(out[..., co:co + 32], oh)
        assert bool((out[..., co + 32:] == -7.0).all())
        plain = torch.full((n, r, rw, co + 4), -7.0, device="cuda")
        amax = torch.zeros(2048, device="cuda")
        L.call("onehot_conv3x3_fwd", lab, table, bias, plain, n, h, w, shift, nl, co, co + 4, 4, relu, -1, amax, 0.0)
        torch.cuda.synchronize()
        assert torch.equal(plain[..., 4:], out[..., :co]) and bool((plain[..., :4] == -7.0).all())
        assert float(amax.max()) == float(plain[..., 4:].abs().max())


# ------------------------------------------------------------------------------------ one-hot 3x3 convolution, weight gradient
# wgrad_parts: chunks of max(256, ceil(M / 512)) pixels, eight pixels per trip.  2 x 23 x 41 = 1886 pixels: seven whole chunks
# and one of 94 pixels, 94 % 8 = 6 -- the tail of a chunk inside a trip.
WGRAD_SHAPES = {"32x32": (2, 32, 32, 0), "32x32s1": (2, 32, 32, 1), "23x41": (2, 23, 41, 0)}
WGRAD_CASES = ([(s, nl, "uniform") for s in sorted(WGRAD_SHAPES) for nl in LS]
               + [("32x32", nl, k) for nl in LS if nl > 2 for k in ("constant", "blocky")])


@pytest.mark.parametrize("ld", [128, 160])
@pytest.mark.parametrize("shape,nl,kind", WGRAD_CASES, ids=["%s-L%d-%s" % c for c in WGRAD_CASES])
def test_onehot_conv3x3_wgrad(shape, nl, kind, ld):
    """dw and db against autograd of ReLU(conv3x3(one-hot)) in float64 (5 * 2e-5, the bound of the 19-class test), act / dact as
    128-column tensors and as the first 128 columns of 160-wide rows (the concatenated SEAN input); L <= 20 runs
    onehot_conv_wgrad_kernel<20>, L >= 21 <32>.  The rows of a class no image holds near a tap are exactly 0."""
    from deepsee_amd import lib as L
    n, h, w, shift = WGRAD_SHAPES[shape]
    ref = _conv_case(WGRAD_SHAPES[shape], nl, kind, CO)
    lab = u8(ref["lab"])

    def rows(t):
        t = t.permute(0, 2, 3, 1).float()
        wide = torch.randn(t.shape[:3] + (ld,), generator=gen(ld))        # (the other 32 columns: any values, positive included)
        wide[..., :CO] = t
        return wide.contiguous().cuda()

    act, dact = rows(ref["act"]), rows(ref["dact"])
    assert bool(((act[..., :CO] > 0).cpu() == (ref["act"].permute(0, 2, 3, 1) > 0)).all())
    dw, db = torch.full((CO, nl, 3, 3), float("nan"), device="cuda"), torch.full((CO,), float("nan"), device="cuda")
    ws = torch.full((L.lib().dsee_onehot_conv3x3_wgrad_workspace(n, h, w, shift, nl) // 4,), float("nan"), device="cuda")
    L.call("onehot_conv3x3_wgrad", lab, dact, ld, act, ld, n, h, w, shift, nl, dw, db, ws)
    torch.cuda.synchronize()
    e_w, e_b = rel(dw.cpu(), ref["dw"]), rel(db.cpu(), ref["db"])
    print("one-hot conv weight gradient %s L=%d %s ld=%d: dw %.2e db %.2e" % (shape, nl, kind, ld, e_w, e_b))
    assert e_w < 5 * TOL and e_b < 5 * TOL
    gone = absent_classes(low(ref["lab"], shift), nl).all(0)             # absent from every image
    assert kind == "uniform" or bool(gone[0])                            # (class 0, by construction of the map)
    assert float(dw[:, gone.cuda()].abs().sum()) == 0.0 and float(ref["dw"][:, gone].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------ gather / segmented sum
# (N, label H, label W, shift): 20 x 28 = 560 pixels are three chunks of seg_chunks (256, 256, 48)
SEG_SHAPES = {"20x28": (2, 20, 28, 0), "32x64s2": (2, 32, 64, 2)}
SEG_CASES = ([(s, nl, "uniform", cs) for s in sorted(SEG_SHAPES) for nl in LS for cs in (4, 128, 256)]
             + [("20x28", nl, k, 128) for nl in LS if nl > 2 for k in ("constant", "blocky")])


@pytest.mark.parametrize("shape,nl,kind,cs", SEG_CASES, ids=["%s-L%d-%s-cs%d" % c for c in SEG_CASES])
def test_label_gather_and_segsum(shape, nl, kind, cs):
    """dsee_label_gather: out = scale * table[b][label] bit for bit (one fp32 product), into columns [coff, coff + Cs) of wider rows
    whose other columns stay untouched.  dsee_label_segsum: scale * sum over the pixels of a class, read from columns at an offset,
    against the float64 einsum with the one-hot (2e-5); rows of absent classes exactly 0."""
    from deepsee_amd import lib as L
    n, h, w, shift = SEG_SHAPES[shape]
    r, rw = h >> shift, w >> shift
    g = gen(nl + cs + h)
    lab = label_map(kind, nl, n, h, w)
    lo = low(lab, shift)
    seg = onehot64(lo, nl)
    for coff, ld, scale in [(0, cs, 1.0), (8, cs + 12, 0.37)]:
        table = torch.randn(n, nl, cs, generator=g)
        out = torch.full((n, r, rw, ld), -7.0, device="cuda")
        L.call("label_gather", u8(lab), table.cuda(), out, n, h, w, shift, nl, cs, ld, coff, scale)
        torch.cuda.synchronize()
        want = torch.stack([table[b][lo[b]] for b in range(n)]) * torch.tensor(scale, dtype=torch.float32)
        assert torch.equal(out[..., coff:coff + cs].cpu(), want)
        assert bool((out[..., :coff] == -7.0).all()) and bool((out[..., coff + cs:] == -7.0).all())
        assert rel(want, torch.einsum("brc,brhw->bhwc", table.double(), seg) * scale) < 1e-6

        feat = torch.randn(n, r, rw, ld, generator=g)
        got = torch.full((n, nl, cs), float("nan"), device="cuda")
        ws = torch.full((L.lib().dsee_label_segsum_workspace(n, h, w, shift, nl, cs) // 4,), float("nan"), device="cuda")
        L.call("label_segsum", u8(lab), feat.cuda(), ld, coff, got, n, h, w, shift, nl, cs, scale, ws)
        torch.cuda.synchronize()
        want_s = torch.einsum("bhwc,brhw->brc", feat[..., coff:coff + cs].double(), seg) * scale
        err = rel(got.cpu(), want_s)
        print("segsum %s L=%d %s Cs=%d coff=%d: %.2e" % (shape, nl, kind, cs, coff, err))
        assert err < TOL
        gone = absent_classes(lo, nl)
        assert kind == "uniform" or bool(gone[:, 0].all())               # (class 0, by construction of the map)
        assert float(got.cpu()[gone].abs().sum()) == 0.0


@pytest.mark.parametrize("nl,kind", MAPS, ids=MAP_IDS)
def test_style_pool_fwd_bwd(nl, kind):
    """ops.StylePool (segsum forward, gather backward) against the oracle's style_pool in float64, the bounds of the 19-class
    test; absent classes pool to exactly 0."""
    from deepsee_amd import ops
    n, c, hf, h = 2, 128, 16, 32
    g = gen(9 + nl)
    lab = label_map(kind, nl, n, h, h)
    f = torch.randn(n, c, hf, hf, generator=g).double().requires_grad_()
    s = O.style_pool(f, onehot64(lab, nl))
    gs = torch.randn(s.shape, generator=g)
    s.backward(gs.double())
    labels = ops.Labels(u8(lab), nl)
    fs = nhwc(f.detach().float()).requires_grad_()
    sd = ops.StylePool.apply(fs, labels, labels.shift_for(hf))
    sd.backward(gs.cuda())
    torch.cuda.synchronize()
    e_s, e_f = rel(sd.detach().cpu(), s.detach()), rel(nchw(fs.grad, c), f.grad)
    print("style pool L=%d %s: s %.2e df %.2e" % (nl, kind, e_s, e_f))
    assert tuple(sd.shape) == (n, nl, c) and e_s < TOL and e_f < TOL
    assert float(sd.detach().cpu()[absent_classes(low(lab, 1), nl)].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------ the 32 one-hot columns, the D input
@pytest.mark.parametrize("coff,pad", [(0, 0), (128, 0), (0, 8), (128, 8)])
@pytest.mark.parametrize("nl", LS)
def test_label_onehot(nl, coff, pad):
    """dsee_label_onehot at shift 0 and 1: columns [coff, coff + 32) equal the float64 one-hot (columns >= L zero), every other
    float of the row keeps its sentinel -- with out_ld exactly coff + 32 and larger."""
    from deepsee_amd import lib as L
    n, h, w = 2, 12, 20
    lab = label_map("uniform", nl, n, h, w)
    for shift in (0, 1):
        r, rw, ld = h >> shift, w >> shift, coff + 32 + pad
        out = torch.full((n, r, rw, ld), -7.0, device="cuda")
        L.call("label_onehot", u8(lab), out, n, h, w, shift, ld, coff)
        torch.cuda.synchronize()
        got = out.cpu()
        assert torch.equal(got[..., coff:coff + nl].double(), onehot64(low(lab, shift), nl).permute(0, 2, 3, 1))
        assert float(got[..., coff + nl:coff + 32].abs().sum()) == 0.0
        assert bool((got[..., :coff] == -7.0).all()) and bool((got[..., coff + 32:] == -7.0).all())


@pytest.mark.parametrize("nl", [1, 2, 20, 21, 29, 32])
def test_dinput_fwd_bwd(nl):
    """ops.DInput bit for bit, as test_preprocess_bicubic_labels_dinput at 19 classes: L + 3 channels stored as pad4(L + 3) -- 21
    as 24 with no padding channel, 29 as 32, 32 as 36 --, padding channels exactly 0, the carried amax the tensor's max."""
    from deepsee_amd import lib as L, ops
    g = gen(13 + nl)
    n, h, w = 2, 12, 20
    lab = label_map("uniform", nl, n, h, w)
    img, fake = torch.rand(n, 3, h, w, generator=g) * 2 - 1, torch.randn(n, 3, h, w, generator=g)
    seg = onehot64(lab, nl).float()
    want = torch.cat([torch.cat([seg, fake], 1), torch.cat([seg, img], 1)], 0)
    fk = nhwc(fake).requires_grad_()
    din = ops.DInput.apply(ops.Labels(u8(lab), nl), fk, nhwc(img))
    ld = L.pad4(nl + 3)
    assert {1: 4, 2: 8, 20: 24, 21: 24, 29: 32, 32: 36}[nl] == ld == din.shape[3]
    assert torch.equal(nchw(din.detach(), nl + 3), want)
    assert ld == nl + 3 or float(din[..., nl + 3:].abs().max()) == 0.0
    assert float(din.dsee_amax.max()) == float(din.detach().abs().max())
    gd = torch.randn(2 * n, nl + 3, h, w, generator=g)
    din.backward(nhwc(gd) if ld == nl + 3 else F.pad(nhwc(gd)[..., :nl + 3], (0, ld - nl - 3), value=float("nan")))
    assert torch.equal(nchw(fk.grad, 3), gd[:n, nl:nl + 3])


# ------------------------------------------------------------------------------------ one-hot x noise convolution
# The tap table 9 L Co floats and the staged tile (4896 bytes) share 64 KB of LDS and Co / 4 must divide 256: at 32 classes that
# admits Co = 32 (36, 40, 44, 48, 52: Co / 4 does not divide 256; 64: 78624 bytes).  The weight gradient keeps L floats per
# thread, max(256, 9 Co rounded up to 64) threads: at 32 classes 448 threads, Co <= 48.
NOISE_SHAPES = [(2, 20, 40, nl, 32) for nl in (1, 20, 32)]


@pytest.mark.parametrize("shape", NOISE_SHAPES)
def test_onehot_noise_conv3x3(shape):
    """forward and weight gradient on an explicit field against float64 F.conv2d(onehot * eps), element-wise bounds of
    tests/test_gpu_random_style.py (1e-6 / 1e-5 of the sum of the absolute terms)."""
    lab, eps, wt, b, dout = TR._inputs(shape, True)
    want, terms, dw, dw_terms, db, db_terms = TR._reference(lab, eps, wt, b, dout, shape[3])
    y, gw, gb = TR._run(lab, eps.cuda(), wt, b, dout, shape[3])
    err = (y.double().cpu() - want).abs()
    ew, eb = (gw.double().cpu() - dw).abs(), (gb.double().cpu() - db).abs()
    print("noise conv %s: forward %.3g, wgrad %.3g of the sum of |terms|" % (
        shape, float((err / terms.clamp_min(1e-30)).max()), float((ew / dw_terms.clamp_min(1e-30)).max())))
    assert bool((err <= 1e-6 * terms + 1e-30).all())
    assert bool((ew <= 1e-5 * dw_terms + 1e-30).all()) and bool((eb <= 1e-5 * db_terms + 1e-30).all())


def test_onehot_noise_conv3x3_widest_at_32_classes():
    """The weight gradient alone at its widest 32-class shape (Co = 48) against float64; the first widths the argument checks
    exclude raise before any launch: forward Co = 36 (nine float4 per pixel) and 64 (LDS), weight gradient Co = 52 (LDS)."""
    from deepsee_amd import lib as L, ops
    shape = (2, 20, 40, 32, 48)
    n, h, w, nl, co = shape
    lab, eps, wt, b, dout = TR._inputs(shape, True)
    _, _, dw, dw_terms, db, db_terms = TR._reference(lab, eps, wt, b, dout, nl)
    gw, gb = ops.new(co, nl, 3, 3), ops.new(co)
    ws = torch.full((L.lib().dsee_onehot_noise_conv3x3_wgrad_workspace(n, h, w, nl, co) // 4,), float("nan"), device="cuda")
    L.call("onehot_noise_conv3x3_wgrad", lab.cuda(), eps.cuda(), 0, 0, 0, dout.cuda(), n, h, w, nl, co, gw, gb, ws)
    torch.cuda.synchronize()
    ew, eb = (gw.double().cpu() - dw).abs(), (gb.double().cpu() - db).abs()
    assert bool((ew <= 1e-5 * dw_terms + 1e-30).all()) and bool((eb <= 1e-5 * db_terms + 1e-30).all())
    out = torch.full((n, h, w, 64), -7.0, device="cuda")
    for bad in (36, 64):
        with pytest.raises(L.DseeError, match="argument check failed"):
            L.call("onehot_noise_conv3x3_fwd", lab.cuda(), eps.cuda(), 0, 0, 0, ops.new(9, nl, bad), None, out, n, h, w, nl, bad)
    with pytest.raises(L.DseeError, match="argument check failed"):
        L.call("onehot_noise_conv3x3_wgrad", lab.cuda(), eps.cuda(), 0, 0, 0, ops.new(n, h, w, 52), n, h, w, nl, 52,
               ops.new(52, nl, 3, 3), None, ws)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ------------------------------------------------------------------------------------ the per-image 32-column style tables
@pytest.mark.parametrize("nl", LS)
def test_style_table_layout_fwd_bwd(nl):
    """[N L][9 rows] <-> [N][9][rows][32] at rows = 128, N = 2: a permutation (bit exact); columns >= L of the table exactly 0,
    amax raised to max |table|; the backward reads the columns < L only."""
    from deepsee_amd import lib as L
    n, rows = 2, 128
    g = gen(nl)
    t = torch.randn(n * nl, 9 * rows, generator=g)
    table = torch.full((n, 9, rows, 32), float("nan"), device="cuda")
    amax = torch.zeros(2048, device="cuda")
    L.call("style_table_layout", t.cuda(), table, n, nl, rows, amax)
    torch.cuda.synchronize()
    want = t.view(n, nl, 9, rows).permute(0, 2, 3, 1)
    assert torch.equal(table[..., :nl].cpu(), want)
    assert nl == 32 or float(table[..., nl:].abs().max()) == 0.0
    assert float(amax.max()) == float(t.abs().max())
    dtab = torch.randn(n, 9, rows, 32, generator=g)
    dt = torch.full((n * nl, 9 * rows), float("nan"), device="cuda")
    L.call("style_table_layout_bwd", dtab.cuda(), dt, n, nl, rows)
    torch.cuda.synchronize()
    assert torch.equal(dt.cpu(), dtab[..., :nl].permute(0, 3, 1, 2).reshape(n * nl, 9 * rows))


# ------------------------------------------------------------------------------------ the norm layers' table weight gradients
def norm_label(kind, nl, n, h, w):
    """float [n, 1, h, w] map for the norm bodies, None for their own uniform draw.  "loader": what the loader hands over without
    a dontcare class -- the files' 255 arrives as the byte L, here in ~6 % of the pixels (an all-zero one-hot vector; < 32, so
    dsee_label_onehot flags column L, which every consumer meets with a zero table column or drops)."""
    if kind == "uniform":
        return None
    if kind == "loader":
        lab = torch.randint(0, nl, (n, h, w), generator=gen(nl + h))
        flat = lab.view(-1)
        flat[torch.randperm(flat.numel(), generator=gen(w))[:flat.numel() // 16]] = nl
        flat[0], flat[-1] = nl, nl
        return lab[:, None].float()
    return label_map(kind, nl, n, h, w)[:, None].float()


NORM_MAPS = MAPS + [(19, "blocky"), (19, "loader")]
NORM_IDS = ["L%d-%s" % m for m in NORM_MAPS]


@pytest.mark.parametrize("nl,kind", NORM_MAPS, ids=NORM_IDS)
def test_spade_sean_norm_direct_path(nl, kind):
    """tests/test_gpu_ops.py::test_spade_sean_norm_fwd_bwd at its smallest SEAN row, L classes: SeanInput (pack, forward, gather)
    and its backward (one-hot weight gradient, segsum) under the bounds of the 19-class rows; rows of absent classes exactly 0."""
    gone = TO.spade_sean_norm_fwd_bwd("sean", 64, 16, 2, Lc=nl, label=norm_label(kind, nl, 2, 32, 32))
    assert kind in ("uniform", "loader") or bool(gone[:, 0].all())


@pytest.mark.parametrize("R", [16, (32, 64, True)], ids=["16", "32x64wino"])
@pytest.mark.parametrize("nl,kind", NORM_MAPS, ids=NORM_IDS)
def test_sean_norm_table_path(nl, kind, R):
    """tests/test_gpu_ops.py::test_sean_norm_table_path with L classes in the 32-column tables: ("sean", 64, 16, 2) -- the
    direct dsee_conv2d_wgrad_table -- and the smallest row in the Winograd domain, 32 x 64 (dsee_wino43_wgrad_table), under the
    bounds of the 19-class rows.  The body asserts exact zeros: columns >= L of the table and of dtable, dtable[b, ..., r] and
    style.grad[b, r] for a class r absent from image b, dw_shared[:, r] for a class absent from every image."""
    h, w = (64, 64) if R == 16 else (2 * R[0], 2 * R[1])
    gone = TO.sean_norm_table_path("sean", 64, R, 2, 256, Lc=nl, label=norm_label(kind, nl, 2, h, w))
    assert kind in ("uniform", "loader") or bool(gone[:, 0].all())


def test_spade_norm_table_path_with_the_loaders_unknown_label():
    """The SPADE-only norm on the loader's map (byte 19 with 19 classes): its mlp_shared weight gradient is the MFMA weight
    gradient over the 32 materialised one-hot columns, of which column 19 is flagged and dropped (cin = L)."""
    TO.sean_norm_table_path("spade", 64, 16, 2, 256, Lc=19, label=norm_label("loader", 19, 2, 64, 64))


@pytest.mark.parametrize("flags", [3, 5], ids=["some", "all"])
@pytest.mark.parametrize("nl", [1, 20, 32])
def test_style_explore(nl, flags):
    """dsee_style_explore on [B][n][L][S] style matrices, the body and bit equality of tests/test_gpu_explore.py: a partial region mask
    with noise and recurrence (L > 1), and every region masked with clamping."""
    if nl == 1 and TE.FLAGS[flags]["mask"] == "some":
        flags = 6                                      # (one region: the mask is all or none)
    TE.style_explore_equals_the_torch_rule(TE.FLAGS[flags], nc=nl)


# ------------------------------------------------------------------------------------ the coarse entry points (coarse.cpp)
# The bodies of tests/test_gpu_ops.py with L classes: the C calls against the Python module's own launches, at the shapes those
# tests use (the smallest the entry points accept).  "sean" runs with the per-image style table, "spade" without.
@pytest.mark.parametrize("kind", ["sean", "spade"])
@pytest.mark.parametrize("nl", [2, 21, 32])
def test_coarse_sean_norm_fwd(nl, kind):
    TO.coarse_sean_norm_fwd(kind, Lc=nl)


@pytest.mark.parametrize("kind", ["sean", "spade"])
@pytest.mark.parametrize("nl", [2, 21, 32])
def test_coarse_spade_resblock_fwd(nl, kind):
    TO.coarse_spade_resblock_fwd(Lc=nl, kind=kind)


def test_coarse_spade_resblock_fwd_without_table_at_19_classes():
    TO.coarse_spade_resblock_fwd(kind="spade")


@pytest.mark.parametrize("kind", ["sean", "spade"])
@pytest.mark.parametrize("nl", [2, 21, 32])
def test_coarse_resblock_training_pair(nl, kind):
    TO.coarse_resblock_training_pair(kind, Lc=nl)


# ------------------------------------------------------------------------------------ label bytes outside [0, L)
# Defined behaviour (label.hip): such a pixel is an all-zero one-hot vector.  The loader produces one: 255 -> label_nc when the
# options hold no dontcare class.  The global-memory tables are the head of a NaN-filled allocation with room for 256 more rows:
# an index formed from such a byte would bring a NaN into the result.
def outside_map(nl, n, h, w):
    """uniform in [0, nl) with nl, nl + 1, 200 and 255 scattered over ~6 % of the pixels (first and last pixel included)"""
    g = gen(5 * h + w + nl)
    lab = torch.randint(0, nl, (n, h, w), generator=g)
    flat = lab.view(-1)
    hit = torch.randperm(flat.numel(), generator=g)[:flat.numel() // 16]
    flat[hit] = torch.tensor([nl, nl + 1, 200, 255])[torch.arange(hit.numel()) % 4]
    flat[0], flat[-1] = 255, nl
    return lab


def onehot64_any(lab, nl):
    return (lab[:, None] == torch.arange(nl)[None, :, None, None]).double()


def in_nan_arena(t, extra_rows):
    """t [..., C] on the device as the head of a NaN-filled allocation with `extra_rows` more rows of C floats behind it"""
    c = t.shape[-1]
    arena = torch.full((t.numel() + extra_rows * c,), float("nan"), device="cuda")
    arena[:t.numel()] = t.reshape(-1).cuda()
    return arena[:t.numel()].view(t.shape), arena


@pytest.mark.parametrize("nl", [1, 19, 32])
@pytest.mark.parametrize("shape", ["global_16x16", "lds4_64x64", "lds_46x46"])
def test_outside_labels_onehot_conv(shape, nl):
    """forward (the three kernels) and weight gradient on a map with bytes >= L against the float64 dense form whose one-hot is zero
    there; forward also bit for bit against the float32 gather-sum that skips those taps."""
    from deepsee_amd import lib as L
    n, h, w, shift = FWD_SHAPES[shape]
    g = gen(nl + h)
    lab = outside_map(nl, n, h, w)
    assert all(bool((lab == v).any()) for v in (nl, nl + 1, 200, 255))
    wt = (torch.randn(CO, nl, 3, 3, generator=g) * 0.3).double().requires_grad_()
    b = (torch.randn(CO, generator=g) * 0.2).double().requires_grad_()
    act = F.relu(F.conv2d(onehot64_any(lab, nl), wt, b, padding=1))
    dact = torch.randn(act.shape, generator=g).double()
    act.backward(dact)
    assert expected_fwd_kernel(n, h, w, nl, CO) == shape.split("_")[0]
    packed = wt.detach().float().permute(2, 3, 1, 0).reshape(9 * nl, CO)
    table, arena = in_nan_arena(packed, 256)
    out = torch.full((n, h, w, CO), float("nan"), device="cuda")
    amax = torch.zeros(2048, device="cuda")
    L.call("onehot_conv3x3_fwd", u8(lab), table, b.detach().float().cuda(), out, n, h, w, 0, nl, CO, CO, 0, 1, -1, amax, 0.0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and float(amax.max()) == float(out.abs().max())
    assert rel(out.cpu(), act.detach().permute(0, 2, 3, 1)) < TOL
    assert torch.equal(out.cpu(), gather_sum_f32(lab, wt.detach().float(), b.detach().float(), nl).clamp_min(0.0))
    dw, db = torch.full((CO, nl, 3, 3), float("nan"), device="cuda"), torch.full((CO,), float("nan"), device="cuda")
    ws = torch.full((L.lib().dsee_onehot_conv3x3_wgrad_workspace(n, h, w, 0, nl) // 4,), float("nan"), device="cuda")
    L.call("onehot_conv3x3_wgrad", u8(lab), dact.permute(0, 2, 3, 1).float().contiguous().cuda(), CO, out, CO, n, h, w, 0, nl,
           dw, db, ws)
    torch.cuda.synchronize()
    assert bool(((out > 0).cpu() == (act.permute(0, 2, 3, 1) > 0)).all())
    assert rel(dw.cpu(), wt.grad) < 5 * TOL and rel(db.cpu(), b.grad) < 5 * TOL


@pytest.mark.parametrize("nl", [1, 19, 32])
@pytest.mark.parametrize("cs", [4, 128, 256])
def test_outside_labels_gather_and_segsum(nl, cs):
    """gather writes zeros for a byte >= L (and reads no table row: the table is the head of a NaN arena); segsum leaves the pixel
    out of every sum; label_onehot and the D input give it an all-zero class vector."""
    from deepsee_amd import lib as L, ops
    n, h, w = 2, 20, 28
    g = gen(nl + cs)
    lab = outside_map(nl, n, h, w)
    seg = onehot64_any(lab, nl)
    tab = torch.randn(n, nl, cs, generator=g)
    table, arena = in_nan_arena(tab, 256)
    out = torch.full((n, h, w, cs), float("nan"), device="cuda")
    L.call("label_gather", u8(lab), table, out, n, h, w, 0, nl, cs, cs, 0, 0.5)
    torch.cuda.synchronize()
    inside = lab < nl
    want = torch.stack([tab[b][lab[b].clamp(max=nl - 1)] for b in range(n)]) * 0.5
    want = torch.where(inside[..., None], want, torch.zeros(()))
    assert torch.equal(out.cpu(), want)
    assert rel(want, torch.einsum("brc,brhw->bhwc", tab.double(), seg) * 0.5) < 1e-6
    feat = torch.randn(n, h, w, cs, generator=g)
    got = torch.full((n, nl, cs), float("nan"), device="cuda")
    ws = torch.full((L.lib().dsee_label_segsum_workspace(n, h, w, 0, nl, cs) // 4,), float("nan"), device="cuda")
    L.call("label_segsum", u8(lab), feat.cuda(), cs, 0, got, n, h, w, 0, nl, cs, 1.0, ws)
    torch.cuda.synchronize()
    assert rel(got.cpu(), torch.einsum("bhwc,brhw->brc", feat.double(), seg)) < TOL
    if cs == 4:
        oh = torch.full((n, h, w, 32), float("nan"), device="cuda")
        L.call("label_onehot", u8(lab), oh, n, h, w, 0, 32, 0)
        torch.cuda.synchronize()
        assert torch.equal(oh.cpu().double(), onehot64_any(lab, 32).permute(0, 2, 3, 1))      # (the raw byte, when it is < 32)
        img = torch.rand(n, 3, h, w, generator=g)
        din = ops.DInput.apply(ops.Labels(u8(lab), nl), nhwc(img))
        assert torch.equal(nchw(din, nl + 3), torch.cat([seg.float(), img], 1))
