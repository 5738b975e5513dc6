"""The generator forward from C (dsee_generator_prepare / dsee_generator_fwd through deepsee_amd.native.NativeGenerator) and the
style-table kernel behind it (dsee_style_table_fwd), on the GPU:

 1. the table kernel against float64 within the fp32 dot-product bound, zero columns, bit reproducibility, the slot semantics of
    its `amax`, once between red zones;
 2. bit identity with SRModel mode "demo" (the Python module keeps rocBLAS for the table product, so the test routes that one
    product through the new kernel and leaves everything else as shipped);
 3. against the CPU oracle, no Python module in the loop;
 4. prepare + forward between red zones (tests/redzone.py), workspace poisoned;
 5. `prepared` is read-only for the forward;
 6. the forward captured into one hipGraph and replayed on new inputs;
 7. export -> from_export gives the same bits.

Weights: O.recipe_state(opt, gain=1.0) with weight_u / weight_v of every SR layer replaced by the leading singular pair of
weight_orig (float64 SVD).  With the recipe's random u, v the eval-mode sigma is far too small, every output element saturates
to +-1 and a comparison of outputs shows nothing; each test therefore first asserts on the ORACLE's output that at most 1 % of it
lies above 0.99 and that two style matrices move the image by >= 1e-2 mean absolute.

Channel count: C = 128 (ngf = 8), where the default plan splits the convolutions' V inside the GEMM at every level, as
dsee_generator_fwd then does too; one more case at C = 256 (ngf = 16) reaches the level rule's other side, the pre-split GEMM at
128 x 128."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

import redzone      # (as tests/test_gpu_redzone.py imports it: one module, one RECORD of what ran guarded)
from oracle import deepsee_oracle as O

pytestmark = pytest.mark.gpu

BASE = dict(start_size=32, crop_size=128, load_size=128, ngf=8, batchSize=4)
CASES = {
    "default": dict(BASE),                                                   # SPADE head, SEAN body: one block of every position
    "sean_head": dict(BASE, norm_G="spectralseansyncbatch3x3"),              # SEAN at 32 x 32: the direct gamma/beta kernel
    "nostyle": dict(BASE, netG="nostyle"),                                   # no tables at all
    "label_nc5": dict(BASE, label_nc=5),
    "rect": dict(BASE, batchSize=2, _lr=(32, 64)),                           # LR 32 x 64 -> 128 x 256
    "c256": dict(BASE, ngf=16),                                              # pre-split GEMM at the top level
}


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def gen(seed):
    return torch.Generator().manual_seed(seed)


@contextlib.contextmanager
def oracle_plan(netG):
    """The oracle's block plan follows opt.netG only with the substitution of tools/gen_golden_ablation.py installed: here for the
    duration of the block."""
    saved = []

    def set_(obj, attr, value):
        saved.append((obj, attr, getattr(obj, attr)))
        setattr(obj, attr, value)

    if netG != "deepsee":
        from tools.gen_golden_ablation import install_ablation
        install_ablation(set_)
    try:
        yield
    finally:
        for obj, attr, value in reversed(saved):
            setattr(obj, attr, value)


STYLE_AMPLITUDE, IMAGE_AMPLITUDE = 0.25, 0.7      # inputs at which the oracle's output is informative (oracle_is_informative)


@functools.lru_cache(maxsize=None)
def case(name):
    """(opt of the package, opt of the oracle, SR state with singular-pair u / v, inputs, the oracle's outputs for two styles) --
    computed once and shared; nothing here is modified by a test."""
    from deepsee_amd.options import make_opt
    over = dict(CASES[name])
    lr_hw = over.pop("_lr", (32, 32))
    opt, oopt = make_opt(no_vgg_loss=True, **over), O.make_opt(no_vgg_loss=True, **over)
    with oracle_plan(oopt.netG):
        sr = O.recipe_state(oopt, gain=1.0)["SR"]
    for k in [k for k in sr if k.endswith("weight_orig")]:
        w = sr[k].reshape(sr[k].shape[0], -1).double()
        u, s, vh = torch.linalg.svd(w, full_matrices=False)
        sr[k[:-len("orig")] + "u"], sr[k[:-len("orig")] + "v"] = u[:, 0].float().contiguous(), vh[0].float().contiguous()
    g = gen(2024)
    n, nc, (h, w) = opt.batchSize, opt.semantic_nc, lr_hw
    H, W = h * 4, w * 4
    label = F.interpolate(torch.randint(0, nc, (n, 1, H // 8, W // 8), generator=g).float(), size=(H, W), mode="nearest")
    image = (torch.rand(n, 3, H, W, generator=g) * 2 - 1) * IMAGE_AMPLITUDE
    image_lr = F.interpolate(image, size=(h, w), mode="bicubic", align_corners=False).clamp(-1, 1)
    styles = [(torch.rand(n, nc, opt.regional_style_size, generator=g) * 2 - 1) * STYLE_AMPLITUDE for _ in range(2)]
    orc = O.Oracle(oopt, {"SR": sr})
    orc.training = False
    with torch.no_grad(), oracle_plan(oopt.netG):
        seg = O.onehot_labels(label, nc)
        want = [orc.sr_forward(image_lr, seg, s).detach() for s in styles]
    return dict(opt=opt, oopt=oopt, sr=sr, label=label, image=image, image_lr=image_lr, styles=styles, want=want,
                reads_style=any(kind != "spade" for _, kind in block_plan_of(opt)))


def block_plan_of(opt):
    from deepsee_amd.sr_model import block_plan
    return block_plan(opt)


def oracle_is_informative(c):
    """The two conditions of the module docstring, on the oracle's own output.  (netG = nostyle has no layer that reads the style
    matrix: there the second condition has nothing to hold for.)"""
    y0, y1 = c["want"]
    sat = float((y0.abs() > 0.99).float().mean())
    moved = float((y0 - y1).abs().mean())
    print("oracle: %.3f %% of |y| > 0.99, mean |y(style 0) - y(style 1)| = %.3f" % (100 * sat, moved))
    assert sat <= 0.01, sat
    assert moved >= 1e-2 or not c["reads_style"], moved


def device_inputs(c, which=0):
    return (c["image_lr"].cuda().contiguous(), c["label"][:, 0].to(torch.uint8).cuda().contiguous(),
            c["styles"][which].cuda().contiguous())


def native_of(c):
    from deepsee_amd.native import NativeGenerator
    return NativeGenerator(c["opt"], c["sr"]).prepare()


def table_by_the_new_kernel(style, wst, rows, amax=None):
    """ops.style_table_packed with its GEMM + layout pair replaced by dsee_style_table_fwd"""
    from deepsee_amd import lib as L, ops
    n, nc, s = style.shape
    t = ops.new(n, 9, rows, 32)
    L.call("style_table_fwd", style.contiguous(), wst.contiguous(), t, n, nc, s, rows, amax)
    t.dsee_amax = amax
    return t


# ------------------------------------------------------------------------------------------------ 1. the table kernel
def slot_max(slot):
    return float(slot.view(64, 32)[:, 0].max())


def run_table(style, wst, rows, slot):
    from deepsee_amd import lib as L
    n, l, s = style.shape
    t = torch.full((n, 9, rows, 32), float("nan"), device="cuda")
    L.call("style_table_fwd", style, wst, t, n, l, s, rows, slot)
    return t


@pytest.mark.parametrize("shape", [(1, 1, 4, 64), (3, 19, 128, 256), (2, 32, 128, 128), (2, 5, 8, 64)])
def test_style_table_kernel_against_float64(shape):
    """|T - T64| <= 2 S 2^-24 sum_s |w| |style| elementwise: the fp32 dot-product bound (S - 1 roundings of at most 2^-24 relative
    each on a sum of magnitude <= sum |w| |style|, rounded up to S) with a factor 2 for the final rounding -- derived, not measured."""
    from deepsee_amd import lib as L
    n, l, s, rows = shape
    g = gen(31 + s + l)
    wst = torch.randn(9 * rows, s, generator=g).cuda()
    style = (torch.rand(n, l, s, generator=g) * 2 - 1).cuda()
    slot = torch.zeros(2048, device="cuda")
    t = run_table(style, wst, rows, slot)
    torch.cuda.synchronize()
    w64, s64 = wst.double().cpu(), style.double().cpu()
    t64 = torch.einsum("qs,nrs->nqr", w64, s64).reshape(n, 9, rows, l)
    bound = 2.0 * s * 2.0 ** -24 * torch.einsum("qs,nrs->nqr", w64.abs(), s64.abs()).reshape(n, 9, rows, l)
    err = (t[..., :l].double().cpu() - t64).abs()
    print("shape %s: max |T - T64| / bound = %.3f" % (shape, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    assert bool((t[..., l:] == 0).all()), "columns r >= L are exactly 0"
    assert torch.equal(run_table(style, wst, rows, torch.zeros(2048, device="cuda")), t), "two runs are bit-equal"
    # the slot: max(previous, max |T|), as dsee_style_table_layout leaves it for the same T -- with a smaller and a larger previous value
    tmax = float(t.abs().max())
    assert slot_max(slot) == tmax
    flat = t[..., :l].permute(0, 3, 1, 2).reshape(n * l, 9 * rows).contiguous()        # the kernel's own T, de-laid-out
    for prev in (0.25 * tmax, 4.0 * tmax):
        a, b = torch.zeros(2048, device="cuda"), torch.zeros(2048, device="cuda")
        a[7 * 32] = b[7 * 32] = prev
        run_table(style, wst, rows, a)
        L.call("style_table_layout", flat, torch.empty_like(t), n, l, rows, b)
        torch.cuda.synchronize()
        assert slot_max(a) == slot_max(b) == max(prev, tmax), (prev, tmax, slot_max(a), slot_max(b))
    # shapes outside the rules are refused before a launch
    for bad in ((n, 33, s, rows), (n, l, s + 2, rows), (n, l, s, rows + 32)):
        with pytest.raises(L.DseeError, match="rows % 64 == 0"):
            L.call("style_table_fwd", style, wst, t, *bad, None)


def test_style_table_kernel_between_red_zones():
    n, l, s, rows = 3, 19, 128, 256
    g = gen(5)
    wst = torch.randn(9 * rows, s, generator=g).cuda()
    style = (torch.rand(n, l, s, generator=g) * 2 - 1).cuda()
    plain = run_table(style, wst, rows, torch.zeros(2048, device="cuda"))
    with redzone.guarded() as rz:
        fenced = run_table(style, wst, rows, torch.zeros(2048, device="cuda"))
    assert not rz.passthrough and "style_table_fwd" in rz.guarded
    assert torch.equal(fenced, plain)


# ------------------------------------------------------------------------------------------------ 2. bit identity
@pytest.mark.parametrize("name", list(CASES))
def test_native_generator_is_bit_identical_to_demo_mode(name, monkeypatch):
    from deepsee_amd import ops
    from deepsee_amd.sr_model import SRModel
    c = case(name)
    oracle_is_informative(c)
    model = SRModel(c["opt"])
    model.load_states({"SR": c["sr"]})
    model.eval()
    image_lr, labels, style = device_inputs(c)
    monkeypatch.setattr(ops, "style_table_packed", table_by_the_new_kernel)
    data = {"image_lr": image_lr, "input_semantics": ops.Labels(labels, c["opt"].semantic_nc), "encoded_style": style}
    want = model(data, "demo")["fake_image"]
    got = model.native_generator()(image_lr, labels, style)
    torch.cuda.synchronize()
    print("%s: native vs demo rel %.2e, vs oracle %.2e" % (name, rel(got.cpu(), want.cpu()), rel(got.cpu(), c["want"][0])))
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 3. the oracle
def test_native_generator_matches_the_oracle():
    """O.Oracle.demo on the batch whose bicubic LR image the C path is given: the bound test_inference_mode_matches_oracle holds
    `demo` to."""
    c = case("default")
    oracle_is_informative(c)
    batch = {"label": c["label"], "image": c["image"]}
    orc = O.Oracle(c["oopt"], {"SR": c["sr"]})
    style = c["styles"][0]
    want = orc.demo({k: v.clone() for k, v in batch.items()}, style)
    image_lr = O.bicubic_down(batch["image"], c["opt"].start_size).cuda().contiguous()
    got = native_of(c)(image_lr, device_inputs(c)[1], style.cuda())
    torch.cuda.synchronize()
    dev = rel(got.cpu(), want)
    print("native generator vs the oracle's demo: %.2e" % dev)
    assert dev < 1e-4, dev


# ------------------------------------------------------------------------------------------------ 4. red zones
def test_native_generator_between_red_zones():
    from deepsee_amd.native import NativeGenerator
    c = case("default")
    image_lr, labels, style = device_inputs(c)
    plain = native_of(c)(image_lr, labels, style)
    with redzone.guarded() as rz:
        gen_ = NativeGenerator(c["opt"], c["sr"])
        gen_.prepared = torch.full(((gen_.prepared_bytes + 3) // 4,), float("nan"), device="cuda")
        gen_.prepare()
        n, _, h, w = image_lr.shape
        ws = torch.full(((gen_.workspace_bytes(n, h, w) + 3) // 4,), float("nan"), device="cuda")
        out = torch.full_like(plain, float("nan"))
        gen_(image_lr, labels, style, out=out, workspace=ws)
    assert not rz.passthrough and {"generator_prepare", "generator_fwd"} <= rz.guarded
    assert bool(torch.isfinite(out).all()), "poison leak: an element of the workspace or of `prepared` was read before it was written"
    assert torch.equal(out, plain)


# ------------------------------------------------------------------------------------------------ 5. prepared is read-only
def test_forward_leaves_prepared_alone():
    c = case("default")
    image_lr, labels, style0 = device_inputs(c, 0)
    _, _, style1 = device_inputs(c, 1)
    gen_ = native_of(c)
    before = gen_.prepared.clone()
    gen_(image_lr, labels, style0)
    second = gen_(image_lr.flip(0).contiguous(), labels.flip(0).contiguous(), style1)
    torch.cuda.synchronize()
    assert torch.equal(gen_.prepared.view(torch.int32), before.view(torch.int32))
    fresh = native_of(c)(image_lr.flip(0).contiguous(), labels.flip(0).contiguous(), style1)
    assert torch.equal(second, fresh)


# ------------------------------------------------------------------------------------------------ 6. capture
def test_forward_is_capturable():
    """One linear hipGraph (a single stream, no parallel branches), captured the way TrainerManager captures its steps and
    replayed twice on new contents of the static input buffers."""
    c = case("default")
    gen_ = native_of(c)
    a = device_inputs(c, 0)
    b = (a[0].flip(0).contiguous(), a[1].flip(0).contiguous(), device_inputs(c, 1)[2])
    eager = [gen_(*a).clone(), gen_(*b).clone()]
    static = [torch.empty_like(t) for t in a]
    out = torch.empty_like(eager[0])
    ws = torch.empty((gen_.workspace_bytes(a[0].shape[0], a[0].shape[2], a[0].shape[3]) + 3) // 4, device="cuda")
    for s, t in zip(static, a):
        s.copy_(t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        gen_(*static, out=out, workspace=ws)
    for inputs, want in ((b, eager[1]), (a, eager[0])):
        for s, t in zip(static, inputs):
            s.copy_(t)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ 7. export
def test_export_round_trip(tmp_path):
    import json
    from deepsee_amd.native import NativeGenerator
    c = case("default")
    inputs = device_inputs(c)
    gen_ = native_of(c)
    want = gen_(*inputs)
    path = str(tmp_path / "generator.f32")
    gen_.export(path)
    doc = json.load(open(path + ".json"))
    assert doc["param_floats"] * 4 == (tmp_path / "generator.f32").stat().st_size
    assert [t["key"] for t in doc["tensors"]] == [k for k, _, _ in gen_.entries]
    again = NativeGenerator.from_export(path).prepare()
    assert bytes(again.desc) == bytes(gen_.desc)
    assert torch.equal(again(*inputs), want)
