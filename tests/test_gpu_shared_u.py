"""The shared + per-image layout of a SEAN norm's Winograd-domain weights (dsee_wino43_weights_table_shared, read by
dsee_spade_fused_fwd with groups = -N; plan.shared_u): the 128 embedding columns, whose weights are the same for every image,
stored once per position and only the 32 style-table columns per image.  Nothing is allowed to change, so every comparison is
byte equality on the raw buffers: the layout against the replicated one of dsee_wino43_weights_table slab by slab, the fused
forward on either layout, the whole norm (forward + backward) under plan.shared_u on and off."""
import pytest
import torch
import torch.nn.functional as F

import redzone

pytestmark = pytest.mark.gpu


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _weights(n, rows, ca, nc, seed):
    """(w2a [rows][ca][3][3], table [N][9][rows][32] with the columns past `nc` zero) on the device"""
    g = gen(seed)
    w2a = torch.randn(rows, ca, 3, 3, generator=g) * 0.05
    table = F.pad(torch.randn(n, 9, rows, nc, generator=g) * 0.05, (0, 32 - nc)).contiguous()
    return w2a.cuda(), table.cuda()


def _replicated(w2a, table, n, rows, ca):
    """(U as [36][N][(ca + 32)/16 slabs][rows][32] int16, amax): the replicated layout from the existing producer.  It takes whole
    128-row tiles: fewer rows are built zero-padded (zero rows move neither the maximum nor any other row) and cut out."""
    from deepsee_amd import lib as L, ops
    rp = (rows + 127) // 128 * 128
    if rp != rows:
        w2a = torch.cat([w2a, torch.zeros(rp - rows, ca, 3, 3, device="cuda")]).contiguous()
        table = torch.cat([table, torch.zeros(n, 9, rp - rows, 32, device="cuda")], 2).contiguous()
    ua = ops.weight_amax(w2a, table)
    u = ops._i16(36 * n * rp * (ca + 32) * 2)
    L.call("wino43_weights_table", w2a, table, u, n, rp, ca, 2, ua)
    return u.view(36, n, (ca + 32) // 16, rp, 32)[:, :, :, :rows].contiguous(), ua


def _shared(w2a, table, n, rows, ca, ua):
    """U in the shared layout as [36][ca/16 + 2 N slabs][rows][32] int16, built inside tests/redzone.py's guard bands"""
    from deepsee_amd import lib as L
    u = torch.full((36 * (ca // 16 + 2 * n) * rows * 32,), -1, dtype=torch.int16, device="cuda")
    with redzone.guarded(poison=False):
        L.call("wino43_weights_table_shared", w2a, table, u, n, rows, ca, 2, ua)
    return u.view(36, ca // 16 + 2 * n, rows, 32)


@pytest.mark.parametrize("n,rows,ca,nc", [(3, 128, 128, 19), (3, 128, 32, 19), (3, 64, 128, 19), (2, 64, 32, 5)])
def test_shared_layout_holds_the_words_of_the_replicated_one(n, rows, ca, nc):
    """For every position: the shared slabs equal the first ca/16 slabs of EVERY image's block of the replicated U (so the
    replicas were identical), the table slabs equal each image's last two."""
    w2a, table = _weights(n, rows, ca, nc, 1000 * n + rows + ca + nc)
    rep, ua = _replicated(w2a, table, n, rows, ca)
    sh = _shared(w2a, table, n, rows, ca, ua)
    torch.cuda.synchronize()
    sa = ca // 16
    assert int((rep != 0).sum()) > rep.numel() // 4          # (the producer wrote something)
    for i in range(n):
        assert torch.equal(sh[:, :sa], rep[:, i, :sa]), "shared slabs, image %d" % i
        assert torch.equal(sh[:, sa + 2 * i:sa + 2 * i + 2], rep[:, i, sa:]), "table slabs, image %d" % i


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("h,w", [(32, 32), (32, 64)])
def test_fused_forward_reads_either_layout_to_the_same_bits(h, w, n, c, with_scale):
    """dsee_spade_fused_fwd with groups = -N on the shared layout against groups = N on the replicated one: same V2, statistics
    and bias.  64 and 128 tiles per image, an even and an odd image count (the image term of the table piece), one and two row
    groups (the rg * 4096 term); out, the saved modulation factor, the sign mask and both maxima."""
    from deepsee_amd import lib as L, ops
    rows, ca, K = 2 * c, 128, 160
    g = gen(h + w + 10 * n + c)
    cat = torch.rand(n, h, w, K, generator=g)
    cat[..., ca:] = 0.0
    cat[..., ca:].scatter_(3, torch.randint(0, 19, (n, h, w, 1), generator=g), 1.0)
    x = (torch.randn(n, h, w, c, generator=g) * 3 + 0.5).cuda()
    mean, invstd = (torch.randn(c, generator=g) * 0.3).cuda(), (torch.rand(c, generator=g) + 0.5).cuda()
    b2 = (torch.randn(rows, generator=g) * 0.1).cuda()
    w2a, table = _weights(n, rows, ca, 19, 7 + c + n)
    catd = cat.cuda()
    ac = ops.tensor_amax(catd)
    v2 = ops._i16(36 * n * (h // 4) * (w // 4) * K * 2)
    L.call("wino43_input_f16x2", catd, v2, n, h, w, K, ac, 100.0)
    rep, ua = _replicated(w2a, table, n, rows, ca)
    sh = _shared(w2a, table, n, rows, ca, ua)

    def run(u, groups):
        out = torch.full_like(x, float("nan"))
        sc = torch.full_like(x, float("nan")) if with_scale else None
        mask = torch.full((n * h * w * (c // 32),), 0x5a5a5a5a, dtype=torch.int32, device="cuda") if with_scale else None
        hm, xm = torch.zeros(ops.AMAX_FLOATS, device="cuda"), torch.zeros(ops.AMAX_FLOATS, device="cuda")
        L.call("spade_fused_fwd", v2, u.reshape(-1), ac, 100.0, ua, b2, x, mean, invstd, out, sc, n, h, w, c, rows, K, groups, 1.0,
               0.2, hm, xm, mask)
        torch.cuda.synchronize()
        return out, sc, mask, hm, xm

    want, got = run(rep, n), run(sh, -n)
    assert torch.isfinite(want[0]).all() and float(want[3].max()) == float(want[0].abs().max())
    for name, a, b in zip(("out", "scale", "sign mask", "amax_h", "amax_xhat"), got, want):
        assert (a is None and b is None) or torch.equal(a, b), name


def test_argument_checks_leave_u_unwritten():
    """ca not a multiple of 32, a split kind other than the two-term one (DSEE_EUNSUPPORTED), NULL pointers: an error code and a
    message, and not a byte of U written.  The fused kernel refuses the shared layout where it has no per-image tables."""
    from deepsee_amd import lib as L, ops
    n, rows = 2, 128
    w2a, table = _weights(n, rows, 128, 19, 5)
    ua = ops.weight_amax(w2a, table)
    u = torch.full((36 * (8 + 2 * n) * rows * 32,), 0x1234, dtype=torch.int16, device="cuda")
    for args, code in [((w2a, table, u, n, rows, 48, 2, ua), -1), ((w2a, table, u, n, rows, 0, 2, ua), -1),
                       ((w2a, table, u, n, rows, 128, 4, ua), -3), ((w2a, table, u, n, rows, 128, 0, ua), -3),
                       ((w2a, table, u, n, rows, 128, 1, ua), -3), ((None, table, u, n, rows, 128, 2, ua), -1),
                       ((w2a, None, u, n, rows, 128, 2, ua), -1), ((w2a, table, u, n, rows, 128, 2, None), -1),
                       ((w2a, table, u, n, 96, 128, 2, ua), -1)]:
        with pytest.raises(L.DseeError, match=r"failed \(%d\)" % code):
            L.call("wino43_weights_table_shared", *args)
    with pytest.raises(L.DseeError, match=r"failed \(-1\)"):
        L.call("wino43_weights_table_shared", w2a, table, None, n, rows, 128, 2, ua)
    torch.cuda.synchronize()
    assert bool((u == 0x1234).all())
    # groups = -N needs N per-image tables behind a whole number of 32-column pieces: not -1 of 2 images, not the packed form
    h = c = 32
    x, out = torch.zeros(n, h, h, c, device="cuda"), torch.zeros(n, h, h, c, device="cuda")
    st, v2 = torch.ones(c, device="cuda"), torch.zeros(36 * n * 64 * 160 * 2, dtype=torch.int16, device="cuda")
    for entry, groups in [("spade_fused_fwd", -1), ("spade_fused_fwd_f16p", -n)]:
        with pytest.raises(L.DseeError, match=r"failed \(-1\)"):
            L.call(entry, v2, u, ua, 100.0, ua, st, x, st, st, out, None, n, h, h, c, 2 * c, 160, groups, 1.0, 0.2, None, None, None)


@pytest.mark.parametrize("r,rw", [(32, 32), (32, 64)])
def test_whole_norm_is_the_same_under_either_layout(r, rw):
    """SeanNormTable forward + backward at N = 2, C = 64 under plan.shared_u on and off: the output and every gradient tensor are
    equal.  32 x 64 is the smallest map on which a norm with per-image tables takes the fused kernel (whole 128-tile GEMM tiles
    per image, ops._wino_chunk): there the two runs must have taken the two builders; at 32 x 32 the layer runs the direct
    kernel under either plan."""
    from deepsee_amd import lib as L, networks as Nw, ops
    from oracle import deepsee_oracle as O
    n, c, s, lc = 2, 64, 128, 19
    g = gen(321 + rw)
    label = F.interpolate(torch.randint(0, lc, (n, 1, 8, 8), generator=g).float(), size=(r, rw), mode="nearest")
    labels = ops.Labels(ops.label_to_u8(label.cuda()), lc)
    style0 = (torch.rand(n, lc, s, generator=g) * 2 - 1).cuda()
    x0 = ops.to_nhwc((torch.randn(n, c, r, rw, generator=g) * 1.5 + 0.3).cuda())
    gy = ops.to_nhwc(torch.randn(n, c, r, rw, generator=g).cuda())
    mod = Nw.SpadeNorm("sean", c, lc, s, 256)
    state = {k: O.recipe_tensor("shared_u", k, v.shape, 1.0) for k, v in mod.state_dict().items()}
    mod.cuda()

    def run(shared):
        mod.load_state_dict(state)
        mod.zero_grad(set_to_none=True)
        x, style = x0.clone().requires_grad_(), style0.clone().requires_grad_()
        names, call = [], L.call

        def spy(name, *a):
            names.append(name)
            return call(name, *a)

        L.call = spy
        try:
            with ops.KernelPlan(shared_u=shared).active():
                h = mod(x, labels, style, True)
                h.backward(gy)
        finally:
            L.call = call
        torch.cuda.synchronize()
        fused = (r // 4) * (rw // 4) % 128 == 0
        assert ("spade_fused_fwd" in names) == fused
        assert ("wino43_weights_table_shared" in names) == (fused and shared)
        assert ("wino43_weights_table" in names) == (fused and not shared)
        grads = {k: p.grad.clone() for k, p in mod.named_parameters() if p.grad is not None}
        return h.detach().clone(), x.grad.clone(), style.grad.clone(), grads

    a, b = run(True), run(False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[3].keys() == b[3].keys() and len(a[3]) >= 4
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
