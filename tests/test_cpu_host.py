"""CPU-only checks: the C-ABI library loads and exports every symbol of include/deepsee_hip.h, the host-side
mirror of the reference interface (state-dict layout, block plan, option presets, conv geometry, packed gamma/beta
row order) and the data-parallel gradient exchange on gloo with world_size 2."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.multiprocessing as mp

from oracle import deepsee_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capi_library_loads_and_exports_header_symbols():
    from deepsee_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    so = ctypes.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "deepsee_hip.h")).read()
    names = sorted(set(re.findall(r"\b(dsee_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 40
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, missing
    so.dsee_version.restype = ctypes.c_int
    assert so.dsee_version() >= 100
    # pure host helpers (no GPU needed)
    assert so.dsee_conv_kpad(3, 3, 512) == 4608 and so.dsee_conv_kpad(4, 4, 24) == 384
    assert so.dsee_conv_wrows(3) == 128 and so.dsee_conv_wrows(512) == 512
    # argument validation returns an error code + message instead of launching
    so.dsee_last_error.restype = ctypes.c_char_p
    rc = so.dsee_conv2d_fwd(None, None, None, None, None, 0, None, 0, ctypes.c_float(0.2), None)
    assert rc == -1 and b"argument check failed" in so.dsee_last_error()


def test_coarse_entry_points_validate_before_they_launch():
    """The coarse entry points (csrc/coarse.cpp) size their caller-owned workspace on the host and refuse bad arguments with an
    error code and a message before any HIP call (so this runs without a GPU)."""
    from deepsee_amd import lib as L
    so = L.lib()
    n1 = so.dsee_sean_norm_fwd_workspace(8, 256, 256, 512, 19, 1)
    n0 = so.dsee_sean_norm_fwd_workspace(8, 256, 256, 512, 19, 0)
    t = 8 * 64 * 64
    # embedding + V2 + U2 dominate: [N,H,W,160] fp32, 36 T 160 two fp16 terms, 36 N 1024 160 two fp16 terms
    assert n1 >= 8 * 256 * 256 * 160 * 4 + 36 * t * 160 * 4 + 36 * 8 * 1024 * 160 * 4 and n1 < 2.2e9
    assert n0 < n1 and n0 >= 8 * 256 * 256 * 128 * 4 + 36 * t * 128 * 4
    nb = so.dsee_spade_resblock_fwd_workspace(8, 256, 256, 512, 19, 1)
    assert nb >= n1 + 2 * 8 * 256 * 256 * 512 * 4 + 2 * 36 * t * 512 * 4 and nb < 9e9
    args = [None] * 24 + [8, 256, 256, 512, None, 0]
    assert len(args) + 1 == len(so.dsee_sean_norm_fwd.argtypes)
    args[1:5] = [256, 256, 0, 19]
    args[13:18] = [1, 1e-5, 0.1, 1.0, 0.2]
    rc = so.dsee_sean_norm_fwd(*args, None)
    assert rc == -1 and b"NULL argument" in so.dsee_last_error()
    rc = so.dsee_spade_resblock_fwd(*([None] * 6), None, 256, 256, 0, 19, None, None, 0, 1, 1e-5, 0.1, 0.2, 8, 256, 256, 512, None,
                                    0, None)
    assert rc == -1 and b"NULL argument" in so.dsee_last_error()
    # round 6: the training pair -- saved area and workspaces sized on the host, NULL / shape validation before any HIP call
    sb = so.dsee_spade_resblock_saved_bytes(8, 64, 64, 512, 19, 1)
    t64 = 8 * 16 * 16
    assert sb >= 3 * 8 * 64 * 64 * 512 * 4 + 2 * 36 * t64 * 512 * 4 + 2 * 36 * t64 * 160 * 4 and sb < 0.7e9
    assert so.dsee_spade_resblock_saved_bytes(8, 64, 64, 512, 19, 0) < sb
    assert so.dsee_spade_resblock_train_fwd_workspace(8, 64, 64, 512, 19, 1) > 36 * t64 * 512 * 4
    assert so.dsee_spade_resblock_bwd_workspace(8, 64, 64, 512, 19, 1, 256, 256, 2) > 36 * t64 * 1024 * 4
    assert len(so.dsee_spade_resblock_train_fwd.argtypes) == 26 and len(so.dsee_spade_resblock_bwd.argtypes) == 26
    rc = so.dsee_spade_resblock_train_fwd(*([None] * 8), 256, 256, 2, 19, None, None, 1e-5, 0.1, 0.2, 8, 64, 64, 512, None, 0, None, 0,
                                          None)
    assert rc == -1 and b"NULL argument" in so.dsee_last_error()
    rc = so.dsee_spade_resblock_bwd(*([None] * 6), 256, 256, 2, 19, *([None] * 6), 0.2, 8, 64, 64, 512, None, 0, None, 0, None)
    assert rc == -1 and b"NULL argument" in so.dsee_last_error()


def test_ctypes_prototypes_come_from_the_header():
    """deepsee_amd.lib binds every entry point with the argtypes / restype parsed from include/deepsee_hip.h: a call with
    the wrong arity, or a float where the header says int, raises instead of corrupting the stack; long / size_t /
    uint64_t arguments are passed at their declared width."""
    import ctypes as C
    from deepsee_amd import lib as L
    protos = L.header_prototypes()
    so = L.lib()
    assert len(protos) >= 75 and all(getattr(so, n).argtypes == a for n, (_, a) in protos.items())
    assert protos["dsee_gemm_bf16x3_af32"][1][3] is C.c_long and protos["dsee_rng_fill"][1][2] is C.c_uint64
    assert protos["dsee_conv2d_wgrad_workspace"][0] is C.c_size_t and protos["dsee_last_error"][0] is C.c_char_p
    # a long that does not fit an int: truncated to 32 bits it would be M = 100 -> 2 partial rows instead of 1024
    assert so.dsee_channel_dot_workspace(100, 512) == 2 * 512 * 4
    assert so.dsee_channel_dot_workspace((1 << 33) + 100, 512) == 1024 * 512 * 4
    with pytest.raises(TypeError):
        so.dsee_conv_kpad(3, 3)
    with pytest.raises(C.ArgumentError):
        so.dsee_conv_kpad(3, 3, 1.5)
    if not torch.cuda.is_available():
        return
    with pytest.raises(L.DseeError):
        L.call("act_fwd", None, None, 4)                                          # arity checked before the call


def test_product_refuses_to_run_without_gpu():
    from deepsee_amd.options import make_opt
    from deepsee_amd.sr_model import SRModel
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        SRModel(make_opt("independent_8x_32"))


@pytest.mark.parametrize("over", [
    dict(), dict(start_size=4, crop_size=32, load_size=32), dict(start_size=16, crop_size=512, load_size=512, add_noise=False),
    dict(netE="fullstyle", noisy_style_scale=0.05, guiding_style_image=True), dict(ngf=8, add_noise=False)])
def test_state_dict_layout_matches_reference_spec(over):
    """Keys/shapes of the build's modules == the oracle's spec, which gen_golden.py asserts equal to the real
    reference's state_dict(): checkpoints interchange."""
    from deepsee_amd import networks as N
    from deepsee_amd.options import make_opt
    from deepsee_amd.sr_model import block_plan
    opt = make_opt(**over)
    oopt = O.make_opt(**over)
    assert block_plan(opt) == O.block_plan(oopt)
    spec = O.net_specs(oopt)
    nets = {"SR": N.DeepSEESR(opt, block_plan(opt)), "D": N.MultiscaleDiscriminator(opt), "E": N.StyleEncoder(opt),
            "VGG": N.VGG19Taps()}
    for label, net in nets.items():
        got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        want = {k: tuple(s) for k, s in spec[label].items()}
        assert got == want, (label, set(got) ^ set(want))
    if "full" not in opt.netE:
        n_main = sum(1 for k, _ in nets["SR"].named_parameters()) + sum(
            1 for k, _ in nets["E"].named_parameters() if "mini" not in k)
        n_low = sum(1 for k, _ in nets["E"].named_parameters() if "mini" in k)
        orc = O.Oracle(oopt, O.init_state(oopt))
        orc.create_optimizers()
        assert [len(g["params"]) for g in orc.opt_G.param_groups] == [n_main, n_low]


def test_option_presets():
    from deepsee_amd.options import make_opt
    o = make_opt("guided_8x_256")
    assert o.netE == "fullstyle" and o.guiding_style_image and o.noisy_style_scale == 0.05 and o.start_size == 32
    o = make_opt("independent_32x_512")
    assert o.start_size == 16 and o.crop_size == 512 and not o.add_noise and o.load_size == 512
    assert make_opt().lr == 2e-4 and make_opt().beta1 == 0.0 and make_opt().beta2 == 0.9


def test_conv_geometry_and_packing_helpers():
    from deepsee_amd import lib as L, ops
    g = L.geom_fwd(2, 17, 17, 24, 32, 4, 2, 2)
    assert (g.Ho, g.Wo) == (9, 9) and (g.mul, g.off, g.kdir, g.dshift) == (2, -2, 1, 0)
    d = L.geom_dgrad(g)
    assert (d.Hi, d.Ho, d.Cin, d.Cout) == (9, 17, 32, 24) and (d.mul, d.off, d.kdir, d.dshift) == (1, 2, -1, 1)
    g = L.geom_fwd(1, 8, 8, 128, 256, 3, 1, 1, ups=1)
    assert (g.Ho, g.Wo) == (16, 16)
    for c in (8, 64, 96, 512):
        idx, rows = ops.packed_perm(c, "cpu")
        assert rows == (c + 63) // 64 * 128
        real = idx[idx < 2 * c]
        assert sorted(real.tolist()) == list(range(2 * c))          # every gamma/beta row appears exactly once
        for p in range(rows):                                        # gamma at p, beta of the same channel at p+32
            if (p % 64) < 32 and idx[p] < 2 * c:
                assert idx[p + 32] == idx[p] + c


GOLD = os.path.join(ROOT, "tests", "golden")


def test_init_weights_statistics_match_reference():
    """deepsee_amd.sr_model.init_weights on the build's parameter holders vs the per-tensor statistics of a
    freshly initialised REFERENCE model (tests/golden/host_logic.json, written by oracle/gen_golden.py): xavier /
    kaiming std of every conv weight incl. spectral-norm weight_orig, biases / noise weights / running_mean exactly 0,
    running_var 1, alpha in [0,1), ||u|| = ||v|| = 1."""
    import json
    from deepsee_amd import networks as N
    from deepsee_amd.options import make_opt
    from deepsee_amd.sr_model import block_plan, init_weights
    from tests.test_oracle_golden import check_init_stats
    host = json.load(open(os.path.join(GOLD, "host_logic.json")))
    for tag, rec in host["init"].items():
        opt = make_opt(**rec["opt"])
        gen = torch.Generator().manual_seed(17)
        nets = {"SR": N.DeepSEESR(opt, block_plan(opt)), "D": N.MultiscaleDiscriminator(opt), "E": N.StyleEncoder(opt)}
        for net in nets.values():
            init_weights(net, opt.init_type, opt.init_variance, gen)
        check_init_stats({"%s/%s" % (n, k): v for n, net in nets.items() for k, v in net.state_dict().items()},
                         rec["stats"])


def test_update_learning_rate_matches_reference_schedule():
    """TrainerManager.update_learning_rate against the learning rates the REAL reference's TrainerManager set
    on every param group at every epoch (tests/golden/host_logic.json; trainer_manager.py:76-96)."""
    import json
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    host = json.load(open(os.path.join(GOLD, "host_logic.json")))

    class Opt:   # optimizer stand-in with the surface update_learning_rate touches
        def __init__(self, lrs):
            self.param_groups = [{"lr": lr} for lr in lrs]

    for tag, rec in host["lr_schedule"].items():
        over = {k: v for k, v in rec["opt"].items() if k != "lr"}
        opt = make_opt(**over)
        assert opt.lr == rec["opt"]["lr"]
        tm = object.__new__(TrainerManager)
        tm.opt, tm.old_lr = opt, opt.lr
        lr_g, lr_d = (opt.lr, opt.lr) if opt.no_TTUR else (opt.lr / 2, opt.lr * 2)
        tm.optimizer_G, tm.optimizer_D = Opt([lr_g, lr_g / 4]), Opt([lr_d])
        for row in rec["rows"]:
            tm.update_learning_rate(row["epoch"])
            assert [g["lr"] for g in tm.optimizer_G.param_groups] == pytest.approx(row["G"], rel=1e-12, abs=1e-18)
            assert [g["lr"] for g in tm.optimizer_D.param_groups] == pytest.approx(row["D"], rel=1e-12, abs=1e-18)
            assert tm.old_lr == pytest.approx(row["old_lr"], rel=1e-12, abs=1e-18)


def _dp_worker(rank, world, port, q):
    # DSEE_ONE_DEVICE: on a box with a GPU, init_distributed binds every rank to cuda:0 (a one-GPU box has no cuda:1); the
    # tensors of these workers stay on the host either way
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DSEE_ONE_DEVICE="1")
    sys.path.insert(0, ROOT)
    import random
    import torch.distributed as dist
    from deepsee_amd import parallel
    r, _, w = parallel.init_distributed(backend="gloo")
    assert (r, w) == (rank, world)
    g = torch.Generator().manual_seed(100 + rank)
    flat = torch.randn(10_007 * 4, generator=g)
    mine = flat.clone()
    hook = parallel.GradAllReduce(world, chunk_mb=0.05)   # ~13k floats per chunk -> several chunks
    scale = hook(flat)
    other = torch.randn(10_007 * 4, generator=torch.Generator().manual_seed(100 + (1 - rank)))
    ok = abs(scale - 0.5) < 1e-12 and torch.allclose(flat, mine + other, atol=1e-6)
    random.seed(1234)                                      # same branch coins on every rank
    coins = [random.random() for _ in range(4)]
    t = torch.tensor(coins, dtype=torch.float64)
    dist.all_reduce(t)
    ok = ok and torch.allclose(t / world, torch.tensor(coins, dtype=torch.float64))
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_grad_allreduce_gloo_world2():
    from deepsee_amd import parallel
    assert parallel.chunk_bounds(10, 4) == [(0, 4), (4, 8), (8, 10)]
    assert parallel.chunk_bounds(8, 3)[0] == (0, 4)        # chunk sizes stay 16-byte aligned
    assert _spawn(_dp_worker) == [(0, True), (1, True)]


def _spawn(fn, world=2, timeout=180):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + ((os.getpid() * 7 + hash(fn.__name__)) % 2000)
    procs = [ctx.Process(target=fn, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=timeout) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    return sorted(res)


def _init_gloo(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DSEE_ONE_DEVICE="1")      # (see _dp_worker)
    sys.path.insert(0, ROOT)
    from deepsee_amd import parallel
    r, _, w = parallel.init_distributed(backend="gloo")
    assert (r, w) == (rank, world)
    return parallel


def _flat_adam_worker(rank, world, port, q):
    """Drives the REAL FlatAdam.step host logic (descriptor upload, `touched` MAX-reduce, block-aligned chunking,
    per-chunk wait -> update, step bump, lr change) under gloo; only the Adam kernel launch itself is replaced by a torch
    emulation reading the same device descriptors (the HIP kernel cannot run without a GPU)."""
    import numpy as np
    import torch.distributed as dist
    parallel = _init_gloo(rank, world, port)
    from deepsee_amd.optim import ADAM_DT, BLOCK, FlatAdam

    class CpuAdam(FlatAdam):
        launches = 0

        def _gather(self):      # torch emulation of dsee_grad_gather: flat gradient (zeros without a gradient) + active flags
            self.grad.zero_()
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                if p.grad is not None:
                    self.grad[o:o + p.numel()].copy_(p.grad.reshape(-1))
                self._active_dev[i] = 0 if p.grad is None else 1
                self.grad[i] = 0.0 if p.grad is None else 1.0      # header flag (rides in the first all-reduced chunk)

        def _launch(self, b0, b1, grad_scale, clip):
            CpuAdam.launches += 1
            desc = np.frombuffer(self.desc_dev.numpy().tobytes(), dtype=ADAM_DT)
            bt = self.block_tensor.numpy()
            b1_, b2_ = self.betas
            for blk in range(b0, b1):
                d = desc[bt[blk]]
                if not d["active"]:
                    continue
                lo = int(d["offset"]) + (blk - int(d["first_block"])) * BLOCK
                hi = min(int(d["offset"] + d["numel"]), lo + BLOCK)
                step = int(d["step"]) + 1
                g = self.grad[lo:hi] * grad_scale
                if clip > 0:
                    g = g.clamp(-clip, clip)
                self.exp_avg[lo:hi].mul_(b1_).add_(g, alpha=1 - b1_)
                self.exp_avg_sq[lo:hi].mul_(b2_).addcmul_(g, g, value=1 - b2_)
                denom = self.exp_avg_sq[lo:hi].sqrt() / (1 - b2_ ** step) ** 0.5 + self.eps
                self.flat[lo:hi].sub_(float(d["lr"]) / (1 - b1_ ** step) * self.exp_avg[lo:hi] / denom)

    sizes = [(3000,), (5,), (32, 32), (2500,), (7,), (1100,)]
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=gen) for s in sizes]
    params = [torch.nn.Parameter(t.clone()) for t in init]
    named = [("p%d" % i, p) for i, p in enumerate(params)]
    opt = CpuAdam([{"params": named[:4], "lr": 1e-2}, {"params": named[4:], "lr": 2.5e-3}], betas=(0.5, 0.9))
    opt.reduce_hook = parallel.GradAllReduce(world, chunk_mb=2000 * 4 / (1 << 20))       # ~2000 floats per chunk
    ranges = opt.chunk_ranges(opt.reduce_hook.chunk_elems)
    ok = len(ranges) >= 3 and ranges[0][2] == 0 and ranges[-1][3] == opt.total
    ok = ok and all(a[3] == b[2] and a[1] == b[0] for a, b in zip(ranges, ranges[1:]))      # tile blocks and elements
    # reference: plain torch Adam on the rank-averaged gradients, every tensor that ANY rank touched is active
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    ropt = torch.optim.Adam([{"params": ref[:4], "lr": 1e-2}, {"params": ref[4:], "lr": 2.5e-3}], betas=(0.5, 0.9))
    for it in range(3):
        coef = [[torch.randn(s, generator=torch.Generator().manual_seed(1000 * it + 10 * r + i))
                 for i, s in enumerate(sizes)] for r in range(world)]
        # tensor 3 gets a gradient on rank 0 only, tensor 4 on no rank in iteration 1 (skipped: its step must not advance)
        def touched(r, i):
            return not (i == 3 and r == 1) and not (i == 4 and it == 1)
        opt.zero_grad()
        sum((p * coef[rank][i]).sum() for i, p in enumerate(params) if touched(rank, i)).backward()
        if it == 2:
            opt.param_groups[0]["lr"] = 5e-3                                                   # update_learning_rate
            ropt.param_groups[0]["lr"] = 5e-3
        opt.step()
        ropt.zero_grad()
        for i, p in enumerate(ref):
            gs = [coef[r][i] for r in range(world) if touched(r, i)]
            p.grad = sum(gs) / world if gs else None
        ropt.step()
    err = max(float((p.detach() - r.detach()).abs().max()) for p, r in zip(params, ref))
    steps = opt.steps().tolist()
    ok = ok and err < 2e-6 and steps == [3, 3, 3, 3, 2, 3] and CpuAdam.launches == 3 * len(ranges)
    # every rank ends with the same parameters
    t = opt.flat.clone()
    dist.all_reduce(t)
    ok = ok and torch.allclose(t / world, opt.flat, atol=0, rtol=0)
    q.put((rank, bool(ok), err, steps))
    dist.barrier()
    dist.destroy_process_group()


def test_flat_adam_chunked_allreduce_gloo_world2():
    res = _spawn(_flat_adam_worker)
    assert [r[:2] for r in res] == [(0, True), (1, True)], res


def _syncbn_worker(rank, world, port, q):
    """SyncBN-over-RCCL protocol under gloo: the product's exchange functions (parallel.gather_stats,
    parallel.allreduce_sums) around torch emulations of the three kernels (dsee_norm_stats_local, dsee_norm_stats_merge,
    the dsee_modulate_bwd reduce/apply halves), against the oracle's restatement of the reference's DataParallel branch
    on the concatenated batch (pinned to the reference by tests/golden/host_logic.json)."""
    import torch.distributed as dist
    parallel = _init_gloo(rank, world, port)
    from oracle import deepsee_oracle as O
    c, eps, mom = 8, 1e-5, 0.1
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(4, c, 6, 6, generator=g) * 3 + 1).double()
    x[:, 7] = 0.25
    shards = [x[:2], x[2:]]
    mine = shards[rank]
    # dsee_norm_stats_local: (mean, M2) of this rank's shard
    flat = mine.transpose(0, 1).reshape(c, -1)
    local = torch.stack([flat.mean(1), ((flat - flat.mean(1, keepdim=True)) ** 2).sum(1)])
    rows = parallel.gather_stats(local, world)
    ok = tuple(rows.shape) == (world, 2, c)
    # dsee_norm_stats_merge: Chan's update in rank order, clamp(var, eps)
    n = mean = m2 = 0.0
    cnt = flat.shape[1]
    for r in range(world):
        d = rows[r, 0] - mean
        nt = n + cnt
        mean = mean + d * cnt / nt
        m2 = m2 + rows[r, 1] + d * d * n * cnt / nt
        n = nt
    var = m2 / n
    inv_std = var.clamp(min=eps) ** -0.5
    rm, rv = mom * mean, (1 - mom) * 1.0 + mom * var * n / (n - 1)
    xs = [s.clone().requires_grad_(True) for s in shards]
    omean, oinv, orm, orv, outs = O.sync_bn_master(xs, torch.zeros(c).double(), torch.ones(c).double(), eps, mom)
    for a, b in ((mean, omean), (inv_std, oinv), (rm, orm), (rv, orv)):
        ok = ok and torch.allclose(a, b.detach(), rtol=1e-9, atol=1e-12)
    # backward: sum d, sum d*xhat over the GLOBAL batch (allreduce_sums), dx = inv_std (d - S0/M - xhat S1/M)
    R = [torch.randn(s.shape, generator=torch.Generator().manual_seed(9 + i)).double() for i, s in enumerate(shards)]
    sum((o * r).sum() for o, r in zip(outs, R)).backward()
    xhat = (mine - mean[None, :, None, None]) * inv_std[None, :, None, None]
    d = R[rank]
    sums = torch.stack([d.transpose(0, 1).reshape(c, -1).sum(1), (d * xhat).transpose(0, 1).reshape(c, -1).sum(1)])
    parallel.allreduce_sums(sums, world)
    m_tot = world * cnt
    dx = inv_std[None, :, None, None] * (d - sums[0][None, :, None, None] / m_tot
                                         - xhat * sums[1][None, :, None, None] / m_tot)
    live = [ch for ch in range(c) if ch != 7]          # the clamped channel has no variance gradient in the reference
    ok = ok and torch.allclose(dx[:, live], xs[rank].grad[:, live], rtol=1e-8, atol=1e-10)
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


def test_syncbn_exchange_protocol_gloo_world2():
    assert _spawn(_syncbn_worker) == [(0, True), (1, True)]


def test_device_input_pipeline_host_side(tmp_path):
    """SURVEY 8 f3, host half: datasets yield the uint8 wire format, FolderDataset pairs files by stem and applies the
    reference's resize + crop (base_dataset.py:87-116,171-201), DeviceLoader shards an epoch disjointly over the ranks;
    the oracle's restatement of ToTensor + Normalize + flip is what the HIP kernels are checked against on the GPU."""
    import numpy as np
    from PIL import Image
    from deepsee_amd import data as D
    from deepsee_amd.options import make_opt
    opt = make_opt(start_size=4, crop_size=32, load_size=40, batchSize=2)
    ds = D.SyntheticDataset(opt, length=10, seed=3)
    s = ds[4]
    assert s["label"].dtype == np.uint8 and s["label"].shape == (32, 32) and int(s["label"].max()) < opt.label_nc
    assert s["image"].dtype == np.uint8 and s["image"].shape == (32, 32, 3) and s["flip"] in (0, 1)
    assert np.array_equal(ds[4]["image"], s["image"])                      # deterministic per index
    for d_ in ("lab", "img"):
        os.makedirs(str(tmp_path / d_))
    rng = np.random.default_rng(0)
    for k in range(3):
        lab = rng.integers(0, 19, size=(48, 48), dtype=np.uint8)
        lab[0, 0] = 255
        Image.fromarray(lab).save(str(tmp_path / "lab" / ("%d.png" % k)))
        Image.fromarray(rng.integers(0, 256, size=(48, 48, 3), dtype=np.uint8)).save(str(tmp_path / "img" / ("%d.png" % k)))
    fd = D.FolderDataset(opt, str(tmp_path / "lab"), str(tmp_path / "img"), seed=1)
    assert len(fd) == 3
    it = fd[1]
    assert it["label"].shape == (32, 32) and it["image"].shape == (32, 32, 3) and it["path"].endswith("1.png")
    # the crop is the same window of the NEAREST-resized label and the BICUBIC-resized image
    full = np.asarray(Image.open(str(tmp_path / "lab" / "1.png")).resize((40, 40), Image.NEAREST))
    assert any(np.array_equal(it["label"], full[y:y + 32, x:x + 32]) for y in range(9) for x in range(9))
    # options: opt.no_flip is honoured (an explicit argument overrides it), unsupported preprocess modes and multi-channel
    # label files are refused instead of silently mis-handled
    import pytest
    assert all(D.FolderDataset(make_opt(start_size=4, crop_size=32, load_size=40, no_flip=True), str(tmp_path / "lab"),
                               str(tmp_path / "img"), seed=s_)[0]["flip"] == 0 for s_ in range(6))
    assert any(D.FolderDataset(opt, str(tmp_path / "lab"), str(tmp_path / "img"), seed=s_)[0]["flip"] == 1 for s_ in range(6))
    with pytest.raises(ValueError):
        D.FolderDataset(make_opt(start_size=4, crop_size=32, load_size=40, preprocess_mode="scale_width"),
                        str(tmp_path / "lab"), str(tmp_path / "img"))
    with pytest.raises(ValueError):
        D.FolderDataset(opt, str(tmp_path / "img"), str(tmp_path / "img"))[0]     # RGB files as label maps
    # sharding: two ranks, disjoint and equally long
    l0 = D.DeviceLoader(ds, opt, shard=(0, 2), seed=5)
    l1 = D.DeviceLoader(ds, opt, shard=(1, 2), seed=5)
    i0, i1 = l0.indices(), l1.indices()
    assert len(i0) == len(i1) == 5 and not set(i0) & set(i1) and len(l0) == 2
    b = l0.collate([ds[i] for i in i0[:2]])
    assert b["label"].dtype == torch.uint8 and tuple(b["image"].shape) == (2, 32, 32, 3) and b["flip"].dtype == torch.uint8
    # oracle restatement of the device half (the GPU test compares the HIP kernels with exactly this)
    img, lab = O.device_pipeline_reference(b["image"], b["label"], b["flip"], opt.label_nc)
    assert tuple(img.shape) == (2, 3, 32, 32) and float(img.min()) >= -1.0 and float(img.max()) <= 1.0
    k = int(torch.nonzero(b["flip"])[0]) if int(b["flip"].sum()) else None
    if k is not None:
        assert torch.equal(lab[k, 0], b["label"][k].flip(-1).float())


def test_bf16x3_split_arithmetic_emulated_on_cpu():
    """The numerical argument behind deepsee_amd/csrc/gemm_bf16x3.hip, emulated with torch on the CPU: an fp32 value is
    EXACTLY the sum of three bf16 terms, and the six partial products of weight above 2^-26 accumulated in fp32 give a
    GEMM error (vs float64) no larger than a plain fp32 GEMM's; with only three products it is ~16x larger."""
    import torch
    g = torch.Generator().manual_seed(0)
    a = torch.randn(256, 512, generator=g) * torch.rand(256, 1, generator=g).exp()
    b = torch.randn(512, 192, generator=g)

    def split(x):
        x0 = x.bfloat16().float()
        r = x - x0
        x1 = r.bfloat16().float()
        r = r - x1
        x2 = r.bfloat16().float()
        assert torch.equal(x0 + x1 + x2, x) and float((r - x2).abs().max()) == 0.0
        return x0, x1, x2

    a0, a1, a2 = split(a)
    b0, b1, b2 = split(b)
    ref = a.double() @ b.double()
    err = lambda y: float((y.double() - ref).norm() / ref.norm())
    acc = torch.zeros(256, 192)
    for k in range(0, 512, 16):                      # one MFMA = 16 k's; smallest terms first, one fp32 accumulator
        s = slice(k, k + 16)
        for x, y in ((a2, b0), (a1, b1), (a0, b2), (a1, b0), (a0, b1), (a0, b0)):
            acc = acc + x[:, s] @ y[s]
    e6, e32 = err(acc), err(a @ b)
    e3 = err(a0 @ b0 + (a0 @ b1 + a1 @ b0))
    assert e6 <= 1.5 * e32 and e6 < 5e-7, (e6, e32)
    assert e3 > 8 * e6                               # the three small products are what makes it fp32-accurate


def test_f16x2_split_arithmetic_emulated_on_cpu():
    """The numerical argument behind the fp16x2 form of deepsee_amd/csrc/gemm_bf16x3.hip, emulated with torch on the
    CPU: after scaling by a power of two that brings the largest element into [2^13, 2^14), an fp32 value differs from
    the sum of two fp16 terms (2 x 11 significand bits) by at most 2^-22 of its magnitude -- rms 2^-24, the size of one
    fp32 rounding -- or 2^-25 absolute where the second term goes subnormal, and the three products a1*b0 + a0*b1 + a0*b0
    accumulated in fp32 give a GEMM error (vs float64) no larger than a plain fp32 GEMM's (the accumulator's rounding
    dominates both) -- also on data spread over e^(+-8)."""
    import math
    g = torch.Generator().manual_seed(0)

    def split(x):
        amax = float(x.abs().max())
        s = 2.0 ** (13 - math.floor(math.log2(amax)))
        xs = x * s
        assert 2.0 ** 13 <= float(xs.abs().max()) < 2.0 ** 14
        h0 = xs.half().float()
        h1 = (xs - h0).half().float()
        err = (xs - h0 - h1).abs()
        assert bool((err <= torch.maximum(xs.abs() * 2.0 ** -22, torch.tensor(2.0 ** -25))).all())
        big = xs.abs() > 1.0
        assert float(((err[big] / xs.abs()[big]) ** 2).mean().sqrt()) < 2.0 ** -23.5
        return h0, h1, s

    for spread in (0.0, 2.0):
        a = torch.randn(256, 512, generator=g) * (torch.randn(256, 512, generator=g) * spread).exp()
        b = torch.randn(512, 192, generator=g) * 0.02
        a0, a1, sa = split(a)
        b0, b1, sb = split(b)
        ref = a.double() @ b.double()
        err = lambda y: float((y.double() - ref).norm() / ref.norm())
        acc = torch.zeros(256, 192)
        for k in range(0, 512, 16):                  # one MFMA = 16 k's; smallest terms first, one fp32 accumulator
            sl = slice(k, k + 16)
            for x, y in ((a1, b0), (a0, b1), (a0, b0)):
                acc = acc + x[:, sl] @ y[sl]
        e3, e32 = err(acc / (sa * sb)), err(a @ b)
        e1 = err((a0 @ b0) / (sa * sb))
        assert e3 <= 1.5 * e32 and e3 < 5e-7, (spread, e3, e32)
        assert e1 > 100 * e3                          # one product alone is fp16 accuracy: the cross terms carry it


def test_style_matrix_csv_roundtrip(tmp_path):
    """deepsee_amd.util.save_style_matrix writes what the reference's util/util.py:150-158 writes (numpy.savetxt with
    ',' delimiter) and load_style_matrix reads it back bit-exactly in fp32."""
    import numpy as np
    import torch
    from deepsee_amd.util import load_style_matrix, save_style_matrix
    m = (torch.rand(19, 128, generator=torch.Generator().manual_seed(3)) * 2 - 1)
    p = str(tmp_path / "sub" / "style.csv")
    save_style_matrix(m, p, create_dir=True)
    want = str(tmp_path / "ref.csv")
    np.savetxt(want, np.array(m), delimiter=",")
    assert open(p).read() == open(want).read()
    assert torch.equal(load_style_matrix(p, device="cpu"), m)
    import pytest
    with pytest.raises(AssertionError):
        save_style_matrix(m[None], p)


def test_rank_core_sets_partition_the_allowed_cores():
    """deepsee_amd.parallel.rank_core_set: the ranks of a node get disjoint, contiguous, equally sized core sets that
    cover the allowed cores (8 launch threads on one host must not share cores); more ranks than cores degrade to sharing."""
    from deepsee_amd import parallel
    cores = list(range(4, 36))
    sets = [parallel.rank_core_set(r, 8, cores) for r in range(8)]
    assert all(len(s) == 4 for s in sets)
    assert sorted(c for s in sets for c in s) == cores
    assert all(s == list(range(s[0], s[0] + 4)) for s in sets)
    assert parallel.rank_core_set(5, 8, [0, 1]) == [0, 1]          # fewer cores than ranks: everybody keeps what there is
    assert parallel.pin_rank_cores(0, 1) is None                   # single rank: untouched


def test_presplit_path_selection_rules():
    """Host-side rules that decide when a Winograd layer takes round 3's pre-split operand kernels (deepsee_amd/ops.py): the
    input's maximum must have been written by its producer, the GEMM must be big enough for 256 x 256 tiles, and -- when the
    weight gradient will read the same V2 -- the reduction width must be one the transpose-read TN kernel takes."""
    import torch
    from deepsee_amd import ops
    x = torch.zeros(1)
    assert not ops._presplit_ok(x, 32768, 32768, 512)                       # no maximum known in advance
    x.dsee_amax = torch.zeros(2048)
    assert ops._presplit_ok(x, 32768, 32768, 512)                           # 512 -> 512 @256^2, bs = 8
    assert ops._presplit_ok(x, 2048, 2048, 512)                             # @64^2: 288 x 2 tiles of 256 x 256
    assert not ops._presplit_ok(x, 512, 512, 512)                           # @32^2: too few tiles, 128 x 128 kernel
    assert not ops._presplit_ok(x, 32768, 32768, 384)                       # output width not a multiple of 256
    assert not ops._presplit_ok(x, 32768, 4096 + 64, 512)                   # group size not a multiple of 256
    assert ops._presplit_ok(x, 32768, 32768, 512, k_s=160, keep=True) and ops._presplit_ok(x, 32768, 32768, 512, 256, True)
    assert not ops._presplit_ok(x, 32768, 32768, 512, k_s=96, keep=True)    # TN kernel: 160 or a multiple of 128 columns
    with ops.KernelPlan(presplit_a=False).active():
        assert not ops._presplit_ok(x, 32768, 32768, 512)
    assert ops.P() is ops.DEFAULT_PLAN and ops._presplit_ok(x, 32768, 32768, 512)
    # the channel sums that ride in the A dY A^T pass / the statistics rows of a producer need 256 % (C/4) == 0
    assert ops._dout_sums_ok(8, 8, 512, 2) and not ops._dout_sums_ok(8, 4, 512, 2) and not ops._dout_sums_ok(8, 8, 512, 1)
    assert ops._stats_rows_ok(512) and ops._stats_rows_ok(64) and not ops._stats_rows_ok(96 * 4 + 4)


def test_carried_operand_bound_is_dropped_after_an_in_place_update():
    """a gradient tensor carries max |g| (written by its producer) to the kernel that pre-splits A g A^T with it.
    The autograd engine sums fan-in gradients IN PLACE into one addend: the sum keeps that addend's Python attributes but may
    be up to 2x larger.  The bound is stored with the tensor version it was measured at and ignored once the version moved."""
    import torch
    from deepsee_amd import ops
    g = torch.ones(4)
    slot = torch.zeros(2048)
    ops.tag_amax(g, slot)
    assert ops.carried_amax(g) is slot
    assert ops.carried_amax(g.contiguous()) is slot          # (the same object)
    g.add_(torch.ones(4))                                    # what InputBuffer::add does to the first gradient
    assert ops.carried_amax(g) is None
    assert not ops._presplit_ok(g, 32768, 32768, 512)
    w = torch.ones(4)
    w.dsee_amax = slot                                       # weights: tagged without a version, always trusted
    assert ops.carried_amax(w) is slot
    # a fan-in in a real graph: y = f(x) + h(x) where both branches return tagged gradients
    class Tagged(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2
        @staticmethod
        def backward(ctx, dy):
            dx = dy * 2
            ops.tag_amax(dx, slot)
            return dx
    seen = []
    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()
        @staticmethod
        def backward(ctx, dy):
            seen.append(ops.carried_amax(dy))
            return dy
    x = torch.ones(4, requires_grad=True)
    p = Probe.apply(x)
    (Tagged.apply(p) + Tagged.apply(p)).sum().backward()
    assert seen == [None]                                    # the engine's sum of two tagged gradients carries no bound
    seen.clear()
    x = torch.ones(4, requires_grad=True)
    Tagged.apply(Probe.apply(x)).sum().backward()
    assert seen == [slot] or seen[0] is slot                 # single consumer: the bound arrives


def test_kernel_plan_is_per_model_and_per_thread():
    """deepsee_amd/plan.py: a plan is an immutable value; activating one is thread-local and nests; an autograd node's
    backward runs under the plan its forward recorded even when another plan is active on the calling thread."""
    import threading
    import torch
    from deepsee_amd import ops, plan as PL
    from deepsee_amd.options import make_opt
    assert PL.current() is PL.DEFAULT_PLAN and not PL.DEFAULT_PLAN.half
    a = PL.from_opt(make_opt(precision="fp16"))
    b = PL.from_opt(make_opt(kernel_plan=dict(gemm_f16x2=False)))
    assert a.half and a.gemm_f16x2 and not b.half and not b.gemm_f16x2
    with pytest.raises(Exception):
        a.half = False                                 # frozen
    with pytest.raises(ValueError):
        PL.from_opt(make_opt(precision="bf16"))
    with pytest.raises(TypeError):
        PL.from_opt(make_opt(kernel_plan=dict(no_such_switch=1)))
    with a.active():
        assert ops.P() is a and ops._split_kind(512, 512) == 3
        with b.active():
            assert ops.P() is b and ops._split_kind(512, 512) == 1
        assert ops.P() is a
        seen = []
        t = threading.Thread(target=lambda: seen.append(PL.current()))
        t.start(); t.join()
        assert seen == [PL.DEFAULT_PLAN]               # another thread is not affected
    assert ops.P() is PL.DEFAULT_PLAN and ops._split_kind(512, 512) == 2

    class Node(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.plan = ops.P()
            return x * 2

        @staticmethod
        @ops._under_plan
        def backward(ctx, dy):
            seen.append(ops.P())
            return dy * 2
    seen.clear()
    x = torch.ones(2, requires_grad=True)
    with a.active():
        y = Node.apply(x)
    with b.active():
        y.sum().backward()
    assert seen == [a]


def test_wgrad_code_table_matches_the_tuple_encoding_it_replaced():
    """ops._wgrad_code on (V form, dM form, mode) gives the `split` argument of dsee_wino43_wgrad[_table] that the tuple
    encoding gave -- (t, amax) fp32 or transposed bf16x3, (t, amax, True) fp16x2, (t, amax, "pk") packed -- for every pairing
    that encoding could produce, under the plans that change _wgrad_split; any other pairing raises."""
    from deepsee_amd import ops, plan as PL
    from deepsee_amd.options import make_opt

    def old_code(v, dm, mode):         # the function as it stood on tuples
        pk = lambda o: len(o) == 3 and o[2] == "pk"
        if pk(v):
            assert pk(dm)
            return 7
        if len(v) == 3:
            return 6 if len(dm) == 3 else 5
        return ops._wgrad_split(mode)

    t = torch.zeros(1)
    old = {ops.FP32: (t, t), ops.F16X2: (t, t, True), ops.F16P: (t, t, "pk"), ops.BF16X3_T: (t, None)}
    legal = [(ops.FP32, ops.FP32, 0), (ops.FP32, ops.FP32, 2), (ops.BF16X3_T, ops.BF16X3_T, 1),
             (ops.F16X2, ops.FP32, 2), (ops.F16X2, ops.F16X2, 2), (ops.F16P, ops.F16P, 2)]
    forms = list(old)
    plans = [PL.DEFAULT_PLAN, PL.from_opt(make_opt(kernel_plan=dict(gemm_f16x2=False))), PL.from_opt(make_opt(precision="fp16"))]
    seen = set()
    for plan in plans:
        with plan.active():
            for vf, df, mode in legal:
                got = ops._wgrad_code(ops.WinoOperand(t, None, vf), ops.WinoOperand(t, None, df), mode)
                assert got == old_code(old[vf], old[df], mode), (vf, df, mode)
                seen.add(got)
            for vf in forms:
                for df in forms:
                    for mode in (0, 1, 2):
                        if (vf, df) in {(a, b) for a, b, _ in legal} and (vf == ops.BF16X3_T) == (mode == 1):
                            continue
                        with pytest.raises(ValueError):
                            ops._wgrad_code(ops.WinoOperand(t, None, vf), ops.WinoOperand(t, None, df), mode)
    assert seen == set(range(8))           # every code of the entry point was exercised
    # the pairing the old function only asserted: a packed V with a non-packed dM
    for df in (ops.FP32, ops.F16X2, ops.BF16X3_T):
        with pytest.raises(ValueError):
            ops._wgrad_code(ops.WinoOperand(t, t, ops.F16P), ops.WinoOperand(t, t, df), 2)


def test_operand_survives_an_autograd_context():
    """ops.save_with_operand / saved_with_operand: an operand of each form (and none) comes back from a context with the same
    form and the same tensors, next to the other saved tensors."""
    from deepsee_amd import ops

    class Ctx:
        def save_for_backward(self, *tensors):
            self.saved_tensors = tensors

    a, b, d, m = torch.zeros(2), None, torch.ones(3), torch.ones(1)
    for form in (ops.FP32, ops.F16X2, ops.F16P, ops.BF16X3_T):
        ctx = Ctx()
        op = ops.WinoOperand(d, None if form == ops.BF16X3_T else m, form)
        ops.save_with_operand(ctx, op, a, b)
        assert all(t is None or isinstance(t, torch.Tensor) for t in ctx.saved_tensors)    # only tensors go through autograd
        (ra, rb), back = ops.saved_with_operand(ctx)
        assert ra is a and rb is None and back.form == form and back.data is d and back.amax is op.amax
    ctx = Ctx()
    ops.save_with_operand(ctx, None, a)
    assert ops.saved_with_operand(ctx) == ([a], None)


# (n, hi, wi, cin_s, cout_s, co, ci, kh, kw, stride, pad, ups, has_res, exact): every distinct convolution of one G + D step of
# the 32 -> 256, ngf = 16 model at batch 2 (generator, encoder with its ups = 1 layer, both discriminator scales at batch 2 and
# 4, the VGG taps), under the default plan and under thin_gemm=False (to-RGB and D's last layer in their 1 x 1 and k x k forms)
F, T = False, True
STEP_CONVS = [
    (2, 16, 16, 512, 512, 512, 512, 3, 3, 1, 1, 0, F, F), (2, 17, 17, 128, 256, 256, 128, 4, 4, 1, 2, 0, F, F),
    (2, 18, 18, 256, 4, 1, 256, 4, 4, 1, 2, 0, F, F), (2, 18, 18, 256, 16, 16, 256, 1, 1, 1, 0, 0, F, T),
    (2, 32, 32, 4, 32, 32, 3, 3, 3, 1, 1, 0, F, F), (2, 32, 32, 4, 256, 256, 3, 3, 3, 1, 1, 0, F, F),
    (2, 32, 32, 32, 64, 64, 32, 3, 3, 1, 1, 0, F, F), (2, 32, 32, 64, 128, 128, 64, 3, 3, 1, 1, 0, F, F),
    (2, 32, 32, 128, 256, 256, 128, 3, 3, 1, 1, 1, F, F), (2, 32, 32, 256, 256, 256, 256, 3, 3, 1, 1, 0, F, F),
    (2, 32, 32, 256, 256, 256, 256, 3, 3, 1, 1, 0, T, F), (2, 32, 32, 256, 512, 512, 256, 3, 3, 1, 1, 0, F, F),
    (2, 32, 32, 512, 512, 512, 512, 3, 3, 1, 1, 0, F, F), (2, 33, 33, 64, 128, 128, 64, 4, 4, 2, 2, 0, F, F),
    (2, 33, 33, 128, 256, 256, 128, 4, 4, 1, 2, 0, F, F), (2, 34, 34, 256, 4, 1, 256, 4, 4, 1, 2, 0, F, F),
    (2, 34, 34, 256, 16, 16, 256, 1, 1, 1, 0, 0, F, T), (2, 64, 64, 128, 256, 256, 128, 3, 3, 1, 1, 0, F, F),
    (2, 64, 64, 128, 256, 256, 128, 3, 3, 1, 1, 1, F, F), (2, 64, 64, 256, 128, 128, 256, 3, 3, 1, 1, 0, F, F),
    (2, 64, 64, 256, 256, 256, 256, 3, 3, 1, 1, 0, F, F), (2, 64, 64, 256, 256, 256, 256, 3, 3, 1, 1, 0, T, F),
    (2, 65, 65, 32, 64, 64, 32, 4, 4, 2, 2, 0, F, F), (2, 65, 65, 64, 128, 128, 64, 4, 4, 2, 2, 0, F, F),
    (2, 128, 128, 24, 32, 32, 22, 4, 4, 2, 2, 0, F, F), (2, 128, 128, 64, 128, 128, 64, 3, 3, 1, 1, 0, F, F),
    (2, 128, 128, 64, 128, 128, 64, 3, 3, 2, 1, 0, F, F), (2, 128, 128, 128, 128, 128, 128, 3, 3, 1, 1, 0, F, F),
    (2, 128, 128, 256, 128, 128, 256, 3, 3, 1, 1, 0, F, F), (2, 128, 128, 256, 256, 256, 256, 3, 3, 1, 1, 0, F, F),
    (2, 128, 128, 256, 256, 256, 256, 3, 3, 1, 1, 0, T, F), (2, 129, 129, 32, 64, 64, 32, 4, 4, 2, 2, 0, F, F),
    (2, 256, 256, 4, 32, 32, 3, 3, 3, 1, 1, 0, F, F), (2, 256, 256, 4, 64, 64, 3, 3, 3, 1, 1, 0, F, F),
    (2, 256, 256, 24, 32, 32, 22, 4, 4, 2, 2, 0, F, F), (2, 256, 256, 32, 64, 64, 32, 3, 3, 2, 1, 0, F, F),
    (2, 256, 256, 64, 64, 64, 64, 3, 3, 1, 1, 0, F, F), (2, 256, 256, 256, 4, 3, 256, 3, 3, 1, 1, 0, F, F),
    (2, 256, 256, 256, 28, 27, 256, 1, 1, 1, 0, 0, F, T), (2, 256, 256, 256, 256, 256, 256, 3, 3, 1, 1, 0, F, F),
    (2, 256, 256, 256, 256, 256, 256, 3, 3, 1, 1, 0, T, F), (4, 17, 17, 128, 256, 256, 128, 4, 4, 1, 2, 0, F, F),
    (4, 18, 18, 256, 4, 1, 256, 4, 4, 1, 2, 0, F, F), (4, 18, 18, 256, 16, 16, 256, 1, 1, 1, 0, 0, F, T),
    (4, 33, 33, 64, 128, 128, 64, 4, 4, 2, 2, 0, F, F), (4, 33, 33, 128, 256, 256, 128, 4, 4, 1, 2, 0, F, F),
    (4, 34, 34, 256, 4, 1, 256, 4, 4, 1, 2, 0, F, F), (4, 34, 34, 256, 16, 16, 256, 1, 1, 1, 0, 0, F, T),
    (4, 65, 65, 32, 64, 64, 32, 4, 4, 2, 2, 0, F, F), (4, 65, 65, 64, 128, 128, 64, 4, 4, 2, 2, 0, F, F),
    (4, 128, 128, 24, 32, 32, 22, 4, 4, 2, 2, 0, F, F), (4, 129, 129, 32, 64, 64, 32, 4, 4, 2, 2, 0, F, F),
    (4, 256, 256, 24, 32, 32, 22, 4, 4, 2, 2, 0, F, F),
]
# ... and what that step does not hold: the bs = 8 flagship's 512 -> 512 layer (weight-gradient mode 2, channel sums in the
# A dY A^T pass) and its to-RGB layer in both forms, a 3 x 3 layer whose height is no multiple of 4, one with a residual that
# Winograd does not take, an odd-sized 4 x 4 / stride 2 layer under an upsampling, a 1 x 1 layer too narrow for the thin kernel
EXTRA_CONVS = [
    (8, 64, 64, 512, 512, 512, 512, 3, 3, 1, 1, 0, F, F), (8, 64, 64, 512, 512, 512, 512, 3, 3, 1, 1, 0, T, F),
    (8, 256, 256, 512, 28, 27, 512, 1, 1, 1, 0, 0, F, T), (8, 256, 256, 512, 4, 3, 512, 3, 3, 1, 1, 0, F, F),
    (2, 30, 32, 256, 256, 256, 256, 3, 3, 1, 1, 0, F, F), (2, 32, 32, 64, 64, 64, 64, 3, 3, 1, 1, 0, T, F),
    (2, 33, 35, 64, 128, 128, 64, 4, 4, 2, 2, 1, F, F), (2, 32, 32, 64, 16, 16, 64, 1, 1, 1, 0, 0, F, F),
    (2, 32, 32, 128, 16, 16, 126, 1, 1, 1, 0, 0, F, T), (2, 32, 32, 128, 16, 16, 128, 1, 1, 1, 0, 0, T, F),
]


def test_conv_path_matches_the_predicates_it_replaced():
    """ops._conv_path names, once per layer, the kernel families that Conv2d.forward (ctx.wino, ctx.thin, the kept V) and
    Conv2d.backward (thin1, fused, the dx and the dw ladder, the three copies of the activation backward, the `sums` condition)
    derived in five places: the same answer on every convolution of the 32 -> 256 step and on the shapes that step lacks, under
    the default plan and with each switch that those predicates read flipped, for all four (x, w) gradient needs."""
    from deepsee_amd import lib as L, ops, plan as PL

    def old(n, hi, wi, cin_s, cout_s, co, ci, kh, kw, stride, pad, ups, has_res, exact, need_dx, need_dw):
        P = ops.P
        geom = L.geom_fwd(n, hi, wi, cin_s, cout_s, kh, stride, pad, ups)
        # forward
        wino = ops._wino_ok(n, hi, wi, cin_s, cout_s, kh, stride, pad, ups)
        thin = (not P().thin_gemm and kh == 3 and stride == 1 and pad == 1 and ups == 0 and co <= 4 and cin_s % 256 == 0
                and cin_s <= 1024 and wi % 64 == 0 and not has_res)
        fwd = "thin3" if thin else "wino" if wino else "direct"
        keep_v = bool(not thin and wino and P().keep_v and need_dw and ops._wgrad_mode(cin_s, cout_s) == 2)
        # backward: the activation's branch that attached a maximum
        g_amax = bool((wino and P().presplit_dm) or (not wino and ops._direct_split_on(exact) and P().conv_amax_out))
        fused = (wino and P().winograd_wgrad and need_dx and need_dw
                 and ops._wgrad_mode(geom.Cin, geom.Cout) != 1 and ops._adjoint_ok(geom.Cout, geom.Cin))
        dout_sums = False
        if wino and P().winograd_wgrad and need_dw:
            nb_w = ops._wino_chunk(geom.N, geom.Hi, geom.Wi, max(geom.Cin, geom.Cout))
            dout_sums = bool(ops._dout_sums_ok(geom.N, nb_w, geom.Cout, ops._wgrad_mode(geom.Cin, geom.Cout)))
        thin1 = (P().thin_gemm and kh == 1 and kw == 1 and geom.ups == 0 and co <= 32 and ci == geom.Cin and not has_res
                 and geom.Ho == geom.Hi and geom.Wo == geom.Wi and geom.Cin >= 128)
        dx = dw = None
        if thin1:
            dx, dw = ("thin1" if need_dx else None), ("thin1" if need_dw else None)
        elif fused:
            dw, dx = "wino", "adjoint"
        elif need_dx and wino:
            dx = "wino"
        elif need_dx and not thin1 and ops._s2_parity_ok(geom, kh, kw):
            dx = "s2_parity"
        elif need_dx and not thin1:
            dx = "direct_sumpool" if geom.ups else "direct"
        if dw is not None or thin1:
            pass
        elif need_dw and thin:
            dw = "thin3"
        elif need_dw and wino and P().winograd_wgrad:
            dw = "wino"
        elif need_dw:
            dw = "direct"
        return (fwd, dx, dw, keep_v, g_amax, dout_sums)

    assert (ops.THIN3, ops.WINO, ops.DIRECT, ops.THIN1, ops.ADJOINT, ops.S2_PARITY, ops.DIRECT_SUMPOOL) == \
        ("thin3", "wino", "direct", "thin1", "adjoint", "s2_parity", "direct_sumpool")
    flips = ["winograd", "winograd_wgrad", "thin_gemm", "gemm_split", "gemm_af32", "adjoint_dgrad", "dgrad_s2_parity", "half",
             "keep_v", "presplit_dm", "conv_amax_out", "dout_sums", "gemm_f16x2"]
    plans = [PL.DEFAULT_PLAN] + [PL.DEFAULT_PLAN.replace(**{f: not getattr(PL.DEFAULT_PLAN, f)}) for f in flips]
    plans.append(PL.DEFAULT_PLAN.replace(conv_f16x2_min_flop=0.0))
    seen = {"fwd": set(), "dgrad": set(), "wgrad": set(), "flags": set()}
    for plan in plans:
        with plan.active():
            for shape in STEP_CONVS + EXTRA_CONVS:
                for need_dx in (False, True):
                    for need_dw in (False, True):
                        got = ops._conv_path(*shape, need_dx, need_dw)
                        assert isinstance(got, ops.ConvPath) and tuple(got) == old(*shape, need_dx, need_dw), \
                            (plan, shape, need_dx, need_dw, got)
                        seen["fwd"].add(got.fwd), seen["dgrad"].add(got.dgrad), seen["wgrad"].add(got.wgrad)
                        seen["flags"].add((got.keep_v, got.g_amax, got.dout_sums))
    assert ops.P() is PL.DEFAULT_PLAN
    # the grid reaches every family the record can name, and both values of every flag
    assert seen["fwd"] == {"thin3", "wino", "direct"}
    assert seen["dgrad"] == {None, "thin1", "adjoint", "wino", "s2_parity", "direct", "direct_sumpool"}
    assert seen["wgrad"] == {None, "thin1", "thin3", "wino", "direct"}
    assert all({f[i] for f in seen["flags"]} == {False, True} for i in range(3))
    with pytest.raises(AttributeError):
        got.fwd = "wino"                                  # frozen


def test_conv2d_hands_every_setting_to_the_node_in_one_spec(monkeypatch):
    """ops.conv2d -> Conv2d.apply(x, w, bias, res, noise_w, res_noise_w, ConvSpec): every non-tensor setting conv2d can set arrives
    in the spec, on each of its four routes (reflect, the thin 27-output split, fused noise, the UpNoise fallbacks); the named
    positions into needs_input_grad are the node's inputs, one gradient each.  No device: the nodes are replaced by recorders."""
    import inspect
    from deepsee_amd import lib as L, ops
    calls = []
    monkeypatch.setattr(ops.Conv2d, "apply", lambda *a: calls.append(("conv",) + a) or "y")
    monkeypatch.setattr(ops.UpNoise, "apply", lambda *a: calls.append(("upnoise",) + a) or "up")
    monkeypatch.setattr(ops.ThinGather, "apply", lambda *a: calls.append(("gather",) + a) or "rgb")

    inputs = list(inspect.signature(ops.Conv2d.forward).parameters)[1:]
    named = [k for k in vars(ops) if k.startswith("IN_")]
    assert inputs == ["x", "w", "bias", "res", "noise_w", "res_noise_w", "spec"]
    assert [k[3:].lower() for k in sorted(named, key=lambda k: getattr(ops, k))] == inputs
    assert sorted(getattr(ops, k) for k in named) == list(range(len(inputs)))
    assert ops.ConvSpec._fields == ("stride", "pad", "ups", "act", "noise_eps", "res_noise_eps", "res_sink", "exact", "stats",
                                    "in_act", "defer_act_bwd", "reflect")
    assert ops.ConvSpec() == (1, 1, 0, L.ACT_NONE, None, None, None, False, False, 0, False, False)
    with pytest.raises(AttributeError):
        ops.ConvSpec().stride = 2                         # frozen

    x = torch.zeros(2, 32, 32, 256, requires_grad=True)
    w, b, res = torch.zeros(256, 256, 3, 3), torch.zeros(256), torch.zeros(2, 32, 32, 256)
    nw, rnw, sink = torch.zeros(256), torch.ones(256), ops.GradSink()
    eps, reps = ops.PhiloxNormal((2, 32, 32, 256), 5, 64), ops.PhiloxNormal((2, 32, 32, 256), 6, 128)

    # every keyword at once, on the route that fuses both noises: one node, no UpNoise
    assert ops.conv2d(x, w, b, res, stride=1, pad=1, ups=0, act=L.ACT_NONE, noise=(nw, eps), res_noise=(rnw, reps), res_sink=sink,
                      stats=1, in_act=L.ACT_LRELU) == "y"
    (kind, *args), = calls
    assert kind == "conv" and len(args) == len(inputs)
    assert all(a is e for a, e in zip(args[:6], (x, w, b, res, nw, rnw)))
    assert args[6] == ops.ConvSpec(1, 1, 0, L.ACT_NONE, eps, reps, sink, False, True, L.ACT_LRELU, False, False)
    assert args[6].noise_eps is eps and args[6].res_noise_eps is reps and args[6].res_sink is sink and args[6].stats is True
    calls.clear()
    ops.conv2d(x, w, b, None, stride=2, pad=0, ups=1, act=L.ACT_LRELU, defer_act_bwd=True)
    assert calls == [("conv", x, w, b, None, None, None, ops.ConvSpec(2, 0, 1, L.ACT_LRELU, defer_act_bwd=True))]
    calls.clear()
    # `in_act` is reset where nothing will differentiate x
    ops.conv2d(x.detach(), w, in_act=L.ACT_LRELU)
    with torch.no_grad():
        ops.conv2d(x, w, in_act=L.ACT_LRELU)
    assert [c[-1].in_act for c in calls] == [0, 0]
    calls.clear()
    # reflect: a plain layer, nothing else set
    ops.conv2d(x, w, b, reflect=True, in_act=L.ACT_LRELU)
    assert calls == [("conv", x, w, b, None, None, None, ops.ConvSpec(1, 1, 0, L.ACT_NONE, reflect=True))]
    for bad in (dict(res=res), dict(act=L.ACT_LRELU), dict(noise=(nw, eps)), dict(res_noise=(rnw, reps))):
        with pytest.raises(AssertionError):
            ops.conv2d(x, w, b, reflect=True, **bad)
    calls.clear()
    # the thin split: 27 outputs of a 1 x 1 layer kept exact, then the gather with the bias and the activation
    w3 = torch.zeros(3, 256, 3, 3)
    assert ops.conv2d(x, w3, b[:3], act=L.ACT_TANH, in_act=L.ACT_LRELU) == "rgb"
    (_, cx, w27, *rest), gather = calls
    assert cx is x and tuple(w27.shape) == (27, 256, 1, 1) and rest[:4] == [None] * 4
    assert rest[4] == ops.ConvSpec(1, 0, 0, L.ACT_NONE, exact=True, in_act=L.ACT_LRELU)
    assert gather[0] == "gather" and gather[1] == "y" and gather[3:] == (3, L.ACT_TANH, 3, 3, 1)
    calls.clear()
    # a noise that cannot ride in the output transform runs as UpNoise: a replayed tensor behind the layer, a residual noise
    # on a layer Winograd does not take (its shortcut then keeps its own node: no sink)
    teps = torch.zeros(2, 32, 32, 256)
    assert ops.conv2d(x, w, b, res, noise=(nw, teps), res_noise=(rnw, reps), res_sink=sink, stats=True, in_act=L.ACT_LRELU) == "up"
    assert calls == [("conv", x, w, b, res, None, rnw, ops.ConvSpec(res_noise_eps=reps, res_sink=sink, in_act=L.ACT_LRELU)),
                     ("upnoise", "y", nw, teps, 0)]
    with pytest.raises(AssertionError):
        ops.conv2d(x, w, b, noise=(nw, teps), act=L.ACT_LRELU, defer_act_bwd=True)
    calls.clear()
    ops.conv2d(x, w, b, res, stride=2, res_noise=(rnw, reps), res_sink=sink)
    assert calls == [("upnoise", res, rnw, reps, 0), ("conv", x, w, b, "up", None, None, ops.ConvSpec(stride=2))]


def _old_split_kind(ops, k_s, r_s):
    """ops._split_kind as it stood on integers: 0 fp32, 1 bf16x3, 2 fp16x2 with an fp32 A operand, 3 one fp16 term"""
    P = ops.P
    if not (P().gemm_split and k_s % 32 == 0 and r_s % 128 == 0):
        return 0
    af32 = P().gemm_af32 and k_s * 4 * 256 < 0x7FFFFFFF
    if P().half and af32:
        return 3
    return 2 if (P().gemm_f16x2 and af32) else 1


def test_wino_kinds_and_backward_decisions_match_the_expressions_they_replaced():
    """ops._u_kind and ops._wino_bwd against the inline expressions they replaced, restated here as they stood: the 3 -> 4
    promotion of _wino_conv; pk, pre_dm and the adjoint-U kind of _wino_wgrad; the `4 if dm.form == F16P else _split_kind(..)` of
    _wino_dgrad_from_dm and _norm_wino_wgrad; `4 if half else 2` of the fused norm and the spectral-norm group; _norm_keeps_v;
    fused_d, as_dm and pre_ok of SeanNormTable.backward.  Grid: every Winograd layer of STEP_CONVS + EXTRA_CONVS and the norm
    shapes (ld 32, 128 and 160; c = 256, 512 and two that are no power of two) x the default plan and each switch those expressions
    read flipped x both values of "x / g carries a maximum" x every kept-V form and none."""
    from deepsee_amd import ops, plan as PL
    from deepsee_amd.lib import GemmKind, WgradMode
    P, NH = ops.P, ops.NHIDDEN
    assert [int(k) for k in GemmKind] == [0, 1, 2, 3, 4] and [int(m) for m in WgradMode] == [0, 1, 2]
    assert ops.GemmKind is GemmKind and ops.WgradMode is WgradMode and ops._split_kind is ops._u_kind

    def old_adjoint_ok(k_s, r_s):
        return bool(P().adjoint_dgrad and P().gemm_af32 and (P().gemm_split and k_s % 32 == 0 and r_s % 128 == 0)
                    and k_s * 4 * 256 < 0x7FFFFFFF)

    def old_wino_wgrad(n, h, wd, cin_s, cout_s, want_dx, g_amax, v_form):
        nb = ops._wino_chunk(n, h, wd, max(cin_s, cout_s))
        t, mode = nb * (h // 4) * (wd // 4), ops._wgrad_mode(cin_s, cout_s)
        with_dx = bool(want_dx and mode != 1 and old_adjoint_ok(cout_s, cin_s))      # (_conv_path's `adjoint`: the caller's promise)
        pk = (v_form is not None and v_form == ops.F16P and P().presplit_dm and mode == 2 and nb == n and g_amax
              and t % 256 == 0 and cout_s % 32 == 0 and (not with_dx or cin_s % 128 == 0))
        u_t = (4 if pk else _old_split_kind(ops, cout_s, cin_s)) if with_dx else None
        pre_dm = pk or (P().presplit_dm and mode == 2 and nb == n and _old_split_kind(ops, cout_s, cin_s) == 2 and t % 256 == 0
                        and cout_s % 16 == 0 and (not with_dx or (cin_s % 256 == 0 and (36 * t // 256) * (cin_s // 256) >= 512)))
        # the form dM then left _wino_wgrad_operands in
        v = v_form if (mode == 2 and nb == n) else None
        pre = bool(pre_dm and g_amax)
        if v == ops.F16P and not pre:
            v = None
        dm_form = ops.BF16X3_T if mode == 1 else (v or ops.FP32) if pre else ops.FP32
        return nb, t, mode, bool(pk), bool(pre_dm), u_t, dm_form

    flips = ["gemm_split", "gemm_af32", "gemm_f16x2", "half", "half_norms", "presplit_a", "presplit_dm", "presplit_gb", "keep_v",
             "adjoint_dgrad", "fuse_dm", "winograd_wgrad"]
    plans = [PL.DEFAULT_PLAN] + [PL.DEFAULT_PLAN.replace(**{f: not getattr(PL.DEFAULT_PLAN, f)}) for f in flips]
    plans.append(PL.DEFAULT_PLAN.replace(half=True, presplit_dm=False))
    wino = sorted({s[:5] for s in STEP_CONVS + EXTRA_CONVS if ops._wino_ok(*s[:5], s[7], *s[9:12])})
    assert len(wino) >= 10 and (8, 64, 64, 512, 512) in wino
    # (n, h, w, c, has_a, has_t): SPADE (ld 128), SEAN (160) and PureSEAN (32) norms; rows = 2 c
    norms = [(n, r, r, c, a, t) for n, r in ((2, 32), (2, 64), (8, 64)) for c in (256, 512, 384, 192)
             for a, t in ((True, False), (True, True), (False, True))] + [(2, 30, 32, 256, True, True), (3, 64, 32, 256, True, False)]
    forms = (None, ops.FP32, ops.F16X2, ops.F16P)
    tagged, bare = torch.zeros(1), torch.zeros(1)
    tagged.dsee_amax = torch.zeros(1)
    seen = {"kind": set(), "mode": set(), "dm": set(), "flags": set(), "norm": set(), "u_t": set()}
    for plan in plans:
        with plan.active():
            for f16_only_caller in ("fused norm", "spectral-norm group"):
                assert ops._u_kind(160, 1024, f16_only=True) == (4 if P().half else 2)
            for n, h, wd, cin_s, cout_s in wino:
                if ops._wino_chunk(n, h, wd, max(cin_s, cout_s)) is None:
                    continue
                # forward, and the rotated-kernel data gradient (transpose_flip)
                for r_s, k_s in ((cout_s, cin_s), (cin_s, cout_s)):
                    assert ops._split_kind(k_s, r_s) == _old_split_kind(ops, k_s, r_s)
                    for x in (tagged, bare):
                        split, nb = _old_split_kind(ops, k_s, r_s), ops._wino_chunk(n, h, wd, max(r_s, k_s))
                        if split == 3 and nb == n and ops._pk_ok(x, n * (h // 4) * (wd // 4), r_s, k_s):
                            split = 4
                        got = ops._u_kind(k_s, r_s, x_pk=nb == n and ops._pk_ok(x, n * (h // 4) * (wd // 4), r_s, k_s))
                        assert isinstance(got, GemmKind) and got == split, (plan, n, h, wd, k_s, r_s)
                        seen["kind"].add(got)
                    for dm_form in (ops.FP32, ops.F16X2, ops.F16P, ops.BF16X3_T):
                        assert ops._u_kind(k_s, r_s, dm_form=dm_form) == (4 if dm_form == ops.F16P else _old_split_kind(ops, k_s, r_s))
                for want_dx in (False, True):
                    for g_amax in (False, True):
                        for v_form in forms:
                            nb, t, mode, pk, pre_dm, u_t, dm_form = old_wino_wgrad(n, h, wd, cin_s, cout_s, want_dx, g_amax, v_form)
                            got = ops._wino_bwd(n, nb, h, wd, cin_s, cout_s, cin_s if want_dx else 0, v_form, g_amax)
                            assert isinstance(got, ops.WinoBwd) and isinstance(got.mode, WgradMode)
                            assert got == (nb, mode, t, mode == 2 and nb == n, pk, pre_dm, u_t, False), (plan, n, h, wd, cin_s, cout_s)
                            assert got.u_t is None or isinstance(got.u_t, GemmKind)
                            seen["mode"].add(got.mode), seen["dm"].add(dm_form), seen["u_t"].add(got.u_t)
                            seen["flags"].add((got.whole, got.pk, got.pre_dm, got.u_t is not None))
            for n, h, wd, c, has_a, has_t in norms:
                rows, ld = 2 * c, (NH if has_a else 0) + (32 if has_t else 0)
                nb = ops._wino_mod_chunk(n, h, wd, c, rows, has_t)
                mode = ops._wgrad_mode(ld, rows)
                for scale in (None, tagged):
                    assert bool(ops._norm_keeps_v(scale, nb, n, ld, rows)) == \
                        bool(P().keep_v and scale is not None and nb == n and mode == 2)
                for need_w2a in (False, True):
                    for v_form in forms:
                        wino_w = bool(nb) and (has_t or need_w2a)
                        fused_d = wino_w and has_a and mode != 1 and old_adjoint_ok(rows, NH)
                        as_dm = (P().fuse_dm and wino_w and nb == n and mode != 1 and (fused_d or not has_a)
                                 and 256 % (c // 4) == 0)
                        pre_ok = v_form is not None and v_form in (ops.F16X2, ops.F16P) and mode == 2 and (not has_a or fused_d)
                        got = ops._wino_bwd(n, nb if wino_w else 0, h, wd, ld, rows, NH if has_a else 0, v_form, norm_c=c)
                        assert (got.mode, got.u_t is not None, got.as_dm, got.pre_dm, got.pk) == \
                            (mode, bool(fused_d), bool(as_dm), bool(pre_ok), False), (plan, n, h, wd, c, has_a, has_t, need_w2a, v_form)
                        assert not wino_w or (got.nb, got.t, got.whole) == (nb, nb * (h // 4) * (wd // 4), mode == 2 and nb == n)
                        for dm_form in (None, ops.FP32, ops.F16X2, ops.F16P):      # (what modulate_bwd / _wino_dout hand on)
                            want = 4 if dm_form == ops.F16P else _old_split_kind(ops, rows, NH)
                            assert ops._u_kind(rows, NH, dm_form=dm_form) == want
                            assert not fused_d or dm_form == ops.F16P or got.u_t == want
                            seen["kind"].add(ops._u_kind(rows, NH, dm_form=dm_form))
                        seen["mode"].add(got.mode), seen["u_t"].add(got.u_t)
                        seen["norm"].add((got.u_t is not None, got.as_dm, got.pre_dm))
    assert ops.P() is PL.DEFAULT_PLAN
    # the grid reaches every member of both enums, every dM form and both values of every flag
    assert seen["kind"] == set(GemmKind) and seen["mode"] == set(WgradMode)
    assert seen["u_t"] == {None} | set(GemmKind) - {GemmKind.FP32}         # (an adjoint GEMM always runs on split operands)
    assert seen["dm"] == {ops.FP32, ops.F16X2, ops.F16P, ops.BF16X3_T}
    assert all({f[i] for f in seen["flags"]} == {False, True} for i in range(4))
    assert all({f[i] for f in seen["norm"]} == {False, True} for i in range(3))
    with pytest.raises(AttributeError):
        got.pk = True                                     # frozen


def test_gemm_kind_tables_equal_the_literals_they_replaced():
    """What a GemmKind carries -- int16 words per weight element, whether a weight maximum is needed, whether the product is scaled
    fp16, the timer name, the byte model -- against the dictionary literals, the `>= 2` and `in (3, 4)` tests and the two ladders
    (_gemm_name, _gemm_bytes) as they stood, for all five kinds; the callers that pass plain integers still can."""
    from deepsee_amd import ops
    from deepsee_amd.lib import GemmKind, WgradMode

    def old_gemm_bytes(t, k_s, r_s, groups, rows, split):
        if split == 4:
            return 2.0 * 36 * t * k_s + 2.0 * groups * rows * k_s + 2.0 * 36 * t * r_s
        if split == 3:
            return 4.0 * 36 * t * k_s + 2.0 * groups * rows * k_s + 2.0 * 36 * t * r_s
        return 4.0 * 36 * t * k_s + (4.0 if split == 2 else 6.0) * groups * rows * k_s + 4.0 * 36 * t * r_s

    words = {1: 3, 2: 2, 3: 1, 4: 1}
    names = {0: "winograd_gemm_128x128(igemm,36 groups)", 1: "winograd_gemm_bf16x3", 2: "winograd_gemm_f16x2",
             3: "winograd_gemm_f16_1term", 4: "winograd_gemm_f16_1term_packed"}
    for split in range(5):
        kind = GemmKind(split)
        assert kind == split and hash(kind) == hash(split) and "%d" % kind == str(split)
        assert kind.words == words.get(split, 2)                 # (fp32 weights: 4 bytes; the literal had no entry, U is fp32 there)
        assert kind.needs_amax is (split >= 2) and kind.f16_product is (split in (3, 4)) and kind.timer == names[split]
        for t, k_s, r_s, groups, rows in ((512, 256, 256, 36, 256), (2048, 160, 1024, 36 * 8, 1024), (8192, 512, 512, 36, 512)):
            assert kind.gemm_bytes(t, k_s, r_s, groups, rows) == old_gemm_bytes(t, k_s, r_s, groups, rows, split)
        assert kind.bytes[2] == (2.0 if split in (3, 4) else 4.0)     # (the product's bytes, as _norm_product_wino modelled them)
    # the functions tests and tools call with plain integers
    assert ops._u_key(False, 2, 128, 160) == ops._u_key(0, GemmKind.F16X2_AF32, 128, 160) == (0, 2, 128, 160)
    assert ops._dout_sums_ok(8, 8, 512, 2) and ops._dout_sums_ok(8, 8, 512, WgradMode.AF32) and not ops._dout_sums_ok(8, 8, 512, 1)
    t = torch.zeros(1)
    assert ops._wgrad_code(ops.WinoOperand(t, None, ops.FP32), ops.WinoOperand(t, None, ops.FP32), 0) == 0
    assert type(ops._wgrad_code(ops.WinoOperand(t, None, ops.BF16X3_T), ops.WinoOperand(t, None, ops.BF16X3_T), 1)) is int
    with pytest.raises(ValueError):
        ops._wgrad_code(ops.WinoOperand(t, None, ops.FP32), ops.WinoOperand(t, None, ops.FP32), 3)       # no such mode
    assert [ops._wgrad_name(m) for m in (0, 1)] == ["winograd_wgrad_128x128(36 groups)", "winograd_wgrad_bf16x3"]


def test_u_cache_key_written_by_the_group_is_the_key_the_layer_looks_up(monkeypatch):
    """SNGroup.wino_weights stores every layer's U under ops._u_key(..); ops._wino_u, asked for the kind the layer's forward
    (flip 0) and its adjoint data gradient (flip 2) run with, finds it there and launches nothing -- in both precisions.  No
    device: the launch and the allocation are replaced by recorders."""
    from types import SimpleNamespace
    from deepsee_amd import lib as L, ops, plan as PL
    from deepsee_amd.options import make_opt
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda name, *a: calls.append((name,) + a))
    monkeypatch.setattr(ops, "_i16", lambda n: torch.empty(n, dtype=torch.int16))
    co = ci = 256       # (weight-gradient mode AF32: the data gradient takes the adjoint form)
    for plan, packed in ((PL.DEFAULT_PLAN, False), (PL.from_opt(make_opt(precision="fp16")), True)):
        with plan.active():
            layer = SimpleNamespace(weight_orig=torch.zeros(co, ci, 3, 3), _pre=torch.zeros(co, ci, 3, 3))
            grp = ops.SNGroup([layer])
            grp.slices, grp.last = [(0, co * ci * 9, 0, co, ci * 9)], (torch.zeros(co * ci * 9), torch.zeros(1, ops.AMAX_FLOATS))
            calls.clear()
            grp.wino_weights(with_adjoint=True)
            assert [c[0] for c in calls] == ["wino43_weights_batch"] * 2
            assert [c[9] for c in calls] == [4 if packed else 2] * 2 and all(type(c[9]) is int for c in calls)
            rows, kp = L.wrows(co), L.kpad(1, 1, ci)
            kind = ops.GemmKind.F16_PACKED if packed else ops.GemmKind.F16X2_AF32
            assert set(layer._pre.dsee_u) == {ops._u_key(0, kind, rows, kp), ops._u_key(2, kind, rows, kp)}
            calls.clear()
            # the reader's side: the kinds _wino_conv and _wino_wgrad arrive at for this layer
            fwd = ops._u_kind(ci, co, x_pk=packed)
            adj = ops._wino_bwd(2, 2, 64, 64, ci, co, ci, ops.F16P if packed else ops.F16X2, g_amax=True).u_t
            assert (fwd, adj) == (kind, kind)
            for flip, k in ((0, fwd), (2, adj), (False, int(fwd))):
                u, amax = ops._wino_u(layer._pre, co, ci, flip, rows, kp, k)
                assert u is layer._pre.dsee_u[(int(flip), int(kind), rows, kp)][0] and amax.numel() == ops.AMAX_FLOATS
            assert calls == []
