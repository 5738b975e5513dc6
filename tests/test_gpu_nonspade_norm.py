"""Discriminator / style-encoder norms (opt.norm_D, opt.norm_E = spectral{batch,sync_batch,none}) on the MI355X: the affine
BatchNorm + act layer against float64 F.batch_norm up to the benchmark's largest D / E shapes, the G+D step and inference
modes against the substituted oracle (tools/gen_golden_nonspade_norm.py; pinned to the reference by
tests/test_nonspade_norm_host.py), the concatenated G-step discriminator pass, replayed graphs, the 16-bit mode, checkpoints
and SyncBN over a 1-rank RCCL group."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import deepsee_oracle as O
from tools.gen_golden_nonspade_norm import CASES as GOLD_CASES, install_nonspade_norm

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nonspade_norm")
SMALL = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-20))


def _bn_layer_run(x, gy, gamma, beta, rm, rv, cnt, act, training=True):
    """One BatchNormAct forward (+ backward in training) on NHWC device tensors; returns y, dx, dgamma, dbeta."""
    from deepsee_amd import ops
    xs = x.clone().requires_grad_(training)
    g = gamma.clone().requires_grad_(training)
    b = beta.clone().requires_grad_(training)
    with torch.set_grad_enabled(training):
        y = ops.BatchNormAct.apply(xs, g, b, rm, rv, cnt, training, act)
        if training:
            y.backward(gy)
    torch.cuda.synchronize()
    if not training:
        return y.detach(), None, None, None
    return y.detach(), xs.grad, g.grad, b.grad


# (N, H, W, C, act): D model1 of the benchmark's G step (2N = 16 images, 65^2 x 64) and encoder `initial` (8 x 256^2 x 32)
LAYER_CASES = [(2, 9, 9, 64, "lrelu"), (3, 16, 16, 128, "tanh"), (2, 5, 7, 256, "lrelu"), (16, 65, 65, 64, "lrelu"),
               (8, 256, 256, 32, "lrelu"), (8, 32, 32, 128, "tanh")]


@pytest.mark.parametrize("N,H,W,C,act", LAYER_CASES)
def test_bn_act_layer_vs_float64(N, H, W, C, act):
    """Forward, dx, dgamma, dbeta, running statistics and num_batches_tracked of the new kernels against float64
    F.batch_norm + act (its LeakyReLU branches taken from the HIP output); eval mode against the running statistics; a second
    identical run is bitwise equal."""
    from deepsee_amd import lib as L
    g = torch.Generator().manual_seed(N * 1000 + C + H)
    k = torch.arange(C, dtype=torch.float32)
    x = (torch.randn(N, H, W, C, generator=g) * (0.5 + k / C) + k / C).cuda()       # per-channel scale and offset
    gy = torch.randn(N, H, W, C, generator=g).cuda()
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).cuda()
    beta = (0.1 * torch.randn(C, generator=g)).cuda()
    rm0, rv0 = (0.1 * torch.randn(C, generator=g)).cuda(), (0.75 + 0.5 * torch.rand(C, generator=g)).cuda()
    a = L.ACT_LRELU if act == "lrelu" else L.ACT_TANH
    runs = []
    for _ in range(2):
        rm, rv = rm0.clone(), rv0.clone()
        cnt = torch.zeros((), dtype=torch.long, device="cuda")
        runs.append(_bn_layer_run(x, gy, gamma, beta, rm, rv, cnt, a) + (rm, rv, cnt))
    for t1, t2 in zip(runs[0], runs[1]):
        assert torch.equal(t1, t2)
    y, dx, dgam, dbet, rm, rv, cnt = runs[0]
    assert int(cnt) == 1
    # float64 yardstick (NCHW, on the device)
    x6 = x.double().permute(0, 3, 1, 2).requires_grad_()
    g6, b6 = gamma.double().requires_grad_(), beta.double().requires_grad_()
    rm6, rv6 = rm0.double().clone(), rv0.double().clone()
    pre = F.batch_norm(x6, rm6, rv6, g6, b6, True, 0.1, 1e-5)
    y_hip = y.permute(0, 3, 1, 2)
    ref = torch.where(y_hip > 0, pre, 0.2 * pre) if act == "lrelu" else torch.tanh(pre)
    ref.backward(gy.double().permute(0, 3, 1, 2))
    errs = {"y": rel(y_hip, ref.detach()), "dx": rel(dx.permute(0, 3, 1, 2), x6.grad), "dgamma": rel(dgam, g6.grad),
            "dbeta": rel(dbet, b6.grad), "running_mean": rel(rm, rm6), "running_var": rel(rv, rv6)}
    print("N=%d %dx%d C=%d %s: %s" % (N, H, W, C, act, {k: "%.1e" % v for k, v in errs.items()}))
    assert errs["y"] < 1e-5 and errs["running_mean"] < 1e-5 and errs["running_var"] < 1e-5, errs
    assert errs["dx"] < 1e-4 and errs["dgamma"] < 1e-4 and errs["dbeta"] < 1e-4, errs
    # eval: the running statistics, no update
    rm_e, rv_e = rm0.clone(), rv0.clone()
    cnt = torch.zeros((), dtype=torch.long, device="cuda")
    ye, _, _, _ = _bn_layer_run(x, gy, gamma, beta, rm_e, rv_e, cnt, a, training=False)
    pe = F.batch_norm(x.double().permute(0, 3, 1, 2), rm0.double(), rv0.double(), gamma.double(), beta.double(), False)
    pe = F.leaky_relu(pe, 0.2) if act == "lrelu" else torch.tanh(pe)
    assert rel(ye.permute(0, 3, 1, 2), pe) < 1e-5
    assert torch.equal(rm_e, rm0) and torch.equal(rv_e, rv0) and int(cnt) == 0


def _case(name):
    return dict(GOLD_CASES[name]["opt"])


@pytest.mark.parametrize("name", sorted(GOLD_CASES))
def test_nonspade_train_step_matches_oracle(name, monkeypatch):
    """G+D step (tape replay, D step from the oracle's post-G state) against the substituted oracle with the bounds and
    post-step state checks of test_gpu_model.py::test_train_step_matches_oracle; num_batches_tracked equals the oracle's."""
    from tests import test_gpu_model as TGM
    install_nonspade_norm(monkeypatch.setattr)
    monkeypatch.setitem(TGM.CASES, name, _case(name))
    captured = {}
    run_case = TGM.run_case

    def spy(*a, **kw):
        out = run_case(*a, **kw)
        captured["r"] = out
        return out
    monkeypatch.setattr(TGM, "run_case", spy)
    TGM.test_train_step_matches_oracle(name)
    orc, tm = captured["r"][0], captured["r"][1]
    for net in ("D", "E"):
        sd = getattr(tm.sr_model, "net" + net).state_dict()
        cnts = {k: int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")}
        assert cnts == {k: int(orc.S[net][k]) for k in cnts}, (net, cnts)
        if _case(name).get("norm_" + net, "spectralinstance") == "spectralbatch":
            assert cnts and max(cnts.values()) > 0, cnts


@pytest.mark.parametrize("name", sorted(GOLD_CASES))
def test_nonspade_statistics_track_oracle_over_iterations(name, monkeypatch):
    """The fixture's iterations (two for indep_dbatch_two_iters) run on the HIP model on its own, with no oracle state loaded
    in between: D's and E's running statistics, moved by the HIP G step and D step of every iteration, and their
    num_batches_tracked equal the oracle's at the end."""
    from tests import test_gpu_model as TGM
    install_nonspade_norm(monkeypatch.setattr)
    iters = GOLD_CASES[name]["iters"]
    orc, tm, out = TGM.run_case(_case(name), seed=101 + len(name), iters=iters, sync_before_d=False)
    assert len(out) == iters
    for it, r in enumerate(out):
        for k, v in r["gl"].items():
            assert abs(r["hgl"][k] - v) <= (1e-4 if it == 0 else 2e-2) * abs(v) + 1e-6, (it, k, r["hgl"][k], v)
    moved = 0
    for net in ("D", "E"):
        sd = getattr(tm.sr_model, "net" + net).state_dict()
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(orc.S[net][k]), (net, k, int(v), int(orc.S[net][k]))
                moved += int(v)
            elif k.endswith(("running_mean", "running_var")):
                assert rel(v.cpu(), orc.S[net][k].detach()) < 2e-3, (net, k, rel(v.cpu(), orc.S[net][k].detach()))
    if "spectralbatch" in (_case(name).get("norm_D"), _case(name).get("norm_E")):
        assert moved >= 2 * iters, moved


@pytest.mark.parametrize("norms", [("spectralbatch", "spectralbatch"), ("spectralsync_batch", "spectralnone"),
                                   ("spectralnone", "spectralsync_batch")])
def test_nonspade_inference_modes_match_oracle(norms, monkeypatch):
    """inference / encode_only / demo (eval mode: E normalises with its running statistics) against the oracle."""
    from tests import test_gpu_model as TGM
    install_nonspade_norm(monkeypatch.setattr)
    monkeypatch.setitem(TGM.CASES, "indep_8to64_ngf8", dict(TGM.CASES["indep_8to64_ngf8"], norm_D=norms[0], norm_E=norms[1]))
    TGM.test_inference_mode_matches_oracle()


def _d_fake_half(norm_d, real_seed):
    """Features of the generated half from SRModel.discriminate(train_d=False) for a fixed fake image and a real image drawn
    with `real_seed`, on a freshly built model (the same initial weights and spectral-norm vectors on every call)."""
    from deepsee_amd import ops
    from deepsee_amd.sr_model import SRModel
    from deepsee_amd.options import make_opt
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m = SRModel(make_opt(**dict(SMALL, norm_D=norm_d, seed=2)))
    batch = O.synthetic_batch(O.make_opt(**SMALL), 2, seed=3)
    labels = ops.Labels(ops.label_to_u8(batch["label"].float().cuda()), 19)
    g = torch.Generator().manual_seed(4)
    fake = ops.to_nhwc((torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).cuda()).requires_grad_()
    real = ops.to_nhwc((torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(real_seed)) * 2 - 1).cuda())
    pred, pred_real = m.discriminate(labels, fake, real, train_d=False)
    loss = sum(ops.mean_loss(p[-1], None, ops.MODE_NEG, 1.0, valid_c=1, lo=0, hi=2) for p in pred)
    loss.backward()
    torch.cuda.synchronize()
    return [t[:2].detach().cpu() for p in pred for t in p], fake.grad.cpu(), [t.cpu() for p in pred_real for t in p]


def test_g_step_fake_half_depends_on_real_half_only_under_batch_norm():
    """With BatchNorm in D the statistics of the G step's D pass span cat([fake; real]): changing only the real images changes
    the generated half's features and its gradient.  With InstanceNorm the generated half is independent of them."""
    for norm_d, depends in (("spectralbatch", True), ("spectralsync_batch", True), ("spectralinstance", False)):
        f1, g1, r1 = _d_fake_half(norm_d, 10)
        f2, g2, r2 = _d_fake_half(norm_d, 11)
        diff = max(rel(a, b) for a, b in zip(f1, f2))
        assert rel(r1[0], r2[0]) > 1e-2
        if depends:
            assert diff > 1e-3 and rel(g1, g2) > 1e-3, (norm_d, diff, rel(g1, g2))
        else:
            assert diff == 0.0 and torch.equal(g1, g2), (norm_d, diff)


def _steps(over, n_steps, batch):
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    tm = TrainerManager(make_opt(**over))
    out = []
    for _ in range(n_steps):
        tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
        fake = tm.get_latest_generated().detach().cpu()
        tm.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
        out.append((fake, {k: float(v.detach()) for k, v in tm.get_latest_losses().items()}))
    torch.cuda.synchronize()
    bufs = {"%s/%s" % (n, k): v.detach().cpu().clone() for n in ("D", "E")
            for k, v in getattr(tm.sr_model, "net" + n).state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    return out, bufs


def test_nonspade_graphs_and_half_mode():
    """Three G+D steps replayed from captured graphs equal the same steps run eagerly: losses, images, running statistics and
    num_batches_tracked (2 per iteration in D, 2 per iteration in the encoder branch the coins picked).  One 16-bit step stays
    within the 16-bit bounds of the InstanceNorm tests (image 3e-2, losses 5 %)."""
    over = dict(SMALL, seed=11, norm_D="spectralbatch", norm_E="spectralbatch")
    batch = O.synthetic_batch(O.make_opt(**SMALL), 2, seed=5)
    eager, eb = _steps(dict(over, hip_graphs=False), 3, batch)
    graph, gb = _steps(dict(over, hip_graphs=True), 3, batch)
    for (fe, le), (fg, lg) in zip(eager, graph):
        assert rel(fg, fe) <= 1e-6, rel(fg, fe)
        for k in le:
            assert abs(lg[k] - le[k]) <= 1e-5 * abs(le[k]) + 1e-7, (k, lg[k], le[k])
    assert set(eb) == set(gb) and eb
    for k in eb:
        if k.endswith("num_batches_tracked"):
            assert int(eb[k]) == int(gb[k]), (k, int(eb[k]), int(gb[k]))
        else:
            assert rel(gb[k], eb[k]) <= 1e-6, k
    dcnt = [int(v) for k, v in eb.items() if k.startswith("D/") and k.endswith("num_batches_tracked")]
    assert dcnt and all(c == 6 for c in dcnt), dcnt
    ecnt = {k: int(v) for k, v in eb.items() if k.startswith("E/") and k.endswith("num_batches_tracked")}
    assert sum(ecnt.values()) > 0 and all(v % 2 == 0 for v in ecnt.values()), ecnt
    half, _ = _steps(dict(over, precision="fp16"), 1, batch)
    assert rel(half[0][0], eager[0][0]) < 3e-2, rel(half[0][0], eager[0][0])
    for k, v in eager[0][1].items():
        assert abs(half[0][1][k] - v) <= 0.05 * abs(v) + 0.05, (k, half[0][1][k], v)


def test_nonspade_checkpoint_roundtrip(tmp_path):
    """save / load_weights round-trips the new D / E entries, running statistics and counters included; the saved keys are
    the reference model's (fixture)."""
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    rec = json.load(open(os.path.join(GOLD, "indep_dbatch_ebatch_4to32_bs2_ngf8.json")))
    over = dict(rec["opt"], checkpoints_dir=str(tmp_path), name="ck", hip_graphs=False)
    batch = O.synthetic_batch(O.make_opt(**SMALL), 2, seed=5)
    tm = TrainerManager(make_opt(**over))
    tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
    tm.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
    torch.cuda.synchronize()
    tm.save("latest")
    tm2 = TrainerManager(make_opt(**dict(over, continue_train=True, seed=5)))
    for net in ("D", "E"):
        ck = torch.load(str(tmp_path / "ck" / ("latest_net_%s.pth" % net)))["model"]
        ref = {k.split("/", 1)[1] for k in rec["iters"][0]["state_norms"] if k.startswith(net + "/")}
        assert set(ck) == ref, set(ck) ^ ref
        a = getattr(tm.sr_model, "net" + net).state_dict()
        b = getattr(tm2.sr_model, "net" + net).state_dict()
        assert set(a) == set(b) == ref
        assert all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])]
        moved = [k for k in a if k.endswith("num_batches_tracked") and int(a[k]) > 0]
        assert moved or net == "E"


def test_nonspade_sync_bn_world1_equals_plain():
    """A 1-rank RCCL group with opt.sync_bn: D / E BatchNorm statistics and backward sums go through the all-gather /
    all-reduce (the identity at world 1) and reproduce the plain single-process step."""
    import torch.distributed as dist
    from deepsee_amd import parallel
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    from tests.test_gpu_model import _free_port
    over = dict(SMALL, norm_D="spectralbatch", norm_E="spectralsync_batch", seed=3, hip_graphs=False,
                kernel_plan=dict(producer_stats=False))
    batch = O.synthetic_batch(O.make_opt(**SMALL), 2, seed=91)

    def steps(tm):
        out = []
        for _ in range(1):
            tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
            tm.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
            out.append({k: float(v) for k, v in tm.get_latest_losses().items()})
        torch.cuda.synchronize()
        bufs = {k: v.detach().cpu().clone() for k, v in tm.sr_model.netD.state_dict().items() if "running" in k}
        return out, tm.optimizer_D.flat.detach().cpu().clone(), bufs

    plain = steps(TrainerManager(make_opt(**over)))
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0, world_size=1)
    try:
        tm = TrainerManager(make_opt(**dict(over, sync_bn=True, sync_bn_clamp=False)))
        parallel.attach(tm, 1, chunk_mb=0.25, force=True)
        assert tm.sr_model.plan.sync_bn is not None
        dp = steps(tm)
    finally:
        dist.destroy_process_group()
    for a, b in zip(plain[0], dp[0]):
        print("plain %s / sync_bn %s" % (a, b))
        for k in a:
            assert abs(a[k] - b[k]) <= 2e-4 * abs(a[k]) + 1e-6, (k, a[k], b[k])
    # beta1 = 0 Adam: elements whose gradient is rounding noise may step the other way (lr_D = 4e-4)
    assert float((plain[1] - dp[1]).abs().max()) <= 2.5 * 4e-4
    for k in plain[2]:
        assert rel(dp[2][k], plain[2][k]) < 1e-4, k


DP_OVER = dict(start_size=8, crop_size=64, load_size=64, ngf=8, add_noise=False, noisy_style_scale=0.0,
               norm_D="spectralbatch", norm_E="spectralbatch")


def _d_grads(tm):
    return {nm: tm.optimizer_D.grad_view(nm).detach().cpu().clone() for nm in tm.optimizer_D.names}


def _two_gpu_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import warnings
    warnings.simplefilter("ignore", RuntimeWarning)
    import torch.distributed as dist
    from deepsee_amd import parallel
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    parallel.init_distributed(backend="nccl")
    tm = TrainerManager(make_opt(seed=3, sync_bn=True, sync_bn_clamp=False, batchSize=2, **DP_OVER))
    parallel.attach(tm, world, chunk_mb=0.25)
    full = O.synthetic_batch(O.make_opt(**dict(DP_OVER, batchSize=2 * world)), 2 * world, seed=91)
    shard = {k: v[2 * rank:2 * rank + 2].clone() for k, v in full.items()}
    tm.run_generator_one_step({k: v.clone() for k, v in shard.items()})
    tm.run_discriminator_one_step({k: v.clone() for k, v in shard.items()})
    torch.cuda.synchronize()
    bufs = {k: v.detach().cpu().clone() for k, v in tm.sr_model.netD.state_dict().items() if "running" in k}
    q.put((rank, _d_grads(tm), bufs, tm.optimizer_D.flat.detach().cpu()))
    dist.barrier()
    tm.close()
    dist.destroy_process_group()


def test_nonspade_two_gpu_sync_bn():
    """Needs TWO MI355X (skipped otherwise): 2 ranks with opt.sync_bn and BatchNorm in D and E against one process on the
    concatenated batch.  The all-reduced backward sums (count = world x local pixels) give the single-process data
    gradients, and dgamma / dbeta from the rank-local sums give, after the gradient all-reduce, the single-process parameter
    gradients (taking the all-reduced sums instead doubles them).  D's running statistics follow the global batch."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the SyncBN path on one GPU: test_nonspade_sync_bn_world1_equals_plain)")
    import torch.multiprocessing as mp
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    from tests.test_gpu_model import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_two_gpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
    assert torch.equal(res[0][3], res[1][3])
    tm = TrainerManager(make_opt(seed=3, batchSize=4, hip_graphs=False, **DP_OVER))
    full = O.synthetic_batch(O.make_opt(**dict(DP_OVER, batchSize=4)), 4, seed=91)
    tm.run_generator_one_step({k: v.clone() for k, v in full.items()})
    tm.run_discriminator_one_step({k: v.clone() for k, v in full.items()})
    torch.cuda.synchronize()
    ref, got = _d_grads(tm), res[0][1]
    # (the flat gradient may carry the 1/world of the mean in the Adam launch: calibrated on model0, a layer without a norm)
    k0 = next(k for k in ref if k.endswith("discriminator_0.model0.0.weight"))
    c = float((got[k0].double() * ref[k0].double()).sum() / ref[k0].double().pow(2).sum())
    assert abs(c - 1.0) < 1e-2 or abs(c - 2.0) < 2e-2, c
    bn = [k for k in ref if ".1.weight" in k or ".1.bias" in k]
    assert bn
    for k in ref:
        assert rel(got[k] / c, ref[k]) < 1e-2, (k, rel(got[k] / c, ref[k]))
    bufs = {k: v.detach().cpu() for k, v in tm.sr_model.netD.state_dict().items() if "running" in k}
    for k in bufs:
        assert rel(res[0][2][k], bufs[k]) < 1e-3, k
