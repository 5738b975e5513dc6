"""Timing of the discriminator / style-encoder norms (opt.norm_D = opt.norm_E) on one MI355X (profiles/nonspade_norm_step.md).

    python tools/time_nonspade_norm.py step NORM PRECISION [--warmup 6] [--steps 20] [--windows 3]
        G+D train steps at independent_8x_256, bs 8, hipGraphs on: ms / step of every timed window (device-synchronised)
    python tools/time_nonspade_norm.py dpass [--iters 10] [--windows 5]
        the generator step's discriminator pass alone (forward + backward of its losses w.r.t. the generated images, D frozen)
        at the same geometry: InstanceNorm split (the default), InstanceNorm over cat([fake; real]) and BatchNorm over
        cat([fake; real]) (what norm_D = spectralbatch runs)
    python tools/time_nonspade_norm.py kernels [--iters 50]
        the new kernels (dsee_bn_act_fwd / _bwd_reduce / _bwd_apply) at D model1 of the G step (16 x 65^2 x 64) and encoder
        `initial` (8 x 256^2 x 32), achieved bytes/s from algorithmic bytes (8 / 12 / 16 B per element)

Each mode prints JSON lines.  One process per configuration: the step times of different configurations compare only within
one job on one machine."""
import argparse
import json
import os
import random
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRESET, BS = "independent_8x_256", 8


def _sync_ms(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def step(a):
    import bench
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    opt = make_opt(PRESET, batchSize=BS, seed=0, norm_D=a.norm, norm_E=a.norm, precision=a.precision)
    random.seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tm = TrainerManager(opt)
    b = bench.synthetic_batch(opt, BS, 1234, "cuda")

    def one():
        tm.run_generator_one_step(b)
        tm.run_discriminator_one_step(b)
    for _ in range(a.warmup):
        one()
    ms = [_sync_ms(one, a.steps) for _ in range(a.windows)]
    losses = {k: round(float(v.detach()), 4) for k, v in tm.get_latest_losses().items()}
    assert all(v == v for v in losses.values()), losses
    print(json.dumps({"mode": "step", "norm": a.norm, "precision": a.precision, "bs": BS, "steps_per_window": a.steps,
                      "ms_per_step": [round(v, 2) for v in ms], "graph_stats": tm.graph_stats, "losses": losses}))


def dpass(a):
    import bench
    from deepsee_amd import ops
    from deepsee_amd.options import make_opt
    from deepsee_amd.sr_model import SRModel
    n = BS
    res = {}
    for label, norm, concat in (("instance_split", "spectralinstance", False),
                                ("instance_concat", "spectralinstance", True),
                                ("batch_concat", "spectralbatch", True)):
        opt = make_opt(PRESET, batchSize=n, seed=0, norm_D=norm, no_vgg_loss=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            m = SRModel(opt)
        b = bench.synthetic_batch(opt, n, 1234, "cuda")
        labels = ops.Labels(ops.label_to_u8(b["label"]), opt.label_nc)
        real = ops.to_nhwc(b["image"])
        g = torch.Generator().manual_seed(3)
        fake = ops.to_nhwc((torch.rand(n, 3, 256, 256, generator=g) * 2 - 1).cuda()).requires_grad_()
        for p in m.netD.parameters():
            p.requires_grad_(False)

        def one():
            if concat:      # one pass over cat([fake; real]); the real half's features detached
                out = m.netD(ops.DInput.apply(labels, fake, real), True)
                pred, pred_real = out, [[t[n:].detach() for t in o] for o in out]
            else:
                pred, pred_real = m.discriminate(labels, fake, real, train_d=False)
            loss = 0
            for p, pr in zip(pred, pred_real):
                loss = loss + ops.mean_loss(p[-1], None, ops.MODE_NEG, 0.5, valid_c=1, lo=0, hi=n)
                for f, r in zip(p[:-1], pr[:-1]):
                    loss = loss + ops.mean_loss(f, r, ops.MODE_L1, 5.0, lo=0, hi=n)
            fake.grad = None
            loss.backward()
        for _ in range(3):
            one()
        res[label] = [round(_sync_ms(one, a.iters), 3) for _ in range(a.windows)]
        del m
        torch.cuda.empty_cache()
    print(json.dumps({"mode": "dpass", "bs": n, "iters_per_window": a.iters, "ms_per_pass": res}))


def kernels(a):
    from deepsee_amd import lib as L
    from deepsee_amd import ops
    out = []
    for what, (n, h, w, c) in (("D model1, G step (2N images)", (16, 65, 65, 64)),
                               ("encoder initial", (8, 256, 256, 32))):
        x = torch.randn(n, h, w, c, device="cuda")
        dy = torch.randn(n, h, w, c, device="cuda")
        gamma = torch.ones(c, device="cuda")
        beta = torch.zeros(c, device="cuda")
        rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        mean, invstd = ops.new(c), ops.new(c)
        L.call("norm_eval_stats", rm, rv, c, 1e-5, mean, invstd)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        sums, dg, db = ops.new(2, c), ops.new(c), ops.new(c)
        ws = torch.empty(L.lib().dsee_norm_workspace(n, h * w, c, 1) // 4, device="cuda")
        elems = n * h * w * c
        calls = {
            "bn_act_fwd": (8, lambda: L.call("bn_act_fwd", x, mean, invstd, gamma, beta, y, n, h * w, c, L.ACT_LRELU, 0.2,
                                             None)),
            "bn_act_bwd_reduce": (12, lambda: L.call("bn_act_bwd_reduce", dy, y, x, mean, invstd, n, h * w, c, L.ACT_LRELU,
                                                     0.2, sums, ws)),
            "bn_act_bwd_apply": (16, lambda: L.call("bn_act_bwd_apply", dy, y, x, mean, invstd, gamma, sums, None,
                                                    1.0 / (n * h * w), dx, dg, db, n, h * w, c, L.ACT_LRELU, 0.2, None)),
        }
        for name, (bpe, fn) in calls.items():
            for _ in range(5):
                fn()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ts = []
            for _ in range(3):
                ev0.record()
                for _ in range(a.iters):
                    fn()
                ev1.record()
                torch.cuda.synchronize()
                ts.append(ev0.elapsed_time(ev1) / a.iters)
            us = sorted(ts)[1] * 1e3
            out.append({"kernel": name, "shape": [n, h, w, c], "what": what, "MB": round(elems * 4 / 1e6, 1),
                        "us_median": round(us, 1), "us_all": [round(t * 1e3, 1) for t in ts],
                        "algorithmic_bytes_per_elem": bpe, "TB_per_s": round(elems * bpe / (us * 1e-6) / 1e12, 3),
                        "frac_of_8TBps": round(elems * bpe / (us * 1e-6) / 8e12, 3)})
    for r in out:
        print(json.dumps(dict(mode="kernels", **r)))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    s = sub.add_parser("step")
    s.add_argument("norm")
    s.add_argument("precision")
    s.add_argument("--warmup", type=int, default=6)
    s.add_argument("--steps", type=int, default=20)
    s.add_argument("--windows", type=int, default=3)
    d = sub.add_parser("dpass")
    d.add_argument("--iters", type=int, default=10)
    d.add_argument("--windows", type=int, default=5)
    k = sub.add_parser("kernels")
    k.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    {"step": step, "dpass": dpass, "kernels": kernels}[a.mode](a)


if __name__ == "__main__":
    main()
