"""The GAN objective (opt.gan_mode) in the train step on one MI355X (profiles/gan_mode_step.md).

    python tools/time_gan_mode.py step GAN_MODE [--precision fp32] [--warmup 6] [--steps 20] [--windows 1] [--gap 1.0]
                                                [--per-step 0]
        G+D train steps at independent_8x_256, bs 8, hipGraphs on: `warmup` steps (eager first occurrences, captures,
        replays), a device synchronisation and `gap` seconds with the device idle, then `per_step` steps timed one by one
        and `windows` x `steps` timed steps
    python tools/time_gan_mode.py trace DIR [--steps 20]
        reads the kernel trace that `rocprofv3 --kernel-trace --output-format csv -d DIR -- ... step ...` wrote and
        splits it at its longest idle gap (the `gap` above): kernel launches per step, and the loss kernels' calls and time
        per step, over the timed steps only

Each mode prints JSON lines."""
import argparse
import csv
import glob
import json
import os
import random
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRESET, BS = "independent_8x_256", 8
LOSS_KERNELS = ("loss_partial_kernel", "loss_grad_kernel", "loss_finalize_kernel")


def step(a):
    import torch
    import bench
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    torch.cuda.set_device(0)
    opt = make_opt(PRESET, batchSize=BS, seed=0, gan_mode=a.gan_mode, precision=a.precision)
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
    torch.cuda.synchronize()
    time.sleep(a.gap)
    per_step = []
    for _ in range(a.per_step):     # device-synchronised one by one: where a slow window spends its time
        t = time.perf_counter()
        one()
        torch.cuda.synchronize()
        per_step.append(round((time.perf_counter() - t) * 1e3, 2))
    ms = []
    for _ in range(a.windows):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.steps):
            one()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3 / a.steps)
    losses = {k: round(float(v.detach()), 4) for k, v in tm.get_latest_losses().items()}
    assert all(v == v for v in losses.values()), losses
    print(json.dumps({"mode": "step", "gan_mode": a.gan_mode, "precision": a.precision, "bs": BS, "warmup": a.warmup,
                      "steps_per_window": a.steps, "ms_per_step": [round(v, 2) for v in ms], "per_step_ms": per_step,
                      "graph_stats": tm.graph_stats, "losses": losses}))
    tm.close()


def trace(a):
    paths = sorted(glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, paths
    rows = []
    with open(paths[0]) as f:
        rd = csv.DictReader(f)
        assert {"Start_Timestamp", "End_Timestamp", "Kernel_Name"} <= set(rd.fieldnames), rd.fieldnames
        for r in rd:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    # the timed region starts after the longest stretch with no kernel running (the host-side sleep)
    end, cut, gap = rows[0][1], 0, -1
    for i in range(1, len(rows)):
        if rows[i][0] - end > gap:
            gap, cut = rows[i][0] - end, i
        end = max(end, rows[i][1])
    timed = rows[cut:]
    n = a.steps
    loss = {}
    for s, e, name in timed:
        short = next((k for k in LOSS_KERNELS if k in name), None)
        if short:
            c, t = loss.get(short, (0, 0))
            loss[short] = (c + 1, t + e - s)
    gpu = sum(e - s for s, e, _ in timed)
    out = {"mode": "trace", "trace": os.path.relpath(paths[0], a.dir), "kernels_in_trace": len(rows),
           "idle_gap_ms": round(gap / 1e6, 1), "timed_kernels": len(timed), "launches_per_step": len(timed) / n,
           "kernel_ms_per_step": round(gpu / 1e6 / n, 3),
           "span_ms_per_step": round((timed[-1][1] - timed[0][0]) / 1e6 / n, 3),
           "loss_kernels_per_step": {k: c / n for k, (c, _) in sorted(loss.items())},
           "loss_kernel_us_per_step": {k: round(t / 1e3 / n, 2) for k, (_, t) in sorted(loss.items())},
           "loss_kernel_us_per_step_total": round(sum(t for _, t in loss.values()) / 1e3 / n, 2)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    s = sub.add_parser("step")
    s.add_argument("gan_mode")
    s.add_argument("--precision", default="fp32")
    s.add_argument("--warmup", type=int, default=6)
    s.add_argument("--steps", type=int, default=20)
    s.add_argument("--windows", type=int, default=1)
    s.add_argument("--gap", type=float, default=1.0)
    s.add_argument("--per-step", type=int, default=0, help="steps timed one by one before the windows")
    t = sub.add_parser("trace")
    t.add_argument("dir")
    t.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    {"step": step, "trace": trace}[a.mode](a)


if __name__ == "__main__":
    main()
