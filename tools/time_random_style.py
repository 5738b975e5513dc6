"""opt.random_style_matrix on one MI355X (profiles/random_style.md).

    python tools/time_random_style.py kernels [--warmup 20] [--calls 50] [--windows 5]
        the fused first encoder layer (dsee_onehot_noise_conv3x3_fwd / _wgrad on a Philox field) against the materialised route
        built from the entry points the project had before: dsee_rng_fill of [N,H,W,pad4(label_nc)], the mask multiply
        (dsee_label_onehot + one element-wise product), ops.conv2d forward and its weight gradient with Cin = label_nc --
        same process, same device.  HIP events around every stage of `calls` back-to-back iterations, `windows` times after
        `warmup` iterations; per stage the median window and (min - max), in microseconds per call.
    python tools/time_random_style.py step [--warmup 10] [--steps 20] [--windows 3]
        G+D train steps of the guided preset (guided_8x_256, bs 8, hipGraphs on) with and without the flag, in one run

Each mode prints JSON lines."""
import argparse
import json
import os
import random
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(8, 256, 256), (1, 512, 512)]
LABEL_NC, NEF = 19, 32


def _stages(fns, warmup, calls, windows):
    """fns: [(name, callable)], run in order per iteration -> {name: (median, min, max)} in us per call."""
    import torch
    for _ in range(warmup):
        for _, f in fns:
            f()
    torch.cuda.synchronize()
    per = {nm: [] for nm, _ in fns}
    for _ in range(windows):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(calls)]
        for i in range(calls):
            ev[i][0].record()
            for j, (_, f) in enumerate(fns):
                f()
                ev[i][j + 1].record()
        torch.cuda.synchronize()
        for j, (nm, _) in enumerate(fns):
            per[nm].append(sum(ev[i][j].elapsed_time(ev[i][j + 1]) for i in range(calls)) * 1e3 / calls)
    return {nm: (round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)) for nm, v in per.items()}


def kernels(a):
    import ctypes as C
    import torch
    from deepsee_amd import lib as L
    from deepsee_amd import networks as N
    from deepsee_amd import ops
    torch.cuda.set_device(0)
    noise = N.DeviceNoise(3)
    noise.begin_step()
    g = torch.Generator().manual_seed(1)
    for n, h, w in CASES:
        cells = torch.randint(0, LABEL_NC, (n, 1, h // 16, w // 16), generator=g).float()
        lab = torch.nn.functional.interpolate(cells, size=(h, w), mode="nearest")[:, 0].to(torch.uint8).cuda()
        labels = ops.Labels(lab, LABEL_NC)
        wt = (torch.randn(NEF, LABEL_NC, 3, 3, generator=g) * 0.1).cuda()
        dout = torch.randn(n, h, w, NEF, generator=g).cuda()
        m, cs = n * h * w, L.pad4(LABEL_NC)
        # ---- fused
        table, out = ops.new(9, LABEL_NC, NEF), ops.new(n, h, w, NEF)
        dw = ops.new(NEF, LABEL_NC, 3, 3)
        ws = ops.scratch(L.lib().dsee_onehot_noise_conv3x3_wgrad_workspace(n, h, w, LABEL_NC, NEF), "ohn")
        seed, off = C.c_uint64(77), C.c_uint64(5)

        def f_fwd():
            L.call("onehot_conv3x3_pack", wt, table, NEF, LABEL_NC)
            L.call("onehot_noise_conv3x3_fwd", lab, None, seed, off, 1, table, None, out, n, h, w, LABEL_NC, NEF)

        def f_wgrad():
            L.call("onehot_noise_conv3x3_wgrad", lab, None, seed, off, 1, dout, n, h, w, LABEL_NC, NEF, dw, None, ws)
        fused = _stages([("fwd", f_fwd), ("wgrad", f_wgrad)], a.warmup, a.calls, a.windows)
        # ---- materialised
        st = {}
        onehot = ops.new(n, h, w, 32)
        wreq = wt.clone().requires_grad_()

        def m_fill():
            st["field"] = ops.rng_fill((n, h, w, cs), 77, 5, True)

        def m_mask():
            L.call("label_onehot", lab, onehot, n, h, w, 0, 32, 0)
            st["x"] = (st["field"] * onehot[..., :cs]).contiguous()

        def m_fwd():
            st["y"] = ops.conv2d(st["x"], wreq, None)

        def m_wgrad():
            wreq.grad = None
            st["y"].backward(dout)
        mat = _stages([("rng_fill", m_fill), ("mask", m_mask), ("conv_fwd", m_fwd), ("conv_wgrad", m_wgrad)], a.warmup, a.calls,
                      a.windows)
        # the two routes compute the same layer (the Philox positions differ: one scalar per pixel against pad4(label_nc))
        f_fwd()
        f_wgrad()
        field = ops.rng_fill((m,), 77, 5, True).reshape(n, h, w)
        x = (field[..., None] * onehot[..., :cs]).contiguous()
        wr = wt.clone().requires_grad_()
        y = ops.conv2d(x, wr, None)
        y.backward(dout)
        torch.cuda.synchronize()
        agree = (float((out - y.detach()).norm() / y.detach().norm()), float((dw - wr.grad).norm() / wr.grad.norm()))
        nbytes = {"fused_fwd": m + 4 * 9 * LABEL_NC * NEF + 4 * m * NEF,
                  "fused_wgrad": m + 4 * m * NEF + 4 * 9 * LABEL_NC * NEF,
                  "materialised_fwd": 4 * m * cs + (m + 4 * m * 32 + 4 * m * 32 + 2 * 4 * m * cs) + (4 * m * cs + 4 * m * NEF),
                  "materialised_wgrad": 4 * m * cs + 4 * m * NEF}
        print(json.dumps({"mode": "kernels", "shape": [n, h, w], "label_nc": LABEL_NC, "nef": NEF, "calls": a.calls,
                          "windows": a.windows, "fused_us": fused, "materialised_us": mat,
                          "fused_total_us": round(sum(v[0] for v in fused.values()), 1),
                          "materialised_total_us": round(sum(v[0] for v in mat.values()), 1),
                          "algorithmic_bytes": nbytes, "routes_agree_rel": [float("%.3g" % v) for v in agree]}))


def step(a):
    import torch
    import bench
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    torch.cuda.set_device(0)
    for flag in (False, True):
        opt = make_opt("guided_8x_256", batchSize=8, seed=0, random_style_matrix=flag)
        random.seed(1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            tm = TrainerManager(opt)
        b = bench.synthetic_batch(opt, 8, 1234, "cuda")

        def one():
            tm.run_generator_one_step(b)
            tm.run_discriminator_one_step(b)
        for _ in range(a.warmup):
            one()
        torch.cuda.synchronize()
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
        print(json.dumps({"mode": "step", "preset": "guided_8x_256", "bs": 8, "random_style_matrix": flag, "warmup": a.warmup,
                          "steps_per_window": a.steps, "ms_per_step": [round(v, 2) for v in ms],
                          "graph_stats": tm.graph_stats, "losses": losses}))
        tm.close()
        del tm, b
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--warmup", type=int, default=20)
    k.add_argument("--calls", type=int, default=50)
    k.add_argument("--windows", type=int, default=5)
    s = sub.add_parser("step")
    s.add_argument("--warmup", type=int, default=10)
    s.add_argument("--steps", type=int, default=20)
    s.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    {"kernels": kernels, "step": step}[a.mode](a)


if __name__ == "__main__":
    main()
