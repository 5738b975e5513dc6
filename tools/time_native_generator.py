"""The generator forward from C on one MI355X (profiles/native_generator.md):

  * dsee_style_table_fwd at 152 x 128 x 9216 (N = 8, L = 19, S = 128, rows = 1024) next to the pair it fuses, the library GEMM of
    ops._style_gemm (rocBLAS through torch.matmul) + dsee_style_table_layout, alternating the two in blocks of --table-iters calls;
  * dsee_generator_fwd (deepsee_amd.native.NativeGenerator) at the benchmark geometry -- 32 -> 256, C = 512 -- per --batches: device
    time and host time per call, eager and replayed from one captured hipGraph, with SRModel mode "demo" (eager Python, the same
    weights and inputs) measured before AND after it: the difference of those two is the run-to-run spread the comparison has;
  * dsee_generator_prepare: wall time of the call (it ends with a stream synchronisation), paid once per checkpoint.

Device time: HIP events around --iters calls, divided by their number.  Host time: time.perf_counter around the same calls before
the synchronisation, i.e. what the calling thread spends enqueueing.  Every shape is warmed up first.  The model keeps its
initialisation weights: timings do not depend on the values.  Prints one JSON line.

    python tools/time_native_generator.py [--iters 10] [--table-iters 200] [--batches 8 4] [--ngf 32]
"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup):
    """(device ms per call, host ms per call) of fn over `iters` calls after `warmup` calls"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, host * 1e3 / iters


def time_table(iters, rounds=3):
    import torch
    from deepsee_amd import lib as L, ops
    n, l, s, rows = 8, 19, 128, 1024
    g = torch.Generator().manual_seed(3)
    style = (torch.rand(n, l, s, generator=g) * 2 - 1).cuda()
    wst = torch.randn(9 * rows, s, generator=g).cuda()
    table, slot = torch.empty(n, 9, rows, 32, device="cuda"), torch.zeros(2048, device="cuda")

    def new_kernel():
        L.call("style_table_fwd", style, wst, table, n, l, s, rows, slot)

    def library_pair():
        L.call("style_table_layout", ops._style_gemm(style.reshape(n * l, s), wst), table, n, l, rows, slot)

    new_kernel()
    mine = table.clone()
    library_pair()
    torch.cuda.synchronize()
    dev = float((mine - table).abs().max() / table.abs().max())
    runs = {"dsee_style_table_fwd": [], "matmul + dsee_style_table_layout": []}
    for _ in range(rounds):          # alternating blocks: other work shares the box
        runs["dsee_style_table_fwd"].append(round(timed(new_kernel, iters, 20)[0] * 1e3, 2))
        runs["matmul + dsee_style_table_layout"].append(round(timed(library_pair, iters, 20)[0] * 1e3, 2))
    nbytes = 4.0 * (n * l * s + 9 * rows * s + n * 9 * rows * 32)
    flop = 2.0 * n * 32 * s * 9 * rows
    best = min(runs["dsee_style_table_fwd"]) * 1e-6
    return {"shape": {"N": n, "L": l, "S": s, "rows": rows}, "device_us_per_call": runs, "iters_per_block": iters,
            "max_abs_difference_over_max_abs": dev, "algorithmic_MB": round(nbytes / 1e6, 2), "MFMA_GFLOP": round(flop / 1e9, 3),
            "new_kernel_GB_per_s": round(nbytes / best / 1e9, 1), "new_kernel_TFLOP_per_s": round(flop / best / 1e12, 2)}


def time_generator(batch, ngf, iters):
    import torch
    from deepsee_amd import ops
    from deepsee_amd.options import make_opt
    from deepsee_amd.sr_model import SRModel
    opt = make_opt(batchSize=batch, ngf=ngf, no_vgg_loss=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        model = SRModel(opt)
    model.eval()
    g = torch.Generator().manual_seed(batch)
    h = opt.start_size
    H = opt.crop_size
    image_lr = (torch.rand(batch, 3, h, h, generator=g) * 2 - 1).cuda()
    labels = torch.randint(0, opt.semantic_nc, (batch, H // 16, H // 16), generator=g).to(torch.uint8)
    labels = labels.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous().cuda()
    style = ((torch.rand(batch, opt.semantic_nc, opt.regional_style_size, generator=g) * 2 - 1) * 0.25).cuda()
    data = {"image_lr": image_lr, "input_semantics": ops.Labels(labels, opt.semantic_nc), "encoded_style": style}
    python_out = []

    def python_demo():
        python_out[:] = [model(dict(data), "demo")["fake_image"]]

    rec = {"batch": batch, "C": 16 * ngf, "lr": [h, h], "hr": [H, H], "iters": iters}
    rec["python_demo_eager_ms"] = [dict(zip(("device", "host"), (round(v, 3) for v in timed(python_demo, iters, 2))))]
    native = model.native_generator()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    native.prepare()
    rec["prepare_ms_first_call"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    native.prepare()
    rec["prepare_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    rec["prepared_MB"] = round(native.prepared_bytes / 1e6, 1)
    rec["workspace_MB"] = round(native.workspace_bytes(batch, h, h) / 1e6, 1)
    out = torch.empty(batch, 3, H, H, device="cuda")
    ws = torch.empty((native.workspace_bytes(batch, h, h) + 3) // 4, device="cuda")

    def native_eager():
        native(image_lr, labels, style, out=out, workspace=ws)

    rec["native_eager_ms"] = dict(zip(("device", "host"), (round(v, 3) for v in timed(native_eager, iters, 2))))
    torch.cuda.synchronize()
    eager_out = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        native_eager()
    rec["native_replayed_ms"] = dict(zip(("device", "host"), (round(v, 3) for v in timed(graph.replay, iters, 2))))
    torch.cuda.synchronize()
    rec["replay_equals_eager"] = bool(torch.equal(out, eager_out))
    rec["python_demo_eager_ms"].append(dict(zip(("device", "host"), (round(v, 3) for v in timed(python_demo, iters, 2)))))
    torch.cuda.synchronize()
    # the Python module forms its style tables with the library GEMM: equal up to that product's summation order -- which untrained
    # weights (sigma from random u, v: pre-tanh activations of 1e7) turn into flipped signs of saturated pixels.  With the module's
    # table product routed through dsee_style_table_fwd the two are the same bits.
    rec["native_vs_python_rel"] = float((eager_out - python_out[0]).norm() / python_out[0].norm())
    shipped = ops.style_table_packed

    def table_by_the_new_kernel(style_, wst, rows, amax=None):
        from deepsee_amd import lib as L
        n, nc, s = style_.shape
        t = ops.new(n, 9, rows, 32)
        L.call("style_table_fwd", style_.contiguous(), wst.contiguous(), t, n, nc, s, rows, amax)
        t.dsee_amax = amax
        return t

    ops.style_table_packed = table_by_the_new_kernel
    try:
        python_demo()
    finally:
        ops.style_table_packed = shipped
    torch.cuda.synchronize()
    rec["native_equals_python_on_the_same_table_kernel"] = bool(torch.equal(eager_out, python_out[0]))
    rec["peak_memory_GiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    del model, native, graph, out, ws
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--table-iters", type=int, default=200)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 4])
    ap.add_argument("--ngf", type=int, default=32)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    rec = {"device": torch.cuda.get_device_name(0), "style_table": time_table(a.table_iters),
           "generator": [time_generator(b, a.ngf, a.iters) for b in a.batches]}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
