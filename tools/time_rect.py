"""A non-square train step on one MI355X (profiles/rect_model.md): wall time of one G+D step of the independent 8x model at
40 x 32 -> 320 x 256 (start_size 32, crop_size 256, aspect_ratio 0.8: what preprocess_mode='fixed' loads), next to the square
32 -> 256 configuration of the same build, per --precisions, with hip_graphs=True.

Each configuration runs --warmup steps (eager first occurrences and captures of every encoder-branch variant) and then --steps
timed ones: time.perf_counter around run_generator_one_step + run_discriminator_one_step + a device synchronisation; the figure is
the median, with min and max.  Steps that were not replays (a variant met for the first or second time) are counted and left out
of the median.  --levels prints, per generator level of a configuration, the kernel family the host dispatch picks (the
conditions of deepsee_amd.ops: _wino_ok for the 3x3 convolutions, _wino_mod_chunk / _fused_norm_ok for the SPADE / SEAN norm),
without a device.  Prints one JSON line.

    python tools/time_rect.py [--steps 20] [--warmup 12] [--precisions fp32 fp16] [--batch 8]
    python tools/time_rect.py --levels            # the dispatch table only (no GPU needed)
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    # (max_fm_size: at least the long side -- the cap on a non-square map is refused, sr_model.check_geometry)
    "rect_40x32_to_320x256": dict(start_size=32, crop_size=256, aspect_ratio=0.8, max_fm_size=320),
    "square_32_to_256": dict(start_size=32, crop_size=256, aspect_ratio=1.0),
}
# the shapes of tests/test_gpu_rect_model.py (tools/gen_golden_rect.py), for the dispatch table
TEST_CASES = {
    "indep_5x4_to_40x32": dict(start_size=4, crop_size=32, aspect_ratio=0.8, batchSize=2, ngf=8),
    "indep_4x8_to_32x64": dict(start_size=8, crop_size=64, aspect_ratio=2.0, batchSize=2, ngf=8),
    "guided_8x4_to_64x32": dict(start_size=4, crop_size=32, aspect_ratio=0.5, batchSize=2, ngf=8, netE="fullstyle"),
}


def levels(over, precision="fp32"):
    """[{level, block, kind, h, w, tiles_per_image, norm, conv}] of a configuration: which kernel family each generator block
    takes, from the host-side dispatch conditions alone."""
    from deepsee_amd import ops
    from deepsee_amd.options import make_opt
    from deepsee_amd.plan import from_opt
    from deepsee_amd.sr_model import block_plan
    from tools.gen_golden_rect import hr_shape
    opt = make_opt(**dict(over, precision=precision))
    n, c = opt.batchSize, 16 * opt.ngf
    H, W = hr_shape(opt)
    lh, lw = ops.lr_shape(opt, H, W)
    rows, level = [], 0
    with from_opt(opt).active():
        for i, (name, kind) in enumerate(block_plan(opt)):
            if i == 1 or i >= 3:
                level += 1
            h, w = lh << level, lw << level
            tpi = (h // 4) * (w // 4) if h % 4 == 0 and w % 4 == 0 else None
            if kind != "spade" and (h * w) % 128:
                norm = "dense (style map gathered, direct kernels)"
            else:
                table = kind != "spade"
                ld = 160 if table else 128
                nb = ops._wino_mod_chunk(n, h, w, c, 2 * c, table)
                if nb and ops._fused_norm_ok(n, h, w, c, 2 * c, ld):
                    norm = "fused SPADE/SEAN forward (Winograd domain)"
                elif nb:
                    norm = "Winograd-domain gamma/beta GEMM"
                else:
                    norm = "table path, direct gamma/beta convolution"
            conv = "Winograd F(4x4,3x3)" if ops._wino_ok(n, h, w, c, c, 3, 1, 1, 0) else "direct implicit GEMM"
            rows.append(dict(level=level, block=name, kind=kind, h=h, w=w, tiles_per_image=tpi, norm=norm, conv=conv))
    return rows


def time_config(name, over, precision, batch, steps, warmup):
    import torch
    from oracle import deepsee_oracle as O
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    from tools.gen_golden_rect import install_rect
    install_rect()
    over = dict(over, batchSize=batch)
    torch.manual_seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tm = TrainerManager(make_opt(**dict(over, precision=precision, hip_graphs=True)))
    data = O.synthetic_batch(O.make_opt(**over), batch, seed=7)
    times, not_replayed = [], 0
    for step in range(warmup + steps):
        before = tm.graph_stats["replayed"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tm.run_generator_one_step(data)
        tm.run_discriminator_one_step(data)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if step >= warmup:
            if tm.graph_stats["replayed"] - before == 2:
                times.append(dt)
            else:
                not_replayed += 1
    shape = tuple(tm.get_latest_generated().shape)
    losses = {k: round(float(v), 5) for k, v in tm.get_latest_losses().items()}
    rec = {"config": name, "precision": precision, "batch": batch, "generated": list(shape), "timed_steps": len(times),
           "steps_not_replayed": not_replayed, "graph_stats": dict(tm.graph_stats), "losses": losses,
           "peak_memory_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    if times:
        med = statistics.median(times)
        rec.update(step_ms={"median": round(med * 1e3, 2), "min": round(min(times) * 1e3, 2), "max": round(max(times) * 1e3, 2)},
                   images_per_s=round(batch / med, 1), megapixels_per_s=round(batch * shape[2] * shape[3] / med / 1e6, 2))
    tm.close()
    del tm
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precisions", nargs="+", default=["fp32", "fp16"])
    ap.add_argument("--levels", action="store_true", help="print the per-level dispatch table and exit (no GPU)")
    a = ap.parse_args()
    table = {name: levels(over) for name, over in TEST_CASES.items()}
    for name, over in CONFIGS.items():
        for p in a.precisions:
            table["%s_bs%d_%s" % (name, a.batch, p)] = levels(dict(over, batchSize=a.batch), p)
    if a.levels:
        print(json.dumps({"levels": table}), flush=True)
        return
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    rec = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "runs": [], "levels": table}
    for p in a.precisions:
        for name, over in CONFIGS.items():
            rec["runs"].append(time_config(name, over, p, a.batch, a.steps, a.warmup))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
