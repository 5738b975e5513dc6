"""Explorative inference on one MI355X (profiles/explore.md): wall time of `inference_interpolation` at the independent 8x
preset (32 -> 256), n_interpolation = 5, region_idx = [1, 2, 5], noise_delta = 0.4, for

  * batched:  model(data, "inference_interpolation") -- one encoder pass, dsee_style_explore, the generator over the B * n
              pairs in passes of opt.explore_chunk, dsee_nhwc_to_nchw_tiled;
  * per_pair: the reference's loop (sr_model.py:219-261) on the modes this project had before: `encode_only` once, then per
              (image, variant) the style edit in torch ops, one `demo` call at batch 1 and the reference's torch.cat's

on the same weights and inputs, for every (B, explore_chunk) of --configs.  The two are run alternately; each figure is the
median over --repeats runs after one untimed run of each (allocations, first launches), timed with time.perf_counter around the
call + a device synchronisation.  The results of the two are compared (relative L2 difference).  Kernel times come from running
this script under `rocprofv3 --kernel-trace --stats` (--repeats 1).  Prints one JSON line.

    python tools/time_explore.py [--repeats 5] [--configs 1:8 8:8 8:40 8:20] [--precision fp32]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", nargs="+", default=["1:8", "8:8", "8:40", "8:20"], help="B:explore_chunk")
    ap.add_argument("--precision", default="fp32")
    a = ap.parse_args()
    import numpy as np
    import torch
    from oracle import deepsee_oracle as O
    from deepsee_amd import ops
    from deepsee_amd.lib import DseeError
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    n, region, delta = 5, [1, 2, 5], 0.4
    opt = make_opt("independent_8x_256", batchSize=8, no_vgg_loss=True, hip_graphs=False, precision=a.precision,
                   n_interpolation=n, region_idx=region, noise_delta=delta)
    torch.manual_seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tm = TrainerManager(opt)
    model = tm.sr_model.eval()

    def batched(data):
        return model(dict(data), "inference_interpolation")["fake_image"]

    def per_pair(data):
        with torch.no_grad():
            style = model(dict(data), "encode_only")
            lr, labels = data["image_lr"], data["input_semantics"]
            images = []
            for b in range(lr.shape[0]):
                samples = []
                for step in np.linspace(-delta, delta, num=n):
                    s = style[b].clone().detach()
                    s[region] = (s[region] + step).clamp(-1, 1)
                    lr_b = lr[b:b + 1]
                    lr_b.dsee_layout = "nhwc"          # (a slice drops the layout tag of the native tensor)
                    one = {"input_semantics": ops.Labels(labels.t[b:b + 1], labels.nc), "image_lr": lr_b,
                           "encoded_style": s.unsqueeze(0)}
                    samples.append(model(one, "demo")["fake_image"])
                images.append(torch.cat(samples, -1))
            return torch.cat(images, 0)

    rec = {"device": torch.cuda.get_device_name(0), "preset": "independent_8x_256", "n": n, "precision": a.precision,
           "repeats": a.repeats, "configs": []}
    for cfg in a.configs:
        B, chunk = (int(v) for v in cfg.split(":"))
        opt.explore_chunk = chunk
        batch = O.synthetic_batch(O.make_opt(batchSize=B), B, seed=7)
        data = tm.preprocess_input({k: v.clone() for k, v in batch.items()})
        times = {"batched": [], "per_pair": []}
        outs = {}
        try:
            for r in range(a.repeats + 1):
                for name, fn in (("batched", batched), ("per_pair", per_pair)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    outs[name] = fn(data)
                    torch.cuda.synchronize()
                    if r > 0:
                        times[name].append(time.perf_counter() - t0)
        except (torch.cuda.OutOfMemoryError, DseeError) as e:    # a pass of `chunk` pairs that does not fit (memory, or a
            # kernel's argument check: 32-bit offsets into an activation): said, not hidden
            rec["configs"].append({"B": B, "explore_chunk": chunk, "error": "%s: %s" % (type(e).__name__, str(e).split("\n")[0])})
            continue
        diff = float((outs["batched"].double() - outs["per_pair"].double()).norm() / outs["per_pair"].double().norm())
        med = {k: statistics.median(v) for k, v in times.items()}
        rec["configs"].append({"B": B, "explore_chunk": chunk, "pairs": B * n,
                               "batched_ms": {"median": round(med["batched"] * 1e3, 2), "min": round(min(times["batched"]) * 1e3, 2),
                                              "max": round(max(times["batched"]) * 1e3, 2)},
                               "per_pair_ms": {"median": round(med["per_pair"] * 1e3, 2), "min": round(min(times["per_pair"]) * 1e3, 2),
                                               "max": round(max(times["per_pair"]) * 1e3, 2)},
                               "ratio": round(med["per_pair"] / med["batched"], 2), "rel_difference": diff,
                               "peak_memory_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)})
    print(json.dumps(rec), flush=True)
    tm.close()


if __name__ == "__main__":
    main()
