"""The output path on one MI355X (profiles/visuals.md): wall time of InferenceManager.run over `batches` batches of the
independent 8x preset (bs = 8, 32 -> 256)

  * plain:  scoring only, nothing written;
  * saved:  run(..., save_to=<folder>): conversion kernels + one D2H copy per batch, PNG encoding on the writer thread;
  * host:   the reference's route restated here: every visual copied to the host as fp32 (`.cpu()`), converted in numpy
            (tensor2im / Colorize arithmetic, np.concatenate for the strip) and written with PIL, all on the calling thread;

and the bytes copied device-to-host per batch by `saved` and by `host`.

    python tools/time_visuals.py [--batches 8] [--repeats 3] [--modes plain saved host] [--baseline]

Each figure is the median over `repeats` runs after one untimed run of the same kind (allocations, first launches, page cache),
timed with time.perf_counter around run() + a device synchronisation; files go to a fresh temporary folder per run.  Kernel times
come from running this script under `rocprofv3 --kernel-trace --stats` (--repeats 1 --modes saved --baseline).  Prints one JSON line."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_route(out, paths, folder, label_nc):
    """save_images_only as the reference runs it: fp32 tensors to the host, numpy, PIL, on this thread.  Returns the bytes copied."""
    import numpy as np
    from deepsee_amd import ops, visuals as V
    from tools.gen_golden_visuals import np_bilinear_up, np_colorize
    copied = 0

    def images(t):
        nonlocal copied
        if getattr(t, "dsee_layout", None) == "nhwc":
            t = ops.to_nchw(t, 3)                                     # (the reference's tensors are NCHW already)
        host = t.detach().cpu().float().numpy()
        copied += host.nbytes
        x = (np.transpose(host, (0, 2, 3, 1)) + 1) / 2.0 * 255.0
        return np.clip(x, 0, 255).astype(np.uint8)

    def colours(labels):
        nonlocal copied
        host = labels.t.cpu().numpy()
        copied += host.size * 4 * label_nc                            # the reference copies the one-hot fp32 map
        return np_colorize(host, V.labelcolormap(label_nc + 2))

    vis = {"input_semantics": colours(out["input_semantics"]), "image_lr": images(out["image_lr"]),
           "fake_image": images(out["fake_image"]), "image_hr": images(out["image_hr"])}
    h, w = vis["fake_image"].shape[1:3]
    for b, p in enumerate(paths):
        name = V._file_name(p)
        for key, v in vis.items():
            V.save_image(v[b], os.path.join(folder, key, name), create_dir=True)
        strip = np.concatenate([vis["input_semantics"][b], np_bilinear_up(vis["image_lr"][b], h, w), vis["fake_image"][b],
                                vis["image_hr"][b]], axis=1)
        V.save_image(strip, os.path.join(folder, "combined", name), create_dir=True)
    return copied


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["plain", "saved", "host"])
    ap.add_argument("--baseline", action="store_true", help="also one run(mode='baseline') (dsee_bicubic_up in a kernel trace)")
    a = ap.parse_args()
    import torch
    from deepsee_amd import visuals as V
    from deepsee_amd.data import DeviceLoader, SyntheticDataset
    from deepsee_amd.managers import InferenceManager, TrainerManager
    from deepsee_amd.options import make_opt
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    opt = make_opt("independent_8x_256", batchSize=8)
    random.seed(1)
    torch.manual_seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tm = TrainerManager(opt)
    model = tm.sr_model
    ds = SyntheticDataset(opt, length=a.batches * opt.batchSize)
    num_samples = a.batches * opt.batchSize - 1                      # run() takes num_samples // batchSize + 1 batches

    class HostRoute(InferenceManager):
        copied = 0

        def run_batch(self, data, model, mode="inference"):
            out = super().run_batch(data, model, mode)
            HostRoute.copied += host_route(out, out["path"], self.host_folder, self.opt.label_nc)
            return out

    def one(mode, folder):
        loader = DeviceLoader(ds, opt, shuffle=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "host":
            im = HostRoute(opt, num_samples)
            im.host_folder = folder
            res = im.run(model, loader)
        else:
            res = InferenceManager(opt, num_samples).run(model, loader, save_to=folder if mode == "saved" else None)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert res["n_samples"] == a.batches * opt.batchSize, res
        return dt

    rec = {"batches": a.batches, "batch_size": opt.batchSize, "size": opt.crop_size, "device": torch.cuda.get_device_name(0)}
    for mode in a.modes:
        times = []
        for r in range(a.repeats + 1):
            with tempfile.TemporaryDirectory() as folder:
                dt = one(mode, folder)
                if mode != "plain" and r == 0:
                    rec[mode + "_files"] = sum(len(f) for _, _, f in os.walk(folder))
            if r > 0:
                times.append(dt)
        rec[mode + "_wall_s"] = {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}
    if "host" in a.modes:
        rec["host_d2h_bytes_per_batch"] = HostRoute.copied // ((a.repeats + 1) * a.batches)
    batch = next(iter(DeviceLoader(ds, opt, shuffle=False)))
    with torch.no_grad():
        out = model.eval()(batch, "inference")
    model.train()
    rec["saved_d2h_bytes_per_batch"] = V._Layout(out).nbytes
    if a.baseline:
        res = InferenceManager(opt, num_samples).run(model, DeviceLoader(ds, opt, shuffle=False), mode="baseline")
        rec["baseline"] = {k: round(float(v), 4) for k, v in res.items()}
    print(json.dumps(rec), flush=True)
    tm.close()


if __name__ == "__main__":
    main()
