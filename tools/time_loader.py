"""Times of the loader's two halves (profiles/loader.md).

Host, on any CPU: FolderDataset[i] (decode + PIL resize + crop) against RawFolderDataset[i] (decode only) per sample, for a
1024 x 1024 JPEG and a 512 x 512 PNG label written to a temporary folder, load_size = crop_size = 256.

Device, with --gpu (fails without one): HIP events around repeated calls after a warm-up, per call --
dsee_resample_u8 for a batch of 8 raw 1024^2 images -> 256^2 (bicubic; tables already on the device) and the matching
512^2 -> 256^2 nearest label batch, the table build + upload + both calls as device_preprocess issues them (host clock around a
synchronise), and dsee_interp_down 256^2 -> 32^2 for bilinear, nearest and area next to dsee_bicubic_down.

    python tools/time_loader.py [--gpu] [--samples 8] [--reps 200]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_files(folder, n):
    from PIL import Image
    os.makedirs(os.path.join(folder, "lab"))
    os.makedirs(os.path.join(folder, "img"))
    rng = np.random.default_rng(0)
    for i in range(n):
        # smooth content + noise: a JPEG of pure noise decodes slower than a photograph
        yy, xx = np.mgrid[0:1024, 0:1024]
        base = np.stack([(np.sin(xx / (37.0 + 5 * c) + i) + np.cos(yy / (53.0 + 3 * c))) * 60 + 128 for c in range(3)], -1)
        img = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(folder, "img", "%03d.jpg" % i), quality=90)
        cells = rng.integers(0, 19, (16, 16), dtype=np.uint8)
        Image.fromarray(np.repeat(np.repeat(cells, 32, 0), 32, 1)).save(os.path.join(folder, "lab", "%03d.png" % i))


def host_times(n):
    from deepsee_amd import data as D
    from deepsee_amd.options import make_opt
    opt = make_opt(load_size=256, crop_size=256)
    out = {}
    with tempfile.TemporaryDirectory() as folder:
        write_files(folder, n)
        for name, cls in (("FolderDataset", D.FolderDataset), ("RawFolderDataset", D.RawFolderDataset)):
            ds = cls(opt, os.path.join(folder, "lab"), os.path.join(folder, "img"))
            ds[0]                                                   # file cache, PIL's lazy imports
            ts = []
            for _ in range(3):
                for i in range(n):
                    t0 = time.perf_counter()
                    ds[i]
                    ts.append(time.perf_counter() - t0)
            out[name + "_ms_per_sample"] = {"median": 1e3 * float(np.median(ts)), "min": 1e3 * min(ts), "max": 1e3 * max(ts)}
    return out


def device_times(reps):
    import torch
    from deepsee_amd import data as D, ops, resample as R
    from deepsee_amd.options import make_opt
    assert torch.cuda.is_available(), "--gpu needs the MI355X"
    opt = make_opt(load_size=256, crop_size=256)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (8, 1024, 1024, 3), generator=g, dtype=torch.uint8).cuda()
    lab = torch.randint(0, 19, (8, 512, 512), generator=g, dtype=torch.uint8).cuda()
    pos = [(0, 0)] * 8

    def tables(wh, filt):
        geos = [R.load_geometry(opt, wh, p) for p in pos]
        tab = R.batch_tables(geos, filt)
        return {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in tab.items()}, geos[0]

    ti, gi = tables((1024, 1024), R.BICUBIC)
    tl, gl = tables((512, 512), R.NEAREST)
    hr = ops.new(8, 256, 256, 4).uniform_(-1, 1)
    hr.dsee_layout = "nhwc"
    work = {
        "resample_u8 image 8 x 1024^2 -> 256^2 bicubic": lambda: ops.resample_u8(img, ti, gi["out"], gi["box"]),
        "resample_u8 label 8 x 512^2 -> 256^2 nearest": lambda: ops.resample_u8(lab, tl, gl["out"], gl["box"]),
        "bicubic_down 8 x 256^2 -> 32^2": lambda: ops.bicubic_down(hr, 32),
        "interp_down bilinear 8 x 256^2 -> 32^2": lambda: ops.interp_down(hr, 32, "bilinear"),
        "interp_down nearest 8 x 256^2 -> 32^2": lambda: ops.interp_down(hr, 32, "nearest"),
        "interp_down area 8 x 256^2 -> 32^2": lambda: ops.interp_down(hr, 32, "area"),
    }
    out = {}
    for name, fn in work.items():
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name + " [us per call, HIP events over %d calls]" % reps] = 1e3 * a.elapsed_time(b) / reps
    # tables + upload + both resamplings as device_preprocess issues them, from device-resident raw tensors
    for _ in range(5):
        D.resample_raw(opt, img, pos, R.BICUBIC), D.resample_raw(opt, lab, pos, R.NEAREST)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        D.resample_raw(opt, img, pos, R.BICUBIC), D.resample_raw(opt, lab, pos, R.NEAREST)
    torch.cuda.synchronize()
    out["tables + upload + resample image and label, batch of 8 [us, host clock over 50 batches]"] = 1e6 * (time.perf_counter() - t0) / 50
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    res = {"host": host_times(a.samples)}
    if a.gpu:
        res["device"] = device_times(a.reps)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
