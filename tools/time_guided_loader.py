"""Throughput of the raw file loader with and without guiding images (profiles/guided_loader.md).

Writes --files pairs of a 1024 x 1024 JPEG and a 512 x 512 PNG label map (the content of tools/time_loader.py) and an identities
file with four files per identity to a temporary folder, then times, for N = 8, load_size = crop_size = 256:

  loader      batches per second of DeviceLoader over RawFolderDataset for every --workers value, unguided and guided: host clock
              over --epochs epochs (one warm-up epoch first), the consumer only synchronises at the end of an epoch;
  device      the device part of one staged batch alone (upload from pinned memory, tables, dsee_resample_u8, normalise, label
              remap, LR image): HIP events on the loader's side stream around --reps calls of device_preprocess.

--package-root <dir> imports deepsee_amd from another tree (a checkout of the parent commit next to its built library), which is
how the unguided numbers of two commits are taken on one box, in alternating processes; --variants unguided is all such a tree
can run.  Uses at most 16 host threads.

    python tools/time_guided_loader.py [--variants unguided,guided] [--workers 0,8,16] [--package-root DIR] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_files(folder, n):
    from PIL import Image
    os.makedirs(os.path.join(folder, "lab"))
    os.makedirs(os.path.join(folder, "img"))
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:1024, 0:1024]
    with open(os.path.join(folder, "identities.txt"), "w") as f:
        for i in range(n):
            # smooth content + noise: a JPEG of pure noise decodes slower than a photograph
            base = np.stack([(np.sin(xx / (37.0 + 5 * c) + i) + np.cos(yy / (53.0 + 3 * c))) * 60 + 128 for c in range(3)], -1)
            img = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(folder, "img", "%03d.jpg" % i), quality=90)
            cells = rng.integers(0, 19, (16, 16), dtype=np.uint8)
            Image.fromarray(np.repeat(np.repeat(cells, 32, 0), 32, 1)).save(os.path.join(folder, "lab", "%03d.png" % i))
            f.write("%03d.jpg %d\n" % (i, i // 4))


def run(a):
    import torch
    from deepsee_amd import data as D
    from deepsee_amd.options import make_opt
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    res = {"package": os.path.dirname(os.path.abspath(D.__file__)), "batch": 8, "files": a.files, "epochs": a.epochs}
    with tempfile.TemporaryDirectory() as folder:
        write_files(folder, a.files)
        lab, img = os.path.join(folder, "lab"), os.path.join(folder, "img")
        for variant in a.variants.split(","):
            guided = variant == "guided"
            opt = make_opt(load_size=256, crop_size=256, batchSize=8, guiding_style_image=guided)
            kw = dict(identities=os.path.join(folder, "identities.txt"), dataset_mode="celeba") if guided else {}
            ds = D.RawFolderDataset(opt, lab, img, seed=0, **kw)
            rec = res.setdefault(variant, {})
            for w in [int(v) for v in a.workers.split(",")]:
                ld = D.DeviceLoader(ds, opt, batch_size=8, shuffle=True, workers=w)
                for _ in ld:
                    pass
                torch.cuda.synchronize()
                t0, n = time.perf_counter(), 0
                for _ in range(a.epochs):
                    for _ in ld:
                        n += 1
                    torch.cuda.synchronize()
                rec["workers=%d batches_per_s" % w] = round(n / (time.perf_counter() - t0), 3)
            ld = D.DeviceLoader(ds, opt, batch_size=8, shuffle=False)
            host = ld.collate([ds[i] for i in range(8)])
            with torch.cuda.stream(ld.side):
                for _ in range(10):
                    D.device_preprocess(opt, host)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ld.side)
                for _ in range(a.reps):
                    D.device_preprocess(opt, host)
                e1.record(ld.side)
            torch.cuda.synchronize()
            rec["device_part_ms_per_batch"] = round(e0.elapsed_time(e1) / a.reps, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="unguided,guided")
    ap.add_argument("--workers", default="0,8,16")
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=None, help="append the JSON result line to this file")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    line = json.dumps(run(a))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
