"""Times of the loader over batches of differently sized files (profiles/mixed_loader.md).  Needs the MI355X; one process.

1. A uniform CelebAMask-HQ batch, 8 x 1024^2 RGB -> 256^2 bicubic and 8 x 512^2 label maps -> 256^2 nearest (tables already on
   the device), through dsee_resample_u8 and through dsee_resample_u8_ragged on the same pixels: `--rounds` rounds that alternate
   the two, each round a warm-up and HIP events around `--reps` calls; per entry point the median and the spread (min ... max) of
   the rounds.  dsee_resample_u8 and its kernels are those of the parent commit, untouched: it is the yardstick, and its own
   spread over the rounds is what the ragged figure is read against.  The two results are compared bit for bit first.  Timed
   twice: the entry points themselves on preallocated buffers, and the ops wrappers (for short kernels the host side of a
   wrapper, not the device, can be what a back-to-back loop measures).
2. A mixed batch: eight files between 600^2 and 1400^2 of varied aspect ratios -> 256^2 (resize_and_crop).  Device time of the
   two ragged calls (images, label maps), bytes uploaded (arenas + tables), host time per batch for the tables and for packing
   the arenas, and the whole device_preprocess of the collated batch (host clock around a synchronise); next to it the same
   eight files through FolderDataset (decode + PIL resize + crop on the host) and through RawFolderDataset (decode only).

    python tools/time_mixed_loader.py [--rounds 7] [--reps 100] [--out FILE]
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

MIXED_WH = [(600, 600), (1400, 1400), (1024, 768), (768, 1024), (1280, 720), (640, 1200), (900, 1350), (1333, 800)]


def spread(us):
    return {"median": float(np.median(us)), "min": float(min(us)), "max": float(max(us)), "rounds": [round(float(v), 2) for v in us]}


def events(fn, reps, warm=10):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def on_device(tab):
    import torch
    return {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in tab.items()}


def uniform_batch(rounds, reps):
    import torch
    from deepsee_amd import lib as L, ops, resample as R
    from deepsee_amd.options import make_opt
    opt = make_opt(load_size=256, crop_size=256)
    g = torch.Generator().manual_seed(0)
    out = {}
    for name, shape, filt, hi in (("image 8 x 1024^2 x 3 -> 256^2 bicubic", (8, 1024, 1024, 3), R.BICUBIC, 256),
                                  ("label 8 x 512^2 -> 256^2 nearest", (8, 512, 512), R.NEAREST, 19)):
        src = torch.randint(0, hi, shape, generator=g, dtype=torch.uint8)
        c = 3 if len(shape) == 4 else 1
        geos = [R.load_geometry(opt, (shape[2], shape[1]), (0, 0)) for _ in range(8)]
        uni = on_device(R.batch_tables(geos, filt))
        buf, offsets = R.pack_arena(list(src.numpy()))
        host = R.ragged_tables(geos, filt, [(shape[2], shape[1], c)] * 8, offsets)
        rag, arena, dev = on_device(host), buf.cuda(), src.cuda()
        wo, ho = geos[0]["out"]
        tmp_rows, kx, ky = uni["tmp_rows"], uni["xtab"].shape[2] - 2, uni["ytab"].shape[2] - 2
        assert (rag["tmp_rows"], rag["xtab"].shape, rag["ytab"].shape) == (tmp_rows, uni["xtab"].shape, uni["ytab"].shape)
        tmp = torch.empty(8 * tmp_rows * wo * c, dtype=torch.uint8, device="cuda")
        dst = torch.empty(8 * ho * wo * c, dtype=torch.uint8, device="cuda")
        row = shape[2] * c
        # the entry points themselves on preallocated buffers (the same host work per call for both), and the ops wrappers, which
        # add the scratch lookup, the output allocation and, for the ragged one, the host asserts on the item table
        work = {"dsee_resample_u8": lambda: L.call("resample_u8", dev, tmp, dst, 8, c, 0, shape[1] * row, row, shape[2], shape[1],
                                                   wo, ho, tmp_rows, uni["xtab"], kx, uni["ytab"], ky, uni["rows"]),
                "dsee_resample_u8_ragged": lambda: L.call("resample_u8_ragged", arena, arena.numel(), rag["items"], tmp, dst, 8, c,
                                                          wo, ho, tmp_rows, rag["xtab"], kx, rag["ytab"], ky, rag["rows"]),
                "ops.resample_u8": lambda: ops.resample_u8(dev, uni, geos[0]["out"], geos[0]["box"]),
                "ops.resample_u8_ragged": lambda: ops.resample_u8_ragged(arena, host["items"], rag, geos[0]["out"], c)}
        assert torch.equal(work["ops.resample_u8"](), work["ops.resample_u8_ragged"]()), name
        work["dsee_resample_u8"]()
        first = dst.clone()
        dst.zero_()
        work["dsee_resample_u8_ragged"]()
        assert torch.equal(first, dst) and torch.equal(dst.view(-1), work["ops.resample_u8"]().view(-1)), name
        us = {k: [] for k in work}
        for r in range(rounds):
            for k in (list(work) if r % 2 == 0 else list(work)[::-1]):
                us[k].append(events(work[k], reps))
        out[name] = {k + " [us per call, HIP events over %d calls, %d alternating rounds]" % (reps, rounds): spread(v)
                     for k, v in us.items()}
        for pre in ("dsee_", "ops."):
            out[name]["%sresample_u8_ragged / %sresample_u8, medians" % (pre, pre)] = \
                float(np.median(us[pre + "resample_u8_ragged"]) / np.median(us[pre + "resample_u8"]))
    return out


def write_files(folder):
    from PIL import Image
    os.makedirs(os.path.join(folder, "lab"))
    os.makedirs(os.path.join(folder, "img"))
    rng = np.random.default_rng(0)
    for i, (w, h) in enumerate(MIXED_WH):
        yy, xx = np.mgrid[0:h, 0:w]          # smooth content + noise: a JPEG of pure noise decodes slower than a photograph
        base = np.stack([(np.sin(xx / (37.0 + 5 * c) + i) + np.cos(yy / (53.0 + 3 * c))) * 60 + 128 for c in range(3)], -1)
        img = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(folder, "img", "%03d.jpg" % i), quality=90)
        cells = rng.integers(0, 19, ((h // 2 + 31) // 32, (w // 2 + 31) // 32), dtype=np.uint8)
        lab = np.repeat(np.repeat(cells, 32, 0), 32, 1)[:h // 2, :w // 2]
        Image.fromarray(lab).save(os.path.join(folder, "lab", "%03d.png" % i))


def mixed_batch(rounds, reps):
    import torch
    from deepsee_amd import data as D, ops, resample as R
    from deepsee_amd.options import make_opt
    opt = make_opt(load_size=256, crop_size=256, start_size=32, batchSize=8)
    out = {"files (w, h)": [list(wh) for wh in MIXED_WH]}
    with tempfile.TemporaryDirectory() as folder:
        write_files(folder)
        dirs = (os.path.join(folder, "lab"), os.path.join(folder, "img"))
        for name, cls in (("FolderDataset (decode + PIL resize + crop)", D.FolderDataset), ("RawFolderDataset (decode only)", D.RawFolderDataset)):
            ds = cls(opt, *dirs)
            ds[0]                                                   # file cache, PIL's lazy imports
            ts = []
            for _ in range(3):
                for i in range(len(ds)):
                    t0 = time.perf_counter()
                    ds[i]
                    ts.append(time.perf_counter() - t0)
            out[name + " [ms per sample, host]"] = {"median": 1e3 * float(np.median(ts)), "mean": 1e3 * float(np.mean(ts)),
                                                    "min": 1e3 * min(ts), "max": 1e3 * max(ts)}
        ds = D.RawFolderDataset(opt, *dirs)
        samples = [ds[i] for i in range(8)]
    ld = D.DeviceLoader(ds, opt, shuffle=False)
    pos = [s["crop_pos"] for s in samples]
    kinds = {"image": ([s["image_raw"] for s in samples], R.BICUBIC, 3), "label": ([s["label_raw"] for s in samples], R.NEAREST, 1)}
    host_us = {"tables": [], "pack_arena": [], "collate (both arenas, pinned)": []}
    calls, upload = {}, 0
    for r in range(rounds * 3):
        t0 = time.perf_counter()
        built = {}
        for kind, (arrays, filt, c) in kinds.items():
            geos = [R.load_geometry(opt, (a.shape[1], a.shape[0]), p) for a, p in zip(arrays, pos)]
            built[kind] = (geos, R.ragged_tables(geos, filt, [(a.shape[1], a.shape[0], c) for a in arrays], [0] * 8))
        t1 = time.perf_counter()
        packed = {kind: R.pack_arena(arrays) for kind, (arrays, filt, c) in kinds.items()}
        t2 = time.perf_counter()
        ld.collate(samples)
        t3 = time.perf_counter()
        for k, v in zip(host_us, (t1 - t0, t2 - t1, t3 - t2)):
            host_us[k].append(1e6 * v)
    for kind, (arrays, filt, c) in kinds.items():
        buf, offsets = packed[kind]
        geos = built[kind][0]
        tab = R.ragged_tables(geos, filt, [(a.shape[1], a.shape[0], c) for a in arrays], offsets)
        upload += buf.numel() + sum(v.nbytes for v in tab.values() if isinstance(v, np.ndarray))
        dev, arena = on_device(tab), buf.cuda()
        calls[kind] = (lambda arena=arena, tab=tab, dev=dev, geos=geos, c=c: ops.resample_u8_ragged(arena, tab["items"], dev, geos[0]["out"], c))
        out["%s: tap rows kx, ky, tmp_rows" % kind] = [tab["xtab"].shape[2] - 2, tab["ytab"].shape[2] - 2, tab["tmp_rows"]]
    for kind, fn in calls.items():
        out["resample_u8_ragged, 8 mixed %s files -> 256^2 [us per call, HIP events over %d calls, %d rounds]" % (kind, reps, rounds)] = \
            spread([events(fn, reps) for _ in range(rounds)])
    out["upload per batch [bytes]: both arenas + their tables"] = int(upload)
    out["host per batch [us], %d repeats" % (rounds * 3)] = {k: spread(v) for k, v in host_us.items()}
    for v in out["host per batch [us], %d repeats" % (rounds * 3)].values():
        v.pop("rounds")
    host = ld.collate(samples)
    whole = []
    for r in range(rounds):
        for _ in range(3):
            D.device_preprocess(opt, host)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            D.device_preprocess(opt, host)
        torch.cuda.synchronize()
        whole.append(1e6 * (time.perf_counter() - t0) / 20)
    out["device_preprocess of the collated mixed batch: upload, tables, 2 ragged calls, normalise, labels, LR image "
        "[us per batch, host clock around a synchronise, 20 batches, %d rounds]" % rounds] = spread(whole)
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is measured on a CPU"
    res = {"device": torch.cuda.get_device_name(0), "uniform batch": uniform_batch(a.rounds, a.reps),
           "mixed batch": mixed_batch(a.rounds, a.reps)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
