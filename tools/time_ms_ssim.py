"""dsee_ms_ssim on one MI355X (profiles/ms_ssim.md): the time of one call on a batch of N = 8 images at 256 x 256 and
512 x 512, next to
  * the float64 restatement the tests keep (tests/test_ms_ssim_host.py: msssim64), run with torch operators on the device,
    sample by sample as the reference's collect_samples loop does (and once more in fp32, the reference's own precision);
  * dsee_psnr_ssim on the same batch, the metric kernel pair already in the tree.

    python tools/time_ms_ssim.py [--n 8] [--sizes 256 512] [--warmup 5] [--calls 30]

Every figure is the median over `calls` timed calls after `warmup` untimed ones, each call bracketed by device events on the
one stream everything runs on (the workspace and the output are allocated outside the timed region).  Before timing, the
kernel's values are compared with the restatement's (on the CPU) on the same images; more than 1e-9 apart fails.
Prints one JSON line per size."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, calls):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    a = ap.parse_args()
    assert a.calls >= 20
    import torch
    from deepsee_amd import lib as L
    from deepsee_amd import ops
    from tools.gen_golden_ms_ssim import host_test_module, images
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    msssim64 = host_test_module().msssim64
    for size in a.sizes:
        fake, real = images(dict(H=size, W=size, N=a.n, kind="noise0.1", seed=7))
        fake, real = fake.cuda(), real.cuda()
        f, r = ops.to_nhwc(fake), ops.to_nhwc(real)
        n, h, w, cs = f.shape
        ws = torch.empty(L.lib().dsee_ms_ssim_workspace(n, h, w) // 8, dtype=torch.float64, device="cuda")
        out = torch.empty(n, 11, dtype=torch.float64, device="cuda")
        ws2 = torch.empty(L.lib().dsee_psnr_ssim_workspace(n, h, w) // 8, dtype=torch.float64, device="cuda")
        out2 = torch.empty(n, 3, dtype=torch.float64, device="cuda")

        def kernel():
            L.call("ms_ssim", f, r, n, h, w, cs, ws, ws.numel() * 8, out)

        def yardstick():
            L.call("psnr_ssim", f, r, n, h, w, cs, ws2, ws2.numel() * 8, out2)

        def restated(dtype):
            return [msssim64(fake[i], real[i], dtype)[0] for i in range(n)]      # (float(): one device sync per sample)

        def timed_or_error(fn):
            try:
                return timed(fn, a.warmup, a.calls)
            except RuntimeError as e:          # (an operator the device build of torch lacks in that type: reported, not hidden)
                return {"error": str(e).splitlines()[0][:200]}

        kernel()
        got = out[:, 0].cpu()
        want = [msssim64(fake[i].cpu(), real[i].cpu())[0] for i in range(n)]
        gap = max(abs(float(g) - v) for g, v in zip(got, want))
        rec = {"n": n, "size": size, "max_abs_kernel_vs_float64_restatement_on_cpu": gap,
               "workspace_mib": round(ws.numel() * 8 / 2 ** 20, 1),
               "dsee_ms_ssim": timed(kernel, a.warmup, a.calls),
               "dsee_psnr_ssim": timed(yardstick, a.warmup, a.calls),
               "torch_float64": timed_or_error(lambda: restated(torch.float64)),
               "torch_float32": timed_or_error(lambda: restated(torch.float32)),
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        assert gap <= 1e-9, gap


if __name__ == "__main__":
    main()
