"""Evaluation metrics on the device: PSNR / SSIM / MS-SSIM / RMSE of generated against ground-truth images.

Mirror of the reference's ``MetricsEvaluator`` (evaluator/evaluation.py:15-158) for the four metrics that need no
pretrained network: ``collect_samples(fake, real, name)`` scores one batch, ``get_result()`` returns the same
``"psnr/mean" ... "n_samples"`` OrderedDict, ``write_details`` appends one CSV row per sample.  The reference loops over
the samples on the CPU (tensor2im -> numpy uint8 -> cv2.filter2D in float64); here one kernel pair
(``dsee_psnr_ssim``) scores the whole batch from the fp32 tensors where they are, and 3 doubles per image come back.
MS-SSIM (evaluator/ssim.py:88-118: five Gaussian-window SSIM passes over an average-pooled pyramid, no weights) is
``dsee_ms_ssim`` on the same tensors; ``MetricsEvaluator(ms_ssim=True)`` adds its column and keys, the default evaluator is
as before.  LPIPS and FID (pretrained AlexNet / Inception weights, downloads in the reference) are out of scope: their columns
are absent from ``columns`` and from ``get_result()``.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import lib as L
from . import ops


def _native_pair(fake, real):
    def native(t):
        if getattr(t, "dsee_layout", None) == "nhwc":
            return t.detach().contiguous()
        assert t.dim() == 4 and t.shape[1] == 3, "NCHW [N,3,H,W] or a tagged native NHWC tensor expected"
        return ops.to_nhwc(t.detach().float().cuda())
    f, r = native(fake), native(real)
    assert f.shape == r.shape, "fake and real differ in shape"
    return f, r


def _psnr_ssim_rmse_device(f, r):
    n, h, w, cs = f.shape
    ws = torch.empty(L.lib().dsee_psnr_ssim_workspace(n, h, w) // 8, dtype=torch.float64, device=f.device)
    out = torch.empty(n, 3, dtype=torch.float64, device=f.device)
    L.call("psnr_ssim", f, r, n, h, w, cs, ws, ws.numel() * 8, out)
    return out


def _ms_ssim_device(f, r):
    n, h, w, cs = f.shape
    # (H or W < 16: the workspace size is 0 and the entry point's own argument check raises, before it launches anything)
    ws = torch.empty(max(1, L.lib().dsee_ms_ssim_workspace(n, h, w) // 8), dtype=torch.float64, device=f.device)
    out = torch.empty(n, 11, dtype=torch.float64, device=f.device)
    L.call("ms_ssim", f, r, n, h, w, cs, ws, ws.numel() * 8, out)
    return out


def psnr_ssim_rmse(fake, real):
    """fake, real: images in [-1, 1]; native NHWC fp32 [N,H,W,>=3] device tensors, or the reference's NCHW [N,3,H,W]
    (any device).  Returns a float64 tensor [N, 3] = (psnr, ssim, rmse) per image on the CPU."""
    return _psnr_ssim_rmse_device(*_native_pair(fake, real)).cpu()


def ms_ssim(fake, real, detail=False):
    """MS-SSIM per image as the reference's collect_samples computes it: msssim(fake255, real255, size_average=True,
    val_range=255) on (x + 1) * 127.5, neither quantised nor clipped (evaluation.py:114,125-127, ssim.py:88-118), in float64.
    Same inputs as psnr_ssim_rmse; H, W >= 16 (the reference raises below 32, on a sixth pooling whose result it never uses).
    Returns a float64 CPU tensor [N]; with detail=True [N, 11] = the value,
    cs_0..cs_4, sim_0..sim_4 (the per-level terms).  As in the reference the value is prod_{l<4}(cs_l^w_l * sim_4^w_4) --
    ssim.py:117 multiplies every cs factor by the last level's term -- and is NaN when cs_0..cs_3 or sim_4 is negative
    (structurally unrelated images): a validation CSV shows what the reference's shows."""
    out = _ms_ssim_device(*_native_pair(fake, real)).cpu()
    return out if detail else out[:, 0].clone()


class MetricsEvaluator:
    """Collects per-sample scores; optionally writes them to ``folder_out/metrics.csv`` (evaluation.py:15-158)."""
    columns = ["ID", "PSNR", "SSIM", "RMSE"]

    def __init__(self, write_details=False, folder_out=None, extra_columns=(), extra_columns_content=(), append=False,
                 ms_ssim=False):
        """ms_ssim=True adds the reference's MSSSIM column (after SSIM, as in its metrics.csv) and the "ms_ssim/mean" /
        "ms_ssim/std" keys (in the reference's order); the default is the three-metric evaluator."""
        assert len(extra_columns) == len(extra_columns_content), "Extra columns and content need to be of the same size"
        self.ms_ssim = bool(ms_ssim)
        if self.ms_ssim:
            self.columns = ["ID", "PSNR", "SSIM", "MSSSIM", "RMSE"]
        self.clear()
        self.write_details = write_details
        self.writer = None
        if write_details:
            self.writer = MetricsWriter(folder_out, self.columns, extra_columns, extra_columns_content, append)

    def clear(self):
        self.psnr_buffer, self.ssim_buffer, self.rmse_buffer, self.n_samples = [], [], [], 0
        self.ms_ssim_buffer = []

    @staticmethod
    def _get_id_from_path(path):
        return os.path.basename(path)[:-4]

    def collect_samples(self, fake, real, name=None):
        assert fake.shape[0] == real.shape[0]
        f, r = _native_pair(fake, real)
        scores = _psnr_ssim_rmse_device(f, r)
        ms = _ms_ssim_device(f, r)[:, 0].cpu().numpy() if self.ms_ssim else None      # one call each; one batch, on the device
        scores = scores.cpu().numpy()
        for i in range(scores.shape[0]):
            psnr, ssim, rmse = (float(v) for v in scores[i])
            self.psnr_buffer.append(psnr)
            self.ssim_buffer.append(ssim)
            self.rmse_buffer.append(rmse)
            if self.ms_ssim:
                self.ms_ssim_buffer.append(float(ms[i]))
            if self.write_details:
                row = [psnr, ssim, float(ms[i]), rmse] if self.ms_ssim else [psnr, ssim, rmse]
                self.writer.append_line([self._get_id_from_path(name[i])] + row)
        self.n_samples += scores.shape[0]

    def get_result(self):
        if self.ms_ssim:
            return OrderedDict([("psnr/mean", np.mean(self.psnr_buffer)), ("ssim/mean", np.mean(self.ssim_buffer)),
                                ("ms_ssim/mean", np.mean(self.ms_ssim_buffer)), ("rmse/mean", np.mean(self.rmse_buffer)),
                                ("psnr/std", np.std(self.psnr_buffer)), ("ssim/std", np.std(self.ssim_buffer)),
                                ("ms_ssim/std", np.std(self.ms_ssim_buffer)), ("rmse/std", np.std(self.rmse_buffer)),
                                ("n_samples", self.n_samples)])
        return OrderedDict([("psnr/mean", np.mean(self.psnr_buffer)), ("ssim/mean", np.mean(self.ssim_buffer)),
                            ("rmse/mean", np.mean(self.rmse_buffer)), ("psnr/std", np.std(self.psnr_buffer)),
                            ("ssim/std", np.std(self.ssim_buffer)), ("rmse/std", np.std(self.rmse_buffer)),
                            ("n_samples", self.n_samples)])


class MetricsWriter:
    """``metrics.csv`` with a header row and optional constant extra columns (evaluation.py:161-200)."""

    def __init__(self, path, metrics, extra_columns=(), extra_columns_content=(), append=False):
        self.path_out = os.path.join(path, "metrics.csv")
        header = list(extra_columns) + list(metrics)
        self.extra_columns_content = list(extra_columns_content)
        new_file = not (append and os.path.exists(self.path_out))
        self.file = open(self.path_out, "a" if append else "w")
        if new_file:
            self.append_line(header, add_extra_content=False)

    def append_line(self, row, add_extra_content=True):
        content = (self.extra_columns_content if add_extra_content else []) + list(row)
        self.file.write(",".join(map(str, content)) + os.linesep)
        self.file.flush()

    def __del__(self):
        if getattr(self, "file", None):
            self.file.close()
