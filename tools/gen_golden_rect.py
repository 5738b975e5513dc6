"""Golden fixtures of non-square (H != W) batches through SRModel, pinned against the real reference the way
tools/gen_golden_random_style.py pins opt.random_style_matrix, without editing the oracle or the reference:

  * O.synthetic_batch is wrapped: with opt.aspect_ratio != 1 the batch is W = crop_size wide and H = round(crop_size /
    aspect_ratio) high (what preprocess_mode='fixed' loads, data/base_dataset.py), its label maps a 4 x 4 grid of cells
    nearest-upsampled to H x W, its images uniform in [-1, 1]; the draws come from the same seeded generator in the same order
    (label, image, guiding label, guiding image).
  * O.Oracle.preprocess is wrapped: the LR image is F.interpolate(img, lr_shape, 'bicubic').clamp(-1, 1) with
    lr_shape = deepsee_amd.ops.lr_shape(opt, H, W) = (H / f, W / f), f = crop_size / start_size.
  * the reference's Preprocessor.downsample_image is wrapped where the reference is loaded (main() below; the tests never load
    it): its `shape` parameter defaults to the same (H / f, W / f) instead of a start_size square.

With aspect_ratio == 1 the three wrappers hand on to what they wrap.  Then gen_golden.run_case drives reference and oracle on each
case (inference, encode_only, demo, G+D step, gradients, post-step state), keeps its own oracle-vs-reference assertions as the
acceptance of a seed, and writes the REFERENCE's numbers to tests/golden/rect/<case>.json.  Seeds: 3, 4 and 8 pass every
assertion; 5, 6 and 7 of the guided case trip run_case's kink-flip checks (a post-step D bias at 2.7e-3 ... 3.8e-3 against 1e-3,
one gradient at 5.5e-3 against 5e-3) -- the situation tools/gen_golden_random_style.py documents for its own seeds.

    python tools/gen_golden_rect.py            # all cases
    python tools/gen_golden_rect.py case_name  # one case
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import deepsee_oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rect")
CELLS = 4

_SMALL = dict(batchSize=2, ngf=8)
CASES = {
    # 5 x 4 -> 40 x 32: the 10 x 8 level is off the Winograd tile grid
    "indep_5x4_to_40x32": dict(opt=dict(_SMALL, start_size=4, crop_size=32, aspect_ratio=0.8), n=2, seed=3, iters=1),
    # 4 x 8 -> 32 x 64: wider than high
    "indep_4x8_to_32x64": dict(opt=dict(_SMALL, start_size=8, crop_size=64, aspect_ratio=2.0), n=2, seed=4, iters=1),
    # 8 x 4 -> 64 x 32, guided: the full encoder on a non-square guiding image
    "guided_8x4_to_64x32": dict(opt=dict(_SMALL, start_size=4, crop_size=32, aspect_ratio=0.5, netE="fullstyle",
                                         noisy_style_scale=0.05, guiding_style_image=True), n=2, seed=8, iters=1),
}


def hr_shape(opt):
    """(H, W) of a batch of preprocess_mode='fixed': W = crop_size, H = round(crop_size / aspect_ratio)."""
    return int(round(opt.crop_size / opt.aspect_ratio)), int(opt.crop_size)


def lr_shape(opt, h, w):
    from deepsee_amd.ops import lr_shape as rule      # (pure host arithmetic: no device, no library)
    return rule(opt, h, w)


def install_rect(setattr_=setattr):
    """Substitute the oracle's batch and LR image -- and, where it is loaded, the reference's LR default -- for
    opt.aspect_ratio != 1 (setattr_: pytest's monkeypatch.setattr)."""
    synthetic_batch, preprocess = O.synthetic_batch, O.Oracle.preprocess

    def synthetic_batch_rect(opt, n, seed=1234, guided=None):
        if getattr(opt, "aspect_ratio", 1.0) == 1.0:
            return synthetic_batch(opt, n, seed=seed, guided=guided)
        g = torch.Generator().manual_seed(seed)
        h, w = hr_shape(opt)

        def lab():
            c = torch.randint(0, opt.semantic_nc, (n, 1, CELLS, CELLS), generator=g).float()
            return F.interpolate(c, size=(h, w), mode="nearest")

        batch = {"label": lab(), "image": torch.rand(n, 3, h, w, generator=g) * 2 - 1}
        if guided if guided is not None else opt.guiding_style_image:
            batch["guiding_label"] = lab()
            batch["guiding_image"] = torch.rand(n, 3, h, w, generator=g) * 2 - 1
        return batch

    def preprocess_rect(self, batch):
        out = preprocess(self, batch)
        img = out["image_hr"]
        shape = lr_shape(self.opt, img.shape[2], img.shape[3])
        if shape != (self.opt.start_size, self.opt.start_size):
            out["image_lr"] = F.interpolate(img, shape, mode="bicubic").clamp(-1, 1)
        return out

    setattr_(O, "synthetic_batch", synthetic_batch_rect)
    setattr_(O.Oracle, "preprocess", preprocess_rect)
    ref = sys.modules.get("data.preprocessor")
    if ref is not None and hasattr(ref, "Preprocessor"):
        downsample_image = ref.Preprocessor.downsample_image

        def downsample_image_rect(self, hr_image, shape=None):
            if shape is None:
                shape = lr_shape(self.opt, hr_image.shape[2], hr_image.shape[3])
            return downsample_image(self, hr_image, shape)

        setattr_(ref.Preprocessor, "downsample_image", downsample_image_rect)


def main():
    from oracle import gen_golden as G
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    assert os.path.isdir(G.REF), "needs the reference sources (%s)" % G.REF
    G.install_torchvision_stub()
    sys.path.insert(0, G.REF)
    torch.set_num_threads(8)
    import data.preprocessor  # noqa: F401  (the reference's: install_rect wraps its downsample_image)
    install_rect()
    for name, spec in CASES.items():
        if a.cases and name not in a.cases:
            continue
        G.run_case(name, spec)
        os.makedirs(OUT, exist_ok=True)
        os.replace(os.path.join(ROOT, "tests", "golden", name + ".json"), os.path.join(OUT, name + ".json"))


if __name__ == "__main__":
    main()
