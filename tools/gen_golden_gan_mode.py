"""Golden fixtures of the GAN objective (opt.gan_mode = ls / original / w / hinge), pinned against the real reference the way
tools/gen_golden_nonspade_norm.py pins the discriminator norms, without editing the oracle:

  * the oracle's hinge term (Oracle.hinge, used by generator_losses and discriminator_losses) is replaced by a restatement
    of GANLoss (loss.py:31-99) keyed on opt.gan_mode: per discriminator scale the mean over every element of its last
    output of
        hinge     G: -x                 D real: -min(x-1, 0)   D fake: -min(-x-1, 0)
        w         G / D real: -x        D fake: x
        ls        target t: (x-t)^2
        original  target t: binary cross-entropy on logits, softplus(-x) for t = 1 and softplus(x) for t = 0
    with the real label t = 1 and the fake label t = 0, then the mean over the scales.  Any other gan_mode raises
    ValueError as GANLoss does.

The D norms go through tools/gen_golden_nonspade_norm.install_nonspade_norm as well (its instance form is the oracle's), so
a case may set norm_D.  Then gen_golden.run_case drives reference and oracle on each case (inference, encode_only, demo, G+D
steps, gradients, post-step state) and writes the reference's numbers to tests/golden/gan_mode/<case>.json.  Needs the
reference sources (gen_golden.REF); the tests read only the fixtures.

    python tools/gen_golden_gan_mode.py            # all cases
    python tools/gen_golden_gan_mode.py case_name  # one case
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import deepsee_oracle as O  # noqa: E402
from tools.gen_golden_nonspade_norm import install_nonspade_norm  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gan_mode")

_SMALL = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)
# (seeds where no near-zero gradient element of the first step flips the sign of its beta1 = 0 Adam update between reference
#  and oracle: such a flip exceeds run_case's post-step state bound of 1e-3 on its own, whatever the GAN mode)
CASES = {
    "indep_ls_4to32_bs2_ngf8": dict(opt=dict(_SMALL, gan_mode="ls"), n=2, seed=60, iters=1),
    "guided_original_4to32_bs2_ngf8": dict(opt=dict(_SMALL, gan_mode="original", netE="fullstyle",
                                                    noisy_style_scale=0.05, guiding_style_image=True), n=2, seed=42,
                                           iters=1),
    "indep_w_4to32_bs2_ngf8": dict(opt=dict(_SMALL, gan_mode="w"), n=2, seed=49, iters=1),
    # batch statistics in D: the generator step's D pass runs over cat([fake; real])
    "indep_ls_dbatch_4to32_bs2_ngf8": dict(opt=dict(_SMALL, gan_mode="ls", norm_D="spectralbatch"), n=2, seed=44,
                                           iters=1),
    "indep_original_two_iters_4to32_ngf8": dict(opt=dict(_SMALL, gan_mode="original"), n=2, seed=56, iters=2),
}

GAN_MODES = ("ls", "original", "w", "hinge")


def gan_term(gan_mode, x, target_is_real, for_d):
    """The loss of one discriminator scale's last output x (a scalar tensor)."""
    if gan_mode not in GAN_MODES:
        raise ValueError("Unexpected gan_mode {}".format(gan_mode))
    if gan_mode == "hinge":
        if for_d:
            mv = torch.min((x - 1) if target_is_real else (-x - 1), torch.zeros(1, dtype=x.dtype))
            return -mv.mean()
        return -x.mean()
    if gan_mode == "w":
        return -x.mean() if target_is_real else x.mean()
    if gan_mode == "ls":
        return (x - (1.0 if target_is_real else 0.0)).square().mean()
    return F.softplus(-x if target_is_real else x).mean()


def install_gan_mode(setattr_=setattr):
    """Substitute the oracle's GAN term by gan_term(opt.gan_mode) (setattr_: pytest's monkeypatch.setattr).  Oracle.hinge
    becomes an instance method: generator_losses / discriminator_losses call it as self.hinge(preds, target_is_real,
    for_d)."""

    def hinge(self, preds, target_is_real, for_d):
        total = 0
        for p in preds:
            total = total + gan_term(self.opt.gan_mode, p[-1], target_is_real, for_d).view(1)
        return total / len(preds)

    setattr_(O.Oracle, "hinge", hinge)


def main():
    from oracle import gen_golden as G
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    assert os.path.isdir(G.REF), "needs the reference sources (%s)" % G.REF
    G.install_torchvision_stub()
    sys.path.insert(0, G.REF)
    torch.set_num_threads(8)
    install_nonspade_norm()
    install_gan_mode()
    for name, spec in CASES.items():
        if a.cases and name not in a.cases:
            continue
        G.run_case(name, spec)
        os.makedirs(OUT, exist_ok=True)
        os.replace(os.path.join(ROOT, "tests", "golden", name + ".json"), os.path.join(OUT, name + ".json"))


if __name__ == "__main__":
    main()
