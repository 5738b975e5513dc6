"""Golden fixtures of opt.random_style_matrix (FullStyleEncoder fed label-masked noise instead of the style image), pinned
against the real reference the way tools/gen_golden_gan_mode.py pins the GAN objectives, without editing the oracle:

  * Oracle.encoder_forward is wrapped: with opt.random_style_matrix its input x is replaced by
        ctl.normal((N, label_nc, crop_size, crop_size), "style_field") * seg
    before the original body runs (encoder.py:116-120: torch.randn(...) * seg, in training and in eval), so the draw is the
    first one of the encoder -- ahead of the style-matrix corruption noise -- and lands on a recorded tape under the tag
    "style_field".  The oracle already sizes initial.0.0 for label_nc input channels (e_spec).  Any netE other than
    'fullstyle' is refused: CombinedstyleEncoder.forward calls encoder_full.forward_main(x) directly (encoder.py:197-198), so the
    replacement never runs there and the RGB image meets a label_nc-channel convolution.
  * Oracle.encode_only is wrapped to seed torch's generator with ENCODE_ONLY_SEED first.  gen_golden.run_case seeds once and
    then runs the reference's and the oracle's `encode_only` back to back; with a draw inside the encoder the two would see
    different fields.  main() wraps the reference's SRModel.forward the same way for mode == 'encode_only'.

Then gen_golden.run_case drives reference and oracle on each case (inference, encode_only, demo, G+D step, gradients, post-step
state) and writes the reference's numbers to tests/golden/random_style/<case>.json.  Needs the reference sources
(gen_golden.REF); the tests read only the fixtures.

    python tools/gen_golden_random_style.py            # all cases
    python tools/gen_golden_random_style.py case_name  # one case
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import deepsee_oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "random_style")
ENCODE_ONLY_SEED = 7411

_SMALL = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)
_GUIDED = dict(_SMALL, netE="fullstyle", noisy_style_scale=0.05, random_style_matrix=True)
# (seeds where no near-kink element of the first step moves an alpha_beta / alpha_gamma scalar's gradient past run_case's 5e-3
#  between reference and oracle: 91 and 95 do, at 5.4e-3 / 6.2e-3, whatever the encoder's input)
CASES = {
    # the style labels are the guiding image's label map
    "guided_random_guide_4to32_bs2_ngf8": dict(opt=dict(_GUIDED, guiding_style_image=True), n=2, seed=92, iters=1),
    # ... and the input's own label map
    "guided_random_4to32_bs2_ngf8": dict(opt=dict(_GUIDED), n=2, seed=93, iters=1),
}


def install_random_style(setattr_=setattr):
    """Substitute the oracle's encoder input and pin encode_only's draw (setattr_: pytest's monkeypatch.setattr)."""
    encoder_forward, encode_only = O.Oracle.encoder_forward, O.Oracle.encode_only

    def encoder_forward_random(self, x, seg, mode, no_noise):
        if getattr(self.opt, "random_style_matrix", False):
            if self.opt.netE != "fullstyle":
                raise ValueError("random_style_matrix needs netE='fullstyle', got netE=%r: CombinedstyleEncoder.forward runs "
                                 "encoder_full.forward_main(x) on the image itself (encoder.py:197-198)" % (self.opt.netE,))
            crop = self.opt.crop_size
            x = self.ctl.normal((seg.shape[0], seg.shape[1], crop, crop), "style_field").to(seg.dtype) * seg
        return encoder_forward(self, x, seg, mode, no_noise)

    def encode_only_seeded(self, batch):
        if getattr(self.opt, "random_style_matrix", False):
            torch.manual_seed(ENCODE_ONLY_SEED)
        return encode_only(self, batch)

    setattr_(O.Oracle, "encoder_forward", encoder_forward_random)
    setattr_(O.Oracle, "encode_only", encode_only_seeded)


def main():
    from oracle import gen_golden as G
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    assert os.path.isdir(G.REF), "needs the reference sources (%s)" % G.REF
    G.install_torchvision_stub()
    sys.path.insert(0, G.REF)
    torch.set_num_threads(8)
    install_random_style()
    from deepsee_models.sr_model import SRModel
    forward = SRModel.forward

    def forward_seeded(self, data, mode, *args, **kw):
        if mode == "encode_only" and self.opt.random_style_matrix:
            torch.manual_seed(ENCODE_ONLY_SEED)
        return forward(self, data, mode, *args, **kw)

    SRModel.forward = forward_seeded
    for name, spec in CASES.items():
        if a.cases and name not in a.cases:
            continue
        G.run_case(name, spec)
        os.makedirs(OUT, exist_ok=True)
        os.replace(os.path.join(ROOT, "tests", "golden", name + ".json"), os.path.join(OUT, name + ".json"))


if __name__ == "__main__":
    main()
