"""Golden fixtures of the discriminator / style-encoder norms (opt.norm_D, opt.norm_E = spectral{batch,sync_batch,none}),
pinned against the real reference the way tools/gen_golden_instance.py pins the InstanceNorm generator, without editing the
oracle:

  * the oracle's D and E layers (Oracle._nlayer_d, Oracle._enc_layer and the `final` layer of Oracle.encoder_forward) are
    replaced by forms that follow get_nonspade_norm_layer (normalization.py:19-56): SN conv + InstanceNorm2d(affine=False),
    SN conv + BatchNorm2d(affine=True) through F.batch_norm (training flag, momentum 0.1, eps 1e-5, running buffers;
    num_batches_tracked += 1 for nn.BatchNorm2d only), or the SN conv alone with its bias;
  * deepsee_oracle.net_specs gets the reference's layouts of those layers ('<conv>.1.*' BatchNorm entries, or the conv one
    level up with a bias), recipe_tensor gives every BatchNorm weight 1 + 0.1 N(0,1) (no gamma near 0), and init_state
    draws it from N(1, init_variance) (base_network.py:28-35).

Then gen_golden.run_case drives reference and oracle on each case (inference, encode_only, demo, G+D steps, gradients,
post-step state incl. running statistics and num_batches_tracked) and writes the reference's numbers to
tests/golden/nonspade_norm/<case>.json.  Needs the reference sources (gen_golden.REF); the tests read only the fixtures.

    python tools/gen_golden_nonspade_norm.py            # all cases
    python tools/gen_golden_nonspade_norm.py case_name  # one case
"""
import argparse
import os
import re
import sys
import zlib
from collections import OrderedDict

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import deepsee_oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "nonspade_norm")

_SMALL = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)
CASES = {
    "indep_dbatch_ebatch_4to32_bs2_ngf8": dict(opt=dict(_SMALL, norm_D="spectralbatch", norm_E="spectralbatch"),
                                               n=2, seed=31, iters=1),
    "indep_dsync_enone_4to32_bs2_ngf8": dict(opt=dict(_SMALL, norm_D="spectralsync_batch", norm_E="spectralnone"),
                                             n=2, seed=32, iters=1),
    "guided_dnone_esync_4to32_bs2_ngf8": dict(opt=dict(_SMALL, netE="fullstyle", noisy_style_scale=0.05,
                                                       guiding_style_image=True, norm_D="spectralnone",
                                                       norm_E="spectralsync_batch"), n=2, seed=33, iters=1),
    # running statistics and num_batches_tracked move twice per iteration (G step and D step), over two iterations
    "indep_dbatch_two_iters_4to32_ngf8": dict(opt=dict(_SMALL, norm_D="spectralbatch"), n=2, seed=34, iters=2),
}


def norm_of(norm_type):
    """get_nonspade_norm_layer's subtype (normalization.py:27-49), exact comparison."""
    if not norm_type.startswith("spectral"):
        raise ValueError(norm_type)
    sub = norm_type[len("spectral"):]
    if sub in ("", "none"):
        return "none"
    if sub not in ("instance", "batch", "sync_batch"):
        raise ValueError("normalization layer %s is not recognized" % sub)
    return sub


def layout(path, norm):
    """(conv path, BatchNorm path or None) of the layer whose conv sits at `path` under a normed layout."""
    parent = path.rsplit(".", 1)[0]
    return (parent if norm == "none" else path), (parent + ".1" if norm in ("batch", "sync_batch") else None)


def norm_act(orc, st, path, norm, x, stride, padding, act):
    cp, bp = layout(path, norm)
    w = O.spectral_weight(st, cp, orc.training)
    x = F.conv2d(x, w, st[cp + ".bias"] if norm == "none" else None, stride=stride, padding=padding)
    if norm == "instance":
        x = O.instance_norm(x)
    elif norm in ("batch", "sync_batch"):
        x = F.batch_norm(x, st[bp + ".running_mean"], st[bp + ".running_var"], st[bp + ".weight"], st[bp + ".bias"],
                         orc.training, O.BN_MOMENTUM, O.BN_EPS)
        if orc.training and norm == "batch":
            with torch.no_grad():
                st[bp + ".num_batches_tracked"].add_(1)
    return act(x)


def _respec(spec, norm):
    """The D / E state layout of `norm` from the InstanceNorm layout (every spectral-norm conv there is a norm layer)."""
    out = OrderedDict()
    for k, shape in spec.items():
        m = re.match(r"(.*)\.(weight_orig|weight_u|weight_v)$", k)
        if m is None:
            out[k] = shape
            continue
        cp, bp = layout(m.group(1), norm)
        if m.group(2) == "weight_orig" and norm == "none":
            out[cp + ".bias"] = (shape[0],)
        out[cp + "." + m.group(2)] = shape
        if m.group(2) == "weight_v" and bp is not None:
            c = spec[m.group(1) + ".weight_u"][0]
            for leaf in ("weight", "bias", "running_mean", "running_var"):
                out[bp + "." + leaf] = (c,)
            out[bp + ".num_batches_tracked"] = ()
    return out


def _is_bn_weight(net, key, shape):
    return net in ("D", "E") and len(tuple(shape)) == 1 and key.endswith(".1.weight")


def install_nonspade_norm(setattr_=setattr):
    """Substitute the oracle's D / E layers, state layout and initial values (setattr_: pytest's monkeypatch.setattr)."""
    specs, recipe, init = O.net_specs, O.recipe_tensor, O.init_state

    def net_specs(opt):
        out = specs(opt)
        out["D"] = _respec(out["D"], norm_of(opt.norm_D))
        out["E"] = _respec(out["E"], norm_of(opt.norm_E))
        return out

    def recipe_tensor(net, key, shape, gain=1.0):
        if _is_bn_weight(net, key, shape):
            g = torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (net, key)).encode()) & 0x7FFFFFFF)
            return 1.0 + 0.1 * torch.randn(tuple(shape), generator=g)
        return recipe(net, key, shape, gain)

    def init_state(opt, seed=0):
        out = init(opt, seed)
        g = torch.Generator().manual_seed(seed + 1)
        for net in ("D", "E"):
            for k, v in out[net].items():
                if _is_bn_weight(net, k, v.shape):
                    out[net][k] = 1.0 + opt.init_variance * torch.randn(v.shape, generator=g)
        return out

    def _nlayer_d(self, st, p, x):
        norm = norm_of(self.opt.norm_D)
        outs = []
        x = O.lrelu(F.conv2d(x, st[p + ".model0.0.weight"], st[p + ".model0.0.bias"], stride=2, padding=2))
        outs.append(x)
        nl = self.opt.n_layers_D
        for n in range(1, nl):
            x = norm_act(self, st, "%s.model%d.0.0" % (p, n), norm, x, 1 if n == nl - 1 else 2, 2, O.lrelu)
            outs.append(x)
        q = "%s.model%d.0" % (p, nl)
        outs.append(F.conv2d(x, st[q + ".weight"], st[q + ".bias"], stride=1, padding=2))
        return outs

    def _enc_layer(self, st, p, x, stride):
        return norm_act(self, st, p, norm_of(self.opt.norm_E), x, stride, 1, O.lrelu)

    def encoder_forward(self, x, seg, mode, no_noise):
        st = self.S["E"]
        combined = self.opt.netE == "combinedstyle"
        prefix = ("encoder_full." if mode == "full" else "encoder_mini.") if combined else ""
        x = self._enc_main(st, prefix, mode, x)
        x = norm_act(self, st, "final.0.0", norm_of(self.opt.norm_E), x, 1, 1, torch.tanh)
        sm = O.style_pool(x, seg)
        if self.opt.noisy_style_scale > 0 and not no_noise:
            nw = torch.sigmoid(st["noise_weights"])[None, :, None]
            if self.opt.noisy_style_dist == "uniform":
                noise = (self.ctl.uniform(tuple(sm.shape), "style_noise") * 2 - 1) * self.opt.noisy_style_scale
            else:
                noise = (self.ctl.normal(tuple(sm.shape), "style_noise") * 2 - 1) * self.opt.noisy_style_scale
            sm = (sm + noise * nw).clamp(-1, 1)
        return sm

    setattr_(O, "net_specs", net_specs)
    setattr_(O, "recipe_tensor", recipe_tensor)
    setattr_(O, "init_state", init_state)
    setattr_(O.Oracle, "_nlayer_d", _nlayer_d)
    setattr_(O.Oracle, "_enc_layer", _enc_layer)
    setattr_(O.Oracle, "encoder_forward", encoder_forward)


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
    for name, spec in CASES.items():
        if a.cases and name not in a.cases:
            continue
        G.run_case(name, spec)
        os.makedirs(OUT, exist_ok=True)
        os.replace(os.path.join(ROOT, "tests", "golden", name + ".json"), os.path.join(OUT, name + ".json"))


if __name__ == "__main__":
    main()
