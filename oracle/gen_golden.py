"""Pin the oracle against the real reference and write golden fixtures.

Runs ONLY in the build container (needs /root/reference, which never travels to
the GPU box).  It imports the reference's TrainerManager (with a stub
``torchvision`` — absent in this image), loads identical recipe
weights into the reference networks and into ``oracle/deepsee_oracle.py``,
drives both with the same seeds, asserts agreement, and writes the reference's
numbers (NOT the oracle's) to ``tests/golden/<case>.json``.

    python oracle/gen_golden.py            # all cases
    python oracle/gen_golden.py case_name  # one case
"""
import argparse
import json
import os
import random
import sys
import types

import numpy as np

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
REF = "/root/reference"
GRAD_TOL_G = 5e-3
GRAD_TOL_D = 5e-2

from oracle import deepsee_oracle as O  # noqa: E402

CASES = {
    # BASELINE config 1: independent 8x (4->32), bs=2, full width
    "indep_4to32_bs2": dict(opt=dict(start_size=4, crop_size=32, load_size=32, batchSize=2), n=2, seed=11, iters=1),
    # stricter regime: O(1) activations, 3 resolutions, narrower net for CPU time
    "indep_8to64_bs2_ngf8": dict(opt=dict(start_size=8, crop_size=64, load_size=64, batchSize=2, ngf=8), n=2,
                                 seed=12, iters=1),
    # guided variant (full encoder on guiding image/label, noise scale .05)
    "guided_4to32_bs2_ngf8": dict(opt=dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8,
                                            netE="fullstyle", noisy_style_scale=0.05, guiding_style_image=True),
                                  n=2, seed=13, iters=1),
    # the other corruption distribution of encoder.py:59-66 ('normal': (randn * 2 - 1) * scale)
    "guided_normal_4to32_bs2_ngf8": dict(opt=dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8,
                                                   netE="fullstyle", noisy_style_scale=0.05, noisy_style_dist="normal",
                                                   guiding_style_image=True), n=2, seed=17, iters=1),
    # two full iterations: double BN/SN update per iteration + Adam
    "indep_4to32_two_iters_ngf8": dict(opt=dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8),
                                       n=2, seed=14, iters=2),
    # PureSEAN tail + max_fm_size bug path (config-5 topology, shrunk): n_blocks=5, load_size>=512
    "puresean_4to128_bs2_ngf4": dict(opt=dict(start_size=4, crop_size=128, load_size=512, batchSize=2, ngf=4,
                                              add_noise=False, max_fm_size=64), n=2, seed=15, iters=1),
    # no-noise, no-TTUR, gradient clipping on
    "indep_clip_4to32_ngf8": dict(opt=dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8,
                                           add_noise=False, no_TTUR=True, gradient_clip=0.01), n=2, seed=16, iters=1),
    # class counts other than 19: a dontcare label (semantic_nc = label_nc + 1 = 20 one-hot channels, the synthetic batch draws
    # from [0, label_nc] inclusive; options/base_options.py:231-234, data/preprocessor.py:37-38) and a small label_nc.
    # noisy_style_scale = 0: with the style corruption on, the reference indexes its label_nc noise weights with the semantic_nc
    # rows of the style matrix (encoder.py:54-56) and raises IndexError in the first forward pass.
    "dontcare_4to32_bs2_ngf8": dict(opt=dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8,
                                             contain_dontcare_label=True, noisy_style_scale=0.0), n=2, seed=18, iters=1),
    "label5_4to32_bs2_ngf8": dict(opt=dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8, label_nc=5),
                                  n=2, seed=19, iters=1),
}


def install_torchvision_stub():
    import torch.nn as nn
    tv = types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    transforms = types.ModuleType("torchvision.transforms")

    def vgg19(pretrained=False, **kw):
        layers, cin = [], 3
        for v in O.VGG_CFG + ["M"] + []:
            if v == "M":
                layers.append(nn.MaxPool2d(2, 2))
            else:
                layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        m = nn.Module()
        m.features = nn.Sequential(*layers)
        return m

    models.vgg19 = vgg19
    tv.models, tv.transforms = models, transforms
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.models"] = models
    sys.modules["torchvision.transforms"] = transforms


def ref_namespace(opt):
    import argparse as ap
    return ap.Namespace(**vars(opt))


def slice_of(t, k=64):
    f = t.detach().reshape(-1)
    idx = torch.linspace(0, f.numel() - 1, min(k, f.numel())).long()
    return [float(x) for x in f[idx]]


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def run_case(name, spec, tol0=2e-5):
    tol = tol0
    opt = O.make_opt(**spec["opt"])
    states = O.recipe_state(opt, gain=1.0)
    batch = O.synthetic_batch(opt, spec["n"], seed=1000 + spec["seed"])

    # ---- reference
    from managers.trainer_manager import TrainerManager
    torch.autograd.set_detect_anomaly(False)
    ropt = ref_namespace(opt)
    tm = TrainerManager(ropt)
    model = tm.sr_model_on_one_gpu
    nets = {"SR": model.netSR, "D": model.netD, "E": model.netE, "VGG": model.criterionVGG.vgg}
    # the reference slices VGG into slice1..5 holding the same conv modules; map by features idx
    vgg_sd = {}
    for sname, sl in [("slice1", nets["VGG"].slice1), ("slice2", nets["VGG"].slice2), ("slice3", nets["VGG"].slice3),
                      ("slice4", nets["VGG"].slice4), ("slice5", nets["VGG"].slice5)]:
        for idx, mod in sl.named_children():
            if hasattr(mod, "weight"):
                mod.weight.data.copy_(states["VGG"]["features.%s.weight" % idx])
                mod.bias.data.copy_(states["VGG"]["features.%s.bias" % idx])
    for net in ("SR", "D", "E"):
        sd = nets[net].state_dict()
        want = O.net_specs(opt)[net]
        assert set(sd.keys()) == set(want.keys()), (net, set(sd.keys()) ^ set(want.keys()))
        for k, v in sd.items():
            assert tuple(v.shape) == tuple(want[k]), (net, k, tuple(v.shape), want[k])
        nets[net].load_state_dict(states[net])
    # optimizer grouping check
    n_g = [len(g["params"]) for g in tm.optimizer_G.param_groups]
    n_d = [len(g["params"]) for g in tm.optimizer_D.param_groups]

    # ---- oracle
    orc = O.Oracle(opt, states)
    orc.create_optimizers()
    assert [len(g["params"]) for g in orc.opt_G.param_groups] == n_g, (n_g,)
    assert [len(g["params"]) for g in orc.opt_D.param_groups] == n_d, (n_d,)

    record = {"case": name, "opt": spec["opt"], "n": spec["n"], "batch_seed": 1000 + spec["seed"],
              "rng_seed": spec["seed"], "iters": [], "opt_groups_G": n_g, "opt_groups_D": n_d,
              "torch": torch.__version__}
    worst = 0.0
    # Inference is pinned on the freshly loaded recipe state: after an Adam step the conv biases
    # that feed a BatchNorm (zero analytic gradient, sign-of-noise update with beta1=0) differ by
    # +-lr between any two implementations, and eval-mode BN no longer cancels them.
    # inference mode (eval BN, no SN iteration, no noise)
    model.eval()
    with torch.no_grad():
        random.seed(spec["seed"])
        torch.manual_seed(spec["seed"])
        b = {k: v.clone() for k, v in batch.items()}
        out = model(tm.preprocess_input(b), mode="inference")
    model.train()
    random.seed(spec["seed"])
    torch.manual_seed(spec["seed"])
    ofake = orc.inference({k: v.clone() for k, v in batch.items()})
    e = rel(ofake, out["fake_image"])
    worst = max(worst, e)
    assert e < tol, (name, "inference", e)
    inference_rec = {"fake_norm": float(out["fake_image"].norm()), "fake_slice": slice_of(out["fake_image"])}
    # encode_only / demo (sr_model.py:92-108), eval mode as the inference and demo managers run them
    model.eval()
    with torch.no_grad():
        b = {k: v.clone() for k, v in batch.items()}
        pre = tm.preprocess_input(b)
        rstyle = model(dict(pre), mode="encode_only")
        # an explicit, perturbed style matrix so that `demo` is not just `inference` again
        given = (rstyle.detach() * 0.5 + 0.1).clamp(-1, 1)
        pre2 = dict(tm.preprocess_input({k: v.clone() for k, v in batch.items()}))
        pre2["encoded_style"] = given
        rdemo = model(pre2, mode="demo")["fake_image"]
    model.train()
    ostyle = orc.encode_only({k: v.clone() for k, v in batch.items()})
    odemo = orc.demo({k: v.clone() for k, v in batch.items()}, given)
    for what, a_, b_ in (("encode_only", ostyle, rstyle), ("demo", odemo, rdemo)):
        e = rel(a_, b_)
        worst = max(worst, e)
        assert e < tol, (name, what, e)
    inference_rec["style_norm"] = float(rstyle.norm())
    inference_rec["style_slice"] = slice_of(rstyle)
    inference_rec["demo_fake_norm"] = float(rdemo.norm())
    inference_rec["demo_fake_slice"] = slice_of(rdemo)
    ref_rng = None
    orc_rng = None
    for it in range(spec["iters"]):
        ent = {}
        for who in ("ref", "orc"):
            # separate but identically-seeded RNG streams for the two implementations
            if it == 0:
                torch.manual_seed(spec["seed"])
                random.seed(spec["seed"])
            else:
                torch.set_rng_state(ref_rng[0] if who == "ref" else orc_rng[0])
                random.setstate(ref_rng[1] if who == "ref" else orc_rng[1])
            b = {k: v.clone() for k, v in batch.items()}
            b["path"] = ["x"] * spec["n"]
            if who == "ref":
                tm.run_generator_one_step(b)
                gl = {k: float(v.detach().reshape(-1)[0]) for k, v in tm.g_losses.items()}
                fake = tm.generated.detach().clone()
                ggrads = {}
                for net in ("SR", "E"):
                    for k, p in nets[net].named_parameters():
                        if p.grad is not None:
                            ggrads["%s/%s" % (net, k)] = p.grad.detach().clone()
                tm.run_discriminator_one_step(b)
                dl = {k: float(v.detach().reshape(-1)[0]) for k, v in tm.d_losses.items()}
                dgrads = {"D/" + k: p.grad.detach().clone() for k, p in nets["D"].named_parameters()
                          if p.grad is not None}
                ref_rng = (torch.get_rng_state(), random.getstate())
                ent["ref"] = (gl, fake, ggrads, dl, dgrads)
            else:
                b.pop("path")
                gl_t, fake = orc.run_generator_one_step(b)
                gl = {k: float(v.detach().reshape(-1)[0]) for k, v in gl_t.items()}
                ggrads = {}
                for net in ("SR", "E"):
                    for k, p in orc.params(net):
                        if p.grad is not None:
                            ggrads["%s/%s" % (net, k)] = p.grad.detach().clone()
                dl_t = orc.run_discriminator_one_step(b)
                dl = {k: float(v.detach().reshape(-1)[0]) for k, v in dl_t.items()}
                dgrads = {"D/" + k: p.grad.detach().clone() for k, p in orc.params("D") if p.grad is not None}
                orc_rng = (torch.get_rng_state(), random.getstate())
                ent["orc"] = (gl, fake.detach().clone(), ggrads, dl, dgrads)
        (rgl, rfake, rgg, rdl, rdg), (ogl, ofake, ogg, odl, odg) = ent["ref"], ent["orc"]
        # From the 2nd iteration on, the two runs start from states that already differ by
        # +-lr in every noise-level-gradient ELEMENT (Adam beta1=0 is sign-like), so agreement
        # is only expected to ~1e-2; iteration 0 is the strict pin.
        tol = tol0 * (1 if it == 0 else 300)
        # ---- compare oracle vs reference
        for k in rgl:
            e = abs(rgl[k] - ogl[k]) / max(abs(rgl[k]), 1e-12)
            worst = max(worst, e)
            assert e < tol, (name, it, "G loss", k, rgl[k], ogl[k])
        for k in rdl:
            e = abs(rdl[k] - odl[k]) / max(abs(rdl[k]), 1e-12)
            worst = max(worst, e)
            # the D step runs after optimizer_G.step(): sign-of-noise Adam updates already separate the runs
            assert e < 50 * tol, (name, it, "D loss", k, rdl[k], odl[k])
        e = rel(ofake, rfake)
        worst = max(worst, e)
        assert e < tol, (name, it, "fake", e)
        assert set(rgg) == set(ogg), set(rgg) ^ set(ogg)
        assert set(rdg) == set(odg), set(rdg) ^ set(odg)
        # conv biases feeding a BatchNorm/InstanceNorm have an analytically-zero gradient: both
        # sides hold rounding noise there, so errors are measured against a floor tied to the
        # largest gradient of the step.
        gmax = max(float(v.norm()) for v in list(rgg.values()) + list(rdg.values()))
        # tensors whose true gradient is zero: with beta1=0 Adam moves them by +-lr*sign(noise)
        zero_grad_keys = sorted(k for k, v in {**rgg, **rdg}.items() if float(v.norm()) < 1e-4 * gmax)
        for k in list(rgg) + list(rdg):
            a, bb = (ogg[k], rgg[k]) if k in rgg else (odg[k], rdg[k])
            e = float((a - bb).norm()) / max(float(bb.norm()), 1e-3 * gmax)
            worst = max(worst, e)
            if os.environ.get("GOLDEN_DEBUG"):
                print("  grad %-60s rel %.3g  norm %.3g" % (k, e, float(bb.norm())))
                continue
            # Noise floor of the REFERENCE ITSELF (oracle/noise_floor.py: image *= 1+1e-7): G-step
            # gradients move by up to 2.6e-3 rel, D-step gradients by 2.3e-2 (L1/hinge sign flips,
            # then the sign-like beta1=0 Adam step in between).  Bounds sit just above that floor.
            assert e < (GRAD_TOL_G if k in rgg else GRAD_TOL_D) * (1 if it == 0 else 4), \
                (name, it, "grad", k, e, float(bb.norm()), gmax)
        # post-step state (params + buffers) agreement
        for net in ("SR", "D", "E"):
            sd = nets[net].state_dict()
            for k, v in sd.items():
                if not v.is_floating_point():
                    assert int(v) == int(orc.S[net][k]), (net, k)
                    continue
                if "%s/%s" % (net, k) in zero_grad_keys:
                    continue
                e = rel(orc.S[net][k].detach(), v)
                worst = max(worst, e)
                assert e < 1e-3 * (1 if it == 0 else 10), (name, it, "state", net, k, e)
        record["iters"].append({
            "g_losses": rgl, "d_losses": rdl,
            "fake_norm": float(rfake.norm()), "fake_slice": slice_of(rfake),
            "grad_norms": {k: float(v.norm()) for k, v in {**rgg, **rdg}.items()},
            "grad_slices": {k: slice_of(v, 16) for k, v in {**rgg, **rdg}.items()
                            if k.endswith(("conv_0.weight_orig", "mlp_gamma.weight", "alpha_gamma", "noise_in.weight",
                                           "initial.weight", "model1.0.0.weight_orig", "final.0.0.weight_orig",
                                           "noise_weights", "mlp_style_gamma.weight", "mlp_shared.0.weight"))},
            "state_norms": {"%s/%s" % (net, k): float(v.float().norm())
                            for net in ("SR", "D", "E") for k, v in nets[net].state_dict().items()},
            "zero_grad_keys": zero_grad_keys,
            "branch": {"full": bool(model.last_encoded_style_is_full), "noisy": bool(model.last_encoded_style_is_noisy)},
        })
    record["inference"] = inference_rec
    record["oracle_vs_reference_worst_rel"] = worst
    os.makedirs(os.path.join(ROOT, "tests", "golden"), exist_ok=True)
    with open(os.path.join(ROOT, "tests", "golden", name + ".json"), "w") as f:
        json.dump(record, f, indent=1)
    print("%-32s OK  worst rel diff oracle-vs-reference = %.3g" % (name, worst))


def layer_kats():
    """Layer-level known answers straight from reference modules (tiny shapes)."""
    import torch.nn.functional as F
    from deepsee_models.networks.normalization import SPADE, SEAN_Block, PureSEAN_Block, NoiseInjection
    from deepsee_models.networks.encoder import CombinedstyleEncoder
    from deepsee_models.networks.loss import GANLoss
    torch.manual_seed(5)
    opt = ref_namespace(O.make_opt(max_fm_size=8, regional_style_size=128, ngf=2, nef=4))
    out = {}
    C, L = 8, 19
    seg = O.onehot_labels(torch.randint(0, L, (2, 1, 16, 16)).float(), L)
    style = torch.rand(2, L, 128) * 2 - 1
    for nm, cls, res in (("spade", SPADE, 8), ("sean", SEAN_Block, 8), ("sean_fmcap", SEAN_Block, 16),
                         ("puresean_fmcap", PureSEAN_Block, 16)):
        cfg = "latesean" + "syncbatch3x3" if cls is SPADE else "seansyncbatch3x3"
        m = cls("lateseansyncbatch3x3" if cls is SPADE else "seansyncbatch3x3", C, L, opt)
        sd = {k: O.recipe_tensor("kat_" + nm, k, v.shape, 1.0) for k, v in m.state_dict().items()}
        m.load_state_dict(sd)
        x = torch.randn(2, C, res, res, generator=torch.Generator().manual_seed(7))
        y = m(x, seg, style)
        out[nm] = {"res": res, "x_seed": 7, "y_norm": float(y.norm()), "y_slice": slice_of(y, 32),
                   "running_mean": slice_of(m.param_free_norm.running_mean, 8),
                   "running_var": slice_of(m.param_free_norm.running_var, 8)}
    # hinge
    gl = GANLoss("hinge", tensor=torch.FloatTensor)
    p = [[torch.randn(2, 1, 5, 5, generator=torch.Generator().manual_seed(i))] for i in (1, 2)]
    out["hinge"] = {"g": float(gl(p, True, for_discriminator=False)), "d_fake": float(gl(p, False)),
                    "d_real": float(gl(p, True))}
    # style pooling + nearest resize
    feat = torch.randn(2, 6, 8, 8, generator=torch.Generator().manual_seed(3))
    enc = CombinedstyleEncoder(ref_namespace(O.make_opt(nef=4)))
    sm = enc.extract_style_matrix(feat, F.interpolate(seg, size=(8, 8), mode="nearest"))
    out["style_pool"] = {"norm": float(sm.norm()), "slice": slice_of(sm, 32)}
    # bicubic preprocess + avgpool
    img = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(9)) * 2 - 1
    lr = F.interpolate(img, (4, 4), mode="bicubic").clamp(-1, 1)
    out["bicubic"] = {"slice": slice_of(lr, 48)}
    ap = F.avg_pool2d(img, 3, 2, [1, 1], count_include_pad=False)
    out["avgpool"] = {"slice": slice_of(ap, 32), "norm": float(ap.norm())}
    with open(os.path.join(ROOT, "tests", "golden", "layer_kats.json"), "w") as f:
        json.dump({"seg_seed": 5, "kats": out, "torch": torch.__version__}, f, indent=1)
    print("layer_kats                       written")


def host_logic():
    """Pins of the host-side rows straight from the reference: (a15) per-tensor statistics of a freshly initialised
    model (base_network.py:28-59 via networks/__init__.py:37-43), (a2) the learning-rate schedule of
    TrainerManager.update_learning_rate (trainer_manager.py:76-96), (f4) the statistics the DataParallel branch of
    SynchronizedBatchNorm2d computes from the replicas' (sum, ssum) (batchnorm.py:128-145, callable on the CPU)."""
    from managers.trainer_manager import TrainerManager
    from deepsee_models.networks.sync_batchnorm import SynchronizedBatchNorm2d
    out = {"torch": torch.__version__}
    # ---- init statistics
    init = {}
    for tag, over in (("indep_ngf8", dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8)),
                      ("guided_kaiming_ngf8", dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8,
                                                   netE="fullstyle", noisy_style_scale=0.05, guiding_style_image=True,
                                                   init_type="kaiming"))):
        torch.manual_seed(123)
        opt = O.make_opt(**over)
        tm = TrainerManager(ref_namespace(opt))
        m = tm.sr_model_on_one_gpu
        rec = {}
        for net, mod in (("SR", m.netSR), ("D", m.netD), ("E", m.netE)):
            for k, v in mod.state_dict().items():
                v = v.detach().float()
                rec["%s/%s" % (net, k)] = {"numel": v.numel(), "std": float(v.std()) if v.numel() > 1 else 0.0,
                                           "mean": float(v.mean()), "norm": float(v.norm()),
                                           "min": float(v.min()), "max": float(v.max())}
        init[tag] = {"opt": over, "stats": rec}
    out["init"] = init
    # ---- learning-rate schedule
    sched = {}
    for tag, over in (("ttur", dict(niter=3, niter_decay=4)), ("no_ttur", dict(niter=2, niter_decay=2, no_TTUR=True))):
        opt = O.make_opt(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=2, nef=4, ndf=4, **over)
        tm = TrainerManager(ref_namespace(opt))
        rows = []
        for epoch in range(1, over["niter"] + over["niter_decay"] + 1):
            tm.update_learning_rate(epoch)
            rows.append({"epoch": epoch, "G": [g["lr"] for g in tm.optimizer_G.param_groups],
                         "D": [g["lr"] for g in tm.optimizer_D.param_groups], "old_lr": tm.old_lr})
        sched[tag] = {"opt": dict(over, lr=opt.lr), "rows": rows}
    out["lr_schedule"] = sched
    # ---- SyncBN master arithmetic on two replicas' sums (8 channels)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(4, 8, 6, 6, generator=g) * torch.rand(1, 8, 1, 1, generator=g) * 3 + torch.randn(1, 8, 1, 1, generator=g)
    x[:, 7] = 0.25                                    # constant channel: var 0 -> the clamp(var, eps) case
    bn = SynchronizedBatchNorm2d(8, affine=False)
    shards = [x[:2], x[2:]]
    sum_ = sum(s.transpose(0, 1).reshape(8, -1).sum(1) for s in shards)
    ssum = sum((s ** 2).transpose(0, 1).reshape(8, -1).sum(1) for s in shards)
    mean, inv_std = bn._compute_mean_std(sum_, ssum, 4 * 36)
    out["syncbn"] = {"x_seed": 77, "shards": 2, "mean": [float(v) for v in mean], "inv_std": [float(v) for v in inv_std],
                     "running_mean": [float(v) for v in bn.running_mean],
                     "running_var": [float(v) for v in bn.running_var],
                     "x": [float(v) for v in x.reshape(-1)], "shape": list(x.shape)}
    with open(os.path.join(ROOT, "tests", "golden", "host_logic.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("host_logic                       written")


def install_cv2_stub():
    """cv2 is absent from this image.  evaluator/calculate_PSNR_SSIM.py needs two of its functions; they are provided
    from OpenCV's documented definitions so that the REFERENCE's PSNR / SSIM code (quantisation, window, cropping,
    constants, the channel loop) runs unmodified:
      getGaussianKernel(ksize, sigma): G_i = alpha * exp(-(i - (ksize-1)/2)^2 / (2 sigma^2)), sum G_i = 1, [ksize,1] float64
      filter2D(src, -1, kernel): correlation, anchor at the kernel centre, BORDER_REFLECT_101, every channel separately
    (the border mode is irrelevant to the reference: it keeps [5:-5, 5:-5] only)."""
    import types
    import numpy as np
    from scipy import ndimage
    cv2 = types.ModuleType("cv2")

    def getGaussianKernel(ksize, sigma):
        x = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
        g = np.exp(-(x ** 2) / (2.0 * sigma ** 2))
        return (g / g.sum()).reshape(ksize, 1)

    def filter2D(src, ddepth, kernel):
        assert ddepth == -1
        if src.ndim == 2:
            return ndimage.correlate(src, kernel, mode="mirror")
        return np.stack([ndimage.correlate(src[..., c], kernel, mode="mirror") for c in range(src.shape[2])], axis=2)

    cv2.getGaussianKernel, cv2.filter2D = getGaussianKernel, filter2D
    sys.modules["cv2"] = cv2


def metrics():
    """(f4) PSNR / SSIM / RMSE of MetricsEvaluator.collect_samples (evaluator/evaluation.py:88-137), from the
    reference's own tensor2im / calculate_psnr / calculate_ssim on seeded image pairs -> tests/golden/metrics.json
    (inputs are regenerated from the recorded seeds by the tests)."""
    install_cv2_stub()
    from evaluator.calculate_PSNR_SSIM import calculate_psnr, calculate_ssim
    from util.util import tensor2im
    cases = []
    for seed, (n, h, w), kind in ((1, (2, 32, 32), "noise"), (2, (3, 48, 40), "close"), (3, (1, 64, 64), "smooth"),
                                 (4, (2, 21, 37), "saturated"), (5, (1, 32, 32), "identical")):
        fake, real = O.metric_case_inputs(seed, n, h, w, kind)
        fake_np, real_np = tensor2im(fake), tensor2im(real)
        psnr = [calculate_psnr(fake_np[i], real_np[i]) for i in range(n)]
        ssim = [float(calculate_ssim(fake_np[i], real_np[i])) for i in range(n)]
        rmse = [float(v) for v in torch.nn.MSELoss(reduction="none")(fake, real).mean(dim=[1, 2, 3]).sqrt()]
        mine = O.psnr_ssim_rmse(fake, real)
        for i in range(n):
            assert (psnr[i] == mine[i, 0]) or abs(psnr[i] - float(mine[i, 0])) < 1e-9 * abs(psnr[i]), (psnr[i], mine[i])
            assert abs(ssim[i] - float(mine[i, 1])) < 1e-10, (ssim[i], mine[i])
            assert abs(rmse[i] - float(mine[i, 2])) < 1e-6 * rmse[i] + 1e-12
        cases.append({"seed": seed, "shape": [n, h, w], "kind": kind, "psnr": [repr(p) for p in psnr], "ssim": ssim,
                      "rmse": rmse, "u8_checksum": [int(fake_np.astype(np.int64).sum()), int(real_np.astype(np.int64).sum())]})
    with open(os.path.join(ROOT, "tests", "golden", "metrics.json"), "w") as f:
        json.dump({"torch": torch.__version__, "cases": cases}, f, indent=1)
    print("metrics                          written")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    assert os.path.isdir(REF), "needs /root/reference (build container only)"
    install_torchvision_stub()
    sys.path.insert(0, REF)
    os.makedirs("/tmp/oracle_ckpt", exist_ok=True)
    torch.set_num_threads(8)
    for name, spec in CASES.items():
        if a.cases and name not in a.cases:
            continue
        run_case(name, spec)
    if not a.cases or "layer_kats" in a.cases:
        layer_kats()
    if not a.cases or "host_logic" in a.cases:
        host_logic()
    if not a.cases or "metrics" in a.cases:
        metrics()


if __name__ == "__main__":
    main()
