"""SRModel — the model facade of the hot path, same surface as the reference's
deepsee_models/sr_model.py::SRModel: attributes netSR / netD / netE / opt / model_variant / logs /
last_encoded_style_is_full / last_encoded_style_is_noisy; forward(data, mode) with modes 'generator', 'encode_only', 'demo',
'discriminator', 'inference', 'baseline' and the six explorative modes of deepsee_amd.explore.MODES (anything else raises
ValueError like sr_model.py:445-446; `style_seed=int` pins the eval-mode style field of opt.random_style_matrix);
create_optimizers(opt);
save(epoch) / load_weights().  All activation-space compute runs in libdeepsee_hip.so.
"""
import math
import os
import sys
import warnings
from collections import OrderedDict

import torch
import torch.nn as nn

from . import explore
from . import lib as L
from . import networks as N
from . import ops
from .optim import FlatAdam
from .plan import from_opt as plan_from_opt


NETG_VALUES = ("deepsee", "nostyle", "nospadenostyle", "puresean")


def block_plan(opt):
    """sr.py:27-51: head_0 SPADE ('late' in norm_G), SEAN blocks, PureSEAN tail iff
    load_size >= 512.  Every layer's param-free norm follows norm_G (networks.param_free_norm_of: raises for a norm_G this build
    does not run).

    opt.netG (NETG_VALUES; an opt without the field: 'deepsee') selects one of the generators of ablation.py instead, by the names
    its find_network_using_name(netG, 'ablation') resolves; any other value raises ValueError:
      nostyle         every block SPADE (style=False), the tail beyond the fourth block PureSEAN iff load_size >= 512
                      (ablation.py:57-74: puresean=True wins over style=False)
      puresean        every block PureSEAN, head included (ablation.py:244-261)
      nospadenostyle  every block the pix2pixHD ResnetBlock, kind 'resnet' (ablation.py:13-29, 151-168)"""
    N.param_free_norm_of(opt.norm_G)
    netG = getattr(opt, "netG", "deepsee")
    if not isinstance(netG, str) or netG not in NETG_VALUES:
        raise ValueError("netG %r: expected one of %s" % (netG, ", ".join(NETG_VALUES)))
    nb = int(round(math.log2(opt.crop_size) - math.log2(opt.start_size)))
    cfg = opt.norm_G.replace("spectral", "")
    sk = "sean" if "sean" in cfg else "spade"
    early = "late" not in opt.norm_G
    head, tail = (sk if early else "spade"), "puresean"
    if netG == "nostyle":
        head = sk = "spade"
    elif netG == "puresean":
        head = sk = "puresean"
    elif netG == "nospadenostyle":
        head = sk = tail = "resnet"
    plan = [("head_0", head), ("G_middle_0", sk), ("G_middle_1", sk)]
    max_nb = 4 if opt.load_size >= 512 else 99
    kinds = [sk] * max(0, min(nb, max_nb) - 1)
    if max_nb != 99:
        kinds += [tail] * max(0, nb - max_nb)
    return plan + [("up_list.%d" % i, k) for i, k in enumerate(kinds)]


def check_geometry(opt, plan, lr_h, lr_w):
    """Refuse, on the host and before any launch, an LR shape the generator cannot run.  `plan` is block_plan(opt); the levels
    are (lr_h << l, lr_w << l): head_0 at l = 0, G_middle_0 / G_middle_1 at 1, up_list.i at 2 + i.  A SEAN or PureSEAN level of
    a NON-SQUARE map larger than opt.max_fm_size on either axis raises ValueError: the reference squashes such a map to
    [min(h, cap), min(w, cap)] with one nearest-neighbour factor per axis (normalization.py:172-174, 188-190), and the label
    kernels here index row h << shift, column w << shift with ONE shift.  That path is not built: set max_fm_size >= the long
    side.  Square maps keep the reference's cap."""
    lr_h, lr_w = int(lr_h), int(lr_w)
    if lr_h < 1 or lr_w < 1:
        raise ValueError("LR image of %d x %d" % (lr_h, lr_w))
    level = 0
    for i, (name, kind) in enumerate(plan):
        if i == 1 or i >= 3:          # G_middle_0 and every up_list block upsample their input by 2
            level += 1
        h, w = lr_h << level, lr_w << level
        if kind in ("sean", "puresean") and h != w and max(h, w) > opt.max_fm_size:
            raise ValueError("generator level %d (%s, %s): the %d x %d map is not square and exceeds max_fm_size=%d; the per-axis "
                             "cap of the reference is not built for non-square maps -- set max_fm_size >= %d"
                             % (level, name, kind, h, w, opt.max_fm_size, max(lr_h, lr_w) << max(len(plan) - 2, 1)))


def init_weights(net, init_type, gain, gen):
    """base_network.py:28-59 semantics on our parameter holders: xavier_normal(gain) (or kaiming / normal) on
    every conv weight incl. spectral-norm weight_orig and the unused Conv1d; biases 0; noise weights 0;
    alpha ~ U(0,1); SN u/v ~ normalised N(0,1); BatchNorm2d(affine=True) of norm_D / norm_E: weight ~ N(1, gain), bias 0."""
    bn_weights = {m + ".weight" for m, mod in net.named_modules() if isinstance(mod, N.BatchNormP)}
    for name, p in list(net.named_parameters()) + list(net.named_buffers()):
        leaf = name.split(".")[-1]
        if name in bn_weights:
            p.data.copy_(1.0 + torch.randn(p.shape, generator=gen) * gain)
        elif leaf in ("running_mean", "num_batches_tracked"):
            p.data.zero_()
        elif leaf == "running_var":
            p.data.fill_(1.0)
        elif leaf in ("weight_u", "weight_v"):
            t = torch.randn(p.shape, generator=gen)
            p.data.copy_(t / t.norm().clamp_min(1e-12))
        elif leaf in ("alpha_beta", "alpha_gamma"):
            p.data.copy_(torch.rand(p.shape, generator=gen))
        elif leaf == "bias" or leaf == "noise_weights" or ".noise_" in name:
            p.data.zero_()
        elif p.dim() >= 3:
            rf = 1
            for s in p.shape[2:]:
                rf *= s
            fan_in, fan_out = p.shape[1] * rf, p.shape[0] * rf
            if init_type == "xavier":
                std = gain * math.sqrt(2.0 / (fan_in + fan_out))
            elif init_type == "kaiming":
                std = math.sqrt(2.0 / fan_in)
            elif init_type == "normal":
                std = gain
            else:
                raise NotImplementedError("initialization method [%s] is not implemented" % init_type)
            p.data.copy_(torch.randn(p.shape, generator=gen) * std)


def gan_loss_modes(gan_mode):
    """opt.gan_mode -> the ops.mean_loss modes (generator, D real, D fake) of GANLoss (loss.py:31-40,60-85): real label 1,
    fake label 0, each the mean over the last output of a discriminator scale.  The mode is compared exactly; any value
    other than 'ls', 'original', 'w' or 'hinge' raises the reference's ValueError."""
    modes = {"hinge": (ops.MODE_NEG, ops.MODE_HINGE_REAL, ops.MODE_HINGE_FAKE),
             "w": (ops.MODE_NEG, ops.MODE_NEG, ops.MODE_W_FAKE),
             "ls": (ops.MODE_LS_REAL, ops.MODE_LS_REAL, ops.MODE_LS_FAKE),
             "original": (ops.MODE_BCE_REAL, ops.MODE_BCE_REAL, ops.MODE_BCE_FAKE)}
    if not isinstance(gan_mode, str) or gan_mode not in modes:
        raise ValueError("Unexpected gan_mode {}".format(gan_mode))
    return modes[gan_mode]


def _sum_terms(terms):
    """Sum of the [1]-shaped loss terms in two launches (cat + reduce) instead of one ATen add per term."""
    if not terms:        # a discriminator without intermediate features (the reference starts its sums from 0, sr_model.py:535)
        return torch.zeros(1, device="cuda")
    return terms[0] if len(terms) == 1 else torch.cat(terms).sum(0, keepdim=True)


class SRModel(nn.Module):
    def __init__(self, opt):
        super().__init__()
        ops.check_label_count(opt.semantic_nc)       # (before anything is allocated: > 32 classes can only fail later, mid-pass)
        if not torch.cuda.is_available():
            raise RuntimeError("deepsee_amd.SRModel needs an MI355X (HIP) device: there is no CPU fallback")
        L.lib()  # fail loudly if libdeepsee_hip.so is missing
        self.opt = opt
        # which of the equivalent kernel paths this model's operators take, and its precision (opt.precision 'fp32' | 'fp16':
        # 16-bit matrix-core GEMMs, fp32 everything else) -- an immutable value owned by THIS model (deepsee_amd/plan.py)
        self.plan = plan_from_opt(opt)
        self.use_E = opt.netE is not None and len(opt.netE) > 0
        self.model_variant = "guided" if (self.use_E and "full" in opt.netE) else "independent"   # sr_model.py:26-30
        gen = torch.Generator().manual_seed(int(getattr(opt, "seed", 0)))
        self._block_plan = block_plan(opt)
        self.netSR = N.DeepSEESR(opt, self._block_plan)
        init_weights(self.netSR, opt.init_type, opt.init_variance, gen)
        self.netD = None
        self.gan_modes = None
        if opt.isTrain:
            self.gan_modes = gan_loss_modes(opt.gan_mode)     # sr_model.py:34-36: the GAN loss exists only for training
            self.netD = N.MultiscaleDiscriminator(opt)
            init_weights(self.netD, opt.init_type, opt.init_variance, gen)
        self.netE = None
        if self.use_E:
            self.netE = N.StyleEncoder(opt)
            init_weights(self.netE, opt.init_type, opt.init_variance, gen)
        self.vgg = None
        if opt.isTrain and not opt.no_vgg_loss:
            # the reference downloads torchvision's pretrained VGG19 (architecture.py:154).  opt.vgg_weights names a
            # local copy of that state dict (torchvision keys 'features.N.weight/bias', or the bare 'N.weight/bias' of
            # vgg19().features); without it the taps are He-initialised random features, NOT a perceptual loss.
            self.vgg = N.VGG19Taps()
            init_weights(self.vgg, "kaiming", 1.0, gen)
            self.vgg_pretrained = False
            path = getattr(opt, "vgg_weights", None)
            if path:
                self.load_vgg_state(torch.load(path, map_location="cpu"))
            else:
                warnings.warn("deepsee_amd: no pretrained VGG19 weights (opt.vgg_weights is unset): the VGG loss term "
                              "(lambda_vgg=%g) runs on randomly initialised features.  Fine for benchmarks and parity "
                              "tests; for real training pass opt.vgg_weights=<torchvision vgg19 state dict> or call "
                              "SRModel.load_vgg_state()." % opt.lambda_vgg, RuntimeWarning, stacklevel=2)
        self.cuda()
        self.noise = N.DeviceNoise(seed=int(getattr(opt, "seed", 0)) * 7919 + 17)
        self.logs = OrderedDict()
        self.last_encoded_style_is_full = True
        self.last_encoded_style_is_noisy = False
        if not opt.isTrain or opt.continue_train:
            self.load_weights()

    # ---- reference surface
    def get_logs(self):
        return self.logs

    def use_gpu(self):
        return True

    def forward(self, data, mode, **kwargs):
        with self.plan.active():       # the backward pass re-activates it per autograd node (ops._under_plan)
            return self._forward(data, mode, **kwargs)

    def _forward(self, data, mode, **kwargs):
        if mode in ("generator", "discriminator", "inference", "demo") or mode in explore.MODES:
            # every mode that runs the generator: the LR shape is checked on the host before the first kernel of this forward
            lr = data.get("image_lr")
            if isinstance(lr, torch.Tensor) and lr.dim() == 4:
                hw = lr.shape[1:3] if getattr(lr, "dsee_layout", None) == "nhwc" else lr.shape[2:4]
                check_geometry(self.opt, self._block_plan, hw[0], hw[1])
        d = self._native(data)
        if mode in ("generator", "discriminator"):
            self.noise.begin_step()     # fresh Philox positions / branch coins for this forward
        else:
            # eval-mode draws (the style field of opt.random_style_matrix) come from a stream of their own; style_seed pins it
            begin_eval = getattr(self.noise, "begin_eval", None)    # (a caller's own noise object may only know begin_step)
            if begin_eval is not None:
                begin_eval(kwargs.get("style_seed"))
        if mode == "generator":
            g_loss, generated = self.compute_generator_loss(d)
            self.logs["image/downsized"] = d["image_lr"]
            return g_loss, generated
        elif mode == "discriminator":
            return self.compute_discriminator_loss(d)
        elif mode == "inference":
            with torch.no_grad():
                fake, _ = self.generate_fake(d, no_noise=True)
            data["fake_image"] = ops.to_nchw(fake, 3)
            return {k: v for k, v in data.items() if v is not None}
        elif mode == "encode_only":
            # sr_model.py:92-99: the (uncorrupted) style matrix [N, label_nc, regional_style_size]
            return self.encode_style(d, no_noise=True)
        elif mode == "demo":
            # sr_model.py:100-108: the generator alone on an explicit style matrix `encoded_style`
            with torch.no_grad():
                style = data["encoded_style"].to("cuda", torch.float32).contiguous()
                fake = self.netSR(d["image_lr"], d["labels"], style, self.noise, self.training)
            data["fake_image"] = ops.to_nchw(fake, 3)
            return {k: v for k, v in data.items() if v is not None}
        elif mode == "baseline":
            # sr_model.py:109-115: bicubic upsampling of the LR image to the HR size, clamped -- no network, no noise, no coins
            hr, lr = d["image_hr"], d["image_lr"]
            if lr.shape[1] == lr.shape[2]:
                up = ops.bicubic_up(lr, hr.shape[1], hr.shape[2], clamp=True)
            else:       # a non-square LR image: the same A = -0.75 formula with one scale per axis (dsee_resize_hw)
                up = ops.resize_hw(lr, hr.shape[1], hr.shape[2], "bicubic", clamp=True)
            return OrderedDict([("input_label", data.get("input_semantics")), ("image_downsized", data.get("image_lr")),
                                ("fake_image", ops.to_nchw(up, 3)), ("image_full", data.get("image_hr"))])
        elif mode in explore.MODES:
            # sr_model.py:219-444: the style variants of the batch, one generator pass over all (image, variant) pairs
            return explore.forward(self, data, d, mode, u8=bool(kwargs.get("u8", False)))
        else:
            raise ValueError("|mode| is invalid")

    def get_noise(self, shape, delta):
        """sr_model.py:448-457: drawn with torch's CPU generator, then uploaded -- the numbers torch.manual_seed gives the
        reference."""
        if self.opt.noise_dist == "normal":
            noise = torch.randn(shape).clamp(-1, 1) * delta
        elif self.opt.noise_dist == "uniform":
            noise = torch.rand(shape).clamp(-1, 1) * delta
        else:
            raise ValueError("Invalid noise distribution: {}".format(self.opt.noise_dist))
        return noise.cuda()

    def encode_with(self, branch, image, labels):
        """The uncorrupted style matrix of an explicit (image, label map) through an explicit encoder branch ('full' | 'mini';
        the guided model has the full one only), in eval mode: no coin is flipped, no spectral-norm vector or running statistic
        advances, and last_encoded_style_is_* keep what the last training forward left."""
        if self.model_variant == "guided":
            assert branch == "full", "the guided model has no mini encoder"
        with torch.no_grad():
            return self.netE(image, labels, branch, True, self.noise, False)

    def load_vgg_state(self, state):
        """Load torchvision's vgg19 weights into the frozen perceptual taps (architecture.py:151-181).  Accepts the
        full model's state dict ('features.N.*', classifier keys ignored) or that of vgg19().features ('N.*')."""
        own = self.vgg.state_dict()
        picked = {}
        for k in own:
            bare = k[len("features."):]
            if k in state:
                picked[k] = state[k]
            elif bare in state:
                picked[k] = state[bare]
            else:
                raise RuntimeError("VGG19 state dict lacks %s" % k)
        self.load_net_state(self.vgg, picked)
        self.vgg_pretrained = True

    def create_optimizers(self, opt):
        """sr_model.py:469-495: G = SR params + non-'mini' E params @ lr/2 (group 0), 'mini' E params @ lr/8
        (group 1); D @ 2*lr; betas (beta1, beta2).  Without a discriminator (isTrain False) opt_D is None."""
        g_main = [("SR." + k, p) for k, p in self.netSR.named_parameters()]
        g_low = []
        if self.use_E:
            for k, p in self.netE.named_parameters():
                (g_low if "mini" in k else g_main).append(("E." + k, p))
        lr_g, lr_d = (opt.lr, opt.lr) if opt.no_TTUR else (opt.lr / 2, opt.lr * 2)
        print("lr G: {}, lr D: {}".format(lr_g, lr_d), file=sys.stderr)   # (sr_model.py:112 prints this; keep stdout clean)
        groups = [{"params": g_main, "lr": lr_g}]
        if g_low:
            groups.append({"params": g_low, "lr": lr_g / 4})
        opt_g = FlatAdam(groups, betas=(opt.beta1, opt.beta2))
        opt_d = None
        if self.netD is not None:
            opt_d = FlatAdam([{"params": [("D." + k, p) for k, p in self.netD.named_parameters()], "lr": lr_d}],
                             betas=(opt.beta1, opt.beta2))
        return opt_g, opt_d

    def _ckpt(self, label, epoch):
        return os.path.join(self.opt.checkpoints_dir, self.opt.name, "%s_net_%s.pth" % (epoch, label))

    def save(self, epoch):
        """util/util.py:217-226: {epoch}_net_{SR,D,E}.pth = {"model": state_dict} with the reference's keys.
        Data-parallel: only rank 0 writes (parameters and spectral-norm buffers are identical on every rank; the
        sync-free BatchNorm running statistics saved are rank 0's shard's, as in the reference DP where only the master
        replica keeps them, sync_batchnorm/batchnorm.py:128-145).  Files are written to a temporary name and renamed,
        so a reader never sees a torn checkpoint."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
            return
        os.makedirs(os.path.join(self.opt.checkpoints_dir, self.opt.name), exist_ok=True)
        for label, net in (("SR", self.netSR), ("D", self.netD), ("E", self.netE)):
            if net is not None:
                path = self._ckpt(label, epoch)
                tmp = "%s.tmp.%d" % (path, os.getpid())
                torch.save({"model": OrderedDict((k, v.detach().cpu().clone()) for k, v in net.state_dict().items())}, tmp)
                os.replace(tmp, path)
        if hasattr(self.noise, "state_dict"):
            # not part of the reference's layout (its noise is torch's global generator, never saved): the position of the
            # Philox / branch-coin sequences, so that --continue_train continues them instead of replaying them from step 0
            path = self._ckpt("noise_state", epoch)
            tmp = "%s.tmp.%d" % (path, os.getpid())
            torch.save(self.noise.state_dict(), tmp)
            os.replace(tmp, path)

    def load_weights(self):
        opt = self.opt
        for label, net in (("SR", self.netSR), ("D", self.netD if opt.isTrain else None), ("E", self.netE)):
            if net is None:
                continue
            ck = torch.load(self._ckpt(label, opt.which_epoch), map_location="cpu")
            self.load_net_state(net, ck["model"] if "model" in ck else ck)
        path = self._ckpt("noise_state", opt.which_epoch)
        if opt.isTrain and os.path.exists(path) and hasattr(self.noise, "load_state_dict"):
            self.noise.load_state_dict(torch.load(path, map_location="cpu"))

    @staticmethod
    def load_net_state(net, state):
        """load_state_dict that keeps parameter storage (flat optimizer buffers stay valid)."""
        own = net.state_dict()
        missing = set(own) - set(state)
        extra = set(state) - set(own)
        if missing or extra:
            raise RuntimeError("state dict mismatch: missing %s, unexpected %s" % (sorted(missing), sorted(extra)))
        for k, v in own.items():
            if tuple(state[k].shape) != tuple(v.shape) and state[k].numel() != v.numel():   # (a [1] for a [] is still taken)
                hint = ""
                if k.startswith("initial.") and v.dim() == 4 and state[k].dim() == 4 and state[k].shape[1] != v.shape[1]:
                    hint = " (a style encoder's first layer has label_nc input channels with opt.random_style_matrix, 3 without)"
                raise RuntimeError("state dict mismatch: %s is %s in the checkpoint, %s in this model%s"
                                   % (k, list(state[k].shape), list(v.shape), hint))
        with torch.no_grad():
            for k, v in own.items():
                v.copy_(state[k].to(v.device, v.dtype))

    def load_states(self, states):
        for label, net in (("SR", self.netSR), ("D", self.netD), ("E", self.netE), ("VGG", self.vgg)):
            if net is not None and label in states:
                self.load_net_state(net, states[label])

    def native_generator(self):
        """The generator of this model's current netSR weights behind the C entry points alone (deepsee_amd.native.NativeGenerator:
        mode "demo" as dsee_generator_prepare + dsee_generator_fwd).  A snapshot: later training steps do not reach it."""
        from .native import NativeGenerator
        return NativeGenerator(self.opt, self.netSR.state_dict())

    # ---- data plumbing
    def _native(self, data):
        """Accepts the manager's native dict (NHWC tensors + ops.Labels) or the reference's dict (one-hot NCHW
        `input_semantics`, NCHW images) and returns the native form."""
        d = {}
        sem = data.get("input_semantics")
        if isinstance(sem, torch.Tensor):
            lab = sem.argmax(1, keepdim=True).float()
            sem = ops.Labels(ops.label_to_u8(lab.cuda()), self.opt.semantic_nc)
        d["labels"] = sem
        gl = data.get("guiding_label")
        if isinstance(gl, torch.Tensor):
            gl = ops.Labels(ops.label_to_u8(gl.argmax(1, keepdim=True).float().cuda()), self.opt.semantic_nc)
        d["guiding_labels"] = gl
        for k in ("image_lr", "image_hr", "guiding_image"):
            v = data.get(k)
            # the layout is tagged by whoever produced the tensor (ops.to_nhwc / bicubic_down / the device input
            # pipeline set .dsee_layout), never guessed from the shape: [N,3,H,4] is a legal NCHW image at start_size 4
            if isinstance(v, torch.Tensor) and getattr(v, "dsee_layout", None) != "nhwc":
                assert v.dim() == 4 and v.shape[1] == 3, "%s: expected an NCHW RGB tensor, got %s" % (k, tuple(v.shape))
                v = ops.to_nhwc(v.cuda())
            d[k] = v
        return d

    # ---- losses (sr_model.py:518-564)
    def compute_generator_loss(self, d):
        opt = self.opt
        losses = OrderedDict()
        fake, _ = self.generate_fake(d)
        # D(fake | real), VGG(fake) and VGG(real) are independent given `fake`: three branches (ops.branches; the two
        # discriminator scales fork again inside netD)
        use_vgg = not opt.no_vgg_loss

        def vgg_real():
            with torch.no_grad():
                return self.vgg(d["image_hr"])
        parts = [lambda: self.discriminate(d["labels"], fake, d["image_hr"], train_d=False)]
        if use_vgg:
            parts += [lambda: self.vgg(fake), vgg_real]
        packed = getattr(self, "_vgg_packed", None)
        if packed is None:
            packed = self._vgg_packed = set()
        if use_vgg and self.plan not in packed:
            # the first forward under a plan builds the frozen VGG weights' packed / transformed images once (ops._frozen_cache
            # entries depend on the plan: precision, storage mode) and both VGG passes read them: that one time they run in
            # order, on one stream -- also when that first forward is a capture (a plan swapped in after construction)
            pred, fx, fy = [f() for f in parts]
            packed.add(self.plan)
        else:
            pred, fx, fy = (ops.branches(*parts, inputs=[fake, d["image_hr"]]) + [None, None])[:3]
        n = fake.shape[0]
        pred, pred_real = pred      # (the generated half with its graph, the real half without: discriminate(train_d=False))
        gan = 0
        g_mode = self.gan_modes[0]
        for p in pred:
            gan = gan + ops.mean_loss(p[-1], None, g_mode, 1.0 / len(pred), valid_c=1, lo=0, hi=n)
        losses["GAN"] = gan
        if not opt.no_ganFeat_loss:
            terms = []
            for p, pr in zip(pred, pred_real):
                for f, real in zip(p[:-1], pr[:-1]):
                    terms.append(ops.mean_loss(f, real, ops.MODE_L1, opt.lambda_feat / len(pred), lo=0, hi=n))
            losses["GAN_Feat"] = _sum_terms(terms)
        if use_vgg:
            losses["VGG"] = _sum_terms([ops.mean_loss(a, b, ops.MODE_L1, w * opt.lambda_vgg)
                                        for w, a, b in zip(N.VGG_WEIGHTS, fx, fy)])
        return losses, ops.ToNCHW.apply(fake, 3)

    def compute_discriminator_loss(self, d):
        with torch.no_grad():
            fake, _ = self.generate_fake(d)
        fake = fake.detach()
        pred = self.discriminate(d["labels"], fake, d["image_hr"], train_d=True)
        n = fake.shape[0]
        losses = OrderedDict()
        df = dr = 0
        _, real_mode, fake_mode = self.gan_modes
        for p in pred:
            df = df + ops.mean_loss(p[-1], None, fake_mode, 1.0 / len(pred), valid_c=1, lo=0, hi=n)
            dr = dr + ops.mean_loss(p[-1], None, real_mode, 1.0 / len(pred), valid_c=1, lo=n, hi=2 * n)
        losses["D_Fake"], losses["D_Real"] = df, dr
        return losses

    def discriminate(self, labels, fake, real, train_d):
        """sr_model.py:655-683: one D pass over cat([fake; real]) on N.  In the generator step the D weights only
        need data gradients (their .grad is zeroed before use), so they enter detached."""
        if train_d:
            return self.netD(ops.DInput.apply(labels, fake, real), self.training)
        if not self.netD.per_sample:
            # norm_D with batch statistics (spectralbatch / spectralsync_batch): the statistics span cat([fake; real])
            # (sr_model.py:659-663), so the real half's activations reach the generated half's gradient through them -- one
            # pass with both halves in the graph; the real half's features enter the losses detached
            req = [p.requires_grad for p in self.netD.parameters()]
            for p in self.netD.parameters():
                p.requires_grad_(False)
            try:
                out = self.netD(ops.DInput.apply(labels, fake, real), self.training)
            finally:
                for p, r in zip(self.netD.parameters(), req):
                    p.requires_grad_(r)
            n = fake.shape[0]
            return out, [[t[n:].detach() for t in o] for o in out]
        # generator step (round 6), D normalising each sample on its own (InstanceNorm or no norm; NLayerD.forward asserts
        # it): the real half enters the losses detached (sr_model.py:547-564) -- it runs as a no-grad pass of its own on the
        # same weights (networks.NLayerD.forward), and the data gradients of the backward pass cover the generated half only.
        # Returns (features of the generated images, features of the real images).
        x = ops.DInput.apply(labels, fake)
        with torch.no_grad():
            xr = ops.DInput.apply(labels, real)
        req = [p.requires_grad for p in self.netD.parameters()]
        for p in self.netD.parameters():
            p.requires_grad_(False)
        try:
            return self.netD(x, self.training, xr)
        finally:
            for p, r in zip(self.netD.parameters(), req):
                p.requires_grad_(r)

    # ---- generator path (sr_model.py:566-650)
    def generate_fake(self, d, no_noise=False):
        style = self.encode_style(d, no_noise)
        fake = self.netSR(d["image_lr"], d["labels"], style, self.noise, self.training)
        return fake, style

    def encoder_branch(self, no_noise=False, step=None):
        """('full' | 'mini', no_noise) of a forward (sr_model.py:601-650): the guided variant always encodes the full
        image; the independent variant flips two coins per training forward.  `step`: look at the coins of that forward
        index instead of the current one (DeviceNoise only)."""
        opt = self.opt
        kw = {} if step is None else {"step": step}
        if self.model_variant == "guided":
            return "full", no_noise
        full = opt.full_style_image or (self.training and self.noise.coin("enc_full", **kw) < 0.5)
        if not no_noise:
            no_noise = self.noise.coin("enc_noise", **kw) < 0.5
        return ("full" if full else "mini"), no_noise

    def encode_style(self, d, no_noise):
        opt = self.opt
        labels, img = d["labels"], d["image_lr"]
        mode, nn_ = self.encoder_branch(no_noise)
        if self.model_variant == "guided":
            if opt.guiding_style_image:
                labels, img = d["guiding_labels"], d["guiding_image"]
            else:
                img = d["image_hr"]
            return self.netE(img, labels, mode, no_noise, self.noise, self.training)
        self.last_encoded_style_is_full = mode == "full"
        if mode == "full":
            if opt.guiding_style_image:
                labels, img = d["guiding_labels"], d["guiding_image"]
            else:
                img = d["image_hr"]
        if not no_noise:
            self.last_encoded_style_is_noisy = not nn_
        return self.netE(img, labels, mode, nn_, self.noise, self.training)
