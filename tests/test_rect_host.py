"""The oracle at the rectangular (H != W) shapes the GPU tests lean on, against plain float64 torch.  tests/golden pins the oracle to
the reference at square fixtures only; a transposed index in one of these helpers would pass there and then let a GPU kernel with
the same mistake through.  Both orientations, label maps at 1x and 2x / 4x the feature size (nearest resize = strided pick)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import deepsee_oracle as O

LC = 19


def _labels(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    # (an asymmetric pattern on top of the noise: rows and columns are distinguishable, so is a flip)
    lab = torch.randint(0, LC, (n, 1, h, w), generator=g)
    lab[:, :, : h // 3] = 3
    lab[:, :, :, : w // 5] = 7
    return lab.float()


@pytest.mark.parametrize("h,w", [(24, 40), (46, 50), (48, 96), (32, 64), (64, 32)])
def test_onehot_labels(h, w):
    lab = _labels(2, h, w, h + w)
    want = F.one_hot(lab[:, 0].long(), LC).permute(0, 3, 1, 2).double()
    got = O.onehot_labels(lab, LC, torch.float64)
    assert got.shape == (2, LC, h, w) and torch.equal(got, want)


@pytest.mark.parametrize("lh,lw,fh,fw", [(32, 64, 16, 32), (64, 32, 64, 32), (64, 32, 16, 8)])
def test_style_pool_is_the_masked_mean_after_a_nearest_resize(lh, lw, fh, fw):
    n, c = 2, 128
    g = torch.Generator().manual_seed(lh + fw)
    lab = _labels(n, lh, lw, lh * fw)
    feat = torch.randn(n, c, fh, fw, generator=g, dtype=torch.float64)
    step = lh // fh
    assert lw // fw == step
    small = lab[:, 0, ::step, ::step].long()                        # nearest: src = floor(dst * in / out) = step * dst
    want = torch.zeros(n, LC, c, dtype=torch.float64)
    for b in range(n):
        for r in range(LC):
            want[b, r] = (feat[b] * (small[b] == r)).sum((1, 2)) / (fh * fw)     # divided by H W, not by the region's area
    got = O.style_pool(feat, O.onehot_labels(lab, LC, torch.float64))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("c,rh,rw,lh,lw", [(8, 16, 8, 64, 32), (64, 64, 32, 128, 64), (64, 8, 16, 32, 64)])
def test_spade_norm_is_batchnorm_conv_modulate(c, rh, rw, lh, lw):
    n = 2
    g = torch.Generator().manual_seed(c + rh)
    lab = _labels(n, lh, lw, rh * lw)
    x = torch.randn(n, c, rh, rw, generator=g, dtype=torch.float64) * 2 + 0.5
    spec = {"n.param_free_norm.running_mean": (c,), "n.param_free_norm.running_var": (c,),
            "n.param_free_norm.num_batches_tracked": (), "n.mlp_shared.0.weight": (128, LC, 3, 3), "n.mlp_shared.0.bias": (128,),
            "n.mlp_gamma.weight": (c, 128, 3, 3), "n.mlp_gamma.bias": (c,), "n.mlp_beta.weight": (c, 128, 3, 3),
            "n.mlp_beta.bias": (c,)}
    st = {k: O.recipe_tensor("rect_spade", k, s, 1.0) for k, s in spec.items()}
    orc = O.Oracle(O.make_opt(), {"SR": st}, dtype=torch.float64)
    got = orc._norm("spade", orc.S["SR"], "n", x, O.onehot_labels(lab, LC, torch.float64), None)
    p = {k: v.double() for k, v in st.items() if v.is_floating_point()}
    step = lh // rh
    seg = F.one_hot(lab[:, 0, ::step, ::step].long(), LC).permute(0, 3, 1, 2).double()
    xn = F.batch_norm(x, None, None, training=True, eps=O.BN_EPS)
    actv = F.relu(F.conv2d(seg, p["n.mlp_shared.0.weight"], p["n.mlp_shared.0.bias"], padding=1))
    gamma = F.conv2d(actv, p["n.mlp_gamma.weight"], p["n.mlp_gamma.bias"], padding=1)
    beta = F.conv2d(actv, p["n.mlp_beta.weight"], p["n.mlp_beta.bias"], padding=1)
    want = xn * (1 + gamma) + beta
    assert got.shape == want.shape == (n, c, rh, rw)
    assert float((got.detach() - want).abs().max()) <= 1e-11 * float(want.abs().max())


def test_labels_shift_checks_both_axes():
    """ops.Labels.shift_for: a feature map that is not the same power-of-two fraction of the label map on both axes raises (the label
    kernels would otherwise index past a row); the one-argument form keeps meaning "the same fraction of the width"."""
    from deepsee_amd import ops
    labels = ops.Labels(torch.zeros(2, 32, 64, dtype=torch.uint8), LC)
    assert labels.shift_for(32, 64) == 0 and labels.shift_for(16, 32) == 1 and labels.shift_for(8, 16) == 2
    assert labels.shift_for(16) == 1
    for r, rw in ((16, 16), (16, 64), (32, 32), (8, 32)):
        with pytest.raises(AssertionError):
            labels.shift_for(r, rw)
    with pytest.raises(AssertionError):
        labels.shift_for(12, 24)
