"""The class count through the options and the model build, on the host: semantic_nc is derived from label_nc and
contain_dontcare_label in both make_opt functions, every consumer takes semantic_nc, and more than 32 classes fail where the model
(or a label map) is built -- in Python and behind the C ABI -- never in the middle of a pass.  Nothing here launches a kernel."""
import ctypes

import pytest
import torch

from oracle import deepsee_oracle as O


def _make_opts():
    from deepsee_amd.options import make_opt
    return [make_opt, O.make_opt]


def test_semantic_nc_is_derived_in_both_make_opt():
    for make_opt in _make_opts():
        assert make_opt().semantic_nc == 19 and make_opt().label_nc == 19
        assert make_opt(label_nc=12).semantic_nc == 12
        assert make_opt(contain_dontcare_label=True).semantic_nc == 20
        assert make_opt(label_nc=5, contain_dontcare_label=True).semantic_nc == 6
        assert make_opt(label_nc=5, contain_dontcare_label=True, semantic_nc=6).semantic_nc == 6     # (consistent: accepted)
        for bad in (dict(label_nc=12, semantic_nc=19), dict(contain_dontcare_label=True, semantic_nc=19), dict(semantic_nc=20)):
            with pytest.raises(ValueError, match="semantic_nc"):
                make_opt(**bad)


def test_specs_and_modules_follow_semantic_nc():
    """The generator's shared SPADE layers and D's first convolution are sized by semantic_nc (label_nc + 1 with a dontcare label:
    what ops.DInput writes for a Labels of that count), in the oracle's specs and in the modules alike."""
    from deepsee_amd import networks as N
    from deepsee_amd.options import make_opt
    over = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8, ndf=8)
    for extra, nc in [(dict(), 19), (dict(contain_dontcare_label=True), 20), (dict(label_nc=5), 5),
                      (dict(label_nc=5, contain_dontcare_label=True), 6), (dict(label_nc=32), 32)]:
        oopt, opt = O.make_opt(**over, **extra), make_opt(**over, **extra)
        assert oopt.semantic_nc == opt.semantic_nc == nc
        sr = O.sr_spec(oopt)
        shared = [v for k, v in sr.items() if k.endswith("mlp_shared.0.weight")]
        assert shared and all(v[1] == nc for v in shared)
        d = O.d_spec(oopt)
        first = [v for k, v in d.items() if k.endswith("model0.0.weight") or k.endswith("model0.0.weight_orig")]
        assert first and all(v[1] == nc + 3 for v in first)
        blk = N.SpadeNorm("sean", 8, opt.semantic_nc, 128, 256)
        assert blk.state_dict()["mlp_shared.0.weight"].shape[1] == nc
        batch = O.synthetic_batch(oopt, 2, seed=3)
        assert int(batch["label"].max()) == nc - 1          # (16 x 16 cells x 2: every value of [0, semantic_nc) occurs)
        assert tuple(O.Oracle(oopt, O.recipe_state(oopt, gain=1.0)).preprocess(batch)["input_semantics"].shape) == (2, nc, 32, 32)


def test_more_than_32_classes_fail_at_build():
    from deepsee_amd import ops
    from deepsee_amd.options import make_opt
    from deepsee_amd.sr_model import SRModel
    for over in (dict(label_nc=33), dict(label_nc=32, contain_dontcare_label=True)):
        with pytest.raises(ValueError, match="32 columns"):
            SRModel(make_opt(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8, **over))
    lab = torch.zeros(1, 4, 4, dtype=torch.uint8)
    assert ops.Labels(lab, 32).nc == 32 and ops.Labels(lab, 1).nc == 1
    for bad in (0, 33, 256):
        with pytest.raises(ValueError, match="32 columns"):
            ops.Labels(lab, bad)


def test_dontcare_label_with_a_label_nc_sized_encoder_input_is_refused_at_build():
    """The reference cannot train with contain_dontcare_label and the style corruption (label_nc noise weights indexed by
    semantic_nc rows, encoder.py:54-56) or random_style_matrix (randn(N, semantic_nc, ..) * seg into a convolution with label_nc
    inputs, encoder.py:78,119): it raises in its first forward pass.  Here the encoder refuses at build; without either the encoder builds."""
    from deepsee_amd import networks as N
    from deepsee_amd.options import make_opt
    base = dict(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8, nef=4, contain_dontcare_label=True)
    with pytest.raises(ValueError, match="noisy_style_scale=0"):
        N.StyleEncoder(make_opt(**base))
    with pytest.raises(ValueError, match="noisy_style_scale=0"):
        N.StyleEncoder(make_opt(**base, noisy_style_scale=0.0, netE="fullstyle", random_style_matrix=True))
    enc = N.StyleEncoder(make_opt(**base, noisy_style_scale=0.0))
    assert not hasattr(enc, "noise_weights")


def test_coarse_entry_points_reject_more_than_32_classes_with_and_without_table():
    """dsee_sean_norm_fwd and the two training entry points of the residual block (block_args_ok) return DSEE_EUNSUPPORTED for
    label_nc = 33 whether or not there is a style table, at shapes they otherwise accept, before they touch a pointer."""
    from deepsee_amd import lib as L
    so = L.lib()
    one = ctypes.c_void_p(4096)                       # non-null, never dereferenced
    for table in (None, one):
        for nc in (33, 0):
            rc = so.dsee_sean_norm_fwd(one, 32, 32, 0, nc, one, one, one, table, one, one, one, one, 1, 1e-5, 0.1, 1.0, 0.2, one, one,
                                       one, one, one, one, 2, 32, 32, 64, one, 1 << 40, None)
            assert rc != 0 and b"label_nc = %d" % nc in so.dsee_last_error(), (table, nc, so.dsee_last_error())
            assert nc == 0 or b"32" in so.dsee_last_error()
    # the block entry points read `table` out of a host struct: all-zero bytes (SPADE) and all-non-zero bytes (SEAN)
    for fill in (b"\x00", b"\x40"):
        norm = ctypes.create_string_buffer(fill * 512, 512)
        np_ = ctypes.cast(norm, ctypes.c_void_p)
        rc = so.dsee_spade_resblock_train_fwd(np_, one, one, np_, one, one, None, one, 128, 128, 0, 33, one, one, 1e-5, 0.1, 0.2,
                                              4, 128, 128, 256, one, 1 << 40, one, 1 << 40, None)
        assert rc != 0 and b"dsee_spade_resblock_train_fwd: label_nc = 33" in so.dsee_last_error(), so.dsee_last_error()
        rc = so.dsee_spade_resblock_bwd(np_, one, np_, one, None, one, 128, 128, 0, 33, one, one, one, np_, one, one, 0.2,
                                        4, 128, 128, 256, one, 1 << 40, one, 1 << 40, None)
        assert rc != 0 and b"dsee_spade_resblock_bwd: label_nc = 33" in so.dsee_last_error(), so.dsee_last_error()
