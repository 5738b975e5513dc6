"""The GAN objective (opt.gan_mode = ls / original / w / hinge) on the host: the mode table sr_model.gan_loss_modes builds,
the reference's ValueError for any other value, and the substituted oracle (tools/gen_golden_gan_mode.py) against fixtures
written from the REAL reference (tests/golden/gan_mode/*.json).  CPU only."""
import glob
import json
import os
import random

import pytest
import torch

from deepsee_amd import ops
from deepsee_amd.sr_model import gan_loss_modes
from oracle import deepsee_oracle as O
from tools.gen_golden_gan_mode import CASES as GEN_CASES, install_gan_mode
from tools.gen_golden_nonspade_norm import install_nonspade_norm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gan_mode")
CASES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLD, "*.json")))


@pytest.mark.parametrize("gan_mode,want", [
    ("hinge", (ops.MODE_NEG, ops.MODE_HINGE_REAL, ops.MODE_HINGE_FAKE)),
    ("w", (ops.MODE_NEG, ops.MODE_NEG, ops.MODE_W_FAKE)),
    ("ls", (ops.MODE_LS_REAL, ops.MODE_LS_REAL, ops.MODE_LS_FAKE)),
    ("original", (ops.MODE_BCE_REAL, ops.MODE_BCE_REAL, ops.MODE_BCE_FAKE))])
def test_gan_loss_modes_table(gan_mode, want):
    assert gan_loss_modes(gan_mode) == want


def test_mode_constants_are_the_c_abi_numbers():
    assert (ops.MODE_L1, ops.MODE_NEG, ops.MODE_HINGE_REAL, ops.MODE_HINGE_FAKE) == (0, 1, 2, 3)
    assert (ops.MODE_W_FAKE, ops.MODE_LS_REAL, ops.MODE_LS_FAKE, ops.MODE_BCE_REAL, ops.MODE_BCE_FAKE) == (4, 5, 6, 7, 8)


@pytest.mark.parametrize("gan_mode", ["LS", "wgan", "", "hinge ", "Original", None])
def test_unknown_gan_mode_raises_like_the_reference(gan_mode):
    with pytest.raises(ValueError, match="^Unexpected gan_mode %s$" % gan_mode):
        gan_loss_modes(gan_mode)


def test_fixtures_present():
    assert CASES == sorted(GEN_CASES), CASES
    modes = {json.load(open(os.path.join(GOLD, c + ".json")))["opt"]["gan_mode"] for c in CASES}
    assert modes == {"ls", "original", "w"}, modes


@pytest.mark.parametrize("case", CASES)
def test_gan_mode_oracle_matches_reference_fixture(case, monkeypatch):
    """The substituted oracle (the yardstick of tests/test_gpu_gan_mode.py) reproduces the reference's inference /
    encode_only / demo outputs, G+D step losses, gradients and post-step state, with the bounds of
    tests/test_oracle_golden.py (those of tests/test_nonspade_norm_host.py)."""
    from tests import test_oracle_golden as TG
    install_nonspade_norm(monkeypatch.setattr)
    install_gan_mode(monkeypatch.setattr)
    monkeypatch.setattr(TG, "GOLD", GOLD)
    TG.test_oracle_matches_reference_fixture(case)


def test_fixture_losses_are_not_the_hinge_losses(monkeypatch):
    """The fixtures pin the selected objective: with the hinge term the oracle misses every fixture's D losses."""
    from tests import test_oracle_golden as TG
    install_nonspade_norm(monkeypatch.setattr)
    for case in CASES:
        rec = json.load(open(os.path.join(GOLD, case + ".json")))
        opt = O.make_opt(**dict(rec["opt"], gan_mode="hinge"))
        orc = O.Oracle(opt, O.recipe_state(opt, gain=1.0))
        orc.create_optimizers()
        batch = O.synthetic_batch(opt, rec["n"], seed=rec["batch_seed"])
        random.seed(rec["rng_seed"])
        torch.manual_seed(rec["rng_seed"])
        orc.run_generator_one_step({k: v.clone() for k, v in batch.items()})
        dl = orc.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
        want = rec["iters"][0]["d_losses"]
        assert any(abs(float(dl[k].detach()) - v) > 10 * TG.TOL_DLOSS * abs(v) for k, v in want.items()), (case, want)


def _hinge_step(case):
    opt = O.make_opt(**dict(GEN_CASES[case]["opt"], gan_mode="hinge"))
    orc = O.Oracle(opt, O.recipe_state(opt, gain=1.0))
    orc.create_optimizers()
    batch = O.synthetic_batch(opt, 2, seed=7)
    random.seed(3)
    torch.manual_seed(3)
    out = []
    for _ in range(2):
        gl, fake = orc.run_generator_one_step({k: v.clone() for k, v in batch.items()})
        dl = orc.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
        out.append(([gl[k].detach().clone() for k in gl] + [fake.detach().clone()] + [dl[k].detach().clone() for k in dl]))
    return out, {net: {k: v.detach().clone() for k, v in orc.S[net].items()} for net in ("SR", "D", "E")}


@pytest.mark.parametrize("case", ["indep_w_4to32_bs2_ngf8", "guided_original_4to32_bs2_ngf8"])
def test_substituted_hinge_is_bit_identical(case, monkeypatch):
    """With gan_mode = 'hinge' the substituted oracle equals the unsubstituted one bit for bit over two G+D iterations:
    losses, generated images and every post-step parameter and buffer."""
    plain, plain_state = _hinge_step(case)
    install_gan_mode(monkeypatch.setattr)
    subst, subst_state = _hinge_step(case)
    for a, b in zip(plain, subst):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for net in plain_state:
        assert set(plain_state[net]) == set(subst_state[net])
        assert all(torch.equal(plain_state[net][k], subst_state[net][k]) for k in plain_state[net]), net


def test_substituted_oracle_refuses_an_unknown_mode(monkeypatch):
    install_gan_mode(monkeypatch.setattr)
    opt = O.make_opt(start_size=4, crop_size=32, load_size=32, batchSize=2, ngf=8, gan_mode="LS")
    orc = O.Oracle(opt, O.recipe_state(opt, gain=1.0))
    batch = O.synthetic_batch(opt, 2, seed=7)
    with pytest.raises(ValueError, match="Unexpected gan_mode LS"):
        orc.run_discriminator_one_step(batch)
