"""--gan_mode wgangp, the host side (no GPU needed).

The fixture tests/golden/sg2d_gp_32.npz is the reference's cal_gradient_penalty (models/networks.py:548-580, autograd's double backward) on
its own StyleGAN2Discriminator in float64 (tools/make_wgangp_golden.py).  Here the forward-over-reverse form the HIP engine runs
(tests/wgangp_ref.py: first-order passes only, on oracle/stylegan2.py's blocks) reproduces its penalty, `gradients` and every
parameter-gradient probe at 1e-10 in float64: that guards the fixture and documents the identity.  Then the option check of the models."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import wgangp_ref as W
from oracle import detrand
from oracle import stylegan2 as sg

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = "--model %s --checkpoints_dir /tmp/vts_test_ckpt --name wgangp_cpu"
TOL = 1e-10


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "sg2d_gp_32.npz"), allow_pickle=False)


def case_of(gold, tag):
    return {k: int(gold["%s/%s" % (tag, k)]) for k in ("size", "ndf", "input_nc", "n", "seed")}


def close(got, ref, scale=None):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(got - ref) <= TOL * max(1.0, float(np.abs(ref).max()) if scale is None else scale)))


@pytest.mark.parametrize("tag", ["s32", "s8"])
def test_forward_over_reverse_reproduces_the_reference_double_backward(gold, tag):
    case = case_of(gold, tag)
    assert tag in [str(t) for t in gold["cases"]]
    real, fake, alpha = W.gp_inputs(case)
    assert np.array_equal(alpha.numpy(), gold[tag + "/alpha"])
    sd = sg.test_weights(sg.d_param_shapes(case["input_nc"], case["ndf"], case["size"]), case["seed"])
    xh = W.interpolate(real.double(), fake.double(), alpha.double())
    pen, g, grads, norms = W.penalty_forward_over_reverse(sd, xh, case["size"])
    assert close(float(pen), float(gold[tag + "/penalty"]))
    assert close(norms.numpy(), gold[tag + "/norms"])
    assert bool((np.abs(gold[tag + "/norms"] - 1.0) >= float(gold["min_gap"])).all())      # the fixture's condition on its inputs
    assert close(detrand.probe(g, "gp_g"), gold[tag + "/g_probe"]) and close(g[:, :, ::4, ::4].numpy(), gold[tag + "/g_sub"])
    stored = sorted(k[len(tag) + 6:] for k in gold.files if k.startswith(tag + "/grad/"))
    assert stored == sorted(grads) and len(stored) >= 7
    for k in stored:
        ref = gold["%s/grad/%s" % (tag, k)]
        assert ref[1] > 0 and close(detrand.probe(grads[k], k), ref, scale=max(1.0, float(ref[1]))), k
    # ... and autograd's double backward on the oracle's blocks says the same (the oracle is the reference's restatement)
    pen2, g2, grads2, _ = W.penalty_autograd(sd, xh, case["size"])
    assert close(float(pen2), float(pen)) and close(g2.numpy(), g.numpy())
    for k in stored:
        assert float((grads2[k] - grads[k]).norm() / grads[k].norm()) < TOL, k


@pytest.mark.parametrize("tag", ["s32", "s8"])
def test_the_zero_gradient_parameters_are_exactly_the_biases(gold, tag):
    case = case_of(gold, tag)
    shapes = sg.d_param_shapes(case["input_nc"], case["ndf"], case["size"])
    zero = [str(k) for k in gold[tag + "/zero_grad"]]
    assert sorted(zero) == sorted(k for k in shapes if k.endswith("bias")) and len(zero) + len(
        [k for k in gold.files if k.startswith(tag + "/grad/")]) == len(shapes)


# ---------------------------------------------------------------------------------------------------------------- the option check
def parse(model="sinskitG", extra="", train=True):
    from options.test_options import TestOptions
    from options.train_options import TrainOptions

    with contextlib.redirect_stdout(io.StringIO()):
        return (TrainOptions if train else TestOptions)(cmd_line=(FLAGS % model) + extra).parse()


WGANGP = " --gan_mode wgangp"


@pytest.mark.parametrize("model", ["sinskitG", "skitG"])
def test_wgangp_accepts_the_one_configuration_the_reference_trains(model):
    from models import find_model_using_name

    cls = find_model_using_name(model)
    g = np.load(os.path.join(HERE, "golden", "sinskitG_wgangp_step_256.npz"), allow_pickle=False)
    flags = json.loads(str(g["flags"]))
    assert flags[flags.index("--gan_mode") + 1] == "wgangp" and flags[flags.index("--lambda_G2_GAN") + 1] == "0"
    drop = ("--checkpoints_dir", "--name")
    extra = " ".join(f for i, f in enumerate(flags) if f not in drop and (i == 0 or flags[i - 1] not in drop))
    cls._check_wgangp(parse(model, " " + extra))
    cls._check_wgangp(parse(model, WGANGP + " --netD stylegan2 --lambda_G2_GAN 0"))
    cls._check_wgangp(parse(model))                                        # the defaults: not wgangp, nothing to check
    cls._check_wgangp(parse(model, WGANGP, train=False))                   # inference builds no discriminator


def test_wgangp_refuses_a_multiscale_image_discriminator():
    from models.sinskitG_model import SinSKITGModel

    with pytest.raises(NotImplementedError, match=r"--netD multiscale.*networks\.py:576"):
        SinSKITGModel._check_wgangp(parse(extra=WGANGP + " --lambda_G2_GAN 0"))


def test_wgangp_refuses_the_default_multiscale_tactile_discriminator():
    from models.sinskitG_model import SinSKITGModel

    with pytest.raises(NotImplementedError, match=r"tactile discriminator \(--netD2 multiscale\).*networks\.py:576"):
        SinSKITGModel._check_wgangp(parse(extra=WGANGP + " --netD stylegan2"))


def test_wgangp_refuses_a_stylegan2_tactile_discriminator_on_patches():
    from models.sinskitG_model import SinSKITGModel

    with pytest.raises(NotImplementedError, match=r"--netD2 stylegan2.*stylegan_networks\.py:181"):
        SinSKITGModel._check_wgangp(parse(extra=WGANGP + " --netD stylegan2 --netD2 stylegan2"))


def test_pix2pix_still_refuses_wgangp():
    from models.pix2pix_model import Pix2PixModel

    with pytest.raises(NotImplementedError, match="not built: gan_mode wgangp"):
        Pix2PixModel._check_unbuilt(parse("pix2pix", WGANGP))
