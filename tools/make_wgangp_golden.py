"""Generate the WGAN-GP fixtures by RUNNING THE REFERENCE on CPU in float64 (build container only; needs the reference checkout that
oracle/ref_import.py points at):

    python tools/make_wgangp_golden.py            # from the repository root

  tests/golden/sg2d_gp_32.npz               the reference's cal_gradient_penalty (models/networks.py:548-580) on its StyleGAN2Discriminator, at
      the configuration of oracle/make_golden.py:golden_sg2 (size 32, ndf 8, 4 channels, N = 3) and at size 8, 3 channels, N = 1: alpha,
      the penalty, probes of `gradients`, probes of every parameter gradient, the names of the parameters whose gradient is zero or None.
  tests/golden/sinskitG_wgangp_step_256.npz   one SinSKITGModel.optimize_parameters of the reference shaped like golden_step_sg2d plus
      --gan_mode wgangp --lambda_G2_GAN 0 (the one configuration in which the reference can train wgangp): the alpha it drew (the
      torch.rand(N, 1) of networks.py:568, captured during the step), the losses, gradient probes of G and D, sub-sampled outputs.

Inputs and weights are regenerated from seeds by committed code, so the fixtures hold seeds, configuration and recorded results only.
Condition on the inputs: every sample has | ||g_n|| - 1 | >= 0.1 (asserted): near 1 the cotangent is a difference of nearly equal
numbers and no float32 bound means anything there.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLD = os.path.join(ROOT, "tests", "golden")
MIN_GAP = 0.1

GP_CASES = [dict(tag="s32", size=32, ndf=8, input_nc=4, n=3, seed=808), dict(tag="s8", size=8, ndf=8, input_nc=3, n=1, seed=818)]


def check_gap(gradients, what):
    norms = (gradients.detach().reshape(gradients.shape[0], -1).double() + 1e-16).norm(2, dim=1)
    assert bool(((norms - 1.0).abs() >= MIN_GAP).all()), "%s: a sample's gradient norm is within %g of 1: %s" % (what, MIN_GAP, norms.tolist())
    return norms


def golden_gp():
    from oracle import detrand, ref_import, stylegan2 as sg
    from wgangp_ref import gp_inputs            # tests/wgangp_ref.py: the tests rebuild the inputs from the seed with it

    ref_import.load()
    from models import networks as RN
    from models import stylegan_networks as R

    out = {"cases": np.array([c["tag"] for c in GP_CASES]), "min_gap": MIN_GAP}
    torch.set_default_dtype(torch.float64)
    try:
        for case in GP_CASES:
            tag, size = case["tag"], case["size"]
            opt = argparse.Namespace(netD="stylegan2", D_patch_size=None, load_size=size, crop_size=size)
            D = R.StyleGAN2Discriminator(case["input_nc"], case["ndf"], 3, False, size=size, opt=opt).double()
            shapes = sg.d_param_shapes(case["input_nc"], case["ndf"], size)
            assert {k: tuple(v.shape) for k, v in D.named_parameters()} == {k: tuple(v) for k, v in shapes.items()}
            D.load_state_dict({k: v.double() for k, v in sg.test_weights(shapes, case["seed"]).items()}, strict=False)
            real, fake, alpha = (t.double() for t in gp_inputs(case))
            drawn = alpha.view(-1, 1).clone()
            rand = torch.rand
            torch.rand = lambda *a, **k: drawn.clone()           # networks.py:568 draws alpha itself: hand it the seeded one
            try:
                penalty, gradients = RN.cal_gradient_penalty(D, real, fake, torch.device("cpu"))
            finally:
                torch.rand = rand
            norms = check_gap(gradients, tag)
            grads = torch.autograd.grad(penalty, list(D.parameters()), allow_unused=True)
            zero = [k for (k, _), g in zip(D.named_parameters(), grads) if g is None or not bool(g.abs().max() > 0)]
            for k, v in case.items():
                if k != "tag":
                    out["%s/%s" % (tag, k)] = v
            out[tag + "/alpha"] = alpha.float().numpy()
            out[tag + "/penalty"] = float(penalty.detach())
            out[tag + "/norms"] = norms.numpy()
            out[tag + "/g_probe"] = detrand.probe(gradients, "gp_g")
            out[tag + "/g_sub"] = gradients.detach().view(real.shape)[:, :, ::4, ::4].numpy()
            out[tag + "/zero_grad"] = np.array(zero)
            for (k, _), g in zip(D.named_parameters(), grads):
                if k not in zero:
                    out["%s/grad/%s" % (tag, k)] = detrand.probe(g, k)
            print(tag, "penalty %.6f" % float(penalty.detach()), "norms", norms.tolist(), "zero / None:", zero)
    finally:
        torch.set_default_dtype(torch.float32)
    np.savez_compressed(os.path.join(GOLD, "sg2d_gp_32.npz"), **out)
    print("wrote sg2d_gp_32.npz (%d entries)" % len(out))


def golden_step(size=256, seed=919, nt=64):
    from oracle import detrand, nets, ref_import, stylegan2 as sg
    from oracle.make_golden import _ref_opt, _synthetic_batch

    ref_import.load()
    from models import networks as RN
    from models.sinskitG_model import SinSKITGModel

    flags = ["--lambda_G1_lpips", "0", "--lambda_G2_lpips", "0", "--use_vision_aided_loss", "False", "--lambda_G2_GAN_feat", "0",
             "--checkpoints_dir", "/tmp/vts_golden_ckpt", "--name", "golden_wgangp", "--netD", "stylegan2", "--load_size", str(size),
             "--crop_size", str(size), "--gan_mode", "wgangp", "--lambda_G2_GAN", "0"]
    opt = _ref_opt("sinskitG", True, flags)
    torch.set_default_dtype(torch.float64)
    try:
        model = SinSKITGModel(opt)
        model.setup(opt)
        assert model.model_names == ["G", "D"]
        shapesD = sg.d_param_shapes(4, opt.ndf, size)
        model.netG.load_state_dict({k: v.double() if v.dtype.is_floating_point else v for k, v in detrand.test_weights(nets.g_param_shapes(), seed).items()})
        model.netD.load_state_dict({k: v.double() for k, v in sg.test_weights(shapesD, seed + 1).items()}, strict=False)
        model.netG.double()
        model.netD.double()
        model.train()
        batch = _synthetic_batch(size, nt, seed)
        batch = {k: (v.double() if torch.is_tensor(v) and v.dtype == torch.float32 else v) for k, v in batch.items()}
        out = {"size": size, "seed": seed, "nt": nt, "ndf": opt.ndf, "flags": json.dumps(flags)}
        model.set_input(batch, phase="train")
        torch.manual_seed(seed)
        out["aug"] = torch.stack([torch.rand(1, 1, 1, 1).flatten() for _ in range(4)]).float().numpy()
        seen = {}
        cal = RN.cal_gradient_penalty

        def spy(netD, real, fake, device, **kw):
            rand = torch.rand

            def rand_spy(*a, **k):
                seen["alpha"] = rand(*a, **k)
                return seen["alpha"]

            torch.rand = rand_spy
            try:
                pen, gradients = cal(netD, real, fake, device, **kw)
            finally:
                torch.rand = rand
            seen["gradients"] = gradients.detach()
            return pen, gradients

        RN.cal_gradient_penalty = spy
        torch.manual_seed(seed)
        try:
            model.optimize_parameters(epoch=1)
        finally:
            RN.cal_gradient_penalty = cal
    finally:
        torch.set_default_dtype(torch.float32)
    out["gp_alpha"] = seen["alpha"].reshape(-1).numpy()          # float64: the test hands the model its float32 rounding
    out["gp_norms"] = check_gap(seen["gradients"], "step").numpy()
    out["gp_g_probe"] = detrand.probe(seen["gradients"], "gp_g")
    losses = model.get_current_losses()
    assert losses["l_D_I_grad_penalty"] != 0.0
    out["loss_names"] = np.array(list(losses.keys()))
    out["loss_values"] = np.array(list(losses.values()), dtype=np.float64)
    for nm, net in (("G", model.netG), ("D", model.netD)):
        for kk, p in net.named_parameters():
            out["grad_%s/%s" % (nm, kk)] = detrand.probe(p.grad, kk)
    out["fake_I_sub"] = model.fake_I.detach()[:, :, ::4, ::4].float().numpy()
    out["pred_fake_I"] = model.pred_fake_I.detach().float().numpy()
    np.savez_compressed(os.path.join(GOLD, "sinskitG_wgangp_step_%d.npz" % size), **out)
    print("wrote sinskitG_wgangp_step_%d.npz (%d entries)" % (size, len(out)))
    print({k: float(v) for k, v in losses.items()}, "alpha", out["gp_alpha"], "norms", out["gp_norms"])


if __name__ == "__main__":
    which = sys.argv[1:] or ["gp", "step"]
    if "gp" in which:
        golden_gp()
    if "step" in which:
        golden_step()
