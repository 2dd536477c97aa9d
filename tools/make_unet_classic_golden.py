"""Write tests/golden/unet_classic.npz: the reference's classic pix2pix UnetGenerator (--netG unet_128 | unet_256) run on the CPU
(TEST INFRASTRUCTURE ONLY; needs the reference tree, see oracle/ref_import.py).  No weights, inputs or Dropout masks are stored:
both sides draw them from oracle.detrand (tests/unet_classic_restated.py).

Every case of unet_classic_restated.CASES runs twice: in float64 (the judge values that are stored) and in float32 (stored only as its
per-tensor relative L2 distance to the float64 run, a JSON dict `f32/<case>`: the yardstick the GPU tests print next to their own
error).  Tensors of up to unet_classic_restated.FULL_MAX elements are stored whole, larger ones as detrand.probe triples.
`step/`: one training step of the reference's SinSKITGModel with --netG unet_256 (golden_step).

  python tools/make_unet_classic_golden.py
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_import  # noqa: E402
import unet_classic_restated as R  # noqa: E402


def level_blocks(G, nd):
    """the reference's nested UnetSkipConnectionBlocks, outermost first"""
    blocks, b = [], G.model
    for i in range(nd):
        blocks.append(b)
        if i < nd - 1:
            b = b.model[1 if i == 0 else 3]
    return blocks


def build(ref_networks, c, dtype):
    nd = R.num_downs(c["net"])
    G = ref_networks.UnetGenerator(R.INPUT_NC, R.OUTPUT_NC, nd, c["ngf"], norm_layer=ref_networks.get_norm_layer(c["norm"]),
                                   use_dropout=c["dropout"])
    shapes, _ = R.param_shapes(c)
    own = {k: tuple(v.shape) for k, v in G.state_dict().items()}
    assert list(own.items()) == [(k, tuple(s)) for k, s in shapes.items()], "state-dict keys / order / shapes differ from the restatement's"
    G.to(dtype)
    G.load_state_dict({k: (v.clone() if v.dtype == torch.long else v.to(dtype)) for k, v in R.weights(c).items()})
    # the case's own Dropout draws in place of nn.Dropout's: a forward hook replaces the module's output by input * keep * 2
    masks = R.dropout_masks(c)
    blocks = level_blocks(G, nd)
    for i, keep in masks.items():
        drop = blocks[i].model[-1]
        assert isinstance(drop, torch.nn.Dropout), (i, type(drop))
        drop.register_forward_hook(lambda m, inp, out, keep=keep: inp[0] * (keep.to(inp[0].dtype) * 2.0) if m.training else out)
    assert sum(isinstance(m, torch.nn.Dropout) for m in G.modules()) == len(masks)
    return G


def run(ref_networks, c, dtype):
    G = build(ref_networks, c, dtype)
    G.train()
    x = R.net_input(c).to(dtype)
    out = G(x)
    (out * R.cotangent(c).to(dtype)).sum().backward()
    res = {"out": out.detach()}
    res.update({"grad/" + k: p.grad.detach().clone() for k, p in G.named_parameters()})
    res.update({"buf1/" + k: v.detach().clone() for k, v in G.state_dict().items() if not R.is_param(k)})
    with torch.no_grad():
        G(x)
        res.update({"buf2/" + k: v.detach().clone() for k, v in G.state_dict().items() if not R.is_param(k)})
        G.eval()
        res["out_eval"] = G(x).detach()
    return res


def golden_step(out):
    """One SinSKITGModel.optimize_parameters of the REFERENCE with --netG unet_256 (default ngf, 256 x 256, 64 tactile patches), made
    the way oracle/make_golden.py:golden_step_variants makes its variants: losses, output probes, gradient and parameter probes and
    buffers of G, D and D2 under `step/`."""
    import random

    from oracle import detrand, nets
    from oracle import make_golden as MG
    from models.sinskitG_model import SinSKITGModel

    size, seed, nt, extra = R.STEP["size"], R.STEP["seed"], R.STEP["nt"], R.STEP["flags"]
    flags = ["--lambda_G1_lpips", "0", "--lambda_G2_lpips", "0", "--use_vision_aided_loss", "False", "--lambda_G2_GAN_feat", "0",
             "--checkpoints_dir", "/tmp/vts_golden_ckpt", "--name", "golden_unet_classic"] + extra
    opt = MG._ref_opt("sinskitG", True, flags)
    model = SinSKITGModel(opt)
    model.setup(opt)
    c = dict(net=opt.netG, ngf=opt.ngf, norm=opt.normG, dropout=not opt.no_dropout, seed=seed)
    input_nc = model.netG.state_dict()["model.model.0.weight"].shape[1]
    sdG = R.weights(c, input_nc)
    assert [(k, tuple(v.shape)) for k, v in model.netG.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sdG.items()]
    assert not c["dropout"], "the step fixture is made at the model's default --no_dropout True"
    shapesD, shapesD2 = nets.d_param_shapes(4, n_layers=opt.n_layers_D), nets.d_param_shapes(7, n_layers=opt.n_layers_D2)
    model.netG.load_state_dict(sdG)
    model.netD.load_state_dict(detrand.test_weights(shapesD, seed + 1))
    model.netD2.load_state_dict(detrand.test_weights(shapesD2, seed + 2))
    model.train()
    model.set_input(MG._synthetic_batch(size, nt, seed), phase="train")
    k = int(nets.dilated_mask_positions(model.M).shape[0])
    torch.manual_seed(seed)
    assert opt.diffaugment == "bs"
    aug = torch.stack([torch.rand(1, 1, 1, 1).flatten() for _ in range(4)])
    random.seed(seed)
    more = np.array(random.sample(range(k), opt.add_fake_T_sample_size), dtype=np.int64)[None]
    torch.manual_seed(seed)
    random.seed(seed)
    model.optimize_parameters(epoch=1)
    tag = "step"
    out[tag + "/cfg"] = np.array(json.dumps(dict(ngf=opt.ngf, norm=opt.normG, input_nc=int(input_nc), n_params=sum(p.numel() for p in model.netG.parameters()))))
    out[tag + "/aug"] = aug.numpy()
    out[tag + "/more_idx"] = more
    losses = model.get_current_losses()
    out[tag + "/loss_names"] = np.array(list(losses.keys()))
    out[tag + "/loss_values"] = np.array(list(losses.values()), dtype=np.float64)
    for nm, net in (("G", model.netG), ("D", model.netD), ("D2", model.netD2)):
        for kk, p in net.named_parameters():
            out["%s/grad_%s/%s" % (tag, nm, kk)] = detrand.probe(p.grad, kk)
            out["%s/param_%s/%s" % (tag, nm, kk)] = detrand.probe(p, kk)
        for kk, b in net.named_buffers():
            out["%s/buf_%s/%s" % (tag, nm, kk)] = b.detach().double().numpy()
    for nm, key in (("fake_I", "fake_I"), ("fake_T", "fake_T"), ("aug_fake_I", "aug_fake_I"), ("aug_real_I", "aug_real_I"),
                    ("pred_fake_T_full", "pftf"), ("pred_fake_I", "pfi")):
        out["%s/%s_probe" % (tag, nm)] = detrand.probe(getattr(model, nm), key)
    out[tag + "/aug_fake_I_sub"] = model.aug_fake_I.detach()[:, :, ::8, ::8].numpy()
    print("reference step", {k: round(float(v), 5) for k, v in losses.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=R.FIXTURE)
    args = ap.parse_args()
    ref_import.load()
    torch.set_num_threads(min(8, torch.get_num_threads()))
    import models.networks as ref_networks

    out = {}
    for name, c in R.CASES.items():
        r64 = run(ref_networks, c, torch.float64)
        r32 = run(ref_networks, c, torch.float32)
        shapes, _ = R.param_shapes(c)
        out["keys/" + name] = np.array(json.dumps([[k, list(s)] for k, s in shapes.items()]))
        zero = set(R.normed_bias_keys(c))
        top = max(v.double().norm().item() for k, v in r64.items() if k.startswith("grad/"))
        for k in zero:      # what the restatement calls identically zero is rounding noise in the reference's float64 run
            assert r64["grad/" + k].double().norm().item() < 1e-9 * top, (name, k)
        f32 = {}
        for k, v in r64.items():
            if v.dtype == torch.long:
                out["%s/%s" % (name, k)] = v.numpy()
                continue
            R.store(out, "%s/%s" % (name, k), v)
            if not (k.startswith("grad/") and k[5:] in zero):
                f32[k] = R.rel_l2(r32[k], v)
        out["f32/" + name] = np.array(json.dumps(f32))
        print(name, "out fp32 distance %.2e" % f32["out"], "worst gradient fp32 distance %.2e" % max(v for k, v in f32.items() if k.startswith("grad/")))
    golden_step(out)
    out["probes"] = np.array(json.dumps(out.get("probes", [])))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
