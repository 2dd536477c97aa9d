"""Write tests/golden/pix2pix_step_32.npz and tests/golden/pix2pix_option_defaults.json: the reference's Pix2PixModel (models/pix2pix_model.py)
run on the CPU for two optimize_parameters calls per case, and its parser's defaults in both phases (TEST INFRASTRUCTURE ONLY; needs the
reference tree, see oracle/ref_import.py).  No weights are stored: both sides draw them from seeds (oracle.detrand.test_weights) over the
key / shape lists the fixture records; the `filt` buffers of the anti-aliasing modules are constants and stay as constructed.

Cases, all at --ngf 8 --ndf 8 --batch_size 4 on 32 x 32 patches:
        default  no further flags                  (resnet_9blocks, anti-aliased, netD basic, vanilla, lambda_L1 100)
        B        --netD n_layers --n_layers_D 2 --gan_mode lsgan --netG resnet_6blocks --no_antialias --no_antialias_up --lambda_L1 10

Every case runs in float64 (the judge values that are stored) and in float32 (stored only as its distance to the float64 run, a JSON dict
`f32/<case>/s<step>`: relative L2 per tensor, absolute difference per loss -- the yardstick the GPU tests print next to their own error).
For the float64 run the tactile tensors, which the reference's set_input forces to float32, are cast on the model after set_input.
Per case an eval-mode inference record on both input contracts: the 32 x 32 patches, and one 48 x 40 image with three tactile patches
(for which the tactile mask M_T, which the reference can only make for square images, is set to the mask itself: see feed()).

  python tools/make_pix2pix_step_golden.py
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import detrand, ref_import  # noqa: E402
from oracle.make_option_fixture import dump as dump_options  # noqa: E402

SIZE, N, STEPS = 32, 4, 2
FULL_H, FULL_W, FULL_NT = 48, 40, 3
BASE = ["--model", "pix2pix", "--ngf", "8", "--ndf", "8", "--batch_size", "4"]
CASES = {
    "default": dict(flags=BASE, seed=925),
    "B": dict(flags=BASE + ["--netD", "n_layers", "--n_layers_D", "2", "--gan_mode", "lsgan", "--netG", "resnet_6blocks", "--no_antialias",
                            "--no_antialias_up", "--lambda_L1", "10"], seed=935),
}
NETS = ("G", "D", "D2")


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def ellipse(n, h, w):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return (((yy - h / 2) / (0.45 * h)) ** 2 + ((xx - w / 2) / (0.4 * w)) ** 2 <= 1).float()[None, None].repeat(n, 1, 1, 1)


def p2p_batch(n, size, seed):
    """synthetic patch batch with the patchskit contract (return_patch=True): what tools/make_spade_step_golden.py:p2p_batch builds"""
    return {"S_images": detrand.uniform((n, 1, size, size), seed, "S"), "M_images": ellipse(n, size, size),
            "I_images": detrand.uniform((n, 3, size, size), seed, "I"), "T_images": 0.3 * detrand.uniform((n, 2, size, size), seed, "T"),
            "I_masks": torch.ones(n, size, size, dtype=torch.float64), "name": ["synthetic"] * n, "S_paths": ["synthetic.png"] * n,
            "augmentation_params": {}}


def full_batch(h, w, nt, size, seed):
    """one full image with nt tactile patches (return_patch=False): S / M / I, 5-D T_images, T_coords and full_T_coords"""
    coords = torch.tensor([[[4 * k, 2 * k, 4 * k + size, 2 * k + size, 0, 0, 0, 0] for k in range(nt)]], dtype=torch.float32)
    return {"S": detrand.uniform((1, 1, h, w), seed, "fS"), "M": ellipse(1, h, w), "I": detrand.uniform((1, 3, h, w), seed, "fI"),
            "T_images": 0.3 * detrand.uniform((1, nt, 2, size, size), seed, "fT"), "I_masks": torch.ones(1, nt, size, size, dtype=torch.float64),
            "T_coords": coords, "full_T_coords": coords.clone(), "name": ["synthetic"], "S_paths": ["synthetic.png"], "augmentation_params": {}}


def ref_opt(is_train, flags):
    from options.test_options import TestOptions
    from options.train_options import TrainOptions
    import models

    o = (TrainOptions if is_train else TestOptions)()
    parser = o.initialize(argparse.ArgumentParser())
    parser = models.get_option_setter("pix2pix")(parser, is_train)
    opt, _ = parser.parse_known_args(list(flags))
    opt.isTrain = is_train
    opt.gpu_ids = []
    return opt


def build(case, is_train=True):
    import models

    opt = ref_opt(is_train, CASES[case]["flags"])
    opt.checkpoints_dir, opt.name = "/tmp/vts_golden_ckpt", "pix2pix_" + case
    os.makedirs(os.path.join(opt.checkpoints_dir, opt.name), exist_ok=True)
    model = models.create_model(opt)
    if is_train:
        model.setup(opt)
    return model, opt


def seed_weights(model, seed, dtype):
    keys = {}
    for i, nm in enumerate(NETS):
        net = getattr(model, "net" + nm)
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        # (the anti-aliasing modules register their fixed blur kernel as a buffer `filt`: a constant, kept as constructed)
        sd = detrand.test_weights({k: s for k, s in shapes.items() if not k.endswith(".filt")}, seed + i)
        net.load_state_dict({k: (v.clone() if v.dtype == torch.long else v.to(dtype)) for k, v in sd.items()}, strict=False)
        assert set(shapes) - set(sd) == {k for k in shapes if k.endswith(".filt")}
        keys[nm] = [[k, list(s)] for k, s in shapes.items()]
    return keys


def feed(model, batch, dtype):
    model.set_input({k: (v.to(dtype) if torch.is_tensor(v) and v.dtype.is_floating_point else v) for k, v in batch.items()}, phase="train")
    for k in ("real_T", "I_masks"):          # set_input forces these to float32
        setattr(model, k, getattr(model, k).to(dtype))
    model.real_gx, model.real_gy = model.real_T[:, 0:1], model.real_T[:, 1:2]
    if model.M.shape[-2] != model.M.shape[-1]:
        # set_input resizes the mask to the SQUARE M.shape[-1] x M.shape[-1] for the tactile output (pix2pix_model.py:322), which at
        # T_resolution_multiplier 1 is the mask itself on the square images of the dataset and a shape error on any other: the mask itself
        model.M_T = model.M


def run_case(case, dtype):
    from models.model_utils import compute_normal

    torch.set_default_dtype(dtype)
    try:
        c = CASES[case]
        model, opt = build(case)
        keys = seed_weights(model, c["seed"], dtype)
        batch = p2p_batch(N, SIZE, c["seed"])
        res = {"keys": keys, "opt": opt, "eval": {}}
        model.eval()
        feed(model, batch, dtype)
        model.test()
        res["eval"]["patch"] = {k: getattr(model, k).detach().clone() for k in ("fake_I", "fake_T", "fake_N")}
        assert torch.equal(model.fake_N, compute_normal(model.fake_T, scale_nz=opt.scale_nz))
        opt.return_patch = False
        feed(model, full_batch(FULL_H, FULL_W, FULL_NT, SIZE, c["seed"]), dtype)
        model.test()
        res["eval"]["full"] = {k: getattr(model, k).detach().clone() for k in ("fake_I", "fake_T", "fake_N")}
        res["eval"]["full_real_T_shape"] = list(model.real_T.shape)
        opt.return_patch = True
        model.train()
        res["steps"] = []
        for it in range(STEPS):
            feed(model, batch, dtype)
            model.optimize_parameters(epoch=1)
            st = {"losses": {k: float(v) for k, v in model.get_current_losses().items()},
                  "fake_I": model.fake_I.detach().clone(), "fake_T": model.fake_T.detach().clone(), "grad": {}, "param": {}, "buf": {}}
            for nm in NETS:
                net = getattr(model, "net" + nm)
                st["grad"][nm] = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
                st["param"][nm] = {k: p.detach().clone() for k, p in net.named_parameters()}
                st["buf"][nm] = {k: b.detach().clone() for k, b in net.named_buffers()}
            res["steps"].append(st)
        res["names"] = {"loss_names": list(model.loss_names), "visual_names": list(model.visual_names), "model_names": list(model.model_names)}
        model.update_learning_rate()
        res["lrs"] = [o.param_groups[0]["lr"] for o in (model.optimizer_G, model.optimizer_D, model.optimizer_D2)]
        return res
    finally:
        torch.set_default_dtype(torch.float32)


def zero_grad_names(grads):
    """the tensors whose gradient norm is below 1e-9 of the largest in their network"""
    norms = {k: g.double().norm().item() for k, g in grads.items()}
    top = max(norms.values())
    return [k for k, v in norms.items() if v < 1e-9 * top]


def test_phase_names():
    """the name lists of a test-phase model.  The reference's constructor builds optimisers over netD in both phases (pix2pix_model.py:281-286)
    and reads opt.gan_mode (:226), which only the training options declare: where it cannot be constructed, the lists are read off the
    assignments the constructor had made by then."""
    import models

    opt = ref_opt(False, BASE)
    opt.checkpoints_dir, opt.name = "/tmp/vts_golden_ckpt", "pix2pix_test"
    cls = models.find_model_using_name("pix2pix")
    m = cls.__new__(cls)
    try:
        cls.__init__(m, opt)
        how = "constructed"
    except AttributeError as e:
        how = "constructor stopped: %s" % e
    return {"loss_names": list(m.loss_names), "visual_names": list(m.visual_names), "model_names": list(m.model_names)}, how


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pix2pix_step_32.npz"))
    ap.add_argument("--opts_out", default=os.path.join(ROOT, "tests", "golden", "pix2pix_option_defaults.json"))
    args = ap.parse_args()
    ref_import.load()
    torch.set_num_threads(min(8, torch.get_num_threads()))
    out = {"size": SIZE, "n": N, "steps": STEPS, "full": np.array([FULL_H, FULL_W, FULL_NT])}
    for case, c in CASES.items():
        r64, r32 = run_case(case, torch.float64), run_case(case, torch.float32)
        out[case + "/seed"] = c["seed"]
        out[case + "/flags"] = np.array(json.dumps(c["flags"]))
        out[case + "/keys"] = np.array(json.dumps(r64["keys"]))
        out[case + "/names"] = np.array(json.dumps(r64["names"]))
        out[case + "/lrs_after_update"] = np.array(r64["lrs"], dtype=np.float64)
        out[case + "/zero_grads"] = np.array(json.dumps({nm: zero_grad_names(g) for nm, g in r64["steps"][0]["grad"].items()}))
        f32_eval = {}
        for contract in ("patch", "full"):
            for k in ("fake_I", "fake_T", "fake_N"):
                out["%s/eval_%s/%s" % (case, contract, k)] = r64["eval"][contract][k].float().numpy()
                f32_eval["%s/%s" % (contract, k)] = rel_l2(r32["eval"][contract][k], r64["eval"][contract][k])
        out[case + "/eval_full/real_T_shape"] = np.array(r64["eval"]["full_real_T_shape"])
        out["f32/%s/eval" % case] = np.array(json.dumps(f32_eval))
        zero = json.loads(str(out[case + "/zero_grads"]))
        for it, (a, b) in enumerate(zip(r64["steps"], r32["steps"])):
            tag = "%s/s%d" % (case, it)
            out[tag + "/loss_names"] = np.array(list(a["losses"].keys()))
            out[tag + "/loss_values"] = np.array(list(a["losses"].values()), dtype=np.float64)
            f32 = {"loss/" + k: abs(b["losses"][k] - v) for k, v in a["losses"].items()}
            for k in ("fake_I", "fake_T"):
                out["%s/%s" % (tag, k)] = a[k].float().numpy()       # (stored in float32: 6e-8 of rounding against bounds of 1e-3)
                f32[k] = rel_l2(b[k], a[k])
            for nm in NETS:
                # one [tensors, 3] array of detrand.probe triples per network, rows in named_parameters order (keys/<net> minus the buffers);
                # the buffers as one flat vector in named_buffers order (the integer counters included), rounded to float32 like the outputs
                out["%s/grad_%s" % (tag, nm)] = np.stack([detrand.probe(g, k) for k, g in a["grad"][nm].items()])
                out["%s/param_%s" % (tag, nm)] = np.stack([detrand.probe(v, k) for k, v in a["param"][nm].items()])
                out["%s/buf_%s" % (tag, nm)] = torch.cat([v.double().reshape(-1) for v in a["buf"][nm].values()]).float().numpy()
                if it == 0:
                    out["%s/param_names_%s" % (case, nm)] = np.array(json.dumps(list(a["grad"][nm].keys())))
                    out["%s/buf_names_%s" % (case, nm)] = np.array(json.dumps([[k, list(v.shape)] for k, v in a["buf"][nm].items()]))
                for k, g in a["grad"][nm].items():
                    if k not in zero[nm]:
                        f32["grad_%s/%s" % (nm, k)] = rel_l2(b["grad"][nm][k], g)
                    f32["param_%s/%s" % (nm, k)] = rel_l2(b["param"][nm][k], a["param"][nm][k])
                for k, v in a["buf"][nm].items():
                    if v.dtype != torch.long and v.double().norm().item() > 0:
                        f32["buf_%s/%s" % (nm, k)] = rel_l2(b["buf"][nm][k], v)
            out["f32/" + tag] = np.array(json.dumps(f32))
            worst = max((v, k) for k, v in f32.items() if k.startswith("grad_"))
            print(tag, {k: round(v, 6) for k, v in a["losses"].items()})
            print(tag, "fp32 distance: fake_I %.2e fake_T %.2e, worst gradient %.2e (%s), worst loss %.2e" %
                  (f32["fake_I"], f32["fake_T"], worst[0], worst[1], max(v for k, v in f32.items() if k.startswith("loss/"))))
        print(case, "entries", {nm: len(v) for nm, v in r64["keys"].items()}, "zero-gradient tensors:", {nm: len(v) for nm, v in zero.items()},
              "eval fp32 distance", f32_eval)
    names, how = test_phase_names()
    print("test-phase model:", how, names)
    out["test/names"] = np.array(json.dumps(names))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")
    opts = {"pix2pix_%s" % phase: dump_options("pix2pix", phase == "train") for phase in ("train", "test")}
    with open(args.opts_out, "w") as f:
        json.dump(opts, f, indent=0, sort_keys=False)
    print("wrote", args.opts_out, {k: len(v) for k, v in opts.items()})


if __name__ == "__main__":
    main()
