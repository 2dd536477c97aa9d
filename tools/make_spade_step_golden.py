"""Write tests/golden/spade_step_32.npz: the reference's SPADEModel (models/spade_model.py) run on the CPU for two optimize_parameters
calls per case (TEST INFRASTRUCTURE ONLY; needs the reference tree, see oracle/ref_import.py).  No weights are stored: both sides draw
them from seeds (the generator: tests/spade_restated.weights; the discriminators: oracle.detrand.test_weights) over the key / shape
lists the fixture records.  torchvision is absent, so `networks.VGGLoss` is oracle.perceptual.VGGLoss on its seeded stand-in weights.

Cases:  default  --model spade --ngf 8 --ndf 8 --batch_size 4          (hinge, two-time-scale rates, sync-batch SPADE, VGG term on)
        B        + --no_TTUR --gan_mode lsgan --no_vgg_loss True, normG = spectralspadeinstance3x3 set on the parsed options

Every case runs in float64 (the judge values that are stored) and in float32 (stored only as its distance to the float64 run, a JSON dict
`f32/<case>/s<step>`: relative L2 per tensor, absolute difference per loss -- the yardstick the GPU tests print next to their own error).
For the float64 run the tactile tensors, which the reference's set_input forces to float32, are cast on the model after set_input, and
the stand-in VGG is built under float32 defaults and then cast (its seeded weights would otherwise differ between the two runs).
The reference's option setter reads --no_TTUR from sys.argv, so the argument list is put there while the options are parsed.

  python tools/make_spade_step_golden.py
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

from oracle import detrand, perceptual, ref_import  # noqa: E402
import spade_restated as R  # noqa: E402

SIZE, N, STEPS = 32, 4, 2
BASE = ["--model", "spade", "--ngf", "8", "--ndf", "8", "--batch_size", "4"]
CASES = {
    "default": dict(flags=BASE, override={}, seed=905),
    "B": dict(flags=BASE + ["--no_TTUR", "--gan_mode", "lsgan", "--no_vgg_loss", "True"], override={"normG": "spectralspadeinstance3x3"}, seed=915),
}
OPT_KEYS = ["beta1", "beta2", "lr", "gan_mode", "normG", "norm", "netD", "batch_size", "output_width", "num_upsampling_layers", "niter_decay"]


def p2p_batch(n, size, seed):
    """synthetic patch batch with the patchskit contract (return_patch=True): what tests/test_pix2pixHD_gpu.py:p2p_batch builds"""
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    M = (((yy - size / 2) / (0.45 * size)) ** 2 + ((xx - size / 2) / (0.4 * size)) ** 2 <= 1).float()[None, None].repeat(n, 1, 1, 1)
    return {"S_images": detrand.uniform((n, 1, size, size), seed, "S"), "M_images": M,
            "I_images": detrand.uniform((n, 3, size, size), seed, "I"), "T_images": 0.3 * detrand.uniform((n, 2, size, size), seed, "T"),
            "I_masks": torch.ones(n, size, size, dtype=torch.float64), "name": ["synthetic"] * n, "S_paths": ["synthetic.png"] * n,
            "augmentation_params": {}}


def ref_opt(is_train, flags):
    from options.test_options import TestOptions
    from options.train_options import TrainOptions
    import models

    argv = sys.argv
    sys.argv = [argv[0]] + list(flags)       # the option setter parses sys.argv itself to see --no_TTUR
    try:
        o = (TrainOptions if is_train else TestOptions)()
        parser = o.initialize(argparse.ArgumentParser())
        parser = models.get_option_setter("spade")(parser, is_train)
        opt, _ = parser.parse_known_args(list(flags))
    finally:
        sys.argv = argv
    opt.isTrain = is_train
    opt.gpu_ids = []
    return opt


def build(case, dtype, is_train=True):
    import models
    from models import networks as ref_networks

    def vgg_loss(gpu_ids=None):
        torch.set_default_dtype(torch.float32)
        try:
            v = perceptual.VGGLoss()
        finally:
            torch.set_default_dtype(dtype)
        return v.to(dtype)

    ref_networks.VGGLoss = vgg_loss
    c = CASES[case]
    opt = ref_opt(is_train, c["flags"])
    for k, v in c["override"].items():
        setattr(opt, k, v)
    opt.checkpoints_dir, opt.name = "/tmp/vts_golden_ckpt", "spade_" + case
    os.makedirs(os.path.join(opt.checkpoints_dir, opt.name), exist_ok=True)
    model = models.create_model(opt)
    if is_train:
        model.setup(opt)
    return model, opt


def seed_weights(model, seed, dtype):
    keys = {}
    for i, nm in enumerate(("G", "D", "D2")):
        net = getattr(model, "net" + nm)
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        sd = R.weights(shapes, seed) if nm == "G" else detrand.test_weights(shapes, seed + i)
        net.load_state_dict({k: (v.clone() if v.dtype == torch.long else v.to(dtype)) for k, v in sd.items()})
        keys[nm] = [[k, list(s)] for k, s in shapes.items()]
    return keys


def feed(model, batch, dtype):
    model.set_input({k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in batch.items()}, phase="train")
    for k in ("real_T", "I_masks"):          # set_input forces these to float32
        setattr(model, k, getattr(model, k).to(dtype))
    model.real_gx, model.real_gy = model.real_T[:, 0:1], model.real_T[:, 1:2]


def run_case(case, dtype):
    torch.set_default_dtype(dtype)
    try:
        c = CASES[case]
        model, opt = build(case, dtype)
        keys = seed_weights(model, c["seed"], dtype)
        batch = p2p_batch(N, SIZE, c["seed"])
        res = {"keys": keys, "opt": opt}
        model.eval()
        feed(model, batch, dtype)
        model.test()
        res["eval"] = {"fake_I": model.fake_I.detach().clone(), "fake_T": model.fake_T.detach().clone()}
        model.train()
        res["steps"] = []
        for it in range(STEPS):
            feed(model, batch, dtype)
            model.optimize_parameters(epoch=1)
            st = {"losses": {k: float(v) for k, v in model.get_current_losses().items()},
                  "fake_I": model.fake_I.detach().clone(), "fake_T": model.fake_T.detach().clone(), "grad": {}, "param": {}, "buf": {}}
            for nm in ("G", "D", "D2"):
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
    """as tools/make_spade_golden.py: the tensors whose gradient norm is below 1e-9 of the largest in their network"""
    norms = {k: g.double().norm().item() for k, g in grads.items()}
    top = max(norms.values())
    return [k for k, v in norms.items() if v < 1e-9 * top]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "spade_step_32.npz"))
    args = ap.parse_args()
    ref_import.load()
    torch.set_num_threads(min(8, torch.get_num_threads()))
    out = {"size": SIZE, "n": N, "steps": STEPS}
    for case, c in CASES.items():
        r64, r32 = run_case(case, torch.float64), run_case(case, torch.float32)
        out[case + "/seed"] = c["seed"]
        out[case + "/flags"] = np.array(json.dumps(c["flags"]))
        out[case + "/override"] = np.array(json.dumps(c["override"]))
        out[case + "/keys"] = np.array(json.dumps(r64["keys"]))
        out[case + "/names"] = np.array(json.dumps(r64["names"]))
        out[case + "/lrs_after_update"] = np.array(r64["lrs"], dtype=np.float64)
        out[case + "/zero_grads"] = np.array(json.dumps({nm: zero_grad_names(g) for nm, g in r64["steps"][0]["grad"].items()}))
        for k in ("fake_I", "fake_T"):
            out["%s/eval/%s" % (case, k)] = r64["eval"][k].float().numpy()
        f32_eval = {k: R.rel_l2(r32["eval"][k], r64["eval"][k]) for k in ("fake_I", "fake_T")}
        out["f32/%s/eval" % case] = np.array(json.dumps(f32_eval))
        for it, (a, b) in enumerate(zip(r64["steps"], r32["steps"])):
            tag = "%s/s%d" % (case, it)
            out[tag + "/loss_names"] = np.array(list(a["losses"].keys()))
            out[tag + "/loss_values"] = np.array(list(a["losses"].values()), dtype=np.float64)
            f32 = {"loss/" + k: abs(b["losses"][k] - v) for k, v in a["losses"].items()}
            for k in ("fake_I", "fake_T"):
                out["%s/%s" % (tag, k)] = a[k].float().numpy()       # (stored in float32: 6e-8 of rounding against bounds of 1e-3)
                f32[k] = R.rel_l2(b[k], a[k])
            zero = json.loads(str(out[case + "/zero_grads"]))
            for nm in ("G", "D", "D2"):
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
                        f32["grad_%s/%s" % (nm, k)] = R.rel_l2(b["grad"][nm][k], g)
                    f32["param_%s/%s" % (nm, k)] = R.rel_l2(b["param"][nm][k], a["param"][nm][k])
                for k, v in a["buf"][nm].items():
                    if v.dtype != torch.long and v.double().norm().item() > 0:
                        f32["buf_%s/%s" % (nm, k)] = R.rel_l2(b["buf"][nm][k], v)
            out["f32/" + tag] = np.array(json.dumps(f32))
            worst = max((v, k) for k, v in f32.items() if k.startswith("grad_"))
            print(tag, {k: round(v, 6) for k, v in a["losses"].items()})
            print(tag, "fp32 distance: fake_I %.2e fake_T %.2e, worst gradient %.2e (%s), worst loss %.2e" %
                  (f32["fake_I"], f32["fake_T"], worst[0], worst[1], max(v for k, v in f32.items() if k.startswith("loss/"))))
        print(case, "zero-gradient tensors:", {nm: len(v) for nm, v in json.loads(str(out[case + "/zero_grads"])).items()}, "eval fp32 distance", f32_eval)
    # parsed options, train and test, with and without --no_TTUR (a flag the phase does not declare reads None)
    opts = {}
    for phase, is_train in (("train", True), ("test", False)):
        for tag, extra in (("", []), ("_no_TTUR", ["--no_TTUR"])):
            o = ref_opt(is_train, ["--model", "spade"] + extra)
            opts[phase + tag] = {k: getattr(o, k, None) for k in OPT_KEYS}
    out["opts"] = np.array(json.dumps(opts))
    tm, _ = build("default", torch.float32, is_train=False)
    out["test/names"] = np.array(json.dumps({"loss_names": list(getattr(tm, "loss_names", [])), "visual_names": list(tm.visual_names),
                                             "model_names": list(tm.model_names)}))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
