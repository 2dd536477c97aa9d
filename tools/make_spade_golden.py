"""Write tests/golden/spade_32.npz: the reference's SPADE modules run on the CPU (TEST INFRASTRUCTURE ONLY; needs the reference tree,
see oracle/ref_import.py).  No weights are stored: both sides draw them from oracle.detrand (tests/spade_restated.weights).

Every case runs twice: in float64 (the judge values that are stored) and in float32 (stored only as its per-tensor relative L2
distance to the float64 run, a JSON dict `f32/<case>`: the yardstick the GPU tests print next to their own error).
Tensors of up to spade_restated.FULL_MAX elements are stored whole, larger ones as detrand.probe triples; the generators' training
output and dseg whole.

  python tools/make_spade_golden.py
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
import spade_restated as R  # noqa: E402


def load_state(mod, sd32, dtype):
    mod.to(dtype)
    own = mod.state_dict()
    assert list(own.keys()) == list(sd32.keys()), (list(own.keys()), list(sd32.keys()))
    mod.load_state_dict({k: (v.clone() if v.dtype == torch.long else v.to(dtype)) for k, v in sd32.items()})
    return mod


def buffers_of(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items() if not R.is_param(k)}


def grads_of(mod):
    # a spectral-normalised convolution's parameter is weight_orig: named_parameters carries the state-dict names
    return {k: p.grad.detach().clone() for k, p in mod.named_parameters()}


def zero_grad_names(grads):
    norms = {k: g.double().norm().item() for k, g in grads.items()}
    top = max(norms.values())
    zero = [k for k, v in norms.items() if v < 1e-9 * top]
    return zero, min(v for k, v in norms.items() if k not in zero)


def run_generator(ref_networks, case, dtype):
    c = R.GEN_CASES[case]
    G = ref_networks.SPADEGenerator(c["input_nc"], c["output_nc"], c["ngf"], R.gen_opt(case))
    shapes = {k: tuple(v.shape) for k, v in G.state_dict().items()}
    load_state(G, R.weights(shapes, c["seed"]), dtype)
    G.train()
    h, w = R.gen_out_hw(c)
    seg = R.seg_input(c["N"], c["input_nc"], h, w, c["seed"]).to(dtype).requires_grad_(True)
    out = G(seg)
    (out * R.cotangent(out.shape, c["seed"]).to(dtype)).sum().backward()
    res = {"out": out.detach(), "dseg": seg.grad.detach()}
    res.update({"grad/" + k: v for k, v in grads_of(G).items()})
    res.update({"buf1/" + k: v for k, v in buffers_of(G).items()})
    with torch.no_grad():
        G(seg)
    res.update({"buf2/" + k: v for k, v in buffers_of(G).items()})
    G.eval()
    with torch.no_grad():
        res["out_eval"] = G(seg).detach()
    return shapes, res


def run_block(ref_arch, shape, norm, dtype):
    fin, fout = shape[:2]
    seed = 900 + R.BLOCK_SHAPES.index(shape) * 2 + (norm == "instance")
    blk = ref_arch.SPADEResnetBlock(fin, fout, R.Opt(normG=R.BLOCK_NORMS[norm], semantic_nc=1))
    shapes = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
    mine = R.block_shapes(fin, fout, kind=norm, prefix="blk")
    assert [("blk." + k, s) for k, s in shapes.items()] == list(mine.items()), "block key order"
    load_state(blk, R.weights({k[4:]: s for k, s in mine.items()}, seed), dtype)
    blk.train()
    res = R.run_block_case(lambda x, seg: blk(x, seg), None, shape, seed, dtype)
    res.update({"grad/" + k: v for k, v in grads_of(blk).items()})
    res.update({"buf1/" + k: v for k, v in buffers_of(blk).items()})
    return seed, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "spade_32.npz"))
    args = ap.parse_args()
    ref_import.load()
    torch.set_num_threads(min(8, torch.get_num_threads()))
    import models.architecture as ref_arch
    import models.networks as ref_networks

    out = {}
    for case in R.GEN_CASES:
        shapes, r64 = run_generator(ref_networks, case, torch.float64)
        _, r32 = run_generator(ref_networks, case, torch.float32)
        out["keys/" + case] = np.array(json.dumps([[k, list(s)] for k, s in shapes.items()]))
        f32 = {}
        grads = {k[5:]: v for k, v in r64.items() if k.startswith("grad/")}
        zero, smallest = zero_grad_names(grads)
        out["zero_grads/" + case] = np.array(json.dumps(zero))
        out["min_nonzero_grad_norm/" + case] = np.float64(smallest)
        out["f32_zero_grad_norm/" + case] = np.float64(max(r32["grad/" + k].double().norm().item() for k in zero) if zero else 0.0)
        for k, v in r64.items():
            if v.dtype == torch.long:
                out["%s/%s" % (case, k)] = v.numpy()
                continue
            R.store(out, "%s/%s" % (case, k), v, always_full=k in ("out", "dseg"))
            if k[5:] not in zero or not k.startswith("grad/"):
                f32[k] = R.rel_l2(r32[k], v)
        out["f32/" + case] = np.array(json.dumps(f32))
        print(case, "out fp32 distance %.2e" % f32["out"], "zero-gradient tensors", zero, "smallest other norm %.3g" % smallest)
    for shape in R.BLOCK_SHAPES:
        for norm in R.BLOCK_NORMS:
            name = R.block_case_name(shape, norm)
            seed, r64 = run_block(ref_arch, shape, norm, torch.float64)
            _, r32 = run_block(ref_arch, shape, norm, torch.float32)
            out["seed/" + name] = np.int64(seed)
            worst, f32 = 0.0, {}
            for k, v in r64.items():
                if v.dtype == torch.long:
                    out["%s/%s" % (name, k)] = v.numpy()
                    continue
                R.store(out, "%s/%s" % (name, k), v)
                if v.double().norm().item() > 1e-9:
                    d = R.rel_l2(r32[k], v)
                    f32[k] = d
                    worst = max(worst, d)
            out["f32/" + name] = np.array(json.dumps(f32))
            print(name, "worst fp32 distance %.2e" % worst)
    out["probes"] = np.array(json.dumps(out["probes"]))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
