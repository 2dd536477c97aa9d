"""Write tests/golden/nets_style_levels.npz: the reference's CustomUnetGenerator with the style code at several decoder levels
(--num_layer_style_code k > 1) run on the CPU (TEST INFRASTRUCTURE ONLY; needs the reference tree, see oracle/ref_import.py).
No weights are stored: both sides draw them from oracle.detrand (tests/style_levels_cases.py lists the cases).

Per case `<name>/`: the sorted state-dict key list (`keys`; tile mode lists the reference's unused style_code_mapping<j> layers under
`dead_keys` instead -- with k = 8 at 256 x 256 they hold 5.7e9 weights that nothing reads, so they are built on the meta device and
dropped), the sub-sampled output, probes of the output, the input gradient and every parameter gradient, d/d style_code, and the
BatchNorm1d running statistics of every style_code_mapping<j> at batch 2.  Tile cases run in float64; project / adain cases cannot
(the reference casts the code to float32, networks.py:1610).  The non-square case goes through oracle/nets.py: upstream builds its
mappings for square inputs only.

  python tools/make_style_levels_golden.py [case ...]
  python tools/make_style_levels_golden.py --pick-seeds [case ...]     # the conditioning scan behind the seeds of style_levels_cases.CASES
"""
import argparse
import os
import sys
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import detrand, ref_import  # noqa: E402
import style_levels_cases as S  # noqa: E402


class _MetaLinear(torch.nn.Linear):
    """nn.Linear without storage: the style_code_mapping<j> layers the reference creates and never uses in tile mode"""

    def __init__(self, in_features, out_features, bias=True, **kw):
        super().__init__(in_features, out_features, bias=bias, device="meta")


def run_reference(c):
    from oracle.make_golden import _ref_opt
    import models.networks as ref_networks

    opt = _ref_opt("skitG", True, ["--use_style_code", "True", "--batch_size", str(c.n), "--style_code_mode", c.mode,
                                  "--style_code_mapping_mode", c.mapping, "--num_layer_style_code", str(c.k)])
    norm = ref_networks.get_norm_layer("instance")
    build = lambda: ref_networks.CustomUnetGenerator(9, 5, S.NUM_DOWNS, S.NGF, norm, False, num_layer_separate=S.NLS, opt=opt, input_size=c.h)
    dead = []
    if c.mapping == "tile":
        with mock.patch.object(torch.nn, "Linear", _MetaLinear):
            G = build()
        for j in range(c.k):
            name = "style_code_mapping%d" % j
            dead += ["%s.%s" % (name, k) for k in getattr(G, name).state_dict().keys()]
            delattr(G, name)
    else:
        G = build()
    mine = S.shapes(c)
    assert {k: tuple(v.shape) for k, v in G.named_parameters()} == {k: tuple(v) for k, v in mine.items()}, "key / shape mismatch in " + c.name
    G.load_state_dict(S.weights(c), strict=False)
    dt = torch.float64 if c.f64 else torch.float32
    G.to(dt).train()
    x, sc, cot = S.inputs(c)
    x, sc = x.to(dt).requires_grad_(True), sc.to(dt).requires_grad_(True)
    y = G(x, style_code=sc)
    (y * cot.to(dt)).sum().backward()
    res = dict(y=y.detach(), dx=x.grad, dstyle=sc.grad, grads={k: p.grad for k, p in G.named_parameters()})
    res["keys"], res["dead"] = sorted(G.state_dict().keys()), sorted(dead)
    res["bn"] = {k: v.detach() for k, v in G.state_dict().items() if k.startswith("style_code_mapping") and "running_" in k}
    return res


def run_oracle(c):
    res = dict(S.oracle_run(c.name))
    res["keys"], res["dead"], res["bn"] = sorted(S.shapes(c).keys()), [], {}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=list(S.CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "nets_style_levels.npz"))
    ap.add_argument("--pick-seeds", action="store_true", help="print, per case, the first seed from FIRST_SEED on whose float32 oracle run "
                    "lies within SEED_BOUND of its float64 run (no reference needed)")
    args = ap.parse_args()
    if args.pick_seeds:
        for name in args.cases:
            for seed in range(S.FIRST_SEED, S.FIRST_SEED + 64):
                v = S.conditioning(name, seed)
                print("%s seed %d: float32 oracle vs float64 oracle, worst gradient tensor %.1e" % (name, seed, v), flush=True)
                if v < S.SEED_BOUND:
                    break
        return
    ref_import.load()
    torch.set_num_threads(min(8, torch.get_num_threads()))
    out = {}
    if os.path.exists(args.out) and set(args.cases) != set(S.CASES):       # regenerate some cases, keep the others
        out.update(np.load(args.out))
    for name in args.cases:
        c = S.case(name)
        r = run_reference(c) if c.via == "reference" else run_oracle(c)
        t = name + "/"
        for k in [k for k in out if k.startswith(t)]:
            del out[k]
        st = S.sub_stride(c)
        assert torch.isfinite(r["y"]).all(), name
        out[t + "seed"] = np.int64(c.seed)
        out[t + "keys"], out[t + "dead_keys"] = np.array(r["keys"]), np.array(r["dead"], dtype=str)
        out[t + "G_out_sub"] = r["y"][:, :, ::st, ::st].to(torch.float32).numpy()
        out[t + "G_out_probe"] = detrand.probe(r["y"], "g_out")
        out[t + "G_dx_probe"] = detrand.probe(r["dx"], "g_dx")
        out[t + "G_dstyle"] = r["dstyle"].to(torch.float64).numpy()
        for k, g in r["grads"].items():
            out[t + "G_grad/" + k] = detrand.probe(g, k)
        for k, v in r["bn"].items():
            out[t + "bn/" + k] = v.to(torch.float32).numpy()
        print(name, "via", c.via, "float64" if c.f64 else "float32", "|y|", float(r["y"].norm()), "|dstyle|", float(r["dstyle"].norm()))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
