"""Writes tests/golden/clip_visual_bwd.npz: the bounds of tests/test_clip_bwd_gpu.py for the CLIP image tower's input-gradient backward.

Nothing but bounds is stored: weights, inputs and cotangents are regenerated from seeds (tests/clip_bwd_restated.py) and the float64
judges are cheap enough for the tests to recompute.  Every value is the relative L2 error, against float64 autograd, of the reference's
own arithmetic -- the same restated computation under torch autograd with everything in fp16 on the CPU (LayerNorm in fp32), at cotangent
scale 1:
  <case>_<a|b|c>_err16   tower backward; cotangent at the embedding (a), at the tapped hidden states (b), at both (c)
  <case>_hid<l>_err16    the taped forward's hidden state after block l
  <attn case>_bwd_err16  the attention core's backward
  e2e_err16              area pre-processing + tower, embedding and taps (1, 2), on a [2, 3, 96, 80] image
It also prints, without storing them, the all-fp16 errors at cotangent scales 2^-12 and 2^8 that the scale test of the HIP backward is
about.  Run from the repository root:  python tools/make_clip_bwd_golden.py      (about a minute: ViT-B/32 backward in fp16 on the CPU)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_bwd_restated as B  # noqa: E402
import clip_restated as R  # noqa: E402


def main():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    out = {}
    for name, (cfg, batch) in R.TOWER_CASES.items():
        sd16, x16, taps = B.weights16(cfg), R.test_input(cfg, batch, B.SEED), B.TAPS[name]
        for case, variant in B.BWD_CASES:
            if case != name:
                continue
            d_out, used, d_hidden = B.cotangents(cfg, batch, taps, variant)
            g64, _, s64 = B.tower_grad(sd16, cfg, x16, d_out, used, d_hidden, torch.float64)
            g16, _, s16 = B.tower_grad(sd16, cfg, x16, d_out, used, d_hidden, torch.float16)
            out["%s_%s_err16" % (name, variant)] = np.float64(R.rel_l2(g16, g64))
            print("%-12s %s all-fp16 backward rel-L2 %.3e  |dx| %.3e" % (name, variant, R.rel_l2(g16, g64), float(g64.norm())), flush=True)
            if variant == "c":
                for l in taps:
                    out["%s_hid%d_err16" % (name, l)] = np.float64(R.rel_l2(s16[l], s64[l]))
                    print("%-12s hidden %2d all-fp16 rel-L2 %.3e" % (name, l, R.rel_l2(s16[l], s64[l])), flush=True)
                if name in ("small224_b2", "vitb32_b1"):
                    for e in (-12, 8):
                        gs, _, _ = B.tower_grad(sd16, cfg, x16, None if d_out is None else (d_out.float() * 2.0 ** e).half(), used,
                                                [(d.float() * 2.0 ** e).half() for d in d_hidden], torch.float16)
                        print("%-12s c at cotangent scale 2^%d: all-fp16 rel-L2 %.3e (not stored)" % (name, e, R.rel_l2(gs, g64 * 2.0 ** e)), flush=True)
    for name, t in R.ATTN_CASES.items():
        qkv, d = R.attn_input(t, B.SEED), B.attn_cot(t)
        e16 = R.rel_l2(B.attention_grad(qkv, d, t, torch.float16), B.attention_grad(qkv, d, t, torch.float64))
        out[name + "_bwd_err16"] = np.float64(e16)
        print("%-12s all-fp16 backward rel-L2 %.3e" % (name, e16), flush=True)
    cfg, taps = B.E2E["cfg"], B.E2E["taps"]
    sd16, img = B.weights16(cfg), B.e2e_image()
    d_out, _, d_hidden = B.cotangents(cfg, img.shape[0], taps, "c")
    e16 = R.rel_l2(B.e2e_grad(sd16, img, d_out, taps, d_hidden, torch.float16), B.e2e_grad(sd16, img, d_out, taps, d_hidden, torch.float64))
    out["e2e_err16"] = np.float64(e16)
    print("e2e          all-fp16 rel-L2 %.3e" % e16, flush=True)
    np.savez_compressed(B.GOLDEN, **out)
    print("wrote", B.GOLDEN, os.path.getsize(B.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
