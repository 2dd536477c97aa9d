"""Writes tests/golden/clip_visual.npz: the judges of tests/test_clip_gpu.py for the CLIP image tower and its attention core.

Inputs and weights are NOT stored: both sides regenerate them from seeds with oracle/detrand.py (tests/clip_restated.py:test_weights /
test_input / attn_input).  Per case the file holds
  <case>_out64   the float64 output of the restatement on the fp16-valued weights and the fp16-rounded input (tower cases only),
  <case>_err16   the relative L2 error of the reference's own arithmetic against it: the same restatement run with everything in fp16 on
                 the CPU (LayerNorm evaluated in fp32 on the fp16 stream, as CLIP's LayerNorm subclass does) -- the bound the HIP tower
                 must not exceed, being the half-precision run it replaces.
Run from the repository root:  python tools/make_clip_golden.py      (a few minutes: ViT-B/32 in float64 and fp16 on the CPU)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_restated as R  # noqa: E402

SEED = 77


def main():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    out = {}
    for name, (cfg, batch) in R.TOWER_CASES.items():
        o64, e16 = R.judge_pair(R.test_weights(cfg, SEED), cfg, R.test_input(cfg, batch, SEED))
        out[name + "_out64"], out[name + "_err16"] = o64.numpy(), np.float64(e16)
        print("%-12s all-fp16 rel-L2 %.3e  |out| %.3f" % (name, e16, float(o64.norm())), flush=True)
    for name, t in R.ATTN_CASES.items():
        qkv = R.attn_input(t, SEED)
        o64 = R.attention(qkv.double(), 3, t, 2)
        e16 = R.rel_l2(R.attention(qkv, 3, t, 2), o64)
        out[name + "_err16"] = np.float64(e16)      # (the float64 judge of the attention cases is cheap: the test recomputes it)
        print("%-12s all-fp16 rel-L2 %.3e" % (name, e16), flush=True)
    np.savez_compressed(R.GOLDEN, **out)
    print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
