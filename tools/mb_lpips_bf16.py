"""Micro-benchmark of one LPIPS loss term (vts/perceptual.py:lpips_term, forward + backward) in fp32 and in bf16 (--lpips_dtype), at the two
shapes of the headline step: the image term at 1024 x 1024 with batch 4, and the tactile term on the step's stack of 32 x 32 patches
(batch 4 x 64 patches x 2 channels = 512 one-channel patches).  Whole-term times are taken inside a HIP graph (as tools/mb_conv_big.py
does); the per-layer table comes from one eager run bracketed by events (ops.TIMER).
   python tools/mb_lpips_bf16.py [--dtypes fp32,bf16] [--reps 5] [--shapes image,tactile]
A tree without the option (the parent of the commit that added it) times fp32 only: the A/B of the two trees runs this same file in both."""
import argparse
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-tactile-synthesis_amd"))
import torch  # noqa: E402

from models import perceptual  # noqa: E402
from vts import ops, perceptual as P  # noqa: E402

dev = torch.device("cuda:0")
PEAK_TF = {"fp32": 157.3, "bf16": 16 * 157.3}       # matrix-core peaks of the MI355X (fp32-input MFMA; bf16 MFMA = 16 x that)
SHAPES = {"image": ((4, 3, 1024, 1024), 1.0), "tactile": ((512, 1, 32, 32), 0.3)}
HAS_DTYPE = "dtype" in inspect.signature(P.lpips_term).parameters


def term(net, a, b, slot, grad, dtype):
    kw = {"dtype": dtype} if HAS_DTYPE else {}
    P.lpips_term(net, a, b, 1.0, slot, grad_into=grad, **kw)


def graph_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ops.freeze_ws("mb_lpips_bf16")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    del g
    ops.release_ws("mb_lpips_bf16")
    return min(times), sorted(times)[len(times) // 2]


def per_layer(fn, dtype):
    ops.TIMER = []
    fn()
    torch.cuda.synchronize()
    rows, ops.TIMER = ops.TIMER, None
    tot = 0.0
    for label, nbytes, flops, e0, e1, detail in rows:
        ms = e0.elapsed_time(e1)
        tot += ms
        tf = flops / ms / 1e9 if flops else 0.0
        print("    %-34s %-44s %8.3f ms %8.1f GB/s %8.1f TF  %5.3f of the %s MFMA peak" % (
            label[:34], detail or "", ms, nbytes / ms / 1e6, tf, tf / PEAK_TF[dtype], dtype))
    print("    sum of the launches %.3f ms (eager, event-bracketed: includes the gaps the graph removes)" % tot)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--shapes", default="image,tactile")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no_layers", action="store_true")
    args = ap.parse_args()
    net = perceptual.LpipsVgg16().to(dev)
    for name in args.shapes.split(","):
        shape, scale = SHAPES[name]
        g = torch.Generator().manual_seed(1)
        a = (scale * (2 * torch.rand(shape, generator=g) - 1)).to(dev)
        b = (scale * (2 * torch.rand(shape, generator=g) - 1)).to(dev)
        slot, grad = ops.loss_slots(1, dev), torch.empty_like(a)
        for dtype in args.dtypes.split(","):
            if dtype != "fp32" and not HAS_DTYPE:
                print("%s %s: this tree has no lpips dtype option" % (name, dtype))
                continue
            fn = lambda: term(net, a, b, slot, grad, dtype)       # noqa: E731
            best, med = graph_ms(fn, args.reps)
            print("lpips_term %-8s N%d %dx%d %s: %.3f ms best, %.3f ms median of %d graph replays (forward + backward)" % (
                name, shape[0], shape[2], shape[3], dtype, best, med, args.reps), flush=True)
            if not args.no_layers:
                per_layer(fn, dtype)
            torch.cuda.empty_cache()
