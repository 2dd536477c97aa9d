"""Micro-benchmark of skitG's style encoder: the CLIP ViT-B/32 tower's C entry (vts_clip_visual_forward) and CLIP's pre-processing
(vts_clip_preprocess) of a 1024 x 1024 image, batches 1 and 4, each inside a HIP graph (the Python / ctypes enqueue costs ~15 us per
call: eager timing floors there), next to the weight-read floor -- the tower's fp16 weight bytes over the HBM bandwidth constant of
bench.py's roofline.  With --step: the skitG fresh-batch training step with the style code computed by the encoder versus supplied
in the batch (bench.py's fresh-input loop, alternated in one process).
   python tools/mb_clip.py [--step] [--reps 10] [--replays 15]
Seeded stand-in weights: times do not depend on the values."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "visual-tactile-synthesis_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
from vts import ops  # noqa: E402


def graph_us(fn, reps, replays):
    """`reps` calls captured in one HIP graph; (median, min, max) microseconds per call over `replays` timed replays"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def tower_and_preprocess(args):
    from models.clip_visual import ClipVisual

    dev = torch.device("cuda:0")
    net = ClipVisual().to(dev)
    flat = net.flat_weights()
    floor_us = 2.0 * flat.numel() / (bench.HBM_PEAK_GBS * 1e9) * 1e6
    out = {"weight_halfs": flat.numel(), "weight_read_floor_us": floor_us, "hbm_GBps": bench.HBM_PEAK_GBS, "reps_per_graph": args.reps,
           "replays": args.replays}
    print("ViT-B/32: %.1f M fp16 weights, %.1f MB; weight-read floor %.1f us at %.0f GB/s" % (flat.numel() / 1e6, 2e-6 * flat.numel(), floor_us,
                                                                                              bench.HBM_PEAK_GBS))
    for batch in (1, 4):
        img = torch.rand(batch, 3, 1024, 1024, device=dev) * 2 - 1
        pre = ops.clip_preprocess(img)
        code = torch.empty(batch, 512, device=dev)
        t_pre = graph_us(lambda: ops.clip_preprocess(img, out=pre), args.reps, args.replays)
        t_tow = graph_us(lambda: ops.clip_visual_forward(net._ccfg, flat, pre, out=code), args.reps, args.replays)
        out["batch%d" % batch] = {"preprocess_1024_us": t_pre, "tower_us": t_tow, "tower_over_floor": t_tow[0] / floor_us}
        print("batch %d: preprocess 1024^2 %7.1f us (min %.1f max %.1f)   tower %7.1f us (min %.1f max %.1f) = %.1f x the weight-read floor"
              % ((batch,) + t_pre + t_tow + (t_tow[0] / floor_us,)))
    return out


def fresh_step(args):
    """bench.py's fresh-input loop on skitG 1024^2 batch 4, the style code supplied in the batch vs computed by the encoder; the two
    forms alternate (A B A B) so that drift of the shared host shows"""
    model, opt = bench.build_model(1024, 4, "skitG")

    def pinned(b, keep_code):
        return {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in b.items() if keep_code or k != "style_code"}

    raw = [bench.make_batch(1024, 4, k, opt.style_code_dim, quantize8=True) for k in (0, 1)]
    forms = {"supplied": [pinned(b, True) for b in raw], "computed": [pinned(b, False) for b in raw]}
    res = {"supplied": [], "computed": []}
    for rnd in range(args.rounds):
        for name in ("supplied", "computed"):
            batches = forms[name]
            for i in range(4):
                model.set_input(batches[i % 2], phase="train")
                model.optimize_parameters(epoch=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                model.set_input(batches[i % 2], phase="train")
                model.optimize_parameters(epoch=1)
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            print("round %d  style code %-8s : %.3f ms per fresh-batch step" % (rnd, name, res[name][-1]), flush=True)
    return {"steps": args.steps, "ms_per_step": res}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="also time the skitG fresh-batch step with the code computed vs supplied")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mb_clip.py needs a GPU: a time cannot be measured without one")
    result = {"encoder": tower_and_preprocess(args)}
    if args.step:
        result["fresh_step"] = fresh_step(args)
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
