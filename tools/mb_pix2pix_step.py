"""Time the `--model pix2pix` training step on one GPU: eager and as replayed HIP graphs, on a synthetic patch batch.  Prints one JSON line
per shape: milliseconds per step (median of --reps timed blocks of --steps steps, after --warmup) and the graph's (nodes, kernel nodes) per
segment.

  python tools/mb_pix2pix_step.py                     # the fixture shape (ngf 8, ndf 8, 4 x 32x32) and the reference's (64, 64, 32 x 32x32)
  python tools/mb_pix2pix_step.py --shape 64,64,32
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "visual-tactile-synthesis_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def batch(n, size, seed=7):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    M = (((yy - size / 2) / (0.45 * size)) ** 2 + ((xx - size / 2) / (0.4 * size)) ** 2 <= 1).float()[None, None].repeat(n, 1, 1, 1)

    def u(*shape):
        return torch.rand(*shape, generator=g) * 2 - 1

    return {"S_images": u(n, 1, size, size), "M_images": M, "I_images": u(n, 3, size, size), "T_images": 0.3 * u(n, 2, size, size),
            "I_masks": torch.ones(n, size, size), "name": ["synthetic"] * n, "S_paths": ["synthetic.png"] * n, "augmentation_params": {}}


def time_steps(model, data, steps, warmup, reps):
    for _ in range(warmup):
        model.set_input(data, phase="train")
        model.optimize_parameters(epoch=1)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            model.set_input(data, phase="train")
            model.optimize_parameters(epoch=1)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / steps)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="ngf,ndf,batch (repeatable)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from models import create_model
    from options.train_options import TrainOptions

    for shape in args.shape or ["8,8,4", "64,64,32"]:
        ngf, ndf, n = (int(v) for v in shape.split(","))
        rec = {"ngf": ngf, "ndf": ndf, "batch": n, "size": 32, "steps": args.steps, "reps": args.reps}
        for mode, flag in (("eager", "False"), ("replayed", "True")):
            opt = TrainOptions(cmd_line="--model pix2pix --gpu_ids 0 --ngf %d --ndf %d --batch_size %d --use_hip_graph %s --dataset_mode patchskit "
                                        "--checkpoints_dir /tmp/vts_mb --name pix2pix_step" % (ngf, ndf, n, flag)).parse()
            opt.quiet = True
            model = create_model(opt)
            model.setup(opt)
            model.parallelize()
            model.train()
            med, lo, hi = time_steps(model, batch(n, 32), args.steps, args.warmup, args.reps)
            rec[mode + "_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
            if mode == "replayed":
                rec["graph_nodes"] = model.graph_nodes
                rec["losses_finite"] = all(v == v and abs(v) < 1e30 for v in model.get_current_losses().values())
            del model
            torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
