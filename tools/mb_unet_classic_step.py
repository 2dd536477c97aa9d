"""Time `--model sinskitG --netG unet_256` on one GPU at 1024 x 1024, batch 1: the training step eager and as replayed HIP graphs, and
inference (test()), at ngf 10 (the model's default: every layer on the 4 x 4 kernels) and ngf 64 (the classic size: the GEMM-class
route above 80 output channels).  Prints one JSON line per ngf: milliseconds (median of --reps timed blocks of --steps, after --warmup).

  python tools/mb_unet_classic_step.py                 # ngf 10 and 64
  python tools/mb_unet_classic_step.py --ngf 64 --size 512
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


def timed(fn, steps, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / steps)
    return {"median": round(statistics.median(times), 3), "min": round(min(times), 3), "max": round(max(times), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngf", type=int, action="append")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--netG", default="unet_256")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from torch.utils.data import default_collate

    from data.synthetic_dataset import make_sample
    from models import create_model
    from options.train_options import TrainOptions

    data = default_collate([make_sample(args.size, 64, 64, 7)])
    for ngf in args.ngf or [10, 64]:
        rec = {"netG": args.netG, "ngf": ngf, "size": args.size, "batch": 1, "steps": args.steps, "reps": args.reps}
        for mode, flag in (("eager", "False"), ("replayed", "True")):
            opt = TrainOptions(cmd_line="--model sinskitG --gpu_ids 0 --netG %s --ngf %d --crop_size %d --batch_size 1 --lambda_G1_lpips 0 "
                                        "--lambda_G2_lpips 0 --use_vision_aided_loss False --use_hip_graph %s --checkpoints_dir /tmp/vts_mb "
                                        "--name unet_classic_step" % (args.netG, ngf, args.size, flag)).parse()
            model = create_model(opt)
            model.setup(opt)
            model.parallelize()
            model.train()

            def step():
                model.set_input(data, phase="train")
                model.optimize_parameters(epoch=1)

            rec["step_%s_ms" % mode] = timed(step, args.steps, args.warmup, args.reps)
            if mode == "replayed":
                rec["graph_nodes"] = model.graph_nodes
                rec["losses_finite"] = all(v == v and abs(v) < 1e30 for v in model.get_current_losses().values())
            model.eval()

            def infer():
                model.set_input(data, phase="test")
                model.test()

            rec["infer_%s_ms" % mode] = timed(infer, args.steps, args.warmup, args.reps)
            rec["params_M"] = round(sum(p.numel() for p in model.netG.parameters()) / 1e6, 2)
            del model
            torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
