"""Time the sinskitG training step with the WGAN-GP gradient penalty on one GPU, and the same step in `wgan` mode (the same losses without the
penalty) from the same run: eager and as replayed HIP graphs, on the synthetic batch.  The configuration is the one wgangp trains in:
--netD stylegan2 --lambda_G2_GAN 0 (no tactile discriminator), no perceptual terms.  Prints one JSON line per shape: milliseconds per step
(median / min / max of --reps timed blocks of --steps steps, after --warmup), the modes alternating within a shape.

  python tools/mb_wgangp_step.py                       # 256 and 1024 pixels, batch 1 and 4
  python tools/mb_wgangp_step.py --shape 256,1
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

FLAGS = ("--model sinskitG --gpu_ids 0 --lambda_G1_lpips 0 --lambda_G2_lpips 0 --use_vision_aided_loss False --lambda_G2_GAN_feat 0 "
         "--checkpoints_dir /tmp/vts_mb --name wgangp_step --crop_size %d --load_size %d --batch_size %d --netD stylegan2 --lambda_G2_GAN 0 "
         "--gan_mode %s --use_hip_graph %s")


def timed_block(model, data, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.set_input(data, phase="train")
        model.optimize_parameters(epoch=1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="size,batch (repeatable)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from torch.utils.data import default_collate

    from data.synthetic_dataset import make_sample
    from models import create_model
    from options.train_options import TrainOptions

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    for shape in args.shape or ["256,1", "256,4", "1024,1", "1024,4"]:
        size, n = (int(v) for v in shape.split(","))
        data = default_collate([make_sample(size, 64, 64, 7 + i) for i in range(n)])
        rec = {"size": size, "batch": n, "steps": args.steps, "reps": args.reps}
        models = {}
        for gan_mode in ("wgan", "wgangp"):
            for sched, flag in (("eager", "False"), ("replayed", "True")):
                opt = TrainOptions(cmd_line=FLAGS % (size, size, n, gan_mode, flag)).parse()
                opt.quiet = True
                m = create_model(opt)
                m.setup(opt)
                m.parallelize()
                m.train()
                timed_block(m, data, args.warmup)
                models[gan_mode + "_" + sched] = m
        times = {k: [] for k in models}
        for _ in range(args.reps):           # alternate the four variants inside every repetition
            for k, m in models.items():
                times[k].append(timed_block(m, data, args.steps))
        for k, v in times.items():
            rec[k + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        rec["penalty_ms_replayed"] = round(rec["wgangp_replayed_ms"]["median"] - rec["wgan_replayed_ms"]["median"], 3)
        rec["graph_nodes"] = {k: m.graph_nodes for k, m in models.items() if k.endswith("replayed")}
        rec["losses_finite"] = all(v == v and abs(v) < 1e30 for m in models.values() for v in m.get_current_losses().values())
        rec["penalty_logged"] = models["wgangp_replayed"].get_current_losses().get("l_D_I_grad_penalty")
        print(json.dumps(rec), flush=True)
        del models
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
