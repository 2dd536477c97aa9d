"""Microbenchmark of the Frechet distance behind the baselines' SIFID / T_FID metrics: the per-pair path (a Python loop of
ops.frechet_distance, one chain of 126 launches per pair, 122 of them a single workgroup) against the batched entry (ops.frechet_distance_batched, three
launches for all pairs) on the same inputs, both replayed from a captured HIP graph; and one whole compute_metrics() of pix2pix at 32 patches.

    python tools/mb_frechet.py [--out profiles/r16_baseline_metrics.json] [--pairs 1 8 64 192] [--loop_max 64]

D = 64, P = 147 * 147 = 21609 (the Inception map of a 299 x 299 input: the T_SIFID shape).  The loop is timed up to --loop_max pairs (its
graph holds 126 kernel nodes per pair); beyond that its time is the per-pair time of the largest measured n, marked `extrapolated`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "visual-tactile-synthesis_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")
import torch  # noqa: E402


def graph_time_ms(fn, reps):
    """median time of one replay of fn() captured in a HIP graph (one eager call first: workspaces grow outside the capture)"""
    from vts import ops
    fn()
    torch.cuda.synchronize()
    ops.freeze_ws("mb_frechet")
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            out = fn()
        g.replay()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
    finally:
        ops.release_ws("mb_frechet")
    times.sort()
    return times[len(times) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8, 64, 192])
    ap.add_argument("--loop_max", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip_model", action="store_true")
    args = ap.parse_args()
    from vts import ops

    dev = torch.device("cuda:0")
    d, p = 64, 147 * 147
    res = {"D": d, "P": p, "device": torch.cuda.get_device_name(0), "rows": []}
    g = torch.Generator(device=dev).manual_seed(16)
    per_pair_loop = None
    for n in args.pairs:
        mix = torch.randn(d, d, generator=g, device=dev) / d ** 0.5 + torch.eye(d, device=dev)      # (inputs only: drawn with torch)
        f1 = mix @ torch.randn(n, d, p, generator=g, device=dev)
        f2 = 1.3 * (mix.t() @ torch.randn(n, d, p, generator=g, device=dev)) + 0.1

        def batched():
            return ops.frechet_distance_batched(f1, f2)

        def loop():
            return torch.cat([ops.frechet_distance(f1[i], f2[i]) for i in range(n)])

        tb, vb = graph_time_ms(batched, args.reps)
        row = {"n": n, "batched_ms": tb, "batched_launches": 3}
        if n <= args.loop_max:
            tl, vl = graph_time_ms(loop, args.reps)
            per_pair_loop = tl / n
            row.update(loop_ms=tl, loop_launches=126 * n, extrapolated=False,
                       max_abs_difference=float((vb - vl).abs().max()), max_value=float(vl.abs().max()))
        elif per_pair_loop is not None:
            row.update(loop_ms=per_pair_loop * n, loop_launches=126 * n, extrapolated=True)
        row["speedup"] = row["loop_ms"] / tb if "loop_ms" in row else None
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del f1, f2
    if not args.skip_model:
        res["compute_metrics"] = model_time(dev, args.reps)
        print(json.dumps(res["compute_metrics"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


def model_time(dev, reps):
    """wall time of one whole compute_metrics() of pix2pix on 32 patches of 32 x 32 (VTS_SIFID=1, --eval_T_FID: 8 - 2 LPIPS + T_FID names),
    with the batched Frechet entry and with engine.sifid_pairs_batched swapped for the per-pair loop engine.sifid_pairs"""
    os.environ["VTS_SIFID"] = "1"
    from models import create_model
    from options.train_options import TrainOptions
    from vts import engine

    opt = TrainOptions(cmd_line="--model pix2pix --gpu_ids 0 --checkpoints_dir /tmp/vts_mb --name mb_frechet --dataset_mode patchskit "
                                "--eval_T_FID --use_hip_graph False").parse()
    model = create_model(opt)
    model.setup(opt)
    model.parallelize()
    n, s = 32, 32
    g = torch.Generator().manual_seed(17)
    batch = {"S_images": torch.rand(n, 1, s, s, generator=g) * 2 - 1, "M_images": torch.ones(n, 1, s, s),
             "I_images": torch.rand(n, 3, s, s, generator=g) * 2 - 1, "T_images": torch.rand(n, 2, s, s, generator=g) * 0.6 - 0.3,
             "I_masks": torch.ones(n, s, s), "name": ["mb"] * n, "S_paths": ["mb.png"] * n, "augmentation_params": {}}
    model.set_input(batch, phase="test")
    model.test()

    def timed():
        model.compute_metrics()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            vals = model.compute_metrics()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2], vals

    t_batched, v_batched = timed()
    keep = engine.sifid_pairs_batched
    engine.sifid_pairs_batched = lambda net, a, b, batch=16: engine.sifid_pairs(net, a, b, batch)
    try:
        t_loop, v_loop = timed()
    finally:
        engine.sifid_pairs_batched = keep
    return {"patches": n, "pairs": 3 * n + 1, "batched_ms": t_batched, "loop_ms": t_loop, "values_batched": v_batched, "values_loop": v_loop}


if __name__ == "__main__":
    main()
