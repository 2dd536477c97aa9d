"""Micro-benchmark of the CLIP ViT-B/32 tower's input-gradient backward (vts_clip_visual_backward) next to the forward it follows
(vts_clip_visual_forward, and vts_clip_visual_forward_tape, which also keeps what the backward reads), and of the differentiable front
end (vts_clip_area_preprocess and its backward on a 1024 x 1024 image), batches 1 and 4, each inside a HIP graph holding `--reps` calls
(the Python / ctypes enqueue costs ~15 us per call: eager timing floors there); median / min / max over `--replays` timed replays.  The
cotangents enter at the embedding and at blocks 4, 8 and 12, as a multi-level discriminator would supply them.
   python tools/mb_clip_bwd.py [--reps 10] [--replays 15] [--json out.json]
Seeded stand-in weights: times do not depend on the values."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "visual-tactile-synthesis_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from mb_clip import graph_us  # noqa: E402
from vts import ops  # noqa: E402

TAPS = (4, 8, 12)


def main(args):
    from models.clip_visual import ClipVisual

    dev = torch.device("cuda:0")
    net = ClipVisual().to(dev)
    flat, flat_t, cfg = net.flat_weights(), net.flat_weights_t(), net._ccfg
    out = {"weight_halfs": flat.numel(), "weight_t_halfs": flat_t.numel(), "taps": TAPS, "reps_per_graph": args.reps, "replays": args.replays}
    for batch in (1, 4):
        img = torch.rand(batch, 3, 1024, 1024, device=dev) * 2 - 1
        x16 = ops.clip_area_preprocess(img)
        tape, ws_f, ws_b = (torch.empty(k, dtype=torch.float32, device=dev) for k in (
            ops.clip_visual_tape_floats(cfg, batch), ops.clip_visual_forward_ws_floats(cfg, batch), ops.clip_visual_backward_ws_floats(cfg, batch)))
        emb, dx, dimg = torch.empty(batch, 512, device=dev), torch.empty(batch, 3, 224, 224, device=dev), torch.empty_like(img)
        d_out, d_hid = torch.randn(batch, 512, device=dev) * 1e-3, torch.randn(len(TAPS), batch, 50, 768, device=dev) * 1e-3
        res = {
            "forward_us": graph_us(lambda: ops.clip_visual_forward(cfg, flat, x16, out=emb, ws=ws_f), args.reps, args.replays),
            "forward_tape_us": graph_us(lambda: ops.clip_visual_forward_tape(cfg, flat, x16, tape, out=emb, ws=ws_f), args.reps, args.replays),
            "backward_us": graph_us(lambda: ops.clip_visual_backward(cfg, flat, flat_t, tape, batch, d_out=d_out, taps=TAPS, d_hidden=d_hid, dx=dx,
                                                                     ws=ws_b), args.reps, args.replays),
            "backward_embedding_only_us": graph_us(lambda: ops.clip_visual_backward(cfg, flat, flat_t, tape, batch, d_out=d_out, dx=dx, ws=ws_b),
                                                   args.reps, args.replays),
            "area_preprocess_1024_us": graph_us(lambda: ops.clip_area_preprocess(img, out=x16), args.reps, args.replays),
            "area_preprocess_bwd_1024_us": graph_us(lambda: ops.clip_area_preprocess_bwd(dx, 1024, 1024, dx=dimg), args.reps, args.replays),
        }
        res["backward_over_forward"] = res["backward_us"][0] / res["forward_us"][0]
        out["batch%d" % batch] = res
        for k, v in res.items():
            if k.endswith("_us"):
                print("batch %d  %-28s %8.1f us (min %.1f max %.1f)" % ((batch, k[:-3]) + v))
        print("batch %d  backward / forward = %.2f" % (batch, res["backward_over_forward"]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mb_clip_bwd.py needs a GPU: a time cannot be measured without one")
    result = main(args)
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
