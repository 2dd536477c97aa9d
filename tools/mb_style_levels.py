"""Timings behind profiles/r17_style_levels.md (--num_layer_style_code > 1, concat + tile).

  python tools/mb_style_levels.py levels      # per decoder level at 1024 x 1024, 4 images: the class-bias route (vts_style_bias(_bwd) beside
                                              # the x / skip launches) against the two-source launches on a MATERIALISED tile, forward and
                                              # weight gradient, each timed as 10 launches inside one HIP graph (the method of tools/mb_px.py)
  python tools/mb_style_levels.py step K...   # ms per replayed skitG training step at 1024 x 1024, 4 images, for each level count K
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-tactile-synthesis_amd"))
import torch  # noqa: E402

from vts import lib as L, ops  # noqa: E402
from vts.ops import Act  # noqa: E402

dev = torch.device("cuda:0")
RELU, TANH = L.ACT_RELU, L.ACT_TANH


def timeit(fn, reps=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def level(i, n=4, size=1024, ngf=10, k=512):
    ch = [ngf * min(2 ** j, 8) for j in range(8)]
    cx, cout, ih = ch[i], (3 if i == 0 else ch[i - 1]), size >> (i + 1)
    csk = 0 if i == 0 else ch[i]
    x = Act(torch.randn(n, cx, ih, ih, device=dev))
    skip = Act(torch.randn(n, csk, ih, ih, device=dev)) if csk else None
    code = torch.randn(n, k, device=dev)
    w = torch.randn(cx + k + csk, cout, 4, 4, device=dev) * 0.05
    dw = torch.zeros_like(w)
    out = torch.zeros(n, cout, 2 * ih, 2 * ih, device=dev)
    g = torch.randn(n, cout, 2 * ih, 2 * ih, device=dev)
    rows, wf, dwf = cout * 16, w.view(-1), dw.view(-1)
    kw = dict(stride=2, pad=1, transposed=True, act_in=RELU)

    def fwd_bias():
        ops.conv4x4(x, w, 16, rows, cout, out, **kw)
        if skip is not None:
            ops.conv4x4(skip, wf[(cx + k) * rows:], 16, rows, cout, out, accumulate=True, **kw)
        ops.style_bias(code, wf[cx * rows:(cx + k) * rows], out, act_out=TANH if i == 0 else 0)

    def dw_bias():
        ops.wgrad4x4(x, Act(g), dwf[:cx * rows], act_lo=RELU, stride=2, pad=1)
        if skip is not None:
            ops.wgrad4x4(skip, Act(g), dwf[(cx + k) * rows:], act_lo=RELU, stride=2, pad=1)
        ops.style_bias_bwd(g, code, dwf[cx * rows:(cx + k) * rows])

    t = dict(fwd_bias=timeit(fwd_bias), dw_bias=timeit(dw_bias), style_bias=timeit(lambda: ops.style_bias(code, wf[cx * rows:(cx + k) * rows], out)),
             style_bias_bwd=timeit(lambda: ops.style_bias_bwd(g, code, dwf[cx * rows:(cx + k) * rows])))
    tile = Act(code[:, :, None, None].expand(-1, -1, ih, ih).contiguous())

    def fwd_tile():
        ops.conv4x4(x, w, 16, rows, cout, out, in1=tile, act_out=TANH if (i == 0) else 0, **kw)
        if skip is not None:
            ops.conv4x4(skip, wf[(cx + k) * rows:], 16, rows, cout, out, accumulate=True, **kw)

    def dw_tile():
        ops.wgrad4x4(x, Act(g), dwf[:(cx + k) * rows], lo1=tile, act_lo=RELU, stride=2, pad=1)
        if skip is not None:
            ops.wgrad4x4(skip, Act(g), dwf[(cx + k) * rows:], act_lo=RELU, stride=2, pad=1)

    t.update(fwd_tile=float("nan"), dw_tile=float("nan"), tile_mb=tile.data.numel() * 4 / 2 ** 20)
    try:
        t.update(fwd_tile=timeit(fwd_tile, reps=3))
        t.update(dw_tile=timeit(dw_tile, reps=3))
    except RuntimeError as e:      # the existing launch may refuse the shape (a 2 GiB operand)
        print("level %d: the tile route is refused: %s" % (i, str(e).splitlines()[0]))
    print("level %d  N%d %d+%d+%d ch %dx%d -> %d ch: forward class-bias %.0f us (style_bias alone %.0f) vs tile %.0f us | dW class-bias %.0f us "
          "(style_bias_bwd alone %.0f) vs tile %.0f us | tile %.0f MiB" % (i, n, cx, k, csk, ih, ih, cout, t["fwd_bias"], t["style_bias"], t["fwd_tile"],
                                                                         t["dw_bias"], t["style_bias_bwd"], t["dw_tile"], t["tile_mb"]), flush=True)


def step(k, n=4, size=1024, steps=20):
    from torch.utils.data import default_collate

    from data.synthetic_dataset import make_sample
    from models import create_model
    from options.train_options import TrainOptions

    flags = ("--model skitG --gpu_ids 0 --lambda_G1_lpips 0 --lambda_G2_lpips 0 --use_vision_aided_loss False --lambda_G2_GAN_feat 0 "
             "--checkpoints_dir /tmp/vts_mb_ckpt --name mb_style_levels --crop_size %d --batch_size %d --num_layer_style_code %d" % (size, n, k))
    opt = TrainOptions(cmd_line=flags).parse()
    model = create_model(opt)
    model.setup(opt)
    model.parallelize()
    model.train()
    batch = default_collate([make_sample(size, 64, 64, 900 + j, style_dim=opt.style_code_dim) for j in range(n)])
    model.set_input(batch, phase="train")
    for _ in range(5):
        model.optimize_parameters(epoch=1)
    torch.cuda.synchronize()
    assert model._graphs is not None
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        model.optimize_parameters(epoch=1)
    e1.record()
    torch.cuda.synchronize()
    print("skitG %dx%d, %d images, num_layer_style_code %d: %.3f ms per replayed step, peak memory %.0f MiB" % (
        size, size, n, k, e0.elapsed_time(e1) / steps, torch.cuda.max_memory_allocated() / 2 ** 20), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "levels":
        for i in (0, 1, 2, 3):
            level(i)
    else:
        for k in sys.argv[2:]:
            step(int(k))
