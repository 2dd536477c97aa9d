"""Micro-benchmark of the SPADE kernels (csrc/vts_spade.hip) and of the SPADE generator's schedules, timed inside HIP graphs (eager timing
floors at the Python enqueue, tools/README.md), best of 5 replays.  Shapes: the reference's training shape (N 16, ngf 64, 32 x 32 patches:
1024 channels at 4 x 4 and 8 x 8, 512 at 16 x 16, 256 at 32 x 32; spectral norm of a 1024 x 9216 weight) and one full-image eval shape.
Bytes are the algorithmic bytes of each kernel (what it must read and write once).

  python tools/mb_spade.py [--eval-width 512]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-tactile-synthesis_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from vts import engine, ops  # noqa: E402
from mb_px import timeit  # noqa: E402

dev = torch.device("cuda:0")
HBM = 8e6        # bytes per microsecond (8 TB/s peak)


def report(name, shape, us, by):
    print("%-22s %-18s: %8.2f us  %8.2f MB  %7.1f GB/s  %.3f of HBM peak" % (name, "x".join(map(str, shape)), us, by / 1e6, by / us / 1e3, by / us / HBM), flush=True)


def best(fn, reps=20):
    return min(timeit(fn, reps) for _ in range(5))


def kernels():
    for shape in ((16, 1024, 4, 4), (16, 1024, 8, 8), (16, 512, 16, 16), (16, 256, 32, 32)):
        n, c, h, w = shape
        x, gamma, beta, g = (torch.randn(shape, device=dev) for _ in range(4))
        gp = torch.randn(n, c, h + 2, w + 2, device=dev)
        a = ops.norm_stats(x, 1)
        out, outp = torch.empty_like(x), torch.empty_like(gp)
        el = 4.0 * x.numel()
        report("modulate", shape, best(lambda: ops.spade_modulate(x, a.mean, a.rstd, gamma, beta, act=1, out=out)), 4 * el)
        report("modulate -> padded", shape, best(lambda: ops.spade_modulate(x, a.mean, a.rstd, gamma, beta, act=1, out_pad=1, out=outp)), 3 * el + 4.0 * gp.numel())
        # backward: reads g, x, gamma, beta, writes dgamma, dbeta, h; the apply pass reads h, x and writes dx
        report("modulate bwd batch", shape, best(lambda: ops.spade_modulate_bwd(gp, x, a.mean, a.rstd, gamma, beta, 1, act=1, g_pad=1)), 10 * el)
        report("modulate bwd instance", shape, best(lambda: ops.spade_modulate_bwd(g, x, a.mean, a.rstd, gamma, beta, 0, act=1)), 10 * el)
        report("modulate bwd frozen", shape, best(lambda: ops.spade_modulate_bwd(g, x, a.mean, a.rstd, gamma, beta, 2, act=1)), 7 * el)
        up, dn = torch.empty(n, c, 2 * h, 2 * w, device=dev), torch.empty_like(x)
        report("nearest up2", shape, best(lambda: ops.nearest_up2(x, out=up)), 5 * el)
        report("nearest up2 adjoint", shape, best(lambda: ops.nearest_up2_bwd(up, dn)), 5 * el)
    seg = torch.randn(16, 1, 32, 32, device=dev)
    for size in ((4, 4), (16, 16)):
        o = torch.empty(16, 1, *size, device=dev)
        report("nearest resize", (16, 1, 32, 32) + size, best(lambda: ops.nearest_resize(seg, size, out=o)), 8.0 * o.numel())
        report("nearest resize adjoint", (16, 1, 32, 32) + size, best(lambda: ops.nearest_resize_bwd(o, seg)), 4.0 * (o.numel() + seg.numel()))
    for shape in ((1024, 1024, 3, 3), (512, 1024, 3, 3), (256, 512, 1, 1)):
        w = torch.randn(shape, device=dev) * 0.01
        co, k = shape[0], w.numel() // shape[0]
        u, v = torch.nn.functional.normalize(torch.randn(co, device=dev), dim=0), torch.nn.functional.normalize(torch.randn(k, device=dev), dim=0)
        w_sn, sigma, dw, g = torch.empty_like(w), torch.empty(1, device=dev), torch.empty_like(w), torch.randn(shape, device=dev)
        el = 4.0 * w.numel()
        report("spectral norm train", (co, k), best(lambda: ops.spectral_norm(w, u, v, True, w_sn, sigma)), 4 * el)       # W read 3 x, W / sigma written
        report("spectral norm eval", (co, k), best(lambda: ops.spectral_norm(w, u, v, False, w_sn, sigma)), 3 * el)
        report("spectral norm bwd", (co, k), best(lambda: ops.spectral_norm_bwd(g, w_sn, u, v, sigma, dw)), 4 * el)        # g read 2 x, W / sigma read, dw written


def generator(ngf, n, width, train, reps):
    import argparse as ap

    from models import networks
    from vts.optim import FlatParams

    opt = ap.Namespace(normG="spectralspadesyncbatch3x3", semantic_nc=1, num_upsampling_layers=3, output_width=width, aspect_ratio=1.0, use_vae=False)
    G = networks.define_G(1, 5, ngf, "spade", norm=opt.normG, opt=opt, init_type="kaiming", gpu_ids=[0])
    FlatParams(G)
    G.train(train)
    seg, cot = torch.randn(n, 1, width, width, device=dev), torch.randn(n, 5, width, width, device=dev)
    us = best(lambda: engine.spade_forward(G, seg, keep=False), reps)
    print("generator ngf %d N %d %dx%d %s forward: %.3f ms" % (ngf, n, width, width, "train" if train else "eval", us / 1e3), flush=True)
    if train:
        def step():
            _, ctx = engine.spade_forward(G, seg)
            engine.spade_backward(G, ctx, cot)
        us = best(step, reps)
        print("generator ngf %d N %d %dx%d forward + backward: %.3f ms" % (ngf, n, width, width, us / 1e3), flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--eval-width", type=int, default=512)
    p.add_argument("--skip-kernels", action="store_true")
    args = p.parse_args()
    if not args.skip_kernels:
        kernels()
    generator(64, 16, 32, True, 3)
    generator(64, 1, args.eval_width, False, 2)
