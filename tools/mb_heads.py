"""Micro-benchmark of the PatchGAN prediction heads and of the few-copy weight-gradient flush, one launch each inside a HIP graph
(20 launches per graph, as tools/mb_small.py):
    python tools/mb_heads.py
  - the twelve head forward shapes of the step (64 -> 1, stride 1, pad 2: full-size maps of D1 / D2's image passes, the 640- / 256-patch
    passes of D2), weights as [1:] views of a flat buffer (the step's layout: parameters sit behind the one-float head bias);
  - the three head weight-gradient shapes (one low-resolution channel), with their reduction;
  - the reduction table of the generator backward's first flush (the ten inner U-Net layers: 116 MB of partials, 4 .. 102 copies per
    job), each job alone and all ten in one launch.
VTS_LIB_PATH=<library> for an A/B of two builds on one box; the last line is the sum."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-tactile-synthesis_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from vts import lib as L, ops  # noqa: E402
from vts.ops import Act  # noqa: E402
from mb_px import timeit  # noqa: E402

dev = torch.device("cuda:0")
TOTAL = [0.0]


def flat_view(*shape):
    w = torch.randn(*shape, device=dev) * 0.1
    flat = torch.empty(w.numel() + 1, device=dev)
    flat[1:].copy_(w.view(-1))
    return flat[1:].view(shape)


def head(N, C, H):
    OH = H + 1
    x = Act(torch.randn(N, C, H, H, device=dev), torch.rand(N * C, device=dev) + 0.5, torch.randn(N * C, device=dev) * 0.1)
    w, b = flat_view(1, C, 4, 4), torch.randn(1, device=dev)
    out = torch.zeros(N, 1, OH, OH, device=dev)
    us = timeit(lambda: ops.conv4x4(x, w, C * 16, 16, 1, out, bias=b, stride=1, pad=2, act_in=L.ACT_LRELU))
    by = 4.0 * (N * C * H * H + out.numel() + w.numel())
    TOTAL[0] += us
    print("head  N%-3d %dx%3d^2 -> 1x%3d^2 : %7.1f us %7.1f GB/s  %s" % (N, C, H, OH, us, by / us / 1e3, L.load().vts_last_kernel().decode()))


def whead(N, CH, HH):
    LH = HH + 1
    lo = Act(torch.randn(N, 1, LH, LH, device=dev))
    hi = Act(torch.randn(N, CH, HH, HH, device=dev), torch.rand(N * CH, device=dev) + 0.5, torch.randn(N * CH, device=dev) * 0.1)
    dw = flat_view(1, CH, 4, 4)
    us = timeit(lambda: ops.wgrad4x4(lo, hi, dw, act_hi=L.ACT_LRELU, stride=1, pad=2, defer=False))
    TOTAL[0] += us
    print("wgrad N%-3d lo 1x%3d^2 hi %dx%3d^2 : %7.1f us  (with its reduction)  %s" % (N, LH, CH, HH, us, L.load().vts_last_kernel().decode()))


# (layer, elements of dw, partial copies) of the generator backward's first flush at 1024^2, batch 4 (copies = workspace floats / elements,
# vts_wgrad4x4_ws_floats of each layer)
FLUSH = [("up3", 102400, 64), ("up4", 204800, 25), ("up5", 204800, 10), ("up6", 204800, 8), ("up7", 757760, 4), ("down7", 102400, 4),
         ("down6", 102400, 8), ("down5", 102400, 16), ("down4", 102400, 25), ("down3", 51200, 102)]


def flush():
    lib = L.load()
    flat = torch.empty(sum(n for _, n, _ in FLUSH) + 1, device=dev)
    jobs = (L.ReduceJob * len(FLUSH))()
    keep, off = [], 1
    for j, (name, nel, pw) in zip(jobs, FLUSH):
        part = torch.randn(pw, nel, device=dev)
        keep.append(part)
        j.dw, j.nel, j.accumulate, j.nseg = flat[off:off + nel].data_ptr(), nel, 0, 1
        j.part[0], j.pw[0] = part.data_ptr(), pw
        off += nel
    for i, (name, nel, pw) in enumerate(FLUSH):
        one = (L.ReduceJob * 1)(jobs[i])
        us = timeit(lambda: L.check(lib.vts_wgrad_reduce_batch(one, 1, L.stream()), "reduce"))
        print("reduce %-6s %7d elements x %3d copies (%5.1f MB) : %7.1f us %7.1f GB/s" % (name, nel, pw, 4e-6 * nel * pw, us, 4.0 * nel * pw / us / 1e3))
    us = timeit(lambda: L.check(lib.vts_wgrad_reduce_batch(jobs, len(FLUSH), L.stream()), "reduce"))
    mb = sum(4e-6 * n * p for _, n, p in FLUSH)
    TOTAL[0] += us
    print("reduce flush of %d jobs (%5.1f MB) : %7.1f us %7.1f GB/s" % (len(FLUSH), mb, us, mb * 1e3 / us))


if __name__ == "__main__":
    print({k: v for k, v in os.environ.items() if k.startswith("VTS_")})
    for N in (4, 8):
        for H in (34, 66, 130):
            head(N, 64, H)
    for H in (6, 4, 3):
        for N in (640, 256):
            head(N, 64, H)
    for H in (130, 66, 34):
        whead(8, 64, H)
    flush()
    print("sum : %7.1f us" % TOTAL[0])
