"""Micro-benchmark of vts_modconv_scale_dot (the HBM-bound pass of the style-vector ModulatedConv2d backward), 20 launches in one HIP
graph per figure, best of 5 replays.   python tools/mb_modconv.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-tactile-synthesis_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from vts import ops  # noqa: E402
from mb_px import timeit  # noqa: E402

dev = torch.device("cuda:0")
HBM = 8e6        # bytes per microsecond (8 TB/s peak)


def case(shape, with_out):
    n, c = shape[0], shape[1]
    a, b = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
    f, dot = torch.rand(n * c, device=dev) + 0.5, torch.empty(n * c, device=dev)
    out = torch.empty_like(a) if with_out else None
    us = min(timeit(lambda: ops.modconv_scale_dot(a, b, dot, f=f if with_out else None, out=out, alpha=0.5)) for _ in range(5))
    by = 4.0 * a.numel() * (3 if with_out else 2)
    print("scale_dot %-18s %-22s: %7.2f us  %6.2f MB  %7.1f GB/s  %.3f of HBM peak" % (
        "x".join(map(str, shape)), "2 reads + 1 write" if with_out else "2 reads", us, by / 1e6, by / us / 1e3, by / us / HBM))


if __name__ == "__main__":
    for shape in ((2, 512, 32, 32), (2, 32, 128, 128), (4, 16, 256, 256)):
        for with_out in (True, False):
            case(shape, with_out)
