"""The PatchGAN prediction heads (forward on full-size and on small maps, weight gradient) and the batched weight-gradient reduction
at the smallest shapes that can still go wrong.

Heads: judged elementwise against float64 with the rule of oracle/launch_ref.py, |got - ref| <= c u sqrt(K) absref with K = 16 C and
c = 2 for the convolution family (K = N LH LW and c = 1.5 for the weight gradient), the constants tests/test_step_launches_gpu.py
holds the step's own launches to.  Reduction: bitwise against a host restatement of its summation order in fp32 tensor adds.
Every operand sits between NaN guard bands (a read outside an operand poisons the result, a write outside the output shows in the
band), and every case runs twice with torch.equal on the results."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detrand  # noqa: E402  (checker only)
from oracle import launch_ref as LR  # noqa: E402

C_CONV, C_WGRAD = 2.0, 1.5
BAND = 1024
LRELU = 1


def _dev():
    return torch.device("cuda:0")


class Banded:
    """a tensor on the device between two NaN bands; off = 1 makes it a [1:]-style view (4-byte aligned only)"""

    def __init__(self, t, off=0, fill=None):
        n = t.numel()
        self.flat = torch.full((2 * BAND + n + off,), float("nan"), dtype=torch.float32, device=_dev())
        assert self.flat.data_ptr() % 16 == 0
        self.lo, self.hi = BAND + off, BAND + off + n
        self.v = self.flat[self.lo:self.hi].view(t.shape)
        if fill is None:
            self.v.copy_(t)
        else:
            self.v.fill_(fill)

    def bands_intact(self):
        return bool(torch.isnan(self.flat[:self.lo]).all()) and bool(torch.isnan(self.flat[self.hi:]).all())


def _affine(n, c, seed):
    return 1.0 + 0.3 * detrand.uniform((n, c), seed, "sc"), 0.2 * detrand.uniform((n, c), seed, "sh")


# ---- head forward ------------------------------------------------------------------------------------------------------------------

def _head_case(N, Cin, IH, IW, *, affine=True, bias=True, pad_dx=0, strided=False, wview=False, seed=7):
    """returns (run, ref, unit, banded operands): run() launches the head on a fresh NaN-filled output and returns (out, bands intact?)"""
    from vts import ops
    from vts.ops import Act
    OH, OW = IH + 1, IW + 1
    x = detrand.uniform((N, Cin, IH, IW), seed, "x") - 0.5
    w = (detrand.uniform((1, Cin, 4, 4), seed, "w") - 0.5) * 0.2
    b = detrand.uniform((1,), seed, "b") if bias else None
    aff = _affine(N, Cin, seed) if affine else None
    act = LRELU if affine else 0
    if strided:     # a channel slice of a wider tensor: the batch stride exceeds the plane (the extra channel stays NaN)
        wide = Banded(torch.empty(N, Cin + 1, IH, IW), fill=float("nan"))
        wide.v[:, :Cin].copy_(x)
        xv, xb = wide.v[:, :Cin], wide
    else:
        xb = Banded(x)
        xv = xb.v
    wb = Banded(w, off=1 if wview else 0)
    sc = Banded(aff[0]) if affine else None
    sh = Banded(aff[1]) if affine else None
    bb = Banded(b) if bias else None
    in0 = Act(xv, sc.v.view(-1), sh.v.view(-1)) if affine else Act(xv)
    d = dict(stride=1, pad=2, pad_dx=pad_dx, OH=OH, OW=OW, transposed=0, in0={"C": Cin}, in1={"C": 0}, act_in=act, act_out=0, Cout=1,
             ws_co=Cin * 16, ws_ci=16, accumulate=0)
    ref, unit = LR.conv4x4(d, LR.Opnd(x, aff[0] if affine else None, aff[1] if affine else None), w, bias=b)["out"]

    def run():
        ob = Banded(torch.empty(N, 2 if strided else 1, OH, OW), fill=float("nan"))
        out = ob.v[:, :1]
        ops.conv4x4(in0, wb.v, Cin * 16, 16, 1, out, bias=bb.v if bias else None, stride=1, pad=2, pad_dx=pad_dx, act_in=act)
        ok = ob.bands_intact() and (not strided or bool(torch.isnan(ob.v[:, 1:]).all()))
        return out.clone(), ok
    return run, ref, unit, [t for t in (xb, wb, sc, sh, bb) if t is not None]


def _judge_head(run, ref, unit, keep, kernel_prefix, tag):
    from vts import lib as L
    out, ok = run()
    k = L.load().vts_last_kernel().decode()
    assert k.startswith(kernel_prefix), k
    ratio, at = LR.worst(out, ref, unit)
    print("%s %s worst err / (u sqrt(K) absref) = %.4f" % (tag, k, ratio))
    assert ok and all(t.bands_intact() for t in keep), "a guard band changed"
    assert ratio <= C_CONV, (tag, ratio, at)
    again, ok2 = run()
    assert ok2 and torch.equal(again, out)


FULL = [(3, 64, 31, 31), (2, 20, 34, 40), (1, 8, 66, 66)]      # one tile with padding on all sides; ragged channels and tiles; the minimum C


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine_lrelu", "plain"])
@pytest.mark.parametrize("geom", FULL, ids=lambda g: "N%d_C%d_%dx%d" % g)
def test_head_forward_full_maps(geom, affine, bias):
    run, ref, unit, keep = _head_case(*geom, affine=affine, bias=bias)
    _judge_head(run, ref, unit, keep, "conv_head_kernel<", "head %s affine %d bias %d" % (geom, affine, bias))


@pytest.mark.parametrize("variant", ["pad_dx", "strided", "weight_view"])
def test_head_forward_full_maps_layouts(variant):
    kw = {"pad_dx": dict(pad_dx=1), "strided": dict(strided=True), "weight_view": dict(wview=True)}[variant]
    run, ref, unit, keep = _head_case(2, 20, 34, 40, seed=11, **kw)
    _judge_head(run, ref, unit, keep, "conv_head_kernel<", "head " + variant)


SMALL = [(33, 64, 6, False), (37, 64, 3, False), (32, 20, 4, False), (33, 64, 6, True)]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "N%d_C%d_%d%s" % (c[0], c[1], c[2], "_wview" if c[3] else ""))
def test_head_forward_small_maps(case):
    N, Cin, H, wview = case
    run, ref, unit, keep = _head_case(N, Cin, H, H, wview=wview, seed=13)
    _judge_head(run, ref, unit, keep, "conv_head_small_kernel", "small head %s" % (case,))


# ---- head weight gradient ----------------------------------------------------------------------------------------------------------

WHEAD = [(2, 64, 35, 35, 2, True), (3, 20, 67, 40, 2, True), (2, 5, 16, 33, 1, False), (8, 64, 131, 131, 2, True), (1, 64, 16, 32, 2, True)]


@pytest.mark.parametrize("shape", WHEAD, ids=lambda s: "N%d_C%d_lo%dx%d_p%d" % s[:5])
def test_head_weight_gradient(shape):
    from vts import lib as L
    from vts import ops
    from vts.ops import Act
    n, ch, lh, lw, pad, affine = shape
    hh, hw = lh - 1 + 4 - 2 * pad, lw - 1 + 4 - 2 * pad
    lo = detrand.uniform((n, 1, lh, lw), 4, "lo") - 0.5
    hi = detrand.uniform((n, ch, hh, hw), 4, "hi") - 0.5
    aff = _affine(n, ch, 4) if affine else None
    act = LRELU if affine else 0
    lob, hib = Banded(lo), Banded(hi)
    sc, sh = (Banded(aff[0]), Banded(aff[1])) if affine else (None, None)
    hi_op = Act(hib.v, sc.v.view(-1), sh.v.view(-1)) if affine else Act(hib.v)
    d = dict(stride=1, pad=pad, pad_dx=0, N=n, LH=lh, LW=lw, act_lo=0, act_hi=act, accumulate=0)
    ref, unit = LR.wgrad4x4(d, LR.Opnd(lo, None, None), LR.Opnd(hi, aff[0] if affine else None, aff[1] if affine else None))["dw"]

    def run():
        dwb = Banded(torch.empty(1, ch, 4, 4), off=1, fill=float("nan"))      # dW lives behind the one-float bias gradient
        ops.wgrad4x4(Act(lob.v), hi_op, dwb.v, act_hi=act, stride=1, pad=pad, defer=False)
        return dwb.v.clone(), dwb.bands_intact()
    dw, ok = run()
    assert L.load().vts_last_kernel().decode() == "wgrad_head_kernel"
    ratio, at = LR.worst(dw, ref, unit)
    print("head wgrad %s worst err / (u sqrt(K) absref) = %.4f" % (shape, ratio))
    assert ok and all(t.bands_intact() for t in (lob, hib, sc, sh) if t is not None), "a guard band changed"
    assert ratio <= C_WGRAD, (shape, ratio, at)
    again, ok2 = run()
    assert ok2 and torch.equal(again, dw)


# ---- batched reduction --------------------------------------------------------------------------------------------------------------

def _tree(a):
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def host_reduce(parts, dw0, accumulate):
    """the summation order of vts_wgrad_reduce_batch in fp32 tensor adds.  parts: [copies, nel] per segment.
    <= 256 copies: "virtual wave" w = 0..15 sums copies w + 16 u + 128 i into a[u] (i ascending, from +0), the segment sum is the
    pairwise tree over a0..a7, segments are added in order into s_w (from +0), result = s_0 + ... + s_15 left to right.
    > 256 copies: wave w's lane group g = 0..3 sums copies 4 w + g + 64 u + 512 i the same way, groups combine as (0 + 1) + (2 + 3)."""
    nel = parts[0].shape[1]
    zero = torch.zeros(nel, dtype=torch.float32)
    narrow = max(p.shape[0] for p in parts) > 256

    def chain(first, step_u, step_i):
        s = zero.clone()
        for p in parts:
            a = [zero.clone() for _ in range(8)]
            for k in range(first, p.shape[0], step_i):
                for u in range(8):
                    if k + step_u * u < p.shape[0]:
                        a[u] = a[u] + p[k + step_u * u]
            s = s + _tree(a)
        return s
    total = None
    for w in range(16):
        if narrow:
            g = [chain(4 * w + cg, 64, 512) for cg in range(4)]
            sw = (g[0] + g[1]) + (g[2] + g[3])
        else:
            sw = chain(w, 16, 128)
        total = sw if w == 0 else total + sw
    return dw0 + total if accumulate else total


def _reduce_jobs(specs, seed):
    """specs: (nel, [copies per segment], accumulate, part offset 0 / 1).  Returns (launch, expected list, the dw holders)."""
    from vts import lib as L
    lib = L.load()
    jobs = (L.ReduceJob * len(specs))()
    g = torch.Generator().manual_seed(seed)
    holders, expect, keep = [], [], []
    for j, (nel, pws, acc, poff) in zip(jobs, specs):
        dw0 = torch.randn(nel, generator=g)
        parts = [torch.randn(pw, nel, generator=g) * (10.0 ** (i - 1)) for i, pw in enumerate(pws)]
        pb = [Banded(p, off=poff) for p in parts]
        keep += pb
        expect.append(host_reduce(parts, dw0, acc))
        holders.append(dw0)
        j.nel, j.accumulate, j.nseg = nel, int(acc), len(pws)
        for i, b in enumerate(pb):
            j.part[i], j.pw[i] = b.v.data_ptr(), pws[i]

    def launch():
        dws = [Banded(d0, off=1) for d0 in holders]      # dW as a [1:] view; seeded (accumulate) or overwritten
        for j, b in zip(jobs, dws):
            j.dw = b.v.data_ptr()
        L.check(lib.vts_wgrad_reduce_batch(jobs, len(specs), L.stream()), "vts_wgrad_reduce_batch")
        torch.cuda.synchronize()
        return [b.v.cpu() for b in dws], all(b.bands_intact() for b in dws + keep)
    return launch, expect


def _check_reduce(specs, seed):
    launch, expect = _reduce_jobs(specs, seed)
    got, ok = launch()
    assert ok, "a guard band changed"
    for spec, g, e in zip(specs, got, expect):
        assert torch.equal(g, e), (spec, float((g - e).abs().max()))
    again, ok2 = launch()
    assert ok2 and all(torch.equal(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize("copies", [1, 4, 16, 17, 128, 129, 256])
def test_reduction_is_bitwise_the_stated_order(copies):
    specs = []
    for nel in (240, 480, 1440, 4096 + 16):
        for acc in (False, True):
            specs.append((nel, [copies], acc, int(acc)))                                        # one segment
            specs.append((nel, [copies, max(1, copies // 2), 1], acc, 1 - int(acc)))            # three segments
    _check_reduce(specs, 100 + copies)


def test_reduction_mixed_forms_in_one_table():
    _check_reduce([(1440, [4], False, 0), (4096 + 16, [129], True, 0), (480, [300], False, 0), (240, [4, 129], True, 1)], 7)


def test_reduction_more_jobs_than_one_table():
    _check_reduce([(240 + 4 * (i % 3), [1 + i % 5], bool(i & 1), i % 2) for i in range(41)], 9)
