"""Every kernel instance of the GEMM-class "wide" family (csrc/vts_conv3x3_wide.hip and the Winograd weight gradient it dispatches to)
against the float64 judges of oracle/launch_ref.py, elementwise, on the hand-built table tests/wide_family_cases.py: the smallest
shapes that reach each instance with every tile dimension ragged.  Nothing is recorded and no shape is a workload's.

Each case goes through the vts.ops wrappers (they take contiguous views) and
  - every operand, the packed weight included, and the output are views inside flat buffers with BAND NaN floats before and after:
    a NaN in a result is a read outside an operand, a changed band a store outside the output;
  - the output is NaN-filled, or seeded where the call accumulates; the shared scratch (ops.workspace) is NaN-filled before every
    call, so a slice element that a k-split kernel never writes is read back as NaN and not as an earlier call's finite leftover;
  - asserted: the kernel instance the table expects (lib.vts_last_kernel(); the last phase's for the four-launch transposed forms),
    |got - ref| <= C u sqrt(K) absref at every element, guard bands and inputs bitwise unchanged, a second identical call bitwise
    identical;
  - run with bias None and with a bias (convolutions), plain and accumulate=True (weight gradients).
The module prints, per kernel instance, the worst err / (u sqrt(K) absref) with its case (pytest -s);
profiles/r11_wide_family_parity.txt is that table from the MI355X."""
import math

import pytest
import torch

import wide_family_cases as T
from oracle import detrand
from oracle import launch_ref as R

pytestmark = pytest.mark.gpu

# One constant per family: |got - ref| <= C * u * sqrt(K) * absref at every element.  C is twice the worst value measured on the MI355X
# (profiles/r11_wide_family_parity.txt), rounded up to two digits: the inputs are fixed, so the maximum moves only with a compiler's
# reassociation, while one dropped product is > 100 units away at this table's K.  For the three direct families a worst value above 4
# would be a finding to explain, not a reason for a larger bound (tests/test_step_launches_gpu.py: measured 0.6-1.3); the Winograd weight
# gradient stands on its own measurement.
# worst measured (MI355X, this module's seeds): conv 0.4566 (conv3x3_wide_kernel<1>, 240 tiles of 12 -> 20 channels at 120 x 510),
# convT 0.7466 (conv_wide_phase_kernel<3>), wgrad 1.1267 (wgrad3x3_flat_kernel<2>, the direct store with accumulate: 6 products per element),
# wgrad_wino 0.2977 (wgrad3x3_wino_kernel, one slice)
C_BOUND = {"conv": 0.92, "convT": 1.5, "wgrad": 2.3, "wgrad_wino": 0.60}
BAND = 4096          # NaN guard floats before and after every operand
WS_FLOATS = 1 << 23  # the scratch is grown to this once, so that no call of the module replaces the NaN-filled tensor by a fresh one
WORST = {}           # kernel instance -> [worst ratio, case, family, calls judged]
TAPS = {"c3s1": 3, "c3s2": 3, "t3": 3, "c4s1": 4, "c4s2": 4, "c4t": 4}


def _bits(t):
    return t.view(torch.int32)


class Buf:
    """a tensor of `shape` as a view inside a flat device buffer, between NaN bands; init None: NaN-filled.  The host copy keeps the
    initial content."""

    def __init__(self, shape, init=None):
        self.shape, self.n = tuple(shape), int(math.prod(shape))
        self.host = torch.full((BAND + self.n + BAND,), float("nan"), dtype=torch.float32)
        if init is not None:
            self.host[BAND:BAND + self.n] = init.reshape(-1).float()
        self.dev = self.host.cuda()
        self.view = self.dev[BAND:BAND + self.n].view(self.shape)

    def reset(self):
        self.dev.copy_(self.host)

    def content(self, flat):
        return flat[BAND:BAND + self.n].view(self.shape)

    def bands_same(self, snap):
        return (torch.equal(_bits(snap[:BAND]), _bits(self.host[:BAND])) and
                torch.equal(_bits(snap[BAND + self.n:]), _bits(self.host[BAND + self.n:])))

    def content_same(self, snap):
        return torch.equal(_bits(self.content(snap)), _bits(self.content(self.host)))


@pytest.fixture(scope="module")
def gpu():
    from vts import lib as L
    from vts import ops
    lib = L.load()
    dev = torch.device("cuda:0")
    ops.workspace(WS_FLOATS, dev)
    yield lib, ops, dev
    if WORST:
        lines = ["# per kernel instance: worst err / (u sqrt(K) absref) over its cases vs float64 (oracle/launch_ref.py), bounds %s"
                 % ", ".join("%s %.3g" % kv for kv in C_BOUND.items()),
                 "# calls = judged calls of tests/wide_family_cases.py that ran the instance (bias / no bias, plain / accumulate, epilogues)",
                 "%-9s %-10s %5s  %-34s %s" % ("worst", "family", "calls", "instance", "at case")]
        for inst, (w, case, fam, calls) in sorted(WORST.items(), key=lambda kv: -kv[1][0]):
            lines.append("%-9.4f %-10s %5d  %-34s %s" % (w, fam, calls, inst, case))
        print("\n[%s]\n%s" % (__name__, "\n".join(lines)))


def run_twice(gpu, call, bufs):
    """(return value, kernel instance, host snapshots of every buffer) of two runs from identical initial state"""
    lib, ops, dev = gpu
    res = []
    for _ in range(2):
        for b in bufs:
            b.reset()
        ws = ops.workspace(1, dev)
        ws.fill_(float("nan"))
        rv = call()
        torch.cuda.synchronize()
        assert ops.workspace(1, dev) is ws, "the scratch was replaced during the call: raise WS_FLOATS"
        res.append((rv, lib.vts_last_kernel().decode(), [b.dev.cpu() for b in bufs]))
    return res


def judge(gpu, tag, expected, fam, call, bufs, inputs, out, ref, unit):
    (rv, kern, snap), (rv2, kern2, snap2) = run_twice(gpu, call, bufs)
    assert kern == expected and kern2 == expected, "%s: ran %s, the table expects %s" % (tag, kern, expected)
    for b, s, s2 in zip(bufs, snap, snap2):
        assert torch.equal(_bits(s), _bits(s2)), "%s: a second identical call is not bitwise identical" % tag
        assert b.bands_same(s), "%s: a guard band changed" % tag
        if b in inputs:
            assert b.content_same(s), "%s: an input changed" % tag
    got = out.content(snap[bufs.index(out)])
    ratio, at = R.worst(got, ref, unit)
    w = WORST.setdefault(kern, [0.0, tag, fam, 0])
    w[3] += 1
    if ratio > w[0]:
        w[0], w[1], w[2] = ratio, tag, fam
    print("%-34s %-10s %.4f  %s" % (kern, fam, ratio, tag))
    assert ratio <= C_BOUND[fam], ("%s: %s err / (u sqrt(K) absref) = %.3g > %g at element %d (got %r, ref %r)"
                                    % (tag, kern, ratio, C_BOUND[fam], at, float(got.reshape(-1)[at]), float(ref.reshape(-1)[at])))
    return rv


def operator_weight(param, mode):
    """the operator's weight as the judges take it, from the parameter tensor and the packing mode (include/vts.h): [B, A, K, K] for the
    convolutions, [A, B, K, K] for the transposed forms"""
    if mode in ("conv_fwd", "convT_adj"):
        return param
    if mode == "conv_adj":
        return param.transpose(0, 1).flip(2, 3)
    assert mode in ("convT_fwd", "conv_s2_adj")
    return param


def param_shape(entry, mode, a, b):
    k = TAPS[entry]
    return (b, a, k, k) if mode in ("conv_fwd", "convT_adj") else (a, b, k, k)


@pytest.mark.parametrize("case", T.CONV, ids=[r[0] for r in T.CONV])
def test_wide_convolution_instances(gpu, case):
    lib, ops, dev = gpu
    cid, entry, mode, (n, a, b, h, w), expected, fam = case
    k = TAPS[entry]
    seed = 1100 + T.CONV.index(case)
    param = detrand.uniform(param_shape(entry, mode, a, b), seed, "w") * math.sqrt(3.0 / (a * k * k))
    wop = operator_weight(param, mode)
    bias = detrand.uniform((b,), seed, "b")
    if entry in ("c3s1", "c4s1", "c4s2"):
        s = 2 if entry == "c4s2" else 1
        p = detrand.uniform((n, a, s * (h - 1) + k, s * (w - 1) + k), seed, "p")
        oshape = (n, b, h, w)
    elif entry == "c3s2":
        s = 2
        p = detrand.uniform((n, a, 2 * h + 2, 2 * w + 2), seed, "p")
        oshape = (n, b, h, w)
    elif entry == "t3":
        p = torch.nn.functional.pad(detrand.uniform((n, a, h, w), seed, "p"), (0, 1, 0, 1))
        oshape = (n, b, 2 * h, 2 * w)
    else:
        p = torch.nn.functional.pad(detrand.uniform((n, a, h // 2 + 1, w // 2 + 1), seed, "p"), (0, 1, 0, 1))
        oshape = (n, b, h, w)
    pb, wb, bb, ob = Buf(p.shape, p), Buf(param.shape, param), Buf((b,), bias), Buf(oshape)
    pack = ops.w4x4_pack if k == 4 else ops.w3x3_pack
    packed = pack(wb.view, mode)
    tb = Buf(packed.shape, packed.cpu())
    torch.cuda.synchronize()
    for with_bias in (False, True):
        bt = bb.view if with_bias else None
        bj = bias if with_bias else None
        if entry == "c3s1":
            call = lambda: ops.conv3x3_wide(pb.view, tb.view, bt, ob.view)
            ref, unit = R.conv_wide(p, wop, bj, K=3, stride=1)["out"]
        elif entry == "c3s2":
            call = lambda: ops.conv3x3s2_wide(pb.view, tb.view, bt, ob.view)
            ref, unit = R.conv_wide(p, wop, bj, K=3, stride=2)["out"]
        elif entry == "t3":
            call = lambda: ops.tconv3x3s2_wide(pb.view, tb.view, bt, ob.view)
            ref, unit = R.tconv3x3s2_wide(p, wop, bj)["out"]
        elif entry == "c4t":
            call = lambda: ops.conv4x4_wide(pb.view, tb.view, bt, ob.view, stride=2, transposed=True)
            ref, unit = R.conv4x4_wide_transposed(p, wop, bj, (h, w))["out"]
        else:
            call = lambda: ops.conv4x4_wide(pb.view, tb.view, bt, ob.view, stride=s)
            ref, unit = R.conv_wide(p, wop, bj, K=4, stride=s, out_hw=(h, w))["out"]
        assert tuple(ref.shape) == oshape
        tag = "%s %s N%d %dx%dx%d -> %dx%dx%d%s" % (cid, mode, n, a, p.shape[2], p.shape[3], b, oshape[2], oshape[3], " bias" if with_bias else "")
        judge(gpu, tag, expected, fam, call, [pb, tb, bb, ob], [pb, tb, bb], ob, ref, unit)


@pytest.mark.parametrize("case", T.WGRAD, ids=[r[0] for r in T.WGRAD])
def test_wide_weight_gradient_instances(gpu, case):
    lib, ops, dev = gpu
    cid, k, s, (n, ci, co, h, w), expected, fam = case
    seed = 1200 + T.WGRAD.index(case)
    p = detrand.uniform((n, ci, s * h + 2, s * w + 2) if k == 3 else (n, ci, s * (h - 1) + 4, s * (w - 1) + 4), seed, "p")
    dout = detrand.uniform((n, co, h, w), seed, "cot")
    dw0 = detrand.uniform((co, ci, k, k), seed, "dw0") * math.sqrt(n * h * w / 3.0)      # the size of the sum itself
    pb, db = Buf(p.shape, p), Buf(dout.shape, dout)
    for acc in (False, True):
        wb = Buf(dw0.shape, dw0 if acc else None)
        if k == 3:
            call = lambda: ops.wgrad3x3_wide(db.view, pb.view, wb.view, accumulate=acc, stride=s)
        else:
            call = lambda: ops.wgrad4x4_wide(db.view, pb.view, wb.view, stride=s, accumulate=acc)
        ref, unit = R.wgrad_wide(dout, p, K=k, stride=s, dw0=dw0 if acc else None)["dw"]
        tag = "%s N%d dout %dx%dx%d in %dx%dx%d s%d%s" % (cid, n, co, h, w, ci, p.shape[2], p.shape[3], s, " acc" if acc else "")
        judge(gpu, tag, expected, fam, call, [pb, db, wb], [pb, db], wb, ref, unit)


def _padded_operands(shape, seed):
    n, ci, co, h, w = shape
    p = detrand.uniform((n, ci, h + 2, w + 2), seed, "p")
    wt = detrand.uniform((co, ci, 3, 3), seed, "w") * math.sqrt(3.0 / (9 * ci))
    bias = detrand.uniform((co,), seed, "b")
    # mask: the padded ReLU'd activation of the layer in front (about half of it zero, zero border); add: that layer's tap gradient
    mask = torch.nn.functional.pad(detrand.uniform((n, co, h, w), seed, "mask").clamp_min(0), (1, 1, 1, 1))
    add = torch.nn.functional.pad(detrand.uniform((n, co, h, w), seed, "add"), (1, 1, 1, 1))
    return p, wt, bias, mask, add


@pytest.mark.parametrize("case", T.PADDED, ids=[r[0] for r in T.PADDED])
def test_wide_padded_epilogues(gpu, case):
    """relu_pad / mask_pad: the interior against the judge, the one-pixel border exactly 0 (the judge's unit is 0 there and the output
    starts as NaN), the bands unchanged"""
    lib, ops, dev = gpu
    cid, shape, expected = case
    n, ci, co, h, w = shape
    p, wt, bias, mask, add = _padded_operands(shape, 1300 + T.PADDED.index(case))
    pb, wb, bb, mb, ab, ob = Buf(p.shape, p), Buf(wt.shape, wt), Buf((co,), bias), Buf(mask.shape, mask), Buf(add.shape, add), Buf((n, co, h + 2, w + 2))
    packed = ops.w3x3_pack(wb.view, "conv_fwd")
    tb = Buf(packed.shape, packed.cpu())
    bufs, inputs = [pb, tb, bb, mb, ab, ob], [pb, tb, bb, mb, ab]
    for with_bias in (False, True):
        ref, unit = R.conv_wide(p, wt, bias if with_bias else None, K=3, stride=1, epilogue="relu_pad")["out"]
        assert (unit[:, :, 0] == 0).all() and (unit[:, :, :, -1] == 0).all() and (ref[:, :, 1:-1, 1:-1] == 0).any()
        call = lambda: ops.conv3x3_wide_relu_pad(pb.view, tb.view, bb.view if with_bias else None, ob.view)
        tag = "%s relu_pad N%d %dx%dx%d -> %dx%dx%d%s" % (cid, n, ci, h, w, co, h, w, " bias" if with_bias else "")
        assert judge(gpu, tag, expected, "conv", call, bufs, inputs, ob, ref, unit) is True
    for with_add in (False, True):
        ref, unit = R.conv_wide(p, wt, None, K=3, stride=1, epilogue="mask_pad", mask=mask, add=add if with_add else None)["out"]
        call = lambda: ops.conv3x3_wide_mask_pad(pb.view, tb.view, ob.view, mb.view, add=ab.view if with_add else None)
        tag = "%s mask_pad N%d %dx%dx%d -> %dx%dx%d%s" % (cid, n, ci, h, w, co, h, w, " add" if with_add else "")
        assert judge(gpu, tag, expected, "conv", call, bufs, inputs, ob, ref, unit) is True


@pytest.mark.parametrize("case", T.PADDED_REFUSED, ids=[r[0] for r in T.PADDED_REFUSED])
def test_wide_padded_epilogues_refuse_what_they_do_not_take(gpu, case):
    """a flat map, a k-split plan and a Cout that is no multiple of 4: "unsupported", and not one float of the output touched"""
    lib, ops, dev = gpu
    cid, shape = case
    n, ci, co, h, w = shape
    p, wt, bias, mask, add = _padded_operands(shape, 1400)
    pb, wb, bb, mb, ab, ob = Buf(p.shape, p), Buf(wt.shape, wt), Buf((co,), bias), Buf(mask.shape, mask), Buf(add.shape, add), Buf((n, co, h + 2, w + 2))
    packed = ops.w3x3_pack(wb.view, "conv_fwd")
    tb = Buf(packed.shape, packed.cpu())
    bufs = [pb, tb, bb, mb, ab, ob]
    for call in (lambda: ops.conv3x3_wide_relu_pad(pb.view, tb.view, bb.view, ob.view),
                 lambda: ops.conv3x3_wide_mask_pad(pb.view, tb.view, ob.view, mb.view, add=ab.view)):
        (rv, _, snap), _ = run_twice(gpu, call, bufs)
        assert rv is False
        for b, s in zip(bufs, snap):
            assert torch.equal(_bits(s), _bits(b.host)), "%s: a refused call wrote" % cid


PACK_MODES = {3: {"conv_fwd": (1, 0, 0), "conv_adj": (0, 1, 1), "conv_s2_adj": (0, 1, 0), "convT_fwd": (0, 1, 0), "convT_adj": (1, 0, 0)},
              4: {"conv_fwd": (1, 0, 0), "conv_adj": (0, 1, 1), "conv_s2_adj": (0, 1, 0)}}     # mode -> (dim of A, dim of B, flip)


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("dims", [(36, 33), (33, 7), (7, 36)])       # both channel counts go through % 4 = 0, 1 and 3; more than one 32-column and 64-row tile
def test_weight_packings_are_the_header_formula(gpu, k, dims):
    """vts_w3x3_pack (5 modes) / vts_w4x4_pack (3 modes): bitwise the permutation of include/vts.h, pitch columns b >= B exactly 0"""
    lib, ops, dev = gpu
    d0, d1 = dims
    t = k * k
    w = detrand.uniform((d0, d1, k, k), 1500 + k, "w")
    wb = Buf(w.shape, w)
    pack = ops.w4x4_pack if k == 4 else ops.w3x3_pack
    for mode, (da, db, flip) in PACK_MODES[k].items():
        A, B = dims[da], dims[db]
        stride = {0: t * d1, 1: t}
        want = R.wtap_pack(w, A, B, stride[da], stride[db], t, flip)
        Bp = (B + 3) // 4 * 4
        assert want.numel() == A * t * Bp and (B == Bp or (want.view(A * t, Bp)[:, B:] == 0).all())
        buf = pack(wb.view, mode, tag="pack-test")
        buf.fill_(float("nan"))
        got = pack(wb.view, mode, tag="pack-test")
        assert got is buf and tuple(got.shape) == (A * t * Bp,)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got.cpu()), _bits(want)), (k, mode, dims)
        snap = wb.dev.cpu()
        assert wb.bands_same(snap) and wb.content_same(snap)
