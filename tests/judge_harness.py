"""Guard-banded operands and the per-call judgement shared by tests/test_step_glue_gpu.py, tests/test_resample_gpu.py, tests/test_perceptual_glue_gpu.py
and tests/test_style_kernels_gpu.py (each passes its own bounds and its own record of worst values).

Every operand is a view (Op) inside a flat device buffer between BAND guard elements: NaN for floats, a sentinel for integers and bytes.
Strided operands live in a larger NaN-filled tensor.  Outputs start NaN-filled, or seeded where the call accumulates.  judge() asserts, per
call: the kernel instance, |got - ref| <= bound * unit at every element (or bitwise equality), everything the call does not own bitwise
unchanged, and a second identical call bitwise identical."""
import math

import torch

from oracle import launch_ref as R

BAND = 4096
FILL = {torch.float32: float("nan"), torch.int32: -12345, torch.int64: -12345, torch.uint8: 0xA5}
LOSS_SCALE = float(2 ** 40)          # the fixed-point scale of an int64 loss slot


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class Op:
    """a tensor of `shape` inside a flat buffer, between guard bands.  Row r (index of the first dimension; one row for a 1-D shape)
    starts at r * ns + lead elements: ns > the row's size leaves a gap between the rows, lead > 0 makes the tensor a channel slice of a
    wider one.  offset: elements the whole content is shifted by (misalignment).  Gaps and bands hold the fill value (NaN / sentinel); init
    None: so does the tensor.  The host copy keeps the initial state."""

    def __init__(self, shape, init=None, dtype=torch.float32, ns=None, lead=0, offset=0):
        self.shape, self.dtype = tuple(shape), dtype
        self.rows = self.shape[0] if len(self.shape) > 1 else 1
        self.inner = int(math.prod(self.shape)) // max(self.rows, 1) if self.rows else 0
        self.ns, self.lead, self.offset = (ns if ns is not None else self.inner), lead, offset
        assert self.lead + self.inner <= self.ns
        self.total = self.rows * self.ns
        self.host = torch.full((BAND + offset + self.total + BAND,), FILL[dtype], dtype=dtype)
        if init is not None:
            self.region(self.host).copy_(init.to(dtype).reshape(self.rows, self.inner))
        self.dev = self.host.cuda()
        self.t = self.region(self.dev).view(self.shape)

    def region(self, flat):
        return flat[BAND + self.offset:BAND + self.offset + self.total].view(self.rows, self.ns)[:, self.lead:self.lead + self.inner]

    def reset(self):
        self.dev.copy_(self.host)

    def content(self, flat):
        return self.region(flat).reshape(self.shape)

    def owned(self, idxs):
        """flat bool mask of the elements the indices (into the tensor; None: all of it) cover"""
        m = torch.zeros(self.shape, dtype=torch.bool)
        for idx in idxs:
            if idx is None:
                m[...] = True
            else:
                m[idx] = True
        flat = torch.zeros(self.host.numel(), dtype=torch.bool)
        self.region(flat).copy_(m.reshape(self.rows, self.inner))
        return flat


def execute(lib, call, opnds):
    """(kernel instance, host snapshots of every buffer) of two runs from identical initial state"""
    res = []
    for _ in range(2):
        for o in opnds:
            o.reset()
        call()
        torch.cuda.synchronize()
        res.append((lib.vts_last_kernel().decode(), [o.dev.cpu() for o in opnds]))
    return res


def judge(lib, tag, expected, call, opnds, outs, bound, worst, per_family=False):
    """outs: (op, index or None, ref, unit, family): unit None: `ref` bitwise (in the output's dtype); ref None: scratch (owned, not
    judged); ref callable: called with stored(op) -> what this run left in an operand, it returns (ref, unit); an int64 op with a unit: a
    loss slot, judged as (slot - start) / 2^40.  bound: the constant C of |got - ref| <= C unit, or
    {family: C}.  worst: kernel instance (per_family: (kernel instance, family)) -> [worst ratio, case, family, outputs judged], updated."""
    (kern, snap), (kern2, snap2) = execute(lib, call, opnds)
    assert kern == expected and kern2 == expected, "%s: ran %s, the table expects %s" % (tag, kern, expected)
    for o in set(e[0] for e in outs):
        assert any(o is p for p in opnds), "%s: an output is missing from the operand list" % tag
    for o, s, s2 in zip(opnds, snap, snap2):
        assert torch.equal(bits(s), bits(s2)), "%s: a second identical call is not bitwise identical" % tag
        keep = ~o.owned([e[1] for e in outs if e[0] is o])
        assert torch.equal(bits(s)[keep], bits(o.host)[keep]), ("%s: an element outside the outputs changed (guard band, input, or a "
                                                                "channel / gap a strided output does not own)" % tag)
    w = None if per_family else worst.setdefault(kern, [0.0, tag, "exact", 0])
    for o, idx, ref, unit, fam in outs:
        if ref is None:
            continue
        if callable(ref):            # a later stage of a staged call: (ref, unit) at what this run stored for the earlier outputs
            ref, unit = ref(lambda p: p.content(snap[[q is p for q in opnds].index(True)]))
        if per_family:
            w = worst.setdefault((kern, fam), [0.0, tag, fam, 0])
        got = o.content(snap[[p is o for p in opnds].index(True)])
        got = got if idx is None else got[idx]
        w[3] += 1
        if unit is None:
            ref = ref.to(o.dtype).reshape(got.shape)
            same = bits(got.contiguous()) == bits(ref.contiguous())
            assert bool(same.all()), "%s: %s differs bitwise at %d elements, first flat index %d" % (
                tag, kern, int((~same).sum()), int(torch.nonzero(~same.reshape(-1))[0]))
            continue
        if o.dtype == torch.int64:
            start = o.content(o.host) if idx is None else o.content(o.host)[idx]
            got = (got - start).double() / LOSS_SCALE
        ratio, at = R.worst(got, ref, unit)
        if ratio >= w[0]:
            w[0], w[1], w[2] = ratio, tag, fam
        print("%-58s %-10s %.4f  %s" % (kern, fam, ratio, tag))
        c = bound[fam] if isinstance(bound, dict) else bound
        assert ratio <= c, ("%s: %s err / unit = %.3g > %g at element %d (got %r, ref %r)"
                            % (tag, kern, ratio, c, at, float(got.reshape(-1)[at]), float(ref.reshape(-1)[at])))
