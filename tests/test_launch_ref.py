"""oracle/launch_ref.py -- the float64 judge of tests/test_step_launches_gpu.py -- against torch autograd in float64 on small random
descriptors that exercise every field it reads, and the reason its error rule is elementwise."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import launch_ref as R

D64 = torch.float64


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=D64)


def act(v, a):
    return {0: v, 1: F.leaky_relu(v, 0.2), 2: F.relu(v)}[a]


def opnd(g, n, c, h, w, affine=True):
    return R.Opnd(rnd(g, n, c, h, w), rnd(g, n, c) if affine else None, rnd(g, n, c) * 0.3 if affine else None)


def opval(op, a):
    v = op.data
    if op.scale is not None:
        v = v * op.scale[:, :, None, None] + op.shift[:, :, None, None]
    return act(v, a)


def wmat(w, cout, cin, ws_co, ws_ci):
    """W[co, ci] built element by element from the header's formula (independent of the judge's as_strided)"""
    idx = torch.tensor([[[co * ws_co + ci * ws_ci + k for k in range(16)] for ci in range(cin)] for co in range(cout)])
    return w[idx].view(cout, cin, 4, 4)


def crop(t, top, left, h, w):
    """t shifted by (top, left) and cut / zero-extended to h x w, with F.pad (negative = crop)"""
    return F.pad(t, (-left, w + left - t.shape[3], -top, h + top - t.shape[2]))


CONV_CASES = [
    # N, C0, C1, Cout, IH, IW, stride, pad, pad_dx, transposed, act_in, act_out, dmask_act, accumulate, bias, weight layout
    (2, 3, 2, 5, 9, 11, 2, 1, 0, 0, 1, 0, 1, 1, True, "conv"),
    (1, 4, 0, 3, 7, 6, 1, 2, 1, 0, 2, 3, 0, 0, True, "convT_w"),
    (2, 2, 3, 4, 8, 9, 2, -1, 2, 0, 0, 0, 2, 0, False, "conv"),
    (2, 3, 2, 4, 5, 6, 2, 1, 0, 1, 1, 0, 1, 1, True, "convT_w"),
    (1, 2, 2, 3, 6, 5, 1, 2, 1, 1, 2, 3, 0, 0, True, "conv"),
    (2, 4, 0, 2, 4, 7, 2, 2, -1, 1, 0, 0, 2, 1, False, "conv"),
    (1, 3, 0, 2, 6, 6, 2, -1, 0, 1, 1, 0, 0, 0, True, "convT_w"),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_judge_matches_autograd(case):
    n, c0, c1, co, ih, iw, s, p, pdx, tr, a_in, a_out, a_m, acc, has_bias, layout = case
    g = torch.Generator().manual_seed(hash(case) % 1000)
    pl = p + pdx
    if tr:
        oh, ow = (ih - 1) * s - 2 * p + 4, (iw - 1) * s - 2 * pl + 4
    else:
        oh, ow = (ih + 2 * p - 4) // s + 1, (iw + 2 * pl - 4) // s + 1
    cin = c0 + c1
    in0 = opnd(g, n, c0, ih, iw)
    in1 = opnd(g, n, c1, ih, iw) if c1 else None
    # the weight as a channel sub-range of a larger tensor (offset 7 floats, a wider row): both layouts of the header
    if layout == "conv":
        ws_co, ws_ci = (cin + 1) * 16, 16
    else:
        ws_co, ws_ci = 16, (co + 2) * 16
    w = rnd(g, 7 + (co - 1) * ws_co + (cin - 1) * ws_ci + 16 + 5)
    wv = w[7:]
    bias = rnd(g, co) if has_bias else None
    dmask = opnd(g, n, co, oh, ow) if a_m else None
    out0 = rnd(g, n, co, oh, ow)
    d = dict(in0={"C": c0}, in1={"C": c1}, N=n, IH=ih, IW=iw, OH=oh, OW=ow, Cout=co, stride=s, pad=p, pad_dx=pdx, transposed=tr,
             ws_co=ws_co, ws_ci=ws_ci, act_in=a_in, act_out=a_out, dmask_act=a_m, accumulate=acc)
    ref, unit = R.conv4x4(d, in0, wv, in1=in1, bias=bias, dmask=dmask, out0=out0)["out"]

    x = opval(in0, a_in)
    if in1 is not None:
        x = torch.cat([x, opval(in1, a_in)], 1)
    W = wmat(wv, co, cin, ws_co, ws_ci)
    if tr:
        full = F.conv_transpose2d(x, W.transpose(0, 1), stride=s)          # rows y' = i*s + k; out[y] = full[y + pad]
        y = crop(full, p, pl, oh, ow)
    else:
        y = F.conv2d(crop(x, -p, -pl, (oh - 1) * s + 4, (ow - 1) * s + 4), W, stride=s)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    if a_out == 3:
        y = torch.tanh(y)
    if dmask is not None:
        v = opval(dmask, 0).detach().requires_grad_(True)
        y = y * torch.autograd.grad(act(v, a_m).sum(), v)[0]
    if acc:
        y = y + out0
    assert ref.shape == y.shape
    assert torch.allclose(ref, y, rtol=1e-12, atol=1e-12)
    assert (unit >= 0).all() and (unit[ref != 0] > 0).all()


WGRAD_CASES = [
    # N, CL0, CL1, CH0, CH1, LH, LW, stride, pad, pad_dx, act_lo, act_hi, accumulate
    (2, 3, 2, 2, 3, 4, 5, 2, 1, 0, 0, 1, 1),
    (1, 2, 0, 3, 0, 6, 5, 1, 2, 1, 1, 2, 0),
    (2, 2, 2, 2, 0, 5, 4, 2, -1, 2, 2, 0, 1),
]


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_wgrad_judge_matches_autograd(case):
    n, cl0, cl1, ch0, ch1, lh, lw, s, p, pdx, a_lo, a_hi, acc = case
    g = torch.Generator().manual_seed(sum(case))
    pl = p + pdx
    hh, hw = (lh - 1) * s + 4 - 2 * p + 1, (lw - 1) * s + 4 - 2 * pl
    lo0, hi0 = opnd(g, n, cl0, lh, lw), opnd(g, n, ch0, hh, hw)
    lo1 = opnd(g, n, cl1, lh, lw) if cl1 else None
    hi1 = opnd(g, n, ch1, hh, hw) if ch1 else None
    dw0 = rnd(g, cl0 + cl1, ch0 + ch1, 4, 4)
    d = dict(N=n, LH=lh, LW=lw, HH=hh, HW=hw, stride=s, pad=p, pad_dx=pdx, act_lo=a_lo, act_hi=a_hi, accumulate=acc)
    ref, unit = R.wgrad4x4(d, lo0, hi0, lo1=lo1, hi1=hi1, dw0=dw0)["dw"]

    lo = opval(lo0, a_lo) if lo1 is None else torch.cat([opval(lo0, a_lo), opval(lo1, a_lo)], 1)
    hi = opval(hi0, a_hi) if hi1 is None else torch.cat([opval(hi0, a_hi), opval(hi1, a_hi)], 1)
    W = torch.zeros(lo.shape[1], hi.shape[1], 4, 4, dtype=D64, requires_grad=True)
    y = F.conv2d(crop(hi, -p, -pl, (lh - 1) * s + 4, (lw - 1) * s + 4), W, stride=s)
    assert y.shape == lo.shape
    dw = torch.autograd.grad((y * lo).sum(), W)[0] + (dw0 if acc else 0)
    assert torch.allclose(ref, dw, rtol=1e-12, atol=1e-12)
    assert (unit > 0).all()


def test_norm_stats_judge_instance_norm():
    g = torch.Generator().manual_seed(3)
    x = rnd(g, 3, 4, 5, 6) * 2 + 1.5
    out = R.norm_stats(x, 0, eps=1e-5, momentum=0.1)
    var, mean = torch.var_mean(x, (2, 3), unbiased=False)
    rstd = 1 / torch.sqrt(var + 1e-5)
    for k, v in (("mean", mean), ("rstd", rstd), ("scale", rstd), ("shift", -mean * rstd)):
        assert torch.allclose(out[k][0], v.reshape(-1), rtol=1e-12, atol=1e-12), k
    y = x * out["scale"][0].view(3, 4, 1, 1) + out["shift"][0].view(3, 4, 1, 1)
    assert torch.allclose(y, F.instance_norm(x, eps=1e-5), atol=1e-12)


def test_norm_stats_judge_batch_norm_groups_running_stats():
    """BatchNorm over three passes batched into one launch (gstart), gamma / beta, running statistics with momentum and the
    unbiased variance, a spliced external pass (ext) and num_batches_tracked: equals the sequential nn.functional.batch_norm calls"""
    g = torch.Generator().manual_seed(4)
    n, c = 7, 3
    x = rnd(g, n, c, 4, 5) * 1.5 + 0.7
    gamma, beta = rnd(g, c), rnd(g, c)
    rm0, rv0 = rnd(g, c), rnd(g, c).abs() + 0.5
    ext_m, ext_v = rnd(g, c), rnd(g, c).abs() + 0.2
    gstart = [0, 2, 5, 7]
    out = R.norm_stats(x, 1, eps=1e-5, momentum=0.1, gamma=gamma, beta=beta, running_mean=rm0, running_var=rv0, nbt=3,
                       gstart=gstart, ext=(ext_m, ext_v, 1), stat_out=True)
    rm, rv = rm0.clone(), rv0.clone()
    for gi, (n0, n1) in enumerate(zip(gstart[:-1], gstart[1:])):
        xs = x[n0:n1]
        y = F.batch_norm(xs, rm, rv, gamma, beta, training=True, momentum=0.1, eps=1e-5)
        sc = out["scale"][0].view(n, c)[n0:n1, :, None, None]
        sh = out["shift"][0].view(n, c)[n0:n1, :, None, None]
        assert torch.allclose(xs * sc + sh, y, atol=1e-12), gi
        if gi == 0:
            var, mean = torch.var_mean(xs, (0, 2, 3), unbiased=True)
            assert torch.allclose(out["stat_mean"][0], mean, atol=1e-12) and torch.allclose(out["stat_uvar"][0], var, atol=1e-12)
        if gi == 1:
            rm.mul_(0.9).add_(0.1 * ext_m)
            rv.mul_(0.9).add_(0.1 * ext_v)
    assert torch.allclose(out["running_mean"][0], rm, atol=1e-12) and torch.allclose(out["running_var"][0], rv, atol=1e-12)
    assert int(out["nbt"][0]) == 3 + 3 + 1
    assert all((u >= 0).all() for _, u in out.values())


@pytest.mark.parametrize("mode", [0, 1])
def test_norm_bwd_judge_matches_autograd(mode):
    g = torch.Generator().manual_seed(5 + mode)
    n, c = 5, 3
    x = (rnd(g, n, c, 4, 6) * 1.3 + 0.4).requires_grad_(True)
    dy = rnd(g, n, c, 4, 6)
    gamma = rnd(g, c).requires_grad_(True)
    beta = rnd(g, c).requires_grad_(True)
    gstart = [0, 2, 5] if mode else None
    if mode == 0:
        y = F.instance_norm(x, eps=1e-5)
        var, mean = torch.var_mean(x.detach(), (2, 3), unbiased=False)
        mean, rstd = mean.reshape(-1), (1 / torch.sqrt(var + 1e-5)).reshape(-1)
    else:
        ys, ms, rs = [], [], []
        for n0, n1 in zip(gstart[:-1], gstart[1:]):
            ys.append(F.batch_norm(x[n0:n1], None, None, gamma, beta, training=True, eps=1e-5))
            var, m = torch.var_mean(x.detach()[n0:n1], (0, 2, 3), unbiased=False)
            ms.append(m.repeat(n1 - n0))
            rs.append((1 / torch.sqrt(var + 1e-5)).repeat(n1 - n0))
        y, mean, rstd = torch.cat(ys), torch.cat(ms), torch.cat(rs)
    dx, dg, db = torch.autograd.grad((y * dy).sum(), (x, gamma, beta), allow_unused=True)
    dg0, db0 = rnd(g, c), rnd(g, c)
    for sums_beta in (None, beta.detach()):
        out = R.norm_bwd(dy, x.detach(), mean, rstd, mode, gamma=gamma.detach(), dgamma0=dg0, dbeta0=db0, accumulate=True,
                         gstart=gstart, sums_beta=sums_beta)
        assert torch.allclose(out["dx"][0].view_as(dx), dx, atol=1e-11)
        assert (out["dx"][1] > 0).all()
        if mode:
            assert torch.allclose(out["dgamma"][0], dg + dg0, atol=1e-11) and torch.allclose(out["dbeta"][0], db + db0, atol=1e-11)


def test_elementwise_rule_catches_one_element_that_rel_l2_misses():
    """a 4 x 20 x 256 x 256 convolution output computed in fp32: it passes the elementwise rule at c = 8; one element moved by
    1e-4 relative fails it, while the relative L2 error of the whole output stays below the 1e-5 bound of the kernel tests"""
    g = torch.Generator().manual_seed(8)
    n, ci, co = 4, 8, 20
    x = torch.randn(n, ci, 512, 512, generator=g)
    w = torch.randn(co * ci * 16, generator=g) * 0.1
    d = dict(in0={"C": ci}, in1={"C": 0}, N=n, IH=512, IW=512, OH=256, OW=256, Cout=co, stride=2, pad=1, pad_dx=0, transposed=0,
             ws_co=ci * 16, ws_ci=16, act_in=0, act_out=0, dmask_act=0, accumulate=0)
    ref, unit = R.conv4x4(d, R.Opnd(x, None, None), w)["out"]
    got = F.conv2d(x, w.view(co, ci, 4, 4), stride=2, padding=1)          # an fp32 evaluation of the same sum
    assert got.shape == (4, 20, 256, 256)
    assert R.worst(got, ref, unit)[0] <= 8
    i = int(torch.argmax(ref.abs() / unit.clamp_min(1e-300)))       # a well-conditioned element: |ref| comparable to absref
    bad = got.clone().view(-1)
    bad[i] = float(ref.view(-1)[i]) * (1 + 1e-4)
    bad = bad.view_as(got)
    rel_l2 = float((bad.double() - ref).norm() / ref.norm())
    assert rel_l2 <= 1e-5
    assert R.worst(bad, ref, unit)[0] > 8
    assert not math.isinf(R.worst(bad, ref, unit)[0])


# ---- the judges of the GEMM-class "wide" ABI (tests/test_wide_family_gpu.py) ---------------------------------------------------

def relerr(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("K,stride,shape", [(3, 1, (2, 5, 4, 6, 7)), (3, 2, (2, 3, 5, 4, 5)), (4, 1, (1, 4, 3, 5, 6)), (4, 2, (2, 3, 2, 5, 4))])
@pytest.mark.parametrize("has_bias", [False, True])
def test_conv_wide_judge_matches_conv2d(K, stride, shape, has_bias):
    n, ci, co, oh, ow = shape
    g = torch.Generator().manual_seed(K * 10 + stride)
    ph, pw = stride * (oh - 1) + K + (stride - 1), stride * (ow - 1) + K + (stride - 1)     # stride 2: one row / column never read
    p, w, b = rnd(g, n, ci, ph, pw), rnd(g, co, ci, K, K), (rnd(g, co) if has_bias else None)
    ref, unit = R.conv_wide(p, w, b, K=K, stride=stride, out_hw=(oh, ow))["out"]
    assert relerr(ref, F.conv2d(p, w, b, stride=stride)[:, :, :oh, :ow]) <= 1e-12
    absref = F.conv2d(p.abs(), w.abs(), None if b is None else b.abs(), stride=stride)[:, :, :oh, :ow]
    assert relerr(unit, R.U * math.sqrt(ci * K * K) * absref) <= 1e-12
    if K == 3:
        assert torch.equal(R.conv_wide(p, w, b, K=K, stride=stride)["out"][0], ref)         # the extent the 3 x 3 entries imply


def test_conv_wide_judge_epilogues():
    g = torch.Generator().manual_seed(5)
    n, ci, co, h, w = 2, 3, 4, 5, 6
    p, wt, b = rnd(g, n, ci, h + 2, w + 2), rnd(g, co, ci, 3, 3), rnd(g, co)
    plain, unit0 = R.conv_wide(p, wt, b, K=3, stride=1)["out"]
    ref, unit = R.conv_wide(p, wt, b, K=3, stride=1, epilogue="relu_pad")["out"]
    assert ref.shape == (n, co, h + 2, w + 2)
    assert torch.equal(ref, F.pad(F.relu(plain), (1, 1, 1, 1))) and torch.equal(unit, F.pad(unit0, (1, 1, 1, 1)))
    assert (plain < 0).any() and (plain > 0).any()
    mask, add = F.relu(rnd(g, n, co, h + 2, w + 2)), rnd(g, n, co, h + 2, w + 2)
    assert (mask[:, :, 1:-1, 1:-1] == 0).any() and (mask[:, :, 0] > 0).any()
    plain, unit0 = R.conv_wide(p, wt, None, K=3, stride=1)["out"]
    for a in (None, add):
        ref, unit = R.conv_wide(p, wt, None, K=3, stride=1, epilogue="mask_pad", mask=mask, add=a)["out"]
        keep = F.pad((mask[:, :, 1:-1, 1:-1] > 0).to(D64), (1, 1, 1, 1))
        want = (F.pad(plain, (1, 1, 1, 1)) + (0 if a is None else a)) * keep
        assert relerr(ref, want) <= 1e-12
        assert torch.equal(unit == 0, keep == 0)                  # masked elements and the border: exact zeros
        assert (ref[keep == 0] == 0).all()
        extra = 0 if a is None else R.U * math.sqrt(ci * 9) * a.abs() * keep
        assert relerr(unit, F.pad(unit0, (1, 1, 1, 1)) * keep + extra) <= 1e-12


@pytest.mark.parametrize("shape", [(2, 3, 4, 3, 5), (1, 5, 2, 4, 1)])
@pytest.mark.parametrize("has_bias", [False, True])
def test_tconv3x3s2_wide_judge_matches_conv_transpose2d(shape, has_bias):
    n, ci, co, ih, iw = shape
    g = torch.Generator().manual_seed(ih * 7 + iw)
    x, w, b = rnd(g, n, ci, ih, iw), rnd(g, ci, co, 3, 3), (rnd(g, co) if has_bias else None)
    ref, unit = R.tconv3x3s2_wide(F.pad(x, (0, 1, 0, 1)), w, b)["out"]
    assert relerr(ref, F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)) <= 1e-12
    absref = F.conv_transpose2d(x.abs(), w.abs(), None if b is None else b.abs(), stride=2, padding=1, output_padding=1)
    terms = torch.tensor([[1.0, 2.0], [2.0, 4.0]], dtype=D64).repeat(ih, iw) * ci        # by output parity (y % 2, x % 2)
    assert relerr(unit, R.U * torch.sqrt(terms) * absref) <= 1e-12


@pytest.mark.parametrize("shape", [(2, 3, 4, 6, 8), (1, 4, 3, 7, 5), (2, 2, 3, 4, 9), (1, 3, 2, 1, 2)])
@pytest.mark.parametrize("has_bias", [False, True])
def test_conv4x4_wide_transposed_judge_matches_autograd(shape, has_bias):
    """the input gradient of Conv2d(4, stride 2, padding 2) by autograd; even and odd extents"""
    n, ci, co, h, w = shape                    # the layer ci -> co on an h x w input
    g = torch.Generator().manual_seed(h * 11 + w)
    x = rnd(g, n, ci, h, w).requires_grad_(True)
    wt, b = rnd(g, co, ci, 4, 4), (rnd(g, ci) if has_bias else None)
    y = F.conv2d(x, wt, None, stride=2, padding=2)
    cot = rnd(g, *y.shape)
    (y * cot).sum().backward()
    ref, unit = R.conv4x4_wide_transposed(F.pad(cot, (0, 1, 0, 1)), wt, b, (h, w))["out"]
    want = x.grad + (0 if b is None else b.view(1, -1, 1, 1))
    assert relerr(ref, want) <= 1e-12
    xa = x.detach().clone().requires_grad_(True)
    (F.conv2d(xa, wt.abs(), None, stride=2, padding=2) * cot.abs()).sum().backward()
    absref = xa.grad + (0 if b is None else b.abs().view(1, -1, 1, 1))
    assert relerr(unit, R.U * math.sqrt(4 * co) * absref) <= 1e-12


@pytest.mark.parametrize("K,stride,shape", [(3, 1, (2, 3, 4, 5, 6)), (3, 2, (2, 4, 3, 3, 5)), (4, 1, (1, 2, 3, 4, 5)), (4, 2, (3, 3, 2, 4, 3))])
@pytest.mark.parametrize("acc", [False, True])
def test_wgrad_wide_judge_matches_autograd(K, stride, shape, acc):
    n, ci, co, h, w = shape
    g = torch.Generator().manual_seed(K + 3 * stride)
    p = rnd(g, n, ci, stride * h + 2, stride * w + 2) if K == 3 else rnd(g, n, ci, stride * (h - 1) + 4, stride * (w - 1) + 4)
    wt = rnd(g, co, ci, K, K).requires_grad_(True)
    cot = rnd(g, n, co, h, w)
    (F.conv2d(p, wt, stride=stride)[:, :, :h, :w] * cot).sum().backward()
    dw0 = rnd(g, co, ci, K, K) if acc else None
    ref, unit = R.wgrad_wide(cot, p, K=K, stride=stride, dw0=dw0)["dw"]
    assert relerr(ref, wt.grad + (dw0 if acc else 0)) <= 1e-12
    wa = wt.detach().clone().requires_grad_(True)
    (F.conv2d(p.abs(), wa, stride=stride)[:, :, :h, :w] * cot.abs()).sum().backward()
    assert relerr(unit, R.U * math.sqrt(n * h * w) * wa.grad + (R.U * dw0.abs() if acc else 0)) <= 1e-12


def test_wtap_pack_formula_is_the_layers_weight():
    """the packing formula with the (A, B, sa, sb, flip) of each mode (include/vts.h) reads back as the operator's weight"""
    g = torch.Generator().manual_seed(9)
    co, ci = 5, 7
    w = rnd(g, co, ci, 3, 3)
    fwd = R.wtap_pack(w, ci, co, 9, 9 * ci, 9, 0).view(ci, 9, 8)
    assert torch.equal(fwd[:, :, :co], w.permute(1, 2, 3, 0).reshape(ci, 9, co)) and (fwd[:, :, co:] == 0).all()
    adj = R.wtap_pack(w, co, ci, 9 * ci, 9, 9, 1).view(co, 9, 8)
    assert torch.equal(adj[:, :, :ci], w.flip(2, 3).permute(0, 2, 3, 1).reshape(co, 9, ci)) and (adj[:, :, ci:] == 0).all()
    w4 = rnd(g, co, ci, 4, 4)
    s2 = R.wtap_pack(w4, co, ci, 16 * ci, 16, 16, 0).view(co, 16, 8)
    assert torch.equal(s2[:, :, :ci], w4.permute(0, 2, 3, 1).reshape(co, 16, ci))


def test_wide_judges_catch_one_dropped_product():
    """one product missing from one element is more than 8 units of u sqrt(K) absref at the largest K of the wide-family table (the signal
    is about 2^24 / K^1.5 units: the table keeps K below 2500, where that is still > 100)"""
    import wide_family_cases as T

    kmax = T.max_k_terms()
    assert kmax <= 2500
    ci = (kmax + 8) // 9
    assert ci * 9 >= kmax
    g = torch.Generator().manual_seed(11)
    p = (torch.rand(1, ci, 5, 6, generator=g, dtype=D64) * 2 - 1).float()
    w = ((torch.rand(4, ci, 3, 3, generator=g, dtype=D64) * 2 - 1) * math.sqrt(3.0 / (9 * ci))).float()
    ref, unit = R.conv_wide(p, w, None, K=3, stride=1)["out"]
    assert R.worst(ref.float(), ref, unit)[0] < 1.0                     # the rounding of the exact result to fp32 passes
    smallest = []
    for y, x in ((0, 0), (2, 3), (1, 2)):
        prods = (p.double()[0, :, y:y + 3, x:x + 3] * w.double()[1]).abs()
        c, ky, kx = [int(v) for v in torch.nonzero(prods == prods.flatten().sort()[0][prods.numel() // 2])[0]]
        got = ref.clone()
        got[0, 1, y, x] -= p.double()[0, c, y + ky, x + kx] * w.double()[1, c, ky, kx]      # the median-size product of that element dropped
        ratio, at = R.worst(got, ref, unit)
        assert at == (1 * 3 + y) * 4 + x
        smallest.append(ratio)
    assert min(smallest) > 8.0, smallest


# ---- the glue judges (loss, optimiser, pyramid, patches, post-processing, augmentation, sampler) against torch / oracle.nets in float64 ----
from oracle import nets  # noqa: E402

TOL = 1e-12


def close(a, b):
    return float((a.reshape(-1) - b.reshape(-1)).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


def flagged(ref, unit):
    """a single element (the one with the largest unit) changed by 16 units is what worst() reports, at that element"""
    ref, unit = ref.reshape(-1), unit.reshape(-1)
    i = int(torch.argmax(unit))
    assert float(unit[i]) > 0
    got = ref.clone()
    got[i] += 16 * unit[i]
    ratio, at = R.worst(got, ref, unit)
    assert at == i and 15.9 < ratio < 16.1, (at, i, ratio)
    assert R.worst(ref.clone(), ref, unit)[0] == 0


@pytest.mark.parametrize("hw", [(1, 1), (1, 4), (2, 2), (5, 7), (17, 130), (66, 65)])
def test_avgpool_judges_match_avg_pool2d_and_its_autograd(hw):
    g = torch.Generator().manual_seed(hw[0] * 131 + hw[1])
    x = rnd(g, 2, 3, *hw).requires_grad_(True)
    y = F.avg_pool2d(x, 3, 2, 1, count_include_pad=False)
    cot, dx0 = rnd(g, *y.shape), rnd(g, 2, 3, *hw)
    (y * cot).sum().backward()
    ref, unit = R.avgpool3s2(x)["y"]
    assert close(ref, y.detach()) and (unit >= 0).all()
    assert close(R.avgpool3s2_bwd(cot, *hw)["dx"][0], x.grad)
    assert close(R.avgpool3s2_bwd(cot, *hw, dx0=dx0)["dx"][0], x.grad + dx0)
    flagged(ref, unit)
    flagged(*R.avgpool3s2_bwd(cot, *hw, dx0=dx0)["dx"])


GAN_NAMES = {0: "nonsaturating", 1: "lsgan", 2: "vanilla", 3: "wgan", 4: "hinge"}


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("real", [True, False])
def test_ganloss_judge_matches_gan_loss_single_in_float64(mode, real):
    g = torch.Generator().manual_seed(mode * 2 + real)
    p = (rnd(g, 3, 1, 9, 11) * 12).requires_grad_(True)          # beyond +-20: the softplus threshold
    label, coeff, gcoeff = (0.75 if real else 0.125), 2.5, -0.75          # exact in fp32
    if mode == 5:
        loss = F.binary_cross_entropy_with_logits(torch.sigmoid(p), torch.full_like(p, label))
    else:
        loss = nets.gan_loss_single(p, real, GAN_NAMES[mode], label, label).mean()
    loss.backward()
    out = R.ganloss(p, mode, real, label, coeff, gcoeff, workgroups=2)
    assert close(out["loss"][0], coeff * loss.detach())
    assert close(out["dpred"][0], gcoeff * p.grad)
    assert float(out["loss"][1]) >= 2 * 2.0 ** -41
    flagged(*out["dpred"])
    flagged(*out["loss"])


def test_l1_judge_matches_l1_loss_and_its_autograd():
    g = torch.Generator().manual_seed(5)
    a, b, g0 = rnd(g, 2, 3, 17, 19).requires_grad_(True), rnd(g, 2, 3, 17, 19), rnd(g, 2 * 3 * 17 * 19)
    b.view(-1)[:40] = a.detach().view(-1)[:40]                    # a stretch of exact ties: sign 0
    coeff = 0.5
    loss = F.l1_loss(a, b, reduction="sum") * coeff
    loss.backward()
    out = R.l1(a, b, coeff)
    assert close(out["loss"][0], loss.detach()) and close(out["grad"][0], a.grad)
    assert (out["grad"][1] == 0).all() and (out["grad"][0][:40] == 0).all()
    acc = R.l1(a, b, coeff, grad0=g0)
    assert close(acc["grad"][0], a.grad.reshape(-1) + g0)
    flagged(*out["loss"])
    flagged(*acc["grad"])


def test_patch_judges_match_gather_patches_and_its_autograd():
    g = torch.Generator().manual_seed(6)
    n, c, h, w, ppi, size = 2, 2, 33, 31, 5, 8
    src = rnd(g, n, c, h, w).requires_grad_(True)
    offx = torch.tensor([0, -5, 28, 40, 0, 3, 3, -20, 30, 12])
    offy = torch.tensor([0, 30, -3, 2, 0, 50, 50, 4, 31, 9])
    img = torch.arange(n).repeat_interleave(ppi)
    ref = torch.cat([nets.gather_patches(src[i:i + 1], offx[i * ppi:(i + 1) * ppi], offy[i * ppi:(i + 1) * ppi], size) for i in range(n)], 0)
    cot, seed = rnd(g, *ref.shape), rnd(g, n, c, h, w)
    (ref * cot).sum().backward()
    assert torch.equal(R.patch_gather(src.detach(), img, offx, offy, size), ref.detach())
    out = R.patch_scatter_bwd(cot, offx, offy, ppi, n, h, w)["dsrc"]
    assert close(out[0], src.grad) and ((out[1] == 0) == (src.grad == 0)).all()
    acc = R.patch_scatter_bwd(cot, offx, offy, ppi, n, h, w, dsrc0=seed)["dsrc"]
    assert close(acc[0], src.grad + seed) and (acc[1][src.grad == 0] == 0).all()
    flagged(*acc)


def test_g_post_and_diffaug_judges_match_the_oracle_nets():
    g = torch.Generator().manual_seed(7)
    n, h, w = 2, 9, 7
    go, S = torch.tanh(rnd(g, n, 5, h, w)), rnd(g, n, 1, h, w)
    M = (rnd(g, n, 1, h, w) > 0).to(D64)
    rb, rs = torch.rand(n, generator=g, dtype=D64), torch.rand(n, generator=g, dtype=D64)
    out = R.g_post(go, M, 0.25, rb, rs, S)
    fI, fT = go[:, :3] * M, go[:, 3:] * M
    assert close(out["fake_I"][0], fI) and close(out["fake_T"][0], fT)
    assert close(out["fake_N"][0], nets.compute_normal(fT, 0.25))
    assert close(out["aug_fake_I"][0], nets.diffaug_bs(fI, rb, rs) * M)
    assert torch.equal(out["stack_S"][0].reshape(-1), S.reshape(-1)) and torch.equal(out["stack_M"][0].reshape(-1), M.reshape(-1))
    zero = R.g_post(go, torch.zeros_like(M), 0.0)["fake_N"]
    assert (zero[0] == 0).all() and (zero[1] == 0).all()          # the 1e-12 clamp: 0 / 1e-12
    x = rnd(g, n, 3, h, w)
    assert close(R.diffaug_bs_mask(x, M, rb, rs)["aug"][0], nets.diffaug_bs(x, rb, rs) * M)
    assert close(R.diffaug_bs_mask(x, None, rb, rs)["aug"][0], nets.diffaug_bs(x, rb, rs))
    for k in ("fake_I", "fake_N", "aug_fake_I"):
        flagged(*out[k])
    flagged(*R.diffaug_bs_mask(x, M, rb, rs)["aug"])


@pytest.mark.parametrize("letter", list("bscton"))
@pytest.mark.parametrize("masked", [False, True])
def test_diffaug_op_judge_matches_the_oracle_diffaug(letter, masked):
    g = torch.Generator().manual_seed(ord(letter))
    n, c, h, w = 2, 3, 9, 7
    x = rnd(g, n, c, h, w) + 3.0
    M = (rnd(g, n, 1, h, w) > 0).to(D64) if masked else None
    d = {"r": torch.rand(n, generator=g, dtype=D64), "tx": torch.tensor([-2, 9]), "ty": torch.tensor([1, -1]),
         "ox": torch.tensor([0, 9]), "oy": torch.tensor([3, 7]), "sigma": torch.tensor([0.05, 0.0], dtype=D64), "noise": rnd(g, n, c, h, w)}
    want = nets.diffaug(x, letter, [d])
    want = want * M if masked else want
    pf = d["sigma"] if letter == "n" else d["r"]
    pi = (d["tx"], d["ty"]) if letter == "t" else (d["ox"], d["oy"])
    ref, unit = R.diffaug_op(x, letter, pf=pf, pi0=pi[0], pi1=pi[1], noise=d["noise"], M=M)["out"]
    assert close(ref, want)
    if letter in "to" and not masked:
        assert (unit == 0).all()
    else:
        flagged(ref, unit)


def test_g_out_grad_judge_matches_autograd_of_the_masked_tanh_outputs():
    g = torch.Generator().manual_seed(8)
    n, h, w = 2, 5, 4
    raw = rnd(g, n, 5, h, w).requires_grad_(True)
    M = (rnd(g, n, 1, h, w) > 0).to(D64)
    dI, dT, dc = rnd(g, n, 3, h, w), rnd(g, n, 2, h, w), rnd(g, n, 3, 3, 2)
    go = torch.tanh(raw)
    fI, fT = go[:, :3] * M, go[:, 3:] * M
    ((fI * dI).sum() + (fT * dT).sum() + (F.avg_pool2d(fI, 3, 2, 1, count_include_pad=False) * dc).sum()).backward()
    out = R.g_out_grad(dI, dT, M, go.detach(), coarse=dc)["d_raw"]
    assert close(out[0], raw.grad)
    plain = R.g_out_grad(None, dT, M, go.detach())["d_raw"]
    assert (plain[0][:, :3] == 0).all() and (plain[1][:, :3] == 0).all()
    flagged(*out)
    flagged(*R.g_out_grad(dI, dT, M, go.detach())["d_raw"])
    flagged(*R.mask_mul(dI, M)["y"])
    assert close(R.mask_mul(dI, M)["y"][0], dI * M)


@pytest.mark.parametrize("dim", [4, 8])
def test_spe_judge_matches_the_oracle_grid_and_carries_the_argument(dim):
    ref, unit = R.spe_grid(2, 3, 1100, dim)["out"]
    assert close(ref, nets.spe_grid(2, 3, 1100, dim, dtype=D64))
    # a few u of relative error in the frequency move sin(pos f) by |pos f| times that: the unit must grow with the position
    assert float(unit[0, 1, 0, 1099]) > 100 * float(unit[0, 1, 0, 0])
    assert float(unit[0, 0, 0, 1099]) <= 2 * R.U           # frequency exactly 1: only the sine's own rounding
    flagged(ref, unit)


@pytest.mark.parametrize("betas", [(0.0, 0.99), (0.5, 0.999)])
def test_adam_judge_matches_adam_update_and_torch_optim_adam(betas):
    g = torch.Generator().manual_seed(9)
    n, lr, eps = 50, 1e-3, 1e-8
    lr32, eps32, b1, b2 = R._f32(lr), R._f32(eps), R._f32(betas[0]), R._f32(betas[1])
    p0 = rnd(g, n)
    grads = [rnd(g, n) * 10.0 ** (-2 * s) for s in range(3)]
    grads[0][:5] = 0
    param = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([param], lr=lr32, betas=(b1, b2), eps=eps32)
    p, m, v = p0.clone(), torch.zeros(n, dtype=D64), torch.zeros(n, dtype=D64)
    pn, mn, vn = p0.clone(), torch.zeros(n, dtype=D64), torch.zeros(n, dtype=D64)
    for step, gr in enumerate(grads, 1):
        param.grad = gr.clone()
        opt.step()
        nets.adam_update(pn, gr, mn, vn, step, lr32, b1, b2, eps32)
        out = R.adam_flat(p, gr * 8, m, v, lr, betas[0], betas[1], eps, step, grad_scale=0.125)
        if step == 1:
            assert (out["p"][1][:5] == 0).all() and torch.equal(out["p"][0][:5], p[:5])      # g = m = v = 0: no update, exactly
            assert (out["p"][1][5:] > 0).all()
        p, m, v = out["p"][0], out["m"][0], out["v"][0]
        assert close(p, param.detach()) and close(p, pn) and close(m, mn) and close(v, vn)
    for k in ("p", "m", "v"):
        flagged(*out[k])


def test_sampler_and_staging_judges():
    g = torch.Generator().manual_seed(10)
    M = torch.zeros(2, 1, 46, 47, dtype=D64)
    M[0, 0, 20:23, 5:9], M[0, 0, 45, 46], M[1, 0, 0, 0] = 1.0, 0.5, 2.0
    cand, prefix = R.mask_candidates(M)
    for i in range(2):
        pos = nets.dilated_mask_positions(M[i:i + 1])
        want = torch.zeros(32, 33, dtype=torch.uint8)
        want[pos[:, 0], pos[:, 1]] = 1
        assert torch.equal(cand[i], want) and int(prefix[i, -1]) == pos.shape[0] and int(prefix[i, 0]) == 0
        ranks = torch.tensor([[0, pos.shape[0] - 1, pos.shape[0] // 2]])
        ox, oy = R.mask_select(cand[i:i + 1], ranks)
        assert torch.equal(oy.long(), pos[ranks[0], 0]) and torch.equal(ox.long(), pos[ranks[0], 1])
    assert (prefix[:, 1:] >= prefix[:, :-1]).all()
    counts = [1000, 70, 3, 0]
    r = R.mask_sample_ranks(counts, 65, 12345)
    assert r.shape == (4, 65) and len(set(r[0].tolist())) == 65 and 0 <= int(r[0].min()) and int(r[0].max()) < 1000
    assert sorted(r[1].tolist()) == sorted(set(r[1].tolist())) and int(r[1].max()) < 70
    assert r[2].tolist() == [q % 3 for q in range(65)] and r[3].tolist() == [0] * 65
    assert not torch.equal(r[0], R.mask_sample_ranks(counts, 65, 12346)[0])
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF                 # the published first output of splitmix64 seeded with 0
    # byte staging: IEEE fp32 division / subtraction, every byte value
    b = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(R.u8_expand(b, False), b.float() / 255.0) and torch.equal(R.u8_expand(b, True), (b.float() / 255.0 - 0.5) / 0.5)
    m, s, i3 = R.input_images_u8(b.view(1, 1, 256), b.view(1, 1, 256).expand(1, 3, 256), b.flip(0).view(1, 1, 256))
    assert torch.equal(s, R.u8_expand(b, True).view(1, 1, 256) * m) and torch.equal(i3[0, 2], s[0, 0])
    # image pool: a later image draws the slot an earlier one has just filled
    imgs, store = rnd(g, 3, 4).float(), rnd(g, 2, 4).float()
    out, st = R.pool_query(imgs, store, torch.tensor([-1, 1, 1]), torch.tensor([1, 1, -1]))
    assert torch.equal(out[0], imgs[0]) and torch.equal(out[1], imgs[0]) and torch.equal(out[2], imgs[1]) and torch.equal(st[1], imgs[1])


# ---- the padding / resampling / FIR judges (tests/test_resample_gpu.py) against independent float64 evaluations ------------------------
import os  # noqa: E402
import sys  # noqa: E402

from oracle import stylegan2 as sg2  # noqa: E402

PAD_MODE = {0: "constant", 1: "reflect", 2: "replicate"}
SLOPE32 = float(torch.tensor(0.2, dtype=torch.float32))


def act32(v, a):
    return {0: v, 1: F.leaky_relu(v, SLOPE32), 2: F.relu(v), 3: torch.tanh(v)}[a]


def refuses(ref, unit, border=True):
    """the two planted errors the judge must refuse: a border element taken from the neighbouring pixel, and one element off by 4 units"""
    ref, unit = ref.clone(), unit.clone()
    if border and ref.shape[-1] > 1:
        got = ref.clone()
        flat = (ref[..., 0, 0] - ref[..., 0, 1]).abs().reshape(-1)
        j = int(torch.argmax(flat))                       # the plane where the two pixels differ most
        got.reshape(-1, *ref.shape[-2:])[j, 0, 0] = ref.reshape(-1, *ref.shape[-2:])[j, 0, 1]
        assert float(flat[j]) > 0 and R.worst(got, ref, unit)[0] > 1.01
    i = int(torch.argmax(unit.reshape(-1)))
    got = ref.clone().reshape(-1)
    if float(unit.reshape(-1)[i]) > 0:
        got[i] += 4 * unit.reshape(-1)[i]
        ratio, at = R.worst(got, ref, unit)
        assert at == i and 3.9 < ratio < 4.1
    else:                                                 # an exact judge: any change at all
        got[i] = got[i] + 2.0 ** -20
        assert R.worst(got, ref, unit)[0] == math.inf
    assert R.worst(ref.clone(), ref, unit)[0] == 0


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("act_", [0, 1, 2, 3])
@pytest.mark.parametrize("pads", [(3, 3, 3, 3), (2, 0, 1, 3), (0, 0, 0, 0), (4, 4, 6, 6)])
def test_pad_judges_match_f_pad_and_its_autograd(mode, act_, pads):
    if mode != 1 and pads == (4, 4, 6, 6):
        pads = (5, 6, 8, 9)                               # beyond the image: legal for zero and replicate
    g = torch.Generator().manual_seed(mode * 16 + act_ * 4 + pads[0])
    n, c, h, w = 2, 3, 5, 7
    pt, pb, pl, pr = pads
    x, sc, sh = rnd(g, n, c, h, w), rnd(g, n, c), rnd(g, n, c) * 0.3
    res = rnd(g, n, c, h + pt + pb, w + pl + pr)
    for aff in (True, False):
        for r in (None, res):
            v = act32(x * sc[:, :, None, None] + sh[:, :, None, None] if aff else x, act_)
            want = F.pad(v, (pl, pr, pt, pb), mode=PAD_MODE[mode]) + (0 if r is None else r)
            ref, unit = R.pad_affine(x, sc if aff else None, sh if aff else None, pads, mode, act_, r)["out"]
            assert close(ref, want)
            if aff or act_ in (1, 3) or r is not None:
                refuses(ref, unit, border=mode == 1 and sum(pads) > 0)
            else:
                assert float(unit.max()) == 0             # a gather: exact
    dpad = rnd(g, n, c, h + pt + pb, w + pl + pr)
    xg = x.clone().requires_grad_(True)
    (F.pad(xg, (pl, pr, pt, pb), mode=PAD_MODE[mode]) * dpad).sum().backward()
    din0 = rnd(g, n, c, h, w)
    assert close(R.pad_bwd(dpad, (h, w), pads, mode)["din"][0], xg.grad)
    ref, unit = R.pad_bwd(dpad, (h, w), pads, mode, din0)["din"]
    assert close(ref, xg.grad + din0)
    refuses(ref, unit)


def test_pad_judge_sizes_one_and_the_tanh_unit():
    g = torch.Generator().manual_seed(3)
    x = rnd(g, 1, 1, 1, 1)
    for mode in (0, 2):
        assert close(R.pad_affine(x, None, None, (2, 1, 1, 2), mode, 0)["out"][0], F.pad(x, (1, 2, 2, 1), mode=PAD_MODE[mode]))
    # tanh: the argument's rounding u |t| (1 - ref^2) plus E u |ref|; without an affine the argument is exact
    x, sc, sh = torch.tensor([[[[2.0]]]], dtype=D64), torch.tensor([[1.5]], dtype=D64), torch.tensor([[-0.5]], dtype=D64)
    ref, unit = R.pad_affine(x, sc, sh, (0, 0, 0, 0), 0, 3)["out"]
    t = math.tanh(2.5)
    assert close(ref, torch.tensor(t, dtype=D64)) and abs(float(unit) - R.U * (3.5 * (1 - t * t) + R.TANH_E * t)) < 1e-20
    assert abs(float(R.pad_affine(x, None, None, (0, 0, 0, 0), 0, 3)["out"][1]) - R.U * R.TANH_E * math.tanh(2.0)) < 1e-20
    assert R.TANH_E == 2 * R.TANH_E_MEASURED + 2


@pytest.mark.parametrize("hw", [(2, 2), (3, 2), (5, 7), (8, 130), (9, 129)])
def test_blur_down_judges_match_the_oracle_and_its_autograd(hw):
    g = torch.Generator().manual_seed(hw[0] * 7 + hw[1])
    x, sc, sh = rnd(g, 2, 3, *hw), rnd(g, 2, 3), rnd(g, 2, 3) * 0.3
    for a in (0, 1, 2):
        ref, unit = R.blur_down(x, sc, sh, a)["out"]
        assert close(ref, nets.blur_down(act32(x * sc[:, :, None, None] + sh[:, :, None, None], a)))
        refuses(ref, unit)
    assert close(R.blur_down(x)["out"][0], nets.blur_down(x))
    xg = x.clone().requires_grad_(True)
    y = nets.blur_down(xg)
    dy, d0 = rnd(g, *y.shape), rnd(g, *x.shape)
    (y * dy).sum().backward()
    assert close(R.blur_down_bwd(dy, hw)["din"][0], xg.grad)
    ref, unit = R.blur_down_bwd(dy, hw, d0)["din"]
    assert close(ref, xg.grad + d0)
    refuses(ref, unit)


@pytest.mark.parametrize("hw", [(1, 1), (1, 3), (5, 33), (3, 64)])
def test_blur_up_judges_match_the_oracle_and_its_autograd(hw):
    g = torch.Generator().manual_seed(hw[0] * 7 + hw[1])
    x, sc, sh = rnd(g, 2, 3, *hw), rnd(g, 2, 3), rnd(g, 2, 3) * 0.3
    for a in (0, 1, 2):
        ref, unit = R.blur_up(x, sc, sh, a)["out"]
        assert close(ref, nets.blur_up(act32(x * sc[:, :, None, None] + sh[:, :, None, None], a)))
        refuses(ref, unit, border=hw != (1, 1))
    xg = x.clone().requires_grad_(True)
    y = nets.blur_up(xg)
    dy, d0 = rnd(g, *y.shape), rnd(g, *x.shape)
    (y * dy).sum().backward()
    assert close(R.blur_up_bwd(dy, hw)["din"][0], xg.grad)
    ref, unit = R.blur_up_bwd(dy, hw, d0)["din"]
    assert close(ref, xg.grad + d0)
    refuses(ref, unit, border=hw[1] > 1)


@pytest.mark.parametrize("K", [1, 3, 5, 7, 8])
@pytest.mark.parametrize("origin", [(0, 0), (4, 0), (0, 4), (4, 4), (-3, -3), (-1, 0), (7, 7)])
def test_tap_judges_match_a_slice_of_the_zero_extended_grid(K, origin):
    g = torch.Generator().manual_seed(K)
    oy, ox = origin
    w = rnd(g, 17, K, K).requires_grad_(True)
    block = F.pad(w, (3, 11 - K, 3, 11 - K))[:, oy + 3:oy + 7, ox + 3:ox + 7]
    assert torch.equal(R.tap_embed(w.detach(), K, oy, ox), block.detach())
    dw4, dw0 = rnd(g, 17, 4, 4), rnd(g, 17, K, K)
    (block * dw4).sum().backward()
    res = R.tap_extract(dw4, K, oy, ox)
    own = torch.zeros(K, K, dtype=torch.bool)
    own[max(oy, 0):max(min(oy + 4, K), 0), max(ox, 0):max(min(ox + 4, K), 0)] = True
    assert torch.equal(res["own"], own) and torch.equal(res["dw"][0], w.grad) and bool((w.grad[:, ~own] == 0).all())
    acc = R.tap_extract(dw4, K, oy, ox, dw0)["dw"]
    assert close(acc[0], dw0 + w.grad) and bool((acc[1][:, ~own] == 0).all()) and torch.equal(acc[0][:, ~own], dw0[:, ~own])
    if bool(own.any()):
        refuses(acc[0], acc[1], border=False)


@pytest.mark.parametrize("geom", [(32, 32, 64, 64), (37, 53, 32, 32), (96, 80, 24, 20), (32, 32, 32, 32), (5, 300, 3, 7)])
def test_resample_table_judge_applies_the_host_built_tables(geom):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visual-tactile-synthesis_amd"))
    from vts import ops
    ih, iw, oh, ow = geom
    g = torch.Generator().manual_seed(ih + oh)
    x, o0 = rnd(g, 1, 2, ih, iw), rnd(g, 1, 2, oh, ow)
    ay, ax = ops._aa_axis(ih, oh), ops._aa_axis(iw, ow)
    ref, unit = R.resample_table(x, ay, ax)["out"]
    # a direct table product, element by element
    want = torch.zeros(1, 2, oh, ow, dtype=D64)
    for y in range(oh):
        for xx in range(ow):
            win = x[:, :, ay[0][y]:ay[0][y] + ay[1][y], ax[0][xx]:ax[0][xx] + ax[1][xx]]
            wy, wx = torch.from_numpy(ay[2][y, :ay[1][y]]).double(), torch.from_numpy(ax[2][xx, :ax[1][xx]]).double()
            want[:, :, y, xx] = torch.einsum("ncji,j,i->nc", win, wy, wx)
    assert close(ref, want)
    k = int(ay[1][1]) * int(ax[1][2])                     # K = ysize * xsize, r = 1
    absref = torch.einsum("oh,hw,pw->op", R.table_matrix(*ay, ih).abs(), x[0, 0].abs(), R.table_matrix(*ax, iw).abs())[1, 2]
    assert abs(float(unit[0, 0, 1, 2]) / (R.U * (k + 1) * float(absref)) - 1) < 1e-12
    # ... which is PyTorch's anti-aliased bicubic up to the tables' fp32 weights
    assert float((ref - F.interpolate(x, (oh, ow), mode="bicubic", align_corners=False, antialias=True)).abs().max()) < 5e-6
    if (ih, iw) == (oh, ow):
        assert torch.equal(ref, x)
    refuses(ref, unit)
    acc = R.resample_table(x, ay, ax, o0)["out"]
    assert close(acc[0], want + o0) and bool((acc[1] > unit).all())
    # the adjoint through the transposed tables is autograd's
    xg = x.clone().requires_grad_(True)
    (torch.einsum("oh,nchw,pw->ncop", R.table_matrix(*ay, ih), xg, R.table_matrix(*ax, iw)) * o0).sum().backward()
    adj, aunit = R.resample_table(o0, ops._aa_transpose(*ay, ih), ops._aa_transpose(*ax, iw))["out"]
    assert close(adj, xg.grad)
    refuses(adj, aunit)


UFD_CASES = [  # kernel shape or taps, up, down, padx, pady, H, W
    ((1, 3, 3, 1), 1, 1, (2, 1), (2, 1), 9, 11), ((1, 3, 3, 1), 1, 1, (1, 1), (1, 1), 17, 65), ((1, 3, 3, 1), 2, 1, (2, 1), (2, 1), 5, 7),
    ((1, 3, 3, 1), 1, 2, (1, 1), (1, 1), 9, 12), ((1, 3, 3, 1), 2, 2, (2, 1), (2, 1), 7, 6), ((1, 3, 3, 1), 1, 1, (-1, 2), (-1, 2), 8, 9),
    ((1,), 1, 1, (0, 0), (0, 0), 4, 5), ((2, 3), 1, 1, (1, 2), (0, 1), 6, 7), ((9, 7), 1, 1, (3, 3), (4, 4), 6, 10), ((2, 3), 3, 2, (2, -1), (-2, 4), 6, 7),
]


def ufd_by_definition(x, k, up, down, padx, pady):
    """zero insertion, F.pad with negative pads as crops, conv2d with the flipped kernel, decimation"""
    n, c, h, w = x.shape
    u = x.new_zeros(n, c, h * up, w * up)
    u[:, :, ::up, ::up] = x
    p = F.pad(u, (padx[0], padx[1], pady[0], pady[1]))
    y = F.conv2d(p.reshape(n * c, 1, *p.shape[-2:]), torch.flip(k, [0, 1])[None, None])
    return y.reshape(n, c, *y.shape[-2:])[:, :, ::down, ::down]


@pytest.mark.parametrize("case", UFD_CASES)
def test_upfirdn2d_judges_match_the_definition_the_oracle_and_autograd(case):
    taps, up, down, padx, pady, h, w = case
    g = torch.Generator().manual_seed(h * 31 + w)
    k = sg2.make_kernel(taps).double() * up * up if len(taps) != 2 else rnd(g, *taps)
    x = rnd(g, 2, 3, h, w).requires_grad_(True)
    want = ufd_by_definition(x, k, up, down, padx, pady)
    ref, unit = R.upfirdn2d(x, k, up, down, padx, pady)["out"]
    assert ref.shape == want.shape and close(ref, want.detach())
    if padx == pady:
        assert close(ref, sg2.upfirdn2d(x.detach(), k, up, down, padx))
    refuses(ref, unit)
    dy, o0, d0 = rnd(g, *want.shape), rnd(g, *want.shape), rnd(g, 2, 3, h, w)
    (want * dy).sum().backward()
    acc = R.upfirdn2d(x, k, up, down, padx, pady, o0)["out"]
    assert close(acc[0], want.detach() + o0) and bool((acc[1] >= unit).all())
    assert close(R.upfirdn2d_bwd(dy, (h, w), k, up, down, padx, pady)["din"][0], x.grad)
    ref, unit = R.upfirdn2d_bwd(dy, (h, w), k, up, down, padx, pady, d0)["din"]
    assert close(ref, x.grad + d0)
    refuses(ref, unit)


def test_upfirdn2d_unit_counts_only_the_taps_that_meet_a_sample():
    k = sg2.make_kernel((1, 3, 3, 1)).double()
    x = torch.ones(1, 1, 4, 4, dtype=D64)
    ref, unit = R.upfirdn2d(x, k, 1, 1, (2, 1), (2, 1))["out"]
    assert abs(float(unit[0, 0, 0, 0]) - R.U * 4 * float(ref[0, 0, 0, 0])) < 1e-22 and abs(float(unit[0, 0, 2, 2]) - R.U * 16) < 1e-22
    ref, unit = R.upfirdn2d(x, k, 1, 1, (5, 5), (0, 0))["out"]                 # outputs that see padding only: exactly 0
    assert float(ref[0, 0, 0, 0]) == 0 and float(unit[0, 0, 0, 0]) == 0 and float(unit[0, 0, 0, 4]) > 0


@pytest.mark.parametrize("sg", [(0.2, math.sqrt(2.0)), (0.2, 0.7), (0.0, 1.0)])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 99)])
def test_bias_act_judges_match_the_fused_leaky_relu_and_autograd(sg, shape):
    g = torch.Generator().manual_seed(shape[2])
    s32, g32 = R._f32(sg[0]), R._f32(sg[1])
    x, b, res, dy = rnd(g, *shape), rnd(g, shape[1]), rnd(g, *shape), rnd(g, *shape)
    x[:, :, ::7] = -b[None, :, None]                                            # exact ties
    for bias in (b, None):
        for r in (res, None):
            xg = x.clone().requires_grad_(True)
            y = F.leaky_relu(xg + (0 if bias is None else bias[None, :, None]), s32) * g32
            ref, unit = R.bias_act(x, bias, r, *sg)["out"]
            assert close(ref, y.detach() + (0 if r is None else r))
            if bias is not None:
                assert bool((ref[:, :, ::7] == (0 if r is None else r[:, :, ::7])).all())
                assert close(ref, sg2.fused_leaky_relu(x, bias, s32, g32) + (0 if r is None else r))
            if float(unit.max()) > 0:
                refuses(ref, unit, border=False)
            (y * dy).sum().backward()
            ref, unit = R.bias_act_bwd(dy, x, bias, *sg)["dx"]
            assert close(ref, xg.grad)                                          # autograd takes the slope branch at 0 as well
            if bias is not None:
                assert close(ref[:, :, ::7], dy[:, :, ::7] * s32 * g32)
            if float(unit.max()) > 0:
                refuses(ref, unit, border=False)
    assert float(R.bias_act(x, None, None, 0.0, 1.0)["out"][1].max()) == 0       # ReLU without bias, gain or residual: exact


@pytest.mark.parametrize("geom", [(14, 6, 46, 74), (9, 3, 111, 123), (46, 74, 14, 6), (7, 9, 7, 9), (5, 6, 10, 12), (30, 20, 4, 6)])
def test_nearest_judges_match_f_interpolate_and_its_autograd(geom):
    ih, iw, oh, ow = geom
    g = torch.Generator().manual_seed(ih + ow)
    x32 = torch.randn(2, 3, ih, iw, generator=g)
    assert torch.equal(R.nearest_resize(x32, (oh, ow)), F.interpolate(x32, (oh, ow), mode="nearest"))
    x = x32.double().requires_grad_(True)
    dy, d0 = rnd(g, 2, 3, oh, ow), rnd(g, 2, 3, ih, iw)
    (F.interpolate(x, (oh, ow), mode="nearest") * dy).sum().backward()
    assert close(R.nearest_resize_bwd(dy, (ih, iw))["din"][0], x.grad)
    ref, unit = R.nearest_resize_bwd(dy, (ih, iw), d0)["din"]
    assert close(ref, x.grad + d0)
    refuses(ref, unit)
    if geom == (30, 20, 4, 6):
        plain = R.nearest_resize_bwd(dy, (ih, iw))["din"]
        assert int((plain[0][0, 0] == 0).sum()) == ih * iw - oh * ow and bool((plain[1][plain[0] == 0] == 0).all())


def test_up2_and_tanh_bwd_judges_match_autograd():
    g = torch.Generator().manual_seed(12)
    x32 = torch.randn(1, 7, 3, 5, generator=g)
    assert torch.equal(R.nearest_up2(x32), F.interpolate(x32, scale_factor=2, mode="nearest"))
    x = x32.double().requires_grad_(True)
    dy, d0 = rnd(g, 1, 7, 6, 10), rnd(g, 1, 7, 3, 5)
    (F.interpolate(x, scale_factor=2, mode="nearest") * dy).sum().backward()
    ref, unit = R.nearest_up2_bwd(dy, d0)["din"]
    assert close(ref, x.grad + d0) and close(R.nearest_up2_bwd(dy)["din"][0], x.grad)
    refuses(ref, unit)
    z = rnd(g, 257).requires_grad_(True)
    y, gz = torch.tanh(z), rnd(g, 257)
    (y * gz).sum().backward()
    ref, unit = R.tanh_bwd(gz, y.detach())["dz"]
    assert close(ref, z.grad) and close(unit, 3 * R.U * gz.abs() * (1 + y.detach() ** 2))
    refuses(ref.view(1, 257), unit.view(1, 257), border=False)
