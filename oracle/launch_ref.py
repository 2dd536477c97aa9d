"""Float64 judge of the C ABI's conv / weight-gradient / normalisation semantics, written from the formulas in include/vts.h (not from
the kernels).  Checker only: the product never imports it.

Every function returns {name: (ref, unit)} with float64 tensors: `ref` the exact value, `unit` the elementwise error scale of an
fp32 evaluation, u * sqrt(K) * absref, where u = 2^-24, K is the number of products summed into the element and absref is the same
expression with every product and addend in absolute value.  A result passes when |got - ref| <= c * unit everywhere, with one
constant c per family (tests/test_step_launches_gpu.py states them next to the worst value measured).  Unlike a relative L2 norm
this does not dilute one bad element by sqrt(numel).

Operands are passed dense: Opnd(data [N, C, H, W], scale [N, C] or None, shift [N, C] or None); their value is
act(data * scale + shift) (vts_operand).  Weights are the flat buffer the descriptor's `w` points to, read as
W(co, ci, ky, kx) = w[co * ws_co + ci * ws_ci + ky * 4 + kx]."""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24
SLOPE = {0: None, 1: 0.2, 2: 0.0}        # VTS_ACT_NONE / LRELU / RELU

Opnd = namedtuple("Opnd", "data scale shift")


def _f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def value(op, act=0):
    """(value, magnitude) of an operand: magnitude = |data * scale| + |shift| through the activation's slope (the fp32 affine
    rounds relative to that)"""
    x = _f64(op.data)
    n, c = x.shape[:2]
    a = x.abs()
    if op.scale is not None:
        s = _f64(op.scale).view(n, c, 1, 1)
        x = x * s
        a = a * s.abs()
    if op.shift is not None:
        b = _f64(op.shift).view(n, c, 1, 1)
        x = x + b
        a = a + b.abs()
    slope = SLOPE[act]
    if slope is not None:
        f = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))
        x, a = x * f, a * f
    return x, a


def dact(op, act):
    """act'(operand value): the derivative mask factor (LRELU: v > 0 ? 1 : 0.2; RELU: v > 0 ? 1 : 0)"""
    v, _ = value(op)
    return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, SLOPE[act]))


def _cat(op0, op1, act):
    v, a = value(op0, act)
    if op1 is not None and op1.data is not None and op1.data.shape[1]:
        v1, a1 = value(op1, act)
        v, a = torch.cat([v, v1], 1), torch.cat([a, a1], 1)
    return v, a


def _window(x, oy, ox, h, w):
    """t[..., r, c] = x[..., r + oy, c + ox], zero outside x"""
    out = x.new_zeros(x.shape[:-2] + (h, w))
    r0, r1 = max(0, -oy), min(h, x.shape[-2] - oy)
    c0, c1 = max(0, -ox), min(w, x.shape[-1] - ox)
    if r1 > r0 and c1 > c0:
        out[..., r0:r1, c0:c1] = x[..., r0 + oy:r1 + oy, c0 + ox:c1 + ox]
    return out


def weights(w, cout, cin, ws_co, ws_ci):
    """W [Cout, Cin, 4, 4] from the flat weight buffer"""
    w = _f64(w).reshape(-1)
    need = (cout - 1) * ws_co + (cin - 1) * ws_ci + 16
    assert w.numel() >= need, (w.numel(), need)
    return torch.as_strided(w, (cout, cin, 4, 4), (ws_co, ws_ci, 4, 1))


def _conv_core(x, W, d):
    """sum over (ci, ky, kx) of the conv / transposed-conv formula of vts_conv_desc, one matmul per tap"""
    n, cin = x.shape[:2]
    cout = W.shape[0]
    s, pt, pl = d["stride"], d["pad"], d["pad"] + d["pad_dx"]
    oh, ow = d["OH"], d["OW"]
    out = x.new_zeros(n, cout, oh, ow)
    if not d["transposed"]:
        # out[oy, ox] += in[oy*s + ky - pt, ox*s + kx - pl] W[ky, kx]
        P = _window(x, -pt, -pl, (oh - 1) * s + 4, (ow - 1) * s + 4)
        for ky in range(4):
            for kx in range(4):
                sl = P[:, :, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s].reshape(n, cin, oh * ow)
                out += torch.matmul(W[:, :, ky, kx], sl).view(n, cout, oh, ow)
        return out
    # transposed: out[y, x] += in[(y + pt - ky) / s, (x + pl - kx) / s] W[ky, kx] where both divide
    for ky in range(4):
        y0 = (ky - pt) % s
        ny = len(range(y0, oh, s))
        for kx in range(4):
            x0 = (kx - pl) % s
            nx = len(range(x0, ow, s))
            if not ny or not nx:
                continue
            sl = _window(x, (y0 + pt - ky) // s, (x0 + pl - kx) // s, ny, nx).reshape(n, cin, ny * nx)
            out[:, :, y0::s, x0::s] += torch.matmul(W[:, :, ky, kx], sl).view(n, cout, ny, nx)
    return out


def conv_terms(d):
    """K: products summed into one output element"""
    cin = d["in0"]["C"] + d["in1"]["C"]
    if d["transposed"]:
        return cin * math.ceil(4 / d["stride"]) ** 2
    return cin * 16


def conv4x4(d, in0, w, *, in1=None, bias=None, dmask=None, out0=None):
    """vts_conv4x4: d = the descriptor's scalar fields (dict keyed like vts_conv_desc; in0/in1 sub-dicts need only "C").
    out0: the output's previous content (accumulate)."""
    x, a = _cat(in0, in1, d["act_in"])
    cin = x.shape[1]
    W = weights(w, d["Cout"], cin, d["ws_co"], d["ws_ci"])
    ref = _conv_core(x, W, d)
    absref = _conv_core(a, W.abs(), d)
    if bias is not None:
        b = _f64(bias).view(1, -1, 1, 1)
        ref, absref = ref + b, absref + b.abs()
    K = conv_terms(d)
    unit = U * math.sqrt(K) * absref
    if d["act_out"] == 3:
        t = torch.tanh(ref)
        unit = unit * (1 - t * t) + 4 * U * t.abs()     # the tanh contracts the sum's error; its own rounding is a few ulp
        ref = t
    if dmask is not None:
        f = dact(dmask, d["dmask_act"])
        ref, unit = ref * f, unit * f
    if d["accumulate"]:
        o = _f64(out0).reshape(ref.shape)
        ref, unit = ref + o, unit + U * o.abs()
    return {"out": (ref, unit)}


def wgrad_terms(d):
    return d["N"] * d["LH"] * d["LW"]


def wgrad4x4(d, lo0, hi0, *, lo1=None, hi1=None, dw0=None):
    """vts_wgrad4x4: dw[cl, ch, ky, kx] = sum_{n, y, x} lo[n, cl, y, x] hi[n, ch, y*s + ky - pad, x*s + kx - pad - pad_dx]
    ([CL, CH, 4, 4]); dw0: the previous content (accumulate)"""
    lo, alo = _cat(lo0, lo1, d["act_lo"])
    hi, ahi = _cat(hi0, hi1, d["act_hi"])
    ref = _wgrad_core(lo, hi, d)
    absref = _wgrad_core(alo, ahi, d)
    unit = U * math.sqrt(wgrad_terms(d)) * absref
    if d["accumulate"] and dw0 is not None:
        o = _f64(dw0).view_as(ref)
        ref, unit = ref + o, unit + U * o.abs()
    return {"dw": (ref, unit)}


def _wgrad_core(lo, hi, d):
    n, cl, lh, lw = lo.shape
    ch = hi.shape[1]
    s, pt, pl = d["stride"], d["pad"], d["pad"] + d["pad_dx"]
    lo2 = lo.transpose(0, 1).reshape(cl, n * lh * lw)
    P = _window(hi, -pt, -pl, (lh - 1) * s + 4, (lw - 1) * s + 4)
    dw = lo.new_zeros(cl, ch, 4, 4)
    for ky in range(4):
        for kx in range(4):
            sl = P[:, :, ky:ky + (lh - 1) * s + 1:s, kx:kx + (lw - 1) * s + 1:s].transpose(0, 1).reshape(ch, n * lh * lw)
            dw[:, :, ky, kx] = lo2 @ sl.T
    return dw


def _passes(n, mode, gstart):
    if mode == 0:
        return [(i, i + 1) for i in range(n)]
    g = list(gstart) if gstart else [0, n]
    return list(zip(g[:-1], g[1:]))


def norm_stats(x, mode, *, eps, momentum, gamma=None, beta=None, running_mean=None, running_var=None, nbt=None, gstart=None,
               ext=None, stat_out=False):
    """vts_norm_stats.  x [N, C, H, W]; mode 0 InstanceNorm (group (n, c)), 1 training BatchNorm (group c per pass; passes
    gstart = [0, g1, ..., N]); running_mean / running_var / nbt: their values before the call (updated per pass with the unbiased
    variance); ext = (mean [C], uvar [C], after): a recorded pass applied after pass `after`; stat_out: also return pass 0's
    batch mean and unbiased variance."""
    x = _f64(x)
    n, c = x.shape[:2]
    x = x.reshape(n, c, -1)
    hw = x.shape[2]
    g = _f64(gamma) if (mode == 1 and gamma is not None) else x.new_ones(c)
    b = _f64(beta) if (mode == 1 and beta is not None) else x.new_zeros(c)
    res = {k: [x.new_zeros(n, c), x.new_zeros(n, c)] for k in ("scale", "shift", "mean", "rstd")}
    rm = [_f64(running_mean), x.new_zeros(c)] if running_mean is not None else None
    rv = [_f64(running_var), x.new_zeros(c)] if running_var is not None else None

    def run_update(mean, em, uvar, euvar):
        for r, v, e in ((rm, mean, em), (rv, uvar, euvar)):
            if r is not None:
                r[1] = (1 - momentum) * r[1] + momentum * e + 2 * U * ((1 - momentum) * r[0].abs() + momentum * v.abs())
                r[0] = (1 - momentum) * r[0] + momentum * v

    stat = None
    for gi, (n0, n1) in enumerate(_passes(n, mode, gstart)):
        xs = x[n0:n1]                                  # [np, C, HW]
        K = (n1 - n0) * hw
        if mode == 0:
            mean = xs.mean(2)[0]
            var = ((xs - mean.view(1, c, 1)) ** 2).mean(2)[0]
            eabs = xs.abs().mean(2)[0]
        else:
            mean = xs.mean((0, 2))
            var = ((xs - mean.view(1, c, 1)) ** 2).mean((0, 2))
            eabs = xs.abs().mean((0, 2))
        em = U * math.sqrt(K) * eabs + U * mean.abs()
        ev = U * math.sqrt(K) * var + em * em
        rstd = 1.0 / torch.sqrt(var + eps)
        ers = rstd * (0.5 * ev / (var + eps) + 2 * U)
        if mode == 0:
            gg, bb, rows = x.new_ones(c), x.new_zeros(c), slice(n0, n1)
        else:
            gg, bb, rows = g, b, slice(n0, n1)
        scale = gg * rstd
        shift = bb - mean * scale
        vals = {"scale": (scale, gg.abs() * ers + U * scale.abs()),
                "shift": (shift, gg.abs() * (em * rstd + mean.abs() * ers) + 2 * U * (bb.abs() + (mean * scale).abs())),
                "mean": (mean, em), "rstd": (rstd, ers)}
        for k, (v, e) in vals.items():
            res[k][0][rows] = v
            res[k][1][rows] = e
        if mode == 1:
            uvar = var * K / (K - 1)
            euvar = ev * K / (K - 1) + U * uvar
            if gi == 0:
                stat = {"stat_mean": (mean, em), "stat_uvar": (uvar, euvar)}
            run_update(mean, em, uvar, euvar)
            if ext is not None and gi == ext[2]:
                m_e, v_e = _f64(ext[0]), _f64(ext[1])
                run_update(m_e, torch.zeros_like(m_e), v_e, torch.zeros_like(v_e))
    out = {k: (v[0].reshape(-1), v[1].reshape(-1)) for k, v in res.items()}
    if rm is not None:
        out["running_mean"] = tuple(rm)
    if rv is not None:
        out["running_var"] = tuple(rv)
    if nbt is not None:
        npass = len(_passes(n, mode, gstart))
        out["nbt"] = (torch.tensor([float(int(nbt) + npass + (1 if ext is not None else 0))], dtype=torch.float64), torch.zeros(1, dtype=torch.float64))
    if stat_out and stat is not None:
        out.update(stat)
    return out


def norm_bwd(dy, x, mean, rstd, mode, *, gamma=None, dgamma0=None, dbeta0=None, accumulate=False, gstart=None, sums_beta=None,
             dy_unit=None):
    """vts_norm_bwd: dx = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)), xhat = (x - mean) rstd, per group (IN: (n, c);
    BN: c per pass, mean / rstd of the pass's first sample); BN also dgamma = sum dy xhat, dbeta = sum dy over every pass
    (+ dgamma0 / dbeta0 with accumulate).  mean / rstd [N * C].
    sums_beta (the BatchNorm shift, or zeros for InstanceNorm): the sums came from a convolution epilogue as S1 = sum dy and
    S2' = sum dy (gamma xhat + beta), so S2 = (S2' - beta S1) / gamma carries the rounding of S2'.  dy_unit: error scale already
    present in dy (a first stage's), propagated."""
    dy, x = _f64(dy), _f64(x)
    n, c = dy.shape[:2]
    dy, x = dy.reshape(n, c, -1), x.reshape(n, c, -1)
    hw = dy.shape[2]
    mean, rstd = _f64(mean).view(n, c), _f64(rstd).view(n, c)
    g = _f64(gamma) if (mode == 1 and gamma is not None) else dy.new_ones(c)
    dx, udx = torch.empty_like(dy), torch.empty_like(dy)
    dg, db = dy.new_zeros(c), dy.new_zeros(c)
    udg, udb = dy.new_zeros(c), dy.new_zeros(c)
    for n0, n1 in _passes(n, mode, gstart):
        m = (n1 - n0) * hw
        mu, rs = mean[n0].view(1, c, 1), rstd[n0].view(1, c, 1)
        ds, xs = dy[n0:n1], x[n0:n1]
        xh = (xs - mu) * rs
        axh = (xs.abs() + mu.abs()) * rs
        s1, s2 = ds.sum((0, 2)), (ds * xh).sum((0, 2))
        us1 = U * math.sqrt(m) * ds.abs().sum((0, 2))
        if sums_beta is not None:
            bb = _f64(sums_beta).view(1, c, 1) if mode == 1 else dy.new_zeros(1, c, 1)
            gg = g.view(1, c, 1)
            us2 = U * math.sqrt(m) * (ds.abs() * (gg.abs() * axh + bb.abs())).sum((0, 2)) / gg.abs().view(c) + bb.abs().view(c) * us1 / gg.abs().view(c)
        else:
            us2 = U * math.sqrt(m) * (ds.abs() * axh).sum((0, 2))
        if dy_unit is not None:
            e = _f64(dy_unit).reshape(n, c, -1)[n0:n1]
            us1 = us1 + e.sum((0, 2))
            us2 = us2 + (e * axh).sum((0, 2))
        A = (g * rs.view(c)).view(1, c, 1)
        v = A * (ds - s1.view(1, c, 1) / m - xh * s2.view(1, c, 1) / m)
        av = A.abs() * (ds.abs() + s1.abs().view(1, c, 1) / m + axh * s2.abs().view(1, c, 1) / m)
        uv = 4 * U * av + A.abs() * (us1.view(1, c, 1) / m + axh * us2.view(1, c, 1) / m)
        if dy_unit is not None:
            uv = uv + A.abs() * _f64(dy_unit).reshape(n, c, -1)[n0:n1]
        dx[n0:n1], udx[n0:n1] = v, uv
        dg, db = dg + s2, db + s1
        udg, udb = udg + us2 + U * s2.abs(), udb + us1 + U * s1.abs()
    out = {"dx": (dx.reshape(n, c, hw), udx.reshape(n, c, hw))}
    if mode == 1:
        if accumulate and dgamma0 is not None:
            dg, udg = dg + _f64(dgamma0), udg + U * _f64(dgamma0).abs()
        if accumulate and dbeta0 is not None:
            db, udb = db + _f64(dbeta0), udb + U * _f64(dbeta0).abs()
        out["dgamma"], out["dbeta"] = (dg, udg), (db, udb)
    return out


# ---- the GEMM-class "wide" ABI (vts_conv3x3_wide / _s2 / vts_tconv3x3s2_wide / vts_conv4x4_wide / vts_wgrad3x3_wide / vts_wgrad4x4_wide) ------
# Written from the formulas of include/vts.h.  Inputs are the PRE-PADDED identity operands the entries take; weights are the operator's
# UNPACKED weight (what vts_w3x3_pack / vts_w4x4_pack read), not the packed buffer.

def _valid_conv(p, w, K, s, oh, ow):
    """sum_{ci, ky, kx} p[n, ci, s y + ky, s x + kx] w[co, ci, ky, kx], one matmul per tap"""
    n, cin = p.shape[:2]
    cout = w.shape[0]
    out = p.new_zeros(n, cout, oh, ow)
    for ky in range(K):
        for kx in range(K):
            sl = p[:, :, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s].reshape(n, cin, oh * ow)
            out += torch.matmul(w[:, :, ky, kx], sl).view(n, cout, oh, ow)
    return out


def _pad1(t):
    return torch.nn.functional.pad(t, (1, 1, 1, 1))


def conv_wide(p, w, bias, *, K, stride, out_hw=None, epilogue=None, mask=None, add=None):
    """vts_conv3x3_wide / vts_conv3x3s2_wide / vts_conv4x4_wide (transposed = 0): the valid K x K convolution (K 3 | 4) of the pre-padded
    p [N, Cin, PH, PW] with the operator weight w [Cout, Cin, K, K], stride 1 | 2; K_terms = Cin K^2.  out_hw: the output extent where the
    entry is told it (4 x 4), else the largest that fits.
    epilogue "relu_pad" (vts_conv3x3_wide_relu_pad): max(ref, 0) inside a one-pixel border of exact zeros, the unit unchanged;
    "mask_pad" (vts_conv3x3_wide_mask_pad): (ref + add) where mask > 0, else exactly 0; mask / add in the padded layout [N, Cout, H + 2, W + 2]."""
    p, w = _f64(p), _f64(w)
    assert w.shape[1] == p.shape[1] and w.shape[2:] == (K, K) and stride in (1, 2)
    oh, ow = out_hw if out_hw is not None else ((p.shape[2] - K) // stride + 1, (p.shape[3] - K) // stride + 1)
    assert p.shape[2] >= stride * (oh - 1) + K and p.shape[3] >= stride * (ow - 1) + K
    ref = _valid_conv(p, w, K, stride, oh, ow)
    absref = _valid_conv(p.abs(), w.abs(), K, stride, oh, ow)
    if bias is not None:
        b = _f64(bias).view(1, -1, 1, 1)
        ref, absref = ref + b, absref + b.abs()
    scale = U * math.sqrt(w.shape[1] * K * K)
    if epilogue is None:
        return {"out": (ref, scale * absref)}
    if epilogue == "relu_pad":
        return {"out": (_pad1(ref.clamp_min(0)), _pad1(scale * absref))}
    assert epilogue == "mask_pad" and mask is not None
    ref, absref = _pad1(ref), _pad1(absref)
    if add is not None:
        ref, absref = ref + _f64(add), absref + _f64(add).abs()
    keep = (_f64(mask) > 0).to(torch.float64)
    keep[:, :, 0], keep[:, :, -1], keep[:, :, :, 0], keep[:, :, :, -1] = 0, 0, 0, 0       # the border is zero whatever the mask holds
    return {"out": (ref * keep, scale * absref * keep)}


def _tconv_s2(p, w, K, pad, oh, ow):
    """out[n, b, 2 i + ky - pad, 2 j + kx - pad] += p[n, a, i, j] w[a, b, ky, kx] (scatter form), and the number of taps that reach
    each output element: (sum [N, B, OH, OW], taps [OH, OW])"""
    n, cin, ih, iw = p.shape
    cout = w.shape[1]
    out = p.new_zeros(n, cout, oh, ow)
    taps = p.new_zeros(oh, ow)
    for ky in range(K):
        ii = [i for i in range(ih) if 0 <= 2 * i + ky - pad < oh]
        for kx in range(K):
            jj = [j for j in range(iw) if 0 <= 2 * j + kx - pad < ow]
            if not ii or not jj:
                continue
            sl = p[:, :, ii[0]:ii[-1] + 1, jj[0]:jj[-1] + 1].reshape(n, cin, len(ii) * len(jj))
            y0, x0 = 2 * ii[0] + ky - pad, 2 * jj[0] + kx - pad
            out[:, :, y0:y0 + 2 * len(ii):2, x0:x0 + 2 * len(jj):2] += torch.matmul(w[:, :, ky, kx].T, sl).view(n, cout, len(ii), len(jj))
            taps[y0 % 2::2, x0 % 2::2] += 1      # every element of that parity phase sums this tap (rows beyond the data are the appended zeros)
    return out, taps


def _tconv_judge(p, w, bias, K, pad, oh, ow):
    p, w = _f64(p), _f64(w)
    assert w.shape[0] == p.shape[1] and w.shape[2:] == (K, K)
    ref, taps = _tconv_s2(p, w, K, pad, oh, ow)
    absref, _ = _tconv_s2(p.abs(), w.abs(), K, pad, oh, ow)
    if bias is not None:
        b = _f64(bias).view(1, -1, 1, 1)
        ref, absref = ref + b, absref + b.abs()
    return {"out": (ref, U * torch.sqrt(p.shape[1] * taps).view(1, 1, oh, ow) * absref)}


def tconv3x3s2_wide(p, w, bias):
    """vts_tconv3x3s2_wide: ConvTranspose2d(3, stride 2, padding 1, output_padding 1) of p [N, Cin, IH + 1, IW + 1] (the input with one zero
    row / column appended) with w [Cin, Cout, 3, 3] -> [N, Cout, 2 IH, 2 IW]; out[y] sums in[i] w[k] over k = y + 1 - 2 i in 0..2, so
    K_terms = Cin {1, 2, 2, 4} by output parity (the unit is per phase)."""
    return _tconv_judge(p, w, bias, 3, 1, 2 * (p.shape[2] - 1), 2 * (p.shape[3] - 1))


def conv4x4_wide_transposed(p, w, bias, out_hw):
    """vts_conv4x4_wide (transposed = 1): the input adjoint of Conv2d(4, stride 2, padding 2).  p [N, Cin, PH, PW] is the output gradient
    with one zero row / column appended, w [Cin, Cout, 4, 4] the layer's weight (its output channels first), out [N, Cout, OH, OW]:
    out[i] = sum over (y, k) with 2 y + k - 2 = i of p[y] w[k]: 2 x 2 taps per element, K_terms = 4 Cin; with odd OH / OW the odd phase
    is one row / column shorter."""
    oh, ow = out_hw
    assert 2 * (p.shape[2] - 1) >= oh + 1 and 2 * (p.shape[3] - 1) >= ow + 1
    return _tconv_judge(p, w, bias, 4, 2, oh, ow)


def wgrad_wide(dout, p, *, K, stride, dw0=None):
    """vts_wgrad3x3_wide / vts_wgrad4x4_wide: dw[co, ci, ky, kx] = sum_{n, y, x} dout[n, co, y, x] p[n, ci, s y + ky, s x + kx]
    (+ dw0 with accumulate); K_terms = N H W"""
    dout, p = _f64(dout), _f64(p)
    n, co, h, w = dout.shape
    ci = p.shape[1]
    assert p.shape[2] >= stride * (h - 1) + K and p.shape[3] >= stride * (w - 1) + K

    def core(d, q):
        d2 = d.transpose(0, 1).reshape(co, n * h * w)
        dw = d.new_zeros(co, ci, K, K)
        for ky in range(K):
            for kx in range(K):
                sl = q[:, :, ky:ky + (h - 1) * stride + 1:stride, kx:kx + (w - 1) * stride + 1:stride].transpose(0, 1).reshape(ci, n * h * w)
                dw[:, :, ky, kx] = d2 @ sl.T
        return dw
    ref = core(dout, p)
    unit = U * math.sqrt(n * h * w) * core(dout.abs(), p.abs())
    if dw0 is not None:
        o = _f64(dw0).view_as(ref)
        ref, unit = ref + o, unit + U * o.abs()
    return {"dw": (ref, unit)}


def wtap_pack(w, A, B, sa, sb, T, flip):
    """vts_w3x3_pack / vts_w4x4_pack (T = 9 | 16), the indexing formula itself: wt[(a T + t) Bp + b] = w[a sa + b sb + (flip ? T - 1 - t : t)]
    for b < B, 0 for B <= b < Bp = B rounded up to 4.  A pure permutation: the result is exact in the input's own dtype."""
    flat = w.detach().cpu().reshape(-1)
    Bp = (B + 3) // 4 * 4
    a = torch.arange(A).view(A, 1, 1)
    t = torch.arange(T).view(1, T, 1)
    b = torch.arange(B).view(1, 1, B)
    wt = flat.new_zeros(A, T, Bp)
    wt[:, :, :B] = flat[a * sa + b * sb + ((T - 1 - t) if flip else t)]
    return wt.reshape(-1)


def worst(got, ref, unit):
    """(max over elements of |got - ref| / unit, index of that element); inf where got is not finite.  An element whose unit is 0
    (an exact zero: masked out, empty sum) must match exactly."""
    got = _f64(got).reshape(-1)
    ref, unit = ref.reshape(-1), unit.reshape(-1)
    err = (got - ref).abs()
    r = torch.where(unit > 0, err / unit.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    i = int(torch.argmax(r))
    return float(r[i]), i
