"""Float64 judge of the C ABI's conv / weight-gradient / normalisation semantics, of the step's glue kernels (loss, optimiser,
pyramid, patches, post-processing, augmentation, staging, sampler) and of the padding / resampling / FIR operators (pad, blur, weight taps,
table resampling, upfirdn2d, bias_act, nearest, tanh_bwd; their units are derived rounding counts, see that section) and of the fp32 glue of
the perceptual terms (pooling, masks, the LPIPS head, the ReLU-L1, input scaling and stacking) and of the kernels that carry the style and
segmentation conditioning (SPADE modulate, eval statistics and spectral norm, AdaIN, the style bias and mapping Linear, the modconv
reductions: the last section, judged by tests/test_style_kernels_gpu.py on the table tests/style_kernel_cases.py, itself checked on the CPU
by tests/test_style_kernel_cases.py), written from the formulas in include/vts.h (not from the kernels).  Checker only: the product never imports it.

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


# ---- the step's glue kernels (csrc/vts_ops.hip): loss, optimiser, pyramid, patch, post-processing, augmentation, staging, sampler ----------
# Written from the formulas of include/vts.h and the reference semantics.  Arithmetic outputs: unit = u * r * absref, r = the number of
# fp32 roundings in the header formula (a libm call counts 2, a constant the caller passes as a float is exact), absref = the same
# expression with every term in absolute value -- a cancellation (1 - beta^t, x - mean) is therefore carried by absref, not by r.  Sums:
# u * sqrt(K) * absref.  Scalars are taken as the fp32 values the C ABI receives (_f32).  Data movement and integer results are exact:
# the judges return them in the output's own dtype and the tests compare bitwise.

def _f32(v):
    """the value a C float argument carries"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _pool_windows(x):
    """(sum of the valid taps, their number [OH, OW]) of AvgPool2d(3, 2, 1, count_include_pad=False) windows"""
    h, w = x.shape[-2:]
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    p = torch.nn.functional.pad(x, (1, 2 * ow - w, 1, 2 * oh - h))      # rows -1 .. 2 OH - 1
    one = torch.nn.functional.pad(x.new_ones(h, w), (1, 2 * ow - w, 1, 2 * oh - h))
    s, cnt = x.new_zeros(x.shape[:-2] + (oh, ow)), x.new_zeros(oh, ow)
    for dy in range(3):
        for dx in range(3):
            s = s + p[..., dy:dy + 2 * oh:2, dx:dx + 2 * ow:2]
            cnt = cnt + one[dy:dy + 2 * oh:2, dx:dx + 2 * ow:2]
    return s, cnt


def avgpool3s2(x):
    """vts_avgpool3s2: y[oy, ox] = mean of the taps x[2 oy + dy, 2 ox + dx], dy, dx in -1..1, that lie inside the map.  K = taps (<= 9)
    addends and one division: unit = u (sqrt(K) + 1) absref."""
    x = _f64(x)
    s, cnt = _pool_windows(x)
    a, _ = _pool_windows(x.abs())
    return {"y": (s / cnt, U * (torch.sqrt(cnt) + 1) * a / cnt)}


def _pool_adjoint(g, h, w):
    """sum over the windows covering (y, x) of g[oy, ox] / taps(oy, ox)"""
    oh, ow = g.shape[-2:]
    assert (oh, ow) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
    _, cnt = _pool_windows(g.new_ones(h, w))
    q = g / cnt
    buf = g.new_zeros(g.shape[:-2] + (2 * oh + 1, 2 * ow + 1))            # rows -1 .. 2 OH - 1
    for dy in range(3):
        for dx in range(3):
            buf[..., dy:dy + 2 * oh:2, dx:dx + 2 * ow:2] += q
    return buf[..., 1:1 + h, 1:1 + w]


def avgpool3s2_bwd(dy, h, w, dx0=None):
    """vts_avgpool3s2_bwd: dx[y, x] (+)= sum over the (<= 4) windows that cover (y, x) of dy[oy, ox] / taps(oy, ox): one division per term,
    sqrt(4) for the sum (r = 3), one more rounding for the accumulate"""
    g = _f64(dy)
    ref, a = _pool_adjoint(g, h, w), _pool_adjoint(g.abs(), h, w)
    unit = 3 * U * a
    if dx0 is not None:
        o = _f64(dx0)
        ref, unit = ref + o, unit + U * (o.abs() + a)
    return {"dx": (ref, unit)}


def _softplus(x):
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))      # F.softplus, threshold 20


GAN_L_ROUNDINGS = {0: 4, 1: 3, 2: 7, 3: 0, 4: 1, 5: 11}
GAN_G_ROUNDINGS = {0: 7, 1: 4, 2: 8, 3: 3, 4: 3, 5: 15}


def ganloss(pred, mode, real, label, coeff, grad_coeff, workgroups=1):
    """vts_ganloss, kernel modes 0-5 (include/vts.h).  per element l, g = dl/dp:
      0 nonsaturating  l = softplus(-+p)                       g = -+sigmoid(-+p)         (upper sign: target real)
      1 lsgan          l = (p - label)^2                       g = 2 (p - label)
      2 vanilla        l = max(p, 0) - p label + log1p(exp(-|p|))   g = sigmoid(p) - label
      3 wgan           l = -+p                                 g = -+1
      4 hinge          l = max(1 -+ p, 0)                      g = -+[1 -+ p > 0]
      5 vanilla on q = sigmoid(p):  l = q - q label + log1p(exp(-q)),  g = (sigmoid(q) - label) q (1 - q)
    "loss" = coeff / total * sum l: what one call adds to the slot, in units of 1.0 (slot / 2^40 minus its start value); K = total
    addends: unit = u (sqrt(K) + r_l + 1) coeff / total * sum absref_l + workgroups * 2^-41 (r_l: roundings of one l, 1: the fp32
    1 / total, 2^-41: each workgroup's rounding to fixed point).  "dpred" = grad_coeff / total * g: r_g roundings, which include 1 / total
    and the two products (GAN_L_ROUNDINGS / GAN_G_ROUNDINGS count them from the lines above: exp, log1p 2 each)."""
    p = _f64(pred).reshape(-1)
    label, coeff, grad_coeff = _f32(label), _f32(coeff), _f32(grad_coeff)
    total = p.numel()
    sg = -1.0 if real else 1.0
    sig = torch.sigmoid
    if mode == 0:
        l, g = _softplus(sg * p), sg * torch.where(sg * p > 20, torch.ones_like(p), sig(sg * p))      # F.softplus: identity above 20
        la, ga = l, g.abs()
    elif mode == 1:
        l, g = (p - label) ** 2, 2 * (p - label)
        la, ga = (p.abs() + abs(label)) ** 2, 2 * (p.abs() + abs(label))
    elif mode == 2:
        l, g = p.clamp_min(0) - p * label + torch.log1p(torch.exp(-p.abs())), sig(p) - label
        la, ga = p.clamp_min(0) + (p * label).abs() + torch.log1p(torch.exp(-p.abs())), sig(p) + abs(label)
    elif mode == 3:
        l, g = sg * p, torch.full_like(p, sg)
        la, ga = p.abs(), torch.ones_like(p)
    elif mode == 4:
        t = 1 + sg * p
        l, g = t.clamp_min(0), torch.where(t > 0, torch.full_like(p, sg), torch.zeros_like(p))
        la, ga = torch.where(t > 0, 1 + p.abs(), torch.zeros_like(p)), g.abs()
    else:
        assert mode == 5
        q = sig(p)
        l, g = q - q * label + torch.log1p(torch.exp(-q)), (sig(q) - label) * q * (1 - q)
        la, ga = q + q * abs(label) + torch.log1p(torch.exp(-q)), (sig(q) + abs(label)) * q * (1 + q)
    k = abs(coeff) / total
    loss = coeff / total * l.sum()
    ul = U * (math.sqrt(total) + GAN_L_ROUNDINGS[mode] + 1) * k * la.sum() + workgroups * 2.0 ** -41
    gk = grad_coeff / total
    return {"loss": (loss.reshape(1), ul.reshape(1)), "dpred": (gk * g, U * GAN_G_ROUNDINGS[mode] * abs(gk) * ga)}


def l1(a, b, coeff, grad0=None, workgroups=1):
    """vts_l1: "loss" = coeff * sum |a - b| (one rounding per term, K = n addends, 2^-41 per workgroup); "grad" (+)= coeff * sign(a - b):
    exact without accumulate (unit 0), one rounding with"""
    a, b = _f64(a).reshape(-1), _f64(b).reshape(-1)
    coeff = _f32(coeff)
    d = a - b
    loss = coeff * d.abs().sum()
    ul = U * (math.sqrt(d.numel()) + 1) * abs(coeff) * (a.abs() + b.abs()).sum() + workgroups * 2.0 ** -41
    g = coeff * torch.sign(d)
    ug = torch.zeros_like(g)
    if grad0 is not None:
        o = _f64(grad0).reshape(-1)
        g, ug = g + o, U * (o.abs() + abs(coeff) * torch.sign(d).abs())
    return {"loss": (loss.reshape(1), ul.reshape(1)), "grad": (g, ug)}


def _clamped(off, size, length):
    return (int(off) + torch.arange(size)).clamp(0, length - 1)


def patch_gather(src, img, offx, offy, size):
    """vts_patch_gather: out[p, c, y, x] = src[img[p], c, clamp(offy[p] + y, 0, H - 1), clamp(offx[p] + x, 0, W - 1)], in src's own dtype"""
    h, w = src.shape[-2:]
    out = [src[int(i)][:, _clamped(oy, size, h)[:, None], _clamped(ox, size, w)[None, :]] for i, ox, oy in zip(img, offx, offy)]
    return torch.stack(out, 0)


def patch_scatter_bwd(dpatch, offx, offy, ppi, n, h, w, dsrc0=None):
    """vts_patch_scatter_bwd, the adjoint of the gather: dsrc[i, c, Y, X] (+)= sum of dpatch[p, c, y, x] over the patches p of image i
    (p // ppi = i) and the (y, x) whose clamped source position is (Y, X).  K = addends of the element; K = 0: exactly 0 (or the seed)."""
    g = _f64(dpatch)
    P, c, size = g.shape[0], g.shape[1], g.shape[2]
    assert P == n * ppi
    ref, a, k = g.new_zeros(n, c, h * w), g.new_zeros(n, c, h * w), g.new_zeros(n, h * w)
    for p in range(P):
        idx = (_clamped(offy[p], size, h)[:, None] * w + _clamped(offx[p], size, w)[None, :]).reshape(-1)
        ref[p // ppi].index_add_(1, idx, g[p].reshape(c, -1))
        a[p // ppi].index_add_(1, idx, g[p].abs().reshape(c, -1))
        k[p // ppi].index_add_(0, idx, g.new_ones(idx.numel()))
    unit = U * torch.sqrt(k).unsqueeze(1) * a
    if dsrc0 is not None:
        o = _f64(dsrc0).reshape(n, c, h * w)
        ref, unit = ref + o, unit + U * (o.abs() + a) * (k > 0).unsqueeze(1)
    return {"dsrc": (ref.view(n, c, h, w), unit.view(n, c, h, w))}


def _bs(x, xa, rb, rs, m, r):
    """DiffAugment 'bs' times the mask on value x / magnitude xa [N, 3, HW]: ((x1 - mean) k + mean) m, x1 = x + (rb - 0.5), k = 2 rs"""
    n = x.shape[0]
    db, k = _f64(rb).view(n, 1, 1) - 0.5, 2 * _f64(rs).view(n, 1, 1)
    x1, a1 = x + db, xa + _f64(rb).abs().view(n, 1, 1) + 0.5
    mean, amean = x1.mean(1, keepdim=True), a1.mean(1, keepdim=True)
    return ((x1 - mean) * k + mean) * m, U * r * ((a1 + amean) * k.abs() + amean) * m.abs()


def g_post(g_out, M, scale_nz, rb=None, rs=None, S=None):
    """vts_g_post / vts_g_post_stack on g_out [N, 5, H, W], M [N, 1, H, W]:
      fake_I = g[:, :3] M, fake_T = g[:, 3:] M (1 rounding);  fake_N = (tx, ty, nz) / max(|(tx, ty, nz)|, 1e-12), nz = scale_nz (r = 7:
      the product with M, squares and adds through the root, the root, the division, the product);  aug_fake_I = bs(fake_I; rb, rs) M
      (r = 10: g M, rb - 0.5, the add, the 3-term mean and its division, subtract, scale, add, mask);  stack_S = S, stack_M = M (copies)."""
    g, m = _f64(g_out), _f64(M)
    n, _, h, w = g.shape
    g, m = g.reshape(n, 5, h * w), m.reshape(n, 1, h * w)
    nz = _f32(scale_nz)
    t = g * m
    out = {"fake_I": (t[:, :3], U * t[:, :3].abs()), "fake_T": (t[:, 3:], U * t[:, 3:].abs())}
    v = torch.cat([t[:, 3:], torch.full_like(t[:, :1], nz)], 1)
    nv = v / v.norm(dim=1, keepdim=True).clamp_min(1e-12)
    out["fake_N"] = (nv, 7 * U * nv.abs())
    if rb is not None:
        out["aug_fake_I"] = _bs(t[:, :3], t[:, :3].abs(), rb, rs, m, 10)
    out["stack_M"] = (m, torch.zeros_like(m))
    if S is not None:
        s = _f64(S).reshape(n, 1, h * w)
        out["stack_S"] = (s, torch.zeros_like(s))
    return out


def diffaug_bs_mask(x, M, rb, rs):
    """vts_diffaug_bs_mask: aug = bs(x; rb, rs) M on x [N, 3, H, W] (M None: no mask); r = 9"""
    x = _f64(x)
    n = x.shape[0]
    x = x.reshape(n, 3, -1)
    m = _f64(M).reshape(n, 1, -1) if M is not None else torch.ones_like(x[:, :1])
    return {"aug": _bs(x, x.abs(), rb, rs, m, 9)}


def diffaug_op(x, op, pf=None, pi0=None, pi1=None, noise=None, M=None):
    """vts_diffaug_op, one letter of b s c t o n on x [N, C, H, W], times M when given (one more rounding); see include/vts.h.
      b r = 2; s r = C + 3 (the channel mean: C - 1 adds and a division; subtract, scale, add); c r = 4 (pf + 0.5, subtract, scale, add)
      plus the mean over K = C H W elements, u (sqrt(K) + 1) mean|x|, through |k| + 1; t, o: copies and exact zeros; n r = 2"""
    x = _f64(x)
    n, c, h, w = x.shape
    m = _f64(M).view(n, 1, h, w) if M is not None else torch.ones_like(x[:, :1])
    rm = 1 if M is not None else 0
    col = lambda t: _f64(t).view(n, 1, 1, 1)
    xa = x.abs()
    if op == "b":
        ref, a, r = x + (col(pf) - 0.5), xa + col(pf).abs() + 0.5, 2
    elif op == "s":
        mean, amean, k = x.mean(1, keepdim=True), xa.mean(1, keepdim=True), 2 * col(pf)
        ref, a, r = (x - mean) * k + mean, (xa + amean) * k.abs() + amean, c + 3
    elif op == "c":
        mean, amean = x.mean((1, 2, 3), keepdim=True), xa.mean((1, 2, 3), keepdim=True)
        k, ka = col(pf) + 0.5, col(pf).abs() + 0.5
        ref, a, r = (x - mean) * k + mean, (xa + amean) * ka + amean, 4
        extra = U * (math.sqrt(c * h * w) + 1) * amean * (ka + 1)
        return {"out": (ref * m, (U * (r + rm) * a + extra) * m.abs())}
    elif op == "t":
        ref = torch.zeros_like(x)
        for i in range(n):
            ref[i] = _window(x[i], int(pi0[i]), int(pi1[i]), h, w)
        a, r = ref.abs(), 0
    elif op == "o":
        ch, cw = int(h * 0.5 + 0.5), int(w * 0.5 + 0.5)
        keep = torch.ones_like(x[:, :1])
        for i in range(n):
            r0, c0 = int(pi0[i]) - ch // 2, int(pi1[i]) - cw // 2
            rows = sorted(set(min(max(r0 + j, 0), h - 1) for j in range(ch)))
            cols = sorted(set(min(max(c0 + j, 0), w - 1) for j in range(cw)))
            keep[i, 0, rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1] = 0
        ref, a, r = x * keep, xa * keep, 0
    else:
        assert op == "n"
        z = _f64(noise)
        ref, a, r = x + col(pf) * z, xa + (col(pf) * z).abs(), 2
    return {"out": (ref * m, U * (r + rm) * a * m.abs())}


def g_out_grad(d_fake_I, d_fake_T, M, g_out, coarse=None):
    """vts_g_out_grad / vts_g_out_grad_pool: d_raw = cat(d_fake_I [+ pool adjoint of `coarse`], d_fake_T) M (1 - g_out^2); a NULL
    gradient is zero.  r = 4 (square, 1 - ., two products) on |up| |M| (1 + g^2); the pooled form adds the adjoint's unit and one add."""
    g, m = _f64(g_out), _f64(M)
    n, _, h, w = g.shape
    up, au, uu = g.new_zeros(n, 5, h, w), g.new_zeros(n, 5, h, w), g.new_zeros(n, 5, h, w)
    if d_fake_I is not None:
        up[:, :3], au[:, :3] = _f64(d_fake_I), _f64(d_fake_I).abs()
    if coarse is not None:
        adj, uadj = avgpool3s2_bwd(coarse, h, w)["dx"]
        aadj = _pool_adjoint(_f64(coarse).abs(), h, w)
        uu[:, :3] = uadj + U * (au[:, :3] + aadj)
        up[:, :3], au[:, :3] = up[:, :3] + adj, au[:, :3] + aadj
    if d_fake_T is not None:
        up[:, 3:], au[:, 3:] = _f64(d_fake_T), _f64(d_fake_T).abs()
    f, fa = m * (1 - g * g), m.abs() * (1 + g * g)
    return {"d_raw": (up * f, 4 * U * au * fa + uu * fa)}


def mask_mul(x, M):
    """vts_mask_mul: y = x M, one rounding"""
    y = _f64(x) * _f64(M)
    return {"y": (y, U * y.abs())}


def spe_grid(n, h, w, dim):
    """vts_spe_grid: out[n, d, y, x], e = d % dim, i = e % (dim / 2), pos = (d < dim ? x : y) + 1, a = pos exp(-i ln(1e4) / (dim / 2 - 1)),
    out = e < dim / 2 ? sin(a) : cos(a).  The unit carries the ARGUMENT: ln (2 roundings), division, the product with i and the
    exponential's own 2 act on t = i ln(1e4) / (half - 1) as a relative error 4 |t| + 2 of the frequency, the product with pos adds 1:
    unit = u (2 |out| + |a| (4 |t| + 3)), t = 0 (frequency exactly 1, a an exact integer): u 2 |out|."""
    half = dim // 2
    i = torch.arange(half, dtype=torch.float64)
    t = i * (math.log(10000.0) / (half - 1))
    f = torch.exp(-t)

    def axis(length):
        a = torch.arange(1, length + 1, dtype=torch.float64).view(1, -1) * f.view(-1, 1)          # [half, L]
        ua = a * (4 * t.view(-1, 1) + 3) * (t.view(-1, 1) > 0)
        v = torch.cat([torch.sin(a), torch.cos(a)], 0)
        return v, U * (2 * v.abs() + torch.cat([ua, ua], 0))
    xv, xu = axis(w)
    yv, yu = axis(h)
    ref = torch.cat([xv[:, None, :].expand(dim, h, w), yv[:, :, None].expand(dim, h, w)], 0)
    unit = torch.cat([xu[:, None, :].expand(dim, h, w), yu[:, :, None].expand(dim, h, w)], 0)
    return {"out": (ref[None].expand(n, 2 * dim, h, w).contiguous(), unit[None].expand(n, 2 * dim, h, w).contiguous())}


def adam_flat(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """vts_adam_flat / vts_adam_flat_dev, torch.optim.Adam's defaults on gr = g grad_scale:
      m' = beta1 m + (1 - beta1) gr (r = 4),  v' = beta2 v + (1 - beta2) gr^2 (r = 6),
      p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),  bc = 1 - beta^step.
    The units of m' and v' are propagated into p'; a bias correction is a power (2 roundings) and a subtraction on absref 1 + beta^step
    (near step 1 that is the cancellation an fp32 evaluation of 1 - beta^step has), the root, the quotient, + eps, the division, the
    product with the step size and the final subtraction one rounding each.  m' = 0 exactly (g = m = 0): p' = p exactly, unit 0."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    lr, b1, b2, eps, gs = _f32(lr), _f32(beta1), _f32(beta2), _f32(eps), _f32(grad_scale)
    gr = g * gs
    m1, ma = b1 * m + (1 - b1) * gr, (b1 * m).abs() + ((1 - b1) * gr).abs()
    v1 = b2 * v + (1 - b2) * gr * gr
    um, uv = 4 * U * ma, 6 * U * v1
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    rel1, rel2 = 3 * U * (1 + b1 ** step) / bc1, 3 * U * (1 + b2 ** step) / bc2
    ss = lr / bc1
    root = torch.sqrt(v1) / math.sqrt(bc2)
    denom = root + eps
    uden = root * (0.5 * 6 * U + 0.5 * rel2 + 3 * U) + U * denom
    upd, upda = ss * m1 / denom, abs(ss) * ma / denom
    uupd = abs(ss) * um / denom + upda * (uden / denom + rel1 + 3 * U)
    up = torch.where(ma > 0, uupd + U * (p.abs() + upda), torch.zeros_like(p))
    return {"p": (p - upd, up), "m": (m1, um), "v": (v1, uv)}


# ---- exact judges: data movement, byte staging, the sampler --------------------------------------------------------------------------------

def patch_jobs(jobs, size):
    """vts_patch_jobs: every job {dst_c0, C, P, and src (+ img, offx, offy: gather; without: copy of src [P, C, size, size]) or fill} as
    (dst_c0, block [P, C, size, size] float32)"""
    out = []
    for q in jobs:
        if q.get("src") is None:
            blk = torch.full((q["P"], q["C"], size, size), q["fill"], dtype=torch.float32)
        elif q.get("img") is None:
            blk = q["src"][:q["P"], :q["C"]].clone()
        else:
            blk = patch_gather(q["src"][:, :q["C"]], q["img"], q["offx"], q["offy"], size)
        out.append((q["dst_c0"], blk))
    return out


def pool_query(images, store, ret_slot, put_slot):
    """vts_pool_query: for n in order: out[n] = ret_slot[n] < 0 ? images[n] : store[ret_slot[n]], then store[put_slot[n]] = images[n]
    (put_slot[n] >= 0); returns (out, the store afterwards)"""
    store, out = store.clone(), torch.empty_like(images)
    for n in range(images.shape[0]):
        r, w = int(ret_slot[n]), int(put_slot[n])
        out[n] = images[n] if r < 0 else store[r]
        if w >= 0:
            store[w] = images[n]
    return out, store


def u8_expand(src, normalize):
    """vts_u8_expand: ToTensor [+ Normalize(0.5, 0.5)] in IEEE fp32: b / 255 [then (t - 0.5) / 0.5], correctly rounded each"""
    t = src.to(torch.float32) / torch.tensor(255.0)
    return (t - 0.5) / 0.5 if normalize else t


def input_images_u8(S, I, M):
    """vts_input_images_u8: (M_out, S_out, I_out) = (M / 255, expand(S) M_out, expand(I) M_out) in IEEE fp32 (M None: mask 1; I None: None)"""
    m = u8_expand(M, False) if M is not None else torch.ones(S.shape, dtype=torch.float32)
    return (m if M is not None else None), u8_expand(S, True) * m, (u8_expand(I, True) * m if I is not None else None)


def mask_candidates(M):
    """vts_mask_candidates: cand[n, y, x] = any(M[n, y - 1 .. y + 15, x - 1 .. x + 15] > 0) on the (H - 14) x (W - 14) grid (uint8) and
    prefix [n, H - 14 + 1] (int32): prefix[n, y] = candidates in the rows before y"""
    n, _, h, w = M.shape
    b = torch.nn.functional.pad((M > 0).to(torch.float64), (1, 1, 1, 1))
    cand = torch.nn.functional.max_pool2d(b, 17, 1).view(n, h - 14, w - 14).to(torch.uint8)
    prefix = torch.zeros(n, h - 14 + 1, dtype=torch.int32)
    prefix[:, 1:] = cand.sum(2, dtype=torch.int64).cumsum(1).to(torch.int32)
    return cand, prefix


def mask_select(cand, ranks):
    """vts_mask_select: (offx, offy) [N * K] int32 of the candidate with row-major rank ranks[n, k]"""
    n, k = ranks.shape
    offx, offy = torch.empty(n, k, dtype=torch.int32), torch.empty(n, k, dtype=torch.int32)
    for i in range(n):
        pos = torch.nonzero(cand[i])
        offy[i], offx[i] = pos[ranks[i], 0].to(torch.int32), pos[ranks[i], 1].to(torch.int32)
    return offx.reshape(-1), offy.reshape(-1)


_M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def mask_sample_ranks(counts, K, seed):
    """vts_mask_sample_ranks in Python integers: per image n with c candidates, Floyd's algorithm over j = c - K .. c - 1 with
    t = mulhi64(splitmix64(splitmix64(seed ^ n 0xD1B54A32D192ED03) + i), j + 1) for draw i, inserting t, or j if t is already drawn;
    c < K: ranks wrap (q % c, or 0 for an empty image).  int64 [N, K]"""
    out = torch.empty(len(counts), K, dtype=torch.int64)
    for n, c in enumerate(int(v) for v in counts):
        if c < K:
            out[n] = torch.tensor([q % c if c > 0 else 0 for q in range(K)])
            continue
        base = splitmix64((seed & _M64) ^ ((n * 0xD1B54A32D192ED03) & _M64))
        seen, order = set(), []
        for i in range(K):
            j = c - K + i
            t = (splitmix64((base + i) & _M64) * (j + 1)) >> 64
            pick = j if t in seen else t
            seen.add(pick)
            order.append(pick)
        out[n] = torch.tensor(order)
    return out


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


# ---- padding, resampling and FIR operators (csrc/vts_resample.hip, the upfirdn2d / bias_act entries of csrc/vts_stylegan2.hip, the nearest /
# tanh_bwd entries of csrc/vts_spade.hip) -------------------------------------------------------------------------------------------------
# Units here are derived worst-case rounding counts with nothing measured in them: unit = (r + K) u absref, K = the products summed into
# the element, r = the other roundings of the formula (an affine fmaf one, an activation slope one, a gain one, a residual or accumulate
# add one each), absref = the same expression with every term in absolute value.  Every term of a K-term fp32 sum passes through at most
# K roundings (its product and K - 1 adds), so a correct one-pass kernel stays within 1 unit to first order in u, in any summation
# order; the tests allow 1.01 for the second-order terms.  The one exception is tanh, whose error depends on the device's tanhf: see TANH_E.
SLOPE32 = {0: None, 1: float(torch.tensor(0.2, dtype=torch.float32)), 2: 0.0}      # the slope as the fp32 constant the formula carries

# worst |torch.tanh(x) - tanh(x)| / (u |tanh(x)|) of PyTorch's own device kernel on the MI355X over 8.4e6 fp32 arguments in [-12, 12]
# (2.4593, at x = -0.64956; 1.26 for |x| >= 1, 1.02 below 0.1).  The bound allows twice that plus one ulp (<= 2 u |ref|): the library's
# tanhf and PyTorch's kernel may take different paths.
TANH_E_MEASURED = 2.4593
TANH_E = 2 * TANH_E_MEASURED + 2


def affine_act(x, scale, shift, act):
    """(value, absvalue, roundings) elementwise of act(fmaf(x, scale, shift)), x [N, C, H, W], scale / shift [N, C] or both None.
    Roundings: the fmaf 1 (0 without an affine), the LeakyReLU slope 1 where the value is negative (ReLU and the positive side are exact).
    act 3 (tanh): value tanh(t) and roundings = None; the caller adds tanh_unit()."""
    x = _f64(x)
    n, c = x.shape[:2]
    a, r = x.abs(), torch.zeros_like(x)
    if scale is not None:
        s, b = _f64(scale).view(n, c, 1, 1), _f64(shift).view(n, c, 1, 1)
        x, a, r = x * s + b, a * s.abs() + b.abs(), r + 1
    if act == 3:
        return torch.tanh(x), a, None
    slope = SLOPE32[act]
    if slope is not None:
        neg = ~(x > 0)
        f = torch.where(neg, torch.full_like(x, slope), torch.ones_like(x))
        x, a = x * f, a * f
        if slope != 0.0:
            r = r + neg.to(r.dtype)
    return x, a, r


def tanh_unit(t_abs, affine, ref):
    """error scale of tanhf(fmaf(x, a, b)): the propagated rounding of the argument, u |t| (1 - ref^2) (absent without an affine), plus
    TANH_E u |ref| for the function itself"""
    return (U * t_abs * (1 - ref * ref) if affine else 0.0) + TANH_E * U * ref.abs()


def pad_index(size, lo, hi, mode):
    """source index of every position of an axis padded by (lo, hi): mode 0 zero (-1), 1 reflect (no edge repeat), 2 replicate"""
    t = torch.arange(-lo, size + hi)
    if mode == 1:
        assert lo < size and hi < size
        s = torch.where(t < 0, -t, torch.where(t >= size, 2 * size - 2 - t, t))
    elif mode == 2:
        s = t.clamp(0, size - 1)
    else:
        s = torch.where((t < 0) | (t >= size), torch.full_like(t, -1), t)
    return s


def _gather2(x, sy, sx):
    """x[..., sy, sx] with zeros where an index is -1"""
    v = x[..., sy.clamp_min(0), :][..., sx.clamp_min(0)]
    keep = ((sy >= 0)[:, None] & (sx >= 0)[None, :]).to(x.dtype)
    return v * keep


def _scatter2(g, sy, sx, h, w):
    """adjoint of _gather2: out[..., sy[i], sx[j]] += g[..., i, j]"""
    g = g * ((sy >= 0)[:, None] & (sx >= 0)[None, :]).to(g.dtype)
    rows = g.new_zeros(g.shape[:-2] + (h, g.shape[-1])).index_add_(-2, sy.clamp_min(0), g)
    return g.new_zeros(g.shape[:-2] + (h, w)).index_add_(-1, sx.clamp_min(0), rows)


def pad_affine(x, scale, shift, pads, mode, act, res=None):
    """vts_pad_affine: out = pad(act(x * scale + shift)) (+ res); pads (top, bottom, left, right); the zero mode pads with 0 (not act(shift)).
    No sum: K = 0; r = affine + slope (+ 1 for the residual add)."""
    pt, pb, pl, pr = pads
    h, w = x.shape[-2:]
    v, a, r = affine_act(x, scale, shift, act)
    sy, sx = pad_index(h, pt, pb, mode), pad_index(w, pl, pr, mode)
    ref, aa = _gather2(v, sy, sx), _gather2(a, sy, sx)
    if act == 3:
        unit, aa = _gather2(tanh_unit(a, scale is not None, v), sy, sx), ref.abs()
    else:
        unit = U * _gather2(r, sy, sx) * aa
    if res is not None:                                  # one more rounding, of the sum
        o = _f64(res)
        unit = unit + U * (aa + o.abs()) if act == 3 else U * (_gather2(r, sy, sx) + 1) * (aa + o.abs())
        ref = ref + o
    return {"out": (ref, unit)}


def _sum_unit(cnt, a, o):
    """unit of a sum of cnt plain addends (cnt - 1 roundings) with absolute sum a, accumulated onto o (one more) or not (o None)"""
    if o is None:
        return U * (cnt - 1).clamp_min(0) * a
    return U * cnt * (a + o.abs())


def pad_bwd(dpad, hw, pads, mode, din0=None):
    """vts_pad_bwd: din (+)= the adjoint of the padding's index map applied to dpad: every source pixel sums the padded positions that read it"""
    h, w = hw
    pt, pb, pl, pr = pads
    g = _f64(dpad)
    sy, sx = pad_index(h, pt, pb, mode), pad_index(w, pl, pr, mode)
    ref, a = _scatter2(g, sy, sx, h, w), _scatter2(g.abs(), sy, sx, h, w)
    cnt = _scatter2(torch.ones(g.shape[-2:], dtype=torch.float64), sy, sx, h, w)
    o = _f64(din0)
    return {"din": (ref if o is None else ref + o, _sum_unit(cnt, a, o))}


def _axis_down(size):
    """(taps, paths) [OH, H] of one axis of Downsample: reflect pad 1, [1 2 1] / 4, stride 2"""
    o = (size - 1) // 2 + 1
    src = pad_index(size, 1, 1, 1)                  # positions -1 .. size
    A, P = torch.zeros(o, size, dtype=torch.float64), torch.zeros(o, size, dtype=torch.float64)
    for y in range(o):
        for i, f in enumerate((0.25, 0.5, 0.25)):
            s = int(src[2 * y + i])
            A[y, s] += f
            P[y, s] += 1
    return A, P


def _axis_up(size):
    """(taps, paths) [2 H, H] of one axis of Upsample: out[y] = sum_u P[u] f[y + 3 - 2 u], P = replicate pad 1, f = [1 3 3 1] / 4"""
    f = (0.25, 0.75, 0.75, 0.25)
    A, P = torch.zeros(2 * size, size, dtype=torch.float64), torch.zeros(2 * size, size, dtype=torch.float64)
    for y in range(2 * size):
        for u in range(size + 2):
            k = y + 3 - 2 * u
            if 0 <= k <= 3:
                s = min(max(u - 1, 0), size - 1)
                A[y, s] += f[k]
                P[y, s] += 1
    return A, P


def _sep(Ay, Ax, x):
    return torch.einsum("oh,nchw,pw->ncop", Ay, x, Ax)


def _blur(axis, x, scale, shift, act, K):
    assert act != 3
    v, a, r = affine_act(x, scale, shift, act)
    h, w = v.shape[-2:]
    (Ay, _), (Ax, _) = axis(h), axis(w)
    return {"out": (_sep(Ay, Ax, v), U * (float(r.max()) + K) * _sep(Ay, Ax, a))}


def _blur_bwd(axis, dout, hw, din0):
    g = _f64(dout)
    (Ay, Py), (Ax, Px) = axis(hw[0]), axis(hw[1])
    ref, a = _sep(Ay.t(), Ax.t(), g), _sep(Ay.t(), Ax.t(), g.abs())
    K = Py.sum(0)[:, None] * Px.sum(0)[None, :]              # products summed into the element (paths, before the reflection folds them)
    o = _f64(din0)
    if o is None:
        return {"din": (ref, U * K * a)}
    return {"din": (ref + o, U * (K + 1) * (a + o.abs()))}


def blur_down(x, scale=None, shift=None, act=0):
    """vts_blur_down: reflect pad 1, depthwise [1 2 1] x [1 2 1] / 16, stride 2, of act(x * scale + shift): K = 9 products"""
    return _blur(_axis_down, x, scale, shift, act, 9)


def blur_down_bwd(dout, hw, din0=None):
    return _blur_bwd(_axis_down, dout, hw, din0)


def blur_up(x, scale=None, shift=None, act=0):
    """vts_blur_up: replicate pad 1, depthwise transposed [1 3 3 1] x [1 3 3 1] * 4 / 64, stride 2, cropped to 2H x 2W: K = 4 products"""
    return _blur(_axis_up, x, scale, shift, act, 4)


def blur_up_bwd(dout, hw, din0=None):
    return _blur_bwd(_axis_up, dout, hw, din0)


def tap_embed(w, K, oy, ox):
    """vts_tap_embed(_at): w4[r, i, j] = w[r, oy + i, ox + j] inside the K x K grid, 0 outside (exact: compare bitwise).  -> [rows, 4, 4]"""
    w = w.reshape(-1, K, K)
    out = torch.zeros(w.shape[0], 4, 4, dtype=w.dtype)
    for i in range(4):
        for j in range(4):
            if 0 <= oy + i < K and 0 <= ox + j < K:
                out[:, i, j] = w[:, oy + i, ox + j]
    return out


def tap_extract(dw4, K, oy, ox, dw0=None):
    """vts_tap_extract(_at): dw[r, oy + i, ox + j] (+)= dw4[r, i, j] inside the K x K grid -> (ref [rows, K, K] with zeros (dw0 given: dw0)
    outside the block, unit, bool mask [K, K] of the elements the call owns)"""
    g = _f64(dw4).reshape(-1, 4, 4)
    ref = torch.zeros(g.shape[0], K, K, dtype=torch.float64) if dw0 is None else _f64(dw0).reshape(-1, K, K).clone()
    unit, own = torch.zeros_like(ref), torch.zeros(K, K, dtype=torch.bool)
    for i in range(4):
        for j in range(4):
            ky, kx = oy + i, ox + j
            if 0 <= ky < K and 0 <= kx < K:
                own[ky, kx] = True
                if dw0 is not None:
                    unit[:, ky, kx] = U * (ref[:, ky, kx].abs() + g[:, i, j].abs())
                    ref[:, ky, kx] += g[:, i, j]
                else:
                    ref[:, ky, kx] = g[:, i, j]
    return {"dw": (ref, unit), "own": own}


def table_matrix(mins, sizes, w, n_in):
    """the table of one axis (first index, window length, weights [n_out, K]) as a dense [n_out, n_in] float64 matrix"""
    mins, sizes, w = [torch.as_tensor(t) for t in (mins, sizes, w)]
    m = torch.zeros(len(mins), n_in, dtype=torch.float64)
    for o in range(len(mins)):
        lo, k = int(mins[o]), int(sizes[o])
        m[o, lo:lo + k] = w[o, :k].double()
    return m


def resample_table(x, ytab, xtab, out0=None):
    """vts_resample_table: out[y, x] (+)= sum_j wy[y][j] sum_i wx[x][i] in[ymin[y] + j][xmin[x] + i], the given tables applied in float64.
    K = ysize[y] * xsize[x] products; r = 1 for the row sum's own rounding on its way into the column sum (+ 1 for the accumulate)"""
    x = _f64(x)
    Wy, Wx = table_matrix(*ytab, x.shape[-2]), table_matrix(*xtab, x.shape[-1])
    ref, a = _sep(Wy, Wx, x), _sep(Wy.abs(), Wx.abs(), x.abs())
    K = torch.as_tensor(ytab[1]).double()[:, None] * torch.as_tensor(xtab[1]).double()[None, :]
    o = _f64(out0)
    if o is None:
        return {"out": (ref, U * (K + 1) * a)}
    return {"out": (ref + o, U * (K + 2) * (a + o.abs()))}


def _ufd_axis(size, k, up, down, p0, p1):
    """[k taps][n_out, size] 0 / 1 selection of one axis of upfirdn2d: tap t of output o reads position o * down + t - p0 of the
    zero-inserted signal (sample i at i * up, length size * up), padded by (p0, p1) (negative: cropped)"""
    n_out = (size * up + p0 + p1 - k) // down + 1
    assert size * up + p0 + p1 >= k and n_out >= 1
    S = torch.zeros(k, n_out, size, dtype=torch.float64)
    for t in range(k):
        for o in range(n_out):
            pos = o * down + t - p0
            if 0 <= pos < size * up and pos % up == 0:
                S[t, o, pos // up] = 1
    return S


def upfirdn2d(x, kernel, up=1, down=1, padx=(0, 0), pady=(0, 0), out0=None):
    """vts_upfirdn2d: zero-insertion upsampling by `up`, padding (negative = crop) per axis, correlation with the flipped kernel,
    decimation by `down`.  K = the taps that meet a sample (not a padding or inserted zero)"""
    x = _f64(x)
    kf = torch.flip(_f64(kernel), [0, 1])
    Sy, Sx = _ufd_axis(x.shape[-2], kf.shape[0], up, down, *pady), _ufd_axis(x.shape[-1], kf.shape[1], up, down, *padx)
    ref = torch.einsum("ab,aoh,nchw,bpw->ncop", kf, Sy, x, Sx)
    a = torch.einsum("ab,aoh,nchw,bpw->ncop", kf.abs(), Sy, x.abs(), Sx)
    K = torch.einsum("aoh,bpw->op", Sy, Sx)
    o = _f64(out0)
    if o is None:
        return {"out": (ref, U * K * a)}
    return {"out": (ref + o, U * (K + 1) * (a + o.abs()))}


def upfirdn2d_bwd(dout, hw, kernel, up=1, down=1, padx=(0, 0), pady=(0, 0), din0=None):
    """vts_upfirdn2d_bwd: din (+)= the adjoint of upfirdn2d (input size hw) applied to dout"""
    g = _f64(dout)
    kf = torch.flip(_f64(kernel), [0, 1])
    Sy, Sx = _ufd_axis(hw[0], kf.shape[0], up, down, *pady), _ufd_axis(hw[1], kf.shape[1], up, down, *padx)
    assert g.shape[-2:] == (Sy.shape[1], Sx.shape[1])
    ref = torch.einsum("ab,aoh,ncop,bpw->nchw", kf, Sy, g, Sx)
    a = torch.einsum("ab,aoh,ncop,bpw->nchw", kf.abs(), Sy, g.abs(), Sx)
    K = torch.einsum("aoh,bpw->hw", Sy, Sx)
    o = _f64(din0)
    if o is None:
        return {"din": (ref, U * K * a)}
    return {"din": (ref + o, U * (K + 1) * (a + o.abs()))}


def _bias_v(x, bias):
    x = _f64(x)
    n, c = x.shape[:2]
    shape = (1, c) + (1,) * (x.dim() - 2)
    if bias is None:
        return x, x.abs(), 0
    b = _f64(bias).reshape(shape)
    return x + b, x.abs() + b.abs(), 1


def bias_act(x, bias, res, slope, gain):
    """vts_bias_act: out = lrelu(x + bias, slope) * gain (+ res).  r: the bias add 1, the slope 1 where x + bias <= 0 (a slope of 0 is
    exact), the gain 1 (a gain of 1 is exact), the residual add 1.  x + bias == 0 gives exactly 0 (+ res)."""
    slope, gain = _f32(slope), _f32(gain)
    v, a, r = _bias_v(x, bias)
    neg = ~(v > 0)
    f = torch.where(neg, torch.full_like(v, slope), torch.ones_like(v)) * gain
    r = r + (neg.double() if slope != 0.0 else 0.0) + (1 if gain != 1.0 else 0)
    ref, a = v * f, a * f.abs()
    if res is not None:
        o = _f64(res)
        ref, a, r = ref + o, a + o.abs(), r + 1
    return {"out": (ref, U * r * a)}


def bias_act_bwd(g, x, bias, slope, gain):
    """vts_bias_act_bwd: dx = g * gain * (x + bias > 0 ? 1 : slope): the gain 1, the slope 1 on its branch (x + bias == 0 takes it)"""
    slope, gain = _f32(slope), _f32(gain)
    v, _, _ = _bias_v(x, bias)
    g = _f64(g)
    neg = ~(v > 0)
    f = torch.where(neg, torch.full_like(v, slope), torch.ones_like(v)) * gain
    r = (1 if gain != 1.0 else 0) + (neg.double() if slope != 0.0 else 0.0)
    return {"dx": (g * f, U * r * (g * f).abs())}


def nearest_index(n_in, n_out):
    """source index of every output position under F.interpolate(mode="nearest") on the CPU (ATen's float rule) -> int64 [n_out]"""
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    return torch.nn.functional.interpolate(src, size=(n_out, 1), mode="nearest").view(n_out).long()


def nearest_resize(x, size):
    """vts_nearest_resize: a gather (exact: compare bitwise) -> the resized tensor in x's dtype"""
    iy, ix = nearest_index(x.shape[-2], size[0]), nearest_index(x.shape[-1], size[1])
    return x[..., iy, :][..., ix]


def nearest_resize_bwd(dout, hw, din0=None):
    """vts_nearest_resize_bwd: din (+)= the sum of the outputs that read the pixel (none: exactly 0)"""
    g = _f64(dout)
    iy, ix = nearest_index(hw[0], g.shape[-2]), nearest_index(hw[1], g.shape[-1])
    ref, a = _scatter2(g, iy, ix, *hw), _scatter2(g.abs(), iy, ix, *hw)
    cnt = _scatter2(torch.ones(g.shape[-2:], dtype=torch.float64), iy, ix, *hw)
    o = _f64(din0)
    return {"din": (ref if o is None else ref + o, _sum_unit(cnt, a, o))}


def nearest_up2(x):
    """vts_nearest_up2: every pixel written to its 2 x 2 cell (exact) -> in x's dtype"""
    return x.repeat_interleave(2, -2).repeat_interleave(2, -1)


def nearest_up2_bwd(dout, din0=None):
    """vts_nearest_up2_bwd: din (+)= the sum of the 2 x 2 cell: 3 roundings (+ 1)"""
    g = _f64(dout)
    cell = lambda t: t[..., 0::2, 0::2] + t[..., 0::2, 1::2] + t[..., 1::2, 0::2] + t[..., 1::2, 1::2]
    ref, a = cell(g), cell(g.abs())
    o = _f64(din0)
    if o is None:
        return {"din": (ref, 3 * U * a)}
    return {"din": (ref + o, 4 * U * (a + o.abs()))}


def tanh_bwd(g, y):
    """vts_tanh_bwd: dz = g (1 - y^2): the square, the subtraction, the product: 3 roundings of |g| (1 + y^2)"""
    g, y = _f64(g), _f64(y)
    return {"dz": (g * (1 - y * y), 3 * U * g.abs() * (1 + y * y))}


# ---- the fp32 glue of the perceptual terms (csrc/vts_perceptual.hip, vts_zero_border) ---------------------------------------------------------
# Written from the formulas of include/vts.h.  Operands are passed DENSE (the interior of a zpad-padded tensor; the test lays them out).
# Data movement, masks and single maxima are bitwise (unit None, the reference already in its final fp32 value, +0.0 for every zero).  The
# arithmetic outputs carry the derived unit of the section above, (r + K) u absref.  Loss slots are judged as (slot - start) / 2^40 against
# the any-order bound of a K-term fp32 sum, (K - 1) u sum |terms|, plus the per-term roundings and 2^-41 for each workgroup's rounding to
# fixed point; rows whose addends sum exactly in fp32 (operands on a dyadic grid) carry the fixed-point rounding alone.

def _zpad(t, pad):
    return torch.nn.functional.pad(t, (pad, pad, pad, pad)) + 0.0


def maxpool2_relu_pad(z, pad):
    """vts_maxpool2_relu_pad: out [NC, H/2 + 2 pad, W/2 + 2 pad] = zero-padded MaxPool2d(2, 2)(relu(z)), z [NC, H, W]; an odd last row /
    column belongs to no window.  A maximum of four inputs and 0: bitwise."""
    z = _f64(z)
    return {"out": (_zpad(torch.nn.functional.max_pool2d(z.clamp_min(0.0).unsqueeze(0), 2, 2)[0], pad), None)}


def maxpool3s2_relu_pad(z, pad):
    """vts_maxpool3s2_relu_pad: the 3 x 3 window at (2 y, 2 x) of relu(z), OH = (H - 3) / 2 + 1, zero border of `pad`: bitwise"""
    z = _f64(z)
    return {"out": (_zpad(torch.nn.functional.max_pool2d(z.clamp_min(0.0).unsqueeze(0), 3, 2)[0], pad), None)}


def s2d4_pad(x, pad, oh, ow):
    """vts_s2d4_pad: out[n, (c * 4 + i) * 4 + j, Y, X] = xp[n, c, 4 Y + i, 4 X + j], xp = x zero-padded by `pad` and zero beyond: bitwise"""
    x = _f64(x)
    n, c, h, w = x.shape
    xp = x.new_zeros(n, c, 4 * oh, 4 * ow)
    hh, ww = max(min(h, 4 * oh - pad), 0), max(min(w, 4 * ow - pad), 0)
    xp[:, :, pad:pad + hh, pad:pad + ww] = x[:, :, :hh, :ww]
    return {"out": (xp.view(n, c, oh, 4, ow, 4).permute(0, 1, 3, 5, 2, 4).reshape(n, 16 * c, oh, ow) + 0.0, None)}


def vgg_stack_input(fake_I, real_I, fake_T, real_T):
    """vts_vgg_stack_input: out [6 N, 3, H + 2, W + 2], zero border, row groups fake_I, fake_gx x 3, fake_gy x 3, real_I, real_gx x 3,
    real_gy x 3 (gx, gy = channels 0, 1 of the tactile tensors): bitwise"""
    rows = []
    for img, tac in ((fake_I, fake_T), (real_I, real_T)):
        img, tac = _f64(img), _f64(tac)
        rows += [img[:, :3], tac[:, 0:1].expand(-1, 3, -1, -1), tac[:, 1:2].expand(-1, 3, -1, -1)]
    return {"out": (_zpad(torch.cat(rows, 0), 1), None)}


def zero_border(buf, pad):
    """vts_zero_border: buf [NC, H + 2 pad, W + 2 pad], the border of `pad` pixels <- 0.  Returns the whole buffer after the call and
    "own", the mask [H + 2 pad, W + 2 pad] of the border (the interior is not the call's: it comes back bitwise)."""
    ref = _f64(buf).clone()
    own = torch.ones(ref.shape[-2:], dtype=torch.bool)
    own[pad:-pad, pad:-pad] = False
    ref[..., own] = 0.0
    return {"buf": (ref, None), "own": own}


def relu_mask_pad(g, g2, z, pad):
    """vts_relu_mask_pad: out = zero-padded (g + g2) where z > 0, else 0; g or g2 may be None.  One fp32 add: exact for operands on a
    common dyadic grid (the test's), then the float64 value is the fp32 result: bitwise"""
    z = _f64(z)
    t = torch.zeros_like(z)
    for a in (g, g2):
        if a is not None:
            t = t + _f64(a)
    return {"out": (_zpad(torch.where(z > 0, t, torch.zeros_like(t)), pad), None)}


def maxpool2_relu_bwd(g, z, g2, pad):
    """vts_maxpool2_relu_bwd: gz [NC, H + 2 pad, W + 2 pad] = zero-padded (g [NC, H/2, W/2] routed to the FIRST element, in row-major order
    of the 2 x 2 window, that holds the window's maximum -- only where that maximum is positive -- plus g2 where z > 0).  Elements of an
    odd last row / column get the tap alone.  One add of two operands on a dyadic grid: bitwise."""
    g, z = _f64(g), _f64(z)
    nc, h, w = z.shape
    oh, ow = h // 2, w // 2
    e = z[:, :2 * oh, :2 * ow].reshape(nc, oh, 2, ow, 2).permute(0, 1, 3, 2, 4).reshape(nc, oh, ow, 4)
    m = e.max(-1).values
    first = torch.full(m.shape, 3, dtype=torch.int64)
    for k in (2, 1, 0):
        first = torch.where(e[..., k] == m, torch.full_like(first, k), first)
    route = torch.zeros_like(e)
    route.scatter_(-1, first.unsqueeze(-1), torch.where(m > 0, g, torch.zeros_like(g)).unsqueeze(-1))
    out = torch.zeros_like(z)
    out[:, :2 * oh, :2 * ow] = route.reshape(nc, oh, ow, 2, 2).permute(0, 1, 3, 2, 4).reshape(nc, 2 * oh, 2 * ow)
    if g2 is not None:
        out = out + torch.where(z > 0, _f64(g2), torch.zeros_like(z))
    return {"gz": (_zpad(out, pad), None)}


def l1_relu(za, zb, coeff, workgroups, exact_sum=False):
    """vts_l1_relu: "loss" = coeff * sum |relu(za) - relu(zb)|, "grad" = coeff * sign(.) (bitwise: +-coeff or 0).  The loss: one rounding
    per term (the subtraction; relu and |.| are exact) and K = n addends in any order: K u coeff sum |d| + workgroups 2^-41.  exact_sum
    (operands on a 2^-6 grid: every partial sum is exact in fp32): the fixed-point rounding alone."""
    coeff = _f32(coeff)
    d = _f64(za).reshape(-1).clamp_min(0.0) - _f64(zb).reshape(-1).clamp_min(0.0)
    unit = workgroups * 2.0 ** -41 + (0.0 if exact_sum else U * d.numel() * abs(coeff) * d.abs().sum())
    return {"loss": ((coeff * d.abs().sum()).reshape(1), torch.as_tensor(unit, dtype=torch.float64).reshape(1)),
            "grad": (coeff * torch.sign(d) + 0.0, None)}


def lpips_input(x, shift3, scale3):
    """vts_lpips_input: y [N, 3, HW] = (x - shift_c) / scale_c, x [N, 1 | 3, HW] (one channel: broadcast).  Three roundings: the host's
    fp32 reciprocal 1 / scale, the host's quotient -shift / scale, the fmaf: unit = 3 u (|x| + |shift|) / |scale|"""
    x = _f64(x)
    sh = torch.tensor([_f32(v) for v in shift3], dtype=torch.float64).view(1, 3, 1)
    sc = torch.tensor([_f32(v) for v in scale3], dtype=torch.float64).view(1, 3, 1)
    x = x.expand(-1, 3, -1)
    return {"y": ((x - sh) / sc, 3 * U * (x.abs() + sh.abs()) / sc.abs())}


def lpips_input_bwd(g, scale3, cx, dx0=None):
    """vts_lpips_input_bwd: dx [N, Cx, HW] (+)= g_c / scale_c (Cx = 3), sum_c g_c / scale_c (Cx = 1), g [N, 3, HW].  Roundings: the host's
    fp32 reciprocal and the product on every term (2: the reciprocal counts here as it does in vts_lpips_input), two adds for the sum of
    three (4), one more with accumulate."""
    g = _f64(g)
    sc = torch.tensor([_f32(v) for v in scale3], dtype=torch.float64).view(1, 3, 1)
    ref, a, r = g / sc, g.abs() / sc.abs(), 2
    if cx == 1:
        ref, a, r = ref.sum(1, keepdim=True), a.sum(1, keepdim=True), 4
    if dx0 is not None:
        o = _f64(dx0)
        ref, a, r = ref + o, a + o.abs(), r + 1
    return {"dx": (ref, r * U * a)}


def vgg_stack_input_bwd(dx, n, dI0=None, dT0=None):
    """vts_vgg_stack_input_bwd: dx [3 N, 3, HW] -> "dI" [N, 3, HW] (+)= dx[0:N] (a copy: unit 0; one rounding with accumulate),
    "dT" [N, 2, HW] (+)= (dx[(1 + c) N + n, 0] + dx[.., 1]) + dx[.., 2] (two roundings; three with accumulate)"""
    dx = _f64(dx)
    dI, aI, rI = dx[:n], dx[:n].abs(), 0
    t = torch.stack([dx[n:2 * n], dx[2 * n:3 * n]], 1)              # [N, 2, 3, HW]
    dT, aT, rT = t.sum(2), t.abs().sum(2), 2
    if dI0 is not None:
        oI, oT = _f64(dI0), _f64(dT0)
        dI, aI, rI, dT, aT, rT = dI + oI, aI + oI.abs(), 1, dT + oT, aT + oT.abs(), 3
    return {"dI": (dI, rI * U * aI), "dT": (dT, rT * U * aT)}


def lpips_layer_judge(f0, f1, w, coeff, grad_coeff, workgroups=None, raw=False, addends=None):
    """f0, f1 [N, C, H, W] >= 0 (float64), w [C].  Returns value (float64 scalar: what the call adds to the slot), its bound,
    dz0 [N, C, H, W] and its fp32 bound (vts_lpips_layer_bf16: bf16-exact operands, and the bf16 store adds 2^-8 |dz0|).
    workgroups: of the fixed-point term (None: the bf16 head's, one per 32 pixels of the padded map); raw: f0 / f1 are raw convolution
    outputs z (vts_lpips_layer with zpad = 0): ReLU on load, gradient exactly 0 where z0 <= 0; addends: the number K of pixel terms the
    slot value sums, for the any-order bound (K - 1) u (None: the bf16 head's 26, below).

    The unit is a derived linear rounding count ((r + K) u absref): nothing in it is measured.
      s = sum_c f^2 (C positive terms, any order)          relative error <= C u
      r = sqrt(s), r + eps, i = 1 / (r + eps)               rho = C / 2 + 3 roundings on i (sqrt, add, divide: one each, correctly rounded)
      t_c = f0_c i0 - f1_c i1                               |dt_c| <= (rho + 2) u A_c, A_c = f0_c i0 + f1_c i1 (two products, one subtraction)
      d = sum_c w_c t_c^2                                   |dd| <= u sum_c w_c (2 (rho + 2) A_c |t_c| + (2 + C) t_c^2)
      value = coeff / HW sum_pixels d                       + 26 u per term for the thread / wave / workgroup sums (<= 16 + 6 + 4 additions on any term's path)
                                                            + 2^-41 per workgroup (its rounding to the fixed-point slot)
      S = sum_c w_c t_c f0_c                                E_S = u sum_c w_c f0_c ((rho + 2) A_c + (2 + C) |t_c|)
      k1 = 2 g / HW i0                                      rho + 3 roundings
      k2 = 2 g / HW S i0^2 / r0                             |dk2| <= |2 g / HW| i0^2 / r0 (E_S + |S| u (2 rho + C / 2 + 6))
      dz0_c = k1 w_c t_c - k2 f0_c where f0_c > 0           u |k1| w_c ((rho + 5) |t_c| + (rho + 2) A_c) + f0_c (|dk2| + u |k2|) + u |dz0_c|"""
    if raw:
        f0, f1 = f0.clamp_min(0.0), f1.clamp_min(0.0)
    n, c, h, wd = f0.shape
    hw = h * wd
    wv = w.view(1, -1, 1, 1).double()
    eps = 1e-10
    r0, r1 = f0.pow(2).sum(1, keepdim=True).sqrt(), f1.pow(2).sum(1, keepdim=True).sqrt()
    i0, i1 = 1.0 / (r0 + eps), 1.0 / (r1 + eps)
    t = f0 * i0 - f1 * i1
    A = f0 * i0 + f1 * i1
    rho = c / 2 + 3
    d = (wv * t * t).sum(1)
    dd = U * (wv * (2 * (rho + 2) * A * t.abs() + (2 + c) * t * t)).sum(1)
    value = coeff / hw * d.sum()
    if workgroups is None:
        workgroups = n * (((h + 2) * (wd + 2) + 31) // 32)
    vbound = abs(coeff) / hw * (dd.sum() + (26 if addends is None else addends - 1) * U * d.sum()) + workgroups * 2.0 ** -41
    S = (wv * t * f0).sum(1, keepdim=True)
    ES = U * (wv * f0 * ((rho + 2) * A + (2 + c) * t.abs())).sum(1, keepdim=True)
    g2 = 2.0 * grad_coeff / hw
    k1 = g2 * i0
    safe_r0 = torch.where(r0 > 0, r0, torch.ones_like(r0))
    k2 = torch.where(r0 > 0, g2 * S * i0 * i0 / safe_r0, torch.zeros_like(r0))
    dk2 = torch.where(r0 > 0, abs(g2) * i0 * i0 / safe_r0 * (ES + S.abs() * U * (2 * rho + c / 2 + 6)), torch.zeros_like(r0))
    live = f0 > 0
    dz = torch.where(live, k1 * wv * t - k2 * f0, torch.zeros_like(f0))
    bound = U * k1.abs() * wv * ((rho + 5) * t.abs() + (rho + 2) * A) + f0 * (dk2 + U * k2.abs()) + U * dz.abs()
    bound = torch.where(live, bound, torch.zeros_like(bound))
    return value, vbound, dz, bound


def lpips_layer(z0, z1, w, coeff, grad_coeff, workgroups, raw, exact_sum=False):
    """vts_lpips_layer (fp32): "loss" = coeff sum_n mean_pixels sum_c w_c (f0n - f1n)^2, "dz0" = grad_coeff d(that sum) / d z0, through
    lpips_layer_judge with K = N HW addends.  workgroups: N ceil(HW / 64) for the register kernels, N min(ceil(HW / 256), 2048) for the
    generic one.  exact_sum (one-hot pixels of value 1.0, dyadic w: r = 1, 1 / (1 + 1e-10) = 1 in fp32, every d dyadic): the loss unit is
    the fixed-point rounding alone (eps itself moves the float64 value by 2e-10 of it: below 1 % of that unit for |value| <= 0.04 N)."""
    z0, z1 = _f64(z0), _f64(z1)
    n, _, h, wd = z0.shape
    value, vbound, dz, bound = lpips_layer_judge(z0, z1, _f64(w), _f32(coeff), _f32(grad_coeff), workgroups=workgroups, raw=raw, addends=n * h * wd)
    if exact_sum:
        vbound = workgroups * 2.0 ** -41
    return {"loss": (value.reshape(1), torch.as_tensor(vbound, dtype=torch.float64).reshape(1)), "dz0": (dz + 0.0, bound)}


# ---- style and segmentation conditioning (csrc/vts_spade.hip: modulate, eval statistics, spectral norm; csrc/vts_style.hip: AdaIN;
# csrc/vts_style_levels.hip: the 16-class style bias and the mapping Linear; the six vts_modconv_* entries of csrc/vts_stylegan2.hip) --------
# Units are derived rounding counts as in the resample section, (r + K) u absref, with two additions.
#
# Special functions.  `/`, sqrtf and rsqrtf get a constant each, measured as TANH_E was: worst |f32 - f64| / (u |f64|) of PyTorch's own
# device kernels on the MI355X over 2^23 log-uniform arguments each (profiles/r22_style_kernels_parity.txt):
#   torch.div    0.9996 at -1.30125928 / -5.204319   (both operands +-[1e-6, 1e6])
#   torch.sqrt   1.0000 at 16777218                  ([1e-12, 1e8])
#   torch.rsqrt  1.0000 at 0.000244140596            ([1e-12, 1e8]; 0.9999 at 0.000976559124 over [1e-6, 64])
# The ROCm installation carries no document that states a bound for them.  The bound allows twice the measured worst plus 2 (one ulp is
# <= 2 u |ref|): the library's own expansion and PyTorch's kernel may differ.
DIV_E_MEASURED, SQRT_E_MEASURED, RSQRT_E_MEASURED = 0.9996, 1.0000, 1.0000
DIV_E, SQRT_E, RSQRT_E = 2 * DIV_E_MEASURED + 2, 2 * SQRT_E_MEASURED + 2, 2 * RSQRT_E_MEASURED + 2
#
# Statistics computed inside a call (AdaIN's means and stds, the demodulation sum, the group means of the modulate backward, sum(g v)).
# Every formula below is written once over values that carry (ref, unit) (class _V): an input is exact (unit 0); each operation gives the
# float64 result, propagates its operands' units to first order through the absolute partial derivatives and adds its own rounding:
#   a + b: ua + ub + u |a + b|          a * b: ua |b| + |a| ub + u |a b|          a / b: ua / |b| + |a| ub / b^2 + DIV_E u |a / b|
#   sqrt a: ua / (2 sqrt a) + SQRT_E u sqrt a      rsqrt a: ua rsqrt a / (2 a) + RSQRT_E u rsqrt a      tanh: ua (1 - tanh^2) + TANH_E u |tanh|
#   sum of K terms: sum of their units + (K - 1) u sum |term|  (any order: each term passes through at most K - 1 adds)
#   times an exact factor (a 0 / 1 mask, the selection of a class): nothing;  times the LeakyReLU slope: one rounding where it applies
# A fused multiply-add has one rounding fewer than the two operations counted.  The products of units dropped are second order in u: the
# tests allow 1.01, and no family needs more: the largest relative unit of an intermediate is that of x - mean on the offset row of AdaIN,
# about (m - 1) 100 u < 1e-3 for m = 129, so the dropped products stay below 0.1 % of a unit.
# Where an output of a call is a function of another output of the same call (spectral norm: v, u, sigma, w / sigma; its backward: the
# total, then dw) each stage is a function of its own: the first takes the inputs, the later ones take the value the call stored for the
# earlier output (read back, exact), so a wrong element in any stage fails that stage.
# Every formula also runs on any other arithmetic `A` (the fp32 one of tests/test_style_kernel_cases.py): A(tensor) lifts an exact input.
class _V:
    __slots__ = ("ref", "unit")

    def __init__(self, ref, unit=None):
        self.ref, self.unit = ref, (torch.zeros_like(ref) if unit is None else unit)

    @staticmethod
    def lift(t):
        return _V(_f64(t))

    @property
    def val(self):
        return self.ref

    @staticmethod
    def _co(o):
        return o if isinstance(o, _V) else _V(torch.tensor(_f32(o), dtype=torch.float64))

    def __add__(self, o):
        o = _V._co(o)
        r = self.ref + o.ref
        return _V(r, self.unit + o.unit + U * r.abs())

    __radd__ = __add__

    def __sub__(self, o):
        o = _V._co(o)
        r = self.ref - o.ref
        return _V(r, self.unit + o.unit + U * r.abs())

    def __mul__(self, o):
        o = _V._co(o)
        r = self.ref * o.ref
        return _V(r, self.unit * o.ref.abs() + self.ref.abs() * o.unit + U * r.abs())

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _V._co(o)
        r = self.ref / o.ref
        return _V(r, self.unit / o.ref.abs() + self.ref.abs() * o.unit / (o.ref * o.ref) + DIV_E * U * r.abs())

    def __rtruediv__(self, o):
        return _V._co(o) / self

    def sqrt(self):
        r = self.ref.sqrt()
        return _V(r, self.unit / (2 * r) + SQRT_E * U * r)

    def rsqrt(self):
        r = self.ref.rsqrt()
        return _V(r, self.unit * r / (2 * self.ref.abs()) + RSQRT_E * U * r)

    def tanh(self):
        r = self.ref.tanh()
        return _V(r, self.unit * (1 - r * r) + TANH_E * U * r.abs())

    def sum(self, dim, keep=False, cnt=None):
        """cnt: the number of terms that are not structural zeros (default: all of them)"""
        dim = (dim,) if isinstance(dim, int) else tuple(dim)
        n = math.prod(self.ref.shape[d] for d in dim) if cnt is None else cnt
        n = torch.as_tensor(n, dtype=torch.float64)
        return _V(self.ref.sum(dim, keepdim=keep), self.unit.sum(dim, keepdim=keep) + U * (n - 1).clamp_min(0) * self.ref.abs().sum(dim, keepdim=keep))

    def clamp_min(self, c):
        return _V(self.ref.clamp_min(c), torch.where(self.ref > c, self.unit, torch.zeros_like(self.unit)))

    def mask(self, m):
        """times an exact 0 / 1 factor"""
        m = m.to(torch.float64)
        return _V(self.ref * m, self.unit * m)

    def slope(self, f, rounds):
        """times the per-element factor f (1 or the fp32 slope); rounds: where that product rounds"""
        f = f.to(torch.float64)
        r = self.ref * f
        return _V(r, self.unit * f.abs() + U * rounds.to(torch.float64) * r.abs())

    def map(self, fn):
        """data movement (view, index, permute, pad with zeros)"""
        return _V(fn(self.ref), fn(self.unit))


def _pack(d, A):
    """{name: (ref, unit)} of the judge; the plain values under another arithmetic"""
    return {k: ((v.ref, v.unit) if A is None else v.val) for k, v in d.items()}


def _lrelu_factor(t, act):
    """(factor, where it rounds) of act'(t) for VTS_ACT_NONE / VTS_ACT_LRELU"""
    neg = ~(t.val > 0) if act == 1 else torch.zeros_like(t.val, dtype=torch.bool)
    return torch.where(neg, torch.full_like(t.val, SLOPE32[1]), torch.ones_like(t.val)), neg


def _planes(A, stat, n, c):
    return A(stat.reshape(n, c, 1, 1))


def _pad_zero(pad):
    return (lambda t: torch.nn.functional.pad(t, (pad,) * 4)) if pad else (lambda t: t)


def spade_modulate(x, mean, rstd, gamma, beta, act, out_pad=0, A=None):
    """vts_spade_modulate: out = act((x - mean) rstd (1 + gamma) + beta), x [N, C, H, W], mean / rstd [N C]; out_pad: inside a zero border
    (unit 0 there; the test compares the border bitwise with +0)"""
    L = A or _V.lift
    n, c = x.shape[:2]
    t = (L(x) - _planes(L, mean, n, c)) * _planes(L, rstd, n, c) * (1.0 + L(gamma)) + L(beta)
    return _pack({"out": t.slope(*_lrelu_factor(t, act)).map(_pad_zero(out_pad))}, A)


def spade_modulate_bwd(g, x, mean, rstd, gamma, beta, mode, act, A=None):
    """vts_spade_modulate_bwd on the dense interior of g: dgamma = g' xhat, dbeta = g', h = g' (1 + gamma);
    mode 0 / 1: dx = rstd ((h - mean_G h) - (xhat - mean_G xhat) mean_G(h xhat)), G = the plane / the channel over the batch; mode 2: dx = rstd h"""
    L = A or _V.lift
    n, c, hh, ww = x.shape
    r = _planes(L, rstd, n, c)
    xh = (L(x) - _planes(L, mean, n, c)) * r
    ga = 1.0 + L(gamma)
    gp = L(g).slope(*_lrelu_factor(xh * ga + L(beta), act))
    h = gp * ga
    out = {"dgamma": gp * xh, "dbeta": gp}
    if mode == 2:
        out["dx"] = h * r
    else:
        dims, cnt = ((2, 3), float(hh * ww)) if mode == 0 else ((0, 2, 3), float(n) * float(hh * ww))
        a, b, e = h.sum(dims, keep=True) / cnt, (h * xh).sum(dims, keep=True) / cnt, xh.sum(dims, keep=True) / cnt
        out["dx"] = r * ((h - a) - (xh - e) * b)
    return _pack(out, A)


def spade_eval_stats(running_mean, running_var, eps, n, A=None):
    """vts_spade_eval_stats: "mean" the running mean repeated over the batch (data movement, bitwise), "rstd" = 1 / sqrt(running_var + eps)"""
    L = A or _V.lift
    rep = lambda t: t.reshape(1, -1).repeat(n, 1).reshape(-1)
    return _pack({"mean": L(running_mean).map(rep), "rstd": (1.0 / (L(running_var) + eps).sqrt()).map(rep)}, A)


def _unit_vector(t, eps):
    return t / (t * t).sum(0).sqrt().clamp_min(_f32(eps))


def spectral_norm_v(w, u, eps, A=None):
    """stage 1 of vts_spectral_norm (training): v = W^T u / max(|W^T u|, eps) from the inputs; w [Co, K]"""
    L = A or _V.lift
    return _pack({"v": _unit_vector((L(w) * L(u.reshape(-1, 1))).sum(0), eps)}, A)


def spectral_norm_u(w, v, eps, A=None):
    """stage 2: u = W v / max(|W v|, eps) at the v the call stored"""
    L = A or _V.lift
    return _pack({"u": _unit_vector((L(w) * L(v.reshape(1, -1))).sum(1), eps)}, A)


def spectral_norm_sigma(w, u, v, A=None):
    """stage 3: sigma = u^T W v at the stored (training) or given u, v"""
    L = A or _V.lift
    return _pack({"sigma": (L(u) * (L(w) * L(v.reshape(1, -1))).sum(1)).sum(0, keep=True)}, A)


def spectral_norm_scale(w, sigma, A=None):
    """stage 4: w_out = w / sigma at the stored sigma"""
    L = A or _V.lift
    return _pack({"w_out": L(w) / L(sigma.reshape(1, 1))}, A)


def spectral_norm_bwd_total(g, w_sn, A=None):
    """stage 1 of vts_spectral_norm_bwd: <g, w_sn>"""
    L = A or _V.lift
    return _pack({"total": (L(g) * L(w_sn)).sum((0, 1)).map(lambda t: t.reshape(1))}, A)


def spectral_norm_bwd_dw(g, total, u, v, sigma, dw0=None, A=None):
    """stage 2: dw (+)= (g - total u v^T) / sigma at the total the call stored"""
    L = A or _V.lift
    val = (L(g) - L(total.reshape(1, 1)) * L(u.reshape(-1, 1)) * L(v.reshape(1, -1))) / L(sigma.reshape(1, 1))
    return _pack({"dw": val if dw0 is None else L(dw0) + val}, A)


def _group_stats(p, m, eps):
    mean = p.sum(1, keep=True) / float(m)
    d = p - mean
    return mean, ((d * d).sum(1, keep=True) / float(m - 1) + eps).sqrt()


def adain(x, s, eps, A=None):
    """vts_adain: out = (x - mean x) / std x * std s + mean s per row of x, s [NC, HW]; std = sqrt(unbiased variance + eps)"""
    L = A or _V.lift
    px, ps = L(x), L(s)
    (mx, sx), (ms, ss) = _group_stats(px, x.shape[1], eps), _group_stats(ps, x.shape[1], eps)
    return _pack({"out": (px - mx) / sx * ss + ms}, A)


def adain_bwd(g, x, s, eps, A=None):
    """vts_adain_bwd: the gradients of vts_adain's output w.r.t. both operands, with xhat = (x - mean x) / std x, gm = mean g,
    r = sum(g xhat) / (m - 1):  dx = std s / std x (g - gm - xhat r),  ds = gm + r (s - mean s) / std s"""
    L = A or _V.lift
    m = x.shape[1]
    pg, px, ps = L(g), L(x), L(s)
    (mx, sx), (ms, ss) = _group_stats(px, m, eps), _group_stats(ps, m, eps)
    xh = (px - mx) / sx
    gm, r = pg.sum(1, keep=True) / float(m), (pg * xh).sum(1, keep=True) / float(m - 1)
    return _pack({"dx": ss / sx * (pg - gm - xh * r), "ds": gm + r * (ps - ms) / ss}, A)


def tconv_taps(size):
    """[size, 4] 0 / 1: kernel index k reaches output position o of ConvTranspose2d(4, stride 2, padding 1) from an input of size / 2
    positions: o = 2 i + k - 1 for some 0 <= i < size / 2"""
    o, k = torch.arange(size).view(-1, 1), torch.arange(4).view(1, -1)
    i2 = o + 1 - k
    return ((i2 % 2 == 0) & (i2 >= 0) & (i2 < size)).to(torch.float64)


def style_bias(code, w, out0, act_out, A=None):
    """vts_style_bias: out = act_out(out0 + ConvTranspose2d(4, 2, 1) of the tile of r = max(code, 0) with the style rows w [K, Cout, 4, 4]).
    The tile is constant, so a position's term is the sum over the taps that reach it of V[n, co, tap] = sum_c r[n, c] w[c, co, tap]; the
    positions with the same taps (the distinct rows of tconv_taps) share the value."""
    L = A or _V.lift
    n, k = code.shape
    oh, ow = out0.shape[-2:]
    V = (L(code.clamp_min(0).reshape(n, k, 1, 1, 1)) * L(w.reshape(1, k, -1, 4, 4))).sum(1)            # [N, Cout, 4, 4]
    (ty, iy), (tx, ix) = [torch.unique(tconv_taps(s), dim=0, return_inverse=True) for s in (oh, ow)]
    taps = ty.view(-1, 1, 4, 1) * tx.view(1, -1, 1, 4)                                                 # [classes y, classes x, 4, 4]
    B = V.map(lambda t: t[:, :, None, None]).mask(taps).sum((4, 5), cnt=taps.sum((2, 3)))              # [N, Cout, classes y, classes x]
    t = L(out0) + B.map(lambda t: t[:, :, iy][:, :, :, ix])
    return _pack({"out": t.tanh() if act_out == 3 else t}, A)


def style_bias_bwd(g, code, k_cout, dw0=None, A=None):
    """vts_style_bias_bwd: dw[c, co, ky, kx] (+)= sum_n r[n, c] S[n, co, ky, kx], S = the sum of g over the positions the tap reaches"""
    L = A or _V.lift
    n, k = code.shape
    oh, ow = g.shape[-2:]
    my, mx = tconv_taps(oh), tconv_taps(ow)
    sx = L(g).map(lambda t: t[..., None]).mask(mx).sum(3, cnt=mx.sum(0))                               # [N, Cout, OH, 4 (kx)]
    S = sx.map(lambda t: t[:, :, :, None, :]).mask(my.view(oh, 4, 1)).sum(2, cnt=my.sum(0).view(4, 1))  # [N, Cout, 4, 4]
    val = (L(code.clamp_min(0).reshape(n, k, 1, 1, 1)) * S.map(lambda t: t[:, None])).sum(0)
    return _pack({"dw": val if dw0 is None else L(dw0) + val}, A)


def style_linear(x, w, A=None):
    """vts_style_linear: z[n, p] = sum_k x[n, k] w[p, k]"""
    L = A or _V.lift
    return _pack({"z": (L(x[:, None, :]) * L(w[None])).sum(2)}, A)


def style_linear_bwd(dz, x, w, dw0=None, want_dx=True, A=None):
    """vts_style_linear_bwd: dw[p, k] (+)= sum_n dz[n, p] x[n, k];  dx[n, k] = sum_p dz[n, p] w[p, k]"""
    L = A or _V.lift
    val = (L(dz[:, :, None]) * L(x[:, None, :])).sum(0)
    out = {"dw": val if dw0 is None else L(dw0) + val}
    if want_dx:
        out["dx"] = (L(dz[:, :, None]) * L(w[None])).sum(1)
    return _pack(out, A)


def modconv_demod(w, s, scale, eps, A=None):
    """vts_modconv_demod: demod[n, co] = rsqrt(scale^2 sum_{ci, k} (w[co, ci, k] s[n, ci])^2 + eps), w [Cout, Cin, KK], s [N, Cin]"""
    L = A or _V.lift
    ws = L(w[None]) * L(s[:, None, :, None])
    sc = L(torch.tensor(_f32(scale)))
    return _pack({"demod": (sc * sc * (ws * ws).sum((2, 3)) + eps).rsqrt()}, A)


def modconv_demod_bwd(dd, d, w, s, scale, dw0=None, ds0=None, A=None):
    """vts_modconv_demod_bwd: q = dd (-1/2) d^3;  dw (+)= 2 scale^2 w sum_n q s^2;  ds (+)= 2 scale^2 s sum_co q sum_k w^2"""
    L = A or _V.lift
    pd, pw, ps = L(d), L(w), L(s)
    q = L(dd) * -0.5 * pd * pd * pd                                                                    # [N, Cout]
    sc = L(torch.tensor(_f32(scale)))
    c2 = 2.0 * sc * sc
    dw = c2 * pw * (q.map(lambda t: t[:, :, None, None]) * (ps * ps).map(lambda t: t[:, None, :, None])).sum(0)
    ds = c2 * ps * (q.map(lambda t: t[:, :, None]) * (pw * pw).sum(2).map(lambda t: t[None])).sum(1)
    return _pack({"dw": dw if dw0 is None else L(dw0) + dw, "ds": ds if ds0 is None else L(ds0) + ds}, A)


def _wt(transpose):
    """[Cout, Cin, KK] -> the stored layout ([Cin, Cout, KK] when transposed)"""
    return (lambda t: t.transpose(0, 1).contiguous()) if transpose else (lambda t: t)


def modconv_weight(w, scale, eps, transpose, A=None):
    """vts_modconv_weight: wout = v d[co], v = scale w, d = rsqrt(sum_{ci, k} v^2 + eps)"""
    L = A or _V.lift
    v = _f32(scale) * L(w)
    return _pack({"wout": (v * ((v * v).sum((1, 2), keep=True) + eps).rsqrt()).map(_wt(transpose))}, A)


def modconv_weight_bwd(w, g, scale, eps, transpose, dw0=None, A=None):
    """vts_modconv_weight_bwd: dw (+)= scale (d g - d^3 v sum(g v)), g in wout's layout"""
    L = A or _V.lift
    v, pg = _f32(scale) * L(w), L(_wt(transpose)(g))
    d = ((v * v).sum((1, 2), keep=True) + eps).rsqrt()
    val = _f32(scale) * (d * pg - d * d * d * v * (pg * v).sum((1, 2), keep=True))
    return _pack({"dw": val if dw0 is None else L(dw0) + val}, A)


def modconv_scale_dot(a, b, f, alpha, want_out, dot0=None, A=None):
    """vts_modconv_scale_dot: out = a f[row] (when asked), dot[row] (+)= alpha sum_i a b; a, b [NC, HW]"""
    L = A or _V.lift
    val = _f32(alpha) * (L(a) * L(b)).sum(1)
    out = {"dot": val if dot0 is None else L(dot0) + val}
    if want_out:
        out["out"] = L(a) * L(f.reshape(-1, 1))
    return _pack(out, A)


def modconv_transpose(w, out0=None, A=None):
    """vts_modconv_transpose: out[ci, co, k] (+)= w[co, ci, k]; data movement without out0 (bitwise)"""
    L = A or _V.lift
    t = L(w).map(_wt(True))
    return _pack({"out": t if out0 is None else L(out0) + t}, A)
