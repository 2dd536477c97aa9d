"""The kernels that carry the style and segmentation conditioning (csrc/vts_spade.hip: modulate, eval statistics, spectral norm;
csrc/vts_style.hip: AdaIN; csrc/vts_style_levels.hip: the 16-class style bias and the mapping Linear; the six vts_modconv_* entries of
csrc/vts_stylegan2.hip) against the float64 judges of oracle/launch_ref.py, elementwise, on the hand-built table tests/style_kernel_cases.py
(the smallest shapes that reach each dispatch alternative, chunk plan, cap, tail wavefront and second grid sweep).

Operands, guard bands and the per-call assertions are those of tests/judge_harness.py: the expected instance string
(lib.vts_last_kernel(), which names every alternative the call took), |got - ref| <= 1.01 unit at every element of an arithmetic output -- the
unit is a derived rounding count propagated through the statistics the call computes, the 1 % covers second-order terms -- or bitwise
equality for the data-movement rows (the transpose, the eval mean, the zero border of a padded output, dx of a 1 x 1 plane), everything the
call does not own bitwise unchanged (guard bands, inputs, u / v when not training, a given workspace in mode 2, the NaN channels around a
channel slice), and a second identical call bitwise identical.  The later outputs of a staged call (spectral norm: u after v, sigma, w /
sigma; its backward: dw after the total) are judged at what the call itself stored for the earlier ones.  Workspaces have exactly the stated
size.  The border of a padded gradient holds NaN.  The module prints the worst err / unit per instance and family (pytest -s);
profiles/r22_style_kernels_parity.txt is that table from the MI355X."""
import pytest
import torch
import torch.nn.functional as F

import style_kernel_cases as T
from judge_harness import Op, judge as _judge
from oracle import launch_ref as R

pytestmark = pytest.mark.gpu

BOUND = 1.01         # every family; a kernel that needs more is a finding, not a reason for a larger constant
WORST = {}
NAN = float("nan")


@pytest.fixture(scope="module")
def gpu():
    from vts import lib as L
    lib = L.load()
    yield lib, L
    if WORST:
        lines = ["# per instance and family: worst err / unit over its rows vs float64 (oracle/launch_ref.py), bound %g for every family" % BOUND,
                 "# unit: derived rounding counts, propagated to first order through the statistics a call computes; DIV_E %.4f SQRT_E %.4f RSQRT_E %.4f"
                 % (R.DIV_E, R.SQRT_E, R.RSQRT_E),
                 "# outputs = judged outputs of tests/style_kernel_cases.py; family 'exact': bitwise, all equal",
                 "%-9s %-16s %7s  %-84s %s" % ("worst", "family", "outputs", "instance", "at case")]
        for (inst, _), (w, case, fam, calls) in sorted(WORST.items(), key=lambda kv: (-kv[1][0], kv[0])):
            lines.append("%-9.4f %-16s %7d  %-84s %s" % (w, fam, calls, inst, case))
        print("\n[%s]\n%s" % (__name__, "\n".join(lines)))


def judge(gpu, tag, expected, call, opnds, outs):
    _judge(gpu[0], tag, expected, call, [o for o in opnds if o is not None], outs, BOUND, WORST, per_family=True)


def ids(rows):
    return [r[0] for r in rows]


def dptr(o):
    return None if o is None else o.t.data_ptr()


def op(t, off=False, shape=None):
    """an input (or a seeded output) between guard bands; off: starting 4 bytes past a 16-byte boundary"""
    o = Op(shape or t.shape, t, offset=1 if off else 0)
    assert o.t.data_ptr() % 16 == (4 if off else 0)
    return o


def blank(shape, off=False):
    o = Op(shape, offset=1 if off else 0)
    assert o.t.data_ptr() % 16 == (4 if off else 0)
    return o


def scratch(floats):
    return Op((int(floats),)) if floats else None


def sliced(shape, init, layout):
    """[N, Cout, ...] dense, or as channels 2 : 2 + Cout of a tensor of Cout + 3 channels whose other channels hold NaN; (op, batch stride)"""
    per = int(torch.tensor(shape[2:]).prod())
    ns, lead = ((shape[1] + T.SLICE_LEAD + T.SLICE_TAIL) * per, T.SLICE_LEAD * per) if layout == "slice" else (shape[1] * per, 0)
    return Op(shape, init, ns=ns, lead=lead), ns


# ---------------------------------------------------------------------------------------------------------------- SPADE modulate
@pytest.mark.parametrize("row", T.MOD, ids=ids(T.MOD))
def test_spade_modulate_both_instances(gpu, row):
    """the padded output is written whole: the interior judged, the border bitwise +0"""
    lib, L = gpu
    rid, n, c, h, w, act, pad, off = row
    x, mean, rstd, gamma, beta, _ = T.mod_inputs(row)
    xo, go, bo = op(x, off == "x"), op(gamma, off == "gamma"), op(beta, off == "beta")
    mo, ro, out = op(mean), op(rstd), blank((n, c, h + 2 * pad, w + 2 * pad), off == "out")
    call = lambda: L.check(lib.vts_spade_modulate(xo.t.data_ptr(), mo.t.data_ptr(), ro.t.data_ptr(), go.t.data_ptr(), bo.t.data_ptr(), n, c, h, w, act,
                                                  out.t.data_ptr(), pad, L.stream()), rid)
    ref, unit = R.spade_modulate(x, mean, rstd, gamma, beta, act, pad)["out"]
    outs = [(out, None, ref, unit, "modulate")]
    if pad:
        border = torch.ones(out.shape, dtype=torch.bool)
        border[:, :, pad:pad + h, pad:pad + w] = False
        outs.append((out, border, torch.zeros(int(border.sum())), None, "exact"))
    judge(gpu, rid, T.mod_instance(row), call, [xo, mo, ro, go, bo, out], outs)


@pytest.mark.parametrize("row", T.MODB, ids=ids(T.MODB))
def test_spade_modulate_bwd_every_plan(gpu, row):
    """g is read at the interior of a NaN border; the workspace is owned scratch in modes 0 / 1 and untouched (or NULL) in mode 2; the 1 x 1
    plane's dx is exactly +0"""
    lib, L = gpu
    rid, n, c, h, w, mode, act, gpad, wsk, off, _ = row
    g, x, mean, rstd, gamma, beta, _ = T.modb_inputs(row)
    go = op(F.pad(g, (gpad,) * 4, value=NAN) if gpad else g)
    xo, mo, ro, gao, bo = op(x, off == "x"), op(mean), op(rstd), op(gamma), op(beta)
    dga, dbe, dx = blank(x.shape), blank(x.shape), blank(x.shape, off == "dx")
    floats = lib.vts_spade_modulate_bwd_ws_floats(n, c)
    assert floats == 6 * n * c
    ws = None if wsk == "null" else (op(T.U((floats,), 7711, rid + "ws")) if wsk == "given" else scratch(floats))
    call = lambda: L.check(lib.vts_spade_modulate_bwd(go.t.data_ptr(), gpad, xo.t.data_ptr(), mo.t.data_ptr(), ro.t.data_ptr(), gao.t.data_ptr(),
                                                      bo.t.data_ptr(), n, c, h, w, mode, act, dga.t.data_ptr(), dbe.t.data_ptr(), dx.t.data_ptr(),
                                                      dptr(ws), L.stream()), rid)
    ref = R.spade_modulate_bwd(g, x, mean, rstd, gamma, beta, mode, act)
    outs = [(o, None, ref[k][0], ref[k][1], "modulate_bwd_" + k) for o, k in ((dga, "dgamma"), (dbe, "dbeta"), (dx, "dx"))]
    if mode == 0 and h * w == 1:
        outs.append((dx, None, torch.zeros(x.shape), None, "exact"))
    if wsk == "own":
        outs.append((ws, None, None, None, "scratch"))
    judge(gpu, rid, T.modb_instance(row), call, [go, xo, mo, ro, gao, bo, dga, dbe, dx, ws], outs)


@pytest.mark.parametrize("row", T.EVS, ids=ids(T.EVS))
def test_spade_eval_stats(gpu, row):
    lib, L = gpu
    rid, n, c = row
    rm, rv = T.evs_inputs(row)
    rmo, rvo, mean, rstd = op(rm), op(rv), blank((n * c,)), blank((n * c,))
    call = lambda: L.check(lib.vts_spade_eval_stats(rmo.t.data_ptr(), rvo.t.data_ptr(), T.EVS_EPS, n, c, mean.t.data_ptr(), rstd.t.data_ptr(), L.stream()), rid)
    ref = R.spade_eval_stats(rm, rv, T.EVS_EPS, n)
    judge(gpu, rid, "spade_eval_stats_kernel", call, [rmo, rvo, mean, rstd],
          [(mean, None, ref["mean"][0], None, "exact"), (rstd, None, ref["rstd"][0], ref["rstd"][1], "eval_stats")])


# ---------------------------------------------------------------------------------------------------------------- spectral norm
@pytest.mark.parametrize("row", T.SN, ids=ids(T.SN))
def test_spectral_norm_in_stages(gpu, row):
    """training: v from the inputs, u at the stored v, sigma at the stored u and v, w / sigma at the stored sigma; not training: u and v are
    inputs the call must leave alone"""
    lib, L = gpu
    rid, co, k, training, off = row
    w, u, v = T.sn_inputs(row)
    wo, uo, vo = op(w, off == "w"), op(u), op(v, off == "v")
    w_out, sigma = blank((co, k)), blank((1,))
    floats = lib.vts_spectral_norm_ws_floats(co, k)
    assert floats == T.sn_ws_floats(co, k)
    ws = scratch(floats)
    call = lambda: L.check(lib.vts_spectral_norm(wo.t.data_ptr(), uo.t.data_ptr(), vo.t.data_ptr(), co, k, training, T.SN_EPS, w_out.t.data_ptr(),
                                                 sigma.t.data_ptr(), ws.t.data_ptr(), floats, L.stream()), rid)
    outs = [(ws, None, None, None, "scratch")]
    if training:
        rv = R.spectral_norm_v(w, u, T.SN_EPS)["v"]
        outs += [(vo, None, rv[0], rv[1], "sn_v"), (uo, None, lambda st: R.spectral_norm_u(w, st(vo), T.SN_EPS)["u"], None, "sn_u")]
    outs += [(sigma, None, lambda st: R.spectral_norm_sigma(w, st(uo), st(vo))["sigma"], None, "sn_sigma"),
             (w_out, None, lambda st: R.spectral_norm_scale(w, st(sigma))["w_out"], None, "sn_scale")]
    judge(gpu, rid, T.sn_instance(row), call, [wo, uo, vo, w_out, sigma, ws], outs)


@pytest.mark.parametrize("row", T.SNB, ids=ids(T.SNB))
def test_spectral_norm_bwd_in_stages(gpu, row):
    """the workspace holds Co row products (scratch) and the total, judged from the inputs; dw is judged at the stored total"""
    lib, L = gpu
    rid, co, k, acc = row
    g, wsn, u, v, sg, dw0 = T.snb_inputs(row)
    go, wo, uo, vo, so = op(g), op(wsn), op(u), op(v), op(sg)
    dw, ws = (op(dw0) if acc else blank((co, k))), scratch(co + 1)
    call = lambda: L.check(lib.vts_spectral_norm_bwd(go.t.data_ptr(), wo.t.data_ptr(), uo.t.data_ptr(), vo.t.data_ptr(), so.t.data_ptr(), co, k,
                                                     dw.t.data_ptr(), acc, ws.t.data_ptr(), co + 1, L.stream()), rid)
    tot = R.spectral_norm_bwd_total(g, wsn)["total"]
    judge(gpu, rid, T.SNB_INSTANCE, call, [go, wo, uo, vo, so, dw, ws],
          [(ws, slice(0, co), None, None, "scratch"), (ws, slice(co, co + 1), tot[0], tot[1], "snb_total"),
           (dw, None, lambda st: R.spectral_norm_bwd_dw(g, st(ws)[co:], u, v, sg, dw0 if acc else None)["dw"], None, "snb_dw")])


# ---------------------------------------------------------------------------------------------------------------- AdaIN
@pytest.mark.parametrize("row", T.ADA, ids=ids(T.ADA))
def test_adain_forward_and_backward(gpu, row):
    lib, L = gpu
    rid, nc, hw, _ = row
    g, x, s = T.ada_inputs(row)
    go, xo, so, out, dx, ds = op(g), op(x), op(s), blank(x.shape), blank(x.shape), blank(x.shape)
    ref = R.adain(x, s, T.ADA_EPS)["out"]
    judge(gpu, rid, "adain_fwd_kernel", lambda: L.check(lib.vts_adain(xo.t.data_ptr(), so.t.data_ptr(), nc, hw, T.ADA_EPS, out.t.data_ptr(), L.stream()), rid),
          [xo, so, out], [(out, None, ref[0], ref[1], "adain")])
    ref = R.adain_bwd(g, x, s, T.ADA_EPS)
    call = lambda: L.check(lib.vts_adain_bwd(go.t.data_ptr(), xo.t.data_ptr(), so.t.data_ptr(), nc, hw, T.ADA_EPS, dx.t.data_ptr(), ds.t.data_ptr(),
                                             L.stream()), rid)
    judge(gpu, rid + "-bwd", "adain_bwd_kernel", call, [go, xo, so, dx, ds],
          [(dx, None, ref["dx"][0], ref["dx"][1], "adain_bwd_dx"), (ds, None, ref["ds"][0], ref["ds"][1], "adain_bwd_ds")])


# ---------------------------------------------------------------------------------------------------------------- style bias, style Linear
@pytest.mark.parametrize("row", T.SB, ids=ids(T.SB))
def test_style_bias_in_place_on_a_seeded_output(gpu, row):
    lib, L = gpu
    rid, n, k, cout, oh, ow, act, layout = row
    code, w, out0 = T.sb_inputs(row)
    co, wo = op(code), op(w)
    out, ns = sliced((n, cout, oh, ow), out0, layout)
    floats = lib.vts_style_bias_ws_floats(n, cout, oh)
    assert floats == T.sb_ws_floats(n, cout, oh)
    ws = scratch(floats)
    call = lambda: L.check(lib.vts_style_bias(co.t.data_ptr(), n, k, wo.t.data_ptr(), cout, oh, ow, out.t.data_ptr(), ns, act, ws.t.data_ptr(), L.stream()), rid)
    ref = R.style_bias(code, w, out0, act)["out"]
    judge(gpu, rid, T.SB_INSTANCE, call, [co, wo, out, ws],
          [(out, None, ref[0], ref[1], "style_bias_tanh" if act == T.ACT_TANH else "style_bias"), (ws, None, None, None, "scratch")])


@pytest.mark.parametrize("row", T.SBB, ids=ids(T.SBB))
def test_style_bias_bwd(gpu, row):
    lib, L = gpu
    rid, n, k, cout, oh, ow, acc, layout = row
    g, code, dw0 = T.sbb_inputs(row)
    go, ns = sliced((n, cout, oh, ow), g, layout)
    co, dw, ws = op(code), (op(dw0) if acc else blank(dw0.shape)), scratch(lib.vts_style_bias_ws_floats(n, cout, oh))
    call = lambda: L.check(lib.vts_style_bias_bwd(go.t.data_ptr(), ns, co.t.data_ptr(), n, k, cout, oh, ow, dw.t.data_ptr(), acc, ws.t.data_ptr(), L.stream()), rid)
    ref = R.style_bias_bwd(g, code, None, dw0 if acc else None)["dw"]
    judge(gpu, rid, T.SBB_INSTANCE, call, [go, co, dw, ws], [(dw, None, ref[0], ref[1], "style_bias_bwd"), (ws, None, None, None, "scratch")])


@pytest.mark.parametrize("row", T.LIN, ids=ids(T.LIN))
def test_style_linear(gpu, row):
    lib, L = gpu
    rid, n, k, p = row
    x, w, _, _ = T.lin_inputs(row)
    xo, wo, z = op(x), op(w), blank((n, p))
    ref = R.style_linear(x, w)["z"]
    judge(gpu, rid, T.LIN_INSTANCE, lambda: L.check(lib.vts_style_linear(xo.t.data_ptr(), wo.t.data_ptr(), n, k, p, z.t.data_ptr(), L.stream()), rid),
          [xo, wo, z], [(z, None, ref[0], ref[1], "linear")])


@pytest.mark.parametrize("row", T.LINB, ids=ids(T.LINB))
def test_style_linear_bwd_with_and_without_dx(gpu, row):
    """without dx the weight and the workspace are NULL"""
    lib, L = gpu
    rid, n, k, p, want_dx, acc = row
    x, w, dz, dw0 = T.lin_inputs(row)
    floats = lib.vts_style_linear_ws_floats(n, k, p)
    assert floats == T.lin_ws_floats(n, k, p)
    zo, xo, dw = op(dz), op(x), (op(dw0) if acc else blank((p, k)))
    wo, dx, ws = (op(w), blank((n, k)), scratch(floats)) if want_dx else (None, None, None)
    call = lambda: L.check(lib.vts_style_linear_bwd(zo.t.data_ptr(), xo.t.data_ptr(), dptr(wo), n, k, p, dw.t.data_ptr(), acc, dptr(dx), dptr(ws), L.stream()), rid)
    ref = R.style_linear_bwd(dz, x, w, dw0 if acc else None, bool(want_dx))
    outs = [(dw, None, ref["dw"][0], ref["dw"][1], "linear_bwd_dw")]
    if want_dx:
        outs += [(dx, None, ref["dx"][0], ref["dx"][1], "linear_bwd_dx"), (ws, None, None, None, "scratch")]
    judge(gpu, rid, T.linb_instance(row), call, [zo, xo, wo, dw, dx, ws], outs)


# ---------------------------------------------------------------------------------------------------------------- modulated convolution
@pytest.mark.parametrize("row", T.DEM, ids=ids(T.DEM))
def test_modconv_demod(gpu, row):
    lib, L = gpu
    rid, n, co, ci, kk, _ = row
    w, s = T.dem_inputs(row)
    wo, so, d = op(w), op(s), blank((n, co))
    sc = T.mod_scale(ci, kk)
    ref = R.modconv_demod(w, s, sc, T.DEM_EPS)["demod"]
    judge(gpu, rid, T.DEM_INSTANCE, lambda: L.check(lib.vts_modconv_demod(wo.t.data_ptr(), so.t.data_ptr(), n, co, ci, kk, sc, T.DEM_EPS, d.t.data_ptr(),
                                                                          L.stream()), rid), [wo, so, d], [(d, None, ref[0], ref[1], "demod")])


@pytest.mark.parametrize("row", T.MODW, ids=ids(T.MODW))
def test_modconv_weight_both_layouts(gpu, row):
    lib, L = gpu
    rid, co, ci, kk, t, _ = row
    w = T.modw_inputs(row)[0]
    wo, out = op(w), blank((ci, co, kk) if t else (co, ci, kk))
    sc = T.mod_scale(ci, kk)
    ref = R.modconv_weight(w, sc, T.DEM_EPS, t)["wout"]
    judge(gpu, rid, T.MODW_INSTANCE, lambda: L.check(lib.vts_modconv_weight(wo.t.data_ptr(), co, ci, kk, sc, T.DEM_EPS, t, out.t.data_ptr(), L.stream()), rid),
          [wo, out], [(out, None, ref[0], ref[1], "modw")])


@pytest.mark.parametrize("row", T.MODWB, ids=ids(T.MODWB))
def test_modconv_weight_bwd_both_layouts(gpu, row):
    lib, L = gpu
    rid, co, ci, kk, t, acc, _ = row
    w, g, dw0 = T.modw_inputs(row)
    wo, go, dw = op(w), op(g), (op(dw0) if acc else blank(w.shape))
    sc = T.mod_scale(ci, kk)
    ref = R.modconv_weight_bwd(w, g, sc, T.DEM_EPS, t, dw0 if acc else None)["dw"]
    call = lambda: L.check(lib.vts_modconv_weight_bwd(wo.t.data_ptr(), go.t.data_ptr(), co, ci, kk, sc, T.DEM_EPS, t, dw.t.data_ptr(), acc, L.stream()), rid)
    judge(gpu, rid, T.MODWB_INSTANCE, call, [wo, go, dw], [(dw, None, ref[0], ref[1], "modw_bwd")])


@pytest.mark.parametrize("row", T.DMB, ids=ids(T.DMB))
def test_modconv_demod_bwd_both_accumulate_flags(gpu, row):
    lib, L = gpu
    rid, n, co, ci, kk, adw, ads = row
    dd, d, w, s, dw0, ds0 = T.dmb_inputs(row)
    ddo, do, wo, so = op(dd), op(d), op(w), op(s)
    dw, ds = (op(dw0) if adw else blank(w.shape)), (op(ds0) if ads else blank(s.shape))
    sc = T.mod_scale(ci, kk)
    ref = R.modconv_demod_bwd(dd, d, w, s, sc, dw0 if adw else None, ds0 if ads else None)
    call = lambda: L.check(lib.vts_modconv_demod_bwd(ddo.t.data_ptr(), do.t.data_ptr(), wo.t.data_ptr(), so.t.data_ptr(), n, co, ci, kk, sc, dw.t.data_ptr(),
                                                     adw, ds.t.data_ptr(), ads, L.stream()), rid)
    judge(gpu, rid, T.DMB_INSTANCE, call, [ddo, do, wo, so, dw, ds],
          [(dw, None, ref["dw"][0], ref["dw"][1], "demod_bwd_dw"), (ds, None, ref["ds"][0], ref["ds"][1], "demod_bwd_ds")])


@pytest.mark.parametrize("row", T.SD, ids=ids(T.SD))
def test_modconv_scale_dot_every_instance_and_plan(gpu, row):
    """without out the factors are NULL; the workspace has exactly vts_modconv_scale_dot_ws_floats floats (NULL where that is 0)"""
    lib, L = gpu
    rid, nc, hw, want_out, off, acc = row
    a, b, f, dot0 = T.sd_inputs(row)
    ao, bo = op(a, off == "a"), op(b, off == "b")
    fo, out = (op(f), blank((nc, hw), off == "out")) if want_out else (None, None)
    dot = op(dot0) if acc else blank((nc,))
    floats = lib.vts_modconv_scale_dot_ws_floats(nc, hw)
    assert floats == T.sd_ws_floats(nc, hw)
    ws = scratch(floats)
    call = lambda: L.check(lib.vts_modconv_scale_dot(ao.t.data_ptr(), bo.t.data_ptr(), dptr(fo), nc, hw, T.SD_ALPHA, dptr(out), dot.t.data_ptr(), acc, dptr(ws),
                                                     floats, L.stream()), rid)
    ref = R.modconv_scale_dot(a, b, f, T.SD_ALPHA, bool(want_out), dot0 if acc else None)
    outs = [(dot, None, ref["dot"][0], ref["dot"][1], "scale_dot")]
    if want_out:
        outs.append((out, None, ref["out"][0], ref["out"][1], "scale"))
    if ws is not None:
        outs.append((ws, None, None, None, "scratch"))
    judge(gpu, rid, T.sd_instance(row), call, [ao, bo, fo, out, dot, ws], outs)


@pytest.mark.parametrize("row", T.TR, ids=ids(T.TR))
def test_modconv_transpose_bitwise_and_accumulating(gpu, row):
    lib, L = gpu
    rid, co, ci, kk, acc = row
    w, o0 = T.tr_inputs(row)
    wo, out = op(w), (op(o0) if acc else blank(o0.shape))
    call = lambda: L.check(lib.vts_modconv_transpose(wo.t.data_ptr(), co, ci, kk, out.t.data_ptr(), acc, L.stream()), rid)
    ref = R.modconv_transpose(w, o0 if acc else None)["out"]
    outs = [(out, None, ref[0], None, "exact")]
    if acc:
        outs.append((out, None, ref[0], ref[1], "transpose_acc"))
    judge(gpu, rid, T.TR_INSTANCE, call, [wo, out], outs)
