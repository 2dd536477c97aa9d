"""The padding, blur, tap-embedding and table-resampling kernels of csrc/vts_resample.hip, upfirdn2d / bias_act of csrc/vts_stylegan2.hip
and the nearest / tanh_bwd kernels of csrc/vts_spade.hip against the float64 and exact judges of oracle/launch_ref.py, elementwise, on the
hand-built table tests/resample_cases.py (the smallest shapes that reach each block edge, dispatch threshold and second grid sweep).

Operands, guard bands and the per-call assertions are those of tests/judge_harness.py: the expected kernel instance
(lib.vts_last_kernel()), |got - ref| <= 1.01 unit at every element of an arithmetic output -- the unit is a derived worst-case rounding
count, the 1 % covers second-order terms -- or bitwise equality for the integer-valued rows, every element the call does not own bitwise
unchanged, and a second identical call bitwise identical.  tanh alone carries a measured constant (R.TANH_E, stated there).
The module prints the worst err / unit per kernel instance (pytest -s); profiles/r18_resample_parity.txt is that table from the MI355X."""
import ctypes as C

import pytest
import torch

import resample_cases as T
from judge_harness import Op, bits, judge as _judge
from oracle import detrand
from oracle import launch_ref as R

pytestmark = pytest.mark.gpu

BOUND = 1.01         # every arithmetic row; a kernel that needs more is a finding, not a reason for a larger constant
WORST = {}


@pytest.fixture(scope="module")
def gpu():
    from vts import lib as L
    from vts import ops
    lib = L.load()
    yield lib, ops, L
    if WORST:
        lines = ["# per kernel instance: worst err / unit over its rows vs float64 (oracle/launch_ref.py), bound %g for every family" % BOUND,
                 "# unit = (r + K) u absref, derived; tanh rows: u |t| (1 - ref^2) + E u |ref|, E = 2 * %.4f + 2 = %.4f (torch.tanh on the MI355X"
                 % (R.TANH_E_MEASURED, R.TANH_E),
                 "# is at most %.4f u |ref| from float64).  outputs = judged outputs of tests/resample_cases.py; family 'exact': bitwise, all equal"
                 % R.TANH_E_MEASURED,
                 "%-9s %-10s %7s  %-28s %s" % ("worst", "family", "outputs", "instance", "at case")]
        for (inst, _), (w, case, fam, calls) in sorted(WORST.items(), key=lambda kv: (-kv[1][0], kv[0])):
            lines.append("%-9.4f %-10s %7d  %-28s %s" % (w, fam, calls, inst, case))
        print("\n[%s]\n%s" % (__name__, "\n".join(lines)))


def judge(gpu, tag, expected, call, opnds, outs):
    _judge(gpu[0], tag, expected, call, opnds, outs, BOUND, WORST, per_family=True)


def ids(rows):
    return [r[0] for r in rows]


def opt(t, shape=None):
    """an Op of the tensor (None: no operand)"""
    return None if t is None else Op(t.shape if shape is None else shape, t)


def dptr(o):
    return None if o is None else o.t.data_ptr()


def some(*ops):
    return [o for o in ops if o is not None]


# ---------------------------------------------------------------------------------------------------------------- padding
@pytest.mark.parametrize("row", T.PAD, ids=ids(T.PAD))
def test_pad_affine_modes_activations_strides(gpu, row):
    lib, ops, L = gpu
    rid, n, c, h, w, pads, mode, act, aff, has_res, layout = row
    pt, pb, pl, pr = pads
    ph, pw = h + pt + pb, w + pl + pr
    x, sc, sh, res, _ = T.pad_inputs(row)
    xo = Op(x.shape, x, ns=c * h * w + 5, lead=2) if layout == "gap" else Op(x.shape, x)
    sco, sho, reso = opt(sc), opt(sh), opt(res)
    if layout == "stack":
        out = Op((n, 7, ph, pw))
        optr, ons, idx = out.t[:, 1:4].data_ptr(), 7 * ph * pw, (slice(None), slice(1, 4))
    else:
        out = Op((n, c, ph, pw))
        optr, ons, idx = out.t.data_ptr(), 0, None
    opnd = L.operand(xo.t, sco.t if aff else None, sho.t if aff else None, C_=c, nstride=xo.ns)
    call = lambda: L.check(lib.vts_pad_affine(C.byref(opnd), n, h, w, pt, pb, pl, pr, mode, act, dptr(reso), optr, ons, L.stream()), "vts_pad_affine")
    ref, unit = R.pad_affine(x, sc, sh, pads, mode, act, res)["out"]
    if act == T.NONE and not aff and not has_res:
        assert float(unit.max()) == 0                         # a pure gather: exact
    judge(gpu, rid, "pad_affine_kernel", call, some(xo, sco, sho, reso, out), [(out, idx, ref, unit, "tanh" if act == T.TANH else "pad")])


@pytest.mark.parametrize("row", T.PAD_BWD, ids=[T.pad_bwd_id(r) for r in T.PAD_BWD])
@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc"])
def test_pad_bwd_bitwise(gpu, row, acc):
    lib, ops, L = gpu
    n, c, h, w, pads, mode = row
    dpad, seed = T.pad_bwd_inputs(row)
    do, di = Op(dpad.shape, dpad), Op(seed.shape, seed if acc else None)
    ref, _ = R.pad_bwd(dpad, (h, w), pads, mode, seed if acc else None)["din"]
    if mode == T.REPLICATE and h > 1 and w > 1:               # the replicate corner collects (pt + 1)(pl + 1) terms
        assert float(R.pad_bwd(torch.ones_like(dpad), (h, w), pads, mode)["din"][0][0, 0, 0, 0]) == (pads[0] + 1) * (pads[2] + 1)
    call = lambda: L.check(lib.vts_pad_bwd(do.t.data_ptr(), n, c, h, w, *pads, mode, di.t.data_ptr(), int(acc), L.stream()), "vts_pad_bwd")
    judge(gpu, "%s-%s" % (T.pad_bwd_id(row), "acc" if acc else "plain"), "pad_bwd_kernel", call, [do, di], [(di, None, ref, None, "exact")])


# ---------------------------------------------------------------------------------------------------------------- blur down / up
@pytest.mark.parametrize("row", T.BLUR, ids=ids(T.BLUR))
def test_blur_down_up(gpu, row):
    lib, ops, L = gpu
    rid, kind, n, c, h, w, variant = row
    x, sc, sh, act, _ = T.blur_inputs(row)
    xo = Op(x.shape, x, ns=c * h * w + 3, lead=1) if variant == "gap" else Op(x.shape, x)
    sco, sho = opt(sc), opt(sh)
    out = Op((n, c) + T.blur_out_hw(kind, h, w))
    opnd = L.operand(xo.t, sco.t if sco else None, sho.t if sho else None, C_=c, nstride=xo.ns)
    fn = lib.vts_blur_down if kind == "down" else lib.vts_blur_up
    call = lambda: L.check(fn(C.byref(opnd), act, n, h, w, out.t.data_ptr(), L.stream()), "vts_blur_" + kind)
    ref, unit = (R.blur_down if kind == "down" else R.blur_up)(x, sc, sh, act)["out"]
    judge(gpu, rid, "blur_%s_kernel" % kind, call, some(xo, sco, sho, out), [(out, None, ref, None if sc is None else unit, "exact" if sc is None else "blur")])


@pytest.mark.parametrize("row", T.BLUR_BWD, ids=["blur-%s-bwd-%dx%d" % r for r in T.BLUR_BWD])
@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc"])
def test_blur_adjoints_bitwise(gpu, row, acc):
    lib, ops, L = gpu
    kind, h, w = row
    g, seed = T.blur_bwd_inputs(row)
    go, di = Op(g.shape, g), Op(seed.shape, seed if acc else None)
    ref, _ = (R.blur_down_bwd if kind == "down" else R.blur_up_bwd)(g, (h, w), seed if acc else None)["din"]
    fn = lib.vts_blur_down_bwd if kind == "down" else lib.vts_blur_up_bwd
    call = lambda: L.check(fn(go.t.data_ptr(), 2, 3, h, w, di.t.data_ptr(), int(acc), L.stream()), "vts_blur_%s_bwd" % kind)
    judge(gpu, "blur-%s-bwd-%dx%d-%s" % (kind, h, w, "acc" if acc else "plain"), "blur_%s_bwd_kernel" % kind, call, [go, di],
          [(di, None, ref, None, "exact")])


# ---------------------------------------------------------------------------------------------------------------- weight taps
@pytest.mark.parametrize("row", T.TAP, ids=ids(T.TAP))
def test_tap_embed_and_extract_bitwise(gpu, row):
    """extract leaves every weight element outside the block bitwise unchanged (NaN there)"""
    lib, ops, L = gpu
    rid, entry, k, p, q, rows = row
    oy, ox = T.tap_origin(row)
    w, g, seed = T.tap_inputs(row)
    emb, ext = (lib.vts_tap_embed, lib.vts_tap_extract) if entry == "ab" else (lib.vts_tap_embed_at, lib.vts_tap_extract_at)
    wo, w4 = Op(w.shape, w), Op((rows, 4, 4))
    judge(gpu, rid + "-embed", "tap_embed_kernel", lambda: L.check(emb(wo.t.data_ptr(), rows, k, p, q, w4.t.data_ptr(), L.stream()), "tap_embed"),
          [wo, w4], [(w4, None, R.tap_embed(w, k, oy, ox), None, "exact")])
    for acc in (False, True):
        res = R.tap_extract(g, k, oy, ox, seed if acc else None)
        own = res["own"]
        init = torch.where(own, seed, torch.full_like(seed, float("nan"))) if acc else None
        go, dw = Op(g.shape, g), Op((rows, k, k), init)
        idx = (slice(None), own)
        outs = [(dw, idx, res["dw"][0][idx], None, "exact")] if bool(own.any()) else []
        judge(gpu, "%s-extract-%s" % (rid, "acc" if acc else "plain"), "tap_extract_kernel",
              lambda: L.check(ext(go.t.data_ptr(), rows, k, p, q, dw.t.data_ptr(), int(acc), L.stream()), "tap_extract"), [go, dw], outs)


# ---------------------------------------------------------------------------------------------------------------- table resampling
def _table_ops(tab):
    mins, sizes, w = [torch.from_numpy(a) for a in tab]
    return [Op(mins.shape, mins, dtype=torch.int32), Op(sizes.shape, sizes, dtype=torch.int32), Op(w.shape, w)]


def _resample_call(lib, L, src, nc, ih, iw, ty, tx, dst, oh, ow, acc):
    return lambda: L.check(lib.vts_resample_table(src.t.data_ptr(), nc, ih, iw, ty[0].t.data_ptr(), ty[1].t.data_ptr(), ty[2].t.data_ptr(), ty[2].shape[1],
                                                  tx[0].t.data_ptr(), tx[1].t.data_ptr(), tx[2].t.data_ptr(), tx[2].shape[1], dst.t.data_ptr(), oh, ow,
                                                  int(acc), L.stream()), "vts_resample_table")


@pytest.mark.parametrize("row", T.RESAMPLE, ids=ids(T.RESAMPLE))
@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc"])
def test_resample_table_and_its_adjoint(gpu, row, acc):
    lib, ops, L = gpu
    rid, nc, ih, iw, oh, ow = row
    ay, ax = ops._aa_axis(ih, oh), ops._aa_axis(iw, ow)
    x, g = detrand.uniform((1, nc, ih, iw), 5250, rid), detrand.uniform((1, nc, oh, ow), 5250, rid + "g")
    seed_o, seed_i = detrand.uniform((1, nc, oh, ow), 5250, rid + "so"), detrand.uniform((1, nc, ih, iw), 5250, rid + "si")
    # forward
    xo, out, ty, tx = Op(x.shape, x), Op((1, nc, oh, ow), seed_o if acc else None), _table_ops(ay), _table_ops(ax)
    ref, unit = R.resample_table(x, ay, ax, seed_o if acc else None)["out"]
    identity = (ih, iw) == (oh, ow) and not acc
    if identity:
        assert torch.equal(ref, x.double())
    judge(gpu, "%s-%s" % (rid, "acc" if acc else "plain"), "resample_table_kernel", _resample_call(lib, L, xo, nc, ih, iw, ty, tx, out, oh, ow, acc),
          [xo, out] + ty + tx, [(out, None, x if identity else ref, None if identity else unit, "exact" if identity else "resample")])
    # adjoint: the same operator on the transposed tables
    by, bx = ops._aa_transpose(*ay, ih), ops._aa_transpose(*ax, iw)
    go, din, ty, tx = Op(g.shape, g), Op((1, nc, ih, iw), seed_i if acc else None), _table_ops(by), _table_ops(bx)
    ref, unit = R.resample_table(g, by, bx, seed_i if acc else None)["out"]
    fwd_t = torch.einsum("oh,ncop,pw->nchw", R.table_matrix(*ay, ih), g.double(), R.table_matrix(*ax, iw))
    assert float((fwd_t + (seed_i.double() if acc else 0) - ref).abs().max()) < 1e-12          # the transposed tables are the transposed operator
    judge(gpu, "%s-adjoint-%s" % (rid, "acc" if acc else "plain"), "resample_table_kernel", _resample_call(lib, L, go, nc, oh, ow, ty, tx, din, ih, iw, acc),
          [go, din] + ty + tx, [(din, None, ref, unit, "resample")])


# ---------------------------------------------------------------------------------------------------------------- upfirdn2d
@pytest.mark.parametrize("row", T.UFD, ids=ids(T.UFD))
@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc"])
def test_upfirdn2d_and_its_adjoint_both_instances(gpu, row, acc):
    lib, ops, L = gpu
    rid, nc, ih, iw, kname, up, down, padx, pady, exact, inst = row
    k = T.ufd_kernel(kname, up)
    kh, kw = k.shape
    karr = (C.c_float * (kh * kw))(*[float(v) for v in k.reshape(-1)])
    oh, ow = T.ufd_out_hw(row)
    assert (oh, ow) == (lib.vts_upfirdn2d_out_size(ih, kh, up, down, *pady), lib.vts_upfirdn2d_out_size(iw, kw, up, down, *padx))
    x, g = T.ufd_input(row, (1, nc, ih, iw), "x"), T.ufd_input(row, (1, nc, oh, ow), "g")
    so, si = T.ufd_input(row, (1, nc, oh, ow), "so"), T.ufd_input(row, (1, nc, ih, iw), "si")
    fam = "exact" if exact else "fir"
    xo, out = Op(x.shape, x), Op((1, nc, oh, ow), so if acc else None)
    ref, unit = R.upfirdn2d(x, k, up, down, padx, pady, so if acc else None)["out"]
    call = lambda: L.check(lib.vts_upfirdn2d(xo.t.data_ptr(), nc, ih, iw, karr, kh, kw, up, down, padx[0], padx[1], pady[0], pady[1], out.t.data_ptr(),
                                             int(acc), L.stream()), "vts_upfirdn2d")
    judge(gpu, "%s-%s" % (rid, "acc" if acc else "plain"), inst, call, [xo, out], [(out, None, ref, None if exact else unit, fam)])
    go, din = Op(g.shape, g), Op((1, nc, ih, iw), si if acc else None)
    ref, unit = R.upfirdn2d_bwd(g, (ih, iw), k, up, down, padx, pady, si if acc else None)["din"]
    call = lambda: L.check(lib.vts_upfirdn2d_bwd(go.t.data_ptr(), nc, ih, iw, karr, kh, kw, up, down, padx[0], padx[1], pady[0], pady[1],
                                                 din.t.data_ptr(), int(acc), L.stream()), "vts_upfirdn2d_bwd")
    judge(gpu, "%s-adjoint-%s" % (rid, "acc" if acc else "plain"), T.UFD_ADJOINT[inst], call, [go, din], [(din, None, ref, None if exact else unit, fam)])


# ---------------------------------------------------------------------------------------------------------------- bias + LeakyReLU + gain
@pytest.mark.parametrize("row", T.BIAS_ACT, ids=ids(T.BIAS_ACT))
def test_bias_act_and_its_derivative_with_exact_ties(gpu, row):
    """x + bias == 0: the forward gives exactly 0 (+ res), the backward takes the slope branch"""
    lib, ops, L = gpu
    rid, n, c, hw, has_b, has_r, slope, gain = row
    x, b, res, g, tie = T.bias_act_inputs(row)
    xo, bo, ro, go, out, dx = Op(x.shape, x), opt(b), opt(res), Op(g.shape, g), Op(x.shape), Op(x.shape)
    ref, unit = R.bias_act(x, b, res, slope, gain)["out"]
    assert torch.equal(ref[tie], res.double()[tie] if has_r else torch.zeros(int(tie.sum()), dtype=torch.float64))
    judge(gpu, rid, "bias_act_kernel",
          lambda: L.check(lib.vts_bias_act(xo.t.data_ptr(), dptr(bo), dptr(ro), n, c, hw, slope, gain, out.t.data_ptr(), L.stream()), "vts_bias_act"),
          some(xo, bo, ro, out), [(out, None, ref, unit, "bias_act")])
    ref, unit = R.bias_act_bwd(g, x, b, slope, gain)["dx"]
    assert torch.equal(ref[tie], g.double()[tie] * R._f32(slope) * R._f32(gain))
    judge(gpu, rid + "-bwd", "bias_act_bwd_kernel",
          lambda: L.check(lib.vts_bias_act_bwd(go.t.data_ptr(), xo.t.data_ptr(), dptr(bo), n, c, hw, slope, gain, dx.t.data_ptr(), L.stream()),
                          "vts_bias_act_bwd"), some(go, xo, bo, dx), [(dx, None, ref, unit, "bias_act")])


# ---------------------------------------------------------------------------------------------------------------- nearest
@pytest.mark.parametrize("row", T.NEAREST, ids=ids(T.NEAREST))
def test_nearest_resize_and_adjoint_follow_the_float_rule_bitwise(gpu, row):
    """sources that no output reads get a gradient of exactly 0 (plain), keep their seed (accumulate)"""
    lib, ops, L = gpu
    rid, nc, ih, iw, oh, ow = row
    x, g, seed = T.nearest_inputs(row)
    xo, out = Op(x.shape, x), Op((1, nc, oh, ow))
    judge(gpu, rid, "nearest_fwd_kernel",
          lambda: L.check(lib.vts_nearest_resize(xo.t.data_ptr(), nc, ih, iw, oh, ow, out.t.data_ptr(), L.stream()), "vts_nearest_resize"),
          [xo, out], [(out, None, R.nearest_resize(x, (oh, ow)), None, "exact")])
    for acc in (False, True):
        go, din = Op(g.shape, g), Op(x.shape, seed if acc else None)
        ref, _ = R.nearest_resize_bwd(g, (ih, iw), seed if acc else None)["din"]
        if "skip" in rid:
            unread = torch.ones(ih, iw, dtype=torch.bool)
            unread[R.nearest_index(ih, oh)[:, None], R.nearest_index(iw, ow)[None, :]] = False
            assert int(unread.sum()) == ih * iw - oh * ow and torch.equal(ref[0, :, unread], seed.double()[0, :, unread] if acc else torch.zeros(nc, int(unread.sum()), dtype=torch.float64))
        judge(gpu, "%s-bwd-%s" % (rid, "acc" if acc else "plain"), "nearest_bwd_kernel",
              lambda: L.check(lib.vts_nearest_resize_bwd(go.t.data_ptr(), nc, ih, iw, oh, ow, din.t.data_ptr(), int(acc), L.stream()),
                              "vts_nearest_resize_bwd"), [go, din], [(din, None, ref, None, "exact")])


@pytest.mark.parametrize("row", T.UP2, ids=ids(T.UP2))
def test_nearest_up2_and_adjoint_bitwise(gpu, row):
    lib, ops, L = gpu
    rid, nc, h, w = row
    x, g, seed = T.up2_inputs(row)
    xo, out = Op(x.shape, x), Op((1, nc, 2 * h, 2 * w))
    assert out.t.data_ptr() % 8 == 0
    judge(gpu, rid, "nearest_up2_kernel", lambda: L.check(lib.vts_nearest_up2(xo.t.data_ptr(), nc, h, w, out.t.data_ptr(), L.stream()), "vts_nearest_up2"),
          [xo, out], [(out, None, R.nearest_up2(x), None, "exact")])
    for acc in (False, True):
        go, din = Op(g.shape, g), Op(x.shape, seed if acc else None)
        ref, _ = R.nearest_up2_bwd(g, seed if acc else None)["din"]
        judge(gpu, "%s-bwd-%s" % (rid, "acc" if acc else "plain"), "nearest_up2_bwd_kernel",
              lambda: L.check(lib.vts_nearest_up2_bwd(go.t.data_ptr(), nc, h, w, din.t.data_ptr(), int(acc), L.stream()), "vts_nearest_up2_bwd"),
              [go, din], [(din, None, ref, None, "exact")])


@pytest.mark.parametrize("n", T.TANH_BWD)
def test_tanh_bwd_three_roundings(gpu, n):
    lib, ops, L = gpu
    g, y = detrand.uniform((n,), 5700, "g"), torch.tanh(detrand.uniform((n,), 5700, "z") * 3)
    go, yo, dz = Op((n,), g), Op((n,), y), Op((n,))
    ref, unit = R.tanh_bwd(g, y)["dz"]
    judge(gpu, "tanh-bwd-%d" % n, "tanh_bwd_kernel", lambda: L.check(lib.vts_tanh_bwd(go.t.data_ptr(), yo.t.data_ptr(), n, dz.t.data_ptr(), L.stream()), "vts_tanh_bwd"),
          [go, yo, dz], [(dz, None, ref, unit, "tanh_bwd")])


# ---------------------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_refuse_without_launching(gpu):
    """through the return code alone: a float2 base off an 8-byte boundary, a reflect pad as large as the image"""
    lib, ops, L = gpu
    x, big = Op((1, 1, 2, 2), torch.zeros(1, 1, 2, 2)), Op((1, 1, 4, 4), torch.zeros(1, 1, 4, 4), offset=1)
    assert x.t.data_ptr() % 8 == 0 and big.t.data_ptr() % 8 == 4
    before = [x.dev.clone(), big.dev.clone()]
    rcs = [lib.vts_nearest_up2(x.t.data_ptr(), 1, 2, 2, big.t.data_ptr(), L.stream()),
           lib.vts_nearest_up2_bwd(big.t.data_ptr(), 1, 2, 2, x.t.data_ptr(), 0, L.stream()),
           lib.vts_pad_bwd(big.t.data_ptr(), 1, 1, 2, 2, 1, 1, 2, 0, T.REFLECT, x.t.data_ptr(), 0, L.stream()),       # pl = W
           lib.vts_pad_bwd(big.t.data_ptr(), 1, 1, 2, 2, 0, 2, 1, 1, T.REFLECT, x.t.data_ptr(), 0, L.stream())]       # pb = H
    torch.cuda.synchronize()
    assert rcs == [-1] * 4, rcs                               # VTS_ERR_ARG
    assert b"reflect pad" in lib.vts_last_error()
    assert torch.equal(bits(x.dev), bits(before[0])) and torch.equal(bits(big.dev), bits(before[1]))
    # the same calls with legal arguments pass
    ok = Op((1, 1, 4, 4))
    L.check(lib.vts_nearest_up2(x.t.data_ptr(), 1, 2, 2, ok.t.data_ptr(), L.stream()), "vts_nearest_up2")
    L.check(lib.vts_pad_bwd(ok.t.data_ptr(), 1, 1, 2, 2, 1, 1, 1, 1, T.REFLECT, x.t.data_ptr(), 0, L.stream()), "vts_pad_bwd")
    torch.cuda.synchronize()
