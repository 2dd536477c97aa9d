"""The fp32 glue kernels of the perceptual terms (csrc/vts_perceptual.hip) and vts_zero_border against the float64 and exact judges of
oracle/launch_ref.py, elementwise, on the hand-built table tests/perceptual_glue_cases.py (the smallest shapes that reach each dispatch
alternative, each 65535-plane chunk, each second grid sweep and each planted tie).

Operands, guard bands and the per-call assertions are those of tests/judge_harness.py: the expected kernel instance
(lib.vts_last_kernel()), |got - ref| <= 1.01 unit at every element of an arithmetic output -- the unit is a derived worst-case rounding
count, the 1 % covers second-order terms -- or bitwise equality for the data-movement, mask and routing rows, loss slots from seeded starts
as (slot - start) / 2^40, every element the call does not own bitwise unchanged (guard bands, inputs, the borders of zpad-padded operands,
the border of dz0, gaps between strided samples, the interior of vts_zero_border's buffer), and a second identical call bitwise identical.
The border of a padded z holds a large positive value (a read of it would win a maximum and open a mask), that of a padded tap gradient NaN.
The module prints the worst err / unit per kernel instance and family (pytest -s); profiles/r20_perceptual_glue_parity.txt is that table
from the MI355X."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import perceptual_glue_cases as T
from judge_harness import Op, bits, judge as _judge
from oracle import launch_ref as R

pytestmark = pytest.mark.gpu

BOUND = 1.01         # every arithmetic row; a kernel that needs more is a finding, not a reason for a larger constant
WORST = {}
Z_BORDER = 777.0


@pytest.fixture(scope="module")
def gpu():
    from vts import lib as L
    lib = L.load()
    yield lib, L
    if WORST:
        lines = ["# per kernel instance and family: worst err / unit over its rows vs float64 (oracle/launch_ref.py), bound %g for every family" % BOUND,
                 "# unit = (r + K) u absref, derived; loss slots: (K - 1) u sum |terms| + per-term roundings + 2^-41 per workgroup, the exact-sum",
                 "# rows 2^-41 per workgroup alone.  outputs = judged outputs of tests/perceptual_glue_cases.py; family 'exact': bitwise, all equal",
                 "%-9s %-12s %7s  %-32s %s" % ("worst", "family", "outputs", "instance", "at case")]
        for (inst, _), (w, case, fam, calls) in sorted(WORST.items(), key=lambda kv: (-kv[1][0], kv[0])):
            lines.append("%-9.4f %-12s %7d  %-32s %s" % (w, fam, calls, inst, case))
        print("\n[%s]\n%s" % (__name__, "\n".join(lines)))


def judge(gpu, tag, expected, call, opnds, outs):
    _judge(gpu[0], tag, expected, call, [o for o in opnds if o is not None], outs, BOUND, WORST, per_family=True)


def ids(rows):
    return [r[0] for r in rows]


def padded(t, zpad, border):
    """the dense interior inside a border of `zpad` elements holding `border`"""
    return F.pad(t, (zpad,) * 4, value=border) if zpad else t


def interior(ndim, pad, h, w):
    return None if pad == 0 else (slice(None),) * (ndim - 2) + (slice(pad, pad + h), slice(pad, pad + w))


def dptr(o):
    return None if o is None else o.t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------- pooling, space-to-depth
@pytest.mark.parametrize("row", T.MP2, ids=ids(T.MP2))
def test_maxpool2_relu_pad_bitwise(gpu, row):
    lib, L = gpu
    rid, nc, h, w, pad, zpad = row
    z = T.pool_input(row, 2)
    zo, out = Op((nc, h + 2 * zpad, w + 2 * zpad), padded(z, zpad, Z_BORDER)), Op((nc, h // 2 + 2 * pad, w // 2 + 2 * pad))
    call = lambda: L.check(lib.vts_maxpool2_relu_pad(zo.t.data_ptr(), nc, h, w, pad, out.t.data_ptr(), zpad, L.stream()), rid)
    judge(gpu, rid, "maxpool2_relu_pad_kernel", call, [zo, out], [(out, None, R.maxpool2_relu_pad(z, pad)["out"][0], None, "exact")])


@pytest.mark.parametrize("row", T.MP3, ids=ids(T.MP3))
def test_maxpool3s2_relu_pad_bitwise(gpu, row):
    lib, L = gpu
    rid, nc, h, w, pad = row
    z = T.pool_input(row, 3)
    zo, out = Op(z.shape, z), Op((nc, (h - 3) // 2 + 1 + 2 * pad, (w - 3) // 2 + 1 + 2 * pad))
    call = lambda: L.check(lib.vts_maxpool3s2_relu_pad(zo.t.data_ptr(), nc, h, w, pad, out.t.data_ptr(), L.stream()), rid)
    judge(gpu, rid, "maxpool3s2_relu_pad_kernel", call, [zo, out], [(out, None, R.maxpool3s2_relu_pad(z, pad)["out"][0], None, "exact")])


@pytest.mark.parametrize("row", T.S2D, ids=ids(T.S2D))
def test_s2d4_pad_bitwise(gpu, row):
    lib, L = gpu
    rid, n, c, h, w, pad, oh, ow = row
    x = T.dyadic((n, c, h, w), 7050, rid)
    xo, out = Op(x.shape, x), Op((n, 16 * c, oh, ow))
    call = lambda: L.check(lib.vts_s2d4_pad(xo.t.data_ptr(), n, c, h, w, pad, oh, ow, out.t.data_ptr(), L.stream()), rid)
    judge(gpu, rid, "s2d4_pad_kernel", call, [xo, out], [(out, None, R.s2d4_pad(x, pad, oh, ow)["out"][0], None, "exact")])


# ---------------------------------------------------------------------------------------------------------------- adjoints and masks
@pytest.mark.parametrize("row", T.MPB, ids=ids(T.MPB))
def test_maxpool2_relu_bwd_both_instances_bitwise(gpu, row):
    """the routed gradient goes to the first maximum of a window, nowhere when that maximum is not positive; the tap is added where z > 0
    (not at 0.0 or -0.0); the zero border of the result is written in full, whatever the number of window rows and columns"""
    lib, L = gpu
    rid, nc, h, w, pad, zpad, tap, inst = row
    g, z, t, _ = T.mpb_inputs(row)
    go, zo = Op(g.shape, g), Op((nc, h + 2 * zpad, w + 2 * zpad), padded(z, zpad, Z_BORDER))
    to = Op(zo.shape, padded(t, zpad, float("nan"))) if tap else None
    out = Op((nc, h + 2 * pad, w + 2 * pad))
    call = lambda: L.check(lib.vts_maxpool2_relu_bwd(go.t.data_ptr(), zo.t.data_ptr(), nc, h, w, out.t.data_ptr(), zpad, dptr(to), pad, L.stream()), rid)
    judge(gpu, rid, inst, call, [go, zo, to, out], [(out, None, R.maxpool2_relu_bwd(g, z, t, pad)["gz"][0], None, "exact")])


@pytest.mark.parametrize("row", T.RMP, ids=ids(T.RMP))
def test_relu_mask_pad_bitwise(gpu, row):
    lib, L = gpu
    rid, nc, h, w, pad, zpad, _ = row
    g, g2, z = T.rmp_inputs(row)
    zo = Op((nc, h + 2 * zpad, w + 2 * zpad), padded(z, zpad, Z_BORDER))
    go = Op(g.shape, g) if g is not None else None
    g2o = Op(zo.shape, padded(g2, zpad, float("nan"))) if g2 is not None else None
    out = Op((nc, h + 2 * pad, w + 2 * pad))
    call = lambda: L.check(lib.vts_relu_mask_pad(dptr(go), dptr(g2o), zo.t.data_ptr(), nc, h, w, pad, out.t.data_ptr(), zpad, L.stream()), rid)
    judge(gpu, rid, "relu_mask_pad_kernel", call, [go, g2o, zo, out], [(out, None, R.relu_mask_pad(g, g2, z, pad)["out"][0], None, "exact")])


@pytest.mark.parametrize("row", T.ZB, ids=ids(T.ZB))
def test_zero_border_owns_the_border_alone(gpu, row):
    lib, L = gpu
    rid, nc, h, w, pad = row
    buf = T.zb_input(row)
    res = R.zero_border(buf, pad)
    bo = Op(buf.shape, buf)
    idx = (slice(None), res["own"])
    call = lambda: L.check(lib.vts_zero_border(bo.t.data_ptr(), nc, h, w, pad, L.stream()), rid)
    judge(gpu, rid, "zero_border_kernel", call, [bo], [(bo, idx, res["buf"][0][idx], None, "exact")])


# ---------------------------------------------------------------------------------------------------------------- the LPIPS head, ReLU-L1
@pytest.mark.parametrize("row", T.LPL, ids=ids(T.LPL))
def test_lpips_layer_all_five_instances(gpu, row):
    """value into a seeded slot and gradient in z0's layout; with zpad the border of dz0 keeps its fill"""
    lib, L = gpu
    rid, n, c, h, w, zpad, variant, seed, inst, exact = row
    z0, z1, wl, _ = T.lpl_inputs(row)
    coeff, gc = T.lpl_coeffs(row)
    shape = (n, c, h + 2 * zpad, w + 2 * zpad)
    z0o, z1o, wo = Op(shape, padded(z0, zpad, Z_BORDER)), Op(shape, padded(z1, zpad, Z_BORDER)), Op(wl.shape, wl)
    slot, dz = Op((1,), torch.tensor([seed]), dtype=torch.int64), Op(shape)
    want_loss, want_grad = variant != "noloss", variant != "nograd"
    call = lambda: L.check(lib.vts_lpips_layer(z0o.t.data_ptr(), z1o.t.data_ptr(), n, c, h * w, wo.t.data_ptr(), coeff, dptr(slot) if want_loss else None,
                                               dptr(dz) if want_grad else None, gc, w, zpad, L.stream()), rid)
    ref = R.lpips_layer(z0, z1, wl, coeff, gc, T.lpl_workgroups(row), zpad == 0, exact_sum=exact)
    outs = []
    if want_loss:
        outs.append((slot, None, ref["loss"][0], ref["loss"][1], "loss_exact" if exact else "loss"))
    if want_grad:
        idx = interior(4, zpad, h, w)
        outs.append((dz, idx, ref["dz0"][0], ref["dz0"][1], "lpips_grad"))
    judge(gpu, "%s-z%d-%s-seed%+d" % (rid, zpad, variant, (seed > 0) - (seed < 0)), inst, call, [z0o, z1o, wo, slot, dz], outs)


@pytest.mark.parametrize("row", T.L1R, ids=ids(T.L1R))
def test_l1_relu_value_and_sign(gpu, row):
    lib, L = gpu
    rid, n, variant, seed, exact = row
    za, zb, _ = T.l1r_inputs(row)
    coeff = T.l1r_coeff(row)
    ao, bo, slot, go = Op((n,), za), Op((n,), zb), Op((1,), torch.tensor([seed]), dtype=torch.int64), Op((n,))
    want_loss, want_grad = variant != "noloss", variant != "nograd"
    call = lambda: L.check(lib.vts_l1_relu(ao.t.data_ptr(), bo.t.data_ptr(), n, coeff, dptr(slot) if want_loss else None,
                                           dptr(go) if want_grad else None, L.stream()), rid)
    ref = R.l1_relu(za, zb, coeff, T.l1r_workgroups(n), exact_sum=exact)
    outs = []
    if want_loss:
        outs.append((slot, None, ref["loss"][0], ref["loss"][1], "loss_exact" if exact else "loss"))
    if want_grad:
        outs.append((go, None, ref["grad"][0], None, "exact"))
    judge(gpu, rid, "l1_relu_kernel", call, [ao, bo, slot, go], outs)


# ---------------------------------------------------------------------------------------------------------------- input scaling, stacking
def _triple(v):
    return (C.c_float * 3)(*v)


@pytest.mark.parametrize("row", T.LIN, ids=ids(T.LIN))
def test_lpips_input_and_adjoint_dense_and_channel_slice(gpu, row):
    lib, L = gpu
    rid, n, cx, hw, layout = row
    x, g, seed = T.lin_inputs(row)
    ns, lead = ((cx + 2) * hw, hw) if layout == "slice" else (cx * hw, 0)
    sh, sc = _triple(T.LPIPS_SHIFT), _triple(T.LPIPS_SCALE)
    xo, y = Op(x.shape, x, ns=ns, lead=lead), Op((n, 3, hw))
    ref, unit = R.lpips_input(x, T.LPIPS_SHIFT, T.LPIPS_SCALE)["y"]
    judge(gpu, rid, "lpips_input_kernel", lambda: L.check(lib.vts_lpips_input(xo.t.data_ptr(), ns, n, cx, hw, sh, sc, y.t.data_ptr(), L.stream()), rid),
          [xo, y], [(y, None, ref, unit, "scale")])
    for acc in (False, True):
        go, dx = Op(g.shape, g), Op(x.shape, seed if acc else None, ns=ns, lead=lead)
        ref, unit = R.lpips_input_bwd(g, T.LPIPS_SCALE, cx, seed if acc else None)["dx"]
        judge(gpu, "%s-bwd-%s" % (rid, "acc" if acc else "plain"), "lpips_input_bwd_kernel",
              lambda: L.check(lib.vts_lpips_input_bwd(go.t.data_ptr(), n, cx, hw, sc, dx.t.data_ptr(), ns, int(acc), L.stream()), rid),
              [go, dx], [(dx, None, ref, unit, "scale_bwd")])


@pytest.mark.parametrize("row", T.VSI, ids=ids(T.VSI))
def test_vgg_stack_input_from_four_strided_sources_bitwise(gpu, row):
    """every source is a channel view with a batch stride beyond what is read; the tactile tensors' third channel is NaN and unread"""
    lib, L = gpu
    rid, n, h, w = row
    hw = h * w
    imgs = [T.dyadic((n, 3, h, w), 7650, rid + k) for k in ("fI", "rI")]
    tacs = [T.dyadic((n, 2, h, w), 7650, rid + k) for k in ("fT", "rT")]
    fI, rI = [Op(t.shape, t, ns=3 * hw + 5, lead=2) for t in imgs]
    fT, rT = [Op(t.shape, t, ns=3 * hw + 3) for t in tacs]
    out = Op((6 * n, 3, h + 2, w + 2))
    call = lambda: L.check(lib.vts_vgg_stack_input(fI.t.data_ptr(), fI.ns, rI.t.data_ptr(), rI.ns, fT.t.data_ptr(), fT.ns, rT.t.data_ptr(), rT.ns,
                                                   n, h, w, out.t.data_ptr(), L.stream()), rid)
    judge(gpu, rid, "vgg_stack_input_kernel", call, [fI, rI, fT, rT, out],
          [(out, None, R.vgg_stack_input(imgs[0], imgs[1], tacs[0], tacs[1])["out"][0], None, "exact")])


@pytest.mark.parametrize("row", T.VSB, ids=ids(T.VSB))
@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc"])
def test_vgg_stack_input_bwd_float4_and_scalar_instances(gpu, row, acc):
    lib, L = gpu
    rid, n, h, w, why, inst = row
    hw = h * w
    nsI, nsT, off = T.vsb_layout(row)
    dx, sI, sT = T.vsb_inputs(row)
    dxo, dI, dT = Op(dx.shape, dx), Op((n, 3, hw), sI if acc else None, ns=nsI), Op((n, 2, hw), sT if acc else None, ns=nsT, offset=off)
    assert dxo.t.data_ptr() % 16 == 0 and dI.t.data_ptr() % 16 == 0 and dT.t.data_ptr() % 16 == 4 * off
    ref = R.vgg_stack_input_bwd(dx, n, sI if acc else None, sT if acc else None)
    call = lambda: L.check(lib.vts_vgg_stack_input_bwd(dxo.t.data_ptr(), n, h, w, dI.t.data_ptr(), nsI, dT.t.data_ptr(), nsT, int(acc), L.stream()), rid)
    judge(gpu, "%s-%s" % (rid, "acc" if acc else "plain"), inst, call, [dxo, dI, dT],
          [(dI, None, ref["dI"][0], ref["dI"][1], "stack_bwd"), (dT, None, ref["dT"][0], ref["dT"][1], "stack_bwd")])


# ---------------------------------------------------------------------------------------------------------------- graph replay
def test_captured_adjoint_mask_and_head_replay_bitwise_like_eager(gpu):
    """vts_maxpool2_relu_bwd, vts_relu_mask_pad and vts_lpips_layer on an 8 x 8, C = 64 map: captured once, replayed twice from reset
    outputs, each replay bitwise the eager result (the slot included: integer adds commute)"""
    lib, L = gpu
    n, c, h, w = 2, 64, 8, 8
    row = ("graph-8x8-c64", n * c, h, w, 1, 0, True, T.WIN)
    g, z, t, _ = [None if v is None else v.cuda() for v in T.mpb_inputs(row)]
    lrow = ("graph-8x8-c64-head", n, c, h, w, 0, "both", T.GAN_SEEDS[1], T.LPL_INSTANCE[64], False)
    z0, z1, wl, _ = [v.cuda() for v in T.lpl_inputs(lrow)]
    gz, mk, dz = [torch.empty(s, device="cuda") for s in ((n * c, h + 2, w + 2), (n * c, h + 2, w + 2), (n, c, h, w))]
    slot = torch.empty(1, dtype=torch.int64, device="cuda")

    def reset():
        for o in (gz, mk, dz):
            o.fill_(float("nan"))
        slot.fill_(T.GAN_SEEDS[1])

    def run():
        L.check(lib.vts_maxpool2_relu_bwd(g.data_ptr(), z.data_ptr(), n * c, h, w, gz.data_ptr(), 0, t.data_ptr(), 1, L.stream()), "bwd")
        L.check(lib.vts_relu_mask_pad(None, t.data_ptr(), z.data_ptr(), n * c, h, w, 1, mk.data_ptr(), 0, L.stream()), "mask")
        L.check(lib.vts_lpips_layer(z0.data_ptr(), z1.data_ptr(), n, c, h * w, wl.data_ptr(), T.LPL_COEFF, slot.data_ptr(), dz.data_ptr(), T.LPL_GCOEFF, w, 0,
                                    L.stream()), "head")

    reset()
    run()
    torch.cuda.synchronize()
    eager = [o.clone() for o in (gz, mk, dz, slot)]
    assert not any(bool(torch.isnan(o).any()) for o in eager[:3]) and int(eager[3]) != T.GAN_SEEDS[1]
    graph = torch.cuda.CUDAGraph()
    reset()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        reset()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((gz, mk, dz, slot), eager):
            assert torch.equal(bits(got), bits(want))
