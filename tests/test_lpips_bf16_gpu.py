"""The bf16 path of the frozen LPIPS-VGG16 stack (--lpips_dtype bf16; csrc/vts_conv3x3_bf16.hip) on the GPU.

Per launch, elementwise against float64 of the SAME bf16-exact operands, inside the guard bands of tests/judge_harness.py (bf16 buffers are
kept as int16 bit patterns there; their fill is the bf16 NaN 0x7FC0).  Bounds are derived, not measured:
    fp32 result      |acc - y64| <= (9 Cin + 2) 2^-24 absref,  absref = sum |x w| + |bias| (+ |add|)   (bf16 products are exact in fp32)
    bf16 result      + 2^-8 |y64| for the store
    LPIPS head       tests/lpips_bf16_ref.py:lpips_layer_judge (a linear rounding count, derived there), + 2^-8 |dz0| for the bf16 store
    pooling, its adjoint, the weight packing, integer cases, every zero border: bitwise
The worst ratio of every case is printed and must be <= 1.

Whole term: relative L2 of the value and of d/d fake against the plain float64 oracle, e_hip <= 2 e_ideal where e_ideal is that of the
ideal bf16 run (tests/lpips_bf16_ref.py:lpips_run with q = rt_bf16: the same quantities rounded at the same places; the kernel's fp32
sums can move a rounding by one bf16 ulp, a second error of equal size)."""
import pytest
import torch

from oracle import perceptual as chk
from tests import judge_harness as H
from tests import lpips_bf16_ref as R

pytestmark = pytest.mark.gpu

H.FILL.setdefault(torch.int16, R.BF16_NAN_BITS)          # bf16 buffers as bit patterns: NaN-filled bands compare bitwise

def kname(ep, h, w):
    """the instance vts_conv3x3_bf16 takes: maps of at most 256 pixels whose padded form fits 576 run whole images flattened into the tile"""
    flat = h * w <= 256 and (h + 2) * (w + 2) <= 576
    return "conv3x3_bf16_kernel<%s%s>" % ({"relu": "relu_pad", "mask": "mask_pad", "dx": "dx_f32"}[ep], ", flat" if flat else "")


def _lib():
    from vts import lib as L

    return L.load()


def bf(op):
    """the bf16 view of an int16 operand"""
    return op.t.view(torch.bfloat16)


def run_checked(tag, expected, call, opnds, outs):
    """two runs from identical state: the kernel instance, bitwise repeatability, nothing outside `outs` touched.  Returns the host
    snapshots of `outs` after the first run."""
    (kern, snap), (kern2, snap2) = H.execute(_lib(), call, opnds)
    assert kern == expected and kern2 == expected, "%s: ran %s, expected %s" % (tag, kern, expected)
    res = []
    for o, s, s2 in zip(opnds, snap, snap2):
        assert torch.equal(H.bits(s), H.bits(s2)), "%s: a second identical call is not bitwise identical" % tag
        mine = any(o is p for p in outs)
        keep = ~o.owned([None] if mine else [])
        assert torch.equal(H.bits(s)[keep], H.bits(o.host)[keep]), "%s: an element outside the outputs changed (guard band or input)" % tag
    for p in outs:
        res.append(p.content(snap[[o is p for o in opnds].index(True)]))
    return res


def rnd(shape, g, scale=1.0):
    return R.rt_bf16(scale * torch.randn(shape, generator=g, dtype=torch.float64))


def judge_padded(tag, got_bits, ref, bound32):
    """got_bits int16 [N, H + 2, W + 2, C]; ref / bound32 [N, C, H, W] float64"""
    got = got_bits.clone()
    border = torch.ones(got.shape[1:3], dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert bool((got[:, border, :] == 0).all()), "%s: the zero border is not bitwise zero" % tag
    g = R.interior_nchw(R.from_bits(got))
    bound = torch.where(bound32 > 0, bound32 + R.UB * ref.abs(), torch.zeros_like(ref))
    r = R.ratio(g, ref, bound)
    print("%-34s %-44s worst ratio %.4f" % (tag.split()[0], tag, r))
    assert r <= 1.0, (tag, r)
    return r


def conv_case(n, ci, co, h, w, eps=("relu", "mask", "dx"), mask_kind="random", integer=False, co_store=None, seed=0):
    from vts import ops

    g = torch.Generator().manual_seed(seed * 7919 + ci * 31 + co * 17 + h * 5 + w + n)
    if integer:                                   # operands in {-1, 0, 1}, sparse: every sum is an integer of magnitude <= 256, exact in bf16
        def tern(shape, p):
            return ((torch.rand(shape, generator=g) < p).double() * (torch.randint(0, 2, shape, generator=g) * 2 - 1).double())
        x, wt, bias, add = tern((n, ci, h, w), 0.25), tern((co, ci, 3, 3), 0.25), tern((co,), 0.5), tern((n, co, h, w), 0.5)
    else:
        x, wt = rnd((n, ci, h, w), g), rnd((co, ci, 3, 3), g, (2.0 / (9 * ci)) ** 0.5)
        bias, add = 0.1 * torch.randn(co, generator=g, dtype=torch.float64).float().double(), rnd((n, co, h, w), g, 0.5)
    mask = R.rt_bf16(torch.rand((n, co, h, w), generator=g, dtype=torch.float64))
    if mask_kind == "random":
        mask = mask * (torch.rand((n, co, h, w), generator=g) < 0.6)
    elif mask_kind == "zero_tile":                # zero on the whole first tile (8 rows x 32 columns of every channel), positive elsewhere
        mask = mask + 2.0 ** -7
        mask[:, :, :8, :32] = 0
    else:
        assert mask_kind == "nowhere_zero"
        mask = mask + 2.0 ** -7
    mask = R.rt_bf16(mask)
    dev = torch.device("cuda:0")
    w32 = wt.float().to(dev)
    xin = H.Op((n, h + 2, w + 2, ci), init=R.to_bits(R.nhwc_pad(x)), dtype=torch.int16)
    worst = {}
    for ep in eps:
        tag = "%s N%d %d->%d %dx%d%s%s" % (ep, n, ci, co, h, w, " int" if integer else "", "" if mask_kind == "random" else " " + mask_kind)
        if ep == "relu":
            pk = ops.w3x3_bf16_pack(w32, "conv_fwd")
            b32 = bias.float().to(dev)
            out = H.Op((n, h + 2, w + 2, co), dtype=torch.int16)
            (got,) = run_checked(tag, kname(ep, h, w), lambda: ops.conv3x3_bf16(bf(xin), pk, b32, bf(out), ops.EP_BF16_RELU_PAD), [xin, out], [out])
            y, b = R.conv_judge(x, wt, bias=bias)
            ref = y.clamp_min(0)
        elif ep == "mask":
            # the input adjoint's packing: the kernel convolves with w'[ci_out][co_in] = w[co_in][ci_out] flipped, so pack the weight whose
            # ADJOINT is the convolution under test
            wadj = wt.flip(2, 3).transpose(0, 1).contiguous()             # [ci, co, 3, 3]: conv_adj of it is the convolution with wt
            pk = ops.w3x3_bf16_pack(wadj.float().to(dev), "conv_adj")
            madd = H.Op((n, h + 2, w + 2, co), init=R.to_bits(R.nhwc_pad(add)), dtype=torch.int16)
            mmask = H.Op((n, h + 2, w + 2, co), init=R.to_bits(R.nhwc_pad(mask)), dtype=torch.int16)
            out = H.Op((n, h + 2, w + 2, co), dtype=torch.int16)
            (got,) = run_checked(tag, kname(ep, h, w), lambda: ops.conv3x3_bf16(bf(xin), pk, None, bf(out), ops.EP_BF16_MASK_PAD, add=bf(madd), mask=bf(mmask)),
                                 [xin, madd, mmask, out], [out])
            y, b = R.conv_judge(x, wt, add=add)
            ref, b = torch.where(mask > 0, y, torch.zeros_like(y)), torch.where(mask > 0, b, torch.zeros_like(b))
        else:
            cs = co if co_store is None else co_store
            pk = ops.w3x3_bf16_pack(w32[:cs].contiguous(), "conv_fwd") if cs != co else ops.w3x3_bf16_pack(w32, "conv_fwd")
            out = H.Op((n, cs, h, w), dtype=torch.float32)
            (got,) = run_checked(tag, kname(ep, h, w), lambda: ops.conv3x3_bf16(bf(xin), pk, None, out.t, ops.EP_BF16_DX), [xin, out], [out])
            y, b = R.conv_judge(x, wt[:cs])
            if integer:
                assert float(y.abs().max()) <= 256
                assert torch.equal(got.view(torch.int32), y.float().view(torch.int32)), tag + ": not bitwise"
            r = R.ratio(got, y, b)
            print("%-34s %-44s worst ratio %.4f" % (tag.split()[0], tag, r))
            assert r <= 1.0, (tag, r)
            worst[ep] = r
            continue
        if integer:
            assert float(ref.abs().max()) <= 256
            assert torch.equal(got, R.to_bits(R.nhwc_pad(ref))), tag + ": not bitwise"
        worst[ep] = judge_padded(tag, got, ref, b)
    return worst


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", [(4, 4), (18, 10), (34, 34)])
@pytest.mark.parametrize("ci,co", [(64, 64), (64, 128), (128, 64), (256, 256)])
def test_conv_every_epilogue_against_float64(ci, co, h, w, n):
    conv_case(n, ci, co, h, w)


@pytest.mark.parametrize("n,h,w", [(3, 18, 40), (2, 16, 16), (2, 16, 17), (5, 8, 8), (40, 2, 2), (3, 6, 10), (1, 1, 1), (2, 1, 300)])
def test_conv_tiled_edges_and_the_flat_threshold(n, h, w):
    """18 x 40: the tiled kernel with edge tiles in both dimensions and H != W (18 x 10 above runs flattened); 16 x 16 | 16 x 17: either side
    of the 256-pixel threshold; 8 x 8 with 5 images: four images per workgroup, the last group short; 2 x 2 with 40: 36 per workgroup
    (the padded maps fill the staged 576 pixels first); 6 x 10: more room than images; 1 x 1; 1 x 300: ten tile columns of one row"""
    assert not kname("relu", 18, 40).endswith("flat>") and kname("relu", 16, 16).endswith("flat>")
    assert not kname("relu", 16, 17).endswith("flat>") and kname("relu", 18, 10).endswith("flat>")
    conv_case(n, 64, 64, h, w)


def test_conv_long_k():
    conv_case(1, 512, 512, 4, 4)
    conv_case(3, 512, 512, 4, 4, eps=("mask",))


@pytest.mark.parametrize("kind", ["zero_tile", "nowhere_zero"])
def test_conv_mask_extremes(kind):
    conv_case(3, 64, 64, 18, 10, eps=("mask",), mask_kind=kind)
    conv_case(1, 128, 64, 34, 34, eps=("mask",), mask_kind=kind)


def test_conv_integer_cases_are_bitwise():
    conv_case(3, 64, 128, 18, 10, integer=True)
    conv_case(1, 128, 64, 34, 34, integer=True)
    conv_case(20, 64, 64, 4, 4, integer=True)


def test_conv_first_layer_adjoint_stores_three_channels():
    """the stem's input adjoint: weights packed with 3 output channels (padded to 32), dense fp32 [N, 3, H, W]"""
    conv_case(3, 64, 32, 18, 10, eps=("dx",), co_store=3)
    conv_case(1, 64, 32, 34, 34, eps=("dx",), co_store=3, integer=True)


def test_stem_operand_and_padded_input_channels():
    """vts_bf16_nhwc_pad (bitwise) and the stem as the kernel sees it: 3 channels padded to 32 zero-filled ones"""
    from vts import ops

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    n, h, w = 3, 18, 10
    x = torch.randn((n, 3, h, w), generator=g)
    src = H.Op((n, 3, h, w), init=x)
    out = H.Op((n, h + 2, w + 2, 32), dtype=torch.int16)
    lib = _lib()
    (got,) = run_checked("nhwc_pad", "bf16_nhwc_pad_kernel",
                         lambda: ops.L.check(lib.vts_bf16_nhwc_pad(src.t.data_ptr(), n, 3, h, w, 32, out.t.data_ptr(), ops.L.stream()), "nhwc_pad"),
                         [src, out], [out])
    xq = R.rt_bf16(x.double())
    want = torch.zeros(n, h + 2, w + 2, 32, dtype=torch.float64)
    want[:, 1:-1, 1:-1, :3] = xq.permute(0, 2, 3, 1)
    assert torch.equal(got, R.to_bits(want))
    wt = rnd((64, 3, 3, 3), g, (2.0 / 27) ** 0.5)
    bias = 0.1 * torch.randn(64, generator=g).double()
    pk = ops.w3x3_bf16_pack(wt.float().to(dev), "conv_fwd")
    xin = H.Op((n, h + 2, w + 2, 32), init=got, dtype=torch.int16)
    o2 = H.Op((n, h + 2, w + 2, 64), dtype=torch.int16)
    b32 = bias.float().to(dev)
    (got2,) = run_checked("stem", kname("relu", h, w), lambda: ops.conv3x3_bf16(bf(xin), pk, b32, bf(o2), ops.EP_BF16_RELU_PAD), [xin, o2], [o2])
    y, b = R.conv_judge(xq, wt, bias=bias)
    judge_padded("stem N3 3(32)->64 18x10", got2, y.clamp_min(0), (9 * 32 + 2) / (9 * 3 + 2) * b)


def test_weight_packing_is_bitwise():
    from vts import ops

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    for co, ci in ((64, 3), (96, 64), (128, 64)):
        w = torch.randn((co, ci, 3, 3), generator=g)
        wq = R.rt_bf16(w.double())
        for mode in ("conv_fwd", "conv_adj"):
            A, B = (ci, co) if mode == "conv_fwd" else (co, ci)
            AP, BP = (A + 31) // 32 * 32, (B + 63) // 64 * 64
            want = torch.zeros(9, AP // 32, BP, 32, dtype=torch.float64)
            for t in range(9):
                src = wq.reshape(co, ci, 9)[:, :, t if mode == "conv_fwd" else 8 - t]           # [co, ci]
                m = src.t() if mode == "conv_fwd" else src                                        # [a, b]
                full = torch.zeros(AP, BP, dtype=torch.float64)
                full[:A, :B] = m
                want[t] = full.reshape(AP // 32, 32, BP).permute(0, 2, 1)
            got = ops.w3x3_bf16_pack(w.to(dev), mode).cpu()
            assert got.numel() == 9 * AP * BP
            assert torch.equal(got.view(torch.int16), R.to_bits(want.reshape(-1))), (co, ci, mode)


def test_conv_declines_without_writing():
    from vts import lib as L

    lib = _lib()
    for n, ci, co in ((1, 3, 64), (1, 48, 64), (2, 64, 16)):
        assert lib.vts_conv3x3_bf16_ok(n, ci, co, 8, 8) == 0
        xin = H.Op((n, 10, 10, ci), init=torch.zeros(n, 10, 10, ci, dtype=torch.int16), dtype=torch.int16)
        wt = H.Op((9 * 64 * 64,), init=torch.zeros(9 * 64 * 64, dtype=torch.int16), dtype=torch.int16)
        out = H.Op((n, 10, 10, co), dtype=torch.int16)
        rc = lib.vts_conv3x3_bf16(xin.t.data_ptr(), wt.t.data_ptr(), None, out.t.data_ptr(), n, ci, co, 8, 8, 1, None, None, co, L.stream())
        torch.cuda.synchronize()
        assert rc == L.ERR_UNSUPPORTED
        assert torch.equal(out.dev.cpu(), out.host)
    assert lib.vts_conv3x3_bf16_ok(1, 64, 64, 8, 8) == 1 and lib.vts_conv3x3_bf16_ok(1, 32, 32, 1, 1) == 1


# ---- pooling, its adjoint, the LPIPS head -----------------------------------------------------------------------------------------------------
def _relu_grid(shape, g, step=0.25):
    """ReLU-like data on a coarse grid: many zeros, many ties inside a window"""
    return (torch.randint(-4, 6, shape, generator=g).double() * step).clamp_min(0)


@pytest.mark.parametrize("h,w", [(6, 10), (32, 32), (7, 5)])
@pytest.mark.parametrize("c", [64, 512])
def test_pooling_and_its_adjoint_are_bitwise(c, h, w):
    import torch.nn.functional as F
    from vts import ops

    g = torch.Generator().manual_seed(c + h)
    n = 2
    z = _relu_grid((n, c, h, w), g)
    zin = H.Op((n, h + 2, w + 2, c), init=R.to_bits(R.nhwc_pad(z)), dtype=torch.int16)
    oh, ow = h // 2, w // 2
    out = H.Op((n, oh + 2, ow + 2, c), dtype=torch.int16)
    lib = _lib()
    L = ops.L

    (got,) = run_checked("pool", "maxpool2_bf16_kernel",
                         lambda: L.check(lib.vts_maxpool2_bf16(zin.t.data_ptr(), n, c, h, w, out.t.data_ptr(), L.stream()), "pool"), [zin, out], [out])
    assert torch.equal(got, R.to_bits(R.nhwc_pad(F.max_pool2d(z, 2, 2))))
    # adjoint: gradients on a 2^-6 grid (sums of two are exact in fp32, so the one bf16 rounding is the reference's)
    gp = torch.randint(-64, 64, (n, c, oh, ow), generator=g).double() * 2.0 ** -6
    t = torch.randint(-64, 64, (n, c, h, w), generator=g).double() * 2.0 ** -6
    _, ind = F.max_pool2d(z, 2, 2, return_indices=True)
    pooled = F.max_pool2d(z, 2, 2)
    routed = F.max_unpool2d(torch.where(pooled > 0, gp, torch.zeros_like(gp)), ind, 2, 2, output_size=(h, w))
    for use_t in (False, True):
        want = R.rt_bf16(routed + (torch.where(z > 0, t, torch.zeros_like(t)) if use_t else 0))
        gin = H.Op((n, oh + 2, ow + 2, c), init=R.to_bits(R.nhwc_pad(gp)), dtype=torch.int16)
        tin = H.Op((n, h + 2, w + 2, c), init=R.to_bits(R.nhwc_pad(t)), dtype=torch.int16)
        gz = H.Op((n, h + 2, w + 2, c), dtype=torch.int16)
        (got,) = run_checked("pool_bwd", "maxpool2_bf16_bwd_kernel",
                             lambda: L.check(lib.vts_maxpool2_bf16_bwd(gin.t.data_ptr(), zin.t.data_ptr(), tin.t.data_ptr() if use_t else None, n, c, h, w,
                                                                       gz.t.data_ptr(), L.stream()), "pool_bwd"), [gin, zin, tin, gz], [gz])
        assert torch.equal(got, R.to_bits(R.nhwc_pad(want))), (c, h, w, use_t)


@pytest.mark.parametrize("h,w", [(6, 10), (32, 32)])
@pytest.mark.parametrize("c", [64, 512])
def test_lpips_head_against_float64(c, h, w):
    from vts import ops

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(c * 3 + h)
    n = 2
    f0, f1 = rnd((n, c, h, w), g).clamp_min(0), rnd((n, c, h, w), g).clamp_min(0)
    f0[0, :, 0, 1] = 0                            # a pixel whose features all vanish: r = 0
    lin = (torch.rand(c, generator=g) * (2.0 / c)).float()
    coeff, gc = 0.7, 1.3
    a = H.Op((n, h + 2, w + 2, c), init=R.to_bits(R.nhwc_pad(f0)), dtype=torch.int16)
    b = H.Op((n, h + 2, w + 2, c), init=R.to_bits(R.nhwc_pad(f1)), dtype=torch.int16)
    dz = H.Op((n, h + 2, w + 2, c), dtype=torch.int16)
    slot = H.Op((1,), init=torch.zeros(1, dtype=torch.int64), dtype=torch.int64)
    lw = lin.to(dev)
    lib = _lib()
    got_dz, got_slot = run_checked("lpips_head", "lpips_layer_bf16_kernel<%d>" % c,
                                   lambda: ops.lpips_layer_bf16(bf(a), bf(b), lw, coeff, slot.t, dz0=bf(dz), grad_coeff=gc), [a, b, dz, slot], [dz, slot])
    value, vbound, ref, bound = R.lpips_layer_judge(f0, f1, lin.double(), float(torch.tensor(coeff).float()), float(torch.tensor(gc).float()))
    rv = abs(float(got_slot[0]) / H.LOSS_SCALE - float(value)) / float(vbound)
    print("lpips_head value C%d %dx%d worst ratio %.4f" % (c, h, w, rv))
    assert rv <= 1.0
    judge_padded("lpips_head dz0 C%d %dx%d" % (c, h, w), got_dz, ref, bound)


# ---- the whole term ---------------------------------------------------------------------------------------------------------------------------
TERM_CASES, term_inputs, NET_SEED = R.TERM_CASES, R.term_inputs, R.NET_SEED      # (with the seed selection: tests/lpips_bf16_ref.py)


_TERM_REF = {}


def _term_ref(name):
    """(lp, fake, real, plain float64 oracle, ideal bf16 run) of a case, computed once"""
    if name not in _TERM_REF:
        case = TERM_CASES[name]
        lp = chk.LPIPS(seed=NET_SEED)
        a, b = term_inputs(case, case["seed"])
        plain = R.lpips_run(lp, a, b, case["coeff"], channels=case["channels"])
        ideal = R.lpips_run(lp, a, b, case["coeff"], q=R.rt_bf16, channels=case["channels"])
        _TERM_REF[name] = (a, b, plain, ideal)
    return _TERM_REF[name]


def _hip_term(name, dtype, net=None):
    """(value, gradient) of the HIP term on a case; the patch case goes through channels= and the stride arguments"""
    from models import perceptual
    from vts import ops, perceptual as P

    dev = torch.device("cuda:0")
    case = TERM_CASES[name]
    a, b, _, _ = _term_ref(name)
    net = net if net is not None else perceptual.LpipsVgg16().to(dev)
    slot = ops.loss_slots(1, dev)
    if case["channels"] == 1:
        fa, fb = a._base.to(dev), b._base.to(dev)          # the whole [8, 2, 32, 32] tensors; the term reads channel 0 of each
        grad = torch.zeros_like(fa)
        P.lpips_term(net, fa[:, 0:1], fb[:, 0:1], case["coeff"], slot, grad_into=grad[:, 0:1], channels=1, nstride_fake=fa.stride(0),
                     nstride_real=fb.stride(0), grad_nstride=grad.stride(0), dtype=dtype)
        assert float(grad[:, 1].abs().max()) == 0.0
        return ops.loss_values(slot)[0], grad[:, 0:1].cpu(), slot.cpu()
    fa, fb = a.to(dev), b.to(dev)
    grad = torch.empty_like(fa)
    P.lpips_term(net, fa, fb, case["coeff"], slot, grad_into=grad, dtype=dtype)
    return ops.loss_values(slot)[0], grad.cpu(), slot.cpu()


@pytest.mark.parametrize("name", ["image", "patches"])
def test_whole_term_is_as_accurate_as_the_ideal_bf16_run(name):
    a, b, (v64, g64), (vi, gi) = _term_ref(name)
    v, g, s = _hip_term(name, "bf16")
    v32, g32, _ = _hip_term(name, "fp32")
    ev_hip, ev_ideal, ev_32 = abs(v - v64) / abs(v64), abs(vi - v64) / abs(v64), abs(v32 - v64) / abs(v64)
    eg_hip, eg_ideal, eg_32 = R.rel_l2(g, g64), R.rel_l2(gi, g64), R.rel_l2(g32, g64)
    print("lpips_term %-8s value    e_hip %.3e  e_ideal %.3e  fp32 path %.3e" % (name, ev_hip, ev_ideal, ev_32))
    print("lpips_term %-8s gradient e_hip %.3e  e_ideal %.3e  fp32 path %.3e" % (name, eg_hip, eg_ideal, eg_32))
    assert ev_hip <= 2 * ev_ideal and eg_hip <= 2 * eg_ideal
    # a second call is bitwise equal
    v2, g2, s2 = _hip_term(name, "bf16")
    assert torch.equal(s, s2) and torch.equal(g.view(torch.int32), g2.view(torch.int32))


def test_whole_term_patch_stack_equals_its_halves_bitwise():
    """mirrors test_lpips_on_a_full_patch_set_equals_its_halves: one call on the stack = two calls on its halves; in the bf16 path bitwise
    (a sample's result does not depend on the batch size or on its index, and the slot is fixed point)"""
    from models import perceptual
    from vts import ops, perceptual as P

    dev = torch.device("cuda:0")
    net = perceptual.LpipsVgg16().to(dev)
    g = torch.Generator().manual_seed(13)
    a, b = (0.3 * (2 * torch.rand((64, 1, 32, 32), generator=g) - 1)).to(dev), (0.3 * (2 * torch.rand((64, 1, 32, 32), generator=g) - 1)).to(dev)
    s_all, s_half = ops.loss_slots(1, dev), ops.loss_slots(1, dev)
    g_all, g_half = torch.empty_like(a), torch.empty_like(a)
    P.lpips_term(net, a, b, 1.0, s_all, grad_into=g_all, dtype="bf16")
    for hs in (slice(0, 32), slice(32, 64)):
        P.lpips_term(net, a[hs], b[hs], 1.0, s_half, grad_into=g_half[hs], dtype="bf16")
    assert ops.loss_values(s_all)[0] > 0 and torch.equal(s_all, s_half)
    assert torch.equal(g_all.view(torch.int32), g_half.view(torch.int32))


def test_whole_term_graph_replay_is_bitwise_equal_to_eager():
    from models import perceptual
    from vts import ops, perceptual as P

    dev = torch.device("cuda:0")
    net = perceptual.LpipsVgg16().to(dev)
    case = TERM_CASES["image"]
    a, b = (t.to(dev) for t in term_inputs(case, case["seed"]))
    slot, grad = ops.loss_slots(1, dev), torch.empty_like(a)
    P.lpips_term(net, a, b, case["coeff"], slot, grad_into=grad, dtype="bf16")           # eager (packs the weights, grows the workspaces)
    torch.cuda.synchronize()
    s0, g0 = slot.clone(), grad.clone()
    slot.zero_()
    grad.fill_(float("nan"))
    ops.freeze_ws("test_lpips_bf16")
    try:
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                P.lpips_term(net, a, b, case["coeff"], slot, grad_into=grad, dtype="bf16")
        torch.cuda.current_stream().wait_stream(side)
        slot.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(slot, s0) and torch.equal(grad.view(torch.int32), g0.view(torch.int32))
    finally:
        ops.release_ws("test_lpips_bf16")


def test_a_declined_layer_raises_in_bf16_mode(monkeypatch):
    from models import perceptual
    from vts import ops, perceptual as P

    dev = torch.device("cuda:0")
    net = perceptual.LpipsVgg16().to(dev)
    a = torch.zeros(1, 3, 32, 32, device=dev)
    monkeypatch.setattr(ops, "conv3x3_bf16_ok", lambda n, ci, co, h, w: ci != 256)
    with pytest.raises(RuntimeError, match="does not mix precisions"):
        P.lpips_term(net, a, a, 1.0, ops.loss_slots(1, dev), dtype="bf16")
    with pytest.raises(ValueError):
        P.lpips_term(net, a, a, 1.0, ops.loss_slots(1, dev), dtype="fp16")


# ---- the training step ------------------------------------------------------------------------------------------------------------------------
STEP_FLAGS = ("--model sinskitG --gpu_ids 0 --lambda_G1_lpips 1 --lambda_G2_lpips 10 --use_vision_aided_loss False --lambda_G2_GAN_feat 0 "
              "--checkpoints_dir /tmp/vts_test_ckpt --name tlb --crop_size 256 --batch_size 1")


def _step_model(extra=""):
    from models import create_model
    from options.train_options import TrainOptions
    from tests.test_step_gpu import load_test_weights

    opt = TrainOptions(cmd_line=STEP_FLAGS + extra).parse()
    model = create_model(opt)
    model.setup(opt)
    model.parallelize()
    model.train()
    load_test_weights(model, 31)
    return model


def _step_batch():
    from torch.utils.data import default_collate

    from data.synthetic_dataset import make_sample

    return default_collate([make_sample(256, 64, 16, 31)])


def _run_steps(model, batch, steps, first=0):
    """steps first .. first + steps - 1, each from its own seed of the host generators (the patch sampler draws from Python's `random`)"""
    import random

    out = []
    for i in range(first, first + steps):
        random.seed(5 + i)
        torch.manual_seed(5 + i)
        model.set_input(batch, phase="train")
        model.optimize_parameters(epoch=1)
        torch.cuda.synchronize()
        out.append(dict(model.get_current_losses()))
    return out


def test_step_with_bf16_lpips_terms_replay_equals_eager():
    """sinskitG at 256^2, batch 1, both LPIPS lambdas on, --lpips_dtype bf16, three steps (eager, capture, replay): it runs and the replayed
    schedule equals the eager one bit for bit (DiffAugment off, as in tests/test_step_gpu.py:test_hip_graph_replay_equals_eager: its draws come
    from torch's device generator, whose stream a captured graph does not share with eager execution)."""
    batch = _step_batch()
    graph = _step_model(" --lpips_dtype bf16 --use_diffaug False")
    assert graph.loss_lpips_dtype == "bf16"
    lg = _run_steps(graph, batch, 3)
    assert graph._graphs is not None and all(v["l_G_lpips"] > 0 and v["l_G2_lpips"] > 0 for v in lg)
    eager = _step_model(" --lpips_dtype bf16 --use_diffaug False --use_hip_graph False")
    le = _run_steps(eager, batch, 3)
    assert eager._graphs is None
    for s in range(3):
        for k in le[s]:
            assert le[s][k] == lg[s][k], ("step %d" % s, k, le[s][k], lg[s][k])
    for nm in ("G", "D", "D2"):
        a, b = getattr(eager, "flat" + nm).flat, getattr(graph, "flat" + nm).flat
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), nm
    assert torch.equal(eager.fake_I.view(torch.int32), graph.fake_I.view(torch.int32))


def test_step_bf16_lpips_losses_agree_with_the_fp32_step():
    """the two LPIPS losses of the same first step, bf16 against fp32, within the whole-term bound: twice the relative error of the ideal bf16
    run on this step's own tensors (the fp32 step stands in for float64 there: its own error, 1e-8 on such a value, is far below).  The
    generator-gradient difference is printed, not asserted (Adam turns rounding noise into +-lr)."""
    batch = _step_batch()
    m16 = _step_model(" --lpips_dtype bf16")
    assert m16.loss_lpips_dtype == "bf16"
    l16 = _run_steps(m16, batch, 1)[0]
    # the ideal bf16 run of the two terms on this step's tensors (CPU, float64, values only)
    lp = chk.LPIPS(sd=m16.netLPIPS.own_state())
    n = m16.real_I.shape[0]
    fI, rI = m16.fake_I.detach().cpu(), m16.real_I.detach().cpu()
    fT, rT = m16.fake_T_concat.detach().cpu(), m16.train_set["real_T"].detach().cpu()
    P2 = 2 * fT.shape[0]
    terms = {"l_G_lpips": (fI, rI, 1.0 / n, None), "l_G2_lpips": (fT.reshape(P2, 1, 32, 32), rT.reshape(P2, 1, 32, 32), 10.0 / n, 1)}
    ideal = {}
    for k, (a, b, coeff, cx) in terms.items():
        v64, _ = R.lpips_run(lp, a, b, coeff, channels=cx, want_grad=False)
        vi, _ = R.lpips_run(lp, a, b, coeff, q=R.rt_bf16, channels=cx, want_grad=False)
        ideal[k] = abs(vi - v64) / abs(v64)
    m32 = _step_model("")
    assert m32.loss_lpips_dtype == "fp32"
    l32 = _run_steps(m32, batch, 1)[0]
    for k in ("l_G_lpips", "l_G2_lpips"):
        e = abs(l16[k] - l32[k]) / abs(l32[k])
        print("step %-10s bf16 %.6f fp32 %.6f  rel diff %.3e  e_ideal %.3e" % (k, l16[k], l32[k], e, ideal[k]))
        assert l16[k] > 0 and e <= 2 * ideal[k], (k, e, ideal[k])
    g16 = {k: p.grad for k, p in m16.netG.named_parameters() if p.grad is not None}
    num = sum(float((g16[k].double() - p.grad.double()).pow(2).sum()) for k, p in m32.netG.named_parameters() if k in g16)
    den = sum(float(p.grad.double().pow(2).sum()) for k, p in m32.netG.named_parameters() if k in g16)
    print("step generator-gradient rel L2 bf16 vs fp32: %.3e (reported, not asserted)" % (num / den) ** 0.5)


# the labels of ops._run over one eager step of the model above with the DEFAULT option (fp32), run-length coded, recorded from the parent
# of the commit that added --lpips_dtype: the default must launch exactly what it launched before
PARENT_LAUNCHES_TEXT = """
conv4x4<conv,s2,nr1>*2 norm_from_partials conv4x4<conv,s2,nr2> norm_stats conv4x4<conv,s1,nr4> norm_stats head_conv4x4<conv,s1,nr1>
head_wgrad4x4<s1> channel_sum conv4x4<convT,s1,nr4> norm_bwd_from_partials wgrad4x4<s1> conv4x4<convT,s1,nr2> norm_bwd wgrad4x4<s2>
conv4x4<convT,s2,nr1> norm_bwd_from_partials wgrad4x4<s2> conv4x4<convT,s2,nr1> wgrad4x4<s2> channel_sum wgrad_reduce_batch
conv4x4<conv,s2,nr1>*2 norm_from_partials conv4x4<conv,s2,nr2> norm_stats conv4x4<conv,s1,nr4> norm_stats head_conv4x4<conv,s1,nr1>
head_wgrad4x4<s1> channel_sum conv4x4<convT,s1,nr4> norm_bwd_from_partials wgrad4x4<s1> conv4x4<convT,s1,nr2> norm_bwd wgrad4x4<s2>
conv4x4<convT,s2,nr1> norm_bwd wgrad4x4<s2> conv4x4<convT,s2,nr1> wgrad4x4<s2> channel_sum conv4x4<conv,s2,nr1>*2 norm_from_partials
conv4x4<conv,s2,nr2> norm_stats conv4x4<conv,s1,nr4> norm_stats head_conv4x4<conv,s1,nr1> head_wgrad4x4<s1> channel_sum
conv4x4<convT,s1,nr4> norm_bwd_from_partials wgrad4x4<s1> conv4x4<convT,s1,nr2> norm_bwd wgrad4x4<s2> conv4x4<convT,s2,nr1> norm_bwd
wgrad4x4<s2> conv4x4<convT,s2,nr1> wgrad4x4<s2> channel_sum wgrad_reduce_batch conv4x4<conv,s2,nr1> conv4x4<conv,s2,nr2>
norm_from_partials conv4x4<conv,s2,nr3> conv4x4<conv,s2,nr5>*5 conv4x4<convT,s2,nr5>*4 conv4x4<convT,s2,nr3> conv4x4<convT,s2,nr2>
conv4x4<convT,s2,nr1> norm_from_partials conv4x4<convT,s2,nr1> conv4x4<convT,s2,nr3> conv4x4<convT,s2,nr2> conv4x4<convT,s2,nr1>
norm_from_partials conv4x4<convT,s2,nr1> pad_affine w3x3_pack conv3x3_wide w3x3_wino_pack conv3x3_wide maxpool2_relu_pad w3x3_wino_pack
conv3x3_wide w3x3_wino_pack conv3x3_wide maxpool2_relu_pad w3x3_pack conv3x3_wide*2 pad_affine w3x3_pack conv3x3_wide*2 pad_affine
w3x3_pack conv3x3_wide*2 maxpool2_relu_pad w3x3_pack conv3x3_wide*2 pad_affine w3x3_pack conv3x3_wide*2 pad_affine w3x3_pack
conv3x3_wide*2 maxpool2_relu_pad w3x3_pack conv3x3_wide*2 pad_affine w3x3_pack conv3x3_wide*2 pad_affine w3x3_pack conv3x3_wide*2
zero_border lpips_layer zero_border lpips_layer*4 relu_mask_pad w3x3_pack conv3x3_wide relu_mask_pad w3x3_pack conv3x3_wide
relu_mask_pad w3x3_pack conv3x3_wide maxpool2_relu_bwd w3x3_pack conv3x3_wide relu_mask_pad w3x3_pack conv3x3_wide relu_mask_pad
w3x3_pack conv3x3_wide maxpool2_relu_bwd w3x3_pack conv3x3_wide relu_mask_pad w3x3_pack conv3x3_wide relu_mask_pad w3x3_pack
conv3x3_wide maxpool2_relu_bwd w3x3_pack conv3x3_wide*2 relu_mask_pad w3x3_pack conv3x3_wide maxpool2_relu_bwd w3x3_wino_pack
conv3x3_wide tap_embed conv4x4<convT,s1,nr1> pad_affine conv3x3_wide*2 maxpool2_relu_pad conv3x3_wide*2 maxpool2_relu_pad w3x3_wino_pack
conv3x3_wide w3x3_wino_pack conv3x3_wide w3x3_wino_pack conv3x3_wide maxpool2_relu_pad w3x3_wino_pack conv3x3_wide w3x3_wino_pack
conv3x3_wide w3x3_wino_pack conv3x3_wide maxpool2_relu_pad conv3x3_wide*2 pad_affine*3 conv3x3_wide*2 pad_affine*3 conv3x3_wide*2
zero_border lpips_layer zero_border lpips_layer zero_border lpips_layer zero_border lpips_layer*2 relu_mask_pad conv3x3_wide
relu_mask_pad conv3x3_wide relu_mask_pad conv3x3_wide maxpool2_relu_bwd conv3x3_wide*2 relu_mask_pad conv3x3_wide*2 relu_mask_pad
conv3x3_wide maxpool2_relu_bwd w3x3_wino_pack conv3x3_wide w3x3_wino_pack conv3x3_wide*2 maxpool2_relu_bwd w3x3_wino_pack conv3x3_wide*2
maxpool2_relu_bwd conv3x3_wide tap_embed patch_conv4x4<convT,s1,nr1> patch_conv4x4<conv,s2,nr1>*2 norm_patch_stats
patch_conv4x4<conv,s2,nr2> norm_patch_stats patch_conv4x4<conv,s1,nr4> norm_patch_stats patch_head_conv4x4<conv,s1,nr1>
patch_head_wgrad4x4<s1> channel_sum patch_conv4x4<convT,s1,nr4> norm_patch_bwd patch_wgrad4x4<s1> patch_conv4x4<convT,s1,nr2>
norm_patch_bwd patch_wgrad4x4<s2> patch_conv4x4<convT,s2,nr1> norm_patch_bwd patch_wgrad4x4<s2> patch_conv4x4<convT,s2,nr1>
patch_wgrad4x4<s2> channel_sum conv4x4<conv,s2,nr1>*2 norm_from_partials conv4x4<conv,s2,nr2> norm_stats conv4x4<conv,s1,nr4> norm_stats
head_conv4x4<conv,s1,nr1> head_wgrad4x4<s1> channel_sum conv4x4<convT,s1,nr4> norm_bwd_from_partials wgrad4x4<s1> conv4x4<convT,s1,nr2>
norm_bwd wgrad4x4<s2> conv4x4<convT,s2,nr1> norm_bwd wgrad4x4<s2> conv4x4<convT,s2,nr1> wgrad4x4<s2> channel_sum wgrad_reduce_batch
patch_conv4x4<conv,s2,nr1>*2 norm_patch_stats patch_conv4x4<conv,s2,nr2> norm_patch_stats patch_conv4x4<conv,s1,nr4> norm_patch_stats
patch_head_conv4x4<conv,s1,nr1> patch_head_wgrad4x4<s1> channel_sum patch_conv4x4<convT,s1,nr4> norm_patch_bwd patch_wgrad4x4<s1>
patch_conv4x4<convT,s1,nr2> norm_patch_bwd patch_wgrad4x4<s2> patch_conv4x4<convT,s2,nr1> norm_patch_bwd patch_wgrad4x4<s2>
patch_conv4x4<convT,s2,nr1> patch_wgrad4x4<s2> channel_sum conv4x4<conv,s2,nr1>*2 norm_from_partials conv4x4<conv,s2,nr2> norm_stats
conv4x4<conv,s1,nr4> norm_stats head_conv4x4<conv,s1,nr1> head_wgrad4x4<s1> channel_sum conv4x4<convT,s1,nr4> norm_bwd_from_partials
wgrad4x4<s1> conv4x4<convT,s1,nr2> norm_bwd wgrad4x4<s2> conv4x4<convT,s2,nr1> norm_bwd wgrad4x4<s2> conv4x4<convT,s2,nr1> wgrad4x4<s2>
channel_sum wgrad_reduce_batch conv4x4<conv,s2,nr1>*2 norm_from_partials conv4x4<conv,s2,nr2> norm_stats conv4x4<conv,s1,nr4> norm_stats
head_conv4x4<conv,s1,nr1> head_wgrad4x4<s1> channel_sum conv4x4<convT,s1,nr4> norm_bwd_from_partials wgrad4x4<s1> conv4x4<convT,s1,nr2>
norm_bwd wgrad4x4<s2> conv4x4<convT,s2,nr1> norm_bwd_from_partials wgrad4x4<s2> conv4x4<convT,s2,nr1> wgrad4x4<s2> channel_sum
patch_conv4x4<conv,s2,nr1>*2 norm_patch_stats patch_conv4x4<conv,s2,nr2> norm_patch_stats patch_conv4x4<conv,s1,nr4> norm_patch_stats
patch_head_conv4x4<conv,s1,nr1> patch_head_wgrad4x4<s1> channel_sum patch_conv4x4<convT,s1,nr4> norm_patch_bwd patch_wgrad4x4<s1>
patch_conv4x4<convT,s1,nr2> norm_patch_bwd patch_wgrad4x4<s2> patch_conv4x4<convT,s2,nr1> norm_patch_bwd patch_wgrad4x4<s2>
patch_conv4x4<convT,s2,nr1> patch_wgrad4x4<s2> channel_sum wgrad_reduce_batch conv4x4<conv,s2,nr1>*2 norm_from_partials
conv4x4<conv,s2,nr2> norm_stats conv4x4<conv,s1,nr4> norm_stats head_conv4x4<conv,s1,nr1> conv4x4<convT,s1,nr4> norm_bwd_from_partials
conv4x4<convT,s1,nr2> norm_bwd conv4x4<convT,s2,nr1> norm_bwd conv4x4<convT,s2,nr1>*2 conv4x4<conv,s2,nr1>*2 norm_from_partials
conv4x4<conv,s2,nr2> norm_stats conv4x4<conv,s1,nr4> norm_stats head_conv4x4<conv,s1,nr1> conv4x4<convT,s1,nr4> norm_bwd_from_partials
conv4x4<convT,s1,nr2> norm_bwd conv4x4<convT,s2,nr1> norm_bwd conv4x4<convT,s2,nr1>*2 conv4x4<conv,s2,nr1>*2 norm_from_partials
conv4x4<conv,s2,nr2> norm_stats conv4x4<conv,s1,nr4> norm_stats head_conv4x4<conv,s1,nr1> conv4x4<convT,s1,nr4> norm_bwd_from_partials
conv4x4<convT,s1,nr2> norm_bwd conv4x4<convT,s2,nr1> norm_bwd_from_partials conv4x4<convT,s2,nr1>*2 wgrad4x4<s2> channel_sum
conv4x4<conv,s2,nr1> norm_bwd_from_partials wgrad4x4<s2> conv4x4<conv,s2,nr2>*2 norm_bwd_from_partials wgrad4x4<s2>
conv4x4<conv,s2,nr3>*2 wgrad4x4<s2> conv4x4<conv,s2,nr5>*2 wgrad_reduce_batch wgrad4x4<s2> channel_sum conv4x4<conv,s2,nr1>
norm_bwd_from_partials wgrad4x4<s2> conv4x4<conv,s2,nr2>*2 norm_bwd_from_partials wgrad4x4<s2> conv4x4<conv,s2,nr3>*2 wgrad4x4<s2>
conv4x4<conv,s2,nr5>*2 wgrad_reduce_batch pad_affine*4 norm_bwd wgrad4x4<s2> conv4x4<conv,s2,nr5>*2 wgrad4x4<s2> conv4x4<conv,s2,nr5>*2
wgrad4x4<s2> conv4x4<conv,s2,nr5>*2 wgrad4x4<s2> conv4x4<conv,s2,nr5> wgrad4x4<s2> channel_sum conv4x4<convT,s2,nr5> wgrad4x4<s2>
conv4x4<convT,s2,nr5> wgrad4x4<s2> conv4x4<convT,s2,nr5> wgrad4x4<s2> conv4x4<convT,s2,nr5> wgrad4x4<s2> conv4x4<convT,s2,nr3>
wgrad4x4<s2> conv4x4<convT,s2,nr2> wgrad4x4<s2> conv4x4<convT,s2,nr1> wgrad4x4<s2> channel_sum wgrad_reduce_batch*2
"""
PARENT_LAUNCHES = [(t.split("*")[0], int(t.split("*")[1]) if "*" in t else 1) for t in PARENT_LAUNCHES_TEXT.split()]
assert sum(c for _, c in PARENT_LAUNCHES) == 501


def test_default_option_launches_the_parents_sequence(monkeypatch):
    from vts import ops

    model = _step_model("")
    labels = []
    orig = ops._run

    def rec(label, *a):
        labels.append(label)
        return orig(label, *a)

    monkeypatch.setattr(ops, "_run", rec)
    _run_steps(model, _step_batch(), 1)
    rle = []
    for lab in labels:
        if rle and rle[-1][0] == lab:
            rle[-1][1] += 1
        else:
            rle.append([lab, 1])
    assert not any("bf16" in lab for lab in labels)
    assert [tuple(e) for e in rle] == [tuple(e) for e in PARENT_LAUNCHES]
