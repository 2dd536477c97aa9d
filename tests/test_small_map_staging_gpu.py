"""Small-map members of the 4x4 convolution family after the staging rewrite (conv_small_kernel's pipelined flat staging at every quad
count, its line-wise path, wgrad_small_kernel's quad staging and its element-wise fallback): every case against
torch.nn.functional.conv2d / autograd evaluated on the CPU in float64 and cast down, rel-L2 <= 1e-5 (the single-op bound of
tests/test_kernels_gpu.py), with the kernel that ran asserted through vts_last_kernel().

Shapes are the smallest at which each path of the staging can go wrong: one / two / several 8-channel chunks (prologue only, one
pipeline step, steady state), maps of 2^2 .. 17^2 (20^2 for the widest quad instance), batches whose last block has absent images
(N = 9, 33, 513 for the convolutions; 33 and 257 for the weight gradient: 1 and 2 images per block), padded cout tiles, views that
are only 4-byte aligned, samples that are not contiguous.

Two cases are not as the task text literally names them: Cin = 7 at 32^2 never reaches the small-map kernel (eight 36 x 37 planes
exceed its LDS cap; the tiled kernel runs it, in the step as here), so it is checked as it dispatches and a 7 x 8 x 34 case reaches the
IW > 32 branch instead; "64/32, stride 1, lo 5^2 / hi 6^2" is a stride-1 geometry only with pad 1
(5 = 6 + 2 - 4 + 1); it runs as stated with pad = 1, and the step's own pad-2 geometry (lo 6^2 / hi 5^2) runs beside it."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import detrand  # noqa: E402  (checker only)

BOUND = 1e-5
LRELU = 1


def _dev():
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _kernel():
    from vts import lib as L
    return L.load().vts_last_kernel().decode()


def _affine(n, c, seed, name):
    return 1.0 + 0.3 * detrand.uniform((n * c,), seed, name + "sc"), 0.2 * detrand.uniform((n * c,), seed, name + "sh")


def _apply64(x, aff, act):
    """float64 activate(normalise(x))"""
    n, c = x.shape[:2]
    v = x.double()
    if aff is not None:
        v = v * aff[0].double().view(n, c, 1, 1) + aff[1].double().view(n, c, 1, 1)
    return F.leaky_relu(v, 0.2) if act == LRELU else v


def _misaligned(t, dev):
    """t on the device as a [1:] view of a flat buffer: 4-byte aligned, never 16-byte aligned"""
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:].view(t.shape)
    v.copy_(t)
    return v


def _act(x, aff, dev, misaligned=False):
    from vts.ops import Act
    xd = _misaligned(x, dev) if misaligned else x.to(dev)
    return Act(xd) if aff is None else Act(xd, aff[0].to(dev), aff[1].to(dev))


# ---- conv_small_kernel, forward ----------------------------------------------------------------------------------------------

CONV_FLAT = [
    # (N, Cin, H, Cout, stride, affine, misaligned weight + input, quads per thread of the instance)
    (9, 8, 2, 1, 1, True, False, 3),        # one chunk: prologue only
    (9, 16, 2, 33, 2, True, False, 3),
    (33, 16, 5, 7, 2, False, False, 3),     # two chunks
    (9, 32, 6, 16, 1, True, False, 3),      # steady state
    (33, 32, 5, 33, 1, True, False, 3),     # NR = 2, padded cout tile
    (33, 8, 9, 33, 2, True, False, 3),
    (33, 16, 9, 32, 2, True, True, 3),      # the step's condition: weights of the flat parameter buffer are 4-byte aligned only
    (9, 16, 17, 16, 2, False, False, 3),
    (33, 32, 17, 7, 2, True, False, 3),
    (513, 8, 17, 16, 2, True, False, 6),    # two images of 17 x 17 per block: 5 quads per thread; the last block has one absent image
    (513, 16, 20, 8, 2, False, False, 10),  # two images of 20 x 20 per block: 7 quads per thread
]


def _conv_fwd(N, C0, C1, H, W, Cout, s, affine, act, misaligned=False):
    from vts import ops
    dev = _dev()
    x0 = detrand.uniform((N, C0, H, W), 61, "x0")
    a0 = _affine(N, C0, 61, "a0") if affine else None
    xs, in1 = [_apply64(x0, a0, act)], None
    if C1:
        x1 = detrand.uniform((N, C1, H, W), 61, "x1")
        a1 = _affine(N, C1, 61, "a1") if affine else None
        xs.append(_apply64(x1, a1, act))
        in1 = _act(x1, a1, dev)
    w = detrand.uniform((Cout, C0 + C1, 4, 4), 62, "w") * 0.2
    b = detrand.uniform((Cout,), 62, "b")
    ref = F.conv2d(torch.cat(xs, 1), w.double(), b.double(), stride=s, padding=2).float()
    wd, bd, in0 = _misaligned(w, dev) if misaligned else w.to(dev), b.to(dev), _act(x0, a0, dev, misaligned)

    def run():
        out = torch.full(ref.shape, float("nan"), device=dev)
        ops.conv4x4(in0, wd, (C0 + C1) * 16, 16, Cout, out, in1=in1, bias=bd, stride=s, pad=2, act_in=act)
        return out
    return run, ref


@pytest.mark.parametrize("case", CONV_FLAT)
def test_conv_flat_staging(case):
    N, Cin, H, Cout, s, affine, mis, nq = case
    run, ref = _conv_fwd(N, Cin, 0, H, H, Cout, s, affine, LRELU, mis)
    out = run()
    k = _kernel()
    assert k.startswith("conv_small_kernel<0, %d," % s) and k.endswith("+flat"), k
    # the instance the host picks: smallest of 3 / 6 / 10 quads per thread that covers the images of a block (asserted so that the
    # cases above keep reaching every instance; IPB as vts_conv_small_try computes it for these shapes)
    oh = (H + 4 - 4) // s + 1
    nr = 2 if Cout > 16 else 1
    cop = nr * 16 + (16 if nr == 2 else 0)
    ipb = max(1, min((4 * 8 * 16) // (oh * oh), (48 * 1024 // 4 - 8 * 16 * cop) // (8 * (H + 4) * (H + 5)), max(1, N * ((Cout + nr * 16 - 1) // (nr * 16)) // 256), N))
    nqt = -(-ipb * 2 * H * H // 256)
    assert (3 if nqt <= 3 else 6 if nqt <= 6 else 10) == nq, (ipb, nqt)
    e = rel(out, ref)
    print("conv flat", case, k, "rel-L2 %.3g" % e)
    assert e <= BOUND
    assert torch.equal(run(), out)          # the same launch twice: bit for bit


CONV_GENERIC = [
    # (N, C0, C1, H, W, Cout, stride, the small-map kernel runs it)
    (10, 3, 4, 16, 12, 8, 2, True),     # dual source
    # Cin = 7 at 32^2, the first layer of the 32 x 32 stack: eight 36 x 37 planes do not fit the small-map kernel's 48 KB, so the dispatch
    # gives this shape to the tiled kernel (as it does in the step); checked against float64 all the same
    (9, 7, 0, 32, 32, 8, 2, False),
    (9, 7, 0, 8, 34, 8, 2, True),       # the IW > 32 branch of the line-wise staging: 34-wide rows, few enough of them to fit
    (9, 12, 0, 9, 9, 16, 2, True),      # ragged last chunk
]


@pytest.mark.parametrize("case", CONV_GENERIC)
def test_conv_line_staging(case):
    N, C0, C1, H, W, Cout, s, small = case
    run, ref = _conv_fwd(N, C0, C1, H, W, Cout, s, True, 0 if C0 == 7 else LRELU)
    out = run()
    k = _kernel()
    assert k.startswith("conv_small_kernel<0, %d," % s) == small and not k.endswith("+flat"), k
    e = rel(out, ref)
    print("conv line-wise", case, k, "rel-L2 %.3g" % e)
    assert e <= BOUND
    assert torch.equal(run(), out)


# ---- conv_small_kernel, transposed (backward-data of Conv2d(Cx -> Cg, 4, stride, pad)) ------------------------------------------

CONVT = [
    # (N, Cg, Cx, XH, stride, pad): the gradient map is GH = (XH + 2 pad - 4) / stride + 1
    (9, 32, 16, 5, 1, 2),       # s1 p2: 6^2 -> 5^2
    (33, 8, 7, 9, 2, 2),        # s2 p2, odd sizes: 5^2 -> 9^2
    (9, 16, 33, 17, 2, 2),      # 9^2 -> 17^2
    (33, 16, 16, 4, 2, 1),      # s2 p1: 2^2 -> 4^2
]


@pytest.fixture(scope="module", params=CONVT, ids=lambda c: "N%d_%dto%d_x%d_s%dp%d" % c)
def convt_ref(request):
    """backward-data reference, computed once per geometry: raw = conv^T(g) in float64, and the derivative-mask operand"""
    N, Cg, Cx, XH, s, p = request.param
    x = detrand.uniform((N, Cx, XH, XH), 71, "x")
    aff = _affine(N, Cx, 71, "a")
    w = detrand.uniform((Cg, Cx, 4, 4), 71, "w") * 0.3
    xl = torch.zeros(N, Cx, XH, XH, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xl, w.double(), None, stride=s, padding=p)
    g = detrand.uniform(tuple(y.shape), 71, "g")
    (y * g.double()).sum().backward()
    raw = xl.grad
    pre = x.double() * aff[0].double().view(N, Cx, 1, 1) + aff[1].double().view(N, Cx, 1, 1)
    masked = raw * torch.where(pre > 0, 1.0, 0.2)
    base = detrand.uniform((N, Cx, XH, XH), 71, "base")
    return request.param, x, aff, w, g, raw, masked, base


@pytest.mark.parametrize("mode", ["plain", "dmask", "dmask_accumulate"])
def test_conv_transposed_flat_staging(convt_ref, mode):
    from vts import ops
    (N, Cg, Cx, XH, s, p), x, aff, w, g, raw, masked, base = convt_ref
    dev = _dev()
    acc = mode == "dmask_accumulate"
    ref = (raw if mode == "plain" else masked) + (base.double() if acc else 0.0)
    dm = _act(x, aff, dev) if mode != "plain" else None
    gd, wd, based = _act(g, None, dev), w.to(dev), base.to(dev)

    def run():
        out = based.clone() if acc else torch.full(x.shape, float("nan"), device=dev)
        ops.conv4x4(gd, wd, 16, Cx * 16, Cx, out, stride=s, pad=p, transposed=True, dmask=dm,
                    dmask_act=LRELU if dm is not None else 0, accumulate=acc)
        return out
    out = run()
    k = _kernel()
    assert k.startswith("conv_small_kernel<1, %d," % s) and k.endswith("+flat"), k
    e = rel(out, ref.float())
    print("convT flat", convt_ref[0], mode, k, "rel-L2 %.3g" % e)
    assert e <= BOUND
    assert torch.equal(run(), out)


# ---- wgrad_small_kernel ---------------------------------------------------------------------------------------------------------

WGRAD = [
    # (CL, CH, LH, HH, stride, pad)
    (8, 7, 17, 32, 2, 2),
    (16, 8, 9, 17, 2, 2),
    (32, 16, 5, 9, 2, 2),
    (64, 32, 5, 6, 1, 1),       # as the task text states it (see the module docstring) ...
    (64, 32, 6, 5, 1, 2),       # ... and the step's geometry
    (1, 64, 7, 6, 1, 2),
]
# (N, affine + LeakyReLU on lo, on hi, accumulate, layout): N = 33 / 257: 1 / 2 images per block, ragged last block
WGRAD_VARIANTS = [
    (33, False, True, False, "contiguous"),
    (257, True, False, True, "contiguous"),
    (257, True, True, False, "misaligned"),      # [1:] views of flat buffers: 4-byte aligned only
    (33, True, True, False, "strided"),          # channel slices of wider tensors: samples not contiguous, element-wise staging
]


def _wgrad_case(geom, variant):
    from vts import ops
    from vts.ops import Act
    CL, CH, LH, HH, s, p = geom
    N, lo_aff, hi_aff, acc, layout = variant
    dev = _dev()
    assert (HH + 2 * p - 4) // s + 1 == LH
    lo = detrand.uniform((N, CL, LH, LH), 81, "lo")
    hi = detrand.uniform((N, CH, HH, HH), 81, "hi")
    al = _affine(N, CL, 81, "l") if lo_aff else None
    ah = _affine(N, CH, 81, "h") if hi_aff else None
    lov, hiv = _apply64(lo, al, LRELU if lo_aff else 0), _apply64(hi, ah, LRELU if hi_aff else 0)
    w = torch.zeros(CL, CH, 4, 4, dtype=torch.float64, requires_grad=True)
    (F.conv2d(hiv, w, None, stride=s, padding=p) * lov).sum().backward()       # dw[cl][ch][ky][kx] = sum lo * hi(shifted)
    base = detrand.uniform((CL, CH, 4, 4), 81, "base")
    ref = (w.grad + (base.double() if acc else 0.0)).float()

    def place(t, aff):
        if layout == "strided":
            wide = torch.full((t.shape[0], t.shape[1] + 1) + tuple(t.shape[2:]), float("nan"), device=dev)
            wide[:, :t.shape[1]] = t.to(dev)
            v = wide[:, :t.shape[1]]
            return Act(v) if aff is None else Act(v, aff[0].to(dev), aff[1].to(dev))
        return _act(t, aff, dev, layout == "misaligned")
    lo_a, hi_a, based = place(lo, al), place(hi, ah), base.to(dev)

    def run():
        dw = based.clone() if acc else torch.full((CL, CH, 4, 4), float("nan"), device=dev)
        ops.wgrad4x4(lo_a, hi_a, dw, act_lo=LRELU if lo_aff else 0, act_hi=LRELU if hi_aff else 0, stride=s, pad=p, accumulate=acc, defer=False)
        return dw
    return run, ref


@pytest.mark.parametrize("variant", WGRAD_VARIANTS, ids=lambda v: "N%d_%s" % (v[0], v[4]))
@pytest.mark.parametrize("geom", WGRAD, ids=lambda g: "%dx%d_lo%d_hi%d_s%dp%d" % g)
def test_wgrad_small_staging(geom, variant):
    run, ref = _wgrad_case(geom, variant)
    dw = run()
    k = _kernel()
    assert k.startswith("wgrad_small_kernel<"), k
    assert k.endswith("+quad") == (variant[4] != "strided"), k
    e = rel(dw, ref)
    print("wgrad small", geom, variant, k, "rel-L2 %.3g" % e)
    assert e <= BOUND
    assert torch.equal(run(), dw)


def test_wgrad_small_staging_several_blocks_per_workgroup():
    """lo 8 x 17^2 / hi 7 x 32^2 holds two images per block in LDS, so 601 images are 301 blocks on 256 workgroups: 45 workgroups stage
    a second block (its first round is issued under the first block's MFMAs), the last of them a ragged block behind a full one"""
    run, ref = _wgrad_case((8, 7, 17, 32, 2, 2), (601, True, True, False, "contiguous"))
    dw = run()
    k = _kernel()
    assert k.startswith("wgrad_small_kernel<1, 2>") and k.endswith("+quad"), k
    e = rel(dw, ref)
    print("wgrad small, 301 blocks", k, "rel-L2 %.3g" % e)
    assert e <= BOUND
    assert torch.equal(run(), dw)


# ---- capture ------------------------------------------------------------------------------------------------------------------

def _captured_equals_eager(run):
    eager = run().clone()                       # (also sizes the shared workspace before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    graph.replay()
    torch.cuda.synchronize()
    return torch.equal(first, eager) and torch.equal(out, eager)


def test_conv_flat_staging_captured_equals_eager():
    run, _ = _conv_fwd(33, 32, 0, 5, 5, 33, 1, True, LRELU)
    assert _captured_equals_eager(run)


def test_wgrad_small_staging_captured_equals_eager():
    run, _ = _wgrad_case((32, 16, 5, 9, 2, 2), (257, True, True, False, "contiguous"))
    assert _captured_equals_eager(run)
