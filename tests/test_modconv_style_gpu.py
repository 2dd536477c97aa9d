"""ModulatedConv2d with a style VECTOR on the GPU: forward in all four forms (plain / up / down / nodemod), its backward, the two new
reduction kernels on their own, and the StyledConv / ToRGB blocks built on it (reference models/stylegan_networks.py:248-437).

Judges: the reference's own numbers in tests/golden/stylegan2_32.npz (oracle/make_golden.py:golden_sg2: output, full style gradient,
probes of the input and parameter gradients) and the float64 autograd of oracle/stylegan2.py:modulated_conv2d, which reproduces those
numbers.  One bound at block level, 2e-5 true relative L2 -- the bound this module's forward already meets against the same fixture;
the same arithmetic in fp32 on the CPU stays below 8.4e-7 on every tensor of every shape used here, so 2e-5 leaves > 20x for another
summation order.  Kernel-level bounds: 1e-6 on an output with one rounding, 1e-5 on a reduction (the operator bound of
tests/test_stylegan2_gpu.py).  Gradients through the three chained blocks of a synthesis step: 2e-4 (that file's stack bound).

Every test prints its figures before it asserts (run with -s to see them).
Worst values measured on an MI355X per form (output / dx / dstyle / parameter gradients), fixture shape and the block shapes of
test_block_shapes_match_float64_oracle together:
  plain    6.8e-7 / 6.9e-7 / 7.1e-7 / 8.1e-7   (all four at Ci = Co = 512, 32 x 32)
  up       2.9e-7 / 5.7e-7 / 3.9e-7 / 4.6e-7
  down     3.9e-7 / 6.8e-7 / 2.9e-7 / 3.5e-7
  nodemod  2.3e-7 / 2.4e-7 / 3.1e-7 / 3.8e-7   (the 1 x 1 ToRGB case included)
The kernels alone: scale_dot 1.3e-7 on dot, 2.8e-8 on out; demod_bwd 2.5e-7.  StyledConv / ToRGB 2.7e-7; the synthesis step 4.1e-7 on the
image, 6.5e-7 on its gradients.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import detrand, stylegan2 as sg  # noqa: E402  (checker only)

BOUND = 2e-5          # block level: output and every gradient of one block
STACK_BOUND = 2e-4    # gradients through a stack of blocks
FORMS = {"plain": {}, "up": {"upsample": True}, "down": {"downsample": True}, "nodemod": {"demodulate": False}}
PNAMES = ("weight", "modulation.weight", "modulation.bias")


def _dev():
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "stylegan2_32.npz"), allow_pickle=False)


def mod_shapes(ci, co, k, sd):
    return {"weight": (1, co, ci, k, k), "modulation.weight": (ci, sd), "modulation.bias": (ci,)}


def oracle_modconv(x, style, w, upsample=False, downsample=False, demodulate=True):
    """sg.modulated_conv2d in the dtype of x.  In float64 the oracle's resampling forms stop at their Blur (make_kernel() is float32), so
    for those the same lines are restated here with the kernel cast; everything else is the oracle's own function."""
    if x.dtype == torch.float32 or not (upsample or downsample):
        return sg.modulated_conv2d(x, style, w["weight"], w["modulation.weight"], w["modulation.bias"], demodulate=demodulate,
                                   upsample=upsample, downsample=downsample)
    n, ci, h, wd = x.shape
    _, co, _, k, _ = w["weight"].shape
    s = sg.equal_linear(style, w["modulation.weight"], w["modulation.bias"]).view(n, 1, ci, 1, 1)
    wgt = (1.0 / math.sqrt(ci * k * k)) * w["weight"] * s
    if demodulate:
        wgt = wgt * torch.rsqrt(wgt.pow(2).sum([2, 3, 4]) + 1e-8).view(n, co, 1, 1, 1)
    kern = sg.make_kernel().to(x.dtype)
    if upsample:
        p = (4 - 2) - (k - 1)
        out = F.conv_transpose2d(x.reshape(1, n * ci, h, wd), wgt.transpose(1, 2).reshape(n * ci, co, k, k), padding=0, stride=2, groups=n)
        out = out.view(n, co, out.shape[2], out.shape[3])
        return sg.upfirdn2d(out, kern * 4, pad=((p + 1) // 2 + 1, p // 2 + 1))
    p = (4 - 2) + (k - 1)
    x = sg.upfirdn2d(x, kern, pad=((p + 1) // 2, p // 2))
    out = F.conv2d(x.reshape(1, n * ci, x.shape[2], x.shape[3]), wgt.view(n * co, ci, k, k), padding=0, stride=2, groups=n)
    return out.view(n, co, out.shape[2], out.shape[3])


def oracle_grads(x, style, w, cot_of, dtype=torch.float64, **form):
    """(y, dx, dstyle, {parameter gradients}, cotangent) of the oracle under autograd in `dtype`"""
    xo = x.detach().to(dtype).clone().requires_grad_(True)
    so = style.detach().to(dtype).clone().requires_grad_(True)
    wo = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in w.items()}
    y = oracle_modconv(xo, so, wo, **form)
    cot = cot_of(tuple(y.shape))
    (y * cot.to(dtype)).sum().backward()
    return y.detach(), xo.grad, so.grad, {k: v.grad for k, v in wo.items()}, cot


def engine_grads(x, style, w, cot, accumulate_twice=False, **form):
    """(y, dx, dstyle, {parameter gradients}) of the HIP path; x, style, w, cot on the CPU"""
    from vts import engine
    dev = _dev()
    wd = {k: v.to(dev) for k, v in w.items()}
    y, ctx = engine.modulated_conv2d_forward(x.to(dev), style.to(dev), wd["weight"], wd["modulation.weight"], wd["modulation.bias"], **form)
    gr = {k: torch.full_like(v, float("nan")) for k, v in wd.items()}
    kw = dict(dweight=gr["weight"], dmod_weight=gr["modulation.weight"], dmod_bias=gr["modulation.bias"])
    dx, dstyle = engine.modulated_conv2d_backward(ctx, cot.to(dev), **kw)
    if accumulate_twice:
        engine.modulated_conv2d_backward(ctx, cot.to(dev), accumulate=True, **kw)
    return y, dx, dstyle, gr


def fixture_case(gold, tag):
    seed = int(gold["seed"])
    w = sg.test_weights(mod_shapes(12, 20, 3, 16), seed + 1)
    x = detrand.uniform((2, 12, 10, 10), seed, "mod_in")
    st = detrand.uniform((2, 16), seed, "mod_style")
    return seed, w, x, st, (lambda shape: detrand.uniform(shape, seed, "mod_cot" + tag))


@pytest.mark.parametrize("tag", list(FORMS))
def test_forward_and_backward_match_reference_fixture(gold, tag):
    """output and dstyle as full tensors, dx and the parameter gradients through detrand.probe, against the reference's stored numbers;
    each probe component is judged relative to the stored NORM (a sum or a dot can cancel)"""
    seed, w, x, st, cot_of = fixture_case(gold, tag)
    ref_out = torch.from_numpy(gold["mod/%s/out" % tag])
    y, dx, dstyle, gr = engine_grads(x, st, w, cot_of(tuple(ref_out.shape)), **FORMS[tag])
    assert y.shape == ref_out.shape
    figs = {"out": rel(y, ref_out), "dstyle": rel(dstyle, torch.from_numpy(gold["mod/%s/dstyle" % tag]))}
    for name, t, key, pname in [("dx", dx, "mod/%s/dx" % tag, "mdx")] + [(k, gr[k], "mod/%s/grad/%s" % (tag, k), k) for k in PNAMES]:
        got, want = detrand.probe(t.cpu(), pname), gold[key]
        figs[name + " probe"] = float(np.abs(got - want).max() / want[1])
    print(tag, {k: "%.2e" % v for k, v in figs.items()})
    for k, v in figs.items():
        assert v < BOUND, (tag, k, v)


@pytest.mark.parametrize("tag", list(FORMS))
def test_full_gradients_match_float64_oracle(gold, tag):
    seed, w, x, st, cot_of = fixture_case(gold, tag)
    yo, dxo, dso, go, cot = oracle_grads(x, st, w, cot_of, **FORMS[tag])
    y, dx, dstyle, gr = engine_grads(x, st, w, cot, **FORMS[tag])
    figs = {"out": rel(y, yo), "dx": rel(dx, dxo), "dstyle": rel(dstyle, dso)}
    figs.update({k: rel(gr[k], go[k]) for k in PNAMES})
    print(tag, {k: "%.2e" % v for k, v in figs.items()})
    for k, v in figs.items():
        assert v < BOUND, (tag, k, v)


# (name, Ci, Co, K, H, form): the shapes the blocks really run at, batch 2, style_dim 512
BLOCK_CASES = [
    ("plain4", 512, 512, 3, 4, "plain"), ("plain8", 512, 512, 3, 8, "plain"), ("plain32", 512, 512, 3, 32, "plain"),
    ("up8", 512, 512, 3, 8, "up"), ("down16", 512, 512, 3, 16, "down"),
    ("narrow128", 32, 16, 3, 128, "plain"),          # the reduction kernel, not the convolution, carries the time
    ("torgb16", 512, 3, 1, 16, "nodemod"),           # ToRGB's convolution: 1 x 1, three outputs, no demodulation
]


@pytest.mark.parametrize("name,ci,co,k,h,form", BLOCK_CASES, ids=[c[0] for c in BLOCK_CASES])
def test_block_shapes_match_float64_oracle(name, ci, co, k, h, form):
    seed, sd, n = 1300 + len(name), 512, 2
    w = sg.test_weights(mod_shapes(ci, co, k, sd), seed)
    x = detrand.uniform((n, ci, h, h), seed, "x")
    st = detrand.uniform((n, sd), seed, "style")
    yo, dxo, dso, go, cot = oracle_grads(x, st, w, lambda shape: detrand.uniform(shape, seed, "cot"), **FORMS[form])
    y, dx, dstyle, gr = engine_grads(x, st, w, cot, **FORMS[form])
    assert y.shape == yo.shape
    figs = {"out": rel(y, yo), "dx": rel(dx, dxo), "dstyle": rel(dstyle, dso)}
    figs.update({kk: rel(gr[kk], go[kk]) for kk in PNAMES})
    print(name, {kk: "%.2e" % v for kk, v in figs.items()})
    for kk, v in figs.items():
        assert v < BOUND, (name, kk, v)


# ---- the new kernels on their own ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 4, 4), (1, 5, 21, 21), (3, 7, 33, 65), (2, 16, 256, 256)], ids=lambda s: "x".join(map(str, s)))
def test_scale_dot_kernel_matches_float64(shape):
    from vts import ops
    dev = _dev()
    n, c = shape[0], shape[1]
    a, b = detrand.uniform(shape, 71, "a"), detrand.uniform(shape, 71, "b")
    f = detrand.uniform((n * c,), 71, "f") + 1.5
    d0 = detrand.uniform((n * c,), 71, "dot0")
    alpha = 0.37
    a64, b64 = a.double().numpy(), b.double().numpy()
    want_dot = alpha * (a64 * b64).reshape(n * c, -1).sum(1)
    want_out = a64 * f.double().numpy().reshape(n, c, 1, 1)
    ad, bd, fd = a.to(dev), b.to(dev), f.to(dev)
    for with_out in (True, False):
        for acc in (False, True):
            dot = d0.to(dev).clone() if acc else torch.full((n * c,), float("nan"), device=dev)
            out = torch.full(shape, float("nan"), device=dev) if with_out else None
            ops.modconv_scale_dot(ad, bd, dot, f=fd if with_out else None, out=out, alpha=alpha, accumulate=acc)
            want = want_dot + (d0.double().numpy() if acc else 0.0)
            e_dot = rel(dot, torch.from_numpy(want))
            e_out = rel(out, torch.from_numpy(want_out)) if with_out else 0.0
            print(shape, "out" if with_out else "no out", "accumulate" if acc else "overwrite", "dot %.2e out %.2e" % (e_dot, e_out))
            assert e_dot < 1e-5 and e_out < 1e-6
    # an unaligned view (scalar path of the same shape): same numbers within the bound
    if shape[2] * shape[3] % 4 == 0:
        buf = torch.empty(a.numel() + 1, device=dev)
        av = buf[1:].view(shape).copy_(ad)
        dot = torch.empty(n * c, device=dev)
        ops.modconv_scale_dot(av, bd, dot, alpha=alpha)
        assert rel(dot, torch.from_numpy(want_dot)) < 1e-5


@pytest.mark.parametrize("n,co,ci,kk", [(2, 20, 12, 9), (3, 512, 512, 9)])
def test_demod_bwd_kernel_matches_float64_autograd(n, co, ci, kk):
    """against autograd of the closed form d = rsqrt(c^2 sum_{ci,k} w^2 s^2 + 1e-8) in float64"""
    from vts import ops
    dev = _dev()
    k = int(round(kk ** 0.5))
    w = detrand.uniform((co, ci, k, k), 83, "w") * math.sqrt(3.0)
    s = detrand.uniform((n, ci), 83, "s") + 1.0
    dd = detrand.uniform((n, co), 83, "dd")
    c = 1.0 / math.sqrt(ci * kk)
    w64, s64 = w.double().requires_grad_(True), s.double().requires_grad_(True)
    d64 = torch.rsqrt(c * c * torch.einsum("oik,ni->no", w64.view(co, ci, kk) ** 2, s64 ** 2) + 1e-8)
    (d64 * dd.double()).sum().backward()
    wd, sdv = w.to(dev), s.to(dev)
    d = ops.modconv_demod(wd, sdv, c)
    assert rel(d, d64) < 1e-5
    dw, ds = torch.full_like(wd, float("nan")), torch.full_like(sdv, float("nan"))
    ops.modconv_demod_bwd(dd.to(dev), d, wd, sdv, c, dw, ds)
    figs = [rel(dw, w64.grad), rel(ds, s64.grad)]
    ops.modconv_demod_bwd(dd.to(dev), d, wd, sdv, c, dw, ds, accumulate_dw=True, accumulate_ds=True)
    figs += [rel(dw, 2 * w64.grad), rel(ds, 2 * s64.grad)]
    print((n, co, ci, kk), "dw %.2e ds %.2e, accumulated dw %.2e ds %.2e" % tuple(figs))
    assert max(figs) < 1e-5


def test_weight_transpose_kernel_is_exact():
    from vts import ops
    dev = _dev()
    w = detrand.uniform((20, 12, 3, 3), 5, "w").to(dev)
    out = torch.full((12, 20, 3, 3), float("nan"), device=dev)
    ops.modconv_transpose(w, out)
    assert torch.equal(out, w.transpose(0, 1).contiguous())
    ops.modconv_transpose(w, out, accumulate=True)
    assert torch.equal(out, 2 * w.transpose(0, 1).contiguous())


# ---- properties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(FORMS))
def test_accumulate_doubles_parameter_gradients(gold, tag):
    seed, w, x, st, cot_of = fixture_case(gold, tag)
    cot = cot_of(tuple(gold["mod/%s/out" % tag].shape))
    _, _, _, once = engine_grads(x, st, w, cot, **FORMS[tag])
    _, _, _, twice = engine_grads(x, st, w, cot, accumulate_twice=True, **FORMS[tag])
    for k in PNAMES:
        e = rel(twice[k], 2 * once[k])
        print(tag, k, "%.2e" % e)
        assert e < 1e-6, (tag, k, e)


def _flat(res):
    y, dx, dstyle, gr = res
    return [y, dx, dstyle] + [gr[k] for k in PNAMES]


@pytest.mark.parametrize("tag", list(FORMS))
def test_two_runs_give_the_same_bits(gold, tag):
    seed, w, x, st, cot_of = fixture_case(gold, tag)
    cot = cot_of(tuple(gold["mod/%s/out" % tag].shape))
    a = _flat(engine_grads(x, st, w, cot, **FORMS[tag]))
    b = _flat(engine_grads(x, st, w, cot, **FORMS[tag]))
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(a, b)), tag


@pytest.mark.parametrize("tag", list(FORMS))
def test_captured_graph_replays_the_same_bits(gold, tag):
    """forward + backward captured on ONE stream after an eager warm-up call (scratch buffers and cached constants are created on first use)"""
    from vts import engine
    dev = _dev()
    seed, w, x, st, cot_of = fixture_case(gold, tag)
    wd = {k: v.to(dev) for k, v in w.items()}
    xd, sdv = x.to(dev), st.to(dev)
    cot = cot_of(tuple(gold["mod/%s/out" % tag].shape)).to(dev)
    gr = {k: torch.zeros_like(v) for k, v in wd.items()}

    def run():
        y, ctx = engine.modulated_conv2d_forward(xd, sdv, wd["weight"], wd["modulation.weight"], wd["modulation.bias"], **FORMS[tag])
        dx, ds = engine.modulated_conv2d_backward(ctx, cot, dweight=gr["weight"], dmod_weight=gr["modulation.weight"],
                                                  dmod_bias=gr["modulation.bias"])
        return [y, dx, ds]

    outs = run()
    torch.cuda.synchronize()
    eager = [t.clone() for t in outs + [gr[k] for k in PNAMES]]
    graph = torch.cuda.CUDAGraph()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):
        with torch.cuda.graph(graph, stream=cs):
            outs = run()
    torch.cuda.current_stream().wait_stream(cs)
    for k in PNAMES:
        gr[k].fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    replay = outs + [gr[k] for k in PNAMES]
    assert all(torch.equal(a, b) for a, b in zip(eager, replay)), tag


@pytest.mark.parametrize("tag", list(FORMS))
def test_wrapper_equals_context_forward(gold, tag):
    from vts import engine
    dev = _dev()
    seed, w, x, st, _ = fixture_case(gold, tag)
    wd = {k: v.to(dev) for k, v in w.items()}
    args = (x.to(dev), st.to(dev), wd["weight"], wd["modulation.weight"], wd["modulation.bias"])
    y, ctx = engine.modulated_conv2d_forward(*args, **FORMS[tag])
    assert ctx is not None and torch.equal(engine.modulated_conv2d(*args, **FORMS[tag]), y)


# ---- blocks --------------------------------------------------------------------------------------------------------------------------
def styled_shapes(ci, co, k, sd):
    return {"conv.weight": (1, co, ci, k, k), "conv.modulation.weight": (ci, sd), "conv.modulation.bias": (ci,), "noise.weight": (1,),
            "activate.bias": (1, co, 1, 1)}


def torgb_shapes(ci, sd):
    return {"conv.weight": (1, 3, ci, 1, 1), "conv.modulation.weight": (ci, sd), "conv.modulation.bias": (ci,), "bias": (1, 3, 1, 1)}


def _conv_w(sd, prefix=""):
    return {k: sd[prefix + "conv." + k] for k in PNAMES}


def oracle_styled_conv(sd, x, style, noise, upsample):
    """StyledConv.forward :408-415 composed from the oracle's functions"""
    out = oracle_modconv(x, style, _conv_w(sd), upsample=upsample)
    if noise is not None:
        out = out + sd["noise.weight"] * noise
    return sg.fused_leaky_relu(out, sd["activate.bias"])


def oracle_to_rgb(sd, x, style, skip):
    """ToRGB.forward :428-437; Upsample :98-116 = upfirdn2d(up 2, kernel * 4, pad (2, 1))"""
    out = oracle_modconv(x, style, _conv_w(sd), demodulate=False) + sd["bias"]
    if skip is not None:
        out = out + sg.upfirdn2d(skip, sg.make_kernel().to(x.dtype) * 4, up=2, down=1, pad=(2, 1))
    return out


def _load(m, sd):
    dev = _dev()
    m.load_state_dict({k: v for k, v in sd.items()}, strict=False)
    m.to(dev)
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = torch.full_like(p, float("nan"))
    return m


def _leaves(sd, *tensors):
    sdo = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    return sdo, [None if t is None else t.double().requires_grad_(True) for t in tensors]


@pytest.mark.parametrize("upsample", [False, True], ids=["plain", "up"])
@pytest.mark.parametrize("with_noise", [False, True], ids=["nonoise", "noise"])
def test_styled_conv_matches_float64_composition(upsample, with_noise):
    from models.stylegan2_blocks import StyledConv
    from vts import engine
    dev = _dev()
    seed, n, ci, co, sdim, h = 2100, 2, 24, 40, 32, 12
    sd = sg.test_weights(styled_shapes(ci, co, 3, sdim), seed)
    x, st = detrand.uniform((n, ci, h, h), seed, "x"), detrand.uniform((n, sdim), seed, "style")
    oh = 2 * h if upsample else h
    noise = detrand.uniform((n, 1, oh, oh), seed, "noise") if with_noise else None
    sdo, (xo, so, no) = _leaves(sd, x, st, noise)
    yo = oracle_styled_conv(sdo, xo, so, no, upsample)
    cot = detrand.uniform(tuple(yo.shape), seed, "cot")
    (yo * cot.double()).sum().backward()
    m = _load(StyledConv(ci, co, 3, sdim, upsample=upsample, inject_noise=with_noise), sd)
    y, saved = engine.styled_conv_forward(m, x.to(dev), st.to(dev), None if noise is None else noise.to(dev))
    dx, dstyle = engine.styled_conv_backward(m, saved, cot.to(dev))
    figs = {"out": rel(y, yo), "dx": rel(dx, xo.grad), "dstyle": rel(dstyle, so.grad)}
    named = dict(m.named_parameters())
    for k, v in sdo.items():
        if k == "noise.weight" and not with_noise:
            continue
        figs[k] = rel(named[k].grad, v.grad)
    print("StyledConv", "up" if upsample else "plain", "noise" if with_noise else "no noise", {k: "%.2e" % v for k, v in figs.items()})
    for k, v in figs.items():
        assert v < BOUND, (k, v)
    once = {k: p.grad.clone() for k, p in named.items()}
    engine.styled_conv_backward(m, saved, cot.to(dev), accumulate=True)
    for k, p in named.items():
        if k == "noise.weight" and not with_noise:
            continue
        assert rel(p.grad, 2 * once[k]) < 1e-6, k


@pytest.mark.parametrize("with_skip", [False, True], ids=["noskip", "skip"])
def test_to_rgb_matches_float64_composition(with_skip):
    from models.stylegan2_blocks import ToRGB
    from vts import engine
    dev = _dev()
    seed, n, ci, sdim, h = 2200, 2, 24, 32, 12
    sd = sg.test_weights(torgb_shapes(ci, sdim), seed)
    x, st = detrand.uniform((n, ci, h, h), seed, "x"), detrand.uniform((n, sdim), seed, "style")
    skip = detrand.uniform((n, 3, h // 2, h // 2), seed, "skip") if with_skip else None
    sdo, (xo, so, ko) = _leaves(sd, x, st, skip)
    yo = oracle_to_rgb(sdo, xo, so, ko)
    cot = detrand.uniform(tuple(yo.shape), seed, "cot")
    (yo * cot.double()).sum().backward()
    m = _load(ToRGB(ci, sdim, upsample=with_skip), sd)
    y, saved = engine.to_rgb_forward(m, x.to(dev), st.to(dev), None if skip is None else skip.to(dev))
    dx, dstyle, dskip = engine.to_rgb_backward(m, saved, cot.to(dev))
    figs = {"out": rel(y, yo), "dx": rel(dx, xo.grad), "dstyle": rel(dstyle, so.grad)}
    if with_skip:
        figs["dskip"] = rel(dskip, ko.grad)
    else:
        assert dskip is None
    named = dict(m.named_parameters())
    figs.update({k: rel(named[k].grad, v.grad) for k, v in sdo.items()})
    print("ToRGB", "skip" if with_skip else "no skip", {k: "%.2e" % v for k, v in figs.items()})
    for k, v in figs.items():
        assert v < BOUND, (k, v)


def test_synthesis_step_matches_float64_composition():
    """one step of the reference's synthesis loop (:604-611): StyledConv(up) -> StyledConv -> ToRGB(skip), ONE latent feeding all three,
    so its three gradients are summed; 512 channels, 8 x 8 -> 16 x 16"""
    from models.stylegan2_blocks import StyledConv, ToRGB
    from vts import engine
    dev = _dev()
    seed, n, ch, sdim, h = 2300, 2, 512, 512, 8
    sds = [sg.test_weights(styled_shapes(ch, ch, 3, sdim), seed), sg.test_weights(styled_shapes(ch, ch, 3, sdim), seed + 1),
           sg.test_weights(torgb_shapes(ch, sdim), seed + 2)]
    x, lat = detrand.uniform((n, ch, h, h), seed, "x"), detrand.uniform((n, sdim), seed, "latent")
    skip = detrand.uniform((n, 3, h, h), seed, "skip")
    nz = [detrand.uniform((n, 1, 2 * h, 2 * h), seed, "nz%d" % i) for i in range(2)]
    sdo = [{k: v.double().requires_grad_(True) for k, v in sd.items()} for sd in sds]
    xo, lo, ko = (t.double().requires_grad_(True) for t in (x, lat, skip))
    o1 = oracle_styled_conv(sdo[0], xo, lo, nz[0].double(), True)
    o2 = oracle_styled_conv(sdo[1], o1, lo, nz[1].double(), False)
    img = oracle_to_rgb(sdo[2], o2, lo, ko)
    cot = detrand.uniform(tuple(img.shape), seed, "cot")
    (img * cot.double()).sum().backward()
    m1 = _load(StyledConv(ch, ch, 3, sdim, upsample=True), sds[0])
    m2 = _load(StyledConv(ch, ch, 3, sdim), sds[1])
    m3 = _load(ToRGB(ch, sdim), sds[2])
    latd = lat.to(dev)
    y1, s1 = engine.styled_conv_forward(m1, x.to(dev), latd, nz[0].to(dev))
    y2, s2 = engine.styled_conv_forward(m2, y1, latd, nz[1].to(dev))
    y3, s3 = engine.to_rgb_forward(m3, y2, latd, skip.to(dev))
    g2, dl3, dskip = engine.to_rgb_backward(m3, s3, cot.to(dev))
    g1, dl2 = engine.styled_conv_backward(m2, s2, g2)
    dx, dl1 = engine.styled_conv_backward(m1, s1, g1)
    e_img = rel(y3, img)
    figs = {"dx": rel(dx, xo.grad), "dlatent": rel(dl1 + dl2 + dl3, lo.grad), "dskip": rel(dskip, ko.grad)}
    for i, (m, so) in enumerate(zip((m1, m2, m3), sdo)):
        named = dict(m.named_parameters())
        figs.update({"%d.%s" % (i, k): rel(named[k].grad, v.grad) for k, v in so.items()})
    print("synthesis step: image %.2e" % e_img, {k: "%.2e" % v for k, v in figs.items()})
    assert e_img < BOUND
    for k, v in figs.items():
        assert v < STACK_BOUND, (k, v)
