"""The CLIP image tower's input-gradient backward on the device (csrc/vts_vit.hip): the taped forward, the LayerNorm and attention
backward kernels, the tower backward with cotangents at the embedding and at tapped hidden states, the differentiable area
pre-processing, and the model-level path ClipVisual.features / features_backward.

Judges: torch autograd in float64 on the SAME fp16-valued weights, inputs and cotangents (tests/clip_bwd_restated.py, pinned by
tests/test_clip_bwd_cpu.py).  For every fp16-regime result the bound is the error of the reference's own arithmetic -- the same
computation under autograd with everything in fp16 -- recorded per case, at cotangent scale 1, in tests/golden/clip_visual_bwd.npz
(tools/make_clip_bwd_golden.py); fp32-only kernels are held to the project's 2e-5.  Every figure is printed before it is asserted; the
measured table is profiles/r11_clip_backward.md.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_bwd_restated as B
import clip_restated as R
from oracle import detrand

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return np.load(B.GOLDEN)


@functools.lru_cache(maxsize=None)
def _tower(cfg_items):
    from models.clip_visual import ClipVisual

    cfg = dict(cfg_items)
    net = ClipVisual(cfg)
    net.load_state_dict(R.test_weights(cfg, B.SEED))
    return net.to(DEV)


def _net(cfg):
    return _tower(tuple(sorted(cfg.items())))


@functools.lru_cache(maxsize=None)
def _judge(name, variant):
    """float64 autograd of one case and cotangent variant, computed once: (dx, embedding, states)"""
    cfg, batch = R.TOWER_CASES[name]
    d_out, used, d_hidden = B.cotangents(cfg, batch, B.TAPS[name], variant)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    return B.tower_grad(B.weights16(cfg), cfg, R.test_input(cfg, batch, B.SEED), d_out, used, d_hidden, torch.float64)


def _device_cotangents(name, variant, scale=1.0):
    cfg, batch = R.TOWER_CASES[name]
    d_out, used, d_hidden = B.cotangents(cfg, batch, B.TAPS[name], variant)
    return (None if d_out is None else (d_out.float() * scale).to(DEV)), used, [(d.float() * scale).to(DEV) for d in d_hidden]


# ---- 1. the taped forward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.TOWER_CASES))
def test_forward_tape(golden, name):
    """vts_clip_visual_forward_tape gives vts_clip_visual_forward's output to the bit, and each tapped hidden state is at least as accurate
    as the all-fp16 run's"""
    cfg, batch = R.TOWER_CASES[name]
    net, x, taps = _net(cfg), R.test_input(cfg, batch, B.SEED).to(DEV), B.TAPS[name]
    plain = net(x)
    emb, hidden, ctx = net.forward_taped(x, taps)
    assert torch.equal(emb, plain) and ctx["taps"] == taps and len(hidden) == len(taps)
    _, _, states = _judge(name, "c")
    t = (cfg["resolution"] // cfg["patch"]) ** 2 + 1
    for l, h in zip(taps, hidden):
        err, bound = R.rel_l2(h.cpu(), states[l]), float(golden["%s_hid%d_err16" % (name, l)])
        print("forward_tape %s hidden %d: rel-L2 %.3e (all-fp16 reference arithmetic %.3e)" % (name, l, err, bound))
        assert h.dtype == torch.float32 and tuple(h.shape) == (batch, t, cfg["width"]) and bool(torch.isfinite(h).all())
        assert err <= bound
    assert torch.equal(net(x), plain)


# ---- 2. LayerNorm backward ------------------------------------------------------------------------------------------------------------
def _ln_case(rows, width):
    x = detrand.uniform((rows, width), 6, "lnx") * 3.0 + 0.7
    gam = (1.0 + 0.2 * detrand.uniform((width,), 6, "lng")).half()
    dy, g = detrand.uniform((rows, width), 6, "lndy"), detrand.uniform((rows, width), 6, "lnstream") * 2.0
    x64 = x.double().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.layer_norm(x64, (width,), gam.double(), None, 1e-5), x64, dy.double())
    return x, gam, dy, g, ref


@pytest.mark.parametrize("rows", [1, 5, 50, 200])
@pytest.mark.parametrize("width", [128, 768])
def test_layernorm_rows_bwd(rows, width):
    from vts import ops

    x, gam, dy, g, ref = _ln_case(rows, width)
    got = ops.layernorm_rows_bwd(dy.to(DEV), x.to(DEV), gam.to(DEV))
    err = R.rel_l2(got.cpu(), ref)
    acc, acc16 = ops.layernorm_rows_bwd(dy.to(DEV), x.to(DEV), gam.to(DEV), out=g.to(DEV), accumulate=True, half_out=True)
    err_acc = R.rel_l2(acc.cpu(), g.double() + ref)
    print("layernorm_rows_bwd %d x %d: rel-L2 %.3e, accumulated into the stream %.3e" % (rows, width, err, err_acc))
    assert err <= 2e-5 and err_acc <= 2e-5
    assert acc16.dtype == torch.float16 and torch.equal(acc16, acc.half())
    assert torch.equal(ops.layernorm_rows_bwd(dy.to(DEV), x.to(DEV), gam.to(DEV)), got)


def test_layernorm_rows_bwd_class_token_rows():
    """ln_post's form: the rows are the class tokens of a [N, T, W] stream (stride T * W), and so are the gradient rows added into"""
    from vts import ops

    n, t, width = 3, 50, 128
    x, gam, dy, g, ref = _ln_case(n * t, width)
    dy = dy[:n].contiguous()
    x64 = x.double()[::t].clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.layer_norm(x64, (width,), gam.double(), None, 1e-5), x64, dy.double())
    xd, gd = x.to(DEV), g.to(DEV)
    ops.layernorm_rows_bwd(dy.to(DEV), xd[::t], gam.to(DEV), out=gd[::t], accumulate=True)
    want = g.double().clone()
    want[::t] += ref
    err = R.rel_l2(gd.cpu()[::t], want[::t])
    print("layernorm_rows_bwd class-token rows (stride %d): rel-L2 %.3e" % (t * width, err))
    assert err <= 2e-5
    keep = torch.ones(n * t, dtype=torch.bool)
    keep[::t] = False
    assert torch.equal(gd.cpu()[keep], g[keep]), "rows between the class tokens were touched"


# ---- the GEMM's side buffer: the tape's pre-activation and the QuickGELU-derivative epilogue --------------------------------------------
@pytest.mark.parametrize("m,n,k", [(37, 384, 128), (200, 3072, 768), (50, 768, 3072)])
def test_gemm_quickgelu_side_buffer(m, n, k):
    """QuickGELU with the side buffer leaves the fp16 pre-activation there and the same output; QuickGELU_BWD multiplies the product by
    s (1 + 1.702 h (1 - s)), s = sigmoid(1.702 h), of the saved h: fp32 epilogue on fp16 operands, 2e-5 against float64; both with and
    without the K split"""
    import math

    from vts import ops

    a = (detrand.uniform((m, k), 4, "ga") * math.sqrt(3.0)).half()
    w = (detrand.uniform((n, k), 4, "gw") * math.sqrt(3.0 / k)).half()
    b = (detrand.uniform((n,), 4, "gb") * 0.5).half()
    h = (detrand.uniform((m, n), 4, "gh") * 3.0).half()
    ad, wd, bd, hd = a.to(DEV), w.to(DEV), b.to(DEV), h.to(DEV)
    pre = torch.full((m, n), float("nan"), dtype=torch.float16, device=DEV)
    act = ops.gemm_f16(ad, wd, bias=bd, epilogue="quickgelu", out_dtype=torch.float16, aux=pre)
    assert torch.equal(act, ops.gemm_f16(ad, wd, bias=bd, epilogue="quickgelu", out_dtype=torch.float16))
    assert torch.equal(pre, ops.gemm_f16(ad, wd, bias=bd, out_dtype=torch.float16))
    s = torch.sigmoid(1.702 * h.double())
    ref = (a.double() @ w.double().t()) * (s * (1 + 1.702 * h.double() * (1 - s)))
    got = ops.gemm_f16(ad, wd, epilogue="quickgelu_bwd", aux=hd)
    err = R.rel_l2(got.cpu(), ref)
    print("gemm_f16 quickgelu_bwd M %d N %d K %d: rel-L2 %.3e" % (m, n, k, err))
    assert err <= 2e-5
    assert torch.equal(ops.gemm_f16(ad, wd, epilogue="quickgelu_bwd", aux=hd, out_dtype=torch.float16), got.half())
    with pytest.raises(RuntimeError, match="pre-activation"):
        ops.gemm_f16(ad, wd, epilogue="residual", out=torch.zeros(m, n, device=DEV), aux=hd)


# ---- 3. attention backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attention_bwd_against_float64(golden, name):
    """2 heads, batch 3: dqkv against float64 autograd of clip_restated.attention on the fp16-valued qkv and cotangent; the whole and each
    of the q, k and v thirds are held to the all-fp16 error of the case"""
    from vts import ops

    t = R.ATTN_CASES[name]
    qkv, d = R.attn_input(t, B.SEED), B.attn_cot(t)
    ref = B.attention_grad(qkv, d, t, torch.float64)
    got = ops.vit_attention_bwd(qkv.to(DEV), d.to(DEV), 3, t, 2)
    bound = float(golden[name + "_bwd_err16"])
    err = R.rel_l2(got.cpu(), ref)
    thirds = [R.rel_l2(got.cpu()[:, i * 128:(i + 1) * 128], ref[:, i * 128:(i + 1) * 128]) for i in range(3)]
    print("vit_attention_bwd T %d: rel-L2 %.3e, dq %.3e dk %.3e dv %.3e (all-fp16 reference arithmetic %.3e)" % ((t, err) + tuple(thirds) + (bound,)))
    assert got.dtype == torch.float16 and got.shape == qkv.shape and bool(torch.isfinite(got).all())
    assert err <= bound and max(thirds) <= bound
    assert torch.equal(ops.vit_attention_bwd(qkv.to(DEV), d.to(DEV), 3, t, 2), got)


# ---- 4. / 5. / 8. the tower backward ---------------------------------------------------------------------------------------------------
def _backward(name, variant, scale=1.0):
    cfg, batch = R.TOWER_CASES[name]
    net, x = _net(cfg), R.test_input(cfg, batch, B.SEED).to(DEV)
    d_out, used, d_hidden = _device_cotangents(name, variant, scale)
    _, _, ctx = net.forward_taped(x, used)
    return net.input_gradient(ctx, d_out, d_hidden)


@pytest.mark.parametrize("name,variant", B.BWD_CASES)
def test_tower_backward(golden, name, variant):
    """cotangents at the embedding (a), at the tapped hidden states (b), at both (c): dx against float64 autograd, no less accurate than
    the all-fp16 autograd of the same variant; finite; bit-identical when the forward and the backward are repeated"""
    cfg, batch = R.TOWER_CASES[name]
    got = _backward(name, variant)
    ref, bound = _judge(name, variant)[0], float(golden["%s_%s_err16" % (name, variant)])
    err = R.rel_l2(got.cpu(), ref)
    print("clip_visual_backward %s %s: rel-L2 %.3e (all-fp16 reference arithmetic %.3e)" % (name, variant, err, bound))
    assert got.dtype == torch.float32 and tuple(got.shape) == (batch, 3, cfg["resolution"], cfg["resolution"]) and bool(torch.isfinite(got).all())
    assert err <= bound
    assert torch.equal(_backward(name, variant), got)


@pytest.mark.parametrize("exponent", [-12, 8])
@pytest.mark.parametrize("name", ["small224_b2", "vitb32_b1"])
def test_tower_backward_cotangent_scale(golden, name, exponent):
    """every cotangent multiplied by 2^-12 (a GAN loss's gradients are small) and by 2^8: the error stays within the SCALE-1 bound, which
    the all-fp16 autograd does not manage (its operands underflow); the device normalises the cotangents by a power of two"""
    got = _backward(name, "c", 2.0 ** exponent)
    ref, bound = _judge(name, "c")[0] * 2.0 ** exponent, float(golden["%s_c_err16" % name])
    err = R.rel_l2(got.cpu(), ref)
    same = torch.equal(got, _backward(name, "c") * 2.0 ** exponent)
    print("clip_visual_backward %s c at cotangent scale 2^%d: rel-L2 %.3e (scale-1 bound %.3e); equals the scaled scale-1 result: %s"
          % (name, exponent, err, bound, same))
    assert bool(torch.isfinite(got).all()) and err <= bound


@pytest.mark.parametrize("name", ["small64_b3", "vitb32_b1"])
def test_forward_tape_and_backward_in_one_graph(name):
    """the two C entries captured in one graph on buffers of their own: two replays give the eager result bit for bit"""
    from vts import ops

    cfg, batch = R.TOWER_CASES[name]
    net, x = _net(cfg), R.test_input(cfg, batch, B.SEED).to(DEV)
    d_out, used, d_hidden = _device_cotangents(name, "c")
    eager_dx, eager_emb = _backward(name, "c"), net(x)
    ccfg, flat, flat_t = net._ccfg, net.flat_weights(), net.flat_weights_t()
    tape, ws_f, ws_b = (torch.empty(k, dtype=torch.float32, device=DEV) for k in (
        ops.clip_visual_tape_floats(ccfg, batch), ops.clip_visual_forward_ws_floats(ccfg, batch), ops.clip_visual_backward_ws_floats(ccfg, batch)))
    dh = torch.stack(d_hidden).contiguous()
    emb, dx = torch.zeros_like(eager_emb), torch.zeros_like(eager_dx)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(), capture_error_mode="thread_local"):
        ops.clip_visual_forward_tape(ccfg, flat, x, tape, out=emb, ws=ws_f)
        ops.clip_visual_backward(ccfg, flat, flat_t, tape, batch, d_out=d_out, taps=used, d_hidden=dh, dx=dx, ws=ws_b)
    for _ in range(2):
        emb.zero_()
        dx.zero_()
        tape.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(emb, eager_emb) and torch.equal(dx, eager_dx)


# ---- 6. the differentiable front end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,res,n", [(64, 64, 64, 2), (448, 448, 224, 1), (200, 300, 224, 2), (100, 100, 224, 1), (1024, 1024, 224, 1)])
def test_area_preprocess(h, w, res, n):
    """identity windows, exact 2 x 2 windows, a non-integer ratio with upscaling in the other axis, upscaling, and the training size:
    forward (fp32 output) and backward against F.interpolate(mode='area') and its autograd in float64; the fp16 output is the fp32
    output rounded"""
    from vts import ops

    x = detrand.uniform((n, 3, h, w), 21, "area%dx%d" % (h, w))
    dy = detrand.uniform((n, 3, res, res), 21, "area_dy%dx%d" % (h, w))
    x64 = x.double().requires_grad_(True)
    ref = B.area_front(x64, res, torch.float64)
    (dref,) = torch.autograd.grad(ref, x64, dy.double())
    y32 = ops.clip_area_preprocess(x.to(DEV), res, out_dtype=torch.float32)
    y16 = ops.clip_area_preprocess(x.to(DEV), res)
    dx = ops.clip_area_preprocess_bwd(dy.to(DEV), h, w)
    e_f, e_b = R.rel_l2(y32.cpu(), ref.detach()), R.rel_l2(dx.cpu(), dref)
    print("clip_area_preprocess %dx%d -> %d: forward rel-L2 %.3e, backward %.3e" % (h, w, res, e_f, e_b))
    assert e_f <= 2e-5 and e_b <= 2e-5
    assert y16.dtype == torch.float16 and torch.equal(y16, y32.half())
    assert torch.equal(ops.clip_area_preprocess_bwd(dy.to(DEV), h, w), dx)


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------
def test_features_end_to_end(golden):
    """ClipVisual.features / features_backward on a [2, 3, 96, 80] image, taps (1, 2) plus the embedding, against float64 autograd of
    (area pre-processing, value rounded to fp16 with a straight-through gradient, tower)"""
    cfg, taps = B.E2E["cfg"], B.E2E["taps"]
    net, img = _net(cfg), B.e2e_image()
    d_out, _, d_hidden = B.cotangents(cfg, img.shape[0], taps, "c")
    ref = B.e2e_grad(B.weights16(cfg), img, d_out, taps, d_hidden, torch.float64)

    def run():
        emb, hidden, ctx = net.features(img.to(DEV), taps)
        assert tuple(emb.shape) == (2, cfg["output_dim"]) and [tuple(h.shape) for h in hidden] == [(2, 5, cfg["width"])] * 2
        return net.features_backward(ctx, d_out.float().to(DEV), [d.float().to(DEV) for d in d_hidden])

    got = run()
    err, bound = R.rel_l2(got.cpu(), ref), float(golden["e2e_err16"])
    print("features / features_backward 96x80: rel-L2 %.3e (all-fp16 reference arithmetic %.3e)" % (err, bound))
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(img.shape) and bool(torch.isfinite(got).all())
    assert err <= bound
    assert torch.equal(run(), got)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------
def test_backward_refusals():
    from vts import lib as L
    from vts import ops

    lib = L.load()
    for bad in (L.ClipVisualCfg(768, 12, 12, 16, 224, 512), L.ClipVisualCfg(768, 12, 8, 32, 224, 512)):      # ViT-B/16; head dimension 96
        for fn in (lib.vts_clip_visual_tape_floats, lib.vts_clip_visual_backward_ws_floats):
            assert fn(ctypes.byref(bad), 1) == -1 and b"out of scope" in lib.vts_last_error()
        assert lib.vts_clip_visual_weight_t_halfs(ctypes.byref(bad)) == -1
    cfg, batch = R.TOWER_CASES["small64_b3"]
    net, x = _net(cfg), R.test_input(cfg, batch, B.SEED).to(DEV)
    _, _, ctx = net.forward_taped(x, (1, 2))
    tape, _, ws = net._backward_buffers(batch, x.device)
    ccfg, flat, flat_t = net._ccfg, net.flat_weights(), net.flat_weights_t()
    d_out = torch.ones(batch, cfg["output_dim"], device=DEV)
    dh = torch.ones(2, batch, 5, cfg["width"], device=DEV)
    dx = torch.zeros(batch, 3, 64, 64, device=DEV)

    def call(c=ccfg, d=d_out, taps=(1, 2), tape_n=tape.numel(), ws_n=ws.numel()):
        arr = (ctypes.c_int * 4)(*taps)
        return lib.vts_clip_visual_backward(ctypes.byref(c), flat.data_ptr(), flat_t.data_ptr(), tape.data_ptr(), tape_n, batch, L.ptr(d), arr, len(taps),
                                            dh.data_ptr(), dx.data_ptr(), ws.data_ptr(), ws_n, L.stream())

    assert call() == 0
    assert call(c=L.ClipVisualCfg(768, 12, 12, 16, 224, 512)) == L.ERR_UNSUPPORTED and b"out of scope" in lib.vts_last_error()
    for taps in ((1, 3), (2, 1), (1, 1), (-1, 2)):
        assert call(taps=taps) == -1 and b"ascend" in lib.vts_last_error(), taps
    assert call(d=None, taps=()) == -1 and b"no cotangent" in lib.vts_last_error()
    assert call(tape_n=tape.numel() - 1) == -1 and b"tape of" in lib.vts_last_error()
    assert call(ws_n=ws.numel() - 1) == -1 and b"workspace of" in lib.vts_last_error()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="no cotangent"):
        net.input_gradient(ctx)
    with pytest.raises(ValueError, match="ascending block numbers"):
        net.forward_taped(x, (2, 1))
    assert ops.clip_visual_weight_t_halfs(ccfg) == flat_t.numel()
