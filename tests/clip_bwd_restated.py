"""Judges of the CLIP image tower's input-gradient backward (TEST INFRASTRUCTURE; imported by test_clip_bwd_cpu.py / test_clip_bwd_gpu.py
and tools/make_clip_bwd_golden.py).  The tower, its attention core and its LayerNorm are clip_restated's, unchanged; this file adds the
cases, the seeded cotangents (oracle/detrand.py, fp16-valued), the restated tower that also returns its hidden states, the differentiable
front end, and the judge: torch autograd in float64 on the fp16-valued weights, inputs and cotangents.  The same computation under
autograd with everything in fp16 (LayerNorm in fp32, as clip_restated._ln) is the reference's own arithmetic: its relative L2 error
against the judge, at cotangent scale 1, is the bound recorded per case in tests/golden/clip_visual_bwd.npz.
"""
import os

import torch
import torch.nn.functional as F

import clip_restated as R
from oracle import detrand

SEED = 77
GOLDEN = os.path.join(R.ROOT, "tests", "golden", "clip_visual_bwd.npz")
# blocks whose hidden state is tapped, per tower case (block l's output is tape index l)
TAPS = {"small64_b3": (1, 2), "small224_b2": (1, 2), "vitb32_b1": (4, 8, 12), "vitb32_b4": (4, 8, 12)}
# cotangent variants: (embedding cotangent, hidden-state cotangents)
VARIANTS = {"a": (True, False), "b": (False, True), "c": (True, True)}
BWD_CASES = [(n, v) for n in ("small64_b3", "small224_b2", "vitb32_b1") for v in "abc"] + [("vitb32_b4", "c")]
E2E = dict(cfg=R.SMALL64, shape=(2, 3, 96, 80), taps=(1, 2))


def tower_states(sd, cfg, x):
    """clip_restated.tower, also returning the residual stream after ln_pre (index 0) and after every block (index l), each [n * t, w]"""
    w, p, heads = cfg["width"], cfg["patch"], cfg["heads"]
    n, g = x.shape[0], cfg["resolution"] // cfg["patch"]
    t = g * g + 1
    rows = x.reshape(n, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * p * p)
    tok = (rows @ sd["conv1.weight"].reshape(w, -1).t()).reshape(n, g * g, w)
    x = torch.cat([sd["class_embedding"].expand(n, 1, w), tok], dim=1) + sd["positional_embedding"]
    x = R._ln(x, sd["ln_pre.weight"], sd["ln_pre.bias"]).reshape(n * t, w)
    states = [x]
    for i in range(cfg["layers"]):
        x = block(sd, "transformer.resblocks.%d." % i, x, n, t, heads)
        states.append(x)
    cls = R._ln(x.reshape(n, t, w)[:, 0, :], sd["ln_post.weight"], sd["ln_post.bias"])
    return cls @ sd["proj"], states


def block(sd, k, x, n, t, heads):
    h = R._ln(x, sd[k + "ln_1.weight"], sd[k + "ln_1.bias"])
    a = R.attention(h @ sd[k + "attn.in_proj_weight"].t() + sd[k + "attn.in_proj_bias"], n, t, heads)
    x = x + (a @ sd[k + "attn.out_proj.weight"].t() + sd[k + "attn.out_proj.bias"])
    h = R._ln(x, sd[k + "ln_2.weight"], sd[k + "ln_2.bias"])
    h = h @ sd[k + "mlp.c_fc.weight"].t() + sd[k + "mlp.c_fc.bias"]
    h = h * torch.sigmoid(1.702 * h)
    return x + (h @ sd[k + "mlp.c_proj.weight"].t() + sd[k + "mlp.c_proj.bias"])


def weights16(cfg, seed=SEED):
    return {k: v.half() for k, v in R.test_weights(cfg, seed).items()}


def cot_out(cfg, batch, seed=SEED):
    return detrand.uniform((batch, cfg["output_dim"]), seed, "d_out").half()


def cot_hidden(cfg, batch, taps, seed=SEED):
    t = (cfg["resolution"] // cfg["patch"]) ** 2 + 1
    return [detrand.uniform((batch, t, cfg["width"]), seed, "d_hidden_%d" % l).half() for l in taps]


def cotangents(cfg, batch, taps, variant, seed=SEED):
    """(d_out or None, taps used, [d_hidden ...]) of a variant, fp16"""
    use_out, use_hid = VARIANTS[variant]
    return (cot_out(cfg, batch, seed) if use_out else None, tuple(taps) if use_hid else (), cot_hidden(cfg, batch, taps, seed) if use_hid else [])


def tower_grad(sd16, cfg, x16, d_out, taps, d_hidden, dtype):
    """autograd of tower_states in `dtype` (weights, input and cotangents cast from their fp16 values): the gradient with respect to the
    input, plus the forward's embedding and tapped hidden states"""
    sd = {k: v.to(dtype) for k, v in sd16.items()}
    x = x16.to(dtype).requires_grad_(True)
    out, states = tower_states(sd, cfg, x)
    outs, cots = [], []
    if d_out is not None:
        outs.append(out)
        cots.append(d_out.to(dtype))
    for l, d in zip(taps, d_hidden):
        outs.append(states[l])
        cots.append(d.to(dtype).reshape(states[l].shape))
    (dx,) = torch.autograd.grad(outs, x, cots)
    return dx.detach(), out.detach(), [s.detach() for s in states]


def attn_cot(tokens, seed=SEED):
    return detrand.uniform((3 * tokens, 128), seed, "attn_dout_%d" % tokens).half()


def attention_grad(qkv16, d16, tokens, dtype):
    qkv = qkv16.to(dtype).requires_grad_(True)
    (g,) = torch.autograd.grad(R.attention(qkv, 3, tokens, 2), qkv, d16.to(dtype))
    return g.detach()


def area_front(image, res, dtype):
    """x * 0.5 + 0.5 -> F.interpolate(mode='area') -> CLIP's normalisation, in `dtype`"""
    mean = torch.tensor(R.CLIP_MEAN, dtype=dtype)[None, :, None, None]
    std = torch.tensor(R.CLIP_STD, dtype=dtype)[None, :, None, None]
    return (F.interpolate(image.to(dtype) * 0.5 + 0.5, size=(res, res), mode="area") - mean) / std


def e2e_image(seed=SEED):
    return detrand.uniform(E2E["shape"], seed, "e2e_image")


def e2e_grad(sd16, image, d_out, taps, d_hidden, dtype):
    """the whole differentiable path.  float64: the judge -- area pre-processing in float64, its value rounded to fp16 with a
    straight-through gradient, the tower in float64.  float16: the reference's own arithmetic -- the pre-processing in fp32 (torch
    has no half-precision area pooling on the CPU), cast to fp16, the tower and every gradient through it in fp16."""
    cfg = E2E["cfg"]
    front = torch.float64 if dtype == torch.float64 else torch.float32
    img = image.to(front).requires_grad_(True)
    v = area_front(img, cfg["resolution"], front)
    x = v + (v.half().to(front) - v).detach() if dtype == torch.float64 else v.half()
    sd = {k: w.to(dtype) for k, w in sd16.items()}
    out, states = tower_states(sd, cfg, x)
    outs, cots = [out], [d_out.to(dtype)]
    for l, d in zip(taps, d_hidden):
        outs.append(states[l])
        cots.append(d.to(dtype).reshape(states[l].shape))
    (dimg,) = torch.autograd.grad(outs, img, cots)
    return dimg.detach()
