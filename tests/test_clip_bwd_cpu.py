"""The judges of the CLIP tower's backward, pinned on the CPU (no GPU, no kernel launch): the float64 autograd judge of
tests/clip_bwd_restated.py is held against a backward of one block and one LayerNorm written out by hand (so that autograd is not its own
witness), the restated tower with hidden states against clip_restated.tower, the fixture of tools/make_clip_bwd_golden.py against the
seeds, and the new entries' declarations, bindings and host-side handling are checked."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_bwd_restated as B
import clip_restated as R
from oracle import detrand


def _ln_bwd(dy, x, gamma, eps=1e-5):
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    rstd = (var + eps) ** -0.5
    xh, a = (x - mean) * rstd, gamma * dy
    return rstd * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))


def _block_bwd(sd, k, x, g, n, t, heads):
    """dL/dx of clip_bwd_restated.block for the cotangent g of its output, by the chain rule, term by term"""
    w = x.shape[1]
    hd = w // heads
    h1 = F.layer_norm(x, (w,), sd[k + "ln_1.weight"], sd[k + "ln_1.bias"], 1e-5)
    qkv = h1 @ sd[k + "attn.in_proj_weight"].t() + sd[k + "attn.in_proj_bias"]
    q, kk, v = (u.reshape(n, t, heads, hd).transpose(1, 2) for u in qkv.split(w, dim=1))
    p = torch.softmax(q @ kk.transpose(-1, -2) * hd ** -0.5, dim=-1)
    att = (p @ v).transpose(1, 2).reshape(n * t, w)
    xm = x + att @ sd[k + "attn.out_proj.weight"].t() + sd[k + "attn.out_proj.bias"]
    f = F.layer_norm(xm, (w,), sd[k + "ln_2.weight"], sd[k + "ln_2.bias"], 1e-5) @ sd[k + "mlp.c_fc.weight"].t() + sd[k + "mlp.c_fc.bias"]
    s = torch.sigmoid(1.702 * f)
    # MLP half
    df = (g @ sd[k + "mlp.c_proj.weight"]) * (s * (1 + 1.702 * f * (1 - s)))
    gm = g + _ln_bwd(df @ sd[k + "mlp.c_fc.weight"], xm, sd[k + "ln_2.weight"])
    # attention half
    do = (gm @ sd[k + "attn.out_proj.weight"]).reshape(n, t, heads, hd).transpose(1, 2)
    dv = p.transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    dq, dk = ds @ kk * hd ** -0.5, ds.transpose(-1, -2) @ q * hd ** -0.5
    dqkv = torch.cat([u.transpose(1, 2).reshape(n * t, w) for u in (dq, dk, dv)], dim=1)
    return gm + _ln_bwd(dqkv @ sd[k + "attn.in_proj_weight"], x, sd[k + "ln_1.weight"])


def test_autograd_judge_equals_hand_written_backward():
    cfg, n = R.SMALL224, 2
    t, w = 50, cfg["width"]
    sd = {k: v.double() for k, v in B.weights16(cfg).items()}
    x = (detrand.uniform((n * t, w), 3, "blk_x") * 1.5).double()
    g = detrand.uniform((n * t, w), 3, "blk_g").double()
    xr = x.clone().requires_grad_(True)
    (auto,) = torch.autograd.grad(B.block(sd, "transformer.resblocks.1.", xr, n, t, cfg["heads"]), xr, g)
    hand = _block_bwd(sd, "transformer.resblocks.1.", x, g, n, t, cfg["heads"])
    assert float(auto.abs().max()) > 0.1 and float((auto - hand).abs().max()) <= 1e-10, float((auto - hand).abs().max())
    gam, bet = sd["ln_post.weight"], sd["ln_post.bias"]
    xr = x.clone().requires_grad_(True)
    (auto,) = torch.autograd.grad(R._ln(xr, gam, bet), xr, g)
    assert float((auto - _ln_bwd(g, x, gam)).abs().max()) <= 1e-10


@pytest.mark.parametrize("name", ["small64_b3", "small224_b2"])
def test_tower_with_states_equals_the_restated_tower(name):
    cfg, batch = R.TOWER_CASES[name]
    sd = {k: v.double() for k, v in B.weights16(cfg).items()}
    x = R.test_input(cfg, batch, B.SEED).double()
    out, states = B.tower_states(sd, cfg, x)
    assert len(states) == cfg["layers"] + 1 and float((out - R.tower(sd, cfg, x)).abs().max()) <= 1e-12


def _close(got, want):
    # the all-fp16 error is a norm over ~1e5 rounding errors: another thread count or BLAS blocking moves single roundings, not the norm
    return abs(got - want) <= 0.02 * want


def test_fixture_is_reproduced_from_the_seeds():
    z = np.load(B.GOLDEN)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    for name in ("small64_b3", "small224_b2"):
        cfg, batch = R.TOWER_CASES[name]
        sd16, x16, taps = B.weights16(cfg), R.test_input(cfg, batch, B.SEED), B.TAPS[name]
        for variant in "abc":
            d_out, used, d_hidden = B.cotangents(cfg, batch, taps, variant)
            g64, _, s64 = B.tower_grad(sd16, cfg, x16, d_out, used, d_hidden, torch.float64)
            g16, _, s16 = B.tower_grad(sd16, cfg, x16, d_out, used, d_hidden, torch.float16)
            assert _close(R.rel_l2(g16, g64), float(z["%s_%s_err16" % (name, variant)])), (name, variant, R.rel_l2(g16, g64))
        for l in taps:
            assert _close(R.rel_l2(s16[l], s64[l]), float(z["%s_hid%d_err16" % (name, l)])), (name, l)
    for name, t in R.ATTN_CASES.items():
        qkv, d = R.attn_input(t, B.SEED), B.attn_cot(t)
        e16 = R.rel_l2(B.attention_grad(qkv, d, t, torch.float16), B.attention_grad(qkv, d, t, torch.float64))
        assert _close(e16, float(z[name + "_bwd_err16"])), (name, e16)
    keys = ["%s_%s_err16" % c for c in B.BWD_CASES] + ["%s_hid%d_err16" % (n, l) for n in R.TOWER_CASES for l in B.TAPS[n]]
    keys += [n + "_bwd_err16" for n in R.ATTN_CASES] + ["e2e_err16"]
    assert sorted(z.files) == sorted(keys)
    for k in keys:
        assert 1e-5 < float(z[k]) < 1e-2, (k, float(z[k]))      # the level half precision gives
    assert os.path.getsize(B.GOLDEN) < 64 * 1024


NEW_ENTRIES = ["vts_gemm_f16_aux", "vts_layernorm_rows_bwd", "vts_vit_attention_bwd", "vts_clip_visual_tape_floats", "vts_clip_visual_forward_tape",
               "vts_clip_visual_weight_t_halfs", "vts_clip_visual_backward_ws_floats", "vts_clip_visual_backward", "vts_clip_area_preprocess",
               "vts_clip_area_preprocess_bwd"]


def test_entries_are_declared_and_bound():
    from vts import lib as L

    header = open(os.path.join(R.ROOT, "include", "vts.h")).read()
    lib = L.load()
    for name in NEW_ENTRIES:
        decl = re.search(r"^(int|int64_t) %s\(([^;]*)\);" % name, header, re.M | re.S)
        assert decl, name + " is not declared in include/vts.h"
        assert name in L.SYMBOLS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == decl.group(2).count(",") + 1, name
    assert "#define VTS_GEMM_QUICKGELU_BWD 3" in header


def test_features_on_the_cpu_are_refused_and_host_side_layout():
    from models.clip_visual import ClipVisual

    cfg = dict(R.SMALL64, output_dim=48)
    net = ClipVisual(cfg, seed=1)
    with pytest.raises(RuntimeError, match="HIP path only"):
        net.features(torch.zeros(1, 3, 96, 80))
    with pytest.raises(RuntimeError, match="HIP path only"):
        net.forward_taped(torch.zeros(1, 3, 64, 64, dtype=torch.float16))
    # the transposed buffer: documented order, proj padded to a multiple of 32 columns with zeros; built on demand only
    assert net._flat_t is None
    w, kp = cfg["width"], 3 * 32 * 32
    ft = net.flat_weights_t()
    assert ft.dtype == torch.float16 and ft.numel() == kp * w + cfg["layers"] * 12 * w * w + w * 64
    assert torch.equal(ft[:kp * w].view(kp, w), net.conv1.weight.reshape(w, kp).t().half())
    blk = net.transformer.resblocks[0]
    assert torch.equal(ft[kp * w:kp * w + 3 * w * w].view(w, 3 * w), blk.attn.in_proj_weight.t().half())
    tail = ft[-w * 64:].view(w, 64)
    assert torch.equal(tail[:, :48], net.proj.half()) and not bool(tail[:, 48:].any())
    net.load_state_dict(net.state_dict())
    assert net._flat_t is None and net._bwd == {}
