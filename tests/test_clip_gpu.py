"""skitG's style encoder on the device: the CLIP ViT image tower's kernels (csrc/vts_vit.hip), its one-call C entry and the model path.

Judges: float64 on the SAME fp16-rounded operands (tests/clip_restated.py, pinned by tests/test_clip_cpu.py); for the tower and the
attention core the bound is the error of the reference's own arithmetic -- the all-fp16 run the encoder replaces -- recorded per case in
tests/golden/clip_visual.npz (tools/make_clip_golden.py).  Every figure is printed before it is asserted.

Worst figures measured on one MI355X (relative L2 against float64; in brackets the bound): GEMM on random data 1.0e-7, with QuickGELU
1.2e-7 (2e-5); LayerNorm 7.0e-8 (2e-5); attention 2.08e-4 at T 5 (all-fp16 reference arithmetic 3.19e-4); tower 3.47e-4 on the 5-token
case (7.96e-4), ViT-B/32 2.74e-4 at batch 1 (1.07e-3) and 2.91e-4 at batch 4 (1.20e-3); integer GEMMs and the pre-processing exact.
The full table is profiles/r10_clip_style.md.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
from torch.utils.data import default_collate

import clip_restated as R
from oracle import detrand

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 77      # tools/make_clip_golden.py


def _ints(shape, name, lo=-2, hi=2):
    """small integers from the deterministic generator: every product and partial sum is exact in fp16 / fp32"""
    return torch.floor((detrand.uniform(shape, 9, name) * 0.5 + 0.5) * (hi - lo + 1) + lo).clamp_(lo, hi)


@functools.lru_cache(maxsize=None)
def _int_case(n, k):
    a, w = _ints((200, k), "A%dx%d" % (n, k)), _ints((n, k), "W%dx%d" % (n, k))
    bias, res = _ints((n,), "b%d" % n, -8, 8), _ints((200, n), "r%d" % n, -64, 64)
    return a, w, bias, res, a.double() @ w.double().t()


@pytest.mark.parametrize("m", [1, 5, 50, 150, 200])
@pytest.mark.parametrize("n,k", [(32, 128), (384, 128), (768, 3072), (512, 768)])
def test_gemm_lane_maps_exact(m, n, k):
    """integer operands in {-2 .. 2}: every sum is exact in fp32, so the fp32 output must EQUAL the float64 product -- any error in the
    A / B / accumulator lane maps of v_mfma_f32_16x16x32_f16, the row-tail masking, the wave split or the K split shows as a mismatch"""
    from vts import ops

    a, w, bias, res, prod = _int_case(n, k)
    ad, wd, bd = a[:m].half().to(DEV), w.half().to(DEV), bias.half().to(DEV)
    assert float(prod.abs().max()) < 2 ** 24
    got = ops.gemm_f16(ad, wd)
    assert torch.equal(got.cpu().double(), prod[:m]), "no epilogue"
    got = ops.gemm_f16(ad, wd, bias=bd)
    assert torch.equal(got.cpu().double(), prod[:m] + bias.double()), "bias"
    out = res[:m].to(DEV).contiguous()
    ops.gemm_f16(ad, wd, bias=bd, epilogue="residual", out=out)
    assert torch.equal(out.cpu().double(), res[:m].double() + prod[:m] + bias.double()), "residual"


def test_gemm_refuses_other_shapes():
    from vts import lib as L
    from vts import ops

    a, w = torch.zeros(4, 48, dtype=torch.float16, device=DEV), torch.zeros(16, 48, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.gemm_f16(a, w)
    a, w = torch.zeros(4, 64, dtype=torch.float16, device=DEV), torch.zeros(24, 64, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="of 16"):
        ops.gemm_f16(a, w)
    out = torch.zeros(4, 4, dtype=torch.float16, device=DEV)
    rc = L.load().vts_vit_attention(out.data_ptr(), 1, 65, 1, 64, out.data_ptr(), L.stream())
    assert rc == L.ERR_UNSUPPORTED and b"T 65" in L.load().vts_last_error()
    rc = L.load().vts_vit_attention(out.data_ptr(), 1, 4, 1, 32, out.data_ptr(), L.stream())
    assert rc == L.ERR_UNSUPPORTED


@pytest.mark.parametrize("m,n,k", [(50, 768, 3072), (200, 512, 768), (37, 384, 128), (200, 3072, 768)])
def test_gemm_random_against_float64(m, n, k):
    """random data: the judge is float64 on the same fp16-rounded operands, so only the fp32 accumulation (and, with QuickGELU, fp32
    expf / division) remains: 2e-5 relative L2, the project's output bound"""
    from vts import ops

    a = (detrand.uniform((m, k), 4, "ga") * math.sqrt(3.0)).half()
    w = (detrand.uniform((n, k), 4, "gw") * math.sqrt(3.0 / k)).half()
    b = (detrand.uniform((n,), 4, "gb") * 0.5).half()
    ref = a.double() @ w.double().t() + b.double()
    ad, wd, bd = a.to(DEV), w.to(DEV), b.to(DEV)
    got = ops.gemm_f16(ad, wd, bias=bd)
    e0 = R.rel_l2(got.cpu(), ref)
    gelu = ops.gemm_f16(ad, wd, bias=bd, epilogue="quickgelu")
    e1 = R.rel_l2(gelu.cpu(), ref * torch.sigmoid(1.702 * ref))
    print("gemm_f16 M %d N %d K %d: rel-L2 %.3e, QuickGELU %.3e" % (m, n, k, e0, e1))
    assert e0 <= 2e-5 and e1 <= 2e-5
    # the fp16 output is the fp32 result rounded to nearest even, and a repeat is bit-identical
    assert torch.equal(ops.gemm_f16(ad, wd, bias=bd, epilogue="quickgelu", out_dtype=torch.float16), gelu.half())
    assert torch.equal(ops.gemm_f16(ad, wd, bias=bd), got)


@pytest.mark.parametrize("rows", [1, 5, 50, 200])
@pytest.mark.parametrize("width", [128, 768])
def test_layernorm_rows(rows, width):
    from vts import ops

    x = detrand.uniform((rows, width), 6, "lnx") * 3.0 + 0.7
    g, b = (1.0 + 0.2 * detrand.uniform((width,), 6, "lng")).half(), (0.3 * detrand.uniform((width,), 6, "lnb")).half()
    ref = torch.nn.functional.layer_norm(x.double(), (width,), g.double(), b.double(), 1e-5)
    y32 = ops.layernorm_rows(x.to(DEV), g.to(DEV), b.to(DEV))
    y16 = ops.layernorm_rows(x.to(DEV), g.to(DEV), b.to(DEV), out_dtype=torch.float16)
    err = R.rel_l2(y32.cpu(), ref)
    print("layernorm_rows %d x %d: rel-L2 %.3e" % (rows, width, err))
    assert err <= 2e-5
    assert y16.dtype == torch.float16 and torch.equal(y16, y32.half())


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attention_against_float64(golden, name):
    """2 heads, batch 3; judged in float64 on the fp16-rounded q, k, v; no less accurate than the all-fp16 evaluation it replaces"""
    from vts import ops

    t = R.ATTN_CASES[name]
    qkv = R.attn_input(t, SEED)
    ref = R.attention(qkv.double(), 3, t, 2)
    got = ops.vit_attention(qkv.to(DEV), 3, t, 2)
    err, bound = R.rel_l2(got.cpu(), ref), float(golden[name + "_err16"])
    print("vit_attention T %d: rel-L2 %.3e (all-fp16 reference arithmetic %.3e)" % (t, err, bound))
    assert got.dtype == torch.float16 and bool(torch.isfinite(got).all())
    assert err <= bound
    assert torch.equal(ops.vit_attention(qkv.to(DEV), 3, t, 2), got)


def _image(n, h, w, seed):
    return detrand.uniform((n, 3, h, w), seed, "img%dx%d" % (h, w))      # [-1, 1): negative values exercise the byte wrap


@pytest.mark.parametrize("h,w,n", [(64, 64, 2), (80, 96, 1), (96, 80, 1), (200, 300, 1), (100, 100, 1), (256, 256, 1)])
def test_preprocess_is_bit_exact(h, w, n):
    """the device chain equals the restated host chain (ToPILImage, Resize(224, BICUBIC), CenterCrop(224), ToTensor, Normalize, .half())
    bit for bit: down- and upscales, both orientations of a non-square image, and a 256 x 256 image with a zeroed background"""
    from vts import ops

    x = _image(n, h, w, 21)
    if (h, w) == (256, 256):
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        x = x * (((yy - 120) ** 2 + (xx - 140) ** 2) < 90 ** 2).float()
    ref = R.preprocess(x)
    got = ops.clip_preprocess(x.to(DEV))
    assert got.dtype == torch.float16 and got.shape == ref.shape
    diff = int((got.cpu().view(torch.int16) != ref.view(torch.int16)).sum())
    print("clip_preprocess %dx%d: %d of %d values differ" % (h, w, diff, ref.numel()))
    assert torch.equal(got.cpu(), ref)


@functools.lru_cache(maxsize=2)
def _tower(cfg_items):
    from models.clip_visual import ClipVisual

    cfg = dict(cfg_items)
    net = ClipVisual(cfg)
    net.load_state_dict(R.test_weights(cfg, SEED))
    return net.to(DEV)


@pytest.mark.parametrize("name", list(R.TOWER_CASES))
def test_whole_tower(golden, name):
    """vts_clip_visual_forward against the float64 judge on the fp16-valued weights and the fp16-rounded input: at least as accurate as
    the half-precision run it replaces (the fixture's all-fp16 error of the same case); finite; bit-identical when repeated; and a
    captured graph of the C entry replays to the same bits"""
    from vts import lib as L
    from vts import ops

    cfg, batch = R.TOWER_CASES[name]
    net = _tower(tuple(sorted(cfg.items())))
    x = R.test_input(cfg, batch, SEED).to(DEV)
    got = net(x)
    ref, bound = torch.from_numpy(golden[name + "_out64"]), float(golden[name + "_err16"])
    err = R.rel_l2(got.cpu(), ref)
    print("clip_visual_forward %s: rel-L2 %.3e (all-fp16 reference arithmetic %.3e)" % (name, err, bound))
    assert got.dtype == torch.float32 and got.shape == ref.shape and bool(torch.isfinite(got).all())
    assert err <= bound
    assert torch.equal(net(x), got)
    # the C entry inside a captured graph, on buffers of its own
    ccfg, flat = net._ccfg, net.flat_weights()
    nws = L.load().vts_clip_visual_forward_ws_floats(ctypes.byref(ccfg), batch)
    ws, out = torch.empty(nws, dtype=torch.float32, device=DEV), torch.zeros_like(got)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(), capture_error_mode="thread_local"):
        ops.clip_visual_forward(ccfg, flat, x, out=out, ws=ws)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, got)


def test_tower_refuses_other_architectures():
    from vts import lib as L

    bad = L.ClipVisualCfg(768, 12, 12, 16, 224, 512)      # ViT-B/16: 197 tokens
    assert L.load().vts_clip_visual_forward_ws_floats(ctypes.byref(bad), 1) == -1 and b"out of scope" in L.load().vts_last_error()
    bad = L.ClipVisualCfg(768, 12, 8, 32, 224, 512)       # head dimension 96
    assert L.load().vts_clip_visual_forward_ws_floats(ctypes.byref(bad), 1) == -1


MODEL_FLAGS = ("--model skitG --gpu_ids 0 --lambda_G1_lpips 0 --lambda_G2_lpips 0 --use_vision_aided_loss False --lambda_G2_GAN_feat 0 "
               "--use_style_code True --checkpoints_dir /tmp/vts_test_ckpt --name clip --crop_size 256 --batch_size 1")


def _model():
    from models import create_model
    from options.train_options import TrainOptions

    opt = TrainOptions(cmd_line=MODEL_FLAGS).parse()
    model = create_model(opt)
    model.setup(opt)
    model.parallelize()
    model.eval()
    return model, opt


def test_model_computes_the_style_code(monkeypatch, capsys):
    """SKITGModel with --use_style_code True and a batch WITHOUT style_code: set_input derives the code on the device (the parent of this
    change raised RuntimeError in test()); the code equals pre-process + tower by hand on the masked real_I, the generator output equals
    bit for bit the run with that code supplied in the batch, style_I / style_M take precedence over real_I, and a batch that carries a
    style_code never constructs the encoder"""
    from data.synthetic_dataset import make_sample
    from vts import ops

    monkeypatch.delenv("VTS_CLIP_WEIGHTS", raising=False)
    batch = default_collate([make_sample(256, 8, 8, 31)])
    assert "style_code" not in batch
    model, opt = _model()
    assert model.net_style is None
    model.set_input(batch, phase="test")
    model.test()
    fake_I, fake_T = model.fake_I.clone(), model.fake_T.clone()
    code = model.style_code.clone()
    assert code.shape == (1, 512) and code.dtype == torch.float32 and bool(torch.isfinite(code).all()) and float(code.abs().max()) > 0
    assert model.style_code_pretrained is False and model.net_style.pretrained is False
    assert "STAND-IN" in capsys.readouterr().out
    # by hand: CLIP's pre-processing of the masked image, then the tower's C entry
    masked = batch["I"].to(DEV) * batch["M"].to(DEV)
    assert torch.equal(model.real_I, masked)
    pre = ops.clip_preprocess(masked.contiguous())
    assert torch.equal(pre.cpu(), R.preprocess(masked.cpu()))
    hand = ops.clip_visual_forward(model.net_style._ccfg, model.net_style.flat_weights(), pre)
    assert torch.equal(hand, code)
    # the same code supplied in the batch: the encoder is never constructed, the generator output is the same to the bit
    model2, _ = _model()
    model2.netG.load_state_dict(model.netG.state_dict())
    model2.set_input(dict(batch, style_code=code.cpu()), phase="test")
    model2.test()
    assert model2.net_style is None and model2.style_code_pretrained is None
    assert torch.equal(model2.fake_I, fake_I) and torch.equal(model2.fake_T, fake_T)
    # style_I / style_M in the batch: the code is taken from those
    other = default_collate([make_sample(256, 8, 8, 32)])
    model.set_input(dict(batch, style_I=other["I"], style_M=other["M"]), phase="test")
    hand2 = model.net_style.encode((other["I"].to(DEV) * other["M"].to(DEV)).contiguous())
    assert torch.equal(model.style_code, hand2) and not torch.equal(hand2, code)
    model.test()
    assert not torch.equal(model.fake_I, fake_I)
    # and back: the first batch again gives the first output again (through the captured inference graph, if one was made)
    model.set_input(batch, phase="test")
    model.test()
    assert torch.equal(model.style_code, code) and torch.equal(model.fake_I, fake_I)
