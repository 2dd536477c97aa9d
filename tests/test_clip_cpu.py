"""The CLIP style encoder's judges, pinned on the CPU (no GPU, no library call): tests/clip_restated.py restates CLIP's image tower and
its pre-processing chain from the published sources (`clip` and `torchvision` are not installed: PARITY UNPINNED for those two); here
the restatement is held against what IS installed -- Pillow's own bicubic resize bit for bit, torch's mul(255).byte(), and an independent
build of the tower from torch.nn.MultiheadAttention / nn.LayerNorm / nn.Conv2d -- and the checkpoint handling of models/clip_visual.py
and the fixture of tools/make_clip_golden.py are checked."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import clip_restated as R
from oracle import detrand

RESIZE_CASES = [((64, 64), (32, 32)), ((96, 80), (50, 41)), ((1536, 1536), (224, 224)), ((300, 200), (336, 224)), ((100, 100), (224, 224)),
                ((37, 53), (24, 35))]      # (in_w, in_h) -> (out_w, out_h), the last but one an upscale


@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_resize_restatement_equals_pillow(src, dst):
    from PIL import Image

    img = ((detrand.uniform((src[1], src[0], 3), 5, "resize") * 0.5 + 0.5) * 255.999).to(torch.uint8).numpy()
    ref = np.asarray(Image.fromarray(img, "RGB").resize(dst, Image.BICUBIC))
    got = R.resize_bicubic(img, dst[0], dst[1])
    assert got.shape == ref.shape and np.array_equal(got, ref), int(np.abs(got.astype(int) - ref.astype(int)).max())


def test_byte_conversion_equals_torch():
    grid = torch.cat([torch.linspace(-1, 1, 20001), torch.tensor([-1.0, -0.5, -0.004, 0.0, 0.004, 0.5, 1.0]), torch.arange(-255, 256) / 255.0])
    ref = grid.mul(255).byte().numpy()
    assert np.array_equal(R.to_bytes(grid.numpy()), ref)
    spot = dict(zip([-1.0, -0.5, -0.004, 1.0], R.to_bytes(np.array([-1.0, -0.5, -0.004, 1.0], dtype=np.float32)).tolist()))
    assert spot == {-1.0: 1, -0.5: 129, -0.004: 255, 1.0: 255}      # negative values wrap: the reference's behaviour on its [-1, 1] images


def test_resized_size_and_crop_window():
    assert R.resized_size(200, 300) == (224, 336) and R.resized_size(96, 80) == (268, 224) and R.resized_size(1536, 1536) == (224, 224)
    x = detrand.uniform((1, 3, 96, 80), 3, "pre")
    out = R.preprocess(x)
    assert out.shape == (1, 3, 224, 224) and out.dtype == torch.float16 and bool(torch.isfinite(out).all())


class _IndependentBlock(nn.Module):
    def __init__(self, w, heads):
        super().__init__()
        self.attn = nn.MultiheadAttention(w, heads)
        self.ln_1, self.ln_2 = nn.LayerNorm(w), nn.LayerNorm(w)
        self.mlp = nn.Sequential()
        self.mlp.add_module("c_fc", nn.Linear(w, 4 * w))
        self.mlp.add_module("c_proj", nn.Linear(4 * w, w))

    def forward(self, x):
        h = self.ln_1(x)
        x = x + self.attn(h, h, h, need_weights=False)[0]
        h = self.mlp.c_fc(self.ln_2(x))
        return x + self.mlp.c_proj(h * torch.sigmoid(1.702 * h))


class _IndependentTower(nn.Module):
    """CLIP's VisionTransformer, built from the torch modules it is made of (sequence-first, as CLIP runs it)"""

    def __init__(self, cfg):
        super().__init__()
        w, t = cfg["width"], (cfg["resolution"] // cfg["patch"]) ** 2 + 1
        self.conv1 = nn.Conv2d(3, w, cfg["patch"], cfg["patch"], bias=False)
        self.class_embedding, self.positional_embedding = nn.Parameter(torch.zeros(w)), nn.Parameter(torch.zeros(t, w))
        self.ln_pre, self.ln_post = nn.LayerNorm(w), nn.LayerNorm(w)
        self.transformer = nn.Module()
        self.transformer.resblocks = nn.Sequential(*[_IndependentBlock(w, cfg["heads"]) for _ in range(cfg["layers"])])
        self.proj = nn.Parameter(torch.zeros(w, cfg["output_dim"]))

    def forward(self, x):
        x = self.conv1(x)
        x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
        x = torch.cat([self.class_embedding + torch.zeros(x.shape[0], 1, x.shape[-1], dtype=x.dtype), x], dim=1) + self.positional_embedding
        x = self.ln_pre(x).permute(1, 0, 2)
        x = self.transformer.resblocks(x).permute(1, 0, 2)
        return self.ln_post(x[:, 0, :]) @ self.proj


@pytest.mark.parametrize("cfg,batch", [(R.SMALL64, 3), (R.SMALL224, 2), (dict(R.SMALL224, width=192, heads=3, layers=3, output_dim=48), 1)])
def test_tower_restatement_equals_independent_build(cfg, batch):
    sd = {k: v.double() for k, v in R.test_weights(cfg, 11).items()}
    net = _IndependentTower(cfg).double()
    net.load_state_dict(sd)      # strict: the restatement's parameter names ARE CLIP's
    x = R.test_input(cfg, batch, 11).double()
    with torch.no_grad():
        ref = net(x)
    got = R.tower(sd, cfg, x)
    assert got.shape == (batch, cfg["output_dim"]) and float(ref.abs().max()) > 0.1
    assert float((got - ref).abs().max()) <= 1e-10, float((got - ref).abs().max())


def test_standin_keeps_activations_order_one():
    from models.clip_visual import standin_state

    cfg = R.SMALL224
    out = R.tower({k: v.double() for k, v in standin_state(cfg).items()}, cfg, R.test_input(cfg, 2, 3).double())
    assert 0.05 < float(out.std()) < 20.0, float(out.std())


def test_checkpoint_round_trip_prefix_and_shape_refusal(tmp_path):
    from models.clip_visual import ClipVisual

    cfg = R.SMALL64
    a, b = ClipVisual(cfg, seed=1), ClipVisual(cfg, seed=2)
    assert sorted(a.state_dict()) == sorted(R.param_shapes(cfg)) and a.pretrained is False
    assert not torch.equal(a.proj, b.proj)
    # a plain state dict, through a file
    path = os.path.join(str(tmp_path), "sd.pt")
    torch.save(a.state_dict(), path)
    b.load_weights(path)
    assert b.pretrained is True and all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    # a whole-model dict: `visual.` prefix, fp16 values, text-tower keys and scalars alongside
    full = {"visual." + k: v.half() for k, v in a.state_dict().items()}
    full.update({"token_embedding.weight": torch.zeros(7, 5), "transformer.resblocks.0.ln_1.weight": torch.zeros(3), "logit_scale": torch.tensor(1.0),
                 "input_resolution": torch.tensor(64)})
    c = ClipVisual(cfg, seed=3)
    c.load_clip_state(full)
    assert c.pretrained is True and torch.equal(c.proj, a.proj.half().float()) and c.proj.dtype == torch.float32
    # a TorchScript archive (clip ships ViT-B-32.pt as one)
    jpath = os.path.join(str(tmp_path), "jit.pt")
    torch.jit.script(_Holder({k.replace(".", "_"): v for k, v in a.state_dict().items()})).save(jpath)
    with pytest.raises(KeyError, match="lack"):      # opened as an archive; its (renamed) keys are not the tower's
        ClipVisual(cfg, seed=4).load_weights(jpath)
    # a wrong shape is refused, naming the key
    bad = dict(full)
    bad["visual.proj"] = torch.zeros(cfg["width"], cfg["output_dim"] + 16)
    with pytest.raises(ValueError, match="visual.proj"):
        ClipVisual(cfg, seed=5).load_clip_state(bad)
    # flat_weights: the documented order and size
    n = cfg["width"]
    t = (cfg["resolution"] // cfg["patch"]) ** 2 + 1
    flat = a.flat_weights()
    assert flat.dtype == torch.float16 and flat.numel() == sum(int(np.prod(s)) for s in R.param_shapes(cfg).values())
    assert torch.equal(flat[:n * 3 * 32 * 32], a.conv1.weight.reshape(-1).half()) and torch.equal(flat[-n * cfg["output_dim"]:], a.proj.t().reshape(-1).half())
    assert torch.equal(flat[n * 3 * 32 * 32 + n:n * 3 * 32 * 32 + n + t * n], a.positional_embedding.reshape(-1).half())


class _Holder(nn.Module):
    def __init__(self, tensors):
        super().__init__()
        for k, v in tensors.items():
            self.register_buffer(k, v.clone())

    def forward(self):
        return self.proj


def test_fixture_holds_the_small_cases():
    """the fixture's float64 outputs are what the restatement gives on the regenerated weights (the small cases: cheap), and every case
    carries the error of the reference's own fp16 arithmetic, at the level half precision gives"""
    z = np.load(R.GOLDEN)
    for name in ("small64_b3", "small224_b2"):
        cfg, batch = R.TOWER_CASES[name]
        o64, e16 = R.judge_pair(R.test_weights(cfg, 77), cfg, R.test_input(cfg, batch, 77))
        assert np.abs(o64.numpy() - z[name + "_out64"]).max() <= 1e-10
    for name in list(R.TOWER_CASES) + list(R.ATTN_CASES):
        assert 1e-5 < float(z[name + "_err16"]) < 1e-2, (name, float(z[name + "_err16"]))
    for name, (cfg, batch) in R.TOWER_CASES.items():
        assert z[name + "_out64"].shape == (batch, cfg["output_dim"]) and z[name + "_out64"].dtype == np.float64
    assert os.path.getsize(R.GOLDEN) < 64 * 1024


@pytest.mark.parametrize("h,w", [(64, 64), (80, 96), (96, 80), (200, 300), (100, 100), (53, 37), (1536, 1536)])
def test_product_tables_reproduce_the_restatement(h, w):
    """the host's share of vts_clip_preprocess (vts/ops.py:clip_preprocess_tables: taps restricted to the crop window, the 3 x 256
    normalisation table), applied with the integer arithmetic the kernels use, gives the restated chain's result bit for bit"""
    from vts import ops

    x = detrand.uniform((1, 3, h, w), 8, "tab")
    hb, hk, vb, vk, lut = (t.numpy() for t in ops.clip_preprocess_tables(h, w, "cpu"))
    assert hb.shape == vb.shape == (224, 2) and lut.shape == (3, 256) and lut.dtype == np.float16
    assert (hb[:, 0] >= 0).all() and (hb[:, 0] + hb[:, 1] <= w).all() and (vb[:, 0] >= 0).all() and (vb[:, 0] + vb[:, 1] <= h).all()
    assert (hb[:, 1] <= hk.shape[1]).all() and (vb[:, 1] <= vk.shape[1]).all()
    b = R.to_bytes(x[0].numpy()).astype(np.int64)                                  # [3, h, w]
    tmp = np.empty((3, h, 224), dtype=np.int64)
    for j in range(224):
        x0, cnt = hb[j]
        tmp[:, :, j] = np.clip(((1 << 21) + (b[:, :, x0:x0 + cnt] * hk[j, :cnt].astype(np.int64)).sum(-1)) >> 22, 0, 255)
    out = np.empty((3, 224, 224), dtype=np.float16)
    for i in range(224):
        y0, cnt = vb[i]
        v = np.clip(((1 << 21) + (tmp[:, y0:y0 + cnt, :] * vk[i, :cnt].astype(np.int64)[None, :, None]).sum(1)) >> 22, 0, 255)
        for c in range(3):
            out[c, i] = lut[c][v[c]]
    ref = R.preprocess(x)[0].numpy()
    assert np.array_equal(out.view(np.int16), ref.view(np.int16))
