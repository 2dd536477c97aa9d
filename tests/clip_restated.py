"""Restatements the CLIP style-encoder tests judge against (TEST INFRASTRUCTURE; imported by test_clip_cpu.py / test_clip_gpu.py and
tools/make_clip_golden.py).

PARITY UNPINNED: neither `clip` nor `torchvision` is installed where this suite runs, so both are restated from their published sources
(openai/CLIP clip/model.py: VisionTransformer, ResidualAttentionBlock, QuickGELU, LayerNorm; clip/clip.py:_transform;
torchvision.transforms.functional: to_pil_image, resize, center_crop, to_tensor, normalize; Pillow src/libImaging/Resample.c), as
oracle/nets.py:ssim is.  What IS pinned: the resize against the installed Pillow bit for bit, the byte conversion against torch, and the
tower against an independent build from torch.nn.MultiheadAttention / nn.LayerNorm / nn.Conv2d (tests/test_clip_cpu.py).
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import detrand  # noqa: E402

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)

# the tower cases of tests/test_clip_gpu.py and the fixture: name -> (config, batch)
VIT_B32 = dict(width=768, layers=12, heads=12, patch=32, resolution=224, output_dim=512)
SMALL64 = dict(width=128, layers=2, heads=2, patch=32, resolution=64, output_dim=32)
SMALL224 = dict(width=128, layers=2, heads=2, patch=32, resolution=224, output_dim=32)
TOWER_CASES = {"small64_b3": (SMALL64, 3), "small224_b2": (SMALL224, 2), "vitb32_b1": (VIT_B32, 1), "vitb32_b4": (VIT_B32, 4)}
ATTN_CASES = {"attn_t5": 5, "attn_t50": 50, "attn_t64": 64}      # 2 heads, batch 3, head dimension 64
GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_visual.npz")


# ---- the tower --------------------------------------------------------------------------------------------------------------------------
def param_shapes(cfg):
    w, t = cfg["width"], (cfg["resolution"] // cfg["patch"]) ** 2 + 1
    s = {"conv1.weight": (w, 3, cfg["patch"], cfg["patch"]), "class_embedding": (w,), "positional_embedding": (t, w),
         "ln_pre.weight": (w,), "ln_pre.bias": (w,)}
    for i in range(cfg["layers"]):
        p = "transformer.resblocks.%d." % i
        s.update({p + "ln_1.weight": (w,), p + "ln_1.bias": (w,), p + "attn.in_proj_weight": (3 * w, w), p + "attn.in_proj_bias": (3 * w,),
                  p + "attn.out_proj.weight": (w, w), p + "attn.out_proj.bias": (w,), p + "ln_2.weight": (w,), p + "ln_2.bias": (w,),
                  p + "mlp.c_fc.weight": (4 * w, w), p + "mlp.c_fc.bias": (4 * w,), p + "mlp.c_proj.weight": (w, 4 * w), p + "mlp.c_proj.bias": (w,)})
    s.update({"ln_post.weight": (w,), "ln_post.bias": (w,), "proj": (w, cfg["output_dim"])})
    return s


def test_weights(cfg, seed):
    """fp32 weights from the project's deterministic generator at CLIP's published scales (clip/model.py:initialize_parameters), which
    keep activations O(1): embeddings and projections width^-0.5, block projections additionally (2 layers)^-0.5, c_fc (2 width)^-0.5,
    LayerNorm gains near 1.  (detrand.uniform has standard deviation 3^-0.5, hence the sqrt(3).)"""
    w, nl = cfg["width"], max(cfg["layers"], 1)
    sd = {}
    for k, shp in param_shapes(cfg).items():
        u = detrand.uniform(shp, seed, k)
        if k == "conv1.weight":
            std = (3 * cfg["patch"] ** 2) ** -0.5
        elif k in ("class_embedding", "positional_embedding", "proj") or k.endswith("in_proj_weight"):
            std = w ** -0.5
        elif k.endswith(("out_proj.weight", "c_proj.weight")):
            std = w ** -0.5 * (2 * nl) ** -0.5
        elif k.endswith("c_fc.weight"):
            std = (2 * w) ** -0.5
        elif ".ln_" in k or k.startswith("ln_"):
            sd[k] = (1.0 + 0.1 * u) if k.endswith("weight") else 0.1 * u
            continue
        else:
            sd[k] = 0.05 * u      # linear biases
            continue
        sd[k] = u * (math.sqrt(3.0) * std)
    return sd


def test_input(cfg, batch, seed):
    """a pre-processed image batch, fp16-valued: CLIP-normalised pixels span about [-1.8, 2.1]"""
    return (detrand.uniform((batch, 3, cfg["resolution"], cfg["resolution"]), seed, "clip_input") * 1.9).half()


def _ln(x, w, b):
    # CLIP's LayerNorm subclass: evaluate in fp32 when the stream is fp16, cast back
    if x.dtype == torch.float16:
        return F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), 1e-5).half()
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def attention(qkv, batch, tokens, heads):
    """nn.MultiheadAttention's core on the packed projection [batch * tokens, 3 * width]: q scaled by hd^-0.5, unmasked softmax, @ v"""
    w = qkv.shape[1] // 3
    hd = w // heads
    q, k, v = (t.reshape(batch, tokens, heads, hd).transpose(1, 2) for t in qkv.split(w, dim=1))
    a = torch.softmax((q * hd ** -0.5) @ k.transpose(-1, -2), dim=-1) @ v
    return a.transpose(1, 2).reshape(batch * tokens, w)


def tower(sd, cfg, x):
    """VisionTransformer.forward in the dtype of x (sd in the same dtype): float64 is the judge, float16 the reference's own arithmetic
    (clip.load holds the tower in fp16 on a GPU and the reference feeds it image.half())"""
    w, p, heads = cfg["width"], cfg["patch"], cfg["heads"]
    n, g = x.shape[0], cfg["resolution"] // cfg["patch"]
    t = g * g + 1
    rows = x.reshape(n, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * p * p)      # conv1: kernel = stride = patch, no bias
    tok = (rows @ sd["conv1.weight"].reshape(w, -1).t()).reshape(n, g * g, w)
    x = torch.cat([sd["class_embedding"].expand(n, 1, w), tok], dim=1) + sd["positional_embedding"]
    x = _ln(x, sd["ln_pre.weight"], sd["ln_pre.bias"]).reshape(n * t, w)
    for i in range(cfg["layers"]):
        k = "transformer.resblocks.%d." % i
        h = _ln(x, sd[k + "ln_1.weight"], sd[k + "ln_1.bias"])
        a = attention(h @ sd[k + "attn.in_proj_weight"].t() + sd[k + "attn.in_proj_bias"], n, t, heads)
        x = x + (a @ sd[k + "attn.out_proj.weight"].t() + sd[k + "attn.out_proj.bias"])
        h = _ln(x, sd[k + "ln_2.weight"], sd[k + "ln_2.bias"])
        h = h @ sd[k + "mlp.c_fc.weight"].t() + sd[k + "mlp.c_fc.bias"]
        h = h * torch.sigmoid(1.702 * h)                                                            # QuickGELU
        x = x + (h @ sd[k + "mlp.c_proj.weight"].t() + sd[k + "mlp.c_proj.bias"])
    cls = _ln(x.reshape(n, t, w)[:, 0, :], sd["ln_post.weight"], sd["ln_post.bias"])
    return cls @ sd["proj"]


def rel_l2(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float((got - ref).norm() / ref.norm())


def judge_pair(sd32, cfg, x16):
    """(float64 output on the fp16-valued weights and input, relative L2 error of the all-fp16 run against it)"""
    sd16 = {k: v.half() for k, v in sd32.items()}
    out64 = tower({k: v.double() for k, v in sd16.items()}, cfg, x16.double())
    out16 = tower(sd16, cfg, x16)
    return out64, rel_l2(out16, out64)


def attn_input(tokens, seed):
    return (detrand.uniform((3 * tokens, 3 * 128), seed, "attn_qkv_%d" % tokens) * math.sqrt(3.0)).half()


# ---- the pre-processing chain -------------------------------------------------------------------------------------------------------------
def to_bytes(x):
    """ToPILImage on a float tensor is pic.mul(255).byte(): truncation toward zero, then mod 256 (negative values wrap)"""
    v = np.trunc(np.asarray(x, dtype=np.float32) * np.float32(255.0)).astype(np.int64)
    return (v % 256).astype(np.uint8)


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _coeffs(in_size, out_size):
    """Resample.c:precompute_coeffs + normalize_coeffs_8bpc (PRECISION_BITS = 32 - 8 - 2 = 22)"""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * (1.0 / fscale)) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        out.append((xmin, np.array([int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in k], dtype=np.int64)))
    return out


def _pass(img, out_size, axis):
    img = np.moveaxis(img, axis, -1).astype(np.int64)
    out = np.empty(img.shape[:-1] + (out_size,), dtype=np.uint8)
    for xx, (xmin, k) in enumerate(_coeffs(img.shape[-1], out_size)):
        ss = (1 << 21) + (img[..., xmin:xmin + len(k)] * k).sum(-1)
        out[..., xx] = np.clip(ss >> 22, 0, 255)
    return np.moveaxis(out, -1, axis)


def resize_bicubic(img, out_w, out_h):
    """PIL.Image.resize((out_w, out_h), BICUBIC) of a uint8 [H, W, C] array: the horizontal pass to uint8, then the vertical pass"""
    return _pass(_pass(img, out_w, 1), out_h, 0)


def resized_size(h, w):
    """torchvision Resize(224) on a PIL image: the shorter side to 224, the longer to int(224 * long / short) -> (h, w)"""
    return (int(224 * h / w), 224) if w <= h else (224, int(224 * w / h))


def preprocess(x):
    """clip.clip._transform(224) applied to each image of the fp32 [N, 3, H, W] tensor x as the reference does (skitG_model.py:715-724),
    then .half() (:1296) -> fp16 [N, 3, 224, 224]"""
    outs = []
    mean, std = torch.tensor(CLIP_MEAN, dtype=torch.float32), torch.tensor(CLIP_STD, dtype=torch.float32)
    for img in x:
        b = to_bytes(img.permute(1, 2, 0).contiguous().numpy())
        oh, ow = resized_size(b.shape[0], b.shape[1])
        b = resize_bicubic(b, ow, oh)
        top, left = int(round((oh - 224) / 2.0)), int(round((ow - 224) / 2.0))
        b = b[top:top + 224, left:left + 224]
        t = torch.from_numpy(np.ascontiguousarray(b)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)      # ToTensor
        outs.append(t.sub_(mean[:, None, None]).div_(std[:, None, None]))                                              # Normalize
    return torch.stack(outs).half()
