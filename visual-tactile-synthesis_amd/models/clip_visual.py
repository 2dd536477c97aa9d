"""ClipVisual: CLIP's image tower (ViT-B/32 by default), frozen -- skitG's style encoder, and a differentiable feature extractor.

The reference derives the style code on every forward with `clip.load("ViT-B/32")`'s `.visual` in half precision (reference
models/skitG_model.py:484-489, 1294-1296).  This module carries the same parameters under the names of CLIP's `VisionTransformer`
(`conv1.weight`, `class_embedding`, `positional_embedding`, `proj`, `ln_pre.*`, `ln_post.*`, `transformer.resblocks.{i}.{ln_1, ln_2,
attn.in_proj_weight, attn.in_proj_bias, attn.out_proj, mlp.c_fc, mlp.c_proj}.*`), so a real checkpoint loads, and computes through ONE C
entry, vts_clip_visual_forward (include/vts.h: f16 MFMA products with fp32 accumulation, fp32 residual stream / LayerNorm / softmax), on
a flat fp16 copy of the weights, as `clip.load` holds them on a GPU.

The published weights cannot exist offline: `--clip_weights <file>` (or $VTS_CLIP_WEIGHTS) loads them; without a file the tower runs on
a seeded stand-in (CLIP's own initialisation scales) and `pretrained` stays False -- style codes then compare builds on the same seed only,
the precedent of `loss_lpips_pretrained` in models/perceptual.py.

The tower is frozen, but an image can be differentiated THROUGH it: `features` returns the embedding and any blocks' hidden states of an
image of any size (area pooling + CLIP's normalisation, ops.clip_area_preprocess: CLIP's own transform goes through 8-bit Pillow and has
no gradient), and `features_backward` takes cotangents of those back to the image (vts_clip_visual_forward_tape /
vts_clip_visual_backward: input gradient only, no parameter gradients).  That is the half of the reference's vision-aided discriminator
D3 that can be built here.

Out of scope (the library reports them): D3's multi-level heads -- small convolutions on the tapped hidden states, defined by a
third-party package whose source is not available, so they cannot be pinned and the models still refuse `--use_vision_aided_loss True`
at the warm-up epoch --, the text tower, and the other CLIP architectures (only head dimension 64 and at most 64 tokens are built).
"""
import os

import torch
import torch.nn as nn

from vts import ops

VIT_B32 = dict(width=768, layers=12, heads=12, patch=32, resolution=224, output_dim=512)
SEED = 20210105


class _Affine(nn.Module):
    """parameter holder of an nn.LayerNorm / nn.Linear (weight, bias)"""

    def __init__(self, *weight_shape):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(*weight_shape), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(weight_shape[0]), requires_grad=False)


class _Attn(nn.Module):
    """parameter holder of nn.MultiheadAttention"""

    def __init__(self, w):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.zeros(3 * w, w), requires_grad=False)
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * w), requires_grad=False)
        self.out_proj = _Affine(w, w)


class _Mlp(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.c_fc = _Affine(4 * w, w)
        self.c_proj = _Affine(w, 4 * w)


class _Block(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.ln_1, self.attn, self.ln_2, self.mlp = _Affine(w), _Attn(w), _Affine(w), _Mlp(w)


class _Transformer(nn.Module):
    def __init__(self, w, layers):
        super().__init__()
        self.resblocks = nn.ModuleList([_Block(w) for _ in range(layers)])


class _Conv(nn.Module):
    def __init__(self, w, patch):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(w, 3, patch, patch), requires_grad=False)


def standin_state(cfg, seed=SEED):
    """seeded stand-in weights at CLIP's published initialisation scales (clip/model.py:initialize_parameters), which keep activations
    O(1): embeddings and projections width^-0.5, block projections additionally (2 layers)^-0.5, c_fc (2 width)^-0.5, LayerNorm gains
    near 1, linear biases zero"""
    g = torch.Generator().manual_seed(seed)
    w, nl, t = cfg["width"], max(cfg["layers"], 1), (cfg["resolution"] // cfg["patch"]) ** 2 + 1
    rn = lambda std, *shape: torch.randn(*shape, generator=g) * std      # noqa: E731
    sd = {"conv1.weight": rn((3 * cfg["patch"] ** 2) ** -0.5, w, 3, cfg["patch"], cfg["patch"]), "class_embedding": rn(w ** -0.5, w),
          "positional_embedding": rn(w ** -0.5, t, w), "proj": rn(w ** -0.5, w, cfg["output_dim"])}
    for name in ["ln_pre", "ln_post"] + ["transformer.resblocks.%d.ln_%d" % (i, j) for i in range(cfg["layers"]) for j in (1, 2)]:
        sd[name + ".weight"], sd[name + ".bias"] = 1.0 + rn(0.02, w), rn(0.02, w)
    for i in range(cfg["layers"]):
        p = "transformer.resblocks.%d." % i
        sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = rn(w ** -0.5, 3 * w, w), torch.zeros(3 * w)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = rn(w ** -0.5 * (2 * nl) ** -0.5, w, w), torch.zeros(w)
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = rn((2 * w) ** -0.5, 4 * w, w), torch.zeros(4 * w)
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = rn(w ** -0.5 * (2 * nl) ** -0.5, w, 4 * w), torch.zeros(w)
    return sd


class ClipVisual(nn.Module):
    def __init__(self, cfg=None, seed=SEED):
        super().__init__()
        self.cfg = dict(VIT_B32 if cfg is None else cfg)
        w, t = self.cfg["width"], (self.cfg["resolution"] // self.cfg["patch"]) ** 2 + 1
        self.conv1 = _Conv(w, self.cfg["patch"])
        self.class_embedding = nn.Parameter(torch.zeros(w), requires_grad=False)
        self.positional_embedding = nn.Parameter(torch.zeros(t, w), requires_grad=False)
        self.ln_pre = _Affine(w)
        self.transformer = _Transformer(w, self.cfg["layers"])
        self.ln_post = _Affine(w)
        self.proj = nn.Parameter(torch.zeros(w, self.cfg["output_dim"]), requires_grad=False)
        self.pretrained = False
        self._flat, self._ws = None, {}
        self._flat_t, self._bwd = None, {}
        self.load_state_dict(standin_state(self.cfg, seed))
        self.eval()

    def load_state_dict(self, sd, strict=True, **kw):
        out = super().load_state_dict(sd, strict=strict, **kw)
        self._flat, self._flat_t, self._bwd = None, None, {}
        return out

    def _apply(self, fn, *a, **kw):
        self._flat, self._ws = None, {}
        self._flat_t, self._bwd = None, {}
        return super()._apply(fn, *a, **kw)

    def load_weights(self, path):
        """a plain state dict or a TorchScript archive (clip's ViT-B-32.pt is one: opened with torch.jit.load(...).state_dict()); keys may
        carry a `visual.` prefix, the text tower's keys are ignored; a wrong shape is refused with the key's name"""
        try:
            sd = torch.load(path, map_location="cpu", weights_only=True)      # (state dicts only: no pickled code from a user path)
        except Exception as e_plain:
            try:
                sd = torch.jit.load(path, map_location="cpu").state_dict()
            except Exception:
                raise RuntimeError("clip weights %s: neither a state dict nor a TorchScript archive (%s)" % (path, e_plain))
        self.load_clip_state(sd.get("state_dict", sd), source=path)
        return self

    def load_clip_state(self, sd, source="state dict"):
        own = self.state_dict()
        prefixed = any(k.startswith("visual.") for k in sd)
        picked = {}
        for k, v in sd.items():
            name = k[len("visual."):] if k.startswith("visual.") else (None if prefixed else k)
            if name in own:
                if tuple(v.shape) != tuple(own[name].shape):
                    raise ValueError("clip weights %s: %s has shape %s, this tower (%s) needs %s"
                                     % (source, k, tuple(v.shape), self.cfg, tuple(own[name].shape)))
                picked[name] = v.detach().to(torch.float32)
        missing = [k for k in own if k not in picked]
        if missing:
            raise KeyError("clip weights %s lack %s" % (source, missing[:4]))
        self.load_state_dict(picked)
        self.pretrained = True

    def flat_weights(self):
        """the flat fp16 weight buffer of vts_clip_visual_forward, in the order include/vts.h documents (proj transposed); built once"""
        if self._flat is None:
            sd = self.state_dict()
            parts = [sd["conv1.weight"], sd["class_embedding"], sd["positional_embedding"], sd["ln_pre.weight"], sd["ln_pre.bias"]]
            for i in range(self.cfg["layers"]):
                p = "transformer.resblocks.%d." % i
                parts += [sd[p + k] for k in ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                                              "attn.out_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias",
                                              "mlp.c_proj.weight", "mlp.c_proj.bias")]
            parts += [sd["ln_post.weight"], sd["ln_post.bias"], sd["proj"].t()]
            self._flat = torch.cat([p.reshape(-1).to(torch.float16) for p in parts]).contiguous()
            self._ccfg = ops.clip_visual_cfg(**self.cfg)
        return self._flat

    def flat_weights_t(self):
        """the second flat fp16 buffer, every matrix transposed (include/vts.h: vts_clip_visual_backward), so that the forward's GEMM
        kernel forms the input gradients; built on the first backward only"""
        if self._flat_t is None:
            sd, w = self.state_dict(), self.cfg["width"]
            parts = [sd["conv1.weight"].reshape(w, -1).t()]
            for i in range(self.cfg["layers"]):
                p = "transformer.resblocks.%d." % i
                parts += [sd[p + k].t() for k in ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")]
            od = self.cfg["output_dim"]
            parts.append(torch.nn.functional.pad(sd["proj"], (0, -od % 32)))
            self._flat_t = torch.cat([p.reshape(-1).to(torch.float16) for p in parts]).contiguous()
        return self._flat_t

    def _backward_buffers(self, n, device):
        """(tape, forward scratch, backward scratch) of batch size n: the tower's own, allocated on first use"""
        b = self._bwd.get(n)
        if b is None:
            self.flat_weights()
            b = self._bwd[n] = tuple(torch.empty(k, dtype=torch.float32, device=device) for k in (
                ops.clip_visual_tape_floats(self._ccfg, n), ops.clip_visual_forward_ws_floats(self._ccfg, n),
                ops.clip_visual_backward_ws_floats(self._ccfg, n)))
        return b

    def forward_taped(self, x16, taps=()):
        """x16: fp16 [N, 3, res, res] -> (embedding fp32 [N, output_dim], [hidden state after block l, fp32 [N, T, W], for l in taps],
        ctx).  The hidden states are views into the tape of this batch size: the next taped forward of that size overwrites them."""
        if not x16.is_cuda:
            raise RuntimeError("ClipVisual: HIP path only (the tower runs through vts_clip_visual_forward_tape); input is on %s" % x16.device)
        taps = tuple(int(t) for t in taps)
        if any(t < 1 or t > self.cfg["layers"] for t in taps) or list(taps) != sorted(set(taps)):
            raise ValueError("ClipVisual: taps %s must be ascending block numbers in 1 .. %d" % (taps, self.cfg["layers"]))
        flat, n = self.flat_weights(), x16.shape[0]
        tape, ws, _ = self._backward_buffers(n, x16.device)
        emb = ops.clip_visual_forward_tape(self._ccfg, flat, x16, tape, ws=ws)
        return emb, [ops.clip_visual_hidden(self._ccfg, tape, n, t) for t in taps], {"n": n, "taps": taps}

    def input_gradient(self, ctx, d_embedding=None, d_hidden=()):
        """cotangents of forward_taped's results (d_hidden: one per tap, in order; either may be absent, not both) -> the gradient with
        respect to x16, fp32 [N, 3, res, res]"""
        taps = ctx["taps"] if len(d_hidden) else ()
        if len(d_hidden) != len(taps):
            raise ValueError("ClipVisual: %d hidden cotangents for taps %s" % (len(d_hidden), ctx["taps"]))
        tape, _, ws = self._backward_buffers(ctx["n"], self._flat.device)
        dh = torch.stack([d.to(torch.float32) for d in d_hidden]).contiguous() if taps else None
        de = None if d_embedding is None else d_embedding.to(torch.float32).contiguous()
        return ops.clip_visual_backward(self._ccfg, self._flat, self.flat_weights_t(), tape, ctx["n"], d_out=de, taps=taps, d_hidden=dh, ws=ws)

    def features(self, image, taps=()):
        """image fp32 [N, 3, H, W] in [-1, 1], any size -> (embedding, [hidden states of the blocks in taps], ctx), differentiable with
        features_backward: area pooling to the tower's resolution and CLIP's normalisation (ops.clip_area_preprocess), then forward_taped"""
        if not image.is_cuda:
            raise RuntimeError("ClipVisual: HIP path only (the tower runs through vts_clip_visual_forward_tape); input is on %s" % image.device)
        emb, hidden, ctx = self.forward_taped(ops.clip_area_preprocess(image.contiguous(), self.cfg["resolution"]), taps)
        ctx["hw"] = tuple(image.shape[2:])
        return emb, hidden, ctx

    def features_backward(self, ctx, d_embedding=None, d_hidden=()):
        """-> d_image fp32 [N, 3, H, W]"""
        return ops.clip_area_preprocess_bwd(self.input_gradient(ctx, d_embedding, d_hidden), *ctx["hw"])

    def forward(self, x, out=None):
        """x: fp16 [N, 3, res, res] (ops.clip_preprocess's output) -> fp32 [N, output_dim]"""
        if not x.is_cuda:
            raise RuntimeError("ClipVisual: HIP path only (the tower runs through vts_clip_visual_forward); input is on %s" % x.device)
        flat = self.flat_weights()
        # a scratch of the tower's own, per batch size (10 MB at batch 4): the call sits in set_input next to captured training graphs,
        # which hold pointers into the shared workspace
        ws = self._ws.get(x.shape[0])
        if ws is None:
            ws = self._ws[x.shape[0]] = torch.empty(ops.clip_visual_forward_ws_floats(self._ccfg, x.shape[0]), dtype=torch.float32, device=x.device)
        return ops.clip_visual_forward(self._ccfg, flat, x, out=out, ws=ws)

    def encode(self, image, out=None):
        """the reference's style code of an fp32 [N, 3, H, W] image in [-1, 1]: CLIP's pre-processing, then the tower, all on the device"""
        return self.forward(ops.clip_preprocess(image.contiguous()), out=out)


def clip_visual(opt=None):
    net = ClipVisual()
    path = (getattr(opt, "clip_weights", None) if opt is not None else None) or os.environ.get("VTS_CLIP_WEIGHTS")
    if path:
        net.load_weights(path)
    return net
