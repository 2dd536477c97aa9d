"""Explicit forward / backward schedules of every network over libvts_hip.so.

There is no autograd on the hot path: the networks are fixed graphs, so their backward passes are written out as kernel sequences (PyTorch
autograd in the reference).  Activations travel as `ops.Act` (raw tensor + per-(n,c) scale/shift): a normalisation layer is a statistics
pass only, and every consumer (next conv, skip concat, derivative mask, weight gradient) normalises on load inside the conv kernels.

In file order, each section under a banner that cites the reference graph it reproduces:
  style-conditioned U-Net (unet_*; CustomUnetGenerator), the classic pix2pix U-Net (unet_classic_*)
  the ResNet family (resnet_*, local_enhancer_forward: ResnetGenerator, pix2pixHD GlobalGenerator / LocalEnhancer), one record per layer
  the multiscale PatchGAN discriminators (msd_*), SideQueue and the lane helpers the step schedules fork with
  StyleGAN2 discriminator, generator and modulated convolutions (sg2d_*, sg2g_*, modulated_conv2d ...)
  SIFID / T_FID evaluation metrics, and the SPADE generator (spade_*)
"""
import ctypes as C
import os
from . import tune

import torch

from . import lanes
from . import lib as L
from . import ops
from .ops import Act

LRELU, RELU, TANH = L.ACT_LRELU, L.ACT_RELU, L.ACT_TANH


def _empty(n, c, h, w, dev):
    return torch.empty(n, c, h, w, dtype=torch.float32, device=dev)


def _as_act(x):
    return x if isinstance(x, Act) else Act(x)


# =====================================================================================
# generator
# =====================================================================================

class UnetCtx:
    __slots__ = ("x", "feats", "ups", "g_out", "style", "style_ctx", "adain_in", "adain_src", "bias_levels", "dstyle")


def dropout_layers(G):
    """the Up blocks that end in Dropout(0.5) when the generator was built with use_dropout (reference networks.py:1508-1519), in the
    order the forward visits them"""
    if not getattr(G, "use_dropout", False):
        return []
    return list(range(G.num_downs - 2, G.num_downs // 2 - 1, -1))


def unet_forward(G, x, style_code=None, keep=True, style_tiles=None, dropout_masks=None):
    """x: [N, input_nc, H, W] tensor / Act, or a pair (x0, x1) that is concatenated on load
    (sketch ++ positional grid).  Returns (g_out [N,5,H,W] post-tanh, ctx).
    style_tiles: {layer index: [N, style_dim, h, w]} the tiled style code when the caller holds it (it depends on the batch only: the
    model tiles it once per set_input instead of once per step)
    dropout_masks: {layer index: keep mask [N, C, h, w] of 0 / 1} for the Up blocks of dropout_layers(G) in train() mode (drawn here with
    torch.bernoulli when absent; tests pass the reference's draws)"""
    if isinstance(x, (tuple, list)):
        x, x_extra = _as_act(x[0]), _as_act(x[1])
    else:
        x, x_extra = _as_act(x), None
    xd = x.data
    n, _, h, w = xd.shape
    dev = xd.device
    nd, ch = G.num_downs, G.channels
    if h % (1 << nd) or w % (1 << nd):
        raise ValueError("unet256_custom needs H, W divisible by %d, got %dx%d" % (1 << nd, h, w))
    feats = []
    a = x
    for i in range(nd):
        blk = getattr(G, "down%d" % i).conv
        cin = blk.weight.shape[1]
        hh, ww = h >> (i + 1), w >> (i + 1)
        out = _empty(n, ch[i], hh, ww, dev)
        normed = 0 < i < nd - 1
        r = ops.conv4x4(a, blk.weight, cin * 16, 16, ch[i], out, in1=x_extra if i == 0 else None, bias=blk.bias, stride=2, pad=1,
                        act_in=LRELU if i else 0, instance_norm=normed)
        a = r if normed else Act(out)
        feats.append(a)

    style = None
    if style_code is not None:
        if not G.use_style:
            raise ValueError("generator was built without style code support")
        style = style_code.to(torch.float32).contiguous()
    g_out = _empty(n, 5, h, w, dev)
    ups = {}
    extras = {}
    style_ctx = {}
    bias_levels = set()     # concat + tile below the innermost level: the tile's term of the output is a 16-class bias, no tile exists
    for i in range(nd):
        if style is not None and i >= nd - G.num_layer_style_code:
            hh, ww = h >> (i + 1), w >> (i + 1)
            if G.style_mapping == "tile":
                if i != nd - 1:
                    bias_levels.add(i)
                    continue
                t = style_tiles.get(i) if style_tiles else None
                extras[i] = Act(t if t is not None else style[:, :, None, None].expand(-1, -1, hh, ww).contiguous())
            else:
                smap, style_ctx[i] = _style_map_forward(G, nd - 1 - i, style, hh, ww)
                if G.style_mode == "concat":
                    extras[i] = Act(smap)
                else:
                    style_ctx[i] += (smap,)

    drop_layers = dropout_layers(G) if G.training else []

    def up(i, name, inp):
        hh, ww = h >> (i + 1), w >> (i + 1)
        skip = None if i in (0, nd - 1) else feats[i]
        extra = extras.get(i)
        blk = getattr(G, name).conv
        outer = blk.weight.shape[1]
        if i == 0:
            c0 = 0 if name == "up0" else 3
            out = g_out[:, c0:c0 + outer]
        else:
            out = _empty(n, outer, hh * 2, ww * 2, dev)
        tiled = i in bias_levels
        if tiled or (skip is not None and extra is not None):
            # three concat sources, ReLU(cat[x, style_i, skip_i]) (unet_parts_custom.py:61-79, networks.py:1620-1623): every source owns
            # a contiguous block of rows of the [Cin, Cout, 4, 4] weight, so each is one accumulating launch on its row block; the
            # tiled code's term is the class bias.  The statistics follow on the sum (a launch's fused ones would miss the other terms).
            c_x, rows, wflat = inp.data.shape[1], outer * 16, blk.weight.view(-1)
            kw = dict(stride=2, pad=1, transposed=True, act_in=RELU)
            ops.conv4x4(inp, blk.weight, 16, rows, outer, out, bias=blk.bias, **kw)
            if extra is not None:
                ops.conv4x4(extra, wflat[c_x * rows:], 16, rows, outer, out, accumulate=True, **kw)
            if skip is not None:
                ops.conv4x4(skip, wflat[(c_x + G.style_nc) * rows:], 16, rows, outer, out, accumulate=True, **kw)
            if tiled:
                ops.style_bias(style, wflat[c_x * rows:(c_x + G.style_nc) * rows], out, act_out=TANH if i == 0 else 0)
            r = ops.norm_stats(out, 0) if i != 0 else None
        else:
            r = ops.conv4x4(inp, blk.weight, 16, outer * 16, outer, out, in1=skip if skip is not None else extra, bias=blk.bias,
                            stride=2, pad=1, transposed=True, act_in=RELU, act_out=TANH if i == 0 else 0, instance_norm=i != 0)
        res = Act(out) if i == 0 else r
        drop = None
        if i in drop_layers:
            # Dropout(0.5) behind the InstanceNorm: the normalised map is materialised, multiplied by keep * 2 (tiny maps: 80 channels at
            # <= 1/16 of the resolution), and the next block reads it as a plain tensor; the backward multiplies by the same map
            keep2 = dropout_masks.get(i) if dropout_masks is not None else None
            if keep2 is None:
                keep2 = torch.bernoulli(torch.full(out.shape, 0.5, device=dev))
            keep2 = (keep2.to(device=dev, dtype=torch.float32) * 2.0).contiguous()
            y = ops.pad_affine(r, (0, 0, 0, 0), 0)
            yd = torch.empty_like(y)
            ops.mask_mul(y.view(-1, 1, y.shape[2], y.shape[3]), keep2.view(-1, 1, y.shape[2], y.shape[3]), out=yd.view(-1, 1, y.shape[2], y.shape[3]))
            drop = (r, keep2)
            res = Act(yd)
        ups[name] = (inp, res, extra, drop)
        return res

    nls = G.num_layer_separate
    xm = feats[nd - 1]
    adain_in, adain_src = {}, {}
    is_adain = G.style_mode == "adain" and bool(style_ctx)
    if is_adain and min(style_ctx) < nls - 1:
        raise NotImplementedError("adain style conditioning of up%d inside the separate decoders (num_layer_style_code %d with num_layer_separate %d): "
                                  "the tactile chain's own x_T = adain(x_T, style) (networks.py:1629-1630) is not built" % (min(style_ctx), G.num_layer_style_code, nls))

    def adain_at(i, xm):
        """x = adaptive_instance_normalization(x, style map) in front of up<i> (networks.py:1624-1630); a content that carries a deferred
        InstanceNorm affine (the block above) is materialised"""
        x_raw = ops.pad_affine(xm, (0, 0, 0, 0), 0) if (xm.scale is not None) else xm.data
        adain_in[i], adain_src[i] = x_raw, xm
        return Act(ops.adain(x_raw, style_ctx[i][-1]))

    for i in range(nd - 1, nls - 1, -1):      # shared trunk
        if is_adain and i in style_ctx:
            xm = adain_at(i, xm)
        xm = up(i, "up%d" % i, xm)
    if is_adain and nls > 0 and (nls - 1) in style_ctx and (nls - 1) not in adain_in:
        xm = adain_at(nls - 1, xm)            # the split point: up<i> and up<i>_T both read the one adain(x) (x_T is x there)

    def chain(lane):                          # the visual (lane 0) and tactile (lane 1) decoders are independent chains
        x = xm
        for i in range(nls - 1, -1, -1):
            x = up(i, "up%d%s" % (i, "_T" if lane else ""), x)

    if nls > 0:
        _run_lanes(2, chain)
    if not keep:
        return g_out, None
    ctx = UnetCtx()
    ctx.x, ctx.feats, ctx.ups, ctx.g_out, ctx.style = (x, x_extra), feats, ups, g_out, style
    ctx.style_ctx, ctx.adain_in, ctx.adain_src, ctx.bias_levels, ctx.dstyle = style_ctx, adain_in, adain_src, bias_levels, None
    return g_out, ctx


def unet_desc(G, x, g_out, style_tile=None, side_stream=None):
    """vts_unet_desc of generator G on the input x (a tensor / Act or a pair that is concatenated on load) writing g_out [N, 5, H, W]:
    the network-level C entry vts_unet_forward (include/vts.h) runs the inference forward from it.  style_tile: [N, style_dim, h, w]
    tiled style code of the innermost block (style_code_mode concat + mapping tile), or None."""
    import ctypes as C

    if isinstance(x, (tuple, list)):
        x0, x1 = _as_act(x[0]), _as_act(x[1])
    else:
        x0, x1 = _as_act(x), None
    n, _, h, w = x0.data.shape
    nd = G.num_downs
    if nd > L.UNET_MAX_DOWNS:
        raise ValueError("vts_unet_forward takes at most %d down blocks" % L.UNET_MAX_DOWNS)
    d = L.UnetDesc()
    d.N, d.H, d.W, d.num_downs, d.num_layer_separate = n, h, w, nd, G.num_layer_separate
    d.in0 = x0.operand()
    d.in1 = x1.operand() if x1 is not None else L.Operand(None, None, None, 0, 0)
    for i in range(nd):
        dn, up = getattr(G, "down%d" % i).conv, getattr(G, "up%d" % i).conv
        d.channels[i] = dn.weight.shape[0]
        d.down_w[i], d.down_b[i] = dn.weight.data_ptr(), L.ptr(dn.bias)
        d.up_w[i], d.up_b[i], d.up_cout[i] = up.weight.data_ptr(), L.ptr(up.bias), up.weight.shape[1]
        if i < G.num_layer_separate:
            ut = getattr(G, "up%d_T" % i).conv
            d.upT_w[i], d.upT_b[i], d.upT_cout[i] = ut.weight.data_ptr(), L.ptr(ut.bias), ut.weight.shape[1]
    d.style = L.operand(style_tile) if style_tile is not None else L.Operand(None, None, None, 0, 0)
    d.out = g_out.data_ptr()
    d.side_stream = side_stream.cuda_stream if side_stream is not None else None     # the tactile branch's lane
    return d


def unet_c_ok(G, style_code):
    """can vts_unet_forward run this generator's inference forward?  (plain U-Net, or the style code tiled into the innermost block;
    every other configuration keeps the Python schedule, which measured the same speed: 0.201 vs 0.200 ms per image, bit-identical)"""
    if G.num_downs > L.UNET_MAX_DOWNS:
        return False
    if G.num_layer_separate >= G.num_downs:     # no shared decoder trunk (every up block duplicated): the C entry's check() refuses it
        return False
    if G.training and dropout_layers(G):     # a forward outside eval() keeps the Dropout of the Up blocks active
        return False
    if style_code is None:
        return True
    return bool(G.use_style) and G.style_mapping == "tile" and G.style_mode == "concat" and G.num_layer_style_code == 1


def unet_forward_infer(G, x, style_code=None, style_tiles=None):
    """inference forward (nothing kept for a backward) -> g_out: ONE call of the network-level C entry where it covers the configuration
    (the tactile decoder branch on the first side lane, as unet_forward runs it), else the Python schedule"""
    if not unet_c_ok(G, style_code):
        return unet_forward(G, x, style_code=style_code, keep=False, style_tiles=style_tiles)[0]
    tile = None
    if style_code is not None:
        i = G.num_downs - 1
        tile = style_tiles.get(i) if style_tiles else None
        if tile is None:
            x0 = _as_act(x[0] if isinstance(x, (tuple, list)) else x).data
            hh, ww = x0.shape[2] >> G.num_downs, x0.shape[3] >> G.num_downs
            tile = style_code.to(torch.float32)[:, :, None, None].expand(-1, -1, hh, ww).contiguous()
    side = lanes.lane(1).stream if PARALLEL_SCALES and G.num_layer_separate > 0 else None
    return unet_forward_c(G, x, style_tile=tile, side_stream=side)


def unet_forward_c(G, x, style_tile=None, g_out=None, side_stream=None):
    """the generator's inference forward through ONE C call (vts_unet_forward); bit-identical to unet_forward(keep=False)"""
    import ctypes as C

    lib = L.load()
    x0 = _as_act(x[0] if isinstance(x, (tuple, list)) else x)
    n, _, h, w = x0.data.shape
    if g_out is None:
        nls = G.num_layer_separate
        oc = G.up0.conv.weight.shape[1] + (G.up0_T.conv.weight.shape[1] if nls > 0 else 0)
        g_out = _empty(n, oc, h, w, x0.data.device)
    d = unet_desc(G, x, g_out, style_tile, side_stream)
    need = lib.vts_unet_forward_ws_floats(C.byref(d))
    if need < 0:
        raise RuntimeError("vts_unet_forward: %s" % lib.vts_last_error().decode())
    ws = torch.empty(int(need), dtype=torch.float32, device=x0.data.device)
    L.check(lib.vts_unet_forward(C.byref(d), ws.data_ptr(), ws.numel(), L.stream()), "vts_unet_forward")
    return g_out


def unet_forward_train_c(G, x, style_tile=None, side_stream=None):
    """the forward through vts_unet_forward into a workspace sized for vts_unet_backward (include/vts.h: the forward's region is its
    prefix): returns (g_out, ctx) for unet_backward_c.  Not the product's path (the training step keeps the Python schedule)."""
    lib = L.load()
    x0 = _as_act(x[0] if isinstance(x, (tuple, list)) else x)
    n, _, h, w = x0.data.shape
    oc = G.up0.conv.weight.shape[1] + (G.up0_T.conv.weight.shape[1] if G.num_layer_separate > 0 else 0)
    g_out = _empty(n, oc, h, w, x0.data.device)
    d = unet_desc(G, x, g_out, style_tile, side_stream)
    need = int(lib.vts_unet_backward_ws_floats(C.byref(d)))
    if need < 0:
        raise RuntimeError("vts_unet_backward_ws_floats: %s" % lib.vts_last_error().decode())
    ws = torch.empty(need, dtype=torch.float32, device=x0.data.device)
    L.check(lib.vts_unet_forward(C.byref(d), ws.data_ptr(), ws.numel(), L.stream()), "vts_unet_forward")
    return g_out, (x, style_tile, g_out, ws)


def unet_grads(G, d_raw):
    """vts_unet_grads over the modules' .grad tensors (allocated where missing)"""
    g = L.UnetGrads()
    g.d_raw, g.d_raw_nstride = d_raw.data_ptr(), d_raw.stride(0)
    for i in range(G.num_downs):
        names = [("down", "down%d" % i), ("up", "up%d" % i)] + ([("upT", "up%d_T" % i)] if i < G.num_layer_separate else [])
        for field, name in names:
            conv = getattr(G, name).conv
            for p in (conv.weight, conv.bias):
                if p is not None and p.grad is None:
                    p.grad = torch.empty_like(p)
            getattr(g, field + "_dw")[i] = conv.weight.grad.data_ptr()
            getattr(g, field + "_db")[i] = L.ptr(conv.bias.grad if conv.bias is not None else None)
    return g


def unet_backward_c(G, ctx, d_raw, side_stream=None):
    """the generator's backward through ONE C call (vts_unet_backward) on the workspace of unet_forward_train_c: overwrites every
    parameter's .grad, bit-identical to unet_backward (tests/test_network_bwd_gpu.py)"""
    lib = L.load()
    x, style_tile, g_out, ws = ctx
    d = unet_desc(G, x, g_out, style_tile, side_stream)
    g = unet_grads(G, d_raw)
    L.check(lib.vts_unet_backward(C.byref(d), C.byref(g), ws.data_ptr(), ws.numel(), L.stream()), "vts_unet_backward")


def _style_linear_wide(P, k):
    """the Linear of a style mapping as a 1 x 1 convolution embeds its weight in 4 x 4 tap blocks (16 x the size, twice: forward and
    gradient): fine for the innermost maps, not for the outer levels of num_layer_style_code > 1 (81920 x 512 at a 128 x 128 map)"""
    return P * k > (1 << 21)


def _style_map_forward(G, j, style, hh, ww):
    """style_code_mapping<j> (networks.py:1459-1465, 1611-1615): Linear(style_dim, P, bias=False) -> BatchNorm1d (batch_size > 1) |
    InstanceNorm1d -> ReLU, reshaped to [N, P / (h w), h, w].  The Linear is a 1 x 1 convolution on a 1 x 1 map; BatchNorm1d over
    [N, P] is BatchNorm2d on [N, P, 1, 1]; InstanceNorm1d on the 2-D tensor normalises every row over its P features (torch treats
    [N, P] as an unbatched (C = N, L = P) input), i.e. InstanceNorm2d on [N, 1, P, 1]."""
    m = getattr(G, "style_code_mapping%d" % j)
    lin = getattr(m, "0")
    bn = getattr(m, "1", None)
    n, k = style.shape
    P = lin.weight.shape[0]
    if P % (hh * ww):
        raise ValueError("style_code_mapping%d emits %d features, not a multiple of the %d x %d map: the reference builds it for a %d-pixel "
                         "input (networks.py:1432, 1458)" % (j, P, hh, ww, 1536))
    z = _empty(n, P, 1, 1, style.device)
    sv = style.reshape(n, k, 1, 1).contiguous()
    if _style_linear_wide(P, k):
        ops.style_linear(sv.view(n, k), lin.weight, out=z.view(n, P))
    else:
        ops.convk(sv, lin.weight.view(P, k, 1, 1), z, pad=0)
    if bn is not None:
        if G.training:
            a = ops.norm_stats(z, 1, gamma=bn.weight, beta=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var, nbt=bn.num_batches_tracked)
        else:
            sc = bn.weight / torch.sqrt(bn.running_var + 1e-5)
            a = Act(z, sc.repeat(n).contiguous(), (bn.bias - bn.running_mean * sc).repeat(n).contiguous())
        y = ops.pad_affine(a, (0, 0, 0, 0), 0, act=RELU)
    else:
        a = ops.norm_stats(z.view(n, 1, P, 1), 0)
        y = ops.pad_affine(a, (0, 0, 0, 0), 0, act=RELU)
    return y.view(n, P // (hh * ww), hh, ww), (j, sv, a, bn)


def _style_map_backward(G, sctx, d_map, want_dstyle=False):
    """parameter gradients of style_code_mapping<j> from the gradient w.r.t. its output map; returns d/d style_code when asked"""
    j, sv, a, bn = sctx[:4]
    m = getattr(G, "style_code_mapping%d" % j)
    lin = getattr(m, "0")
    n, k = sv.shape[0], sv.shape[1]
    P = lin.weight.shape[0]
    g = d_map.reshape(a.data.shape).contiguous()
    dz = torch.empty_like(g)
    ops.act_bwd(g, a, RELU, dz)
    if bn is not None:
        if G.training:
            ops.norm_bwd(dz, a, 1, gamma=bn.weight, dgamma=bn.weight.grad, dbeta=bn.bias.grad)
        else:
            raise NotImplementedError("backward through an eval-mode BatchNorm1d")
    else:
        ops.norm_bwd(dz, a, 0)
    dz = dz.view(n, P, 1, 1)
    if _style_linear_wide(P, k):
        return ops.style_linear_bwd(dz.view(n, P), sv.view(n, k), lin.weight, lin.weight.grad, want_dx=want_dstyle)
    ops.wgradk(dz, sv, lin.weight.grad.view(P, k, 1, 1), pad=0)
    if not want_dstyle:
        return None
    ds = torch.empty_like(sv)
    ops.convk_bwd_data(dz, lin.weight.view(P, k, 1, 1), ds, pad=0)
    return ds.view(n, k)


def _add_dstyle(ctx, ds):
    """ctx.dstyle += one style mapping's d/d style_code [N, style_dim]"""
    if ctx.dstyle is None:
        ctx.dstyle = ds
    else:
        n = ds.shape[0]
        ctx.dstyle = ops.pad_affine(ctx.dstyle.view(n, -1, 1, 1), (0, 0, 0, 0), 0, res=ds.view(n, -1, 1, 1)).view(n, -1)


def unet_backward(G, ctx, d_raw):
    """d_raw: [N,5,H,W] gradient wrt the pre-tanh outputs of up0 / up0_T.
    Writes every parameter's .grad (overwrite) -- the G step has a single backward.
    The deterministic reduction of all weight-gradient partials is ONE launch at the end (ops.deferred_wgrad)."""
    with ops.deferred_wgrad():
        _unet_backward(G, ctx, d_raw)


def unet_backward_decoder(G, ctx, d_raw):
    """first half of unet_backward: every decoder (up*) gradient is complete when it returns (data-parallel runs all-reduce that
    bucket while unet_backward_encoder runs).  Returns the state the second half needs."""
    with ops.deferred_wgrad():
        return _unet_backward(G, ctx, d_raw, part="decoder")


def unet_backward_encoder(G, ctx, state):
    with ops.deferred_wgrad():
        _unet_backward(G, ctx, None, part="encoder", state=state)


def _unet_backward(G, ctx, d_raw, part="all", state=None):
    if part == "encoder":
        dfeat = state
        feats = ctx.feats
        nd = G.num_downs
        dev = dfeat[nd - 1].device
        sq = SideQueue()
        return _unet_backward_encoder(G, ctx, dfeat, feats, nd, dev, sq)
    nd, ch = G.num_downs, G.channels
    n = d_raw.shape[0]
    dev = d_raw.device
    feats = ctx.feats
    sq = SideQueue()         # weight / bias gradients: off the critical path
    dfeat = [None] * nd      # grad wrt the normalised feats[i] (pre-activation), accumulated over consumers
    dx = {}                  # id(Act) of an up-output -> grad wrt its normalised value

    def add_grad(store, key, shape):
        """returns (tensor, accumulate?)"""
        if key in store and store[key] is not None:
            return store[key], True
        t = torch.empty(shape, dtype=torch.float32, device=dev)
        store[key] = t
        return t, False

    dropped = {id(v[1]) for v in ctx.ups.values() if v[3] is not None}

    def dropped_input(inp):
        """the block's primary input is a Dropout output: its gradient is not yet the gradient of a normalised map (no fused sums)"""
        return id(inp) in dropped

    dmaps = {}               # styled level -> grad wrt its projected style map (both decoders' parts summed): feeds style_code_mapping<j>

    def up_bwd(i, name, dx, dfeat, wq, dmaps, lane_mode=False):
        """backward of one up block: weight gradient (through wq: side queue, or inline inside a lane), gradient w.r.t.
        the block input into dx / dfeat[nd-1], gradient w.r.t. the skip feature into dfeat[i], gradient w.r.t. a concatenated
        projected style map into dmaps[i]"""
        skip = None if i in (0, nd - 1) else feats[i]
        blk = getattr(G, name).conv
        inp, outp, extra, drop = ctx.ups[name]
        outer = blk.weight.shape[1]
        if i == 0:
            c0 = 0 if name == "up0" else 3
            g = d_raw[:, c0:c0 + outer]  # channel-slice view: batch stride stays 5*H*W
        else:
            g = dx.pop(id(outp))
            if drop is not None:     # Dropout backward: the same keep * 2 map, then the InstanceNorm backward on the block's own statistics
                gd = torch.empty_like(g)
                ops.mask_mul(g.view(-1, 1, g.shape[2], g.shape[3]), drop[1].view(-1, 1, g.shape[2], g.shape[3]), out=gd.view(-1, 1, g.shape[2], g.shape[3]))
                g = gd
                ops.norm_bwd(g, drop[0], 0)
            else:
                ops.norm_bwd(g, outp, 0)
        gop = Act(g)
        second = skip if skip is not None else extra
        c_in0 = inp.data.shape[1]
        tiled = i in ctx.bias_levels
        three = tiled or (skip is not None and extra is not None)      # ReLU(cat[x, style_i, skip_i]): one row block of the weight per source
        c_sk = c_in0 + (G.style_nc if three else 0)                    # first weight row of the skip source
        if three:
            rows, dwf = outer * 16, blk.weight.grad.view(-1)
            wq(lambda: ops.wgrad4x4(inp, gop, dwf[:c_in0 * rows], act_lo=RELU, stride=2, pad=1), g)
            if extra is not None:
                wq(lambda: ops.wgrad4x4(extra, gop, dwf[c_in0 * rows:c_sk * rows], act_lo=RELU, stride=2, pad=1), g)
            if tiled:      # the tiled code's rows: class sums of g (no tile is read)
                wq(lambda: ops.style_bias_bwd(g, ctx.style, dwf[c_in0 * rows:c_sk * rows]), g)
            if skip is not None:
                wq(lambda: ops.wgrad4x4(skip, gop, dwf[c_sk * rows:], act_lo=RELU, stride=2, pad=1), g)
        else:
            wq(lambda: ops.wgrad4x4(inp, gop, blk.weight.grad, lo1=second, act_lo=RELU, stride=2, pad=1), g)
        if i == 0:
            wq(lambda: ops.channel_sum(g, blk.bias.grad), g)
        # else: the bias feeds an InstanceNorm, so its gradient is identically zero (the norm removes any
        # per-channel constant).  The reference computes ~1e-9 rounding noise there; the flat gradient
        # buffer is zero-initialised and this slot is never written, i.e. exactly 0.
        # grad wrt the primary input (normalised output of the previous up block, or feats[nd-1])
        if i == nd - 1:
            tgt, acc = add_grad_list(dfeat, nd - 1, inp.data.shape, dev)
        else:
            tgt, acc = add_grad(dx, id(inp), inp.data.shape)
        # (the tensor goes straight into the InstanceNorm backward of the block below unless it is the un-normalised innermost feature
        #  or the split point i == nls - 1, where up{i} and up{i}_T BOTH contribute -- as two lanes or, with VTS_PARALLEL_SCALES=0, as
        #  two accumulating calls: the fused sums (and the k-split epilogue's fused backward) would see only one part of the gradient;
        #  nor where the input is an AdaIN output: its gradient passes through adain_bwd before it reaches that InstanceNorm backward)
        ops.conv4x4(gop, blk.weight, outer * 16, 16, c_in0, tgt, stride=2, pad=1, dmask=inp, dmask_act=RELU, accumulate=acc,
                    bwd_sums="in" if (i != nd - 1) and not (nls > 0 and i == nls - 1) and not dropped_input(inp) and i not in ctx.adain_in else False)
        if skip is not None:
            tgt, acc = add_grad_list(dfeat, i, skip.data.shape, dev)
            wv = blk.weight.view(-1)[c_sk * outer * 16:]
            ops.conv4x4(gop, wv, outer * 16, 16, skip.data.shape[1], tgt, stride=2, pad=1, dmask=skip, dmask_act=RELU,
                        accumulate=acc)
        if extra is not None and i in ctx.style_ctx and G.style_mode == "concat":
            # projected style map as a concat source: its gradient (backward-data on its row block) feeds style_code_mapping<j>'s
            # parameters, after the parts of up<i> and up<i>_T have been summed
            d_map, acc = add_grad(dmaps, i, extra.data.shape)
            wv = blk.weight.view(-1)[c_in0 * outer * 16:]
            ops.conv4x4(gop, wv, outer * 16, 16, extra.data.shape[1], d_map, stride=2, pad=1, dmask=extra, dmask_act=RELU, accumulate=acc)

    def adain_bwd_at(i):
        """up<i> (and up<i>_T at the split point) consumed adain(x, style map), x the normalised output of up<i+1>: the gradient of
        that input splits into the content part, which goes on into the InstanceNorm backward of up<i+1>, and the style part"""
        if i not in ctx.adain_in or i == nd - 1:      # (the innermost level's content is feats[nd-1]: _unet_backward_encoder)
            return
        gin = dx.pop(id(ctx.ups["up%d" % i][0]))
        dxr, dsm = ops.adain_bwd(gin.contiguous(), ctx.adain_in[i], ctx.style_ctx[i][-1])
        dx[id(ctx.adain_src[i])] = dxr
        dmaps[i] = dsm

    nls = G.num_layer_separate
    if nls > 0 and PARALLEL_SCALES:
        # the visual and the tactile decoder are independent chains: two lanes with their own gradient buffers,
        # summed where the chains share a tensor (skip features, the split point)
        lane_dx, lane_df, lane_dm = [{}, {}], [[None] * nd, [None] * nd], [{}, {}]

        def inline(fn, *keep):
            fn()

        def chain(lane):
            # (weight gradients inline.  Round 4 re-measured them on a queue of their own per lane -- four streams, both queues forked
            # from the launch stream in front of the lanes: + 0.22 ms on the step, as with one shared queue in round 3.  Round 6: the
            # lanes' SKIP-feature gradients -- first read when the encoder's backward reaches their level -- enqueued on the side queue
            # behind the lanes instead of inside them: 5.31 - 5.34 against 5.25 - 5.28 ms (profiles/r06a_experiments.md section 2b).  The backward
            # is throughput-bound: work moved beside its chain slows the chain by as much.)
            for i in range(nls):
                up_bwd(i, "up%d%s" % (i, "_T" if lane else ""), lane_dx[lane], lane_df[lane], inline, lane_dm[lane], lane_mode=True)

        _run_lanes(2, chain)

        def total(a, b):
            return a if b is None else (b if a is None else ops.pad_affine(a, (0, 0, 0, 0), 0, res=b))

        for i in range(nd):
            dfeat[i] = total(lane_df[0][i], lane_df[1][i])
        for key in set(lane_dx[0]) | set(lane_dx[1]):
            dx[key] = total(lane_dx[0].get(key), lane_dx[1].get(key))
        for i in sorted(set(lane_dm[0]) | set(lane_dm[1])):
            dmaps[i] = total(lane_dm[0].get(i), lane_dm[1].get(i))
        first_shared = nls
        adain_bwd_at(nls - 1)
    else:
        first_shared = 0
    for i in range(first_shared, nd):
        names = ["up%d" % i] + (["up%d_T" % i] if nls >= i + 1 else [])
        for name in names:
            up_bwd(i, name, dx, dfeat, sq.run, dmaps)
        adain_bwd_at(i)
    for i in sorted(dmaps, reverse=True):     # d/d style_code: the sum over the levels from the inside out, a fixed order (an innermost
                                              # AdaIN level joins last, in _unet_backward_encoder)
        _add_dstyle(ctx, _style_map_backward(G, ctx.style_ctx[i], dmaps[i], want_dstyle=True))

    if part == "decoder":
        sq.join()
        return dfeat
    return _unet_backward_encoder(G, ctx, dfeat, feats, nd, dev, sq)


def _unet_backward_encoder(G, ctx, dfeat, feats, nd, dev, sq):
    if (nd - 1) in ctx.adain_in:      # up7 consumed adain(feats[7], style map): split its input gradient into content and style parts
        x_raw = ctx.adain_in[nd - 1]
        smap = ctx.style_ctx[nd - 1][-1]
        dxr, dsm = ops.adain_bwd(dfeat[nd - 1].contiguous(), x_raw, smap)
        dfeat[nd - 1] = dxr
        _add_dstyle(ctx, _style_map_backward(G, ctx.style_ctx[nd - 1], dsm, want_dstyle=True))
    for i in range(nd - 1, -1, -1):
        blk = getattr(G, "down%d" % i).conv
        g = dfeat[i]
        if 0 < i < nd - 1:
            ops.norm_bwd(g, feats[i], 0)
        src, src1 = ctx.x if i == 0 else (feats[i - 1], None)
        sq.run(lambda: ops.wgrad4x4(Act(g), src, blk.weight.grad, hi1=src1, act_hi=LRELU if i else 0, stride=2, pad=1), g)
        if not (0 < i < nd - 1):
            sq.run(lambda: ops.channel_sum(g, blk.bias.grad), g)   # bias gradients of normalised layers are identically zero (see above)
        if i > 0:
            cin = blk.weight.shape[1]
            tgt, acc = add_grad_list(dfeat, i - 1, feats[i - 1].data.shape, dev)
            ops.conv4x4(Act(g), blk.weight, 16, cin * 16, cin, tgt, stride=2, pad=1, transposed=True, dmask=feats[i - 1],
                        dmask_act=LRELU, accumulate=acc, bwd_sums="in" if i - 1 > 0 else False)     # the last contribution to dfeat[i-1]: its InstanceNorm backward is next
        dfeat[i] = None
    sq.join()


# -------------------------------------------------------------------------------------
# classic pix2pix U-Net (--netG unet_128 | unet_256): reference models/networks.py:1327-1426
# -------------------------------------------------------------------------------------
# Level i (0 = outermost): feats[i] = [norm](down<i>(LeakyReLU(feats[i-1]))), u[i] = [norm](up<i>(ReLU(cat[feats[i], u[i+1]]))).  The
# reference's in-place LeakyReLU rewrites the skip before the cat, but every consumer of a cat starts with ReLU and
# ReLU(LeakyReLU(x)) = ReLU(x): the skip is ReLU(raw feature) in the forward and in the gradient.
#
# A launch whose OUTPUT has at most 80 channels runs on the 4 x 4 kernels (vts_conv4x4: operands on load), as every layer of the
# model's default ngf = 10 does.  Above that the 4 x 4 kernels would loop over 80-channel groups that each re-read the input; those
# launches take the GEMM-class family on operands pre-padded by one (vts_pad_affine: one call per concat source into its channel slice,
# with the pending norm and activation):
#   down forward, up input adjoint      vts_conv4x4_wide(stride 2)
#   up forward, down input adjoint      vts_tconv4x4s2p1_wide on input maps of <= 128 pixels (its flattened-batch kernel, k-split; see
#                                       _uc_tconv_wide for the one band of batch sizes left out).  On larger maps its tiled parity-phase
#                                       kernel (four launches, no k-split) measured 1.3 - 7x SLOWER than the group loop on every shape
#                                       of unet_256 at ngf 64 (profiles/r24_unet_classic.md): those launches STAY on vts_conv4x4, group
#                                       loop included -- with the band, 10 of the 12 such launches of unet_256 at ngf 64 and 1024 x 1024, batch 1
# with the derivative mask of the consumer applied behind the adjoint (vts_act_bwd), as in the wide PatchGAN backward.

UC_WIDE_MIN_CO = 81
UC_TRACE = None      # a list: every convolution launch of the classic U-Net appends (layer, role, output channels, vts_last_kernel)


def _uc_wide(cout):
    """more than 80 output channels, in 16-byte packed weight rows (a count that is no multiple of 4, ngf 41's 82, stays on vts_conv4x4)"""
    return cout >= UC_WIDE_MIN_CO and cout % 4 == 0


def _uc_tconv_wide(cout, n, ih, iw):
    """the padding-1 transposed member serves this launch: more than 80 output channels on an input map its flattened-batch kernel takes
    (<= 128 pixels), unless the flattened batch fills between a quarter and all of one 128-pixel tile (32 < n ih iw < 128): there half the
    MFMA columns are empty under the deepest k-split, and the entry measured 8 - 27 % slower than vts_conv4x4 on all four such shapes of
    unet_256 at ngf 64, against 0.51 - 0.94 of its time at 128 pixels and more and 0.81 - 1.03 at 32 and fewer (profiles/r24_unet_classic.md)"""
    return _uc_wide(cout) and not (32 < n * ih * iw < 128) and ops.tconv4x4s2p1_flat_ok(ih, iw)


def _uc_note(layer, role, cout):
    if UC_TRACE is not None:
        UC_TRACE.append((layer, role, cout, L.load().vts_last_kernel().decode()))


def _uc_padded(srcs, act):
    """act(norm(cat(srcs))) zero-padded by one as one identity tensor: each source is written into its channel slice"""
    srcs = [s for s in srcs if s is not None]
    n, _, h, w = srcs[0].data.shape
    buf = torch.empty(n, sum(s.data.shape[1] for s in srcs), h + 2, w + 2, dtype=torch.float32, device=srcs[0].data.device)
    c0 = 0
    for s in srcs:
        c = s.data.shape[1]
        ops.pad_affine(s, (1, 1, 1, 1), 0, out=buf[:, c0:c0 + c], act=act, out_nstride=buf.stride(0))
        c0 += c
    return buf


def _uc_bn_kw(bn):
    return dict(gamma=bn.weight, beta=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var, nbt=bn.num_batches_tracked)


class UnetClassicCtx:
    __slots__ = ("x", "feats", "ups", "below", "drops", "padded", "g_out")


def unet_classic_forward(G, x, keep=True, dropout_masks=None):
    """x: [N, input_nc, H, W] tensor / Act, or a pair (x0, x1) concatenated on load (sketch ++ positional grid).
    Returns (g_out [N, output_nc, H, W] post-tanh, ctx).  train() mode: BatchNorm uses the batch statistics and advances the running
    ones, Dropout is live; eval(): the running statistics, no Dropout.
    dropout_masks: {level: keep mask [N, C, h, w] of 0 / 1} for G.dropout_levels() (drawn with torch.bernoulli when absent)"""
    if isinstance(x, (tuple, list)):
        x, x_extra = _as_act(x[0]), _as_act(x[1])
    else:
        x, x_extra = _as_act(x), None
    n, _, h, w = x.data.shape
    dev = x.data.device
    nd, ch = G.num_downs, G.channels
    if h % (1 << nd) or w % (1 << nd):
        raise ValueError("unet_%d needs H, W divisible by %d, got %dx%d" % (1 << nd, 1 << nd, h, w))
    feats, padded = [], {}
    a = x
    for i in range(nd):
        conv, bn = G.down(i), G.down_norm(i)
        normed = 0 < i < nd - 1
        out = _empty(n, ch[i], h >> (i + 1), w >> (i + 1), dev)
        act_in = LRELU if i else 0
        if _uc_wide(ch[i]):
            p = padded[i] = _uc_padded((a, x_extra if i == 0 else None), act_in)
            ops.conv4x4_wide(p, ops.w4x4_pack(conv.weight, "conv_fwd"), conv.bias, out, stride=2)
            _uc_note("down%d" % i, "forward", ch[i])
            r = _g_norm(G, out, bn) if normed else Act(out)
        else:
            cin = conv.weight.shape[1]
            fused = normed and (bn is None or G.training)
            kw = {} if not fused else (dict(instance_norm=True) if bn is None else dict(batch_norm=_uc_bn_kw(bn)))
            r = ops.conv4x4(a, conv.weight, cin * 16, 16, ch[i], out, in1=x_extra if i == 0 else None, bias=conv.bias, stride=2, pad=1,
                            act_in=act_in, **kw)
            _uc_note("down%d" % i, "forward", ch[i])
            if not fused:
                r = _g_norm(G, out, bn) if normed else Act(out)
        feats.append(r)
        a = r

    g_out = _empty(n, G.output_nc, h, w, dev)
    drop_levels = G.dropout_levels() if G.training else []
    ups, below, drops = [None] * nd, [None] * nd, {}
    u = None
    for i in range(nd - 1, -1, -1):
        conv, bn = G.up(i), G.up_norm(i)
        below[i] = u
        outer = conv.weight.shape[1]
        hh, ww = h >> (i + 1), w >> (i + 1)
        out = g_out if i == 0 else _empty(n, outer, 2 * hh, 2 * ww, dev)
        normed = i != 0
        if _uc_tconv_wide(outer, n, hh, ww):
            p = _uc_padded((feats[i], u), RELU)
            ops.tconv4x4s2p1_wide(p, ops.w4x4_pack(conv.weight, "convT_fwd"), conv.bias, out)
            _uc_note("up%d" % i, "forward", outer)
            r = _g_norm(G, out, bn)      # (the outermost layer has output_nc channels: never here)
        else:
            fused = normed and (bn is None or G.training)
            kw = {} if not fused else (dict(instance_norm=True) if bn is None else dict(batch_norm=_uc_bn_kw(bn)))
            r = ops.conv4x4(feats[i], conv.weight, 16, outer * 16, outer, out, in1=u, bias=conv.bias, stride=2, pad=1, transposed=True,
                            act_in=RELU, act_out=TANH if i == 0 else 0, **kw)
            _uc_note("up%d" % i, "forward", outer)
            if not fused:
                r = _g_norm(G, out, bn) if normed else Act(out)
        ups[i] = r
        if i in drop_levels:
            # Dropout(0.5) behind the norm: the normalised map is materialised and multiplied by keep * 2 (small maps: 8 ngf channels at
            # <= 1/16 of the resolution); the level above reads it as a plain tensor, the backward multiplies by the same map
            keep2 = dropout_masks.get(i) if dropout_masks is not None else None
            if keep2 is None:
                keep2 = torch.bernoulli(torch.full(out.shape, 0.5, device=dev))
            keep2 = (keep2.to(device=dev, dtype=torch.float32) * 2.0).contiguous()
            y = ops.pad_affine(r, (0, 0, 0, 0), 0)
            yd = torch.empty_like(y)
            ops.mask_mul(y.view(-1, 1, y.shape[2], y.shape[3]), keep2.view(-1, 1, y.shape[2], y.shape[3]), out=yd.view(-1, 1, y.shape[2], y.shape[3]))
            drops[i] = keep2
            r = Act(yd)
        u = r
    if not keep:
        return g_out, None
    ctx = UnetClassicCtx()
    ctx.x, ctx.feats, ctx.ups, ctx.below, ctx.drops, ctx.padded, ctx.g_out = (x, x_extra), feats, ups, below, drops, padded, g_out
    return g_out, ctx


def unet_classic_backward(G, ctx, d_raw):
    """d_raw: [N, output_nc, H, W] gradient w.r.t. the pre-tanh output.  Writes every parameter's .grad (overwrite; allocated where
    missing).  A conv bias that feeds a normalisation has an identically zero gradient: its .grad is zeroed, not computed.  Weight-gradient
    partials are reduced deterministically, in a fixed order, by one launch at the end (ops.deferred_wgrad).  No gradient w.r.t. the
    network input is formed."""
    if not G.training and G.norm == "batch":
        raise RuntimeError("unet_classic_backward: BatchNorm backward needs the batch statistics of a train() forward")
    nd, ch = G.num_downs, G.channels
    dev = d_raw.device
    feats = ctx.feats
    for p in G.parameters():
        if p.grad is None:
            p.grad = torch.zeros_like(p)

    def norm_bwd(g, a, bn):
        if bn is None:
            ops.norm_bwd(g, a, 0)
        else:
            ops.norm_bwd(g, a, 1, gamma=bn.weight, dgamma=bn.weight.grad, dbeta=bn.bias.grad)

    with ops.deferred_wgrad():
        dfeat = [None] * nd
        g = d_raw
        for i in range(nd):
            conv, bn = G.up(i), G.up_norm(i)
            outer = conv.weight.shape[1]
            if i:
                if i in ctx.drops:      # Dropout backward: the same keep * 2 map
                    gd = torch.empty_like(g)
                    ops.mask_mul(g.view(-1, 1, g.shape[2], g.shape[3]), ctx.drops[i].view(-1, 1, g.shape[2], g.shape[3]), out=gd.view(-1, 1, g.shape[2], g.shape[3]))
                    g = gd
                norm_bwd(g, ctx.ups[i], bn)
            gop = Act(g)
            skip, below = feats[i], ctx.below[i]      # the concat sources up<i> consumed (below: the level below's output, behind its Dropout)
            # (vts_wgrad4x4_wide with the roles swapped -- the activated input as dout, the padded gradient as p, both materialised --
            #  measured slower than this on 7 of the 8 full-size up layers of unet_256 at ngf 64: profiles/r24_unet_classic.md)
            ops.wgrad4x4(skip, gop, conv.weight.grad, lo1=below, act_lo=RELU, stride=2, pad=1)
            if i == 0:
                ops.channel_sum(g, conv.bias.grad)
            elif conv.bias is not None:
                conv.bias.grad.zero_()
            c = ch[i]
            srcs = [(skip, 0)] + ([(below, c)] if below is not None else [])
            q = ops.pad_affine(g, (1, 1, 1, 1), 0) if _uc_wide(c) else None
            g_next = None
            for src, c0 in srcs:
                if src is skip:
                    tgt, acc = add_grad_list(dfeat, i, src.data.shape, dev)
                else:
                    tgt, acc = torch.empty_like(src.data), False
                    g_next = tgt
                wv = conv.weight[c0:c0 + c]      # this source's rows of the [Cin, Cout, 4, 4] weight: contiguous
                if q is not None:
                    raw = torch.empty_like(src.data)
                    ops.conv4x4_wide(q, ops.w4x4_pack(wv, "convT_adj"), None, raw, stride=2)
                    _uc_note("up%d" % i, "adjoint", c)
                    ops.act_bwd(raw, src, RELU, tgt, accumulate=acc)
                else:
                    ops.conv4x4(gop, wv, outer * 16, 16, c, tgt, stride=2, pad=1, dmask=src, dmask_act=RELU, accumulate=acc)
                    _uc_note("up%d" % i, "adjoint", c)
            g = g_next
        for i in range(nd - 1, -1, -1):
            conv, bn = G.down(i), G.down_norm(i)
            g = dfeat[i]
            if 0 < i < nd - 1:
                norm_bwd(g, feats[i], bn)
            src, src1 = ctx.x if i == 0 else (feats[i - 1], None)
            p = ctx.padded.get(i)
            if p is not None and not ops.conv4x4_flat_ok(g.shape[2], g.shape[3], p.shape[2], p.shape[3]):
                ops.wgrad4x4_wide(g, p, conv.weight.grad, stride=2)      # full-size map: GEMM-class
            else:
                ops.wgrad4x4(Act(g), src, conv.weight.grad, hi1=src1, act_hi=LRELU if i else 0, stride=2, pad=1)
            if conv.bias is not None:
                if 0 < i < nd - 1:
                    conv.bias.grad.zero_()
                else:
                    ops.channel_sum(g, conv.bias.grad)
            if i > 0:
                cin = conv.weight.shape[1]
                prev = feats[i - 1]
                tgt, acc = add_grad_list(dfeat, i - 1, prev.data.shape, dev)
                if _uc_tconv_wide(cin, g.shape[0], g.shape[2], g.shape[3]):
                    raw = torch.empty_like(prev.data)
                    ops.tconv4x4s2p1_wide(ops.pad_affine(g, (1, 1, 1, 1), 0), ops.w4x4_pack(conv.weight, "conv_s2_adj"), None, raw)
                    _uc_note("down%d" % i, "adjoint", cin)
                    ops.act_bwd(raw, prev, LRELU, tgt, accumulate=acc)
                else:
                    ops.conv4x4(Act(g), conv.weight, 16, cin * 16, cin, tgt, stride=2, pad=1, transposed=True, dmask=prev, dmask_act=LRELU,
                                accumulate=acc)
                    _uc_note("down%d" % i, "adjoint", cin)
            dfeat[i] = None


# -------------------------------------------------------------------------------------
# ResNet family (--netG resnet_{4,6,9}blocks, pix2pixHD global / local): reference models/networks.py:1051-1154, 1897-1980
# -------------------------------------------------------------------------------------

class ResnetCtx:
    __slots__ = ("steps", "g_out")

    def __init__(self, steps, g_out):
        self.steps, self.g_out = steps, g_out


def _g_norm(G, r, bn):
    """normalisation of a raw conv output as an Act: InstanceNorm (bn None) or BatchNorm2d (train: batch
    statistics + running-stat update; eval: the running statistics)."""
    if bn is None:
        return ops.norm_stats(r, 0)
    if G.training:
        return ops.norm_stats(r, 1, gamma=bn.weight, beta=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var,
                              nbt=bn.num_batches_tracked)
    n = r.shape[0]
    sc = bn.weight / torch.sqrt(bn.running_var + 1e-5)     # [C] vectors: plumbing, not arithmetic on activations
    sh = bn.bias - bn.running_mean * sc
    return Act(r, sc.repeat(n).contiguous(), sh.repeat(n).contiguous())


def _g_norm_bwd(buf, a, bn):
    if bn is None:
        ops.norm_bwd(buf, a, 0)
    else:
        ops.norm_bwd(buf, a, 1, gamma=bn.weight, dgamma=bn.weight.grad, dbeta=bn.bias.grad)


def _through_norm_relu(g_act, a, bn):
    """gradient w.r.t. relu(norm(r)) -> gradient w.r.t. the raw conv output r (in a fresh buffer)"""
    buf = torch.empty_like(a.data)
    ops.act_bwd(g_act, a, RELU, buf)
    _g_norm_bwd(buf, a, bn)
    return buf


def _into_producer(d, inp, inp_act, bn_of):
    """gradient w.r.t. a layer's input as loaded -> w.r.t. what the layer below produced: through relu(norm(.)) where a ReLU was pending (bn_of: _bn_map)"""
    return _through_norm_relu(d, inp, bn_of.get(id(inp))) if inp_act == RELU else d


def _mask_mul(x, keep2):
    """x * keep2 in a fresh buffer (Dropout and its backward: the same keep * 2 map)"""
    v = lambda t: t.view(-1, 1, t.shape[2], t.shape[3])
    return ops.mask_mul(v(x), v(keep2)).view(x.shape)


class _Flow:
    """what a segment's forward threads through its layers: cur, the activation (an Act whose `pending` activation the consumer applies on load, or an
    identity tensor; None in front of the network input, whose `srcs` are concatenated on store), G for the train / eval mode, the unused Dropout masks"""
    __slots__ = ("G", "cur", "pending", "srcs", "masks")


class _Step:
    """One record per layer of a segment, next to its pair: _<kind>_forward(f, e, *modules) takes the _Flow and the layout entry, returns the record;
    _<kind>_backward(st, g, sq, bn_of) takes the gradient w.r.t. the layer's output (the raw conv output where the kind ends in a norm), writes the
    parameters' .grad through the side queue and returns the gradient w.r.t. what the layer below produced.  `wide` / `wino`: the kernel routes the
    forward chose; the backward reads them."""
    __slots__ = ()
    out = bn = None     # kinds that end in a norm: the normalised output (Act) and its BatchNorm module (None: InstanceNorm)

    def weights(self):      # the convolution weights this step owns
        return [self.conv.weight] if hasattr(self, "conv") else []


def _pad3_conv7(conv, f):
    """ReflectionPad2d(3) + 7x7 convolution (4x4 tap blocks) -> (padded operand, the Act it was padded from | None, raw output)"""
    if f.cur is None:    # network input: concat the sources while padding
        n, _, h, w = f.srcs[0].data.shape
        p = _empty(n, sum(s.data.shape[1] for s in f.srcs), h + 6, w + 6, f.srcs[0].data.device)
        c0 = 0
        for s in f.srcs:
            c = s.data.shape[1]
            ops.pad_affine(s, (3, 3, 3, 3), 1, out=p[:, c0:c0 + c], out_nstride=p.stride(0))
            c0 += c
        src = None
    else:
        p = ops.pad_affine(f.cur, (3, 3, 3, 3), 1, act=f.pending)
        src = f.cur if isinstance(f.cur, Act) else None
    r = _empty(p.shape[0], conv.weight.shape[0], p.shape[2] - 6, p.shape[3] - 6, p.device)
    ops.convk(p, conv.weight, r, bias=conv.bias, pad=0)
    return p, src, r


class Conv7Ctx(_Step):
    """ReflectionPad2d(3) + Conv2d(7) + norm + relu (the ReLU rides on `out` as the pending activation)"""
    __slots__ = ("conv", "p", "src", "out", "bn")


def _conv7_forward(f, e, conv, bn):
    st = Conv7Ctx()
    st.conv, st.bn = conv, bn
    st.p, st.src, r = _pad3_conv7(conv, f)
    st.out = f.cur = _g_norm(f.G, r, bn)
    f.pending = RELU
    return st


def _conv7_backward(st, g, sq, bn_of):
    sq.run(lambda: ops.wgradk(g, st.p, st.conv.weight.grad, pad=0), g)  # network input: no gradient needed below
    return g


class Conv7OutCtx(_Step):
    """the final ReflectionPad2d(3) + Conv2d(7) + tanh; src: the Act relu(norm(r_prev)) the operand p was padded from"""
    __slots__ = ("conv", "p", "src")


def _conv7_out_forward(f, e, conv, _):
    st = Conv7OutCtx()
    st.conv = conv
    st.p, st.src, r = _pad3_conv7(conv, f)
    f.cur = ops.pad_affine(r, (0, 0, 0, 0), 0, act=TANH)
    return st


def _conv7_out_backward(st, g, sq, bn_of):
    conv, p = st.conv, st.p
    sq.run(lambda: (ops.wgradk(g, p, conv.weight.grad, pad=0), ops.channel_sum(g, conv.bias.grad)), g)
    dp = ops.convk_bwd_data(g, conv.weight, torch.empty_like(p), pad=0)
    da = ops.pad_bwd(dp, (3, 3, 3, 3), 1, _empty(p.shape[0], p.shape[1], p.shape[2] - 6, p.shape[3] - 6, g.device))
    return _through_norm_relu(da, st.src, bn_of.get(id(st.src)))


class Conv3Ctx(_Step):
    """Conv2d(3, pad 1, stride 1 | 2) + norm + relu.  wide: on the GEMM-class kernels, whose operand xp = act(inp) was materialised with
    its zero padding once; else on the 4x4 family, which applies inp_act on load"""
    __slots__ = ("conv", "inp", "inp_act", "out", "bn", "stride", "wide", "xp")


def _conv3_forward(f, e, conv, bn):
    st = Conv3Ctx()
    st.conv, st.bn, st.inp, st.inp_act, st.stride, st.xp = conv, bn, f.cur, f.pending, e["stride"], None
    stride, x = st.stride, _as_act(f.cur).data
    n, _, ih, iw = x.shape
    co, ci = conv.weight.shape[:2]
    r = _empty(n, co, (ih - 1) // stride + 1, (iw - 1) // stride + 1, x.device)
    if stride == 2 and (ih % 2 or iw % 2):
        raise ValueError("stride-2 3x3 convolutions need even sizes, got %dx%d" % (ih, iw))
    st.wide = ops.conv3_wide(conv.weight)
    if st.wide:
        st.xp = ops.pad_affine(st.inp, (1, 1, 1, 1), 0, act=st.inp_act)
        wt = ops.w3x3_pack(conv.weight, "conv_fwd")
        (ops.conv3x3_wide if stride == 1 else ops.conv3x3s2_wide)(st.xp, wt, conv.bias, r)
    elif stride == 1:
        ops.convk(st.inp, conv.weight, r, bias=conv.bias, pad=1, act_in=st.inp_act)
    else:
        ops.conv4x4(st.inp, ops.tap_embed3(conv.weight), ci * 16, 16, co, r, bias=conv.bias, stride=2, pad=1, act_in=st.inp_act)
    st.out = f.cur = _g_norm(f.G, r, bn)
    f.pending = RELU
    return st


def _conv3_backward(st, g, sq, bn_of):
    conv, inp, inp_act, stride, xp = st.conv, st.inp, st.inp_act, st.stride, st.xp
    hi_act = _as_act(inp)
    din = torch.empty_like(hi_act.data)
    if st.wide:
        sq.run(lambda: ops.wgrad3x3_wide(g, xp, conv.weight.grad, stride=stride), g)
        if stride == 1:
            ops.pad_bwd(ops.conv3_valid_adjoint(g, conv.weight, torch.empty_like(xp)), (1, 1, 1, 1), 0, din)
        else:
            ops.tconv3x3s2_wide(ops.pad_affine(g, (0, 1, 0, 1), 0), ops.w3x3_pack(conv.weight, "conv_s2_adj"), None, din)
    elif stride == 1:
        sq.run(lambda: ops.wgradk(g, hi_act, conv.weight.grad, pad=1, act_hi=inp_act), g)
        ops.convk_bwd_data(g, conv.weight, din, pad=1)
    else:
        ci = conv.weight.shape[1]
        dw4 = ops._w4_scratch(conv.weight.grad, 3, "grad")[0]
        sq.run(lambda: (ops.wgrad4x4(g, hi_act, dw4, stride=2, pad=1, act_hi=inp_act, defer=False), ops.tap_extract(dw4, 3, 0, 0, conv.weight.grad)), g)
        ops.conv4x4(g, ops.tap_embed3(conv.weight), 16, ci * 16, ci, din, stride=2, pad=1, transposed=True)
    return _into_producer(din, inp, inp_act, bn_of)


class ConvT3Ctx(_Step):
    """ConvTranspose2d(3, stride 2, pad 1, output_padding 1) + norm + relu.  wide: on the GEMM-class kernels, z = the materialised act(inp)"""
    __slots__ = ("conv", "inp", "inp_act", "out", "bn", "wide", "z")


def _convT3_forward(f, e, conv, bn):
    st = ConvT3Ctx()
    st.conv, st.bn, st.inp, st.inp_act, st.z = conv, bn, f.cur, f.pending, None
    inp, inp_act, x = st.inp, st.inp_act, _as_act(f.cur).data
    n, _, ih, iw = x.shape
    co = conv.weight.shape[1]
    r = _empty(n, co, 2 * ih, 2 * iw, x.device)
    st.wide = ops.conv3_wide(conv.weight)
    if st.wide:
        st.z = ops.pad_affine(inp, (0, 0, 0, 0), 0, act=inp_act) if (inp_act or isinstance(inp, Act)) else inp
        ops.tconv3x3s2_wide(ops.pad_affine(st.z, (0, 1, 0, 1), 0), ops.w3x3_pack(conv.weight, "convT_fwd"), conv.bias, r)
    else:
        ops.conv4x4(inp, ops.tap_embed3(conv.weight), 16, co * 16, co, r, bias=conv.bias, stride=2, pad=1, transposed=True, act_in=inp_act)
    st.out = f.cur = _g_norm(f.G, r, bn)
    f.pending = RELU
    return st


def _convT3_backward(st, g, sq, bn_of):
    conv, inp, inp_act, z = st.conv, st.inp, st.inp_act, st.z
    ci, co = conv.weight.shape[:2]
    lo_act = _as_act(inp)
    din = torch.empty_like(lo_act.data)
    if st.wide:
        gp = ops.pad_affine(g, (1, 1, 1, 1), 0)
        sq.run(lambda: ops.wgrad3x3_wide(z, gp, conv.weight.grad, stride=2), gp)
        ops.conv3x3s2_wide(gp, ops.w3x3_pack(conv.weight, "convT_adj"), None, din)
    else:
        dw4 = ops._w4_scratch(conv.weight.grad, 3, "grad")[0]
        sq.run(lambda: (ops.wgrad4x4(lo_act, g, dw4, stride=2, pad=1, act_lo=inp_act, defer=False), ops.tap_extract(dw4, 3, 0, 0, conv.weight.grad)), g)
        ops.conv4x4(g, ops.tap_embed3(conv.weight), co * 16, 16, ci, din, stride=2, pad=1)
    return _into_producer(din, inp, inp_act, bn_of)


class DownCtx(_Step):
    """anti-aliased Downsample of inp = an Act, relu(norm(r)) on load"""
    __slots__ = ("inp",)


def _down_forward(f, e, *_):
    st = DownCtx()
    st.inp = f.cur
    f.cur, f.pending = ops.blur_down(f.cur, act=f.pending), 0
    return st


def _down_backward(st, g, sq, bn_of):
    da = torch.empty_like(st.inp.data)
    ops.blur_down_bwd(g, da)
    return _through_norm_relu(da, st.inp, bn_of.get(id(st.inp)))


class UpCtx(_Step):
    """anti-aliased Upsample of act(inp)"""
    __slots__ = ("inp", "inp_act")


def _up_forward(f, e, *_):
    st = UpCtx()
    st.inp, st.inp_act = f.cur, f.pending
    f.cur, f.pending = ops.blur_up(f.cur, act=f.pending), 0
    return st


def _up_backward(st, g, sq, bn_of):
    da = torch.empty_like(_as_act(st.inp).data)
    ops.blur_up_bwd(g, da)
    return _into_producer(da, st.inp, st.inp_act, bn_of)


class BlockCtx(_Step):
    """ResnetBlock, x + norm(conv(reflpad(relu(norm(conv(reflpad(x))))))): convolutions ca / cb with norms na / nb, padded operands
    p1 / p2, normalised outputs a1 / a2.  src, src_act: what the identity input was materialised from (the first block behind a strided
    conv), else None.  keep2: the Dropout map keep * 2, or None.  wide; wino / wino_adj: the forwards / the input adjoints take Winograd"""
    __slots__ = ("ca", "cb", "na", "nb", "p1", "a1", "p2", "a2", "src", "src_act", "keep2", "wide", "wino", "wino_adj")

    def weights(self):
        return [self.ca.weight, self.cb.weight]


def _block_forward(f, e, ca, na, cb, nb):
    st = BlockCtx()
    st.ca, st.na, st.cb, st.nb = ca, na, cb, nb
    st.src = st.src_act = st.keep2 = None
    if f.pending or isinstance(f.cur, Act):   # first block after a strided conv: materialise relu(norm(r))
        st.src, st.src_act = f.cur, f.pending
        f.cur, f.pending = ops.pad_affine(f.cur, (0, 0, 0, 0), 0, act=f.pending), 0
    xb = f.cur           # identity tensor
    n, c, h, w = xb.shape
    dev = xb.device
    st.wide = ops.conv3_wide(ca.weight)     # (both convolutions of a block are c -> c: one route, one pair of Winograd answers)
    st.wino = st.wide and ops.conv3x3_wino_ok(n, c, c, h, w)
    st.wino_adj = st.wide and ops.conv3x3_wino_ok(n, c, c, h + 2, w + 2)     # on the gradient zero-padded by 2
    st.p1 = ops.pad_affine(xb, (1, 1, 1, 1), 1)
    r1 = ops.conv3_valid(st.p1, ca.weight, ca.bias, _empty(n, c, h, w, dev), wino=st.wino)
    st.a1 = _g_norm(f.G, r1, na)
    if getattr(f.G, "use_dropout", False) and f.G.training:
        # Dropout(0.5) between the ReLU and the second reflection pad (networks.py:1305-1306): relu(norm(r1)) is materialised,
        # multiplied by keep * 2, and padded as a plain tensor; the backward multiplies by the same map
        k = f.masks.pop(0) if f.masks else torch.bernoulli(torch.full(r1.shape, 0.5, device=dev))
        st.keep2 = (k.to(device=dev, dtype=torch.float32) * 2.0).contiguous()
        st.p2 = ops.pad_affine(_mask_mul(ops.pad_affine(st.a1, (0, 0, 0, 0), 0, act=RELU), st.keep2), (1, 1, 1, 1), 1)
    else:
        st.p2 = ops.pad_affine(st.a1, (1, 1, 1, 1), 1, act=RELU)
    r2 = ops.conv3_valid(st.p2, cb.weight, cb.bias, _empty(n, c, h, w, dev), wino=st.wino)
    st.a2 = _g_norm(f.G, r2, nb)
    f.cur = ops.pad_affine(st.a2, (0, 0, 0, 0), 0, res=xb)
    return st


def _block_backward(st, g, sq, bn_of):
    g2 = g.clone()
    _g_norm_bwd(g2, st.a2, st.nb)
    sq.run(lambda: ops.conv3_valid_wgrad(g2, st.p2, st.cb.weight.grad), g2)
    dp2 = ops.conv3_valid_adjoint(g2, st.cb.weight, torch.empty_like(st.p2), wino=st.wino_adj)
    da1 = ops.pad_bwd(dp2, (1, 1, 1, 1), 1, torch.empty_like(st.a1.data))
    if st.keep2 is not None:      # Dropout backward
        da1 = _mask_mul(da1, st.keep2)
    g1 = _through_norm_relu(da1, st.a1, st.na)
    sq.run(lambda: ops.conv3_valid_wgrad(g1, st.p1, st.ca.weight.grad), g1)
    dp1 = ops.conv3_valid_adjoint(g1, st.ca.weight, torch.empty_like(st.p1), wino=st.wino_adj)
    ops.pad_bwd(dp1, (1, 1, 1, 1), 1, g, accumulate=True)   # + the skip path, into the incoming gradient
    return _into_producer(g, st.src, st.src_act, bn_of)


_FORWARD_OF = {"conv7": _conv7_forward, "conv7_out": _conv7_out_forward, "conv3": _conv3_forward, "convT3": _convT3_forward,
               "down": _down_forward, "up": _up_forward, "block": _block_forward}      # layout kind -> forward, record class -> backward
_BACKWARD_OF = {Conv7Ctx: _conv7_backward, Conv7OutCtx: _conv7_out_backward, Conv3Ctx: _conv3_backward, ConvT3Ctx: _convT3_backward,
                DownCtx: _down_backward, UpCtx: _up_backward, BlockCtx: _block_backward}


def _seq_units(lay):
    """a layout (the reference's nn.Sequential, entry by entry) as the units the engine runs: (kind, the unit's own entry, index of its
    norm module | None).  The pad in front of a 7x7 convolution and the norm / relu / tanh entries behind a convolution are consumed here."""
    i = 0
    while i < len(lay):
        e = lay[i]
        kind = e["kind"]
        if kind == "pad":      # ReflectionPad2d(3) + conv7 + (norm + relu | tanh)
            i, e = i + 1, lay[i + 1]
            kind = "conv7" if lay[i + 1]["kind"] == "norm" else "conv7_out"
        if kind not in _FORWARD_OF:
            raise RuntimeError("unexpected layout entry %r" % (e,))
        normed = kind in ("conv7", "conv3", "convT3")
        yield kind, e, lay[i + 1]["idx"] if normed else None
        i += 3 if normed else 2 if kind == "conv7_out" else 1


def _seq_forward(G, seq, srcs, cur, pending, dropout_masks=None):
    """Run one nn.Sequential-like segment (`seq.layout` over `seq.mod` / `seq.block_mods`).  srcs: the network input(s) (Acts, concatenated on
    store into the first padded tensor) when the segment starts at the input (cur None); otherwise cur is the incoming activation (Act with `pending`
    activation, or an identity tensor).  Returns (cur, pending, steps); steps: one record per layer.  G supplies the train / eval mode."""
    f = _Flow()
    f.G, f.cur, f.pending, f.srcs, f.masks = G, cur, pending, srcs, dropout_masks
    steps = []
    for kind, e, norm_idx in _seq_units(seq.layout):
        mods = seq.block_mods(e["idx"]) if kind == "block" else (seq.mod(e["idx"]), None if norm_idx is None else seq.mod(norm_idx))
        steps.append(_FORWARD_OF[kind](f, e, *mods))
    return f.cur, f.pending, steps


def _seq_backward(steps, g, sq, bn_of, start=0, stop=None):
    """backward of one segment: g = gradient w.r.t. its output (the pre-tanh output for a final conv7, else w.r.t. the raw output of its last conv /
    the identity output of its last block).  Writes the parameters' .grad (overwrite; through the side queue sq) and returns the gradient flowing
    into the layer below the segment.  start / stop: only steps[start:stop] (the stages of resnet_backward_stage)."""
    for st in reversed(steps[start:stop]):
        g = _BACKWARD_OF[type(st)](st, g, sq, bn_of)
    return g


def _bn_map(*step_lists):
    """Act -> the BatchNorm module that produced its affine (None: InstanceNorm)"""
    return {id(st.out): st.bn for steps in step_lists for st in steps if st.out is not None}


def resnet_forward(G, x, keep=True, dropout_masks=None):
    """x: tensor / Act, or a pair (x0, x1) concatenated on store into the first padded tensor.
    Returns (g_out [N,output_nc,H,W] post-tanh, ctx).  Every 3x3 / 7x7 conv runs as 4x4 tap blocks
    (ops.convk) or, for wide layers, on the GEMM-class kernels; normalisation is a statistics pass only and is
    applied on load by the consumer."""
    if getattr(G, "is_local_enhancer", False):
        return local_enhancer_forward(G, x, keep)
    srcs = [_as_act(t) for t in (x if isinstance(x, (tuple, list)) else (x,))]
    cur, _, steps = _seq_forward(G, G, srcs, None, 0, dropout_masks=list(dropout_masks) if dropout_masks else None)
    return cur, (ResnetCtx(steps, cur) if keep else None)


class LocalLevelCtx:
    """one enhancer of a LocalEnhancer: the steps of model<n>_1 (down) and model<n>_2 (up), which runs on relu(norm(a)) + relu(norm(b)) --
    a: the output of the level below, b: the output of `down`"""
    __slots__ = ("down", "up", "a", "b")


def local_enhancer_forward(G, x, keep=True):
    """pix2pixHD LocalEnhancer.forward (networks.py:1933-1949): the global trunk on the input average-pooled L = n_local_enhancers times,
    then enhancer n = 1 .. L: its downsampling branch on pyramid level L - n, plus the output below, through its upsampling branch"""
    x = _as_act(x)
    L = G.n_local_enhancers
    pyr = [x]
    for _ in range(L):
        pyr.append(Act(ops.avgpool(pyr[-1].data)))
    a, pa, steps_g = _seq_forward(G, G.seq_global, [pyr[-1]], None, 0)
    levels = []
    for n in range(1, L + 1):
        lv = LocalLevelCtx()
        lv.a = a
        lv.b, pb, lv.down = _seq_forward(G, G.seq_down[n - 1], [pyr[L - n]], None, 0)
        bm = ops.pad_affine(lv.b, (0, 0, 0, 0), 0, act=pb)
        s = ops.pad_affine(a, (0, 0, 0, 0), 0, act=pa, res=bm)
        a, pa, lv.up = _seq_forward(G, G.seq_up[n - 1], None, s, 0)
        levels.append(lv)
    return a, (ResnetCtx((steps_g, levels), a) if keep else None)


def resnet_backward(G, ctx, d_raw):
    """d_raw: gradient w.r.t. the pre-tanh output.  Writes every parameter's .grad (overwrite).
    Biases that feed a normalisation have identically zero gradient and are never written."""
    sq = SideQueue()     # weight / bias gradients: off the critical path of the backward-data chain
    if getattr(G, "is_local_enhancer", False):
        steps_g, levels = ctx.steps
        bn_of = _bn_map(steps_g, *[lv.down for lv in levels], *[lv.up for lv in levels])
        g = d_raw
        for lv in reversed(levels):
            g_s = _seq_backward(lv.up, g, sq, bn_of)         # gradient w.r.t. relu(norm(a)) + relu(norm(b))
            _seq_backward(lv.down, _through_norm_relu(g_s, lv.b, bn_of.get(id(lv.b))), sq, bn_of)
            g = _through_norm_relu(g_s, lv.a, bn_of.get(id(lv.a)))   # ... w.r.t. the raw output of the level below
        _seq_backward(steps_g, g, sq, bn_of)
    else:
        _seq_backward(ctx.steps, d_raw, sq, _bn_map(ctx.steps))
    sq.join()


def resnet_stage_bounds(ctx, cut_params):
    """Step indices at which a backward pass is cut so that, once stage j (steps[b[j]:b[j+1]], run from the last stage to the first) has
    finished, every parameter of gradient bucket j has its final gradient (vts/optim.py:FlatParams.chunk: every bucket but the first
    starts at a convolution weight).  A bucket that starts inside a two-convolution block is complete after the stage that holds the
    block (the block's first convolution then belongs to the next bucket down and is simply early).  Returns [0, s_1, .., s_K-1, len(steps)]."""
    steps = ctx.steps
    where = {w.data_ptr(): i for i, st in enumerate(steps) for w in st.weights()}
    bounds = [0]
    for p in cut_params:
        i = where.get(p.data_ptr())
        if i is None:
            raise RuntimeError("a gradient bucket does not start at a layer of this generator's backward")
        bounds.append(max(i, bounds[-1]))
    bounds.append(len(steps))
    return bounds


def resnet_backward_stage(G, ctx, g, lo, hi):
    """steps[lo:hi] of resnet_backward (single generator), weight gradients joined: on return every parameter of these steps has its
    final .grad, and the returned tensor is the gradient flowing into steps[:lo].  Chaining the stages from the last to the first equals
    resnet_backward; a data-parallel step starts the all-reduce of a stage's gradient bucket behind it (models/pix2pixHD_model.py)."""
    if getattr(G, "is_local_enhancer", False):
        raise NotImplementedError("staged backward of the local enhancer")
    sq = SideQueue()
    g = _seq_backward(ctx.steps, g, sq, _bn_map(ctx.steps), lo, hi)
    sq.join()
    return g


def add_grad_list(lst, idx, shape, dev):
    if lst[idx] is not None:
        return lst[idx], True
    lst[idx] = torch.empty(shape, dtype=torch.float32, device=dev)
    return lst[idx], False


# =====================================================================================
# multiscale discriminator
# =====================================================================================

class MsdCtx:
    __slots__ = ("scales",)


def _pool_act(a):
    return None if a is None else Act(ops.avgpool(a.data))


# The scales of a multiscale discriminator are independent chains of small kernels (the D2 passes over 32x32
# tactile patches never fill 256 CUs): they run concurrently on side HIP streams, forked from and joined back
# into the launch stream (so the schedule is still a DAG that torch.cuda.CUDAGraph captures as such).
PARALLEL_SCALES = tune.get("VTS_PARALLEL_SCALES", "1") != "0"
SIDE_QUEUES = 2     # round 4: one -> two 5.65 -> 5.59 ms (three: 5.61); round 6, chained schedule: one / three + 0.04 / + 0.05 ms


class SideQueue:
    """Work that nothing on the launch stream waits for until the end of a phase -- the weight / bias gradients of a
    backward pass (28 % of the step's kernel time, all of it off the critical path of the backward-data chain) --
    is enqueued on side streams: `run` forks at the current point of the launch stream (the operands are ready
    there) and keeps the operand tensors alive; `join` makes the launch stream wait once, at the end.  Round 4: the items alternate
    between TWO streams (the generator backward's trunk / encoder phase has the launch chain and nothing else on the other queues, and
    its weight gradients take longer than its backward-data chain: the join used to wait for them)."""
    LANE = 7

    def __init__(self):
        # items alternate between two lanes of fixed number, reserved: no other fork may grow into them
        self.fork = lanes.Fork(reserve=[SideQueue.LANE - k for k in range(SIDE_QUEUES)])
        self.turn = 0
        self.keep = []
        self.on = PARALLEL_SCALES

    def run(self, fn, *tensors):
        if not self.on:
            return fn()
        k = self.turn % len(self.fork.lanes)
        self.turn += 1
        self.fork.fork(k)
        try:
            with self.fork.on(k):
                fn()
        except BaseException:
            ops.wgrad_discard()
            self.fork.join()
            raise
        self.keep.extend(tensors)

    def join(self):
        if self.on:
            for k in range(len(self.fork.lanes)):
                with self.fork.on(k):
                    ops.wgrad_flush()       # this queue's deferred weight-gradient reduction, on its own stream
            self.fork.join()
        self.keep = []


def _run_lanes(n_lanes, body):
    """body(lane) for lane in range(n_lanes): lane 0 on the current stream, the others on side streams forked
    from it and joined back into it (a flat fork: nested forks made hipStreamEndCapture crash), each with its own
    scratch buffer.  The discriminator scales -- and the D1 / D2 updates of one step -- are independent chains
    of mostly small kernels; run side by side they fill the CUs that one chain leaves idle, and the schedule
    is still a DAG that torch.cuda.CUDAGraph captures as such."""
    if n_lanes == 1 or not PARALLEL_SCALES:
        for lane in range(n_lanes):
            body(lane)
        return
    # A call made from the launch-stream lane of an enclosing call (the generator forward's two decoder lanes inside the lane set of
    # _msd_multi(extra_main=True)) takes the lanes BEHIND the enclosing call's: the fork holds them while body(0) runs.  (From a SIDE lane
    # a fork is still forbidden: hipStreamEndCapture does not survive it.)
    with lanes.Fork(n_lanes - 1) as f:      # a lane body raised: no stale partial jobs for the next backward, no dangling fork
        f.fork()
        for lane in range(1, n_lanes):
            with f.on(lane - 1):
                body(lane)
                ops.wgrad_flush()           # deferred weight-gradient reductions of this lane, on its own stream
        f.hold()
        try:
            body(0)
        finally:
            f.release()
        ops.wgrad_flush()


def fork_lane(fn):
    """fn() on a side stream forked from the current stream, with its own scratch lane; returns a handle for join_lane.  Until the
    join, lane calls made on the launch stream (_run_lanes, msd_chain) take the side streams BEHIND this one -- the lane may stay open
    across several of them (the D2 chain of the training step runs beside the D1 chain AND the generator's backward).  fn must not
    fork lanes itself (no fork from a side stream: hipStreamEndCapture does not survive one).  Serial schedule: fn() runs inline."""
    if not PARALLEL_SCALES:
        fn()
        return None
    f = lanes.Fork(1)
    f.fork()
    f.hold()
    try:
        with f.on(0):
            fn()
    except BaseException:
        f.close()
        raise
    return f


def join_lane(handle):
    """the current stream waits for the lane fork_lane opened; its side stream is free for other lanes again"""
    if handle is not None:
        handle.close(torch.cuda.current_stream())


def _pyramid(D, in0, in1):
    in0 = _as_act(in0)
    in1 = _as_act(in1) if in1 is not None else None
    pyr = [(in0, in1)]
    for s in range(1, D.num_D):
        pyr.append((_pool_act(pyr[-1][0]), _pool_act(pyr[-1][1])))
    return pyr


FLAT_D = tune.get("VTS_FLAT_D", "1") != "0"
FLAT_MIN_C = 64   # small maps: channels from which the flattened GEMM-class kernel takes over (32, the D2 patch layers too: no gain, 10.7 vs 10.6 ms)


WIDE_MIN_CI = int(tune.get("VTS_WIDE_MIN_CI", "64"))   # round 3 A/B: 32 / 64 (D1 layer 3 on the GEMM-class kernels) costs + 1.0 - 1.4 ms per step
WIDE_MIN_CO = int(tune.get("VTS_WIDE_MIN_CO", "128"))


def _flat4(conv, j, h, w, oh, ow, st):
    """whether this PatchGAN layer takes the GEMM-class route with 16-tap packed weights (vts_conv4x4_wide: flattened-batch kernel
    for maps of <= 128 pixels, tiled kernel above): wide layers only; Cout = 1 heads only on small maps"""
    co, ci = conv.weight.shape[0], conv.weight.shape[1]
    if not FLAT_D or j == 0 or ci < min(FLAT_MIN_C, WIDE_MIN_CI):
        return False
    small = ops.conv4x4_flat_ok(oh, ow, st * (oh - 1) + 4, st * (ow - 1) + 4)
    if small:
        return co >= FLAT_MIN_C or ci >= 256
    if ci < WIDE_MIN_CI:                     # full-size maps of the reference's own ndf = 8 discriminators stay on the 4x4 kernels
        return False
    return co >= WIDE_MIN_CO and co % 4 == 0 and ci % 4 == 0


def _packed4(conv, mode, cache):
    """16-tap packing of a PatchGAN layer's weight, once per discriminator invocation: the passes of one scale run back to back in
    one lane and the weights only change between invocations (Adam), so `cache` (created per msd_multi / msd_forward call) is safe"""
    if cache is None:
        return ops.w4x4_pack(conv.weight, mode)
    key = (id(conv), mode)
    buf = cache.get(key)
    if buf is None:
        buf = cache[key] = ops.w4x4_pack(conv.weight, mode)
    return buf


def _msd_scale_forward(D, s, a0, a1, update_stats, cache=None, groups=None, stat_rec=None, ext=None, skip_head=False):
    """one PatchGAN of the pyramid: returns the list of layer outputs (Act), the last one is the prediction.
    groups: sample indices where the passes batched into this call start (BatchNorm statistics per pass: ops.norm_stats);
    stat_rec: dict filled with {bn layer: (mean, unbiased var)} of this call; ext: (such a dict, after) whose running-statistics
    updates are spliced in after pass `after`."""
    n, dev = a0.data.shape[0], a0.data.device
    layer = getattr(D, "layer%d" % (D.num_D - 1 - s))
    acts = []
    cur0, cur1 = a0, a1
    h, w = cur0.data.shape[2], cur0.data.shape[3]
    for j, ci in enumerate(D.CONV_IDX):
        if skip_head and j == len(D.CONV_IDX) - 1:
            break      # a pass that only advances BatchNorm statistics at this scale: the prediction head has no normalisation behind it
        conv = getattr(layer, str(ci))
        st = D.STRIDE[ci]
        cout, cin = conv.weight.shape[0], conv.weight.shape[1]
        oh, ow = (h + 4 - 4) // st + 1, (w + 4 - 4) // st + 1
        out = _empty(n, cout, oh, ow, dev)
        if _flat4(conv, j, h, w, oh, ow, st):
            ph, pw = st * (oh - 1) + 4, st * (ow - 1) + 4
            p = ops.pad_affine(cur0, (2, ph - h - 2, 2, pw - w - 2), 0, act=LRELU)
            cur0.padded = p
            ops.conv4x4_wide(p, _packed4(conv, "conv_fwd", cache), conv.bias, out, stride=st)
            flat = True
        else:
            flat = False
        bnkw = None
        if ci in D.BN_IDX:
            bn = getattr(layer, str(D.BN_IDX[ci]))
            stat_out = None
            if stat_rec is not None:
                stat_out = stat_rec[ci] = (torch.empty(cout, dtype=torch.float32, device=dev), torch.empty(cout, dtype=torch.float32, device=dev))
            bnkw = dict(gamma=bn.weight, beta=bn.bias, running_mean=bn.running_mean if update_stats else None,
                        running_var=bn.running_var if update_stats else None,
                        nbt=bn.num_batches_tracked if update_stats else None, groups=groups, stat_out=stat_out,
                        ext=(ext[0][ci][0], ext[0][ci][1], ext[1]) if ext is not None else None)
        if not flat:     # Conv2d -> BatchNorm2d: the statistics come out of the convolution's epilogue where the tiled kernel runs
            a = ops.conv4x4(cur0, conv.weight, cin * 16, 16, cout, out, in1=cur1, bias=conv.bias, stride=st, pad=2,
                            act_in=LRELU if j else 0, batch_norm=bnkw)
            if bnkw is None:
                a = Act(out)
        elif bnkw is not None:
            a = ops.norm_stats(out, 1, **bnkw)
        else:
            a = Act(out)
        acts.append(a)
        cur0, cur1 = a, None
        h, w = oh, ow
    return acts


MSD_C = tune.get("VTS_MSD_C", "1") != "0"     # forward-only discriminator passes through the network-level C entry (0: the Python schedule)


def patchgan_desc(D, s, a0, a1, update_stats=True, stat_rec=None, run_head=True, pred=None):
    """vts_patchgan_desc of scale s of a multiscale discriminator (include/vts.h): weights from the module in the reference's state-dict
    layout, BatchNorm running buffers when update_stats, `stat_rec` {conv index: (mean, uvar)} filled with recording buffers"""
    layer = getattr(D, "layer%d" % (D.num_D - 1 - s))
    d = L.PatchganDesc()
    d.in0, d.in1 = ops._op(a0), ops._op(a1)
    x = a0.data if isinstance(a0, Act) else a0
    d.N, d.H, d.W = x.shape[0], x.shape[2], x.shape[3]
    d.n_convs = len(D.CONV_IDX)
    d.eps, d.momentum = 1e-5, 0.1
    keep = []
    for j, ci in enumerate(D.CONV_IDX):
        conv = getattr(layer, str(ci))
        d.cout[j], d.stride[j] = conv.weight.shape[0], D.STRIDE[ci]
        d.w[j], d.b[j] = conv.weight.data_ptr(), L.ptr(conv.bias)
        if ci in D.BN_IDX:
            bn = getattr(layer, str(D.BN_IDX[ci]))
            d.gamma[j], d.beta[j] = bn.weight.data_ptr(), bn.bias.data_ptr()
            if update_stats:
                d.running_mean[j], d.running_var[j] = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
                d.num_batches_tracked[j] = bn.num_batches_tracked.data_ptr()
            if stat_rec is not None:
                so = stat_rec[ci] = (torch.empty(conv.weight.shape[0], dtype=torch.float32, device=x.device),
                                     torch.empty(conv.weight.shape[0], dtype=torch.float32, device=x.device))
                d.stat_mean_out[j], d.stat_uvar_out[j] = so[0].data_ptr(), so[1].data_ptr()
    d.run_head = int(bool(run_head))
    if run_head:
        h, w = d.H, d.W
        for ci in D.CONV_IDX:
            h, w = h // D.STRIDE[ci] + 1, w // D.STRIDE[ci] + 1
        if pred is None:
            pred = _empty(d.N, 1, h, w, x.device)
        d.pred = pred.data_ptr()
    return d, pred, keep


def patchgan_c_ok(D, h, w):
    """the C entry runs every layer on the 4x4 convolution family: not where the Python schedule sends a wide layer to the GEMM-class
    kernels (_flat4: pix2pixHD's ndf = 64, depth >= 4 at ndf = 8), and PatchGAN depths within the descriptor; h, w: the input map"""
    if not MSD_C or len(D.CONV_IDX) > L.PATCHGAN_MAX_CONVS:
        return False
    layer = getattr(D, "layer0")
    for j, ci in enumerate(D.CONV_IDX):
        conv = getattr(layer, str(ci))
        st = D.STRIDE[ci]
        oh, ow = h // st + 1, w // st + 1
        if _flat4(conv, j, h, w, oh, ow, st) or conv.weight.shape[0] > 80:
            return False
        h, w = oh, ow
    return True


def patchgan_forward_c(D, s, a0, a1, update_stats=True, stat_rec=None, run_head=True):
    """scale s of a multiscale discriminator, training-mode forward, nothing kept: ONE call of vts_patchgan_forward (the path of the
    product's forward-only passes; bit-identical to _msd_scale_forward: tests/test_network_abi_gpu.py).  Returns the prediction map or None."""
    d, pred, _ = patchgan_desc(D, s, a0, a1, update_stats, stat_rec, run_head)
    lib = L.load()
    need = int(lib.vts_patchgan_forward_ws_floats(C.byref(d)))
    if need < 0:
        raise RuntimeError("vts_patchgan_forward: %s" % lib.vts_last_error().decode())
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=pred.device if pred is not None else (a0.data if isinstance(a0, Act) else a0).device)
    L.check(lib.vts_patchgan_forward(C.byref(d), ws.data_ptr(), ws.numel(), L.stream()), "vts_patchgan_forward")
    return pred


def _msd_scale_backward(D, s, a0, a1, acts, g, param_grads, accumulate, want_input_grad, cache=None, groups=None, into=None):
    """backward of one PatchGAN; returns the gradient w.r.t. the second concat source (or None).
    into = (tensor, accumulate?): write / add that gradient straight into the caller's buffer (the full-resolution scale: saves the
    separate add of the merged pyramid gradient)"""
    layer = getattr(D, "layer%d" % (D.num_D - 1 - s))
    for j in range(len(D.CONV_IDX) - 1, -1, -1):
        ci = D.CONV_IDX[j]
        conv = getattr(layer, str(ci))
        st = D.STRIDE[ci]
        cin = conv.weight.shape[1]
        if ci in D.BN_IDX:
            bn = getattr(layer, str(D.BN_IDX[ci]))
            ops.norm_bwd(g, acts[j], 1, gamma=bn.weight, dgamma=bn.weight.grad if param_grads else None,
                         dbeta=bn.bias.grad if param_grads else None, accumulate=accumulate, groups=groups, beta=bn.bias)
        src0, src1 = (a0, a1) if j == 0 else (acts[j - 1], None)
        if param_grads:
            pp = src0.padded if j else None
            if pp is not None and not ops.conv4x4_flat_ok(g.shape[2], g.shape[3], pp.shape[2], pp.shape[3]):
                ops.wgrad4x4_wide(g, pp, conv.weight.grad, stride=st, accumulate=accumulate)     # full-size map: GEMM-class
            else:
                ops.wgrad4x4(Act(g), src0, conv.weight.grad, hi1=src1, act_hi=LRELU if j else 0, stride=st, pad=2,
                             accumulate=accumulate)
            if ci not in D.BN_IDX:   # a conv bias in front of a BatchNorm has an identically zero gradient
                ops.channel_sum(g, conv.bias.grad, accumulate=accumulate)
        if j > 0:
            prev = acts[j - 1]
            tgt = torch.empty_like(prev.data)
            h, w, oh, ow = prev.data.shape[2], prev.data.shape[3], g.shape[2], g.shape[3]
            qh, qw = (oh + 2, ow + 2) if st == 1 else (oh + 1, ow + 1)
            if _flat4(conv, j, h, w, oh, ow, st) and (cin % 4 == 0 or ops.conv4x4_flat_ok(h, w, qh, qw, st == 2)):
                raw = torch.empty_like(prev.data)
                if st == 1:   # adjoint of the stride-1 conv: the same operator on the padded gradient, flipped taps
                    ops.conv4x4_wide(ops.pad_affine(g, (1, 1, 1, 1), 0), _packed4(conv, "conv_adj", cache), None, raw)
                else:
                    ops.conv4x4_wide(ops.pad_affine(g, (0, 1, 0, 1), 0), _packed4(conv, "conv_s2_adj", cache), None, raw,
                                     stride=2, transposed=True)
                ops.act_bwd(raw, prev, LRELU, tgt)
            else:
                ops.conv4x4(Act(g), conv.weight, 16, cin * 16, cin, tgt, stride=st, pad=2, transposed=True, dmask=prev,
                            dmask_act=LRELU, bwd_sums=D.CONV_IDX[j - 1] in D.BN_IDX)
            g = tgt
        elif want_input_grad:      # w.r.t. the second concat source, or the only one (D1 without the sketch: --use_cGAN False)
            src = a1 if a1 is not None else a0
            c0 = a0.data.shape[1] if a1 is not None else 0
            c1 = src.data.shape[1]
            tgt, acc_in = (torch.empty_like(src.data), False) if into is None else into
            ops.conv4x4(Act(g), conv.weight.view(-1)[c0 * 16:], 16, cin * 16, c1, tgt, stride=st, pad=2, transposed=True, accumulate=acc_in)
            return tgt
    return None


def msd_forward_train_c(D, in0, in1=None):
    """the multiscale discriminator's training-mode forward through ONE vts_msd_forward call into a workspace sized for vts_msd_backward
    (include/vts.h: the forward's region is its prefix).  in0 (++ in1): plain tensors.  Returns (preds, ctx) for msd_backward_c.  Not the
    product's path (the training step keeps the Python schedule)."""
    lib = L.load()
    n, _, h, w = in0.shape
    d = L.MsdDesc()
    d.num_D = D.num_D
    preds = []
    hs, ws_ = h, w
    for s in range(D.num_D):
        ph, pw = hs, ws_
        for ci in D.CONV_IDX:
            ph, pw = ph // D.STRIDE[ci] + 1, pw // D.STRIDE[ci] + 1
        pred = _empty(n, 1, ph, pw, in0.device)
        sub, _, _ = patchgan_desc(D, s, in0, in1, pred=pred)      # (scale s's weights; the call fills in the pooled inputs and sizes)
        d.scale[s] = sub
        preds.append(pred)
        hs, ws_ = (hs + 1) // 2, (ws_ + 1) // 2
    need = int(lib.vts_msd_backward_ws_floats(C.byref(d)))
    if need < 0:
        raise RuntimeError("vts_msd_backward_ws_floats: %s" % lib.vts_last_error().decode())
    ws = torch.empty(need, dtype=torch.float32, device=in0.device)
    L.check(lib.vts_msd_forward(C.byref(d), ws.data_ptr(), ws.numel(), L.stream()), "vts_msd_forward")
    return preds, (d, ws)


def msd_grads(D, dpreds, param_grads=True, accumulate=False, input_grad=None):
    """vts_msd_grads over the modules' .grad tensors (allocated where missing); arguments as msd_backward"""
    g = L.MsdGrads()
    for s in range(D.num_D):
        layer = getattr(D, "layer%d" % (D.num_D - 1 - s))
        sg = g.scale[s]
        sg.dpred, sg.accumulate = dpreds[s].data_ptr(), int(accumulate)
        if not param_grads:
            continue
        for j, ci in enumerate(D.CONV_IDX):
            mods = [("dw", "db", getattr(layer, str(ci)))]
            if ci in D.BN_IDX:
                mods.append(("dgamma", "dbeta", getattr(layer, str(D.BN_IDX[ci]))))
            for fw, fb, m in mods:
                for p in (m.weight, m.bias):
                    if p is not None and p.grad is None:
                        p.grad = torch.zeros_like(p)
                getattr(sg, fw)[j] = m.weight.grad.data_ptr()
                getattr(sg, fb)[j] = L.ptr(m.bias.grad if m.bias is not None else None)
    if input_grad is not None:
        g.d_in, g.d_in_accumulate = input_grad[0].data_ptr(), int(bool(input_grad[1]))
    return g


def msd_backward_c(D, ctx, dpreds, param_grads=True, accumulate=False, input_grad=None):
    """the multiscale discriminator's backward through ONE vts_msd_backward call on the workspace of msd_forward_train_c; arguments and
    results as msd_backward (bit-identical to it: tests/test_network_bwd_gpu.py).  The running statistics are not touched."""
    d, ws = ctx
    g = msd_grads(D, dpreds, param_grads, accumulate, input_grad)
    L.check(L.load().vts_msd_backward(C.byref(d), C.byref(g), ws.data_ptr(), ws.numel(), L.stream()), "vts_msd_backward")


def _merge_input_grads(din_scales, input_grad, defer_last=False):
    """d in1 = d0 + pool^T(d1 + pool^T(d2 ...)) into input_grad = (tensor, accumulate?).
    defer_last (only where the full-resolution scale wrote into the caller's buffer): the last, full-resolution pool^T is left to the
    caller -- returns d1 + pool^T(d2 ...), which ops.g_out_grad(coarse=...) adds on the fly."""
    dst, acc = input_grad
    last = 1 if (defer_last and len(din_scales) > 1 and din_scales[0] is dst and din_scales[1].is_contiguous()) else 0
    for s in range(len(din_scales) - 1, last, -1):
        ops.avgpool_bwd(din_scales[s], din_scales[s - 1], accumulate=True)
    if last:
        return din_scales[1]
    if din_scales[0] is dst:      # the full-resolution scale already wrote / accumulated into the caller's buffer
        return
    if acc:
        dst.add_(din_scales[0])
    else:
        dst.copy_(din_scales[0])


def msd_forward(D, in0, in1=None, keep=True, update_stats=True):
    """in0 (++ in1): channel-concatenated input, each a tensor/Act [N,C,H,W].
    Returns (preds: list over scales (full resolution first) of [N,1,h,w], ctx).
    BatchNorm runs in training mode (batch statistics); running buffers are updated when
    update_stats (every reference D call in a train step does: sinskitG_model.py:1361,1374,1490,...)."""
    pyr = _pyramid(D, in0, in1)
    scales = [None] * D.num_D

    def lane(s):
        scales[s] = (pyr[s][0], pyr[s][1], _msd_scale_forward(D, s, pyr[s][0], pyr[s][1], update_stats))

    _run_lanes(D.num_D, lane)
    preds = [sc[2][-1].data for sc in scales]
    if not keep:
        return preds, None
    ctx = MsdCtx()
    ctx.scales = scales
    return preds, ctx


def msd_backward(D, ctx, dpreds, param_grads=True, accumulate=False, input_grad=None):
    """dpreds: list over scales of d loss / d pred.
    param_grads: write (accumulate=False) or add (accumulate=True) into every parameter's .grad.
    input_grad: None, or (tensor [N,C1,H,W], accumulate_flag) receiving the gradient wrt `in1`
    (the second concat source: fake_I in the G step), summed over the pyramid."""
    din_scales = [None] * D.num_D

    def lane(s):
        a0, a1, acts = ctx.scales[s]
        din_scales[s] = _msd_scale_backward(D, s, a0, a1, acts, dpreds[s], param_grads, accumulate, input_grad is not None)

    with ops.deferred_wgrad():
        _run_lanes(D.num_D, lane)
    if input_grad is not None:
        _merge_input_grads(din_scales, input_grad)
    return None


def msd_multi(jobs, criterion, extra=None, extra_cost=0.1, extra_main=False, streams=None):
    """Several discriminators' passes of one training phase, all scales of all of them side by side.
    extra: a callable that runs as ONE MORE lane beside them (work of the phase that needs no discriminator: the generator's L1 /
    perceptual terms, which only read the forward's outputs); extra_cost: its rough time in ms (for the packing of lanes into streams).

    jobs: [(D, [pass, ...]), ...]; the passes of one D run in order (BatchNorm running statistics and gradient
    accumulation are order dependent), different D's and different scales are independent lanes.
    pass: dict(in0, in1=None, real: bool, coeff, slot, grad_coeff=None (None: no gradient / no backward),
               param_grads=True, accumulate=False, input_grad=None, loss=True, pyr=None); `preds` is filled in.
    pyr: [(Act, Act | None)] * num_D, the average-pooled input pyramid when the caller already holds it (the sketch / real-image
    levels do not change within a step, the fake-image levels are shared by the D update and the G step).
    A pass may BATCH several of the reference's discriminator calls (same weights, same input shape) along the sample axis:
      groups=[dict(n0, n1, real, coeff, slot, grad_coeff), ...]  -- samples [n0, n1) are one reference call: own BatchNorm batch
      statistics and running-statistics update (in list order), own loss term; one backward for all of them.
    stat_only=True: a forward-only pass that only RECORDS its BatchNorm statistics; ext_from=<that pass>, ext_after=k splices
    its running-statistics update after group k of this pass (keeps the reference's call order: sinskitG_model.py:1490-1584).
    The first job's first scale (put the full-resolution discriminator first) runs on the launch stream.
    A StyleGAN2 discriminator (`--netD stylegan2`) in `jobs` runs its passes on the launch stream after the lanes have joined; among them
    may be dict(gradient_penalty=True, real=(in0, in1), fake=(in0, in1), alpha, coeff, grad_coeff, slot): sg2d_gradient_penalty, whose
    weight gradients add to what the passes in front of it left (`gan_mode wgangp`)."""
    sg_jobs = [j for j in jobs if getattr(j[0], "is_stylegan2_d", False)]
    jobs = [j for j in jobs if not getattr(j[0], "is_stylegan2_d", False)]
    if jobs:
        _msd_multi(jobs, criterion, extra, extra_cost, extra_main, streams)
    elif extra is not None:
        extra()
    for D, passes in sg_jobs:
        _sg2d_passes(D, passes, criterion)


def _sg2d_passes(D, passes, criterion):
    """the pass dictionaries of msd_multi for a single-output StyleGAN2 discriminator"""
    for p in passes:
        if p.get("gradient_penalty"):      # dict(gradient_penalty=True, real=(in0, in1), fake=(in0, in1), alpha, coeff, grad_coeff, slot)
            sources = lambda pair: tuple(t for t in pair if t is not None)
            p["gradients"] = sg2d_gradient_penalty(D, sources(p["real"]), sources(p["fake"]), p["alpha"], p["slot"], coeff=p["coeff"],
                                                   grad_coeff=p["grad_coeff"], lambda_gp=p.get("lambda_gp", 10.0), constant=p.get("constant", 1.0))
            continue
        in0, in1 = p["in0"], p.get("in1")
        n, c0, h, w = in0.shape
        if in1 is not None:   # torch.cat([in0, in1], 1) as concat-on-store
            x = _empty(n, c0 + in1.shape[1], h, w, in0.device)
            ops.pad_affine(in0, (0, 0, 0, 0), 0, out=x[:, :c0], out_nstride=x.stride(0))
            ops.pad_affine(in1, (0, 0, 0, 0), 0, out=x[:, c0:], out_nstride=x.stride(0))
        else:
            x = in0
        gc = p.get("grad_coeff")
        y, ctx = sg2d_forward(D, x, keep=gc is not None and p.get("loss", True))
        pred = y.view(n, 1, 1, 1)
        p["preds"] = [pred]
        if not p.get("loss", True):
            continue
        g = criterion.accumulate([pred], p["real"], p["coeff"], p["slot"], grad_coeff=gc, want_grad=gc is not None)[0]
        if gc is None:
            continue
        want_in = p.get("input_grad") is not None
        dx = sg2d_backward(D, ctx, g, accumulate=p.get("accumulate", False), input_grad=want_in, param_grads=p.get("param_grads", True))
        if want_in:
            dst, acc = p["input_grad"]
            src = dx[:, c0:] if in1 is not None else dx
            dst.add_(src) if acc else dst.copy_(src)


KO_LANES = tuple(int(k) for k in tune.get("VTS_KO_LANES", "").split(",") if k)
if KO_LANES:      # timing experiment (tools/probes/r02_ko.sh): the named discriminator lanes are skipped, losses and gradients are WRONG
    import sys
    print("WARNING: VTS_KO_LANES=%s -- discriminator lanes are knocked out, this run's results are wrong (timing experiment only)"
          % ",".join(str(k) for k in KO_LANES), file=sys.stderr, flush=True)


LANE_STREAMS = int(tune.get("VTS_LANE_STREAMS", "4"))


def _lane_groups(costs, env="VTS_LANE_GROUPS", streams=None):
    """Which lanes share a stream.  The part runs at most FOUR hardware queues side by side (GPU_MAX_HW_QUEUES, default 4; with 5 - 8 the
    step takes 10 - 11 ms instead of 5.9: the queues beyond four are time-sliced), and a replayed graph maps its parallel branches onto
    them round-robin in capture order -- with one stream per lane (six or seven) WHICH lanes end up sharing a queue was an accident of
    the enqueue order (measured 5.87 .. 6.26 ms over permutations of the same lanes; round 4).  So the lanes are packed into
    VTS_LANE_STREAMS (4) streams here, longest-processing-time first on `costs` (ms estimates), the heavier lane of a stream first.
    VTS_LANE_GROUPS="0|1,5|3|2,4" (discriminator updates) / VTS_LANE_GROUPS_G (the generator step's passes, insensitive: 5.67 - 5.72 ms
    over eleven groupings) override the packing (measurement); VTS_LANE_STREAMS=0: one stream per lane.
    Measured and dropped on top of the packing (round 4): the launch-stream lane's weight gradients appended to the lightest other
    stream (5.95 vs 5.67 ms); side-queue items issued one item late, so that the launch chain's own edge leaves a fork node of the
    captured graph first (5.87 vs 5.67 ms); 2 / 3 / 5 / all side-queue items of the generator backward behind ONE wait on the launch
    stream (5.63 - 5.70 ms: no effect); the decoder lanes' weight gradients on queues of their own (+ 0.22 ms)."""
    n = len(costs)
    spec = tune.get(env, "")
    if spec:
        groups = [[int(t) for t in g.split(",") if t.strip() != "" and int(t) < n] for g in spec.split("|")]
        groups = [g for g in groups if g]
        seen = sorted(i for g in groups for i in g)
        if len(seen) != len(set(seen)):
            raise ValueError("VTS_LANE_GROUPS names a lane twice: %s" % spec)
        return groups + [[i] for i in range(n) if i not in seen]      # lanes the spec does not mention keep their own stream
    limit = LANE_STREAMS if streams is None else min(LANE_STREAMS, streams) if LANE_STREAMS > 0 else 0
    if limit <= 0 or n <= limit:
        return [[i] for i in range(n)]
    order = sorted(range(1, n), key=lambda i: -costs[i])
    bins, load = [[0]], [costs[0]]            # lane 0 (the caller puts its heaviest lane first) stays on the launch stream
    for i in order:
        if len(bins) < limit:
            bins.append([i])
            load.append(costs[i])
            continue
        k = min(range(len(bins)), key=lambda b: load[b])
        bins[k].append(i)
        load[k] += costs[i]
    return bins


def _lane_cost(passes, s):
    """rough time of one discriminator scale over its passes, ms: a latency floor (its ~25 dependent launches) + a term per input pixel"""
    px = 0
    for p in passes:
        a0 = p["_pyr"][0][0]          # (level 0: asking a lazily pooled pyramid for level s here would pool on the caller's stream)
        t = a0.data if isinstance(a0, Act) else a0
        h, w = t.shape[2], t.shape[3]
        for _ in range(s):
            h, w = (h + 1) // 2, (w + 1) // 2
        px += t.shape[0] * h * w
    return 0.35 + 1e-7 * px


LAZY_PYRAMID = tune.get("VTS_LAZY_PYRAMID", "1") != "0"


class _LanePyramid:
    """Input pyramid whose level s is pooled INSIDE the lane that asks for it (s average pools from the full-resolution level, on that
    lane's stream).  Pooling all levels up front (`_pyramid`) put 2 x (num_D - 1) launches on the serial stretch in front of every fork of
    the lanes -- the D2 full-resolution stack and the patch stacks: 67 us per step with nothing beside them; here scale 2 repeats scale 1's
    first pool on its own stream instead (same values bit for bit).  Serial schedule (PARALLEL_SCALES off): levels are shared."""

    def __init__(self, in0, in1):
        self.base = (_as_act(in0), _as_act(in1) if in1 is not None else None)
        self.levels = {0: self.base}

    def __getitem__(self, s):
        if s in self.levels:
            return self.levels[s]
        cur = self.base
        for t in range(1, s + 1):
            if t in self.levels:
                cur = self.levels[t]
                continue
            cur = (_pool_act(cur[0]), _pool_act(cur[1]))
            if not PARALLEL_SCALES:
                self.levels[t] = cur
        return cur


def _prepare_passes(jobs):
    """per-pass bookkeeping of msd_multi / msd_chain: the input pyramid (the caller's, or pooled inside the lanes), result slots"""
    for D, passes in jobs:
        for p in passes:
            if p.get("pyr"):
                p["_pyr"] = p["pyr"]                                          # the caller's precomputed input pyramid
            elif LAZY_PYRAMID:
                p["_pyr"] = _LanePyramid(p["in0"], p.get("in1"))
            else:
                p["_pyr"] = _pyramid(D, p["in0"], p.get("in1"))
            p["preds"] = [None] * D.num_D
            p["_din"] = [None] * D.num_D


def _finish_passes(jobs):
    for D, passes in jobs:
        for p in passes:
            if p.get("input_grad") is not None:
                p["coarse_grad"] = _merge_input_grads(p["_din"], p["input_grad"], defer_last=bool(p.get("defer_merge")))
            p.pop("_pyr"), p.pop("_din")
            if not p.get("keep_stats"):
                p.pop("_stats", None)


def _scale_lane(D, s, passes, criterion, knocked_out=False):
    """the passes of ONE scale of one multiscale discriminator, in order (the body of a lane of msd_multi / msd_chain)"""
    cache = {}      # packed weights of this scale: shared by its passes (they run in order in this lane)
    for p in passes:
        prep = p.get("prep")
        if prep and s in prep:
            prep[s]()       # per-scale preparation inside the lane (pooling of this scale's input level)
        a0, a1 = p["_pyr"][s]
        if knocked_out:   # timing experiment only (VTS_KO_LANES; results are wrong): what a lane costs on the step's critical path
            p["preds"][s] = torch.zeros(1, 1, 1, 1, device=a0.data.device)
            if p.get("input_grad") is not None:
                p["_din"][s] = torch.zeros_like((a1 if a1 is not None else a0).data)
            continue
        ig = p.get("input_grad")
        gsrc = a1 if a1 is not None else a0
        into = (ig[0], ig[1]) if (ig is not None and s == 0 and ig[0].shape == gsrc.data.shape and ig[0].is_contiguous()) else None
        groups = p.get("groups")
        gstarts = [gr["n0"] for gr in groups] if groups else None
        stat_rec = p.setdefault("_stats", {}).setdefault(s, {}) if p.get("stat_only") else None
        src = p.get("ext_from")
        if KO_LANES and src is not None:
            src.setdefault("_stats", {}).setdefault(s, {})
        ext = (src["_stats"][s], p.get("ext_after", 0)) if src is not None else None
        if KO_LANES and src is not None and not ext[0]:      # (timing experiment: the early pass of this lane was knocked out too)
            ext = None
        # pred_scales: the scales whose prediction map the caller reads, for a pass without loss (the full-resolution D2 visualisation pass
        # shows the coarsest scale only; at the other scales it exists for the BatchNorm running statistics: their head is not run)
        skip_head = not p.get("loss", True) and p.get("pred_scales") is not None and s not in p["pred_scales"]
        forward_only = not groups and ext is None and (not p.get("loss", True) or p.get("grad_coeff") is None)
        # (per-launch timing and label knock-outs need the single launches: they take the Python schedule)
        if forward_only and ops.TIMER is None and not ops.KNOCKOUT and patchgan_c_ok(D, a0.data.shape[2], a0.data.shape[3]):
            # nothing of this pass is needed again: the whole scale as ONE call of the network-level C entry (vts_patchgan_forward)
            acts = None
            pred = patchgan_forward_c(D, s, a0, a1, not p.get("stat_only", False), stat_rec, run_head=not skip_head)
        else:
            acts = _msd_scale_forward(D, s, a0, a1, not p.get("stat_only", False), cache, gstarts, stat_rec, ext, skip_head=skip_head)
            pred = None if skip_head else acts[-1].data
        if skip_head:
            continue
        p["preds"][s] = pred
        if groups:
            want = any(gr.get("grad_coeff") is not None for gr in groups)
            g = torch.empty_like(pred) if want else None
            for gr in groups:
                gc = gr.get("grad_coeff")
                if want and gc is None:
                    g[gr["n0"]:gr["n1"]].zero_()
                criterion.accumulate([pred[gr["n0"]:gr["n1"]]], gr["real"], gr["coeff"], gr["slot"], grad_coeff=gc,
                                     want_grad=gc is not None, out_grads=[g[gr["n0"]:gr["n1"]]] if gc is not None else None,
                                     pre_sigmoid=getattr(D, "use_sigmoid", False))
            if want:
                p["_din"][s] = _msd_scale_backward(D, s, a0, a1, acts, g, p.get("param_grads", True), p.get("accumulate", False),
                                                   p.get("input_grad") is not None, cache, gstarts, into=into)
            continue
        if not p.get("loss", True):
            continue
        gc = p.get("grad_coeff")
        g = criterion.accumulate([pred], p["real"], p["coeff"], p["slot"], grad_coeff=gc, want_grad=gc is not None,
                                 pre_sigmoid=getattr(D, "use_sigmoid", False))[0]
        if gc is not None:
            p["_din"][s] = _msd_scale_backward(D, s, a0, a1, acts, g, p.get("param_grads", True), p.get("accumulate", False),
                                               p.get("input_grad") is not None, cache, into=into)


def _msd_multi(jobs, criterion, extra=None, extra_cost=0.1, extra_main=False, streams=None):
    lanes = []
    _prepare_passes(jobs)
    for D, passes in jobs:
        for s in range(D.num_D):
            lanes.append((D, s, passes))
    costs = [_lane_cost(passes, s) for _, s, passes in lanes]
    if extra is not None and extra_main:      # the extra work IS the launch-stream lane (it may fork lanes of its own: the generator forward)
        lanes.insert(0, (None, -1, extra))
        costs.insert(0, float(extra_cost))
    elif extra is not None:
        lanes.append((None, -1, extra))
        costs.append(float(extra_cost))

    def lane(i):
        D, s, passes = lanes[i]
        if D is None:
            passes()
            return
        _scale_lane(D, s, passes, criterion, knocked_out=i in KO_LANES)

    nograd = all(not p.get("param_grads", True) for _, passes in jobs for p in passes)     # the generator step's passes
    groups = _lane_groups(costs, "VTS_LANE_GROUPS_G" if nograd else "VTS_LANE_GROUPS", streams)
    with ops.deferred_wgrad():    # (_run_lanes reduces the weight-gradient partials of each lane on the lane's own stream)
        _run_lanes(len(groups), lambda gi: [lane(i) for i in groups[gi]])
    _finish_passes(jobs)


D_CHAINS = tune.get("VTS_D_CHAINS", "1") != "0"


def msd_chain(chain, criterion, side=None, side_cost=0.1, serial=False):
    """One discriminator's part of a training step as ONE dependency chain:
        update passes (its scales side by side)  ->  `mid` (its optimiser step)  ->  its passes of the generator step.
    msd_multi joins the lanes of ALL discriminators between those stages (and the stages were separate graphs): the step waited for the
    slowest lane of the update phase, ran the weight-gradient reductions and both Adam launches alone on the chip, and forked again --
    although D1's optimiser step needs only D1's lanes, and the generator's backward only D1's chain (the D2 term of the generator is a
    logged value).  The chain's scales share TWO streams: the launch stream (the chain's join points, `mid`, the merge of the input
    gradients) and one side stream.
    serial=True: everything on the current stream -- for a chain that the caller runs inside a lane of its own (fork_lane).
    MEASURED (round 6): a chain led by a SIDE stream needs side <-> side waits (its own join in front of its optimiser step), and
    hipStreamEndCapture crashes on those exactly as on a fork from a side stream: only the chain on the launch stream can have two streams.

    chain: dict(D=, index0=<lane number of scale 0, for VTS_KO_LANES>, update=[passes], mid=callable, gstep=callable -> [passes])
    (pass dictionaries as for msd_multi).  side: callable that runs as one more lane inside the chain's stream pair and is complete before
    `mid` (the generator's L1 terms: the D1 pass of the generator step accumulates onto their gradient)."""
    D = chain["D"]
    _prepare_passes([(D, chain["update"])])

    def stage_lanes(passes):
        """[(cost, body)] per scale"""
        return [(_lane_cost(passes, s), (lambda s=s: _scale_lane(D, s, passes, criterion, knocked_out=(chain.get("index0", 0) + s) in KO_LANES)))
                for s in range(D.num_D)]

    def split2(items):
        """two bins, longest first, the heaviest item first on bin 0 (the launch stream)"""
        order = sorted(range(len(items)), key=lambda i: -items[i][0])
        bins, load = ([], []), [0.0, 0.0]
        for i in order:
            k = 0 if load[0] <= load[1] else 1
            bins[k].append(items[i][1])
            load[k] += items[i][0]
        return bins

    if serial or not PARALLEL_SCALES:
        with ops.deferred_wgrad():
            for _, body in stage_lanes(chain["update"]):
                body()
            if side is not None:
                side()
            ops.wgrad_flush()            # in front of `mid`, the optimiser step (the context's exit would reduce too late)
            _finish_passes([(D, chain["update"])])
            chain["mid"]()
            g = chain["gstep"]()
            _prepare_passes([(D, g)])
            for _, body in stage_lanes(g):
                body()
            _finish_passes([(D, g)])
        return

    with lanes.Fork(1) as f:      # (also on an exception: no stale partial jobs, the base rewound, the second stream joined)
        f.hold()
        with ops.deferred_wgrad():
            f.fork()
            items = stage_lanes(chain["update"])
            if side is not None:
                items.append((float(side_cost), side))
            b_main, b_second = split2(items)
            with f.on(0):
                for b in b_second:
                    b()
                ops.wgrad_flush()
            for b in b_main:
                b()
            ops.wgrad_flush()
            f.join()                                  # the chain's own join, its optimiser step
            _finish_passes([(D, chain["update"])])
            chain["mid"]()
            g = chain["gstep"]()
            _prepare_passes([(D, g)])
            f.fork()
            b_main, b_second = split2(stage_lanes(g))
            with f.on(0):
                for b in b_second:
                    b()
            for b in b_main:
                b()
            f.join()
            _finish_passes([(D, g)])


# ======================================================================================================================
# StyleGAN2 discriminator (`--netD stylegan2`; reference models/stylegan_networks.py:696-786)
# The equalised-learning-rate scale 1/sqrt(fan_in) (:166, :214) is an operand affine of the conv kernels (normalise-on-load),
# ResBlock's 1/sqrt 2 (:691) is folded into conv2's activation gain and into the skip convolution's operand scale, Blur is
# vts_upfirdn2d, the stride-2 3x3 / 1x1 convolutions run on the stride-2 4x4 kernels (ops.convk_s2), EqualLinear(C*16, C) on the
# flattened 4x4 map is a valid 4x4 convolution.
# ======================================================================================================================
_CONST = {}
SQRT2 = 2.0 ** 0.5


def _const(n, v, dev):
    key = (n, float(v), str(dev))
    t = _CONST.get(key)
    if t is None:
        t = _CONST[key] = torch.full((n,), float(v), dtype=torch.float32, device=dev)
    return t


def _scaled(t, s):
    """operand t * s (per-(n, c) affine with a constant scale); s None: t is an operand that carries its affine already"""
    if s is None:
        assert isinstance(t, Act)
        return t
    nc = t.shape[0] * t.shape[1]
    return Act(t, _const(nc, s, t.device), _const(nc, 0.0, t.device))


def _sg_layer_forward(m, x, gain=SQRT2, res=None, extra_scale=1.0):
    """ConvLayer (:622-668).  Returns (output, saved) with saved = (blurred input or x, pre-activation z, operand scale)"""
    from models.stylegan2_blocks import BLUR_KERNEL
    conv, act = m.conv[0], m.act[0]
    n = x.shape[0]
    t = ops.upfirdn2d(x, BLUR_KERNEL, pad=m.blur_pad) if m.downsample else x
    s = extra_scale / (m.cin * m.k * m.k) ** 0.5
    if m.downsample:
        oh, ow = (t.shape[2] - m.k) // 2 + 1, (t.shape[3] - m.k) // 2 + 1
        z = _empty(n, m.cout, oh, ow, x.device)
        ops.convk_s2(_scaled(t, s), conv.weight, z, bias=getattr(conv, "bias", None))
    else:
        z = _empty(n, m.cout, t.shape[2], t.shape[3], x.device)
        ops.convk(_scaled(t, s), conv.weight, z, bias=getattr(conv, "bias", None), pad=m.k // 2)
    if m.activate:
        y = ops.bias_act(z, act.bias if act is not None else None, 0.2, gain, res=res)
    else:
        assert res is None
        y = z
    return y, (t, z, s)


def _sg_layer_backward(m, x_shape, saved, g, gain, accumulate, want_dx=True, dx=None, dx_accumulate=False, param_grads=True, bias_grads=True):
    """backward of _sg_layer_forward: parameter gradients into .grad (bias_grads False: of the weights only), returns the gradient
    w.r.t. the layer input"""
    from models.stylegan2_blocks import BLUR_KERNEL
    conv, act = m.conv[0], m.act[0]
    t, z, s = saved
    if m.activate:
        dz = ops.bias_act_bwd(g, z, act.bias if act is not None else None, 0.2, gain)
        if act is not None and param_grads and bias_grads:
            ops.channel_sum(dz, act.bias.grad.view(-1), accumulate=accumulate)
    else:
        dz = g
        if getattr(conv, "bias", None) is not None and param_grads and bias_grads:
            ops.channel_sum(dz, conv.bias.grad, accumulate=accumulate)
    if not param_grads:
        pass
    elif m.downsample:
        ops.wgradk_s2(dz, _scaled(t, s), conv.weight.grad, accumulate=accumulate)
    else:
        ops.wgradk(dz, _scaled(t, s), conv.weight.grad, pad=m.k // 2, accumulate=accumulate)
    if not want_dx:
        return None
    if m.downsample:
        dt = torch.empty_like(t)
        ops.convk_s2_bwd_data(_scaled(dz, s), conv.weight, dt)
        if dx is None:
            dx = torch.empty(x_shape, dtype=torch.float32, device=g.device)
        ops.upfirdn2d_bwd(dt, dx, BLUR_KERNEL, pad=m.blur_pad, accumulate=dx_accumulate)
    else:
        if dx is None:
            dx = torch.empty(x_shape, dtype=torch.float32, device=g.device)
        ops.convk_bwd_data(_scaled(dz, s), conv.weight, dx, pad=m.k // 2, accumulate=dx_accumulate)
    return dx


class Sg2dCtx:
    __slots__ = ("x_shape", "first", "blocks", "final", "lin")


def sg2d_forward(D, x, keep=True):
    """StyleGAN2Discriminator.forward (:755-786) for netD = 'stylegan2'.  x [N, C, size, size] -> ([N, 1], ctx)"""
    n, dev = x.shape[0], x.device
    ctx = Sg2dCtx()
    ctx.x_shape = tuple(x.shape)
    y, ctx.first = _sg_layer_forward(D.convs[0], x)
    ctx.blocks = []
    for blk in list(D.convs)[1:]:
        y1, s1 = _sg_layer_forward(blk.conv1, y)
        sk, ss = _sg_layer_forward(blk.skip, y, extra_scale=1.0 / SQRT2)
        out, s2 = _sg_layer_forward(blk.conv2, y1, gain=1.0, res=sk)     # sqrt 2 (activation gain) / sqrt 2 (residual merge)
        ctx.blocks.append((tuple(y.shape), s1, tuple(y1.shape), s2, ss))
        y = out
    yf, ctx.final = _sg_layer_forward(D.final_conv, y)
    l0, l1 = D.final_linear[0], D.final_linear[1]
    c4 = l0.weight.shape[0]
    assert yf.shape[2:] == (4, 4), "the discriminator is built for inputs of its `size`"
    z0 = _empty(n, c4, 1, 1, dev)
    s0 = 1.0 / (c4 * 16) ** 0.5
    ops.conv4x4(_scaled(yf, s0), l0.weight, c4 * 16, 16, c4, z0, stride=1, pad=0)         # EqualLinear(C*16 -> C) :199-227
    a0 = ops.bias_act(z0, l0.bias, 0.2, SQRT2)
    s1l = 1.0 / c4 ** 0.5
    out = _empty(n, 1, 1, 1, dev)
    ops.convk(_scaled(a0, s1l), l1.weight.view(1, c4, 1, 1), out, bias=l1.bias, pad=0)
    ctx.lin = (tuple(y.shape), yf, z0, a0, s0, s1l)
    if not keep:
        ctx = None
    return out.view(n, 1), ctx


def sg2d_backward(D, ctx, dout, accumulate=False, input_grad=False, param_grads=True, bias_grads=True):
    """gradients of all parameters into .grad (param_grads; bias_grads False: no bias gradient is touched); returns d/dx when input_grad"""
    l0, l1 = D.final_linear[0], D.final_linear[1]
    c4 = l0.weight.shape[0]
    y_shape, yf, z0, a0, s0, s1l = ctx.lin
    n = dout.shape[0]
    g = dout.reshape(n, 1, 1, 1).contiguous()
    pg, bg = param_grads, param_grads and bias_grads
    kw = dict(param_grads=pg, bias_grads=bias_grads)
    if bg:
        ops.channel_sum(g, l1.bias.grad, accumulate=accumulate)
    if pg:
        ops.wgradk(g, _scaled(a0, s1l), l1.weight.grad.view(1, c4, 1, 1), pad=0, accumulate=accumulate)
    da0 = torch.empty_like(a0)
    ops.convk_bwd_data(_scaled(g, s1l), l1.weight.view(1, c4, 1, 1), da0, pad=0)
    dz0 = ops.bias_act_bwd(da0, z0, l0.bias, 0.2, SQRT2)
    if bg:
        ops.channel_sum(dz0, l0.bias.grad, accumulate=accumulate)
    if pg:
        ops.wgrad4x4(dz0, _scaled(yf, s0), l0.weight.grad, stride=1, pad=0, accumulate=accumulate)
    dyf = torch.empty_like(yf)
    ops.conv4x4(_scaled(dz0, s0), l0.weight, 16, c4 * 16, c4, dyf, stride=1, pad=0, transposed=True)
    g = _sg_layer_backward(D.final_conv, y_shape, ctx.final, dyf, SQRT2, accumulate, **kw)
    blocks = list(D.convs)[1:]
    for blk, (x_shape, s1, y1_shape, s2, ss) in zip(reversed(blocks), reversed(ctx.blocks)):
        dy1 = _sg_layer_backward(blk.conv2, y1_shape, s2, g, 1.0, accumulate, **kw)
        dx = _sg_layer_backward(blk.skip, x_shape, ss, g, 1.0, accumulate, **kw)
        g = _sg_layer_backward(blk.conv1, x_shape, s1, dy1, SQRT2, accumulate, dx=dx, dx_accumulate=True, **kw)
    return _sg_layer_backward(D.convs[0], ctx.x_shape, ctx.first, g, SQRT2, accumulate, want_dx=input_grad, **kw)


# ---- WGAN-GP gradient penalty on the StyleGAN2 discriminator (reference models/networks.py:550-583, cal_gradient_penalty 'mixed') ----
# The discriminator is piecewise linear in its input and couples no samples (its minibatch-stddev branch is off: stylegan_networks.py:
# 744, 769), so with g = dD(x^)/dx^ (dout = 1), P = lambda / N sum_n (||g_n + 1e-16|| - c)^2 and v = dP/dg the parameter gradient of P is the
# ordinary first-order weight gradient with every layer INPUT replaced by the tangent of v pushed forward through the network (same
# convolutions, no biases, each activation replaced by its derivative at the saved pre-activation) under the backward signals of
# dout = 1:  dP/dW_k = delta_k (x) t_{k-1}.  No bias receives a gradient.  Forward over reverse instead of autograd's double backward:
# the penalty runs on the discriminator's own conv / FIR / bias_act_bwd / weight-gradient kernels.
def _sg_layer_tangent(m, tx, saved, gain=SQRT2, tres=None, extra_scale=1.0):
    """tangent of _sg_layer_forward at its saved pre-activation: (tangent output, saved in the layer's format with the tangent input)"""
    from models.stylegan2_blocks import BLUR_KERNEL
    conv, act = m.conv[0], m.act[0]
    _, z, _ = saved
    first = isinstance(tx, Act)             # the cotangent v = Act(g, scale, shift): it carries the layer's operand scale itself
    assert not (first and m.downsample)
    tt = ops.upfirdn2d(tx, BLUR_KERNEL, pad=m.blur_pad) if m.downsample else tx
    s = None if first else extra_scale / (m.cin * m.k * m.k) ** 0.5
    tz = torch.empty_like(z)
    if m.downsample:
        ops.convk_s2(_scaled(tt, s), conv.weight, tz)
    else:
        ops.convk(_scaled(tt, s), conv.weight, tz, pad=m.k // 2)
    if m.activate:
        ty = ops.bias_act_bwd(tz, z, act.bias if act is not None else None, 0.2, gain)
        if tres is not None:
            ty = ops.pad_affine(ty, (0, 0, 0, 0), 0, res=tres)
    else:
        assert tres is None
        ty = tz
    return ty, (tt, z, s)


def sg2d_first_scale(D):
    """the equalised-lr operand scale of the discriminator's first convolution"""
    m = D.convs[0]
    return 1.0 / (m.cin * m.k * m.k) ** 0.5


def sg2d_tangent_forward(D, ctx, v):
    """Pushes the input tangent v through the discriminator linearised at ctx (of sg2d_forward(keep=True)), layer by layer: Blur where
    the layer downsamples, the same convolution with the same operand scale and no bias, bias_act_bwd at the saved pre-activation in
    place of the activation (plus the skip branch's tangent where bias_act took `res`), the EqualLinear pair likewise.
    v: a tensor [N, C, size, size], or an Act whose affine ALREADY includes sg2d_first_scale(D) (the cotangent of vts_gp_penalty applied on
    load).  Returns an Sg2dCtx whose saved layer inputs are the tangents and whose pre-activations are ctx's: sg2d_backward on it under
    the same dout gives d<v, dD/dx> / d weights."""
    tc = Sg2dCtx()
    tc.x_shape = ctx.x_shape
    ty, tc.first = _sg_layer_tangent(D.convs[0], v, ctx.first)
    tc.blocks = []
    for blk, (x_shape, s1, y1_shape, s2, ss) in zip(list(D.convs)[1:], ctx.blocks):
        ty1, t1 = _sg_layer_tangent(blk.conv1, ty, s1)
        tsk, ts = _sg_layer_tangent(blk.skip, ty, ss, extra_scale=1.0 / SQRT2)
        ty, t2 = _sg_layer_tangent(blk.conv2, ty1, s2, gain=1.0, tres=tsk)
        tc.blocks.append((x_shape, t1, y1_shape, t2, ts))
    tyf, tc.final = _sg_layer_tangent(D.final_conv, ty, ctx.final)
    l0 = D.final_linear[0]
    c4 = l0.weight.shape[0]
    y_shape, _, z0, _, s0, s1l = ctx.lin
    tz0 = torch.empty_like(z0)
    ops.conv4x4(_scaled(tyf, s0), l0.weight, c4 * 16, 16, c4, tz0, stride=1, pad=0)
    ta0 = ops.bias_act_bwd(tz0, z0, l0.bias, 0.2, SQRT2)
    tc.lin = (y_shape, tyf, z0, ta0, s0, s1l)
    return tc


def sg2d_gradient_penalty(D, real, fake, alpha, slot, coeff=1.0, grad_coeff=1.0, lambda_gp=10.0, constant=1.0, param_grads=True):
    """cal_gradient_penalty(netD, real, fake, type='mixed', constant, lambda_gp) (networks.py:550-583) for the StyleGAN2 discriminator.
    real / fake: a tensor [N, C, size, size] or a tuple of up to two concat sources (ops.gp_interp); alpha: device [N].
    coeff * penalty is added to the loss slot `slot`; with param_grads, grad_coeff * d penalty / d weights is ADDED to every weight's
    .grad (no bias .grad is touched: those gradients are exactly zero).  Returns g = dD(x^)/dx^ [N, C, size, size] over all channels
    (the reference's `gradients`).  Launches only; capturable; a second call gives the same bits.
    Two-pass form: the (dout = 1) backward-data chain runs once for g and once more under the tangents."""
    xh = ops.gp_interp(real, fake, alpha)
    n = xh.shape[0]
    ones = _const(n, 1.0, xh.device)
    _, ctx = sg2d_forward(D, xh, keep=True)
    g = sg2d_backward(D, ctx, ones, input_grad=True, param_grads=False)
    scale, shift = ops.gp_penalty(g, slot, coeff, grad_coeff * sg2d_first_scale(D), lambda_gp=lambda_gp, constant=constant)
    if param_grads:
        tctx = sg2d_tangent_forward(D, ctx, Act(g, scale, shift))
        sg2d_backward(D, tctx, ones, accumulate=True, param_grads=True, bias_grads=False, input_grad=False)
    return g


_SG_BUF = {}


def _sg_buf(tag, like, shape):
    """persistent scratch tied to a parameter (its address is stable, so captured graphs keep pointing at the same buffer)"""
    key = (tag, like.data_ptr(), tuple(shape))
    t = _SG_BUF.get(key)
    if t is None:
        t = _SG_BUF[key] = torch.empty(shape, dtype=torch.float32, device=like.device)
    return t


def _k4():
    from models.stylegan2_blocks import BLUR_KERNEL
    return [[4.0 * v for v in row] for row in BLUR_KERNEL]


class ModConvCtx:
    """what modulated_conv2d_backward needs: the input, the style, s = modulation(style), the operand scale c * s, the demodulation
    coefficients d (None without demodulation), the output y, the blurred operand (downsampling form), the weight views"""
    __slots__ = ("form", "x", "style", "s", "cs", "d", "y", "tb", "wt", "wT", "mod_weight", "scale", "k", "pads")


def modulated_conv2d_forward(x, style, weight, mod_weight, mod_bias, demodulate=True, upsample=False, downsample=False, keep=True):
    """ModulatedConv2d.forward (:304-348) with a style vector, all four forms.  Instead of the reference's per-sample weights in a
    grouped convolution: y = conv(x * s[n,ci] / sqrt(fan_in), W) * demod[n,co] on the shared weight W = weight[0]; both factors ride on
    the operand affines.  style [N, style_dim]; the modulation is EqualLinear(style_dim, Ci, bias_init=1) (:199-227), a 1 x 1 convk.
    plain: pad K // 2.  downsample: Blur (:277-283), then stride 2.  upsample: the transposed stride-2 convolution (:320-330) is the input
    adjoint of the stride-2 K x K convolution on the weight in [Ci, Co, K, K] order, then demod, then Blur with the 4x kernel (:269-275).
    Returns (y, ctx); ctx is None unless keep."""
    from models.stylegan2_blocks import BLUR_KERNEL
    assert not (upsample and downsample)
    n, ci, h, w_ = x.shape
    wt = weight.view(weight.shape[-4], ci, weight.shape[-2], weight.shape[-1])
    co, k = wt.shape[0], wt.shape[2]
    sd = style.shape[1]
    st4 = style.reshape(n, sd, 1, 1).contiguous()
    s = _empty(n, ci, 1, 1, x.device)
    ops.convk(_scaled(st4, 1.0 / sd ** 0.5), mod_weight.view(ci, sd, 1, 1), s, bias=mod_bias, pad=0)
    scale = 1.0 / (ci * k * k) ** 0.5
    cs = (s.view(-1) * scale).contiguous()
    xin = Act(x, cs, _const(n * ci, 0.0, x.device))
    demod = ops.modconv_demod(wt, s.view(n, ci), scale) if demodulate else None
    tb = wT = pads = None
    if upsample:
        p = 2 - (k - 1)
        pads = ((p + 1) // 2 + 1, p // 2 + 1)
        wT = ops.modconv_transpose(wt, _sg_buf("modconv_wT", weight, (ci, co, k, k)))
        pre = _empty(n, co, 2 * (h - 1) + k, 2 * (w_ - 1) + k, x.device)
        ops.convk_s2_bwd_data(xin, wT, pre)
        out = ops.upfirdn2d(pre, _k4(), pad=pads)                      # d[n,co] is per channel: it commutes with the Blur
    elif downsample:
        p = 2 + (k - 1)
        pads = ((p + 1) // 2, p // 2)
        t = ops.pad_affine(xin, (0, 0, 0, 0), 0)                      # materialise x * s, then Blur (:323-327), then stride 2
        tb = ops.upfirdn2d(t, BLUR_KERNEL, pad=pads)
        out = _empty(n, co, (tb.shape[2] - k) // 2 + 1, (tb.shape[3] - k) // 2 + 1, x.device)
        ops.convk_s2(tb, wt, out)
    else:
        out = _empty(n, co, h, w_, x.device)
        ops.convk(xin, wt, out, pad=k // 2)
    y = out if demod is None else ops.pad_affine(Act(out, demod.view(-1), _const(n * co, 0.0, x.device)), (0, 0, 0, 0), 0)
    if not keep:
        return y, None
    ctx = ModConvCtx()
    ctx.form = "up" if upsample else ("down" if downsample else "plain")
    ctx.x, ctx.style, ctx.s, ctx.cs, ctx.d, ctx.y, ctx.tb, ctx.wt, ctx.wT = x, st4, s, cs, demod, y, tb, wt, wT
    ctx.mod_weight, ctx.scale, ctx.k, ctx.pads = mod_weight, scale, k, pads
    return y, ctx


def modulated_conv2d(x, style, weight, mod_weight, mod_bias, demodulate=True, downsample=False, upsample=False):
    """ModulatedConv2d.forward (:304-348) without a context: modulated_conv2d_forward(...)[0]"""
    return modulated_conv2d_forward(x, style, weight, mod_weight, mod_bias, demodulate=demodulate, upsample=upsample, downsample=downsample,
                                    keep=False)[0]


def modulated_conv2d_backward(ctx, g, *, dweight, dmod_weight, dmod_bias, accumulate=False, want_dx=True, want_dstyle=True):
    """backward of modulated_conv2d_forward for g = dL/dy: the parameter gradients are written into (accumulate: added to) dweight
    [1,Co,Ci,K,K], dmod_weight [Ci, style_dim], dmod_bias [Ci]; returns (dx or None, dstyle [N, style_dim] or None).
    With u = x c s, z = conv(u, W), y = z d:  dz = g d (an operand affine), dd = sum_hw g y / d, du = conv^T(dz, W), dx = du c s,
    ds = c sum_hw du x + the demodulation's share (vts_modconv_demod_bwd), dW = wgrad(u, dz) + the demodulation's share; the
    modulation layer's backward runs on the 1 x 1 members of the convolution family like its forward.  No atomics anywhere: two calls
    give the same bits."""
    from models.stylegan2_blocks import BLUR_KERNEL
    x, wt, k, scale = ctx.x, ctx.wt, ctx.k, ctx.scale
    n, ci, h, w_ = x.shape
    co, dev = wt.shape[0], x.device
    g = g.contiguous()
    dw = dweight.view(co, ci, k, k)
    xin = Act(x, ctx.cs, _const(n * ci, 0.0, dev))
    du = _empty(n, ci, h, w_, dev)
    if ctx.form == "up":
        gb = _empty(n, co, 2 * (h - 1) + k, 2 * (w_ - 1) + k, dev)
        ops.upfirdn2d_bwd(g, gb, _k4(), pad=ctx.pads)                  # Blur^T first, d afterwards (per channel: they commute)
        dz = gb if ctx.d is None else Act(gb, ctx.d.view(-1), _const(n * co, 0.0, dev))
        ops.convk_s2(dz, ctx.wT, du)
        dwT = _sg_buf("modconv_dwT", dweight, (ci, co, k, k))
        ops.wgradk_s2(xin, dz, dwT)                                    # weight gradient of the stride-2 convolution pairing (dz -> u)
        ops.modconv_transpose(dwT, dw, accumulate=accumulate)
    else:
        dz = g if ctx.d is None else Act(g, ctx.d.view(-1), _const(n * co, 0.0, dev))
        if ctx.form == "down":
            dtb = torch.empty_like(ctx.tb)
            ops.convk_s2_bwd_data(dz, wt, dtb)
            ops.wgradk_s2(dz, ctx.tb, dw, accumulate=accumulate)
            ops.upfirdn2d_bwd(dtb, du, BLUR_KERNEL, pad=ctx.pads)
        else:
            ops.convk_bwd_data(dz, wt, du, pad=k // 2)
            ops.wgradk(dz, xin, dw, pad=k // 2, accumulate=accumulate)
    ds = torch.empty(n, ci, dtype=torch.float32, device=dev)
    dx = torch.empty_like(x) if want_dx else None
    ops.modconv_scale_dot(du, x, ds, f=ctx.cs, out=dx, alpha=scale)    # dx = du c s  and  ds = c sum_hw du x  in one pass
    if ctx.d is not None:
        gy = torch.empty(n, co, dtype=torch.float32, device=dev)
        ops.modconv_scale_dot(g, ctx.y, gy)                            # sum_hw g y = dd d  (y is what the forward keeps, d > 0)
        ops.modconv_demod_bwd(gy / ctx.d, ctx.d, wt, ctx.s.view(n, ci), scale, dw, ds, accumulate_dw=True, accumulate_ds=True)
    sd = ctx.style.shape[1]
    ds4 = ds.view(n, ci, 1, 1)
    mw = ctx.mod_weight.view(ci, sd, 1, 1)
    ops.wgradk(ds4, _scaled(ctx.style, 1.0 / sd ** 0.5), dmod_weight.view(ci, sd, 1, 1), pad=0, accumulate=accumulate)
    ops.channel_sum(ds4, dmod_bias, accumulate=accumulate)
    dstyle = None
    if want_dstyle:
        dstyle = _empty(n, sd, 1, 1, dev)
        ops.convk_bwd_data(_scaled(ds4, 1.0 / sd ** 0.5), mw, dstyle, pad=0)
        dstyle = dstyle.view(n, sd)
    return dx, dstyle


def _grad(p):
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


def styled_conv_forward(m, x, style, noise=None):
    """StyledConv.forward with a style (:408-415; m: models.stylegan2_blocks.StyledConv): ModulatedConv2d plain or upsampling ->
    NoiseInjection (:351-363; the reference draws fresh N(0, 1) noise when none is given -- the draw is an input here) -> FusedLeakyReLU.
    Returns (y, saved)."""
    c = m.conv
    z, ctx = modulated_conv2d_forward(x, style, c.weight, c.modulation.weight, c.modulation.bias, demodulate=c.demodulate, upsample=c.upsample)
    if m.inject_noise:
        if noise is None:
            noise = torch.randn(z.shape[0], 1, z.shape[2], z.shape[3], device=x.device)
        z = ops.pad_affine(z, (0, 0, 0, 0), 0, res=(noise * m.noise.weight).expand(-1, z.shape[1], -1, -1).contiguous())
    y = ops.bias_act(z, m.activate.bias, 0.2, SQRT2)
    return y, (ctx, z, noise)


def styled_conv_backward(m, saved, g, accumulate=False, want_dx=True, want_dstyle=True):
    """parameter gradients into .grad (created when missing); returns (dx, dstyle)"""
    ctx, z, noise = saved
    c = m.conv
    dz = ops.bias_act_bwd(g.contiguous(), z, m.activate.bias, 0.2, SQRT2)
    ops.channel_sum(dz, _grad(m.activate.bias).view(-1), accumulate=accumulate)
    if m.inject_noise:
        gw = (dz.sum(1, keepdim=True) * noise).sum().view(1)           # one scalar parameter: d weight = <dz summed over channels, noise>
        ng = _grad(m.noise.weight)
        ng.copy_(ng + gw if accumulate else gw)
    return modulated_conv2d_backward(ctx, dz, dweight=_grad(c.weight), dmod_weight=_grad(c.modulation.weight), dmod_bias=_grad(c.modulation.bias),
                                     accumulate=accumulate, want_dx=want_dx, want_dstyle=want_dstyle)


def to_rgb_forward(m, x, style, skip=None):
    """ToRGB.forward (:428-437; m: models.stylegan2_blocks.ToRGB): 1 x 1 modulated convolution without demodulation + bias
    (+ Upsample(blur_kernel) of the skip image, :98-116).  Returns (y, saved)."""
    c = m.conv
    z, ctx = modulated_conv2d_forward(x, style, c.weight, c.modulation.weight, c.modulation.bias, demodulate=False)
    up = None
    if skip is not None:
        assert m.has_upsample, "ToRGB(upsample=False) takes no skip image"
        up = ops.upfirdn2d(skip, _k4(), up=2, down=1, pad=m.up_pad)
    y = ops.bias_act(z, m.bias, 1.0, 1.0, res=up)                      # slope 1, gain 1: z + bias (+ upsampled skip)
    return y, (ctx, None if skip is None else tuple(skip.shape))


def to_rgb_backward(m, saved, g, accumulate=False, want_dx=True, want_dstyle=True):
    """parameter gradients into .grad (created when missing); returns (dx, dstyle, dskip or None)"""
    ctx, skip_shape = saved
    c = m.conv
    g = g.contiguous()
    ops.channel_sum(g, _grad(m.bias).view(-1), accumulate=accumulate)
    dskip = None
    if skip_shape is not None:
        dskip = torch.empty(skip_shape, dtype=torch.float32, device=g.device)
        ops.upfirdn2d_bwd(g, dskip, _k4(), up=2, down=1, pad=m.up_pad)
    dx, dstyle = modulated_conv2d_backward(ctx, g, dweight=_grad(c.weight), dmod_weight=_grad(c.modulation.weight),
                                           dmod_bias=_grad(c.modulation.bias), accumulate=accumulate, want_dx=want_dx, want_dstyle=want_dstyle)
    return dx, dstyle, dskip


# ---- generator side (`--netG stylegan2 | smallstylegan2`; reference stylegan_networks.py:800-930) ------------------------------------
def _sg_resblock_forward(blk, y):
    """ResBlock :671-693 with skip_gain 1: (conv2(conv1(x)) + skip(x)) / sqrt 2; the 1 / sqrt 2 rides on conv2's activation gain and on
    the skip operand (identity skip: one scaled copy)"""
    y1, s1 = _sg_layer_forward(blk.conv1, y)
    if blk.skip is not None:
        sk, ss = _sg_layer_forward(blk.skip, y, extra_scale=1.0 / SQRT2)
    else:
        sk, ss = ops.pad_affine(_scaled(y, 1.0 / SQRT2), (0, 0, 0, 0), 0), None
    out, s2 = _sg_layer_forward(blk.conv2, y1, gain=1.0, res=sk)
    return out, (tuple(y.shape), s1, tuple(y1.shape), s2, ss)


def _sg_resblock_backward(blk, saved, g, accumulate, pg=True):
    x_shape, s1, y1_shape, s2, ss = saved
    dy1 = _sg_layer_backward(blk.conv2, y1_shape, s2, g, 1.0, accumulate, param_grads=pg)
    if blk.skip is not None:
        dx = _sg_layer_backward(blk.skip, x_shape, ss, g, 1.0, accumulate, param_grads=pg)
    else:
        dx = ops.pad_affine(_scaled(g, 1.0 / SQRT2), (0, 0, 0, 0), 0)
    return _sg_layer_backward(blk.conv1, x_shape, s1, dy1, SQRT2, accumulate, dx=dx, dx_accumulate=True, param_grads=pg)


def _styled_up_forward(m, x, noise=None):
    """StyledConv(upsample=True) with style None (:399-407 -> ModulatedConv2d :304-330 -> Blur -> NoiseInjection -> FusedLeakyReLU):
    the demodulated weight depends on the parameters only (vts_modconv_weight); the transposed stride-2 convolution is the input
    adjoint of the stride-2 K x K convolution the library already has (ops.convk_s2_bwd_data), then Blur with the 4x kernel, pad (1, 1)."""
    n, ci, h, w = x.shape
    wt = ops.modconv_weight(m.conv.weight, transpose=True)            # [Ci, Co, 3, 3]
    pre = _empty(n, m.cout, 2 * h + 1, 2 * w + 1, x.device)
    ops.convk_s2_bwd_data(x, wt, pre)
    z = ops.upfirdn2d(pre, _k4(), pad=(1, 1))
    if m.inject_noise:
        # image + weight * noise (:358-363); the reference draws fresh N(0, 1) noise per call -- the draw is an input here (tests pass it)
        if noise is None:
            noise = torch.randn(n, 1, z.shape[2], z.shape[3], device=x.device)
        z = ops.pad_affine(z, (0, 0, 0, 0), 0, res=(noise * m.noise.weight).expand(-1, m.cout, -1, -1).contiguous())
    y = ops.bias_act(z, m.activate.bias, 0.2, SQRT2)
    return y, (x, wt, z, noise)


def _styled_up_backward(m, saved, g, accumulate, pg=True, want_dx=True):
    x, wt, z, noise = saved
    dz = ops.bias_act_bwd(g, z, m.activate.bias, 0.2, SQRT2)
    n, co = dz.shape[0], dz.shape[1]
    if pg:
        ops.channel_sum(dz, m.activate.bias.grad.view(-1), accumulate=accumulate)
        if m.inject_noise:
            gw = (dz.sum(1, keepdim=True) * noise).sum().view(1)       # one scalar parameter: d weight = <dz summed over channels, noise>
            m.noise.weight.grad.copy_(m.noise.weight.grad + gw if accumulate else gw)
    dpre = _empty(n, co, 2 * x.shape[2] + 1, 2 * x.shape[3] + 1, x.device)
    ops.upfirdn2d_bwd(dz, dpre, _k4(), pad=(1, 1))
    if pg:
        dwt = torch.empty_like(wt)
        ops.wgradk_s2(x, dpre, dwt)                                    # weight gradient of the stride-2 convolution pairing (dpre -> x)
        ops.modconv_weight_bwd(m.conv.weight, dwt, m.conv.weight.grad, transpose=True, accumulate=accumulate)
    if not want_dx:
        return None
    dx = torch.empty_like(x)
    ops.convk_s2(dpre, wt, dx)
    return dx


class Sg2gCtx:
    __slots__ = ("x_shape", "first", "enc", "dec", "ups", "last")


def sg2g_forward(G, x, keep=True, noises=None):
    """StyleGAN2Generator.forward (:922-930): encoder -> decoder.  x [N, C, size, size] -> ([N, 3, size, size], ctx)"""
    ctx = Sg2gCtx()
    ctx.x_shape = tuple(x.shape)
    enc, dec = list(G.encoder.convs), list(G.decoder.convs)
    y, ctx.first = _sg_layer_forward(enc[1], x)
    ctx.enc, ctx.dec, ctx.ups = [], [], []
    for blk in enc[2:]:
        y, sv = _sg_resblock_forward(blk, y)
        ctx.enc.append(sv)
    nb = G.n_blocks // 2
    for blk in dec[:nb]:
        y, sv = _sg_resblock_forward(blk, y)
        ctx.dec.append(sv)
    for i, m in enumerate(dec[nb:-1]):
        y, sv = _styled_up_forward(m, y, None if noises is None else noises[i])
        ctx.ups.append(sv)
    shape = tuple(y.shape)
    out, sv = _sg_layer_forward(dec[-1], y)
    ctx.last = (shape, sv)
    return out, (ctx if keep else None)


def sg2g_backward(G, ctx, dout, accumulate=False, input_grad=False):
    """gradients of all parameters into .grad; returns d/dx when input_grad"""
    enc, dec = list(G.encoder.convs), list(G.decoder.convs)
    nb = G.n_blocks // 2
    shape, sv = ctx.last
    g = _sg_layer_backward(dec[-1], shape, sv, dout, SQRT2, accumulate)
    for m, sv in zip(reversed(dec[nb:-1]), reversed(ctx.ups)):
        g = _styled_up_backward(m, sv, g, accumulate)
    for blk, sv in zip(reversed(dec[:nb]), reversed(ctx.dec)):
        g = _sg_resblock_backward(blk, sv, g, accumulate)
    for blk, sv in zip(reversed(enc[2:]), reversed(ctx.enc)):
        g = _sg_resblock_backward(blk, sv, g, accumulate)
    return _sg_layer_backward(enc[1], ctx.x_shape, ctx.first, g, SQRT2, accumulate, want_dx=input_grad)


# ======================================================================================================================
# SIFID (reference models/sifid.py:205-233, models/inception.py:57-67, models/model_utils.py:481-488, 541-555): Inception-v3 block 0
# on the convolution kernels of this library + the Frechet distance of the activation statistics, per image
# ======================================================================================================================
def inception_block0(net, x):
    """x [N,3,H,W] (network input, i.e. after InceptionV3.forward's 2x - 1) -> [N,64,h,w] features.  BatchNorm (eval, eps 0.001) and
    ReLU of a layer are applied by the next convolution on load; the last layer's are materialised."""
    n, dev = x.shape[0], x.device
    cur, act = x, 0
    for m, (ci, co, stride, pad) in zip(net.blocks[0], _INCEPTION_SPEC):
        h, w = (cur.data if isinstance(cur, Act) else cur).shape[2:]
        oh, ow = (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1
        out = _empty(n, co, oh, ow, dev)
        if stride == 2:
            ops.convk_s2(cur, m.conv.weight, out, act_in=act)
        else:
            ops.convk(cur, m.conv.weight, out, pad=pad, act_in=act)
        sc = m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps)      # [C] vectors: plumbing, not arithmetic on activations
        sh = m.bn.bias - m.bn.running_mean * sc
        cur, act = Act(out, sc.repeat(n).contiguous(), sh.repeat(n).contiguous()), RELU
    return ops.pad_affine(cur, (0, 0, 0, 0), 0, act=RELU)


_INCEPTION_SPEC = ((3, 32, 2, 0), (32, 32, 1, 0), (32, 64, 1, 1))   # (cin, cout, stride, padding): torchvision's Conv2d_1a / 2a / 2b


def sifid_pairs(net, a, b, batch=16):
    """per-image SIFID of two stacks of network inputs [N,3,H,W] (calculate_sifid_given_arrays: the statistics are taken over the
    positions of ONE image's feature map): device tensor [N]"""
    n = a.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    for i0 in range(0, n, batch):
        fa, fb = inception_block0(net, a[i0:i0 + batch]), inception_block0(net, b[i0:i0 + batch])
        for j in range(fa.shape[0]):
            out[i0 + j:i0 + j + 1].copy_(ops.frechet_distance(fa[j].reshape(fa.shape[1], -1), fb[j].reshape(fb.shape[1], -1)))
    return out


def sifid_images(net, real_I, fake_I):
    """I_SIFID (model_utils.py:481-488): both images min-max normalised by the REAL image's range, the fake one clamped; mean over images"""
    lohi = ops.minmax(real_I)
    a = ops.sifid_input(real_I, 0, 3, lohi=lohi)
    b = ops.sifid_input(fake_I, 0, 3, lohi=lohi, clamp01=True)
    return sifid_pairs(net, a, b, batch=1).mean()


def sifid_tactile(net, real_T, fake_T, size=299):
    """T_SIFID (model_utils.py:541-555): fake patches clamped to (0, 1) (:519), nearest resize to 299 x 299, gx and gy each tiled to
    three channels, per-patch SIFID, mean of (gx + gy) / 2"""
    vals = []
    for c in (0, 1):
        a = ops.sifid_input(real_T, c, 1, size=(size, size))
        b = ops.sifid_input(fake_T, c, 1, size=(size, size), clamp01=True)
        vals.append(sifid_pairs(net, a, b))
    return ((vals[0] + vals[1]) * 0.5).mean()


def sifid_pairs_batched(net, a, b, batch=16):
    """sifid_pairs for a batch (the baselines' metrics): Inception block 0 on slices of `batch` images, then ONE batched Frechet call per
    slice (ops.frechet_distance_batched: three launches for all its pairs); device tensor [N]"""
    n = a.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    for i0 in range(0, n, batch):
        fa, fb = inception_block0(net, a[i0:i0 + batch]), inception_block0(net, b[i0:i0 + batch])
        k, d = fa.shape[:2]
        out[i0:i0 + k].copy_(ops.frechet_distance_batched(fa.reshape(k, d, -1), fb.reshape(k, d, -1)))
    return out


def sifid_images_batched(net, real_I, fake_I, batch=16):
    """I_SIFID of a batch of images (model_utils.py:481-493): min-max by the range of the whole REAL batch, fake side clamped, one
    distance per image, mean over images"""
    lohi = ops.minmax(real_I)
    a = ops.sifid_input(real_I, 0, 3, lohi=lohi)
    b = ops.sifid_input(fake_I, 0, 3, lohi=lohi, clamp01=True)
    return sifid_pairs_batched(net, a, b, batch).mean()


def sifid_tactile_batched(net, real_T, fake_T, size=299, batch=16):
    """T_SIFID (model_utils.py:541-555) as sifid_tactile, the per-patch distances from batched Frechet calls"""
    vals = []
    for c in (0, 1):
        a = ops.sifid_input(real_T, c, 1, size=(size, size))
        b = ops.sifid_input(fake_T, c, 1, size=(size, size), clamp01=True)
        vals.append(sifid_pairs_batched(net, a, b, batch))
    return ((vals[0] + vals[1]) * 0.5).mean()


def tactile_patch_fid(real_T, fake_T, reduction="none", clamp_fake=True):
    """T_FID (models/tactile_patch_fid.py:119-154 TactilePatchFID): Frechet distance over the 18-dimensional valid 3 x 3 crops of the
    2-channel patches [N, 2, h, w]; clamp_fake: the fake side clamped to [0, 1] as compute_evaluation_metric does first (model_utils.py:517).
    reduction 'none': one distance over the crops of all patches (what compute_evaluation_metric reports); 'mean': one distance per
    patch pair, all in one batched call, then their mean.  Device scalar."""
    n, _, h, w = real_T.shape
    if fake_T.shape[0] != n and reduction == "mean":
        raise ValueError("The number of images in the two groups are not equal")
    f1, f2 = ops.tfid_features(real_T.contiguous()), ops.tfid_features(fake_T.contiguous(), clamp01=clamp_fake)
    if reduction == "none":
        return ops.frechet_distance_batched(f1.unsqueeze(0), f2.unsqueeze(0))[0]
    if reduction != "mean":
        raise NotImplementedError("reduction %s is not implemented" % reduction)
    # [18, N P] -> [N, 18, P]: the crops of one patch are one pair's feature set (a copy: plumbing)
    f1 = f1.view(18, n, -1).permute(1, 0, 2).contiguous()
    f2 = f2.view(18, n, -1).permute(1, 0, 2).contiguous()
    return ops.frechet_distance_batched(f1, f2).mean()


# ======================================================================================================================
# SPADE generator (`--netG spade`; reference models/networks.py:2075-2200, models/architecture.py:21-68, models/normalization.py:68-112)
# Every 3x3 convolution reads a pre-padded operand (the modulate kernel stores that layout directly) through conv3_valid and its adjoint /
# weight gradient, the dispatch of the ResNet blocks, never on Winograd: layers of >= 64 x 64 channels run on the GEMM-class kernels,
# the rest (label_nc = 1 inputs, the output_nc-channel image head) and the 1x1 shortcut on the 4x4 family.
# ======================================================================================================================
class _SnState:
    """what one spectral-normalised convolution keeps between the generator's forward and backward: W / sigma, sigma, a gradient buffer"""
    __slots__ = ("w", "sigma", "g")


def _sn_state(conv):
    st = getattr(conv, "_sn_state", None)
    w = conv.weight_orig
    if st is None or st.w.shape != w.shape or st.w.device != w.device:
        st = _SnState()
        st.w, st.g, st.sigma = torch.empty_like(w), torch.empty_like(w), torch.empty(1, dtype=torch.float32, device=w.device)
        object.__setattr__(conv, "_sn_state", st)
    return st


def _sn_convs(mod):
    return [m for m in mod.modules() if hasattr(m, "weight_u")]


def spectral_weights(mod, training):
    """the spectral-norm forward of every such convolution below `mod`: one power iteration each in training (u / v advance in place),
    W / sigma left in the convolution's state.  Runs once per forward of the network, not once per use of a weight."""
    for conv in _sn_convs(mod):
        st = _sn_state(conv)
        ops.spectral_norm(conv.weight_orig, conv.weight_u, conv.weight_v, training, st.w, st.sigma)


def _sp_weight(conv):
    return _sn_state(conv).w if hasattr(conv, "weight_u") else conv.weight


def _sp_param_grads(conv, g, p, k3=True):
    """weight (+ bias) gradient of a block convolution from its output gradient g and its operand p"""
    if conv.bias is not None:
        ops.channel_sum(g, _grad(conv.bias))
    sn = hasattr(conv, "weight_u")
    dw = _sn_state(conv).g if sn else _grad(conv.weight)
    if k3:
        ops.conv3_valid_wgrad(g, p, dw)
    else:
        ops.wgradk(g, p, dw, pad=0)
    if sn:
        st = _sn_state(conv)
        ops.spectral_norm_bwd(st.g, st.w, conv.weight_u, conv.weight_v, st.sigma, _grad(conv.weight_orig))


class SpadeNormCtx:
    __slots__ = ("x", "mean", "rstd", "gamma", "beta", "a_raw", "p_act", "s_pad", "mode", "act", "seg_shape")


def _seg_at(seg, h, w, cache):
    """zero-padded nearest resize of the segmentation map to h x w; one per resolution and network forward (cache)"""
    key = (h, w)
    if cache is not None and key in cache:
        return cache[key]
    s = seg if tuple(seg.shape[2:]) == (h, w) else ops.nearest_resize(seg, (h, w))
    sp = ops.pad_affine(s, (1, 1, 1, 1), 0)
    if cache is not None:
        cache[key] = sp
    return sp


def spade_norm_forward(m, x, seg, act=0, out_pad=0, keep=True, cache=None, training=None):
    """SPADE.forward (normalization.py:98-112) followed by `act` (0 | LRELU).  m: models.networks.SPADE.  Returns (out, ctx);
    out_pad 1: out is the zero-bordered [N,C,H+2,W+2] operand of the next 3x3 convolution."""
    n, c, h, w = x.shape
    training = m.training if training is None else training
    pf = m.param_free_norm
    if pf.kind == "instance":
        a, mode = ops.norm_stats(x, 0), 0
        mean, rstd = a.mean, a.rstd
    elif training:
        # nn.BatchNorm2d counts its batches; SynchronizedBatchNorm2d's single-device path (F.batch_norm) leaves the counter alone
        a, mode = ops.norm_stats(x, 1, running_mean=pf.running_mean, running_var=pf.running_var,
                                 nbt=pf.num_batches_tracked if pf.kind == "batch" else None), 1
        mean, rstd = a.mean, a.rstd
    else:
        mode = 2
        mean, rstd = ops.spade_eval_stats(pf.running_mean, pf.running_var, n)
    s_pad = _seg_at(seg, h, w, cache)
    sh = getattr(m.mlp_shared, "0")
    a_raw = _empty(n, m.NHIDDEN, h, w, x.device)
    ops.conv3_valid(s_pad, sh.weight, sh.bias, a_raw)
    p_act = ops.pad_affine(a_raw, (1, 1, 1, 1), 0, act=RELU)
    gamma, beta = _empty(n, c, h, w, x.device), _empty(n, c, h, w, x.device)
    ops.conv3_valid(p_act, m.mlp_gamma.weight, m.mlp_gamma.bias, gamma)
    ops.conv3_valid(p_act, m.mlp_beta.weight, m.mlp_beta.bias, beta)
    out = ops.spade_modulate(x, mean, rstd, gamma, beta, act=act, out_pad=out_pad)
    if not keep:
        return out, None
    ctx = SpadeNormCtx()
    ctx.x, ctx.mean, ctx.rstd, ctx.gamma, ctx.beta, ctx.a_raw, ctx.p_act, ctx.s_pad = x, mean, rstd, gamma, beta, a_raw, p_act, s_pad
    ctx.mode, ctx.act, ctx.seg_shape = mode, act, tuple(seg.shape)
    return out, ctx


def spade_norm_backward(m, ctx, g, g_pad=0, dsegs=None, want_dseg=True):
    """g: gradient of spade_norm_forward's output (g_pad 1: in the padded layout).  Writes the six parameter gradients, returns
    (dx, dseg).  dsegs: {(h, w): gradient w.r.t. the resized map}, the per-resolution accumulators of a network backward -- with it
    dseg is None and the caller folds the accumulators back to the map's own size once (spade_dseg).  want_dseg False: nobody reads the
    map's gradient (a training step: the sketch is data), so mlp_shared's input adjoint is not run and dseg is None."""
    n, c, h, w = ctx.x.shape
    dgamma, dbeta, dx = ops.spade_modulate_bwd(g, ctx.x, ctx.mean, ctx.rstd, ctx.gamma, ctx.beta, ctx.mode, act=ctx.act, g_pad=g_pad)
    dev = dx.device
    da_sum = _empty(n, m.NHIDDEN, h, w, dev)
    for i, (conv, dmap) in enumerate(((m.mlp_gamma, dgamma), (m.mlp_beta, dbeta))):
        ops.channel_sum(dmap, _grad(conv.bias))
        ops.conv3_valid_wgrad(dmap, ctx.p_act, _grad(conv.weight))
        dp = ops.conv3_valid_adjoint(dmap, conv.weight, _empty(n, m.NHIDDEN, h + 2, w + 2, dev))
        ops.pad_bwd(dp, (1, 1, 1, 1), 0, da_sum, accumulate=i > 0)
    da = _empty(n, m.NHIDDEN, h, w, dev)
    ops.act_bwd(da_sum, ctx.a_raw, RELU, da)
    sh = getattr(m.mlp_shared, "0")
    ops.channel_sum(da, _grad(sh.bias))
    ops.conv3_valid_wgrad(da, ctx.s_pad, _grad(sh.weight))
    if not want_dseg:
        return dx, None
    dsp = ops.conv3_valid_adjoint(da, sh.weight, _empty(n, ctx.seg_shape[1], h + 2, w + 2, dev))
    own = dsegs is None
    if own:
        dsegs = {}
    acc = dsegs.get((h, w))
    if acc is None:
        dsegs[(h, w)] = ops.pad_bwd(dsp, (1, 1, 1, 1), 0, _empty(n, ctx.seg_shape[1], h, w, dev))
    else:
        ops.pad_bwd(dsp, (1, 1, 1, 1), 0, acc, accumulate=True)
    return dx, (spade_dseg(dsegs, ctx.seg_shape, dev) if own else None)


def spade_dseg(dsegs, seg_shape, dev):
    """fold the per-resolution gradients of the resized maps back onto the segmentation map (adjoint of the nearest resizes)"""
    dseg = torch.empty(seg_shape, dtype=torch.float32, device=dev)
    for i, key in enumerate(sorted(dsegs)):
        ops.nearest_resize_bwd(dsegs[key], dseg, accumulate=i > 0)
    return dseg


class SpadeBlockCtx:
    __slots__ = ("n0", "p0", "n1", "p1", "ns", "ps", "x_shape")


def spade_block_forward(blk, x, seg, keep=True, cache=None, weights_ready=False):
    """SPADEResnetBlock.forward (architecture.py:50-68).  weights_ready: the caller already ran spectral_weights for this forward."""
    if not weights_ready:
        spectral_weights(blk, blk.training)
    n, fin, h, w = x.shape
    dev = x.device
    ctx = SpadeBlockCtx()
    ctx.x_shape = tuple(x.shape)
    if blk.learned_shortcut:
        ws = _sp_weight(blk.conv_s)
        ctx.ps, ctx.ns = spade_norm_forward(blk.norm_s, x, seg, act=0, out_pad=0, keep=keep, cache=cache, training=blk.training)
        x_s = ops.convk(ctx.ps, ws, _empty(n, ws.shape[0], h, w, dev), pad=0)
    else:
        x_s = x
    w0, w1 = _sp_weight(blk.conv_0), _sp_weight(blk.conv_1)
    ctx.p0, ctx.n0 = spade_norm_forward(blk.norm_0, x, seg, act=LRELU, out_pad=1, keep=keep, cache=cache, training=blk.training)
    d0 = ops.conv3_valid(ctx.p0, w0, blk.conv_0.bias, _empty(n, w0.shape[0], h, w, dev))
    ctx.p1, ctx.n1 = spade_norm_forward(blk.norm_1, d0, seg, act=LRELU, out_pad=1, keep=keep, cache=cache, training=blk.training)
    d1 = ops.conv3_valid(ctx.p1, w1, blk.conv_1.bias, _empty(n, w1.shape[0], h, w, dev))
    out = ops.pad_affine(d1, (0, 0, 0, 0), 0, res=x_s)
    return out, (ctx if keep else None)


def spade_block_backward(blk, ctx, g, dsegs=None, want_dseg=True):
    """g: gradient of the block's output.  Parameter gradients into .grad (overwritten); returns (dx, dseg) -- dseg and want_dseg as
    spade_norm_backward"""
    g = g.contiguous()
    n, fin, h, w = ctx.x_shape
    dev = g.device
    own = dsegs is None
    if own:
        dsegs = {}
    w0, w1 = _sp_weight(blk.conv_0), _sp_weight(blk.conv_1)
    _sp_param_grads(blk.conv_1, g, ctx.p1)
    dp1 = ops.conv3_valid_adjoint(g, w1, _empty(n, w1.shape[1], h + 2, w + 2, dev))
    dd0, _ = spade_norm_backward(blk.norm_1, ctx.n1, dp1, g_pad=1, dsegs=dsegs, want_dseg=want_dseg)
    _sp_param_grads(blk.conv_0, dd0, ctx.p0)
    dp0 = ops.conv3_valid_adjoint(dd0, w0, _empty(n, fin, h + 2, w + 2, dev))
    dx, _ = spade_norm_backward(blk.norm_0, ctx.n0, dp0, g_pad=1, dsegs=dsegs, want_dseg=want_dseg)
    if blk.learned_shortcut:
        ws = _sp_weight(blk.conv_s)
        _sp_param_grads(blk.conv_s, g, ctx.ps, k3=False)
        dps = ops.convk_bwd_data(g, ws, _empty(n, fin, h, w, dev), pad=0)
        dxs, _ = spade_norm_backward(blk.norm_s, ctx.ns, dps, g_pad=0, dsegs=dsegs, want_dseg=want_dseg)
    else:
        dxs = g
    dx = ops.pad_affine(dx, (0, 0, 0, 0), 0, res=dxs)
    seg_shape = ctx.n0.seg_shape
    return dx, (spade_dseg(dsegs, seg_shape, dev) if own and want_dseg else None)


class SpadeCtx:
    __slots__ = ("seg_shape", "s0_pad", "blocks", "x_last", "p_last", "out")


def _spade_plan(G):
    """(block, upsample in front of it) in forward order behind head_0 (networks.py:2153-2193)"""
    L = G.num_upsampling_layers
    plan = [(G.head_0, 0), (G.G_middle_0, 1), (G.G_middle_1, 1 if L > 5 else 0), (G.up_0, 1), (G.up_1, 1)]
    if L > 3:
        plan.append((G.up_2, 1))
    if L > 4:
        plan.append((G.up_3, 1))
    if L > 6:
        plan.append((G.up_4, 1))
    return plan


def spade_forward(G, seg, keep=True):
    """SPADEGenerator.forward (networks.py:2135-2200) of the segmentation map seg [N, input_nc, H, W] -> ([N, output_nc, H', W'], ctx)"""
    seg = seg.contiguous()
    n, dev = seg.shape[0], seg.device
    spectral_weights(G, G.training)
    cache = {}
    ctx = SpadeCtx()
    ctx.seg_shape = tuple(seg.shape)
    ctx.s0_pad = _seg_at(seg, G.sh, G.sw, cache)
    x = ops.conv3_valid(ctx.s0_pad, G.fc.weight, G.fc.bias, _empty(n, G.fc.weight.shape[0], G.sh, G.sw, dev))
    ctx.blocks = []
    for blk, up in _spade_plan(G):
        if up:
            x = ops.nearest_up2(x)
        x, bctx = spade_block_forward(blk, x, seg, keep=keep, cache=cache, weights_ready=True)
        ctx.blocks.append(bctx)
    ctx.x_last = x
    ctx.p_last = ops.pad_affine(x, (1, 1, 1, 1), 0, act=LRELU)
    out = ops.conv3_valid(ctx.p_last, G.conv_img.weight, G.conv_img.bias, _empty(n, G.conv_img.weight.shape[0], x.shape[2], x.shape[3], dev), act_out=TANH)
    ctx.out = out
    return out, (ctx if keep else None)


def spade_backward(G, ctx, dout, want_dseg=True, pre_tanh=False):
    """dout: gradient of the generator's (post-tanh) output.  Every parameter's .grad is overwritten; returns dseg.  want_dseg False: everything
    that only serves the map's gradient is skipped (the input adjoints of every mlp_shared and of fc, the per-resolution accumulators, their
    fold) and None is returned; the parameter gradients are the same launches on the same operands.  pre_tanh: dout is already the
    gradient of the image head's PRE-tanh output (ops.g_out_grad folds the mask multiply and the tanh adjoint into one pass)."""
    dev = dout.device
    n = dout.shape[0]
    x = ctx.x_last
    dz = dout.contiguous() if pre_tanh else ops.tanh_bwd(dout.contiguous(), ctx.out)
    ops.channel_sum(dz, _grad(G.conv_img.bias))
    ops.conv3_valid_wgrad(dz, ctx.p_last, _grad(G.conv_img.weight))
    dp = ops.conv3_valid_adjoint(dz, G.conv_img.weight, _empty(n, x.shape[1], x.shape[2] + 2, x.shape[3] + 2, dev))
    gc = ops.pad_bwd(dp, (1, 1, 1, 1), 0, torch.empty_like(x))
    g = ops.act_bwd(gc, x, LRELU, torch.empty_like(x))
    dsegs = {}
    for (blk, up), bctx in zip(reversed(_spade_plan(G)), reversed(ctx.blocks)):
        g, _ = spade_block_backward(blk, bctx, g, dsegs=dsegs, want_dseg=want_dseg)
        if up:
            g = ops.nearest_up2_bwd(g)
    ops.channel_sum(g, _grad(G.fc.bias))
    ops.conv3_valid_wgrad(g, ctx.s0_pad, _grad(G.fc.weight))
    if not want_dseg:
        return None
    ds0 = ops.conv3_valid_adjoint(g, G.fc.weight, _empty(n, ctx.seg_shape[1], G.sh + 2, G.sw + 2, dev))
    acc = dsegs.get((G.sh, G.sw))
    if acc is None:
        dsegs[(G.sh, G.sw)] = ops.pad_bwd(ds0, (1, 1, 1, 1), 0, _empty(n, ctx.seg_shape[1], G.sh, G.sw, dev))
    else:
        ops.pad_bwd(ds0, (1, 1, 1, 1), 0, acc, accumulate=True)
    return spade_dseg(dsegs, ctx.seg_shape, dev)
