"""The ResNet-family generators and the SPADE generator launch what they launched before their layers were paired on named records.

One forward + backward of six small configurations that between them reach every arm of `engine._seq_forward / _seq_backward` and of the
shared 3x3 dispatch (`ops.conv3_valid` and its adjoint / weight gradient).  Every `ops._run` label is recorded; behind a launch of the
conv / wgrad families the kernel instance that `vts_last_kernel()` reports is recorded with it.  The run-length-coded sequences must equal
`tests/golden/resnet_schedule.json`, which the same recorder (`record`) wrote on the parent of the commit that introduced the records."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
FAMILIES = ("conv4x4", "wgrad4x4", "conv3x3_wide", "wgrad3x3_wide")     # labels whose kernel instance is taken too


def _seed_params(G, seed):
    """seeded weights (only launches are compared: any finite values do); BatchNorm scales around 1"""
    gen = torch.Generator().manual_seed(seed)
    for k, p in G.named_parameters():
        v = torch.randn(p.shape, generator=gen) * 0.1
        p.data.copy_(1.0 + v if p.dim() == 1 and k.endswith(".weight") else v)
    return G


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0


def _resnet(seed, size, **kw):
    from models import networks
    from vts.optim import FlatParams

    torch.manual_seed(seed)
    G = _seed_params(networks.ResnetGenerator(3, 5, **kw), seed).to(DEV).train()
    return G, FlatParams(G), _rand(size, seed + 1).to(DEV)


def _backward_whole(G, ctx, d_raw):
    from vts import engine

    engine.resnet_backward(G, ctx, d_raw)


def _resnet_run(G, x, masks=None, backward=_backward_whole):
    from vts import engine

    y, ctx = engine.resnet_forward(G, x, dropout_masks=masks)
    backward(G, ctx, (_rand(tuple(y.shape), 5).to(DEV) * (1.0 - y * y)).contiguous())
    return y


STRIDED = dict(norm="batch", down="stride", up="convT")


def _reference_defaults():
    """InstanceNorm, reflect padding, blur down / up, Dropout with given masks: narrow conv7, conv3 s1, down, up, block, conv7_out"""
    G, flat, x = _resnet(31, (1, 3, 64, 64), ngf=8, n_blocks=2, use_dropout=True)
    masks = [(_rand((1, 32, 16, 16), 40 + i) > 0).float() for i in range(2)]
    return G, lambda: _resnet_run(G, x, masks)


def _strided_wide():
    """the network of test_resnet_generator_strided_variants_wide (48 -> 96 -> 192 channels): narrow and wide stride-2 conv3, wide and
    narrow convT3, wide direct blocks"""
    G, flat, x = _resnet(17, (1, 3, 24, 40), ngf=48, n_blocks=2, n_downsampling=2, **STRIDED)
    return G, lambda: _resnet_run(G, x)


def _winograd():
    """64-channel blocks on 128 x 128 maps, N 4: the Winograd arms of the block forward and of both input adjoints"""
    from vts import ops

    # forward: 64 x 64 tiles of 2 x 2 outputs over 128 x 128; adjoint: the same on the 130 x 130 padded gradient
    assert ops.conv3x3_wino_ok(4, 64, 64, 128, 128) and ops.conv3x3_wino_ok(4, 64, 64, 130, 130)
    G, flat, x = _resnet(23, (4, 3, 512, 512), ngf=16, n_blocks=1, n_downsampling=2, **STRIDED)
    return G, lambda: _resnet_run(G, x)


def _local_enhancer():
    from models import networks
    from vts.optim import FlatParams

    g = np.load(os.path.join(GOLDEN, "local_64x32.npz"), allow_pickle=False)
    h, w, ngf, nd, nbg, nbl = (int(g[k]) for k in ("h", "w", "ngf", "n_down", "n_blocks_global", "n_blocks_local"))
    nl = int(g["n_local"]) if "n_local" in g.files else 1
    G = networks.LocalEnhancer(1, 5, ngf=ngf, n_downsample_global=nd, n_blocks_global=nbg, n_local_enhancers=nl, n_blocks_local=nbl)
    G = _seed_params(G, 61).to(DEV).train()
    flat = FlatParams(G)
    x = _rand((2, 1, h, w), 62).to(DEV)
    return G, lambda: _resnet_run(G, x)


def _staged():
    """configuration _strided_wide, its backward as resnet_backward_stage chained over resnet_stage_bounds: one cut inside the first
    block (at its second convolution), one at the first transposed convolution"""
    from vts import engine

    G, flat, x = _resnet(17, (1, 3, 24, 40), ngf=48, n_blocks=2, n_downsampling=2, **STRIDED)
    blk = next(e["idx"] for e in G.layout if e["kind"] == "block")
    up = next(e["idx"] for e in G.layout if e["kind"] == "convT3")
    cuts = [G.block_mods(blk)[2].weight, G.mod(up).weight]

    def backward(G, ctx, g):
        b = engine.resnet_stage_bounds(ctx, cuts)
        assert len(b) == 4 and b[0] < b[1] < b[2] < b[3], b
        for j in range(len(b) - 2, -1, -1):
            g = engine.resnet_backward_stage(G, ctx, g, b[j], b[j + 1])

    return G, lambda: _resnet_run(G, x, backward=backward)


def _spade():
    """the `g8` generator case of spade_32.npz's table (spectral norm on; 128 -> 64 -> 32 channels, label_nc 1: convolutions on both
    sides of the 64 x 64-channel threshold)"""
    import spade_restated as R
    from models import networks
    from vts import engine
    from vts.optim import FlatParams

    c = R.GEN_CASES["g8"]
    torch.manual_seed(81)      # the spectral-norm vectors are drawn at construction
    G = networks.define_G(c["input_nc"], c["output_nc"], c["ngf"], "spade", norm=c["normG"], opt=R.gen_opt("g8"), gpu_ids=[0])
    _seed_params(G, 82).train()
    flat = FlatParams(G)
    h, w = R.gen_out_hw(c)
    seg, cot = _rand((c["N"], c["input_nc"], h, w), 83).to(DEV), _rand((c["N"], c["output_nc"], h, w), 84).to(DEV)

    def run():
        out, ctx = engine.spade_forward(G, seg)
        engine.spade_backward(G, ctx, cot)
        return out

    return G, run


CONFIGS = {"reference_defaults": _reference_defaults, "strided_wide": _strided_wide, "winograd": _winograd,
           "local_enhancer": _local_enhancer, "staged_backward": _staged, "spade": _spade}


def record(name):
    """run configuration `name` once with every ops._run label recorded -> (run-length-coded text, output, network)"""
    from vts import lib as L
    from vts import ops

    G, run = CONFIGS[name]()
    labels = []
    orig = ops._run

    def rec(label, *a):
        r = orig(label, *a)
        labels.append(label + "|" + L.load().vts_last_kernel().decode().replace(" ", "") if label.startswith(FAMILIES) else label)
        return r

    ops._run = rec
    try:
        out = run()
        torch.cuda.synchronize()
    finally:
        ops._run = orig
    rle = []
    for lab in labels:
        if rle and rle[-1][0] == lab:
            rle[-1][1] += 1
        else:
            rle.append([lab, 1])
    return " ".join(lab if c == 1 else "%s*%d" % (lab, c) for lab, c in rle), out, G


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLDEN, "resnet_schedule.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_launches_the_parents_sequence(parent, name):
    got = record(name)[0].split()
    want = parent[name].split()
    print(name, len(got), "runs of launches")
    if name == "winograd":
        assert sum("wino" in t and t.startswith("conv3x3_wide|") for t in got) >= 4       # two forward, two adjoint launches
    if name == "spade":
        assert not any(t.startswith("w3x3_wino_pack") for t in got)
        assert any(t.startswith("conv3x3_wide|") for t in got) and any(t.startswith("tap_embed") for t in got)
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, ("first difference at run %d" % first, got[first:first + 3], want[first:first + 3])


def test_staged_backward_launches_what_the_whole_backward_launches(parent):
    """cutting the backward into stages joins the side queue per stage and changes no launch"""
    assert parent["staged_backward"] == parent["strided_wide"]
