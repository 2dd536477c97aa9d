"""ResNet generator (--netG resnet_{4,6,9}blocks) on the HIP path: operator parity against plain PyTorch
fp32 CPU evaluations, and network forward / backward parity against the CPU oracle (which is pinned to the
reference module by tests/golden/resnet_64.npz) and against the committed reference outputs themselves.
Tolerances: rel-L2 <= 1e-5 per operator, 2e-4 for whole-network gradients (fp32, different summation order)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import detrand, nets  # noqa: E402  (checker only)


def _dev():
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _affine(n, c, seed, name):
    return 1.0 + 0.3 * detrand.uniform((n * c,), seed, name + "sc"), 0.2 * detrand.uniform((n * c,), seed, name + "sh")


def _apply(x, sc, sh, act):
    n, c = x.shape[:2]
    v = x * sc.view(n, c, 1, 1) + sh.view(n, c, 1, 1)
    return {0: v, 1: F.leaky_relu(v, 0.2), 2: F.relu(v), 3: torch.tanh(v)}[act]


@pytest.mark.parametrize("K,pad,shape", [(3, 1, (2, 10, 20, 37, 41)), (3, 0, (1, 40, 40, 30, 30)), (7, 0, (2, 9, 10, 38, 70)),
                                         (7, 3, (1, 10, 5, 33, 64)), (3, 1, (1, 20, 10, 128, 128))])
def test_convk_forward_backward_wgrad(K, pad, shape):
    """K x K stride-1 convolution as 4x4 tap blocks: forward, adjoint w.r.t. the input, weight gradient."""
    from vts import ops
    from vts.ops import Act
    n, ci, co, h, w = shape
    dev = _dev()
    x = detrand.uniform((n, ci, h, w), 5, "x")
    sc, sh = _affine(n, ci, 5, "a")
    wt = detrand.uniform((co, ci, K, K), 5, "w") * 0.2
    b = detrand.uniform((co,), 5, "b")
    xa = _apply(x, sc, sh, 2).requires_grad_(True)
    wr = wt.clone().requires_grad_(True)
    ref = F.conv2d(xa, wr, b, padding=pad)
    cot = detrand.uniform(tuple(ref.shape), 5, "cot")
    (ref * cot).sum().backward()

    out = torch.full(ref.shape, float("nan"), device=dev)
    ops.convk(Act(x.to(dev), sc.to(dev), sh.to(dev)), wt.to(dev), out, bias=b.to(dev), pad=pad, act_in=2)
    assert rel(out, ref) < 1e-5
    din = torch.full(x.shape, float("nan"), device=dev)
    ops.convk_bwd_data(cot.to(dev), wt.to(dev), din, pad=pad)
    assert rel(din, xa.grad) < 1e-5
    dw = torch.full(wt.shape, float("nan"), device=dev)
    ops.wgradk(cot.to(dev), Act(x.to(dev), sc.to(dev), sh.to(dev)), dw, pad=pad, act_hi=2)
    assert rel(dw, wr.grad) < 2e-5
    dw2 = dw.clone()
    ops.wgradk(cot.to(dev), Act(x.to(dev), sc.to(dev), sh.to(dev)), dw2, pad=pad, act_hi=2, accumulate=True)
    assert rel(dw2, 2 * wr.grad) < 2e-5


@pytest.mark.parametrize("mode,pads", [(1, (3, 3, 3, 3)), (1, (1, 1, 1, 1)), (2, (1, 1, 1, 1)), (0, (2, 1, 0, 3)), (1, (2, 0, 1, 3))])
@pytest.mark.parametrize("shape", [(2, 5, 17, 23), (1, 3, 64, 70)])
def test_pad_affine_and_adjoint(mode, pads, shape):
    from vts import ops
    from vts.ops import Act
    n, c, h, w = shape
    dev = _dev()
    pt, pb, pl, pr = pads
    x = detrand.uniform(shape, 7, "x")
    sc, sh = _affine(n, c, 7, "a")
    xa = _apply(x, sc, sh, 2).requires_grad_(True)
    ref = F.pad(xa, (pl, pr, pt, pb), mode={0: "constant", 1: "reflect", 2: "replicate"}[mode])
    res = detrand.uniform(tuple(ref.shape), 7, "res")
    out = ops.pad_affine(Act(x.to(dev), sc.to(dev), sh.to(dev)), pads, mode, act=2, res=res.to(dev))
    assert rel(out, ref + res) < 1e-6
    cot = detrand.uniform(tuple(ref.shape), 7, "cot")
    (ref * cot).sum().backward()
    din = torch.full(shape, float("nan"), device=dev)
    ops.pad_bwd(cot.to(dev), pads, mode, din)
    assert rel(din, xa.grad) < 1e-6
    ops.pad_bwd(cot.to(dev), pads, mode, din, accumulate=True)
    assert rel(din, 2 * xa.grad) < 1e-6


def test_pad_affine_concat_on_store_and_tanh():
    from vts import ops
    dev = _dev()
    a, b = detrand.uniform((2, 1, 20, 24), 8, "a"), detrand.uniform((2, 8, 20, 24), 8, "b")
    p = torch.full((2, 9, 26, 30), float("nan"), device=dev)
    ops.pad_affine(a.to(dev), (3, 3, 3, 3), 1, out=p[:, 0:1], out_nstride=p.stride(0))
    ops.pad_affine(b.to(dev), (3, 3, 3, 3), 1, out=p[:, 1:9], out_nstride=p.stride(0))
    assert rel(p, F.pad(torch.cat([a, b], 1), (3, 3, 3, 3), mode="reflect")) < 1e-7
    t = ops.pad_affine(b.to(dev), (0, 0, 0, 0), 0, act=3)
    assert rel(t, torch.tanh(b)) < 1e-6


@pytest.mark.parametrize("shape", [(2, 6, 32, 32), (1, 3, 17, 21), (1, 4, 64, 50), (2, 2, 2, 2)])
def test_blur_down_up_and_adjoints(shape):
    """Downsample / Upsample of the reference (oracle.nets.blur_down / blur_up restate them)."""
    from vts import ops
    from vts.ops import Act
    n, c, h, w = shape
    dev = _dev()
    x = detrand.uniform(shape, 9, "x")
    sc, sh = _affine(n, c, 9, "a")
    for name, fwd, bwd, oracle_fn in (("down", ops.blur_down, ops.blur_down_bwd, nets.blur_down), ("up", ops.blur_up, ops.blur_up_bwd, nets.blur_up)):
        xa = _apply(x, sc, sh, 2).requires_grad_(True)
        ref = oracle_fn(xa)
        out = fwd(Act(x.to(dev), sc.to(dev), sh.to(dev)), act=2)
        assert out.shape == ref.shape, name
        assert rel(out, ref) < 1e-6, name
        cot = detrand.uniform(tuple(ref.shape), 9, "cot" + name)
        (ref * cot).sum().backward()
        din = torch.full(shape, float("nan"), device=dev)
        bwd(cot.to(dev), din)
        assert rel(din, xa.grad) < 1e-6, name
        bwd(cot.to(dev), din, accumulate=True)
        assert rel(din, 2 * xa.grad) < 1e-6, name


def _build_G(nb, ngf, seed, dev):
    from models import networks
    from vts.optim import FlatParams
    G = networks.ResnetGenerator(9, 5, ngf=ngf, n_blocks=nb).to(dev)
    sd = detrand.test_weights(nets.resnet_param_shapes(9, 5, ngf, nb), seed)
    G.load_state_dict(sd, strict=False)
    flat = FlatParams(G)
    return G, flat, sd


def test_resnet_generator_matches_reference_and_oracle(golden_dir):
    """forward vs the committed reference output; backward vs oracle autograd on the same weights / cotangent"""
    from vts import engine
    g = np.load(os.path.join(golden_dir, "resnet_64.npz"), allow_pickle=False)
    size, seed, nb, ngf = int(g["size"]), int(g["seed"]), int(g["n_blocks"]), int(g["ngf"])
    dev = _dev()
    G, flat, sd = _build_G(nb, ngf, seed, dev)
    x = detrand.uniform((2, 9, size, size), seed, "g_in")
    y, ctx = engine.resnet_forward(G, (x[:, :1].contiguous().to(dev), x[:, 1:].contiguous().to(dev)))
    assert rel(y, torch.from_numpy(g["G_out"])) < 2e-5
    # oracle autograd
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    yo = nets.resnet_forward(sdo, x, nb)
    cot = detrand.uniform(tuple(yo.shape), seed, "g_cot")
    (yo * cot).sum().backward()
    d_raw = (cot.to(dev) * (1.0 - y * y)).contiguous()     # through the tanh
    flat.grad.zero_()
    engine.resnet_backward(G, ctx, d_raw)
    named = dict(G.named_parameters())
    last_bias = "model.%d.bias" % max(int(k.split(".")[1]) for k in sdo)
    for k, v in sdo.items():
        ref = v.grad
        got = named[k].grad
        if k.endswith(".bias") and k != last_bias:
            assert ref.norm() < 2e-3                       # autograd: rounding noise around 0
            assert got.abs().max().item() == 0.0, k        # bias in front of an InstanceNorm: exactly zero here
            continue
        assert rel(got, ref) < 2e-4, (k, rel(got, ref))
        p = detrand.probe(got.cpu(), k)
        rp = g["G_grad/" + k]
        assert abs(p[1] - rp[1]) <= 5e-4 * max(abs(rp[1]), 1e-12), (k, p, rp)


def test_resnet_inference_forward_odd_size():
    """sizes that are not multiples of the tile shapes; 6-block variant"""
    from vts import engine
    dev = _dev()
    G, _, sd = _build_G(6, 8, 11, dev)
    x = detrand.uniform((1, 9, 52, 76), 11, "x")
    y, _ = engine.resnet_forward(G, x.to(dev), keep=False)
    yo = nets.resnet_forward(sd, x, 6)
    assert rel(y, yo) < 2e-5


def test_train_step_with_resnet_generator_matches_oracle():
    """sinskitG step through create_model with --netG resnet_6blocks vs the CPU oracle step (same nets, same draws)"""
    import random

    from torch.utils.data import default_collate

    from data.synthetic_dataset import make_sample
    from models import create_model
    from options.train_options import TrainOptions
    from oracle import step

    size, nt, seed, nb = 128, 64, 41, 6
    flags = ("--model sinskitG --gpu_ids 0 --lambda_G1_lpips 0 --lambda_G2_lpips 0 --use_vision_aided_loss False "
             "--lambda_G2_GAN_feat 0 --checkpoints_dir /tmp/vts_test_ckpt --name tr --crop_size %d --batch_size 1 "
             "--netG resnet_%dblocks" % (size, nb))
    opt = TrainOptions(cmd_line=flags).parse()
    model = create_model(opt)
    model.setup(opt)
    model.parallelize()
    model.train()
    sdG = detrand.test_weights(nets.resnet_param_shapes(9, 5, opt.ngf, nb), seed)
    sdD, sdD2 = detrand.test_weights(nets.d_param_shapes(4), seed + 1), detrand.test_weights(nets.d_param_shapes(7), seed + 2)
    model.netG.load_state_dict(sdG, strict=False)
    model.netD.load_state_dict(sdD)
    model.netD2.load_state_dict(sdD2)
    batch = default_collate([make_sample(size, nt, nt, seed)])
    random.seed(5)
    cnt = int(nets.dilated_mask_positions(batch["M"].float()).shape[0])
    draws = {"aug": detrand.uniform((4, 1), 3, "aug") * 0.5 + 0.5, "more_idx": torch.tensor([random.sample(range(cnt), 32)])}
    adam = {k: step.new_adam_state() for k in ("G", "D", "D2")}
    ref = step.train_step(sdG, sdD, sdD2, adam, batch, draws, opt=step.hp(netG="resnet_%dblocks" % nb))
    model._draws = draws
    model.set_input(batch, phase="train")
    model.optimize_parameters(epoch=1)
    losses = model.get_current_losses()
    for k, v in ref["losses"].items():
        assert abs(losses["l_" + k] - v) <= 1e-3 * max(1.0, abs(v)), (k, losses["l_" + k], v)
    assert rel(model.fake_I, ref["fake_I"]) < 1e-3 and rel(model.fake_T, ref["fake_T"]) < 1e-3
    last_bias = "model.%d.bias" % max(int(k.split(".")[1]) for k in sdG)
    for k, p in model.netG.named_parameters():
        if k.endswith(".bias") and k != last_bias:
            continue
        assert rel(p.grad, ref["grad_G"][k]) < 2e-3, k
    # the step also runs captured (HIP graph) and keeps training: losses stay finite and weights move
    model._draws = None
    w0 = model.flatG.flat.clone()
    for _ in range(3):
        model.set_input(batch, phase="train")
        model.optimize_parameters(epoch=1)
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in model.get_current_losses().values())
    assert (model.flatG.flat - w0).abs().max().item() > 0


def _check_param_grads(G, sdo, norm_bias_zero=True):
    named = dict(G.named_parameters())
    last_bias = "model.%d.bias" % max(int(k.split(".")[1]) for k in sdo)
    for k, v in sdo.items():
        if not (v.dtype.is_floating_point and v.requires_grad):
            continue
        ref, got = v.grad, named[k].grad
        is_conv_bias = k.endswith(".bias") and k != last_bias and k.replace(".bias", ".weight") in sdo and sdo[k.replace(".bias", ".weight")].dim() == 4
        if is_conv_bias:
            assert ref.norm() < 5e-3, k                    # autograd: rounding noise around 0
            assert got.abs().max().item() == 0.0, k        # here: exactly zero (the normalisation removes it)
            continue
        assert rel(got, ref) < 3e-4, (k, rel(got, ref))


def test_global_generator_matches_reference_and_oracle(golden_dir):
    """pix2pixHD GlobalGenerator (BatchNorm train mode, stride-2 3x3 convs, ConvTranspose2d): forward vs the committed
    reference output, BN running statistics, backward vs oracle autograd"""
    from models import networks
    from vts import engine
    from vts.optim import FlatParams
    g = np.load(os.path.join(golden_dir, "global_64x32.npz"), allow_pickle=False)
    h, w, seed, ngf, nd, nb = (int(g[k]) for k in ("h", "w", "seed", "ngf", "n_down", "n_blocks"))
    dev = _dev()
    shapes = nets.resnet_param_shapes(1, 5, ngf, nb, nd, norm="batch", down="stride", up="convT", conv_bias=True)
    sd = detrand.test_weights(shapes, seed)
    G = networks.GlobalGenerator(1, 5, ngf=ngf, n_downsampling=nd, n_blocks=nb).to(dev)
    G.load_state_dict(sd)
    flat = FlatParams(G)
    G.train()
    x = detrand.uniform((2, 1, h, w), seed, "g_in")
    y, ctx = engine.resnet_forward(G, x.to(dev))
    assert rel(y, torch.from_numpy(g["G_out"])) < 5e-5
    for k, b in G.named_buffers():
        if b.dtype.is_floating_point:
            assert rel(b, torch.from_numpy(g["G_buf/" + k])) < 1e-4, k
    sdo = {k: v.clone() for k, v in sd.items()}
    for k, v in sdo.items():
        if v.dtype.is_floating_point and "running" not in k:
            v.requires_grad_(True)
    yo = nets.resnet_forward(sdo, x, nb, nd, norm="batch", down="stride", up="convT", training=True)
    cot = detrand.uniform(tuple(yo.shape), seed, "g_cot")
    (yo * cot).sum().backward()
    flat.grad.zero_()
    engine.resnet_backward(G, ctx, (cot.to(dev) * (1.0 - y * y)).contiguous())
    _check_param_grads(G, sdo)
    # eval mode uses the running statistics
    G.eval()
    ye, _ = engine.resnet_forward(G, x.to(dev), keep=False)
    sde = {k: v.detach() for k, v in sdo.items()}
    assert rel(ye, nets.resnet_forward(sde, x, nb, nd, norm="batch", down="stride", up="convT", training=False)) < 5e-5


def test_global_generator_default_size_matches_oracle_at_512x256():
    """the REAL pix2pixHD GlobalGenerator (ngf 64, 4 downsamplings to 1024 channels, 9 blocks: 182.5 M parameters) on a 512 x 256
    image: forward and every parameter gradient against the CPU oracle evaluated in FLOAT64 (GEMM-class 3x3 kernels on full-size maps,
    BatchNorm train).  At this depth (45 layers of 9216-term dot products) two fp32 implementations drift apart by a few 1e-3 in the
    gradient -- the fp32 oracle itself is that far from its float64 evaluation -- so the judge here is float64: the HIP path must
    not be further from it than twice the fp32 oracle's own distance."""
    from models import networks
    from vts import engine
    from vts.optim import FlatParams
    dev = _dev()
    ngf, nd, nb, seed, h, w = 64, 4, 9, 29, 256, 512
    shapes = nets.resnet_param_shapes(1, 5, ngf, nb, nd, norm="batch", down="stride", up="convT", conv_bias=True)
    sd = detrand.test_weights(shapes, seed)
    # keep the output tanh out of saturation: with O(0.1) random weights the 64 x 49-term output conv gives |y| ~ 1 and the tanh
    # derivative 1 - y^2 cancels catastrophically in fp32 (in ANY implementation) -- that would measure the test, not the kernels
    last = [k for k, v in sd.items() if v.ndim == 4 and v.shape[0] == 5][-1]
    sd[last] = sd[last] * 0.02
    G = networks.GlobalGenerator(1, 5, ngf=ngf, n_downsampling=nd, n_blocks=nb).to(dev)
    G.load_state_dict(sd)
    flat = FlatParams(G)
    assert flat.numel > 182e6
    G.train()
    x = detrand.uniform((1, 1, h, w), seed, "g_in")
    y, ctx = engine.resnet_forward(G, x.to(dev))
    cot = None
    res = {}
    for dt in (torch.float64, torch.float32):
        sdo = {k: (v.clone().to(dt) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
        for k, v in sdo.items():
            if v.dtype.is_floating_point and "running" not in k:
                v.requires_grad_(True)
        yo = nets.resnet_forward(sdo, x.to(dt), nb, nd, norm="batch", down="stride", up="convT", training=True)
        if cot is None:
            cot = detrand.uniform(tuple(yo.shape), seed, "g_cot")
        (yo * cot.to(dt)).sum().backward()
        res[dt] = (yo.detach(), {k: v.grad for k, v in sdo.items() if v.requires_grad})
    y64, g64 = res[torch.float64]
    y32, g32 = res[torch.float32]
    assert rel(y, y64) < 1e-3
    flat.grad.zero_()
    engine.resnet_backward(G, ctx, (cot.to(dev) * (1.0 - y * y)).contiguous())
    ours, cpu32 = [], []
    for k, p in G.named_parameters():
        ref = g64[k]
        if k.endswith("bias") and p.grad.abs().max().item() == 0.0 and ref.norm() < 1e-6 * max(1.0, float(g64[k.replace("bias", "weight")].norm())):
            continue      # conv bias in front of a BatchNorm: mathematically zero (exactly zero here, ~1e-12 in float64)
        ours.append((rel(p.grad, ref), k))
        cpu32.append(rel(g32[k], ref))
    ours.sort(reverse=True)
    print("GlobalGenerator 512x256 vs float64: forward HIP %.2e / CPU fp32 %.2e; gradient worst HIP %.2e (%s) / CPU fp32 %.2e" % (
        rel(y, y64), rel(y32, y64), ours[0][0], ours[0][1], max(cpu32)))
    # measured: HIP 4.0e-3, PyTorch-CPU fp32 2.8e-3 (worst parameter, both against float64; forward 1e-6 both): the gradient of this
    # 45-layer batch-1 BatchNorm stack is conditioned that way in fp32 -- the bar is "fp32 class": within 2x of PyTorch's own fp32 error
    assert ours[0][0] < 8e-3 and ours[0][0] < 2 * max(max(cpu32), 5e-4), ours[:5]


def test_global_generator_2048x1024_forward_properties():
    """BASELINE config 3's image size (2048 x 1024), forward in eval mode (running statistics = identity normalisation here), properties
    that need no oracle: the map is translation-covariant for shifts by the total stride (16 px) away from the reflect-padded borders,
    finite, inside tanh's range, and deterministic"""
    from models import networks
    from vts import engine
    dev = _dev()
    G = networks.GlobalGenerator(1, 5, ngf=64, n_downsampling=4, n_blocks=9).to(dev)
    G.load_state_dict(detrand.test_weights(nets.resnet_param_shapes(1, 5, 64, 9, 4, norm="batch", down="stride", up="convT", conv_bias=True), 31))
    G.eval()
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(1, 1, 1024, 2048, generator=g) * 2 - 1).to(dev)
    y, _ = engine.resnet_forward(G, x, keep=False)
    y2, _ = engine.resnet_forward(G, x, keep=False)
    assert torch.equal(y, y2) and torch.isfinite(y).all() and float(y.abs().max()) <= 1.0 and y.shape == (1, 5, 1024, 2048)
    xs = torch.roll(x, shifts=(16, 32), dims=(2, 3))
    ys, _ = engine.resnet_forward(G, xs, keep=False)
    m = 400       # receptive field of the stack from the borders / the wrap-around seam of the roll
    assert rel(ys[:, :, m + 16:-m, m + 32:-m], y[:, :, m:-m - 16, m:-m - 32]) < 1e-4


def test_resnet_generator_strided_variants_wide():
    """--no_antialias / --no_antialias_up ResnetGenerator with BatchNorm (no conv biases) and > 80 channels
    (the output-channel group loop of vts_conv4x4)"""
    from models import networks
    from vts import engine
    from vts.optim import FlatParams
    dev = _dev()
    ngf, nb, nd, seed = 48, 2, 2, 17          # 48 -> 96 -> 192 channels
    shapes = nets.resnet_param_shapes(3, 5, ngf, nb, nd, norm="batch", down="stride", up="convT")
    sd = detrand.test_weights(shapes, seed)
    G = networks.ResnetGenerator(3, 5, ngf=ngf, n_blocks=nb, n_downsampling=nd, norm="batch", down="stride", up="convT").to(dev)
    assert sorted(G.state_dict().keys()) == sorted(sd.keys())
    G.load_state_dict(sd)
    flat = FlatParams(G)
    G.train()
    x = detrand.uniform((1, 3, 24, 40), seed, "x")
    y, ctx = engine.resnet_forward(G, x.to(dev))
    sdo = {k: v.clone() for k, v in sd.items()}
    for k, v in sdo.items():
        if v.dtype.is_floating_point and "running" not in k:
            v.requires_grad_(True)
    yo = nets.resnet_forward(sdo, x, nb, nd, norm="batch", down="stride", up="convT", training=True)
    assert rel(y, yo) < 5e-5
    cot = detrand.uniform(tuple(yo.shape), seed, "cot")
    (yo * cot).sum().backward()
    flat.grad.zero_()
    engine.resnet_backward(G, ctx, (cot.to(dev) * (1.0 - y * y)).contiguous())
    _check_param_grads(G, sdo)


# maps of <= 128 pixels take the flattened-batch variants (several whole images per pixel tile, k-split)
FLAT_SHAPES = [(32, 64, 128, 2, 2), (5, 132, 68, 4, 4), (7, 40, 64, 3, 5), (3, 72, 136, 8, 8), (2, 36, 132, 9, 11), (33, 256, 128, 1, 1)]


# widths just above a multiple of 32 (64 .. 94): the row-run kernel (runs of 128 flattened pixels)
ROWRUN_SHAPES = [(2, 64, 128, 66, 66), (1, 72, 132, 19, 70), (3, 16, 8, 5, 65), (1, 128, 64, 130, 66), (2, 8, 4, 33, 94), (1, 64, 64, 66, 130), (1, 16, 8, 7, 134), (2, 8, 8, 9, 106)]


@pytest.mark.parametrize("shape", [(1, 64, 128, 16, 32), (2, 20, 132, 9, 37), (1, 256, 256, 8, 64), (1, 8, 4, 5, 5)] + FLAT_SHAPES + ROWRUN_SHAPES)
def test_conv3x3_wide_forward_and_input_adjoint(shape):
    """GEMM-class 3x3 kernel vs F.conv2d on the padded input; the adjoint through the flipped / transposed packing"""
    from vts import ops
    n, ci, co, h, w = shape
    dev = _dev()
    p = detrand.uniform((n, ci, h + 2, w + 2), 21, "p").requires_grad_(True)
    wt = (detrand.uniform((co, ci, 3, 3), 21, "w") * float(np.sqrt(3.0 / (9 * ci)))).requires_grad_(True)
    b = detrand.uniform((co,), 21, "b")
    ref = F.conv2d(p, wt, b)
    cot = detrand.uniform(tuple(ref.shape), 21, "cot")
    (ref * cot).sum().backward()
    out = torch.full(ref.shape, float("nan"), device=dev)
    wd = wt.detach().to(dev)
    ops.conv3x3_wide(p.detach().to(dev), ops.w3x3_pack(wd, "conv_fwd"), b.to(dev), out)
    assert rel(out, ref) < 1e-5
    if ci % 4 == 0:
        q = ops.pad_affine(cot.to(dev), (2, 2, 2, 2), 0)
        dp = torch.full(p.shape, float("nan"), device=dev)
        ops.conv3x3_wide(q, ops.w3x3_pack(wd, "conv_adj"), None, dp)
        assert rel(dp, p.grad) < 1e-5


def test_conv3x3_wide_ksplit_small_map():
    """few tiles: a k-split path with its deterministic reduction.  8 x 16 = 128 pixels is a flat map, so this is the flattened kernel's
    k-split (16 slices); the tiled kernels' k-split is judged in tests/test_wide_family_gpu.py"""
    from vts import lib as L
    from vts import ops
    dev = _dev()
    n, ci, co, h, w = 1, 256, 128, 8, 16
    p = detrand.uniform((n, ci, h + 2, w + 2), 22, "p")
    wt = detrand.uniform((co, ci, 3, 3), 22, "w") * float(np.sqrt(3.0 / (9 * ci)))
    b = detrand.uniform((co,), 22, "b")
    out = torch.full((n, co, h, w), float("nan"), device=dev)
    ops.conv3x3_wide(p.to(dev), ops.w3x3_pack(wt.to(dev), "conv_fwd"), b.to(dev), out)
    assert L.load().vts_last_kernel().decode() == "conv_flat_kernel<8, 9>+ksplit"
    assert rel(out, F.conv2d(p, wt, b)) < 1e-5
    out2 = torch.empty_like(out)
    ops.conv3x3_wide(p.to(dev), ops.w3x3_pack(wt.to(dev), "conv_fwd"), b.to(dev), out2)
    assert torch.equal(out, out2)          # deterministic


@pytest.mark.parametrize("shape", [(1, 64, 128, 16, 32), (2, 70, 132, 9, 37), (1, 256, 64, 8, 64), (3, 8, 4, 5, 5), (32, 64, 128, 2, 2),
                                   (5, 70, 132, 4, 4), (9, 136, 72, 3, 5), (2, 64, 64, 8, 8), (33, 130, 64, 1, 1), (32, 1024, 512, 2, 2), (2, 128, 192, 40, 56), (3, 72, 64, 33, 17)])
def test_wgrad3x3_wide(shape):
    """GEMM-class weight gradient vs autograd; accumulate; run-to-run determinism"""
    from vts import ops
    n, ci, co, h, w = shape
    dev = _dev()
    p = detrand.uniform((n, ci, h + 2, w + 2), 23, "p")
    wt = (detrand.uniform((co, ci, 3, 3), 23, "w") * 0.1).requires_grad_(True)
    cot = detrand.uniform((n, co, h, w), 23, "cot")
    (F.conv2d(p, wt) * cot).sum().backward()
    dw = torch.full(wt.shape, float("nan"), device=dev)
    ops.wgrad3x3_wide(cot.to(dev), p.to(dev), dw)
    assert rel(dw, wt.grad) < 2e-5
    dw2 = dw.clone()
    ops.wgrad3x3_wide(cot.to(dev), p.to(dev), dw2, accumulate=True)
    assert rel(dw2, 2 * wt.grad) < 2e-5
    dw3 = torch.empty_like(dw)
    ops.wgrad3x3_wide(cot.to(dev), p.to(dev), dw3)
    assert torch.equal(dw, dw3)


@pytest.mark.parametrize("shape", [(1, 64, 128, 16, 32), (2, 68, 72, 6, 20), (1, 128, 64, 10, 48), (32, 64, 68, 2, 2), (5, 72, 64, 4, 4),
                                   (3, 68, 64, 1, 2), (2, 64, 64, 8, 8)])
def test_wide_strided_and_transposed_family(shape):
    """stride-2 3x3 conv and ConvTranspose2d(3, s2, p1, op1) on the GEMM-class kernels: forward, input adjoint
    (each is the other's adjoint) and weight gradient vs autograd; n, ci, co, oh, ow = low-resolution side"""
    from vts import ops
    n, ci, co, oh, ow = shape
    dev = _dev()
    # --- stride-2 conv: x [n,ci,2oh,2ow] -> y [n,co,oh,ow]
    x = detrand.uniform((n, ci, 2 * oh, 2 * ow), 31, "x").requires_grad_(True)
    w = (detrand.uniform((co, ci, 3, 3), 31, "w") * float(np.sqrt(3.0 / (9 * ci)))).requires_grad_(True)
    b = detrand.uniform((co,), 31, "b")
    ref = F.conv2d(x, w, b, stride=2, padding=1)
    cot = detrand.uniform(tuple(ref.shape), 31, "cot")
    (ref * cot).sum().backward()
    xd, wd, cd = x.detach().to(dev), w.detach().to(dev), cot.to(dev)
    xp = ops.pad_affine(xd, (1, 1, 1, 1), 0)
    out = torch.full(ref.shape, float("nan"), device=dev)
    ops.conv3x3s2_wide(xp, ops.w3x3_pack(wd, "conv_fwd"), b.to(dev), out)
    assert rel(out, ref) < 1e-5
    dx = torch.full(x.shape, float("nan"), device=dev)
    ops.tconv3x3s2_wide(ops.pad_affine(cd, (0, 1, 0, 1), 0), ops.w3x3_pack(wd, "conv_s2_adj"), None, dx)
    assert rel(dx, x.grad) < 1e-5
    dw = torch.full(w.shape, float("nan"), device=dev)
    ops.wgrad3x3_wide(cd, xp, dw, stride=2)
    assert rel(dw, w.grad) < 2e-5
    # --- transposed conv: z [n,co,oh,ow] -> u [n,ci,2oh,2ow], weight [co, ci, 3, 3] (ConvTranspose2d layout [in, out])
    z = detrand.uniform((n, co, oh, ow), 32, "z").requires_grad_(True)
    wt = (detrand.uniform((co, ci, 3, 3), 32, "wt") * float(np.sqrt(3.0 / (4 * co)))).requires_grad_(True)
    bt = detrand.uniform((ci,), 32, "bt")
    reft = F.conv_transpose2d(z, wt, bt, stride=2, padding=1, output_padding=1)
    cott = detrand.uniform(tuple(reft.shape), 32, "cott")
    (reft * cott).sum().backward()
    zd, wtd, ctd = z.detach().to(dev), wt.detach().to(dev), cott.to(dev)
    u = torch.full(reft.shape, float("nan"), device=dev)
    ops.tconv3x3s2_wide(ops.pad_affine(zd, (0, 1, 0, 1), 0), ops.w3x3_pack(wtd, "convT_fwd"), bt.to(dev), u)
    assert rel(u, reft) < 1e-5
    ctp = ops.pad_affine(ctd, (1, 1, 1, 1), 0)
    dz = torch.full(z.shape, float("nan"), device=dev)
    ops.conv3x3s2_wide(ctp, ops.w3x3_pack(wtd, "convT_adj"), None, dz)
    assert rel(dz, z.grad) < 1e-5
    dwt = torch.full(wt.shape, float("nan"), device=dev)
    ops.wgrad3x3_wide(zd, ctp, dwt, stride=2)
    assert rel(dwt, wt.grad) < 2e-5


@pytest.mark.parametrize("shape,stride", [((32, 64, 128, 17, 17), 2), ((32, 256, 512, 5, 5), 1), ((5, 128, 68, 9, 9), 2), ((3, 36, 64, 3, 3), 1),
                                          ((7, 64, 32, 4, 6), 2), ((2, 32, 36, 7, 10), 1), ((33, 512, 64, 2, 2), 1), ((32, 512, 1, 6, 6), 1), ((3, 70, 5, 4, 5), 2),
                                          ((2, 64, 128, 70, 75), 2), ((1, 256, 512, 40, 33), 1), ((2, 128, 64, 37, 41), 2), ((1, 36, 132, 129, 129), 1)])
def test_conv4x4_flat_forward_and_input_adjoint(shape, stride):
    """the PatchGAN layers Conv2d(4, stride, padding 2) of a wide discriminator on the GEMM-class kernels (flattened for maps of
    <= 128 pixels, tiled above) vs F.conv2d, and its input adjoint (stride 1: flipped packing on the padded gradient; stride 2: parity phases) vs autograd"""
    from vts import ops
    n, ci, co, h, w = shape
    dev = _dev()
    x = detrand.uniform((n, ci, h, w), 41, "x").requires_grad_(True)
    wt = (detrand.uniform((co, ci, 4, 4), 41, "w") * float(np.sqrt(3.0 / (16 * ci)))).requires_grad_(True)
    b = detrand.uniform((co,), 41, "b")
    ref = F.conv2d(x, wt, b, stride=stride, padding=2)
    cot = detrand.uniform(tuple(ref.shape), 41, "cot")
    (ref * cot).sum().backward()
    oh, ow = ref.shape[2:]
    ph, pw = stride * (oh - 1) + 4, stride * (ow - 1) + 4
    xd, wd, cd = x.detach().to(dev), wt.detach().to(dev), cot.to(dev)
    p = ops.pad_affine(xd, (2, ph - h - 2, 2, pw - w - 2), 0)
    out = torch.full(ref.shape, float("nan"), device=dev)
    ops.conv4x4_wide(p, ops.w4x4_pack(wd, "conv_fwd"), b.to(dev), out, stride=stride)
    assert rel(out, ref) < 1e-5
    dx = torch.full(x.shape, float("nan"), device=dev)
    if stride == 1:
        ops.conv4x4_wide(ops.pad_affine(cd, (1, 1, 1, 1), 0), ops.w4x4_pack(wd, "conv_adj"), None, dx)
    else:
        ops.conv4x4_wide(ops.pad_affine(cd, (0, 1, 0, 1), 0), ops.w4x4_pack(wd, "conv_s2_adj"), None, dx, stride=2, transposed=True)
    assert rel(dx, x.grad) < 1e-5


@pytest.mark.parametrize("shape,stride", [((2, 64, 128, 70, 75), 2), ((1, 256, 512, 40, 33), 1), ((2, 132, 68, 37, 41), 2), ((1, 64, 64, 129, 129), 1)])
def test_wgrad4x4_wide(shape, stride):
    """weight gradient of Conv2d(4, stride, padding 2) on the GEMM-class kernel (two tap-row launches) vs autograd"""
    from vts import ops
    n, ci, co, h, w = shape
    dev = _dev()
    x = detrand.uniform((n, ci, h, w), 43, "x")
    wt = (detrand.uniform((co, ci, 4, 4), 43, "w") * 0.1).requires_grad_(True)
    ref = F.conv2d(x, wt, stride=stride, padding=2)
    cot = detrand.uniform(tuple(ref.shape), 43, "cot")
    (ref * cot).sum().backward()
    oh, ow = ref.shape[2:]
    ph, pw = stride * (oh - 1) + 4, stride * (ow - 1) + 4
    p = ops.pad_affine(x.to(dev), (2, ph - h - 2, 2, pw - w - 2), 0)
    dw = torch.full(wt.shape, float("nan"), device=dev)
    ops.wgrad4x4_wide(cot.to(dev), p, dw, stride=stride)
    assert rel(dw, wt.grad) < 2e-5
    dw2 = dw.clone()
    ops.wgrad4x4_wide(cot.to(dev), p, dw2, stride=stride, accumulate=True)
    assert rel(dw2, 2 * wt.grad) < 2e-5
    dw3 = torch.empty_like(dw)
    ops.wgrad4x4_wide(cot.to(dev), p, dw3, stride=stride)
    assert torch.equal(dw, dw3)


@pytest.mark.parametrize("fixture", ["local_64x32.npz", "local2_64x32.npz"])
def test_local_enhancer_matches_reference_and_oracle(golden_dir, fixture):
    """pix2pixHD LocalEnhancer (define_G netG='local', --n_local_enhancers 1 and 2): forward vs the committed reference output, BN
    buffers, backward vs oracle"""
    from models import networks
    from vts import engine
    from vts.optim import FlatParams
    g = np.load(os.path.join(golden_dir, fixture), allow_pickle=False)
    h, w, seed, ngf, nd, nbg, nbl = (int(g[k]) for k in ("h", "w", "seed", "ngf", "n_down", "n_blocks_global", "n_blocks_local"))
    nl = int(g["n_local"]) if "n_local" in g.files else 1
    dev = _dev()
    sd = detrand.test_weights(nets.local_enhancer_param_shapes(1, 5, ngf, nd, nbg, nbl, nl), seed)
    G = networks.LocalEnhancer(1, 5, ngf=ngf, n_downsample_global=nd, n_blocks_global=nbg, n_local_enhancers=nl, n_blocks_local=nbl).to(dev)
    G.load_state_dict(sd)
    flat = FlatParams(G)
    G.train()
    x = detrand.uniform((2, 1, h, w), seed, "g_in")
    y, ctx = engine.resnet_forward(G, x.to(dev))
    assert rel(y, torch.from_numpy(g["G_out"])) < 5e-5
    for k, b in G.named_buffers():
        if b.dtype.is_floating_point:
            assert rel(b, torch.from_numpy(g["G_buf/" + k])) < 1e-4, k
    sdo = {k: v.clone() for k, v in sd.items()}
    for k, v in sdo.items():
        if v.dtype.is_floating_point and "running" not in k:
            v.requires_grad_(True)
    yo = nets.local_enhancer_forward(sdo, x, nd, nbg, nbl, n_local=nl)
    cot = detrand.uniform(tuple(yo.shape), seed, "g_cot")
    (yo * cot).sum().backward()
    flat.grad.zero_()
    engine.resnet_backward(G, ctx, (cot.to(dev) * (1.0 - y * y)).contiguous())
    named = dict(G.named_parameters())
    last_bias = "model%d_2.%d.bias" % (nl, nbl + 4)
    for k, v in sdo.items():
        if not (v.dtype.is_floating_point and v.requires_grad):
            continue
        if k.endswith(".bias") and k != last_bias and sdo[k.replace(".bias", ".weight")].dim() == 4:
            assert named[k].grad.abs().max().item() == 0.0, k
            continue
        assert rel(named[k].grad, v.grad) < 3e-4, (k, rel(named[k].grad, v.grad))
