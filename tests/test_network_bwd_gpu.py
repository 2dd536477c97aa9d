"""The network-level backward C entries (include/vts.h; SURVEY 8b's `vts_unet_bwd` / `vts_msd_bwd`): vts_unet_backward,
vts_patchgan_backward / vts_msd_backward on the workspace their forward left.

  * against the Python schedule of the product (vts/engine.py:unet_backward, msd_backward), bit for bit, with and without the side stream
  * the U-Net's gradients against the oracle's generator in float64 under autograd (independent of the Python schedule)
  * capturable into one HIP graph, repeatable, and bad arguments refused before any launch
(the builders and seeded inputs are those of tests/test_network_abi_gpu.py)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detrand, nets  # noqa: E402  (checker only)

FLAGS = ("--model %s --gpu_ids 0 --lambda_G1_lpips 0 --lambda_G2_lpips 0 --use_vision_aided_loss False "
         "--lambda_G2_GAN_feat 0 --checkpoints_dir /tmp/vts_test_ckpt --name t --crop_size %d --batch_size %d")
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def generator(size, n, model_name="sinskitG", seed=77, nls=None):
    if nls is not None:
        from models.networks import CustomUnetGenerator

        G = CustomUnetGenerator(9, 5, num_downs=8, ngf=10, num_layer_separate=nls).to(DEV)
        G.load_state_dict(detrand.test_weights({k: tuple(v.shape) for k, v in G.state_dict().items()}, seed))
        return G.eval(), None
    from models import create_model
    from options.train_options import TrainOptions

    opt = TrainOptions(cmd_line=FLAGS % (model_name, size, n)).parse()
    model = create_model(opt)
    model.setup(opt)
    model.parallelize()
    G = model.netG
    if model_name == "sinskitG":
        G.load_state_dict(detrand.test_weights(nets.g_param_shapes(), seed))
    else:
        G.load_state_dict(detrand.test_weights(nets.g_param_shapes(style_nc=opt.style_code_dim, num_layer_style_code=opt.num_layer_style_code), seed))
    return G.eval(), opt


def unet_params(G):
    """(name, parameter) of every convolution the U-Net entries cover"""
    out = []
    for i in range(G.num_downs):
        for name in ["down%d" % i, "up%d" % i] + (["up%d_T" % i] if i < G.num_layer_separate else []):
            conv = getattr(G, name).conv
            out += [(name + ".weight", conv.weight), (name + ".bias", conv.bias)]
    return out


def py_unet_grads(G, x, d_raw, style_code=None):
    from vts import engine

    for _, p in unet_params(G):
        p.grad = torch.zeros_like(p)       # the Python schedule never writes the (identically zero) normalised-layer biases
    y, ctx = engine.unet_forward(G, x, style_code=style_code)
    engine.unet_backward(G, ctx, d_raw)
    torch.cuda.synchronize()
    return y.clone(), {k: p.grad.clone() for k, p in unet_params(G)}


def c_unet_grads(G, x, d_raw, style_tile=None, side=None):
    from vts import engine

    for _, p in unet_params(G):
        p.grad = torch.full_like(p, float("nan"))      # every gradient must be overwritten
    y, ctx = engine.unet_forward_train_c(G, x, style_tile=style_tile, side_stream=side)
    engine.unet_backward_c(G, ctx, d_raw, side_stream=side)
    torch.cuda.synchronize()
    return y.clone(), {k: p.grad.clone() for k, p in unet_params(G)}


def assert_same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, rel(a[k], b[k]))


def inputs(n, size, seed=5):
    s = detrand.uniform((n, 1, size, size), seed, "sketch").to(DEV)
    grid = detrand.uniform((n, 8, size, size), seed, "grid").to(DEV)
    d_raw = (detrand.uniform((n, 5, size, size), seed, "d_raw") - 0.5).to(DEV)
    return s, grid, d_raw


@pytest.mark.parametrize("size,n,nls", [(256, 1, None), (512, 2, None), (1024, 4, None), (256, 2, 0), (256, 2, 1)])
def test_unet_c_backward_equals_the_python_schedule_bit_for_bit(size, n, nls):
    G, _ = generator(size, n, nls=nls)
    s, grid, d_raw = inputs(n, size)
    y_py, g_py = py_unet_grads(G, (s, grid), d_raw)
    for side in (None, torch.cuda.Stream()):
        y_c, g_c = c_unet_grads(G, (s, grid), d_raw, side=side)
        assert torch.equal(y_c, y_py)
        assert_same(g_c, g_py)
    # the biases in front of an InstanceNorm: exact zeros
    assert not g_c["down3.bias"].any() and not g_c["up3.bias"].any()


def test_unet_c_backward_one_source_input_and_strided_d_raw():
    G, _ = generator(256, 2)
    s, grid, d_raw = inputs(2, 256, seed=6)
    x = torch.cat([s, grid], 1)
    _, g_py = py_unet_grads(G, x, d_raw)
    wide = torch.zeros(2, 7, 256, 256, device=DEV)
    wide[:, :5] = d_raw                         # a channel slice of a wider tensor: batch stride 7 * H * W
    _, g_c = c_unet_grads(G, x, wide[:, :5])
    assert_same(g_c, g_py)


def test_unet_c_backward_with_the_tiled_style_code():
    G, opt = generator(256, 2, model_name="skitG")
    x = detrand.uniform((2, 9, 256, 256), 9, "g_in").to(DEV)
    d_raw = (detrand.uniform((2, 5, 256, 256), 9, "d_raw") - 0.5).to(DEV)
    sc = detrand.uniform((2, opt.style_code_dim), 9, "style")
    sc = (sc / sc.norm(dim=1, keepdim=True)).to(DEV)
    _, g_py = py_unet_grads(G, x, d_raw, style_code=sc)
    tile = sc[:, :, None, None].expand(-1, -1, 256 >> G.num_downs, 256 >> G.num_downs).contiguous()
    for side in (None, torch.cuda.Stream()):
        _, g_c = c_unet_grads(G, x, d_raw, style_tile=tile, side=side)
        assert_same(g_c, g_py)


def test_unet_c_backward_against_float64_autograd():
    """the oracle's CustomUnetGenerator (CPU, float64, torch autograd) judges every gradient tensor: relative L2 1e-3, or -- where a ReLU /
    LeakyReLU input sits within rounding distance of zero (a kink: fp32 and float64 disagree about the side) -- 1e-3 against the fp32 CPU
    oracle, which took the same side (the nearer-judge rule of tests/test_step_gpu.py)"""
    seed = 81
    G, _ = generator(256, 1, seed=seed)
    sd = detrand.test_weights(nets.g_param_shapes(), seed)
    x = detrand.uniform((1, 9, 256, 256), seed, "g_in")
    R = detrand.uniform((1, 5, 256, 256), seed, "R") - 0.5
    y, _ = c_unet_grads(G, x.to(DEV), R.to(DEV) * 0)      # (shape of the output)
    d_raw = (R.to(DEV) * (1 - y * y)).contiguous()        # d sum(R * tanh(z)) / dz
    _, g_c = c_unet_grads(G, x.to(DEV), d_raw)
    judges = {}
    for dt in (torch.float64, torch.float32):
        sdt = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd.items()}
        out = nets.unet_forward(sdt, x.to(dt))
        (out * R.to(dt)).sum().backward()
        judges[dt] = {k: v.grad for k, v in sdt.items()}
    sdkey = {}
    for k in sd:
        blk, rest = k.split(".model.")
        sdkey[blk + "." + rest.split(".")[1]] = k
    nd = G.num_downs
    checked = 0
    for name, grad in g_c.items():
        k = sdkey[name]
        blk, kind = name.split(".")
        i = int(blk[len("down") if blk.startswith("down") else len("up"):].split("_")[0])
        if kind == "bias" and ((blk.startswith("down") and 0 < i < nd - 1) or (blk.startswith("up") and i > 0)):
            assert not grad.any(), name           # in front of an InstanceNorm: identically zero (the reference holds rounding noise)
            continue
        e64, e32 = rel(grad, judges[torch.float64][k]), rel(grad, judges[torch.float32][k])
        assert min(e64, e32) < 1e-3, (name, e64, e32)
        checked += 1
    assert checked == len(g_c) - (nd - 2) - (nd - 1) - (G.num_layer_separate - 1)


# ---- the discriminators ----------------------------------------------------------------------------------------------------------------

def _discriminator(input_nc, n_layers=3, seed=31):
    from models import networks

    D = networks.MultiscaleDiscriminator(input_nc, ndf=8, n_layers=n_layers, num_D=3).to(DEV)
    D.load_state_dict(detrand.test_weights(nets.d_param_shapes(input_nc, n_layers=n_layers), seed))
    return D


def _buffers(D):
    return {k: b.detach().clone() for k, b in D.named_buffers()}


def _dgrads(D):
    return {k: p.grad.clone() for k, p in D.named_parameters()}


def _set_grads(D, value):
    for p in D.parameters():
        p.grad = torch.full_like(p, value)


def _run_d(which, D, x0, x1, dpreds, param_grads, accumulate, input_grad):
    from vts import engine

    if which == "py":
        preds, ctx = engine.msd_forward(D, x0, x1)
        bufs = _buffers(D)
        engine.msd_backward(D, ctx, dpreds, param_grads=param_grads, accumulate=accumulate, input_grad=input_grad)
    else:
        preds, ctx = engine.msd_forward_train_c(D, x0, x1)
        bufs = _buffers(D)
        engine.msd_backward_c(D, ctx, dpreds, param_grads=param_grads, accumulate=accumulate, input_grad=input_grad)
    torch.cuda.synchronize()
    assert all(torch.equal(v, bufs[k]) for k, v in _buffers(D).items()), "the backward touched the running statistics"
    return [p.clone() for p in preds]


def _dpreds(n, h, w, n_layers, seed):
    out = []
    for s in range(3):
        ph, pw = h, w
        for st in [2] * n_layers + [1, 1]:
            ph, pw = ph // st + 1, pw // st + 1
        out.append((detrand.uniform((n, 1, ph, pw), seed + s, "dpred") - 0.5).to(DEV))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


@pytest.mark.parametrize("shape,n_layers", [((2, 256, 256), 3), ((4, 130, 98), 3), ((96, 32, 32), 3), ((2, 128, 128), 2), ((3, 64, 64), 4)])
def test_msd_c_backward_equals_the_python_schedule_bit_for_bit(shape, n_layers):
    """parameter gradients overwritten, then accumulated (the real + fake passes of a D update), input gradient merged over the pyramid
    (written, then accumulated); the running statistics untouched by the backward.  Depth 4 has a layer the Python forward sends to the
    GEMM-class kernel (engine._flat4) while the C forward keeps the 4x4 family: equal to rounding there, as the forward entry is."""
    from vts import engine

    n, h, w = shape
    x0 = detrand.uniform((n, 1, h, w), 41, "s").to(DEV)
    x1 = detrand.uniform((n, 3, h, w), 41, "i").to(DEV)
    dp = [_dpreds(n, h, w, n_layers, 50), _dpreds(n, h, w, n_layers, 60)]
    res = {}
    for which in ("py", "c"):
        D = _discriminator(4, n_layers)
        _set_grads(D, 0.0 if which == "py" else float("nan"))     # (the Python schedule leaves the BatchNorm-fed conv biases alone)
        d_in = torch.full_like(x1, float("nan"))
        p1 = _run_d(which, D, x0, x1, dp[0], True, False, (d_in, False))
        g1, i1 = _dgrads(D), d_in.clone()
        p2 = _run_d(which, D, x0, x1, dp[1], True, True, (d_in, True))
        res[which] = (p1 + p2, g1, i1, _dgrads(D), d_in.clone(), _buffers(D))
    exact = all(engine.patchgan_c_ok(D, (h + (1 << s) - 1) >> s, (w + (1 << s) - 1) >> s) for s in range(3))
    assert exact == (n_layers <= 3)
    same = torch.equal if exact else (lambda u, v: rel(u, v) < 2e-3)
    a, b = res["py"], res["c"]
    for u, v in zip(a[0], b[0]):
        assert same(u, v)
    for part in (1, 3):
        for k in a[part]:
            assert same(a[part][k], b[part][k]), (part, k, rel(a[part][k], b[part][k]))
    assert same(a[2], b[2]) and same(a[4], b[4])
    for k in a[5]:
        assert same(a[5][k].float(), b[5][k].float()), k


@pytest.mark.parametrize("shape", [(2, 256, 256), (4, 130, 98)])
def test_msd_c_backward_input_gradient_only(shape):
    """the generator step: every parameter pointer NULL, the parameter gradients untouched; with two sources and with one (in1.C == 0,
    --use_cGAN False), the input gradient written and accumulated"""
    n, h, w = shape
    x0 = detrand.uniform((n, 1, h, w), 42, "s").to(DEV)
    x1 = detrand.uniform((n, 3, h, w), 42, "i").to(DEV)
    x01 = torch.cat([x0, x1], 1)
    dp = _dpreds(n, h, w, 3, 70)
    for src0, src1 in ((x0, x1), (x01, None)):
        res = {}
        for which in ("py", "c"):
            D = _discriminator(4)
            _set_grads(D, 7.0)
            tgt = src1 if src1 is not None else src0
            d_in = (detrand.uniform(tuple(tgt.shape), 43, "acc") - 0.5).to(DEV)
            first = torch.empty_like(tgt)
            _run_d(which, D, src0, src1, dp, False, False, (first, False))
            _run_d(which, D, src0, src1, dp, False, False, (d_in, True))
            assert all(bool((p.grad == 7.0).all()) for p in D.parameters())
            res[which] = (first, d_in)
        assert torch.equal(res["py"][0], res["c"][0]) and torch.equal(res["py"][1], res["c"][1])


def test_forward_and_backward_of_both_families_capture_into_one_graph():
    """U-Net (tactile branch on a side stream) and discriminator, forward + backward: two eager calls agree, and the replay of one captured
    graph gives the eager results bit for bit"""
    from vts import engine, lib as L

    lib = L.load()
    G, _ = generator(256, 1)
    D = _discriminator(4)
    s, grid, d_raw = inputs(1, 256, seed=8)
    x1 = detrand.uniform((1, 3, 256, 256), 44, "i").to(DEV)
    dp = _dpreds(1, 256, 256, 3, 80)
    d_in = torch.empty_like(x1)
    side = torch.cuda.Stream()
    y, uctx = engine.unet_forward_train_c(G, (s, grid), side_stream=side)
    ud = engine.unet_desc(G, (s, grid), y, None, side)
    ug = engine.unet_grads(G, d_raw)
    preds, (md, mws) = engine.msd_forward_train_c(D, s, x1)
    mg = engine.msd_grads(D, dp, input_grad=(d_in, False))
    uws = uctx[3]

    def step():
        st = L.stream()
        L.check(lib.vts_unet_forward(C.byref(ud), uws.data_ptr(), uws.numel(), st), "vts_unet_forward")
        L.check(lib.vts_unet_backward(C.byref(ud), C.byref(ug), uws.data_ptr(), uws.numel(), st), "vts_unet_backward")
        L.check(lib.vts_msd_forward(C.byref(md), mws.data_ptr(), mws.numel(), st), "vts_msd_forward")
        L.check(lib.vts_msd_backward(C.byref(md), C.byref(mg), mws.data_ptr(), mws.numel(), st), "vts_msd_backward")

    def results():
        torch.cuda.synchronize()
        return ([y.clone(), d_in.clone()] + [p.clone() for p in preds] + [p.grad.clone() for _, p in unet_params(G)]
                + [p.grad.clone() for p in D.parameters()])

    step()
    eager = results()
    step()
    again = results()
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    graph = torch.cuda.CUDAGraph()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):
        with torch.cuda.graph(graph, stream=cs):
            step()
    torch.cuda.current_stream().wait_stream(cs)
    for t in [y, d_in] + [p.grad for _, p in unet_params(G)] + [p.grad for p in D.parameters()]:
        t.fill_(float("nan"))
    graph.replay()
    replay = results()
    assert all(torch.equal(a, b) for a, b in zip(eager, replay))


def test_bad_backward_arguments_are_refused_through_the_abi():
    from vts import engine, lib as L

    lib = L.load()
    G, _ = generator(256, 1)
    s, grid, d_raw = inputs(1, 256, seed=9)
    y, (x, _, g_out, ws) = engine.unet_forward_train_c(G, (s, grid))
    d = engine.unet_desc(G, (s, grid), g_out)
    g = engine.unet_grads(G, d_raw)
    need = lib.vts_unet_backward_ws_floats(C.byref(d))
    assert need >= lib.vts_unet_forward_ws_floats(C.byref(d)) > 0 and need == ws.numel()
    assert lib.vts_unet_backward(C.byref(d), C.byref(g), ws.data_ptr(), need - 1, L.stream()) == -1
    assert b"workspace" in lib.vts_last_error()
    g.d_raw = None
    assert lib.vts_unet_backward(C.byref(d), C.byref(g), ws.data_ptr(), need, L.stream()) == -1 and b"d_raw" in lib.vts_last_error()
    g = engine.unet_grads(G, d_raw)
    g.up_dw[5] = None
    assert lib.vts_unet_backward(C.byref(d), C.byref(g), ws.data_ptr(), need, L.stream()) == -1 and b"up5" in lib.vts_last_error()
    assert lib.vts_unet_backward(C.byref(d), None, ws.data_ptr(), need, L.stream()) == -1
    # the discriminator: a scale without dpred, a short workspace, a partial set of parameter gradients
    D = _discriminator(4)
    x1 = detrand.uniform((1, 3, 256, 256), 44, "i").to(DEV)
    preds, (md, mws) = engine.msd_forward_train_c(D, s, x1)
    dp = _dpreds(1, 256, 256, 3, 90)
    mg = engine.msd_grads(D, dp)
    mg.scale[1].dpred = None
    assert lib.vts_msd_backward(C.byref(md), C.byref(mg), mws.data_ptr(), mws.numel(), L.stream()) == -1
    assert b"scale 1 has no dpred" in lib.vts_last_error()
    mg = engine.msd_grads(D, dp)
    assert lib.vts_msd_backward(C.byref(md), C.byref(mg), mws.data_ptr(), 8, L.stream()) == -1 and b"workspace" in lib.vts_last_error()
    mg.scale[2].dw[1] = None
    assert lib.vts_msd_backward(C.byref(md), C.byref(mg), mws.data_ptr(), mws.numel(), L.stream()) == -1
    assert b"parameter gradient missing" in lib.vts_last_error()
    pg = L.PatchganGrads()
    assert lib.vts_patchgan_backward(C.byref(md.scale[0]), C.byref(pg), mws.data_ptr(), mws.numel(), L.stream()) == -1
    assert b"dpred" in lib.vts_last_error()
    torch.cuda.synchronize()


TRAIN_HOST = os.path.join(ROOT, "visual-tactile-synthesis_amd", "bin", "unet_train_host")


@pytest.mark.skipif(not os.path.exists(TRAIN_HOST), reason="examples/unet_train_host.cpp not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_a_cpp_host_trains_the_generator_without_python(tmp_path):
    """examples/unet_train_host.cpp: 3 generator steps (forward, L1 against a target, mask + Tanh backward, vts_unet_backward, Adam over a
    flat buffer) at 256 x 256, N = 2 -- its final weights equal bit for bit the same sequence driven from Python (engine.unet_forward /
    unet_backward, then the ops wrappers of vts_l1, vts_g_out_grad and vts_adam_flat in the host's order)"""
    from test_network_abi_gpu import write_host_input
    from vts import engine, lib as L, ops

    size, n, steps = 256, 2, 3
    G, _ = generator(size, n)
    s, grid, _ = inputs(n, size, seed=11)
    target = (detrand.uniform((n, 5, size, size), 11, "target") * 2 - 1)
    fin, ftgt, fout = str(tmp_path / "in.bin"), str(tmp_path / "target.bin"), str(tmp_path / "w.bin")
    write_host_input(fin, G, s, grid)
    target.numpy().astype("<f4").tofile(ftgt)
    r = subprocess.run([TRAIN_HOST, fin, ftgt, str(steps), fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("L1 loss") == steps
    # the same sequence from Python, parameters in the host's (in.bin's) order
    params = []
    for i in range(G.num_downs):
        for name in ["down%d" % i, "up%d" % i] + (["up%d_T" % i] if i < G.num_layer_separate else []):
            conv = getattr(G, name).conv
            params += [conv.weight, conv.bias]
    flat = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
    gflat, m, v = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat)
    tgt = target.to(DEV)
    mask = torch.ones(n, 1, size, size, device=DEV)
    dI, dT = torch.empty(n, 3, size, size, device=DEV), torch.empty(n, 2, size, size, device=DEV)
    d_raw = torch.empty(n, 5, size, size, device=DEV)
    slot = torch.zeros(1, dtype=torch.int64, device=DEV)
    coeff = 1.0 / (n * 5 * size * size)
    lib = L.load()
    for step in range(1, steps + 1):
        o = 0
        for p in params:
            p.data.copy_(flat[o:o + p.numel()].view_as(p))
            p.grad = torch.zeros_like(p)
            o += p.numel()
        y, ctx = engine.unet_forward(G, (s, grid))
        for k in range(n):
            ops.l1(y[k, :3], tgt[k, :3].contiguous(), coeff, slot, grad=dI[k])
            ops.l1(y[k, 3:], tgt[k, 3:].contiguous(), coeff, slot, grad=dT[k])
        L.check(lib.vts_g_out_grad(dI.data_ptr(), dT.data_ptr(), mask.data_ptr(), y.data_ptr(), n, size, size, d_raw.data_ptr(), L.stream()),
                "vts_g_out_grad")
        engine.unet_backward(G, ctx, d_raw)
        gflat.copy_(torch.cat([p.grad.reshape(-1) for p in params]))
        L.check(lib.vts_adam_flat(flat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), flat.numel(), 2e-4, 0.5, 0.999, 1e-8, step, 1.0,
                                  L.stream()), "vts_adam_flat")
    torch.cuda.synchronize()
    got = torch.from_numpy(np.fromfile(fout, dtype="<f4"))
    assert got.numel() == flat.numel() and torch.equal(got, flat.cpu())
