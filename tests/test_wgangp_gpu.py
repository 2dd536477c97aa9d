"""--gan_mode wgangp on the GPU: the two kernels of csrc/vts_gradpen.hip on tests/judge_harness.py, engine.sg2d_gradient_penalty against the
reference's cal_gradient_penalty (tests/golden/sg2d_gp_32.npz) and float64 autograd on oracle/stylegan2.py, and the training step against
the reference's own (tests/golden/sinskitG_wgangp_step_256.npz).

Kernel bounds (derived, nothing measured in them):
  vts_gp_interp   |err| <= 4 u (|a r| + |(1 - a) f|), u = 2^-24: the roundings of 1 - a, of the two products and of the sum.
  vts_gp_penalty  value, scale, shift within 8 u relative of float64: the squares are summed in double (error ~ M 2^-53, far below u), what
                  remains is the final rounding to float32 (and the product with 1e-16 for the shift): a handful of u.
                  The slot increment: one unit of the 2^-40 fixed point plus double round-off.
Operator and step bounds are the project's gradient-parity bounds: values 1e-3 max(1, |v|), gradients 1e-3 relative L2.
Worst values measured on the MI355X: profiles/r26_wgangp.md."""
import json
import math
import os

import numpy as np
import pytest
import torch

import wgangp_ref as W
from judge_harness import Op, judge as _judge
from oracle import detrand
from oracle import stylegan2 as sg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BOUND = {"interp": 4.0, "penalty": 8.0, "slot": 1.0}
WORST = {}
GP_BLOCK, GP_MAX_WG = 4096, 256          # csrc/vts_gradpen.hip: elements per partial block, workgroups per sample at most


@pytest.fixture(scope="module")
def gpu():
    from vts import lib as L
    from vts import ops
    lib = L.load()
    yield lib, ops, L
    if WORST:
        print("\n[%s] worst err / unit per kernel instance" % __name__)
        for (inst, fam), (w, case, _, calls) in sorted(WORST.items(), key=lambda kv: -kv[1][0]):
            print("%-9.4f %-8s %5d  %-70s %s" % (w, fam, calls, inst, case))


def judge(gpu, tag, expected, call, opnds, outs):
    _judge(gpu[0], tag, expected, call, opnds, outs, BOUND, WORST, per_family=True)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


# ---------------------------------------------------------------------------------------------------------------- vts_gp_interp
# (id, N, H, W, real split, fake split, strided, alpha): per-sample sizes 1, 63, 64, 65, 4 * 32 * 32, 3 * 17 * 19; one or two sources per side
# (the splits of the two sides may differ); strided = every source is a channel slice of a wider buffer; alpha 0, 1 and values in between
INTERP = [
    ("m1-a0", 1, 1, 1, (1,), (1,), False, (0.0,)),
    ("m1-a1", 1, 1, 1, (1,), (1,), True, (1.0,)),
    ("m63", 1, 7, 9, (1,), (1,), False, (0.3125,)),
    ("m64-two", 3, 4, 4, (1, 3), (1, 3), True, (0.0, 1.0, 0.618034)),
    ("m65-two", 1, 13, 1, (2, 3), (4, 1), False, (0.9016131,)),
    ("m65-a1", 1, 13, 1, (5,), (2, 3), True, (1.0,)),
    ("m4096-cat", 3, 32, 32, (1, 3), (1, 3), True, (0.25, 0.0, 0.7071068)),
    ("m4096-one", 1, 32, 32, (4,), (4,), False, (0.0,)),
    ("m969-mixed", 3, 17, 19, (1, 2), (3,), True, (1.0, 0.1234567, 0.5)),
]


def _sources(split, n, h, w, strided, seed, name):
    ops_, full = [], detrand.uniform((n, sum(split), h, w), seed, name) * 3.0
    c0 = 0
    for i, c in enumerate(split):
        init = full[:, c0:c0 + c]
        if strided:      # channels [2, 2 + c) of a buffer with c + 5 channels
            ops_.append(Op((n, c, h, w), init, ns=(c + 5) * h * w, lead=2 * h * w))
        else:
            ops_.append(Op((n, c, h, w), init))
        c0 += c
    return ops_, full


@pytest.mark.parametrize("row", INTERP, ids=[r[0] for r in INTERP])
def test_gp_interp(gpu, row):
    lib, ops, L = gpu
    rid, n, h, w, rs, fs, strided, alpha = row
    ro, real = _sources(rs, n, h, w, strided, 11, "gp_r" + rid)
    fo, fake = _sources(fs, n, h, w, strided, 12, "gp_f" + rid)
    a = torch.tensor(alpha, dtype=torch.float32)
    ao, out = Op((n,), a), Op((n, sum(rs), h, w))
    ad = a.double().view(n, 1, 1, 1)
    t0, t1 = ad * real.double(), (1.0 - ad) * fake.double()
    call = lambda: ops.gp_interp(tuple(o.t for o in ro), tuple(o.t for o in fo), ao.t, out=out.t)
    judge(gpu, "interp-" + rid, "gp_interp_kernel", call, ro + fo + [ao, out], [(out, None, t0 + t1, U * (t0.abs() + t1.abs()), "interp")])
    got = out.content(out.dev.cpu())
    for i, v in enumerate(alpha):          # the end points are exact: the interpolate IS the real / the fake sample
        if v in (0.0, 1.0):
            assert torch.equal(got[i], (real if v == 1.0 else fake)[i]), (rid, i)


# ---------------------------------------------------------------------------------------------------------------- vts_gp_penalty
# (id, N, C, M, lambda, constant, coeff, grad_coeff, amplitude): M = 1, 63, 64, 65, 4097 and one sample of 258 partial blocks (more than
# the 256 workgroups a sample gets, so two workgroups walk two blocks and every sample spans several)
PENALTY = [
    ("m1", 2, 1, 1, 10.0, 1.0, 1.0, 0.5, 0.0005),
    ("m63", 3, 3, 63, 10.0, 1.0, 0.5, 0.25, 0.01),
    ("m64", 1, 4, 64, 10.0, 1.0, 1.0, 0.5, 0.05),
    ("m65", 2, 5, 65, 2.5, 0.75, 2.0, 1.0, 0.2),
    ("m4097", 3, 17, 4097, 10.0, 1.0, 1.0, 0.5, 0.002),
    ("m258blocks", 2, 1, GP_BLOCK * (GP_MAX_WG + 1) + 5, 10.0, 1.0, 1.0, 0.5, 0.0004),
]


@pytest.mark.parametrize("row", PENALTY, ids=[r[0] for r in PENALTY])
def test_gp_penalty(gpu, row):
    lib, ops, L = gpu
    rid, n, c, m, lam, const, coeff, gc, amp = row
    g = detrand.uniform((n, m), 21, "gp_g" + rid) * amp
    g[:, 0] *= 64.0            # the first and the last element of every sample carry 64 x the amplitude: a dropped edge cannot hide
    g[:, -1] *= 64.0
    blocks = -(-m // GP_BLOCK)
    wgs = min(blocks, GP_MAX_WG)
    nws = int(lib.vts_gp_penalty_ws_floats(n, m))
    assert nws == 2 * n * wgs
    if rid == "m258blocks":
        assert blocks > wgs > 1, "a sample must span several workgroups and a workgroup several blocks"
    go, slot = Op((n, c, m // c, 1), g), Op((1,), torch.tensor([-(7 << 40) + 12345]), dtype=torch.int64)
    val, sc, sh, ws = Op((1,)), Op((n * c,)), Op((n * c,)), Op((nws,))
    norms = ((g.double() + 1e-16) ** 2).sum(1).sqrt()
    assert bool(((norms - const).abs() >= 0.1).all())
    pen = lam / n * ((norms - const) ** 2).sum()
    scale = (gc * 2.0 * lam / n * (norms - const) / norms).view(n, 1).expand(n, c).reshape(-1)
    shift = scale * 1e-16
    call = lambda: ops.gp_penalty(go.t, slot.t, coeff, gc, lambda_gp=lam, constant=const, value=val.t, ws=ws.t, out=(sc.t, sh.t))
    inc = (coeff * pen).view(1)
    outs = [(val, None, pen.view(1), U * pen.abs().view(1), "penalty"), (sc, None, scale, U * scale.abs(), "penalty"),
            (sh, None, shift, U * shift.abs(), "penalty"), (slot, None, inc, 2.0 ** -40 + 64 * 2.0 ** -53 * inc.abs(), "slot"), (ws, None, None, None, "scratch")]
    judge(gpu, "penalty-" + rid, "gp_sumsq_kernel[%d blocks on %d workgroups]+gp_finish_kernel" % (blocks, wgs), call, [go, slot, val, sc, sh, ws], outs)


def test_gp_entries_reject_bad_arguments(gpu):
    lib, ops, L = gpu
    x = torch.zeros(2, 3, 4, 4, device="cuda")
    a = torch.zeros(2, device="cuda")
    p, st = x.data_ptr(), L.stream()
    assert lib.vts_gp_interp(p, 48, 3, None, 0, 0, p, 32, 2, None, 0, 0, a.data_ptr(), 2, 16, p, st) == -1       # 3 channels vs 2
    assert b"channels" in lib.vts_last_error()
    assert lib.vts_gp_interp(p, 47, 3, None, 0, 0, p, 48, 3, None, 0, 0, a.data_ptr(), 2, 16, p, st) == -1       # stride < sample
    assert lib.vts_gp_penalty(p, 2, 48, 3, 10.0, 1.0, 1.0, 1.0, None, None, None, None, None, st) == -1           # no workspace
    assert lib.vts_gp_penalty_ws_floats(0, 5) == 0


# ---------------------------------------------------------------------------------------------------------------- the operator
def _build_D(cin, ndf, size, seed):
    from models.stylegan2_blocks import StyleGAN2Discriminator
    from vts.optim import FlatParams
    D = StyleGAN2Discriminator(cin, ndf, size).to("cuda")
    sd = sg.test_weights(sg.d_param_shapes(cin, ndf, size), seed)
    D.load_state_dict(sd, strict=False)
    return D, FlatParams(D), sd


def _fixture_case(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "sg2d_gp_32.npz"), allow_pickle=False)
    return {k: int(g["%s/%s" % (tag, k)]) for k in ("size", "ndf", "input_nc", "n", "seed")}, g


OPERATOR = [("fixture-s32", None), ("fixture-s8", None), ("s8-c3-n5", dict(size=8, ndf=8, input_nc=3, n=5, seed=31)),
            ("s16-c4-n1", dict(size=16, ndf=8, input_nc=4, n=1, seed=32)), ("s64-c4-n5", dict(size=64, ndf=8, input_nc=4, n=5, seed=33))]


@pytest.mark.parametrize("rid,case", OPERATOR, ids=[r[0] for r in OPERATOR])
def test_gradient_penalty_operator(gpu, golden_dir, rid, case):
    """penalty, g and every weight gradient against float64 (the fixture where there is one, and autograd's double backward on the oracle);
    every bias .grad bitwise unchanged; accumulate adds; eager, capture and replay bitwise equal"""
    from vts import engine
    lib, ops, L = gpu
    gold = None
    if case is None:
        case, gold = _fixture_case(golden_dir, rid.split("-")[1])
    size, cin, n = case["size"], case["input_nc"], case["n"]
    D, flat, sd = _build_D(cin, case["ndf"], size, case["seed"])
    real, fake, alpha = W.gp_inputs(case)
    xh = W.interpolate(real.double(), fake.double(), alpha.double())
    pen, g_ref, grads, norms = W.penalty_autograd(sd, xh, size)
    assert bool(((norms - 1.0).abs() >= 0.1).all()), norms
    coeff, gcoeff = 2.0, 0.5
    rd, fd, ad = real.cuda(), fake.cuda(), alpha.cuda()
    if cin == 4:         # the conditional D1's form: cat(S, I) read in place from slices of wider buffers
        wide_r, wide_f = torch.zeros(n, 7, size, size, device="cuda"), torch.zeros(n, 6, size, size, device="cuda")
        wide_r[:, 1:2], wide_r[:, 3:6], wide_f[:, 0:1], wide_f[:, 2:5] = rd[:, :1], rd[:, 1:], fd[:, :1], fd[:, 1:]
        srcs = ((wide_r[:, 1:2], wide_r[:, 3:6]), (wide_f[:, 0:1], wide_f[:, 2:5]))
    else:
        srcs = (rd, fd)
    slot = ops.loss_slots(1, "cuda")
    named = dict(D.named_parameters())

    state = torch.zeros_like(flat.grad)

    def run():
        flat.grad.copy_(state)
        slot.zero_()
        return engine.sg2d_gradient_penalty(D, srcs[0], srcs[1], ad, slot, coeff=coeff, grad_coeff=gcoeff)

    def seed_of(p):          # each .grad is a view into the flat gradient buffer: its part of `state`, by address
        off = (p.grad.data_ptr() - flat.grad.data_ptr()) // 4
        return state[off:off + p.numel()].view_as(p.grad)

    g = run()
    torch.cuda.synchronize()
    value = ops.loss_values(slot)[0] / coeff
    print("%s penalty %.9g (float64 %.9g) norms %s" % (rid, value, float(pen), norms.tolist()))
    assert abs(value - float(pen)) <= 1e-3 * max(1.0, abs(float(pen)))
    assert tuple(g.shape) == tuple(real.shape)
    print("%-28s %.3e" % ("g", rel(g, g_ref)))
    assert rel(g, g_ref) < 1e-3
    first = {k: p.grad.clone() for k, p in named.items()}
    for k, p in named.items():
        if k.endswith("bias"):
            assert grads[k] is None or float(grads[k].abs().max()) == 0.0
            assert not bool(p.grad.any()), k
            continue
        print("%-28s %.3e" % (k, rel(p.grad, gcoeff * grads[k])))
        assert rel(p.grad, gcoeff * grads[k]) < 1e-3, k
    if gold is not None:       # the reference's own numbers
        tag = rid.split("-")[1]
        assert abs(value - float(gold[tag + "/penalty"])) <= 1e-3 * max(1.0, float(gold[tag + "/penalty"]))
        assert rel(g[:, :, ::4, ::4], torch.from_numpy(gold[tag + "/g_sub"])) < 1e-3
        for k, p in named.items():
            if not k.endswith("bias"):
                pr, rp = detrand.probe(p.grad.cpu() / gcoeff, k), gold["%s/grad/%s" % (tag, k)]
                # l2 norm at 1e-3; the projection on a vector of entries in [-1, 1): |<d, r>| <= |d| |r| <= 1e-3 |x| sqrt(numel)
                assert abs(pr[1] - rp[1]) <= 1e-3 * rp[1] and abs(pr[2] - rp[2]) <= 1e-3 * rp[1] * math.sqrt(p.numel()), (k, pr, rp)
    # accumulate really adds, and no bias gradient is touched: every bias gradient seeded with a pattern, every weight gradient with half of
    # what the call adds (the sum is then 1.5 x; a float32 add of terms of like size: 1e-5 relative L2 leaves room for the order of the sum)
    state.copy_((detrand.uniform((state.numel(),), 5, "gp_seed") * 0.01).cuda())
    for k, p in named.items():
        if not k.endswith("bias"):
            seed_of(p).copy_(0.5 * first[k])
    g2 = run()
    torch.cuda.synchronize()
    eager = [g2.clone(), flat.grad.clone(), slot.clone()]
    assert torch.equal(g2, g)
    for k, p in named.items():
        if k.endswith("bias"):
            assert torch.equal(p.grad.view(torch.int32), seed_of(p).view(torch.int32)) and bool(p.grad.any()), "bias gradient %s changed" % k
        else:
            assert rel(p.grad, 1.5 * first[k]) < 1e-5, (k, rel(p.grad, 1.5 * first[k]))
    # a second eager call, then capture and replay: the same bits
    g3 = run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, [g3, flat.grad, slot]))
    graph, cs = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    ops.freeze_ws(("test_wgangp", rid))
    try:
        cs.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cs):
            with torch.cuda.graph(graph, stream=cs):
                gg = engine.sg2d_gradient_penalty(D, srcs[0], srcs[1], ad, slot, coeff=coeff, grad_coeff=gcoeff)
        torch.cuda.current_stream().wait_stream(cs)
        for _ in range(2):
            flat.grad.copy_(state)
            slot.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(eager, [gg, flat.grad, slot]))
    finally:
        del graph
        ops.release_ws(("test_wgangp", rid))


def test_backward_without_bias_grads_and_tangent_of_a_plain_tensor(gpu):
    """sg2d_backward(bias_grads=False) writes every weight gradient as before and touches no bias gradient; sg2d_tangent_forward takes a
    plain tensor as well: for a piecewise-linear network without biases in the tangent, <1, J v> equals <g, v>"""
    from vts import engine
    lib, ops, L = gpu
    D, flat, sd = _build_D(3, 8, 16, 41)
    x = detrand.uniform((2, 3, 16, 16), 41, "x").cuda()
    v = detrand.uniform((2, 3, 16, 16), 41, "v").cuda()
    ones = torch.ones(2, device="cuda")
    _, ctx = engine.sg2d_forward(D, x, keep=True)
    flat.grad.zero_()
    g = engine.sg2d_backward(D, ctx, ones, input_grad=True)
    full = flat.grad.clone()
    flat.grad.fill_(7.0)
    engine.sg2d_backward(D, ctx, ones, bias_grads=False)
    torch.cuda.synchronize()
    for k, p in D.named_parameters():
        off = (p.grad.data_ptr() - flat.grad.data_ptr()) // 4
        if k.endswith("bias"):
            assert bool((p.grad == 7.0).all()), k
        else:
            assert torch.equal(p.grad.reshape(-1), full[off:off + p.numel()]), k
    tctx = engine.sg2d_tangent_forward(D, ctx, v)
    l1 = D.final_linear[1]
    ta0 = tctx.lin[3].view(2, -1)
    jv = (ta0.double() @ l1.weight.double().t()).view(-1) / math.sqrt(l1.weight.shape[1])
    gv = (g.double() * v.double()).sum((1, 2, 3))
    assert float((jv - gv).abs().max()) <= 1e-4 * float(gv.abs().max()), (jv, gv)


# ---------------------------------------------------------------------------------------------------------------- the step
FLAGS = ("--model sinskitG --gpu_ids 0 --lambda_G1_lpips 0 --lambda_G2_lpips 0 --use_vision_aided_loss False --lambda_G2_GAN_feat 0 "
         "--checkpoints_dir /tmp/vts_test_ckpt --name twgangp --crop_size %d --load_size %d --batch_size %d --netD stylegan2 "
         "--gan_mode wgangp --lambda_G2_GAN 0")


def _model(size, n, seed, extra=""):
    from models import create_model
    from options.train_options import TrainOptions
    from oracle import nets

    opt = TrainOptions(cmd_line=(FLAGS % (size, size, n)) + extra).parse()
    model = create_model(opt)
    model.setup(opt)
    model.parallelize()
    model.train()
    assert model.model_names == ["G", "D"] and getattr(model.netD, "is_stylegan2_d", False)
    model.netG.load_state_dict(detrand.test_weights(nets.g_param_shapes(), seed))
    model.netD.load_state_dict(sg.test_weights(sg.d_param_shapes(4, opt.ndf, size), seed + 1), strict=False)
    return model, opt


def _batch(size, nt, seed, n=1):
    from torch.utils.data import default_collate

    from data.synthetic_dataset import make_sample
    return default_collate([make_sample(size, nt, nt, seed + i) for i in range(n)])


def test_first_step_matches_the_reference(golden_dir):
    """the reference's own SinSKITGModel.optimize_parameters with --gan_mode wgangp --netD stylegan2 --lambda_G2_GAN 0 (float64), with the
    alpha it drew injected: losses (D_I_grad_penalty included), outputs, gradient probes of G and D"""
    g = np.load(os.path.join(golden_dir, "sinskitG_wgangp_step_256.npz"), allow_pickle=False)
    size, seed, nt = int(g["size"]), int(g["seed"]), int(g["nt"])
    flags = json.loads(str(g["flags"]))
    assert flags[flags.index("--gan_mode") + 1] == "wgangp" and flags[flags.index("--lambda_G2_GAN") + 1] == "0"
    assert bool((np.abs(g["gp_norms"] - 1.0) >= 0.1).all())
    model, opt = _model(size, 1, seed)
    model._draws = {"aug": torch.from_numpy(g["aug"]), "gp_alpha": torch.from_numpy(g["gp_alpha"]).float()}
    model.set_input(_batch(size, nt, seed), phase="train")
    model.optimize_parameters(epoch=1)
    losses = model.get_current_losses()
    ref = dict(zip([str(s) for s in g["loss_names"]], g["loss_values"]))
    assert "l_D_I_grad_penalty" in ref and ref["l_D_I_grad_penalty"] != 0.0 and losses["l_D_I_grad_penalty"] != 0.0
    print({k: (losses[k], float(v)) for k, v in ref.items()})
    for k, v in ref.items():
        assert abs(losses[k] - v) <= 1e-3 * max(1.0, abs(v)), (k, losses[k], v)
    assert rel(model.fake_I[:, :, ::4, ::4], torch.from_numpy(g["fake_I_sub"])) < 1e-3
    assert rel(model.pred_fake_I.reshape(-1), torch.from_numpy(g["pred_fake_I"]).reshape(-1)) < 1e-3
    for nm, net in (("G", model.netG), ("D", model.netD)):
        for k, p in net.named_parameters():
            if nm == "G" and k.endswith("bias") and not any(k.startswith(q) for q in ("down0.", "down7.", "up0.", "up0_T.")):
                continue                                   # bias in front of a norm: analytically zero gradient
            pr, rp = detrand.probe(p.grad.cpu(), k), g["grad_%s/%s" % (nm, k)]
            print("%s %-28s l2 %.3e  proj %.3e" % (nm, k, abs(pr[1] - rp[1]) / max(rp[1], 1e-300), abs(pr[2] - rp[2]) / max(rp[1] * math.sqrt(p.numel()), 1e-300)))
            # l2 norm at 1e-3; the projection on a vector of entries in [-1, 1): |<d, r>| <= |d| |r| <= 1e-3 |x| sqrt(numel)
            assert abs(pr[1] - rp[1]) <= 1e-3 * rp[1] and abs(pr[2] - rp[2]) <= 1e-3 * rp[1] * math.sqrt(p.numel()), (nm, k, pr, rp)


def test_graph_replay_equals_eager_with_injected_draws():
    """three steps with the same device-resident draws: all eager, and eager + capture + replay: bitwise the same weights and losses"""
    size, n, seed = 256, 1, 77
    batches = [_batch(size, 64, seed + 10 * s, n) for s in range(3)]
    res = []
    for graph in (False, True):
        model, opt = _model(size, n, seed, " --use_hip_graph %s" % graph)
        model._draws = {"aug": (detrand.uniform((4, n), 3, "aug") * 0.5 + 0.5).cuda(), "gp_alpha": torch.tensor([0.37], device="cuda"),
                        "device_resident": True}
        for b in batches:
            model.set_input(b, phase="train")
            model.optimize_parameters(epoch=1)
        torch.cuda.synchronize()
        assert (model._graphs is not None) == graph
        res.append((model.flatG.flat.clone(), model.flatD.flat.clone(), model._loss_buf.clone(), model.fake_I.clone()))
    assert int(res[0][2][list(model.LOSS_SLOTS).index("D_I_grad_penalty")]) != 0
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_batch_two_step_runs_and_logs_the_operators_penalty(gpu):
    """a batch-2 step (random alpha drawn on the device, then captured and replayed): finite losses, and D_I_grad_penalty is the operator's
    value on the tensors the step's D1 passes saw, at the weights they saw them with"""
    from models.stylegan2_blocks import StyleGAN2Discriminator
    from vts import engine
    lib, ops, L = gpu
    size, n, seed = 256, 2, 81
    model, opt = _model(size, n, seed)
    torch.manual_seed(3)
    twin = StyleGAN2Discriminator(4, opt.ndf, size).to("cuda")
    twin.load_state_dict(model.netD.state_dict())
    model.set_input(_batch(size, 64, seed, n), phase="train")
    model.optimize_parameters(epoch=1)
    losses = model.get_current_losses()
    assert all(np.isfinite(v) for v in losses.values()) and losses["l_D_I_grad_penalty"] > 0.0
    alpha = model._gp_alpha
    assert tuple(alpha.shape) == (n,) and bool(((alpha >= 0) & (alpha < 1)).all()) and float(alpha[0]) != float(alpha[1])
    slot = ops.loss_slots(1, "cuda")
    g = engine.sg2d_gradient_penalty(twin, (model.real_S, model.real_I), (model.real_S, model.fake_I), alpha, slot, param_grads=False)
    torch.cuda.synchronize()
    assert tuple(g.shape) == (n, 4, size, size)
    assert ops.loss_values(slot)[0] == losses["l_D_I_grad_penalty"]
    for _ in range(2):          # capture, replay
        model.set_input(_batch(size, 64, seed, n), phase="train")
        model.optimize_parameters(epoch=1)
    torch.cuda.synchronize()
    assert model._graphs is not None and all(np.isfinite(v) for v in model.get_current_losses().values())
