"""The classic pix2pix U-Net generator (--netG unet_128 | unet_256) on the HIP path.

1. The new member of the GEMM-class 4 x 4 family, vts_tconv4x4s2p1_wide (ConvTranspose2d(4, 2, 1) / the input adjoint of Conv2d(4, 2, 1)
   on the operand zero-padded by one), alone: judged elementwise in float64 on guard-banded operands (tests/judge_harness.py), the
   kernel instance asserted, |got - ref| <= C u sqrt(4 Cin) absref at every element with the transposed family's existing constant
   (tests/test_wide_family_gpu.py: C = 1.5), and compared with what the 4 x 4 kernels (vts_conv4x4, transposed, pad 1) give on the same
   operands at the same bound.
2. engine.unet_classic_forward / unet_classic_backward on the cases of tests/unet_classic_restated.py against the reference's float64
   run (tests/golden/unet_classic.npz, which test_unet_classic_cpu.py pins the restatement to at 1e-10; the restatement supplies the whole
   tensors where the fixture keeps probe triples, so every error below is a true relative L2): forward 2e-5 (the bound of
   tests/test_resnet_gpu.py), eval-mode forward 5e-5 and BatchNorm buffers 1e-4 (the same file's bounds), gradients 1e-3 per tensor
   with the nearer-judge rule of tests/test_step_gpu.py:check_grad.  Measured errors are printed beside the fixture's float32 yardstick.
3. Which kernels ran (at the fixture's sizes -- maps of 1 ... 64 pixels, batch 2 -- no layer of more than 80 output channels on the
   4 x 4 kernels' group loop; on larger maps the engine leaves the transposed launches there, profiles/r24_unet_classic.md), bitwise
   repeatability, and graph replay equal to the eager pass bit for bit.

Every test here needs networks.define_G('unet_*') or the new C entry, so each fails on a tree without them.
"""
import functools
import math

import pytest
import torch

import judge_harness as J
import unet_classic_restated as U
from oracle import detrand
from oracle import launch_ref as R

pytestmark = pytest.mark.gpu

C_CONVT = 1.5        # tests/test_wide_family_gpu.py C_BOUND["convT"]
OUT_TOL, EVAL_TOL, BUF_TOL, GRAD_TOL = 2e-5, 5e-5, 1e-4, 1e-3
WORST = {}
WIDE_KERNELS = ("conv_flat_kernel<4, 16>", "conv_flat_kernel<4, 16>+ksplit", "conv4x4_wide_kernel<2>", "conv4x4_wide_kernel<2>+ksplit",
                "conv_wide_phase_kernel<4>")


@pytest.fixture(scope="module")
def gpu():
    from vts import lib as L
    from vts import ops
    lib = L.load()
    dev = torch.device("cuda:0")
    ops.workspace(1 << 22, dev)
    yield lib, ops, dev
    if WORST:
        print("\n[%s] vts_tconv4x4s2p1_wide, worst err / (u sqrt(K) absref) per kernel instance (bound %.2f):" % (__name__, C_CONVT))
        for inst, (w, case, fam, calls) in sorted(WORST.items(), key=lambda kv: -kv[1][0]):
            print("%-9.4f %5d calls  %-34s %s" % (w, calls, inst, case))


# ---- 1. the new kernel alone ---------------------------------------------------------------------------------------------------------
CHANNELS = [(128, 96), (384, 192), (64, 84)]
# The family's rule (vts_conv4x4_flat_ok, transposed: a parity phase of <= 128 pixels) puts every input map of <= 128 pixels on the
# flattened-batch kernel: 8 x 16 is the flat limit, 12 x 11 the first tiled case, 16 x 17 spans several row tiles.
MAPS = [(1, 1), (3, 5), (4, 8), (8, 8), (9, 7), (8, 16), (12, 11), (16, 17)]


@pytest.mark.parametrize("hw", MAPS, ids=["%dx%d" % m for m in MAPS])
@pytest.mark.parametrize("chan", CHANNELS, ids=["%dto%d" % c for c in CHANNELS])
def test_tconv4x4s2p1_wide_elementwise(gpu, chan, hw):
    lib, ops, dev = gpu
    cin, cout = chan
    ih, iw = hw
    seed = 2500 + 10 * CHANNELS.index(chan) + MAPS.index(hw)
    wt = detrand.uniform((cin, cout, 4, 4), seed, "w") * math.sqrt(3.0 / (4 * cin))
    bias = detrand.uniform((cout,), seed, "b")
    flat = ih * iw <= 128
    assert bool(lib.vts_tconv4x4s2p1_flat_ok(ih, iw)) == flat
    for n in (1, 3):
        x = detrand.uniform((n, cin, ih, iw), seed + n, "x")
        p = torch.nn.functional.pad(x, (1, 1, 1, 1))
        # One packing serves both roles: a ConvTranspose2d weight [Ci,Co,4,4] in its forward and a Conv2d weight [Co,Ci,4,4] in its input
        # adjoint are both [operator input channels, operator output channels, 4, 4] (ops.w4x4_pack: convT_fwd is an alias of conv_s2_adj)
        mode = "convT_fwd"
        pb, wb, bb, ob = J.Op(p.shape, p), J.Op(wt.shape, wt), J.Op((cout,), bias), J.Op((n, cout, 2 * ih, 2 * iw))
        packed = ops.w4x4_pack(wb.t, mode, tag="unet-classic-test")
        assert packed is ops.w4x4_pack(wb.t, "conv_s2_adj", tag="unet-classic-test")      # the same packing, the same buffer
        tb = J.Op(packed.shape, packed.cpu())
        torch.cuda.synchronize()
        ksplit = lib.vts_tconv4x4s2p1_wide_ws_floats(n, cin, cout, ih, iw) > 0
        expected = ("conv_flat_kernel<4, 16>" + ("+ksplit" if ksplit else "")) if flat else "conv_wide_phase_kernel<4>"
        for with_bias in (False, True):
            ref, unit = R._tconv_judge(x, wt, bias if with_bias else None, 4, 1, 2 * ih, 2 * iw)["out"]
            assert tuple(ref.shape) == ob.shape

            def call():
                ops.workspace(1, dev).fill_(float("nan"))      # a k-split slice element never written reads back as NaN
                ops.tconv4x4s2p1_wide(pb.t, tb.t, bb.t if with_bias else None, ob.t)

            tag = "N%d %dx%dx%d -> %dx%dx%d%s" % (n, cin, ih, iw, cout, 2 * ih, 2 * iw, " bias" if with_bias else "")
            J.judge(lib, tag, expected, call, [pb, wb, tb, bb, ob], [(ob, None, ref, unit, "convT")], C_CONVT, WORST)
        # the 4 x 4 kernels on the same operands (unpadded input, parameter tensor), at the family's bound
        old = torch.full((n, cout, 2 * ih, 2 * iw), float("nan"), device=dev)
        ops.conv4x4(pb.t[:, :, 1:-1, 1:-1].contiguous(), wb.t, 16, cout * 16, cout, old, bias=bb.t, stride=2, pad=1, transposed=True)
        torch.cuda.synchronize()
        ratio, at = R.worst(ob.t.cpu(), old.cpu().double(), unit)
        print("%-58s vs vts_conv4x4 %.4f" % (tag, ratio))
        assert ratio <= C_CONVT, (chan, hw, n, ratio, at)


def test_tconv4x4s2p1_wide_refuses_bad_arguments(gpu):
    lib, ops, dev = gpu
    p = torch.zeros(1, 8, 14, 14, device=dev)
    out = torch.zeros(1, 6, 24, 24, device=dev)       # a tiled map (12 x 12 > 128 pixels) with Cout % 4 != 0: refused before any launch
    wt = torch.zeros(8 * 16 * 8, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.tconv4x4s2p1_wide(p, wt, None, out)


# ---- 2. the network ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def judges(case):
    """(float64 run, float32 run) of the restatement on the CPU, computed once per case and left unchanged"""
    c = U.CASES[case] if case in U.CASES else U.EXTRA_CASES[case]
    torch.set_num_threads(min(8, torch.get_num_threads()))
    return U.run_case(c, torch.float64), U.run_case(c, torch.float32)


@pytest.fixture(scope="module")
def gold():
    return U.load_fixture()


def build(c, dev):
    from models import networks

    G = networks.define_G(U.INPUT_NC, U.OUTPUT_NC, c["ngf"], c["net"], c["norm"], use_dropout=c["dropout"]).to(dev)
    G.load_state_dict(U.weights(c))
    G.train()
    return G


def run_hip(c, dev, pair=False, trace=None):
    """the HIP path's counterpart of unet_classic_restated.run_case"""
    from vts import engine

    G = build(c, dev)
    x = U.net_input(c).to(dev)
    xin = (x[:, :1].contiguous(), x[:, 1:].contiguous()) if pair else x
    masks = {i: m.to(dev) for i, m in U.dropout_masks(c).items()} or None
    engine.UC_TRACE = trace
    try:
        out, ctx = engine.unet_classic_forward(G, xin, keep=True, dropout_masks=masks)
        d_raw = (U.cotangent(c).to(dev) * (1.0 - out * out)).contiguous()      # through the Tanh: the engine takes the pre-tanh gradient
        engine.unet_classic_backward(G, ctx, d_raw)
    finally:
        engine.UC_TRACE = None
    torch.cuda.synchronize()
    res = {"out": out.clone()}
    res.update({"grad/" + k: p.grad.clone() for k, p in G.named_parameters()})
    res.update({"buf1/" + k: v.clone() for k, v in G.state_dict().items() if not U.is_param(k)})
    engine.unet_classic_forward(G, xin, keep=False, dropout_masks=masks)
    res.update({"buf2/" + k: v.clone() for k, v in G.state_dict().items() if not U.is_param(k)})
    G.eval()
    res["out_eval"] = engine.unet_classic_forward(G, xin, keep=False)[0].clone()
    torch.cuda.synchronize()
    return G, res


def check_case(case, c, res, gold=None):
    r64, r32 = judges(case)
    f32 = U.f32_distance(gold, case) if gold is not None else {}
    zero = {"grad/" + k for k in U.normed_bias_keys(c)}
    assert set(res) == set(r64)
    worst_grad = (0.0, None)
    for k, ref in r64.items():
        got = res[k]
        if ref.dtype == torch.long:
            assert int(got) == int(ref), k
            continue
        if k in zero:       # a bias in front of a normalisation: exactly zero here, rounding noise in autograd
            assert float(got.abs().max()) == 0.0, k
            continue
        e64 = U.rel_l2(got, ref)
        yard = f32.get(k, float("nan"))
        if k.startswith("grad/"):
            e32, e_cpu = U.rel_l2(got, r32[k]), U.rel_l2(r32[k], ref)
            print("%-18s %-44s HIP|f64 %.2e  HIP|f32 %.2e  restated f32|f64 %.2e  reference f32|f64 %.2e" % (case, k, e64, e32, e_cpu, yard))
            worst_grad = max(worst_grad, (min(e64, e32), k))
            assert min(e64, e32) < GRAD_TOL, (k, "HIP vs float64 %.3e" % e64, "HIP vs fp32 CPU %.3e" % e32, "fp32 CPU vs float64 %.3e" % e_cpu)
        else:
            tol = OUT_TOL if k == "out" else EVAL_TOL if k == "out_eval" else BUF_TOL
            print("%-18s %-44s HIP|f64 %.2e  bound %.0e  reference f32|f64 %.2e" % (case, k, e64, tol, yard))
            assert e64 < tol, (k, e64)
        if gold is not None:      # and against what the fixture itself stores (whole tensor or probe triple)
            d = U.check_stored(gold, "%s/%s" % (case, k), got)
            assert d < (GRAD_TOL if k.startswith("grad/") else BUF_TOL if k.startswith("buf") else EVAL_TOL) or \
                (k.startswith("grad/") and U.rel_l2(got, r32[k]) < GRAD_TOL), (k, d)
    print("%s: worst gradient distance to the nearer judge %.2e (%s)" % (case, worst_grad[0], worst_grad[1]))


@pytest.mark.parametrize("case", list(U.CASES))
def test_network_against_the_reference(gpu, gold, case):
    lib, ops, dev = gpu
    c = U.CASES[case]
    trace = []
    G, res = run_hip(c, dev, pair=case.startswith("c1"), trace=trace)
    check_case(case, c, res, gold)
    wide = [t for t in trace if t[2] > 80]
    for layer, role, cout, kern in wide:
        assert kern in WIDE_KERNELS, "%s %s with %d output channels ran %s: the 80-channel group loop" % (layer, role, cout, kern)
    if c["ngf"] == 24:
        # channels 24 .. 192: Cout 96 and 192, a 384-channel cat input; the new member at 1 x 1 -> 2 x 2 (up6) and as down adjoint
        assert {(t[0], t[1]) for t in wide} >= {("down2", "forward"), ("down6", "forward"), ("up6", "forward"), ("up4", "forward"),
                                                ("up3", "forward"), ("up4", "adjoint"), ("down4", "adjoint"), ("down6", "adjoint")}
        assert dict(((t[0], t[1]), t[3]) for t in trace)[("up6", "forward")].startswith("conv_flat_kernel<4, 16>")
        assert sum(t[3].startswith("conv_flat_kernel<4, 16>") for t in wide if t[1] == "forward" and t[0].startswith("up")) == 4      # up6 .. up3
        assert all(t[2] <= 80 for t in trace if t[0] in ("down0", "down1", "up0", "up1", "up2") and t[1] == "forward")
    else:
        assert not wide and len(trace) == 5 * G.num_downs - 2      # thin kernels only


@pytest.mark.parametrize("name", list(U.EXTRA_CASES))
def test_further_shape_against_the_restatement(gpu, name):
    """judged against the float64 restatement alone: 128 x 384, batch 1, ngf 24 under two seeds (the first one has a ReLU argument of
    4.2e-7 that the fp32 run takes on the other side: 8.8e-4 measured on the gradients behind it, within the bound), and ngf 41, whose
    82-channel layers are wide but no multiple of 4"""
    lib, ops, dev = gpu
    _, res = run_hip(U.EXTRA_CASES[name], dev)
    check_case(name, U.EXTRA_CASES[name], res)


# ---- 3. repeatability and graph capture ------------------------------------------------------------------------------------------------
def _pass(G, x, cot, masks):
    from vts import engine

    out, ctx = engine.unet_classic_forward(G, x, keep=True, dropout_masks=masks)
    d_raw = (cot * (1.0 - out * out)).contiguous()
    engine.unet_classic_backward(G, ctx, d_raw)
    return out


@pytest.mark.parametrize("case", ["c3_128_ngf24_bn", "c4_256_ngf8_drop"])
def test_two_runs_are_bitwise_equal(gpu, case):
    lib, ops, dev = gpu
    c = U.CASES[case]
    runs = []
    for _ in range(2):
        _, res = run_hip(c, dev)
        runs.append(res)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("case", ["c3_128_ngf24_in", "c2_128_ngf8_bn"])
def test_graph_replay_equals_the_eager_pass(gpu, case):
    lib, ops, dev = gpu
    c = U.CASES[case]
    x, cot = U.net_input(c).to(dev), U.cotangent(c).to(dev)
    G = build(c, dev)
    eager_out = _pass(G, x, cot, None).clone()        # also allocates every .grad, packed weight and scratch outside the capture
    torch.cuda.synchronize()
    eager = {k: p.grad.clone() for k, p in G.named_parameters()}
    eager_buf = {k: v.clone() for k, v in G.state_dict().items() if not U.is_param(k)}
    G.load_state_dict(U.weights(c))                    # the BatchNorm buffers back to their start
    ops.freeze_ws("unet-classic-test")
    graph = None
    try:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=torch.cuda.Stream(), capture_error_mode="thread_local"):      # as models/graphed_step.py captures
            out = _pass(G, x, cot, None)
        G.load_state_dict(U.weights(c))
        for p in G.parameters():
            p.grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager_out)
        for k, p in G.named_parameters():
            assert torch.equal(p.grad, eager[k]), k
        for k, v in G.state_dict().items():
            if not U.is_param(k):
                assert torch.equal(v, eager_buf[k]), k
    finally:
        del graph
        ops.release_ws("unet-classic-test")


# ---- 4. the model: --model sinskitG --netG unet_256 ------------------------------------------------------------------------------------
STEP_FLAGS = ("--model sinskitG --gpu_ids 0 --lambda_G1_lpips 0 --lambda_G2_lpips 0 --use_vision_aided_loss False --lambda_G2_GAN_feat 0 "
              "--checkpoints_dir /tmp/vts_test_ckpt --name unet_classic_gpu --crop_size %d --batch_size 1 %s")
STEP_TOL = 1e-3      # tests/test_step_gpu.py:test_step_variants_match_reference_golden


def probe_close(t, ref, name, rtol):
    p = detrand.probe(t.detach().cpu(), name)
    scale = max(abs(ref[1]), 1e-12)
    assert abs(p[1] - ref[1]) <= rtol * scale, (name, p, ref)
    assert abs(p[2] - ref[2]) <= 4 * rtol * scale, (name, p, ref)


def make_step_model(extra=""):
    import json

    from models import create_model
    from options.train_options import TrainOptions
    from oracle import nets

    s = U.STEP
    opt = TrainOptions(cmd_line=STEP_FLAGS % (s["size"], " ".join(s["flags"]) + extra)).parse()
    model = create_model(opt)
    model.setup(opt)
    model.parallelize()
    model.train()
    g = U.load_fixture()
    cfg = json.loads(str(g["step/cfg"]))
    c = dict(net=opt.netG, ngf=opt.ngf, norm=opt.normG, dropout=not opt.no_dropout, seed=s["seed"])
    sds = (U.weights(c, cfg["input_nc"]), detrand.test_weights(nets.d_param_shapes(4, n_layers=opt.n_layers_D), s["seed"] + 1),
           detrand.test_weights(nets.d_param_shapes(7, n_layers=opt.n_layers_D2), s["seed"] + 2))
    for net, sd in zip((model.netG, model.netD, model.netD2), sds):
        assert list(net.state_dict().keys()) == list(sd.keys())
        net.load_state_dict(sd)
    return model, opt, g, sds


def step_batch():
    from torch.utils.data import default_collate

    from data.synthetic_dataset import make_sample

    s = U.STEP
    return default_collate([make_sample(s["size"], s["nt"], s["nt"], s["seed"])])


def test_model_step_against_the_reference_step(gpu):
    """one SinSKITGModel.optimize_parameters with --netG unet_256 (ngf 10, InstanceNorm: every layer on the 4 x 4 kernels) against the
    reference's own step recorded under step/ of the fixture: losses, outputs, gradient and parameter probes of G, D and D2"""
    import json

    model, opt, g, _ = make_step_model()
    cfg = json.loads(str(g["step/cfg"]))
    assert (opt.ngf, opt.normG) == (cfg["ngf"], cfg["norm"]) and sum(p.numel() for p in model.netG.parameters()) == cfg["n_params"]
    model._draws = {"more_idx": torch.from_numpy(g["step/more_idx"]), "aug": torch.from_numpy(g["step/aug"])}
    model.set_input(step_batch(), phase="train")
    model.optimize_parameters(epoch=1)
    ref = dict(zip([str(s) for s in g["step/loss_names"]], g["step/loss_values"]))
    for k, v in model.get_current_losses().items():
        print("%-22s %.6f  reference %.6f" % (k, v, ref[k]))
        assert abs(v - ref[k]) <= STEP_TOL * max(1.0, abs(ref[k])), (k, v, ref[k])
    assert U.rel_l2(model.aug_fake_I[:, :, ::8, ::8], torch.from_numpy(g["step/aug_fake_I_sub"])) < STEP_TOL
    for nm in ("fake_I", "fake_T", "aug_fake_I", "aug_real_I", "pred_fake_T_full", "pred_fake_I"):
        key = {"pred_fake_T_full": "pftf", "pred_fake_I": "pfi"}.get(nm, nm)
        probe_close(getattr(model, nm).contiguous(), g["step/%s_probe" % nm], key, 2 * STEP_TOL)
    zero_bias = set(U.normed_bias_keys(dict(net=opt.netG, norm=opt.normG)))
    for nm, net in (("G", model.netG), ("D", model.netD), ("D2", model.netD2)):
        bn_convs = () if nm == "G" else tuple(str(c) for c in net.BN_IDX)
        for k, p in net.named_parameters():
            if (nm == "G" and k in zero_bias) or (nm != "G" and k.endswith("bias") and k.split(".")[1] in bn_convs):
                continue      # a bias in front of a normalisation: identically zero gradient, rounding noise in the reference
            probe_close(p.grad, g["step/grad_%s/%s" % (nm, k)], k, 2 * STEP_TOL)
            probe_close(p.data, g["step/param_%s/%s" % (nm, k)], k, STEP_TOL)
        for k, buf in net.named_buffers():
            refb = torch.from_numpy(g["step/buf_%s/%s" % (nm, k)])
            if k.endswith("running_mean"):
                scale = float(g["step/buf_%s/%s" % (nm, k.replace("running_mean", "running_var"))].max()) ** 0.5
                assert (buf.double().cpu() - refb).abs().max().item() < STEP_TOL * scale, (nm, k)
            elif buf.dtype.is_floating_point:
                assert U.rel_l2(buf, refb) < STEP_TOL, (nm, k)
            else:
                assert int(buf) == int(refb), (nm, k)


def test_model_replayed_step_equals_the_eager_step_and_inference_runs(gpu):
    """two models from the same state: one takes its steps eagerly, the other captures the step after its first one and replays it
    (--use_hip_graph); after three steps every parameter is bitwise the same.  Then test() (eager, captured, replayed) on both."""
    import contextlib
    import io

    batch = step_batch()
    models = []
    import random

    for flag in (" --use_diffaug False --use_hip_graph False", " --use_diffaug False --use_hip_graph True"):
        with contextlib.redirect_stdout(io.StringIO()):
            model, opt, g, _ = make_step_model(flag)
        random.seed(11)         # (the patch positions of the step: tests/test_style_levels_gpu.py does the same)
        torch.manual_seed(11)
        for _ in range(3):
            model.set_input(batch, phase="train")
            model.optimize_parameters(epoch=1)
        torch.cuda.synchronize()
        models.append(model)
    assert models[1]._graphs is not None and models[0]._graphs is None
    for nm in ("G", "D", "D2"):
        assert torch.equal(getattr(models[0], "flat" + nm).flat, getattr(models[1], "flat" + nm).flat), nm
        assert torch.equal(getattr(models[0], "optimizer_" + nm).m, getattr(models[1], "optimizer_" + nm).m), nm
    assert models[0].get_current_losses() == models[1].get_current_losses()
    outs = []
    for model in models:
        model.eval()
        for _ in range(3):
            model.set_input(batch, phase="test")
            model.test()
        torch.cuda.synchronize()
        outs.append((model.fake_I.clone(), model.fake_T.clone()))
        assert torch.isfinite(outs[-1][0]).all() and tuple(outs[-1][0].shape) == (1, 3, 256, 256) and tuple(outs[-1][1].shape)[:2] == (1, 2)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_checkpoint_round_trip_through_the_reference_keys(gpu, tmp_path):
    import contextlib
    import io

    with contextlib.redirect_stdout(io.StringIO()):
        model, opt, g, sds = make_step_model(" --normG batch")
    model.save_dir = str(tmp_path)
    model.save_networks("7")
    saved = torch.load(str(tmp_path / "7_net_G.pth"), map_location="cpu", weights_only=True)
    shapes, _ = U.param_shapes(dict(net=opt.netG, ngf=opt.ngf, norm="batch"), saved["model.model.0.weight"].shape[1])
    assert [(k, tuple(v.shape)) for k, v in saved.items()] == [(k, tuple(s)) for k, s in shapes.items()]      # the reference's keys, in its order
    before = {k: v.clone() for k, v in model.netG.state_dict().items()}
    with torch.no_grad():
        for p in model.netG.parameters():
            p.add_(1.0)
    model.load_networks("7")
    for k, v in model.netG.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_train_and_test_scripts_run_with_the_classic_unet(tmp_path):
    """the reference's flow: train.py --model sinskitG --netG unet_256 (with dropout: masks drawn on the device; first step eager, then
    replayed graphs), its checkpoint files, and test.py reloading the generator through the reference's keys"""
    import os
    import subprocess
    import sys

    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visual-tactile-synthesis_amd")
    common = ["--model", "sinskitG", "--netG", "unet_256", "--no_dropout", "False", "--gpu_ids", "0", "--dataset_mode", "synthetic",
              "--crop_size", "256", "--checkpoints_dir", str(tmp_path), "--name", "e2e_unet"]
    train = [sys.executable, os.path.join(pkg, "train.py")] + common + [
        "--lambda_G1_lpips", "0", "--lambda_G2_lpips", "0", "--use_vision_aided_loss", "False", "--data_len", "3", "--n_epochs", "1",
        "--n_epochs_decay", "0", "--print_freq", "1", "--save_latest_freq", "2", "--save_epoch_freq", "1", "--batch_size", "1"]
    out = subprocess.run(train, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = os.path.join(str(tmp_path), "e2e_unet")
    for f in ("latest_net_G.pth", "latest_net_D.pth", "latest_net_D2.pth", "loss_log.txt"):
        assert os.path.exists(os.path.join(d, f)), f
    sd = torch.load(os.path.join(d, "latest_net_G.pth"), map_location="cpu", weights_only=True)
    assert len(sd) == 32 and list(sd)[:2] == ["model.model.0.weight", "model.model.0.bias"] and all(torch.isfinite(v).all() for v in sd.values())
    log = open(os.path.join(d, "loss_log.txt")).read()
    assert "l_G_GAN" in log and "l_G2_L1" in log and "nan" not in log.lower()
    test = [sys.executable, os.path.join(pkg, "test.py")] + common + ["--epoch", "latest", "--eval", "--results_dir", str(tmp_path / "res"),
                                                                       "--num_test", "2", "--data_len", "2"]
    out = subprocess.run(test, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count("processed synthetic_") == 2
