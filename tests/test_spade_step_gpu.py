"""SPADE baseline step on the HIP path (models/spade_model.py) through create_model, against tests/golden/spade_step_32.npz: the REFERENCE's
SPADEModel run in float64 on the CPU (tools/make_spade_step_golden.py), two optimize_parameters calls per case; plus the pieces the step
adds: the stacked VGG input and its adjoint, the stacked VGG feature term, and spade_backward without the sketch gradient.

Cases: `default` (hinge, two-time-scale rates, sync-batch SPADE, VGG term on stand-in weights) and `B` (--no_TTUR, lsgan, no VGG term,
instance SPADE).  ngf 8, ndf 8, N = 4, 32 x 32.  Every comparison prints its figure, and the reference's own float32-to-float64 distance
the fixture stores (f32/...), before it asserts.
"""
import json
import os

import numpy as np
import pytest
import torch

import spade_restated as R
from oracle import detrand

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spade_step_32.npz")
DEV = "cuda"
COMMON = " --gpu_ids 0 --checkpoints_dir /tmp/vts_test_ckpt --name spade --dataset_mode patchskit"
NETS = ("G", "D", "D2")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN, allow_pickle=False)


def p2p_batch(n, size, seed):
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    M = (((yy - size / 2) / (0.45 * size)) ** 2 + ((xx - size / 2) / (0.4 * size)) ** 2 <= 1).float()[None, None].repeat(n, 1, 1, 1)
    return {"S_images": detrand.uniform((n, 1, size, size), seed, "S"), "M_images": M,
            "I_images": detrand.uniform((n, 3, size, size), seed, "I"), "T_images": 0.3 * detrand.uniform((n, 2, size, size), seed, "T"),
            "I_masks": torch.ones(n, size, size, dtype=torch.float64), "name": ["synthetic"] * n, "S_paths": ["synthetic.png"] * n,
            "augmentation_params": {}}


def case_flags(gold, case):
    return " ".join(json.loads(str(gold[case + "/flags"]))) + COMMON


def make_model(gold, case, extra="", train=True, save_dir=None):
    """the fixture's flags; a non-default normG is set on the parsed options (the base parser's `choices` do not list it, as upstream)"""
    from models import create_model
    from options.test_options import TestOptions
    from options.train_options import TrainOptions

    opt = (TrainOptions if train else TestOptions)(cmd_line=case_flags(gold, case) + extra).parse()
    for k, v in json.loads(str(gold[case + "/override"])).items():
        setattr(opt, k, v)
    model = create_model(opt)
    if save_dir is not None:
        model.save_dir = save_dir
    model.setup(opt)
    model.parallelize()
    (model.train if train else model.eval)()
    return model


def seed_weights(gold, case, model):
    keys = json.loads(str(gold[case + "/keys"]))
    seed = int(gold[case + "/seed"])
    for i, nm in enumerate(NETS):
        net = getattr(model, "net" + nm)
        shapes = {k: tuple(s) for k, s in keys[nm]}
        assert list(net.state_dict().keys()) == list(shapes), nm
        net.load_state_dict(R.weights(shapes, seed) if nm == "G" else detrand.test_weights(shapes, seed + i))


def snapshot(model):
    rec = {"losses": model.get_current_losses(), "fake_I": model.fake_I.clone(), "fake_T": model.fake_T.clone()}
    for nm in NETS:
        net = getattr(model, "net" + nm)
        rec["grad_" + nm] = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
        rec["buf_" + nm] = {k: b.detach().cpu().clone() for k, b in net.named_buffers()}
    return rec


_RUNS = {}


def two_eager_steps(gold, case):
    """two eager optimize_parameters calls from the seed weights on the fixture's batch, run once per case and shared by the tests below"""
    if case not in _RUNS:
        model = make_model(gold, case, " --use_hip_graph False")
        seed_weights(gold, case, model)
        batch = p2p_batch(int(gold["n"]), int(gold["size"]), int(gold[case + "/seed"]))
        recs = []
        for _ in range(2):
            model.set_input(batch, phase="train")
            model.optimize_parameters(epoch=1)
            recs.append(snapshot(model))
        _RUNS[case] = recs
    return _RUNS[case]


@pytest.mark.parametrize("case", ["default", "B"])
def test_first_step_matches_the_reference(gold, case):
    """losses 1e-3 max(1, |v|), outputs 1e-3 relative L2, gradient probe l2 within 2e-3, float buffers (weight_u, weight_v and the running
    statistics included) within 1e-3 max(1, max|ref|): the bounds of test_pix2pixHD_gpu.py::test_step_matches_reference_golden.  The
    tensors whose float64 gradient is zero (biases in front of a normalisation; the fixture names them) are not skipped: their gradient
    norm here is <= 1e-6 of their network's largest."""
    rec = two_eager_steps(gold, case)[0]
    f32 = json.loads(str(gold["f32/%s/s0" % case]))
    tag = case + "/s0"
    ref = dict(zip([str(k) for k in gold[tag + "/loss_names"]], gold[tag + "/loss_values"]))
    assert list(rec["losses"]) == list(ref)
    worst = max(abs(rec["losses"][k] - v) / max(1.0, abs(v)) for k, v in ref.items())
    print(case, "losses: worst scaled error %.2e (reference float32: %.2e)" % (worst, max(v for k, v in f32.items() if k.startswith("loss/"))))
    for k, v in ref.items():
        assert abs(rec["losses"][k] - v) <= 1e-3 * max(1.0, abs(v)), (k, rec["losses"][k], v)
    for k in ("fake_I", "fake_T"):
        d = R.rel_l2(rec[k], torch.from_numpy(gold["%s/%s" % (tag, k)]))
        print(case, k, "relative L2 %.2e (reference float32: %.2e)" % (d, f32[k]))
        assert d < 1e-3, (k, d)
    zero = json.loads(str(gold[case + "/zero_grads"]))
    assert sum(len(v) for v in zero.values()) <= 27, zero
    for nm in NETS:
        names = json.loads(str(gold["%s/param_names_%s" % (case, nm)]))
        probes = gold["%s/grad_%s" % (tag, nm)]
        assert list(rec["grad_" + nm]) == names
        top = float(probes[:, 1].max())
        worst, worst_zero = (0.0, None), 0.0
        for k, rp in zip(names, probes):
            g = rec["grad_" + nm][k]
            if k in zero[nm]:
                worst_zero = max(worst_zero, g.double().norm().item() / top)
                continue
            pr = detrand.probe(g, k)
            worst = max(worst, (abs(pr[1] - rp[1]) / abs(rp[1]), k))
        yard = max(v for k, v in f32.items() if k.startswith("grad_%s/" % nm))
        print(case, nm, "gradient l2: worst relative error %.2e at %s (reference float32, relative L2: %.2e); zero-gradient tensors %.2e of the largest"
              % (worst[0], worst[1], yard, worst_zero))
        assert worst[0] <= 2e-3, (nm, worst)
        assert worst_zero <= 1e-6, (nm, worst_zero)
        flat, o, worst_b = torch.from_numpy(gold["%s/buf_%s" % (tag, nm)]).double(), 0, 0.0
        bufs = rec["buf_" + nm]
        assert list(bufs) == [k for k, _ in json.loads(str(gold["%s/buf_names_%s" % (case, nm)]))]
        for k, b in bufs.items():
            rb = flat[o:o + b.numel()].reshape(b.shape)
            o += b.numel()
            err = (b.double() - rb).abs().max().item() / max(1.0, float(rb.abs().max()))
            worst_b = max(worst_b, err)
            assert err <= 1e-3, (nm, k, err)
        assert o == flat.numel()
        print(case, nm, "buffers: worst scaled error %.2e" % worst_b)


@pytest.mark.parametrize("case", ["default", "B"])
def test_second_step_matches_the_reference(gold, case):
    """The same model one step on: losses within 2e-3 max(1, |v|) (the reference's own two precisions differ by 6e-5), outputs within
    max(1e-3, 4 x the reference's own float32-to-float64 distance at this step; the factor 4 is headroom for another summation order).
    The gradients of step 2 are NOT compared: with beta1 = 0 the first Adam update is lr sign(g), so on noise-level gradients (the biases in
    front of a normalisation) the parameters after step 1 depend on rounding, and the reference's own float32 and float64 runs are then
    4e-2 to 6e-2 apart on some step-2 gradients."""
    rec = two_eager_steps(gold, case)[1]
    f32 = json.loads(str(gold["f32/%s/s1" % case]))
    tag = case + "/s1"
    ref = dict(zip([str(k) for k in gold[tag + "/loss_names"]], gold[tag + "/loss_values"]))
    worst = max(abs(rec["losses"][k] - v) / max(1.0, abs(v)) for k, v in ref.items())
    print(case, "step 2 losses: worst scaled error %.2e (reference float32: %.2e)" % (worst, max(v for k, v in f32.items() if k.startswith("loss/"))))
    for k, v in ref.items():
        assert abs(rec["losses"][k] - v) <= 2e-3 * max(1.0, abs(v)), (k, rec["losses"][k], v)
    for k in ("fake_I", "fake_T"):
        d = R.rel_l2(rec[k], torch.from_numpy(gold["%s/%s" % (tag, k)]))
        bound = max(1e-3, 4 * f32[k])
        print(case, "step 2", k, "relative L2 %.2e, bound %.2e (reference float32: %.2e)" % (d, bound, f32[k]))
        assert d <= bound, (k, d, bound)


def test_graph_replay_equals_eager(gold):
    """three steps, captured graphs from the second on, against three eager steps from the same seeds: bit for bit"""
    batch = p2p_batch(int(gold["n"]), int(gold["size"]), int(gold["default/seed"]))
    res = []
    for extra in ("", " --use_hip_graph False"):
        model = make_model(gold, "default", extra)
        seed_weights(gold, "default", model)
        for _ in range(3):
            model.set_input(batch, phase="train")
            model.optimize_parameters(epoch=1)
        torch.cuda.synchronize()
        res.append((model, model.get_current_losses()))
    (mg, lg), (me, le) = res
    assert mg._graphs is not None and me._graphs is None
    print("graph nodes per segment (nodes, kernel nodes):", mg.graph_nodes)
    assert lg == le, (lg, le)
    for f in ("flatG", "flatD", "flatD2"):
        assert torch.equal(getattr(mg, f).flat, getattr(me, f).flat), f
    us = [(k, b) for k, b in mg.netG.named_buffers() if k.endswith("weight_u")]
    eb = dict(me.netG.named_buffers())
    assert us and all(torch.equal(b, eb[k]) for k, b in us)


@pytest.mark.parametrize("case", ["default", "B"])
def test_inference_and_checkpoint(gold, case, tmp_path):
    model = make_model(gold, case, save_dir=str(tmp_path))
    seed_weights(gold, case, model)
    model.save_networks("latest")
    keys = json.loads(str(gold[case + "/keys"]))
    for nm in NETS:
        saved = torch.load(os.path.join(str(tmp_path), "latest_net_%s.pth" % nm))
        assert list(saved.keys()) == [k for k, _ in keys[nm]], nm
    tm = make_model(gold, case, " --return_patch True --output_width 32", train=False, save_dir=str(tmp_path))
    assert tm.model_names == ["G"]
    assert all(torch.equal(v, dict(tm.netG.state_dict())[k]) for k, v in model.netG.state_dict().items())
    tm.set_input(p2p_batch(int(gold["n"]), int(gold["size"]), int(gold[case + "/seed"])), phase="test")
    tm.test()
    f32 = json.loads(str(gold["f32/%s/eval" % case]))
    for k in ("fake_I", "fake_T"):
        d = R.rel_l2(getattr(tm, k), torch.from_numpy(gold["%s/eval/%s" % (case, k)]))
        print(case, "eval", k, "relative L2 %.2e (reference float32: %.2e)" % (d, f32[k]))
        assert d < 1e-3, (k, d)


@pytest.mark.parametrize("case", ["default", "B"])
def test_update_learning_rate_gives_the_reference_rates(gold, case):
    """all three optimisers land on old_lr - lr / niter_decay: the two-time-scale ratio is gone after the first call, as upstream"""
    model = make_model(gold, case)
    g_lr, d_lr = model.learning_rates(model.opt)
    assert [o.param_groups[0]["lr"] for o in (model.optimizer_G, model.optimizer_D, model.optimizer_D2)] == [g_lr, d_lr, d_lr]
    model.update_learning_rate()
    got = [o.param_groups[0]["lr"] for o in (model.optimizer_G, model.optimizer_D, model.optimizer_D2)]
    ref = [float(v) for v in gold[case + "/lrs_after_update"]]
    print(case, got, ref)
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got, ref)), (got, ref)


# ---- the stacked VGG input and its adjoint ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (4, 32, 32)])
def test_vgg_stack_input_and_adjoint_are_torch_indexing(n, h, w):
    """exact: copies, and sums of three added in the stated order.  fake_T is a channel view of a wider tensor (odd sizes take the scalar
    adjoint, 32 x 32 the 4-wide one); both accumulate values; the border is exactly zero"""
    from vts import ops

    fake_I, real_I = detrand.uniform((n, 3, h, w), 1, "fI").to(DEV), detrand.uniform((n, 3, h, w), 1, "rI").to(DEV)
    wide = detrand.uniform((n, 5, h, w), 1, "wide").to(DEV)
    fake_T, real_T = wide[:, 3:5], detrand.uniform((n, 2, h, w), 1, "rT").to(DEV)
    assert not fake_T.is_contiguous()
    out = ops.vgg_stack_input(fake_I, fake_T, real_I, real_T)
    rows = [fake_I] + [fake_T[:, c:c + 1].expand(-1, 3, -1, -1) for c in (0, 1)] + [real_I] + [real_T[:, c:c + 1].expand(-1, 3, -1, -1) for c in (0, 1)]
    want = torch.zeros(6 * n, 3, h + 2, w + 2, device=DEV)
    want[:, :, 1:-1, 1:-1] = torch.cat(rows, 0)
    assert out.shape == want.shape and torch.equal(out, want)
    border = out.clone()
    border[:, :, 1:-1, 1:-1] = 0
    assert not border.any()
    dx = detrand.uniform((3 * n, 3, h, w), 2, "dx").to(DEV)
    want_I = dx[:n]
    want_T = torch.stack([dx[(1 + c) * n:(2 + c) * n, 0] + dx[(1 + c) * n:(2 + c) * n, 1] + dx[(1 + c) * n:(2 + c) * n, 2] for c in (0, 1)], 1)
    for accumulate in (False, True):
        d_I = detrand.uniform((n, 3, h, w), 3, "dI").to(DEV)
        d_wide = detrand.uniform((n, 5, h, w), 3, "dwide").to(DEV)
        before_I, before_wide = d_I.clone(), d_wide.clone()
        ops.vgg_stack_input_bwd(dx, d_I, d_wide[:, 3:5], accumulate=accumulate)
        assert torch.equal(d_I, before_I + want_I if accumulate else want_I), accumulate
        assert torch.equal(d_wide[:, 3:5], before_wide[:, 3:5] + want_T if accumulate else want_T), accumulate
        assert torch.equal(d_wide[:, :3], before_wide[:, :3])       # the channels in front of the view are untouched


def test_stacked_vgg_term_equals_three_separate_terms():
    """vgg_feature_l1_stacked against three vgg_feature_l1 calls (what the pix2pixHD step does) at N = 2, 16 x 16: the same arithmetic per
    row, another order of summation only -- slots 1e-6 relative, gradients 1e-5 relative L2"""
    from models import perceptual as MP
    from vts import ops
    from vts import perceptual as P

    n, s, lam = 2, 16, 10.0
    net = MP.build_vgg19(None, torch.device(DEV))
    fake_I, real_I = detrand.uniform((n, 3, s, s), 5, "fI").to(DEV), detrand.uniform((n, 3, s, s), 5, "rI").to(DEV)
    fake_T, real_T = 0.3 * detrand.uniform((n, 2, s, s), 5, "fT").to(DEV), 0.3 * detrand.uniform((n, 2, s, s), 5, "rT").to(DEV)
    slots = ops.loss_slots(4, DEV)
    d_I, d_T = P.vgg_feature_l1_stacked(net, fake_I, fake_T, real_I, real_T, lam, slots[0:1], slots[1:2])
    want_I = P.vgg_feature_l1(net, fake_I, real_I, lam, slots[2:3])
    want_T = torch.empty_like(d_T)
    for c in (0, 1):
        f3, r3 = (t[:, c:c + 1].expand(-1, 3, -1, -1).contiguous() for t in (fake_T, real_T))
        g3 = P.vgg_feature_l1(net, f3, r3, lam, slots[3:4])
        want_T[:, c] = g3[:, 0] + g3[:, 1] + g3[:, 2]
    v = ops.loss_values(slots)
    eI, eT = abs(v[0] - v[2]) / abs(v[2]), abs(v[1] - v[3]) / abs(v[3])
    gI, gT = R.rel_l2(d_I, want_I), R.rel_l2(d_T, want_T)
    print("slots", v, "relative differences %.2e %.2e; gradients relative L2 %.2e %.2e" % (eI, eT, gI, gT))
    assert v[2] > 0 and v[3] > 0 and eI <= 1e-6 and eT <= 1e-6
    assert gI <= 1e-5 and gT <= 1e-5


def test_spade_backward_without_the_sketch_gradient():
    """want_dseg=False returns None and leaves every parameter gradient bit-identical to the want_dseg=True run; so does pre_tanh=True
    given the gradient of the pre-tanh output"""
    from models import networks
    from vts import engine
    from vts.optim import FlatParams

    c = R.GEN_CASES["g8"]
    G = networks.define_G(c["input_nc"], c["output_nc"], c["ngf"], "spade", norm=c["normG"], opt=R.gen_opt("g8"), gpu_ids=[0])
    G.load_state_dict(R.weights({k: tuple(v.shape) for k, v in G.state_dict().items()}, c["seed"]))
    G.train()
    flat = FlatParams(G)
    h, w = R.gen_out_hw(c)
    seg = R.seg_input(c["N"], c["input_nc"], h, w, c["seed"]).to(DEV)
    out, ctx = engine.spade_forward(G, seg)
    cot = R.cotangent(out.shape, c["seed"]).to(DEV)
    flat.grad.fill_(float("nan"))
    dseg = engine.spade_backward(G, ctx, cot)
    with_dseg = flat.grad.clone()
    flat.grad.fill_(float("nan"))
    none = engine.spade_backward(G, ctx, cot, want_dseg=False)
    assert dseg is not None and none is None
    assert not torch.isnan(with_dseg).any() and torch.equal(flat.grad, with_dseg)
    # pre_tanh: the caller has already applied the tanh adjoint (what ops.g_out_grad hands the training step)
    from vts import ops
    flat.grad.fill_(float("nan"))
    engine.spade_backward(G, ctx, ops.tanh_bwd(cot.contiguous(), ctx.out), want_dseg=False, pre_tanh=True)
    assert torch.equal(flat.grad, with_dseg)
