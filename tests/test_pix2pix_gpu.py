"""pix2pix baseline on the HIP path (models/pix2pix_model.py) through create_model, against tests/golden/pix2pix_step_32.npz: the
REFERENCE's Pix2PixModel run in float64 on the CPU (tools/make_pix2pix_step_golden.py), two optimize_parameters calls per case, and its
eval-mode outputs on both input contracts; plus the piece the model adds to the networks: the single PatchGAN of define_D('basic' |
'n_layers') and the loss the reference takes of its output, against float64 autograd of a plain-torch restatement kept below.

Cases: `default` (resnet_9blocks anti-aliased, netD basic, vanilla, lambda_L1 100) and `B` (resnet_6blocks with strided / transposed
convolutions, netD n_layers of depth 2, lsgan, lambda_L1 10).  ngf 8, ndf 8, N = 4, 32 x 32.  Every comparison prints its figure, and the
reference's own float32-to-float64 distance the fixture stores (f32/...), before it asserts.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import detrand, nets

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pix2pix_step_32.npz")
DEV = "cuda"
COMMON = " --gpu_ids 0 --checkpoints_dir /tmp/vts_test_ckpt --name pix2pix --dataset_mode patchskit"
NETS = ("G", "D", "D2")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN, allow_pickle=False)


def rel_l2(a, b):
    """true relative L2 of a against the judge b (both moved to float64 on the CPU)"""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def ellipse(n, h, w):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return (((yy - h / 2) / (0.45 * h)) ** 2 + ((xx - w / 2) / (0.4 * w)) ** 2 <= 1).float()[None, None].repeat(n, 1, 1, 1)


def p2p_batch(n, size, seed):
    return {"S_images": detrand.uniform((n, 1, size, size), seed, "S"), "M_images": ellipse(n, size, size),
            "I_images": detrand.uniform((n, 3, size, size), seed, "I"), "T_images": 0.3 * detrand.uniform((n, 2, size, size), seed, "T"),
            "I_masks": torch.ones(n, size, size, dtype=torch.float64), "name": ["synthetic"] * n, "S_paths": ["synthetic.png"] * n,
            "augmentation_params": {}}


def full_batch(h, w, nt, size, seed):
    """one full image with nt tactile patches (return_patch=False), as tools/make_pix2pix_step_golden.py:full_batch builds it"""
    coords = torch.tensor([[[4 * k, 2 * k, 4 * k + size, 2 * k + size, 0, 0, 0, 0] for k in range(nt)]], dtype=torch.float32)
    return {"S": detrand.uniform((1, 1, h, w), seed, "fS"), "M": ellipse(1, h, w), "I": detrand.uniform((1, 3, h, w), seed, "fI"),
            "T_images": 0.3 * detrand.uniform((1, nt, 2, size, size), seed, "fT"), "I_masks": torch.ones(1, nt, size, size, dtype=torch.float64),
            "T_coords": coords, "full_T_coords": coords.clone(), "name": ["synthetic"], "S_paths": ["synthetic.png"], "augmentation_params": {}}


def case_flags(gold, case):
    return " ".join(json.loads(str(gold[case + "/flags"]))) + COMMON


def make_model(gold, case, extra="", train=True, save_dir=None):
    from models import create_model
    from options.test_options import TestOptions
    from options.train_options import TrainOptions

    opt = (TrainOptions if train else TestOptions)(cmd_line=case_flags(gold, case) + extra).parse()
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
        assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == keys[nm], nm
        # (the `filt` buffers of the anti-aliasing modules are constants: kept as constructed, as the fixture's tool does)
        sd = detrand.test_weights({k: s for k, s in shapes.items() if not k.endswith(".filt")}, seed + i)
        net.load_state_dict({**{k: v for k, v in net.state_dict().items() if k.endswith(".filt")}, **sd})


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


# ---- 1. define_D("basic" | "n_layers") alone -------------------------------------------------------------------------------------------
def torch_patchgan(cin, ndf, n_layers):
    """plain-torch restatement of the single PatchGAN: 4x4 convolutions with padding 2; stride 2 for the first n_layers of them, then two of
    stride 1, the last one to a single channel; BatchNorm behind every convolution but the first and the last; LeakyReLU(0.2) between"""
    mods = [nn.Conv2d(cin, ndf, 4, 2, 2), nn.LeakyReLU(0.2)]
    c = ndf
    for j in range(1, n_layers + 1):
        c2 = min(2 * c, 512)
        mods += [nn.Conv2d(c, c2, 4, 2 if j < n_layers else 1, 2), nn.BatchNorm2d(c2), nn.LeakyReLU(0.2)]
        c = c2
    mods.append(nn.Conv2d(c, 1, 4, 1, 2))
    return nn.Sequential(*mods)


def torch_gan_loss(pred, real, mode, label):
    """the reference's loss of one prediction map per sample, mean over the batch (networks.py:500-522)"""
    if mode == "lsgan":
        return F.mse_loss(pred, torch.full_like(pred, label))
    if mode == "vanilla":
        return F.binary_cross_entropy_with_logits(pred, torch.full_like(pred, label))
    if mode == "wgan":
        return -pred.mean() if real else pred.mean()
    sign = -1.0 if real else 1.0
    per = F.softplus(sign * pred) if mode == "nonsaturating" else F.relu(1.0 + sign * pred)
    return per.reshape(pred.shape[0], -1).mean(1).mean()


@pytest.mark.parametrize("netD,n_layers,cin,n,h,w,mode,case,net", [("basic", 3, 4, 4, 32, 32, "vanilla", "default", "D"),
                                                                     ("n_layers", 2, 3, 2, 37, 29, "lsgan", "B", "D2")])
def test_single_patchgan_against_float64_autograd(gold, netD, n_layers, cin, n, h, w, mode, case, net):
    """keys and shapes against the fixture's lists; prediction map, BatchNorm running statistics, loss, the gradient into the second concat
    source and every parameter gradient against float64 autograd: the bounds of tests/test_discriminator_gpu.py (1e-3 forward, buffers and
    loss, 2e-3 gradients).  The loss here is GANLoss over ALL samples with label 0.8, so every sample's map carries a gradient."""
    from models import networks
    from vts import engine, ops

    seed = 41 + n_layers
    D = networks.define_D(cin, 8, netD, 7 if netD == "basic" else n_layers, "batch", "xavier", 0.02, False, gpu_ids=[0],
                          opt=SimpleNamespace(gan_mode="vanilla"))
    keys = json.loads(str(gold[case + "/keys"]))[net]
    assert [[k, list(v.shape)] for k, v in D.state_dict().items()] == keys
    assert D.num_D == 1 and D.use_sigmoid is False
    sd = detrand.test_weights({k: tuple(s) for k, s in keys}, seed)
    D.load_state_dict(sd)
    D.train()
    ref = torch_patchgan(cin, 8, n_layers).double()
    assert list(ref.state_dict().keys()) == [k[len("model."):] for k, _ in keys]
    ref.load_state_dict({k[len("model."):]: (v if v.dtype == torch.long else v.double()) for k, v in sd.items()})
    ref.train()
    x0 = detrand.uniform((n, 1, h, w), seed, "x0")
    x1 = detrand.uniform((n, cin - 1, h, w), seed, "x1")
    x1r = x1.double().requires_grad_(True)
    pred_ref = ref(torch.cat([x0.double(), x1r], 1))
    loss_ref = torch_gan_loss(pred_ref, True, mode, 0.8) * 2.5
    loss_ref.backward()
    for p in D.parameters():
        p.grad = torch.full_like(p, float("nan"))
    crit = networks.GANLoss(mode, target_real_label=0.8)
    preds, ctx = engine.msd_forward(D, x0.to(DEV), x1.to(DEV), keep=True)
    assert len(preds) == 1 and preds[0].shape == pred_ref.shape
    slot = ops.loss_slots(1, DEV)
    dp = crit.accumulate(preds, True, 2.5, slot)
    din = torch.full((n, cin - 1, h, w), float("nan"), device=DEV)
    engine.msd_backward(D, ctx, dp, param_grads=True, accumulate=False, input_grad=(din, False))
    torch.cuda.synchronize()
    e_pred = rel_l2(preds[0], pred_ref)
    e_loss = abs(ops.loss_values(slot)[0] - loss_ref.item()) / max(1.0, abs(loss_ref.item()))
    print(netD, "prediction %s relative L2 %.2e, loss scaled error %.2e" % (tuple(preds[0].shape), e_pred, e_loss))
    assert e_pred < 1e-3 and e_loss <= 1e-3
    rsd = ref.state_dict()
    for k, b in D.named_buffers():
        rb = rsd[k[len("model."):]]
        if not b.dtype.is_floating_point:
            assert int(b) == int(rb) == 1, k
        elif k.endswith("running_mean"):
            scale = float(rsd[k[len("model."):].replace("running_mean", "running_var")].max().sqrt())
            assert (b.cpu().double() - rb).abs().max().item() < 1e-3 * scale, k
        else:
            assert rel_l2(b, rb) < 1e-3, k
    worst = (0.0, None)
    rp = dict(ref.named_parameters())
    for k, p in D.named_parameters():
        idx = int(k.split(".")[1])
        if k.endswith("bias") and idx in D.BN_IDX:      # conv bias in front of a BatchNorm: identically zero gradient, never written
            assert torch.isnan(p.grad).all(), k
            continue
        worst = max(worst, (rel_l2(p.grad, rp[k[len("model."):]].grad), k))
    e_in = rel_l2(din, x1r.grad)
    print(netD, "worst parameter gradient relative L2 %.2e at %s, input gradient %.2e" % (worst[0], worst[1], e_in))
    assert worst[0] < 2e-3 and e_in < 2e-3
    # the module's own forward takes the concatenated input and returns the map itself, not a list
    out = D(torch.cat([x0, x1], 1).to(DEV))
    assert torch.is_tensor(out) and out.shape == pred_ref.shape
    # (a second training-mode pass over the same batch: the same batch statistics, so the same map)
    assert rel_l2(out, pred_ref) < 1e-3


@pytest.mark.parametrize("mode", ["vanilla", "lsgan", "hinge", "nonsaturating", "wgan"])
def test_gan_loss_of_a_tensor_is_the_last_sample_s(mode):
    """GANLossLastSample against the reference's indexing restated: criterion(pred, real) with pred a TENSOR evaluates pred[-1].  Value
    1e-5 max(1, |v|), gradient 1e-5 relative L2 (elementwise float32 arithmetic on 77 values against float64); rows 0 .. N-2 exactly zero."""
    from models import networks
    from vts import ops

    crit = networks.GANLossLastSample(mode)
    for real in (True, False):
        p = (detrand.uniform((3, 1, 7, 11), 13, "p" + mode) * 3).double().requires_grad_(True)
        last = p[-1]
        ref = torch_gan_loss(last[None], real, mode, 1.0 if real else 0.0) * 0.5
        ref.backward()
        slot = ops.loss_slots(1, DEV)
        g = crit.accumulate([p.detach().float().to(DEV)], real, 0.5, slot, grad_coeff=0.5)[0]
        v = ops.loss_values(slot)[0]
        assert abs(v - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (mode, real, v, ref.item())
        assert not g[:-1].any() and rel_l2(g[-1], p.grad[-1]) < 1e-5, (mode, real)
        assert abs(float(crit(p.detach().float().to(DEV), real)) - 2 * ref.item()) <= 1e-5 * max(1.0, abs(2 * ref.item()))


# ---- 2. / 3. the training step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["default", "B"])
def test_first_step_matches_the_reference(gold, case):
    """losses 1e-3 max(1, |v|), outputs 1e-3 relative L2, gradient probe l2 within 2e-3, float buffers within 1e-3 max(1, max|ref|): the
    bounds of the SPADE and pix2pixHD step tests.  The tensors whose float64 gradient is zero (the discriminators' conv biases in front of
    a BatchNorm; the fixture names them) are not skipped: their gradient norm here is <= 1e-6 of their network's largest."""
    rec = two_eager_steps(gold, case)[0]
    f32 = json.loads(str(gold["f32/%s/s0" % case]))
    tag = case + "/s0"
    ref = dict(zip([str(k) for k in gold[tag + "/loss_names"]], gold[tag + "/loss_values"]))
    assert list(rec["losses"]) == list(ref) == ["l_" + n for n in ("G_GAN", "G_L1", "D_real", "D_fake", "D2_real", "D2_fake")]
    worst = max(abs(rec["losses"][k] - v) / max(1.0, abs(v)) for k, v in ref.items())
    print(case, "losses: worst scaled error %.2e (reference float32: %.2e)" % (worst, max(v for k, v in f32.items() if k.startswith("loss/"))))
    for k, v in ref.items():
        assert abs(rec["losses"][k] - v) <= 1e-3 * max(1.0, abs(v)), (k, rec["losses"][k], v)
    for k in ("fake_I", "fake_T"):
        d = rel_l2(rec[k], torch.from_numpy(gold["%s/%s" % (tag, k)]))
        print(case, k, "relative L2 %.2e (reference float32: %.2e)" % (d, f32[k]))
        assert d < 1e-3, (k, d)
    zero = json.loads(str(gold[case + "/zero_grads"]))
    n_bn = {"default": 3, "B": 2}[case]
    assert {nm: len(v) for nm, v in zero.items()} == {"G": 0, "D": n_bn, "D2": n_bn}, zero
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
    """The same model one step on: losses within 2e-3 max(1, |v|), outputs within max(1e-3, 4 x the reference's own float32-to-float64
    distance at this step).  The gradients of step 2 and the post-Adam values of the zero-gradient tensors are NOT compared: in float64 the
    reference's gradient of a bias in front of a BatchNorm is rounding noise, Adam moves that bias by +- lr per step, and the HIP path never
    writes such a gradient (tests/test_spade_step_gpu.py::test_second_step_matches_the_reference)."""
    rec = two_eager_steps(gold, case)[1]
    f32 = json.loads(str(gold["f32/%s/s1" % case]))
    tag = case + "/s1"
    ref = dict(zip([str(k) for k in gold[tag + "/loss_names"]], gold[tag + "/loss_values"]))
    worst = max(abs(rec["losses"][k] - v) / max(1.0, abs(v)) for k, v in ref.items())
    print(case, "step 2 losses: worst scaled error %.2e (reference float32: %.2e)" % (worst, max(v for k, v in f32.items() if k.startswith("loss/"))))
    for k, v in ref.items():
        assert abs(rec["losses"][k] - v) <= 2e-3 * max(1.0, abs(v)), (k, rec["losses"][k], v)
    for k in ("fake_I", "fake_T"):
        d = rel_l2(rec[k], torch.from_numpy(gold["%s/%s" % (tag, k)]))
        bound = max(1e-3, 4 * f32[k])
        print(case, "step 2", k, "relative L2 %.2e, bound %.2e (reference float32: %.2e)" % (d, bound, f32[k]))
        assert d <= bound, (k, d, bound)


# ---- 4. captured graphs ----------------------------------------------------------------------------------------------------------------
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
    assert len(mg.graph_nodes) == 3 and all(k > 0 for _, k in mg.graph_nodes)
    assert lg == le, (lg, le)
    for f in ("flatG", "flatD", "flatD2"):
        assert torch.equal(getattr(mg, f).flat, getattr(me, f).flat), f


# ---- 5. checkpoint round trip and inference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["default", "B"])
def test_inference_and_checkpoint(gold, case, tmp_path):
    """saved keys = the fixture's; a test-phase model loads G only; its eval-mode outputs on one 48 x 40 image with three tactile patches
    (the test phase's default contract) and on the 32 x 32 patches: 1e-3 relative L2.  fake_N against compute_normal (oracle/nets.py) of
    this model's own fake_T in float64: 1e-5 absolute on unit vectors (a float32 division and square root: a few 6e-8 roundings)."""
    model = make_model(gold, case, save_dir=str(tmp_path))
    seed_weights(gold, case, model)
    model.save_networks("latest")
    keys = json.loads(str(gold[case + "/keys"]))
    assert sorted(os.listdir(str(tmp_path))) == sorted("latest_net_%s.pth" % nm for nm in NETS)
    for nm in NETS:
        saved = torch.load(os.path.join(str(tmp_path), "latest_net_%s.pth" % nm))
        assert [[k, list(v.shape)] for k, v in saved.items()] == keys[nm], nm
    tm = make_model(gold, case, train=False, save_dir=str(tmp_path))
    assert tm.model_names == ["G"] and not hasattr(tm, "netD") and tm.opt.return_patch is False
    assert all(torch.equal(v, dict(tm.netG.state_dict())[k]) for k, v in model.netG.state_dict().items())
    f32 = json.loads(str(gold["f32/%s/eval" % case]))
    seed, size = int(gold[case + "/seed"]), int(gold["size"])
    fh, fw, nt = (int(v) for v in gold["full"])
    for contract, batch in (("full", full_batch(fh, fw, nt, size, seed)), ("patch", p2p_batch(int(gold["n"]), size, seed))):
        tm.opt.return_patch = contract == "patch"
        tm.set_input(batch, phase="test")
        tm.test()
        if contract == "full":
            assert list(tm.real_T.shape) == [int(v) for v in gold[case + "/eval_full/real_T_shape"]] == [nt, 2, size, size]
            assert tuple(tm.fake_T.shape) == (1, 2, fh, fw) and tm.T_coords is not None and tm.full_T_coords is not None
        else:
            assert tm.T_coords is None
        for k in ("fake_I", "fake_T", "fake_N"):
            d = rel_l2(getattr(tm, k), torch.from_numpy(gold["%s/eval_%s/%s" % (case, contract, k)]))
            print(case, "eval", contract, k, "relative L2 %.2e (reference float32: %.2e)" % (d, f32["%s/%s" % (contract, k)]))
            assert d < 1e-3, (contract, k, d)
        want_N = nets.compute_normal(tm.fake_T.double().cpu(), tm.opt.scale_nz)
        e = (tm.fake_N.double().cpu() - want_N).abs().max().item()
        print(case, "eval", contract, "fake_N against compute_normal(fake_T, %g): max abs %.2e" % (tm.opt.scale_nz, e))
        assert tm.opt.scale_nz == 0.25 and e <= 1e-5
        assert set(tm.get_current_visuals()) == {"real_S", "M", "real_I", "fake_I", "fake_gx", "fake_gy", "fake_N"}


# ---- 6. learning rates -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["default", "B"])
def test_update_learning_rate_gives_the_reference_rates(gold, case):
    """G and D start at lr, D2 at lr_G2, with the reference's betas; one update_learning_rate (BaseModel's schedulers) leaves the three
    rates the reference's own call left"""
    model = make_model(gold, case)
    o = model.opt
    opts = (model.optimizer_G, model.optimizer_D, model.optimizer_D2)
    assert [p.param_groups[0]["lr"] for p in opts] == [o.lr, o.lr, o.lr_G2] == [2e-4, 2e-4, 5e-4]
    assert [tuple(p.param_groups[0]["betas"]) for p in opts] == [(o.beta1, 0.999), (o.beta1, 0.999), (o.beta1, o.beta2)]
    model.update_learning_rate()
    got = [p.param_groups[0]["lr"] for p in opts]
    ref = [float(v) for v in gold[case + "/lrs_after_update"]]
    print(case, got, ref)
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got, ref)), (got, ref)
