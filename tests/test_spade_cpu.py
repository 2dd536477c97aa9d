"""SPADE generator, the checks that need no GPU: the modules' state-dict surface against the reference's (tests/golden/spade_32.npz,
written by tools/make_spade_golden.py from the reference's own modules), the plain-torch restatement (tests/spade_restated.py) pinned
to that fixture at 1e-10, the configurations that must raise, and the spectral-norm gradient formula against autograd."""
import argparse
import json
import os

import pytest
import torch

import spade_restated as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spade_32.npz")


@pytest.fixture(scope="module")
def gold():
    return R.load_fixture(GOLDEN)


def _define(case, **over):
    from models import networks

    c = dict(R.GEN_CASES[case])
    opt = argparse.Namespace(normG=c["normG"], semantic_nc=c["input_nc"], num_upsampling_layers=c["num_upsampling_layers"],
                             output_width=c["output_width"], aspect_ratio=c["aspect_ratio"], use_vae=False)
    for k, v in over.items():
        setattr(opt, k, v)
    return networks.define_G(c["input_nc"], c["output_nc"], c["ngf"], "spade", norm=opt.normG, opt=opt)


@pytest.mark.parametrize("case", sorted(R.GEN_CASES))
def test_define_G_spade_has_the_reference_keys(gold, case):
    G = _define(case)
    got = [(k, tuple(v.shape)) for k, v in G.state_dict().items()]
    want = R.fixture_keys(gold, case)
    print(case, len(got), "keys")
    assert got == want
    named = dict(G.named_parameters())
    for k, _ in want:
        assert (k in named) == R.is_param(k), k           # u, v, running statistics and the counter are buffers
    u = G.head_0.conv_0.weight_u
    assert abs(u.norm().item() - 1.0) < 1e-5 and G.head_0.conv_0.weight_orig.abs().sum() > 0     # init_weights draws weight_orig (the project's choice: networks._SNConvParams)
    from vts.optim import FlatParams

    flat = FlatParams(G)
    assert flat.numel == sum(p.numel() for p in G.parameters())
    assert all(p.grad is not None and p.grad.data_ptr() >= flat.grad.data_ptr() for p in G.parameters())


@pytest.mark.parametrize("case", sorted(R.GEN_CASES))
def test_restatement_matches_the_reference_generator(gold, case):
    c = R.GEN_CASES[case]
    sd = R.cast(R.weights(dict(R.fixture_keys(gold, case)), c["seed"]), torch.float64)
    h, w = R.gen_out_hw(c)
    seg = R.seg_input(c["N"], c["input_nc"], h, w, c["seed"]).double().requires_grad_(True)
    out = R.spade_generator(sd, seg, c, True)
    (out * R.cotangent(out.shape, c["seed"]).double()).sum().backward()
    zero = json.loads(str(gold["zero_grads/" + case]))
    worst = {"out": R.check_stored(gold, case + "/out", out), "dseg": R.check_stored(gold, case + "/dseg", seg.grad)}
    worst["grad"] = max(R.check_stored(gold, "%s/grad/%s" % (case, k), v.grad) for k, v in sd.items() if R.is_param(k) and k not in zero)
    top = float(gold["min_nonzero_grad_norm/" + case])
    worst["zero grads / smallest other"] = max(sd[k].grad.norm().item() for k in zero) / top
    bufs = lambda: {k: v for k, v in sd.items() if not R.is_param(k)}   # noqa: E731
    worst["buf1"] = max(R.check_stored(gold, "%s/buf1/%s" % (case, k), v) for k, v in bufs().items())
    with torch.no_grad():
        R.spade_generator(sd, seg, c, True)
    worst["buf2"] = max(R.check_stored(gold, "%s/buf2/%s" % (case, k), v) for k, v in bufs().items())
    with torch.no_grad():
        worst["out_eval"] = R.check_stored(gold, case + "/out_eval", R.spade_generator(sd, seg, c, False))
    worst["buf after eval"] = max(R.check_stored(gold, "%s/buf2/%s" % (case, k), v) for k, v in bufs().items())
    print(case, {k: "%.2e" % v for k, v in worst.items()})
    assert all(v <= 1e-10 for v in worst.values()), worst


@pytest.mark.parametrize("norm", sorted(R.BLOCK_NORMS))
@pytest.mark.parametrize("shape", R.BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_matches_the_reference_block(gold, shape, norm):
    name = R.block_case_name(shape, norm)
    seed = int(gold["seed/" + name])
    shapes = R.block_shapes(shape[0], shape[1], kind=norm)
    sd = R.cast({"blk." + k: v for k, v in R.weights({k[4:]: s for k, s in shapes.items()}, seed).items()}, torch.float64)
    res = R.run_block_case(lambda x, seg: R.spade_block(sd, "blk", x, seg, R.BLOCK_NORMS[norm], True), sd, shape, seed, torch.float64)
    worst = {k: R.check_stored(gold, "%s/%s" % (name, k), v) for k, v in res.items()}
    for k, v in sd.items():
        if not R.is_param(k):
            worst["buf1/" + k[4:]] = R.check_stored(gold, "%s/buf1/%s" % (name, k[4:]), v)
        elif R.stored_norm(gold, "%s/grad/%s" % (name, k[4:])) > 1e-9:     # (conv_0.bias feeds a normalisation: its true gradient is 0)
            worst["grad/" + k[4:]] = R.check_stored(gold, "%s/grad/%s" % (name, k[4:]), v.grad)
    print(name, "worst %.2e over %d tensors" % (max(worst.values()), len(worst)))
    assert max(worst.values()) <= 1e-10, {k: v for k, v in worst.items() if v > 1e-10}


def test_unsupported_configurations_raise():
    with pytest.raises(ValueError, match="final_nc"):
        _define("g8", num_upsampling_layers=2)
    with pytest.raises(NotImplementedError, match="use_vae"):
        _define("g8", use_vae=True)
    with pytest.raises(NotImplementedError, match="5x5"):
        _define("g8", normG="spectralspadesyncbatch5x5")


@pytest.mark.parametrize("co,ci,k", [(8, 8, 3), (20, 45, 3), (64, 128, 1)])
def test_spectral_norm_gradient_formula_is_autograd(co, ci, k):
    """(G - <G, W/sigma> u v^T) / sigma against autograd through torch.nn.utils.spectral_norm, float64"""
    torch.manual_seed(0)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(ci, co, k, bias=False).double())
    conv.train()
    x = torch.randn(2, ci, 5, 5, dtype=torch.float64)
    w0, u0, v0 = conv.weight_orig.detach().clone(), conv.weight_u.clone(), conv.weight_v.clone()
    y = conv(x)                                            # one power iteration; conv.weight is W / sigma of this call
    cot = torch.randn_like(y)
    G, = torch.autograd.grad((y * cot).sum(), conv.weight, retain_graph=True)
    (y * cot).sum().backward()
    # the restatement's forward leaves the same u, v and weight ...
    sd = {"c.weight_orig": w0.clone().requires_grad_(True), "c.weight_u": u0.clone(), "c.weight_v": v0.clone()}
    w_sn = R.spectral_weight(sd, "c", True)
    d_fwd = max(R.rel_l2(w_sn, conv.weight), R.rel_l2(sd["c.weight_u"], conv.weight_u), R.rel_l2(sd["c.weight_v"], conv.weight_v))
    # ... and its gradient formula is what autograd computes
    d_bwd = R.rel_l2(R.spectral_norm_grad(G, w0, conv.weight_u, conv.weight_v), conv.weight_orig.grad)
    print("forward %.2e backward %.2e" % (d_fwd, d_bwd))
    assert d_fwd <= 1e-12 and d_bwd <= 1e-12
