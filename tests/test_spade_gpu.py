"""SPADE generator on the HIP path: the new kernels alone, SPADEResnetBlock, and the generator (both fixture cases), forward and backward.

Judge: float64 -- the fixture tests/golden/spade_32.npz (the reference's own modules) and, for shapes it does not hold, the plain-torch
restatement tests/spade_restated.py run in float64 on the CPU (tests/test_spade_cpu.py pins it to the fixture at 1e-10).
Bounds, true relative L2 per tensor: outputs / dx / dseg / buffers 2e-5, parameter gradients 1e-3; tensors whose true gradient is zero
(a bias in front of a parameter-free normalisation; the fixture names them) |g| <= 2e-4 x the smallest other float64 gradient norm of
that network; everything stated as exact or bit-identical: torch.equal.  Every test prints its figures before it asserts.

The second generator case (ngf 4, a 1 x 2 latent) normalises head_0 over two pixels per channel.  That is ill-conditioned wherever a channel's
two values nearly coincide, and float32 then loses digits whatever the implementation: with another draw of weights (seed 812) the reference's
own float32 run is 2.4e-5 (output) and 3.9e-4 (dseg) away from its float64 run.  The 2e-5 bound on this case therefore holds for
well-conditioned draws only; the draw in use (spade_restated.GEN_CASES, seed 820) is one, chosen by the reference's own float32 distance.

Worst figures measured on an MI355X (profiles/r08_spade.md), relative L2 against the float64 judge:
  nearest resize / x2 and their adjoints       exact (torch.equal) on all six cases
  spectral norm, four shapes                   W/sigma 2.4e-7, sigma 2.4e-7, u / v after three calls 1.2e-7 / 1.9e-7, backward 2.4e-7; eval leaves u, v bit-identical
  modulate, 36 cases                           output 6.5e-8, dx 7.5e-8, dgamma 6.5e-8, dbeta 6.0e-9, running mean / variance 6.6e-8 / 4.2e-8
  SPADEResnetBlock, six cases                  output 3.3e-7, dx 3.2e-7, dseg 4.9e-7, buffers 1.7e-7, parameter gradients 7.7e-7 (the reference's own
                                               float32 run: 9.0e-7), zero-gradient tensors 4.3e-7 of the smallest other norm
  generator ngf 8 (sync-batch, L 3)            output 7.1e-7 (float32 reference 6.9e-7), dseg 7.9e-7 (8.5e-7), eval output 5.0e-7, buffers after one / two
                                               forwards 3.0e-7 / 2.7e-7, parameter gradients 1.2e-6 (1.5e-6), zero-gradient tensors 1.1e-6
  generator ngf 4 (instance, 1 x 2 latent, L 5) output 1.0e-6 (1.1e-6), dseg 3.4e-6 (4.0e-6), eval output 6.4e-7, buffers 2.4e-7 / 2.6e-7, parameter
                                               gradients 8.7e-6 (9.6e-6), zero-gradient tensors 2.5e-5
  two runs bit-identical; state dict round trip; HIP-graph replay of forward + backward equals the eager run bit for bit (both cases)
"""
import io
import json
import os

import pytest
import torch
import torch.nn.functional as F

import spade_restated as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spade_32.npz")
OUT_BOUND, GRAD_BOUND, ZERO_BOUND = 2e-5, 1e-3, 2e-4
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    return R.load_fixture(GOLDEN)


def _ints(shape, seed):
    """small integer-valued floats: sums of a few of them are exact in any order"""
    return torch.round(R.detrand.uniform(shape, seed, "ints") * 8)


# ---- nearest resize ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ih,iw,oh,ow", [(32, 32, 4, 4), (32, 32, 16, 16), (32, 32, 32, 32), (30, 20, 4, 6), (4, 6, 30, 20)])
def test_nearest_resize_is_interpolate(ih, iw, oh, ow):
    from vts import ops

    x = _ints((2, 3, ih, iw), 1).to(DEV).requires_grad_(True)
    want = F.interpolate(x, size=(oh, ow), mode="nearest")
    got = ops.nearest_resize(x.detach(), (oh, ow))
    cot = _ints((2, 3, oh, ow), 2).to(DEV)
    want_d, = torch.autograd.grad((want * cot).sum(), x)
    got_d = ops.nearest_resize_bwd(cot, torch.full_like(x.detach(), float("nan")))
    got_acc = ops.nearest_resize_bwd(cot, got_d.clone(), accumulate=True)
    print("forward equal", torch.equal(got, want), "adjoint equal", torch.equal(got_d, want_d))
    assert torch.equal(got, want.detach()) and torch.equal(got_d, want_d) and torch.equal(got_acc, 2 * want_d)


def test_nearest_up2_and_its_adjoint():
    from vts import ops

    x = _ints((3, 5, 4, 6), 3).to(DEV).requires_grad_(True)
    want = F.interpolate(x, scale_factor=2)
    got = ops.nearest_up2(x.detach())
    cot = _ints((3, 5, 8, 12), 4).to(DEV)
    want_d, = torch.autograd.grad((want * cot).sum(), x)
    got_d = ops.nearest_up2_bwd(cot)
    got_acc = ops.nearest_up2_bwd(cot, got_d.clone(), accumulate=True)
    print("forward equal", torch.equal(got, want), "adjoint equal", torch.equal(got_d, want_d))
    assert torch.equal(got, want.detach()) and torch.equal(got_d, want_d) and torch.equal(got_acc, 2 * want_d)


# ---- spectral norm -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(128, 128, 3, 3), (64, 128, 1, 1), (20, 45, 3, 3), (8, 8, 3, 3)], ids=lambda s: "%dx%d" % (s[0], s[1] * s[2] * s[3]))
def test_spectral_norm_forward_state_and_backward(shape):
    from vts import ops

    co, k = shape[0], shape[1] * shape[2] * shape[3]
    sd32 = R.weights({"c.weight_orig": shape, "c.weight_u": (co,), "c.weight_v": (k,)}, 31)
    sd = R.cast(sd32, torch.float64, grad=False)
    w, u, v = (sd32[n].to(DEV) for n in ("c.weight_orig", "c.weight_u", "c.weight_v"))
    w_sn, sigma = torch.empty_like(w), torch.empty(1, device=DEV)
    figs = {}
    for call in range(3):                                    # the state carries over from call to call
        ops.spectral_norm(w, u, v, True, w_sn, sigma)
        ref = R.spectral_weight(sd, "c", True)
        ref_sigma = (sd["c.weight_orig"].norm() / ref.norm()).item()
        figs["w/sigma call %d" % call] = R.rel_l2(w_sn, ref)
        figs["sigma call %d" % call] = abs(sigma.item() - ref_sigma) / abs(ref_sigma)
    figs["u after 3"], figs["v after 3"] = R.rel_l2(u, sd["c.weight_u"]), R.rel_l2(v, sd["c.weight_v"])
    u0, v0 = u.clone(), v.clone()
    ops.spectral_norm(w, u, v, False, w_sn, sigma)           # eval: the stored vectors are used as they are
    figs["w/sigma eval"] = R.rel_l2(w_sn, R.spectral_weight(sd, "c", False))
    frozen = torch.equal(u, u0) and torch.equal(v, v0)
    G = R.cotangent(shape, 32)
    dw = torch.full_like(w, float("nan"))
    ops.spectral_norm_bwd(G.to(DEV), w_sn, u, v, sigma, dw)
    ref_dw = R.spectral_norm_grad(G.double(), sd["c.weight_orig"], sd["c.weight_u"], sd["c.weight_v"])
    figs["dw"] = R.rel_l2(dw, ref_dw)
    ops.spectral_norm_bwd(G.to(DEV), w_sn, u, v, sigma, dw, accumulate=True)
    figs["dw accumulated"] = R.rel_l2(dw, 2 * ref_dw)
    print(shape, "eval leaves u, v untouched:", frozen, {n: "%.2e" % e for n, e in figs.items()})
    assert frozen
    assert all(e <= (GRAD_BOUND if n.startswith("dw") else OUT_BOUND) for n, e in figs.items()), figs


# ---- modulate ------------------------------------------------------------------------------------------------------------------------------
def _modulate_judge(x, gamma, beta, mode, act, rm, rv, cot):
    x, gamma, beta = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    if mode == 2:
        xh = (x - rm.double().view(1, -1, 1, 1)) / torch.sqrt(rv.double().view(1, -1, 1, 1) + 1e-5)
    else:
        dims = (2, 3) if mode == 0 else (0, 2, 3)
        m = x.mean(dims, keepdim=True)
        var = ((x - m) ** 2).mean(dims, keepdim=True)
        xh = (x - m) / torch.sqrt(var + 1e-5)
    out = xh * (1 + gamma) + beta
    if act:
        out = F.leaky_relu(out, 0.2)
    (out * cot.double()).sum().backward()
    res = {"out": out.detach(), "dx": x.grad, "dgamma": gamma.grad, "dbeta": beta.grad}
    if mode == 1:
        cnt = x.numel() // x.shape[1]
        res["running_mean"] = 0.9 * rm.double() + 0.1 * m.detach().reshape(-1)
        res["running_var"] = 0.9 * rv.double() + 0.1 * var.detach().reshape(-1) * cnt / (cnt - 1)
    return res


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("act", [0, 1], ids=["noact", "lrelu"])
@pytest.mark.parametrize("mode,shape", [(1, (1, 64, 4, 4)), (1, (3, 12, 8, 4)), (1, (4, 128, 16, 16)), (0, (3, 12, 8, 4)), (0, (4, 128, 16, 16)),
                                        (2, (3, 12, 8, 4)), (1, (2, 6, 36, 30)), (1, (2, 5, 7, 9)), (0, (2, 5, 7, 9))],
                         ids=lambda v: {0: "instance", 1: "batch", 2: "eval"}[v] if isinstance(v, int) else "x".join(map(str, v)))
def test_modulate_forward_backward(mode, shape, act, pad):
    """beyond the shapes of the generator: 36 x 30 planes (more than 1024 pixels: the backward's one-workgroup-per-plane form) and 7 x 9 planes
    (H W % 4 != 0: the scalar forward also without padding)"""
    from vts import ops

    n, c, h, w = shape
    x = R.detrand.uniform(shape, 41, "x") * 2 + 0.3
    gamma, beta = R.detrand.uniform(shape, 41, "gamma"), R.detrand.uniform(shape, 41, "beta")
    rm, rv = 0.2 * R.detrand.uniform((c,), 41, "rm"), 1.0 + 0.5 * R.detrand.uniform((c,), 41, "rv")
    cot = R.cotangent(shape, 41)
    want = _modulate_judge(x, gamma, beta, mode, act, rm, rv, cot)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    if mode == 2:
        mean, rstd = ops.spade_eval_stats(rmd, rvd, n)
    else:
        a = ops.norm_stats(xd, mode, running_mean=rmd if mode else None, running_var=rvd if mode else None)
        mean, rstd = a.mean, a.rstd
    out = ops.spade_modulate(xd, mean, rstd, gd, bd, act=act, out_pad=pad)
    g = F.pad(cot, (pad,) * 4, value=7.0).to(DEV).contiguous()       # the border of a padded gradient must not be read
    dgamma, dbeta, dx = ops.spade_modulate_bwd(g, xd, mean, rstd, gd, bd, mode, act=act, g_pad=pad)
    got = {"out": out[:, :, pad:pad + h, pad:pad + w], "dx": dx, "dgamma": dgamma, "dbeta": dbeta}
    if mode == 1:
        got["running_mean"], got["running_var"] = rmd, rvd
    figs = {k: R.rel_l2(v, want[k]) for k, v in got.items()}
    print(shape, "mode", mode, "act", act, "pad", pad, {k: "%.2e" % v for k, v in figs.items()})
    if pad:
        assert out[:, :, 0].abs().max() == 0 and out[:, :, -1].abs().max() == 0 and out[..., 0].abs().max() == 0 and out[..., -1].abs().max() == 0
    assert all(v <= OUT_BOUND for v in figs.values()), figs


# ---- SPADEResnetBlock ------------------------------------------------------------------------------------------------------------------------
def _load(mod, sd32):
    mod.load_state_dict({k: v.clone() for k, v in sd32.items()})
    return mod


def _check_grads(named_grads, judge_grads, zero_names, f32=None):
    """{name: (ours, fixture's float32 distance)} of the non-zero gradients, and the zero-gradient figure; asserts both rules"""
    norms = {k: v.double().norm().item() for k, v in judge_grads.items()}
    smallest = min(v for k, v in norms.items() if k not in zero_names)
    figs = {k: R.rel_l2(named_grads[k], judge_grads[k]) for k in judge_grads if k not in zero_names}
    zfig = max(named_grads[k].double().norm().item() for k in zero_names) / smallest if zero_names else 0.0
    worst = max(figs, key=figs.get)
    print("  parameter gradients: worst %.2e (%s; the reference's own float32 run: %s), zero-gradient tensors %.2e of the smallest other norm"
          % (figs[worst], worst, "%.2e" % f32["grad/" + worst] if f32 and ("grad/" + worst) in f32 else "n/a", zfig))
    if f32:
        for k in sorted(figs, key=figs.get)[-3:]:
            print("    %-48s ours %.2e   float32 reference %.2e" % (k, figs[k], f32.get("grad/" + k, float("nan"))))
    assert set(named_grads) == set(judge_grads)
    assert all(v <= GRAD_BOUND for v in figs.values()), {k: v for k, v in figs.items() if v > GRAD_BOUND}
    assert zfig <= ZERO_BOUND, zfig


@pytest.mark.parametrize("norm", sorted(R.BLOCK_NORMS))
@pytest.mark.parametrize("shape", R.BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spade_resnet_block(gold, shape, norm):
    from models import networks
    from vts import engine
    from vts.optim import FlatParams

    fin, fout, n, h, w = shape
    name = R.block_case_name(shape, norm)
    seed = int(gold["seed/" + name])
    shapes = R.block_shapes(fin, fout, kind=norm)
    sd32 = R.weights({k[4:]: s for k, s in shapes.items()}, seed)
    jsd = R.cast({"blk." + k: v for k, v in sd32.items()}, torch.float64)
    want = R.run_block_case(lambda x, seg: R.spade_block(jsd, "blk", x, seg, R.BLOCK_NORMS[norm], True), jsd, shape, seed, torch.float64)
    pinned = max(R.check_stored(gold, "%s/%s" % (name, k), v) for k, v in want.items())
    blk = _load(networks.SPADEResnetBlock(fin, fout, R.Opt(normG=R.BLOCK_NORMS[norm], semantic_nc=1)), sd32).to(DEV).train()
    FlatParams(blk)
    x = R.detrand.uniform((n, fin, h, w), seed, "x").to(DEV)
    seg = R.seg_input(n, 1, 32, 32, seed).to(DEV)
    out, ctx = engine.spade_block_forward(blk, x, seg)
    dx, dseg = engine.spade_block_backward(blk, ctx, R.cotangent(out.shape, seed).to(DEV))
    f32 = R.f32_distance(gold, name)
    figs = {"out": R.rel_l2(out, want["out"]), "dx": R.rel_l2(dx, want["dx"]), "dseg": R.rel_l2(dseg, want["dseg"])}
    for k, v in blk.state_dict().items():
        if not R.is_param(k) and v.dtype != torch.long:
            figs["buffer " + k] = R.rel_l2(v, jsd["blk." + k])
    counters = [(k, int(v), int(jsd["blk." + k])) for k, v in blk.state_dict().items() if v.dtype == torch.long]
    print(name, "judge vs fixture %.1e;" % pinned, {k: "%.2e" % v for k, v in figs.items() if not k.startswith("buffer")},
          "worst buffer %.2e;" % max(v for k, v in figs.items() if k.startswith("buffer")),
          "float32 reference: out %.2e dx %.2e dseg %.2e" % (f32["out"], f32["dx"], f32["dseg"]))
    assert pinned <= 1e-10
    assert all(v <= OUT_BOUND for v in figs.values()), {k: v for k, v in figs.items() if v > OUT_BOUND}
    assert all(a == b for _, a, b in counters), counters
    grads = {k: p.grad for k, p in blk.named_parameters()}
    _check_grads(grads, {k[4:]: v.grad for k, v in jsd.items() if R.is_param(k)}, ["conv_0.bias"], f32)


# ---- generator -----------------------------------------------------------------------------------------------------------------------------
_JUDGE = {}


def _judge(gold, case):
    """the float64 judge of a generator case, computed once: training forward + backward, a second training forward, an eval forward"""
    if case in _JUDGE:
        return _JUDGE[case]
    c = R.GEN_CASES[case]
    sd = R.cast(R.weights(dict(R.fixture_keys(gold, case)), c["seed"]), torch.float64)
    h, w = R.gen_out_hw(c)
    seg = R.seg_input(c["N"], c["input_nc"], h, w, c["seed"]).double().requires_grad_(True)
    out = R.spade_generator(sd, seg, c, True)
    (out * R.cotangent(out.shape, c["seed"]).double()).sum().backward()
    j = {"out": out.detach(), "dseg": seg.grad, "grads": {k: v.grad for k, v in sd.items() if R.is_param(k)}}
    j["pinned"] = max(R.check_stored(gold, case + "/out", j["out"]), R.check_stored(gold, case + "/dseg", j["dseg"]))
    with torch.no_grad():
        R.spade_generator(sd, seg, c, True)
        j["out_eval"] = R.spade_generator(sd, seg, c, False)
    j["pinned"] = max(j["pinned"], R.check_stored(gold, case + "/out_eval", j["out_eval"]))
    _JUDGE[case] = j
    return j


def _generator(gold, case):
    from models import networks
    from vts.optim import FlatParams

    c = R.GEN_CASES[case]
    G = networks.define_G(c["input_nc"], c["output_nc"], c["ngf"], "spade", norm=c["normG"], opt=R.gen_opt(case), gpu_ids=[0])
    sd32 = R.weights(dict(R.fixture_keys(gold, case)), c["seed"])
    _load(G, sd32).train()
    flat = FlatParams(G)
    h, w = R.gen_out_hw(c)
    seg = R.seg_input(c["N"], c["input_nc"], h, w, c["seed"]).to(DEV)
    cot = R.cotangent((c["N"], c["output_nc"], h, w), c["seed"]).to(DEV)
    return G, flat, sd32, seg, cot


def _buffer_figs(gold, G, case, tag):
    figs, exact = {}, True
    for k, v in G.state_dict().items():
        if R.is_param(k):
            continue
        if v.dtype == torch.long:
            exact = exact and int(v) == int(gold["%s/%s/%s" % (case, tag, k)])
        else:
            figs[k] = R.check_stored(gold, "%s/%s/%s" % (case, tag, k), v)
    return figs, exact


@pytest.mark.parametrize("case", sorted(R.GEN_CASES))
def test_generator_against_the_fixture(gold, case):
    from vts import engine

    j = _judge(gold, case)
    G, flat, sd32, seg, cot = _generator(gold, case)
    f32 = R.f32_distance(gold, case)
    out, ctx = engine.spade_forward(G, seg)
    dseg = engine.spade_backward(G, ctx, cot)
    figs = {"out": R.rel_l2(out, torch.from_numpy(gold[case + "/out"])), "dseg": R.rel_l2(dseg, torch.from_numpy(gold[case + "/dseg"]))}
    b1, exact1 = _buffer_figs(gold, G, case, "buf1")
    grads = {k: p.grad.clone() for k, p in G.named_parameters()}
    engine.spade_forward(G, seg, keep=False)
    b2, exact2 = _buffer_figs(gold, G, case, "buf2")
    before = {k: v.clone() for k, v in G.state_dict().items()}
    G.eval()
    out_eval, _ = engine.spade_forward(G, seg, keep=False)
    figs["out_eval"] = R.rel_l2(out_eval, j["out_eval"])
    untouched = all(torch.equal(v, before[k]) for k, v in G.state_dict().items())
    figs["buffers after one forward"], figs["buffers after two"] = max(b1.values()), max(b2.values())
    print(case, "judge vs fixture %.1e;" % j["pinned"], {k: "%.2e" % v for k, v in figs.items()},
          "float32 reference: out %.2e dseg %.2e;" % (f32["out"], f32["dseg"]), "counters exact:", exact1 and exact2,
          "eval leaves the state untouched:", untouched)
    assert j["pinned"] <= 1e-10
    assert all(v <= OUT_BOUND for v in figs.values()), figs
    assert exact1 and exact2 and untouched
    zero = json.loads(str(gold["zero_grads/" + case]))
    _check_grads(grads, j["grads"], zero, f32)
    # the probes of the fixture itself, for the tensors it stores as probes or whole
    pf = {k: R.check_stored(gold, "%s/grad/%s" % (case, k), g) for k, g in grads.items() if k not in zero}
    print("  gradient probes against the fixture: worst %.2e" % max(pf.values()))
    assert max(pf.values()) <= GRAD_BOUND


def test_generator_state_dict_round_trip_and_repeatability(gold):
    from vts import engine

    case = "g8"
    G, flat, sd32, seg, cot = _generator(gold, case)

    def run():
        out, ctx = engine.spade_forward(G, seg)
        dseg = engine.spade_backward(G, ctx, cot)
        torch.cuda.synchronize()
        return [out.clone(), dseg.clone(), flat.grad.clone()] + [v.clone() for k, v in G.state_dict().items() if not R.is_param(k)]

    first = run()
    buf = io.BytesIO()
    torch.save(G.state_dict(), buf)                       # the state after one step, u / v and running statistics included
    buf.seek(0)
    saved = torch.load(buf)
    _load(G, sd32)
    second = run()
    same = all(torch.equal(a, b) for a, b in zip(first, second))
    G.load_state_dict(saved)
    back = all(torch.equal(v.cpu(), saved[k].cpu()) for k, v in G.state_dict().items()) and list(saved) == [k for k, _ in R.fixture_keys(gold, case)]
    print("two runs bit-identical:", same, "round trip:", back)
    assert same and back


@pytest.mark.parametrize("case", sorted(R.GEN_CASES))
def test_generator_graph_replay_equals_eager(gold, case):
    from vts import engine

    G, flat, sd32, seg, cot = _generator(gold, case)
    res = {}

    def step():
        out, ctx = engine.spade_forward(G, seg)
        res["out"], res["dseg"] = out, engine.spade_backward(G, ctx, cot)

    def results():
        torch.cuda.synchronize()
        return [res["out"].clone(), res["dseg"].clone(), flat.grad.clone()] + [v.clone() for k, v in G.state_dict().items() if not R.is_param(k)]

    step()
    eager = results()
    _load(G, sd32)                                        # the step advances u / v and the running statistics: start the replay from the same state
    graph = torch.cuda.CUDAGraph()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):
        with torch.cuda.graph(graph, stream=cs):
            step()
    torch.cuda.current_stream().wait_stream(cs)
    flat.grad.fill_(float("nan"))
    graph.replay()
    replay = results()
    same = [torch.equal(a, b) for a, b in zip(eager, replay)]
    print(case, "replay equals eager:", all(same), "(%d tensors)" % len(same))
    assert all(same)
