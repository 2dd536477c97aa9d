"""Every kernel of csrc/vts_ops.hip that the training step launches -- loss, Adam, the AvgPool pyramid and its adjoint, patch gather / jobs /
scatter, g_post, DiffAugment, g_out_grad(_pool), the u8 input staging, the "more fake T" sampler, step_begin, copy_words -- against the
float64 and exact judges of oracle/launch_ref.py, elementwise, on the hand-built table tests/step_glue_cases.py (the smallest shapes at
which each kernel can still go wrong; nothing is recorded).

Every operand, index array and output is a view (Op of tests/judge_harness.py) inside a flat device buffer between guard bands: NaN for floats, a sentinel
for integers and bytes.  Strided operands live in a larger NaN-filled tensor (a channel slice of a stack, a batch stride beyond the
sample).  Outputs start NaN-filled, or seeded where the call accumulates or read-modify-writes.  Each call asserts
  - the kernel instance the table expects (lib.vts_last_kernel());
  - |got - ref| <= C unit at every element of an arithmetic output (one constant C per family), bitwise equality for data movement and
    integer results;
  - every element the call does not own -- guard bands, inputs, the channels and gaps of a strided output -- bitwise unchanged;
  - a second identical call from the same initial state bitwise identical.
The module prints the worst err / unit per kernel instance (pytest -s); profiles/r12_step_glue_parity.txt is that table from the MI355X."""
import math

import pytest
import torch

import step_glue_cases as T
from judge_harness import Op, bits as _bits, judge as _judge
from oracle import detrand
from oracle import launch_ref as R

pytestmark = pytest.mark.gpu

# One constant per arithmetic family: |got - ref| <= C * unit at every element, unit = u r absref (u sqrt(K) absref for sums) as the judges
# state it.  C is twice the worst value measured on the MI355X (profiles/r12_step_glue_parity.txt), rounded up to two digits.  These are
# one-pass fp32 formulas with the unit counted per rounding: a worst value above 4 would be a finding to explain, not a reason for a
# larger bound.
# worst measured (MI355X, this module's inputs): pool 0.9812 (avgpool_bwd_kernel, 33 x 130), loss 0.2284 (lsgan, one element),
# loss_grad 0.7160 (lsgan, 3 x 35 x 35), l1 0.9962 (vec=0, n = 262147, accumulate; vec=1 0.9923), adam 0.9912 (both forms, n = 262147,
# step 1000), scatter 0.9373 (size 32, 70 patches per image), g_post 0.9801 (mask_mul, one rounding; g_post_kernel 0.3496), diffaug 0.4986
# ('n' without mask), g_out_grad 0.3896 (66 x 65 with the coarse level), spe 0.9383 (the 1100-wide row)
C_BOUND = {"pool": 2.0, "loss": 0.46, "loss_grad": 1.5, "l1": 2.0, "adam": 2.0, "scatter": 1.9, "g_post": 2.0, "diffaug": 1.0,
           "g_out_grad": 0.78, "spe": 1.9}
WORST = {}           # kernel instance -> [worst ratio, case, family, outputs judged]


@pytest.fixture(scope="module")
def gpu():
    from vts import lib as L
    from vts import ops
    lib = L.load()
    yield lib, ops, L
    if WORST:
        lines = ["# per kernel instance: worst err / unit over its rows vs float64 (oracle/launch_ref.py), bounds %s"
                 % ", ".join("%s %.3g" % kv for kv in C_BOUND.items()),
                 "# outputs = judged outputs of tests/step_glue_cases.py that the instance wrote; family 'exact': bitwise only",
                 "%-9s %-10s %7s  %-58s %s" % ("worst", "family", "outputs", "instance", "at case")]
        for inst, (w, case, fam, calls) in sorted(WORST.items(), key=lambda kv: (-kv[1][0], kv[0])):
            lines.append("%-9.4f %-10s %7d  %-58s %s" % (w, fam, calls, inst, case))
        print("\n[%s]\n%s" % (__name__, "\n".join(lines)))


def judge(gpu, tag, expected, call, opnds, outs):
    _judge(gpu[0], tag, expected, call, opnds, outs, C_BOUND, WORST)


def ids(rows):
    return [r[0] for r in rows]


def u01(shape, seed, name):
    return (detrand.uniform(shape, seed, name) + 1.0) * 0.5


def mask01(shape, seed):
    return (detrand.uniform(shape, seed, "M") > -0.3).float()


# ---------------------------------------------------------------------------------------------------------------- AvgPool pyramid
@pytest.mark.parametrize("row", T.AVGPOOL, ids=ids(T.AVGPOOL))
def test_avgpool_instances(gpu, row):
    lib, ops, L = gpu
    rid, h, w, layout, expected = row
    x = detrand.uniform((2, 3, h, w), 3000, rid)
    hw = h * w
    lay = {"pad2": dict(ns=3 * hw + 2), "pad3": dict(ns=3 * hw + 3), "odd": dict(ns=3 * hw + 1), "slice7": dict(ns=7 * hw, lead=hw, offset=1)}[layout]
    xo, yo = Op(x.shape, x, **lay), Op((2, 3, (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    ref, unit = R.avgpool3s2(x)["y"]
    judge(gpu, rid, expected, lambda: ops.avgpool(xo.t, yo.t), [xo, yo], [(yo, None, ref, unit, "pool")])


@pytest.mark.parametrize("hw", T.POOL_BWD, ids=["%dx%d" % s for s in T.POOL_BWD])
@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc"])
def test_avgpool_adjoint_into_a_channel_slice(gpu, hw, acc):
    lib, ops, L = gpu
    h, w = hw
    dy = detrand.uniform((2, 3, (h - 1) // 2 + 1, (w - 1) // 2 + 1), 3100, "dy")
    dx0 = detrand.uniform((2, 3, h, w), 3100, "dx0")
    dyo, dxo = Op(dy.shape, dy), Op((2, 3, h, w), dx0 if acc else None, ns=7 * h * w, lead=2 * h * w)
    ref, unit = R.avgpool3s2_bwd(dy, h, w, dx0 if acc else None)["dx"]
    judge(gpu, "pool-bwd-%dx%d-%s" % (h, w, "acc" if acc else "plain"), "avgpool_bwd_kernel",
          lambda: ops.avgpool_bwd(dyo.t, dxo.t, accumulate=acc), [dyo, dxo], [(dxo, None, ref, unit, "pool")])


# the pooled form needs a map of at least 2 x 2 (include/vts.h): 1 x 1 runs the plain form only
G_OUT_GRAD = [(hw, v) for hw in T.POOL_BWD for v in ("I+coarse+T", "I+coarse", "I", "T") if hw != (1, 1) or "coarse" not in v]


@pytest.mark.parametrize("hw,variant", G_OUT_GRAD, ids=["%dx%d-%s" % (hw + (v,)) for hw, v in G_OUT_GRAD])
def test_g_out_grad_and_its_pooled_form(gpu, hw, variant):
    """d_fake_T NULL, d_fake_I only, d_fake_I NULL; with a coarse level also bitwise equal to avgpool_bwd(accumulate) + g_out_grad"""
    lib, ops, L = gpu
    h, w = hw
    oh, ow = (h + 1) // 2, (w + 1) // 2
    dI, dT, dc = detrand.uniform((2, 3, h, w), 3200, "dI"), detrand.uniform((2, 2, h, w), 3200, "dT"), detrand.uniform((2, 3, oh, ow), 3200, "dc")
    g, M = detrand.uniform((2, 5, h, w), 3200, "g") * 0.97, mask01((2, 1, h, w), 3200)
    dIo, dTo, dco, go, Mo, do = Op(dI.shape, dI), Op(dT.shape, dT), Op(dc.shape, dc), Op(g.shape, g), Op(M.shape, M), Op((2, 5, h, w))
    useI, useT, usec = variant.startswith("I"), variant.endswith("T"), "coarse" in variant
    call = lambda: ops.g_out_grad(dIo.t if useI else None, dTo.t if useT else None, Mo.t, go.t, do.t, coarse=dco.t if usec else None)
    ref, unit = R.g_out_grad(dI if useI else None, dT if useT else None, M, g, coarse=dc if usec else None)["d_raw"]
    judge(gpu, "g-out-grad-%dx%d-%s" % (h, w, variant), "g_out_grad_kernel", call, [dIo, dTo, dco, go, Mo, do], [(do, None, ref, unit, "g_out_grad")])
    if usec:
        fused = do.t.clone()
        merged, two = dIo.t.clone(), torch.full_like(do.t, float("nan"))
        ops.avgpool_bwd(dco.t, merged, accumulate=True)
        ops.g_out_grad(merged, dTo.t if useT else None, Mo.t, go.t, two)
        torch.cuda.synchronize()
        assert torch.equal(_bits(fused.cpu()), _bits(two.cpu())), "the fused pool adjoint is not bitwise avgpool_bwd(accumulate) + g_out_grad"


# ---------------------------------------------------------------------------------------------------------------- losses
@pytest.mark.parametrize("row", T.gan_rows(), ids=ids(T.gan_rows()))
def test_ganloss_modes_totals_and_slot_states(gpu, row):
    lib, ops, L = gpu
    rid, mode, real, n, m, label, variant, seed = row
    p = T.gan_pred(row)
    po, slot, dp = Op(p.shape, p), Op((1,), torch.tensor([seed]), dtype=torch.int64), Op(p.shape)
    want_loss, want_grad = variant != "noloss", variant != "nograd"
    call = lambda: ops.ganloss(po.t, T.GAN_MODE_NAMES[mode], real, T.GAN_COEFF, slot.t if want_loss else None, dp.t if want_grad else None,
                               label=label, grad_coeff=T.GAN_GCOEFF)
    ref = R.ganloss(p, mode, real, label, T.GAN_COEFF, T.GAN_GCOEFF, workgroups=T.gan_workgroups(n * m))
    outs = []
    if want_loss:
        outs.append((slot, None, ref["loss"][0], ref["loss"][1], "loss"))
    if want_grad:
        outs.append((dp, None, ref["dpred"][0], ref["dpred"][1], "loss_grad"))
    if mode == 4 and n * m >= 255:
        assert float(ref["dpred"][0][17]) == 0 and float(ref["dpred"][1][17]) == 0           # the exact tie: gradient exactly 0
    judge(gpu, "%s-%s-seed%+d" % (rid, variant, (seed > 0) - (seed < 0)), "ganloss_kernel", call, [po, slot, dp], outs)


@pytest.mark.parametrize("row", T.L1, ids=ids(T.L1))
@pytest.mark.parametrize("variant", ["plain", "acc", "nograd"])
def test_l1_both_instances(gpu, row, variant):
    lib, ops, L = gpu
    rid, n, boff, vec = row
    a, b, g0 = T.l1_inputs(row)
    coeff = 100.0 / n
    seed = T.GAN_SEEDS[(n + len(variant)) % 3]
    ao, bo, slot = Op((n,), a), Op((n,), b, offset=boff), Op((1,), torch.tensor([seed]), dtype=torch.int64)
    go = Op((n,), g0 if variant == "acc" else None)
    call = lambda: ops.l1(ao.t, bo.t, coeff, slot.t, None if variant == "nograd" else go.t, accumulate=variant == "acc")
    ref = R.l1(a, b, coeff, grad0=g0 if variant == "acc" else None, workgroups=T.l1_workgroups(n, vec))
    outs = [(slot, None, ref["loss"][0], ref["loss"][1], "l1")]
    if variant != "nograd":
        outs.append((go, None, ref["grad"][0], ref["grad"][1], "l1"))
    if n >= 1024 and variant == "plain":
        assert (ref["grad"][0][T.L1_TIES[0]:T.L1_TIES[1]] == 0).all()
    judge(gpu, "%s-%s" % (rid, variant), "l1_kernel vec=%d" % vec, call, [ao, bo, slot, go], outs)


# ---------------------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("row", T.ADAM, ids=ids(T.ADAM))
@pytest.mark.parametrize("form", ["host", "dev"])
def test_adam_both_forms_against_one_judge(gpu, row, form):
    lib, ops, L = gpu
    rid, n, step, (b1, b2), gs = row
    p, g, m, v = T.adam_inputs(row)
    po, go, mo, vo = Op((n,), p), Op((n,), g), Op((n,), m), Op((n,), v)
    lr, st = Op((1,), torch.tensor([T.ADAM_LR])), Op((1,), torch.tensor([step]), dtype=torch.int32)
    if form == "host":
        call = lambda: ops.adam_flat(po.t, go.t, mo.t, vo.t, T.ADAM_LR, b1, b2, T.ADAM_EPS, step, grad_scale=gs)
    else:
        call = lambda: ops.adam_flat_dev(po.t, go.t, mo.t, vo.t, lr.t, b1, b2, T.ADAM_EPS, st.t, grad_scale=gs)
    ref = R.adam_flat(p, g, m, v, T.ADAM_LR, b1, b2, T.ADAM_EPS, step, gs)
    if n > 1:
        zero = torch.arange(n) % 7 == 0
        assert (ref["p"][1][zero] == 0).all() and torch.equal(ref["p"][0][zero], p.double()[zero])       # no update, exactly
    judge(gpu, "%s-%s" % (rid, form), "adam_kernel" if form == "host" else "adam_dev_kernel", call, [po, go, mo, vo, lr, st],
          [(po, None) + ref["p"] + ("adam",), (mo, None) + ref["m"] + ("adam",), (vo, None) + ref["v"] + ("adam",)])


# ---------------------------------------------------------------------------------------------------------------- patches
def _i32(op_list, *tensors):
    made = [Op(t.shape, t, dtype=torch.int32) for t in tensors]
    op_list += made
    return made


@pytest.mark.parametrize("row", T.GATHER, ids=ids(T.GATHER))
def test_patch_gather_from_a_channel_slice(gpu, row):
    lib, ops, L = gpu
    rid, size, h, w = row
    P = 10
    src = detrand.uniform((2, 2, h, w), 3300, "src")
    offx, offy = T.patch_offsets(h, w, size, P, 3300)
    img = (torch.arange(P) % 2).int()
    so, out = Op((2, 2, h, w), src, ns=4 * h * w, lead=h * w), Op((P, 5, size, size))
    opnds = [so, out]
    io, xo, yo = _i32(opnds, img, offx, offy)
    ref = R.patch_gather(src, img, offx, offy, size)
    judge(gpu, rid, "patch_gather_kernel", lambda: ops.patch_gather(so.t, io.t, xo.t, yo.t, size, out.t, c0=2), opnds,
          [(out, (slice(None), slice(2, 4)), ref, None, "exact")])


@pytest.mark.parametrize("row", T.PATCH_JOBS, ids=ids(T.PATCH_JOBS))
def test_patch_jobs_gather_copy_fill(gpu, row):
    lib, ops, L = gpu
    rid, njobs, size = row
    h, w = 33, 31
    src = detrand.uniform((2, 2, h, w), 3400, "src")
    so = Op((2, 2, h, w), src, ns=4 * h * w, lead=2 * h * w)
    opnds, jobs, want, outs = [so], [], [], []
    for j in range(njobs):
        P, c0, kind = 1 + (j * 3) % 7, j % 3, j % 3
        dst = Op((P, 5, size, size))
        opnds.append(dst)
        if kind == 0:
            offx, offy = T.patch_offsets(h, w, size, P, 3400 + j)
            img = ((torch.arange(P) + j) % 2).int()
            io, xo, yo = _i32(opnds, img, offx, offy)
            jobs.append(dict(dst=dst.t, c0=c0, src=so.t, img=io.t, offx=xo.t, offy=yo.t))
            want.append(dict(dst_c0=c0, C=2, P=P, src=src, img=img, offx=offx, offy=offy))
        elif kind == 1:
            patches = detrand.uniform((P, 2, size, size), 3400 + j, "patches")
            po = Op(patches.shape, patches)
            opnds.append(po)
            jobs.append(dict(dst=dst.t, c0=c0, src=po.t))
            want.append(dict(dst_c0=c0, C=2, P=P, src=patches))
        else:
            jobs.append(dict(dst=dst.t, c0=c0, channels=1, fill=0.25 * j - 1.0))
            want.append(dict(dst_c0=c0, C=1, P=P, fill=0.25 * j - 1.0))
        blk = R.patch_jobs(want[-1:], size)[0][1]
        outs.append((dst, (slice(None), slice(c0, c0 + blk.shape[1])), blk, None, "exact"))
    judge(gpu, rid, "patch_jobs_kernel", lambda: ops.patch_jobs(jobs, size=size), opnds, outs)


@pytest.mark.parametrize("row", T.SCATTER, ids=ids(T.SCATTER))
@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc"])
def test_patch_scatter_into_a_channel_slice(gpu, row, acc):
    """plain: tiles no patch touches become exactly 0; accumulate: they keep their seed (unit 0 there: exact)"""
    lib, ops, L = gpu
    rid, size, h, w, ppi = row
    P = 2 * ppi
    dp = detrand.uniform((P, 4, size, size), 3500, "dp")
    seed = detrand.uniform((2, 2, h, w), 3500, "seed")
    offx, offy = T.patch_offsets(h, w, size, P, 3500 + ppi)
    dpo, dso = Op(dp.shape, dp), Op((2, 2, h, w), seed if acc else None, ns=4 * h * w, lead=h * w)
    opnds = [dpo, dso]
    xo, yo = _i32(opnds, offx, offy)
    ref, unit = R.patch_scatter_bwd(dp[:, 1:3], offx, offy, ppi, 2, h, w, dsrc0=seed if acc else None)["dsrc"]
    if ppi == 1 and size == 5:
        assert float((unit == 0).double().mean()) > 0.5                # most of the image is touched by no patch
    judge(gpu, "%s-%s" % (rid, "acc" if acc else "plain"), "patch_scatter_kernel",
          lambda: ops.patch_scatter_bwd(dpo.t, 1, 2, xo.t, yo.t, ppi, size, dso.t, accumulate=acc), opnds, [(dso, None, ref, unit, "scatter")])


# ---------------------------------------------------------------------------------------------------------------- generator post-processing
@pytest.mark.parametrize("row", T.G_POST, ids=ids(T.G_POST))
def test_g_post_outputs_strides_and_null_pointers(gpu, row):
    lib, ops, L = gpu
    rid, h, w, variant = row
    hw = h * w
    g, M, S = detrand.uniform((2, 5, h, w), 3600, "g") * 0.97, mask01((2, 1, h, w), 3600), detrand.uniform((2, 1, h, w), 3600, "S")
    rb, rs = u01((2,), 3600, "rb"), u01((2,), 3600, "rs")
    nz = 0.0 if variant == "nz0" else 0.5
    go, Mo, So, rbo, rso = Op(g.shape, g), Op(M.shape, M), Op(S.shape, S), Op((2,), rb), Op((2,), rs)
    fI, fN = Op((2, 3, h, w)), Op((2, 3, h, w))
    opnds = [go, Mo, So, rbo, rso, fI, fN]
    skip = variant[3:] if variant.startswith("no-") else None
    useS = variant != "stackM" and variant != "dense"
    ref = R.g_post(g, M, nz, rb, rs, S if useS else None)
    outs = []

    def want(name, op, idx):
        if name != skip:
            v, u = ref[name]
            outs.append((op, idx, v.reshape((2, -1, h, w)), u.reshape((2, -1, h, w)), "g_post"))
            return True
        return False
    a = lambda name, view: view if name != skip else None
    want("fake_I", fI, None), want("fake_N", fN, None)
    if variant == "dense":
        fT, aug = Op((2, 2, h, w)), Op((2, 3, h, w))
        opnds += [fT, aug]
        want("fake_T", fT, None), want("aug_fake_I", aug, None)
        call = lambda: L.check(lib.vts_g_post(L.ptr(go.t), L.ptr(Mo.t), 2, h, w, nz, L.ptr(rbo.t), L.ptr(rso.t), L.ptr(fI.t), L.ptr(fT.t), 0,
                                              L.ptr(fN.t), L.ptr(aug.t), 0, L.stream()), "vts_g_post")
    else:
        stack = Op((2, 7, h, w))
        opnds.append(stack)
        views = {"fake_T": slice(0, 2), "stack_S": slice(2, 3), "aug_fake_I": slice(3, 6), "stack_M": slice(6, 7)}
        for name, sl in views.items():
            if name == "stack_S" and not useS:
                continue
            want(name, stack, (slice(None), sl))
        v = lambda name: a(name, stack.t[:, views[name]])
        sS = v("stack_S") if useS else None
        call = lambda: ops.g_post(go.t, Mo.t, nz, rbo.t, rso.t, fake_I=a("fake_I", fI.t), fake_T=v("fake_T"), fake_N=a("fake_N", fN.t),
                                  aug_fake_I=v("aug_fake_I"), S=So.t if sS is not None else None, stack_S=sS, stack_M=v("stack_M"))
    if variant == "nz0":
        off = (M.reshape(2, 1, hw) == 0).expand(2, 3, hw)
        assert off.any() and (ref["fake_N"][0][off] == 0).all() and (ref["fake_N"][1][off] == 0).all()     # 0 / 1e-12: exactly 0
    judge(gpu, rid, "g_post_kernel", call, opnds, outs)


# ---------------------------------------------------------------------------------------------------------------- DiffAugment
@pytest.mark.parametrize("row", T.DIFFAUG_BS, ids=ids(T.DIFFAUG_BS))
def test_diffaug_bs_mask(gpu, row):
    lib, ops, L = gpu
    rid, h, w, masked = row
    x, M = detrand.uniform((2, 3, h, w), 3700, "x"), mask01((2, 1, h, w), 3700)
    rb, rs = u01((2,), 3700, "rb"), u01((2,), 3700, "rs")
    xo, Mo, rbo, rso, out = Op(x.shape, x), Op(M.shape, M), Op((2,), rb), Op((2,), rs), Op(x.shape)
    ref, unit = R.diffaug_bs_mask(x, M if masked else None, rb, rs)["aug"]
    judge(gpu, rid, "diffaug_kernel", lambda: ops.diffaug_bs_mask(xo.t, Mo.t if masked else None, rbo.t, rso.t, out.t),
          [xo, Mo, rbo, rso, out], [(out, None, ref.reshape(x.shape), unit.reshape(x.shape), "diffaug")])


@pytest.mark.parametrize("row", T.DIFFAUG_OPS, ids=ids(T.DIFFAUG_OPS))
def test_diffaug_op_letters_strided(gpu, row):
    """x and out with a batch stride beyond the sample ('c' takes a contiguous x: include/vts.h); 'c' on a sample whose mean is far from 0"""
    lib, ops, L = gpu
    rid, op, c, h, w, masked = row
    chw = c * h * w
    x = detrand.uniform((2, c, h, w), 3800, "x")
    x[1] += 3.0
    M, noise = mask01((2, 1, h, w), 3800), detrand.uniform((2, c, h, w), 3800, "z")
    pf = torch.tensor([0.07, 0.0]) if op == "n" else torch.tensor([0.3, 0.9])
    pi0, pi1 = T.diffaug_ints(op, h, w)
    xo = Op(x.shape, x) if op == "c" else Op(x.shape, x, ns=chw + 5, lead=2)
    out, Mo, pfo, zo = Op(x.shape, ns=chw + 3), Op(M.shape, M), Op((2,), pf), Op(x.shape, noise)
    ws = Op((int(lib.vts_diffaug_op_ws_floats(2)),))
    opnds = [xo, out, Mo, pfo, zo, ws]
    i0, i1 = _i32(opnds, pi0, pi1)
    call = lambda: L.check(lib.vts_diffaug_op(L.ptr(xo.t), xo.ns, L.ptr(out.t), out.ns, 2, c, h, w, ord(op), L.ptr(pfo.t), L.ptr(i0.t), L.ptr(i1.t),
                                              L.ptr(zo.t), L.ptr(Mo.t) if masked else None, L.ptr(ws.t), L.stream()), "vts_diffaug_op")
    ref, unit = R.diffaug_op(x, op, pf=pf, pi0=pi0, pi1=pi1, noise=noise, M=M if masked else None)["out"]
    outs = [(out, None, ref, unit, "diffaug")]
    if op == "c":
        outs.append((ws, None, None, None, "diffaug"))
    judge(gpu, rid, "diffaug_mean_part_kernel+diffaug_op_kernel" if op == "c" else "diffaug_op_kernel", call, opnds, outs)


# ---------------------------------------------------------------------------------------------------------------- mask_mul, spe, pool, copies
@pytest.mark.parametrize("hw", T.MASK_MUL_HW)
def test_mask_mul(gpu, hw):
    lib, ops, L = gpu
    x, M = detrand.uniform((2, 3, 1, hw), 3900, "x"), mask01((2, 1, 1, hw), 3900) * u01((2, 1, 1, hw), 3900, "m")
    xo, Mo, yo = Op(x.shape, x), Op(M.shape, M), Op(x.shape)
    ref, unit = R.mask_mul(x, M)["y"]
    judge(gpu, "mask-mul-%d" % hw, "mask_mul_kernel", lambda: ops.mask_mul(xo.t, Mo.t, yo.t), [xo, Mo, yo], [(yo, None, ref, unit, "g_post")])


@pytest.mark.parametrize("row", T.SPE, ids=ids(T.SPE))
def test_spe_grid_with_the_argument_in_its_unit(gpu, row):
    lib, ops, L = gpu
    rid, dim, h, w, c0 = row
    out = Op((2, c0 + 2 * dim + 1, h, w))
    ref, unit = R.spe_grid(2, h, w, dim)["out"]
    judge(gpu, rid, "spe_kernel", lambda: ops.spe_grid(out.t, dim, c0=c0), [out], [(out, (slice(None), slice(c0, c0 + 2 * dim)), ref, unit, "spe")])


@pytest.mark.parametrize("row", T.POOL_QUERY, ids=ids(T.POOL_QUERY))
def test_pool_query_in_batch_order(gpu, row):
    lib, ops, L = gpu
    rid, elems = row
    images, store = detrand.uniform((3, elems), 4000, "images"), detrand.uniform((4, elems), 4000, "store")
    ret, put = torch.tensor(T.POOL_SLOTS[0], dtype=torch.int32), torch.tensor(T.POOL_SLOTS[1], dtype=torch.int32)
    io, so, oo = Op(images.shape, images), Op(store.shape, store), Op(images.shape)
    opnds = [io, so, oo]
    ro, po = _i32(opnds, ret, put)
    want_out, want_store = R.pool_query(images, store, ret, put)
    assert torch.equal(want_out[1], images[0]) and torch.equal(want_out[2], images[1])          # drawn from the slot just filled
    judge(gpu, rid, "pool_query_kernel", lambda: ops.pool_query(io.t, so.t, ro.t, po.t, oo.t), opnds,
          [(oo, None, want_out, None, "exact"), (so, None, want_store, None, "exact")])


@pytest.mark.parametrize("n", T.COPY_WORDS)
def test_copy_words(gpu, n):
    lib, ops, L = gpu
    src = (detrand.uniform((n,), 4100, "w") * 2 ** 30).int()
    so, do = Op((n,), src, dtype=torch.int32), Op((n,), dtype=torch.int32)
    judge(gpu, "copy-words-%d" % n, "copy_words_kernel", lambda: L.check(lib.vts_copy_words(L.ptr(so.t), L.ptr(do.t), n, L.stream()), "vts_copy_words"),
          [so, do], [(do, None, src, None, "exact")])


@pytest.mark.parametrize("counts", T.STEP_BEGIN, ids=["%d-%d" % c for c in T.STEP_BEGIN])
def test_step_begin_leaves_the_next_slot_and_counter(gpu, counts):
    lib, ops, L = gpu
    ns, nc = counts
    slots0, cnt0 = torch.arange(ns + 1, dtype=torch.int64) * 1000003 - 77, torch.arange(nc + 1, dtype=torch.int32) * 7 - 3
    so, co = Op((ns + 1,), slots0, dtype=torch.int64), Op((nc + 1,), cnt0, dtype=torch.int32)
    outs = []
    if ns:
        outs.append((so, slice(0, ns), torch.zeros(ns, dtype=torch.int64), None, "exact"))
    if nc:
        outs.append((co, slice(0, nc), cnt0[:nc] + 1, None, "exact"))
    judge(gpu, "step-begin-%d-%d" % counts, "step_begin_kernel", lambda: ops.step_begin(so.t[:ns], co.t[:nc] if nc else None), [so, co], outs)


# ---------------------------------------------------------------------------------------------------------------- byte staging
@pytest.mark.parametrize("n", T.U8_EXPAND)
@pytest.mark.parametrize("normalize", [0, 1])
def test_u8_expand_is_the_ieee_fp32_transform(gpu, n, normalize):
    lib, ops, L = gpu
    src = ((torch.arange(n) * 37 + 11) % 256).to(torch.uint8)
    so, out = Op((n,), src, dtype=torch.uint8), Op((n,))
    judge(gpu, "u8-expand-%d-%d" % (n, normalize), "u8_expand_kernel", lambda: ops.u8_expand(so.t, normalize, out.t), [so, out],
          [(out, None, R.u8_expand(src, normalize), None, "exact")])


@pytest.mark.parametrize("row", T.INPUT_U8, ids=ids(T.INPUT_U8))
def test_input_images_u8_both_instances(gpu, row):
    lib, ops, L = gpu
    rid, hw, variant, expected = row
    byte = lambda shape, k: ((torch.arange(math.prod(shape)) * k + 5 * k) % 256).to(torch.uint8).view(shape)
    S, I, M = byte((2, 1, 1, hw), 37), byte((2, 3, 1, hw), 101), byte((2, 1, 1, hw), 29)
    M.view(-1)[::3] = 0
    M.view(-1)[1::5] = 255
    hasI, hasM, hasS2 = variant != "no-I", variant != "no-M", variant != "no-S2"
    So, Io, Mb = Op(S.shape, S, dtype=torch.uint8, offset=1 if variant == "off1" else 0), Op(I.shape, I, dtype=torch.uint8), Op(M.shape, M, dtype=torch.uint8)
    Mo, S1, S2, I1 = Op(S.shape), Op(S.shape), Op(S.shape), Op(I.shape)
    m, s, i3 = R.input_images_u8(S, I if hasI else None, M if hasM else None)
    outs = [(S1, None, s, None, "exact")]
    if hasM:
        outs.append((Mo, None, m, None, "exact"))
    if hasS2:
        outs.append((S2, None, s, None, "exact"))
    if hasI:
        outs.append((I1, None, i3, None, "exact"))
    call = lambda: ops.input_images_u8(So.t, Io.t if hasI else None, Mb.t if hasM else None, Mo.t if hasM else None, S1.t, S2.t if hasS2 else None,
                                       I1.t if hasI else None)
    judge(gpu, rid, expected, call, [So, Io, Mb, Mo, S1, S2, I1], outs)


# ---------------------------------------------------------------------------------------------------------------- the "more fake T" sampler
@pytest.mark.parametrize("row", T.MASKS, ids=ids(T.MASKS))
def test_mask_candidates_ranks_and_select_exactly(gpu, row):
    lib, ops, L = gpu
    rid, h, w, pattern, K = row
    M = T.mask_input(row)
    cand, prefix = R.mask_candidates(M)
    hc, wc = h - 14, w - 14
    Mo, co, po = Op(M.shape, M), Op((2, hc, wc), dtype=torch.uint8), Op((2, hc + 1), dtype=torch.int32)
    judge(gpu, rid + "-candidates", "mask_cand_kernel+mask_rowcount_kernel+mask_prefix_kernel", lambda: ops.mask_candidates(Mo.t, co.t, po.t),
          [Mo, co, po], [(co, None, cand, None, "exact"), (po, None, prefix, None, "exact")])
    counts = prefix[:, -1].tolist()
    ranks = R.mask_sample_ranks(counts, K, T.MASK_SEED)
    pi, ro = Op(prefix.shape, prefix, dtype=torch.int32), Op((2, K), dtype=torch.int64)
    judge(gpu, rid + "-ranks", "mask_sample_ranks_kernel", lambda: ops.mask_sample_ranks(pi.t, h, K, T.MASK_SEED, ro.t), [pi, ro],
          [(ro, None, ranks, None, "exact")])
    for c, r in zip(counts, ranks):
        assert (c >= K and len(set(r.tolist())) == K and 0 <= int(r.min()) and int(r.max()) < c) or (c < K and r.tolist() == [q % c if c else 0 for q in range(K)])
    if min(counts) == 0:
        return              # an empty image has no candidate to select
    sel = ranks.clone()
    sel[0, 0], sel[1, -1] = 0, counts[1] - 1             # the first and the last candidate
    sel[0, -1] = counts[0] - 1 if K > 1 else sel[0, -1]
    ci, ri = Op(cand.shape, cand, dtype=torch.uint8), Op(sel.shape, sel, dtype=torch.int64)
    ox, oy = Op((2 * K,), dtype=torch.int32), Op((2 * K,), dtype=torch.int32)
    wx, wy = R.mask_select(cand, sel)
    call = lambda: L.check(lib.vts_mask_select(L.ptr(ci.t), L.ptr(pi.t), 2, h, w, L.ptr(ri.t), K, L.ptr(ox.t), L.ptr(oy.t), L.stream()), "vts_mask_select")
    judge(gpu, rid + "-select", "mask_select_kernel", call, [ci, pi, ri, ox, oy], [(ox, None, wx, None, "exact"), (oy, None, wy, None, "exact")])
