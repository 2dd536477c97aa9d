"""The case table of tests/test_perceptual_glue_gpu.py against csrc/vts_perceptual.hip and vts_zero_border: every __global__ kernel and every
instance string of the source is claimed by a row, no row claims an instance the source does not name, both alternatives of every dispatch
(and every chunk loop, second sweep and stride) have a row; the planted ties and kink margins are what the table says; the bitwise rows have
dyadic inputs and fp32-representable references; the exact-sum rows sum exactly in fp32 in two orders; and the derived units are honest: a
plain fp32 evaluation of each formula, in two summation orders, stays within 1.0 unit of the float64 reference, while a reference moved by
3 units at one element, or a loss with one pixel dropped, is rejected."""
import os
import re

import torch

import perceptual_glue_cases as T
from oracle import launch_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visual-tactile-synthesis_amd", "csrc")
ENTRIES = ["vts_maxpool2_relu_pad", "vts_maxpool3s2_relu_pad", "vts_s2d4_pad", "vts_maxpool2_relu_bwd", "vts_relu_mask_pad", "vts_lpips_layer",
           "vts_l1_relu", "vts_lpips_input", "vts_lpips_input_bwd", "vts_vgg_stack_input", "vts_vgg_stack_input_bwd"]
BOUND = 1.01


def source(name="vts_perceptual.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def global_kernels():
    return sorted(set(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(", source())))


def instance_strings(text):
    out = []
    for call in re.findall(r"\bvts_set_kernel\(([^;]*)\);", text):
        found = re.findall(r'"([^"]*)"', call)
        assert found, call
        out += found
    return sorted(set(out))


def entry_body(name, text):
    m = re.search(r'extern "C" int %s\(.*?\n}\n' % name, text, re.S)
    assert m, name
    return m.group(0)


def zero_border_body():
    return entry_body("vts_zero_border", source("vts_conv3x3_wide.hip"))


# ---------------------------------------------------------------------------------------------------------------- table against the sources
def test_the_source_is_read_as_expected():
    k, s = global_kernels(), instance_strings(source())
    assert len(k) == 13 and "lpips_layer_regs_kernel" in k and "vgg_stack_input_bwd_kernel" in k and "maxpool2_relu_bwd_win_kernel" in k, k
    assert "lpips_layer_regs_kernel<64,8>" in s and "vgg_stack_input_bwd_kernel<1>" in s and "l1_relu_kernel" in s, s


def test_every_entry_names_its_instance():
    for name in ENTRIES:
        named = instance_strings(entry_body(name, source()))
        assert named, "%s does not call vts_set_kernel" % name
        assert set(named) <= T.claimed_instances(), (name, named)
    assert instance_strings(zero_border_body()) == ["zero_border_kernel"]


def test_every_kernel_and_instance_of_the_source_is_claimed_by_a_row():
    claimed = T.claimed_instances()
    unclaimed = [s for s in instance_strings(source()) if s not in claimed]
    assert not unclaimed, "instances without a row in tests/perceptual_glue_cases.py: %s" % unclaimed
    names = {T.kernels_of(c) for c in claimed}
    missing = [k for k in global_kernels() if k not in names]
    assert not missing, "__global__ kernels without a row in tests/perceptual_glue_cases.py: %s" % missing


def test_every_row_claims_an_instance_the_source_names():
    named = set(instance_strings(source())) | set(instance_strings(zero_border_body()))
    unknown = [c for c in T.claimed_instances() if c not in named]
    assert not unknown, unknown
    assert "zero_border_kernel" in source("vts_conv3x3_wide.hip")


def test_both_alternatives_of_every_dispatch_have_rows():
    assert {r[7] for r in T.MPB} == {T.WIN, T.ELEM}
    for r in T.MPB:
        assert (r[7] == T.WIN) == (r[2] % 2 == 0 and r[3] % 2 == 0), r[0]
    # the per-window kernel with one window row, one window column, and both at once, under every pad
    for pad in (0, 1, 2):
        for hw in ((2, 2), (2, 10), (10, 2)):
            assert any(r[2:4] == hw and r[4] == pad and r[6] for r in T.MPB), (hw, pad)
    assert {r[8] for r in T.LPL} == set(T.LPL_INSTANCE.values()) | {T.GENERIC}
    for r in T.LPL:
        assert r[8] == T.LPL_INSTANCE.get(r[2], T.GENERIC), r[0]
    for inst in {r[8] for r in T.LPL}:
        rows = [r for r in T.LPL if r[8] == inst and not r[9]]
        assert {r[5] for r in rows} == {0, 1, 2} and {r[6] for r in rows} == set(T.VARIANTS) and {r[1] for r in rows} == {1, 3}, inst
        assert {r[7] for r in rows} == set(T.GAN_SEEDS), inst
        assert any(int((T.lpl_inputs(r)[3] == 1).sum()) for r in rows), "%s: no pixel with r0 = 0" % inst
    # vgg_stack_input_bwd: the float4 instance when all three conditions hold, the scalar one when exactly one fails, each one once
    failing = []
    for r in T.VSB:
        cond = T.vsb_conditions(r)
        assert (r[5] == T.V4) == all(cond), r[0]
        if r[5] == T.V1:
            assert sum(not c for c in cond) == 1, r[0]
            failing.append(cond.index(False))
    assert sorted(failing) == [0, 1, 2]


def test_chunk_loops_second_sweeps_and_strides_have_rows():
    for rows in (T.MP2, T.MP3, T.MPB, T.RMP, T.ZB):
        assert any(r[1] > 65535 for r in rows)
    chunk = [r for r in T.MPB if r[1] > 65535]
    assert all(r[5] == 2 and r[6] for r in chunk)                            # zpad = 2 and the tap: the three per-chunk offsets differ
    assert any(r[1] > 65535 and r[5] > 0 for r in T.MP2) and any(r[1] > 65535 and r[5] > 0 for r in T.RMP)
    assert any((r[2] // 2 + 2 * r[4]) * (r[3] // 2 + 2 * r[4]) > T.SWEEP for r in T.MP2)
    assert any(r[3] * r[4] > T.SWEEP and r[8] == T.GENERIC and r[9] for r in T.LPL)
    assert any(r[1] // 4 + 1 > T.SWEEP and r[4] for r in T.L1R)
    assert any(r[3] > T.SWEEP and r[2] == 1 for r in T.LIN) and any(r[3] > T.SWEEP and r[2] == 3 for r in T.LIN)
    assert any(2 * r[4] * (r[3] + 2 * r[4] + r[2]) > 64 * 256 for r in T.ZB)
    assert any(r[4] == "slice" for r in T.LIN) and any(r[4] == "dense" for r in T.LIN)
    # the space-to-depth row that reads beyond the padded image
    assert any(4 * r[6] > r[3] + 2 * r[5] + 4 for r in T.S2D)
    # every loss row with more than 1024 addends is an exact-sum row
    assert all(r[4] == (r[1] > 1024) for r in T.L1R) and all(r[9] == (r[1] * r[3] * r[4] > 1024) for r in T.LPL)


def test_row_ids_are_unique():
    ids = T.row_ids()
    assert len(ids) == len(set(ids)) and len(ids) > 300


# ---------------------------------------------------------------------------------------------------------------- kinks and planted ties
def test_kink_margins_and_planted_zeros_of_the_lpips_head_rows():
    planted = 0
    for row in T.LPL:
        z0, z1, w, pl = T.lpl_inputs(row)
        assert float(w.min()) > 0
        for z in (z0, z1):
            a = z.abs()
            assert bool(((a >= 2 * T.KINK) | (z == 0)).all()), row[0]
            if row[5] == 0 and not row[9]:
                assert bool((z != 0).all()) and (z.numel() < 8 or bool((z < 0).any())), row[0]         # raw: negatives, no exact zero
            if row[5] > 0:
                assert bool((z >= 0).all()), row[0]
        f0, f1 = z0.clamp_min(0), z1.clamp_min(0)
        assert bool((f0.sum(1)[(pl == 1) | (pl == 3)] == 0).all()) and bool((f1.sum(1)[(pl == 2) | (pl == 3)] == 0).all()), row[0]
        planted += int((pl > 0).sum())
    assert planted >= 3 * 30


def test_kink_margins_and_planted_ties_of_the_relu_l1_rows():
    for row in T.L1R:
        za, zb, tie = T.l1r_inputs(row)
        d = (za.double().clamp_min(0) - zb.double().clamp_min(0)).abs()
        assert bool((d[tie] == 0).all()) and bool((d[~tie] >= T.KINK).all()), row[0]
        if row[1] >= 255:
            assert bool(tie[T.L1R_TIES[0]:T.L1R_TIES[1]].all()) and bool((za[T.L1R_TIES[0]:T.L1R_TIES[1]] > 0).any())
            s = slice(*T.L1R_NEG)
            assert bool((za[s] < 0).all()) and bool((zb[s] < 0).all())
            assert int((~tie).sum()) > row[1] // 4


def test_planted_windows_of_the_pooling_rows():
    for rows, k in ((T.MP2, 2), (T.MP3, 3)):
        for row in rows:
            z = T.pool_input(row, k)
            assert bool((z[0, :k, :k] == 0.375).all()), row[0]
            neg = z[row[1] - 1, :k, :k] if row[1] > 1 else z[0, :k, 4:4 + k]
            assert bool((neg < 0).all()), row[0]
    for row in T.MPB:
        g, z, t, pat = T.mpb_inputs(row)
        nc, h, w = z.shape
        oh, ow = h // 2, w // 2
        e = z[:, :2 * oh, :2 * ow].reshape(nc, oh, 2, ow, 2).permute(0, 1, 3, 2, 4).reshape(nc, oh, ow, 4)
        m = e.max(-1).values
        for i, pos in enumerate(T.PATTERNS):
            sel = pat == i
            assert bool(sel.any()) or nc * oh * ow <= i, row[0]
            for k in range(4):
                assert bool(((e[..., k] == m) == (k in pos))[sel].all()) and bool((m[sel] > 0).all()), (row[0], i, k)
        sel = pat == 7
        assert bool(sel.any()) and bool((m[sel] <= 0).all()), row[0]
        assert bool((e[..., 0][sel] == 0).all()) and not bool(torch.signbit(e[..., 0][sel]).any()), row[0]
        assert bool((e[..., 1][sel] == 0).all()) and bool(torch.signbit(e[..., 1][sel]).all()), row[0]
        assert bool((g != 0).all()) and (t is None or bool((t != 0).all())), row[0]
    for row in T.RMP:
        z = T.rmp_inputs(row)[2].reshape(-1)
        zero = z == 0
        assert bool(zero[0::7].all()) and bool(zero[3::7].all()) and int(zero.sum()) == len(z[0::7]) + len(z[3::7]), row[0]
        assert bool(torch.signbit(z[3::7]).all()) and not bool(torch.signbit(z[0::7]).any()), row[0]


# ---------------------------------------------------------------------------------------------------------------- bitwise rows
def _bitwise(rid, inputs, refs):
    for t in inputs:
        if t is not None:
            assert T.is_dyadic(t), "%s: an input is not on the 2^-10 grid in [-4, 4]" % rid
    for r in refs:
        assert r.dtype == torch.float64 and torch.equal(r.float().double(), r), "%s: the float64 reference is not representable in fp32" % rid
        assert not bool(torch.signbit(r[r == 0]).any()), "%s: a negative zero in the reference" % rid


def test_bitwise_rows_have_dyadic_inputs_and_fp32_representable_references():
    n = 0
    for row in T.MP2:
        z = T.pool_input(row, 2)
        _bitwise(row[0], [z], [R.maxpool2_relu_pad(z, row[4])["out"][0]])
        n += 1
    for row in T.MP3:
        z = T.pool_input(row, 3)
        _bitwise(row[0], [z], [R.maxpool3s2_relu_pad(z, row[4])["out"][0]])
        n += 1
    for row in T.S2D:
        x = T.dyadic(row[1:5], 7050, row[0])
        ref = R.s2d4_pad(x, row[5], row[6], row[7])["out"][0]
        _bitwise(row[0], [x], [ref])
        assert ref.shape == (row[1], 16 * row[2], row[6], row[7])
        n += 1
    for row in T.MPB:
        g, z, t, _ = T.mpb_inputs(row)
        _bitwise(row[0], [g, z, t], [R.maxpool2_relu_bwd(g, z, t, row[4])["gz"][0]])
        n += 1
    for row in T.RMP:
        g, g2, z = T.rmp_inputs(row)
        _bitwise(row[0], [g, g2, z], [R.relu_mask_pad(g, g2, z, row[4])["out"][0]])
        n += 1
    for row in T.ZB:
        buf = T.zb_input(row)
        res = R.zero_border(buf, row[4])
        p = row[4]
        _bitwise(row[0], [buf[:, p:-p, p:-p]], [res["buf"][0]])
        assert int(res["own"].sum()) == 2 * p * (row[3] + 2 * p + row[2])
        n += 1
    assert n == len(T.MP2 + T.MP3 + T.S2D + T.MPB + T.RMP + T.ZB)


def test_the_pooling_adjoint_judge_follows_autograd():
    """the first-maximum rule is PyTorch's: relu -> max_pool2d -> <g, .>, plus <tap, relu(z)>, differentiated by autograd"""
    for row in [r for r in T.MPB if r[1] == T.NCR and r[4] == 1 and r[5] == 0]:
        g, z, t, _ = T.mpb_inputs(row)
        zz = z.double().requires_grad_(True)
        f = torch.relu(zz)
        loss = (torch.nn.functional.max_pool2d(f.unsqueeze(0), 2, 2)[0] * g.double()).sum() + ((f * t.double()).sum() if t is not None else 0.0)
        loss.backward()
        ref = R.maxpool2_relu_bwd(g, z, t, 0)["gz"][0]
        assert torch.equal(ref, zz.grad + 0.0), row[0]


# ---------------------------------------------------------------------------------------------------------------- exact-sum rows
def test_exact_sum_rows_sum_exactly_in_fp32_in_two_orders():
    seen = 0
    for row in T.L1R:
        if not row[4]:
            continue
        za, zb, _ = T.l1r_inputs(row)
        assert torch.equal(za * 64, torch.round(za * 64)) and torch.equal(zb * 64, torch.round(zb * 64))
        d = (za.clamp_min(0) - zb.clamp_min(0)).abs()
        exact = float(d.double().sum())
        assert float(torch.cumsum(d, 0)[-1]) == exact and float(torch.cumsum(d.flip(0), 0)[-1]) == exact and float(d.sum()) == exact, row[0]
        seen += 1
    for row in T.LPL:
        if not row[9]:
            continue
        z0, z1, w, _ = T.lpl_inputs(row)
        assert torch.equal(w * 8, torch.round(w * 8))
        f0, f1 = z0.clamp_min(0), z1.clamp_min(0)
        assert bool((f0.sum(1) == 1).all()) and bool((f1.sum(1) == 1).all()) and bool(((f0 == 0) | (f0 == 1)).all())
        one = torch.tensor(1.0) / (torch.tensor(1.0) + torch.tensor(1e-10))
        assert float(one) == 1.0                                                  # 1 / (1 + eps) in fp32
        t = f0 - f1
        d = (w.view(1, 3, 1, 1) * t * t).sum(1).reshape(-1)
        exact = float(d.double().sum())
        assert float(torch.cumsum(d, 0)[-1]) == exact and float(torch.cumsum(d.flip(0), 0)[-1]) == exact, row[0]
        # the float64 value carries eps: 2e-10 of it, below 1 % of the row's unit
        c, gc = T.lpl_coeffs(row)
        ref, unit = R.lpips_layer(z0, z1, w, c, gc, T.lpl_workgroups(row), True, exact_sum=True)["loss"]
        assert abs(float(ref) - c / d.numel() * exact) < 0.01 * float(unit), row[0]
        seen += 1
    assert seen == 3


# ---------------------------------------------------------------------------------------------------------------- honest units
def _head32(z0, z1, w, coeff, gc, flip):
    """plain fp32 evaluation of the header formula of vts_lpips_layer, channels summed in ascending or descending order"""
    if flip:
        z0, z1, w = z0.flip(1), z1.flip(1), w.flip(0)
    f0, f1 = z0.float().clamp_min(0), z1.float().clamp_min(0)
    n, c, h, wd = f0.shape
    hw = h * wd
    wv = w.float().view(1, -1, 1, 1)
    eps = torch.tensor(1e-10, dtype=torch.float32)
    r0, r1 = torch.cumsum(f0 * f0, 1)[:, -1:].sqrt(), torch.cumsum(f1 * f1, 1)[:, -1:].sqrt()
    i0, i1 = 1.0 / (r0 + eps), 1.0 / (r1 + eps)
    t = f0 * i0 - f1 * i1
    d = torch.cumsum(wv * t * t, 1)[:, -1]
    S = torch.cumsum(wv * t * f0, 1)[:, -1:]
    g2 = torch.tensor(2.0 * gc, dtype=torch.float32) / float(hw)
    k1 = g2 * i0
    k2 = torch.where(r0 > 0, g2 * S * i0 * i0 / torch.where(r0 > 0, r0, torch.ones_like(r0)), torch.zeros_like(r0))
    dz = torch.where(f0 > 0, k1 * wv * t - k2 * f0, torch.zeros_like(f0))
    dd = d.reshape(-1)
    value = float(torch.cumsum(dd.flip(0) if flip else dd, 0)[-1].double()) * coeff / hw
    return value, (dz.flip(1) if flip else dz)


def _rejects(got, ref, unit):
    """a reference moved by 3 units at the element with the largest unit is rejected"""
    i = int(torch.argmax(unit.reshape(-1)))
    if float(unit.reshape(-1)[i]) == 0:
        return True
    bad = ref.clone().reshape(-1)
    bad[i] += 3 * unit.reshape(-1)[i]
    return R.worst(got, bad.reshape(ref.shape), unit)[0] > BOUND


def test_units_of_the_lpips_head_are_honest():
    for row in T.LPL:
        if row[9]:
            continue
        z0, z1, w, _ = T.lpl_inputs(row)
        c, gc = T.lpl_coeffs(row)
        ref = R.lpips_layer(z0, z1, w, c, gc, T.lpl_workgroups(row), row[5] == 0)
        for flip in (False, True):
            value, dz = _head32(z0, z1, w, R._f32(c), R._f32(gc), flip)
            assert R.worst(dz, *ref["dz0"])[0] <= 1.0, (row[0], flip, R.worst(dz, *ref["dz0"]))
            assert R.worst(torch.tensor([value]), *ref["loss"])[0] <= 1.0, (row[0], flip)
            assert _rejects(dz, *ref["dz0"]), row[0]
        # the pixel with the largest term dropped from the loss: at least 10 times the bound
        n, _, h, wd = z0.shape
        one = [R.lpips_layer_judge(z0.double()[:, :, y:y + 1, x:x + 1], z1.double()[:, :, y:y + 1, x:x + 1], w.double(), 1.0, 1.0, raw=True)[0]
               for y in range(h) for x in range(wd)]
        if n * h * wd >= 4:
            assert abs(R._f32(c)) / (h * wd) * float(max(one)) / n >= 10 * float(ref["loss"][1]), row[0]


def test_units_of_the_relu_l1_are_honest():
    for row in T.L1R:
        za, zb, _ = T.l1r_inputs(row)
        c = T.l1r_coeff(row)
        ref, unit = R.l1_relu(za, zb, c, T.l1r_workgroups(row[1]), exact_sum=row[4])["loss"]
        d = (za.clamp_min(0) - zb.clamp_min(0)).abs()
        for v in (d, d.flip(0)):
            got = float(torch.cumsum(v, 0)[-1].double()) * c
            assert abs(got - float(ref)) <= float(unit), row[0]
        i = int(torch.argmax(d))
        assert row[1] == 1 or float(d[i]) * c >= 10 * float(unit), row[0]          # one dropped element
        g = R.l1_relu(za, zb, c, 1)["grad"][0]
        assert set(g.tolist()) <= {c, -c, 0.0} and torch.equal(g.float().double(), g)


def test_units_of_the_input_scaling_and_the_stack_adjoint_are_honest():
    sh, sc = torch.tensor(T.LPIPS_SHIFT), torch.tensor(T.LPIPS_SCALE)
    for row in T.LIN:
        rid, n, cx, hw, _ = row
        x, g, seed = T.lin_inputs(row)
        ref, unit = R.lpips_input(x, T.LPIPS_SHIFT, T.LPIPS_SCALE)["y"]
        got = (x.expand(-1, 3, -1) - sh.view(1, 3, 1)) / sc.view(1, 3, 1)
        assert R.worst(got, ref, unit)[0] <= 1.0 and _rejects(got, ref, unit), rid
        for acc in (False, True):
            ref, unit = R.lpips_input_bwd(g, T.LPIPS_SCALE, cx, seed if acc else None)["dx"]
            p = g * (1.0 / sc).view(1, 3, 1)
            for order in ((0, 1, 2), (2, 1, 0)):
                got = (p[:, order[0]] + p[:, order[1]] + p[:, order[2]]).unsqueeze(1) if cx == 1 else p
                got = got + seed if acc else got
                assert R.worst(got, ref, unit)[0] <= 1.0 and _rejects(got, ref, unit), (rid, acc)
    for row in T.VSB:
        rid, n, h, w = row[:4]
        dx, sI, sT = T.vsb_inputs(row)
        for acc in (False, True):
            ref = R.vgg_stack_input_bwd(dx, n, sI if acc else None, sT if acc else None)
            t = torch.stack([dx[n:2 * n], dx[2 * n:]], 1)
            for a, b, c in ((0, 1, 2), (2, 1, 0)):
                gT, gI = (t[:, :, a] + t[:, :, b]) + t[:, :, c], dx[:n]
                if acc:
                    gT, gI = gT + sT, gI + sI
                assert R.worst(gT, *ref["dT"])[0] <= 1.0 and R.worst(gI, *ref["dI"])[0] <= 1.0, (rid, acc)
                assert _rejects(gT, *ref["dT"]) and (not acc or _rejects(gI, *ref["dI"])), (rid, acc)
        assert float(R.vgg_stack_input_bwd(dx, n)["dI"][1].max()) == 0           # a copy: exact


def test_the_moved_head_judge_is_the_one_the_bf16_tests_use():
    from tests import lpips_bf16_ref as B
    assert B.lpips_layer_judge is R.lpips_layer_judge
    f0, f1 = torch.rand(2, 5, 3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1)), torch.rand(2, 5, 3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    w = torch.rand(5, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    v, vb, dz, b = R.lpips_layer_judge(f0, f1, w, 0.3, 0.3)
    # the defaults are the bf16 head's: one workgroup per 32 pixels of the padded map, 26 roundings on a term's path
    v2, vb2, dz2, b2 = R.lpips_layer_judge(f0, f1, w, 0.3, 0.3, workgroups=2 * ((5 * 6 + 31) // 32), addends=27)
    assert float(v) == float(v2) and float(vb) == float(vb2) and torch.equal(dz, dz2) and torch.equal(b, b2)
