"""The case table of tests/test_resample_gpu.py: the smallest shapes at which the padding / blur / tap / table-resampling kernels of
csrc/vts_resample.hip, the upfirdn2d and bias_act kernels of csrc/vts_stylegan2.hip and the nearest / tanh_bwd kernels of csrc/vts_spade.hip
can still go wrong, with the kernel instance each row expects and its deterministic inputs (oracle.detrand).  Plain data and CPU tensors:
it imports without a GPU, and tests/test_resample_cases.py holds it against the kernel and instance names in the sources.

Exact rows: wherever the arithmetic allows, the inputs are small-integer-valued floats (round(8 uniform)) and the taps dyadic ([1 2 1]^2 / 16,
[1 3 3 1]^2 / 16 or / 64, 1 / 64), so every sum is exact in fp32 in any order and the row is judged bitwise.  The other rows (affine +
activation, a non-dyadic FIR kernel, the bicubic tables, bias_act, tanh) are judged against the derived unit of oracle/launch_ref.py.

Kinks: fmaf(x, scale, shift) = 0 of the activations, x + bias = 0 of bias_act.  Apart from the planted exact ties no input lies within KINK
of one."""
import math

import numpy as np
import torch

from oracle import detrand
from step_glue_cases import KINK, away  # noqa: F401  (away: the margin rule of the kinked rows without an affine)

NONE, LRELU, RELU, TANH = 0, 1, 2, 3
ZERO, REFLECT, REPLICATE = 0, 1, 2


def ints(shape, seed, name):
    """small-integer-valued floats in [-8, 8] (+ 0.0: no negative zero, whose sign a sum does not keep)"""
    return torch.round(detrand.uniform(shape, seed, name) * 8) + 0.0


def affine(n, c, seed):
    """(scale, shift) [N, C]: |scale| in [0.5, 1.5] with both signs, |shift| <= 0.3"""
    s = detrand.uniform((n, c), seed, "scale")
    return torch.where(s >= 0, 0.5 + s, -0.5 + s).float(), (detrand.uniform((n, c), seed, "shift") * 0.3).float()


def off_kink(x, scale, shift):
    """x with every element whose fmaf(x, scale, shift) lies within 2 KINK of 0 moved so that it lies 4 KINK further"""
    n, c = x.shape[:2]
    s, b = scale.double().view(n, c, 1, 1), shift.double().view(n, c, 1, 1)
    t = x.double() * s + b
    return torch.where(t.abs() < 2 * KINK, x.double() + 4 * KINK / s, x.double()).float()


def act_input(shape, seed, name, act, with_affine):
    """(x, scale, shift, tie mask) of a row with an activation: kept off the kink; without an affine one planted exact tie x == 0"""
    n, c = shape[:2]
    x = detrand.uniform(shape, seed, name) * (3.0 if act == TANH else 1.0)
    tie = torch.zeros(shape, dtype=torch.bool)
    if with_affine:
        sc, sh = affine(n, c, seed)
        return (off_kink(x, sc, sh) if act in (LRELU, RELU) else x), sc, sh, tie
    if act in (LRELU, RELU):
        x = away(x, 0.0)
        x.view(-1)[x.numel() // 2] = 0.0
        tie.view(-1)[x.numel() // 2] = True
    return x, None, None, tie


# ---- vts_pad_affine / vts_pad_bwd.  (id, N, C, H, W, (pt, pb, pl, pr), mode, act, affine, res, layout)
# layout: 'dense'; 'gap' = input batch stride 5 elements beyond the sample (NaN between); 'stack' = output is channels 1:4 of a 7-channel
# stack (out_nstride) whose other channels must stay NaN (C = 3)
_PADS4 = [(3, 3, 3, 3), (1, 1, 1, 1), (0, 0, 0, 0), (2, 0, 1, 3)]
PAD = []
for _m in (ZERO, REFLECT, REPLICATE):
    for _i, _p in enumerate(_PADS4):
        _k = _m * 4 + _i
        PAD.append(("pad-m%d-p%d%d%d%d-5x7" % ((_m,) + _p), 2, 3, 5, 7, _p, _m, _k % 4, _k % 3 != 0, _k % 2 == 1, ("dense", "gap", "stack")[_k % 3]))
PAD += [
    ("pad-reflect-max-5x7", 2, 3, 5, 7, (4, 4, 6, 6), REFLECT, LRELU, True, False, "dense"),       # pad = size - 1, the legal maximum
    ("pad-reflect-max-2x2", 1, 1, 2, 2, (1, 1, 1, 1), REFLECT, NONE, False, False, "dense"),
    ("pad-replicate-1x1", 1, 1, 1, 1, (2, 1, 1, 2), REPLICATE, RELU, True, True, "dense"),
    ("pad-zero-1x1", 1, 1, 1, 1, (2, 1, 1, 2), ZERO, TANH, True, False, "dense"),
    ("pad-replicate-1x9", 2, 3, 1, 9, (3, 0, 2, 2), REPLICATE, NONE, False, False, "gap"),
    ("pad-zero-9x1", 2, 3, 9, 1, (0, 3, 2, 2), ZERO, LRELU, False, True, "stack"),
    ("pad-pw64-ph4", 2, 3, 2, 58, (1, 1, 3, 3), REFLECT, TANH, True, True, "dense"),                # PW = 64: one full x block; PH = 4
    ("pad-pw65-ph5", 2, 3, 3, 62, (1, 1, 3, 0), REPLICATE, LRELU, True, False, "stack"),            # PW = 65: x = 64 is the image's last column
    ("pad-pw67-edge-in-image", 2, 3, 5, 62, (2, 2, 3, 2), REFLECT, RELU, False, True, "gap"),      # PW = 67, PH = 9; x = 64 inside the image
    ("pad-pw67-edge-in-pad", 2, 3, 5, 60, (2, 2, 3, 4), REFLECT, NONE, True, False, "dense"),      # x = 64 inside the right pad
    ("pad-pw67-edge-in-pad-replicate", 1, 1, 5, 60, (2, 2, 3, 4), REPLICATE, TANH, False, False, "dense"),
    ("pad-pw67-edge-in-pad-zero", 2, 3, 5, 60, (2, 2, 3, 4), ZERO, LRELU, True, True, "stack"),
]
# the adjoint: every (shape, pads, mode) of PAD once, with and without accumulate; the replicate corner collects (pt + 1)(pl + 1) terms
PAD_BWD = sorted({(r[1], r[2], r[3], r[4], r[5], r[6]) for r in PAD})


def pad_inputs(row):
    """(x, scale, shift, res or None, tie mask)"""
    rid, n, c, h, w, (pt, pb, pl, pr), mode, act, aff, res, _ = row
    x, sc, sh, tie = act_input((n, c, h, w), 5000, rid, act, aff)
    r = detrand.uniform((n, c, h + pt + pb, w + pl + pr), 5000, rid + "res") if res else None
    return x, sc, sh, r, tie


# ---- vts_blur_down / vts_blur_up and adjoints.  (id, kind, N, C, H, W, variant): 'plain' (integers: bitwise), 'gap' (plain, input batch
# stride with a NaN gap), 'lrelu' / 'relu' (affine + activation: the unit bound)
_DOWN = [(2, 2), (3, 2), (5, 7), (8, 130), (9, 129)]        # OW = 65 from an even and from an odd width (the odd one reads the reflected column)
_UP = [(1, 1), (1, 3), (5, 33), (3, 64)]                    # OW = 66 and 128
BLUR = []
for _kind, _shapes in (("down", _DOWN), ("up", _UP)):
    for _i, (_h, _w) in enumerate(_shapes):
        for _v in ("plain", "gap", "lrelu", "relu"):
            _n, _c = (1, 1) if (_i == 0 and _v == "plain") else (2, 3)
            BLUR.append(("blur-%s-%dx%d-%s" % (_kind, _h, _w, _v), _kind, _n, _c, _h, _w, _v))
BLUR_BWD = [(k, h, w) for k, shapes in (("down", _DOWN), ("up", _UP)) for h, w in shapes]          # N = 2, C = 3; x accumulate


def blur_inputs(row):
    """(x, scale, shift, act, tie mask)"""
    rid, _, n, c, h, w, v = row
    if v in ("plain", "gap"):
        return ints((n, c, h, w), 5100, rid), None, None, NONE, None
    act = LRELU if v == "lrelu" else RELU
    x, sc, sh, tie = act_input((n, c, h, w), 5100, rid, act, True)
    return x, sc, sh, act, tie


# ---- vts_tap_embed / vts_tap_extract (a, b) and the _at forms.  (id, entry, K, oy or a, ox or b, rows); rows * 16 crosses 256 at 17
TAP = [("tap-ab-k%d-%d%d" % (k, a, b), "ab", k, a, b, (1, 16, 17)[(k + 2 * a + b) % 3]) for k in (1, 3, 5, 7, 8) for a in (0, 1) for b in (0, 1)]
TAP += [("tap-at-k%d-%+d%+d" % (k, oy, ox), "at", k, oy, ox, (17, 1, 16)[(k + oy + ox) % 3])
        for k in (1, 3, 8) for oy, ox in ((-3, -3), (-1, -1), (-1, 0), (7, 7), (4, 0))]

# ---- vts_resample_table with the host-built anti-aliased bicubic tables.  (id, NC, IH, IW, OH, OW)
RESAMPLE = [
    ("resample-32x32-64x64", 6, 32, 32, 64, 64), ("resample-37x53-32x32", 6, 37, 53, 32, 32),
    ("resample-96x80-24x20", 6, 96, 80, 24, 20),                    # wide windows (scale 4: 17 taps per axis)
    ("resample-identity-32x32", 6, 32, 32, 32, 32),                 # bitwise equal to the input
    ("resample-5x300-3x7", 6, 5, 300, 3, 7),
    ("resample-total-255", 1, 20, 23, 15, 17), ("resample-total-256", 1, 24, 24, 16, 16), ("resample-total-257", 1, 3, 300, 1, 257),
]

# ---- vts_upfirdn2d / _bwd through the C entry.  (id, NC, IH, IW, kernel, up, down, (px0, px1), (py0, py1), exact, forward instance)
# kernels: 'k4' make_kernel([1 3 3 1]) * up^2 (multiples of 1/64), 'k3' make_kernel([1 2 1]), 'k8' 8 x 8 of 1/64, 'k1' [[1]],
# 'k2x3' and 'k9x7' asymmetric, non-dyadic (the unit bound)
TILE, GEN, TILE_ADJ, GEN_ADJ = "ufd_tile_kernel", "upfirdn2d_kernel", "ufd_tile_kernel adjoint", "upfirdn2d_adj_kernel"
UFD = [
    ("ufd-tile-k4-p21-15x63", 6, 15, 63, "k4", 1, 1, (2, 1), (2, 1), True, TILE),
    ("ufd-tile-k4-p11-16x64", 6, 17, 65, "k4", 1, 1, (1, 1), (1, 1), True, TILE),
    ("ufd-tile-k4-p21-17x65", 6, 17, 65, "k4", 1, 1, (2, 1), (2, 1), True, TILE),
    ("ufd-tile-k8-17x65", 6, 17, 65, "k8", 1, 1, (4, 3), (4, 3), True, TILE),         # KW = 8: the last lane reads column 71 of the pitch-72 row
    ("ufd-tile-k1-17x65", 6, 17, 65, "k1", 1, 1, (0, 0), (0, 0), True, TILE),
    ("ufd-tile-k2x3-16x65", 6, 16, 64, "k2x3", 1, 1, (1, 2), (0, 1), False, TILE),
    ("ufd-tile-negpad-17x65", 6, 19, 67, "k4", 1, 1, (-1, 2), (-1, 2), True, TILE),
    ("ufd-tile-nc1-1x1", 1, 1, 1, "k4", 1, 1, (2, 1), (2, 1), True, TILE),
    ("ufd-gen-up2", 6, 5, 33, "k4", 2, 1, (2, 1), (2, 1), True, GEN),
    ("ufd-gen-down2", 6, 9, 67, "k4", 1, 2, (1, 1), (1, 1), True, GEN),
    ("ufd-gen-up2-down2", 6, 7, 35, "k4", 2, 2, (2, 1), (2, 1), True, GEN),
    ("ufd-gen-k9x7", 6, 6, 40, "k9x7", 1, 1, (3, 3), (4, 4), False, GEN),             # above UT_MAXK
    ("ufd-gen-nc65536", 65536, 2, 2, "k3", 1, 1, (1, 1), (1, 1), True, GEN),          # above the grid-z limit
]
UFD_ADJOINT = {TILE: TILE_ADJ, GEN: GEN_ADJ}


def ufd_kernel(name, up):
    from oracle.stylegan2 import make_kernel
    if name == "k4":
        return make_kernel((1, 3, 3, 1)) * float(up * up)
    if name == "k3":
        return make_kernel((1, 2, 1))
    if name == "k8":
        return torch.full((8, 8), 1.0 / 64)
    if name == "k1":
        return torch.ones(1, 1)
    shape = {"k2x3": (2, 3), "k9x7": (9, 7)}[name]
    return (detrand.uniform(shape, 5300, name) * (2.0 / math.sqrt(shape[0] * shape[1]))).float()


def ufd_out_hw(row):
    _, _, ih, iw, kname, up, down, (px0, px1), (py0, py1), _, _ = row
    kh, kw = ufd_kernel(kname, up).shape
    return (ih * up + py0 + py1 - kh) // down + 1, (iw * up + px0 + px1 - kw) // down + 1


def ufd_input(row, shape, name):
    return ints(shape, 5300, row[0] + name) if row[9] else detrand.uniform(shape, 5300, row[0] + name)


# ---- vts_bias_act / _bwd.  (id, N, C, HW, bias, res, slope, gain)
BIAS_ACT = []
for _i, (_n, _c, _hw) in enumerate([(1, 1, 1), (2, 3, 99), (1, 5, 256), (3, 2, 257)]):
    for _j, (_s, _g) in enumerate([(0.2, math.sqrt(2.0)), (0.2, 0.7), (0.0, 1.0)]):
        _k = _i + _j
        BIAS_ACT.append(("bias-act-%dx%dx%d-s%g-g%.2g-%s%s" % (_n, _c, _hw, _s, _g, "b" if _k % 2 == 0 else "", "r" if _k % 4 < 2 else ""),
                         _n, _c, _hw, _k % 2 == 0, _k % 4 < 2, _s, _g))


def bias_act_inputs(row):
    """(x, bias, res, g, tie mask): x + bias kept off 0 apart from planted exact ties x = -bias (x = 0 without a bias)"""
    rid, n, c, hw, has_b, has_r, _, _ = row
    x = detrand.uniform((n, c, hw), 5400, rid)
    b = (detrand.uniform((c,), 5400, rid + "b") * 0.5).float() if has_b else None
    bb = b.view(1, c, 1) if has_b else torch.zeros(1, 1, 1)
    x = (away(x + bb, 0.0) - bb).float()
    tie = torch.zeros(n, c, hw, dtype=torch.bool)
    tie[:, :, ::7] = True
    x = torch.where(tie, (-bb).expand(n, c, hw), x).contiguous()
    r = detrand.uniform((n, c, hw), 5400, rid + "r") if has_r else None
    return x, b, r, detrand.uniform((n, c, hw), 5400, rid + "g"), tie


# ---- vts_nearest_resize / _bwd.  (id, NC, IH, IW, OH, OW).  DIFFER: per-axis size pairs at which ATen's float rule
# min(floor(dst * (float)in / (float)out), in - 1) and exact integer division dst * in / out disagree at some dst.
DIFFER = [(14, 46), (6, 74), (9, 111), (3, 123)]
SECOND_SWEEP = 4096 * 256            # the grid-stride kernels launch at most 4096 workgroups of 256
NEAREST = [
    ("nearest-14x6-46x74", 6, 14, 6, 46, 74), ("nearest-9x3-111x123", 6, 9, 3, 111, 123),
    ("nearest-46x74-14x6", 6, 46, 74, 14, 6), ("nearest-111x123-9x3", 6, 111, 123, 9, 3),       # the reverse direction
    ("nearest-identity-7x9", 6, 7, 9, 7, 9), ("nearest-double-5x6", 6, 5, 6, 10, 12),
    ("nearest-skip-30x20-4x6", 6, 30, 20, 4, 6),          # sources no output reads: their gradient is exactly 0
    ("nearest-nc1-1x1-3x5", 1, 1, 1, 3, 5),
    ("nearest-second-sweep-fwd", 1, 2, 2, 1025, 1024),    # the forward's second sweep
    ("nearest-second-sweep-bwd", 1, 1025, 1024, 2, 2),    # the adjoint's second sweep
]


def rules_differ(n_in, n_out):
    """whether the fp32 rule and integer division give a different source index for some destination"""
    dst = np.arange(n_out)
    scale = np.float32(n_in) / np.float32(n_out)
    f = np.minimum(np.floor(dst.astype(np.float32) * scale).astype(np.int64), n_in - 1)
    return bool((f != dst * n_in // n_out).any())


# ---- vts_nearest_up2 / _bwd (NC, H, W) and vts_tanh_bwd (n)
UP2 = [("up2-7x3x5", 7, 3, 5), ("up2-1x1x1", 1, 1, 1), ("up2-second-sweep", 1, 1025, 1024)]
TANH_BWD = [1, 257, SECOND_SWEEP + 3]


def kink_rows():
    """(row id, distance of every element from the row's kink, planted ties)"""
    out = []
    for row in PAD:
        if row[7] in (LRELU, RELU):
            x, sc, sh, _, tie = pad_inputs(row)
            out.append((row[0], _kink_distance(x, sc, sh), tie))
    for row in BLUR:
        if row[6] in ("lrelu", "relu"):
            x, sc, sh, _, tie = blur_inputs(row)
            out.append((row[0], _kink_distance(x, sc, sh), tie))
    for row in BIAS_ACT:
        x, b, _, _, tie = bias_act_inputs(row)
        v = x.double() + (b.double().view(1, -1, 1) if b is not None else 0.0)
        out.append((row[0], v.abs(), tie))
    return out


def _kink_distance(x, sc, sh):
    n, c = x.shape[:2]
    if sc is None:
        return x.double().abs()
    return (x.double() * sc.double().view(n, c, 1, 1) + sh.double().view(n, c, 1, 1)).abs()


def pad_bwd_id(r):
    return "pad-bwd-%dx%dx%dx%d-p%d.%d.%d.%d-m%d" % (r[:4] + r[4] + (r[5],))


def pad_bwd_inputs(r):
    """(dpad, din seed): integers"""
    n, c, h, w, (pt, pb, pl, pr), _ = r
    return ints((n, c, h + pt + pb, w + pl + pr), 5050, pad_bwd_id(r)), ints((n, c, h, w), 5050, pad_bwd_id(r) + "seed")


def blur_out_hw(kind, h, w):
    return ((h - 1) // 2 + 1, (w - 1) // 2 + 1) if kind == "down" else (2 * h, 2 * w)


def blur_bwd_inputs(r):
    kind, h, w = r
    return ints((2, 3) + blur_out_hw(kind, h, w), 5150, "g%s%dx%d" % r), ints((2, 3, h, w), 5150, "seed%s%dx%d" % r)


def tap_inputs(row):
    """(w [rows, K, K], dw4 [rows, 4, 4], dw seed [rows, K, K]): integers"""
    rid, _, k, _, _, rows = row
    return ints((rows, k, k), 5200, rid), ints((rows, 4, 4), 5200, rid + "g"), ints((rows, k, k), 5200, rid + "seed")


def tap_origin(row):
    """(oy, ox): position of the block's tap (0, 0) in the K x K grid"""
    return (4 * row[3], 4 * row[4]) if row[1] == "ab" else (row[3], row[4])


def nearest_inputs(row):
    rid, nc, ih, iw, oh, ow = row
    return ints((1, nc, ih, iw), 5500, rid), ints((1, nc, oh, ow), 5500, rid + "g"), ints((1, nc, ih, iw), 5500, rid + "seed")


def up2_inputs(row):
    rid, nc, h, w = row
    return ints((1, nc, h, w), 5600, rid), ints((1, nc, 2 * h, 2 * w), 5600, rid + "g"), ints((1, nc, h, w), 5600, rid + "seed")


def claimed_instances():
    """every instance string a row of this table expects vts_last_kernel() to report"""
    c = {r[10] for r in UFD} | {UFD_ADJOINT[r[10]] for r in UFD}
    c |= {"pad_affine_kernel", "pad_bwd_kernel", "blur_down_kernel", "blur_down_bwd_kernel", "blur_up_kernel", "blur_up_bwd_kernel",
          "tap_embed_kernel", "tap_extract_kernel", "resample_table_kernel", "bias_act_kernel", "bias_act_bwd_kernel", "nearest_fwd_kernel",
          "nearest_bwd_kernel", "nearest_up2_kernel", "nearest_up2_bwd_kernel", "tanh_bwd_kernel"}
    return c


# kernels of the three sources judged elsewhere: elementwise by tests/test_style_kernels_gpu.py, whose table (tests/style_kernel_cases.py)
# claims the instance strings their entries report
_MODCONV = _SPADE = "tests/test_style_kernels_gpu.py"
COVERED_ELSEWHERE = {k: _MODCONV for k in ("demod_kernel", "modw_kernel", "modw_bwd_kernel", "scale_dot_rows_kernel", "scale_dot_split_kernel",
                                           "scale_dot_finish_kernel", "demod_bwd_w_kernel", "demod_bwd_s_kernel", "wtranspose_kernel")}
COVERED_ELSEWHERE.update({k: _SPADE for k in ("spade_mod_fwd_v4", "spade_mod_fwd_pad", "spade_mod_bwd_sums", "spade_mod_bwd_means", "spade_mod_bwd_apply",
                                              "spade_mod_bwd_apply_v4", "spade_eval_stats_kernel", "sn_wtu_kernel", "sn_v_kernel", "sn_wv_kernel",
                                              "sn_sigma_kernel", "sn_scale_kernel", "sn_bwd_dot_kernel", "sn_bwd_total_kernel", "sn_bwd_apply_kernel")})


def row_ids():
    ids = [r[0] for r in PAD + BLUR + TAP + RESAMPLE + UFD + BIAS_ACT + NEAREST + UP2]
    ids += [pad_bwd_id(r) for r in PAD_BWD]
    ids += ["blur-%s-bwd-%dx%d" % r for r in BLUR_BWD] + ["tanh-bwd-%d" % n for n in TANH_BWD]
    return ids
