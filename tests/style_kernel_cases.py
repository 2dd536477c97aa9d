"""The case table of tests/test_style_kernels_gpu.py: the smallest shapes at which the kernels that carry the style and segmentation
conditioning can still go wrong (csrc/vts_spade.hip: modulate, eval statistics, spectral norm; csrc/vts_style.hip: AdaIN;
csrc/vts_style_levels.hip: the 16-class style bias and the mapping Linear; the six vts_modconv_* entries of csrc/vts_stylegan2.hip), with the
instance string each row expects and its deterministic inputs (oracle.detrand).  Plain data and CPU tensors: it imports without a GPU, and
tests/test_style_kernel_cases.py holds it against the kernel names, the instance strings and the launch plans of the sources (the plan
formulas are restated here).

Every input is the DENSE tensor; the GPU test lays it out (padded borders, channel slices, misalignment, guard bands).  The arguments of a
LeakyReLU keep KINK away from 0 apart from the planted exact zeros (gamma = -1 and beta = 0 at PLANT positions)."""
import math

import torch

from oracle import detrand
from step_glue_cases import KINK  # noqa: F401

U = detrand.uniform
GRID_CAP = 4096 * 256            # flat_grid of vts_spade.hip: 4096 workgroups of 256 threads; more work and a thread sweeps again
ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 3
PLANT = 7                        # every PLANT-th element of a LeakyReLU row has the argument exactly 0


def cdiv(a, b):
    return -(-a // b)


def dyadic(shape, seed, name):
    """multiples of 2^-10 in [-4, 4], no negative zero: one fp32 add of two of them is exact"""
    return torch.round(U(shape, seed, name) * 4096) / 1024 + 0.0


# ---------------------------------------------------------------------------------------------------------------- vts_spade_modulate
# (id, N, C, H, W, act, out_pad, pointer 4 bytes off alignment or None)
V4, PAD = "spade_mod_fwd_v4", "spade_mod_fwd_pad"
MOD = [("mod-v4-lrelu", 2, 3, 4, 6, ACT_LRELU, 0, None), ("mod-v4-none", 2, 3, 4, 6, ACT_NONE, 0, None), ("mod-v4-1x8", 2, 3, 1, 8, ACT_LRELU, 0, None),
       ("mod-pad-lrelu", 2, 3, 4, 6, ACT_LRELU, 1, None), ("mod-pad-none", 2, 3, 4, 6, ACT_NONE, 1, None),
       ("mod-scalar-hw25", 2, 3, 5, 5, ACT_LRELU, 0, None)]
MOD += [("mod-scalar-%s-off" % p, 2, 3, 4, 6, ACT_LRELU, 0, p) for p in ("x", "gamma", "beta", "out")]
MOD += [("mod-%dx%d-p%d" % (h, w, p), 2, 3, h, w, ACT_LRELU, p, None) for h, w in ((1, 1), (1, 7), (7, 1)) for p in (0, 1)]
MOD += [("mod-v4-second-sweep", 2, 2, 1090, 962, ACT_LRELU, 0, None),          # 4 * 1048580 / 4 lanes of work > GRID_CAP
        ("mod-pad-second-sweep", 2, 2, 511, 511, ACT_NONE, 1, None)]           # 4 * 513 * 513 > GRID_CAP


def mod_instance(row):
    _, n, c, h, w, _, pad, off = row
    return V4 if pad == 0 and (h * w) % 4 == 0 and off is None else PAD


def mod_work(row):
    """threads' worth of work of the launch: four pixels per lane in the v4 instance, one (padded) pixel otherwise"""
    _, n, c, h, w, _, pad, _ = row
    return n * c * h * w // 4 if mod_instance(row) == V4 else n * c * (h + 2 * pad) * (w + 2 * pad)


def _away_from_kink(beta, p, plant):
    """beta moved so that |p + beta| >= 2 KINK; planted positions get beta = 0 (1 + gamma is exactly 0 there)"""
    t = p + beta.double()
    beta = torch.where(t.abs() < 4 * KINK, beta + 8 * KINK * torch.where(t < 0, -1.0, 1.0).float(), beta)
    return torch.where(plant, torch.zeros_like(beta), beta)


def _stats(x, kind, rid, batch=False):
    """mean / rstd [N C]: the fp32-rounded float64 statistics of x ("own": of each plane, or with `batch` of each channel over the batch,
    repeated), or of something else ("other")"""
    n, c = x.shape[:2]
    if kind == "own" and batch:
        v = x.double().transpose(0, 1).reshape(c, -1)
        return v.mean(1).float().repeat(n), (v.var(1, unbiased=False) + 1e-5).rsqrt().float().repeat(n)
    if kind == "own":
        v = x.double().reshape(n * c, -1)
        return v.mean(1).float(), (v.var(1, unbiased=False) + 1e-5).rsqrt().float()
    return 0.5 * U((n * c,), 7702, rid + "m"), 0.75 + 0.5 * U((n * c,), 7702, rid + "r").abs()


def mod_inputs(row, stats="other", lrelu=None, batch=False):
    """(x, mean, rstd, gamma, beta, planted mask)"""
    rid, n, c, h, w = row[:5]
    lrelu = (row[5] == ACT_LRELU) if lrelu is None else lrelu
    x, gamma, beta = [U((n, c, h, w), 7700, rid + k) for k in ("x", "gamma", "beta")]
    mean, rstd = _stats(x, stats, rid, batch)
    plant = torch.zeros(x.numel(), dtype=torch.bool)
    if lrelu:
        plant[3::PLANT] = True
    plant = plant.view(x.shape)
    gamma = torch.where(plant, torch.full_like(gamma, -1.0), gamma)
    if lrelu:
        p = (x.double() - mean.double().view(n, c, 1, 1)) * rstd.double().view(n, c, 1, 1) * (1 + gamma.double())
        beta = _away_from_kink(beta, p, plant)
    return x, mean, rstd, gamma, beta, plant


# ---------------------------------------------------------------------------------------------------------------- vts_spade_modulate_bwd
# (id, N, C, H, W, mode, act, g_pad, ws: "own" (modes 0 / 1) | "null" | "given" (mode 2), pointer off or None, statistics "own" | "other")
MODB = [("mb-wave-hw1024-nc5", 1, 5, 32, 32, 0, ACT_LRELU, 0, "own", None, "own"), ("mb-block-hw1025-nc5", 1, 5, 25, 41, 0, ACT_LRELU, 1, "own", None, "own"),
        ("mb-wave-hw1024-nc1", 1, 1, 32, 32, 0, ACT_NONE, 1, "own", None, "own"), ("mb-block-hw1025-nc1", 1, 1, 25, 41, 0, ACT_NONE, 0, "own", None, "own"),
        ("mb-mode1-wave", 3, 2, 6, 6, 1, ACT_LRELU, 0, "own", None, "own"), ("mb-mode1-block", 3, 2, 25, 41, 1, ACT_LRELU, 1, "own", None, "own"),
        ("mb-mode2-wave-null", 2, 3, 6, 6, 2, ACT_LRELU, 1, "null", None, "own"), ("mb-mode2-wave-given", 2, 3, 6, 6, 2, ACT_NONE, 0, "given", None, "own"),
        ("mb-mode2-block-null", 2, 3, 25, 41, 2, ACT_LRELU, 0, "null", None, "own"), ("mb-mode2-block-given", 2, 3, 25, 41, 2, ACT_LRELU, 1, "given", None, "own"),
        ("mb-apply-v4-hw36", 2, 3, 6, 6, 0, ACT_LRELU, 1, "own", None, "own"), ("mb-apply-hw25", 2, 3, 5, 5, 0, ACT_LRELU, 1, "own", None, "own"),
        ("mb-apply-x-off", 2, 3, 6, 6, 0, ACT_LRELU, 0, "own", "x", "own"), ("mb-apply-dx-off", 2, 3, 6, 6, 0, ACT_LRELU, 0, "own", "dx", "own"),
        ("mb-apply-second-sweep", 1, 1, 1025, 1025, 0, ACT_NONE, 0, "own", None, "own"),           # 1025^2 > GRID_CAP
        ("mb-apply-v4-second-sweep", 2, 2, 1090, 962, 0, ACT_LRELU, 0, "own", None, "own"),        # 4 * 1048580 / 4 > GRID_CAP
        ("mb-1x1-mode0", 2, 3, 1, 1, 0, ACT_LRELU, 0, "own", None, "own"),
        ("mb-other-statistics", 2, 3, 6, 6, 0, ACT_LRELU, 0, "own", None, "other"), ("mb-other-statistics-mode1", 3, 2, 5, 5, 1, ACT_NONE, 1, "own", None, "other")]


def modb_instance(row):
    _, n, c, h, w, mode, _, _, _, off, _ = row
    sums = "spade_mod_bwd_sums<%s>" % ("wave" if h * w <= 1024 else "block")
    if mode == 2:
        return sums + " frozen"
    return sums + "+spade_mod_bwd_means+spade_mod_bwd_apply" + ("_v4" if (h * w) % 4 == 0 and off is None else "")


def modb_apply_work(row):
    _, n, c, h, w = row[:5]
    return n * c * h * w // (4 if modb_instance(row).endswith("_v4") else 1)


def modb_inputs(row):
    """(g, x, mean, rstd, gamma, beta, planted mask); a 1 x 1 plane's own statistics are mean = x, rstd = 1 / sqrt(eps)"""
    x, mean, rstd, gamma, beta, plant = mod_inputs(row, stats=row[10], lrelu=row[6] == ACT_LRELU, batch=row[5] == 1)
    return U(x.shape, 7710, row[0] + "g"), x, mean, rstd, gamma, beta, plant


# ---------------------------------------------------------------------------------------------------------------- vts_spade_eval_stats
EVS_EPS = 1e-5
EVS = [("evs-nc%d" % (n * c), n, c) for n, c in ((1, 1), (2, 128), (1, 257))]            # (id, N, C): one block, a full one, a second one


def evs_inputs(row):
    """(running_mean, running_var): channel 0 has variance 0"""
    rid, _, c = row
    rv = U((c,), 7720, rid + "v").abs() + 0.01
    rv[0] = 0.0
    return U((c,), 7720, rid + "m"), rv


# ---------------------------------------------------------------------------------------------------------------- spectral norm
# forward (id, Co, K, training, pointer off or None); backward (id, Co, K, accumulate)
SN_EPS = 1e-12
SN_CO, SN_K = (1, 64, 65, 130), (1, 255, 257, 576, 1025)
SN = [("sn-co%d-k%d-train" % (co, k), co, k, 1, None) for co in SN_CO for k in SN_K]
SN += [("sn-co%d-k%d-eval" % (co, k), co, k, 0, None) for co, k in ((1, 1), (65, 576), (130, 257), (64, 1025))]
SN += [("sn-co65-k576-%s-off-%s" % (p, "train" if t else "eval"), 65, 576, t, p) for p in ("w", "v") for t in (1, 0)]
SNB = [("snb-co%d-k%d-%s" % (co, k, "acc" if a else "plain"), co, k, a) for i, co in enumerate(SN_CO) for j, k in enumerate(SN_K) for a in ((i + j) % 2,)]
SNB += [("snb-co3-k4100-plain", 3, 4100, 0), ("snb-co3-k4100-acc", 3, 4100, 1), ("snb-co65-k576-both-acc", 65, 576, 1), ("snb-co64-k257-plain", 64, 257, 0)]


def sn_instance(row):
    _, co, k, training, off = row
    wv = "sn_wv_kernel<%s>+sn_sigma_kernel+sn_scale_kernel" % ("vec" if k % 4 == 0 and off is None else "scalar")
    return ("sn_wtu_kernel+sn_v_kernel+" if training else "") + wv


SNB_INSTANCE = "sn_bwd_dot_kernel+sn_bwd_total_kernel+sn_bwd_apply_kernel"


def sn_ws_floats(co, k):
    return cdiv(co, 64) * k + co


def snb_columns_stride(k):
    """the backward's column grid is capped at 16 workgroups of 256"""
    return cdiv(k, 256) > 16


def sn_inputs(row):
    """(w [Co, K], u [Co], v [K]): u and v are the unit vectors an earlier iteration left"""
    rid, co, k = row[:3]
    w = U((co, k), 7730, rid + "w") * (3.0 / k) ** 0.5
    u, v = U((co,), 7730, rid + "u") + 0.05, U((k,), 7730, rid + "v") + 0.05
    return w, (u.double() / u.double().norm()).float(), (v.double() / v.double().norm()).float()


def snb_inputs(row):
    """(g, w_sn, u, v, sigma [1], seeded dw)"""
    rid, co, k = row[:3]
    w, u, v = sn_inputs(row)
    return U((co, k), 7740, rid + "g"), w * 1.3, u, v, torch.tensor([0.77]), U((co, k), 7740, rid + "dw")


# ---------------------------------------------------------------------------------------------------------------- AdaIN
# (id, NC, HW, kind): "plain"; "offset": |mean x| = 100 std x; "scales": x and s on very different scales
ADA_EPS = 1e-5
ADA = [("ada-nc%d-hw%d" % (nc, hw), nc, hw, "plain") for hw in (2, 36, 63, 64, 65, 129) for nc in (1, 4, 5)]
ADA += [("ada-offset-100-std", 5, 36, "offset"), ("ada-offset-100-std-hw129", 4, 129, "offset"), ("ada-scales-1e3-1e-3", 5, 36, "scales")]


def ada_inputs(row):
    """(g, x, s)"""
    rid, nc, hw, kind = row
    g, x, s = [U((nc, hw), 7750, rid + k) for k in ("g", "x", "s")]
    if kind == "offset":
        x = x + 100.0 * float(x.double().std(1, unbiased=True).mean())
    if kind == "scales":
        x, s = x * 1000.0, s * 0.001
    return g, x, s


# ---------------------------------------------------------------------------------------------------------------- style bias
# forward (id, N, K, Cout, OH, OW, act_out, layout "dense" | "slice"); backward (id, N, K, Cout, OH, OW, accumulate, layout)
SB_SHAPES = [(2, 2), (2, 4), (4, 2), (4, 4), (6, 10), (34, 62), (34, 122), (18, 6), (34, 6), (2, 130), (4, 130)]
SB_K, SB_COUT = (1, 3, 4, 5, 512), (1, 4, 5)
SB = [("sb-%dx%d-k%d-co%d-%s-%s" % (oh, ow, SB_K[i % 5], SB_COUT[i % 3], ("none", "tanh")[i % 2], ("dense", "slice")[(i // 2) % 2]),
       2, SB_K[i % 5], SB_COUT[i % 3], oh, ow, (ACT_NONE, ACT_TANH)[i % 2], ("dense", "slice")[(i // 2) % 2]) for i, (oh, ow) in enumerate(SB_SHAPES)]
SB += [("sb-%dx%d-k%d-co%d-%s-%s" % (oh, ow, k, co, ("none", "tanh")[a == ACT_TANH], lay), 3, k, co, oh, ow, a, lay)
       for oh, ow, k, co, a, lay in ((4, 4, 512, 5, ACT_TANH, "slice"), (6, 10, 1, 4, ACT_NONE, "slice"), (4, 4, 4, 1, ACT_TANH, "dense"), (6, 10, 5, 5, ACT_NONE, "dense"))]
SB += [("sb-1024x514-chunk-cap", 1, 1, 1, 1024, 514, ACT_TANH, "dense")]
SBB = [("sbb-%dx%d-k%d-co%d-%s-%s" % (oh, ow, SB_K[(i + 2) % 5], SB_COUT[(i + 1) % 3], ("plain", "acc")[i % 2], ("dense", "slice")[(i // 2 + 1) % 2]),
        2, SB_K[(i + 2) % 5], SB_COUT[(i + 1) % 3], oh, ow, i % 2, ("dense", "slice")[(i // 2 + 1) % 2]) for i, (oh, ow) in enumerate(SB_SHAPES)]
SBB += [("sbb-1026x2-row-chunk-cap", 1, 3, 1, 1026, 2, 1, "dense"), ("sbb-1024x514", 1, 1, 1, 1024, 514, 0, "dense"),
        ("sbb-4x4-k512-co5-acc-slice", 3, 512, 5, 4, 4, 1, "slice"), ("sbb-6x10-k1-co4-plain-slice", 3, 1, 4, 6, 10, 0, "slice")]
SB_INSTANCE, SBB_INSTANCE = "style_v_kernel+style_bias_apply_kernel", "style_class_sums_kernel+style_dv_kernel+style_dw_kernel"
SLICE_LEAD, SLICE_TAIL = 2, 1            # a "slice" is channels 2 : 2 + Cout of a tensor of Cout + 3 channels


def sb_pixel_chunks(oh, ow):
    """(workgroups per plane of the forward's apply launch, pixels of each)"""
    gx = min(256, cdiv(oh * ow, 2048))
    return gx, cdiv(oh * ow, gx)


def sb_row_chunks(oh):
    """(row chunks of the backward's class sums, rows of each, chunks that own no row)"""
    chunks = min(max(cdiv(oh, 16), 1), 64)
    rows = cdiv(oh, chunks)
    return chunks, rows, sum(1 for k in range(chunks) if k * rows >= oh)


def sb_ws_floats(n, cout, oh):
    return n * cout * 16 * (sb_row_chunks(oh)[0] + 1)


def sb_code(row):
    """the code [N, K]: negatives throughout, +0 at element 1 and -0 at element 2 where it is that long"""
    rid, n, k = row[:3]
    code = U((n, k), 7760, rid + "code")
    flat = code.view(-1)
    if flat.numel() > 1:
        flat[1] = 0.0
    if flat.numel() > 2:
        flat[2] = -0.0
    return code


def sb_inputs(row):
    """(code, w [K, Cout, 4, 4], seeded out [N, Cout, OH, OW])"""
    rid, n, k, cout, oh, ow = row[:6]
    return sb_code(row), U((k, cout, 4, 4), 7760, rid + "w") * (2.0 / k) ** 0.5, U((n, cout, oh, ow), 7760, rid + "out")


def sbb_inputs(row):
    """(g [N, Cout, OH, OW], code, seeded dw [K, Cout, 4, 4])"""
    rid, n, k, cout, oh, ow = row[:6]
    return U((n, cout, oh, ow), 7770, rid + "g"), sb_code(row), U((k, cout, 4, 4), 7770, rid + "dw")


# ---------------------------------------------------------------------------------------------------------------- style Linear
# forward (id, N, K, P); backward (id, N, K, P, dx wanted, accumulate)
LIN_P, LIN_K = (1, 3, 4, 5, 257, 131073), (1, 63, 64, 65, 257)
LIN = [("lin-n%d-k2-p%d" % (n, p), n, 2, p) for i, p in enumerate(LIN_P) for n in ((1, 3)[i % 2],)]
LIN += [("lin-n%d-k%d-p5" % (n, k), n, k, 5) for i, k in enumerate(LIN_K) for n in ((3, 1)[i % 2],)]
LINB = [("linb-n%d-k%d-p%d-%s-%s" % (r[1], r[2], r[3], ("nodx", "dx")[i % 2], ("plain", "acc")[(i // 2) % 2]), r[1], r[2], r[3], i % 2, (i // 2) % 2)
        for i, r in enumerate(LIN)]
LINB += [("linb-n1-k2-p1-dx-plain", 1, 2, 1, 1, 0), ("linb-n3-k2-p131073-dx-acc", 3, 2, 131073, 1, 1), ("linb-n1-k2-p257-dx-plain", 1, 2, 257, 1, 0), ("linb-n1-k257-p5-dx-acc", 1, 257, 5, 1, 1)]
LIN_INSTANCE = "style_linear_kernel"


def linb_instance(row):
    return "style_linear_dw_kernel" + ("+style_linear_dx_kernel+style_linear_dx_sum_kernel" if row[4] else "")


def lin_chunks(p):
    """(chunks of the dx partial sums, rows of each)"""
    chunks = min(max(cdiv(p, 256), 1), 512)
    return chunks, cdiv(p, chunks)


def lin_ws_floats(n, k, p):
    return lin_chunks(p)[0] * n * k


def lin_inputs(row):
    """(x [N, K], w [P, K], dz [N, P], seeded dw [P, K])"""
    rid, n, k, p = row[:4]
    return U((n, k), 7780, "x%d-%d" % (n, k)), U((p, k), 7780, "w%d-%d" % (p, k)) * (3.0 / k) ** 0.5, U((n, p), 7780, "dz%d-%d" % (n, p)), U((p, k), 7780, rid + "dw")


# ---------------------------------------------------------------------------------------------------------------- modconv: demod, weight
# (id, N, Cout, Cin, KK, weight magnitude): Cin KK in {1, 27, 256, 261}; "tiny": scale^2 sum (w s)^2 of the order of eps
DEM_EPS = 1e-8
DEM = [("dem-n%d-co%d-ci%d-kk%d" % (n, co, ci, kk), n, co, ci, kk, 1.0)
       for i, (ci, kk) in enumerate(((1, 1), (3, 9), (16, 16), (29, 9))) for n, co in (((1, 5), (3, 1))[i % 2], ((3, 5), (1, 1))[i % 2])]
DEM += [("dem-eps-matters", 3, 5, 3, 9, 1e-4)]
MODW = [(r[0].replace("dem-", "modw-") + ("-t" if t else ""), r[2], r[3], r[4], t, r[5]) for r in DEM for t in (0, 1)]                   # (id, Cout, Cin, KK, transpose, mag)
MODWB = [(r[0].replace("modw-", "modwb-") + ("-acc" if (i // 2) % 2 else ""), r[1], r[2], r[3], r[4], (i // 2) % 2, r[5]) for i, r in enumerate(MODW)]
DEM_INSTANCE, MODW_INSTANCE, MODWB_INSTANCE = "demod_kernel", "modw_kernel", "modw_bwd_kernel"


def mod_scale(cin, kk):
    return 1.0 / math.sqrt(cin * kk)


def dem_inputs(row):
    """(w [Cout, Cin, KK], s [N, Cin])"""
    rid, n, co, ci, kk, mag = row
    return U((co, ci, kk), 7790, "w%d-%d-%d" % (co, ci, kk)) * mag, 1.0 + 0.5 * U((n, ci), 7790, "s%d-%d" % (n, ci))


def modw_inputs(row):
    """(w, g in wout's layout, seeded dw)"""
    rid, co, ci, kk, t, mag = row[0], row[1], row[2], row[3], row[4], row[-1]
    gshape = (ci, co, kk) if t else (co, ci, kk)
    return U((co, ci, kk), 7790, "w%d-%d-%d" % (co, ci, kk)) * mag, U(gshape, 7791, rid + "g"), U((co, ci, kk), 7791, rid + "dw")


# ---------------------------------------------------------------------------------------------------------------- modconv: demod backward
# (id, N, Cout, Cin, KK, accumulate_dw, accumulate_ds): the ds kernel tiles 256 / KK input channels per workgroup
DMB = [("dmb-n%d-co%d-ci%d-kk%d-dw%d-ds%d" % (n, co, ci, kk, i % 2, (i // 2) % 2), n, co, ci, kk, i % 2, (i // 2) % 2)
       for i, (n, co, ci, kk) in enumerate(((3, 5, 256, 1), (1, 6, 257, 1), (3, 5, 28, 9), (3, 6, 29, 9), (1, 5, 2, 129), (3, 7, 2, 256), (1, 1, 1, 1), (3, 3, 57, 9)))]
DMB_INSTANCE = "demod_bwd_w_kernel+demod_bwd_s_kernel"


def dmb_tile(kk):
    return 256 // kk


def dmb_inputs(row):
    """(dd, d, w, s, seeded dw, seeded ds): d is the demodulation of (w, s)"""
    rid, n, co, ci, kk = row[:5]
    w, s = dem_inputs((rid, n, co, ci, kk, 1.0))
    sc = mod_scale(ci, kk)
    d = (sc * sc * ((w.double()[None] * s.double()[:, None, :, None]) ** 2).sum((2, 3)) + DEM_EPS).rsqrt().float()
    return U((n, co), 7800, rid + "dd"), d, w, s, U(w.shape, 7800, rid + "dw"), U(s.shape, 7800, rid + "ds")


# ---------------------------------------------------------------------------------------------------------------- modconv: scale_dot
# (id, NC, HW, out wanted, pointer off or None, accumulate)
SD_ALPHA = 0.375
SD = [("sd-rows16-vec-hw256", 17, 256, 1, None, 0), ("sd-rows64-vec-hw260", 17, 260, 1, None, 1), ("sd-rows64-vec-hw1024", 5, 1024, 0, None, 0),
      ("sd-rows16-scalar-hw64-a-off", 17, 64, 1, "a", 0), ("sd-rows64-scalar-hw65", 17, 65, 1, None, 1), ("sd-rows16-scalar-hw63", 1, 63, 0, None, 0),
      ("sd-rows16-vec-nc1", 1, 64, 1, None, 1), ("sd-rows64-vec-nc1", 1, 1024, 1, None, 0), ("sd-rows64-scalar-nc1-hw1023", 1, 1023, 1, None, 1),
      ("sd-rows64-scalar-b-off", 17, 256, 1, "b", 0), ("sd-rows64-scalar-out-off", 17, 256, 1, "out", 1), ("sd-rows64-scalar-a-off", 17, 256, 0, "a", 0),
      ("sd-split-vec-s1-hw1028", 3, 1028, 1, None, 0), ("sd-split-scalar-s1-hw1026", 3, 1026, 0, None, 1), ("sd-split-scalar-hw2049", 3, 2049, 1, None, 1),
      ("sd-split-vec-hw4100-nc1", 1, 4100, 1, None, 0), ("sd-split-vec-hw4100-nc1-noout", 1, 4100, 0, None, 1), ("sd-split-scalar-out-off-hw4100", 2, 4100, 1, "out", 0),
      ("sd-split-vec-nc1025-two-chunks", 1025, 4100, 0, None, 1)]         # 2048 / NC workgroups allow 2 chunks where the length asks for 3


def sd_plan(nc, hw):
    """(chunk, chunks per row) of planes of more than 1024 elements"""
    if hw <= 1024:
        return hw, 1
    s = max(min(cdiv(hw, 2048), cdiv(2048, nc)), 1)
    c = cdiv(cdiv(hw, s), 4) * 4
    return c, cdiv(hw, c)


def sd_ws_floats(nc, hw):
    s = sd_plan(nc, hw)[1]
    return nc * s if s > 1 else 0


def sd_instance(row):
    _, nc, hw, out, off, _ = row
    vec = "vec" if hw % 4 == 0 and (off is None or (off == "out" and not out)) else "scalar"
    if hw <= 1024:
        return "scale_dot_rows_kernel<%d,%s>" % (16 if hw <= (256 if vec == "vec" else 64) else 64, vec)
    return "scale_dot_split_kernel<%s>" % vec + ("+scale_dot_finish_kernel" if sd_plan(nc, hw)[1] > 1 else "")


def sd_inputs(row):
    """(a, b [NC, HW], f [NC], seeded dot [NC])"""
    rid, nc, hw = row[:3]
    return U((nc, hw), 7810, rid + "a"), U((nc, hw), 7810, rid + "b"), 1.0 + 0.5 * U((nc,), 7810, rid + "f"), U((nc,), 7810, rid + "dot")


# ---------------------------------------------------------------------------------------------------------------- modconv: transpose
TR = [("tr-co%d-ci%d-kk%d-%s" % (co, ci, kk, "acc" if a else "plain"), co, ci, kk, a) for co, ci, kk in ((1, 1, 1), (5, 3, 9), (3, 29, 9), (2, 16, 16), (65, 5, 1)) for a in (0, 1)]
TR_INSTANCE = "wtranspose_kernel"


def tr_inputs(row):
    """(w [Cout, Cin, KK], seeded out [Cin, Cout, KK]), dyadic: the accumulating add is exact as well"""
    rid, co, ci, kk = row[:4]
    return dyadic((co, ci, kk), 7820, rid + "w"), dyadic((ci, co, kk), 7820, rid + "o")


# ---------------------------------------------------------------------------------------------------------------- the table as a whole
TABLES = {"MOD": MOD, "MODB": MODB, "EVS": EVS, "SN": SN, "SNB": SNB, "ADA": ADA, "SB": SB, "SBB": SBB, "LIN": LIN, "LINB": LINB, "DEM": DEM,
          "MODW": MODW, "MODWB": MODWB, "DMB": DMB, "SD": SD, "TR": TR}


def row_ids():
    return [r[0] for rows in TABLES.values() for r in rows]


def claimed_instances():
    s = {mod_instance(r) for r in MOD} | {modb_instance(r) for r in MODB} | {sn_instance(r) for r in SN} | {linb_instance(r) for r in LINB}
    s |= {sd_instance(r) for r in SD}
    return s | {"spade_eval_stats_kernel", SNB_INSTANCE, "adain_fwd_kernel", "adain_bwd_kernel", SB_INSTANCE, SBB_INSTANCE, LIN_INSTANCE, DEM_INSTANCE,
                MODW_INSTANCE, MODWB_INSTANCE, DMB_INSTANCE, TR_INSTANCE}


def kernels_of(instance):
    """the __global__ kernels an instance string names"""
    return {part.split("<")[0].split(" ")[0] for part in instance.split("+")}
