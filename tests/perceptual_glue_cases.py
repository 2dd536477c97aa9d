"""The case table of tests/test_perceptual_glue_gpu.py: the smallest shapes at which the fp32 glue kernels of the perceptual terms
(csrc/vts_perceptual.hip, and vts_zero_border of csrc/vts_conv3x3_wide.hip) can still go wrong, with the kernel instance each row expects and
its deterministic inputs (oracle.detrand).  Plain data and CPU tensors: it imports without a GPU, and tests/test_perceptual_glue_cases.py
holds it against the kernel and instance names in the sources.

Bitwise rows (pooling, space-to-depth, stacking, masks, the pooling adjoint): inputs on a dyadic grid, multiples of 2^-10 in [-4, 4] without
negative zeros apart from the planted ones, so the one fp32 add of two of them is exact.  Arithmetic rows: uniform draws; the feature maps of
the LPIPS head and the operands of the ReLU-L1 keep 2 KINK away from their kink (z = 0, relu(za) = relu(zb)) apart from the planted exact
zeros / ties.  Exact-sum rows (more than 1024 addends in a loss slot): operands whose partial sums are all exact in fp32.

Every input is the DENSE interior; the GPU test lays it out (zpad borders, batch strides, guard bands)."""
import torch

from oracle import detrand
from step_glue_cases import GAN_SEEDS, KINK  # noqa: F401

NCR = 11                      # planes of an ordinary row: enough for every planted pattern at one window per plane
CHUNK = 65537                 # planes of a chunk-loop row: the entries launch 65535 planes at a time
SWEEP = 2048 * 256            # blocks_1d caps the grid at 2048 workgroups of 256: beyond it a thread sweeps a second time
GRID = 2.0 ** -10


def dyadic(shape, seed, name, nonzero=False):
    """multiples of 2^-10 in [-4, 4], no negative zero; nonzero: exact zeros moved to 2^-10"""
    v = torch.round(detrand.uniform(shape, seed, name) * 4096) / 1024 + 0.0
    return torch.where(v == 0, torch.full_like(v, GRID), v) if nonzero else v


def is_dyadic(t):
    s = t * 1024
    return bool(torch.equal(s, torch.round(s))) and float(t.abs().max()) <= 4.0


# ---- vts_maxpool2_relu_pad (id, NC, H, W, pad, zpad) / vts_maxpool3s2_relu_pad (id, NC, H, W, pad)
MP2 = [("mp2-%dx%d-p%d-z%d" % (h, w, p, zp), NCR, h, w, p, zp)
       for h, w in ((2, 2), (2, 3), (3, 2), (5, 7), (8, 12), (34, 66)) for p in (0, 1) for zp in (0, 1, 2)]
MP2 += [("mp2-chunk-loop", CHUNK, 2, 2, 1, 1),
        ("mp2-second-sweep", 1, 1452, 1452, 1, 0)]            # padded output 728 x 728 > 2048 * 256
MP3 = [("mp3-%dx%d-p%d" % (h, w, p), NCR, h, w, p) for h, w in ((3, 3), (4, 5), (7, 6), (13, 13), (55, 55)) for p in (0, 1, 2)]
MP3 += [("mp3-chunk-loop", CHUNK, 3, 3, 1)]


def pool_input(row, k):
    """z [NC, H, W] with one k x k window of equal positive values (plane 0, window (0, 0)) and one all-negative window (the last plane's
    window (0, 0); with one plane: window (0, 2))"""
    rid, nc, h, w = row[:4]
    z = dyadic((nc, h, w), 7000, rid)
    z[0, 0:k, 0:k] = 0.375
    if nc > 1:
        z[nc - 1, 0:k, 0:k] = (-z[nc - 1, 0:k, 0:k].abs() - GRID).clamp_min(-4.0)
    else:
        z[0, 0:k, 4:4 + k] = (-z[0, 0:k, 4:4 + k].abs() - GRID).clamp_min(-4.0)
    return z


# ---- vts_s2d4_pad (id, N, C, H, W, pad, OH, OW): the stem's own OH = (H + 2 pad - 11) / 4 + 3
def stem_out(h):
    return (h + 4 - 11) // 4 + 3


S2D = [("s2d-c%d-%dx%d" % (c, h, w), 2, c, h, w, 2, stem_out(h), stem_out(w)) for c in (1, 3) for h, w in ((11, 11), (31, 35), (64, 64))]
S2D += [("s2d-beyond-the-padded-image", 2, 3, 11, 11, 2, 6, 7)]      # 4 OH = 24 > H + 2 pad = 15: zeros beyond

# ---- vts_maxpool2_relu_bwd (id, NC, H, W, pad, zpad, tap, instance)
WIN, ELEM = "maxpool2_relu_bwd_win_kernel", "maxpool2_relu_bwd_kernel"
MPB = [("mpb-%dx%d-p%d-z%d-%s" % (h, w, p, zp, "tap" if t else "notap"), NCR, h, w, p, zp, t, WIN if h % 2 == 0 and w % 2 == 0 else ELEM)
       for h, w in ((2, 2), (2, 10), (10, 2), (6, 6), (32, 32), (5, 7), (2, 3), (3, 2)) for p in (0, 1, 2) for zp in (0, 1, 2) for t in (True, False)]
MPB += [("mpb-chunk-loop", CHUNK, 2, 2, 1, 2, True, WIN)]
# planted patterns, by window index (plane-major) modulo 10: the positions (row-major in the window) that share the window's maximum;
# 7: an all-nonpositive window holding 0.0 and -0.0; 8, 9: untouched
PATTERNS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1, 2, 3)]


def mpb_inputs(row):
    """(g [NC, OH, OW], z [NC, H, W], tap [NC, H, W] or None, pattern index of every window [NC, OH, OW])"""
    rid, nc, h, w, _, _, tap, _ = row
    oh, ow = h // 2, w // 2
    z = dyadic((nc, h, w), 7100, rid)
    e = z[:, :2 * oh, :2 * ow].reshape(nc, oh, 2, ow, 2).permute(0, 1, 3, 2, 4).reshape(nc, oh, ow, 4).clone()
    pat = (torch.arange(nc * oh * ow) % 10).view(nc, oh, ow)
    m = e.max(-1).values
    m = torch.where(m > 0, m, torch.full_like(m, 0.5))
    for i, pos in enumerate(PATTERNS):
        sel = pat == i
        for k in range(4):
            v = m if k in pos else torch.where(e[..., k] >= m, m - GRID, e[..., k])
            e[..., k] = torch.where(sel, v, e[..., k])
    sel = pat == 7
    low = (-e.abs() - GRID).clamp_min(-4.0)
    for k, v in enumerate((torch.zeros_like(m), -torch.zeros_like(m), low[..., 2], low[..., 3])):
        e[..., k] = torch.where(sel, v, e[..., k])
    z[:, :2 * oh, :2 * ow] = e.reshape(nc, oh, ow, 2, 2).permute(0, 1, 3, 2, 4).reshape(nc, 2 * oh, 2 * ow)
    g = dyadic((nc, oh, ow), 7100, rid + "g", nonzero=True)
    t = dyadic((nc, h, w), 7100, rid + "tap", nonzero=True) if tap else None
    return g, z, t, pat


# ---- vts_relu_mask_pad (id, NC, H, W, pad, zpad, variant): 'g' (dense gradient only), 'g2' (tap gradient only), 'both'
RMP = [("rmp-%dx%d-p%d-z%d-%s" % (h, w, p, zp, v), NCR, h, w, p, zp, v)
       for h, w in ((1, 1), (9, 11), (32, 32)) for p in (0, 1, 2) for zp in (0, 1, 2) for v in ("g", "g2", "both")]
RMP += [("rmp-chunk-loop", CHUNK, 2, 2, 1, 1, "both")]


def rmp_inputs(row):
    """(g or None, g2 or None, z): z has 0.0 at every 7th element and -0.0 three after it"""
    rid, nc, h, w, _, _, v = row
    z = dyadic((nc, h, w), 7200, rid, nonzero=True)
    z.view(-1)[0::7] = 0.0
    z.view(-1)[3::7] = -0.0
    g = dyadic((nc, h, w), 7200, rid + "g", nonzero=True) if v in ("g", "both") else None
    g2 = dyadic((nc, h, w), 7200, rid + "g2", nonzero=True) if v in ("g2", "both") else None
    return g, g2, z


# ---- vts_zero_border (id, NC, H, W, pad)
ZB = [("zb-%dx%d-p%d" % (h, w, p), NCR, h, w, p) for h, w in ((1, 1), (5, 7)) for p in (1, 2, 8)]
ZB += [("zb-stride-600x600-p8", 1, 600, 600, 8),             # 2 * 8 * (616 + 600) = 19456 border elements > 64 * 256
       ("zb-chunk-loop", CHUNK, 1, 1, 1)]


def zb_input(row):
    """the buffer before the call: a dyadic interior inside a NaN border"""
    rid, nc, h, w, p = row
    buf = torch.full((nc, h + 2 * p, w + 2 * p), float("nan"))
    buf[:, p:p + h, p:p + w] = dyadic((nc, h, w), 7300, rid)
    return buf


# ---- vts_lpips_layer (id, N, C, H, W, zpad, variant, slot seed, instance, exact)
LPL_C = (1, 5, 96, 64, 128, 256, 512)
LPL_HW = ((1, 1), (2, 2), (7, 9), (8, 8), (5, 13), (10, 13))
LPL_INSTANCE = {64: "lpips_layer_regs_kernel<16,4>", 128: "lpips_layer_regs_kernel<32,4>", 256: "lpips_layer_regs_kernel<64,4>",
                512: "lpips_layer_regs_kernel<64,8>"}
GENERIC = "lpips_layer_kernel"
VARIANTS = ("both", "nograd", "noloss")
LPL = []
for _ci, _c in enumerate(LPL_C):
    for _hi, (_h, _w) in enumerate(LPL_HW):
        LPL.append(("lpl-c%d-%dx%d" % (_c, _h, _w), (1, 3)[(_ci + _hi) % 2], _c, _h, _w, (_ci + _hi) % 3, VARIANTS[(_hi + _hi // 3 + _ci) % 3],
                    GAN_SEEDS[(_ci + 2 * _hi) % 3], LPL_INSTANCE.get(_c, GENERIC), False))
LPL += [("lpl-exact-second-sweep", 1, 3, 1, SWEEP + 257, 0, "both", GAN_SEEDS[1], GENERIC, True)]
LPL_COEFF, LPL_GCOEFF = 0.3, -0.7
LPL_EXACT_W, LPL_EXACT_COEFF = (0.25, 0.5, 0.125), 2.0 ** -4


def lpl_workgroups(row):
    _, n, c, h, w = row[:5]
    return n * ((h * w + 63) // 64) if c in LPL_INSTANCE else n * min((h * w + 255) // 256, 2048)


def lpl_coeffs(row):
    return (LPL_EXACT_COEFF, 0.5) if row[9] else (LPL_COEFF, LPL_GCOEFF)


def lpl_inputs(row):
    """(z0, z1 [N, C, H, W], w [C], planted [N, H, W]: 1 all of f0 zero, 2 all of f1 zero, 3 both).  zpad = 0: raw convolution outputs
    (negatives: ReLU on load); zpad > 0: the ReLU'd values the padded layout holds (exact zeros).  Exact rows: one-hot pixels."""
    rid, n, c, h, w, zpad, _, _, _, exact = row
    if exact:
        hot0 = (detrand.uniform((n, 1, h, w), 7400, rid + "a") * 1.5 + 1.5).long().clamp(0, 2)
        hot1 = (detrand.uniform((n, 1, h, w), 7400, rid + "b") * 1.5 + 1.5).long().clamp(0, 2)
        z0 = torch.zeros(n, 3, h, w).scatter_(1, hot0, 1.0)
        z1 = torch.full((n, 3, h, w), -1.0).scatter_(1, hot1, 1.0)          # raw negatives beside the hot channel
        return z0, z1, torch.tensor(LPL_EXACT_W), torch.zeros(n, h, w, dtype=torch.long)
    zs = []
    for name in ("z0", "z1"):
        z = detrand.uniform((n, c, h, w), 7400, rid + name) * 2
        zs.append(torch.where(z.abs() < 2 * KINK, torch.where(z >= 0, 3 * KINK, -3 * KINK), z).float())
    z0, z1 = zs
    planted = torch.zeros(n * h * w, dtype=torch.long)
    if n * h * w >= 4:
        planted[0], planted[1], planted[2] = 1, 2, 3
    planted = planted.view(n, h, w)
    dead0, dead1 = (planted == 1) | (planted == 3), (planted == 2) | (planted == 3)
    z0 = torch.where(dead0.unsqueeze(1), -z0.abs(), z0)
    z1 = torch.where(dead1.unsqueeze(1), -z1.abs(), z1)
    if zpad:
        z0, z1 = z0.clamp_min(0.0), z1.clamp_min(0.0)
    wl = (detrand.uniform((c,), 7400, rid + "w") + 1.02) * 0.05
    return z0, z1, wl.float(), planted


# ---- vts_l1_relu (id, n, variant, slot seed, exact)
L1R = [("l1r-1", 1, "both", GAN_SEEDS[0], False), ("l1r-255-both", 255, "both", GAN_SEEDS[1], False),
       ("l1r-255-nograd", 255, "nograd", GAN_SEEDS[2], False), ("l1r-255-noloss", 255, "noloss", GAN_SEEDS[0], False),
       ("l1r-1025-exact", 1025, "both", GAN_SEEDS[2], True),                    # two workgroups; more than 1024 addends
       ("l1r-exact-second-sweep", 4 * SWEEP + 1027, "both", GAN_SEEDS[1], True)]
L1R_TIES, L1R_NEG = (100, 137), (140, 170)        # za == zb, and both negative, on these stretches of the rows with n >= 255


def l1r_workgroups(n):
    return min((n // 4 + 1 + 255) // 256, 2048)


def l1r_coeff(row):
    return float(torch.tensor(0.7 / row[1], dtype=torch.float32))


def l1r_inputs(row):
    """(za, zb, ties: relu(za) == relu(zb) exactly)"""
    rid, n, _, _, exact = row
    za, zb = detrand.uniform((n,), 7500, rid + "a") * 2, detrand.uniform((n,), 7500, rid + "b") * 2
    if exact:
        za, zb = torch.round(za * 2) / 64, torch.round(zb * 2) / 64          # |d| <= 4 / 64: n of them sum exactly below 2^24 / 64
    else:
        fb = zb.clamp_min(0.0)
        near = ((za.clamp_min(0.0) - fb).abs() < 4 * KINK) & ((za > 0) | (zb > 0))
        za = torch.where(near, fb + 6 * KINK, za).float()
    if n >= 255:
        za[L1R_TIES[0]:L1R_TIES[1]] = zb[L1R_TIES[0]:L1R_TIES[1]]
        za[L1R_NEG[0]:L1R_NEG[1]] = -za[L1R_NEG[0]:L1R_NEG[1]].abs() - 0.25
        zb[L1R_NEG[0]:L1R_NEG[1]] = -zb[L1R_NEG[0]:L1R_NEG[1]].abs() - 0.25
    return za, zb, za.clamp_min(0.0) == zb.clamp_min(0.0)


# ---- vts_lpips_input / vts_lpips_input_bwd (id, N, Cx, HW, layout): 'slice' = channels 1 : 1 + Cx of a (Cx + 2)-channel stack
LPIPS_SHIFT, LPIPS_SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
LIN = [("lin-c%d-hw%d-%s" % (cx, hw, lay), 2, cx, hw, lay) for cx in (1, 3) for i, hw in enumerate((1, 255, 257))
       for lay in (("dense", "slice") if hw == 255 else (("slice", "dense")[(i + cx) % 2],))]
LIN += [("lin-c1-second-sweep", 1, 1, SWEEP + 3, "dense"), ("lin-c3-second-sweep", 1, 3, SWEEP + 3, "slice")]


def lin_inputs(row):
    """(x, g [N, 3, HW], dx seed)"""
    rid, n, cx, hw, _ = row
    return detrand.uniform((n, cx, hw), 7600, rid), detrand.uniform((n, 3, hw), 7600, rid + "g"), detrand.uniform((n, cx, hw), 7600, rid + "seed")


# ---- vts_vgg_stack_input (id, N, H, W) / vts_vgg_stack_input_bwd (id, N, H, W, why, instance)
VSI = [("vsi-n%d-%dx%d" % (n, h, w), n, h, w) for n in (1, 2) for h, w in ((1, 1), (5, 7), (32, 32))]
V4, V1 = "vgg_stack_input_bwd_kernel<4>", "vgg_stack_input_bwd_kernel<1>"
VSB = [("vsb-v4-8x8", 2, 8, 8, "v4", V4), ("vsb-hw-5x7", 2, 5, 7, "hw", V1), ("vsb-stride-8x8", 2, 8, 8, "stride", V1),
       ("vsb-offset-8x8", 2, 8, 8, "offset", V1)]


def vsb_layout(row):
    """(d_fake_I batch stride, d_fake_T batch stride, element offset of d_fake_T's base): gaps behind every sample; exactly one of the
    three conditions of the float4 instance fails on a <1> row"""
    _, _, h, w, why, _ = row
    hw = h * w
    return (3 * hw + 7) // 4 * 4 + (2 if why == "stride" else 0), (2 * hw + 7) // 4 * 4, 1 if why == "offset" else 0


def vsb_conditions(row):
    """the conditions of the float4 instance that hold: (HW % 4 == 0, both strides % 4 == 0, every base on 16 bytes)"""
    nsI, nsT, off = vsb_layout(row)
    return (row[2] * row[3]) % 4 == 0, nsI % 4 == 0 and nsT % 4 == 0, off % 4 == 0


def vsb_inputs(row):
    """(dx [3 N, 3, HW], seeds of d_fake_I [N, 3, HW] and d_fake_T [N, 2, HW])"""
    rid, n, h, w = row[:4]
    return (detrand.uniform((3 * n, 3, h * w), 7700, rid), detrand.uniform((n, 3, h * w), 7700, rid + "I"),
            detrand.uniform((n, 2, h * w), 7700, rid + "T"))


def claimed_instances():
    """every instance string a row of this table expects vts_last_kernel() to report"""
    c = {r[7] for r in MPB} | {r[8] for r in LPL} | {r[5] for r in VSB}
    c |= {"maxpool2_relu_pad_kernel", "maxpool3s2_relu_pad_kernel", "s2d4_pad_kernel", "relu_mask_pad_kernel", "zero_border_kernel",
          "l1_relu_kernel", "lpips_input_kernel", "lpips_input_bwd_kernel", "vgg_stack_input_kernel"}
    return c


def kernels_of(instance):
    """the __global__ kernel an instance string names: 'lpips_layer_regs_kernel<16,4>'"""
    return instance.split("<")[0]


def row_ids():
    return [r[0] for r in MP2 + MP3 + S2D + MPB + RMP + ZB + LPL + L1R + LIN + VSI + VSB]
