"""The case table of tests/test_step_glue_gpu.py: the smallest shapes at which each kernel of csrc/vts_ops.hip (loss, optimiser, AvgPool
pyramid, patches, generator post-processing, DiffAugment, input staging, the "more fake T" sampler, step_begin) can still go wrong, and the
deterministic inputs (oracle.detrand) of the rows whose formulas have kinks.  Plain data and CPU tensors: it imports without a GPU, and
tests/test_step_glue_cases.py holds it against the kernel and instance names in the source and checks the kink margin of every row.

Kinks: the hinge (1 -+ p = 0), |p| of the BCE forms, the sign of a - b in L1, M > 0 of the candidate map.  Apart from the deliberate exact
ties (hinge t == 0, lsgan p == label, a == b on a stretch, M == 0) no element lies within KINK of one: away() moves the draws that do."""
import torch

from oracle import detrand

KINK = 1e-3
R4, PLAIN = "avgpool_rows4_kernel", "avgpool_kernel"


def away(v, k, margin=2 * KINK):
    """v with the elements closer than `margin` to the kink k moved to k +- 1.5 margin"""
    d = v - k
    return torch.where(d.abs() < margin, k + torch.where(d >= 0, 1.5 * margin, -1.5 * margin), v).float()


# ---- AvgPool2d(3, 2, 1): N = 2, C = 3.  (id, H, W, source layout, expected instance).  Every source has a batch stride larger than the
# operand (NaN between the samples): "pad2" / "pad3" = 3 H W + 2 | 3, "odd" = 3 H W + 1 (an odd batch stride: no 8-byte rows),
# "slice7" = channels 1:4 of a 7-channel stack whose base is 4 bytes off an 8-byte boundary
AVGPOOL = [
    ("r4-1x4", 1, 4, "pad2", R4), ("r4-2x4", 2, 4, "pad2", R4),
    ("r4-17x130", 17, 130, "pad2", R4),          # OW = 65: lane 0 of the second 64-lane block fetches its left neighbour from memory
    ("r4-65x6", 65, 6, "pad2", R4),              # OH = 33: three row groups, the last one ragged
    ("r4-33x46", 33, 46, "pad2", R4),
    ("pl-1x1", 1, 1, "pad3", PLAIN), ("pl-2x2", 2, 2, "pad2", PLAIN), ("pl-5x7", 5, 7, "pad3", PLAIN),
    ("pl-66x130-slice7", 66, 130, "slice7", PLAIN),
    ("pl-6x8-odd-stride", 6, 8, "odd", PLAIN),
]
# adjoint and the fused g_out_grad_pool: (H, W); dx is channels 2:5 of a 7-channel stack.  (1, 1): the adjoint only
POOL_BWD = [(1, 1), (2, 2), (5, 4), (33, 130), (66, 65)]

# ---- GAN loss: all six kernel modes x real / fake x totals; (N, M) of the call
GAN_MODE_NAMES = {0: "nonsaturating", 1: "lsgan", 2: "vanilla", 3: "wgan", 4: "hinge", 5: "vanilla_sigmoid"}
GAN_TOTALS = [(1, 1), (1, 255), (1, 257), (3, 35 * 35), (1, 65536 + 257)]       # the last: the 256-workgroup grid strides a second time
GAN_COEFF, GAN_GCOEFF = 2.5, -0.75
GAN_SEEDS = [0, int(3.25 * 2 ** 40) + 12345, -int(1.5 * 2 ** 40) - 7]            # slot start values


def gan_rows():
    """(id, mode, real, N, M, label, variant, slot seed); variant: 'both', 'nograd' (dpred NULL), 'noloss' (loss NULL)"""
    rows = []
    for mode in range(6):
        for real in (True, False):
            for ti, (n, m) in enumerate(GAN_TOTALS):
                k = mode * 2 + int(real) + ti
                rows.append(("gan-%s-%s-%d" % (GAN_MODE_NAMES[mode], "real" if real else "fake", n * m), mode, real, n, m,
                             0.8 if real else 0.1, ("both", "nograd", "noloss", "both")[k % 4], GAN_SEEDS[k % 3]))
    return rows


def gan_label(row):
    return float(torch.tensor(row[5], dtype=torch.float32))


def gan_pred(row):
    """predictions in +-6 with +-25 (softplus threshold) and +-45 (sigmoid tails) planted; wgan: shifted so that the real row's total is
    negative; hinge: away from the kink with two exact ties t == 0; lsgan: two exact ties p == label; vanilla: away from |p| = 0"""
    _, mode, real, n, m, _, _, _ = row
    total = n * m
    p = detrand.uniform((total,), 2000 + mode, "p%d%d" % (real, total)) * 6
    if mode == 3:
        p = p + 2.0
    if total >= 8:
        p[1], p[2], p[5], p[6] = 25.0, -25.0, 45.0, -45.0
    kink = {4: 1.0 if real else -1.0, 2: 0.0}.get(mode)
    if kink is not None:
        p = away(p, kink)
    if total >= 255:
        if mode == 4:
            p[17], p[total - 3] = kink, kink
        if mode == 1:
            p[17], p[total - 3] = gan_label(row), gan_label(row)
    return p.float().view(n, m)


def gan_workgroups(total):
    return min((total + 255) // 256, 256)


def gan_kink_distance(row):
    """(distance of every element from the row's kink, mask of the planted exact ties), None for a smooth mode"""
    mode, real = row[1], row[2]
    if mode not in (2, 4):
        return None
    p = gan_pred(row).reshape(-1).double()
    d = (p - ({4: 1.0 if real else -1.0, 2: 0.0}[mode])).abs()
    tie = torch.zeros_like(d, dtype=torch.bool)
    if mode == 4 and p.numel() >= 255:
        tie[17], tie[p.numel() - 3] = True, True
    return d, tie


# ---- L1: (id, n, b offset in floats, expected vec)
L1 = [
    ("l1-vec-4", 4, 0, 1), ("l1-vec-1024", 1024, 0, 1), ("l1-vec-second-sweep", 4 * (262144 + 3), 0, 1),
    ("l1-1", 1, 0, 0), ("l1-1938", 1938, 0, 0), ("l1-262147", 262147, 0, 0), ("l1-1024-b-off-1", 1024, 1, 0),
]
L1_TIES = (100, 137)         # a == b exactly on [100, 137) of the rows with n >= 1024


def l1_inputs(row):
    n = row[1]
    a, b = detrand.uniform((n,), 2100, "a%d" % n), detrand.uniform((n,), 2100, "b%d" % n)
    d = a - b
    a = torch.where(d.abs() < 4 * KINK, b + torch.where(d >= 0, 6 * KINK, -6 * KINK), a).float()
    if n >= 1024:
        a[L1_TIES[0]:L1_TIES[1]] = b[L1_TIES[0]:L1_TIES[1]]
    return a, b, detrand.uniform((n,), 2100, "g%d" % n)


def l1_workgroups(n, vec):
    return min(((n // 4 if vec else n) + 255) // 256, 1024)


def l1_kink_distance(row):
    a, b, _ = l1_inputs(row)
    d = (a.double() - b.double()).abs()
    tie = torch.zeros_like(d, dtype=torch.bool)
    if row[1] >= 1024:
        tie[L1_TIES[0]:L1_TIES[1]] = True
    return d, tie


# ---- Adam: (id, n, step, (beta1, beta2), grad_scale); both forms run every row
ADAM = [("adam-%d-s%d-b%d-gs%d" % (n, s, bi, gi), n, s, b, gs)
        for n in (1, 1000, 262147) for s in (1, 2, 1000) for bi, b in enumerate([(0.0, 0.99), (0.5, 0.999)]) for gi, gs in enumerate([1.0, 0.125])]
ADAM_LR, ADAM_EPS = 1e-3, 1e-8


def adam_inputs(row):
    """p alternates O(1) and O(1e-3) (a wrong update shows against the final subtraction's rounding); |g| spans 1e-8 .. 1e2 with exact
    zeros at every 7th element, where m = v = 0 too; m = v = 0 everywhere at step 1"""
    _, n, step, _, _ = row
    i = torch.arange(n)
    p = detrand.uniform((n,), 2200, "p") * torch.where(i % 2 == 0, 1.0, 1e-3)
    scale = 10.0 ** ((i % 11) - 8).float()
    g = detrand.uniform((n,), 2200, "g") * scale
    m, v = detrand.uniform((n,), 2200, "m") * scale, (detrand.uniform((n,), 2200, "v") * scale) ** 2
    if n > 1:
        zero = i % 7 == 0
        g[zero], m[zero], v[zero] = 0.0, 0.0, 0.0
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    return p.float(), g.float(), m.float(), v.float()


# ---- patches
def patch_offsets(h, w, size, count, seed):
    """(offx, offy) int32 [count]: fully inside, clamped on each border, entirely outside the image, a duplicate, then draws over the
    whole range (size beyond the image on every side)"""
    fixed = [(3, 4), (-(size // 2), 5), (w - size // 2, 7), (6, -(size // 2)), (6, h - size // 2), (-size - 3, 2), (w + 5, h + 9), (3, 4)]
    ux, uy = detrand.uniform((count,), seed, "ox"), detrand.uniform((count,), seed, "oy")
    offs = [fixed[i] if i < len(fixed) else (int(ux[i] * (w + size) / 2 + (w - size) / 2), int(uy[i] * (h + size) / 2 + (h - size) / 2))
            for i in range(count)]
    return torch.tensor([o[0] for o in offs], dtype=torch.int32), torch.tensor([o[1] for o in offs], dtype=torch.int32)


# gather: (id, size, H, W).  N = 2 images, C = 2 channels read as channels 1:3 of a 4-channel source, written to channels 2:4 of 5
GATHER = [("gather-32-70x90", 32, 70, 90), ("gather-5-70x90", 5, 70, 90), ("gather-32-33x31", 32, 33, 31), ("gather-5-33x31", 5, 33, 31)]
# scatter: (id, size, H, W, patches per image); dpatch channels 1:3 of 4 (dp_c0 = 1), dsrc channels 1:3 of a 4-channel tensor (batch stride)
SCATTER = [("scatter-32-70x90-p7", 32, 70, 90, 7), ("scatter-32-33x31-p1", 32, 33, 31, 1), ("scatter-5-33x31-p70", 5, 33, 31, 70),
           ("scatter-5-70x90-p1", 5, 70, 90, 1), ("scatter-32-70x90-p70", 32, 70, 90, 70), ("scatter-5-70x90-p7", 5, 70, 90, 7)]
PATCH_JOBS = [("jobs-1", 1, 32), ("jobs-16", 16, 5), ("jobs-16-32", 16, 32)]        # (id, jobs, size)

# ---- generator post-processing: N = 2.  (id, H, W, variant)
#   stack   fake_T, S, aug_fake_I, M into channels 0:2, 2, 3:6, 6 of one 7-channel stack (batch stride 7 H W), fake_I / fake_N dense
#   stackM  the same without S / stack_S;  dense: vts_g_post, everything contiguous;  nz0: scale_nz = 0 (masked-out pixels: 0 / 1e-12)
#   no-X    output X NULL
G_POST = [(("gpost-%dx%d-%s" % (h, w, v)), h, w, v) for h, w in ((1, 1), (15, 17), (40, 56)) for v in ("stack", "stackM", "dense", "nz0")]
G_POST += [("gpost-15x17-no-%s" % x, 15, 17, "no-" + x) for x in ("fake_I", "fake_T", "fake_N", "aug_fake_I", "stack_S", "stack_M")]

# ---- DiffAugment: N = 2; shapes x channels x letters x mask
DIFFAUG_HW = [(1, 1), (9, 7), (40, 56)]
DIFFAUG_OPS = [(("aug-%s-c%d-%dx%d-%s" % (op, c, h, w, "mask" if mk else "nomask")), op, c, h, w, mk)
               for op in "bscton" for c in (3, 1) for h, w in DIFFAUG_HW for mk in (True, False)]
DIFFAUG_BS = [(("bs-%dx%d-%s" % (h, w, "mask" if mk else "nomask")), h, w, mk) for h, w in DIFFAUG_HW for mk in (True, False)]


def diffaug_ints(op, h, w):
    """per-sample integer draws: 't' one small shift and one that leaves the map entirely; 'o' the lower and the upper clamp"""
    if op == "t":
        return torch.tensor([1, h], dtype=torch.int32), torch.tensor([-1, 0], dtype=torch.int32)
    ch, cw = int(h * 0.5 + 0.5), int(w * 0.5 + 0.5)
    return torch.tensor([0, h - 1 + (1 - ch % 2)], dtype=torch.int32), torch.tensor([0, w - 1 + (1 - cw % 2)], dtype=torch.int32)


# ---- the rest of the float glue
MASK_MUL_HW = [1, 255, 257]                                                          # N = 2, C = 3
SPE = [("spe-d4-w1", 4, 3, 1, 0), ("spe-d4-w256", 4, 2, 256, 0), ("spe-d8-w257-c0", 8, 3, 257, 2), ("spe-d8-w1100", 8, 2, 1100, 0),
       ("spe-d4-w1100-c0", 4, 1, 1100, 1)]                                          # (id, dim, H, W, c0); N = 2
POOL_QUERY = [("pool-1", 1), ("pool-257", 257)]                                      # N = 3 images, 4 slots
POOL_SLOTS = ([-1, 2, 2], [2, 2, -1])          # image 1 draws the slot image 0 has just filled and refills it; image 2 draws that
COPY_WORDS = [1, 1025]
STEP_BEGIN = [(0, 0), (1, 1), (256, 256), (3, 0), (0, 2)]                            # (slots, counters)

# ---- byte staging
U8_EXPAND = [1, 1023, 1024, 1028]
VT, VF = "input_images_u8_kernel<true>", "input_images_u8_kernel<false>"
# (id, HW, variant, expected): variant 'all', 'no-I', 'no-M', 'no-S2', 'off1' (the S plane one byte off a 4-byte boundary)
INPUT_U8 = [("u8in-1", 1, "all", VF), ("u8in-1023", 1023, "all", VF), ("u8in-1024", 1024, "all", VT), ("u8in-1028", 1028, "all", VT),
            ("u8in-1028-no-I", 1028, "no-I", VT), ("u8in-1024-no-M", 1024, "no-M", VT), ("u8in-1023-no-M", 1023, "no-M", VF),
            ("u8in-1028-no-S2", 1028, "no-S2", VT), ("u8in-1023-no-I", 1023, "no-I", VF), ("u8in-1024-off1", 1024, "off1", VF)]

# ---- the "more fake T" sampler: (id, H, W, mask pattern, K); N = 2
MASKS = [("mask-15x15-corners-k1", 15, 15, "corners", 1), ("mask-15x15-corners-k65", 15, 15, "corners", 65),      # c = 1 < K: ranks wrap
         ("mask-46x47-borders-k65", 46, 47, "borders", 65),
         ("mask-80x96-empty-full-k1024", 80, 96, "empty-full", 1024), ("mask-143x79-corners-k65", 143, 79, "corners", 65),
         ("mask-143x79-borders-k1", 143, 79, "borders", 1), ("mask-46x47-empty-full-k65", 46, 47, "empty-full", 65),
         ("mask-15x15-empty-full-k65", 15, 15, "empty-full", 65)]          # the last: one candidate per image at most, c < K
MASK_SEED = 0x1234ABCD5678


def mask_input(row):
    _, h, w, pattern, _ = row
    m = torch.zeros(2, 1, h, w)
    if pattern == "corners":
        m[0, 0, 0, 0], m[0, 0, h - 1, w - 1] = 1.0, 0.3
        m[1, 0, h // 2:h // 2 + 3, w // 3:w // 3 + 2] = 1.0
        m[1, 0, h // 2 + 1, w // 3] = 0.0
    elif pattern == "borders":
        m[0, 0, :, 0], m[0, 0, 0, :] = 1.0, 0.5
        m[1, 0, h - 1, :], m[1, 0, :, w - 1] = 2.0, 1.0
    else:
        assert pattern == "empty-full"
        m[1] = 1.0
    return m


def mask_kink_distance(row):
    m = mask_input(row).reshape(-1).double()
    return m.abs(), m == 0


def kink_rows():
    """(row id, distances, planted ties) of every row with a kink"""
    out = []
    for row in gan_rows():
        d = gan_kink_distance(row)
        if d is not None:
            out.append((row[0],) + d)
    out += [(row[0],) + l1_kink_distance(row) for row in L1]
    out += [(row[0],) + mask_kink_distance(row) for row in MASKS]
    return out


def claimed_instances():
    """every instance string a row of this table expects vts_last_kernel() to report"""
    c = {r[4] for r in AVGPOOL} | {r[3] for r in INPUT_U8} | {"l1_kernel vec=%d" % r[3] for r in L1}
    c |= {"avgpool_bwd_kernel", "g_out_grad_kernel", "ganloss_kernel", "adam_kernel", "adam_dev_kernel", "patch_gather_kernel",
          "patch_jobs_kernel", "patch_scatter_kernel", "g_post_kernel", "diffaug_kernel", "diffaug_op_kernel",
          "diffaug_mean_part_kernel+diffaug_op_kernel", "mask_mul_kernel", "spe_kernel", "pool_query_kernel", "copy_words_kernel",
          "step_begin_kernel", "u8_expand_kernel", "mask_cand_kernel+mask_rowcount_kernel+mask_prefix_kernel", "mask_select_kernel",
          "mask_sample_ranks_kernel"}
    return c


# kernels of csrc/vts_ops.hip judged elsewhere
COVERED_ELSEWHERE = {"patchnce_kernel": "tests/test_kernels_gpu.py", "l2norm_kernel": "tests/test_kernels_gpu.py"}


def row_ids():
    ids = [r[0] for r in AVGPOOL + gan_rows() + L1 + ADAM + GATHER + SCATTER + PATCH_JOBS + G_POST + DIFFAUG_OPS + DIFFAUG_BS + SPE + POOL_QUERY
           + INPUT_U8 + MASKS]
    return ids

