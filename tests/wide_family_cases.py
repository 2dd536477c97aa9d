"""The case table of tests/test_wide_family_gpu.py: the smallest shapes that reach every kernel instance of the GEMM-class "wide" family
(csrc/vts_conv3x3_wide.hip and the Winograd weight gradient of csrc/vts_conv3x3_wino.hip) with every tile dimension ragged.  Plain
data: it imports without a GPU, and tests/test_wide_family_cases.py holds it against the instance names in the sources.

A convolution row is (id, entry, packing mode, (N, A, B, H, W), expected instance, family):
  A / B are the LAUNCH's input / output channels and H x W its grid of output pixels as the dispatch sees it (one parity phase for
  the transposed forms), so an input adjoint is listed with the layer's channels swapped.  entry:
    c3s1   ops.conv3x3_wide        p [N, A, H + 2, W + 2]         -> [N, B, H, W]
    c3s2   ops.conv3x3s2_wide      p [N, A, 2 H + 2, 2 W + 2]     -> [N, B, H, W]
    t3     ops.tconv3x3s2_wide     p [N, A, H + 1, W + 1]         -> [N, B, 2 H, 2 W]
    c4s1 / c4s2   ops.conv4x4_wide p [N, A, s (H - 1) + 4, ...]   -> [N, B, H, W]
    c4t    ops.conv4x4_wide(transposed) p [N, A, OH // 2 + 2, OW // 2 + 2] -> [N, B, OH, OW]; here H x W is the OUTPUT extent OH x OW
  For the four-launch transposed forms the expected instance is the last phase's.
A weight-gradient row is (id, K, stride, (N, Cin, Cout, H, W) with H x W the extent of dout, expected instance, family).

Keep every K_terms of the table (max_k_terms(): now 9 x 132 = 1188) below 2500: the signal of one dropped product is about
2^24 / K^1.5 units of u sqrt(K) absref, still > 100 there, far above any bound C of the GPU test
(tests/test_launch_ref.py::test_wide_judges_catch_one_dropped_product checks it at the table's largest K)."""

CONV = [
    # stride-1 3 x 3
    ("c3s1-flat", "c3s1", "conv_fwd", (3, 12, 8, 5, 7), "conv_flat_kernel<8, 9>", "conv"),                # 3 images per tile, idle lanes, ragged chunk
    ("c3s1-flat-ksplit", "c3s1", "conv_fwd", (9, 132, 68, 4, 4), "conv_flat_kernel<8, 9>+ksplit", "conv"),  # 6 slices, last chunk 4 channels, 8 + 1 images
    ("c3s1-tiled", "c3s1", "conv_fwd", (2, 20, 132, 9, 37), "conv3x3_wide_kernel<1>", "conv"),            # 128 + 4 channels, 2 x 4 + 1 rows, 32 + 5 columns
    ("c3s1-tiled-ksplit", "c3s1", "conv_fwd", (2, 100, 132, 9, 37), "conv3x3_wide_kernel<1>+ksplit", "conv"),   # slices of 5 / 5 / 3 chunks
    ("c3s1-rowrun", "c3s1", "conv_fwd", (1, 16, 8, 5, 65), "conv3x3_rowrun_kernel", "conv"),              # last run of 128 partly outside the map
    ("c3s1-rowrun-ksplit", "c3s1", "conv_fwd", (1, 72, 132, 19, 70), "conv3x3_rowrun_kernel+ksplit", "conv"),
    ("c3s1-wide64", "c3s1", "conv_fwd", (1, 12, 20, 125, 510), "conv3x3_wide64_kernel", "conv"),          # exactly 256 tiles of 8 rows, ragged at 125
    ("c3s1-240-tiles", "c3s1", "conv_fwd", (1, 12, 20, 120, 510), "conv3x3_wide_kernel<1>", "conv"),      # 240 tiles: back on the 128-channel tile
    # their input adjoints (flipped / transposed packing on the gradient padded by 2): channels swapped, grid H + 2 x W + 2
    ("c3s1-adj-flat", "c3s1", "conv_adj", (3, 8, 12, 7, 9), "conv_flat_kernel<8, 9>", "conv"),
    ("c3s1-adj-tiled-ksplit", "c3s1", "conv_adj", (2, 132, 20, 11, 39), "conv3x3_wide_kernel<1>+ksplit", "conv"),
    ("c3s1-adj-rowrun", "c3s1", "conv_adj", (1, 8, 16, 7, 67), "conv3x3_rowrun_kernel", "conv"),
    # stride-2 3 x 3 (the second packing is ConvTranspose2d's input adjoint)
    ("c3s2-tiled", "c3s2", "conv_fwd", (2, 20, 36, 9, 37), "conv3x3_wide_kernel<2>", "conv"),
    ("c3s2-flat", "c3s2", "convT_adj", (3, 20, 12, 5, 6), "conv_flat_kernel<8, 9>", "conv"),
    ("c3s2-flat-ksplit", "c3s2", "conv_fwd", (5, 132, 68, 4, 4), "conv_flat_kernel<8, 9>+ksplit", "conv"),
    # ConvTranspose2d(3, s2, p1, op1) and the stride-2 convolution's input adjoint: four parity-phase launches
    ("t3-phase", "t3", "convT_fwd", (2, 40, 36, 9, 37), "conv_wide_phase_kernel<3>", "convT"),            # 16-channel chunks: 2 x 16 + 8
    ("t3-phase-s2adj", "t3", "conv_s2_adj", (2, 40, 36, 9, 37), "conv_wide_phase_kernel<3>", "convT"),
    ("t3-flat", "t3", "convT_fwd", (3, 20, 12, 5, 6), "conv_flat_kernel<8, 9>", "convT"),                 # output stride 2
    ("t3-flat-ksplit", "t3", "conv_s2_adj", (5, 132, 68, 4, 4), "conv_flat_kernel<8, 9>+ksplit", "convT"),   # strided scatter of the slice reduction
    # 4 x 4, padding 2
    ("c4s1-tiled", "c4s1", "conv_fwd", (1, 12, 36, 10, 38), "conv4x4_wide_kernel<1>", "conv"),
    ("c4s1-tiled-ksplit", "c4s1", "conv_fwd", (1, 40, 132, 10, 38), "conv4x4_wide_kernel<1>+ksplit", "conv"),
    ("c4s1-adj-tiled-ksplit", "c4s1", "conv_adj", (1, 36, 12, 9, 37), "conv4x4_wide_kernel<1>+ksplit", "conv"),
    ("c4s2-tiled", "c4s2", "conv_fwd", (1, 8, 36, 10, 38), "conv4x4_wide_kernel<2>", "conv"),
    ("c4t-phase", "c4t", "conv_s2_adj", (1, 36, 8, 18, 74), "conv_wide_phase_kernel<4>", "convT"),
    ("c4t-phase-odd", "c4t", "conv_s2_adj", (1, 36, 8, 17, 73), "conv_wide_phase_kernel<4>", "convT"),    # odd extents: the four phases differ in size
    ("c4s2-tiled-ksplit", "c4s2", "conv_fwd", (2, 64, 128, 36, 38), "conv4x4_wide_kernel<2>+ksplit", "conv"),
    ("c4s1-rowrun", "c4s1", "conv_fwd", (1, 12, 8, 6, 67), "conv4x4_rowrun_kernel", "conv"),
    ("c4s1-rowrun-ksplit", "c4s1", "conv_fwd", (1, 36, 132, 20, 71), "conv4x4_rowrun_kernel+ksplit", "conv"),
    ("c4s2-flat-ksplit", "c4s2", "conv_fwd", (3, 70, 5, 3, 3), "conv_flat_kernel<4, 16>+ksplit", "conv"),   # Cout 5: not a multiple of 4
    ("c4t-flat", "c4t", "conv_s2_adj", (3, 5, 70, 4, 5), "conv_flat_kernel<4, 16>", "convT"),             # odd width, Cout 70
]

WGRAD = [
    ("wg3-direct-thin-cin", 3, 1, (2, 36, 132, 9, 37), "wgrad3x3_wide_kernel<1>", "wgrad"),               # Cin < 64
    ("wg3-direct-low-map", 3, 1, (2, 70, 132, 5, 40), "wgrad3x3_wide_kernel<1>", "wgrad"),                # H < 8
    ("wg3-direct-s2", 3, 2, (2, 68, 72, 6, 20), "wgrad3x3_wide_kernel<2>", "wgrad"),
    ("wg3-wino-one-slice", 3, 1, (1, 68, 72, 9, 9), "wgrad3x3_wino_kernel", "wgrad_wino"),                # odd map: last 2 x 2 tile row / column half outside
    ("wg3-wino-slices", 3, 1, (2, 70, 132, 9, 37), "wgrad3x3_wino_kernel", "wgrad_wino"),
    ("wg3-flat-direct", 3, 2, (3, 68, 64, 1, 2), "wgrad3x3_flat_kernel<2>", "wgrad"),                     # one slice: stored straight into dw
    ("wg3-flat-slices", 3, 1, (40, 20, 12, 3, 3), "wgrad3x3_flat_kernel<1>", "wgrad"),
    ("wg3-flat-slices-s2", 3, 2, (32, 64, 68, 2, 2), "wgrad3x3_flat_kernel<2>", "wgrad"),
    ("wg4-s1", 4, 1, (2, 36, 132, 9, 37), "wgrad4x4_wide_kernel<1>", "wgrad"),                            # two half-tap launches, advanced `in`
    ("wg4-s2", 4, 2, (2, 68, 72, 6, 20), "wgrad4x4_wide_kernel<2>", "wgrad"),
]

# padded epilogues (ops.conv3x3_wide_relu_pad / _mask_pad): (id, (N, Cin, Cout, H, W), expected instance)
PADDED = [
    ("pad-tiled", (2, 20, 132, 9, 37), "conv3x3_wide_kernel<1>"),
    ("pad-wide64", (1, 12, 20, 125, 510), "conv3x3_wide64_kernel"),
]
# ... and the shapes those entries must refuse, leaving the output untouched: a flat map, a k-split plan, Cout not a multiple of 4
PADDED_REFUSED = [("flat", (3, 12, 8, 5, 7)), ("ksplit", (2, 100, 132, 9, 37)), ("cout-130", (2, 20, 130, 9, 37))]

# instances judged in float64 elsewhere
COVERED_ELSEWHERE = {
    "conv3x3_wino8_kernel": "tests/test_perceptual_gpu.py::test_winograd_convolution_against_float64_and_the_direct_kernel",
    "zero_border_kernel": "tests/test_perceptual_glue_gpu.py::test_zero_border_owns_the_border_alone",
}


def claimed_instances():
    return set(r[4] for r in CONV) | set(r[4] for r in WGRAD) | set(r[2] for r in PADDED) | set(COVERED_ELSEWHERE)


def max_k_terms():
    """the largest number of products one element of any row sums"""
    taps = {"c3s1": 9, "c3s2": 9, "t3": 4, "c4s1": 16, "c4s2": 16, "c4t": 4}
    k = [r[3][1] * taps[r[1]] for r in CONV] + [r[3][0] * r[3][3] * r[3][4] for r in WGRAD] + [r[1][1] * 9 for r in PADDED]
    return max(k)
