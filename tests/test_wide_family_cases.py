"""Every kernel instance the wide family's dispatch can name (the vts_set_kernel format strings of csrc/vts_conv3x3_wide.hip and
csrc/vts_conv3x3_wino.hip) is claimed by a row of the case table of tests/test_wide_family_gpu.py: a new instance needs a new row."""
import os
import re

import wide_family_cases as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visual-tactile-synthesis_amd", "csrc")


def instance_formats():
    fmts = []
    for name in ("vts_conv3x3_wide.hip", "vts_conv3x3_wino.hip"):
        with open(os.path.join(CSRC, name)) as f:
            src = f.read()
        for call in re.findall(r"\bvts_set_kernel\(([^;]*)\);", src):
            found = re.findall(r'"([^"]*)"', call)
            assert found, call
            fmts += found
    return sorted(set(fmts))


def as_regex(fmt):
    return re.compile("^" + re.escape(fmt).replace("%d", r"\d+") + "$")


def test_the_sources_name_the_instances_this_reads():
    fmts = instance_formats()
    assert len(fmts) >= 14, fmts
    for must in ("conv3x3_wide64_kernel", "conv_flat_kernel<%d, %d>+ksplit", "wgrad3x3_wino_kernel", "wgrad4x4_wide_kernel<%d>"):
        assert must in fmts, fmts


def test_every_instance_format_is_claimed_by_a_case():
    claimed = T.claimed_instances()
    unclaimed = [f for f in instance_formats() if not any(as_regex(f).match(c) for c in claimed)]
    assert not unclaimed, "kernel instances without a row in tests/wide_family_cases.py: %s" % unclaimed


def test_every_case_names_an_instance_the_sources_can_produce():
    regs = [as_regex(f) for f in instance_formats()]
    unknown = [c for c in T.claimed_instances() if not any(r.match(c) for r in regs)]
    assert not unknown, unknown


def test_every_template_argument_the_dispatch_passes_is_claimed():
    """<1> and <2>, <3> and <4>, <8, 9> and <4, 16>, with and without +ksplit: the instantiations, not only the format"""
    want = ["conv3x3_wide_kernel<1>", "conv3x3_wide_kernel<1>+ksplit", "conv3x3_wide_kernel<2>", "conv3x3_wide64_kernel", "conv3x3_rowrun_kernel",
            "conv3x3_rowrun_kernel+ksplit", "conv_wide_phase_kernel<3>", "conv_wide_phase_kernel<4>", "conv4x4_wide_kernel<1>",
            "conv4x4_wide_kernel<1>+ksplit", "conv4x4_wide_kernel<2>", "conv4x4_wide_kernel<2>+ksplit", "conv4x4_rowrun_kernel",
            "conv4x4_rowrun_kernel+ksplit", "conv_flat_kernel<8, 9>", "conv_flat_kernel<8, 9>+ksplit", "conv_flat_kernel<4, 16>",
            "conv_flat_kernel<4, 16>+ksplit", "wgrad3x3_wide_kernel<1>", "wgrad3x3_wide_kernel<2>", "wgrad3x3_flat_kernel<1>",
            "wgrad3x3_flat_kernel<2>", "wgrad3x3_wino_kernel", "wgrad4x4_wide_kernel<1>", "wgrad4x4_wide_kernel<2>"]
    missing = [w for w in want if w not in T.claimed_instances()]
    assert not missing, missing


def test_case_ids_are_unique_and_k_stays_small():
    ids = [r[0] for r in T.CONV + T.WGRAD + T.PADDED]
    assert len(ids) == len(set(ids))
    assert T.max_k_terms() <= 2500
