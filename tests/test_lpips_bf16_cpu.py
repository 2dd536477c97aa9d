"""CPU side of the bf16 LPIPS path (--lpips_dtype bf16): the rounding helper, the float64 restatement the GPU tests judge against, the
seed selection of the whole-term test, and the option."""
import pytest
import torch

from oracle import perceptual as chk
from tests import lpips_bf16_ref as R


def test_rt_bf16_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(20000, generator=g) * torch.exp2(torch.randint(-40, 40, (20000,), generator=g).float()),
                   torch.randn(2000, generator=g) * 2.0 ** -130,                                    # bf16 subnormals
                   torch.tensor([0.0, -0.0, 1.0, 2.0 ** -126, 2.0 ** -133, 2.0 ** -134, 3.0e38])])
    # exact ties: a bf16 value plus half an ulp, on even and odd significands, both signs
    m = torch.arange(128, 256, dtype=torch.float64)
    ties = torch.cat([(m + 0.5) * 2.0 ** e for e in (-20, -7, 0, 9)] + [(torch.arange(0, 64, dtype=torch.float64) + 0.5) * 2.0 ** -133])
    x = torch.cat([x, ties.float(), -ties.float()])
    want = x.to(torch.bfloat16)
    got = R.rt_bf16(x)
    assert got.dtype == x.dtype
    assert torch.equal(got.view(torch.int32), want.float().view(torch.int32))
    # float64 in, no double rounding through fp32: 1 + 2^-8 + 2^-40 lies above the tie and rounds up, its fp32 rounding is the tie itself
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert float(R.rt_bf16(v)) == 1.0 + 2.0 ** -7 and float(v.float().to(torch.bfloat16)) == 1.0
    assert torch.equal(R.rt_bf16(got), got)


def _pair(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(1000 + seed)
    return scale * (2 * torch.rand(shape, generator=g) - 1), scale * (2 * torch.rand(shape, generator=g) - 1)


@pytest.mark.parametrize("shape,scale", [((2, 3, 32, 32), 1.0), ((3, 1, 32, 32), 0.3)])
def test_restatement_without_rounding_is_the_plain_oracle(shape, scale):
    lp = chk.LPIPS(seed=7)
    a, b = _pair(0, shape, scale)
    v, g = R.lpips_run(lp, a, b, 0.7)
    vr, gr = R.oracle_autograd(lp, a, b, 0.7)
    assert abs(v - vr) <= 1e-12 * abs(vr)
    assert R.rel_l2(g, gr) <= 1e-12


def test_ideal_bf16_run_rounds_and_stays_close():
    lp = chk.LPIPS(seed=7)
    a, b = _pair(1, (1, 3, 32, 32))
    v, g = R.lpips_run(lp, a, b, 1.0)
    vq, gq = R.lpips_run(lp, a, b, 1.0, q=R.rt_bf16)
    assert v != vq and 0 < abs(vq - v) / v < 0.05 and 0 < R.rel_l2(gq, g) < 0.2


def test_whole_term_seed_selection():
    """the seed hard-coded in tests/lpips_bf16_ref.py:TERM_CASES: the first of 0 .. 9 whose ideal-run gradient error is within a factor two of
    the median (ReLU-kink flips then do not decide the case), for both shapes of that test"""
    lp = chk.LPIPS(seed=R.NET_SEED)
    for name, case in R.TERM_CASES.items():
        errs = []
        for s in range(10):
            a, b = R.term_inputs(case, s)
            _, g = R.lpips_run(lp, a, b, case["coeff"], channels=case["channels"])
            _, gq = R.lpips_run(lp, a, b, case["coeff"], q=R.rt_bf16, channels=case["channels"])
            errs.append(R.rel_l2(gq, g))
        med = sorted(errs)[len(errs) // 2]
        first = next(s for s, e in enumerate(errs) if med / 2 <= e <= 2 * med)
        assert first == case["seed"], (name, errs, first)


def _opts(extra):
    from options.train_options import TrainOptions

    return TrainOptions(cmd_line="--model sinskitG --gpu_ids -1 --checkpoints_dir /tmp/vts_t --name a " + extra).parse()


def test_option_parses_defaults_and_rejects():
    assert _opts("").lpips_dtype == "fp32"
    assert _opts("--lpips_dtype bf16").lpips_dtype == "bf16"
    assert _opts("--lpips_dtype fp32").lpips_dtype == "fp32"
    with pytest.raises(SystemExit):
        _opts("--lpips_dtype fp16")
    from options.train_options import TrainOptions

    assert TrainOptions(cmd_line="--model skitG --gpu_ids -1 --checkpoints_dir /tmp/vts_t --name a --lpips_dtype bf16").parse().lpips_dtype == "bf16"
