"""vts_frechet_distance_batched / vts_tfid_features / engine.tactile_patch_fid on the GPU.

Yardstick: the REFERENCE's calculate_frechet_distance and TactilePatchFID on the seeded inputs of tools/make_baseline_metrics_golden.py
(tests/golden/baseline_metrics.npz); where the fixture has no value, the oracle's nets.frechet_distance (scipy, float64, itself pinned to
the reference by tests/golden/metrics.npz).  Tolerance: that of test_frechet_distance_matches_reference, 2e-5 * max(1, |ref|) -- float32
inputs, float64 arithmetic, a float32 result.  Every comparison prints its figure before it asserts (pytest -s)."""
import os

import numpy as np
import pytest
import torch

from oracle import nets
from tools import make_baseline_metrics_golden as T

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_metrics.npz")
DEV = "cuda"
TOL = 2e-5


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN, allow_pickle=False)


_CASES = {}


def case(i, seed):
    """(f1, f2) on the host, drawn once per case and shared by the tests"""
    if i not in _CASES:
        _CASES[i] = T.fd_case(i, seed)
    return _CASES[i]


def check(got, ref, what):
    err = abs(got - ref) / max(1.0, abs(ref))
    print("%s: got %.8f reference %.8f, error / max(1, |ref|) %.2e (bound %.0e)" % (what, got, ref, err, TOL))
    assert err <= TOL, (what, got, ref)


@pytest.mark.parametrize("i", range(len(T.FD_CASES)))
def test_batched_distance_matches_the_reference(gold, i):
    from vts import ops
    f1, f2 = case(i, int(gold["seed"]))
    assert tuple(f1.shape) == (T.FD_CASES[i][3], T.FD_CASES[i][0], T.FD_CASES[i][1])
    got = ops.frechet_distance_batched(f1.to(DEV), f2.to(DEV)).cpu().tolist()
    for j, (g, r) in enumerate(zip(got, gold["fd/%d" % i].tolist())):
        check(g, r, "case %d %s pair %d" % (i, T.FD_CASES[i], j))
        # the fixture's value and the oracle agree far below the bound, so either serves as the yardstick (1e-7: scipy's Schur-based
        # sqrtm moves by some 1e-9 with the BLAS of the machine it runs on)
        assert abs(nets.frechet_distance(f1[j], f2[j]) - r) <= 1e-7 * max(1.0, abs(r))


def test_pair_strides_with_nan_in_the_gaps(gold):
    """pairs that lie 37 / 5 floats further apart than D * P, the gaps filled with NaN: never read"""
    from vts import ops
    f1, f2 = case(1, int(gold["seed"]))
    n, d, p1 = f1.shape
    p2 = f2.shape[2]
    a = torch.full((n, d * p1 + 37), float("nan"))
    b = torch.full((n, d * p2 + 5), float("nan"))
    a[:, :d * p1] = f1.reshape(n, -1)
    b[:, :d * p2] = f2.reshape(n, -1)
    a, b = a.to(DEV), b.to(DEV)
    va, vb = a[:, :d * p1].view(n, d, p1), b[:, :d * p2].view(n, d, p2)
    assert va.stride(0) == d * p1 + 37 and vb.stride(0) == d * p2 + 5
    got = ops.frechet_distance_batched(va, vb).cpu()
    dense = ops.frechet_distance_batched(f1.to(DEV), f2.to(DEV)).cpu()
    assert torch.isfinite(got).all() and torch.equal(got, dense)
    for j, r in enumerate(gold["fd/1"].tolist()):
        check(float(got[j]), r, "strided pair %d" % j)


def test_a_pair_does_not_depend_on_the_batch_or_its_index_and_repeats_bitwise(gold):
    """cross-pair leakage through LDS or the workspace would show here: pair i alone, in its batch, at another index of a batch padded
    with other pairs, and in a second call -- all bitwise equal"""
    from vts import ops
    for i in (0, 1, 3):
        f1, f2 = (t.to(DEV) for t in case(i, int(gold["seed"])))
        n = f1.shape[0]
        batch = ops.frechet_distance_batched(f1, f2).cpu()
        assert torch.equal(batch, ops.frechet_distance_batched(f1, f2).cpu())
        for j in range(n):
            alone = ops.frechet_distance_batched(f1[j:j + 1].contiguous(), f2[j:j + 1].contiguous()).cpu()
            assert torch.equal(alone[0], batch[j]), (i, j, float(alone[0]), float(batch[j]))
        perm = list(range(1, n)) + [0]
        moved = ops.frechet_distance_batched(f1[perm].contiguous(), f2[perm].contiguous()).cpu()
        assert torch.equal(moved, batch[perm]), (i, moved, batch[perm])
        big = ops.frechet_distance_batched(torch.cat([f1, f1, f1]), torch.cat([f2, f2, f2])).cpu()
        assert torch.equal(big, torch.cat([batch, batch, batch]))


def test_identical_sets_give_zero(gold):
    from vts import ops
    for i in (0, 2, 4):
        f1, _ = case(i, int(gold["seed"]))
        d = ops.frechet_distance_batched(f1.to(DEV), f1.to(DEV)).cpu()
        print("identical sets, case %d: %s" % (i, d.tolist()))
        assert (d.abs() < 1e-4).all(), d


def test_captured_in_a_hip_graph_and_replayed(gold):
    from vts import ops
    f1, f2 = (t.to(DEV) for t in case(0, int(gold["seed"])))
    eager = ops.frechet_distance_batched(f1, f2).clone()        # (also grows the workspace before the capture)
    torch.cuda.synchronize()
    ops.freeze_ws("test_frechet_graph")
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            out = ops.frechet_distance_batched(f1, f2)
        for _ in range(2):
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager), (out, eager)
    finally:
        ops.release_ws("test_frechet_graph")


def test_bad_arguments_are_refused_before_any_launch():
    from vts import lib as L
    lib = L.load()
    assert lib.vts_frechet_batched_ws_floats(0) == 0 and lib.vts_frechet_batched_ws_floats(3) == 3 * lib.vts_frechet_batched_ws_floats(1)
    n = 2
    f = torch.zeros(n, 64, 100, device=DEV)
    ws = torch.zeros(lib.vts_frechet_batched_ws_floats(n) + 2, device=DEV)
    out = torch.full((n,), -7.0, device=DEV)
    st = L.stream()

    def call(f1=f.data_ptr(), f2=f.data_ptr(), D=64, P1=100, P2=100, npairs=n, s1=6400, s2=6400, o=out.data_ptr(), w=ws.data_ptr()):
        return lib.vts_frechet_distance_batched(f1, f2, D, P1, P2, npairs, s1, s2, o, w, st)

    for kw, word in ((dict(D=65), "D <= 64"), (dict(P1=1), "P >= 2"), (dict(P2=1), "P >= 2"), (dict(npairs=0), "npairs"), (dict(f1=None), "bad args"),
                     (dict(o=None), "bad args"), (dict(w=ws.data_ptr() + 4), "8-byte aligned"), (dict(s1=6399), "stride"), (dict(D=0), "bad args")):
        rc = call(**kw)
        msg = lib.vts_last_error().decode()
        assert rc != 0 and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (out == -7.0).all()        # nothing was launched
    assert lib.vts_tfid_features(None, 1, 8, 8, 0, out.data_ptr(), st) != 0 and "vts_tfid_features" in lib.vts_last_error().decode()
    assert lib.vts_tfid_features(f.data_ptr(), 1, 2, 8, 0, out.data_ptr(), st) != 0


def crops_numpy(x):
    """the 3 x 3 valid crops of one patch x [C, H, W] as the reference's Im2col orders them (models/tactile_patch_fid.py:88-100): row
    c * 9 + fh * 3 + fw holds x[c, fh:fh + H - 2, fw:fw + W - 2] flattened row-major"""
    c, h, w = x.shape
    return np.stack([x[ch, fh:fh + h - 2, fw:fw + w - 2].reshape(-1) for ch in range(c) for fh in range(3) for fw in range(3)])


def tfid_inputs(seed):
    _, _, real_T, fake_T = T.metric_batch(seed)
    return (real_T, fake_T), T.tfid_nonsquare(seed)


def test_tfid_features_are_im2col_exactly(gold):
    from vts import ops
    for real, fake in tfid_inputs(int(gold["seed"])):
        for src, clamp in ((real, False), (fake, False), (fake, True)):
            got = ops.tfid_features(src.to(DEV), clamp01=clamp).cpu().numpy()
            x = torch.clamp(src, 0, 1) if clamp else src
            want = np.hstack([crops_numpy(p) for p in x.numpy()])
            assert got.shape == want.shape == (18, src.shape[0] * (src.shape[2] - 2) * (src.shape[3] - 2))
            assert np.array_equal(got, want), (tuple(src.shape), clamp)


def test_tfid_matches_the_reference_in_both_reductions(gold):
    from vts import engine
    (real, fake), (nr, nf) = tfid_inputs(int(gold["seed"]))
    check(float(engine.tactile_patch_fid(real.to(DEV), fake.to(DEV), "none")), float(gold["m/T_FID"]), "T_FID none [3, 2, 32, 32]")
    check(float(engine.tactile_patch_fid(real.to(DEV), fake.to(DEV), "mean")), float(gold["tfid_mean"]), "T_FID mean [3, 2, 32, 32]")
    check(float(engine.tactile_patch_fid(nr.to(DEV), nf.to(DEV), "none")), float(gold["tfid_none_nonsquare"]), "T_FID none [2, 2, 12, 20]")
    check(float(engine.tactile_patch_fid(nr.to(DEV), nf.to(DEV), "mean")), float(gold["tfid_mean_nonsquare"]), "T_FID mean [2, 2, 12, 20]")
    with pytest.raises(NotImplementedError):
        engine.tactile_patch_fid(real.to(DEV), fake.to(DEV), "sum")
