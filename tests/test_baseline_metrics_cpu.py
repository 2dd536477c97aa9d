"""The baselines' evaluation metrics, the parts that need no GPU: the fixture tests/golden/baseline_metrics.npz (regenerated from the
reference where it is present), the metric name lists against the reference's, and the new flags."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "baseline_metrics.npz")
MODELS = ("pix2pix", "spade", "pix2pixHD")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN, allow_pickle=False)


def parse(model, train=True, extra=""):
    from options.test_options import TestOptions
    from options.train_options import TrainOptions

    with contextlib.redirect_stdout(io.StringIO()):
        return (TrainOptions if train else TestOptions)(cmd_line="--model %s --gpu_ids -1 --checkpoints_dir /tmp/vts_test_ckpt --name bm_cpu%s"
                                                                 % (model, extra)).parse()


def test_fixture_is_small_and_holds_numbers_only(gold):
    assert os.path.getsize(GOLDEN) < 64 * 1024
    from tools.make_baseline_metrics_golden import FD_CASES
    assert [tuple(r) for r in gold["fd_cases"].tolist()] == FD_CASES
    for i, (_, _, _, n) in enumerate(FD_CASES):
        assert gold["fd/%d" % i].shape == (n,) and np.isfinite(gold["fd/%d" % i]).all()
    for k in gold.files:
        assert gold[k].size <= 64, k          # seeds, values and name lists: no tensors
    for k in ("m/T_AE", "m/T_MSE", "m/T_FID", "m/I_SIFID", "m/T_SIFID", "tfid_mean", "tfid_mean_nonsquare", "tfid_none_nonsquare"):
        assert np.isfinite(float(gold[k])), k


def test_fixture_regenerates_bit_for_bit(gold, tmp_path):
    """the tool run again on the reference (in a process of its own: it puts the reference's packages in front of this project's) gives
    the committed numbers exactly"""
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("the reference tree is not on this machine")
    out = str(tmp_path / "baseline_metrics.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_baseline_metrics_golden.py"), "--out", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    new = np.load(out, allow_pickle=False)
    assert sorted(new.files) == sorted(gold.files)
    for k in gold.files:
        assert new[k].dtype == gold[k].dtype and np.array_equal(new[k], gold[k]), (k, new[k], gold[k])


@pytest.mark.parametrize("model", MODELS)
def test_metric_name_lists_are_the_references(gold, model):
    from vts import metrics
    for flag in (0, 1):
        assert metrics.metric_name_list(bool(flag)) == json.loads(str(gold["names/%s/%d" % (model, flag)]))
    assert metrics.metric_name_list(True, edited=True) == []
    assert metrics.EVAL_METRICS == json.loads(str(gold["names/%s/0" % model]))


@pytest.mark.parametrize("model", MODELS)
def test_metric_flags_parse_with_defaults_off(model, golden_dir):
    for train in (True, False):
        opt = parse(model, train)
        assert opt.eval_T_FID is False and opt.inception_weights == "" and opt.lpips_weights == "" and opt.lpips_alex_weights == ""
        opt = parse(model, train, " --eval_T_FID --inception_weights a.pth --lpips_weights b.pth --lpips_alex_weights c.pth")
        assert opt.eval_T_FID is True and (opt.inception_weights, opt.lpips_weights, opt.lpips_alex_weights) == ("a.pth", "b.pth", "c.pth")
    # the reference-default option dumps: every reference flag keeps its default beside the new ones
    name, key = ("pix2pix_option_defaults.json", "pix2pix_%s") if model == "pix2pix" else ("ref_option_defaults.json", model + "_%s")
    dumps = json.load(open(os.path.join(golden_dir, name)))
    for train in (True, False):
        ref = dumps.get(key % ("train" if train else "test"))
        if ref is None:
            continue
        opt = parse(model, train)
        for k, v in ref.items():
            if k in ("gpu_ids", "checkpoints_dir", "model", "name"):      # given on the command line
                continue
            d = float("inf") if v["default"] == "inf" else v["default"]
            assert getattr(opt, k) == d or str(getattr(opt, k)) == str(d), (k, getattr(opt, k), d)
        assert not {"eval_T_FID", "inception_weights", "lpips_weights", "lpips_alex_weights"} & set(ref)      # none is a reference flag


def test_lpips_size_check_raises_with_the_reason():
    from vts import metrics
    metrics.lpips_check_size(96, 96, "alex")
    metrics.lpips_check_size(32, 32, "vgg")
    with pytest.raises(ValueError, match="at least 31 x 31"):
        metrics.lpips_check_size(24, 96, "alex")
    with pytest.raises(ValueError, match="at least 16 x 16"):
        metrics.lpips_check_size(96, 12, "vgg")
