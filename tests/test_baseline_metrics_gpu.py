"""Evaluation metrics of the three baselines (vts/metrics.py; compute_metrics of pix2pix, SPADE, pix2pixHD) on the GPU.

1. the shared evaluator on the fixture's seeded batch against the REFERENCE's compute_evaluation_metric values
   (tests/golden/baseline_metrics.npz); PSNR / SSIM, which the reference gets from torchmetrics, against the oracle.
2. each model at the smallest configuration its own GPU test builds: patch contract, N = 2 patches of 32 x 32, seeded weights, VTS_SIFID=1;
   test() then compute_metrics(), against the oracle evaluated on the model's own fake_I / fake_T (generator parity is judged elsewhere).
3. pix2pix on the full-image contract (one 48 x 40 image, three tactile patches): T_* on the gathered fake patches.
4. I_LPIPS / T_LPIPS for both backbones through pix2pix at 96 x 96 patches.

Tolerances are those of the existing tests for the same names (tests/test_step_gpu.py): kernels against the oracle 1e-4 * max(1, |ref|),
through a model 2e-3 * max(1, |ref|); the SIFID chain 2e-3 relative against a reference fixture and 5e-3 relative against the oracle through
a model; T_FID 2e-5 * max(1, |ref|) (test_frechet_distance_matches_reference); LPIPS 1e-3 relative.  Figures are printed before they are
asserted (pytest -s)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_pix2pix_gpu as P2P
import test_pix2pixHD_gpu as HD
import test_spade_step_gpu as SP
from oracle import nets
from tools import make_baseline_metrics_golden as T

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
NO_NET = ["I_PSNR", "I_SSIM", "T_AE", "T_MSE"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "baseline_metrics.npz"), allow_pickle=False)


def close(got, ref, rel, what, floor=0.0):
    bound = rel * max(floor, abs(ref))
    print("%s: got %.8g reference %.8g, |difference| %.3e (bound %.3e)" % (what, got, ref, abs(got - ref), bound))
    assert abs(got - ref) <= bound, (what, got, ref)


def inception():
    from models import inception as inc
    net = inc.InceptionBlock0()
    sd = {k: v.clone() for k, v in net.state_dict().items()}        # the oracle's copy stays on the host
    return net.to(DEV), sd


def tfid_oracle(real_T, fake_T):
    """TactilePatchFID(reduction='none') restated: the 3 x 3 crops of all patches stacked, fake side clamped, oracle Frechet distance"""
    def crops(t):
        n, c, h, w = t.shape
        rows = [t[:, ch, fh:fh + h - 2, fw:fw + w - 2].reshape(n, -1) for ch in range(c) for fh in range(3) for fw in range(3)]
        return torch.stack(rows).reshape(c * 9, -1).contiguous()
    return nets.frechet_distance(crops(real_T), crops(torch.clamp(fake_T, 0, 1)))


def oracle_metrics(real_I, fake_I, real_T, fake_T, sd):
    ref = dict(nets.eval_metrics(real_I, fake_I, real_T, fake_T))
    ref["I_SIFID"], ref["T_SIFID"] = nets.sifid_images(real_I, fake_I, sd), nets.sifid_tactile(real_T, fake_T, sd)
    ref["T_FID"] = tfid_oracle(real_T, fake_T)
    return ref


def compare_with_oracle(m, ref, prefix=""):
    for k in NO_NET:
        close(m[prefix + k], ref[k], 2e-3, prefix + k, floor=1.0)
    for k in ("I_SIFID", "T_SIFID"):
        close(m[prefix + k], ref[k], 5e-3, prefix + k)
    if prefix + "T_FID" in m:
        close(m[prefix + "T_FID"], ref["T_FID"], 2e-5, prefix + "T_FID", floor=1.0)


# ---- 1. the shared evaluator against the reference --------------------------------------------------------------------------------------
def test_evaluator_matches_the_reference_on_the_fixture_batch(gold):
    from vts import metrics
    net, _ = inception()
    real_I, fake_I, real_T, fake_T = T.metric_batch(int(gold["seed"]))
    m = metrics.evaluate(real_I.to(DEV), fake_I.to(DEV), real_T.to(DEV), fake_T.to(DEV), sifid_net=net, want_tfid=True)
    assert list(m) == ["I_SIFID", "I_PSNR", "I_SSIM", "T_SIFID", "T_AE", "T_MSE", "T_FID"]
    close(m["I_SIFID"], float(gold["m/I_SIFID"]), 2e-3, "I_SIFID vs reference")
    close(m["T_SIFID"], float(gold["m/T_SIFID"]), 2e-3, "T_SIFID vs reference")
    close(m["T_AE"], float(gold["m/T_AE"]), 1e-4, "T_AE vs reference", floor=1.0)
    close(m["T_MSE"], float(gold["m/T_MSE"]), 1e-4, "T_MSE vs reference", floor=1.0)
    close(m["T_FID"], float(gold["m/T_FID"]), 2e-5, "T_FID vs reference", floor=1.0)
    ref = nets.eval_metrics(real_I, fake_I, real_T, fake_T)
    close(m["I_PSNR"], ref["I_PSNR"], 1e-4, "I_PSNR vs oracle", floor=1.0)
    close(m["I_SSIM"], ref["I_SSIM"], 1e-4, "I_SSIM vs oracle", floor=1.0)
    # without the optional networks: the four weight-free metrics, in the reference's order
    assert list(metrics.evaluate(real_I.to(DEV), fake_I.to(DEV), real_T.to(DEV), fake_T.to(DEV))) == NO_NET


def test_lpips_on_a_refused_size_raises_before_any_launch(gold):
    from vts import metrics
    real_I, fake_I, real_T, fake_T = (t.to(DEV) for t in T.metric_batch(int(gold["seed"]), n=2, size=24))
    with pytest.raises(ValueError, match="at least 31 x 31"):
        metrics.evaluate(real_I, fake_I, real_T, fake_T, lpips_net=object(), lpips_backbone="alex")


# ---- 2. the three models, patch contract --------------------------------------------------------------------------------------------------
def build_pix2pix(extra, train=True, tmp=None):
    """the `default` case of tests/golden/pix2pix_step_32.npz on seeded weights; train=False: a test-phase model (TestOptions) that loads
    the generator a training-phase model saved under tmp"""
    g = np.load(os.path.join(GOLDEN, "pix2pix_step_32.npz"), allow_pickle=False)
    model = P2P.make_model(g, "default", " --use_hip_graph False" + (extra if train else ""), save_dir=tmp)
    P2P.seed_weights(g, "default", model)
    if not train:
        model.save_networks("latest")
        model = P2P.make_model(g, "default", extra, train=False, save_dir=tmp)
    return model, int(g["default/seed"])


def build_spade(extra):
    g = np.load(os.path.join(GOLDEN, "spade_step_32.npz"), allow_pickle=False)
    model = SP.make_model(g, "B", " --use_hip_graph False" + extra)
    SP.seed_weights(g, "B", model)
    return model, int(g["B/seed"])


def build_pix2pixHD(extra):
    model, _ = HD.make_model(" --use_hip_graph False" + extra)
    HD.load_weights(model, 71)
    return model, 71


BUILDERS = {"pix2pix": build_pix2pix, "spade": build_spade, "pix2pixHD": build_pix2pixHD}


@pytest.mark.parametrize("name", list(BUILDERS))
def test_model_metrics_on_patches_match_the_oracle(gold, name, monkeypatch):
    monkeypatch.setenv("VTS_SIFID", "1")
    monkeypatch.delenv("VTS_LPIPS_METRICS", raising=False)
    model, seed = BUILDERS[name](" --eval_T_FID")
    _, sd = inception()
    model.set_input(P2P.p2p_batch(2, 32, seed), phase="test")
    model.test()
    m = model.compute_metrics()
    assert model.metric_T_contract == "patch" and model.metric_sifid_pretrained is False and model.metric_ssim_pinned == "restatement"
    ref = oracle_metrics(model.real_I.cpu(), model.fake_I.cpu(), model.real_T.cpu(), model.fake_T.cpu(), sd)
    compare_with_oracle(m, ref)
    # the names: the reference's list and order (the LPIPS pair joins it when its network is there, test 4), T_FID behind it on request
    want = [k for k in json.loads(str(gold["names/%s/0" % name])) if "LPIPS" not in k]
    assert list(model.get_current_metrics()) == ["m_" + k for k in want + ["T_FID"]]
    assert all(model.get_current_metrics()["m_" + k] == m[k] for k in want)
    # without --eval_T_FID, and with the training patches' prefix as train_for_each_epoch adds it
    model.opt.eval_T_FID = False
    model.metric_names = []
    mt = model.compute_metrics("train_")
    m0 = model.compute_metrics()
    assert "T_FID" not in m0 and all(m0[k] == m[k] and mt["train_" + k] == m[k] for k in want)
    want2 = [k for k in json.loads(str(gold["names/%s/1" % name])) if "LPIPS" not in k]
    assert list(model.get_current_metrics()) == ["m_" + k for k in want2]
    # edited sketches: upstream skips the metrics
    model.test_edit_S = True
    assert model.compute_metrics() == {}


# ---- 3. pix2pix on the full-image contract ------------------------------------------------------------------------------------------------
def test_pix2pix_full_image_contract_gathers_the_fake_patches(gold, monkeypatch, tmp_path):
    monkeypatch.setenv("VTS_SIFID", "1")
    monkeypatch.delenv("VTS_LPIPS_METRICS", raising=False)
    g = np.load(os.path.join(GOLDEN, "pix2pix_step_32.npz"), allow_pickle=False)
    h, w, nt = (int(v) for v in g["full"])
    model, seed = build_pix2pix(" --eval_T_FID", train=False, tmp=str(tmp_path))
    assert model.opt.return_patch is False
    _, sd = inception()
    batch = P2P.full_batch(h, w, nt, int(g["size"]), seed)
    # T_coords in the dataset's format (ROI_x, ROI_y, ROI_h, ROI_w, 32, resize_ratio, crop_x, crop_y): the fixture's batch leaves the last
    # four zero, which nothing read so far; windows inside the image and one that the gather clamps at the right border
    coords = torch.tensor([[[0, 1, 40, 40, 32, 1, 3, 2], [2, 6, 40, 40, 32, 1, 1, 7], [5, 0, 40, 40, 32, 1, 6, 4]]], dtype=torch.float64)
    assert nt == 3
    batch["T_coords"], batch["full_T_coords"] = coords, coords.clone()
    model.set_input(batch, phase="test")
    model.test()
    assert tuple(model.fake_T.shape) == (1, 2, h, w) and tuple(model.real_T.shape) == (nt, 2, 32, 32)
    m = model.compute_metrics()
    assert model.metric_T_contract == "gathered"
    ox, oy, cs = nets.find_coords_for_patch(batch["T_coords"][0])
    assert (cs == 32).all()
    fake_patches = nets.gather_patches(model.fake_T.cpu(), ox, oy, 32)
    ref = oracle_metrics(model.real_I.cpu(), model.fake_I.cpu(), model.real_T.cpu(), fake_patches, sd)
    compare_with_oracle(m, ref)


# ---- 4. LPIPS, one case per backbone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", ["vgg", "alex"])
def test_pix2pix_lpips_metrics_match_the_oracle(gold, backbone, monkeypatch, tmp_path):
    """96 x 96 patches, N = 2.  The chain's argument checks admit this size: AlexNet's maps are 23 -> 11 -> 5 (vts_maxpool3s2_relu_pad
    needs 3 x 3 in front of each pool, i.e. images of 31 x 31 at least), VGG16's 96 -> 48 -> 24 -> 12 -> 6 (vts_maxpool2_relu_pad needs
    2 x 2); the tactile side always runs at 224 x 224."""
    from oracle import perceptual as chk
    monkeypatch.setenv("VTS_LPIPS_METRICS", "1")
    monkeypatch.setenv("VTS_SIFID", "1")
    train = backbone == "vgg"        # eval_LPIPS: VGG16 while training, AlexNet in the test phase (pix2pix_model.py:230-233)
    model, seed = build_pix2pix("" if train else " --return_patch True", train=train, tmp=str(tmp_path))
    model.set_input(P2P.p2p_batch(2, 96, seed), phase="test")
    model.test()
    m = model.compute_metrics()
    assert model.metric_lpips_backbone == backbone and model.metric_lpips_pretrained is False
    lp = chk.LPIPS(net=backbone)
    with torch.no_grad():
        ref_I = float(lp(model.real_I.cpu(), model.fake_I.cpu()).mean())
        rT = F.interpolate(model.real_T.cpu(), (224, 224))
        fT = F.interpolate(model.fake_T.cpu().clamp(0, 1), (224, 224))
        ref_T = float(lp(rT[:, 0:1], fT[:, 0:1]).mean() + lp(rT[:, 1:2], fT[:, 1:2]).mean())
    close(m["I_LPIPS"], ref_I, 1e-3, "I_LPIPS (%s)" % backbone)
    close(m["T_LPIPS"], ref_T, 1e-3, "T_LPIPS (%s)" % backbone)
    # with both optional networks the names are exactly the reference's eight, in its order
    assert list(model.get_current_metrics()) == ["m_" + k for k in json.loads(str(gold["names/pix2pix/0"]))]
