"""The classic pix2pix U-Net generator (--netG unet_128 | unet_256), host side, no GPU needed: the plain-torch restatement
(tests/unet_classic_restated.py) equals the reference's float64 run recorded in tests/golden/unet_classic.npz to 1e-10, the parameter
container has the reference's state-dict keys in its order, the option survives the parser, and the three baselines go on refusing it."""
import contextlib
import io
import json

import pytest
import torch

import unet_classic_restated as R


@pytest.fixture(scope="module")
def gold():
    return R.load_fixture()


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_equals_the_reference_float64_run(gold, case):
    c = R.CASES[case]
    torch.set_num_threads(min(8, torch.get_num_threads()))
    res = R.run_case(c, torch.float64)
    zero = {"grad/" + k for k in R.normed_bias_keys(c)}
    top = max(v.norm().item() for k, v in res.items() if k.startswith("grad/"))
    worst = 0.0
    for k, v in res.items():
        if v.dtype == torch.long:
            assert int(v) == int(gold["%s/%s" % (case, k)]), k
            continue
        if k in zero:      # rounding noise on both sides: a bias in front of a normalisation has no gradient
            assert v.norm().item() < 1e-9 * top, k
            continue
        d = R.check_stored(gold, "%s/%s" % (case, k), v)
        worst = max(worst, d)
        assert d < 1e-10, (k, d)
    print(case, "worst distance to the fixture %.2e" % worst)
    assert set(R.f32_distance(gold, case)) == {k for k, v in res.items() if v.dtype != torch.long and k not in zero}


@pytest.mark.parametrize("case", list(R.CASES))
def test_container_has_the_reference_keys_in_order(gold, case):
    from models import networks

    c = R.CASES[case]
    G = networks.define_G(R.INPUT_NC, R.OUTPUT_NC, c["ngf"], c["net"], c["norm"], use_dropout=c["dropout"])
    assert isinstance(G, networks.UnetGenerator)
    want = [(k, tuple(s)) for k, s in json.loads(str(gold["keys/" + case]))]
    assert [(k, tuple(v.shape)) for k, v in G.state_dict().items()] == want
    G.load_state_dict(R.weights(c))      # strict: the reference's checkpoint loads
    assert G.dropout_levels() == R.dropout_levels(c)


def test_unet_128_has_28_entries_under_instance_norm():
    from models import networks

    sd = networks.define_G(3, 5, 10, "unet_128", "instance").state_dict()
    assert len(sd) == 28 and list(sd)[:3] == ["model.model.0.weight", "model.model.0.bias", "model.model.1.model.1.weight"]
    bn = networks.define_G(3, 5, 10, "unet_128", "batch").state_dict()
    assert [k for k in bn if k.endswith("bias") and "model.3.bias" in k and k.count(".model.") == 1] == ["model.model.3.bias"]
    assert sum(k.endswith("num_batches_tracked") for k in bn) == 11      # 5 down norms + 6 up norms


def test_define_G_refuses_other_norms_and_names_the_new_generators():
    from models import networks

    with pytest.raises(NotImplementedError, match="norm none is not built"):
        networks.define_G(3, 5, 8, "unet_256", "none")
    with pytest.raises(NotImplementedError, match=r"built: .*unet_128, unet_256"):
        networks.define_G(3, 5, 8, "resnet_cat", "instance")


def test_init_weights_reaches_every_layer():
    from models import networks

    G = networks.define_G(3, 5, 8, "unet_128", "batch", init_type="normal", init_gain=0.02)
    for k, v in G.state_dict().items():
        if k.endswith("weight") and v.dim() == 4:
            assert 0.01 < v.std().item() < 0.03, k
        elif k.endswith("bias"):
            assert v.abs().max().item() == 0.0, k


@pytest.mark.parametrize("name", ["unet_128", "unet_256"])
def test_option_round_trip(name):
    from options.train_options import TrainOptions

    with contextlib.redirect_stdout(io.StringIO()):
        opt = TrainOptions(cmd_line="--model sinskitG --gpu_ids -1 --checkpoints_dir /tmp/vts_test_ckpt --name unet_classic_cpu --netG %s --normG batch "
                                    "--no_dropout False" % name).parse()
    assert opt.netG == name and opt.normG == "batch" and opt.no_dropout is False


@pytest.mark.parametrize("model,cls,mod", [("pix2pix", "Pix2PixModel", "pix2pix_model"), ("pix2pixHD", "Pix2PixHDModel", "pix2pixHD_model"),
                                           ("spade", "SPADEModel", "spade_model")])
def test_baselines_still_refuse(model, cls, mod):
    import importlib

    from options.train_options import TrainOptions

    with contextlib.redirect_stdout(io.StringIO()):
        opt = TrainOptions(cmd_line="--model %s --checkpoints_dir /tmp/vts_test_ckpt --name unet_classic_cpu" % model).parse()
    opt.netG = "unet_256"
    klass = getattr(importlib.import_module("models." + mod), cls)
    with pytest.raises(NotImplementedError, match="netG unet_256"):
        klass._check_unbuilt(opt)
