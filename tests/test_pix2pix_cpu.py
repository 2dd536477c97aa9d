"""The pix2pix baseline model's host side, no GPU needed: the model resolves, its parsed options and name lists equal what the reference's own
parser and model give (recorded in tests/golden/pix2pix_option_defaults.json and pix2pix_step_32.npz by tools/make_pix2pix_step_golden.py),
it refuses what it does not build, and define_D's new names leave the other models' refusals as they were."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pix2pix_step_32.npz")
DEFAULTS = os.path.join(HERE, "golden", "pix2pix_option_defaults.json")
FLAGS = "--model pix2pix --checkpoints_dir /tmp/vts_test_ckpt --name pix2pix_cpu"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN, allow_pickle=False)


def parse(train=True, extra="", flags=FLAGS):
    from options.test_options import TestOptions
    from options.train_options import TrainOptions

    with contextlib.redirect_stdout(io.StringIO()):
        return (TrainOptions if train else TestOptions)(cmd_line=flags + extra).parse()


def test_model_resolves():
    from models import find_model_using_name
    from models.base_model import BaseModel

    cls = find_model_using_name("pix2pix")
    assert cls.__name__ == "Pix2PixModel" and issubclass(cls, BaseModel)


@pytest.mark.parametrize("phase", ["train", "test"])
def test_parsed_defaults_equal_the_reference_parser(phase):
    """every flag the reference's parser declares for this model and phase: present, with the reference's default, key for key; the model's
    own flags carry the reference's types"""
    ref = json.load(open(DEFAULTS))["pix2pix_" + phase]
    opt = parse(phase == "train", " --gpu_ids -1", flags="--model pix2pix --checkpoints_dir /tmp/vts_test_ckpt")
    assert len(ref) > 60
    for k, v in ref.items():
        if k in ("gpu_ids", "checkpoints_dir", "model"):   # given on the command line
            continue
        assert hasattr(opt, k), k
        d = float("inf") if v["default"] == "inf" else v["default"]
        assert getattr(opt, k) == d or str(getattr(opt, k)) == str(d), (k, getattr(opt, k), d)
        if v["model"] and d is not None:
            assert type(getattr(opt, k)).__name__ == {"str2bool": "bool"}.get(v["type"], v["type"]), (k, v["type"])
    # the defaults the option setter moves: the issue's table
    want = dict(netG="resnet_9blocks", norm="batch", netD="basic", n_layers_D=3, no_dropout=True, init_type="xavier", dataset_mode="aligned",
                dataset="patchskit", scale_nz=0.25, T_resolution_multiplier=1, lambda_L1=100.0, lr_G2=5e-4)
    if phase == "train":
        want.update(gan_mode="vanilla", lr=2e-4, beta1=0.5, beta2=0.999, pool_size=0, return_patch=True, batch_size=32)
    else:
        want.update(return_patch=False, batch_size=1)
    assert {k: getattr(opt, k) for k in want} == want


REFUSALS = [
    ({"netG": "unet_256"}, "not built: netG unet_256"),
    ({"netG": "unet256_custom"}, "not built: netG unet256_custom"),
    ({"netD": "pixel"}, "not built: netD pixel"),
    ({"netD": "multiscale"}, "not built: netD multiscale"),
    ({"norm": "instance"}, "not built: norm instance"),
    ({"no_dropout": False}, "not built: no_dropout False"),
    ({"use_bg_mask": False}, "not built: use_bg_mask False"),
    ({"T_resolution_multiplier": 2}, "not built: T_resolution_multiplier != 1"),
    ({"gan_mode": "wgangp"}, "not built: gan_mode wgangp"),
    ({"gpu_ids": [0, 1]}, "not built: data-parallel"),
]


@pytest.mark.parametrize("override,message", REFUSALS, ids=["%s=%s" % (list(o)[0], list(o.values())[0]) for o, _ in REFUSALS])
def test_check_unbuilt_refuses(override, message):
    from models.pix2pix_model import Pix2PixModel

    opt = parse(True)
    for k, v in override.items():
        setattr(opt, k, v)
    with pytest.raises(NotImplementedError, match=message):
        Pix2PixModel._check_unbuilt(opt)


def test_check_unbuilt_lists_one_line_per_reason():
    from models.pix2pix_model import Pix2PixModel

    opt = parse(True)
    opt.netD, opt.norm = "pixel", "instance"
    with pytest.raises(NotImplementedError) as e:
        Pix2PixModel._check_unbuilt(opt)
    assert str(e.value).count("not built: ") == 2


def test_check_unbuilt_refuses_a_data_parallel_launch(monkeypatch):
    from models.pix2pix_model import Pix2PixModel

    opt = parse(True)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="own BatchNorm batch"):
        Pix2PixModel._check_unbuilt(opt)


def test_check_unbuilt_accepts_the_defaults_and_the_fixture_cases(gold):
    from models.pix2pix_model import Pix2PixModel

    Pix2PixModel._check_unbuilt(parse(True))
    Pix2PixModel._check_unbuilt(parse(False))
    for mode in ("lsgan", "hinge", "nonsaturating", "wgan"):
        Pix2PixModel._check_unbuilt(parse(True, " --gan_mode " + mode))
    for case in ("default", "B"):
        Pix2PixModel._check_unbuilt(parse(True, " " + " ".join(json.loads(str(gold[case + "/flags"])))))


@pytest.mark.parametrize("case", ["default", "B", "test"])
def test_name_lists_equal_the_reference_model(gold, case):
    from models.pix2pix_model import Pix2PixModel

    ref = json.loads(str(gold[case + "/names"]))
    extra = "" if case == "test" else " " + " ".join(json.loads(str(gold[case + "/flags"])))
    loss, visual, model = Pix2PixModel.name_lists(parse(case != "test", extra))
    assert loss == ref["loss_names"] == ["G_GAN", "G_L1", "D_real", "D_fake", "D2_real", "D2_fake"]
    assert visual == ref["visual_names"] and model == ref["model_names"]
    assert model == (["G"] if case == "test" else ["G", "D", "D2"])
    edit = parse(False, " --dataroot ./datasets/edit_S")
    assert "real_I" not in Pix2PixModel.name_lists(edit)[1]


@pytest.mark.parametrize("netD,n_layers_D,depth", [("basic", 3, 3), ("basic", 2, 3), ("n_layers", 2, 2)])
def test_define_D_builds_the_single_patchgan_with_reference_keys(gold, netD, n_layers_D, depth):
    """a parameter container (no compute): the reference's keys and shapes at --ndf 8, 25 entries for 3 layers and 18 for 2; 'basic' is
    depth 3 whatever --n_layers_D says; one scale, never a Sigmoid"""
    from types import SimpleNamespace

    from models import networks

    keys = json.loads(str(gold[("default" if depth == 3 else "B") + "/keys"]))
    for nm, cin in (("D", 4), ("D2", 3)):
        D = networks.define_D(cin, 8, netD, n_layers_D, "batch", "xavier", 0.02, False, opt=SimpleNamespace(gan_mode="vanilla"))
        assert [[k, list(v.shape)] for k, v in D.state_dict().items()] == keys[nm]
        assert len(keys[nm]) == {3: 25, 2: 18}[depth]
        assert D.num_D == 1 and D.use_sigmoid is False and D.layer0 is D.model and D.n_layers == depth


@pytest.mark.parametrize("case", ["default", "B"])
def test_define_G_lists_the_reference_keys_in_the_reference_order(gold, case):
    """the ResNet generator under BatchNorm, anti-aliased (default) and with strided / transposed convolutions (B): the reference's
    state-dict list, order included (144 and 104 entries)"""
    from models import networks

    opt = parse(True, " " + " ".join(json.loads(str(gold[case + "/flags"]))))
    G = networks.define_G(opt.sketch_nc, opt.image_nc + opt.touch_nc, opt.ngf, opt.netG, opt.norm, not opt.no_dropout, opt.init_type,
                          opt.init_gain, opt.no_antialias, opt.no_antialias_up, (), opt)
    keys = json.loads(str(gold[case + "/keys"]))["G"]
    assert [[k, list(v.shape)] for k, v in G.state_dict().items()] == keys and len(keys) == {"default": 144, "B": 104}[case]


def test_define_D_keeps_refusing_what_is_not_built():
    from models import networks

    with pytest.raises(NotImplementedError, match="built for norm=batch only"):
        networks.define_D(4, 8, "basic", 3, "instance")
    for name in ("pixel", "patch", "tilestylegan2"):
        with pytest.raises(NotImplementedError, match=r"built: basic, n_layers, multiscale, stylegan2"):
            networks.define_D(4, 8, name, 3, "batch")


def test_the_other_models_still_refuse_the_single_patchgan():
    """define_D building `basic` / `n_layers` does not make them reachable from the steps that were never wired to them"""
    from models.pix2pixHD_model import Pix2PixHDModel
    from models.spade_model import SPADEModel

    opt = parse(True, flags="--model spade --checkpoints_dir /tmp/vts_test_ckpt --name pix2pix_cpu")
    opt.netD = "basic"
    with pytest.raises(NotImplementedError, match="not built: netD basic"):
        SPADEModel._check_unbuilt(opt)
    opt = parse(True, flags="--model pix2pixHD --checkpoints_dir /tmp/vts_test_ckpt --name pix2pix_cpu")
    Pix2PixHDModel._check_unbuilt(opt)
    opt.netD = "n_layers"
    with pytest.raises(NotImplementedError, match="netD n_layers"):
        Pix2PixHDModel._check_unbuilt(opt)


def test_aligned_stays_a_parser_default_only():
    from data import create_dataset

    opt = parse(True, " --gpu_ids -1")
    assert opt.dataset_mode == "aligned"
    with pytest.raises(NotImplementedError, match="dataset_mode aligned"):
        create_dataset(opt)
