"""The SPADE baseline model's host side, no GPU needed: the model resolves, its parsed options and name lists equal what the reference's own
parser and model give (recorded in tests/golden/spade_step_32.npz by tools/make_spade_step_golden.py), and it refuses what it does not build."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spade_step_32.npz")
FLAGS = "--model spade --checkpoints_dir /tmp/vts_test_ckpt --name spade_cpu"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN, allow_pickle=False)


def parse(train=True, extra="", flags=FLAGS):
    from options.test_options import TestOptions
    from options.train_options import TrainOptions

    return (TrainOptions if train else TestOptions)(cmd_line=flags + extra).parse()


def test_model_resolves():
    from models import find_model_using_name
    from models.base_model import BaseModel

    cls = find_model_using_name("spade")
    assert cls.__name__ == "SPADEModel" and issubclass(cls, BaseModel)


@pytest.mark.parametrize("phase", ["train", "test"])
@pytest.mark.parametrize("no_ttur", [False, True])
def test_parsed_defaults_equal_the_reference_parser(gold, phase, no_ttur):
    ref = json.loads(str(gold["opts"]))[phase + ("_no_TTUR" if no_ttur else "")]
    opt = parse(phase == "train", " --no_TTUR" if no_ttur else "")
    got = {k: getattr(opt, k, None) for k in ref}
    assert got == ref, {k: (got[k], ref[k]) for k in ref if got[k] != ref[k]}
    assert opt.no_TTUR is no_ttur and opt.netG == "spade"


def test_an_explicit_beta_wins_over_the_no_ttur_default():
    opt = parse(True, " --no_TTUR --beta1 0.25")
    assert (opt.beta1, opt.beta2) == (0.25, 0.999)


def test_learning_rates_follow_no_ttur():
    from models.spade_model import SPADEModel

    opt = parse(True)
    assert SPADEModel.learning_rates(opt) == (opt.lr / 2, opt.lr * 2)
    assert SPADEModel.learning_rates(parse(True, " --no_TTUR")) == (opt.lr, opt.lr)


REFUSALS = [
    ({"use_vae": True}, "passes norm twice"),
    ({"use_features": True}, "not reachable in the reference"),
    ({"no_instance": False}, "not reachable in the reference"),
    ({"label_nc": 3}, "not reachable in the reference"),
    ({"T_resolution_multiplier": 2}, "not built: T_resolution_multiplier"),
    ({"use_bg_mask": False}, "not built: use_bg_mask False"),
    ({"no_gan_loss": True}, "not built: no_gan_loss"),
    ({"netG": "global"}, "not built: netG global"),
    ({"netD": "basic"}, "not built: netD basic"),
    ({"gpu_ids": [0, 1]}, "not built: data-parallel"),
]


@pytest.mark.parametrize("override,message", REFUSALS, ids=[list(o)[0] for o, _ in REFUSALS])
def test_check_unbuilt_refuses(override, message):
    from models.spade_model import SPADEModel

    opt = parse(True)
    for k, v in override.items():
        setattr(opt, k, v)
    with pytest.raises(NotImplementedError, match=message):
        SPADEModel._check_unbuilt(opt)


def test_check_unbuilt_refuses_a_data_parallel_launch(monkeypatch):
    from models.spade_model import SPADEModel

    opt = parse(True)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="syncbatch statistics across"):
        SPADEModel._check_unbuilt(opt)


def test_check_unbuilt_accepts_the_defaults_and_the_fixture_cases(gold):
    from models.spade_model import SPADEModel

    SPADEModel._check_unbuilt(parse(True))
    SPADEModel._check_unbuilt(parse(False))
    for case in ("default", "B"):
        opt = parse(True, " " + " ".join(json.loads(str(gold[case + "/flags"]))))
        for k, v in json.loads(str(gold[case + "/override"])).items():
            setattr(opt, k, v)
        SPADEModel._check_unbuilt(opt)


@pytest.mark.parametrize("case", ["default", "B", "test"])
def test_name_lists_equal_the_reference_model(gold, case):
    from models.spade_model import SPADEModel

    ref = json.loads(str(gold[case + "/names"]))
    extra = "" if case == "test" else " " + " ".join(json.loads(str(gold[case + "/flags"])))
    loss, visual, model = SPADEModel.name_lists(parse(case != "test", extra))
    assert ["l_" + n for n in loss] == ["l_" + n for n in ref["loss_names"]]
    assert visual == ref["visual_names"] and model == ref["model_names"]
    edit = parse(False, " --dataroot ./datasets/edit_S")
    assert "real_I" not in SPADEModel.name_lists(edit)[1]
