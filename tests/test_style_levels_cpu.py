"""The style code at several decoder levels (--num_layer_style_code k > 1) on the CPU: the unchanged oracle (oracle/nets.py:unet_forward
+ autograd) reproduces the reference's results of tests/golden/nets_style_levels.npz, the parameter containers carry the reference's
state-dict keys, and the combination the reference cannot run is refused with its reason."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import detrand

import style_levels_cases as S


def _close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=rtol, atol=atol)


def _probe_close(t, ref, name, rtol=2e-4):
    """probe = (sum, l2, projection), compared relative to the tensor's l2 norm (the bounds of tests/test_oracle_golden.py)"""
    p = detrand.probe(t, name)
    scale = max(abs(ref[1]), 1e-12)
    assert abs(p[1] - ref[1]) <= rtol * scale, (name, p, ref)
    assert abs(p[2] - ref[2]) <= rtol * scale * 4, (name, p, ref)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "nets_style_levels.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", list(S.CASES))
def test_oracle_reproduces_the_reference(golden, name):
    """bounds of test_style_code_generator_fwd_bwd (tests/test_oracle_golden.py) for nets_style_256.npz"""
    c, t = S.case(name), name + "/"
    assert int(golden[t + "seed"]) == c.seed
    r = S.oracle_run_as_reference(name)
    st = S.sub_stride(c)
    _close(r["y"][:, :, ::st, ::st].numpy(), golden[t + "G_out_sub"], rtol=1e-4, atol=2e-5)
    _probe_close(r["y"], golden[t + "G_out_probe"], "g_out")
    _probe_close(r["dx"], golden[t + "G_dx_probe"], "g_dx")
    _close(r["dstyle"].numpy(), golden[t + "G_dstyle"], rtol=2e-3, atol=1e-6)
    assert sorted(r["grads"]) == sorted(k[len(t) + 7:] for k in golden.files if k.startswith(t + "G_grad/"))
    for k, g in r["grads"].items():
        if not c.f64 and S.null_grad_bias(c, k):      # float32 rounding residue of an identically zero gradient (float64 cases: compared)
            continue
        _probe_close(g, golden[t + "G_grad/" + k], k)


@pytest.mark.parametrize("name", list(S.CASES))
def test_container_keys_and_shapes_equal_the_reference(golden, name, monkeypatch):
    """a checkpoint of the reference loads: same keys (tile mode: without the mappings upstream creates and never reads), same shapes"""
    from models import networks

    c, t = S.case(name), name + "/"
    monkeypatch.setattr(networks, "STYLE_INPUT_SIZE", c.h)
    G = networks.CustomUnetGenerator(9, 5, num_downs=S.NUM_DOWNS, ngf=S.NGF, num_layer_separate=S.NLS, opt=S.opt_of(c))
    sd = G.state_dict()
    assert sorted(sd.keys()) == sorted(golden[t + "keys"].tolist())
    assert all(k.startswith("style_code_mapping") for k in golden[t + "dead_keys"].tolist())
    assert (len(golden[t + "dead_keys"]) > 0) == (c.mapping == "tile" and c.via == "reference")
    want = S.shapes(c)       # (the fixture tool asserted these shapes against the reference module's)
    assert {k: tuple(v.shape) for k, v in G.named_parameters()} == {k: tuple(v) for k, v in want.items()}
    assert G.num_layer_style_code == c.k


def test_adain_beyond_five_levels_is_refused_with_the_channel_mismatch():
    """the reference dies with an AssertionError at up2: 4 ngf content channels against the 8 ngf of every style map"""
    from models import networks

    opt = SimpleNamespace(use_style_code=True, style_code_mode="adain", style_code_mapping_mode="project", style_code_dim=512,
                          num_layer_style_code=6, batch_size=1)
    with pytest.raises(ValueError, match=r"channel mismatch at up2.* 40 channels .* 80"):
        networks.CustomUnetGenerator(9, 5, num_downs=8, ngf=10, num_layer_separate=4, opt=opt)
    opt.num_layer_style_code = 5
    assert networks.CustomUnetGenerator(9, 5, num_downs=8, ngf=10, num_layer_separate=4, opt=opt).num_layer_style_code == 5


def test_style_tiles_are_allocated_for_the_innermost_level_only():
    """SinSKITGModel._tile_style_code: the levels below the innermost one take the code as a class bias, so no tile is held for them"""
    from models.sinskitG_model import SinSKITGModel

    made = []
    stub = SimpleNamespace(netG=SimpleNamespace(use_style=True, style_mapping="tile", num_downs=8, num_layer_style_code=8),
                           style_code=torch.ones(2, 512))
    stub._buf = lambda tag, shape: made.append((tag, shape)) or torch.empty(shape)
    SinSKITGModel._tile_style_code(stub, "train", 2, 256, 256)
    assert made == [("train_style_tile7", (2, 512, 1, 1))] and list(stub._style_tiles) == [7]
