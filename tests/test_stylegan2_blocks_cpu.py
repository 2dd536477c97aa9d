"""CPU side of the style-conditioned StyleGAN2 blocks: the parameter containers carry exactly the reference's state-dict keys and shapes
(so a reference checkpoint loads with strict=True), and the new C entries refuse bad arguments on the host (no GPU needed: they return
before any launch)."""
import ctypes

import pytest
import torch

# names and shapes of the reference's modules (models/stylegan_networks.py:378-437), taken once from its own classes
REFERENCE_STATE = {
    "StyledConv(8, 6, 3, 16)": [
        ("conv.weight", (1, 6, 8, 3, 3)), ("conv.modulation.weight", (8, 16)), ("conv.modulation.bias", (8,)), ("noise.weight", (1,)),
        ("activate.bias", (1, 6, 1, 1))],
    "StyledConv(8, 6, 3, 16, upsample=True)": [
        ("conv.weight", (1, 6, 8, 3, 3)), ("conv.blur.kernel", (4, 4)), ("conv.modulation.weight", (8, 16)), ("conv.modulation.bias", (8,)),
        ("noise.weight", (1,)), ("activate.bias", (1, 6, 1, 1))],
    "ToRGB(8, 16)": [
        ("bias", (1, 3, 1, 1)), ("upsample.kernel", (4, 4)), ("conv.weight", (1, 3, 8, 1, 1)), ("conv.modulation.weight", (8, 16)),
        ("conv.modulation.bias", (8,))],
    "ToRGB(8, 16, upsample=False)": [
        ("bias", (1, 3, 1, 1)), ("conv.weight", (1, 3, 8, 1, 1)), ("conv.modulation.weight", (8, 16)), ("conv.modulation.bias", (8,))],
}
REFERENCE_PARAMETERS = {"conv.weight", "conv.modulation.weight", "conv.modulation.bias", "noise.weight", "activate.bias", "bias"}


@pytest.mark.parametrize("ctor", list(REFERENCE_STATE))
def test_blocks_have_the_reference_state_dict(ctor):
    from models.stylegan2_blocks import StyledConv, ToRGB, make_kernel

    m = eval(ctor, {"StyledConv": StyledConv, "ToRGB": ToRGB})
    want = dict(REFERENCE_STATE[ctor])
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert {k for k, _ in m.named_parameters()} == set(want) & REFERENCE_PARAMETERS
    # a state dict with the reference's keys loads strictly; the resampling kernels are the reference's (make_kernel * factor^2)
    m.load_state_dict({k: torch.zeros(s) for k, s in want.items()}, strict=True)
    fresh = eval(ctor, {"StyledConv": StyledConv, "ToRGB": ToRGB}).state_dict()
    for k in want:
        if k.endswith("kernel"):
            assert torch.equal(fresh[k], make_kernel() * 4), k
    assert float(fresh["conv.modulation.bias"].min()) == 1.0      # EqualLinear(bias_init=1)


def test_modulated_conv2d_container():
    from models.stylegan2_blocks import ModulatedConv2d, make_kernel

    for kw, kern in (({}, None), ({"upsample": True}, make_kernel() * 4), ({"downsample": True}, make_kernel()), ({"demodulate": False}, None)):
        sd = ModulatedConv2d(12, 20, 3, 16, **kw).state_dict()
        want = {"weight": (1, 20, 12, 3, 3), "modulation.weight": (12, 16), "modulation.bias": (12,)}
        if kern is not None:
            want["blur.kernel"] = (4, 4)
            assert torch.equal(sd["blur.kernel"], kern)
        assert {k: tuple(v.shape) for k, v in sd.items()} == want


def test_new_entries_refuse_bad_arguments():
    """null pointers and non-positive sizes return -1 with a message in vts_last_error() before anything is launched"""
    from vts import lib as L

    lib = L.load()
    p = ctypes.c_void_p(64)        # never dereferenced on the host; every call below is refused before a launch
    calls = [
        ("vts_modconv_scale_dot", (None, p, None, 4, 16, 1.0, None, p, 0, None, 0, None)),
        ("vts_modconv_scale_dot", (p, p, None, 4, 16, 1.0, None, None, 0, None, 0, None)),
        ("vts_modconv_scale_dot", (p, p, None, 4, 16, 1.0, p, p, 0, None, 0, None)),          # out without its factors
        ("vts_modconv_scale_dot", (p, p, None, 0, 16, 1.0, None, p, 0, None, 0, None)),
        ("vts_modconv_scale_dot", (p, p, None, 4, 0, 1.0, None, p, 0, None, 0, None)),
        ("vts_modconv_scale_dot", (p, p, None, 4, 1 << 20, 1.0, None, p, 0, None, 0, None)),  # long planes need the workspace
        ("vts_modconv_demod_bwd", (None, p, p, p, 2, 4, 4, 9, 0.1, p, 0, p, 0, None)),
        ("vts_modconv_demod_bwd", (p, p, p, p, 2, 4, 4, 9, 0.1, None, 0, p, 0, None)),
        ("vts_modconv_demod_bwd", (p, p, p, p, 0, 4, 4, 9, 0.1, p, 0, p, 0, None)),
        ("vts_modconv_demod_bwd", (p, p, p, p, 2, 4, -1, 9, 0.1, p, 0, p, 0, None)),
        ("vts_modconv_demod_bwd", (p, p, p, p, 2, 4, 4, 0, 0.1, p, 0, p, 0, None)),
        ("vts_modconv_transpose", (None, 4, 4, 9, p, 0, None)),
        ("vts_modconv_transpose", (p, 4, 0, 9, p, 0, None)),
    ]
    for name, args in calls:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name.encode() in lib.vts_last_error(), (name, lib.vts_last_error())
    assert lib.vts_modconv_scale_dot_ws_floats(4, 16) == 0 and lib.vts_modconv_scale_dot_ws_floats(4, 1 << 20) > 0
    assert lib.vts_modconv_scale_dot_ws_floats(0, 16) == 0
