"""The classic pix2pix U-Net generator (--netG unet_128 | unet_256) restated in plain torch (TEST INFRASTRUCTURE ONLY).

A functional forward over a state dict with the reference's nested keys, differentiable by autograd in any dtype; the cases of the
fixture tests/golden/unet_classic.npz (made by tools/make_unet_classic_golden.py from the reference run in float64); the weights,
inputs, cotangents and Dropout masks both sides draw from oracle.detrand, so the fixture stores none of them.

Level i (0 = outermost) owns  down<i>: Conv2d(4, 2, 1) ch[i-1] -> ch[i]  and  up<i>: ConvTranspose2d(4, 2, 1) 2 ch[i] -> ch[i-1]
(the innermost one ch[i] -> ch[i-1]), ch = ngf * (1, 2, 4, 8, 8, ...):
  f[0] = down0(x)                              f[i] = norm(down<i>(lrelu(f[i-1])))        f[nd-1] = down(lrelu(f[nd-2]))   (no norm)
  u[nd-1] = norm(up(relu(f[nd-1])))            u[i] = [dropout](norm(up<i>(relu(cat[f[i], u[i+1]]))))
  out = tanh(up0(relu(cat[f[0], u[1]])))
The reference applies its LeakyReLU in place, so its cat holds lrelu(f[i]); relu(lrelu(t)) = relu(t), so the raw f[i] gives the
same values and the same gradient.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import detrand  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "unet_classic.npz")
FULL_MAX = 4096     # tensors up to this many elements are stored whole in the fixture, larger ones as detrand.probe triples

# name: net, ngf, norm, (H, W), batch, dropout
CASES = {
    "c1_128_ngf8_in": dict(net="unet_128", ngf=8, norm="instance", hw=(128, 128), N=2, dropout=False, seed=2401),
    "c2_128_ngf8_bn": dict(net="unet_128", ngf=8, norm="batch", hw=(128, 256), N=3, dropout=False, seed=2402),
    "c3_128_ngf24_in": dict(net="unet_128", ngf=24, norm="instance", hw=(128, 128), N=2, dropout=False, seed=2403),
    "c3_128_ngf24_bn": dict(net="unet_128", ngf=24, norm="batch", hw=(128, 128), N=2, dropout=False, seed=2404),
    "c4_256_ngf8_drop": dict(net="unet_256", ngf=8, norm="instance", hw=(256, 256), N=1, dropout=True, seed=2405),
}
# the further shape the GPU test judges against this restatement alone (float64): non-square, batch 1, the wide path, two seeds.
# No seed keeps every ReLU / LeakyReLU argument of its float64 run clear of fp32 rounding (~5e-7 on these O(1) values).  Seed 2406 has one of
# 4.2e-7 in front of up1: the MI355X run lands on the other side of that kink and every gradient behind it is 8.8e-4 from both judges
# (1e-6 on the others), inside the 1e-3 bound.  Seed 2419 has the widest margin of 2406 .. 2419 (1.9e-6) and measures 1.3e-6 throughout.
EXTRA_CASES = {
    "extra_128x384_ngf24_s2406": dict(net="unet_128", ngf=24, norm="instance", hw=(128, 384), N=1, dropout=False, seed=2406),
    "extra_128x384_ngf24_s2419": dict(net="unet_128", ngf=24, norm="instance", hw=(128, 384), N=1, dropout=False, seed=2419),
    # ngf 41: 82 output channels are more than 80 and no multiple of 4 (those launches stay on the 4 x 4 kernels), 164 and 328 are
    "extra_128x128_ngf41": dict(net="unet_128", ngf=41, norm="batch", hw=(128, 128), N=1, dropout=False, seed=2420),
}
INPUT_NC, OUTPUT_NC = 3, 5
# the reference step of the fixture: one SinSKITGModel.optimize_parameters with --netG unet_256 at the model's defaults (ngf 10, InstanceNorm)
STEP = dict(size=256, seed=2450, nt=64, flags=["--netG", "unet_256"])


def num_downs(net):
    return {"unet_128": 7, "unet_256": 8}[net]


def channels(c):
    return [c["ngf"] * min(2 ** i, 8) for i in range(num_downs(c["net"]))]


def level_prefix(i):
    """state-dict prefix of level i's nn.Sequential: model.model / model.model.1.model / model.model.1.model.3.model / ..."""
    return "model.model" + (".1.model" if i >= 1 else "") + ".3.model" * max(i - 1, 0)


def level_keys(i, nd):
    """(down conv, down norm, up conv, up norm) module names of level i; None where the level has none"""
    p = level_prefix(i)
    if i == 0:
        return p + ".0", None, p + ".3", None
    if i == nd - 1:
        return p + ".1", None, p + ".3", p + ".4"
    return p + ".1", p + ".2", p + ".5", p + ".6"


def dropout_levels(c):
    return list(range(4, num_downs(c["net"]) - 1)) if c["dropout"] else []


def param_shapes(c, input_nc=INPUT_NC, output_nc=OUTPUT_NC):
    """{key: shape} in the reference's state-dict order, and the set of ConvTranspose2d weight keys"""
    nd, ch = num_downs(c["net"]), channels(c)
    bn, bias = c["norm"] == "batch", c["norm"] == "instance"
    transposed = set()

    def norm_entries(name, n):
        if not bn or name is None:
            return []
        return [(name + ".weight", (n,)), (name + ".bias", (n,)), (name + ".running_mean", (n,)), (name + ".running_var", (n,)),
                (name + ".num_batches_tracked", ())]

    def walk(i):
        dk, dn, uk, un = level_keys(i, nd)
        cin, cout = (ch[i - 1] if i else input_nc), (ch[i - 1] if i else output_nc)
        items = [(dk + ".weight", (ch[i], cin, 4, 4))] + ([(dk + ".bias", (ch[i],))] if bias else [])
        items += norm_entries(dn, ch[i])
        if i < nd - 1:
            items += walk(i + 1)
        items += [(uk + ".weight", (ch[i] * (1 if i == nd - 1 else 2), cout, 4, 4))] + ([(uk + ".bias", (cout,))] if (bias or i == 0) else [])
        transposed.add(uk + ".weight")
        items += norm_entries(un, cout)
        return items

    return dict(walk(0)), transposed


def weights(c, input_nc=INPUT_NC):
    """float32 state dict: convolution weights at a scale that keeps activations O(1), small biases, BatchNorm gamma near 1, fresh
    running statistics"""
    shapes, transposed = param_shapes(c, input_nc)
    sd = {}
    for k, shp in shapes.items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.long)
        elif k.endswith("running_mean"):
            sd[k] = torch.zeros(shp)
        elif k.endswith("running_var"):
            sd[k] = torch.ones(shp)
        elif len(shp) == 4:
            fan_in = shp[0] * 4 if k in transposed else shp[1] * 16      # a transposed stride-2 output sums 2 x 2 taps of every input channel
            sd[k] = detrand.uniform(shp, c["seed"], k) * float(np.sqrt(3.0 / fan_in))
        elif k.endswith("weight"):
            sd[k] = 1.0 + 0.1 * detrand.uniform(shp, c["seed"], k)
        else:
            sd[k] = 0.1 * detrand.uniform(shp, c["seed"], k)
    return sd


def is_param(k):
    return not k.endswith(("running_mean", "running_var", "num_batches_tracked"))


def net_input(c):
    return detrand.uniform((c["N"], INPUT_NC) + tuple(c["hw"]), c["seed"], "x")


def cotangent(c):
    return detrand.uniform((c["N"], OUTPUT_NC) + tuple(c["hw"]), c["seed"], "cot")


def dropout_masks(c):
    """{level: keep mask [N, ch[level - 1], h, w] of 0 / 1} for the levels whose up output passes Dropout(0.5)"""
    ch = channels(c)
    h, w = c["hw"]
    return {i: (detrand.uniform((c["N"], ch[i - 1], h >> i, w >> i), c["seed"], "drop%d" % i) > 0).float() for i in dropout_levels(c)}


def cast(sd, dtype, grad=True):
    out = {}
    for k, v in sd.items():
        if v.dtype == torch.long:
            out[k] = v.clone()
        else:
            out[k] = v.detach().to(dtype).clone()
            if grad and is_param(k):
                out[k].requires_grad_(True)
    return out


def rel_l2(a, b):
    """true relative L2 of a against the judge b (both moved to float64 on the CPU)"""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def _norm(sd, name, t, kind, training):
    if kind == "instance":
        return F.instance_norm(t, eps=1e-5)
    rm, rv = sd[name + ".running_mean"], sd[name + ".running_var"]
    if training:
        sd[name + ".num_batches_tracked"] += 1
    return F.batch_norm(t, rm, rv, sd[name + ".weight"], sd[name + ".bias"], training=training, momentum=0.1, eps=1e-5)


def unet(sd, x, c, training=True, masks=None):
    """forward of the generator over the state dict `sd` (BatchNorm buffers are advanced in place in training mode)"""
    nd, kind = num_downs(c["net"]), c["norm"]
    f, t = [], x
    for i in range(nd):
        dk, dn, _, _ = level_keys(i, nd)
        t = F.conv2d(F.leaky_relu(t, 0.2) if i else t, sd[dk + ".weight"], sd.get(dk + ".bias"), stride=2, padding=1)
        if dn is not None:
            t = _norm(sd, dn, t, kind, training)
        f.append(t)
    u = None
    for i in range(nd - 1, -1, -1):
        _, _, uk, un = level_keys(i, nd)
        src = f[i] if u is None else torch.cat([f[i], u], 1)
        u = F.conv_transpose2d(F.relu(src), sd[uk + ".weight"], sd.get(uk + ".bias"), stride=2, padding=1)
        if i == 0:
            return torch.tanh(u)
        u = _norm(sd, un, u, kind, training)
        if training and masks is not None and i in masks:
            u = u * (masks[i].to(u.dtype) * 2.0)


def buffers_of(sd):
    return {k: v.detach().clone() for k, v in sd.items() if not is_param(k)}


def run_case(c, dtype, forward=None, sd=None):
    """out, parameter gradients under the case's cotangent, BatchNorm buffers after one and two training passes, and the eval-mode
    output after those.  forward(sd, x, training) defaults to this restatement."""
    sd = cast(weights(c), dtype) if sd is None else sd
    masks = dropout_masks(c) or None
    fwd = forward or (lambda s, x, training: unet(s, x, c, training, masks))
    x = net_input(c).to(dtype)
    out = fwd(sd, x, True)
    (out * cotangent(c).to(dtype)).sum().backward()
    res = {"out": out.detach()}
    res.update({"grad/" + k: v.grad.detach().clone() for k, v in sd.items() if is_param(k)})
    res.update({"buf1/" + k: v for k, v in buffers_of(sd).items()})
    with torch.no_grad():
        fwd(sd, x, True)
        res.update({"buf2/" + k: v for k, v in buffers_of(sd).items()})
        res["out_eval"] = fwd(sd, x, False).detach()
    return res


def normed_bias_keys(c):
    """conv biases that feed a normalisation: their true gradient is zero (the reference computes rounding noise there)"""
    if c["norm"] != "instance":
        return []
    nd = num_downs(c["net"])
    keys = []
    for i in range(nd):
        dk, dn, uk, un = level_keys(i, nd)
        if dn is not None:
            keys.append(dk + ".bias")
        if un is not None:
            keys.append(uk + ".bias")
    return keys


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def load_fixture(path=FIXTURE):
    return np.load(path, allow_pickle=False)


def f32_distance(z, case):
    """{tensor name: relative L2 of the reference's own float32 run to its float64 run}"""
    return json.loads(str(z["f32/" + case]))


_PROBES = {}


def _is_probe(z, name):
    if id(z) not in _PROBES:
        _PROBES.clear()
        _PROBES[id(z)] = set(json.loads(str(z["probes"])))
    return name in _PROBES[id(z)]


def check_stored(z, name, t):
    """relative distance of tensor t to what the fixture stores under `name` (whole tensor: relative L2; probe triple: worst component
    relative to the stored l2 norm)"""
    ref = z[name]
    t = t.detach().double().cpu()
    if not _is_probe(z, name):
        ref_t = torch.from_numpy(np.asarray(ref)).double().reshape(t.shape)
        den = ref_t.norm().item()
        return (t - ref_t).norm().item() / den if den > 0 else (t - ref_t).norm().item()
    p = detrand.probe(t, name.split("/")[-1])
    return float(np.abs(p - ref).max()) / max(abs(float(ref[1])), 1e-300)


def store(out, name, t):
    """fixture side of check_stored"""
    t = t.detach().double().cpu()
    if t.numel() <= FULL_MAX:
        out[name] = t.numpy()
    else:
        out[name] = detrand.probe(t, name.split("/")[-1])
        out.setdefault("probes", []).append(name)
