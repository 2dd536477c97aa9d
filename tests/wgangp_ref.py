"""Float64 references of the WGAN-GP gradient penalty on the StyleGAN2 discriminator, in plain torch on oracle/stylegan2.py's blocks; shared
by tests/test_wgangp_cpu.py and tests/test_wgangp_gpu.py (and tools/make_wgangp_golden.py for the interpolate).

  penalty_autograd            cal_gradient_penalty as the reference computes it (models/networks.py:548-580): autograd's double backward.
  penalty_forward_over_reverse  the form the HIP engine runs.  The discriminator is piecewise linear in its input and couples no samples,
      so at a fixed activation pattern D(x) = L(x; W) + (terms without x), with L the LINEARISED network: the same Blur / convolutions /
      linear layers without biases, every fused_leaky_relu replaced by the multiplication with its derivative at the saved
      pre-activation.  Then g = dD/dx = d sum L(x; W) / dx does not depend on x, P = lambda / N sum_n (||g_n + 1e-16|| - c)^2, v = dP/dg,
      and  dP/dW = d <v, g(W)> / dW = d sum L(v; W) / dW:  the ordinary FIRST-order weight gradient of the network evaluated on the
      tangent v under the backward signals of dout = 1.  No bias appears in L, so no bias receives a gradient.
"""
import math

import torch
import torch.nn.functional as F

from oracle import detrand
from oracle import stylegan2 as sg

EPS = 1e-16


def gp_inputs(case):
    """(real, fake, alpha) of a cal_gradient_penalty case dict(size, input_nc, n, seed): float32, from the seed (the fixture holds no inputs)"""
    shape = (int(case["n"]), int(case["input_nc"]), int(case["size"]), int(case["size"]))
    alpha = (detrand.uniform((shape[0],), int(case["seed"]), "gp_alpha") + 1.0) * 0.5
    return detrand.uniform(shape, int(case["seed"]), "gp_real"), detrand.uniform(shape, int(case["seed"]), "gp_fake"), alpha


def interpolate(real, fake, alpha):
    a = alpha.reshape(-1, 1, 1, 1).to(real.dtype)
    return a * real + (1 - a) * fake


def d_pass(sd, x, size, deriv=None):
    """deriv None: StyleGAN2Discriminator.forward (oracle.stylegan2.discriminator_forward), returns (out [N, 1], the derivative map of every
    fused_leaky_relu in call order).  deriv given: the linearised network L(x; W) at those maps, returns (out, [])."""
    sd = dict(sd)
    for k, v in sg.d_buffers(0, 0, size).items():
        sd[k] = v.to(x.dtype)
    rec, it = [], (iter(deriv) if deriv is not None else None)

    def act(z, b):
        if it is not None:
            return z * next(it)
        b = b.view(1, -1, *([1] * (z.ndim - 2)))
        rec.append(torch.where(z + b > 0, torch.ones_like(z), torch.full_like(z, 0.2)).detach() * sg.SQRT2)
        return F.leaky_relu(z + b, 0.2) * sg.SQRT2

    def conv(prefix, x, k, down, activate=True):
        i, stride, padding = 0, 1, k // 2
        if down:
            p = 2 + (k - 1)
            x = sg.upfirdn2d(x, sd[prefix + "0.kernel"], pad=((p + 1) // 2, p // 2))
            i, stride, padding = 1, 2, 0
        z = sg.equal_conv2d(x, sd[prefix + "%d.weight" % i], None, stride, padding)
        return act(z, sd[prefix + "%d.bias" % (i + 1)]) if activate else z

    out = conv("convs.0.", x, 1, False)
    for n in range(int(math.log2(size)) - 2):
        p = "convs.%d." % (n + 1)
        o = conv(p + "conv2.", conv(p + "conv1.", out, 3, False), 3, True)
        out = (o + conv(p + "skip.", out, 1, True, activate=False)) / sg.SQRT2
    out = conv("final_conv.", out, 3, False).reshape(x.shape[0], -1)
    w0, w1 = sd["final_linear.0.weight"], sd["final_linear.1.weight"]
    out = act(F.linear(out, w0 / math.sqrt(w0.shape[1])), sd["final_linear.0.bias"])
    out = F.linear(out, w1 / math.sqrt(w1.shape[1]), None if it is not None else sd["final_linear.1.bias"])
    return out, rec


def _params(sd, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if not k.endswith("kernel")}


def penalty_value(g, lambda_gp=10.0, constant=1.0):
    norms = (g.reshape(g.shape[0], -1) + EPS).norm(2, dim=1)
    return ((norms - constant) ** 2).mean() * lambda_gp, norms


def penalty_autograd(sd, xh, size, lambda_gp=10.0, constant=1.0, dtype=torch.float64):
    """(penalty, g, {parameter: gradient or None}) by double backward, as networks.py:573-580"""
    p = _params(sd, dtype)
    xh = xh.detach().to(dtype).requires_grad_(True)
    y = sg.discriminator_forward(dict(p, **{k: v.to(dtype) for k, v in sg.d_buffers(0, 0, size).items()}), xh, size)
    g, = torch.autograd.grad(y, xh, grad_outputs=torch.ones_like(y), create_graph=True, retain_graph=True)
    pen, norms = penalty_value(g, lambda_gp, constant)
    grads = torch.autograd.grad(pen, list(p.values()), allow_unused=True)
    return pen.detach(), g.detach(), dict(zip(p, grads)), norms.detach()


def penalty_forward_over_reverse(sd, xh, size, lambda_gp=10.0, constant=1.0, dtype=torch.float64):
    """(penalty, g, {weight: gradient}; the biases are absent) with first-order passes only"""
    p = _params(sd, dtype)
    xh = xh.detach().to(dtype)
    with torch.no_grad():
        _, deriv = d_pass(p, xh, size)                                   # forward: the activation pattern
    x0 = torch.zeros_like(xh).requires_grad_(True)
    g, = torch.autograd.grad(d_pass(p, x0, size, deriv)[0].sum(), x0)    # backward of dout = 1 to the input
    n = g.shape[0]
    pen, norms = penalty_value(g, lambda_gp, constant)
    v = ((2.0 * lambda_gp / n) * (norms - constant) / norms).view(n, 1, 1, 1) * (g + EPS)     # dP/dg
    weights = {k: t for k, t in p.items() if k.endswith("weight")}
    grads = torch.autograd.grad(d_pass(p, v.detach(), size, deriv)[0].sum(), list(weights.values()))   # tangent forward + backward of dout = 1
    return pen.detach(), g.detach(), dict(zip(weights, grads)), norms.detach()
