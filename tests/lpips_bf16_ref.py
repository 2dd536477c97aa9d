"""CPU helpers of the bf16 LPIPS tests (tests/test_lpips_bf16_cpu.py, tests/test_lpips_bf16_gpu.py).  Checker only.

  rt_bf16          round to nearest even onto the bf16 grid, in float64 (no double rounding through fp32)
  lpips_run        oracle/perceptual.py's VGG16 + LPIPS head evaluated in float64 with a hand-written backward, every quantity the bf16 path
                   STORES AS bf16 passed through `q`:
                       every convolution's input and weights, forward and adjoint (the scaled input image, the weights),
                       every stored activation (relu(conv + bias)), every tap gradient, every gradient map an adjoint or a pooling adjoint writes.
                   q = rt_bf16 is the "ideal bf16 run"; q = identity is the plain float64 oracle (test_lpips_bf16_cpu.py pins that against
                   autograd on oracle.perceptual.LPIPS to 1e-12).  Biases, the LPIPS arithmetic, the pooling (a selection) and the final
                   input gradient stay float64.
  conv_judge       float64 reference, absref and the derived bound of one vts_conv3x3_bf16 launch
  lpips_layer_judge  the same for vts_lpips_layer_bf16 (it lives in oracle/launch_ref.py, beside the judges of the fp32 head)
"""
import math

import torch
import torch.nn.functional as F

from oracle.launch_ref import lpips_layer_judge  # noqa: F401  (the bf16 tests call it as R.lpips_layer_judge)

U = 2.0 ** -24          # fp32 unit roundoff
UB = 2.0 ** -8          # bf16: 8 significant bits, so half an ulp is at most 2^-8 of the value
BF16_NAN_BITS = 0x7FC0


def rt_bf16(x):
    """x (any float dtype) rounded to the nearest bf16 value, ties to even, subnormals kept (ulp 2^-133); returned in x's dtype"""
    d = x.detach().to(torch.float64)
    _, e = torch.frexp(d)                                   # |d| = m 2^e, m in [0.5, 1): the 8-bit significand has ulp 2^(e - 8)
    ulp = torch.exp2(torch.clamp(e - 8, min=-133).to(torch.float64))
    r = torch.round(d / ulp) * ulp                          # torch.round: half to even; the scaling by a power of two is exact
    r = torch.where(r.abs() > 3.3895313892515355e38, torch.sign(r) * math.inf, r)
    r = torch.where(torch.isfinite(d), r, d)
    return r.to(x.dtype)


def ident(x):
    return x


def to_bits(x):
    """int16 bit patterns of a tensor of bf16-exact values"""
    b = x.to(torch.float32).to(torch.bfloat16)
    assert torch.equal(b.to(torch.float64), x.to(torch.float64)), "not bf16-exact"
    return b.view(torch.int16)


def from_bits(b):
    return b.contiguous().view(torch.bfloat16).to(torch.float64)


def nhwc_pad(x):
    """[N, C, H, W] -> [N, H + 2, W + 2, C] with a zero border"""
    return F.pad(x, (1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous()


def interior_nchw(p):
    return p[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).contiguous()


def conv_judge(x, w, bias=None, add=None):
    """x [N, Ci, H, W], w [Co, Ci, 3, 3] (bf16-exact, float64), bias [Co] / add [N, Co, H, W] or None.  Returns (y64, bound_fp32):
    y64 = conv + bias + add; bound_fp32 = (9 Cin + 2) 2^-24 absref with absref = sum |x w| + |bias| + |add|: the project's linear rounding
    count (bf16 products are exact in fp32; each of the 9 Cin terms passes through at most 9 Cin additions, + the bias / add and one more)."""
    y = F.conv2d(x, w, None, padding=1)
    a = F.conv2d(x.abs(), w.abs(), None, padding=1)
    if bias is not None:
        y, a = y + bias.view(1, -1, 1, 1), a + bias.abs().view(1, -1, 1, 1)
    if add is not None:
        y, a = y + add, a + add.abs()
    return y, (9 * x.shape[1] + 2) * U * a


def ratio(got, ref, bound):
    """worst |got - ref| / bound; where the bound is 0 (an exact zero) the value must be exact; non-finite results are infinitely wrong"""
    got, ref, bound = got.reshape(-1).double(), ref.reshape(-1).double(), bound.reshape(-1).double()
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    return float(r.max())


# ---- the LPIPS head of one tap: oracle/launch_ref.py:lpips_layer_judge (imported above; the fp32 head of csrc/vts_perceptual.hip is judged by it too)


# ---- the whole term ---------------------------------------------------------------------------------------------------------------------------
def _layout(cfg):
    out, k, pool = [], 0, False
    for v in cfg:
        if v == "M":
            pool = True
        else:
            out.append((k, pool))
            pool = False
            k += 1
    return out


def lpips_run(lp, fake, real, coeff, q=ident, channels=None, want_grad=True):
    """(value, d value / d fake) of coeff * sum_n LPIPS(fake_n, real_n) on the oracle module `lp` (oracle.perceptual.LPIPS, VGG variant), in
    float64, with `q` applied to everything the bf16 path stores as bf16 (module docstring).  fake / real [N, 3 | 1, H, W]."""
    net = lp.net
    taps = net.taps
    lay = [e for e in _layout(net.cfg) if e[0] <= max(taps)]
    W = [q(m.weight.detach().double()) for m in net.convs]
    B = [m.bias.detach().double() for m in net.convs]
    lins = [p.detach().double().view(-1) for p in lp.lins]
    shift, scale = lp.shift.double(), lp.scale.double()
    n = fake.shape[0]
    x = torch.cat([fake, real], 0).double()
    x = q((x - shift) / scale)                              # the ScalingLayer broadcasts one channel to three
    acts, pools = {}, {}
    prev = x
    for k, pooled in lay:
        if pooled:
            prev = F.max_pool2d(prev, 2, 2)
            pools[k] = prev
        prev = q(F.relu(F.conv2d(prev, W[k], B[k], padding=1)))
        acts[k] = prev
    value = torch.zeros((), dtype=torch.float64)
    tg = {}
    eps = 1e-10
    for i, k in enumerate(taps):
        f0, f1 = acts[k][:n], acts[k][n:]
        hw = f0.shape[2] * f0.shape[3]
        wv = lins[i].view(1, -1, 1, 1)
        r0, r1 = f0.pow(2).sum(1, keepdim=True).sqrt(), f1.pow(2).sum(1, keepdim=True).sqrt()
        i0, i1 = 1.0 / (r0 + eps), 1.0 / (r1 + eps)
        t = f0 * i0 - f1 * i1
        value = value + coeff / hw * (wv * t * t).sum()
        S = (wv * t * f0).sum(1, keepdim=True)
        k2 = torch.where(r0 > 0, S * i0 * i0 / torch.where(r0 > 0, r0, torch.ones_like(r0)), torch.zeros_like(r0))
        if want_grad:
            g = 2.0 * coeff / hw * (i0 * wv * t - k2 * f0)
            tg[k] = q(torch.where(f0 > 0, g, torch.zeros_like(g)))
    if not want_grad:
        return float(value), None
    G = None
    top = max(taps)
    for idx in range(len(lay) - 1, 0, -1):
        k, pooled = lay[idx]
        if k > top:
            continue
        if k == top:
            G = tg[k]
        kf = lay[idx - 1][0]
        ft = acts[kf][:n]
        T = tg.get(kf)
        gin = F.conv_transpose2d(G, W[k], None, padding=1)         # the input adjoint: taps flipped, channels swapped
        if pooled:
            pm = pools[k][:n]
            gin = q(torch.where(pm > 0, gin, torch.zeros_like(gin)))
            _, ind = F.max_pool2d(ft, 2, 2, return_indices=True)    # the first maximum of a window in row-major order
            routed = F.max_unpool2d(gin, ind, 2, 2, output_size=ft.shape[2:])
            if T is not None:
                routed = routed + T                                 # T carries the ReLU mask already
            G = q(routed)
        else:
            if T is not None:
                gin = gin + T
            G = q(torch.where(ft > 0, gin, torch.zeros_like(gin)))
    dx = F.conv_transpose2d(G, W[0], None, padding=1) / scale
    cx = fake.shape[1] if channels is None else channels
    if cx == 1:
        dx = dx.sum(1, keepdim=True)
    return float(value), dx


def oracle_autograd(lp, fake, real, coeff):
    """the plain oracle: autograd through oracle.perceptual.LPIPS in float64"""
    lp = lp.double()
    a = fake.double().clone().requires_grad_(True)
    v = coeff * lp(a, real.double()).sum()
    v.backward()
    return float(v.detach()), a.grad


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- the cases of the whole-term GPU test ----
NET_SEED = 20180111        # models/perceptual.py:LpipsVgg16.SEED, the seeded stand-in weights

# seed: the first of 0 .. 9 whose ideal-run gradient error lies within a factor two of the median over those seeds (computed on the CPU:
# tests/test_lpips_bf16_cpu.py:test_whole_term_seed_selection recomputes it), as tests/style_levels_cases.py picks its own
TERM_CASES = {
    "image": {"shape": (2, 3, 64, 64), "scale": 1.0, "channels": None, "coeff": 0.5, "seed": 0},
    "patches": {"shape": (8, 2, 32, 32), "scale": 0.3, "channels": 1, "coeff": 10.0, "seed": 0},
}


def term_inputs(case, seed):
    """(fake, real) as the term sees them: the image pair, or channel 0 of a [8, 2, 32, 32] patch stack as 8 one-channel patches"""
    g = torch.Generator().manual_seed(4000 + seed)
    a = case["scale"] * (2 * torch.rand(case["shape"], generator=g) - 1)
    b = case["scale"] * (2 * torch.rand(case["shape"], generator=g) - 1)
    if case["channels"] == 1:
        return a[:, 0:1], b[:, 0:1]
    return a, b
