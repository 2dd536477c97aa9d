"""Layer times of the classic pix2pix U-Net (--netG unet_256) at ngf 64: every layer with >= 64 channels on both sides, at 1024 x 1024
batch 1 and 256 x 256 batch 4, each as 20 launches in one HIP graph (tools/mb_px.py:timeit).  Per layer and role the GEMM-class route
engine.unet_classic_forward / _backward takes above 80 output channels (padding pass + kernel, and the kernel alone) against the 4 x 4
kernels' 80-channel group loop on the same shape (vts_conv4x4, operands on load) -- what a tree without the wide route would run -- and the
route the engine takes.  Also the weight gradient of the transposed layers on full-size maps: vts_wgrad4x4_wide with swapped roles against
vts_wgrad4x4.

  python tools/mb_unet_classic_layers.py            (profiles/r24_unet_classic.md holds the MI355X table)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-tactile-synthesis_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from vts import lib as L, ops  # noqa: E402
from vts.ops import Act  # noqa: E402
from mb_px import timeit  # noqa: E402

dev = torch.device("cuda:0")
RELU, LRELU = L.ACT_RELU, L.ACT_LRELU


def kern():
    return L.load().vts_last_kernel().decode()


def up_forward(n, cin, cout, h, w):
    """ConvTranspose2d(4, 2, 1) cin -> cout on an h x w map: new member vs the group loop"""
    x, wt = torch.randn(n, cin, h, w, device=dev), torch.randn(cin, cout, 4, 4, device=dev) * 0.05
    out = torch.empty(n, cout, 2 * h, 2 * w, device=dev)
    a = Act(x, torch.ones(n * cin, device=dev), torch.zeros(n * cin, device=dev))
    p = ops.pad_affine(a, (1, 1, 1, 1), 0, act=RELU)
    packed = ops.w4x4_pack(wt, "convT_fwd")
    t_k = timeit(lambda: ops.tconv4x4s2p1_wide(p, packed, None, out))
    k_new = kern()
    t_pk = timeit(lambda: (ops.pad_affine(a, (1, 1, 1, 1), 0, out=p, act=RELU), ops.tconv4x4s2p1_wide(p, packed, None, out)))
    t_old = timeit(lambda: ops.conv4x4(a, wt, 16, cout * 16, cout, out, stride=2, pad=1, transposed=True, act_in=RELU))
    return t_k, t_pk, t_old, k_new, kern()


def down_forward(n, cin, cout, h, w):
    """Conv2d(4, 2, 1) cin -> cout on an h x w map: vts_conv4x4_wide(stride 2) vs the group loop"""
    x, wt = torch.randn(n, cin, h, w, device=dev), torch.randn(cout, cin, 4, 4, device=dev) * 0.05
    out = torch.empty(n, cout, h // 2, w // 2, device=dev)
    a = Act(x, torch.ones(n * cin, device=dev), torch.zeros(n * cin, device=dev))
    p = ops.pad_affine(a, (1, 1, 1, 1), 0, act=LRELU)
    packed = ops.w4x4_pack(wt, "conv_fwd")
    t_k = timeit(lambda: ops.conv4x4_wide(p, packed, None, out, stride=2))
    k_new = kern()
    t_pk = timeit(lambda: (ops.pad_affine(a, (1, 1, 1, 1), 0, out=p, act=LRELU), ops.conv4x4_wide(p, packed, None, out, stride=2)))
    t_old = timeit(lambda: ops.conv4x4(a, wt, cin * 16, 16, cout, out, stride=2, pad=1, act_in=LRELU))
    return t_k, t_pk, t_old, k_new, kern()


def down_adjoint(n, cin, cout, h, w):
    """input adjoint of Conv2d(4, 2, 1) cin -> cout (h x w input map): new member + vts_act_bwd vs the group loop with its mask on store"""
    g, wt = torch.randn(n, cout, h // 2, w // 2, device=dev), torch.randn(cout, cin, 4, 4, device=dev) * 0.05
    prev = Act(torch.randn(n, cin, h, w, device=dev))
    raw, tgt = torch.empty(n, cin, h, w, device=dev), torch.empty(n, cin, h, w, device=dev)
    q = ops.pad_affine(g, (1, 1, 1, 1), 0)
    packed = ops.w4x4_pack(wt, "conv_s2_adj")
    t_k = timeit(lambda: ops.tconv4x4s2p1_wide(q, packed, None, raw))
    k_new = kern()
    t_pk = timeit(lambda: (ops.pad_affine(g, (1, 1, 1, 1), 0, out=q), ops.tconv4x4s2p1_wide(q, packed, None, raw), ops.act_bwd(raw, prev, LRELU, tgt)))
    t_old = timeit(lambda: ops.conv4x4(Act(g), wt, 16, cin * 16, cin, tgt, stride=2, pad=1, transposed=True, dmask=prev, dmask_act=LRELU))
    return t_k, t_pk, t_old, k_new, kern()


def up_adjoint(n, c, cout, h, w):
    """input adjoint of ConvTranspose2d(4, 2, 1) w.r.t. ONE concat source of c channels (h x w map): vts_conv4x4_wide(stride 2) + vts_act_bwd"""
    g, wt = torch.randn(n, cout, 2 * h, 2 * w, device=dev), torch.randn(c, cout, 4, 4, device=dev) * 0.05
    src = Act(torch.randn(n, c, h, w, device=dev))
    raw, tgt = torch.empty(n, c, h, w, device=dev), torch.empty(n, c, h, w, device=dev)
    q = ops.pad_affine(g, (1, 1, 1, 1), 0)
    packed = ops.w4x4_pack(wt, "convT_adj")
    t_k = timeit(lambda: ops.conv4x4_wide(q, packed, None, raw, stride=2))
    k_new = kern()
    t_pk = timeit(lambda: (ops.pad_affine(g, (1, 1, 1, 1), 0, out=q), ops.conv4x4_wide(q, packed, None, raw, stride=2), ops.act_bwd(raw, src, RELU, tgt)))
    t_old = timeit(lambda: ops.conv4x4(Act(g), wt, cout * 16, 16, c, tgt, stride=2, pad=1, dmask=src, dmask_act=RELU))
    return t_k, t_pk, t_old, k_new, kern()


def up_wgrad(n, cin, cout, h, w):
    """weight gradient of ConvTranspose2d(4, 2, 1) cin -> cout (h x w input map): vts_wgrad4x4_wide with the roles swapped (the activated
    input as `dout`, the gradient padded by one as `p`; both materialised by vts_pad_affine) against vts_wgrad4x4 with operands on load,
    which is what the engine runs"""
    x, g = torch.randn(n, cin, h, w, device=dev), torch.randn(n, cout, 2 * h, 2 * w, device=dev)
    a = Act(x, torch.ones(n * cin, device=dev), torch.zeros(n * cin, device=dev))
    dw = torch.empty(cin, cout, 4, 4, device=dev)
    xa, q = ops.pad_affine(a, (0, 0, 0, 0), 0, act=RELU), ops.pad_affine(g, (1, 1, 1, 1), 0)
    t_k = timeit(lambda: ops.wgrad4x4_wide(xa, q, dw, stride=2))
    k_new = kern()
    t_pk = timeit(lambda: (ops.pad_affine(a, (0, 0, 0, 0), 0, out=xa, act=RELU), ops.pad_affine(g, (1, 1, 1, 1), 0, out=q), ops.wgrad4x4_wide(xa, q, dw, stride=2)))
    t_old = timeit(lambda: ops.wgrad4x4(a, Act(g), dw, act_lo=RELU, stride=2, pad=1, defer=False))
    return t_k, t_pk, t_old, k_new, kern()


def route(role, args):
    """what engine.unet_classic_forward / _backward run for this launch"""
    from vts import engine
    n, a, b, h, w = args
    if role == "forward-down":
        return "wide" if engine._uc_wide(b) else "4x4"
    if role == "adjoint-up":
        return "wide" if engine._uc_wide(a) else "4x4"
    if role == "forward-up":
        return "wide" if engine._uc_tconv_wide(b, n, h, w) else "4x4"
    if role == "adjoint-down":
        return "wide" if engine._uc_tconv_wide(a, n, h // 2, w // 2) else "4x4"
    return "4x4"


if __name__ == "__main__":
    ngf, nd = 64, 8
    ch = [ngf * min(2 ** i, 8) for i in range(nd)]
    print("| size | layer | role | shape | wide kernel us | wide + pad (+ mask) us | 4x4 kernels us | engine runs | wide instance | 4x4 instance |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for size, n in ((1024, 1), (256, 4)):
        rows = []
        for i in range(1, nd):
            h = size >> i          # input map of down<i>
            rows.append(("down%d" % i, "forward-down", down_forward, (n, ch[i - 1], ch[i], h, h)))
            rows.append(("down%d" % i, "adjoint-down", down_adjoint, (n, ch[i - 1], ch[i], h, h)))
        for i in range(nd - 1, 0, -1):
            h = size >> (i + 1)    # input map of up<i>
            cin = ch[i] * (1 if i == nd - 1 else 2)
            rows.append(("up%d" % i, "forward-up", up_forward, (n, cin, ch[i - 1], h, h)))
            rows.append(("up%d" % i, "adjoint-up", up_adjoint, (n, ch[i], ch[i - 1], h, h)))
            if h * h > 128:        # (vts_wgrad4x4_wide is the full-size form; small maps stay on vts_wgrad4x4 as in the PatchGAN backward)
                rows.append(("up%d" % i, "wgrad-up", up_wgrad, (n, cin, ch[i - 1], h, h)))
        for layer, role, fn, args in rows:
            t_k, t_pk, t_old, k_new, k_old = fn(*args)
            print("| %d^2 N%d | %s | %s | %d -> %d @ %dx%d | %.1f | %.1f | %.1f | %s | %s | %s |" % (
                size, n, layer, role, args[1], args[2], args[3], args[4], t_k, t_pk, t_old, route(role, args), k_new, k_old), flush=True)
            torch.cuda.empty_cache()
