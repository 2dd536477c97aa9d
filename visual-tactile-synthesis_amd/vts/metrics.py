"""Evaluation metrics of the baselines (pix2pix, SPADE, pix2pixHD) on a batch: the reference's compute_evaluation_metric
(models/model_utils.py:431-561), called by all three models on real_I / fake_I / real_T / fake_T of the current batch
(pix2pix_model.py:574-587, spade_model.py:808-, pix2pixHD_model.py:826-).

`evaluate` is the shared arithmetic; `model_metrics` is what a model's compute_metrics() calls: the gating of the optional networks, the
two input contracts and the metric_* attributes.  Everything per pair runs in batched launches (engine.sifid_pairs_batched,
engine.tactile_patch_fid -> ops.frechet_distance_batched).
"""
import os

import numpy as np
import torch

from . import engine, ops

# the reference's eval_metrics of the three baselines, in its order (pix2pix_model.py:211); T_FID (model_utils.py:534-536) is known to
# compute_evaluation_metric but in none of upstream's lists: it is reported last, on request (--eval_T_FID)
EVAL_METRICS = ["I_SIFID", "I_LPIPS", "I_PSNR", "I_SSIM", "T_SIFID", "T_LPIPS", "T_AE", "T_MSE"]


def metric_name_list(train_for_each_epoch, edited=False, names=EVAL_METRICS):
    """the reference's metric_names (pix2pix_model.py:210-223): the metrics, then the same with 'train_' when train_for_each_epoch"""
    if edited:
        return []
    return [p + m for p in ([""] + (["train_"] if train_for_each_epoch else [])) for m in names]


def add_metric_flags(parser):
    """the flags of the optional metric networks (none is a reference flag: upstream downloads the weights) on a baseline's parser"""
    have = {s for a in parser._actions for s in a.option_strings}
    for name in ("inception_weights", "lpips_weights", "lpips_alex_weights"):
        if "--" + name not in have:
            parser.add_argument("--" + name, type=str, default="")
    if "--eval_T_FID" not in have:
        parser.add_argument("--eval_T_FID", action="store_true", default=False)
    return parser


def lpips_check_size(h, w, backbone):
    """raise with the reason when an LPIPS backbone cannot run on h x w images instead of launching on a size a kernel refuses"""
    if backbone == "alex":
        # conv0 11 x 11 / 4, padding 2 -> MaxPool(3, 2) -> conv1 -> MaxPool(3, 2) -> conv2-4: vts_maxpool3s2_relu_pad refuses maps below 3 x 3
        o = [(s + 4 - 11) // 4 + 1 for s in (h, w)]
        p1 = [(s - 3) // 2 + 1 for s in o]
        p2 = [(s - 3) // 2 + 1 for s in p1]
        if min(h, w) < 11 or min(o) < 3 or min(p1) < 3 or min(p2) < 1:
            raise ValueError("LPIPS (alex) on %d x %d images: the AlexNet stack (11 x 11 / 4 convolution, two 3 x 3 / 2 max-pools) needs a 3 x 3 "
                             "map in front of each pool, i.e. images of at least 31 x 31" % (h, w))
    else:
        if min(h, w) < 16:
            raise ValueError("LPIPS (vgg) on %d x %d images: vts_maxpool2_relu_pad refuses maps below 2 x 2 and the stack has four pools, i.e. "
                             "images of at least 16 x 16 are needed" % (h, w))


def evaluate(real_I, fake_I, real_T, fake_T, sifid_net=None, lpips_net=None, lpips_backbone="vgg", want_tfid=False):
    """The metrics of one batch: real_I / fake_I [N, 3, H, W], real_T / fake_T [P, 2, h, w] (device, contiguous).  Returns an ordered
    {name: float} in the reference's order; I_SIFID / T_SIFID need sifid_net (models/inception.py), I_LPIPS / T_LPIPS need lpips_net
    (VGG16 or AlexNet LPIPS of models/perceptual.py, lpips_backbone says which), T_FID is added last when want_tfid."""
    real_I, fake_I, real_T, fake_T = (t.contiguous() for t in (real_I, fake_I, real_T, fake_T))
    if real_T.shape != fake_T.shape:
        raise ValueError("tactile patches: real %s against fake %s" % (tuple(real_T.shape), tuple(fake_T.shape)))
    P = real_T.shape[0]
    dev = real_I.device
    if lpips_net is not None:
        lpips_check_size(real_I.shape[2], real_I.shape[3], lpips_backbone)
    base = ops.eval_metrics(real_I, fake_I, real_T, fake_T)       # [I_PSNR, T_AE, T_MSE, I_SSIM]
    extra = {}
    if sifid_net is not None:
        extra["I_SIFID"] = engine.sifid_images_batched(sifid_net, real_I, fake_I)
        extra["T_SIFID"] = engine.sifid_tactile_batched(sifid_net, real_T, fake_T)
    if want_tfid:
        extra["T_FID"] = engine.tactile_patch_fid(real_T, fake_T, "none")
    lv = None
    if lpips_net is not None:
        from . import perceptual as P_
        buf = ops.loss_slots(2, dev)
        if lpips_backbone == "alex":
            term = lambda a, b, coeff, slot: P_.lpips_alex_value(lpips_net, a, b, coeff, slot)      # noqa: E731
        else:
            term = lambda a, b, coeff, slot: P_.lpips_term(lpips_net, a, b, coeff, slot)            # noqa: E731
        n_img = real_I.shape[0]
        for i0 in range(0, n_img, 32):
            term(real_I[i0:i0 + 32], fake_I[i0:i0 + 32], 1.0 / n_img, buf[0:1])
        for c in (0, 1):     # nearest resize to 224 x 224, fake clamped to [0, 1], each channel tiled to three; mean over patches, gx + gy
            a = ops.sifid_input(real_T, c, 1, size=(224, 224))
            b = ops.sifid_input(fake_T, c, 1, size=(224, 224), clamp01=True)
            for i0 in range(0, P, 32):
                term(a[i0:i0 + 32], b[i0:i0 + 32], 1.0 / P, buf[1:2])
        lv = ops.loss_values(buf)
    keys = list(extra)
    host = torch.cat([base] + [extra[k].reshape(1) for k in keys]).cpu().tolist()       # the one device -> host copy of the values
    vals = dict(zip(["I_PSNR", "T_AE", "T_MSE", "I_SSIM"] + keys, host))
    if lv is not None:
        vals["I_LPIPS"], vals["T_LPIPS"] = lv[0], lv[1]
    return {k: vals[k] for k in EVAL_METRICS + ["T_FID"] if k in vals}


def _patch_offsets(coords):
    """find_coords_for_patch (models/model_utils.py:23-69) on the host for all samples: int32 (offx, offy, cutout), flattened"""
    c = np.asarray(coords, dtype=np.float64)
    ox = np.round(c[..., 0] + c[..., -2] / c[..., -3])
    oy = np.round(c[..., 1] + c[..., -1] / c[..., -3])
    cs = np.round(c[..., -4] / c[..., -3])
    to_i = lambda a: np.ascontiguousarray(a.astype(np.float32).astype(np.int32).reshape(-1))      # noqa: E731
    return to_i(ox), to_i(oy), to_i(cs)


def gather_fake_patches(fake_T, T_coords, size):
    """full-image contract: the fake tactile patches [N * NT, 2, size, size] cut from fake_T [N, 2, H, W] at T_coords [N, NT, 8] with the
    patch gather of sinskitG (ops.patch_gather; find_coords_for_patch + get_patch_in_input, model_utils.py:23-69, 252-333)"""
    coords = torch.as_tensor(T_coords).numpy()
    n = fake_T.shape[0]
    ox, oy, cs = _patch_offsets(coords.reshape(n, -1, 8))
    if not (cs == size).all():
        raise NotImplementedError("patch cutout != %d px (resize_ratio != 1): the resampling branch of get_patch_in_input is not wired" % size)
    nt = ox.size // n
    dev = fake_T.device
    img = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int32), nt)).to(dev)
    out = torch.empty(n * nt, 2, size, size, dtype=torch.float32, device=dev)
    return ops.patch_gather(fake_T, img, torch.from_numpy(ox).to(dev), torch.from_numpy(oy).to(dev), size, out, c0=0, channels=2)


def _nets(model):
    """(sifid_net, lpips_net, backbone) of a baseline under sinskitG's gating: SIFID with --inception_weights or VTS_SIFID=1; LPIPS with the
    weight flag of the phase or VTS_LPIPS_METRICS=1 -- VGG16 while training, AlexNet in the test phase (pix2pix_model.py:230-233)"""
    opt = model.opt
    if not hasattr(model, "_inception"):
        model._inception = None
        if getattr(opt, "inception_weights", "") or os.environ.get("VTS_SIFID", "0") == "1":
            from models import inception
            model._inception = inception.build(opt, model.device)
    backbone = "vgg" if model.isTrain else "alex"
    flag = getattr(opt, "lpips_weights", "") if model.isTrain else getattr(opt, "lpips_alex_weights", "")
    lp = None
    if flag or os.environ.get("VTS_LPIPS_METRICS", "0") == "1":
        lp = getattr(model, "_metric_lpips_" + backbone, None)
        if lp is None:
            from models import perceptual
            lp = (perceptual.build_lpips if backbone == "vgg" else perceptual.build_lpips_alex)(opt, model.device)
            setattr(model, "_metric_lpips_" + backbone, lp)
    return model._inception, lp, backbone


def model_metrics(model, prefix=""):
    """compute_metrics() of a baseline: the metrics of the outputs of its last forward() / test(), set as metric_<prefix><name> and
    listed in metric_names (in the reference's order); {} for edited sketches, which upstream skips.
    Patch contract (return_patch): exactly the reference's call, on real_T / fake_T as they are.  Full images: the reference's call fails
    there (real_T is [N * NT, 2, h, w], fake_T [N, 2, H, W]); I_* are computed as upstream and T_* on the fake patches gathered at
    T_coords, as sinskitG does -- metric_T_contract says which."""
    if model.test_edit_S or not hasattr(model, "real_I") or not hasattr(model, "fake_I"):
        return {}
    real_T, fake_T = model.real_T, model.fake_T
    if tuple(real_T.shape) == tuple(fake_T.shape):
        model.metric_T_contract = "patch"
    else:
        coords = getattr(model, "T_coords", None)
        if coords is None or real_T.shape[2] != real_T.shape[3]:
            raise ValueError("tactile patches %s against the generator's output %s: the full-image contract needs T_coords and square patches"
                             % (tuple(real_T.shape), tuple(fake_T.shape)))
        fake_T = gather_fake_patches(fake_T, coords, real_T.shape[2])
        model.metric_T_contract = "gathered"
    sifid_net, lpips_net, backbone = _nets(model)
    vals = evaluate(model.real_I, model.fake_I, real_T, fake_T, sifid_net=sifid_net, lpips_net=lpips_net, lpips_backbone=backbone,
                    want_tfid=bool(getattr(model.opt, "eval_T_FID", False)))
    if sifid_net is not None:
        model.metric_sifid_pretrained = bool(sifid_net.pretrained)
    if lpips_net is not None:
        model.metric_lpips_pretrained, model.metric_lpips_backbone = bool(lpips_net.pretrained), backbone
    # I_SSIM: torchmetrics cannot be run here -- the kernel is pinned to a restatement of its published algorithm (oracle/nets.py:ssim)
    model.metric_ssim_pinned = "restatement"
    for name, v in vals.items():
        setattr(model, "metric_%s%s" % (prefix, name), v)
        if prefix + name not in model.metric_names:
            model.metric_names.append(prefix + name)
    order = EVAL_METRICS + ["T_FID"]      # the reference lists the plain names first, then the 'train_' ones (pix2pix_model.py:213-223)
    model.metric_names.sort(key=lambda m: (m.startswith("train_"), order.index(m[6:] if m.startswith("train_") else m)))
    return {prefix + n: v for n, v in vals.items()}
