"""pix2pix baseline on the HIP path (reference: models/pix2pix_model.py).

The reference trains this baseline patch-wise like the other two (`return_patch=True`: 32x32 sketch / image / tactile patches, batch 32)
with the ResNet generator under BatchNorm (`resnet_9blocks`; the 32-pixel patches are too small for the U-Net of the paper), two single
PatchGAN discriminators (`define_D('basic' | 'n_layers')`; D: sketch ++ image, D2: sketch ++ tactile) and the GAN + L1 objective:

    forward             pix2pix_model.py:369-389     G(S) -> fake_I = out[:, :3] * M, fake_T = out[:, -2:] * M_T
    backward_D          :391-422                     0.5 (D_fake + D_real) + 0.5 (D2_fake + D2_real); fake and real are SEPARATE passes
    backward_G          :424-446                     G_GAN_I + G_GAN_T (through the updated discriminators) + lambda_L1 (L1_I + L1_T)
    optimize_parameters :448-470                     ONE generator forward, D and D2 step, then G step

The discriminators return one tensor, and the reference's GANLoss takes `input[-1]` of what it is given (networks.py:536-542): of a tensor
[N, 1, h, w] that is the map of the LAST SAMPLE.  Every GAN term of this model is therefore the loss of the batch's last prediction map
(the other samples still reach it through the BatchNorm statistics); networks.GANLossLastSample restates that.
Optimisers: G and D at `lr` with betas (beta1, 0.999), D2 at `lr_G2` with (beta1, beta2) (:281-286); the schedulers are BaseModel's.
"""
import os

import torch

from vts.misc import str2bool
from vts import engine, metrics, ops
from vts.ops import Act
from vts.optim import FlatAdam, FlatParams

from . import networks
from .base_model import BaseModel
from .sinskitG_model import add_model_flags

B = str2bool

# (flag, type, default)  -- reference: pix2pix_model.py:54-132
MODEL_FLAGS = [
    ("lambda_L1", float, 100.0), ("lr_G2", float, 0.0005), ("sketch_nc", int, 1), ("image_nc", int, 3), ("touch_nc", int, 2),
    ("data_len", int, 200), ("center_w", int, 1280), ("center_h", int, 960), ("num_touch_patch_for_logging", int, 10),
    ("use_bg_mask", B, True), ("T_resolution_multiplier", int, 1), ("padded_size", int, 1800), ("sample_bbox_per_patch", int, 2),
    ("save_S_patch", B, False), ("save_T_concat_tensor", B, False), ("save_raw_arr_vis", B, False), ("scale_nz", float, 0.25),
    ("return_patch", B, False),
]

LOSS_SLOTS = ["G_GAN", "G_L1", "D_real", "D_fake", "D2_real", "D2_fake", "G_GAN_I", "G_GAN_T"]
RESNETS = ("resnet_6blocks", "resnet_9blocks")
PATCHGANS = ("basic", "n_layers")


class Pix2PixModel(BaseModel):
    @staticmethod
    def modify_commandline_options(parser, is_train=True):
        add_model_flags(parser, MODEL_FLAGS)
        parser.add_argument("--use_hip_graph", type=B, default=True)   # not a reference flag: replay captured HIP graphs
        # not reference flags: weight files of the optional metric networks (upstream downloads them) and --eval_T_FID (T_FID is known to
        # compute_evaluation_metric but in none of upstream's metric lists)
        metrics.add_metric_flags(parser)
        parser.set_defaults(norm="batch", netG="resnet_9blocks", dataset_mode="aligned", dataset="patchskit", crop_size=1536)
        verbose_freq = 320
        if is_train:
            parser.set_defaults(pool_size=0, gan_mode="vanilla", return_patch=True, batch_size=32, display_freq=verbose_freq,
                                print_freq=verbose_freq, save_latest_freq=verbose_freq, validation_freq=verbose_freq, save_epoch_freq=50,
                                display_id=0, save_raw_arr_vis=False)
        else:
            parser.set_defaults(return_patch=False, batch_size=1, save_S_patch=True, save_raw_arr_vis=False, sample_bbox_per_patch=1,
                                data_len=1)
        return parser

    def __init__(self, opt):
        BaseModel.__init__(self, opt)
        if not self.gpu_ids or not torch.cuda.is_available():
            raise RuntimeError("Pix2PixModel runs on the MI355X HIP path only (no CPU fallback): pass --gpu_ids 0 on a GPU box")
        self._check_unbuilt(opt)
        self.test_edit_S = "edit" in opt.dataroot
        self.loss_names, self.visual_names, self.model_names = self.name_lists(opt)
        self.netG = networks.define_G(opt.sketch_nc, opt.image_nc + opt.touch_nc, opt.ngf, opt.netG, opt.norm, not opt.no_dropout,
                                      opt.init_type, opt.init_gain, opt.no_antialias, opt.no_antialias_up, self.gpu_ids, opt)
        self.flatG = FlatParams(self.netG)
        if self.isTrain:
            self.criterionGAN = networks.GANLossLastSample(opt.gan_mode)
            self.netD = networks.define_D(opt.image_nc + opt.sketch_nc, opt.ndf, opt.netD, opt.n_layers_D, opt.norm, opt.init_type,
                                          opt.init_gain, opt.no_antialias, gpu_ids=self.gpu_ids, opt=opt)
            self.netD2 = networks.define_D(opt.touch_nc + opt.sketch_nc, opt.ndf, opt.netD, opt.n_layers_D, opt.norm, opt.init_type,
                                           opt.init_gain, opt.no_antialias, gpu_ids=self.gpu_ids, opt=opt)
            self.flatD, self.flatD2 = FlatParams(self.netD), FlatParams(self.netD2)
            self.optimizer_G = FlatAdam(self.flatG, opt.lr, (opt.beta1, 0.999))
            self.optimizer_D = FlatAdam(self.flatD, opt.lr, (opt.beta1, 0.999))
            self.optimizer_D2 = FlatAdam(self.flatD2, opt.lr_G2, (opt.beta1, opt.beta2))
            self.optimizers += [self.optimizer_G, self.optimizer_D, self.optimizer_D2]
        self._loss_buf = ops.loss_slots(len(LOSS_SLOTS), self.device)     # int64 fixed point (order-independent accumulation)
        self._slot = {n: self._loss_buf[i:i + 1] for i, n in enumerate(LOSS_SLOTS)}
        self._bufs = {}
        self._graphs = None
        self._eager_steps_done = 0
        self.ddp = None

    @staticmethod
    def name_lists(opt):
        """(loss_names, visual_names, model_names), pix2pix_model.py:193-206: the loss names are listed in both phases"""
        model_names = ["G", "D", "D2"] if opt.isTrain else ["G"]
        visual_names = ["real_S", "M", "fake_I", "fake_gx", "fake_gy", "fake_N"]
        if "edit" not in opt.dataroot:
            visual_names.insert(2, "real_I")
        return ["G_GAN", "G_L1", "D_real", "D_fake", "D2_real", "D2_fake"], visual_names, model_names

    @staticmethod
    def _check_unbuilt(opt):
        bad = []
        if opt.netG not in RESNETS:
            bad.append("netG %s (built: %s)" % (opt.netG, ", ".join(RESNETS)))
        if opt.netD not in PATCHGANS:
            bad.append("netD %s (built: %s)" % (opt.netD, ", ".join(PATCHGANS)))
        if opt.norm != "batch":
            bad.append("norm %s (built: batch)" % opt.norm)
        if not opt.no_dropout:
            bad.append("no_dropout False")
        if not opt.use_bg_mask:
            bad.append("use_bg_mask False")
        if opt.T_resolution_multiplier != 1:
            bad.append("T_resolution_multiplier != 1")
        if getattr(opt, "gan_mode", None) == "wgangp":
            bad.append("gan_mode wgangp")
        if len(opt.gpu_ids) > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            bad.append("data-parallel runs: upstream's nn.DataParallel gives every replica its own BatchNorm batch, which one-process-per-GPU "
                       "ranks would not reproduce")
        if bad:
            raise NotImplementedError("pix2pix on the HIP path: " + "; ".join("not built: " + b for b in bad))

    def parallelize(self):
        from vts import ddp
        if ddp.active():
            raise NotImplementedError("pix2pix on the HIP path: not built: data-parallel runs")
        BaseModel.parallelize(self)

    # ------------------------------------------------------------------ input
    def _drop_graphs(self):
        if self._graphs is not None:
            self._graphs = None
            ops.release_ws((id(self), "train"))

    def _load(self, name, host):
        t = torch.as_tensor(host)
        buf = self._bufs.get(name)
        if buf is None or tuple(buf.shape) != tuple(t.shape):
            buf = self._bufs[name] = torch.empty(tuple(t.shape), dtype=torch.float32, device=self.device)
            self._drop_graphs()
        buf.copy_(t.to(torch.float32), non_blocking=True)
        return buf

    def set_input(self, input, phase="train", timing=False, verbose=False):
        """pix2pix_model.py:288-367.  Patches (return_patch): S_images / M_images / I_images [N, c, h, w], T_images [N, 2, h, w], I_masks
        [N, h, w].  Full images: S / M / I [N, c, H, W] with T_coords, full_T_coords and T_images [N, NT, 2, h, w], I_masks [N, NT, h, w]:
        the tactile patches are flattened to [N * NT, 2, h, w] and masked; the generator runs on the whole sketch."""
        self.data_phase = phase
        sk, mk, ik = ("S_images", "M_images", "I_images") if self.opt.return_patch else ("S", "M", "I")
        S = self._load("S", input[sk])
        self.M = self._load("M", input[mk])
        self.name = input["name"]
        self.image_paths = input["S_paths"]
        self.augmentation_params = input.get("augmentation_params")
        self.real_S = ops.mask_mul(S, self.M, out=S)
        if self.test_edit_S:
            return
        I = self._load("I", input[ik])
        self.real_I = ops.mask_mul(I, self.M, out=I)
        if "T_images" not in input:
            raise KeyError("T_images not in input keys")
        if self.opt.return_patch:
            self.T_coords = None
        else:
            if "T_coords" not in input:
                raise KeyError("T_coords is required for running full images")
            self.T_coords, self.full_T_coords = input["T_coords"], input["full_T_coords"]
            self.train_T_coords = torch.as_tensor(input["T_coords"]).numpy()
        t = torch.as_tensor(input["T_images"])
        if t.dim() not in (4, 5):
            raise ValueError("T_images should be 4D or 5D")
        c, h, w = t.shape[-3:]
        T = self._load("T", t.reshape(-1, c, h, w))
        self.I_masks = self._load("I_masks", torch.as_tensor(input["I_masks"]).reshape(-1, 1, h, w))
        self.real_T = ops.mask_mul(T, self.I_masks, out=T)
        self.real_gx, self.real_gy = self.real_T[:, 0:1], self.real_T[:, 1:2]

    # ------------------------------------------------------------------ forward
    def forward(self, keep=False):
        n, _, h, w = self.real_S.shape
        dev = self.device
        g_out, self._g_ctx = engine.resnet_forward(self.netG, Act(self.real_S), keep=keep)
        self.g_out = g_out
        self.fake_I = torch.empty(n, 3, h, w, device=dev)
        self.fake_T = torch.empty(n, 2, h, w, device=dev)
        self.fake_N = torch.empty(n, 3, h, w, device=dev)
        ops.g_post(g_out, self.M, self.opt.scale_nz, fake_I=self.fake_I, fake_T=self.fake_T, fake_N=self.fake_N)
        self.fake_gx, self.fake_gy = self.fake_T[:, 0:1], self.fake_T[:, 1:2]

    def test(self, timing=False):
        with torch.no_grad():
            self.forward(keep=False)

    # ------------------------------------------------------------------ training step
    def _seg_forward_d(self):
        """the step's ONE generator forward, then backward_D: both discriminators side by side (engine.msd_multi); per discriminator a fake
        pass and a real pass, two BatchNorm batches in that order (pix2pix_model.py:399-418)"""
        slot = self._slot
        self._loss_buf.zero_()
        self.forward(keep=True)

        def pair(fake, real, s_fake, s_real):
            return [dict(in0=self.real_S, in1=fake, real=False, coeff=1.0, slot=slot[s_fake], grad_coeff=0.5),
                    dict(in0=self.real_S, in1=real, real=True, coeff=1.0, slot=slot[s_real], grad_coeff=0.5, accumulate=True)]

        engine.msd_multi([(self.netD, pair(self.fake_I, self.real_I, "D_fake", "D_real")),
                          (self.netD2, pair(self.fake_T, self.real_T, "D2_fake", "D2_real"))], self.criterionGAN)

    def _seg_adam_d_g(self):
        slot, dev = self._slot, self.device
        n, _, h, w = self.real_S.shape
        self.optimizer_D.step(1.0)
        self.optimizer_D2.step(1.0)
        d_fake_I = torch.empty(n, 3, h, w, device=dev)
        d_fake_T = torch.empty(n, 2, h, w, device=dev)
        engine.msd_multi([(self.netD, [dict(in0=self.real_S, in1=self.fake_I, real=True, coeff=1.0, slot=slot["G_GAN_I"], grad_coeff=1.0,
                                            param_grads=False, input_grad=(d_fake_I, False))]),
                          (self.netD2, [dict(in0=self.real_S, in1=self.fake_T, real=True, coeff=1.0, slot=slot["G_GAN_T"], grad_coeff=1.0,
                                             param_grads=False, input_grad=(d_fake_T, False))])], self.criterionGAN)
        slot["G_GAN"].copy_(slot["G_GAN_I"] + slot["G_GAN_T"])
        # (L1(fake_I, real_I) + L1(fake_T, real_T)) * lambda_L1, each a mean (:440-442): value into one slot, sign(.) added to the gradients
        lam = self.opt.lambda_L1
        ops.l1(self.fake_I, self.real_I, lam / self.fake_I.numel(), slot["G_L1"], grad=d_fake_I, accumulate=True)
        ops.l1(self.fake_T, self.real_T, lam / self.fake_T.numel(), slot["G_L1"], grad=d_fake_T, accumulate=True)
        d_raw = torch.empty(n, 5, h, w, device=dev)
        ops.g_out_grad(d_fake_I, d_fake_T, self.M, self.g_out, d_raw)
        engine.resnet_backward(self.netG, self._g_ctx, d_raw)

    def _seg_adam_g(self):
        self.optimizer_G.step(1.0)

    def _segments(self):
        return [self._seg_forward_d, self._seg_adam_d_g, self._seg_adam_g]

    def _capture_graphs(self):
        torch.cuda.synchronize()
        pool = torch.cuda.graph_pool_handle()
        stream = torch.cuda.Stream()
        counts = [o.step_count for o in self.optimizers]
        graphs, nodes = [], []
        ops.freeze_ws((id(self), "train"))
        try:
            for seg in self._segments():
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool, stream=stream, capture_error_mode="thread_local"):
                    seg()
                    nodes.append(ops.capture_node_count())
                graphs.append(g)
        except Exception:
            ops.release_ws((id(self), "train"))
            raise
        for o, c in zip(self.optimizers, counts):
            o.step_count = c
        self._graphs = graphs
        self.graph_nodes = nodes

    def optimize_parameters(self, epoch=0, timing=False):
        real_T = getattr(self, "real_T", None)
        if real_T is None or tuple(real_T.shape[2:]) != tuple(self.real_S.shape[2:]) or real_T.shape[0] != self.real_S.shape[0]:
            raise ValueError("the training step runs on paired patches (--return_patch True): tactile %s against sketch %s"
                             % (None if real_T is None else tuple(real_T.shape), tuple(self.real_S.shape)))
        for o in self.optimizers:
            o.sync_lr()
        use_graph = bool(getattr(self.opt, "use_hip_graph", False))
        if use_graph and self._graphs is None and self._eager_steps_done >= 1:
            self._capture_graphs()
        replay = use_graph and self._graphs is not None
        for i, seg in enumerate(self._segments()):
            if replay:
                self._graphs[i].replay()
            else:
                seg()
        if replay:
            for o in self.optimizers:
                o.step_count += 1
        else:
            self._eager_steps_done += 1

    # ------------------------------------------------------------------ logging
    def get_current_losses(self):
        vals = ops.loss_values(self._loss_buf)
        for i, name in enumerate(LOSS_SLOTS):
            setattr(self, "loss_" + name, vals[i])
        return BaseModel.get_current_losses(self)

    def compute_metrics(self, prefix=""):
        """the evaluation metrics of the outputs of the last forward() / test() (pix2pix_model.py:572-590 -> compute_evaluation_metric):
        vts/metrics.py, shared by the three baselines"""
        return metrics.model_metrics(self, prefix)

    def compute_visuals(self):
        pass
