"""SPADE / GauGAN baseline on the HIP path (reference: models/spade_model.py).

The reference trains this baseline patch-wise like pix2pixHD (`return_patch=True`: 32x32 sketch / image / tactile patches, batch 16)
with the SPADE generator (spectral-normalised blocks, sync-batch statistics), two plain multiscale PatchGAN discriminators (D: sketch ++
image, D2: sketch ++ tactile; BatchNorm, no intermediate features: its options hold no getIntermFeat_D, and --normD never reaches
define_D) and the hinge objective:

    forward             spade_model.py:573-599     G(S) -> fake_I = out[:, :3] * M, fake_T = out[:, -2:] * M_T
    backward_D          :601-621                   0.5 (D_fake + D_real) + 0.5 (D2_fake + D2_real); fake and real are SEPARATE passes
    backward_G          :623-679                   G_GAN_I + G_GAN_T (target real: relu(1 - pred)) (+ feature matching + VGG)
    optimize_parameters :681-704                   ONE generator forward, D and D2 step, then G step

The feature-matching term compares every discriminator feature with itself detached (:638-660), value and gradient 0: reported as 0.
The three VGG feature terms (the image; gx and gy tiled to three channels) run as one stacked batch (vts.perceptual.vgg_feature_l1_stacked);
pretrained VGG19 weights come from `--vgg_weights`, otherwise seeded stand-ins are used and `loss_vgg_pretrained` is False.
The generator's forward runs once per step, so every spectral-norm u / v advances once per step, as upstream.
"""
import argparse
import os

import torch

from vts.misc import str2bool
from vts import engine, metrics, ops
from vts.optim import FlatAdam, FlatParams

from . import networks
from .base_model import BaseModel
from .sinskitG_model import add_model_flags

B = str2bool

# (flag, type, default[, choices])  -- reference: spade_model.py:47-205
MODEL_FLAGS = [
    ("lambda_L1", float, 100.0), ("lr_G2", float, 0.0005), ("sketch_nc", int, 1), ("image_nc", int, 3), ("touch_nc", int, 2),
    ("center_w", int, 1280), ("center_h", int, 960), ("num_touch_patch_for_logging", int, 10), ("use_bg_mask", B, True),
    ("data_len", int, 200), ("T_resolution_multiplier", int, 1), ("padded_size", int, 1800), ("sample_bbox_per_patch", int, 2),
    ("save_S_patch", B, False), ("save_T_concat_tensor", B, False), ("save_raw_arr_vis", B, False), ("scale_nz", float, 0.25),
    ("return_patch", B, False), ("label_nc", int, 0), ("feat_num", int, 3), ("n_downsample_E", int, 4), ("num_D_D1", int, 2),
    ("num_D_D2", int, 2), ("no_gan_loss", B, False), ("niter_decay", int, 100), ("separate_val_set", B, False),
    ("use_features", B, False), ("normE", str, "spectralinstance"), ("semantic_nc", int, 1), ("z_dim", int, 256), ("no_instance", B, True),
    ("nef", int, 16), ("use_vae", "flag", False), ("lambda_feat", float, 10.0), ("lambda_vgg", float, 10.0),
    ("no_ganFeat_loss", B, False), ("no_vgg_loss", B, False), ("lambda_kld", float, 0.05), ("num_upsampling_layers", int, 3),
    ("output_width", int, 32), ("aspect_ratio", float, 1.0),
]

LOSS_SLOTS = ["G_GAN_I", "G_GAN_T", "G_GAN", "D_real", "D_fake", "D2_real", "D2_fake", "G_GAN_Feat", "G_GAN_Feat_I", "G_GAN_Feat_T",
              "G_VGG", "G_VGG_I", "G_VGG_T"]


class _NoTTUR(argparse.Action):
    """--no_TTUR.  The reference's option setter parses the command line itself to see this flag and moves the DEFAULTS of beta1 / beta2 to
    (0.5, 0.999) (spade_model.py:254-258); here the flag does that when the parser meets it -- the option passes that follow (the dataset's,
    the final one) then start from those defaults, and an explicit --beta1 / --beta2 still wins."""

    def __init__(self, option_strings, dest, **kw):
        super().__init__(option_strings, dest, nargs=0, default=False, required=False)

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, True)
        parser.set_defaults(beta1=0.5, beta2=0.999)


class SPADEModel(BaseModel):
    @staticmethod
    def modify_commandline_options(parser, is_train=True):
        add_model_flags(parser, [r for r in MODEL_FLAGS if r[1] != "flag"])
        for name, _, _ in [r for r in MODEL_FLAGS if r[1] == "flag"]:
            parser.add_argument("--" + name, action="store_true", default=False)
        parser.add_argument("--no_TTUR", action=_NoTTUR)
        parser.add_argument("--use_hip_graph", type=B, default=True)   # not a reference flag: replay captured HIP graphs
        # not reference flags: weight files of the optional metric networks (upstream downloads them) and --eval_T_FID (T_FID is known to
        # compute_evaluation_metric but in none of upstream's metric lists)
        metrics.add_metric_flags(parser)
        # not a reference flag: torchvision vgg19 state dict for VGGLoss (the reference downloads it, models/networks.py:2040); without a
        # file the term runs on seeded stand-in weights and `loss_vgg_pretrained` says so
        parser.add_argument("--vgg_weights", type=str, default="")
        # (normG / normD / netG arrive as defaults: the base parser's `choices` list none of these values, as upstream)
        parser.set_defaults(norm="batch", ngf=64, dataset_mode="aligned", dataset="patchskit", crop_size=1536, pool_size=0, n_epochs=50,
                            n_epcohs_decay=0, netG="spade", netD="multiscale", normG="spectralspadesyncbatch3x3", normD="spectralinstance",
                            lr=0.0002, gan_mode="hinge", num_D_D1=2, num_D_D2=2, beta1=0.0, beta2=0.9)
        verbose_freq = 320
        if is_train:
            parser.set_defaults(return_patch=True, batch_size=16, display_freq=verbose_freq, print_freq=verbose_freq,
                                save_latest_freq=verbose_freq, validation_freq=verbose_freq, save_epoch_freq=50, display_id=0,
                                save_raw_arr_vis=False, output_width=32)
        else:
            parser.set_defaults(return_patch=False, batch_size=1, save_S_patch=True, save_raw_arr_vis=False, sample_bbox_per_patch=1,
                                data_len=1, load_size=1800, output_width=1536)
        return parser

    def __init__(self, opt):
        BaseModel.__init__(self, opt)
        if not self.gpu_ids or not torch.cuda.is_available():
            raise RuntimeError("SPADEModel runs on the MI355X HIP path only (no CPU fallback): pass --gpu_ids 0 on a GPU box")
        self._check_unbuilt(opt)
        self.test_edit_S = "edit" in opt.dataroot
        self.loss_names, self.visual_names, self.model_names = self.name_lists(opt)
        self.netG = networks.define_G(opt.sketch_nc, opt.image_nc + opt.touch_nc, opt.ngf, "spade", opt.norm, gpu_ids=self.gpu_ids, opt=opt)
        self.flatG = FlatParams(self.netG)
        if self.isTrain:
            self.criterionGAN = networks.GANLoss(opt.gan_mode)
            self.netD = networks.define_D(opt.image_nc + opt.sketch_nc, opt.ndf, "multiscale", opt.n_layers_D, opt.norm, num_D=opt.num_D_D1,
                                          gpu_ids=self.gpu_ids, opt=opt)
            self.netD2 = networks.define_D(opt.touch_nc + opt.sketch_nc, opt.ndf, "multiscale", opt.n_layers_D, opt.norm, num_D=opt.num_D_D2,
                                           gpu_ids=self.gpu_ids, opt=opt)
            self.flatD, self.flatD2 = FlatParams(self.netD), FlatParams(self.netD2)
            self.old_lr = opt.lr
            g_lr, d_lr = self.learning_rates(opt)
            betas = (opt.beta1, opt.beta2)
            self.optimizer_G = FlatAdam(self.flatG, g_lr, betas)
            self.optimizer_D = FlatAdam(self.flatD, d_lr, betas)
            self.optimizer_D2 = FlatAdam(self.flatD2, d_lr, betas)
            self.optimizers += [self.optimizer_G, self.optimizer_D, self.optimizer_D2]
            if opt.pool_size > 0 and len(self.gpu_ids) > 1:
                raise NotImplementedError("Fake Pool Not Implemented for MultiGPU")      # (spade_model.py:331-332)
            # (the reference constructs fake_pool and never queries it, :333 / :601-621: nothing to build)
        self.netVGG = None
        if self.isTrain and not opt.no_vgg_loss:      # criterionVGG = VGGLoss(gpu_ids) (spade_model.py:338-339; networks.py:2021-2067): frozen
            from . import perceptual
            self.netVGG = perceptual.build_vgg19(opt, self.device)
            self.loss_vgg_pretrained = bool(self.netVGG.pretrained)
        self._loss_buf = ops.loss_slots(len(LOSS_SLOTS), self.device)     # int64 fixed point (order-independent accumulation)
        self._slot = {n: self._loss_buf[i:i + 1] for i, n in enumerate(LOSS_SLOTS)}
        self._bufs = {}
        self._graphs = None
        self._eager_steps_done = 0
        self.ddp = None

    @staticmethod
    def name_lists(opt):
        """(loss_names, visual_names, model_names), spade_model.py:287-311"""
        model_names = ["G", "D", "D2"] if opt.isTrain else ["G"]
        visual_names = ["real_S", "M", "fake_I", "fake_gx", "fake_gy", "fake_N"]
        if "edit" not in opt.dataroot:
            visual_names.insert(2, "real_I")
        loss_names = []
        if opt.isTrain:
            if not opt.no_gan_loss:
                loss_names += ["G_GAN_I", "G_GAN_T", "G_GAN", "D_real", "D_fake", "D2_real", "D2_fake"]
            if not opt.no_ganFeat_loss:
                loss_names += ["G_GAN_Feat", "G_GAN_Feat_I", "G_GAN_Feat_T"]
            if not opt.no_vgg_loss:
                loss_names += ["G_VGG", "G_VGG_I", "G_VGG_T"]
        return loss_names, visual_names, model_names

    @staticmethod
    def learning_rates(opt):
        """(G, D) initial rates, spade_model.py:415-423: the two-time-scale rule halves G's and doubles the discriminators' unless --no_TTUR"""
        return (opt.lr, opt.lr) if opt.no_TTUR else (opt.lr / 2, opt.lr * 2)

    def update_learning_rate(self):
        """spade_model.py:873-884: every call sets the rate of ALL THREE optimisers to old_lr - opt.lr / niter_decay, old_lr starting at opt.lr.
        The two-time-scale ratio (G lr / 2, D lr * 2) is therefore lost at the first call -- the reference's behaviour, kept on purpose."""
        lr = self.old_lr - self.opt.lr / self.opt.niter_decay
        for o in (self.optimizer_D, self.optimizer_D2, self.optimizer_G):
            for g in o.param_groups:
                g["lr"] = lr
        if self.opt.verbose:
            print("update learning rate: %f -> %f" % (self.old_lr, lr))
        self.old_lr = lr

    @staticmethod
    def _check_unbuilt(opt):
        upstream, bad = [], []
        if opt.use_vae:
            # spade_model.py:392-400: define_G(output_nc, feat_num, nef, "conv_encoder", n_downsample_E, norm=opt.norm, ...) -- the fifth
            # positional parameter of define_G IS norm
            upstream.append("--use_vae: the reference builds its encoder with define_G(output_nc, feat_num, nef, 'conv_encoder', n_downsample_E, "
                            "norm=...), which passes norm twice (models/spade_model.py:392-400): a TypeError upstream, no behaviour to restate")
        if opt.use_features or not opt.no_instance or opt.label_nc != 0:
            upstream.append("--use_features / --no_instance False / label_nc != 0: not reachable in the reference either (its forward() feeds the "
                            "sketch alone, models/spade_model.py:573-586; 'E' is listed without a netE, :289-290), so there is no behaviour to restate")
        if opt.T_resolution_multiplier != 1:
            bad.append("T_resolution_multiplier != 1")
        if not opt.use_bg_mask:
            bad.append("use_bg_mask False")
        if opt.isTrain and opt.no_gan_loss:
            bad.append("no_gan_loss")
        if opt.netG != "spade":
            bad.append("netG %s (built: spade)" % opt.netG)
        if opt.netD != "multiscale":
            bad.append("netD %s (built: multiscale)" % opt.netD)
        if len(opt.gpu_ids) > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            bad.append("data-parallel runs: syncbatch statistics across one-process-per-GPU ranks are not implemented, and per-rank statistics "
                       "would silently differ from the reference")
        if upstream or bad:
            raise NotImplementedError("SPADE on the HIP path: " + "; ".join(upstream + ["not built: " + b for b in bad]))

    def parallelize(self):
        from vts import ddp
        if ddp.active():
            raise NotImplementedError("SPADE on the HIP path: not built: data-parallel runs (syncbatch statistics across ranks)")
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
        """spade_model.py:425-504 (pix2pixHD's contract): mask multiply; tactile patches reshaped to [N, 2, h, w] and masked."""
        self.data_phase = phase
        sk, mk, ik = ("S_images", "M_images", "I_images") if self.opt.return_patch else ("S", "M", "I")
        S = self._load("S", input[sk])
        self.M = self._load("M", input[mk])
        self.name = input["name"]
        self.image_paths = input["S_paths"]
        self.augmentation_params = input.get("augmentation_params")
        self.real_S = ops.mask_mul(S, self.M, out=S)
        if not self.test_edit_S:
            I = self._load("I", input[ik])
            self.real_I = ops.mask_mul(I, self.M, out=I)
            t = torch.as_tensor(input["T_images"])
            h, w = t.shape[-2:]
            T = self._load("T", t.reshape(-1, 2, h, w))
            masks = self._load("I_masks", torch.as_tensor(input["I_masks"]).reshape(-1, 1, h, w))
            self.real_T = ops.mask_mul(T, masks, out=T)
            self.real_gx, self.real_gy = self.real_T[:, 0:1], self.real_T[:, 1:2]
            self.T_coords = None if self.opt.return_patch else input.get("T_coords")      # full images: where compute_metrics cuts the fake patches

    # ------------------------------------------------------------------ forward
    def forward(self, infer=False, keep=False):
        n, _, h, w = self.real_S.shape
        dev = self.device
        g_out, self._g_ctx = engine.spade_forward(self.netG, self.real_S, keep=keep)
        if tuple(g_out.shape[2:]) != (h, w):
            raise ValueError("SPADE generator output %dx%d does not match the %dx%d input: --output_width / --aspect_ratio / "
                             "--num_upsampling_layers fix the output size" % (g_out.shape[2], g_out.shape[3], h, w))
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
        """the step's ONE generator forward, then backward_D: both discriminators, all scales side by side (engine.msd_multi); per
        discriminator a fake pass and a real pass, two BatchNorm batches in that order (spade_model.py:606-617)"""
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
        if self.netVGG is not None:
            # VGG feature matching (spade_model.py:662-675): the image, and gx / gy each tiled to three channels, as one batch of 6 N rows
            from vts import perceptual as P_
            P_.vgg_feature_l1_stacked(self.netVGG, self.fake_I, self.fake_T, self.real_I, self.real_T, self.opt.lambda_vgg,
                                      slot["G_VGG_I"], slot["G_VGG_T"], d_fake_I=d_fake_I, d_fake_T=d_fake_T, accumulate=True)
            slot["G_VGG"].copy_(slot["G_VGG_I"] + slot["G_VGG_T"])
        d_raw = torch.empty(n, 5, h, w, device=dev)
        ops.g_out_grad(d_fake_I, d_fake_T, self.M, self.g_out, d_raw)
        # (d_raw is the gradient of the PRE-tanh output: g_out_grad applies the tanh adjoint; the sketch is data: nobody reads its gradient)
        engine.spade_backward(self.netG, self._g_ctx, d_raw, want_dseg=False, pre_tanh=True)

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
        """the evaluation metrics of the outputs of the last forward() / test() (spade_model.py:806-822 -> compute_evaluation_metric):
        vts/metrics.py, shared by the three baselines"""
        return metrics.model_metrics(self, prefix)

    def compute_visuals(self):
        pass
