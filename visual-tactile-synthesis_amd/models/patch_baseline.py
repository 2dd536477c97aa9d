"""PatchBaselineModel: what the three patch-wise baselines (pix2pix, pix2pixHD, SPADE) share on the HIP path.

The reference trains all three on 32x32 sketch / image / tactile patches with one generator G(S) -> (fake_I, fake_T) and two discriminators
(D: sketch ++ image, D2: sketch ++ tactile), and steps them in the same order: ONE generator forward, backward_D of both discriminators,
D and D2 step, the generator's GAN terms through the updated discriminators plus the model's own terms, G step.  That step, its input
contract, the inference path and the evaluation metrics live here; a model file keeps its flags, what it refuses, its networks and
optimisers, its generator's forward / backward calls and its extra generator terms.
"""
import torch

from vts.misc import str2bool
from vts import engine, metrics, ops
from vts.optim import FlatParams

from . import networks
from .graphed_step import GraphedStepModel
from .sinskitG_model import add_model_flags

B = str2bool

# (flag, type, default): the rows the three reference parsers have in common
COMMON_FLAGS = [
    ("lambda_L1", float, 100.0), ("lr_G2", float, 0.0005), ("sketch_nc", int, 1), ("image_nc", int, 3), ("touch_nc", int, 2),
    ("data_len", int, 200), ("center_w", int, 1280), ("center_h", int, 960), ("num_touch_patch_for_logging", int, 10),
    ("use_bg_mask", B, True), ("T_resolution_multiplier", int, 1), ("padded_size", int, 1800), ("sample_bbox_per_patch", int, 2),
    ("save_S_patch", B, False), ("save_T_concat_tensor", B, False), ("save_raw_arr_vis", B, False), ("scale_nz", float, 0.25),
]

# the loss slots of pix2pixHD and SPADE (pix2pix has its own)
GAN_FEAT_VGG_SLOTS = ("G_GAN_I", "G_GAN_T", "G_GAN", "D_real", "D_fake", "D2_real", "D2_fake", "G_GAN_Feat", "G_GAN_Feat_I", "G_GAN_Feat_T",
                      "G_VGG", "G_VGG_I", "G_VGG_T")


def add_baseline_flags(parser, own, vgg=False):
    """COMMON_FLAGS, the model's own rows (type "flag": a store_true switch) and the flags that are not the reference's"""
    rows = COMMON_FLAGS + list(own)
    add_model_flags(parser, [r for r in rows if r[1] != "flag"])
    for r in rows:
        if r[1] == "flag":
            parser.add_argument("--" + r[0], action="store_true", default=False)
    parser.add_argument("--use_hip_graph", type=B, default=True)   # not a reference flag: replay captured HIP graphs
    # not reference flags: weight files of the optional metric networks (upstream downloads them) and --eval_T_FID (T_FID is known to
    # compute_evaluation_metric but in none of upstream's metric lists)
    metrics.add_metric_flags(parser)
    if vgg:
        # not a reference flag: torchvision vgg19 state dict for VGGLoss (the reference downloads it, models/networks.py:2040); without a
        # file the term runs on seeded stand-in weights and `loss_vgg_pretrained` says so
        parser.add_argument("--vgg_weights", type=str, default="")


def set_phase_defaults(parser, is_train, batch_size):
    """the defaults the three reference option setters move alike per phase (batch_size: the training one)"""
    verbose_freq = 320
    if is_train:
        parser.set_defaults(return_patch=True, batch_size=batch_size, display_freq=verbose_freq, print_freq=verbose_freq,
                            save_latest_freq=verbose_freq, validation_freq=verbose_freq, save_epoch_freq=50, display_id=0,
                            save_raw_arr_vis=False)
    else:
        parser.set_defaults(return_patch=False, batch_size=1, save_S_patch=True, save_raw_arr_vis=False, sample_bbox_per_patch=1,
                            data_len=1)


class PatchBaselineModel(GraphedStepModel):
    LOSS_SLOTS = GAN_FEAT_VGG_SLOTS
    GAN_LOSS = networks.GANLoss

    def __init__(self, opt):
        GraphedStepModel.__init__(self, opt)
        if not self.gpu_ids or not torch.cuda.is_available():
            raise RuntimeError("%s runs on the MI355X HIP path only (no CPU fallback): pass --gpu_ids 0 on a GPU box" % type(self).__name__)
        self._check_unbuilt(opt)
        self.test_edit_S = "edit" in opt.dataroot
        self.loss_names, self.visual_names, self.model_names = self.name_lists(opt)
        self.netG = self._define_G(opt)
        self.flatG = FlatParams(self.netG)
        if self.isTrain:
            self.criterionGAN = self.GAN_LOSS(opt.gan_mode)
            self.netD, self.netD2 = self._define_Ds(opt)
            self.flatD, self.flatD2 = FlatParams(self.netD), FlatParams(self.netD2)
            self.old_lr = opt.lr     # (update_learning_rate below; pix2pix steps BaseModel's schedulers and never reads it)
            self.optimizer_G, self.optimizer_D, self.optimizer_D2 = self._make_optimizers(opt)
            self.optimizers += [self.optimizer_G, self.optimizer_D, self.optimizer_D2]
        self._build_own(opt)
        self._init_step_state()

    # ---- what a model file supplies (besides modify_commandline_options and _check_unbuilt) ----
    def _define_G(self, opt):
        raise NotImplementedError

    def _define_Ds(self, opt):
        """(netD, netD2)"""
        raise NotImplementedError

    def _make_optimizers(self, opt):
        """(optimizer_G, optimizer_D, optimizer_D2) over flatG / flatD / flatD2"""
        raise NotImplementedError

    def _build_own(self, opt):
        """whatever else the model constructs, in both phases and after the optimisers: cuts of a gradient bucket, an image pool, a
        frozen feature network"""

    def _build_vgg(self, opt):
        """criterionVGG = VGGLoss(gpu_ids) of pix2pixHD and SPADE (networks.py:2021-2067): frozen, not a saved network"""
        self.netVGG = None
        if self.isTrain and not opt.no_vgg_loss:
            from . import perceptual
            self.netVGG = perceptual.build_vgg19(opt, self.device)
            self.loss_vgg_pretrained = bool(self.netVGG.pretrained)

    def _g_forward(self, keep):
        """(g_out, context for the backward) of the generator on self.real_S"""
        raise NotImplementedError

    def _g_backward(self, d_raw):
        raise NotImplementedError

    def _g_extra_terms(self, d_fake_I, d_fake_T):
        """the generator's terms besides the GAN ones: values into their loss slots, gradients ADDED to d_fake_I / d_fake_T"""
        raise NotImplementedError

    def _pool_fake(self, job):
        """pix2pixHD: what D's fake pass sees in place of (real_S, fake_I)"""

    # ------------------------------------------------------------------ names
    @staticmethod
    def loss_name_list(opt):
        """the list pix2pixHD and SPADE share (spade_model.py:287-311)"""
        names = []
        if opt.isTrain:
            if not opt.no_gan_loss:
                names += ["G_GAN_I", "G_GAN_T", "G_GAN", "D_real", "D_fake", "D2_real", "D2_fake"]
            if not opt.no_ganFeat_loss:
                names += ["G_GAN_Feat", "G_GAN_Feat_I", "G_GAN_Feat_T"]
            if not opt.no_vgg_loss:
                names += ["G_VGG", "G_VGG_I", "G_VGG_T"]
        return names

    @classmethod
    def name_lists(cls, opt):
        """(loss_names, visual_names, model_names)"""
        model_names = ["G", "D", "D2"] if opt.isTrain else ["G"]
        visual_names = ["real_S", "M", "fake_I", "fake_gx", "fake_gy", "fake_N"]
        if "edit" not in opt.dataroot:
            visual_names.insert(2, "real_I")
        return cls.loss_name_list(opt), visual_names, model_names

    def update_learning_rate(self):
        """pix2pixHD_model.py:951-962, spade_model.py:873-884: every call sets the rate of ALL THREE optimisers to old_lr - opt.lr /
        niter_decay, old_lr starting at opt.lr (the reference overrides BaseModel's scheduler step with this, and has no floor).  SPADE's
        two-time-scale ratio (G lr / 2, D lr * 2) is therefore lost at the first call -- the reference's behaviour, kept on purpose."""
        lr = self.old_lr - self.opt.lr / self.opt.niter_decay
        for o in (self.optimizer_D, self.optimizer_D2, self.optimizer_G):
            for g in o.param_groups:
                g["lr"] = lr
        if self.opt.verbose:
            print("update learning rate: %f -> %f" % (self.old_lr, lr))
        self.old_lr = lr

    # ------------------------------------------------------------------ input
    def _set_sketch(self, input, phase):
        """the sketch half of set_input: real_S, M and the bookkeeping; returns the batch key of the image"""
        self.data_phase = phase
        sk, mk, ik = ("S_images", "M_images", "I_images") if self.opt.return_patch else ("S", "M", "I")
        S = self._load("S", input[sk])
        self.M = self._load("M", input[mk])
        self.name = input["name"]
        self.image_paths = input["S_paths"]
        self.augmentation_params = input.get("augmentation_params")
        self.real_S = ops.mask_mul(S, self.M, out=S)
        return ik

    def set_input(self, input, phase="train", timing=False, verbose=False):
        """pix2pixHD_model.py:431-509, spade_model.py:425-504: mask multiply; tactile patches reshaped to [N, 2, h, w] and masked."""
        ik = self._set_sketch(input, phase)
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
        g_out, self._g_ctx = self._g_forward(keep)
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
        discriminator a fake pass and a real pass, two BatchNorm batches in that order (pix2pix_model.py:399-418, spade_model.py:606-617)"""
        slot = self._slot
        self._loss_buf.zero_()
        self.forward(keep=True)

        def pair(fake, real, s_fake, s_real):
            return [dict(in0=self.real_S, in1=fake, real=False, coeff=1.0, slot=slot[s_fake], grad_coeff=0.5),
                    dict(in0=self.real_S, in1=real, real=True, coeff=1.0, slot=slot[s_real], grad_coeff=0.5, accumulate=True)]

        jobs_D = pair(self.fake_I, self.real_I, "D_fake", "D_real")
        self._pool_fake(jobs_D[0])
        engine.msd_multi([(self.netD, jobs_D),
                          (self.netD2, pair(self.fake_T, self.real_T, "D2_fake", "D2_real"))], self.criterionGAN)

    def _seg_adam_d_g(self):
        slot, dev = self._slot, self.device
        n, _, h, w = self.real_S.shape
        self.optimizer_D.step(self._gscale)
        self.optimizer_D2.step(self._gscale)
        d_fake_I = torch.empty(n, 3, h, w, device=dev)
        d_fake_T = torch.empty(n, 2, h, w, device=dev)
        engine.msd_multi([(self.netD, [dict(in0=self.real_S, in1=self.fake_I, real=True, coeff=1.0, slot=slot["G_GAN_I"], grad_coeff=1.0,
                                            param_grads=False, input_grad=(d_fake_I, False))]),
                          (self.netD2, [dict(in0=self.real_S, in1=self.fake_T, real=True, coeff=1.0, slot=slot["G_GAN_T"], grad_coeff=1.0,
                                             param_grads=False, input_grad=(d_fake_T, False))])], self.criterionGAN)
        slot["G_GAN"].copy_(slot["G_GAN_I"] + slot["G_GAN_T"])
        self._g_extra_terms(d_fake_I, d_fake_T)
        d_raw = torch.empty(n, 5, h, w, device=dev)
        ops.g_out_grad(d_fake_I, d_fake_T, self.M, self.g_out, d_raw)
        self._g_backward(d_raw)

    def _seg_adam_g(self):
        self.optimizer_G.step(self._gscale)

    def _segments(self):
        return [(self._seg_forward_d, (), ()), (self._seg_adam_d_g, (), ()), (self._seg_adam_g, (), ())]

    def optimize_parameters(self, epoch=0, timing=False):
        self._run_step()

    # ------------------------------------------------------------------ logging
    def compute_metrics(self, prefix=""):
        """the evaluation metrics of the outputs of the last forward() / test() (pix2pix_model.py:572-590, pix2pixHD_model.py:824-840,
        spade_model.py:806-822 -> compute_evaluation_metric): vts/metrics.py"""
        return metrics.model_metrics(self, prefix)

    def compute_visuals(self):
        pass
