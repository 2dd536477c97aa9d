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
The step itself is PatchBaselineModel's (models/patch_baseline.py).
"""
import os

import torch

from vts.misc import str2bool
from vts import engine, ops
from vts.ops import Act
from vts.optim import FlatAdam

from . import networks
from .base_model import BaseModel
from .patch_baseline import PatchBaselineModel, add_baseline_flags, set_phase_defaults

B = str2bool

# (flag, type, default) besides patch_baseline.COMMON_FLAGS  -- reference: pix2pix_model.py:54-132
MODEL_FLAGS = [("return_patch", B, False)]

RESNETS = ("resnet_6blocks", "resnet_9blocks")
PATCHGANS = ("basic", "n_layers")


class Pix2PixModel(PatchBaselineModel):
    LOSS_SLOTS = ("G_GAN", "G_L1", "D_real", "D_fake", "D2_real", "D2_fake", "G_GAN_I", "G_GAN_T")
    GAN_LOSS = networks.GANLossLastSample

    @staticmethod
    def modify_commandline_options(parser, is_train=True):
        add_baseline_flags(parser, MODEL_FLAGS)
        parser.set_defaults(norm="batch", netG="resnet_9blocks", dataset_mode="aligned", dataset="patchskit", crop_size=1536)
        if is_train:
            parser.set_defaults(pool_size=0, gan_mode="vanilla")
        set_phase_defaults(parser, is_train, batch_size=32)
        return parser

    def _define_G(self, opt):
        return networks.define_G(opt.sketch_nc, opt.image_nc + opt.touch_nc, opt.ngf, opt.netG, opt.norm, not opt.no_dropout,
                                 opt.init_type, opt.init_gain, opt.no_antialias, opt.no_antialias_up, self.gpu_ids, opt)

    def _define_Ds(self, opt):
        return [networks.define_D(nc + opt.sketch_nc, opt.ndf, opt.netD, opt.n_layers_D, opt.norm, opt.init_type, opt.init_gain,
                                  opt.no_antialias, gpu_ids=self.gpu_ids, opt=opt) for nc in (opt.image_nc, opt.touch_nc)]

    def _make_optimizers(self, opt):
        return (FlatAdam(self.flatG, opt.lr, (opt.beta1, 0.999)), FlatAdam(self.flatD, opt.lr, (opt.beta1, 0.999)),
                FlatAdam(self.flatD2, opt.lr_G2, (opt.beta1, opt.beta2)))

    @staticmethod
    def loss_name_list(opt):
        """pix2pix_model.py:193-206: the loss names are listed in both phases"""
        return ["G_GAN", "G_L1", "D_real", "D_fake", "D2_real", "D2_fake"]

    update_learning_rate = BaseModel.update_learning_rate      # (the reference keeps BaseModel's schedulers for this model)

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
    def set_input(self, input, phase="train", timing=False, verbose=False):
        """pix2pix_model.py:288-367.  Patches (return_patch): S_images / M_images / I_images [N, c, h, w], T_images [N, 2, h, w], I_masks
        [N, h, w].  Full images: S / M / I [N, c, H, W] with T_coords, full_T_coords and T_images [N, NT, 2, h, w], I_masks [N, NT, h, w]:
        the tactile patches are flattened to [N * NT, 2, h, w] and masked; the generator runs on the whole sketch."""
        ik = self._set_sketch(input, phase)
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

    # ------------------------------------------------------------------ training step
    def _g_forward(self, keep):
        return engine.resnet_forward(self.netG, Act(self.real_S), keep=keep)

    def _g_extra_terms(self, d_fake_I, d_fake_T):
        # (L1(fake_I, real_I) + L1(fake_T, real_T)) * lambda_L1, each a mean (:440-442): value into one slot, sign(.) added to the gradients
        lam, slot = self.opt.lambda_L1, self._slot
        ops.l1(self.fake_I, self.real_I, lam / self.fake_I.numel(), slot["G_L1"], grad=d_fake_I, accumulate=True)
        ops.l1(self.fake_T, self.real_T, lam / self.fake_T.numel(), slot["G_L1"], grad=d_fake_T, accumulate=True)

    def _g_backward(self, d_raw):
        engine.resnet_backward(self.netG, self._g_ctx, d_raw)

    def optimize_parameters(self, epoch=0, timing=False):
        real_T = getattr(self, "real_T", None)
        if real_T is None or tuple(real_T.shape[2:]) != tuple(self.real_S.shape[2:]) or real_T.shape[0] != self.real_S.shape[0]:
            raise ValueError("the training step runs on paired patches (--return_patch True): tactile %s against sketch %s"
                             % (None if real_T is None else tuple(real_T.shape), tuple(self.real_S.shape)))
        self._run_step()
