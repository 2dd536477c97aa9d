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
The step itself is PatchBaselineModel's (models/patch_baseline.py).
"""
import argparse
import os

from vts.misc import str2bool
from vts import engine
from vts.optim import FlatAdam

from . import networks
from .base_model import BaseModel
from .patch_baseline import PatchBaselineModel, add_baseline_flags, set_phase_defaults

B = str2bool

# (flag, type, default[, choices]) besides patch_baseline.COMMON_FLAGS  -- reference: spade_model.py:47-205
MODEL_FLAGS = [
    ("return_patch", B, False), ("label_nc", int, 0), ("feat_num", int, 3), ("n_downsample_E", int, 4), ("num_D_D1", int, 2),
    ("num_D_D2", int, 2), ("no_gan_loss", B, False), ("niter_decay", int, 100), ("separate_val_set", B, False),
    ("use_features", B, False), ("normE", str, "spectralinstance"), ("semantic_nc", int, 1), ("z_dim", int, 256), ("no_instance", B, True),
    ("nef", int, 16), ("use_vae", "flag", False), ("lambda_feat", float, 10.0), ("lambda_vgg", float, 10.0),
    ("no_ganFeat_loss", B, False), ("no_vgg_loss", B, False), ("lambda_kld", float, 0.05), ("num_upsampling_layers", int, 3),
    ("output_width", int, 32), ("aspect_ratio", float, 1.0),
]


class _NoTTUR(argparse.Action):
    """--no_TTUR.  The reference's option setter parses the command line itself to see this flag and moves the DEFAULTS of beta1 / beta2 to
    (0.5, 0.999) (spade_model.py:254-258); here the flag does that when the parser meets it -- the option passes that follow (the dataset's,
    the final one) then start from those defaults, and an explicit --beta1 / --beta2 still wins."""

    def __init__(self, option_strings, dest, **kw):
        super().__init__(option_strings, dest, nargs=0, default=False, required=False)

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, True)
        parser.set_defaults(beta1=0.5, beta2=0.999)


class SPADEModel(PatchBaselineModel):
    @staticmethod
    def modify_commandline_options(parser, is_train=True):
        add_baseline_flags(parser, MODEL_FLAGS, vgg=True)
        parser.add_argument("--no_TTUR", action=_NoTTUR)
        # (normG / normD / netG arrive as defaults: the base parser's `choices` list none of these values, as upstream)
        parser.set_defaults(norm="batch", ngf=64, dataset_mode="aligned", dataset="patchskit", crop_size=1536, pool_size=0, n_epochs=50,
                            n_epcohs_decay=0, netG="spade", netD="multiscale", normG="spectralspadesyncbatch3x3", normD="spectralinstance",
                            lr=0.0002, gan_mode="hinge", num_D_D1=2, num_D_D2=2, beta1=0.0, beta2=0.9)
        set_phase_defaults(parser, is_train, batch_size=16)
        if is_train:
            parser.set_defaults(output_width=32)
        else:
            parser.set_defaults(load_size=1800, output_width=1536)
        return parser

    def _define_G(self, opt):
        return networks.define_G(opt.sketch_nc, opt.image_nc + opt.touch_nc, opt.ngf, "spade", opt.norm, gpu_ids=self.gpu_ids, opt=opt)

    def _define_Ds(self, opt):
        return [networks.define_D(nc + opt.sketch_nc, opt.ndf, "multiscale", opt.n_layers_D, opt.norm, num_D=num_D, gpu_ids=self.gpu_ids, opt=opt)
                for nc, num_D in ((opt.image_nc, opt.num_D_D1), (opt.touch_nc, opt.num_D_D2))]

    def _make_optimizers(self, opt):
        g_lr, d_lr = self.learning_rates(opt)
        betas = (opt.beta1, opt.beta2)
        return FlatAdam(self.flatG, g_lr, betas), FlatAdam(self.flatD, d_lr, betas), FlatAdam(self.flatD2, d_lr, betas)

    def _build_own(self, opt):
        if self.isTrain and opt.pool_size > 0 and len(self.gpu_ids) > 1:
            raise NotImplementedError("Fake Pool Not Implemented for MultiGPU")      # (spade_model.py:331-332)
        # (the reference constructs fake_pool and never queries it, :333 / :601-621: nothing to build)
        self._build_vgg(opt)      # (spade_model.py:338-339)

    @staticmethod
    def learning_rates(opt):
        """(G, D) initial rates, spade_model.py:415-423: the two-time-scale rule halves G's and doubles the discriminators' unless --no_TTUR"""
        return (opt.lr, opt.lr) if opt.no_TTUR else (opt.lr / 2, opt.lr * 2)

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

    # ------------------------------------------------------------------ training step
    def _g_forward(self, keep):
        h, w = self.real_S.shape[2:]
        g_out, ctx = engine.spade_forward(self.netG, self.real_S, keep=keep)
        if tuple(g_out.shape[2:]) != (h, w):
            raise ValueError("SPADE generator output %dx%d does not match the %dx%d input: --output_width / --aspect_ratio / "
                             "--num_upsampling_layers fix the output size" % (g_out.shape[2], g_out.shape[3], h, w))
        return g_out, ctx

    def _g_extra_terms(self, d_fake_I, d_fake_T):
        if self.netVGG is None:
            return
        # VGG feature matching (spade_model.py:662-675): the image, and gx / gy each tiled to three channels, as one batch of 6 N rows
        from vts import perceptual as P_
        slot = self._slot
        P_.vgg_feature_l1_stacked(self.netVGG, self.fake_I, self.fake_T, self.real_I, self.real_T, self.opt.lambda_vgg,
                                  slot["G_VGG_I"], slot["G_VGG_T"], d_fake_I=d_fake_I, d_fake_T=d_fake_T, accumulate=True)
        slot["G_VGG"].copy_(slot["G_VGG_I"] + slot["G_VGG_T"])

    def _g_backward(self, d_raw):
        # (d_raw is the gradient of the PRE-tanh output: g_out_grad applies the tanh adjoint; the sketch is data: nobody reads its gradient)
        engine.spade_backward(self.netG, self._g_ctx, d_raw, want_dseg=False, pre_tanh=True)
