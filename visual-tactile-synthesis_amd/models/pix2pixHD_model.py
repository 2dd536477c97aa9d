"""pix2pixHD baseline on the HIP path (reference: models/pix2pixHD_model.py).

The reference trains this baseline patch-wise (`return_patch=True`: 32x32 sketch / image / tactile patches,
batch 32) with the coarse `GlobalGenerator`, two multiscale PatchGAN discriminators (D: sketch ++ image,
D2: sketch ++ tactile, both with `getIntermFeat`) and the LSGAN objective:

    forward            pix2pixHD_model.py:587-619     G(S) -> fake_I = out[:, :3] * M, fake_T = out[:, -2:] * M_T
    backward_D         :621-644                        0.5 (D_fake + D_real) + 0.5 (D2_fake + D2_real), one backward
    backward_G         :646-700                        G_GAN_I + G_GAN_T (+ feature matching + VGG)
    optimize_parameters :702-722                       D and D2 step, then G step

The GAN feature-matching term of the reference compares every discriminator feature with ITSELF (.detach(),
:662-680), so its value and gradient are identically zero: it is reported as 0.  The VGG feature term (VGGLoss on torchvision's VGG19,
networks.py:2021-2067) runs on the GEMM-class kernels (vts/perceptual.py); its pretrained weights cannot exist offline:
`--vgg_weights` loads them, otherwise seeded stand-ins are used and `loss_vgg_pretrained` is False.
The step itself is PatchBaselineModel's (models/patch_baseline.py); what is this model's own: the image pool in front of D's fake pass, the
generator's optimiser over a parameter span (--niter_fix_global), and the generator's backward in stages under its gradient buckets.
"""
import os

from vts.misc import str2bool
from vts import engine, ops
from vts.ops import Act
from vts.optim import FlatAdam

from . import networks
from .patch_baseline import PatchBaselineModel, add_baseline_flags, set_phase_defaults

B = str2bool

# (flag, type, default[, choices]) besides patch_baseline.COMMON_FLAGS  -- reference: pix2pixHD_model.py:45-200
MODEL_FLAGS = [
    ("return_patch", B, True), ("label_nc", int, 0), ("data_type", int, 32, [8, 16, 32]), ("no_instance", B, True),
    ("instance_feat", B, False), ("label_feat", B, False), ("feat_num", int, 3), ("load_features", "flag", False),
    ("n_downsample_E", int, 4), ("nef", int, 16), ("n_clusters", int, 10), ("n_downsample_global", int, 4),
    ("n_blocks_global", int, 9), ("n_blocks_local", int, 3), ("n_local_enhancers", int, 1), ("niter_fix_global", int, 0),
    ("getIntermFeat_D", B, True), ("num_D_D1", int, 2), ("num_D_D2", int, 2), ("no_gan_loss", B, False),
    ("no_ganFeat_loss", B, False), ("no_vgg_loss", B, False), ("lambda_feat", float, 10.0), ("lambda_vgg", float, 10.0),
    ("niter_decay", int, 100), ("separate_val_set", B, False), ("fp16", "flag", False),
]


class Pix2PixHDModel(PatchBaselineModel):
    @staticmethod
    def modify_commandline_options(parser, is_train=True):
        add_baseline_flags(parser, MODEL_FLAGS, vgg=True)
        parser.set_defaults(norm="batch", netG="global", netD="multiscale", ngf=64, dataset_mode="aligned", dataset="patchskit",
                            crop_size=1536, normG="instance", normD="instance", pool_size=0, n_epochs=50, n_epcohs_decay=150,
                            gan_mode="lsgan")
        set_phase_defaults(parser, is_train, batch_size=32)
        return parser

    def _define_G(self, opt):
        return networks.define_G(opt.sketch_nc, opt.image_nc + opt.touch_nc, opt.ngf, opt.netG, opt.norm, gpu_ids=self.gpu_ids, opt=opt)

    def _define_Ds(self, opt):
        return [networks.define_D(nc + opt.sketch_nc, opt.ndf, opt.netD, opt.n_layers_D, opt.norm, num_D=num_D, gpu_ids=self.gpu_ids, opt=opt)
                for nc, num_D in ((opt.image_nc, opt.num_D_D1), (opt.touch_nc, opt.num_D_D2))]

    def _make_optimizers(self, opt):
        betas = (opt.beta1, 0.999)
        return (FlatAdam(self.flatG, opt.lr, betas, span=self._finetune_span(opt)), FlatAdam(self.flatD, opt.lr, betas),
                FlatAdam(self.flatD2, opt.lr, betas))

    def _build_own(self, opt):
        # data parallel: the generator's gradient travels as up to 8 buckets cut at layer boundaries, each started as soon as the backward
        # has written it (_segments); VTS_G_BUCKETS=1: one bucket behind the whole backward; VTS_G_BUCKET_MIN_MB: smallest bucket worth a collective
        if not getattr(self.netG, "is_local_enhancer", False):     # (the local enhancer's backward is a tree, not a chain: one bucket)
            self.flatG.chunk(int(os.environ.get("VTS_G_BUCKETS", "8")), min_floats=int(float(os.environ.get("VTS_G_BUCKET_MIN_MB", "16")) * (1 << 18)))
        if self.isTrain:
            if opt.pool_size > 0 and len(self.gpu_ids) > 1:
                raise NotImplementedError("Fake Pool Not Implemented for MultiGPU")      # (pix2pixHD_model.py:332-333)
            from util.image_pool import ImagePool
            self.fake_pool = ImagePool(opt.pool_size)
        self._build_vgg(opt)

    def _finetune_span(self, opt):
        """--niter_fix_global > 0 (pix2pixHD_model.py:403-421): optimizer_G is built over the parameters whose name starts with
        "model<n_local_enhancers>" only -- the last local enhancer, the tail of the flat buffer -- until update_fixed_params()."""
        if opt.niter_fix_global <= 0:
            return None
        prefix = "model" + str(opt.n_local_enhancers)
        lo, o, seen = None, 0, False
        for k, p in self.netG.named_parameters():
            hit = k.startswith(prefix)
            if hit and lo is None:
                lo = o
            if seen and not hit:
                raise RuntimeError("niter_fix_global: the finetuned parameters are not one contiguous range of the flat buffer")
            seen = seen or hit
            o += p.numel()
        if lo is None:     # netG 'global' has no such layer: the reference's Adam raises on the empty list
            raise ValueError("optimizer got an empty parameter list (--niter_fix_global needs --netG local)")
        print("------------- Only training the local enhancer network (for %d epochs) ------------" % opt.niter_fix_global)
        return (lo, o)

    def update_fixed_params(self):
        """pix2pixHD_model.py:942-949 (train.py:209-211 calls it at epoch niter_fix_global): a NEW Adam over all of netG -- fresh moments,
        step 0, the initial rate until the next update_learning_rate"""
        self.optimizer_G = FlatAdam(self.flatG, self.opt.lr, (self.opt.beta1, 0.999))
        self.optimizers[0] = self.optimizer_G
        self._drop_graphs()
        if self.opt.verbose:
            print("------------ Now also finetuning global generator -----------")

    @staticmethod
    def _check_unbuilt(opt):
        bad = []
        if not opt.no_instance or opt.instance_feat or opt.label_feat or opt.label_nc != 0 or opt.load_features:
            # not reachable in the reference either: its forward() hands encode_input inst = image = feat = None (pix2pixHD_model.py:592-597),
            # so --no_instance False dies on `inst_map.data` (:545-546), --instance_feat / --label_feat on netE.forward(None, ..) (:601-603)
            # and --load_features on `feat_map.data` (:558-559); --label_nc > 0 one-hots the SKETCH values (:533-541)
            bad.append("instance / label feature inputs (netE, label_nc > 0): the reference's forward() passes inst = image = feat = None "
                       "(models/pix2pixHD_model.py:592-603), so these flags fail upstream as well and there is no behaviour to restate")
        if opt.netG not in ("global", "local"):
            bad.append("netG %s (built: global, local)" % opt.netG)
        if opt.netD in ("basic", "n_layers"):      # define_D builds these for the pix2pix baseline; this step is not wired to them
            bad.append("netD %s (built: multiscale)" % opt.netD)
        if opt.fp16 or opt.T_resolution_multiplier != 1 or not opt.use_bg_mask:
            bad.append("fp16 / T_resolution_multiplier != 1 / use_bg_mask False")
        if opt.isTrain and opt.no_gan_loss:
            bad.append("no_gan_loss")
        if bad:
            raise NotImplementedError("pix2pixHD on the HIP path: " + "; ".join(bad))

    # ------------------------------------------------------------------ training step
    def _g_forward(self, keep):
        return engine.resnet_forward(self.netG, Act(self.real_S), keep=keep)

    def _pool_fake(self, job):
        if self.fake_pool.pool_size > 0:
            # backward_D's fake pass of D sees fake_pool.query(cat(label, fake_I)) (pix2pixHD_model.py:582, 626): label and image pooled
            # as parallel stores under one plan (drawn in optimize_parameters, outside the captured graphs)
            job["in0"] = self.fake_pool.apply("label", self.real_S)
            job["in1"] = self.fake_pool.apply("image", self.fake_I)

    def _g_extra_terms(self, d_fake_I, d_fake_T):
        if self.netVGG is None:
            return
        # VGG feature matching (pix2pixHD_model.py:680-693): the image, and gx / gy each tiled to three channels
        from vts import perceptual as P_
        lam, slot = self.opt.lambda_vgg, self._slot
        d_fake_I.add_(P_.vgg_feature_l1(self.netVGG, self.fake_I, self.real_I, lam, slot["G_VGG_I"]))
        for c in (0, 1):
            f3 = self.fake_T[:, c:c + 1].expand(-1, 3, -1, -1).contiguous()
            r3 = self.real_T[:, c:c + 1].expand(-1, 3, -1, -1).contiguous()
            g3 = P_.vgg_feature_l1(self.netVGG, f3, r3, lam, slot["G_VGG_T"])
            ops.lpips_input_bwd(g3, (1.0, 1.0, 1.0), d_fake_T[:, c:c + 1], 1, accumulate=True)     # adjoint of the tiling: sum of the three
        slot["G_VGG"].copy_(slot["G_VGG_I"] + slot["G_VGG_T"])

    def _g_backward(self, d_raw):
        if self._g_stages():
            # data parallel, chunked generator bucket: only the LAST stage of the backward here (the layers of the last bucket)
            b = engine.resnet_stage_bounds(self._g_ctx, self.flatG.cut_params)
            self._g_bounds = b
            self._g_flow = engine.resnet_backward_stage(self.netG, self._g_ctx, d_raw, b[-2], b[-1])
        else:
            engine.resnet_backward(self.netG, self._g_ctx, d_raw)

    def _seg_g_stage(self, j):
        """stage j of the generator's backward (the layers of gradient bucket G_j), j = K-2 .. 0"""
        b = self._g_bounds
        self._g_flow = engine.resnet_backward_stage(self.netG, self._g_ctx, self._g_flow, b[j], b[j + 1])

    def _g_stages(self):
        """number of stages of the generator's backward = chunks of its gradient bucket when the step runs data parallel, else 0"""
        from vts import ddp as _ddp
        if self.ddp is None or not _ddp.active() or not getattr(self.flatG, "cuts", None):
            return 0
        return len(self.flatG.cuts) + 1

    def _segments(self):
        """(segment, buckets to wait for before it, buckets to start after it).  Data parallel: the generator's gradient (730 MB at the
        reference's ngf 64) travels as K buckets cut at layer boundaries; the backward runs as K stages from the output layer down, and
        the all-reduce of bucket j starts as soon as stage j has written it, under the stages below."""
        K = self._g_stages()
        if not K:
            return [(self._seg_forward_d, (), ("D", "D2")), (self._seg_adam_d_g, ("D", "D2"), ("G",)), (self._seg_adam_g, ("G",), ())]
        segs = [(self._seg_forward_d, (), ("D", "D2")), (self._seg_adam_d_g, ("D", "D2"), ("G_%d" % (K - 1),))]
        for j in range(K - 2, -1, -1):
            segs.append((lambda j=j: self._seg_g_stage(j), (), ("G_%d" % j,)))
        segs.append((self._seg_adam_g, tuple("G_%d" % j for j in range(K - 1, -1, -1)), ()))
        return segs

    def optimize_parameters(self, epoch=0, timing=False):
        if self.fake_pool.pool_size > 0:
            if self.ddp is not None:
                from vts import ddp as _ddp
                if _ddp.active():
                    raise NotImplementedError("Fake Pool Not Implemented for MultiGPU")
            self.fake_pool.next_batch(self.real_S.shape[0], self.device)
        self._run_step()
