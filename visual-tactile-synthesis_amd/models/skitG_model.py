"""SKITGModel: the multi-object variant -- SinSKITGModel plus style-code conditioning.

Reference: /root/reference/models/skitG_model.py.  Its flags (:44-350) and forward
(:1284-1336, style code tiled over the innermost map and concatenated, networks.py:1600-1623)
are mirrored; its published optimize_parameters is broken (argument mismatches at :625-632 /
:651-653, SURVEY.md finding 3), so the train step follows the consistent SinSKITGModel
schedule, as the survey prescribes.

The style code comes from a frozen CLIP ViT-B/32 image tower run in half precision on the masked
visual image (`net_style`, :484-489, 704-724, 1294-1296).  A batch that carries a ready 512-d
`style_code` keeps precedence (the synthetic dataset emits a seeded unit vector, the `skit` dataset a
pre-computed `style_code.npy`) and the encoder is then never constructed.  Without one, set_input
computes the code on the device: `style_I` (x `style_M` under use_bg_mask) when the batch has it, else
the masked `real_I`, through CLIP's pre-processing (vts_clip_preprocess, bit-exact with the host chain)
and the tower (models/clip_visual.py -> vts_clip_visual_forward).  The published weights cannot exist
offline: `--clip_weights` / $VTS_CLIP_WEIGHTS loads them, otherwise the tower runs on seeded stand-in
weights, announced once, and `style_code_pretrained` is False.
Not built: the vision-aided discriminator D3 (it needs the tower's backward and CLIP's multi-level heads).
"""
from vts import ops
from vts.misc import str2bool

from .sinskitG_model import SinSKITGModel, add_model_flags

B = str2bool

STYLE_FLAGS = [
    ("use_style_code", B, False), ("style_code_mode", str, "concat", ["concat", "adain"]),
    ("style_code_mapping_mode", str, "tile", ["tile", "project"]), ("style_code_dim", int, 512),
    ("num_layer_style_code", int, 1), ("use_external_test_input", B, False),
    ("test_sketch_material", str, "BlackJeans"), ("test_style_material", str, "BlackJeans"),
]


class SKITGModel(SinSKITGModel):
    MODEL_NAME = "skitG"
    DATASET_MODE = "skit"
    DATAROOT = "./datasets/singleskit_BluePants_padded_1800_x1/"
    DATA_LEN = 100

    @staticmethod
    def add_extra_flags(parser):
        add_model_flags(parser, STYLE_FLAGS)
        parser.add_argument("--material_list", type=str, nargs="+", default=[])
        # (not a reference flag) the CLIP checkpoint of the style encoder: a state dict or clip's TorchScript archive (ViT-B-32.pt)
        parser.add_argument("--clip_weights", type=str, default="")
        parser.set_defaults(use_style_code=True)

    net_style = None                 # the frozen CLIP image tower: built by the first batch that carries no style_code
    style_code_pretrained = None     # False: the stored style code came from seeded stand-in weights

    def _style_encoder(self):
        if self.net_style is None:
            from .clip_visual import clip_visual

            if self.opt.style_code_dim != 512:
                raise ValueError("--style_code_dim %d: the CLIP ViT-B/32 style encoder emits 512 values" % self.opt.style_code_dim)
            self.net_style = clip_visual(self.opt).to(self.device)
            self.style_code_pretrained = bool(self.net_style.pretrained)
            if not self.net_style.pretrained:
                print("WARNING: the style code is computed by a CLIP ViT-B/32 tower on SEEDED STAND-IN weights: no --clip_weights / "
                      "$VTS_CLIP_WEIGHTS given.  Such codes compare runs of this package on the same seed only (style_code_pretrained False); "
                      "pass --clip_weights <clip ViT-B-32.pt or its state dict> or put a style_code in the batch.", flush=True)
        return self.net_style

    def set_input(self, input, phase="train", timing=False, verbose=False):
        super().set_input(input, phase=phase, timing=timing, verbose=verbose)
        if not self.opt.use_style_code or "style_code" in input:
            return
        # the reference's set_input (:705-724) and forward (:1294-1296), on the device: no host round trip, no PIL
        if "style_I" in input:
            src = self._load(phase + "_style_I", input["style_I"])
            if self.opt.use_bg_mask:
                src = ops.mask_mul(src, self._load(phase + "_style_M", input["style_M"]), out=self._buf(phase + "_style_IM", src.shape))
        elif hasattr(self, "real_I"):
            src = self.real_I
        else:
            self.style_code = None      # _style() reports it
            return
        n, _, h, w = self.real_S.shape
        self.style_code = self._style_encoder().encode(src, out=self._buf(phase + "_style", (src.shape[0], self.opt.style_code_dim)))
        self._tile_style_code(phase, n, h, w)

    def _style(self):
        if not self.opt.use_style_code:
            return None
        if self.style_code is None:
            raise RuntimeError("skitG with --use_style_code True needs batch['style_code'] ([N, %d]), or an image to encode one from "
                               "(batch['style_I'] or batch['I'])" % self.opt.style_code_dim)
        return self.style_code
