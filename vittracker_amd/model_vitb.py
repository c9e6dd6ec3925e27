"""Model-level drop-in for the plain-ViT OSTrack path (ViT-Base, BASELINE config 4, ViT-Large, ViT-Small, ViT-Tiny): ``build_ostrack(cfg, training=False) -> OSTrack``
with the surface the reference's callers use (``lib/models/ostrack/ostrack.py:22-151,164-286``):

    net = build_ostrack(cfg, training=False)            # MODEL.BACKBONE.TYPE = vit_base_patch16_224[_ce] | vit_{large,small,tiny}_patch16_224, HEAD = CENTER / 256
    net = build_small_ostrack(cfg, training=False)      # the reference's depth-3 students: TYPE vit_base_patch16_224_ce, CHANNELS / HEADS = 192 / 3, 384 / 6, 768 / 12
    net.load_state_dict(ckpt['net'], strict=False)      # keys backbone.* / box_head.*
    net = net.cuda(); net.eval()
    out = net.forward(template=z, search=x)             # {'pred_boxes','score_map','size_map','offset_map'}
    net.box_head.cal_bbox(score, size, offset)

Arithmetic runs in ``libvittrack_hip.so`` (bf16 MFMA contractions, f32 accumulate / LayerNorm / softmax / residual stream);
no CPU execution path.

The candidate-elimination backbone ``vit_base_patch16_224_ce`` (``lib/models/ostrack/vit_ce.py``; every published OSTrack checkpoint) is
accepted with a non-empty ``CE_LOC`` of the length of ``CE_KEEP_RATIO`` and runs in one of two forms (``native.Model.set_candidate_elimination``,
DESIGN.md 11.4): by key masking (``ce_form="masked"``, the default: no token moves, nothing is faster) or compacted (``ce_form="compact"``:
the kept tokens are gathered into shorter frames behind every stage, as the reference does).  Either way the kept tokens take the
reference's values and removed tokens come back as zeros.  ``ce_form=None`` reads the environment variable ``VB_CE_FORM``.  The template rows of
the score come from ``CE_TEMPLATE_RANGE`` as ``lib/utils/ce_utils.py:15-49`` picks them (``ALL``, ``CTR_POINT``, ``CTR_REC``), one
selection per model.  Not implemented (NotImplementedError): candidate elimination at any width but 768 (ViT-Large, ViT-Small and ViT-Tiny CE), ``CE_TEMPLATE_RANGE: GT_BOX``, a ``ce_keep_rate`` argument
of ``forward``, a ``_ce`` TYPE without ``CE_LOC``, and the prompt / draw variants (``MODEL.PROCESS.*``)."""
from __future__ import annotations

from collections import OrderedDict

from . import native, synth
from .config import geometry
from .model import CenterHead, OstrackDist


#: what MODEL.BACKBONE.TYPE fixes for the large backbone (lib/models/ostrack/vit.py:393-400: embed_dim, num_heads, depth).  As in the
#: reference the TYPE decides: CHANNELS / HEADS of the YAML are not read for it.
VIT_LARGE = {"channels": 1024, "heads": 16, "depth": 24}
#: the small students under timm's names (DeiT-Small / DeiT-Tiny; the reference ships no such TYPE): again the TYPE decides
VIT_SMALL = {"channels": 384, "heads": 6, "depth": 12}
VIT_TINY = {"channels": 192, "heads": 3, "depth": 12}
TYPE_FIXES = {"vit_large_patch16_224": VIT_LARGE, "vit_small_patch16_224": VIT_SMALL, "vit_tiny_patch16_224": VIT_TINY}
#: (CHANNELS, HEADS) build_small_ostrack accepts (lib/models/ostrack/ostrack.py:301-308 passes them on as they are; these are the widths with kernels)
SMALL_WIDTHS = ((192, 3), (384, 6), (768, 12))

#: generate_mask_cond (lib/utils/ce_utils.py:22-49): the slice of template map rows AND columns that is set, per template map side of the two geometries (8: 128 px, 12: 192 px)
CE_RANGE_SLICES = {"CTR_POINT": {8: (3, 4), 12: (5, 6)}, "CTR_REC": {8: (3, 5), 12: (5, 7)}}


def ce_template_rows(template_range: str, feat_sz_z: int):
    """box_mask_z of generate_mask_cond (lib/utils/ce_utils.py:15-49) for one sample, as a list of feat_sz_z ** 2 booleans; None for ALL
    (every row).  CTR_POINT: row 27 at 8 x 8, row 65 at 12 x 12; CTR_REC: rows 27, 28, 35, 36 and 65, 66, 77, 78."""
    template_range = str(template_range)
    if template_range == "ALL":
        return None
    if template_range == "GT_BOX":
        raise NotImplementedError("CE_TEMPLATE_RANGE GT_BOX (a template mask per frame from the ground-truth box) is not implemented: "
                                  "ALL, CTR_POINT and CTR_REC are")
    sl = CE_RANGE_SLICES.get(template_range, {}).get(int(feat_sz_z))
    if sl is None:
        raise NotImplementedError(f"CE_TEMPLATE_RANGE {template_range!r} at a {feat_sz_z} x {feat_sz_z} template map")      # ce_utils.py:32,46,63
    rows = [False] * (feat_sz_z * feat_sz_z)
    for y in range(*sl):
        for x in range(*sl):
            rows[y * feat_sz_z + x] = True
    return rows


class OSTrack(OstrackDist):
    family = "vit"      # vt_create_vit: 384 / 6 and 192 / 3 are LeViT-stem vit_dist models under vt_create

    def __init__(self, cfg, depth=None, max_batch=1, ce_form=None, small=False, precision=None):
        """small: build_small_ostrack's model -- TYPE vit_base_patch16_224_ce at depth 3 with the YAML's CHANNELS / HEADS, CE_LOC may be empty.
        precision: "bf16" | "fp32" (native.Model.set_precision: the fp32-equivalent mode on three-piece bf16 operands); None:
        the environment variable VB_PRECISION, else "bf16".  The fp32 mode and a candidate-elimination backbone exclude each other."""
        g = geometry(cfg)
        if g["head_type"] != "CENTER":
            raise ValueError("HEAD TYPE %s is not supported." % g["head_type"])
        bb_type = str(cfg.MODEL.BACKBONE.TYPE)
        self.ce_loc, self.ce_keep_ratio, self.ce_rows = [], [], None
        self.ce_form = native.ce_form_name(ce_form)      # "masked" | "compact"; read by a candidate-elimination backbone only
        self.precision = native.vit_precision_name(precision)
        if small:
            if bb_type != "vit_base_patch16_224_ce":
                raise NotImplementedError(f"build_small_ostrack: backbone {cfg.MODEL.BACKBONE.TYPE!r}: only vit_base_patch16_224_ce (depth 3, CHANNELS / HEADS "
                                          "from the YAML) is implemented")
            if (g["channels"], g["heads"]) not in SMALL_WIDTHS:
                raise NotImplementedError(f"build_small_ostrack: (CHANNELS, HEADS) = ({g['channels']}, {g['heads']}): implemented are "
                                          + ", ".join(str(w) for w in SMALL_WIDTHS))
            depth = 3 if depth is None else depth
            self.ce_loc = [int(v) for v in cfg.MODEL.BACKBONE.CE_LOC]
            if self.ce_loc:      # (an empty CE_LOC: the plain depth-3 model, CE_KEEP_RATIO is not read)
                self.ce_keep_ratio = [float(v) for v in cfg.MODEL.BACKBONE.CE_KEEP_RATIO]
                if g["channels"] != 768:
                    raise NotImplementedError("candidate elimination is implemented for width 768 only")
                if len(self.ce_loc) != len(self.ce_keep_ratio):
                    raise ValueError(f"CE_LOC {self.ce_loc} and CE_KEEP_RATIO {self.ce_keep_ratio} must have the same length")
                self.ce_rows = ce_template_rows(cfg.MODEL.BACKBONE.CE_TEMPLATE_RANGE, g["template_size"] // g["stride"])
        elif bb_type in TYPE_FIXES:
            fixed = TYPE_FIXES[bb_type]
            g["channels"], g["heads"] = fixed["channels"], fixed["heads"]
            depth = fixed["depth"] if depth is None else depth
        elif bb_type == "vit_base_patch16_224":
            depth = 12 if depth is None else depth
        elif bb_type == "vit_base_patch16_224_ce":
            depth = 12 if depth is None else depth
            self.ce_loc = [int(v) for v in cfg.MODEL.BACKBONE.CE_LOC]
            self.ce_keep_ratio = [float(v) for v in cfg.MODEL.BACKBONE.CE_KEEP_RATIO]
            if not self.ce_loc or not self.ce_keep_ratio:
                raise NotImplementedError("backbone 'vit_base_patch16_224_ce' without CE_LOC / CE_KEEP_RATIO: give MODEL.BACKBONE.CE_LOC and "
                                          "CE_KEEP_RATIO (the published models: [3, 6, 9] and [0.7, 0.7, 0.7]) or use TYPE vit_base_patch16_224")
            if len(self.ce_loc) != len(self.ce_keep_ratio):
                raise ValueError(f"CE_LOC {self.ce_loc} and CE_KEEP_RATIO {self.ce_keep_ratio} must have the same length")
            self.ce_rows = ce_template_rows(cfg.MODEL.BACKBONE.CE_TEMPLATE_RANGE, g["template_size"] // g["stride"])
        else:
            raise NotImplementedError(f"backbone {cfg.MODEL.BACKBONE.TYPE!r}: only vit_base_patch16_224, vit_base_patch16_224_ce, "
                                      "vit_large_patch16_224, vit_small_patch16_224 and vit_tiny_patch16_224 are implemented")
        if self.precision == "fp32" and self.ce_loc:
            raise NotImplementedError("precision 'fp32' and candidate elimination (CE_LOC %s) exclude each other: the fp32 mode ranks no tokens; "
                                      "use TYPE vit_base_patch16_224 or precision 'bf16'" % self.ce_loc)
        if str(cfg.MODEL.BACKBONE.CAT_MODE) != "direct":
            raise NotImplementedError("only CAT_MODE 'direct' (template tokens first) is implemented")
        self.geom, self.depth, self.mode, self.head_type, self.max_batch = g, depth, "eval", "CENTER", max_batch
        self.feat_sz_s, self.feat_len_s = g["feat_sz"], g["len_x"]
        self.box_head = CenterHead(self, g["feat_sz"], g["stride"])
        self._state = OrderedDict(synth.synth_vitb_state_dict(0, C=g["channels"], depth=depth, heads=g["heads"],
                                                              head_ch=g["head_channels"], len_z=g["len_z"], len_x=g["len_x"]))
        self._nat, self._device, self.training = None, None, False

    def _native(self) -> native.Model:
        fresh = self._nat is None
        nat = OstrackDist._native(self)
        if fresh and nat.precision != self.precision:      # (VB_PRECISION has chosen at vt_create already; an explicit argument overrides it)
            nat.set_precision(self.precision)
        if fresh and self.ce_loc:      # every entry point of the native model (forward, forward_u8, track_step*, captures) then runs with it
            nat.set_candidate_elimination(self.ce_loc, self.ce_keep_ratio, self.ce_rows, form=self.ce_form)
        return nat

    def _check_ce_mask(self, mask, B):
        """The model has ONE selection of template rows (per-frame masks are not implemented): `mask` must repeat it for every sample."""
        import torch
        lz = self.geom["len_z"]
        want = torch.tensor(self.ce_rows if self.ce_rows is not None else [True] * lz, dtype=torch.bool)
        if not (isinstance(mask, torch.Tensor) and mask.dtype == torch.bool and tuple(mask.shape) == (B, lz)):
            raise ValueError(f"ce_template_mask must be None or a ({B}, {lz}) bool tensor, got {type(mask).__name__} "
                             f"{tuple(getattr(mask, 'shape', ()))} {getattr(mask, 'dtype', '')}")
        if not bool((mask.cpu() == want[None]).all()):
            raise ValueError("ce_template_mask differs from the model's template rows (CE_TEMPLATE_RANGE "
                             "fixes one selection per model; per-frame masks are not implemented)")

    def forward(self, template, search, ce_template_mask=None, ce_keep_rate=None, **unused):
        """OSTrack.forward (ostrack.py:47-120).  Plain backbone: no CE mask, no template / search pre-processing.  CE backbone:
        ce_template_mask None or the model's own rows for every sample; the dict gains 'removed_indexes_s', per stage the (B, r_k) int64
        global search indices removed there, ascending (the reference: descending score, as floats; only its visualisation reads them)."""
        extra = {k: v for k, v in unused.items() if v is not None and v is not False}
        if not self.ce_loc:
            if ce_template_mask is not None:
                extra["ce_template_mask"] = ce_template_mask
            if ce_keep_rate is not None:
                extra["ce_keep_rate"] = ce_keep_rate
        if extra:
            raise NotImplementedError(f"OSTrack.forward arguments {sorted(extra)} belong to variants that are not implemented")
        if not self.ce_loc:
            return OstrackDist.forward(self, template, search)
        if ce_keep_rate is not None:
            raise NotImplementedError("ce_keep_rate (the training schedule's keep rate) is not implemented: the model runs CE_KEEP_RATIO")
        B = search.shape[0]
        if ce_template_mask is not None:
            self._check_ce_mask(ce_template_mask, B)
        out = OstrackDist.forward(self, template, search)
        out["removed_indexes_s"] = self.removed_indexes(B)
        return out

    def removed_indexes(self, B):
        """Per stage the (B, r_k) int64 global search indices the last call removed there, ascending; no host synchronisation."""
        import torch
        nat = self._native()
        removed, _ = nat.ce_result(B)
        out, prev = [], nat.len_x
        for k, keep in enumerate(nat.ce_keep):
            # a stable sort of "not removed at this stage" puts the stage's tokens first, in index order
            order = torch.sort((removed != k + 1).to(torch.uint8), dim=1, stable=True).indices
            out.append(order[:, :prev - keep].contiguous())
            prev = keep
        return out

    __call__ = forward


def build_ostrack(cfg, training=False, max_batch=1, ce_form=None, precision=None):
    """ce_form: "masked" | "compact", the form a candidate-elimination backbone runs in; None: VB_CE_FORM, else "masked".
    precision: "bf16" | "fp32" (the fp32-equivalent mode); None: VB_PRECISION, else "bf16"."""
    if training:
        raise NotImplementedError("inference graph only")
    return OSTrack(cfg, max_batch=max_batch, ce_form=ce_form, precision=precision)


def build_small_ostrack(cfg, training=False, max_batch=1, ce_form=None, precision=None):
    """The reference's build_small_ostrack (lib/models/ostrack/ostrack.py:288-342; its tracking/profile_model*.py and onnxexport.py build exactly
    this): TYPE vit_base_patch16_224_ce at depth 3, width / heads from MODEL.BACKBONE.CHANNELS / HEADS -- (192, 3), (384, 6) or (768, 12).  An
    empty CE_LOC is the plain depth-3 model; a non-empty one runs at width 768 through build_ostrack's candidate-elimination machinery and
    raises NotImplementedError at the small widths."""
    if training:
        raise NotImplementedError("inference graph only")
    return OSTrack(cfg, max_batch=max_batch, ce_form=ce_form, small=True, precision=precision)
