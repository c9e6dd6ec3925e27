"""One place that turns a config tree into a network: ``build_network(cfg)`` picks the ViT-Base / ViT-Large OSTrack model
(:mod:`vittracker_amd.model_vitb`, ``lib/models/ostrack/ostrack.py:164``) or the distilled vit_48 one (:mod:`vittracker_amd.model`,
``lib/models/vit_dist/vit_dist.py:159``) from ``MODEL.BACKBONE.TYPE`` / ``CHANNELS``, so that every tracker front end
(``BatchedVitTracker`` and what stands on it, the plugins' host-crop path) serves both YAML families."""
from __future__ import annotations


def network_builder(cfg):
    """The build function of cfg's model family.  The vit_dist YAMLs keep the config default ``TYPE: vit_base_patch16_224`` (the
    reference's vit_dist builder never reads it), so the width decides: 768 channels is the ViT-Base backbone, anything else
    the distilled stem + blocks of that width.  No vit_dist YAML names ``vit_large_patch16_224``: that TYPE alone selects the ViT-Large
    backbone (its width comes from the TYPE, as in the reference's build_ostrack); likewise ``vit_small_patch16_224`` / ``vit_tiny_patch16_224``
    (384 / 6 and 192 / 3).  A vit_dist YAML of 384 or 192 channels keeps the default TYPE and stays a distilled model."""
    from .model import build_ostrack_dist
    from .model_vitb import build_ostrack
    bb = cfg.MODEL.BACKBONE
    if int(bb.CHANNELS) == 768 and str(bb.TYPE).startswith("vit_base_patch16_224"):
        return build_ostrack
    if str(bb.TYPE).startswith("vit_large_patch16_224"):
        return build_ostrack
    if str(bb.TYPE) in ("vit_small_patch16_224", "vit_tiny_patch16_224"):      # timm's names: the TYPE alone selects them, as for ViT-Large
        return build_ostrack
    return build_ostrack_dist


def build_network(cfg, max_batch: int = 1, ce_form=None, precision=None):
    """ce_form: the form a candidate-elimination backbone runs in (model_vitb.build_ostrack); the vit_48 family has none.
    precision: "bf16" | "fp32", the arithmetic mode of a patch-16 ViT model (model_vitb.build_ostrack); the vit_48 family has none."""
    from .model_vitb import build_ostrack
    builder = network_builder(cfg)
    if builder is build_ostrack:
        return builder(cfg, max_batch=max_batch, ce_form=ce_form, precision=precision)
    if precision is not None:
        raise ValueError(f"precision={precision!r}: the vit_48 family has no bf16 / fp32 mode (its library is chosen by native.Model(precision=))")
    if ce_form is not None:
        raise ValueError(f"ce_form={ce_form!r}: the vit_48 family has no candidate elimination")
    return builder(cfg, max_batch=max_batch)
