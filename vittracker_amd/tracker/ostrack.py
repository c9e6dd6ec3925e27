"""Tracker plugin: ``OSTrack`` -- the ViT-Base / ViT-Large OSTrack tracker with the reference's ``initialize() / track()`` contract
(``lib/test/tracker/ostrack.py:23-189`` for the ``vit_base_patch16_224`` / ``vit_base_patch16_224_ce`` / ``vit_large_patch16_224`` backbones and the small students ``vit_small_patch16_224`` / ``vit_tiny_patch16_224``), on the
MI355X-native library.

The frame step of the two reference trackers is the same statement -- ``sample_target``, ``Preprocessor.process``, the network,
the Hann-windowed ``cal_bbox``, ``map_box_back`` + ``clip_box(margin=10)`` -- and they differ in the network behind it.  So this class
IS :class:`vittracker_amd.tracker.vit_dist.Vit_dist` with the network chosen by the cfg (:mod:`vittracker_amd.factory`): the per-process
pipeline pool, the device pipeline by default (crop -> uint8 patch -> network on the cached template -> state tail as one captured
library call, ``native.Image`` frames accepted), ``params.host_crop = True`` for the reference's structure, ``save_all_boxes``, and
``confidence`` as a Python float where the reference leaves a 0-d tensor.

The candidate-elimination backbone (``vit_base_patch16_224_ce``, every published OSTrack checkpoint: ``experiments/ostrack/
vitb_256_mae_ce_32x4_ep300.yaml`` / ``vitb_384_mae_ce_32x4_ep300.yaml``) runs through the same class: its ``box_mask_z``
(``generate_mask_cond``, :57-62) is fixed per model from ``CE_TEMPLATE_RANGE`` when the network is built, so ``initialize()`` has nothing
to generate.  ``params.ce_form`` (``"masked"`` | ``"compact"``, ``None``: the environment variable ``VB_CE_FORM``, else masked) picks the form the
stages run in -- removed tokens as absent keys, or the kept tokens gathered into shorter frames -- with the same results.
``params.precision`` (``"bf16"`` | ``"fp32"``, ``None``: ``VB_PRECISION``, else bf16) selects the fp32-equivalent mode of the plain backbones.  Not implemented, as in :mod:`vittracker_amd.model_vitb`: ViT-Large CE, ``CE_TEMPLATE_RANGE: GT_BOX``, ``ce_keep_rate``,
``MODEL.PROCESS.*`` and the debug visualisation (``removed_indexes_s`` is returned by the model's ``forward``; nothing draws it)."""
from __future__ import annotations

from .vit_dist import BaseTracker, Vit_dist  # noqa: F401


class OSTrack(Vit_dist):
    def __init__(self, params, dataset_name):
        from ..factory import network_builder
        from ..model_vitb import build_ostrack
        if network_builder(params.cfg) is not build_ostrack:
            raise ValueError("the ostrack tracker runs the ViT-Base OSTrack model (MODEL.BACKBONE.TYPE vit_base_patch16_224, CHANNELS 768) or the "
                             "ViT-Large / -Small / -Tiny ones (TYPE vit_large_patch16_224, vit_small_patch16_224, vit_tiny_patch16_224); "
                             "this cfg names another one (tracker vit_dist runs the distilled models)")
        super().__init__(params, dataset_name)


def get_tracker_class():
    return OSTrack
