"""Tracker plugin: ``OSTrack`` -- the ViT-Base / ViT-Large OSTrack tracker with the reference's ``initialize() / track()`` contract
(``lib/test/tracker/ostrack.py:23-189`` for the plain ``vit_base_patch16_224`` / ``vit_large_patch16_224`` backbones), on the MI355X-native library.

The frame step of the two reference trackers is the same statement -- ``sample_target``, ``Preprocessor.process``, the network,
the Hann-windowed ``cal_bbox``, ``map_box_back`` + ``clip_box(margin=10)`` -- and they differ in the network behind it.  So this class
IS :class:`vittracker_amd.tracker.vit_dist.Vit_dist` with the network chosen by the cfg (:mod:`vittracker_amd.factory`): the per-process
pipeline pool, the device pipeline by default (crop -> uint8 patch -> network on the cached template -> state tail as one captured
library call, ``native.Image`` frames accepted), ``params.host_crop = True`` for the reference's structure, ``save_all_boxes``, and
``confidence`` as a Python float where the reference leaves a 0-d tensor.

Not implemented, as in :mod:`vittracker_amd.model_vitb`: the candidate-elimination backbone and its ``box_mask_z``
(``generate_mask_cond``, :57-62 -- the plain backbone never reads it), ``MODEL.PROCESS.*`` and the debug visualisation."""
from __future__ import annotations

from .vit_dist import BaseTracker, Vit_dist  # noqa: F401


class OSTrack(Vit_dist):
    def __init__(self, params, dataset_name):
        from ..factory import network_builder
        from ..model_vitb import build_ostrack
        if network_builder(params.cfg) is not build_ostrack:
            raise ValueError("the ostrack tracker runs the ViT-Base OSTrack model (MODEL.BACKBONE.TYPE vit_base_patch16_224, CHANNELS 768) or the "
                             "ViT-Large one (TYPE vit_large_patch16_224); "
                             "this cfg names another one (tracker vit_dist runs the distilled models)")
        super().__init__(params, dataset_name)


def get_tracker_class():
    return OSTrack
