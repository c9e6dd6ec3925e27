"""Tracker plugin: ``Vit_dist`` with the reference's ``initialize() / track()`` contract
(``lib/test/tracker/vit_dist.py:21-156``, ``lib/test/tracker/basetracker.py:10-26``), running the
device step on the MI355X-native library.

Differences from the reference that a caller can observe (all deliberate):
  * by default the WHOLE frame step runs on the device: the uint8 frame is uploaded, ``vt_crop`` does ``sample_target`` +
    ``Preprocessor.process`` (bit-identical to the host statement in ``host_ops``), the network replays as a graph and
    ``vt_update_state`` does the map-back / clip; one device->host copy of the new state and the confidence ends the frame
    (the lock-step ``BatchedVitTracker`` with one sequence).  ``params.host_crop = True`` keeps the reference's structure --
    crop and pre-processing on the host (a numpy statement of cv2's resize: ~30 frames/s), ONE graph replay, five floats back.
    The reference launches ~130 kernels and syncs in ``.tolist()`` (:108-109) while leaving ``confidence`` as a 0-d device
    tensor (:148); here ``confidence`` is a Python float.
  * ``box_mask_z`` (``generate_mask_cond``, :62-66) is not computed: ``OstrackDist.forward``
    never consumes it, and the reference's helper raises NotImplementedError for template
    feature sizes other than 8/12/7/14 (``lib/utils/ce_utils.py:22-32``), i.e. for G128.
  * ``params.debug`` visualisation (visdom / cv2 windows, :114-138) is not implemented.
"""
from __future__ import annotations

import os

import numpy as np

from ..host_ops import Preprocessor, clip_box, hann2d, sample_target
from ..batched import check_params_geometry
from ..factory import build_network
from ..native import Image, VtError


class BaseTracker:
    """lib/test/tracker/basetracker.py:10-26 (the abstract part)."""

    def __init__(self, params):
        self.params = params
        self.visdom = None

    def predicts_segmentation_mask(self):
        return False

    def initialize(self, image, info: dict) -> dict:
        raise NotImplementedError

    def track(self, image, info: dict = None) -> dict:
        raise NotImplementedError


_PIPELINES: dict = {}      # (checkpoint, sizes, factors) -> free BatchedVitTracker(B = 1) objects of this process


class Vit_dist(BaseTracker):
    def __init__(self, params, dataset_name):
        super().__init__(params)
        import torch
        self.cfg = params.cfg
        self.preprocessor = Preprocessor()
        self.state = None
        self.feat_sz = self.cfg.TEST.SEARCH_SIZE // self.cfg.MODEL.BACKBONE.STRIDE
        self.debug = getattr(params, "debug", 0)
        self.frame_id = 0
        self.save_all_boxes = params.save_all_boxes
        self.z_dict1 = {}
        self._bt = None
        if not getattr(params, "host_crop", False):
            from ..batched import BatchedVitTracker
            # The harness makes a new tracker object per sequence (lib/test/evaluation/tracker.py:90-104); the device pipeline --
            # weights, workspaces, captured graphs -- goes back to a per-process pool when its tracker object dies and is handed
            # to the next one (initialize() resets all per-sequence state); objects alive at the same time get their own.
            key = (getattr(params, "checkpoint", None), bool(getattr(params, "allow_synthetic_weights", False)),
                   params.template_size, params.search_size, float(params.template_factor), float(params.search_factor),
                   getattr(params, "yaml_name", None), getattr(params, "ce_form", None), getattr(params, "precision", None))
            pool = _PIPELINES.setdefault(key, [])
            bt = pool.pop() if pool else BatchedVitTracker(params, 1)   # builds the network, loads the checkpoint, sets the Hann window
            bt.params = params
            self._bt = bt
            import weakref
            weakref.finalize(self, pool.append, bt)          # back to the pool when this tracker object goes away
            self.network = self._bt.net
            self.output_window = hann2d(torch.tensor([self.feat_sz, self.feat_sz]).long(), centered=True).cuda()
            return
        network = build_network(params.cfg, ce_form=getattr(params, "ce_form", None), precision=getattr(params, "precision", None))
        ckpt_path = getattr(params, "checkpoint", None)
        if ckpt_path and os.path.isfile(ckpt_path):
            network.load_state_dict(torch.load(ckpt_path, map_location="cpu")["net"], strict=False)  # :25
        elif not getattr(params, "allow_synthetic_weights", False):
            raise FileNotFoundError(
                f"checkpoint {ckpt_path!r} not found (the reference fails in torch.load at "
                f"lib/test/tracker/vit_dist.py:25); set params.allow_synthetic_weights=True to run on the "
                f"seeded synthetic weights")
        self.network = network.cuda()
        self.network.eval()
        # motion constraint (:34); the same values drive the fused device-side decode
        self.output_window = hann2d(torch.tensor([self.feat_sz, self.feat_sz]).long(), centered=True).cuda()
        nat = self.network._native()
        check_params_geometry(params, nat)
        nat.set_window(self.output_window.cpu().numpy())

        # static device buffers + captured graph of the whole device step
        tz, tx = self.params.template_size, self.params.search_size
        self._z = torch.zeros(1, 3, tz, tz, device="cuda")
        self._x = torch.zeros(1, 3, tx, tx, device="cuda")
        self._graph, self._out = nat.capture(self._z, self._x)
        self._rec = torch.empty(5, device="cuda")
        self._rec_host = torch.empty(5).pin_memory()

    def initialize(self, image, info: dict):
        """image: an (H, W, 3) RGB array, or a native.Image (any layout of include/vittrack.h -- NV12 / NV21, BGR, RGBA / BGRA, ...;
        Image.chw(t) for a (3, H, W) frame) that the device crop reads directly."""
        if isinstance(image, Image) and self._bt is None:
            raise VtError("an Image frame needs the device pipeline (params.host_crop is set)")
        if self._bt is not None:
            self._bt.initialize([image] if isinstance(image, Image) else image[None], [list(info["init_bbox"])])
            self.box_mask_z = None
            self.state = info["init_bbox"]
            self.frame_id = 0
            if self.save_all_boxes:
                return {"all_boxes": info["init_bbox"] * 1}
            return None
        z_patch_arr, resize_factor, z_amask_arr = sample_target(image, info["init_bbox"], self.params.template_factor,
                                                                output_sz=self.params.template_size)
        self.z_patch_arr = z_patch_arr
        template = self.preprocessor.process(z_patch_arr, z_amask_arr)
        self.z_dict1 = template
        self._z.copy_(template.tensors)
        self.box_mask_z = None
        self.state = info["init_bbox"]
        self.frame_id = 0
        if self.save_all_boxes:
            return {"all_boxes": info["init_bbox"] * 1}

    def track(self, image, info: dict = None):
        import torch
        if isinstance(image, Image) and self._bt is None:
            raise VtError("an Image frame needs the device pipeline (params.host_crop is set)")
        H, W, _ = image.shape
        self.frame_id += 1
        if self._bt is not None:
            rec = self._bt.track_record([image] if isinstance(image, Image) else image[None])[0].tolist()      # [x, y, w, h, confidence] of this frame, on the host
            self.state = rec[:4]
            if self.save_all_boxes:
                # rare mode: two more small copies for the un-clipped box (the windowed decode and this frame's resize factor)
                pred_boxes = self._bt.out.hann_boxes.cpu().view(-1, 4)
                resize_factor = float(self._bt.rf.cpu()[0])
                return {"target_bbox": self.state, "all_boxes": self._all_boxes(pred_boxes, resize_factor)}
            return {"target_bbox": self.state, "confidence": float(np.float32(rec[4]))}
        x_patch_arr, resize_factor, x_amask_arr = sample_target(image, self.state, self.params.search_factor,
                                                                output_sz=self.params.search_size)
        search = self.preprocessor.process(x_patch_arr, x_amask_arr)
        self._x.copy_(search.tensors)

        # network.forward + hann window + cal_bbox (:86-105) = one graph replay
        self._graph.launch()
        self._rec[:4].copy_(self._out.hann_boxes.view(-1))
        self._rec[4:].copy_(self._out.conf)
        self._rec_host.copy_(self._rec, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        rec = self._rec_host

        # Baseline: mean over the (single) predicted box, scaled back to crop pixels (:107-109)
        pred_box = (rec[:4].view(1, 4).mean(dim=0) * self.params.search_size / resize_factor).tolist()
        self.state = clip_box(self.map_box_back(pred_box, resize_factor), H, W, margin=10)

        if self.save_all_boxes:
            return {"target_bbox": self.state, "all_boxes": self._all_boxes(rec[:4].clone().view(1, 4), resize_factor)}
        return {"target_bbox": self.state, "confidence": float(rec[4])}

    def map_box_back(self, pred_box: list, resize_factor: float):
        """:150-156"""
        cx_prev, cy_prev = self.state[0] + 0.5 * self.state[2], self.state[1] + 0.5 * self.state[3]
        cx, cy, w, h = pred_box
        half_side = 0.5 * self.params.search_size / resize_factor
        cx_real = cx + (cx_prev - half_side)
        cy_real = cy + (cy_prev - half_side)
        return [cx_real - 0.5 * w, cy_real - 0.5 * h, w, h]


    def map_box_back_batch(self, pred_box, resize_factor: float):
        """:158-164 -- float32 tensor arithmetic, offsets from Python floats, like the reference"""
        import torch
        cx_prev, cy_prev = self.state[0] + 0.5 * self.state[2], self.state[1] + 0.5 * self.state[3]
        cx, cy, w, h = pred_box.unbind(-1)
        half_side = 0.5 * self.params.search_size / resize_factor
        cx_real = cx + (cx_prev - half_side)
        cy_real = cy + (cy_prev - half_side)
        return torch.stack([cx_real - 0.5 * w, cy_real - 0.5 * h, w, h], dim=-1)

    def _all_boxes(self, pred_boxes, resize_factor: float):
        """`save_all_boxes` record of one frame (:141-146): every predicted box (one here) scaled to crop pixels and mapped
        back WITHOUT clipping -- and, as in the reference, relative to `self.state` as it is at that point, i.e. the state
        this frame has just produced, not the one the crop was taken around."""
        all_boxes = self.map_box_back_batch(pred_boxes * self.params.search_size / resize_factor, resize_factor)
        return all_boxes.view(-1).tolist()


def get_tracker_class():
    return Vit_dist
