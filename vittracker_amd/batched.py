"""Lock-step batched tracking of B independent sequences on one GPU, state resident on the device.

The reference runs one tracker object per sequence and per process
(``lib/test/evaluation/tracker.py:90-152``, ``running.py:105-112``): per frame a host crop
(cv2), an H2D copy, ~130 kernel launches and a ``.tolist()`` sync.  Here B sequences advance
together: one H2D copy of the raw uint8 frames, then ``crop -> forward -> state update`` as one captured
graph on the stream with no host synchronisation; boxes are read back whenever the caller wants them
(every frame, or once at the end of the sequence).

Semantics per sequence are those of ``Vit_dist.initialize / track``
(``lib/test/tracker/vit_dist.py:53-148``); the crop and the state update run in
``vt_crop`` / ``vt_update_state`` (include/vittrack.h), the network in the captured graph.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from .config import geometry
from .host_ops import hann2d
from .factory import build_network
from .native import FrameTable, Image, ImageTable, VtError, pack_image_offsets, pack_offsets


def check_params_geometry(params, nat):
    """The tracker crops at params.{template,search}_size (TEST.*_SIZE) while the model is built from
    DATA.*.SIZE: a YAML that sets only one of them raises a shape error at the pos-embed add in the
    reference (lib/models/vit_dist/vit_dist.py:81-82); here the mismatch is refused up front."""
    if (params.template_size, params.search_size) != (nat.template_size, nat.search_size):
        raise VtError(f"tracker crop sizes (TEST.TEMPLATE_SIZE={params.template_size}, TEST.SEARCH_SIZE="
                      f"{params.search_size}) differ from the model geometry (DATA.TEMPLATE.SIZE={nat.template_size}, "
                      f"DATA.SEARCH.SIZE={nat.search_size})")


class _Arena:
    """A pinned host buffer and its device twin, [descriptor table | frames or planes]: the CPU packs a step's host frames into `np`
    (the numpy view of `host`) and they reach `dev` with ONE copy.  It grows by doubling; each capacity has its own device address."""

    def __init__(self):
        self.cap, self.host, self.np, self.dev, self.copied = 0, None, None, None, None

    def reserve(self, end: int):
        """Make room for `end` bytes and wait until the CPU may write them.  Returns the device address the arena had when it had to
        grow (the caller drops the graph captured on it), else None."""
        import torch
        old = None
        if self.cap < end:
            torch.cuda.current_stream().synchronize()       # nothing may still read the old arena
            old = self.dev.data_ptr() if self.dev is not None else None
            self.cap = max(end, 2 * self.cap)
            self.host = torch.empty(self.cap, dtype=torch.uint8).pin_memory()
            self.np = self.host.numpy()
            self.dev = torch.empty(self.cap, dtype=torch.uint8, device="cuda")
            self.copied = None
        if self.copied is not None:
            self.copied.synchronize()                         # the previous copy out of the pinned arena has been read
        return old

    def flush(self, end: int):
        """Copy [0, end) to the device and record the event the next reserve() waits for.  Returns the device tensor."""
        import torch
        self.dev[:end].copy_(self.host[:end], non_blocking=True)
        self.copied = torch.cuda.Event()
        self.copied.record()
        return self.dev


class BatchedVitTracker:
    ZERO_COPY_MAX_BYTES = 2 << 20      # host frames up to this size (all sequences together) are read in place from pinned memory

    def __init__(self, params, batch: int, form_batch: int = 0):
        """form_batch: this tracker steps `batch` sequences of a larger group of `form_batch` (a shard of ShardedBatchedTracker, a rank
        of run_dataset_batched): its kernels take the forms the whole group would run (native.Model.set_form_batch), so that the
        group's results do not depend on how it is sharded."""
        import torch
        self.params = params
        self.cfg = params.cfg
        self.B = batch
        g = geometry(self.cfg)
        self.net = build_network(self.cfg, max_batch=batch, ce_form=getattr(params, "ce_form", None), precision=getattr(params, "precision", None))      # vit_48 or ViT-Base OSTrack, by the cfg
        ckpt = getattr(params, "checkpoint", None)
        import os
        if ckpt and os.path.isfile(ckpt):
            self.net.load_state_dict(torch.load(ckpt, map_location="cpu")["net"], strict=False)
        elif not getattr(params, "allow_synthetic_weights", False):
            raise FileNotFoundError(f"checkpoint {ckpt!r} not found")
        self.net.cuda().eval()
        self.nat = self.net._native()
        if form_batch:
            self.nat.set_form_batch(form_batch)
        check_params_geometry(params, self.nat)
        F = params.search_size // self.cfg.MODEL.BACKBONE.STRIDE
        self.nat.set_window(hann2d(torch.tensor([F, F]).long()).numpy())
        self.mean, self.std = list(self.cfg.DATA.MEAN), list(self.cfg.DATA.STD)
        dev = "cuda"
        self.z = torch.zeros(batch, 3, params.template_size, params.template_size, device=dev)
        self.x = torch.zeros(batch, 3, params.search_size, params.search_size, device=dev)
        self.states = torch.zeros(batch, 4, dtype=torch.float64, device=dev)
        self.rf = torch.zeros(batch, dtype=torch.float64, device=dev)
        from .native import Outputs
        self.out = Outputs(batch, F, dev)
        self.graph = None            # captured at the first initialize(): the forward reads the cached template (z = None)
        self._chunk_graphs = {}      # (frame buffer address, n, H, W) -> whole-step graph of n frames (track_chunk)
        self._held = None            # hold_states(): open loop, every step searches around the boxes it was switched on with
        self._chunk_buf = None
        self.frames = None
        self._fast_shape = None
        self._fast = [None, None]    # per pinned frame slot: (numpy view of the slot, its whole-step graph, numpy view of its pinned record)
        self._slot = 0
        self.hw = None
        self.frame_id = 0
        # the two table routes -- frames of different sizes (vt_track_step_frames) and frames in other pixel formats
        # (vt_track_step_images) --, each with the arena of its host frames and its graphs: device table address -> (graph, device
        # record, pinned host record, table)
        self._routes = {FrameTable: SimpleNamespace(arena=_Arena(), graphs={}, step=self.nat.track_step_frames),
                        ImageTable: SimpleNamespace(arena=_Arena(), graphs={}, step=self.nat.track_step_images)}
        self._dev_table = None       # FrameTable of caller-owned device frames
        self._img_keep = []          # device planes the image table of the last step points into

    # ---- frames of different sizes ------------------------------------------------------------------------------------
    @staticmethod
    def _is_mixed(frames):
        """A list / tuple of frames whose sizes differ: the frame-table path.  Same-size input keeps the dense path untouched."""
        if isinstance(frames, np.ndarray) or not isinstance(frames, (list, tuple)) or len(frames) < 2:
            return False
        s0 = tuple(frames[0].shape)
        return any(tuple(f.shape) != s0 for f in frames[1:])

    def _frame_table(self, frames):
        """The device vt_frame table of B frames of any sizes.  Caller-owned CUDA tensors go in by pointer (only the table is copied);
        host frames are packed into a pinned arena at 256-byte offsets behind the table and reach the device arena with ONE copy.  The
        arena grows by doubling; each capacity has its own table address, hence its own captured step."""
        import torch
        if len(frames) != self.B:
            raise ValueError(f"expected {self.B} frames, got {len(frames)}")
        if all(isinstance(f, torch.Tensor) and f.is_cuda for f in frames):
            if self._dev_table is None:
                self._dev_table = FrameTable(self.B, "cuda")
            for i, f in enumerate(frames):
                self._dev_table.set_tensor(i, f)
            return self._dev_table.upload()
        arrs = []
        for f in frames:
            a = f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("every frame must be an (H, W, 3) uint8 array")
            arrs.append(a)
        tb = self.B * FrameTable.ITEM
        offs, end = pack_offsets([a.shape[:2] for a in arrs], start=tb)
        r = self._routes[FrameTable]
        ar = r.arena
        r.graphs.pop(ar.reserve(end), None)
        tab = ar.np[:tb].view(FrameTable.DTYPE)
        base = ar.dev.data_ptr()
        for i, (a, o) in enumerate(zip(arrs, offs)):
            H, W = a.shape[:2]
            pitch = FrameTable.check(base + o, H, W, 0, nbytes=ar.cap - o)
            tab[i] = (base + o, H, W, pitch)
            ar.np[o:o + H * W * 3].reshape(H, W, 3)[...] = a
        return ar.flush(end)[:tb]

    # ---- frames in other pixel formats (NV12 / NV21, BGR, RGBA / BGRA) ---------------------------------------------------------
    @staticmethod
    def _has_image(frames):
        """A list / tuple of frames of which at least one is an Image: the image-table path.  Lists without one take today's routes."""
        return isinstance(frames, (list, tuple)) and any(isinstance(f, Image) for f in frames)

    @staticmethod
    def _as_image(f):
        """An Image as it is; an RGB frame (host array or CUDA tensor) as Image.rgb."""
        import torch
        if isinstance(f, Image):
            return f
        if isinstance(f, torch.Tensor) and not f.is_cuda:
            f = f.numpy()
        return Image.rgb(f)

    def _image_table(self, frames):
        """The device vt_image table of B frames of any formats and sizes.  Device images go in by pointer; the planes of host images
        are packed into a pinned arena at 256-byte offsets behind the table and reach the device arena, table included, with ONE
        copy.  The arena grows by doubling; each capacity has its own table address, hence its own captured step."""
        if len(frames) != self.B:
            raise ValueError(f"expected {self.B} frames, got {len(frames)}")
        ims = [self._as_image(f) for f in frames]
        tb = self.B * ImageTable.ITEM
        host_ims = [im for im in ims if not im.is_cuda]
        offs, end = pack_image_offsets(host_ims, start=tb)
        r = self._routes[ImageTable]
        ar = r.arena
        r.graphs.pop(ar.reserve(end), None)
        tab = ar.np[:tb].view(ImageTable.DTYPE)
        base = ar.dev.data_ptr()
        self._img_keep = [im for im in ims if im.is_cuda]     # device planes the step reads in place
        it = iter(offs)
        for i, im in enumerate(ims):
            if im.is_cuda:
                d, room = im.descriptor(), (None, None)
            else:
                po = next(it)
                rows = im.plane_rows()
                for a, o, (n, rb) in zip(im.host_planes(), po, rows):
                    ar.np[o:o + n * rb].reshape(n, rb)[...] = np.asarray(a).reshape(n, rb)
                d = im.descriptor([base + o for o in po], [rb for _, rb in rows])
                room = (ar.cap - po[0], ar.cap - po[1] if len(po) > 1 else None)
            ImageTable.check_descriptor(d, *room)
            tab[i] = d
        return ar.flush(end)[:tb]

    def _route(self, frames, restart=False):
        """Which source `frames` are, and the table or tensor for it: a list with at least one Image takes the image table
        (ImageTable, device table), any other list of differing sizes the frame table (FrameTable, device table), everything else the
        dense path (None, the (B,H,W,3) tensor).  restart: the frames of reinitialize(), one per restarted slot -- always a table, made
        of device copies of their own (the arenas and the dense buffers belong to the running step)."""
        import torch
        if self._has_image(frames):
            if not restart:
                return ImageTable, self._image_table(frames)
            ims = []
            for f in map(self._as_image, frames):
                if not f.is_cuda:
                    f = Image(f.format, [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in f.host_planes()], f.H, f.W,
                              [rb for _, rb in f.plane_rows()])
                ims.append(f)
            return ImageTable, ImageTable.of(ims)
        if restart:
            return FrameTable, FrameTable.of([f if isinstance(f, torch.Tensor) and f.is_cuda else torch.from_numpy(np.ascontiguousarray(f)).cuda()
                                              for f in frames])
        if self._is_mixed(frames):
            return FrameTable, self._frame_table(frames)
        return None, self._upload(frames)

    def _track_table(self, route, tab, sync):
        """One replay of the whole step on a descriptor table (route.step: nat.track_step_frames or nat.track_step_images -> record),
        captured once per table address in route.graphs: the table's contents change between replays, its address does not."""
        import torch
        hit = route.graphs.get(tab.data_ptr())
        if hit is None:
            rec = torch.empty(self.B, 5, dtype=torch.float64, device="cuda")
            host = torch.empty(self.B, 5, dtype=torch.float64).pin_memory()
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.graph(g, stream=side):
                route.step(tab, self.states, self.params.search_factor, self.mean, self.std, self.x, self.rf, self.out,
                           record=rec, margin=10, stream=torch.cuda.current_stream())
            torch.cuda.current_stream().wait_stream(side)
            hit = route.graphs[tab.data_ptr()] = (g, rec, host, tab)
        g, rec, host, _ = hit
        g.replay()
        self.frame_id += 1
        if sync:
            return self._result(self._records(rec, host))
        return {"target_bbox": self.states, "confidence": self.out.conf, "record": rec}

    def reinitialize(self, slots, frames, boxes):
        """Restart the sequences of `slots` on new frames and boxes (Vit_dist.initialize, lib/test/tracker/vit_dist.py:52-65) while
        the other slots go on: their templates are cropped from their own frames (any sizes; host arrays or CUDA tensors), their states
        set, and the template cache rewritten for those slots only (vt_set_template_slots).  No other slot's state or cache changes
        and no graph is recaptured."""
        import torch
        slots = [int(v) for v in slots]
        n = len(slots)
        if n == 0:
            return
        if self.graph is None:
            raise VtError("reinitialize before initialize")
        if len(set(slots)) != n or min(slots) < 0 or max(slots) >= self.B:
            raise ValueError(f"slots must be distinct indices in [0, {self.B})")
        if len(frames) != n:
            raise ValueError(f"expected {n} frames for {n} slots, got {len(frames)}")
        boxes = np.asarray(boxes, dtype=np.float64).reshape(n, 4)
        for f in (self.params.template_factor, self.params.search_factor):
            if not np.all(np.ceil(np.sqrt(boxes[:, 2] * boxes[:, 3]) * f) >= 1):
                raise Exception("Too small bounding box.")   # processing_utils.py:33-34
        st = torch.as_tensor(boxes).cuda()
        z = torch.empty(n, 3, self.params.template_size, self.params.template_size, device="cuda")
        rf = torch.empty(n, dtype=torch.float64, device="cuda")
        kind, tab = self._route(frames, restart=True)
        self.nat._crop(kind, tab, st, self.params.template_factor, self.params.template_size, (self.mean, self.std), z, rf, None)
        idx = torch.as_tensor(slots, device="cuda")
        self.states.index_copy_(0, idx, st)
        self.z.index_copy_(0, idx, z)
        self.nat.set_template_slots(z, slots)

    def _upload(self, frames):
        """Host frames are copied straight from the caller's array into one of two device frame buffers with ONE blocking copy
        (the runtime stages pageable memory itself: 53 GB/s for a 236 MB batch, ~20 us for one 230 KB frame; an explicit
        pinned staging buffer filled by the CPU and DMA-ed from measured 6.7 GB/s and 2 ms -- tools/upload_probe.py).  The
        copy returns when the caller's array has been read, so there is no staging buffer a later call could overwrite; it is
        queued behind the previous step on the stream, whose kernels may still be reading the OTHER device buffer."""
        import torch
        if isinstance(frames, torch.Tensor) and frames.is_cuda:
            t = frames
            if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.shape[0] != self.B or not t.is_contiguous():
                raise ValueError(f"frames must be a contiguous (B={self.B}, H, W, 3) uint8 tensor (a (B, 3, H, W) batch: pass native.images_from_chw(frames))")
        else:
            a = np.ascontiguousarray(np.stack(frames) if not isinstance(frames, np.ndarray) else frames)
            if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3 or a.shape[0] != self.B:
                raise ValueError(f"frames must be (B={self.B}, H, W, 3) uint8 (a (B, 3, H, W) batch: pass native.images_from_chw(frames))")
            zero_copy = a.nbytes <= self.ZERO_COPY_MAX_BYTES
            if self.frames is None or tuple(self.frames[0].shape) != a.shape or self.frames[0].is_cuda == zero_copy:
                torch.cuda.current_stream().synchronize()      # nothing may still read the old buffers
                self._fast = [None, None]
                if zero_copy:
                    # A few small frames (the plugin's one-sequence step): no upload at all.  The CPU copies the frame into one of
                    # two PINNED host slots (230 KB: ~3 us) and the crop kernel reads the pixels it needs over the bus (+1 us on the
                    # kernel) -- against ~19 us for the blocking copy from pageable memory (tools/zero_copy_probe.py).
                    self.frames = [torch.empty(a.shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
                    self._frames_np = [f.numpy() for f in self.frames]
                    self._slot_done = [None, None]
                else:
                    self.frames = [torch.empty(a.shape, dtype=torch.uint8, device="cuda") for _ in range(2)]
            k = self._slot
            self._slot ^= 1
            if zero_copy:
                if self._slot_done[k] is not None:
                    self._slot_done[k].synchronize()           # the step that last read this slot (two calls ago) has finished
                np.copyto(self._frames_np[k], a)
                self._cur_slot = k
            else:
                self.frames[k].copy_(torch.from_numpy(a))
                self._cur_slot = None
            t = self.frames[k]
        self.hw = (int(t.shape[1]), int(t.shape[2]))
        return t

    def _mark_slot(self, synced=False):
        """After the launch that reads the current pinned frame slot: an event the next writer of that slot waits for (none when
        the caller synchronises on this step anyway)."""
        import torch
        k = getattr(self, "_cur_slot", None)
        if k is None:
            return
        if synced:
            self._slot_done[k] = None
            return
        if self._slot_done[k] is None:
            self._slot_done[k] = torch.cuda.Event()
        self._slot_done[k].record()

    def initialize(self, frames, init_boxes):
        """frames: (B,H,W,3) uint8 (numpy, list of arrays or CUDA tensor) -- or a list of B frames of different sizes, any of which
        may be a native.Image (any layout of include/vittrack.h: NV12 / NV21, P010, I420, YUYV, GRAY8, BGR, RGBA / BGRA, RGB, planar RGB /
        I444 / I422 -- native.images_from_chw(batch) for a (B, 3, H, W) tensor);
        init_boxes: (B,4) [x,y,w,h]."""
        import torch
        kind, fr = self._route(frames)
        boxes = np.asarray(init_boxes, dtype=np.float64)
        if boxes.shape != (self.B, 4):
            raise ValueError(f"init_boxes must be (B={self.B}, 4) [x, y, w, h]")
        for f in (self.params.template_factor, self.params.search_factor):
            side = np.ceil(np.sqrt(boxes[:, 2] * boxes[:, 3]) * f)
            if not np.all(side >= 1):         # also catches NaN / negative sizes
                raise Exception("Too small bounding box.")   # processing_utils.py:33-34
        self.states.copy_(torch.as_tensor(boxes))
        self.nat._crop(kind, fr, self.states, self.params.template_factor, self.params.template_size, (self.mean, self.std), self.z, self.rf, None)
        if kind is None:
            self._mark_slot()
        # The template never changes after this (lib/test/tracker/vit_dist.py:57-60): its patch embedding and block 0's
        # LayerNorm-1 + qkv rows are computed once here (vt_set_template, bit-identical to recomputing them every frame);
        # graphs captured with z = None read that cache, so they stay valid across re-initialisation.
        self.nat.set_template(self.z)
        if self.graph is None:
            self.graph, _ = self.nat.capture(None, self.x, self.out)
        self.frame_id = 0

    def hold_states(self, on: bool = True):
        """Benchmark / study aid: with on=True every later step searches around the boxes the sequences have NOW (open loop,
        vt_set_open_loop: the step's boxes are in the records and the returned confidence, `states` stay) instead of around the previous
        step's result.  On synthetic noise frames with random weights a free-running tracker's boxes drift to the clip limits within a
        few frames, and the crop then reads windows no real sequence has (tracking/track_batch_demo.py --hold-boxes)."""
        self._held = bool(on) or None
        self.nat.set_open_loop(bool(on))
        self._chunk_graphs.clear()      # the flag is an argument of the captured kernels
        for route in self._routes.values():
            route.graphs.clear()
        self._fast = [None, None]

    def track_record(self, frames):
        """track(frames, sync=True) for callers that want the raw per-sequence records: a (B,5) float64 numpy array
        [x, y, w, h, confidence] that the caller owns.
        The plugin tracker's per-frame call: for host frames that are read in place (see _upload) a repeat call is one CPU copy,
        one graph launch, one stream synchronisation and nothing else."""
        import torch
        a = frames
        if type(a) is np.ndarray and self.frames is not None and a.shape == self._fast_shape and a.dtype == np.uint8 and a.flags.c_contiguous:
            k = self._slot
            ent = self._fast[k]
            if ent is not None:
                if self.graph is None:
                    raise VtError("track before initialize")
                self._slot = k ^ 1
                if self._slot_done[k] is not None:            # a step queued by track(sync=False) / initialize() may still read this slot
                    self._slot_done[k].synchronize()
                    self._slot_done[k] = None
                np.copyto(ent[0], a)
                self._cur_slot = k
                ent[1].replay()
                torch.cuda.current_stream().synchronize()
                self.frame_id += 1
                return ent[2][0].copy()                       # the caller owns it (40 bytes per sequence), as on the slow path
        out = self.track(frames, sync=True)
        return torch.cat([out["target_bbox"], out["confidence"].double().view(-1, 1)], dim=1).numpy()

    def track(self, frames, sync: bool = True):
        """Advance every sequence by one frame.  Returns {'target_bbox': (B,4) float64, 'confidence': (B,)}
        as CPU tensors when sync=True, else the device tensors (valid until the next call)."""
        if self.graph is None:
            raise VtError("track before initialize")
        kind, fr = self._route(frames)
        if kind is not None:            # frames of different sizes or in other pixel formats: one step on their descriptor table
            return self._track_table(self._routes[kind], fr, sync)
        H, W = self.hw
        self.frame_id += 1
        if self.frames is not None and any(fr.data_ptr() == f.data_ptr() for f in self.frames):
            # host frames land in one of two fixed device slots: the whole step (crop -> forward -> state update) is one
            # captured graph per slot -- one launch instead of three, no launch gaps inside the step
            g, rec, host, _ = self._chunk_graph(fr.unsqueeze(0), to_host=sync)
            g.replay()
            self._mark_slot(synced=sync)
            k = getattr(self, "_cur_slot", None)
            if sync and k is not None and host is None and self._fast[k] is None:      # pinned frame slot + pinned record: the fast path of track_record
                self._fast[k] = (self._frames_np[k], g, rec.numpy())
                self._fast_shape = tuple(self._frames_np[k].shape)
            if sync:
                return self._result(self._records(rec, host)[0])
            return {"target_bbox": self.states, "confidence": self.out.conf}
        # a caller-owned device tensor (a new address every call would mean a new capture every call): eager launches, as ONE library
        # call (vt_track_step: crop -> network on the cached template with the state update on the head's decoding lane)
        self.nat.track_step(fr, self.states, self.params.search_factor, self.mean, self.std, self.x, self.rf, self.out, margin=10)
        if sync:
            return {"target_bbox": self.states.cpu(), "confidence": self.out.conf.cpu()}
        return {"target_bbox": self.states, "confidence": self.out.conf}

    # ---- n frames per launch ------------------------------------------------------------------------------------
    def _chunk_graph(self, buf, to_host=False):
        """The whole tracker step -- crop -> forward -> map back / clip / state update -> record -- for the n frames of `buf`
        (n,B,H,W,3), captured once per frame buffer into ONE graph: no host work and one launch gap per n frames."""
        import torch
        n, _, H, W, _ = buf.shape
        to_host = bool(to_host) and self.B * n <= 64
        key = (buf.data_ptr(), n, H, W, to_host)
        hit = self._chunk_graphs.get(key)
        if hit is not None:
            return hit
        if len(self._chunk_graphs) >= 4:                      # a caller cycling through many buffers: keep the table small
            self._chunk_graphs.pop(next(iter(self._chunk_graphs)))
        # Per-frame result records [x, y, w, h, confidence] (float64).  vt_update_state_record writes them where the caller reads
        # them: small batches straight into PINNED host memory (device-mapped; 40 bytes per sequence over the bus, no copy kernel
        # and no device -> host copy after the step -- the plugin's one-sequence step), large batches into device memory (read
        # back on demand).
        # (to_host: the caller synchronises after every launch -- track(sync=True) of a few sequences)
        rec = torch.empty(n, self.B, 5, dtype=torch.float64).pin_memory() if to_host else torch.empty(n, self.B, 5, dtype=torch.float64, device="cuda")
        host = None if to_host else torch.empty(n, self.B, 5, dtype=torch.float64).pin_memory()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(g, stream=side):
            cs = torch.cuda.current_stream()
            for i in range(n):
                # vt_track_step = vt_crop -> vt_forward on the cached template -> vt_update_state_record in one library call
                self.nat.track_step(buf[i], self.states, self.params.search_factor, self.mean, self.std, self.x, self.rf, self.out,
                                    record=rec[i], margin=10, stream=cs)
        torch.cuda.current_stream().wait_stream(side)
        self._chunk_graphs[key] = (g, rec, host, buf)   # buf: the graph's kernels read it, keep it alive
        return self._chunk_graphs[key]

    def track_chunk(self, frames, sync: bool = True):
        """Advance every sequence by n = len(frames) frames with ONE graph launch: frames (n,B,H,W,3) uint8, a CUDA tensor (used in
        place: the graph is captured on its address and reused whenever the same buffer comes back) or host data (uploaded into
        an internal n-deep device buffer).  For callers that have the next frames at hand -- offline evaluation reads whole
        sequences (lib/test/evaluation/running.py:56-102).  Frame by frame the same kernels run in the same order as in
        track(): results are bit-identical.  Returns {'target_bbox': (n,B,4) float64, 'confidence': (n,B)}."""
        import torch
        if self.graph is None:
            raise VtError("track_chunk before initialize")
        if isinstance(frames, (list, tuple)) and any(self._is_mixed(f) for f in frames):
            # n steps of B frames of different sizes: n replays of the frame-table step, records gathered on the device, one sync
            recs = torch.empty(len(frames), self.B, 5, dtype=torch.float64, device="cuda")
            for j, f in enumerate(frames):
                recs[j].copy_(self._track_table(self._routes[FrameTable], self._frame_table(f), sync=False)["record"])
            return self._result(self._records(recs, torch.empty(recs.shape, dtype=torch.float64).pin_memory()) if sync else recs, sync)
        if isinstance(frames, torch.Tensor) and frames.is_cuda:
            buf = frames
            if buf.dtype != torch.uint8 or buf.dim() != 5 or buf.shape[1] != self.B or buf.shape[4] != 3 or not buf.is_contiguous():
                raise ValueError(f"frames must be a contiguous (n, B={self.B}, H, W, 3) uint8 tensor")
        else:
            a = np.ascontiguousarray(np.stack(frames) if not isinstance(frames, np.ndarray) else frames)
            if a.dtype != np.uint8 or a.ndim != 5 or a.shape[1] != self.B or a.shape[4] != 3:
                raise ValueError(f"frames must be (n, B={self.B}, H, W, 3) uint8")
            if self._chunk_buf is None or tuple(self._chunk_buf.shape) != a.shape:
                torch.cuda.current_stream().synchronize()
                self._chunk_buf = torch.empty(a.shape, dtype=torch.uint8, device="cuda")
            self._chunk_buf.copy_(torch.from_numpy(a))        # one blocking copy from the caller's array (see _upload)
            buf = self._chunk_buf
        n = int(buf.shape[0])
        self.hw = (int(buf.shape[2]), int(buf.shape[3]))
        g, rec, host, _ = self._chunk_graph(buf, to_host=sync)
        g.replay()
        self.frame_id += n
        return self._result(self._records(rec, host) if sync else rec, sync)

    @staticmethod
    def _result(r, host: bool = True):
        """Records (..., 5) [x, y, w, h, confidence] as the dict track() returns; host records give the confidence in float32."""
        return {"target_bbox": r[..., :4], "confidence": r[..., 4].float() if host else r[..., 4]}

    @staticmethod
    def _records(rec, host):
        """The records of the launch that was just queued, as a CPU tensor the caller owns: one stream synchronisation; records
        that live in pinned host memory were written by the kernel itself, device records take one async copy first."""
        import torch
        if host is not None:
            host.copy_(rec, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return (rec if host is None else host).clone()


class ShardedBatchedTracker:
    """B sequences as `shards` independent groups, each a BatchedVitTracker of its own -- its own model workspaces, states, frame
    buffers and graphs -- stepped under its own HIP stream.  Every kernel of the step is one workgroup per frame with most of a
    CU's LDS, so a single stream leaves the chip idle at each kernel's ramp and tail and between two graph launches; with two
    groups in flight the next graph's first kernel takes over the CUs the previous graph's last kernel is leaving (DESIGN.md 4.5:
    +5 % end to end at B = 2 x 256, +10-18 % on the network alone).  Same interface and the same results per sequence as one
    BatchedVitTracker of B sequences (initialize / track / track_chunk; host or device frames), bit for bit: every shard's model
    selects its kernel forms by the WHOLE group's size (vt_set_form_batch; the forms of a stage differ by fp32 rounding, and the
    library picks them by batch size), and within one form a sequence's kernels do not depend on which other sequences share
    its batch (tests/test_gpu_harness.py: B = 256 in two shards at both geometries)."""

    def __init__(self, params, batch: int, shards: int = 2):
        import torch
        self.sizes = self.shard_sizes(batch, shards)
        self.offsets = [sum(self.sizes[:k]) for k in range(len(self.sizes))]
        self.B = int(batch)
        self.params = params
        self.trackers = [BatchedVitTracker(params, n, form_batch=self.B) for n in self.sizes]
        self.streams = [torch.cuda.Stream() for _ in self.sizes]
        self.frame_id = 0

    @staticmethod
    def shard_sizes(batch: int, shards: int):
        """Contiguous groups of near-equal size, the first `batch % shards` one sequence larger; never an empty group."""
        shards = max(1, min(int(shards), int(batch)))
        base, extra = divmod(int(batch), shards)
        return [base + (1 if k < extra else 0) for k in range(shards)]

    def _slices(self):
        return [slice(o, o + n) for o, n in zip(self.offsets, self.sizes)]

    def _each(self, fn):
        """fn(tracker, slice) under the shard's stream, for every shard, without waiting in between."""
        import torch
        cur = torch.cuda.current_stream()
        out = []
        for t, st, sl in zip(self.trackers, self.streams, self._slices()):
            st.wait_stream(cur)                      # what the caller queued (e.g. the frames' producer) comes first
            with torch.cuda.stream(st):
                out.append(fn(t, sl))
        return out

    def _join(self):
        import torch
        cur = torch.cuda.current_stream()
        for st in self.streams:
            cur.wait_stream(st)

    def _gather(self, res, sync, dim):
        """The shards' results as one: per-shard lists of device tensors (sync=False), or host tensors concatenated along the batch
        axis `dim` after one asynchronous copy per shard on its own stream."""
        import torch
        if not sync:
            self._join()
            return {"target_bbox": [r["target_bbox"] for r in res], "confidence": [r["confidence"] for r in res]}
        host = []
        for r, st in zip(res, self.streams):
            with torch.cuda.stream(st):
                host.append((r["target_bbox"].to("cpu", non_blocking=True), r["confidence"].to("cpu", non_blocking=True)))
        for st in self.streams:
            st.synchronize()
        return {"target_bbox": torch.cat([h[0] for h in host], dim=dim), "confidence": torch.cat([h[1] for h in host], dim=dim).float()}

    def initialize(self, frames, init_boxes):
        boxes = np.asarray(init_boxes, dtype=np.float64)
        self._each(lambda t, sl: t.initialize(frames[sl], boxes[sl]))
        self._join()
        self.frame_id = 0

    def reinitialize(self, slots, frames, boxes):
        raise VtError("continuous batching (reinitialize, frames of different sizes) is implemented for BatchedVitTracker only, "
                      "not for ShardedBatchedTracker")

    def track(self, frames, sync: bool = True):
        """One frame for every sequence: frames (B,H,W,3) uint8, host or device.  sync=True: {'target_bbox': (B,4) float64,
        'confidence': (B,)} on the host; sync=False: the same keys as LISTS of per-shard device tensors (valid until the next call)."""
        res = self._each(lambda t, sl: t.track(frames[sl], sync=False))
        self.frame_id += 1
        return self._gather(res, sync, 0)

    def track_chunk(self, frames, sync: bool = True):
        """n frames per launch and shard: frames (n,B,H,W,3) uint8 host data, or a list of per-shard contiguous CUDA tensors
        (n,B_k,H,W,3) -- a slice of one device tensor along its batch axis is not contiguous, and the graphs are captured on
        buffer addresses.  Returns what BatchedVitTracker.track_chunk returns, batch axes concatenated (sync=True) or per shard."""
        import torch
        if isinstance(frames, (list, tuple)) and len(frames) == len(self.trackers) and all(isinstance(f, torch.Tensor) for f in frames):
            parts = list(frames)
        else:
            a = np.stack(frames) if not isinstance(frames, np.ndarray) else frames
            parts = [np.ascontiguousarray(a[:, sl]) for sl in self._slices()]
        idx = {id(t): k for k, t in enumerate(self.trackers)}
        res = self._each(lambda t, sl: t.track_chunk(parts[idx[id(t)]], sync=False))
        self.frame_id += int(parts[0].shape[0])
        return self._gather(res, sync, 1)
