#!/usr/bin/env python3
"""Counterpart of the reference's ``tracking/test.py`` (``:14-56``): run a tracker on a dataset.

    python tracking/test.py vit_dist vit_48_h32_noKD --dataset_name synthetic:16x50 --threads 0 --num_gpus 1
    python tracking/test.py vit_dist vit_48_h32_noKD --dataset_name synthetic:512x100 --batch 256      # lock-step batches
    python tracking/test.py vit_dist vit_48_h32_noKD --dataset_name folder:/videos --batch 64 --continuous   # any frame sizes
    python tracking/test.py ostrack vitb_256 --dataset_name synthetic:4x20 --synthetic_weights [--batch 4 [--continuous]]   # ViT-Base OSTrack
    python tracking/test.py ostrack vitl_256 --dataset_name synthetic:4x6 --synthetic_weights [--batch 4]   # ViT-Large OSTrack (also vitl_384)
    python tracking/test.py ostrack vits_256 --dataset_name synthetic:2x4 --synthetic_weights [--batch 2]   # ViT-Small / ViT-Tiny (vits_384, vitt_256, vitt_384)

Same positional arguments and options as the reference, plus ``--batch B`` (> 0 selects the MI355X-native lock-step
batched runner; with ``--continuous`` the continuous-batching runner, which keeps B slots busy across frame sizes and
lengths) and ``--synthetic_weights`` (no trained checkpoint exists in the reference tree).  Result files:
``<save_dir>/test/tracking_results/<tracker>/<param>[_<runid>]/<seq>.txt`` and ``<seq>_time.txt``."""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def run_tracker(tracker_name, tracker_param, run_id=None, dataset_name="synthetic", sequence=None, debug=0, threads=0,
                num_gpus=8, batch=0, synthetic_weights=False, frames_per_launch=1, shards=1, continuous=False, ce_form=None, precision=None):
    from vittracker_amd.evaluation import Tracker, get_dataset
    from vittracker_amd.evaluation.running import run_dataset, run_dataset_batched, run_dataset_continuous
    dataset = get_dataset(dataset_name)
    if sequence is not None:
        dataset = type(dataset)([dataset[sequence]])
    tracker = Tracker(tracker_name, tracker_param, dataset_name, run_id)
    if synthetic_weights or ce_form is not None or precision is not None:
        _get = tracker.get_parameters

        def get_parameters():
            p = _get()
            if synthetic_weights:
                p.allow_synthetic_weights = True
            if ce_form is not None:
                p.ce_form = ce_form
            if precision is not None:
                p.precision = precision
            return p
        tracker.get_parameters = get_parameters
    if batch > 0:
        rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        if world > 1:
            import torch
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        if continuous:
            if shards > 1 or frames_per_launch > 1 or world > 1:
                raise SystemExit("--continuous runs one BatchedVitTracker on one GPU: --shards, --frames_per_launch and multi-GPU runs "
                                 "are not supported with it")
            run_dataset_continuous(dataset, tracker, batch=batch)
        else:
            run_dataset_batched(dataset, tracker, batch=batch, rank=rank, world=world, frames_per_launch=frames_per_launch, shards=shards)
    elif continuous:
        raise SystemExit("--continuous needs --batch B")
    else:
        run_dataset(dataset, [tracker], debug, threads, num_gpus=num_gpus)


def main():
    p = argparse.ArgumentParser(description="Run tracker on sequence or dataset.")
    p.add_argument("tracker_name", type=str, help="Name of tracking method.")
    p.add_argument("tracker_param", type=str, help="Name of config file.")
    p.add_argument("--runid", type=int, default=None, help="The run id.")
    p.add_argument("--dataset_name", type=str, default="synthetic", help="synthetic[:NxT], synthetic_mixed[:NxT] or folder:<path>")
    p.add_argument("--sequence", type=str, default=None, help="Sequence number or name.")
    p.add_argument("--debug", type=int, default=0, help="Debug level.")
    p.add_argument("--threads", type=int, default=0, help="Number of worker processes (0 = sequential).")
    p.add_argument("--num_gpus", type=int, default=8)
    p.add_argument("--batch", type=int, default=0, help="> 0: lock-step batches of this many sequences per GPU")
    p.add_argument("--shards", type=int, default=1,
                   help="with --batch: step a group's sequences as this many independent sub-groups on their own HIP streams (ShardedBatchedTracker)")
    p.add_argument("--frames_per_launch", type=int, default=1,
                   help="with --batch: frames read ahead and tracked per graph launch (BatchedVitTracker.track_chunk)")
    p.add_argument("--continuous", action="store_true",
                   help="with --batch: continuous batching -- B slots across every frame size; a finished sequence's slot takes the next one")
    p.add_argument("--synthetic_weights", action="store_true", help="run on the seeded synthetic weights")
    p.add_argument("--ce_form", choices=("masked", "compact"), default=None,
                   help="candidate-elimination models (ostrack *_ce_* YAMLs): key masking, or the kept tokens gathered into shorter "
                        "frames behind every stage; default: the environment variable VB_CE_FORM, else masked")
    p.add_argument("--precision", choices=("bf16", "fp32"), default=None,
                   help="patch-16 ViT models (ostrack YAMLs): bf16 operands, or the fp32-equivalent mode on three-piece bf16 operands; "
                        "default: the environment variable VB_PRECISION, else bf16")
    a = p.parse_args()
    try:
        seq = int(a.sequence)
    except (TypeError, ValueError):
        seq = a.sequence
    more = {} if a.precision is None else {"precision": a.precision}
    run_tracker(a.tracker_name, a.tracker_param, a.runid, a.dataset_name, seq, a.debug, a.threads, a.num_gpus, a.batch,
                a.synthetic_weights, a.frames_per_launch, a.shards, a.continuous, a.ce_form, **more)


if __name__ == "__main__":
    main()
