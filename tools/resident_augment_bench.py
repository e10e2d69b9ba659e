"""What the resident loader's augmentation costs with everything on (data.ResidentLoader(augment=data.Augment(camera, lidar,
map))): the gather launches alone, for a kernel trace, and the training rate.  B = 32, vec, lane_bucket = 16, 768 phase-1 frames
per epoch - the workload of resident_jitter_bench.py, whose frames and packed store it shares (--store).

  resident_augment_bench.py gather [--augment none|camera|all] [--compact] [--store DIR]
        ResidentLoader alone: one warm epoch + three timed; trace it with rocprofv3 --kernel-trace --stats
  resident_augment_bench.py train [--augment none|camera|all] [--compact] [--dtype f32|bf16] [--store DIR]
        Trainer.train, graph replay: one warm epoch + two timed

none: the plain loader, one launch per batch (gather_batch_kernel).  camera: augment=CameraJitter(0.4, 0.4, 0.4, erase_prob 0.5),
two launches (camera_jitter_kernel takes the camera field).  all: Augment(camera=that, lidar=LidarDropout(cell_prob 0.1, erase_prob
0.5), map=MapNoise(shift 0.5, yaw_deg 2, lane_drop 0.1, target_shift 0.5)), three launches: gather_augment_kernel takes the LiDAR
frame, the lane set and the target point.  --compact keeps the LiDAR histogram as 4-bit codes."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mmfn_amd import data as D  # noqa: E402
from mmfn_amd.config import GlobalConfig  # noqa: E402
from trainer_bench import gather_bytes, packed_store  # noqa: E402

LAUNCHES = {"none": 1, "camera": 2, "all": 3}


def make_augment(kind):
    if kind == "none":
        return None
    jitter = D.CameraJitter(brightness=0.4, contrast=0.4, saturation=0.4, erase_prob=0.5, seed=1)
    if kind == "camera":
        return jitter
    return D.Augment(camera=jitter, lidar=D.LidarDropout(cell_prob=0.1, erase_prob=0.5, seed=2),
                     map=D.MapNoise(shift=0.5, yaw_deg=2.0, lane_drop=0.1, target_shift=0.5, seed=3))


def make_loader(root, n, cfg, B, augment, compact):
    packed = packed_store(root, n, cfg)
    res = D.ResidentFrames(packed, "cuda:0", cfg, "vec", compact=compact)
    return res, D.ResidentLoader(res, batch_size=B, lane_bucket=16, augment=make_augment(augment))


def run_gather(root, B=32, n=768, epochs=3, augment="none", compact=False):
    """Wall time per batch (host clock over whole epochs that end in a synchronise, after a warm epoch; it holds the host's work per
    batch too) and the bytes the batch's launches move, from the shapes; the kernels' own times are the trace's."""
    cfg = GlobalConfig()
    res, loader = make_loader(root, n, cfg, B, augment, compact)
    read = written = batches = 0
    for inp, gt in loader:      # warm epoch: the byte counts (which read lane_num back) stay outside the timed window
        r, w = gather_bytes(res, inp, gt)
        read, written, batches = read + r, written + w, batches + 1
    torch.cuda.synchronize()
    t0 = time.time()
    timed = 0
    for _ in range(epochs):
        for inp, gt in loader:
            timed += 1
    torch.cuda.synchronize()
    dt = time.time() - t0
    return {"augment": augment, "compact": bool(compact), "batches": batches + timed, "launches_per_batch": LAUNCHES[augment],
            "wall_us_per_batch": round(dt / timed * 1e6, 1), "bytes_read_per_batch": read // batches,
            "bytes_written_per_batch": written // batches}


def run_train(root, B=32, n=768, epochs=2, dtype="f32", augment="none", compact=False):
    from mmfn_amd.model import MMFN
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import Trainer
    cfg = GlobalConfig(act_dtype=dtype)
    _, loader = make_loader(root, n, cfg, B, augment, compact)
    torch.manual_seed(0)
    net = MMFN(cfg, "cuda:0")
    opt = FusedAdamW(net, lr=1e-4)
    tr = Trainer("cuda:0", None)
    tr.train(net, loader, cfg, opt, graph=True)     # warm epoch (buffers, capture)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(epochs):
        tr.train(net, loader, cfg, opt, graph=True)
    torch.cuda.synchronize()
    dt = time.time() - t0
    return {"dtype": dtype, "augment": augment, "compact": bool(compact), "samples_per_s": round(epochs * n / dt, 1),
            "ms_per_step": round(dt / (epochs * n / B) * 1e3, 2), "train_loss": [round(v, 5) for v in tr.train_loss]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gather", "train"])
    ap.add_argument("--augment", default="none", choices=sorted(LAUNCHES), help="none: the plain loader; camera: CameraJitter; all: "
                    "Augment(camera, lidar, map) with every part on")
    ap.add_argument("--compact", action="store_true", help="ResidentFrames(compact=True): the LiDAR histogram as 4-bit codes")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="train: f32 = the parity path, bf16 = the bf16 training mode")
    ap.add_argument("--store", default=None, help="directory that keeps the frames and their packed form between runs")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        root = args.store or tmp
        os.makedirs(root, exist_ok=True)
        if args.mode == "gather":
            out = run_gather(root, augment=args.augment, compact=args.compact)
        else:
            out = run_train(root, dtype=args.dtype, augment=args.augment, compact=args.compact)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
