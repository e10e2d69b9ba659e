"""What the resident loader's radar and speed augmentation costs (data.ResidentLoader(augment=data.Augment(radar=RadarNoise,
speed=SpeedNoise))): the gather launches alone, for a kernel trace, and the training rate.  768 phase-1 frames per epoch, the
frames and packed store of trainer_bench.py (--store keeps them between runs); lane_bucket = 16; B = 16 for the radar model
('rad'), B = 32 for 'vec' unless --batch says otherwise.

  resident_radar_bench.py gather [--variant rad|vec] [--augment none|radar|speed|both] [--batch B] [--store DIR]
        ResidentLoader alone: one warm epoch + three timed; trace it with rocprofv3 --kernel-trace --stats
  resident_radar_bench.py train [--variant rad|vec] [--augment none|radar|speed|both] [--dtype f32|bf16] [--batch B] [--store DIR]
        Trainer.train, graph replay: one warm epoch + two timed

none: the plain loader, one launch per batch (gather_batch_kernel).  radar: Augment(radar=RadarNoise(point_drop 0.2, depth_std 0.5,
angle_std 0.02, velocity_std 0.5)), 'rad' only; speed: Augment(speed=SpeedNoise(std 0.5, drop_prob 0.2)); both: the two together.
Each is two launches: gather_batch_kernel without radar, radar_adj and / or velocity, and radar_speed_kernel (one workgroup per
sample; with the radar part it writes 405 + 6561 floats per sample, with the speed part alone one)."""
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

LAUNCHES = {"none": 1, "radar": 2, "speed": 2, "both": 2}
BATCH = {"rad": 16, "vec": 32}


def make_augment(kind):
    if kind == "none":
        return None
    radar = D.RadarNoise(point_drop=0.2, depth_std=0.5, angle_std=0.02, velocity_std=0.5, seed=5)
    speed = D.SpeedNoise(std=0.5, drop_prob=0.2, seed=6)
    return D.Augment(radar=radar if kind in ("radar", "both") else None, speed=speed if kind in ("speed", "both") else None)


def make_loader(root, n, cfg, variant, B, augment):
    packed = packed_store(root, n, cfg)
    res = D.ResidentFrames(packed, "cuda:0", cfg, variant)
    return res, D.ResidentLoader(res, batch_size=B, lane_bucket=16, augment=make_augment(augment))


def run_gather(root, variant="rad", B=16, n=768, epochs=3, augment="none"):
    """Wall time per batch (host clock over whole epochs that end in a synchronise, after a warm epoch; it holds the host's work per
    batch too) and the bytes the batch's launches move, from the shapes; the kernels' own times are the trace's."""
    cfg = GlobalConfig()
    res, loader = make_loader(root, n, cfg, variant, B, augment)
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
    return {"variant": variant, "batch": B, "augment": augment, "batches": batches + timed, "launches_per_batch": LAUNCHES[augment],
            "wall_us_per_batch": round(dt / timed * 1e6, 1), "bytes_read_per_batch": read // batches,
            "bytes_written_per_batch": written // batches}


def run_train(root, variant="rad", B=16, n=768, epochs=2, dtype="f32", augment="none"):
    from mmfn_amd.model import MMFN
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import Trainer
    cfg = GlobalConfig(act_dtype=dtype)
    _, loader = make_loader(root, n, cfg, variant, B, augment)
    torch.manual_seed(0)
    net = MMFN(cfg, "cuda:0", variant)
    opt = FusedAdamW(net, lr=1e-4)
    tr = Trainer("cuda:0", None)
    tr.train(net, loader, cfg, opt, graph=True)     # warm epoch (buffers, capture)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(epochs):
        tr.train(net, loader, cfg, opt, graph=True)
    torch.cuda.synchronize()
    dt = time.time() - t0
    return {"variant": variant, "batch": B, "dtype": dtype, "augment": augment, "samples_per_s": round(epochs * n / dt, 1),
            "ms_per_step": round(dt / (epochs * n / B) * 1e3, 2), "train_loss": [round(v, 5) for v in tr.train_loss]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gather", "train"])
    ap.add_argument("--variant", default="rad", choices=sorted(BATCH), help="rad: the radar model's store; vec: no radar field (none, speed)")
    ap.add_argument("--augment", default="none", choices=sorted(LAUNCHES), help="none: the plain loader; radar: RadarNoise; speed: "
                    "SpeedNoise; both: the two in one launch")
    ap.add_argument("--batch", type=int, default=None, help="samples per batch (default: 16 for rad, 32 for vec)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="train: f32 = the parity path, bf16 = the bf16 training mode")
    ap.add_argument("--store", default=None, help="directory that keeps the frames and their packed form between runs")
    args = ap.parse_args()
    B = args.batch or BATCH[args.variant]
    with tempfile.TemporaryDirectory() as tmp:
        root = args.store or tmp
        os.makedirs(root, exist_ok=True)
        if args.mode == "gather":
            out = run_gather(root, args.variant, B, augment=args.augment)
        else:
            out = run_train(root, args.variant, B, dtype=args.dtype, augment=args.augment)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
