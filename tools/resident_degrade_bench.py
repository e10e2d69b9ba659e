"""What the resident loader's camera degradation costs (data.ResidentLoader(augment=data.Augment(camera, degrade=CameraDegrade))):
the gather launches alone, for a kernel trace, and the training rate.  B = 32, vec, lane_bucket = 16, 768 phase-1 frames per epoch -
the workload of resident_jitter_bench.py and resident_augment_bench.py, whose frames and packed store it shares (--store).

  resident_degrade_bench.py gather [--augment none|jitter|hue|blur|noise|all] [--store DIR]
        ResidentLoader alone: one warm epoch + three timed; trace it with rocprofv3 --kernel-trace --stats
  resident_degrade_bench.py train [--augment none|jitter|all] [--dtype f32|bf16] [--store DIR]
        Trainer.train, graph replay: one warm epoch + two timed

none: the plain loader, one launch per batch (gather_batch_kernel).  jitter: augment=CameraJitter(0.4, 0.4, 0.4, erase_prob 0.5),
two launches, the camera field through camera_jitter_kernel.  hue / blur / noise: Augment(camera=that jitter, degrade=
CameraDegrade(...)) with ONE stage on at probability 1 (hue 0.1; blur_sigma (0.5, 2.0), radius 6; noise_std (2, 12)), two launches,
the camera field through camera_degrade_kernel.  all: hue 0.1, blur_prob 0.5, noise_prob 0.5: half the samples take the tiled path."""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mmfn_amd import data as D  # noqa: E402
import resident_augment_bench as base  # noqa: E402

DEGRADE = {"hue": dict(hue=0.1), "blur": dict(blur_prob=1.0), "noise": dict(noise_prob=1.0),
           "all": dict(hue=0.1, blur_prob=0.5, noise_prob=0.5)}
LAUNCHES = {"none": 1, "jitter": 2, "hue": 2, "blur": 2, "noise": 2, "all": 2}


def make_augment(kind):
    if kind == "none":
        return None
    jitter = D.CameraJitter(brightness=0.4, contrast=0.4, saturation=0.4, erase_prob=0.5, seed=1)
    if kind == "jitter":
        return jitter
    return D.Augment(camera=jitter, degrade=D.CameraDegrade(seed=4, **DEGRADE[kind]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gather", "train"])
    ap.add_argument("--augment", default="none", choices=sorted(LAUNCHES), help="none: the plain loader; jitter: CameraJitter (the "
                    "jitter launch); hue, blur, noise: the degrade launch with that stage alone; all: every stage")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="train: f32 = the parity path, bf16 = the bf16 training mode")
    ap.add_argument("--store", default=None, help="directory that keeps the frames and their packed form between runs")
    args = ap.parse_args()
    base.make_augment, base.LAUNCHES = make_augment, LAUNCHES          # the loops and the store are that tool's
    with tempfile.TemporaryDirectory() as tmp:
        root = args.store or tmp
        os.makedirs(root, exist_ok=True)
        if args.mode == "gather":
            out = base.run_gather(root, augment=args.augment)
        else:
            out = base.run_train(root, dtype=args.dtype, augment=args.augment)
    out.pop("compact", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
