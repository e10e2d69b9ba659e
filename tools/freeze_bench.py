"""Frozen parameters on the replayed step: ms per step with (a) nothing frozen, (b) the three trunks and VectorNet frozen,
(c) only the head trainable - one process, one captured step (parallel.GraphedStep) per case, the cases interleaved round by
round so that drift hits all of them alike.  B = 32 vec, fp32 and bf16.  Prints one line per dtype with the mean over the
rounds and the round-to-round spread (min .. max) of every case, and writes the same lines to --out.

    python tools/freeze_bench.py [--batch 32] [--rounds 5] [--steps 20] [--dtypes f32,bf16] [--out profiles/freeze_bench.txt]
    python tools/freeze_bench.py --only b --dtypes f32 --rounds 1 --steps 40     # one case alone, e.g. under a kernel trace:
                                                                                 # two step counts give the kernels per step
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

TRUNKS = ("encoder.image_encoder.", "encoder.lidar_encoder.", "encoder.img_map_encoder.", "encoder.vectornet_encoder.")
HEAD = ("join.", "decoder.", "output.")
CASES = {"a": "nothing frozen", "b": "trunks + VectorNet frozen", "c": "only the head trainable"}


def _time(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _freeze(net, case):
    if case == "b":
        net.freeze(*TRUNKS)
    elif case == "c":
        net.freeze()
        net.unfreeze(*HEAD)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed replays per case and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--only", default="abc", help="the cases to run, e.g. 'b'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeze_bench.txt"))
    a = ap.parse_args()
    import bench
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    from mmfn_amd.parallel import GraphedStep
    dev = torch.device("cuda:0")
    inp, gt = bench.synth_inputs(a.batch, dev, seed=0)
    lines = []
    for dtype in a.dtypes.split(","):
        steps = {}
        for case in a.only:
            torch.manual_seed(0)
            net = MMFN(GlobalConfig(act_dtype=dtype), dev).train()
            _freeze(net, case)
            steps[case] = GraphedStep(net._engine_for(), None, inp, gt, warm=2)
            for _ in range(a.warmup):
                steps[case]()
        ms = {case: [] for case in steps}
        for _ in range(a.rounds):
            for case, step in steps.items():
                ms[case].append(_time(step, a.steps))
        rec = {"dtype": dtype, "batch": a.batch, "rounds": a.rounds, "steps": a.steps}
        for case, v in ms.items():
            rec[case] = {"what": CASES[case], "ms_per_step": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        if "a" in ms:
            rec["spread_a_ms"] = round(max(ms["a"]) - min(ms["a"]), 3)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del steps
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
