"""Cost of an attached weight average on the replayed step: ms per step of parallel.GraphedStep captured without and with an
attached EMA (the AVG instance of the grouped AdamW, the BatchNorm buffer copy and the count advance), same process, same
inputs, alternating windows.  Writes one JSON line.

    python tools/average_bench.py --batch 32 [--dtype bf16] [--steps 20] [--rounds 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def _time(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--steps", type=int, default=20, help="replays per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="alternating (plain, averaged) window pairs")
    a = ap.parse_args()
    import bench
    from mmfn_amd.averaging import AveragedMMFN
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    from mmfn_amd.parallel import GraphedStep
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = MMFN(GlobalConfig(act_dtype=a.dtype), dev).train()
    inp, gt = bench.synth_inputs(a.batch, dev, seed=0)
    eng = net._engine_for()
    avg = AveragedMMFN(net, "ema", decay=0.999)
    plain = GraphedStep(eng, None, inp, gt, warm=2)
    eng.attach_average(avg)
    averaged = GraphedStep(eng, None, inp, gt, warm=1)
    ms_plain, ms_avg = [], []
    for r in range(a.rounds + 1):   # round 0 warms both graphs
        eng.detach_average()
        t0 = _time(plain, a.steps)
        eng.attach_average(avg)
        t1 = _time(averaged, a.steps)
        if r:
            ms_plain.append(t0)
            ms_avg.append(t1)
    p, q = min(ms_plain), min(ms_avg)
    out = {"batch": a.batch, "dtype": a.dtype, "steps": a.steps, "rounds": a.rounds,
           "ms_plain_step": round(p, 3), "ms_ema_step": round(q, 3), "delta_ms": round(q - p, 3), "overhead": round(q / p - 1.0, 4),
           "ms_plain_all": [round(x, 3) for x in ms_plain], "ms_ema_all": [round(x, 3) for x in ms_avg],
           "n_averaged": int(avg.n_averaged.item())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
