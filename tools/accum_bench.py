"""Gradient accumulation on the replayed step: ms per micro-step, ms per optimizer step and samples/s of k-step groups
(k - 1 "micro" replays + one "final" replay, parallel.GraphedStep variants) against the plain replayed step, same process,
same inputs.  Writes one JSON line.

    python tools/accum_bench.py --accum 8 --batch 32 [--dtype bf16] [--clip 1.0] [--steps 10] [--warmup 2]
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
    ap.add_argument("--accum", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--clip", type=float, default=None)
    ap.add_argument("--steps", type=int, default=10, help="timed optimizer steps (groups of --accum micro-steps)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import bench
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    from mmfn_amd.parallel import GraphedStep
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = MMFN(GlobalConfig(act_dtype=a.dtype), dev).train()
    inp, gt = bench.synth_inputs(a.batch, dev, seed=0)
    eng = net._engine_for()
    plain = GraphedStep(eng, None, inp, gt, warm=2)
    micro = GraphedStep(eng, None, inp, gt, warm=1, variant="micro")
    final = GraphedStep(eng, None, inp, gt, warm=1, variant="final", clip_grad_norm=a.clip)
    k = a.accum

    def group():
        for _ in range(k - 1):
            micro()
        final()

    for _ in range(a.warmup):
        plain()
        group()
    n_plain = a.steps * k
    ms_plain = _time(plain, n_plain)
    ms_group = _time(group, a.steps)
    ms_micro = _time(micro, n_plain)
    eng.discard_accumulated()
    ms_final = _time(final, n_plain)
    sps_plain = a.batch * 1000.0 / ms_plain
    sps_accum = k * a.batch * 1000.0 / ms_group
    out = {"accum": k, "batch": a.batch, "dtype": a.dtype, "clip": a.clip, "global_batch": k * a.batch,
           "ms_plain_step": round(ms_plain, 3), "ms_per_micro_step": round(ms_group / k, 3),
           "ms_per_optimizer_step": round(ms_group, 3), "ms_micro_alone": round(ms_micro, 3), "ms_final_alone": round(ms_final, 3),
           "samples_per_s_plain": round(sps_plain, 1), "samples_per_s_accum": round(sps_accum, 1),
           "ratio": round(sps_accum / sps_plain, 4),
           "grad_norm": None if a.clip is None else float(eng.last_grad_norm.item())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
