"""Cost of the non-finite guard on the replayed step, and of the per-tensor statistics pass.  Writes one JSON line.

    python tools/guard_bench.py --side guard   [--batch 32] [--dtype bf16] [--steps 30] [--warmup 5]
    python tools/guard_bench.py --side clipinf ...   the unguarded step with clip_grad_norm=inf (the guard's launch sequence
                                                     without the flag, the snapshot copies and the gated restore)
    python tools/guard_bench.py --side plain ...     the plain step (no norm pass at all), for information

--side clipinf and plain use nothing this option added, so the same file times a checkout of an older commit.  --side guard
also times one Engine.tensor_stats("grads") pass and the plain grouped AdamW launch over the same buffers (the statistics pass
reads 4 B per parameter, AdamW moves 28 B: it must not be the slower one).  Compare sides by alternating whole runs.
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
    ap.add_argument("--side", choices=("guard", "clipinf", "plain"), required=True)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import bench
    from mmfn_amd import ops
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    from mmfn_amd.parallel import GraphedStep
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = MMFN(GlobalConfig(act_dtype=a.dtype), dev).train()
    inp, gt = bench.synth_inputs(a.batch, dev, seed=0)
    eng, L = net._engine_for(), net._layout
    if a.side == "guard":
        eng.set_nonfinite_guard(True)
    if a.side == "plain":
        step = GraphedStep(eng, None, inp, gt, warm=2)
    else:
        step = GraphedStep(eng, None, inp, gt, warm=2, variant="final", fold=False,
                           clip_grad_norm=None if a.side == "guard" else float("inf"))
    for _ in range(a.warmup):
        step()
    out = {"side": a.side, "batch": a.batch, "dtype": a.dtype, "steps": a.steps, "ms_per_step": round(_time(step, a.steps), 4)}
    if a.side != "plain":
        out["grad_norm"] = float(eng.last_grad_norm.item())
    if a.side == "guard":
        out["skipped_steps"] = int(eng.skipped_steps.item())
        eng.tensor_stats("grads")
        out["ms_tensor_stats"] = round(_time(lambda: eng.tensor_stats("grads"), 20), 4)
        snap = [t.clone() for t in (L.params, L.exp_avg, L.exp_avg_sq)]
        scratch_step = eng.step_count.clone()
        adam = lambda: ops.adamw_groups(L.params, L.grads, L.exp_avg, L.exp_avg_sq, scratch_step, eng.opt_hyper, 1, n=L.tail)
        adam()
        out["ms_adamw_groups"] = round(_time(adam, 20), 4)
        for dst, src in zip((L.params, L.exp_avg, L.exp_avg_sq), snap):
            dst.copy_(src)
        out["params"] = int(L.tail)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
