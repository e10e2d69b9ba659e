"""amsgrad: what the fifth stream costs in the AdamW launch, and the parity of both launches with torch.

(1) The AdamW launch alone over the full flat buffer of the vec model (104.6 M trained floats, independent of the batch), two
    optimizer groups (decay / no decay):
    plain    mmfn_adamw_groups_f32: 28 B per parameter (p, m, v read and written, g read)
    amsgrad  mmfn_adamw_groups_ams_f32 with the flag set in both groups: 36 B per parameter (vmax read and written as well)
    off      mmfn_adamw_groups_ams_f32 with the flag clear in both groups: the bytes of `plain` through the new kernel
    The cases alternate round by round; times are device events around `iters` back-to-back launches.  Expected from the bytes
    moved: amsgrad / plain = 36 / 28 = 1.29.  Under `rocprofv3 --kernel-trace --stats -- python tools/amsgrad_bench.py --only adamw`
    the kernels appear as optim_step_kernel<AdamwRule, GroupSlots, ...> and optim_step_kernel<AdamwAmsRule, GroupSlots, ...>.
(2) The `amsgrad-err` lines of tests/test_amsgrad_gpu.py (max deviation of both launches from torch.optim.AdamW in float64), when
    --errors names a pytest log that holds them.

    (amsgrad steps are not captured - parallel.GraphedStep - so there is no replayed step to time.)

    python tools/amsgrad_bench.py [--rounds 5] [--iters 50] [--errors LOG] [--out profiles/amsgrad_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def _summary(v):
    return {"ms": round(sum(v) / len(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def adamw_cases(net, rounds, iters):
    from mmfn_amd import ops
    from mmfn_amd.optim import FusedAdamW, configure_optimizers
    L, dev = net._layout, net._layout.device
    gid = FusedAdamW(net, param_groups=configure_optimizers(net)).group_table().to(dev)     # decay = 0, no decay = 1
    L.grads[:L.tail].normal_().mul_(0.01)
    vmax = L.ensure_max_exp_avg_sq()
    hyper = {}
    for name, flag in (("off", 0.0), ("on", 1.0)):
        h = torch.zeros(16, 8, device=dev)
        for i, wd in enumerate((1e-2, 0.0)):
            h[i] = torch.tensor([1e-4, 0.9, 0.999, 1e-8, wd, 1.0, 0.0, flag], device=dev)
        hyper[name] = h
    step = torch.full((1,), 5, dtype=torch.int64, device=dev)
    pgmv = (L.params, L.grads, L.exp_avg, L.exp_avg_sq)
    cases = {
        "plain": lambda: ops.adamw_groups(*pgmv, step, hyper["off"], 2, group_of=gid, n=L.tail),
        "amsgrad": lambda: ops.adamw_groups(*pgmv, step, hyper["on"], 2, group_of=gid, n=L.tail, vmax=vmax),
        "off": lambda: ops.adamw_groups(*pgmv, step, hyper["off"], 2, group_of=gid, n=L.tail, vmax=vmax),
    }
    for fn in cases.values():
        _time(fn, 5)
    ms = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            ms[k].append(_time(fn, iters))
    rec = {"what": "AdamW launch alone", "floats": L.tail, "rounds": rounds, "iters": iters,
           "plain": dict(_summary(ms["plain"]), what="mmfn_adamw_groups_f32, 2 groups", bytes_per_param=28),
           "amsgrad": dict(_summary(ms["amsgrad"]), what="mmfn_adamw_groups_ams_f32, flag set in both groups", bytes_per_param=36),
           "off": dict(_summary(ms["off"]), what="mmfn_adamw_groups_ams_f32, flag clear in both groups", bytes_per_param=28)}
    for k in cases:
        rec[k]["GB_per_s"] = round(rec[k]["bytes_per_param"] * L.tail / (rec[k]["ms"] * 1e-3) / 1e9, 1)
    rec["ratio_amsgrad_over_plain"] = round(rec["amsgrad"]["ms"] / rec["plain"]["ms"], 4)
    rec["ratio_expected_from_bytes"] = round(36 / 28, 4)
    rec["spread_plain_ms"] = round(max(ms["plain"]) - min(ms["plain"]), 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="timed AdamW launches per case and round")
    ap.add_argument("--only", default="adamw")
    ap.add_argument("--errors", default=None, help="a pytest log of tests/test_amsgrad_gpu.py (-s): its amsgrad-err lines are copied")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amsgrad_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("amsgrad_bench measures on the GPU: none found")
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    lines = []
    if "adamw" in a.only:
        torch.manual_seed(0)
        net = MMFN(GlobalConfig(), torch.device("cuda:0")).train()
        lines.append(json.dumps(adamw_cases(net, a.rounds, a.iters)))
        del net
        torch.cuda.empty_cache()
    if a.errors:
        lines += [l.strip() for l in open(a.errors, errors="replace") if "amsgrad-err" in l]
    for line in lines:
        print(line, flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
