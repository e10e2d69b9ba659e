"""Momentum SGD: what the SGD launch costs beside the AdamW launch, and that the AdamW step is left alone.

(1) The optimizer launch alone over the trained range of the vec model's flat buffer (104.6 M floats, independent of the batch),
    two optimizer groups (decay / no decay):
    adamw     mmfn_adamw_groups_f32: 28 B per parameter (p, m, v read and written, g read)
    sgd       mmfn_sgd_groups_f32, momentum 0.9 in both groups: 20 B per parameter (p, buf read and written, g read)
    masked    the same through the MASK instance with nothing frozen: the same bytes
    rows      mmfn_sgd_rows_f32, two step classes (the first and the second half of the tensors) x the two groups: 4 rows
    momentum0 mmfn_sgd_groups_f32 with momentum 0 in both groups: buf is neither loaded nor stored, 12 B per parameter
    The cases alternate round by round; times are device events around `iters` back-to-back launches.  Expected from the bytes
    moved: sgd / adamw = 20 / 28 = 0.71.  Under `rocprofv3 --kernel-trace --stats -- python tools/sgd_bench.py --only launch` the
    kernels appear as optim_step_kernel<AdamwRule, GroupSlots, ...>, <SgdRule, GroupSlots, ...> and <SgdRule, RowSlots, ...>.
(2) The B = 32 replayed AdamW step with nothing frozen and no FusedSGD constructed: ms per step, and the entry points one eager step
    calls (name: count).  Run `tools/unfreeze_bench.py --only step` on the parent commit and compare the two "launches" lines:
    they must be identical call for call.
(3) The `sgd-err` lines of tests/test_sgd_gpu.py (max deviation from torch.optim.SGD in float64), when --errors names a pytest log
    that holds them.

    python tools/sgd_bench.py [--rounds 5] [--iters 50] [--steps 20] [--only launch,step] [--errors LOG] [--out profiles/sgd_bench.txt]
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


def launch_cases(net, rounds, iters):
    from mmfn_amd import ops
    from mmfn_amd.optim import FusedAdamW, configure_optimizers
    L, dev = net._layout, net._layout.device
    opt = FusedAdamW(net, param_groups=configure_optimizers(net))
    gid = opt.group_table().to(dev)     # decay = 0, no decay = 1
    L.grads[:L.tail].normal_().mul_(0.01)
    adam = torch.zeros(16, 8, device=dev)
    sgd, sgd0 = torch.zeros(16, 8, device=dev), torch.zeros(16, 8, device=dev)
    for i, wd in enumerate((1e-2, 0.0)):
        adam[i] = torch.tensor([1e-4, 0.9, 0.999, 1e-8, wd, 1.0, 0.0, 0.0], device=dev)
        sgd[i] = torch.tensor([1e-4, 0.9, 0.0, 0.0, wd, 1.0, 0.0, 0.0], device=dev)
        sgd0[i] = torch.tensor([1e-4, 0.0, 0.0, 0.0, wd, 1.0, 0.0, 0.0], device=dev)
    step = torch.full((1,), 5, dtype=torch.int64, device=dev)
    # two step classes: the tensors of the first and of the second half of the trained range; rows = (group, class)
    half = L.tail // 2
    cls = torch.zeros(L.total // 4, dtype=torch.uint8)
    for n in L.step_classes.names:
        b, e = L.span(n)
        if b >= half:
            cls[b // 4:(e + 3) // 4] = 1
    row_of = (gid.cpu() + 2 * cls).to(torch.uint8).to(dev)
    rows = torch.tensor([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=torch.int32)
    class_steps = torch.tensor([5, 3], dtype=torch.int64, device=dev)
    pgb = (L.params, L.grads, L.exp_avg)
    cases = {
        "adamw": lambda: ops.adamw_groups(L.params, L.grads, L.exp_avg, L.exp_avg_sq, step, adam, 2, group_of=gid, n=L.tail),
        "sgd": lambda: ops.sgd_groups(*pgb, step, sgd, 2, group_of=gid, n=L.tail),
        "masked": lambda: ops.sgd_groups(*pgb, step, sgd, 2, group_of=gid, n=L.tail, mask=True),
        "rows": lambda: ops.sgd_rows(*pgb, class_steps, 2, sgd, 2, row_of, rows, n=L.tail),
        "momentum0": lambda: ops.sgd_groups(*pgb, step, sgd0, 2, group_of=gid, n=L.tail),
    }
    what = {"adamw": ("mmfn_adamw_groups_f32, 2 groups", 28), "sgd": ("mmfn_sgd_groups_f32, 2 groups, momentum 0.9", 20),
            "masked": ("mmfn_sgd_groups_f32 | MASK, nothing frozen", 20), "rows": ("mmfn_sgd_rows_f32, 2 classes x 2 groups", 20),
            "momentum0": ("mmfn_sgd_groups_f32, momentum 0 in both groups", 12)}
    for fn in cases.values():
        _time(fn, 5)
    ms = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            ms[k].append(_time(fn, iters))
    rec = {"what": "optimizer launch alone", "floats": L.tail, "rounds": rounds, "iters": iters}
    for k in cases:
        rec[k] = dict(_summary(ms[k]), what=what[k][0], bytes_per_param=what[k][1])
        rec[k]["GB_per_s"] = round(what[k][1] * L.tail / (rec[k]["ms"] * 1e-3) / 1e9, 1)
    rec["ratio_sgd_over_adamw"] = round(rec["sgd"]["ms"] / rec["adamw"]["ms"], 4)
    rec["ratio_expected_from_bytes"] = round(20 / 28, 4)
    rec["spread_adamw_ms"] = round(max(ms["adamw"]) - min(ms["adamw"]), 4)
    return rec


class _LaunchLog(object):
    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("mmfn_"):
            return fn

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


def step_case(net, inp, gt, rounds, steps):
    """The AdamW step as tools/unfreeze_bench.py measures it (the same "launches" line format, so the parent's line compares)."""
    from mmfn_amd import _lib
    from mmfn_amd.parallel import GraphedStep
    eng = net._engine_for()
    eng.train_step(inp, gt)      # sizes the buffers
    torch.cuda.synchronize()
    real = _lib.lib()
    log = _lib._lib = _LaunchLog(real)
    try:
        eng.train_step(inp, gt)
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
    replay = GraphedStep(eng, None, inp, gt, warm=1)
    for _ in range(3):
        replay()
    ms = [_time(replay, steps) for _ in range(rounds)]
    tail = {k: v for k, v in sorted(log.calls.items()) if "adamw" in k or "sgd" in k or "step" in k}
    return (dict(_summary(ms), what="replayed AdamW step, nothing frozen", batch=int(gt.shape[0]), rounds=rounds, steps=steps,
                 optimizer_launches=tail),
            "launches " + " ".join("%s:%d" % kv for kv in sorted(log.calls.items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="timed optimizer launches per case and round")
    ap.add_argument("--steps", type=int, default=20, help="timed replays per round")
    ap.add_argument("--only", default="launch,step")
    ap.add_argument("--errors", default=None, help="a pytest log of tests/test_sgd_gpu.py (-s): its sgd-err lines are copied")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgd_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgd_bench measures on the GPU: none found")
    import bench
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = MMFN(GlobalConfig(), dev).train()
    lines = []
    if "step" in a.only:      # first: the launch cases below overwrite the gradients and step the parameters many times
        inp, gt = bench.synth_inputs(a.batch, dev, seed=0)
        rec, launches = step_case(net, inp, gt, a.rounds, a.steps)
        lines += [json.dumps(rec), launches]
    if "launch" in a.only:
        lines.append(json.dumps(launch_cases(net, a.rounds, a.iters)))
    if a.errors:
        lines += [l.strip().lstrip(".") for l in open(a.errors, errors="replace") if "sgd-err" in l and "print(" not in l]
    for line in lines:
        print(line, flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
