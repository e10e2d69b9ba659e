"""Per-tensor step counts: what the AdamW launch with step classes costs, and that the nothing-frozen step is left alone.

(1) The AdamW launch alone over the full flat buffer of the vec model (104.8 M trained parameters, independent of the batch):
    a  the existing masked instance (mmfn_adamw_groups_f32 | MASK), two optimizer groups, one shared step counter
    b  the instance with step classes (mmfn_adamw_rows_f32), one class x the same two groups: 2 rows
    c  the same with four classes (the four backward stages of the layout) x two groups: 8 rows
    every case reads the same byte table shape and moves the same p / g / m / v bytes; the cases alternate round by round.
(2) The B = 32 replayed step with nothing frozen: ms per step, and the entry points one eager step calls (name: count).  Run
    the same command on the parent commit (--only step) and compare the two "launches" lines: they must be identical - that is
    the check, the time only has to sit inside the run-to-run spread.

    python tools/unfreeze_bench.py [--rounds 5] [--iters 50] [--steps 20] [--only adamw,step] [--out profiles/unfreeze_bench.txt]
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
    from mmfn_amd.params import StepClasses
    L, dev = net._layout, net._layout.device
    gid = FusedAdamW(net, param_groups=configure_optimizers(net)).group_table()     # decay = 0, no decay = 1; nothing frozen
    L.grads[:L.tail].normal_().mul_(0.01)
    hyper = torch.zeros(16, 8, device=dev)
    for i, wd in enumerate((1e-2, 0.0)):
        hyper[i, :6] = torch.tensor([1e-4, 0.9, 0.999, 1e-8, wd, 1.0], device=dev)
    names = [n for n in L.offsets if n not in L.unused]
    one, four = StepClasses(names), StepClasses(names)
    one.set_steps([5] * len(names))
    four.set_steps([5 + L.stage_of(n) for n in names])
    tab1, rows1 = one.row_table(L, frozenset(), gid)
    tab4, rows4 = four.row_table(L, frozenset(), gid)
    assert rows1.shape[0] == 2 and rows4.shape[0] == 8
    gid_d, tab1, tab4 = gid.to(dev), tab1.to(dev), tab4.to(dev)
    step = torch.full((1,), 5, dtype=torch.int64, device=dev)
    cs1 = torch.tensor(one.values, dtype=torch.int64, device=dev)
    cs4 = torch.tensor(four.values, dtype=torch.int64, device=dev)
    pgmv = (L.params, L.grads, L.exp_avg, L.exp_avg_sq)
    cases = {
        "a": lambda: ops.adamw_groups(*pgmv, step, hyper, 2, group_of=gid_d, n=L.tail, mask=True),
        "b": lambda: ops.adamw_rows(*pgmv, cs1, 1, hyper, 2, tab1, rows1, n=L.tail),
        "c": lambda: ops.adamw_rows(*pgmv, cs4, 4, hyper, 2, tab4, rows4, n=L.tail),
    }
    for fn in cases.values():
        _time(fn, 5)
    ms = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            ms[k].append(_time(fn, iters))
    rec = {"what": "AdamW launch alone", "floats": L.tail, "rounds": rounds, "iters": iters,
           "a": dict(_summary(ms["a"]), what="masked instance, shared counter, 2 groups"),
           "b": dict(_summary(ms["b"]), what="step classes: 1 class x 2 groups"),
           "c": dict(_summary(ms["c"]), what="step classes: 4 classes x 2 groups")}
    rec["spread_a_ms"] = round(max(ms["a"]) - min(ms["a"]), 4)
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
    tail = {k: v for k, v in sorted(log.calls.items()) if "adamw" in k or "step" in k}
    return (dict(_summary(ms), what="replayed step, nothing frozen", batch=int(gt.shape[0]), rounds=rounds, steps=steps,
                 optimizer_launches=tail),
            "launches " + " ".join("%s:%d" % kv for kv in sorted(log.calls.items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="timed AdamW launches per case and round")
    ap.add_argument("--steps", type=int, default=20, help="timed replays per round")
    ap.add_argument("--only", default="adamw,step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unfreeze_bench.txt"))
    a = ap.parse_args()
    import bench
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = MMFN(GlobalConfig(), dev).train()
    lines = []
    if "step" in a.only:      # first: the AdamW cases below overwrite the gradients and step the parameters many times
        inp, gt = bench.synth_inputs(a.batch, dev, seed=0)
        rec, launches = step_case(net, inp, gt, a.rounds, a.steps)
        lines += [json.dumps(rec), launches]
    if "adamw" in a.only:
        lines.append(json.dumps(adamw_cases(net, a.rounds, a.iters)))
    for line in lines:
        print(line, flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
