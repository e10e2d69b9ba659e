"""Waypoint objectives: what the head launches with the objective as a parameter cost beside the original pair, and that the default
step is left alone.

(1) The two head launches alone at B = 32, pred_len = 4 (one wave per sample; both sit near the launch floor):
    fwd_old / bwd_old   mmfn_gru_head_fwd_f32 (+ the loss finalize) / mmfn_gru_head_bwd_f32: the hard-coded mean L1
    fwd_new / bwd_new   mmfn_gru_head_fwd_loss_f32 (+ the same finalize) / mmfn_gru_head_bwd_loss_f32 with smooth-L1(beta = 2),
                        horizon weights and sample weights: about ten more operations per element of pred, two more outputs
    The cases alternate round by round; times are device events around `iters` back-to-back launches.  There is no threshold: the
    record says whether the new pair lies outside the old pair's run-to-run spread.
(2) `bench.py --gpus 1 --steps S --warmup W` of this tree alternated with a tree of the parent commit (--parent DIR, built), with no
    loss set: the default step runs the original launches, so the two must agree within their spread.

    python tools/loss_bench.py [--rounds 5] [--iters 200] [--parent DIR] [--bench-rounds 3] [--out profiles/loss_bench.txt]
"""
import argparse
import json
import os
import subprocess
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
    return {"us": round(1e3 * sum(v) / len(v), 3), "min": round(1e3 * min(v), 3), "max": round(1e3 * max(v), 3)}


def launch_cases(B, steps, rounds, iters):
    from mmfn_amd import ops
    from mmfn_amd._lib import lib
    from mmfn_amd.losses import WaypointLoss
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    gru, out = torch.nn.GRUCell(2, 64), torch.nn.Linear(64, 2)
    P = [t.detach().to(dev).contiguous() for t in (gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh, out.weight, out.bias)]
    w_ih, w_hh, b_ih, b_hh, w_out, b_out = P
    z0, target = torch.randn(B, 64, generator=g).to(dev), (torch.randn(B, 2, generator=g) * 5).to(dev)
    gt = (torch.randn(B, steps, 2, generator=g) * 3).to(dev)
    sw = (torch.rand(B, generator=g) * 3).to(dev)
    mk = lambda *s: torch.empty(*s, device=dev)
    pred, hs, gates, xin = mk(B, steps, 2), mk(B, steps + 1, 64), mk(B, steps, 4, 64), mk(B, steps, 2)
    lt, loss, l1, dz0, part = mk(B), mk(1), mk(B), mk(B, 64), mk(B, lib().mmfn_gru_head_part_floats())
    obj = WaypointLoss("smooth_l1", beta=2.0, step_weights=[2.0, 1.0, 0.5, 0.25, 1.0, 1.0, 1.0, 1.0][:steps])
    table = torch.tensor(obj.table(steps), dtype=torch.float32, device=dev)
    gscale = 1.0 / (B * steps * 2)
    cases = {
        "fwd_old": lambda: ops.gru_head_fwd(z0, target, w_ih, w_hh, b_ih, b_hh, w_out, b_out, gt, pred, hs, gates, xin, lt, loss, steps),
        "fwd_new": lambda: ops.gru_head_fwd_loss(z0, target, w_ih, w_hh, b_ih, b_hh, w_out, b_out, gt, pred, hs, gates, xin, lt, loss,
                                                 obj.kind_code, table, sw, l1, steps),
        "bwd_old": lambda: ops.gru_head_bwd(pred, gt, None, gscale, w_ih, w_hh, w_out, hs, gates, xin, dz0, part, steps),
        "bwd_new": lambda: ops.gru_head_bwd_loss(pred, gt, gscale, w_ih, w_hh, w_out, hs, gates, xin, dz0, part, obj.kind_code, table,
                                                 sw, steps),
    }
    for fn in cases.values():
        _time(fn, 10)
    ms = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            ms[k].append(_time(fn, iters))
    rec = {"what": "head launches alone, us per call (the forward includes the loss finalize launch)", "batch": B, "steps": steps,
           "rounds": rounds, "iters": iters, "new": "smooth_l1(beta=2), horizon weights, sample weights"}
    for k in cases:
        rec[k] = _summary(ms[k])
    for way in ("fwd", "bwd"):
        old, new = rec[way + "_old"], rec[way + "_new"]
        rec[way + "_new_over_old"] = round(new["us"] / old["us"], 4)
        rec[way + "_new_outside_old_spread"] = not (old["min"] <= new["us"] <= old["max"])
    return rec


def bench_rounds(parent, rounds, steps, warmup):
    """bench.py of the parent tree and of this one, alternating, each run a process of its own."""
    lines, vals = [], {"parent": [], "build": []}
    for r in range(rounds):
        for name, root in (("parent", parent), ("build", ROOT)):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=root,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("bench.py failed in %s:\n%s" % (root, (p.stdout + p.stderr)[-2000:]))
            rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            vals[name].append(float(rec["value"]))
            lines.append("%s round %d: %.2f samples/s, %.3f ms per step, loss %s" % (name, r + 1, rec["value"], rec["ms_per_step"],
                                                                                   rec.get("loss")))
    pa, bu = sorted(vals["parent"]), sorted(vals["build"])
    head = ("# bench.py --gpus 1 --steps %d --warmup %d alternated with the parent commit, %d rounds each, no loss set: parent %.2f - %.2f "
            "(median %.2f), this build %.2f - %.2f (median %.2f); the build's median lies %s the parent's range"
            % (steps, warmup, rounds, pa[0], pa[-1], pa[len(pa) // 2], bu[0], bu[-1], bu[len(bu) // 2],
               "inside" if pa[0] <= bu[len(bu) // 2] <= pa[-1] else "OUTSIDE"))
    return [head] + lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--pred-len", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200, help="timed launches per case and round")
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: bench.py alternates with it")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=60)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench measures on the GPU: none found")
    lines = ["# tools/loss_bench.py on one MI355X.  (1) the head launches alone at B = %d, pred_len = %d, cases alternating per round "
             "(us per call from device events: mean, min, max over the rounds); nothing was aimed at" % (a.batch, a.pred_len),
             json.dumps(launch_cases(a.batch, a.pred_len, a.rounds, a.iters))]
    if a.parent:
        torch.cuda.synchronize()
        lines += bench_rounds(os.path.abspath(a.parent), a.bench_rounds, a.bench_steps, a.bench_warmup)
    else:
        lines.append("# not measured: bench.py against the parent commit (no --parent tree given)")
    for line in lines:
        print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
