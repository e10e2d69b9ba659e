"""The non-finite guard under data parallelism, run under torch.distributed.run with 2 ranks (tests/test_nonfinite_guard_gpu.py).

Every rank arms the guard and runs one step whose batch is poisoned on rank 1 ONLY (a NaN in velocity[1]); the norm is taken
after the gradient reduction, so every rank must reach the same decision with no extra collective.  Then one clean step.  Per
case (fp32 buckets, bf16 buckets) it prints
    <case>: both ranks skipped <skipped_steps == 1 everywhere>, parameters untouched <identical across ranks and equal to the start>,
            lock step after the next step <the clean step changed the parameters, identically on all ranks>
Ranks share cuda:0 over gloo when fewer devices than ranks are visible (RCCL refuses two ranks per device).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    backend = "nccl" if torch.cuda.device_count() >= world else "gloo"
    local = rank if backend == "nccl" else 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group("gloo")
    import bench
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    from mmfn_amd.parallel import DataParallel
    from oracle import harness
    torch.set_num_threads(max(1, bench.usable_cores() // world))
    net = MMFN(GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0), dev)
    net.load_state_dict(harness.build_oracle("vec", dropout=0.0).state_dict(), strict=True)
    net.train()
    eng, L = net._engine_for(), net._layout
    eng.set_nonfinite_guard(True)
    first = bench.synth_inputs(2, dev, seed=60 + rank, lanes=16, n_lidar=4096)
    second = bench.synth_inputs(2, dev, seed=70 + rank, lanes=16, n_lidar=4096)
    if rank == 1:
        vel = first[0]["velocity"].clone()
        vel[1] = float("nan")
        first = (dict(first[0], velocity=vel), first[1])

    def gathered(t):
        out = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(out, t)
        return out

    ok_all = True
    for case in ("f32", "bf16"):
        dp = DataParallel(net, dist, grad_dtype=case)
        dp.broadcast_parameters()
        torch.cuda.synchronize()
        start = [t.clone() for t in (L.params, L.exp_avg, L.exp_avg_sq, L.buffers_flat, L.counters_flat, eng.step_count)]
        skipped0 = int(eng.skipped_steps.item())
        eng.train_step(*first, dp=dp)
        torch.cuda.synchronize()
        counts = gathered(eng.skipped_steps - skipped0)
        skipped = all(int(c.item()) == 1 for c in counts) and not bool(torch.isfinite(eng.last_grad_norm).item())
        ps = gathered(L.params)
        untouched = all(torch.equal(ps[0], p) for p in ps) and all(
            torch.equal(a, b) for a, b in zip(start, (L.params, L.exp_avg, L.exp_avg_sq, L.buffers_flat, L.counters_flat, eng.step_count)))
        eng.train_step(*second, dp=dp)
        torch.cuda.synchronize()
        ps = gathered(L.params)
        counts = gathered(eng.skipped_steps - skipped0)
        lock = all(torch.equal(ps[0], p) for p in ps) and not torch.equal(L.params, start[0]) and \
            bool(torch.isfinite(L.params).all().item()) and all(int(c.item()) == 1 for c in counts) and \
            int(eng.step_count.item()) == int(start[5].item()) + 1
        ok_all = ok_all and skipped and untouched and lock
        if rank == 0:
            print("%s: both ranks skipped %s, parameters untouched %s, lock step after the next step %s" % (case, skipped, untouched, lock),
                  flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok_all else 1)


if __name__ == "__main__":
    main()
