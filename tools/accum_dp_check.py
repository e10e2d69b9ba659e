"""Gradient accumulation under data parallelism, run under torch.distributed.run with 2 ranks (tests/test_grad_accum_gpu.py).

Every rank runs k = 2 micro-batches (Engine.accumulate_step, then Engine.train_step(dp=...)); a single-rank k = 4 run over the
same four micro-batches (rank r's are micro-batches 2r, 2r + 1) is computed in every process beside it.  Per case (fp32 buckets,
fp32 + clipping, bf16 buckets + clipping) it prints
    <case>: lock step <parameters identical on all ranks>, micro-step collectives <reduce() calls during the micro-step>,
            matches one rank <reduced gradient, norm and updated weights equal the single-rank run>
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
    sd = harness.build_oracle("vec", dropout=0.0).state_dict()
    cfg = GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    net, one = MMFN(cfg, dev), MMFN(cfg, dev)
    for m in (net, one):
        m.load_state_dict(sd, strict=True)
        m.train()
    k = 2
    data = [bench.synth_inputs(2, dev, seed=40 + i, lanes=16, n_lidar=4096) for i in range(k * world)]
    mine = data[k * rank:k * rank + k]

    def state(m):
        L, e = m._layout, m._engine_for()
        return [L.params, L.exp_avg, L.exp_avg_sq, L.buffers_flat, L.counters_flat, e.step_count, e.rng_state]

    for m in (net, one):   # warm (filter-transform tables, buffers), then every case starts from the same state
        m._engine_for().accumulate_step(*data[0])
        m._engine_for().discard_accumulated()
    torch.cuda.synchronize()
    snaps = [[t.clone() for t in state(m)] for m in (net, one)]
    eng, ref = net._engine_for(), one._engine_for()
    L, R = net._layout, one._layout
    ok_all = True
    for case, grad_dtype, clip in (("f32", "f32", None), ("f32+clip", "f32", 1e-3), ("bf16+clip", "bf16", 1e-3)):
        for m, snap in zip((net, one), snaps):
            for dst, src in zip(state(m), snap):
                dst.copy_(src)
        torch.cuda.synchronize()
        p0 = L.params.clone()
        dp = DataParallel(net, dist, grad_dtype=grad_dtype)
        dp.broadcast_parameters()
        calls = [0]
        reduce = dp.reduce

        def counting(key, reduce=reduce):
            calls[0] += 1
            return reduce(key)

        dp.reduce = counting
        for inp, gt in mine[:-1]:
            eng.accumulate_step(inp, gt)
        micro_calls = calls[0]
        eng.train_step(*mine[-1], dp=dp, clip_grad_norm=clip)
        final_calls = calls[0] - micro_calls
        for inp, gt in data[:-1]:
            ref.accumulate_step(inp, gt)
        ref.train_step(*data[-1], clip_grad_norm=clip)
        torch.cuda.synchronize()
        ps = [torch.empty_like(L.params) for _ in range(world)]
        dist.all_gather(ps, L.params)
        lock = all(torch.equal(ps[0], p) for p in ps) and final_calls > 0
        # the reduced, folded gradient (a sum: the 1 / (k * world) is in AdamW) against the single-rank sum of four
        g, gr = L.grads[:L.tail].double(), R.grads[:R.tail].double()
        tol = 1e-5 if grad_dtype == "f32" else 2e-2
        grad_ok = (g - gr).norm().item() <= tol * gr.norm().item()
        norm_ok = True
        if clip is not None:
            a, b = float(eng.last_grad_norm.item()), float(ref.last_grad_norm.item())
            norm_ok = abs(a - b) <= tol * b and float(eng._norm["out"][1].item()) < 1.0
        # updated weights on every element whose gradient sign the two summation orders cannot flip
        # (bf16 buckets: relative gradient errors near 1 % would move updates in AdamW's eps regime; demand 1 % separation)
        sure = gr.abs() > (10.0 if grad_dtype == "f32" else 100.0) * (g - gr).abs() + 1e-6 * gr.abs().max()
        du = (L.params[:L.tail].double() - p0[:L.tail].double()) - (R.params[:R.tail].double() - p0[:R.tail].double())
        upd_ok = bool(sure.float().mean().item() >= 0.1) and du[sure].abs().max().item() <= 2e-6
        match = grad_ok and norm_ok and upd_ok
        ok_all = ok_all and lock and match and micro_calls == 0
        if rank == 0:
            print("%s: lock step %s, micro-step collectives %d, matches one rank %s   (gradient %s, norm %s, update %s)"
                  % (case, lock, micro_calls, match, grad_ok, norm_ok, upd_ok), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok_all else 1)


if __name__ == "__main__":
    main()
