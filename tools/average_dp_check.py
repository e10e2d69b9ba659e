"""An attached weight average under data parallelism, run under torch.distributed.run with 2 ranks (tests/test_weight_average_gpu.py).

Every rank attaches its own EMA (decay 0.9) and runs three data-parallel train_steps on its own batches; the average is updated
inside each rank's AdamW launch with no collective.  torch's get_ema_multi_avg_fn over the post-step parameters is computed
beside it.  Prints
    average: lock step <averages bit-identical on all ranks>, matches torch <lerp over the post-step parameters, <= 1 ulp>
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
    from torch.optim.swa_utils import get_ema_multi_avg_fn
    from mmfn_amd.averaging import AveragedMMFN
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    from mmfn_amd.parallel import DataParallel
    from oracle import harness
    torch.set_num_threads(max(1, bench.usable_cores() // world))
    net = MMFN(GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0), dev)
    net.load_state_dict(harness.build_oracle("vec", dropout=0.0).state_dict(), strict=True)
    net.train()
    eng, L = net._engine_for(), net._layout
    data = [bench.synth_inputs(2, dev, seed=50 + 3 * rank + i, lanes=16, n_lidar=4096) for i in range(3)]
    dp = DataParallel(net, dist)
    dp.broadcast_parameters()
    avg = AveragedMMFN(net, "ema", decay=0.9)
    if rank == 1:
        avg.module._layout.params.mul_(0.5)     # out of step on purpose: broadcast_average brings it back (as after a resume)
    dp.broadcast_average(avg)
    eng.attach_average(avg)
    ref, fn = None, get_ema_multi_avg_fn(0.9)
    for i, (inp, gt) in enumerate(data):
        eng.train_step(inp, gt, dp=dp)
        torch.cuda.synchronize()
        if ref is None:
            ref = L.params[:L.tail].clone()
        else:
            r = [ref]
            fn(r, [L.params[:L.tail]], torch.tensor(i, device=dev))
    A = avg.module._layout
    got = A.params[:A.tail]
    ps = [torch.empty_like(got) for _ in range(world)]
    dist.all_gather(ps, got)
    lock = all(torch.equal(ps[0], p) for p in ps) and int(avg.n_averaged.item()) == 3

    def ordered(t):
        b = t.contiguous().view(torch.int32).long()
        return torch.where(b < 0, -(b & 0x7FFFFFFF), b)

    ulps = int((ordered(got) - ordered(ref)).abs().max().item())
    match = ulps <= 1 and torch.equal(A.params[A.tail:], L.params[L.tail:])
    if rank == 0:
        print("average: lock step %s, matches torch %s   (%s)" % (lock, match, "bit-identical" if ulps == 0 else "%d ulp" % ulps),
              flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if lock and match else 1)


if __name__ == "__main__":
    main()
