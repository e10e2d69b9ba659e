"""amsgrad on a module built on the CPU (no engine): FusedAdamW's constructor and groups, the state_dict / load_state_dict layout
with max_exp_avg_sq, and the float64 restatement of torch's single-tensor amsgrad step that tests/test_amsgrad_gpu.py uses as its
yardstick, checked here against torch.optim.AdamW(amsgrad=True) itself."""
import functools

import pytest
import torch

SCALES = (1.0, 1.0, 0.1, 0.01, 0.01, 0.01)   # gradients shrink after the second step: vmax > v for most elements from step 3 on
BOUND = 1e-6   # max |dp| against torch at lr ~ 1e-4, |p| < 1.5: tests/test_kernels_gpu.py::test_adamw_matches_torch, tests/test_tensor_steps_gpu.py


def shrinking_grads(n, seed, steps=len(SCALES)):
    """One seeded normal draw per step, scaled by SCALES."""
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * SCALES[i] for i in range(steps)]


def amsgrad_reference(p, grads, groups, spans):
    """torch's single-tensor AdamW (non-capturable) restated in float64 over a flat vector: `groups` are dicts with lr, betas, eps,
    weight_decay, amsgrad (and optionally grad_scale); spans[i] = (begin, end) of group i.  Returns the trajectory: per step a
    dict of float64 p, m, v, vmax (vmax stays zero where amsgrad is off)."""
    p = p.double().clone()
    m, v, vmax = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t, g in enumerate(grads, 1):
        for grp, (b, e) in zip(groups, spans):
            beta1, beta2 = grp["betas"]
            gg = g[b:e].double() * grp.get("grad_scale", 1.0)
            p[b:e] *= 1.0 - grp["lr"] * grp["weight_decay"]
            m[b:e] = m[b:e] + (gg - m[b:e]) * (1.0 - beta1)
            v[b:e] = v[b:e] * beta2 + (1.0 - beta2) * gg * gg
            bc1, bc2_sqrt = 1.0 - beta1 ** t, (1.0 - beta2 ** t) ** 0.5
            if grp["amsgrad"]:
                vmax[b:e] = torch.maximum(vmax[b:e], v[b:e])
                denom = vmax[b:e].sqrt() / bc2_sqrt + grp["eps"]
            else:
                denom = v[b:e].sqrt() / bc2_sqrt + grp["eps"]
            p[b:e] = p[b:e] - (grp["lr"] / bc1) * (m[b:e] / denom)
        out.append(dict(p=p.clone(), m=m.clone(), v=v.clone(), vmax=vmax.clone()))
    return out


def torch_reference(p, grads, groups, spans, dtype=torch.float64):
    """torch.optim.AdamW itself on CPU tensors, one parameter per group; the same trajectory format."""
    refs = [torch.nn.Parameter(p[b:e].to(dtype).clone()) for b, e in spans]
    opt = torch.optim.AdamW([dict(params=[r], lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"],
                                  amsgrad=g["amsgrad"]) for r, g in zip(refs, groups)])
    out = []
    for g in grads:
        for r, (b, e) in zip(refs, spans):
            r.grad = g[b:e].to(dtype).clone()
        opt.step()
        cat = lambda key: torch.cat([opt.state[r][key] if key in opt.state[r] else torch.zeros_like(r) for r in refs]).double().clone()
        out.append(dict(p=torch.cat([r.detach() for r in refs]).double().clone(), m=cat("exp_avg"), v=cat("exp_avg_sq"),
                        vmax=cat("max_exp_avg_sq")))
    return out


# beta2 well below the default 0.999 in the amsgrad groups: v then falls 5 - 10 % per step once the gradients shrink, the denominator
# built from vmax differs from the one built from v by as much, and the two trajectories part by hundreds of BOUND at these rates
# (at 0.999 v stays within 0.1 % of vmax per step and the difference would sit below the bound: such inputs would show nothing)
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.9), eps=1e-8, weight_decay=1e-2, amsgrad=True),
          dict(lr=2e-3, betas=(0.85, 0.99), eps=1e-8, weight_decay=2e-2, amsgrad=False),
          dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=0.0, amsgrad=True)]


def test_restatement_equals_torch_amsgrad_and_the_inputs_tell_amsgrad_from_plain():
    n = 4 * (3 * 256 + 1)
    spans = [(0, 1000), (1000, 2104), (2104, n)]
    p0 = torch.rand(n, generator=torch.Generator().manual_seed(5)) * 3.0 - 1.5
    grads = shrinking_grads(n, 6)
    mine, ref = amsgrad_reference(p0, grads, GROUPS, spans), torch_reference(p0, grads, GROUPS, spans)
    for a, b in zip(mine, ref):
        for k in ("p", "m", "v", "vmax"):
            # float64 against float64: two evaluation orders of the same expression, a few ulps of float64
            assert (a[k] - b[k]).abs().max().item() < 1e-13, k
    # the inputs distinguish amsgrad from the plain step by far more than the GPU tests' tolerance ...
    plain = amsgrad_reference(p0, grads, [dict(g, amsgrad=False) for g in GROUPS], spans)
    on = torch.cat([torch.arange(b, e) for g, (b, e) in zip(GROUPS, spans) if g["amsgrad"]])
    off = torch.arange(*spans[1])
    assert (mine[-1]["p"][on] - plain[-1]["p"][on]).abs().median().item() > 100 * BOUND
    assert torch.equal(mine[-1]["p"][off], plain[-1]["p"][off])
    # ... and vmax is not v in at least half the elements of the amsgrad groups
    assert (mine[-1]["vmax"][on] != mine[-1]["v"][on]).float().mean().item() >= 0.5
    assert bool((mine[-1]["vmax"][off] == 0).all())


# ------------------------------------------------------------------------------------------------ FusedAdamW on a CPU module
@functools.lru_cache(maxsize=None)
def _net():
    from mmfn_amd.config import GlobalConfig
    import mmfn_amd.model as M
    return M.MMFN(GlobalConfig(), "cpu")


def _fresh(net):
    """(the module is shared between the tests: every one starts from a layout without the fifth buffer and without counts)"""
    L = net._layout
    L.max_exp_avg_sq = None
    L.exp_avg.zero_()
    L.exp_avg_sq.zero_()
    L.step_classes.set_steps([0] * len(L.step_classes.names))
    return net


def test_constructor_and_groups():
    from mmfn_amd.optim import FusedAdamW, configure_optimizers
    net = _fresh(_net())
    plain = FusedAdamW(net, lr=1e-4)
    assert plain.defaults["amsgrad"] is False and plain.amsgrad_flags() == (False,) and net._layout.max_exp_avg_sq is None
    assert plain.state_dict()["param_groups"][0]["amsgrad"] is False
    assert len(plain.hyper_rows()[0]) == 5                      # the rows stay 5-tuples: the flags travel beside them
    opt = FusedAdamW(net, lr=1e-4, amsgrad=True)
    L = net._layout
    assert opt.amsgrad_flags() == (True,) and opt.state_dict()["param_groups"][0]["amsgrad"] is True
    assert L.max_exp_avg_sq is not None and L.max_exp_avg_sq.shape == L.params.shape and not bool(L.max_exp_avg_sq.any())
    assert len(opt.hyper_rows()[0]) == 5
    # a group dict's own "amsgrad" wins over the constructor's, like the four hyper-parameters
    groups = configure_optimizers(net)
    groups[0]["amsgrad"] = True
    mixed = FusedAdamW(_fresh(net), lr=1e-4, param_groups=groups)
    assert mixed.amsgrad_flags() == (True, False)
    assert [g["amsgrad"] for g in mixed.state_dict()["param_groups"]] == [True, False]
    groups[1]["amsgrad"] = True
    assert FusedAdamW(net, lr=1e-4, param_groups=groups, amsgrad=False).amsgrad_flags() == (True, True)
    # torch lets a caller flip the flag of a live group: the buffer appears with it
    late = FusedAdamW(_fresh(net), lr=1e-4)
    assert net._layout.max_exp_avg_sq is None
    late.param_groups[0]["amsgrad"] = True
    late.hyper_rows()
    assert net._layout.max_exp_avg_sq is not None


def _torch_amsgrad_state(net, amsgrad=True, steps=2):
    """A torch.optim.AdamW(amsgrad=...) state dict over CPU copies of the model's parameters after `steps` steps on seeded
    shrinking gradients; every never-trained parameter keeps grad = None, as in a reference run."""
    L = net._layout
    names = [n for n, _ in net.named_parameters()]
    params = [torch.nn.Parameter(p.detach().clone()) for p in net.parameters()]
    opt = torch.optim.AdamW(params, lr=1e-4, amsgrad=amsgrad)
    gen = torch.Generator().manual_seed(3)
    for i in range(steps):
        for n, r in zip(names, params):
            r.grad = None if n in L.unused else torch.randn(r.shape, generator=gen) * (1.0, 0.1)[i % 2]
        opt.step()
    return opt, names, params


def test_state_dict_round_trip_with_torch_in_checkpoint_shape():
    from mmfn_amd.optim import FusedAdamW
    net = _fresh(_net())
    L = net._layout
    topt, names, params = _torch_amsgrad_state(net)
    sd = topt.state_dict()
    opt = FusedAdamW(net, lr=1e-3)                # amsgrad off here: the checkpoint's groups decide
    opt.load_state_dict(sd)
    assert opt.amsgrad_flags() == (True,) and L.max_exp_avg_sq is not None
    # one convolution filter element by element: OIHW in the checkpoint, OHWI in the flat buffer
    conv = "encoder.lidar_encoder._model.layer2.0.conv1.weight"
    idx = names.index(conv)
    want = sd["state"][idx]["max_exp_avg_sq"]
    o, i, kh, kw = want.shape
    off, n = L.offsets[conv]
    flat = L.max_exp_avg_sq[off:off + n].view(o, kh, kw, i)
    assert float(want.abs().max()) > 0
    for (a, b, c, d) in ((0, 0, 0, 0), (3, 5, 1, 2), (o - 1, i - 1, kh - 1, kw - 1), (7, 2, 2, 0)):
        assert flat[a, c, d, b].item() == want[a, b, c, d].item()
    # ... and every stepped tensor's second moment is below its maximum where the second gradient was the smaller one
    off, n = L.offsets["join.0.bias"]
    assert bool((L.max_exp_avg_sq[off:off + n] >= L.exp_avg_sq[off:off + n]).all())
    # a never-trained tensor has no entry: zeros
    u = sorted(L.unused)[0]
    off, n = L.offsets[u]
    assert not bool(L.max_exp_avg_sq[off:off + n].any())
    # back out: torch accepts it and finds max_exp_avg_sq in parameter shape, equal to what it wrote
    out = opt.state_dict()
    assert out["param_groups"][0]["amsgrad"] is True and set(out["state"]) == set(sd["state"])
    fresh = torch.optim.AdamW(params, lr=1e-4, amsgrad=True)
    fresh.load_state_dict(out)
    for k in (idx, names.index("join.0.bias")):
        assert fresh.state[params[k]]["max_exp_avg_sq"].shape == params[k].shape
        assert torch.equal(out["state"][k]["max_exp_avg_sq"], sd["state"][k]["max_exp_avg_sq"])
        assert torch.equal(out["state"][k]["exp_avg_sq"], sd["state"][k]["exp_avg_sq"])
    # a checkpoint without amsgrad switches an amsgrad optimizer off (the groups come from the checkpoint) and carries no maximum
    popt, _, _ = _torch_amsgrad_state(net, amsgrad=False)
    opt.load_state_dict(popt.state_dict())
    assert opt.amsgrad_flags() == (False,) and not bool(L.max_exp_avg_sq.any())
    out = opt.state_dict()
    assert out["param_groups"][0]["amsgrad"] is False and all("max_exp_avg_sq" not in st for st in out["state"].values())


def test_amsgrad_checkpoint_without_the_maximum_is_refused():
    from mmfn_amd.optim import FusedAdamW
    net = _fresh(_net())
    topt, names, _ = _torch_amsgrad_state(net, steps=1)
    sd = topt.state_dict()
    del sd["state"][names.index("join.0.bias")]["max_exp_avg_sq"]
    opt = FusedAdamW(net, lr=1e-3)
    before = net._layout.exp_avg.clone()
    with pytest.raises(ValueError, match="max_exp_avg_sq"):
        opt.load_state_dict(sd)
    assert opt.amsgrad_flags() == (False,) and torch.equal(net._layout.exp_avg, before)     # refused before anything changed


# ------------------------------------------------------------------------------------------------ data parallel (gloo, two ranks)
def _dp_worker(rank, world, port, out):
    import os
    import torch.distributed as dist
    import torch.nn as nn
    from mmfn_amd.parallel import DataParallel
    from mmfn_amd.params import FlatLayout
    from mmfn_amd.trainer import Trainer, sync_resume_state
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(100 + rank)
    m = nn.Module()
    m.encoder = nn.Module()
    m.encoder.transformer4 = nn.Linear(8, 8)
    m.encoder.layer3 = nn.Conv2d(4, 4, 3, bias=False)
    m.join = nn.Linear(4, 2)
    object.__setattr__(m, "_layout", FlatLayout(m, ()).materialize("cpu"))
    L = m._layout
    if rank == 0:   # what a resume of an amsgrad checkpoint left on rank 0 alone
        L.ensure_max_exp_avg_sq().copy_(torch.arange(L.total, dtype=torch.float32) + 1.0)
    DataParallel(m, dist, max_bucket_bytes=64).broadcast_parameters()
    got = None if L.max_exp_avg_sq is None else L.max_exp_avg_sq.clone()

    class _Opt(object):
        def __init__(self):
            self.param_groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, params=[]),
                                 dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, params=[])]
            self.synced = 0

        def sync_amsgrad(self):
            self.synced += 1

    opt = _Opt()
    if rank == 0:
        opt.param_groups[1]["amsgrad"] = True
    sync_resume_state(Trainer("cpu", None), opt, dist)
    out.put((rank, got, [g["amsgrad"] for g in opt.param_groups], opt.synced))
    dist.barrier()
    dist.destroy_process_group()


def test_broadcast_carries_max_exp_avg_sq_and_the_ranks_agree_on_the_flags_gloo():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((out.get(timeout=120) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, a, fa, sa), (_, b, fb, sb) = res
    assert a is not None and b is not None and torch.equal(a, b) and float(b[3]) == 4.0      # rank 1 allocated it and received it
    assert fa == fb == [False, True] and sa == sb == 1
