"""FusedSGD on a module built on the CPU (no engine): constructor, validation, the torch.optim.SGD state_dict / load_state_dict
layout, sync_resume_state's SGD group keys over two gloo ranks - and the yardstick of tests/test_sgd_gpu.py, torch.optim.SGD itself
on CPU tensors in float64, with the launch tests' inputs checked here: torch's own float32 step stays within 2.7e-7 (p) / 2.4e-7
(buf) of it, and every wrong variant of the rule is separated from it by a median |dp| of at least 1000 bounds."""
import functools

import pytest
import torch

BOUND = 1e-6   # max |d| of p and buf against float64 torch.optim.SGD: the bound of the AdamW parity tests (tests/test_amsgrad_cpu.py)

N4 = 3 * 256 + 1                                  # float4s: three workgroups and one float4 of a fourth
N = 4 * N4
CUTS = (250, 526)                                 # the group byte changes inside a workgroup's range
SPANS = [(0, 4 * CUTS[0]), (4 * CUTS[0], 4 * CUTS[1]), (4 * CUTS[1], N)]
GROUPS = [dict(lr=0.01, momentum=0.9, dampening=0.0, nesterov=True, weight_decay=0.01),
          dict(lr=0.02, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0),
          dict(lr=0.005, momentum=0.8, dampening=0.3, nesterov=False, weight_decay=0.1)]
STEPS = 6


def spans_for(n4, cuts=CUTS):
    return [(0, 4 * cuts[0]), (4 * cuts[0], 4 * cuts[1]), (4 * cuts[1], 4 * n4)]


def launch_inputs(n=N, steps=STEPS):
    """(p0, grads): p0 = rand(seed 5) * 3 - 1.5, `steps` draws of 0.3 * randn from seed 6."""
    p0 = torch.rand(n, generator=torch.Generator().manual_seed(5)) * 3.0 - 1.5
    gen = torch.Generator().manual_seed(6)
    return p0, [0.3 * torch.randn(n, generator=gen) for _ in range(steps)]


def sgd_reference(p, grads, groups, spans, dtype=torch.float64, first_step_dampening=False):
    """torch.optim.SGD itself on CPU tensors of `dtype`, one parameter per group (a group may carry grad_scale: the gradient is
    scaled in `dtype` before the step).  Returns the trajectory: per step a dict of float64 p and buf (buf stays zero where torch
    holds no momentum_buffer).  first_step_dampening: the WRONG rule, for the separation checks - the first step blends
    (1 - dampening) * d into a zero buffer instead of copying d."""
    refs = [torch.nn.Parameter(p[b:e].to(dtype).clone()) for b, e in spans]
    opt = torch.optim.SGD([dict(params=[r], lr=g["lr"], momentum=g["momentum"], dampening=g["dampening"], nesterov=g["nesterov"],
                                weight_decay=g["weight_decay"]) for r, g in zip(refs, groups)])
    if first_step_dampening:
        for r, g in zip(refs, groups):
            if g["momentum"] != 0:
                opt.state[r]["momentum_buffer"] = torch.zeros_like(r)
    out = []
    for g in grads:
        for r, grp, (b, e) in zip(refs, groups, spans):
            r.grad = g[b:e].to(dtype) * grp.get("grad_scale", 1.0)
        opt.step()
        buf = torch.cat([opt.state[r]["momentum_buffer"] if opt.state[r].get("momentum_buffer") is not None else torch.zeros_like(r)
                         for r in refs])
        out.append(dict(p=torch.cat([r.detach() for r in refs]).double().clone(), buf=buf.double().clone()))
    return out


@functools.lru_cache(maxsize=None)
def launch_reference():
    """The float64 trajectory of the launch inputs: computed once, shared, never written to."""
    p0, grads = launch_inputs()
    return sgd_reference(p0, grads, GROUPS, SPANS)


def test_torch_float32_stays_close_to_float64_on_the_launch_inputs():
    p0, grads = launch_inputs()
    ref, f32 = launch_reference(), sgd_reference(p0, grads, GROUPS, SPANS, dtype=torch.float32)
    dp = max((a["p"] - b["p"]).abs().max().item() for a, b in zip(ref, f32))
    db = max((a["buf"] - b["buf"]).abs().max().item() for a, b in zip(ref, f32))
    print("torch float32 against float64: max |dp| %.3g, max |dbuf| %.3g; max |p| %.3g, max |buf| %.3g"
          % (dp, db, max(a["p"].abs().max().item() for a in ref), max(a["buf"].abs().max().item() for a in ref)))
    assert dp < 3e-7 and db < 3e-7        # (2.7e-7 and 2.4e-7 as measured: a third of the bound is torch's own rounding)
    assert BOUND > 2 * max(dp, db)


def test_the_reference_separates_every_wrong_variant():
    """A test that cannot tell the variants apart shows nothing: each wrong rule moves the final p of its group by a median of at
    least 1000 bounds, and leaves the other groups' bits alone."""
    p0, grads = launch_inputs()
    ref = launch_reference()[-1]["p"]

    def median_dp(groups, gi, **kw):
        got = sgd_reference(p0, grads, groups, SPANS, **kw)[-1]["p"]
        for j, (b, e) in enumerate(SPANS):
            if j != gi:
                assert torch.equal(got[b:e], ref[b:e])
        b, e = SPANS[gi]
        return (got[b:e] - ref[b:e]).abs().median().item()

    swap = lambda gi, **kw: [dict(g, **kw) if i == gi else g for i, g in enumerate(GROUPS)]
    figures = {"g0 without nesterov": median_dp(swap(0, nesterov=False), 0),
               "g2 with dampening 0": median_dp(swap(2, dampening=0.0), 2),
               "g2 without decay": median_dp(swap(2, weight_decay=0.0), 2),
               "g0 without decay": median_dp(swap(0, weight_decay=0.0), 0),
               "g1 given momentum": median_dp(swap(1, momentum=0.9), 1),
               "dampening applied on the first step": median_dp(GROUPS, 2, first_step_dampening=True)}
    print(figures)
    for name, d in figures.items():
        assert d >= 1000 * BOUND, (name, d)


# ------------------------------------------------------------------------------------------------ FusedSGD on a CPU module
@functools.lru_cache(maxsize=None)
def _net():
    from mmfn_amd.config import GlobalConfig
    import mmfn_amd.model as M
    return M.MMFN(GlobalConfig(), "cpu")


def _fresh(net):
    """(the module is shared between the tests: every one starts from zero state and zero counts)"""
    L = net._layout
    L.exp_avg.zero_()
    L.exp_avg_sq.zero_()
    L.step_classes.set_steps([0] * len(L.step_classes.names))
    return net


def test_constructor_validation_and_rows():
    from mmfn_amd.optim import FusedSGD, configure_optimizers
    net = _fresh(_net())
    opt = FusedSGD(net, lr=0.1)
    assert opt.defaults == dict(lr=0.1, momentum=0, dampening=0, weight_decay=0, nesterov=False)
    assert opt.hyper_rows() == [(0.1, 0, 0, 0.0, 0)]
    groups = configure_optimizers(net, weight_decay=0.05)
    groups[1]["momentum"] = 0.0
    opt = FusedSGD(net, lr=0.01, momentum=0.9, nesterov=False, dampening=0.1, param_groups=groups)
    assert opt.hyper_rows() == [(0.01, 0.9, 0.1, 0.0, 0.05), (0.01, 0.0, 0.1, 0.0, 0.0)]
    assert FusedSGD(net, lr=0.01, momentum=0.9, nesterov=True).hyper_rows() == [(0.01, 0.9, 0, 1.0, 0)]
    # torch's validation and messages
    with pytest.raises(ValueError, match="Invalid learning rate: -0.1"):
        FusedSGD(net, lr=-0.1)
    with pytest.raises(ValueError, match="Invalid momentum value: -0.5"):
        FusedSGD(net, lr=0.1, momentum=-0.5)
    with pytest.raises(ValueError, match="Invalid weight_decay value: -1"):
        FusedSGD(net, lr=0.1, weight_decay=-1)
    for kw in (dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
            FusedSGD(net, lr=0.1, **kw)
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
        FusedSGD(net, lr=0.1, param_groups=[dict(params=list(net.parameters()), nesterov=True)])
    with pytest.raises(TypeError):
        FusedSGD(net, lr=0.1, maximize=True)
    with pytest.raises(ValueError, match="maximize"):
        FusedSGD(net, lr=0.1, param_groups=[dict(params=list(net.parameters()), maximize=True)])
    # a value assigned to a live group is checked where the rows are read
    opt.param_groups[0]["nesterov"] = True
    with pytest.raises(ValueError, match="Nesterov"):
        opt.hyper_rows()
    with pytest.raises(ValueError, match="at most 16"):
        ps = list(net.parameters())
        FusedSGD(net, lr=0.1, param_groups=[dict(params=[p]) for p in ps[:17]] + [dict(params=ps[17:])])


def _torch_sgd_state(net, steps=2, **kw):
    """A torch.optim.SGD over CPU copies of the model's parameters in configure_optimizers' two groups after `steps` steps on seeded
    gradients; every never-trained parameter keeps grad = None, as in a reference run.  kw: per-group overrides of group 1."""
    from mmfn_amd.optim import configure_optimizers
    L = net._layout
    by_id = {id(p): n for n, p in net.named_parameters()}
    groups = configure_optimizers(net, weight_decay=0.01)
    names = [by_id[id(p)] for g in groups for p in g["params"]]
    copies = [[torch.nn.Parameter(p.detach().clone()) for p in g["params"]] for g in groups]
    opt = torch.optim.SGD([dict(params=copies[0], weight_decay=0.01), dict(dict(params=copies[1], weight_decay=0.0), **kw)],
                          lr=0.01, momentum=0.9, dampening=0.2)
    params = copies[0] + copies[1]
    gen = torch.Generator().manual_seed(3)
    for i in range(steps):
        for n, r in zip(names, params):
            r.grad = None if n in L.unused else torch.randn(r.shape, generator=gen) * (1.0, 0.1)[i % 2]
        opt.step()
    return opt, names, params, groups


def test_state_dict_round_trip_with_torch_in_checkpoint_shape():
    from mmfn_amd.optim import FusedSGD
    net = _fresh(_net())
    L = net._layout
    topt, names, params, groups = _torch_sgd_state(net, momentum=0.0)   # the no-decay group runs without momentum
    sd = topt.state_dict()
    opt = FusedSGD(net, lr=0.5, param_groups=groups)                   # other hyper-parameters here: the checkpoint's groups decide
    opt.load_state_dict(sd)
    assert [(g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]) for g in opt.param_groups] == \
        [(0.01, 0.9, 0.2, 0.01, False), (0.01, 0.0, 0.2, 0.0, False)]
    # one convolution filter element by element: OIHW in the checkpoint, OHWI in the flat buffer
    conv = "encoder.lidar_encoder._model.layer2.0.conv1.weight"
    idx = names.index(conv)
    want = sd["state"][idx]["momentum_buffer"]
    o, i, kh, kw = want.shape
    off, n = L.offsets[conv]
    flat = L.exp_avg[off:off + n].view(o, kh, kw, i)
    assert float(want.abs().max()) > 0
    for (a, b, c, d) in ((0, 0, 0, 0), (3, 5, 1, 2), (o - 1, i - 1, kh - 1, kw - 1), (7, 2, 2, 0)):
        assert flat[a, c, d, b].item() == want[a, b, c, d].item()
    # an entry is count 1 (torch's SGD stores no step: only "has stepped" matters); no entry - a never-trained tensor, every tensor
    # of the momentum-0 group - is count 0 and a zero buffer
    steps = opt.tensor_steps()
    assert steps[conv] == 1 and steps["join.0.bias"] == 0
    off, n = L.offsets["join.0.bias"]
    assert not bool(L.exp_avg[off:off + n].any()) and not bool(L.exp_avg_sq.any())
    # back out: exactly torch's keys, entries for the same ids (none in the momentum-0 group), and torch loads it
    out = opt.state_dict()
    assert set(out["state"]) == {k for k, st in sd["state"].items() if st.get("momentum_buffer") is not None}
    n0 = len(groups[0]["params"])
    assert out["state"] and all(k < n0 for k in out["state"]) and all(set(st) == {"momentum_buffer"} for st in out["state"].values())
    for mine, theirs in zip(out["param_groups"], sd["param_groups"]):
        assert set(mine) == {"lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize", "foreach", "differentiable",
                             "fused", "params"}
        assert mine["params"] == theirs["params"] and mine["maximize"] is False and mine["foreach"] is None
        assert mine["differentiable"] is False and mine["fused"] is None
    fresh = torch.optim.SGD([dict(params=params[:n0]), dict(params=params[n0:])], lr=0.3)
    fresh.load_state_dict(out)
    assert fresh.state[params[idx]]["momentum_buffer"].shape == params[idx].shape
    assert torch.equal(fresh.state[params[idx]]["momentum_buffer"], want)
    assert fresh.param_groups[0]["momentum"] == 0.9 and fresh.param_groups[1]["momentum"] == 0.0


def test_refusals_maximize_stepped_state_and_foreign_checkpoints():
    from mmfn_amd.optim import FusedAdamW, FusedSGD
    net = _fresh(_net())
    L = net._layout
    topt, names, params, groups = _torch_sgd_state(net, steps=1)
    sd = topt.state_dict()
    opt = FusedSGD(net, lr=0.1, param_groups=groups)
    before = L.exp_avg.clone()
    sd["param_groups"][1]["maximize"] = True
    with pytest.raises(ValueError, match="maximize"):
        opt.load_state_dict(sd)
    assert torch.equal(L.exp_avg, before) and opt.param_groups[0]["lr"] == 0.1     # refused before anything changed
    with pytest.raises(ValueError, match="momentum"):                              # an AdamW checkpoint is not an SGD one
        FusedSGD(net, lr=0.1).load_state_dict(FusedAdamW(net, lr=1e-3).state_dict())
    # handing over from AdamW: the tensors have stepped and exp_avg holds a first moment
    L.step_classes.set_steps([3] * len(L.step_classes.names))
    L.exp_avg.fill_(0.25)
    L.exp_avg_sq.fill_(0.5)
    with pytest.raises(RuntimeError, match="reset_state=True"):
        FusedSGD(net, lr=0.1, momentum=0.9)
    assert bool((L.exp_avg == 0.25).all())
    opt = FusedSGD(net, lr=0.1, momentum=0.9, reset_state=True)
    assert not bool(L.exp_avg.any()) and not bool(L.exp_avg_sq.any()) and set(opt.tensor_steps().values()) == {0}
    assert opt.state_dict()["state"] == {}


# ------------------------------------------------------------------------------------------------ data parallel (gloo, two ranks)
def _dp_worker(rank, world, port, out):
    import os
    import torch.distributed as dist
    from mmfn_amd.trainer import Trainer, sync_resume_state
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    class _Opt(object):
        def __init__(self):
            self.param_groups = [dict(lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, params=[]),
                                 dict(lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, params=[])]

    opt = _Opt()
    if rank == 0:   # what a resume left on rank 0 alone
        opt.param_groups[0].update(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
        opt.param_groups[1].update(lr=0.02, momentum=0.8, dampening=0.3)
    sync_resume_state(Trainer("cpu", None), opt, dist)
    mixed = None
    if rank == 1:   # a rank that holds the other optimizer's groups is told so
        opt.param_groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, params=[]) for _ in range(2)]
    try:
        sync_resume_state(Trainer("cpu", None), opt, dist)
    except ValueError as exc:
        mixed = str(exc)
    out.put((rank, [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups], mixed))
    dist.barrier()
    dist.destroy_process_group()


def test_sync_resume_state_carries_the_sgd_group_keys_gloo():
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
    (_, a, ma), (_, b, mb) = res
    want = [dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=True),
            dict(lr=0.02, momentum=0.8, dampening=0.3, weight_decay=0.0, nesterov=False)]
    assert a == want and ma is None
    assert mb is not None and "AdamW" in mb and "betas" in b[0]      # rank 1's AdamW groups were refused, not overwritten
