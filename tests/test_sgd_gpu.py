"""Momentum SGD on the fused step: mmfn_sgd_groups_f32 / mmfn_sgd_rows_f32 against torch.optim.SGD and, bit for bit, among their own
instances; then the engine, captured steps, frozen tensors, the guard, an attached average, FusedSGD's state dict and the trainer.

Yardstick: torch.optim.SGD on CPU tensors in float64 (tests/test_sgd_cpu.py holds the helpers, the launch inputs and the checks
that these inputs separate every wrong variant of the rule by >= 1000 bounds).  Bound: max |d| < 1e-6 for p and buf, the bound of the
AdamW parity tests.  Against float64 the deviation is the kernel's own rounding: per step p takes one rounding (p - lr * u is one
fma), half an ulp of |p| < 2, 6e-8, so 3.6e-7 over six steps; buf takes two (momentum * buf, then the fma with (1 - dampening) * d)
at half an ulp of |buf| < 4, 2.4e-7 at worst per step but shrinking by `momentum` each step; torch's own float32 SGD sits at
2.7e-7 / 2.4e-7 on the same inputs.  Measured on an MI355X, max |d| for p / buf: small case, six steps, 2.64e-07 / 2.35e-07; large
case, three steps, 1.78e-07 / 2.58e-07.  The model tests feed the engine's own gradients, under which elements of the momentum
buffers grow to 27 (51 in the bf16 mode) in four steps: p is held to 1e-6 there too (measured 2.2e-7), buf to the larger of 1e-6 and
1.5 * ulp(max |buf| of the float64 twin) * steps, derived in _errors() below (measured 3.1e-6 at max |buf| 27.3, 1.6 ulp).  Each
comparison prints an `sgd-err` line; profiles/sgd_bench.txt holds them."""
import functools
import math
import os
import pickle
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_sgd_cpu as R   # noqa: E402  (the float64 yardstick, the launch inputs, the three groups, the bound)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = R.BOUND
SENTINEL = 123.0
N4_SMALL = R.N4


def _big_n4():
    from mmfn_amd import ops
    return ops.adamw_max_blocks() * 256 + 37   # past what the capped grid covers in one trip: the grid-stride loop goes round


def _cuts(n4):
    return R.CUTS if n4 == N4_SMALL else (300001, n4 - 50)     # (the last group sits in the second trip)


def _spans(n4):
    return R.spans_for(n4, _cuts(n4))


def _group_of(n4):
    a, b = _cuts(n4)
    t = torch.zeros(n4, dtype=torch.uint8)
    t[a:b], t[b:] = 1, 2
    return t.to(DEV)


def _hyper(groups, grad_scale=1.0):
    h = torch.zeros(16, 8)
    for i, g in enumerate(groups):
        h[i] = torch.tensor([g["lr"], g["momentum"], g["dampening"], float(g["nesterov"]), g["weight_decay"], grad_scale, 0.0, 0.0])
    return h.to(DEV)


def _step(t):
    return torch.tensor([t], dtype=torch.int64, device=DEV)


def _elements(n4, groups):
    m = torch.zeros(4 * n4, dtype=torch.bool)
    for gi in groups:
        b, e = _spans(n4)[gi]
        m[b:e] = True
    return m.to(DEV)


# ------------------------------------------------------------------------------------------------ 1. against torch
@pytest.mark.parametrize("size", ["small", "past_one_grid_trip"])
def test_grouped_launch_matches_torch_sgd(size):
    """Nesterov + decay, momentum 0, dampening + decay in one launch, from the first step (buf = d) on; the momentum-0 group's range
    of buf holds a sentinel and keeps its bits."""
    from mmfn_amd import ops
    n4 = N4_SMALL if size == "small" else _big_n4()
    n, spans = 4 * n4, _spans(n4)
    steps = R.STEPS if size == "small" else 3                  # (the large case is about the second grid trip, not the sequence)
    if size == "small":
        (p0, grads), ref = R.launch_inputs(), R.launch_reference()
    else:
        p0, grads = R.launch_inputs(n, steps)
        ref = R.sgd_reference(p0, grads, R.GROUPS, spans)
    hyper, group_of = _hyper(R.GROUPS), _group_of(n4)
    off = _elements(n4, (1,))
    p, buf = p0.to(DEV), torch.zeros(n, device=DEV)
    buf[off] = SENTINEL
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    worst = dict(p=0.0, buf=0.0)
    for t, g in enumerate(grads):
        ops.step_advance(step)
        ops.sgd_groups(p, g.to(DEV), buf, step, hyper, 3, group_of=group_of)
        assert bool((buf[off] == SENTINEL).all())
        got = buf.clone()
        got[off] = 0.0
        e = dict(p=(p.cpu().double() - ref[t]["p"]).abs().max().item(), buf=(got.cpu().double() - ref[t]["buf"]).abs().max().item())
        worst = {k: max(worst[k], e[k]) for k in worst}
        assert e["p"] < BOUND and e["buf"] < BOUND, (t, e)
    print("sgd-err %s n=%d steps=%d: max |d| vs torch float64  p %.3g  buf %.3g" % (size, n, steps, worst["p"], worst["buf"]))


# ------------------------------------------------------------------------------------------------ 2. the instances, bit for bit
def _case(n4=N4_SMALL, seed=0):
    """Three buffers mid-run and an average beside them."""
    n = 4 * n4
    gen = torch.Generator(device=DEV).manual_seed(2000 + seed + n4)
    mk = lambda: torch.randn(n, device=DEV, generator=gen)
    return dict(p=mk(), g=mk() * 0.3, b=mk() * 0.5, a=mk())


def _clone(b):
    return {k: t.clone() for k, t in b.items()}


def _run(b, hyper, n4=N4_SMALL, t=5, coef=None, avg=None, ok=None, mask=None):
    from mmfn_amd import ops
    table = _group_of(n4) if mask is None else mask
    ops.sgd_groups(b["p"], b["g"], b["b"], _step(t), hyper, 3, group_of=table, coef=coef,
                   avg=None if avg is None else (b["a"],) + avg, ok=ok, mask=mask is not None)
    torch.cuda.synchronize()
    return b


def _same(a, b, keys="pgba", where=None):
    for k in keys:
        x, y = (a[k], b[k]) if where is None else (a[k][where], b[k][where])
        assert torch.equal(x, y), k


@pytest.mark.parametrize("t", [1, 5])
def test_mask_with_nothing_frozen_and_rows_with_one_class_per_group_are_the_grouped_launch(t):
    from mmfn_amd import ops
    base = _case()
    hyper = _hyper(R.GROUPS)
    want = _run(_clone(base), hyper, t=t)
    assert not torch.equal(want["p"], base["p"]) and not torch.equal(want["b"], base["b"])
    _same(_run(_clone(base), hyper, t=t, mask=_group_of(N4_SMALL)), want)
    got = _clone(base)
    rows = torch.tensor([[0, 0], [1, 1], [2, 2]], dtype=torch.int32)
    ops.sgd_rows(got["p"], got["g"], got["b"], torch.full((3,), t, dtype=torch.int64, device=DEV), 3, hyper, 3, _group_of(N4_SMALL), rows)
    torch.cuda.synchronize()
    _same(got, want)
    # the momentum-0 group's buffer is never written, whatever the count
    off = _elements(N4_SMALL, (1,))
    assert torch.equal(want["b"][off], base["b"][off])


def test_coef_is_grad_scale():
    base = _case()
    half = torch.tensor([0.5], device=DEV)
    _same(_run(_clone(base), _hyper(R.GROUPS, 0.8), coef=half), _run(_clone(base), _hyper(R.GROUPS, 0.4)))
    assert not torch.equal(_run(_clone(base), _hyper(R.GROUPS, 0.8))["p"], _run(_clone(base), _hyper(R.GROUPS, 0.4))["p"])


@pytest.mark.parametrize("mode,count", [("ema", 2), ("swa", 0), ("swa", 3)])
def test_avg_instance_has_the_bits_without_avg_and_the_average_of_a_pass_afterwards(mode, count):
    from mmfn_amd import ops
    base = _case()
    hyper = _hyper(R.GROUPS)
    cnt, w = torch.tensor([count], dtype=torch.int64, device=DEV), torch.tensor([0.1], device=DEV)
    code = ops.AVG_EMA if mode == "ema" else ops.AVG_SWA
    got = _run(_clone(base), hyper, avg=(cnt, w, code))
    want = _run(_clone(base), hyper)
    ops.weight_average(want["a"], want["p"], cnt, w, code)      # (ATen's lerp of the new p; count 0: the first update copies)
    torch.cuda.synchronize()
    _same(got, want)
    assert not torch.equal(got["a"], base["a"])
    if count == 0:
        assert torch.equal(got["a"], got["p"])


@pytest.mark.parametrize("with_avg", [False, True])
def test_guard_flag(with_avg):
    from mmfn_amd import ops
    base = _case()
    hyper = _hyper(R.GROUPS)
    coef = torch.tensor([0.37], device=DEV)
    avg = (torch.tensor([2], dtype=torch.int64, device=DEV), torch.tensor([0.1], device=DEV), ops.AVG_EMA) if with_avg else None
    ok0, ok1 = (torch.full((1,), x, dtype=torch.int32, device=DEV) for x in (0, 1))
    _same(_run(_clone(base), hyper, coef=coef, avg=avg, ok=ok0), base)                     # skipped: p, buf and the average
    _same(_run(_clone(base), hyper, coef=coef, avg=avg, ok=ok1), _run(_clone(base), hyper, coef=coef, avg=avg))


@pytest.mark.parametrize("with_avg", [False, True])
def test_masked_float4s_keep_p_and_buf_and_the_average_follows_frozen_p(with_avg):
    from mmfn_amd import ops
    base = _case()
    hyper = _hyper(R.GROUPS)
    avg = (torch.tensor([2], dtype=torch.int64, device=DEV), torch.tensor([0.1], device=DEV), ops.AVG_EMA) if with_avg else None
    table = _group_of(N4_SMALL)
    cold4 = torch.zeros(N4_SMALL, dtype=torch.bool, device=DEV)
    cold4[100:300] = True          # across the first group boundary, starting and ending inside workgroups
    cold4[600:] = True
    table[cold4] = ops.ADAMW_FROZEN
    cold = cold4.repeat_interleave(4)
    base["p"][cold] = SENTINEL
    base["b"][cold] = float("nan")   # a frozen float4 is neither loaded nor stored (NaN would spread through any arithmetic)
    base["g"][cold] = float("nan")
    got = _run(_clone(base), hyper, avg=avg, mask=table)
    free = _clone(base)
    for k in "pbg":
        free[k][cold] = 1.0
    want = _run(free, hyper, avg=avg)
    _same(got, want, "pb", ~cold)
    assert bool(torch.isnan(got["b"][cold]).all()) and bool((got["p"][cold] == SENTINEL).all())
    if with_avg:
        _same(got, want, "a", ~cold)
        ref = base["a"].clone()
        ops.weight_average(ref, base["p"], avg[0], avg[1], avg[2])
        torch.cuda.synchronize()
        assert torch.equal(got["a"][cold], ref[cold])
    else:
        _same(got, base, "a")


# ------------------------------------------------------------------------------------------------ 3. the first-step rule per class
def test_first_step_copies_d_for_the_class_at_count_one_and_blends_for_the_other():
    """One rows launch, one group (momentum 0.8, dampening 0.3, decay 1/8: g + p / 8 is then a single rounding in float32 however
    it is evaluated), two classes at counts 1 and 3 and a frozen tail."""
    from mmfn_amd import ops
    n4 = N4_SMALL
    base = _case(n4, seed=2)
    grp = dict(lr=0.005, momentum=0.8, dampening=0.3, nesterov=False, weight_decay=0.125)
    hyper = _hyper([grp])
    row_of = torch.full((n4,), ops.ADAMW_FROZEN, dtype=torch.uint8)
    row_of[:300], row_of[300:700] = 0, 1
    first = torch.zeros(4 * n4, dtype=torch.bool, device=DEV)
    first[:1200] = True
    later = torch.zeros_like(first)
    later[1200:2800] = True
    got = _clone(base)
    ops.sgd_rows(got["p"], got["g"], got["b"], torch.tensor([1, 3], dtype=torch.int64, device=DEV), 2, hyper, 1, row_of.to(DEV),
                 torch.tensor([[0, 0], [0, 1]], dtype=torch.int32))
    torch.cuda.synchronize()
    d = base["g"] + 0.125 * base["p"]
    assert torch.equal(got["b"][first], d[first])                           # copied: no dampening, the old buffer is not read
    assert (got["p"][first].double() - (base["p"].double() - 0.005 * d.double())[first]).abs().max().item() < BOUND
    want = 0.8 * base["b"].double() + (1.0 - 0.3) * d.double()
    assert (got["b"][later].double() - want[later]).abs().max().item() < BOUND
    assert (got["b"][later] - d[later]).abs().median().item() > 1000 * BOUND
    assert (got["p"][later].double() - (base["p"].double() - 0.005 * want)[later]).abs().max().item() < BOUND
    cold = ~(first | later)
    _same(got, base, "pb", cold)


# ------------------------------------------------------------------------------------------------ 4. argument checks
def test_entry_points_refuse_what_they_would_dereference():
    from mmfn_amd import ops
    from mmfn_amd._lib import lib
    n4 = N4_SMALL
    base = _case(n4)
    b = _clone(base)
    hyper, table = _hyper(R.GROUPS), _group_of(n4)
    step, s = _step(3), torch.cuda.current_stream().cuda_stream
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    P = lambda t: t.data_ptr()

    def groups(**kw):
        a = dict(p=P(b["p"]), g=P(b["g"]), b=P(b["b"]), n=4 * n4, table=P(table), hyper=P(hyper), n_groups=3, step=P(step), variant=0,
                 coef=None, ok=None)
        a.update(kw)
        return lib().mmfn_sgd_groups_f32(a["p"], a["g"], a["b"], a["n"], a["table"], a["hyper"], a["n_groups"], a["step"], a["variant"],
                                         a["coef"], None, None, None, 0, a["ok"], s)
    for bad in (dict(variant=ops.ADAMW_COEF), dict(variant=ops.ADAMW_COEF | ops.ADAMW_GUARD, coef=P(hyper)),
                dict(variant=ops.ADAMW_COEF | ops.ADAMW_GUARD, ok=P(flag)), dict(variant=ops.ADAMW_MASK, table=None),
                dict(n=4 * n4 - 2), dict(n_groups=17), dict(n_groups=0), dict(b=None), dict(b=P(b["b"]) + 4), dict(p=None), dict(g=None),
                dict(hyper=None), dict(step=None), dict(variant=ops.ADAMW_GUARD), dict(variant=ops.ADAMW_AVG), dict(variant=16),
                dict(variant=-1)):
        assert groups(**bad) == -1, bad
    rows = torch.tensor([[0, 0], [1, 0], [2, 1]], dtype=torch.int32)
    cs = torch.ones(2, dtype=torch.int64, device=DEV)

    def rowsf(**kw):
        a = dict(p=P(b["p"]), g=P(b["g"]), b=P(b["b"]), n=4 * n4, table=P(table), hyper=P(hyper), n_groups=3, rows=rows.data_ptr(),
                 n_rows=3, cs=P(cs), n_classes=2, variant=0, coef=None, ok=None)
        a.update(kw)
        return lib().mmfn_sgd_rows_f32(a["p"], a["g"], a["b"], a["n"], a["table"], a["hyper"], a["n_groups"], a["rows"], a["n_rows"],
                                       a["cs"], a["n_classes"], a["variant"], a["coef"], None, None, None, 0, a["ok"], s)
    for bad in (dict(variant=ops.ADAMW_COEF), dict(variant=ops.ADAMW_COEF | ops.ADAMW_GUARD, coef=P(hyper)), dict(table=None),
                dict(n=4 * n4 - 2), dict(n_groups=17), dict(b=None), dict(p=None), dict(rows=None), dict(cs=None), dict(n_rows=0),
                dict(n_rows=255), dict(n_classes=1), dict(n_groups=2), dict(variant=4), dict(variant=8)):
        assert rowsf(**bad) == -1, bad
    # ... and through ops they surface as the library's error or a ValueError, before anything is launched
    with pytest.raises(Exception, match="mmfn_sgd_groups_f32"):
        ops.sgd_groups(b["p"], b["g"], b["b"], step, hyper, 17, group_of=table)
    with pytest.raises(ValueError, match="momentum_buffer"):
        ops.sgd_groups(b["p"], b["g"], b["b"][:100], step, hyper, 3, group_of=table)
    with pytest.raises(ValueError, match="coefficient instance"):
        ops.sgd_groups(b["p"], b["g"], b["b"], step, hyper, 3, group_of=table, ok=flag)
    with pytest.raises(ValueError, match="group table"):
        ops.sgd_groups(b["p"], b["g"], b["b"], step, hyper, 3, mask=True)
    torch.cuda.synchronize()
    _same(b, base)                                                  # no refused call launched anything


# ------------------------------------------------------------------------------------------------ engine helpers
@functools.lru_cache(maxsize=None)
def _weights():
    from oracle import harness
    return harness.build_oracle("vec", dropout=0.0).state_dict()


def _net(**cfg):
    from mmfn_amd.config import GlobalConfig
    import mmfn_amd.model as M
    net = M.MMFN(GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0, **cfg), DEV)
    net.load_state_dict(_weights(), strict=True)
    net.train()
    return net


@functools.lru_cache(maxsize=None)
def _inputs():
    sys.path.insert(0, ROOT)
    import bench
    return bench.synth_inputs(2, torch.device(DEV), seed=42, variant="vec")


def _sgd(net, **kw):
    """FusedSGD over configure_optimizers' two groups: nesterov + decay on the weights, dampening without decay on the rest."""
    from mmfn_amd.optim import FusedSGD, configure_optimizers
    groups = configure_optimizers(net, weight_decay=0.01)
    groups[0].update(lr=1e-3, momentum=0.9, nesterov=True)
    groups[1].update(lr=2e-3, momentum=0.8, dampening=0.3)
    return FusedSGD(net, lr=1e-3, param_groups=groups, **kw)


def _twin(net, opt):
    """torch.optim.SGD in float64 over CPU copies of the parameters, in the optimizer's groups and order; (twin, names, params)."""
    named = dict(net.named_parameters())
    copies = [[torch.nn.Parameter(named[n].detach().cpu().double().clone()) for n in names] for names in opt._group_names]
    twin = torch.optim.SGD([dict(params=c, **{k: g[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov")})
                            for c, g in zip(copies, opt.param_groups)])
    return twin, [n for names in opt._group_names for n in names], [r for c in copies for r in c]


def _feed(net, names, params, scale=1.0):
    """The engine's own flat gradient, as the last backward (and fold) left it, times `scale`, into the twin's parameters."""
    L, frozen = net._layout, net._engine_for().frozen
    for n, r in zip(names, params):
        r.grad = None if n in L.unused or n in frozen else L.grad_views[n].detach().cpu().double() * scale


def _errors(net, opt, twin, names, params, steps=1):
    """(max |d| of p, max |d| of the momentum buffers, the bound for the latter) against the twin after `steps` steps.

    p is held to BOUND.  The model's real gradients are not the launch tests' 0.3 * randn: at these rates the largest element of the
    momentum buffers is 2.1, 5.5, 24.5, 27.3 after steps 1 .. 4 (51 in the bf16 mode), where one float32 ulp is 1.9e-6 .. 3.8e-6
    and BOUND is below a single rounding (measured there: buf 9.1e-8, 2.6e-7, 1.6e-6, 3.1e-6; p 2.2e-7 after four steps).  Per step
    buf takes three roundings - d = g + wd * p, momentum * buf, and the fma that adds (1 - dampening) * d - each at most half an
    ulp of the largest |buf|, and what earlier steps left is carried over times momentum < 1: at most 1.5 * ulp(max |buf|) * steps,
    with max |buf| read from the float64 twin, never from the kernel.  The bound is that figure where it exceeds BOUND."""
    torch.cuda.synchronize()
    got = dict(net.named_parameters())
    dp = max((got[n].detach().cpu().double() - r.detach()).abs().max().item() for n, r in zip(names, params))
    sd = opt.state_dict()["state"]
    db, top = 0.0, 0.0
    for idx, r in enumerate(params):
        buf = twin.state[r].get("momentum_buffer") if r in twin.state else None
        assert (idx in sd) == (buf is not None), names[idx]
        if buf is not None:
            db = max(db, (sd[idx]["momentum_buffer"].cpu().double() - buf).abs().max().item())
            top = max(top, buf.abs().max().item())
    ulp = 2.0 ** (math.floor(math.log2(top)) - 23) if top > 0 else 0.0
    return dp, db, max(BOUND, 1.5 * ulp * steps)


def _bits(net):
    L, eng = net._layout, net._engine_for()
    torch.cuda.synchronize()
    return [t.clone() for t in (L.params, L.exp_avg, L.buffers_flat, L.counters_flat, eng.step_count, eng.rng_state)]


TRUNK = "encoder.lidar_encoder."


# ------------------------------------------------------------------------------------------------ 5. model steps against torch
@pytest.mark.parametrize("mode", ["plain", "clipped", "accumulated", "bf16"])
def test_train_steps_match_torch_sgd_on_the_engines_own_gradients(mode):
    inp, gt = _inputs()
    net = _net(**(dict(act_dtype="bf16") if mode == "bf16" else {}))
    opt = _sgd(net)
    eng = net._engine_for()
    assert eng.opt_kind == "sgd"
    twin, names, params = _twin(net, opt)
    worst = [0.0, 0.0]
    for i in range(4):
        if mode == "accumulated":
            eng.accumulate_step(inp, gt)
        eng.train_step(inp, gt, lr=1e-3, clip_grad_norm=1.0 if mode == "clipped" else None, groups=opt.hyper_rows())
        _feed(net, names, params, 0.5 if mode == "accumulated" else 1.0)
        if mode == "clipped":
            norm = torch.nn.utils.clip_grad_norm_([r for r in params if r.grad is not None], 1.0)
            assert abs(float(eng.last_grad_norm.item()) - float(norm)) <= 1e-5 * float(norm)
        twin.step()
        dp, db, bound = _errors(net, opt, twin, names, params, steps=i + 1)
        worst = [max(worst[0], dp), max(worst[1], db)]
        top = max(twin.state[r]["momentum_buffer"].abs().max().item() for r in params if r in twin.state)
        print("sgd-err model %s step %d: max |d| vs torch float64  p %.3g  buf %.3g (max |buf| %.3g, bound for buf %.3g)"
              % (mode, i + 1, dp, db, top, bound))
        assert dp < BOUND and db < bound, (i, dp, db, bound)
    print("sgd-err model %s: max |d| vs torch float64 over 4 steps  p %.3g  buf %.3g" % (mode, worst[0], worst[1]))
    assert set(opt.tensor_steps().values()) == {4}
    if mode == "bf16":
        assert eng.act_dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------------ 6. capture and replay
@pytest.mark.parametrize("shape", ["step", "final_clipped_averaged"])
def test_replayed_sgd_steps_have_the_bits_of_eager_ones(shape):
    from mmfn_amd.averaging import AveragedMMFN
    from mmfn_amd.parallel import GraphedStep
    inp, gt = _inputs()
    eager, graphed = _net(), _net()
    opts = [_sgd(eager), _sgd(graphed)]
    full = shape != "step"
    avgs = []
    for net in (eager, graphed):
        if full:
            avgs.append(AveragedMMFN(net, "ema", decay=0.9))
            net.attach_average(avgs[-1])
    kw = dict(variant="final", fold=False, clip_grad_norm=0.5) if full else {}
    step = GraphedStep(graphed._engine_for(), None, inp, gt, lr=1e-3, warm=1, groups=opts[1].hyper_rows(), **kw)   # 1 eager + capture
    for _ in range(3):
        step()
    for _ in range(4):
        eager._engine_for().train_step(inp, gt, lr=1e-3, clip_grad_norm=0.5 if full else None, groups=opts[0].hyper_rows())
    for a, b in zip(_bits(eager), _bits(graphed)):
        assert torch.equal(a, b)
    assert bool(eager._layout.exp_avg.any()) and set(opts[1].tensor_steps().values()) == {4}
    if full:
        assert torch.equal(avgs[0].module._layout.params, avgs[1].module._layout.params) and int(avgs[1].n_averaged.item()) == 4


def test_kind_changes_refuse_the_replay_and_each_optimizer_claims_its_kind():
    from mmfn_amd.optim import FusedAdamW, FusedSGD
    from mmfn_amd.parallel import GraphedStep
    inp, gt = _inputs()
    net = _net()
    eng, L = net._engine_for(), net._layout
    sgd = _sgd(net)
    step = GraphedStep(eng, None, inp, gt, lr=1e-3, warm=1, groups=sgd.hyper_rows())
    step()
    torch.cuda.synchronize()
    assert set(sgd.tensor_steps().values()) == {2}
    with pytest.raises(ValueError, match="one of"):
        eng.set_optimizer("adam")
    adam = FusedAdamW(net, lr=1e-4)                   # a second optimizer on the same model claims the kind ...
    assert eng.opt_kind == "adamw"
    before = _bits(net)
    with pytest.raises(RuntimeError, match="captured with the sgd launch"):
        step()                                        # ... and the captured SGD step refuses to run under it
    for a, b in zip(before, _bits(net)):
        assert torch.equal(a, b)
    sgd.hyper_rows()                                  # the stale one claims the kind back where it hands over its rows
    assert eng.opt_kind == "sgd"
    step()
    adam.hyper_rows()
    assert eng.opt_kind == "adamw"
    # amsgrad and SGD exclude each other
    with pytest.raises(ValueError, match="amsgrad"):
        eng.set_amsgrad((True,))
        eng.set_optimizer("sgd")
    eng.set_amsgrad(())
    eng.set_optimizer("sgd")
    with pytest.raises(ValueError, match="amsgrad"):
        eng.set_amsgrad((True,))
    # not while micro-steps are pending
    eng.accumulate_step(inp, gt)
    with pytest.raises(RuntimeError, match="pending"):
        eng.set_optimizer("adamw")
    eng.discard_accumulated()
    # handing over: the tensors have stepped, exp_avg holds another rule's state
    eng.set_optimizer("adamw")
    with pytest.raises(RuntimeError, match="reset_state=True"):
        FusedSGD(net, lr=1e-3, momentum=0.9)
    assert eng.opt_kind == "adamw"
    L.exp_avg_sq.fill_(1.0)
    fresh = _sgd(net, reset_state=True)
    assert eng.opt_kind == "sgd" and set(fresh.tensor_steps().values()) == {0} and int(eng.step_count.item()) == 0
    assert not bool(L.exp_avg.any()) and not bool(L.exp_avg_sq.any())
    # ... and the first SGD step copies: against a twin that starts without buffers
    twin, names, params = _twin(net, fresh)
    eng.train_step(inp, gt, lr=1e-3, groups=fresh.hyper_rows())
    _feed(net, names, params)
    twin.step()
    dp, db, bound = _errors(net, fresh, twin, names, params)
    assert dp < BOUND and db < bound, (dp, db, bound)


# ------------------------------------------------------------------------------------------------ 7. frozen tensors, the guard, an average
def test_tensor_unfrozen_late_starts_with_buf_equal_d():
    from mmfn_amd import ops
    inp, gt = _inputs()
    net = _net()
    opt = _sgd(net)
    eng, L = net._engine_for(), net._layout
    trunk = torch.zeros(L.total, dtype=torch.bool, device=DEV)
    for n in L.offsets:
        if n.startswith(TRUNK):
            b, e = L.span(n)
            trunk[b:e] = True
    net.freeze(TRUNK)
    p_before = L.params[trunk].clone()
    for _ in range(2):
        eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    torch.cuda.synchronize()
    assert not bool(L.exp_avg[trunk].any()) and torch.equal(L.params[trunk], p_before) and bool(L.exp_avg[~trunk].any())
    net.unfreeze(TRUNK)
    eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    torch.cuda.synchronize()
    steps = opt.tensor_steps()
    assert all(t == (1 if n.startswith(TRUNK) else 3) for n, t in steps.items())
    # the trunk's first step: the grouped launch with *step = 1 on copies, whose buffer is d = g + wd * p itself
    ref_p, ref_b = torch.zeros(L.total, device=DEV), torch.full((L.total,), SENTINEL, device=DEV)
    ref_p[trunk] = p_before
    d = L.grads.double() + 0.01 * ref_p.double()
    ops.sgd_groups(ref_p, L.grads, ref_b, _step(1), eng.opt_hyper, 2, group_of=eng.opt_group_of, n=L.tail)
    torch.cuda.synchronize()
    assert torch.equal(L.exp_avg[trunk], ref_b[trunk]) and torch.equal(L.params[trunk], ref_p[trunk])
    decay = torch.zeros(L.total, dtype=torch.bool, device=DEV)
    for n in opt._group_names[0]:
        b, e = L.span(n)
        decay[b:e] = True
    assert (L.exp_avg[trunk & decay].double() - d[trunk & decay]).abs().max().item() < 1e-7
    assert torch.equal(L.exp_avg[trunk & ~decay], L.grads[trunk & ~decay])      # no decay: d is the gradient, dampening not applied
    # the others blended: a third step is not a copy of d
    rest = ~trunk & decay
    rest[L.tail:] = False
    assert (L.exp_avg[rest] - L.grads[rest]).abs().max().item() > 1e-4


def test_guard_skips_a_nan_step_and_the_next_one_is_still_first(monkeypatch):
    from mmfn_amd.averaging import AveragedMMFN
    inp, gt = _inputs()
    net = _net()
    opt = _sgd(net)
    eng, L = net._engine_for(), net._layout
    eng.set_nonfinite_guard(True)
    avg = AveragedMMFN(net, "ema", decay=0.9)
    net.attach_average(avg)
    A = avg.module._layout.params
    name = "join.0.bias"
    off, _ = L.offsets[name]
    bad_key = (L.stage_of(name), L.GROUPS[L.group_of(name)])
    real = eng.backward
    poison = [True]

    def backward(on_ready=None):
        def hook(key):
            if key == bad_key and poison[0]:
                L.grads[off] = float("nan")
            if on_ready is not None:
                on_ready(key)
        return real(on_ready=hook)

    monkeypatch.setattr(eng, "backward", backward)
    torch.cuda.synchronize()
    before = [t.clone() for t in (L.params, L.exp_avg, eng.step_count, A, avg.n_averaged)]
    eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    torch.cuda.synchronize()
    assert int(eng.skipped_steps.item()) == 1
    for a, b in zip(before, (L.params, L.exp_avg, eng.step_count, A, avg.n_averaged)):
        assert torch.equal(a, b)
    assert set(opt.tensor_steps().values()) == {0} and opt.state_dict()["state"] == {}
    # the next finite step is still the first: buf = d, against a twin without buffers; the average follows
    poison[0] = False
    twin, names, params = _twin(net, opt)
    eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    _feed(net, names, params)
    twin.step()
    dp, db, bound = _errors(net, opt, twin, names, params)
    assert dp < BOUND and db < bound, (dp, db, bound)
    assert set(opt.tensor_steps().values()) == {1} and int(eng.skipped_steps.item()) == 1
    assert int(avg.n_averaged.item()) == 1 and torch.equal(A[:L.tail], L.params[:L.tail])     # the first update copies
    first = A[:L.tail].clone()
    eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    torch.cuda.synchronize()
    assert int(avg.n_averaged.item()) == 2
    want = first.double() + float(avg.ema_weight.item()) * (L.params[:L.tail].double() - first.double())      # the EMA's lerp
    assert (A[:L.tail].double() - want).abs().max().item() < BOUND and not torch.equal(A[:L.tail], first)


# ------------------------------------------------------------------------------------------------ 8. checkpoints and the trainer
def test_state_dict_goes_to_torch_and_a_torch_state_dict_comes_back():
    from mmfn_amd.optim import FusedSGD, configure_optimizers
    inp, gt = _inputs()
    net = _net()
    groups = configure_optimizers(net, weight_decay=0.01)
    groups[0].update(lr=1e-3, momentum=0.9, nesterov=True)
    groups[1].update(lr=2e-3, momentum=0.0)                       # a momentum-0 group: no entries
    opt = FusedSGD(net, lr=1e-3, param_groups=groups)
    eng, L = net._engine_for(), net._layout
    for _ in range(2):
        eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    sd = opt.state_dict()
    n0 = len(opt._group_names[0])
    assert sd["state"] and all(k < n0 for k in sd["state"]) and all(set(st) == {"momentum_buffer"} for st in sd["state"].values())
    assert not any(n in L.unused for k, n in enumerate(opt._group_names[0]) if k in sd["state"])
    # into a real torch.optim.SGD over CPU copies, float64: one further step agrees at the bound
    named = dict(net.named_parameters())
    names = [n for g in opt._group_names for n in g]
    params = [torch.nn.Parameter(named[n].detach().cpu().double().clone()) for n in names]
    theirs = torch.optim.SGD([dict(params=params[:n0]), dict(params=params[n0:])], lr=0.5)
    theirs.load_state_dict(sd)                                     # torch accepts it; the checkpoint's hyper-parameters win
    assert theirs.param_groups[0]["nesterov"] is True and theirs.param_groups[1]["momentum"] == 0.0
    conv = "encoder.lidar_encoder._model.layer2.0.conv1.weight"
    idx = names.index(conv)
    held = theirs.state[params[idx]]["momentum_buffer"]
    off, n = L.offsets[conv]
    o, i, kh, kw = held.shape
    assert held.shape == params[idx].shape and torch.equal(held.float(), L.exp_avg[off:off + n].view(o, kh, kw, i).permute(0, 3, 1, 2).cpu())
    eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    _feed(net, names, params)
    theirs.step()
    dp, db, bound = _errors(net, opt, theirs, names, params)
    print("sgd-err checkpoint: one step after torch loaded the state  p %.3g  buf %.3g (bound for buf %.3g)" % (dp, db, bound))
    assert dp < BOUND and db < bound
    # the reverse: torch's own (float64) state into a fresh FusedSGD on another module
    tsd = theirs.state_dict()
    net2 = _net()
    groups2 = configure_optimizers(net2)
    back = FusedSGD(net2, lr=0.7, param_groups=groups2)
    back.load_state_dict(tsd)
    assert back.param_groups[0]["momentum"] == 0.9 and back.param_groups[0]["nesterov"] is True and back.param_groups[1]["lr"] == 2e-3
    L2 = net2._layout
    live = torch.zeros(L.total, dtype=torch.bool, device=DEV)
    live[:L.tail] = True
    want = tsd["state"][idx]["momentum_buffer"].float()               # float32 of torch's float64 buffer, OIHW -> OHWI
    assert torch.equal(L2.exp_avg[off:off + n].view(o, kh, kw, i).permute(0, 3, 1, 2).cpu(), want)
    assert (L2.exp_avg[live] - L.exp_avg[live]).abs().max().item() < bound       # (the twin's buffers beside the engine's own)
    steps = back.tensor_steps()
    held = {k for k, st in tsd["state"].items() if st.get("momentum_buffer") is not None}
    assert held and all(steps[n] == (1 if k in held else 0) for k, n in enumerate(names) if n in steps)
    assert set(back.state_dict()["state"]) == held
    tsd["param_groups"][0]["maximize"] = True
    with pytest.raises(ValueError, match="maximize"):
        back.load_state_dict(tsd)


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from oracle import fixtures
    root = tmp_path_factory.mktemp("sgd_train")
    samples = fixtures.synthetic_samples((5, 9, 3, 7), seed=3, radar_counts=(50, 81, 81, 20))
    for i, s in enumerate(samples):
        with open(root / ("%d.pkl" % i), "wb") as fd:
            pickle.dump(s, fd)
    return D.FrameStore(str(root), GlobalConfig(), "train")


def test_trainer_captures_sgd_steps_and_save_resume_continue_with_the_same_bits(store, tmp_path):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.parallel import StaticBatchStep
    from mmfn_amd.trainer import Trainer
    cfg = GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    loader = D.make_loader(store, batch_size=2, num_workers=0)
    logdir = str(tmp_path / "log")
    net = _net()
    opt = _sgd(net)
    tr = Trainer(DEV, logdir)
    tr.train(net, loader, cfg, opt)
    tr.train(net, loader, cfg, opt)
    captured = [k for k, v in tr._static_steps.items() if isinstance(v, StaticBatchStep)]
    assert captured and all(("optimizer", "sgd") in k for k in captured)        # SGD steps are captured, under a signature of their own
    tr.save(net, opt)
    osd = torch.load(os.path.join(logdir, "recent_optim.pth"))
    assert set(osd["state"][0]) == {"momentum_buffer"} and osd["param_groups"][0]["nesterov"] is True
    tr.train(net, loader, cfg, opt)                                   # the uninterrupted run, one more epoch
    net2 = _net()
    opt2 = _sgd(net2)
    opt2.param_groups[0]["lr"] = 0.5                                  # (the checkpoint brings the hyper-parameters)
    tr2 = Trainer(DEV, logdir)
    assert tr2.resume(net2, opt2, which="recent") is True
    assert opt2.param_groups[0]["lr"] == 1e-3 and net2._engine_for().opt_kind == "sgd"
    tr2.train(net2, loader, cfg, opt2)
    torch.cuda.synchronize()
    L1, L2 = net._layout, net2._layout
    assert torch.equal(L1.params, L2.params) and torch.equal(L1.exp_avg, L2.exp_avg) and bool(L1.exp_avg.any())
