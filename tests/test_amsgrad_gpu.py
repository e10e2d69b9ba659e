"""amsgrad on the fused AdamW step: mmfn_adamw_groups_ams_f32 / mmfn_adamw_rows_ams_f32 against torch.optim.AdamW(amsgrad=True) and,
bit for bit, against the launches without amsgrad; then the engine, FusedAdamW's state dict, the trainer's resume, the guard and
frozen tensors.  amsgrad steps run eagerly (parallel.GraphedStep refuses to capture them), so no test here captures a step.

Yardstick: torch.optim.AdamW on CPU tensors in float64 (tests/test_amsgrad_cpu.py holds the helpers and checks the float64
restatement against torch).  Bound: max |d| < 1e-6 for p, m and v, the bound at which tests/test_kernels_gpu.py::test_adamw_matches_torch
and tests/test_tensor_steps_gpu.py hold the launch without amsgrad; that launch is held to it first, on the same inputs.  Against a
float64 reference the deviation is the kernel's own rounding: p is rounded once per step (p * decay - step_size * q is one fma), half
an ulp of p, 6e-8 for |p| in [1, 2), so at most 3.6e-7 over six steps with |p| < 1.5; the step term lr * m / denom <= 3e-3 carries a
relative error of a few 1e-7, i.e. 1e-9.  m stays below 1.  v = beta2 * v + (1 - beta2) * g * g takes three roundings per step at
the magnitude of its largest element: about 0.3 over the 3076 floats of the small case, but up to 3 - 5 among the 4.2 M of the large
one (a 5-sigma draw squared, times 1 - beta2 = 0.1, twice), where an ulp is 2.4e-7 to 4.8e-7 - the same in both launches, whose m and
v have the same bits.  Measured on an MI355X, max |d| for p / m / v: small case, six steps, plain 3.28e-07 / 1.28e-07 / 3.24e-07,
amsgrad 3.68e-07 / 1.28e-07 / 3.24e-07; large case, three steps, plain 2.36e-07 / 1.78e-07 / 7.72e-07, amsgrad 2.30e-07 / 1.78e-07
/ 7.72e-07; the model's four optimizer steps 8.3e-08, 1.5e-07, 2.2e-07, 2.7e-07 for p (profiles/amsgrad_bench.txt; each comparison
prints an `amsgrad-err` line).

The inputs tell amsgrad from plain AdamW: six steps whose gradients shrink (1, 1, 0.1, 0.01, 0.01, 0.01 times a seeded normal draw)
and beta2 of 0.9 / 0.95 in the amsgrad groups; the CPU reference alone shows the two trajectories hundreds of bounds apart and
vmax != v in most elements (asserted below and in tests/test_amsgrad_cpu.py)."""
import functools
import os
import pickle
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_amsgrad_cpu as R   # noqa: E402  (the float64 yardstick, the step sequence, the three groups, the bound)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = R.BOUND
SENTINEL = 123.0

N4_SMALL = 3 * 256 + 1                 # n = 4 * (3 * 256 + 1): the group map changes inside a workgroup's range (float4s 250, 526)
CUTS_SMALL = (250, 526)


def _big_n4():
    from mmfn_amd import ops
    return ops.adamw_max_blocks() * 256 + 37   # past what the capped grid covers in one trip: the grid-stride loop goes round


def _cuts(n4):
    return CUTS_SMALL if n4 == N4_SMALL else (300001, n4 - 50)     # (the last group sits in the second trip)


def _spans(n4):
    a, b = _cuts(n4)
    return [(0, 4 * a), (4 * a, 4 * b), (4 * b, 4 * n4)]


def _group_of(n4):
    a, b = _cuts(n4)
    t = torch.zeros(n4, dtype=torch.uint8)
    t[a:b], t[b:] = 1, 2
    return t.to(DEV)


def _hyper(groups, grad_scale=1.0):
    h = torch.zeros(16, 8)
    for i, g in enumerate(groups):
        h[i] = torch.tensor([g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], grad_scale, 0.0, float(g["amsgrad"])])
    return h.to(DEV)


def _step(t):
    return torch.tensor([t], dtype=torch.int64, device=DEV)


def _case(n4=N4_SMALL, seed=0):
    """Five buffers mid-run: vmax above v for about half of the elements, an average beside them."""
    n = 4 * n4
    gen = torch.Generator(device=DEV).manual_seed(1000 + seed + n4)
    mk = lambda: torch.randn(n, device=DEV, generator=gen)
    return dict(p=mk(), g=mk() * 0.3, m=mk() * 0.1, v=mk().abs() * 0.01, x=mk().abs() * 0.01, a=mk())


def _clone(b):
    return {k: t.clone() for k, t in b.items()}


def _run(b, hyper, n4, t=5, coef=None, avg=None, ok=None, mask=None, ams=True):
    """One launch in place over the buffers b: the amsgrad entry point (ams) or the existing one."""
    from mmfn_amd import ops
    table = _group_of(n4) if mask is None else mask
    ops.adamw_groups(b["p"], b["g"], b["m"], b["v"], _step(t), hyper, 3, group_of=table, coef=coef,
                     avg=None if avg is None else (b["a"],) + avg, ok=ok, mask=mask is not None, vmax=b["x"] if ams else None)
    torch.cuda.synchronize()
    return b


def _same(a, b, keys="pmvxag", where=None):
    for k in keys:
        x, y = (a[k], b[k]) if where is None else (a[k][where], b[k][where])
        assert torch.equal(x, y), k


def _elements(n4, groups):
    """bool mask over the floats of the named groups"""
    m = torch.zeros(4 * n4, dtype=torch.bool)
    for gi in groups:
        b, e = _spans(n4)[gi]
        m[b:e] = True
    return m.to(DEV)


# ------------------------------------------------------------------------------------------------ 1. against torch
@pytest.mark.parametrize("size", ["small", "past_one_grid_trip"])
def test_grouped_launch_matches_torch_amsgrad_over_shrinking_gradients(size):
    """First the existing launch (no group with amsgrad) against torch.optim.AdamW in float64, then the amsgrad launch (group 1
    off) against torch.optim.AdamW with the groups' amsgrad, on the same parameters and gradients, at the same bound; after every
    step vmax is, bitwise, torch.maximum of what it was and the kernel's own new v - and untouched where the flag is off."""
    from mmfn_amd import ops
    n4 = N4_SMALL if size == "small" else _big_n4()
    n, spans = 4 * n4, _spans(n4)
    steps = len(R.SCALES) if size == "small" else 3            # (the large case is about the second grid trip, not the sequence)
    p0 = torch.rand(n, generator=torch.Generator().manual_seed(5)) * 3.0 - 1.5
    grads = R.shrinking_grads(n, 6, steps)
    group_of = _group_of(n4)
    on, off = _elements(n4, (0, 2)), _elements(n4, (1,))
    worst = {}
    for name, groups in (("plain", [dict(g, amsgrad=False) for g in R.GROUPS]), ("amsgrad", R.GROUPS)):
        ref = R.torch_reference(p0, grads, groups, spans)
        if name == "amsgrad" and size == "small":   # the reference alone: these inputs tell the two apart
            plain_ref = R.torch_reference(p0, grads, [dict(g, amsgrad=False) for g in R.GROUPS], spans)
            assert (ref[-1]["p"] - plain_ref[-1]["p"]).abs().cpu()[on.cpu()].median().item() > 100 * BOUND
            assert (ref[-1]["vmax"] != ref[-1]["v"])[on.cpu()].float().mean().item() >= 0.5
        hyper = _hyper(groups)
        p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        x = torch.zeros(n, device=DEV)
        x[off] = SENTINEL
        step = torch.zeros(1, dtype=torch.int64, device=DEV)
        worst[name] = dict(p=0.0, m=0.0, v=0.0)
        for t, g in enumerate(grads):
            ops.step_advance(step)
            before = x.clone()
            ops.adamw_groups(p, g.to(DEV), m, v, step, hyper, 3, group_of=group_of, vmax=x if name == "amsgrad" else None)
            for key, got in (("p", p), ("m", m), ("v", v)):
                worst[name][key] = max(worst[name][key], (got.cpu().double() - ref[t][key]).abs().max().item())
            if name == "amsgrad":
                assert torch.equal(x[on], torch.maximum(before[on], v[on]))
                assert bool((x[off] == SENTINEL).all())
                assert (x[on].cpu().double() - ref[t]["vmax"][on.cpu()]).abs().max().item() < BOUND
        print("amsgrad-err %s n=%d steps=%d %s: max |d| vs torch float64  p %.3g  m %.3g  v %.3g"
              % (size, n, steps, name, worst[name]["p"], worst[name]["m"], worst[name]["v"]))
        assert all(e < BOUND for e in worst[name].values()), (name, worst[name])
        if name == "amsgrad" and size == "small":
            assert (x[on] != v[on]).float().mean().item() >= 0.5


# ------------------------------------------------------------------------------------------------ 2. against the launches without
@pytest.mark.parametrize("size", ["small", "past_one_grid_trip"])
def test_flag_off_group_and_all_flags_off_have_the_existing_bits(size):
    n4 = N4_SMALL if size == "small" else _big_n4()
    base = _case(n4)
    base["x"][_elements(n4, (1,))] = SENTINEL
    old = _run(_clone(base), _hyper(R.GROUPS), n4, ams=False)                     # (the existing launch ignores the last column)
    got = _run(_clone(base), _hyper(R.GROUPS), n4)
    off, on = _elements(n4, (1,)), _elements(n4, (0, 2))
    _same(got, old, "pmv", off)
    assert bool((got["x"][off] == SENTINEL).all())
    assert torch.equal(got["x"][on], torch.maximum(base["x"][on], got["v"][on]))
    _same(got, old, "mv", on)                                                       # the moments do not depend on the flag
    assert not torch.equal(got["p"][on], old["p"][on])
    # every flag off: the whole launch is the existing one, vmax is not touched anywhere
    none = [dict(g, amsgrad=False) for g in R.GROUPS]
    base["x"].fill_(SENTINEL)
    _same(_run(_clone(base), _hyper(none), n4), _run(_clone(base), _hyper(none), n4, ams=False))


def test_coef_is_grad_scale():
    base = _case()
    half = torch.tensor([0.5], device=DEV)
    _same(_run(_clone(base), _hyper(R.GROUPS, 0.8), N4_SMALL, coef=half), _run(_clone(base), _hyper(R.GROUPS, 0.4), N4_SMALL))


@pytest.mark.parametrize("mode,count", [("ema", 2), ("swa", 0), ("swa", 3)])
def test_avg_instance_has_the_bits_without_avg_and_the_average_of_a_pass_afterwards(mode, count):
    from mmfn_amd import ops
    base = _case()
    hyper = _hyper(R.GROUPS)
    cnt, w = torch.tensor([count], dtype=torch.int64, device=DEV), torch.tensor([0.1], device=DEV)
    code = ops.AVG_EMA if mode == "ema" else ops.AVG_SWA
    got = _run(_clone(base), hyper, N4_SMALL, avg=(cnt, w, code))
    want = _run(_clone(base), hyper, N4_SMALL)
    ops.weight_average(want["a"], want["p"], cnt, w, code)
    torch.cuda.synchronize()
    _same(got, want)
    assert not torch.equal(got["a"], base["a"])


@pytest.mark.parametrize("with_avg", [False, True])
def test_guard_flag(with_avg):
    from mmfn_amd import ops
    base = _case()
    hyper = _hyper(R.GROUPS)
    coef = torch.tensor([0.37], device=DEV)
    avg = (torch.tensor([2], dtype=torch.int64, device=DEV), torch.tensor([0.1], device=DEV), ops.AVG_EMA) if with_avg else None
    ok0, ok1 = (torch.full((1,), x, dtype=torch.int32, device=DEV) for x in (0, 1))
    _same(_run(_clone(base), hyper, N4_SMALL, coef=coef, avg=avg, ok=ok0), base)                 # skipped: all five buffers, avg
    _same(_run(_clone(base), hyper, N4_SMALL, coef=coef, avg=avg, ok=ok1), _run(_clone(base), hyper, N4_SMALL, coef=coef, avg=avg))


@pytest.mark.parametrize("with_avg", [False, True])
def test_masked_float4s_keep_all_four_buffers_and_the_average_follows_frozen_p(with_avg):
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
    for k in "pmvx":               # sentinels: a frozen float4 is neither loaded nor stored (NaN would spread through any arithmetic)
        base[k][cold] = float("nan") if k != "p" else SENTINEL
    got = _run(_clone(base), hyper, N4_SMALL, avg=avg, mask=table)
    free = _clone(base)
    for k in "pmvx":
        free[k][cold] = 1.0
    want = _run(free, hyper, N4_SMALL, avg=avg)
    _same(got, want, "pmvx", ~cold)
    for k in "mvx":
        assert bool(torch.isnan(got[k][cold]).all())
    assert bool((got["p"][cold] == SENTINEL).all())
    if with_avg:
        _same(got, want, "a", ~cold)
        ref = base["a"].clone()
        ops.weight_average(ref, base["p"], avg[0], avg[1], avg[2])
        torch.cuda.synchronize()
        assert torch.equal(got["a"][cold], ref[cold])
    else:
        _same(got, base, "a")


@pytest.mark.parametrize("variant", ["plain", "coef_avg_guard"])
def test_rows_launch_has_the_bits_of_the_grouped_launch_per_class(variant):
    """Two classes with counts 1 and 5, two groups (the second without amsgrad), a frozen span: every row's float4s have the bits of
    mmfn_adamw_groups_ams_f32 run with *step = the class's count."""
    from mmfn_amd import ops
    n4 = N4_SMALL
    base = _case(n4, seed=1)
    groups = [R.GROUPS[0], R.GROUPS[1]]
    hyper = _hyper(groups, 0.5)
    counts = (1, 5)
    # (float4 range, group, class): rows are (group, class) pairs
    parts = [((0, 100), 0, 0), ((100, 259), 1, 0), ((259, 517), 0, 1), ((517, 700), 1, 1), ((700, n4), None, None)]
    rows = torch.tensor([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=torch.int32)
    row_of = torch.full((n4,), ops.ADAMW_FROZEN, dtype=torch.uint8)
    group_of, class_of = torch.zeros(n4, dtype=torch.uint8), torch.full((n4,), -1, dtype=torch.int64)
    for (b, e), grp, cls in parts:
        if grp is not None:
            row_of[b:e] = rows.tolist().index([grp, cls])
            group_of[b:e], class_of[b:e] = grp, cls
    full = variant != "plain"
    coef = torch.tensor([0.37], device=DEV) if full else None
    avg = (torch.tensor([2], dtype=torch.int64, device=DEV), torch.tensor([0.1], device=DEV), ops.AVG_EMA) if full else None
    class_steps = torch.tensor(counts + (99,), dtype=torch.int64, device=DEV)
    for okv in ((1, 0) if full else (None,)):
        ok = None if okv is None else torch.full((1,), okv, dtype=torch.int32, device=DEV)
        got = _clone(base)
        ops.adamw_rows(got["p"], got["g"], got["m"], got["v"], class_steps, 2, hyper, 2, row_of.to(DEV), rows, coef=coef,
                       avg=None if avg is None else (got["a"],) + avg, ok=ok, vmax=got["x"])
        torch.cuda.synchronize()
        if okv == 0:
            _same(got, base)
            continue
        want = _clone(base)
        for c, t in enumerate(counts):
            table = torch.where(class_of == c, group_of, torch.full_like(group_of, ops.ADAMW_FROZEN)).to(DEV)
            ref = _clone(base)
            ops.adamw_groups(ref["p"], ref["g"], ref["m"], ref["v"], _step(t), hyper, 2, group_of=table, coef=coef,
                             avg=None if avg is None else (ref["a"],) + avg, ok=ok, mask=True, vmax=ref["x"])
            mine = (class_of == c).repeat_interleave(4).to(DEV)
            for k in "pmvxa":
                want[k][mine] = ref[k][mine]
            if full and c == 0:
                cold = (class_of < 0).repeat_interleave(4).to(DEV)
                want["a"][cold] = ref["a"][cold]
        torch.cuda.synchronize()
        _same(got, want)
        live = (class_of >= 0).repeat_interleave(4).to(DEV)
        assert not torch.equal(got["p"][live], base["p"][live]) and torch.equal(got["x"][~live], base["x"][~live])
        ams = ((class_of >= 0) & (group_of == 0)).repeat_interleave(4).to(DEV)
        assert torch.equal(got["x"][ams], torch.maximum(base["x"][ams], got["v"][ams])) and torch.equal(got["x"][~ams], base["x"][~ams])


def test_nan_gradient_leaves_nan_in_vmax_of_that_element_alone():
    base = _case()
    spot = 4 * 10 + 2          # an element of group 0 (amsgrad on); one of group 1 (off) for contrast
    other = 4 * 300 + 1
    base["g"][spot] = float("nan")
    base["g"][other] = float("nan")
    got = _run(_clone(base), _hyper(R.GROUPS), N4_SMALL)
    bad = torch.isnan(got["x"]).nonzero().flatten().tolist()
    assert bad == [spot], bad                                     # torch.maximum propagates NaN; fmaxf would have dropped it
    assert torch.isnan(got["v"]).nonzero().flatten().tolist() == [spot, other]
    assert torch.equal(got["x"][other], base["x"][other])
    # ... and a NaN already in vmax stays
    base2 = _case()
    base2["x"][spot] = float("nan")
    got2 = _run(_clone(base2), _hyper(R.GROUPS), N4_SMALL)
    assert torch.isnan(got2["x"]).nonzero().flatten().tolist() == [spot] and bool(torch.isnan(got2["p"][spot]))


def test_entry_points_refuse_what_they_would_dereference():
    from mmfn_amd import ops
    from mmfn_amd._lib import lib
    n4 = N4_SMALL
    base = _case(n4)
    b = _clone(base)
    hyper, table = _hyper(R.GROUPS), _group_of(n4)
    step, s = _step(3), torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()

    def groups(**kw):
        a = dict(p=P(b["p"]), g=P(b["g"]), m=P(b["m"]), v=P(b["v"]), x=P(b["x"]), n=4 * n4, table=P(table), hyper=P(hyper), n_groups=3,
                 step=P(step), variant=0, coef=None, ok=None)
        a.update(kw)
        return lib().mmfn_adamw_groups_ams_f32(a["p"], a["g"], a["m"], a["v"], a["x"], a["n"], a["table"], a["hyper"], a["n_groups"],
                                               a["step"], a["variant"], a["coef"], None, None, None, 0, a["ok"], s)
    for bad in (dict(x=None), dict(x=P(b["x"]) + 4), dict(x=P(b["x"]) + 8), dict(p=None), dict(g=None), dict(m=None), dict(v=None),
                dict(hyper=None), dict(step=None), dict(n_groups=0), dict(n_groups=17), dict(n=4 * n4 - 2), dict(variant=4),
                dict(variant=6), dict(variant=16), dict(variant=-1), dict(variant=1), dict(variant=2), dict(variant=5, coef=P(step)),
                dict(variant=8, table=None)):
        assert groups(**bad) == -1, bad
    rows = torch.tensor([[0, 0], [1, 0], [2, 1]], dtype=torch.int32)
    cs = torch.ones(2, dtype=torch.int64, device=DEV)

    def rowsf(**kw):
        a = dict(p=P(b["p"]), g=P(b["g"]), m=P(b["m"]), v=P(b["v"]), x=P(b["x"]), n=4 * n4, table=P(table), hyper=P(hyper), n_groups=3,
                 rows=rows.data_ptr(), n_rows=3, cs=P(cs), n_classes=2, variant=0)
        a.update(kw)
        return lib().mmfn_adamw_rows_ams_f32(a["p"], a["g"], a["m"], a["v"], a["x"], a["n"], a["table"], a["hyper"], a["n_groups"],
                                             a["rows"], a["n_rows"], a["cs"], a["n_classes"], a["variant"], None, None, None, None, 0,
                                             None, s)
    for bad in (dict(x=None), dict(x=P(b["x"]) + 4), dict(p=None), dict(v=None), dict(table=None), dict(rows=None), dict(cs=None),
                dict(n_rows=0), dict(n_rows=255), dict(n_classes=1), dict(n_groups=2), dict(variant=4), dict(variant=8), dict(variant=1)):
        assert rowsf(**bad) == -1, bad
    with pytest.raises(ValueError, match="vmax"):
        ops.adamw_groups(b["p"], b["g"], b["m"], b["v"], step, hyper, 3, group_of=table, vmax=b["x"][:100])
    with pytest.raises(ValueError, match="vmax"):
        ops.adamw_groups(b["p"], b["g"], b["m"], b["v"], step, hyper, 3, group_of=table, vmax=b["x"].double())
    torch.cuda.synchronize()
    _same(b, base)                                                  # no refused call launched anything


# ------------------------------------------------------------------------------------------------ engine helpers
@functools.lru_cache(maxsize=None)
def _weights():
    from oracle import harness
    return harness.build_oracle("vec", dropout=0.0).state_dict()


def _net():
    from mmfn_amd.config import GlobalConfig
    import mmfn_amd.model as M
    net = M.MMFN(GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0), DEV)
    net.load_state_dict(_weights(), strict=True)
    net.train()
    return net


@functools.lru_cache(maxsize=None)
def _inputs():
    sys.path.insert(0, ROOT)
    import bench
    return bench.synth_inputs(2, torch.device(DEV), seed=42, variant="vec")


def _state(net):
    L, eng = net._layout, net._engine_for()
    out = [L.params, L.exp_avg, L.exp_avg_sq, L.buffers_flat, L.counters_flat, eng.step_count, eng.rng_state]
    return out + ([L.max_exp_avg_sq] if L.max_exp_avg_sq is not None else [])


def _bits(net):
    torch.cuda.synchronize()
    return [t.clone() for t in _state(net)]


def _shrinking_grads(net, gen, i):
    eng, L = net._engine_for(), net._layout
    eng.trainable_mask()        # (new flags zero the frozen gradient ranges: before the gradients are written)
    L.grads[:L.tail].normal_(generator=gen).mul_(0.01 * R.SCALES[min(i + 1, len(R.SCALES) - 1)])
    if eng.frozen:
        for n in eng.frozen:
            b, e = L.span(n)
            L.grads[b:e] = 0


BETAS = (0.9, 0.9)      # (beta2 = 0.9: v falls fast enough behind vmax for the two denominators to differ, see the module docstring)
TRUNK = "encoder.lidar_encoder."


# ------------------------------------------------------------------------------------------------ 3. engine and optimizer
def test_train_steps_keep_the_running_maximum_and_are_not_captured():
    import types
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.parallel import GraphedStep
    inp, gt = _inputs()
    nets = []
    for _ in range(2):                                                        # twice: the steps are reproducible bit for bit
        net = _net()
        opt = FusedAdamW(net, lr=1e-3, betas=BETAS, amsgrad=True)            # (TypeError before amsgrad existed)
        eng, L = net._engine_for(), net._layout
        assert L.max_exp_avg_sq is not None and not bool(L.max_exp_avg_sq.any())
        running = torch.zeros_like(L.exp_avg_sq)
        for _ in range(4):
            eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
            running = torch.maximum(running, L.exp_avg_sq)
        torch.cuda.synchronize()
        assert torch.equal(L.max_exp_avg_sq, running)
        assert (L.max_exp_avg_sq[:L.tail] != L.exp_avg_sq[:L.tail]).float().mean().item() > 0.1     # (not just v again)
        nets.append(net)
    for a, b in zip(_bits(nets[0]), _bits(nets[1])):
        assert torch.equal(a, b)
    # amsgrad steps are not captured: the capture is refused before anything is recorded, and so is the replay of a step that
    # was captured before a flag was set (the checks of GraphedStep.__call__ on a stand-in that holds no capture)
    before = _bits(net)
    with pytest.raises(RuntimeError, match="amsgrad"):
        GraphedStep(eng, None, inp, gt, lr=1e-3, warm=1, groups=opt.hyper_rows())
    stale = types.SimpleNamespace(engine=eng, variant="final", fold=False, average=None, mask=eng.trainable_mask(),
                                  class_epoch=eng.classes.epoch, guard=False)
    with pytest.raises(RuntimeError, match="amsgrad"):
        GraphedStep.__call__(stale)
    for a, b in zip(before, _bits(net)):
        assert torch.equal(a, b)


@pytest.fixture(scope="module")
def fidelity():
    """Four optimizer.step() calls on seeded shrinking gradients written into the flat gradient buffer, beside
    torch.optim.AdamW(amsgrad=True) in float64 on CPU copies of the parameters (checkpoint shapes, named_parameters() order)."""
    from mmfn_amd.optim import FusedAdamW
    net = _net()
    L = net._layout
    opt = FusedAdamW(net, lr=1e-3, betas=BETAS, amsgrad=True)
    names = [n for n, _ in net.named_parameters()]
    params = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in net.parameters()]
    twin = torch.optim.AdamW(params, lr=1e-3, betas=BETAS, amsgrad=True)
    gen = torch.Generator(device=DEV).manual_seed(2025)
    errs = []
    for i in range(4):
        _shrinking_grads(net, gen, i)
        for n, r in zip(names, params):
            r.grad = None if n in L.unused else L.grad_views[n].detach().cpu().double().clone()
        twin.step()
        opt.step()
        torch.cuda.synchronize()
        got = dict(net.named_parameters())
        errs.append(max((got[n].detach().cpu().double() - r.detach()).abs().max().item() for n, r in zip(names, params)))
    return net, opt, twin, names, params, errs


def test_optimizer_steps_match_torch_amsgrad(fidelity):
    net, opt, twin, names, params, errs = fidelity
    print("amsgrad-err model: max |dp| vs torch float64 per step: " + ", ".join("%.3g" % e for e in errs))
    assert all(e < BOUND for e in errs), errs
    # the same run without amsgrad is far outside the bound: the comparison can tell
    L = net._layout
    assert (L.max_exp_avg_sq[:L.tail] != L.exp_avg_sq[:L.tail]).float().mean().item() >= 0.5
    sd = opt.state_dict()
    worst = 0.0
    for idx, r in enumerate(params):
        if r in twin.state:
            st = twin.state[r]
            worst = max(worst, (sd["state"][idx]["max_exp_avg_sq"].cpu().double() - st["max_exp_avg_sq"]).abs().max().item())
            assert sd["state"][idx]["max_exp_avg_sq"].shape == r.shape
        else:
            assert idx not in sd["state"]
    assert worst < BOUND


def test_state_dict_goes_to_torch_and_a_torch_state_dict_comes_back(fidelity):
    from mmfn_amd.optim import FusedAdamW
    net, opt, twin, names, params, _ = fidelity
    L = net._layout
    sd = opt.state_dict()
    assert sd["param_groups"][0]["amsgrad"] is True
    cpu_params = [torch.nn.Parameter(p.detach().cpu().clone()) for p in net.parameters()]
    theirs = torch.optim.AdamW(cpu_params, lr=1e-4, amsgrad=True)
    theirs.load_state_dict(sd)                                               # torch accepts it
    conv = "encoder.lidar_encoder._model.layer2.0.conv1.weight"
    idx = names.index(conv)
    held = theirs.state[cpu_params[idx]]["max_exp_avg_sq"]
    held = held.cpu()
    assert held.shape == cpu_params[idx].shape and float(held.max()) > 0
    off, n = L.offsets[conv]
    o, i, kh, kw = held.shape
    assert torch.equal(held, L.max_exp_avg_sq[off:off + n].view(o, kh, kw, i).permute(0, 3, 1, 2).cpu())
    # the reverse: torch's own (float64) amsgrad state into a fresh FusedAdamW - the flat vmax, the convolution layout included
    tsd = twin.state_dict()
    before = L.max_exp_avg_sq.clone()
    L.max_exp_avg_sq.fill_(SENTINEL)
    back = FusedAdamW(net, lr=1e-4)                                          # (amsgrad off: the checkpoint's groups decide)
    back.load_state_dict(tsd)
    assert back.amsgrad_flags() == (True,) and net._engine_for().opt_amsgrad == (True,)
    want = tsd["state"][idx]["max_exp_avg_sq"].float().cpu()
    flat = L.max_exp_avg_sq[off:off + n].view(o, kh, kw, i).cpu()
    for a in range(0, o, 17):
        for b in range(0, i, 13):
            for c in range(kh):
                for d in range(kw):
                    assert flat[a, c, d, b].item() == want[a, b, c, d].item()
    out = back.state_dict()["state"]       # every tensor's maximum is float32 of torch's float64 one, in checkpoint shape
    assert set(out) == set(tsd["state"])
    for k in list(out)[::7]:
        assert torch.equal(out[k]["max_exp_avg_sq"].cpu(), tsd["state"][k]["max_exp_avg_sq"].float())
    live = L.max_exp_avg_sq != 0             # (the padding between tensors and the absent ids are zero now)
    assert (L.max_exp_avg_sq - before)[live].abs().max().item() < BOUND
    u = sorted(L.unused)[0]
    b, e = L.span(u)
    assert not bool(L.max_exp_avg_sq[b:e].any())
    # an amsgrad checkpoint group whose stepped entry lacks the maximum is refused
    del tsd["state"][idx]["max_exp_avg_sq"]
    with pytest.raises(ValueError, match="max_exp_avg_sq"):
        back.load_state_dict(tsd)


def test_amsgrad_on_the_decay_group_only_leaves_the_others_on_the_plain_trajectory():
    from mmfn_amd.optim import FusedAdamW, configure_optimizers
    inp, gt = _inputs()
    nets = []
    for on in (True, False):
        net = _net()
        groups = configure_optimizers(net)
        for g in groups:
            g["betas"] = BETAS
        groups[0]["amsgrad"] = on
        opt = FusedAdamW(net, lr=1e-3, param_groups=groups)
        gen = torch.Generator(device=DEV).manual_seed(7)
        for i in range(3):
            _shrinking_grads(net, gen, i)
            opt.step()
        torch.cuda.synchronize()
        nets.append((net, opt))
    (a, oa), (b, ob) = nets
    La, Lb = a._layout, b._layout
    assert Lb.max_exp_avg_sq is None and La.max_exp_avg_sq is not None
    assert "max_exp_avg_sq" not in str(ob.state_dict()["state"][0].keys())
    decay = torch.zeros(La.total, dtype=torch.bool, device=DEV)
    for n in oa._group_names[0]:
        s, e = La.span(n)
        decay[s:e] = True
    live = torch.zeros_like(decay)
    live[:La.tail] = True
    rest = live & ~decay
    for x, y in ((La.params, Lb.params), (La.exp_avg, Lb.exp_avg), (La.exp_avg_sq, Lb.exp_avg_sq)):
        assert torch.equal(x[rest], y[rest])
    assert not bool(La.max_exp_avg_sq[rest].any()) and not torch.equal(La.params[decay], Lb.params[decay])
    sd = oa.state_dict()
    n0 = len(oa._group_names[0])
    assert "max_exp_avg_sq" in sd["state"][0] and "max_exp_avg_sq" not in sd["state"][n0]
    assert [g["amsgrad"] for g in sd["param_groups"]] == [True, False]


def test_plain_optimizer_allocates_nothing_and_issues_the_existing_entry_points(monkeypatch):
    from mmfn_amd import ops
    from mmfn_amd.optim import FusedAdamW
    inp, gt = _inputs()
    net = _net()
    opt = FusedAdamW(net, lr=1e-3)
    seen = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (seen.append(name) if "adamw" in name else None, real(name, *a))[1])
    eng = net._engine_for()
    eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    eng.train_step(inp, gt, lr=1e-3, clip_grad_norm=1.0, groups=opt.hyper_rows())
    torch.cuda.synchronize()
    assert seen == ["mmfn_adamw_groups_f32"] * 2
    assert net._layout.max_exp_avg_sq is None and eng.opt_amsgrad == (False,)
    sd = opt.state_dict()
    assert sd["param_groups"][0]["amsgrad"] is False and all("max_exp_avg_sq" not in st for st in sd["state"].values())
    assert float(eng.opt_hyper[:, 7].abs().max()) == 0.0


def test_guard_keeps_vmax_through_a_skipped_step(monkeypatch):
    """The guard armed and a NaN written into the gradient buffer (in front of the readiness group's norm pass, as the backward
    reports the group): the step is skipped on the device and all five buffers keep their bits."""
    from mmfn_amd.optim import FusedAdamW
    inp, gt = _inputs()
    net = _net()
    opt = FusedAdamW(net, lr=1e-3, betas=BETAS, amsgrad=True)
    eng, L = net._engine_for(), net._layout
    eng.set_nonfinite_guard(True)
    eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    torch.cuda.synchronize()
    assert int(eng.skipped_steps.item()) == 0 and bool(L.max_exp_avg_sq.any())
    before = [t.clone() for t in (L.params, L.exp_avg, L.exp_avg_sq, L.max_exp_avg_sq, eng.step_count)]
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
    eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    torch.cuda.synchronize()
    assert int(eng.skipped_steps.item()) == 1 and bool(torch.isnan(L.grads[off]))
    for a, b in zip(before, (L.params, L.exp_avg, L.exp_avg_sq, L.max_exp_avg_sq, eng.step_count)):
        assert torch.equal(a, b)
    # a finite gradient afterwards steps again, vmax with it
    poison[0] = False
    eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    torch.cuda.synchronize()
    assert int(eng.skipped_steps.item()) == 1 and int(eng.step_count.item()) == 2
    assert torch.equal(L.max_exp_avg_sq, torch.maximum(before[3], L.exp_avg_sq))


def test_frozen_trunk_keeps_zero_vmax_and_starts_at_t_1_through_the_rows_launch(monkeypatch):
    from mmfn_amd import ops
    from mmfn_amd.optim import FusedAdamW
    net = _net()
    opt = FusedAdamW(net, lr=1e-3, betas=BETAS, amsgrad=True)
    eng, L = net._engine_for(), net._layout
    trunk = torch.zeros(L.total, dtype=torch.bool, device=DEV)
    for n in L.offsets:
        if n.startswith(TRUNK):
            b, e = L.span(n)
            trunk[b:e] = True
    seen = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (seen.append(name) if "adamw" in name else None, real(name, *a))[1])
    gen = torch.Generator(device=DEV).manual_seed(99)
    net.freeze(TRUNK)
    p_before = L.params[trunk].clone()
    for i in range(2):
        _shrinking_grads(net, gen, i)
        opt.step()
    torch.cuda.synchronize()
    assert seen == ["mmfn_adamw_groups_ams_f32"] * 2                       # the masked instance: one shared counter serves everybody
    assert not bool(L.max_exp_avg_sq[trunk].any()) and not bool(L.exp_avg_sq[trunk].any()) and torch.equal(L.params[trunk], p_before)
    assert bool(L.max_exp_avg_sq[~trunk][:1000].any())
    net.unfreeze(TRUNK)
    _shrinking_grads(net, gen, 2)
    g = L.grads.clone()
    opt.step()
    torch.cuda.synchronize()
    assert seen[-1] == "mmfn_adamw_rows_ams_f32"                           # the trunk's class is behind: per-class counters
    # the trunk's first step is a t = 1 amsgrad step from zero state: the grouped launch with *step = 1 on copies
    ref = dict(p=p_before.new_zeros(L.total), m=torch.zeros(L.total, device=DEV), v=torch.zeros(L.total, device=DEV),
               x=torch.zeros(L.total, device=DEV))
    ref["p"][trunk] = p_before
    ops.adamw_groups(ref["p"], g, ref["m"], ref["v"], _step(1), eng.opt_hyper, 1, vmax=ref["x"])
    torch.cuda.synchronize()
    for got, key in ((L.params, "p"), (L.exp_avg, "m"), (L.exp_avg_sq, "v"), (L.max_exp_avg_sq, "x")):
        assert torch.equal(got[trunk], ref[key][trunk]), key
    assert torch.equal(L.max_exp_avg_sq[trunk], L.exp_avg_sq[trunk])
    steps = dict(zip(eng.classes.names, eng.tensor_steps().tolist()))
    assert all(t == (1 if n.startswith(TRUNK) else 3) for n, t in steps.items())


def test_frozen_vmax_keeps_its_bits_through_accumulated_clipped_guarded_averaged_steps():
    """A trunk frozen after it has stepped holds a non-zero vmax: accumulated, clipped, guarded steps with an attached average
    (the COEF | AVG | GUARD | MASK instance) leave its p / m / v / vmax bits alone while everything else steps and the average
    follows the frozen parameters."""
    from mmfn_amd.averaging import AveragedMMFN
    from mmfn_amd.optim import FusedAdamW
    inp, gt = _inputs()
    net = _net()
    opt = FusedAdamW(net, lr=1e-3, betas=BETAS, amsgrad=True)
    eng, L = net._engine_for(), net._layout
    eng.train_step(inp, gt, lr=1e-3, groups=opt.hyper_rows())
    trunk = torch.zeros(L.total, dtype=torch.bool, device=DEV)
    for n in L.offsets:
        if n.startswith(TRUNK):
            b, e = L.span(n)
            trunk[b:e] = True
    net.freeze(TRUNK)
    eng.set_nonfinite_guard(True)
    avg = AveragedMMFN(net, "ema", decay=0.9)
    net.attach_average(avg)
    torch.cuda.synchronize()
    held = [t[trunk].clone() for t in (L.params, L.exp_avg, L.exp_avg_sq, L.max_exp_avg_sq)]
    assert bool(held[3].any())
    rest = ~trunk
    rest[L.tail:] = False
    eng.accumulate_step(inp, gt)
    eng.train_step(inp, gt, lr=1e-3, clip_grad_norm=1.0, groups=opt.hyper_rows())
    torch.cuda.synchronize()
    after_first = L.max_exp_avg_sq[rest].clone()
    eng.train_step(inp, gt, lr=1e-3, clip_grad_norm=1.0, groups=opt.hyper_rows())
    torch.cuda.synchronize()
    assert int(eng.skipped_steps.item()) == 0 and int(eng.step_count.item()) == 3
    for was, now in zip(held, (L.params, L.exp_avg, L.exp_avg_sq, L.max_exp_avg_sq)):
        assert torch.equal(was, now[trunk])
    assert torch.equal(L.max_exp_avg_sq[rest], torch.maximum(after_first, L.exp_avg_sq[rest]))
    assert int(avg.n_averaged.item()) == 2 and not torch.equal(avg.module._layout.params[rest], L.params[rest])
    A = avg.module._layout.params
    assert torch.equal(A[trunk], L.params[trunk])      # the average of a parameter that never moved is that parameter


# ------------------------------------------------------------------------------------------------ 4. trainer
@pytest.fixture(scope="module")
def store(tmp_path_factory):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from oracle import fixtures
    root = tmp_path_factory.mktemp("amsgrad_train")
    samples = fixtures.synthetic_samples((5, 9, 3, 7), seed=3, radar_counts=(50, 81, 81, 20))
    for i, s in enumerate(samples):
        with open(root / ("%d.pkl" % i), "wb") as fd:
            pickle.dump(s, fd)
    return D.FrameStore(str(root), GlobalConfig(), "train")


def test_save_and_resume_continue_with_the_same_bits(store, tmp_path):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import Trainer
    cfg = GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    loader = D.make_loader(store, batch_size=2, num_workers=0)
    logdir = str(tmp_path / "log")
    net = _net()
    opt = FusedAdamW(net, lr=1e-3, betas=BETAS, amsgrad=True)
    tr = Trainer(DEV, logdir)
    tr.train(net, loader, cfg, opt)                                   # (graph=True as a user would: amsgrad steps run eagerly)
    assert not tr._static_steps                                       # nothing was captured
    tr.save(net, opt)
    osd = torch.load(os.path.join(logdir, "recent_optim.pth"))
    assert osd["param_groups"][0]["amsgrad"] is True and "max_exp_avg_sq" in osd["state"][0]
    tr.train(net, loader, cfg, opt)                                   # the uninterrupted run, one more epoch
    net2 = _net()
    opt2 = FusedAdamW(net2, lr=5e-4)                                  # (no amsgrad here: the checkpoint brings it)
    tr2 = Trainer(DEV, logdir)
    assert tr2.resume(net2, opt2, which="recent") is True
    assert opt2.amsgrad_flags() == (True,) and opt2.param_groups[0]["betas"] == BETAS
    tr2.train(net2, loader, cfg, opt2)
    torch.cuda.synchronize()
    L1, L2 = net._layout, net2._layout
    for a, b in ((L1.params, L2.params), (L1.exp_avg, L2.exp_avg), (L1.exp_avg_sq, L2.exp_avg_sq), (L1.max_exp_avg_sq, L2.max_exp_avg_sq)):
        assert torch.equal(a, b)
    assert (L1.max_exp_avg_sq[:L1.tail] != L1.exp_avg_sq[:L1.tail]).any()
