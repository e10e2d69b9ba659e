"""The non-finite guard of the fused training step and the per-tensor statistics pass: the guarded kernels against the plain
ones, a skipped step leaves every trained bit alone (BatchNorm statistics rolled back), a taken step is the unguarded step,
accumulation, weight averages, graph replay, data parallelism and the trainer's option.

Injection: a NaN goes into target_point[0, 0] (the gradient turns non-finite, the BatchNorm statistics stay finite) or into
velocity[1] (the BatchNorm statistics turn non-finite too: the rollback case).  Both enter arithmetic only."""
import functools
import json
import os
import pickle
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------------ kernels on flat arrays
def _flat_case(n, groups):
    gen = torch.Generator(device=DEV).manual_seed(n + groups)
    mk = lambda: torch.randn(n, device=DEV, generator=gen)
    p, g, m, v = mk(), mk(), mk() * 0.1, mk().abs() * 0.01
    hyper = torch.zeros(16, 8, device=DEV)
    for i in range(groups):   # lr, beta1, beta2, eps, weight decay, grad_scale, max_norm (below the norm: coef < 1)
        hyper[i, :7] = torch.tensor([1e-3 * (i + 1), 0.9, 0.999, 1e-8, 1e-2 * i, 0.5, 0.05], device=DEV)
    group_of = (torch.arange(n // 4, device=DEV) % groups).to(torch.uint8) if groups > 1 else None
    return p, g, m, v, hyper, group_of


def _partials(g):
    from mmfn_amd import ops
    part = torch.zeros(ops.grad_accum_blocks(g.numel()), dtype=torch.float64, device=DEV)
    ops.grad_accum(g, None, ops.ACCUM_NONE, part)
    return part


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("n", [4, 4 * 1021, (1 << 20) + 12])
def test_guarded_kernels_take_a_finite_step_bitwise_and_skip_a_non_finite_one(n, groups):
    from mmfn_amd import ops
    p, g, m, v, hyper, group_of = _flat_case(n, groups)
    scale, max_norm = hyper[0, 5:6], hyper[0, 6:7]
    src = torch.randn(n, device=DEV)

    def guarded(g):
        """The guarded launch sequence on clones: finalize, step count, both gated copies, AdamW."""
        q, mm, vv = p.clone(), m.clone(), v.clone()
        out = torch.zeros(2, device=DEV)
        ok = torch.full((1,), 7, dtype=torch.int32, device=DEV)
        skipped = torch.zeros(1, dtype=torch.int64, device=DEV)
        step = torch.full((1,), 3, dtype=torch.int64, device=DEV)
        on_skip, on_take = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        ops.grad_norm_finalize(_partials(g), scale, max_norm, out[0:1], out[1:2], ok=ok, skipped=skipped)
        ops.step_advance(step, ok=ok)
        ops.copy_if(on_skip, src, ok, when=False)
        ops.copy_if(on_take, src, ok, when=True)
        ops.adamw_groups(q, g, mm, vv, step, hyper, groups, group_of=group_of, coef=out[1:2], ok=ok)
        torch.cuda.synchronize()
        return q, mm, vv, out, int(ok.item()), int(skipped.item()), int(step.item()), on_skip, on_take

    # finite gradient: the plain clipped step, bit for bit
    rp, rm, rv = p.clone(), m.clone(), v.clone()
    rout = torch.zeros(2, device=DEV)
    rstep = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    ops.grad_norm_finalize(_partials(g), scale, max_norm, rout[0:1], rout[1:2])
    ops.step_advance(rstep)
    ops.adamw_groups(rp, g, rm, rv, rstep, hyper, groups, group_of=group_of, coef=rout[1:2])
    q, mm, vv, out, ok, skipped, step, on_skip, on_take = guarded(g)
    assert float(rout[1].item()) < 1.0 and not torch.equal(rp, p)
    assert torch.equal(q, rp) and torch.equal(mm, rm) and torch.equal(vv, rv) and torch.equal(out, rout)
    assert (ok, skipped, step) == (1, 0, 4)
    assert not on_skip.any() and torch.equal(on_take, src)

    # one non-finite gradient element: nothing is touched, the step is counted as skipped
    for bad in (INF, NAN):
        gb = g.clone()
        gb[n // 2 + 1] = bad
        q, mm, vv, out, ok, skipped, step, on_skip, on_take = guarded(gb)
        assert torch.equal(q, p) and torch.equal(mm, m) and torch.equal(vv, v)
        assert (ok, skipped, step) == (0, 1, 3)
        assert not torch.isfinite(out[0]).item()
        assert torch.equal(on_skip, src) and not on_take.any()


def test_guarded_kernels_refuse_null_or_misaligned_arguments():
    from mmfn_amd._lib import lib
    L = lib()
    f = lambda n=64: torch.zeros(n, device=DEV)
    p, g, m, v, hyper, avg = f(), f(), f(), f(), torch.zeros(16, 8, device=DEV), f()
    part = torch.zeros(8, dtype=torch.float64, device=DEV)
    out = f(4)
    ok = torch.ones(2, dtype=torch.int32, device=DEV)
    i64 = torch.zeros(4, dtype=torch.int64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    P = lambda t, byte=0: t.data_ptr() + byte

    fin = lambda **k: L.mmfn_grad_norm_finalize_guard(k.get("part", P(part)), k.get("n", 8), P(out), P(out) + 4, P(out) + 8,
                                                      k.get("coef", P(out) + 12), k.get("ok", P(ok)), k.get("skipped", P(i64)), s)
    assert fin(part=None) == -1 and fin(n=0) == -1 and fin(coef=None) == -1 and fin(ok=None) == -1 and fin(skipped=None) == -1
    assert fin(ok=P(ok, 2)) == -1 and fin(skipped=P(i64, 4)) == -1 and fin(part=P(part, 4)) == -1
    assert fin() == 0

    assert L.mmfn_step_advance_if(None, P(ok), s) == -1 and L.mmfn_step_advance_if(P(i64), None, s) == -1
    assert L.mmfn_step_advance_if(P(i64, 4), P(ok), s) == -1 and L.mmfn_step_advance_if(P(i64), P(ok, 2), s) == -1

    COEF, AVG, GUARD = 1, 2, 4   # the variant bits of mmfn_adamw_groups_f32 (include/mmfn_hip.h)
    adam = lambda **k: L.mmfn_adamw_groups_f32(k.get("p", P(p)), P(g), P(m), P(v), k.get("n", 64), None, P(hyper), 1, P(i64),
                                               COEF | GUARD, k.get("coef", P(out)), None, None, None, 0, k.get("ok", P(ok)), s)
    assert adam(ok=None) == -1 and adam(ok=P(ok, 1)) == -1 and adam(coef=None) == -1 and adam(p=P(p, 4)) == -1 and adam(n=62) == -1
    adam_avg = lambda **k: L.mmfn_adamw_groups_f32(P(p), P(g), P(m), P(v), 64, None, P(hyper), 1, P(i64), COEF | AVG | GUARD, P(out),
                                                   k.get("avg", P(avg)), P(i64, 8), P(out, 4), 0, k.get("ok", P(ok)), s)
    assert adam_avg(ok=None) == -1 and adam_avg(avg=P(avg, 4)) == -1 and adam_avg(avg=None) == -1
    wavg = lambda **k: L.mmfn_weight_average_if_f32(k.get("avg", P(avg)), k.get("src", P(p)), k.get("n", 64), P(i64), P(out), 0,
                                                    k.get("ok", P(ok)), s)
    assert wavg(ok=None) == -1 and wavg(src=P(p, 4)) == -1 and wavg(avg=None) == -1 and wavg(n=6) == -1

    cp = lambda **k: L.mmfn_copy_if(k.get("dst", P(p)), k.get("src", P(g)), k.get("nbytes", 256), k.get("flag", P(ok)), 1, s)
    assert cp(dst=None) == -1 and cp(src=None) == -1 and cp(flag=None) == -1 and cp(dst=P(p, 4)) == -1 and cp(src=P(g, 8)) == -1
    assert cp(nbytes=250) == -1 and cp(flag=P(ok, 2)) == -1 and cp(nbytes=0) == 0

    table = torch.tensor([[0, 64, 0]], dtype=torch.int64, device=DEV)
    ws = torch.zeros(8, dtype=torch.float64, device=DEV)
    st = lambda **k: L.mmfn_tensor_stats_f32(k.get("flat", P(p)), k.get("table", P(table)), k.get("n", 1), k.get("chunks", 1), 1.0,
                                             k.get("out", P(part)), k.get("ws", P(ws)), s)
    assert st(flat=None) == -1 and st(flat=P(p, 4)) == -1 and st(table=None) == -1 and st(table=P(table, 4)) == -1
    assert st(out=None) == -1 and st(out=P(part, 4)) == -1 and st(ws=None) == -1 and st(n=0) == -1 and st(chunks=0) == -1
    assert st() == 0
    torch.cuda.synchronize()


def test_adamw_groups_refuses_variants_without_an_instance_and_a_bad_average():
    from mmfn_amd import ops
    from mmfn_amd._lib import lib
    L = lib()
    f = lambda: torch.zeros(64, device=DEV)
    p, g, m, v, avg, hyper = f(), f(), f(), f(), f(), torch.zeros(16, 8, device=DEV)
    hyper[0, :6] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0])
    step, cnt = torch.ones(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    coef, w = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    ok = torch.ones(1, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    COEF, AVG, GUARD = ops.ADAMW_COEF, ops.ADAMW_AVG, ops.ADAMW_GUARD
    assert (COEF, AVG, GUARD) == (1, 2, 4)

    def adam(variant, mode=ops.AVG_EMA, ema_w=w.data_ptr()):   # every pointer given and legal unless the case withholds it
        return L.mmfn_adamw_groups_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 64, None, hyper.data_ptr(), 1,
                                       step.data_ptr(), variant, coef.data_ptr(), avg.data_ptr(), cnt.data_ptr(), ema_w, mode,
                                       ok.data_ptr(), s)

    for variant in (GUARD, AVG | GUARD, 8, -1):
        assert adam(variant) == -1, variant
    assert adam(COEF | AVG | GUARD, mode=7) == -1
    assert adam(AVG, mode=ops.AVG_EMA, ema_w=None) == -1
    assert adam(AVG, mode=ops.AVG_SWA, ema_w=None) == 0
    for variant in (0, COEF, AVG, COEF | AVG, COEF | GUARD, COEF | AVG | GUARD):   # the six instances that exist
        assert adam(variant) == 0, variant
    torch.cuda.synchronize()


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("n", [4, 4 * 1021])     # one float4 in one lane; a partial last wave
def test_guarded_averaging_adamw_is_the_unguarded_launch_when_ok_and_touches_nothing_otherwise(n, groups):
    from mmfn_amd import ops
    p, g, m, v, hyper, group_of = _flat_case(n, groups)
    a = torch.randn(n, device=DEV)
    step = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    coef, w = torch.tensor([0.37], device=DEV), torch.tensor([0.1], device=DEV)
    flag = {x: torch.full((1,), x, dtype=torch.int32, device=DEV) for x in (0, 1)}

    def run(avg_args, ok):
        q, mm, vv, aa = p.clone(), m.clone(), v.clone(), a.clone()
        ops.adamw_groups(q, g, mm, vv, step, hyper, groups, group_of=group_of, coef=coef, avg=(aa,) + avg_args, ok=ok)
        return q, mm, vv, aa

    for mode in (ops.AVG_EMA, ops.AVG_SWA):
        for k in (0, 2):
            avg_args = (torch.tensor([k], dtype=torch.int64, device=DEV), w, mode)
            ref, taken, skipped = run(avg_args, None), run(avg_args, flag[1]), run(avg_args, flag[0])
            torch.cuda.synchronize()
            assert not torch.equal(ref[0], p) and (torch.equal(ref[3], ref[0]) if k == 0 else not torch.equal(ref[3], ref[0]))
            for x, y in zip(taken, ref):
                assert torch.equal(x, y), (mode, k)
            for x, y in zip(skipped, (p, m, v, a)):
                assert torch.equal(x, y), (mode, k)


# ------------------------------------------------------------------------------------------------ per-tensor statistics
def test_stats_kernel_matches_torch_on_a_synthetic_table():
    from mmfn_amd import ops
    sizes = [1, 2, 3, 4, 5, 64, 4099, (1 << 20) + 4]
    ranges, off = [], 0
    for n in sizes:
        ranges.append((off, n))
        off += (n + 3) // 4 * 4
    gen = torch.Generator(device=DEV).manual_seed(7)
    flat = torch.full((off,), NAN, device=DEV)           # the padding is never read: a NaN there would show
    for o, n in ranges:
        flat[o:o + n] = torch.randn(n, device=DEV, generator=gen) * 3.0
    flat[ranges[4][0] + 2] = -INF
    flat[ranges[6][0] + 4097] = NAN
    tab = ops.tensor_stats_table(ranges, DEV)
    assert tab["n_chunks"] == 6 + 2 + 257
    got = ops.tensor_stats(flat, tab)
    again = ops.tensor_stats(flat, tab)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(sizes), 3)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))       # bit-identical, NaNs included
    for i, (o, n) in enumerate(ranges):
        x = flat[o:o + n].double()
        fin = torch.isfinite(x)
        norm, mx, bad = (float(t) for t in got[i])
        assert bad == float((~fin).sum().item()) and bad == (1.0 if i in (4, 6) else 0.0)
        assert mx == float(x[fin].abs().max().item())
        if bad:
            assert not torch.isfinite(got[i, 0]).item()
        else:
            ref = float(x.pow(2).sum().sqrt().item())
            assert abs(norm - ref) <= 1e-12 * ref
    half = ops.tensor_stats(flat, tab, scale=-0.5)         # the step's grad_scale: norm and max scale, the count does not
    torch.cuda.synchronize()
    ok = [i for i in range(len(sizes)) if i not in (4, 6)]
    assert torch.equal(half[ok, 0], got[ok, 0] * 0.5) and torch.equal(half[:, 1], got[:, 1] * 0.5)
    assert torch.equal(half[:, 2], got[:, 2])


# ------------------------------------------------------------------------------------------------ engine helpers
@functools.lru_cache(maxsize=None)
def _weights():
    from oracle import harness
    return harness.build_oracle("vec", dropout=0.0).state_dict()


def _net(act_dtype="f32"):
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    net = MMFN(GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0, act_dtype=act_dtype), DEV)
    net.load_state_dict(_weights(), strict=True)
    net.train()
    return net


def _inputs(B, seed):
    sys.path.insert(0, ROOT)
    import bench
    return bench.synth_inputs(B, torch.device(DEV), seed=seed, lanes=16, n_lidar=4096)


def _poison(batch, where):
    inp, gt = batch
    inp = dict(inp)
    t = inp[where].clone()
    if where == "target_point":
        t[0, 0] = NAN
    else:
        t[1] = NAN
    inp[where] = t
    return inp, gt


def _state(net):
    L, eng = net._layout, net._engine_for()
    return [L.params, L.exp_avg, L.exp_avg_sq, L.buffers_flat, L.counters_flat, eng.step_count, eng.rng_state]


def _snapshot(net):
    return [t.clone() for t in _state(net)]


def _restore(net, snap):
    for dst, src in zip(_state(net), snap):
        dst.copy_(src)
    torch.cuda.synchronize()


def _same(a, b, rng=True):
    """Bitwise equality of two _state lists (rng=False: all but rng_state, which a skipped step advances)."""
    k = len(a) if rng else len(a) - 1
    return all(torch.equal(x, y) for x, y in zip(a[:k], b[:k]))


def _skipped(eng):
    return int(eng.skipped_steps.item())


def test_tensor_stats_on_the_engine_sum_to_the_global_norm_and_name_the_bad_tensors():
    net = _net()
    eng, L = net._engine_for(), net._layout
    assert eng.skipped_steps is None
    net.guard_nonfinite()
    net.train_step(*_inputs(2, 1))
    names, table = net.tensor_stats("grads")
    torch.cuda.synchronize()
    assert names == [n for n in L.offsets if n not in L.unused] and tuple(table.shape) == (len(names), 3)
    assert _skipped(eng) == 0 and not table[:, 2].any()
    total = float(table[:, 0].pow(2).sum().sqrt().float().item())     # fp64 sums of the same squares, rounded once to fp32
    norm = float(eng.last_grad_norm.item())
    assert abs(total - norm) <= 1e-6 * norm
    _, ptable = net.tensor_stats("params")
    o, n = L.offsets["join.0.bias"]
    assert abs(float(ptable[names.index("join.0.bias"), 0]) - float(L.params[o:o + n].double().norm())) <= 1e-12
    stem = "encoder.image_encoder.features.conv1.weight"
    L.grads[o + n - 1] = INF
    o2, n2 = L.offsets[stem]
    L.grads[o2 + n2 // 2] = NAN
    names, table = eng.tensor_stats("grads")
    flagged = {names[i]: float(table[i, 2]) for i in range(len(names)) if float(table[i, 2]) > 0}
    assert flagged == {"join.0.bias": 1.0, stem: 1.0}
    assert not torch.isfinite(table[names.index(stem), 0]).item()
    with pytest.raises(ValueError):
        eng.tensor_stats("moments")


# ------------------------------------------------------------------------------------------------ the guarded step
@pytest.mark.parametrize("act_dtype", ["f32", "bf16"])
def test_a_clean_guarded_step_is_the_unguarded_step_bitwise(act_dtype):
    net = _net(act_dtype)
    eng = net._engine_for()
    warm, batch = _inputs(2, 1), _inputs(2, 2)
    eng.train_step(*warm, clip_grad_norm=INF)
    snap = _snapshot(net)
    eng.train_step(*batch, clip_grad_norm=INF)
    unclipped = _snapshot(net)
    norm = float(eng.last_grad_norm.item())
    _restore(net, snap)
    eng.train_step(*batch, clip_grad_norm=0.5 * norm)
    clipped = _snapshot(net)
    assert not _same(clipped, unclipped)
    eng.set_nonfinite_guard(True)
    _restore(net, snap)
    eng.train_step(*batch)                                  # no max_norm: measured against inf
    torch.cuda.synchronize()
    assert _same(_state(net), unclipped) and float(eng.last_grad_norm.item()) == norm
    _restore(net, snap)
    eng.train_step(*batch, clip_grad_norm=0.5 * norm)
    torch.cuda.synchronize()
    assert _same(_state(net), clipped)
    assert _skipped(eng) == 0


@pytest.mark.parametrize("where", ["target_point", "velocity"])
@pytest.mark.parametrize("act_dtype", ["f32", "bf16"])
def test_a_non_finite_step_changes_nothing_trained_and_the_run_continues(act_dtype, where):
    net = _net(act_dtype)
    eng, L = net._engine_for(), net._layout
    eng.set_nonfinite_guard(True)
    warm, clean = _inputs(2, 1), _inputs(2, 2)
    bad = _poison(_inputs(2, 3), where)
    eng.train_step(*warm)
    snap = _snapshot(net)
    eng.train_step(*clean)                                   # the clean step from here, before anything non-finite was seen
    want = _snapshot(net)
    _restore(net, snap)
    eng.train_step(*bad)
    torch.cuda.synchronize()
    assert _same(_state(net), snap, rng=False)
    assert _skipped(eng) == 1 and not torch.isfinite(eng.last_grad_norm).item()
    assert not torch.equal(eng.rng_state, snap[-1])           # documented: the RNG advances through a skipped step
    # the run goes on as if the batch had never been seen
    eng.rng_state.copy_(snap[-1])
    eng.train_step(*clean)
    torch.cuda.synchronize()
    assert _same(_state(net), want) and _skipped(eng) == 1
    assert int(eng.step_count.item()) == int(snap[5].item()) + 1
    assert torch.isfinite(L.params).all().item() and torch.isfinite(L.buffers_flat).all().item()
    # control: without the guard one such batch destroys the weights
    eng.set_nonfinite_guard(False)
    _restore(net, snap)
    eng.train_step(*_poison(_inputs(2, 3), "target_point"))
    torch.cuda.synchronize()
    assert not torch.isfinite(L.params[:L.tail]).all().item()


def test_a_poisoned_micro_step_drops_its_whole_accumulation_group():
    nets = [_net(), _net()]
    data = [_inputs(2, 10 + i) for i in range(4)]
    for net in nets:                          # the same eager history on both
        net._engine_for().accumulate_step(*data[0])
        net._engine_for().discard_accumulated()
    ea, eb = nets[0]._engine_for(), nets[1]._engine_for()
    ea.set_nonfinite_guard(True)
    snap = _snapshot(nets[0])
    ea.accumulate_step(*_poison(data[1], "velocity"))
    torch.cuda.synchronize()
    assert not torch.isfinite(nets[0]._layout.buffers_flat).all().item()     # the forward did poison the running statistics
    ea.train_step(*data[2])
    torch.cuda.synchronize()
    assert ea.accum_pending == 0 and not ea.grad_acc.any() and _skipped(ea) == 1
    assert _same(_state(nets[0]), snap, rng=False)         # BatchNorm statistics and counters of the group's start included
    # the next clean group of two, against a net that never saw the poisoned one (unguarded, norm measured)
    ea.accumulate_step(*data[2])
    ea.train_step(*data[3])
    eb.accumulate_step(*data[2])
    eb.train_step(*data[3], clip_grad_norm=INF)
    torch.cuda.synchronize()
    assert _same(_state(nets[0]), _state(nets[1]), rng=False) and _skipped(ea) == 1
    assert int(ea.step_count.item()) == 1


def _avg_state(avg):
    A = avg.module._layout
    return [A.params, A.buffers_flat, A.counters_flat, avg.n_averaged]


@pytest.mark.parametrize("use_buffers", [False, True])
def test_a_skipped_step_leaves_the_attached_average_alone(use_buffers):
    from mmfn_amd.averaging import AveragedMMFN
    nets = [_net(), _net()]
    data = [_inputs(2, 30 + i) for i in range(3)]
    avgs = [AveragedMMFN(n, "ema", decay=0.9, use_buffers=use_buffers) for n in nets]
    for net, avg in zip(nets, avgs):
        net.attach_average(avg)
    ea, eb = nets[0]._engine_for(), nets[1]._engine_for()
    ea.set_nonfinite_guard(True)
    ea.train_step(*data[0])
    eb.train_step(*data[0], clip_grad_norm=INF)
    ea.train_step(*data[1])                                   # (two updates: the second one lerps)
    eb.train_step(*data[1], clip_grad_norm=INF)
    before = [t.clone() for t in _avg_state(avgs[0])]
    ea.train_step(*_poison(data[2], "velocity"))
    torch.cuda.synchronize()
    assert _skipped(ea) == 1 and int(avgs[0].n_averaged.item()) == 2
    assert all(torch.equal(x, y) for x, y in zip(before, _avg_state(avgs[0])))
    ea.train_step(*data[2])
    eb.train_step(*data[2], clip_grad_norm=INF)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(_avg_state(avgs[0]), _avg_state(avgs[1])))
    assert not torch.equal(before[0], avgs[0].module._layout.params) and int(avgs[0].n_averaged.item()) == 3
    assert _same(_state(nets[0]), _state(nets[1]), rng=False)


def test_guarded_graph_replay_equals_eager_bitwise_and_refuses_a_changed_arming(monkeypatch):
    from mmfn_amd.parallel import StaticBatchStep
    data = [_inputs(2, 20 + i) for i in range(4)]
    nets = [_net(), _net()]
    for net in nets:                           # the same eager history on both: sizes the buffers for the captures
        net._engine_for().accumulate_step(*data[0])
        net._engine_for().discard_accumulated()
        net.guard_nonfinite()
    ea, eb = nets[0]._engine_for(), nets[1]._engine_for()
    with pytest.raises(ValueError, match="final"):
        StaticBatchStep(eb, None, data[0][0], data[0][1], 1e-4)          # the plain step has no norm to decide on
    micro = StaticBatchStep(eb, None, data[0][0], data[0][1], 1e-4, variant="micro")
    final = StaticBatchStep(eb, None, data[0][0], data[0][1], 1e-4, variant="final")
    n_graphs = (micro.seg.recorder.n_graphs, final.seg.recorder.n_graphs)
    plan = [data[0], data[1], _poison(data[2], "velocity"), data[3], data[1], data[2]]   # three groups of k = 2
    for j, (inp, gt) in enumerate(plan):
        if j % 2 == 0:
            ea.accumulate_step(inp, gt)
            micro(inp, gt)
        else:
            ea.train_step(inp, gt, lr=2e-4)
            final(inp, gt, lr=2e-4)
            torch.cuda.synchronize()
            assert _skipped(ea) == _skipped(eb) == (0 if j == 1 else 1)
            if j == 3:      # the poisoned group: a NaN norm on both
                assert not torch.isfinite(ea.last_grad_norm).item() and not torch.isfinite(eb.last_grad_norm).item()
            else:
                assert torch.equal(ea.last_grad_norm, eb.last_grad_norm)
    assert (micro.seg.recorder.n_graphs, final.seg.recorder.n_graphs) == n_graphs
    assert _same(_state(nets[0]), _state(nets[1]))
    assert int(eb.step_count.item()) == 2 and torch.isfinite(nets[1]._layout.params).all().item()
    eb.set_nonfinite_guard(False)
    with pytest.raises(RuntimeError, match="guard"):
        final(*data[0])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        ea.set_nonfinite_guard(False)                      # arming or disarming is not a thing a capture can record
    assert ea.nonfinite_guard


# ------------------------------------------------------------------------------------------------ data parallel
def test_two_ranks_skip_together_when_one_rank_sees_a_bad_batch():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", os.path.join(ROOT, "tools", "guard_dp_check.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    for case in ("f32", "bf16"):
        assert ("%s: both ranks skipped True, parameters untouched True, lock step after the next step True" % case) in r.stdout, tail


# ------------------------------------------------------------------------------------------------ trainer
def _store(root, poisoned):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from oracle import fixtures
    samples = fixtures.synthetic_samples((5, 9, 3, 7, 4, 6), seed=3, radar_counts=(50, 81, 81, 20, 60, 81))
    for i, s in enumerate(samples):
        if i in poisoned:
            s["target_point"] = (NAN, s["target_point"][1])
        with open(root / ("%d.pkl" % i), "wb") as fd:
            pickle.dump(s, fd)
    return D.FrameStore(str(root), GlobalConfig(), "train")


def test_trainer_skips_the_poisoned_step_and_stops_when_nothing_is_left(tmp_path_factory, monkeypatch):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import Trainer
    cfg = GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    one_bad = D.make_loader(_store(tmp_path_factory.mktemp("guard_one"), {2}), batch_size=2, num_workers=0)   # 3 batches, the 2nd bad
    net = _net()
    logdir = tmp_path_factory.mktemp("guard_log")
    tr = Trainer(DEV, str(logdir))
    logs = []
    opt = FusedAdamW(net, lr=1e-4)
    tr.train(net, one_bad, cfg, opt, skip_nonfinite=True, log_every=3, on_log=logs.append)
    eng, L = net._engine_for(), net._layout
    assert not eng.nonfinite_guard                            # armed for the epoch only
    assert tr.cur_iter == 3 and int(eng.step_count.item()) == 2 and _skipped(eng) == 1
    assert torch.isfinite(L.params).all().item() and torch.isfinite(L.buffers_flat).all().item()
    assert len(logs) == 1 and logs[0]["skipped_steps"] == 1 and logs[0]["loss"] == logs[0]["loss"]
    assert tr.skipped_steps == 1 and tr.train_loss[-1] == tr.train_loss[-1] and abs(tr.train_loss[-1]) < INF
    from mmfn_amd import trainer as T
    monkeypatch.setattr(T, "_atomic_save", lambda obj, path: None)    # recent.log alone: the weight files are not the subject
    tr.save(net, opt)
    with open(os.path.join(str(logdir), "recent.log")) as f:
        assert json.load(f)["skipped_steps"] == 1

    # control: the same data without the option ends with non-finite weights, and its recent.log has no such key
    ctl = _net()
    ctl_dir = tmp_path_factory.mktemp("guard_ctl")
    ctr = Trainer(DEV, str(ctl_dir))
    copt = FusedAdamW(ctl, lr=1e-4)
    ctr.train(ctl, one_bad, cfg, copt)
    torch.cuda.synchronize()
    assert not torch.isfinite(ctl._layout.params[:ctl._layout.tail]).all().item()
    ctr.save(ctl, copt)
    with open(os.path.join(str(ctl_dir), "recent.log")) as f:
        assert "skipped_steps" not in json.load(f)
    monkeypatch.undo()

    # every sample poisoned: the trainer says which tensors, instead of spinning through the epoch
    all_bad = D.make_loader(_store(tmp_path_factory.mktemp("guard_all"), set(range(6))), batch_size=2, num_workers=0)
    dead = _net()
    with pytest.raises(RuntimeError, match=r"skipped.*(weight|bias)"):
        Trainer(DEV, None).train(dead, all_bad, cfg, FusedAdamW(dead, lr=1e-4), skip_nonfinite=True)
    assert not dead._engine_for().nonfinite_guard and torch.isfinite(dead._layout.params).all().item()
    with pytest.raises(NotImplementedError):
        Trainer(DEV, None).train(dead, all_bad, cfg, FusedAdamW(dead, lr=1e-4), skip_nonfinite=True, fused=False)
