"""Per-tensor AdamW step counts (torch.optim.AdamW's state[p]["step"]): the AdamW launch with step classes against the existing
launch bit for bit and against torch.optim.AdamW, the engine's optimizer step through a freeze / unfreeze schedule, the default
step left as it was, graph replay, the non-finite guard and accumulation, the optimizer checkpoint, the data-parallel broadcast
and fit(unfreeze_at=...).

Bound against torch: max |dp| < 1e-6 at lr 1e-4, the bound of test_adamw_matches_torch (tests/test_kernels_gpu.py): a few fp32
ulps at |p| ~ 3.  One shared step counter misses it by ~4e-5 on the first step of a tensor unfrozen after three steps
(0.42 * lr).  The model-level cases run the B = 2 synthetic vec batch of tests/test_frozen_params_gpu.py with dropout 0."""
import functools
import os
import pickle
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRUNK = "encoder.lidar_encoder."
ONE = "join.0.bias"
NEVER = "encoder.transformer2.pos_emb"     # stays frozen through every schedule below: no optimizer state, as in torch
VARIANTS = {"plain": (False, False, False), "coef": (True, False, False), "coef_avg": (True, True, False),
            "coef_guard_avg": (True, True, True)}


# ------------------------------------------------------------------------------------------------ 1. against the existing launch
def _flat_case(n4, cuts):
    """n4 float4s cut at `cuts` (float4 indices) into spans of (hyper group, step class or None = frozen)."""
    from mmfn_amd import ops
    n = 4 * n4
    gen = torch.Generator(device=DEV).manual_seed(77 + n4)
    mk = lambda: torch.randn(n, device=DEV, generator=gen)
    bufs = dict(p=mk(), g=mk(), m=mk() * 0.1, v=mk().abs() * 0.01, a=mk())
    hyper = torch.zeros(16, 8, device=DEV)
    for i in range(2):   # lr, beta1, beta2, eps, weight decay, grad_scale
        hyper[i, :6] = torch.tensor([1e-3 * (i + 1), 0.9 - 0.05 * i, 0.999 - 0.009 * i, 1e-8, 1e-2 * (i + 1), 0.5], device=DEV)
    rows, row_of = [], torch.full((n4,), ops.ADAMW_FROZEN, dtype=torch.uint8)
    group_of, class_of = torch.zeros(n4, dtype=torch.uint8), torch.full((n4,), -1, dtype=torch.int64)
    for (b, e), (grp, cls) in cuts:
        if cls is None:
            continue
        if (grp, cls) not in rows:
            rows.append((grp, cls))
        row_of[b:e] = rows.index((grp, cls))
        group_of[b:e] = grp
        class_of[b:e] = cls
    return bufs, hyper, torch.tensor(rows, dtype=torch.int32), row_of.to(DEV), group_of, class_of


def _run_rows_against_groups(n4, cuts, variant):
    """The launch with step classes once, against mmfn_adamw_groups_f32 once per class on clones (every other class masked 255,
    step = that class's count): p, m, v - and the average - bit for bit; with ok = 0 nothing moves."""
    from mmfn_amd import ops
    counts = (1, 4, 9)
    bufs, hyper, rows, row_of, group_of, class_of = _flat_case(n4, cuts)
    n = 4 * n4
    with_coef, with_avg, with_guard = VARIANTS[variant]
    coef = torch.tensor([0.37], device=DEV) if with_coef else None
    cnt, w = torch.tensor([2], dtype=torch.int64, device=DEV), torch.tensor([0.1], device=DEV)
    class_steps = torch.tensor(counts + (123,), dtype=torch.int64, device=DEV)
    for okv in ((1, 0) if with_guard else (None,)):
        ok = None if okv is None else torch.full((1,), okv, dtype=torch.int32, device=DEV)
        got = {k: t.clone() for k, t in bufs.items()}
        ops.adamw_rows(got["p"], got["g"], got["m"], got["v"], class_steps, 3, hyper, 2, row_of, rows, coef=coef,
                       avg=(got["a"], cnt, w, ops.AVG_EMA) if with_avg else None, ok=ok)
        want = {k: t.clone() for k, t in bufs.items()}
        for c, t in enumerate(counts):
            if okv == 0:
                break
            table = torch.where(class_of == c, group_of, torch.full_like(group_of, ops.ADAMW_FROZEN)).to(DEV)
            ref = {k: x.clone() for k, x in bufs.items()}
            ops.adamw_groups(ref["p"], ref["g"], ref["m"], ref["v"], torch.tensor([t], dtype=torch.int64, device=DEV), hyper, 2,
                             group_of=table, coef=coef, avg=(ref["a"], cnt, w, ops.AVG_EMA) if with_avg else None, ok=ok, mask=True)
            mine = (class_of == c).repeat_interleave(4).to(DEV)
            assert bool(mine.any())
            for k in ("p", "m", "v", "a"):
                want[k][mine] = ref[k][mine]
            if with_avg and c == 0:     # the average follows the frozen float4s too: the same in every yardstick run
                cold = (class_of < 0).repeat_interleave(4).to(DEV)
                want["a"][cold] = ref["a"][cold]
        torch.cuda.synchronize()
        for k in ("p", "m", "v", "a", "g"):
            assert torch.equal(got[k], want[k]), (variant, okv, k)
        if okv != 0:
            live = (class_of >= 0).repeat_interleave(4).to(DEV)
            assert not torch.equal(got["p"][live], bufs["p"][live]) and torch.equal(got["p"][~live], bufs["p"][~live])
        assert class_steps.tolist() == list(counts) + [123]      # the launch reads the counters


# 4 * (3 * 256 + 5) floats: three tensors cut at float4s that are no multiples of 256 (the first in two optimizer groups: rows
# are (group, class) pairs, not classes), then a frozen span
SMALL = (3 * 256 + 5, [((0, 100), (0, 0)), ((100, 259), (1, 0)), ((259, 517), (1, 1)), ((517, 700), (0, 2)), ((700, 773), (0, None))])
# 4 * (4096 * 256 + 37) floats: the grid-stride loop (4096 workgroups of 256) takes a second trip, over a stepping span
BIG_N4 = 4096 * 256 + 37
BIG = (BIG_N4, [((0, 300001), (0, 0)), ((300001, 300050), (0, None)), ((300050, 4096 * 256 - 3), (1, 1)),
                ((4096 * 256 - 3, BIG_N4), (0, 2))])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_rows_launch_equals_the_groups_launch_per_class_bitwise(variant):
    assert 4 * SMALL[0] == 4 * (3 * 256 + 5)
    _run_rows_against_groups(SMALL[0], SMALL[1], variant)


def test_rows_launch_equals_the_groups_launch_past_the_first_grid_trip():
    _run_rows_against_groups(BIG[0], BIG[1], "coef_guard_avg")


def test_class_counters_advance_behind_the_active_bytes_and_the_flag():
    from mmfn_amd import ops
    from mmfn_amd._lib import lib
    n = 300       # more than one workgroup of 256
    steps = torch.arange(n, dtype=torch.int64, device=DEV) * 3
    active = (torch.arange(n, device=DEV) % 3 != 1).to(torch.uint8)
    want = steps.clone()
    ok0, ok1 = (torch.full((1,), x, dtype=torch.int32, device=DEV) for x in (0, 1))
    ops.class_steps_advance(steps, active, n, ok=ok0)
    torch.cuda.synchronize()
    assert torch.equal(steps, want)                                # a skipped step: no counter moves
    ops.class_steps_advance(steps, active, n, ok=ok1)
    ops.class_steps_advance(steps, active, n - 1)
    torch.cuda.synchronize()
    want += 2 * active.to(torch.int64)
    want[n - 1] -= int(active[n - 1])
    assert torch.equal(steps, want)
    # the entry points refuse what they would dereference
    s = torch.cuda.current_stream().cuda_stream
    assert lib().mmfn_class_steps_advance(None, active.data_ptr(), n, None, s) == -1
    assert lib().mmfn_class_steps_advance(steps.data_ptr(), None, n, None, s) == -1
    assert lib().mmfn_class_steps_advance(steps.data_ptr(), active.data_ptr(), 0, None, s) == -1
    bufs, hyper, rows, row_of, _, _ = _flat_case(SMALL[0], SMALL[1])
    p, g, m, v = (bufs[k] for k in "pgmv")
    cs = torch.ones(3, dtype=torch.int64, device=DEV)

    def call(**kw):
        a = dict(p=p.data_ptr(), g=g.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), n=p.numel(), row_of=row_of.data_ptr(),
                 hyper=hyper.data_ptr(), n_groups=2, rows=rows.data_ptr(), n_rows=rows.shape[0], cs=cs.data_ptr(), n_classes=3, variant=0)
        a.update(kw)
        return lib().mmfn_adamw_rows_f32(a["p"], a["g"], a["m"], a["v"], a["n"], a["row_of"], a["hyper"], a["n_groups"], a["rows"],
                                         a["n_rows"], a["cs"], a["n_classes"], a["variant"], None, None, None, None, 0, None, s)
    for bad in (dict(p=None), dict(g=None), dict(row_of=None), dict(hyper=None), dict(rows=None), dict(cs=None), dict(n_rows=0),
                dict(n_rows=255), dict(n_classes=2), dict(n_groups=1), dict(n_groups=17), dict(variant=4), dict(variant=8),
                dict(variant=1), dict(n=p.numel() - 2), dict(p=p.data_ptr() + 4)):
        assert call(**bad) == -1, bad
    with pytest.raises(ValueError, match="255"):
        ops.adamw_rows(p, g, m, v, cs, 3, hyper, 2, row_of, torch.zeros(255, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.adamw_rows(p, g, m, v, cs, 3, hyper, 2, row_of[:100], rows)
    torch.cuda.synchronize()
    assert torch.equal(p, _flat_case(SMALL[0], SMALL[1])[0]["p"])      # no refused call launched anything


# ------------------------------------------------------------------------------------------------ 2. against torch
def test_rows_launch_matches_torch_adamw_with_tensors_sitting_out():
    """Three tensors, six steps; B sits out steps 1-3, C sits out steps 3-4 after taking part in steps 1-2: torch.optim.AdamW on
    the CPU with grad = None on those steps keeps a step count per tensor, and so do the class counters.

    The bound is test_adamw_matches_torch's 1e-6.  Two fp32 evaluation orders of p * decay - step_size * m / denom (the kernel's,
    which is the existing kernel's bit for bit, and ATen's mul_ then addcdiv_) may round p differently by one ulp of p per step,
    and the differences add up over the steps a tensor takes: 3 steps at |p| < 4 there (3 * 2.4e-7), up to 6 steps here, so the
    parameters are drawn from (-1.5, 1.5), where one ulp is 1.2e-7 and six of them stay under the bound.  (Measured with
    parameters from randn, |p| up to 3.4: 2.4e-7, 4.8e-7, 7.2e-7, 9.5e-7, 9.5e-7, 1.19e-6 after steps 1 .. 6 - one ulp of
    [2, 4) per step, the sixth step past 1e-6.)  A shared counter is off by 4.2e-5 on B's first step."""
    from mmfn_amd import ops
    sizes = (1000, 1036, 1012)
    offs = (0, 1000, 2036)
    n = sum(sizes)
    gen = torch.Generator().manual_seed(11)
    p0 = torch.rand(n, generator=gen) * 3.0 - 1.5
    grads = [torch.randn(n, generator=gen) for _ in range(6)]
    out = {"B": (1, 2, 3), "C": (3, 4)}
    refs = [torch.nn.Parameter(p0[o:o + k].clone()) for o, k in zip(offs, sizes)]
    opt = torch.optim.AdamW(refs, lr=1e-4)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    hyper = torch.zeros(16, 8, device=DEV)
    hyper[0, :6] = torch.tensor([1e-4, 0.9, 0.999, 1e-8, 1e-2, 1.0], device=DEV)
    class_steps = torch.zeros(3, dtype=torch.int64, device=DEV)
    rows = torch.tensor([[0, 0], [0, 1], [0, 2]], dtype=torch.int32)
    worst = 0.0
    for step in range(1, 7):
        sits = [False, step in out["B"], step in out["C"]]
        row_of = torch.cat([torch.full((k // 4,), 255 if s else c, dtype=torch.uint8) for c, (k, s) in enumerate(zip(sizes, sits))])
        active = torch.tensor([0 if s else 1 for s in sits], dtype=torch.uint8, device=DEV)
        g = grads[step - 1]
        for r, o, k, s in zip(refs, offs, sizes, sits):
            r.grad = None if s else g[o:o + k].clone()
        opt.step()
        ops.class_steps_advance(class_steps, active, 3)
        ops.adamw_rows(p, g.to(DEV), m, v, class_steps, 3, hyper, 1, row_of.to(DEV), rows)
        err = (p.cpu() - torch.cat([r.detach() for r in refs])).abs().max().item()
        worst = max(worst, err)
        print("step %d: max |dp| vs torch %.3g" % (step, err))
        assert err < 1e-6, (step, err)
    assert class_steps.tolist() == [6, 3, 4] == [int(opt.state[r]["step"]) for r in refs]


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
    return [L.params, L.exp_avg, L.exp_avg_sq, L.buffers_flat, L.counters_flat, eng.step_count, eng.rng_state]


def _steps(net):
    eng = net._engine_for()
    return dict(zip(eng.classes.names, eng.tensor_steps().tolist()))


def _expect_steps(net, late, early, never=0):
    """Every trained tensor's count: `late` for the trunk and the bias unfrozen late, `never` for NEVER, `early` for the rest."""
    got = _steps(net)
    for n, t in got.items():
        want = never if n == NEVER else (late if n.startswith(TRUNK) or n == ONE else early)
        assert t == want, (n, t, want)
    assert sum(n.startswith(TRUNK) for n in got) > 50 and ONE in got and NEVER in got


class _TorchTwin(object):
    """torch.optim.AdamW on CPU clones of the model's parameters (checkpoint shapes, named_parameters() order), fed the flat
    gradient buffer through the layout's checkpoint-shaped views; a frozen or never-trained parameter gets grad = None."""

    def __init__(self, net, lr=1e-4):
        self.net, self.names = net, [n for n, _ in net.named_parameters()]
        self.params = [torch.nn.Parameter(p.detach().cpu().clone()) for p in net.parameters()]
        self.opt = torch.optim.AdamW(self.params, lr=lr)

    def step(self):
        L = self.net._layout
        frozen = set(L.frozen_names())
        for n, r in zip(self.names, self.params):
            r.grad = None if (n in L.unused or n in frozen) else L.grad_views[n].detach().cpu().clone()
        self.opt.step()

    def worst(self):
        got = dict(self.net.named_parameters())
        return max((got[n].detach().cpu() - r.detach()).abs().max().item() for n, r in zip(self.names, self.params))

    def steps(self):
        return {n: int(self.opt.state[r]["step"]) if r in self.opt.state else 0 for n, r in zip(self.names, self.params)}


def _random_grads(net, gen):
    eng, L = net._engine_for(), net._layout
    eng.trainable_mask()        # (new flags zero the frozen gradient ranges: before the gradients are written)
    L.grads[:L.tail].normal_(generator=gen).mul_(0.01)


@pytest.fixture(scope="module")
def schedule():
    """The optimizer alone through a gradual-unfreezing schedule on seeded random gradients: the lidar trunk and join.0.bias
    frozen for two steps, then trained for two; one tensor frozen throughout.  Beside it torch.optim.AdamW on the CPU."""
    net = _net()
    eng = net._engine_for()
    twin = _TorchTwin(net)
    gen = torch.Generator(device=DEV).manual_seed(2024)
    net.freeze(TRUNK, ONE, NEVER)
    errs = []
    for i in range(4):
        if i == 2:
            net.unfreeze(TRUNK, ONE)
        _random_grads(net, gen)
        twin.step()
        eng.optimizer_step(lr=1e-4)
        torch.cuda.synchronize()
        errs.append(twin.worst())
    return net, twin, errs, _steps(net), twin.steps()


# ------------------------------------------------------------------------------------------------ 3. the engine's optimizer step
def test_engine_steps_match_torch_through_freeze_and_unfreeze(schedule):
    net, twin, errs, got, want = schedule    # (the counts as the schedule left them: a later test steps this model further)
    print("max |dp| vs torch per step: " + ", ".join("%.3g" % e for e in errs))
    assert all(e < 1e-6 for e in errs), errs
    for n, t in got.items():
        assert t == (0 if n == NEVER else (2 if n.startswith(TRUNK) or n == ONE else 4)), (n, t)
    assert sum(n.startswith(TRUNK) for n in got) > 50 and ONE in got and NEVER in got
    assert all(got[n] == want[n] for n in got)            # torch's state[p]["step"]


# ------------------------------------------------------------------------------------------------ 4. the default path
class _LaunchLog(object):
    """Stands in for the ctypes handle: notes the name of every entry point that takes a stream, then makes the call."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        import ctypes
        from mmfn_amd import _lib
        fn = getattr(self._real, name)
        sig = _lib._SIGNATURES.get(name)
        if sig is None or not sig[1] or sig[1][-1] is not ctypes.c_void_p:
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def test_nothing_frozen_launches_what_it_always_launched(monkeypatch):
    from mmfn_amd import _lib
    inp, gt = _inputs()
    plain, told = _net(), _net()
    eng = told._engine_for()
    eng.set_tensor_steps([0] * len(eng.classes.names))          # one common value: still one class on the shared counter
    assert eng.classes.n_classes == 1 and eng.classes.uniform()
    for _ in range(3):
        plain.train_step(inp, gt, lr=1e-3)
    log = _LaunchLog(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", log)
    for i in range(3):
        del log.calls[:]
        told.train_step(inp, gt, lr=1e-3)
        assert log.calls.count("mmfn_adamw_groups_f32") == 1 and log.calls[-1] == "mmfn_adamw_groups_f32", i
        assert log.calls.count("mmfn_step_advance") == 1
        assert "mmfn_adamw_rows_f32" not in log.calls and "mmfn_class_steps_advance" not in log.calls
    torch.cuda.synchronize()
    for a, b in zip(_state(plain), _state(told)):
        assert torch.equal(a, b)
    assert set(_steps(told).values()) == {3}
    # frozen tensors that stay frozen: still the masked instance of the existing entry point
    told.freeze(TRUNK)
    del log.calls[:]
    told.train_step(inp, gt, lr=1e-3)
    assert log.calls[-1] == "mmfn_adamw_groups_f32" and "mmfn_adamw_rows_f32" not in log.calls
    # ... and once they train again with a count of their own, the launch with step classes and its counter advance
    told.unfreeze(TRUNK)
    del log.calls[:]
    told.train_step(inp, gt, lr=1e-3)
    assert log.calls[-1] == "mmfn_adamw_rows_f32" and log.calls.count("mmfn_class_steps_advance") == 1
    assert "mmfn_adamw_groups_f32" not in log.calls and log.calls.count("mmfn_step_advance") == 1
    torch.cuda.synchronize()
    assert {(n.startswith(TRUNK), t) for n, t in _steps(told).items()} == {(True, 4), (False, 5)}


# ------------------------------------------------------------------------------------------------ 5. replay, guard, accumulation
def test_replay_equals_eager_and_guard_and_accumulation_move_no_counter():
    from mmfn_amd.parallel import GraphedStep
    inp, gt = _inputs()
    eager, graphed = _net(), _net()
    for net in (eager, graphed):
        net.freeze(TRUNK, ONE, NEVER)
    eng = graphed._engine_for()
    first = GraphedStep(eng, None, inp, gt, lr=1e-3, warm=1)        # one eager warm-up step + one replay
    first()
    graphed.unfreeze(TRUNK, ONE)
    with pytest.raises(RuntimeError, match="requires_grad"):
        first()
    again = GraphedStep(eng, None, inp, gt, lr=1e-3, warm=1)        # captured again: the launch with step classes
    again()
    for i in range(4):
        if i == 2:
            eager.unfreeze(TRUNK, ONE)
        eager.train_step(inp, gt, lr=1e-3)
    torch.cuda.synchronize()
    for a, b in zip(_state(eager), _state(graphed)):
        assert torch.equal(a, b)
    _expect_steps(eager, late=2, early=4)
    _expect_steps(graphed, late=2, early=4)
    # a replay after the counts were set by hand is refused: the capture holds the classes of its moment
    eng.set_tensor_steps([1] * len(eng.classes.names))
    with pytest.raises(RuntimeError, match="step counts"):
        again()
    # the guard: a step whose input is not finite moves no counter, no parameter, no moment
    eager.guard_nonfinite(True)
    e = eager._engine_for()
    assert not e.classes.uniform()
    before = [t.clone() for t in _state(eager)]
    steps_before = e.tensor_steps()
    image = torch.rand(2, 3, 256, 256, device=DEV) * 255.0
    image[1, 2, 100, 7] = float("nan")
    bad = {k: v for k, v in inp.items() if k != "rgb_u8"}
    bad["image"] = image
    eager.train_step(bad, gt, lr=1e-3)
    torch.cuda.synchronize()
    assert int(e.skipped_steps.item()) == 1
    for now, was in zip(_state(eager)[:-1], before[:-1]):              # (rng_state advances either way)
        assert torch.equal(now, was)
    assert torch.equal(e.tensor_steps(), steps_before)
    # accumulation micro-steps move no counter; the guarded step that closes the group moves every one that steps
    eager.accumulate_step(inp, gt)
    torch.cuda.synchronize()
    assert torch.equal(e.tensor_steps(), steps_before) and int(e.step_count.item()) == 4
    eager.train_step(inp, gt, lr=1e-3)
    torch.cuda.synchronize()
    assert int(e.skipped_steps.item()) == 1
    _expect_steps(eager, late=3, early=5)
    assert not torch.equal(_state(eager)[0], before[0])


# ------------------------------------------------------------------------------------------------ 6. checkpoints
def test_checkpoint_carries_the_counts_and_a_torch_checkpoint_with_differing_counts_loads(schedule):
    from mmfn_amd.optim import FusedAdamW
    net, twin = schedule[:2]
    L, eng = net._layout, net._engine_for()
    assert int(eng.step_count.item()) == 4
    names = twin.names
    sd = FusedAdamW(net, lr=1e-4).state_dict()
    for idx, n in enumerate(names):
        want = None if (n in L.unused or n == NEVER) else (2 if n.startswith(TRUNK) or n == ONE else 4)
        assert (float(sd["state"][idx]["step"]) if idx in sd["state"] else None) == want, n
    ref = torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu().clone()) for p in net.parameters()], lr=1e-4)
    ref.load_state_dict(sd)
    assert sorted({int(s["step"]) for s in ref.state.values()}) == [2, 4] and len(ref.state) == len(sd["state"])
    # torch's own state dict of the same run, differing counts and all, into a fresh FusedAdamW over scrambled engine state
    tsd = twin.opt.state_dict()
    assert sorted({int(s["step"]) for s in tsd["state"].values()}) == [2, 4]
    eng.set_tensor_steps([7] * len(eng.classes.names), step_count=7)
    L.exp_avg.fill_(0.5)
    L.exp_avg_sq.fill_(0.5)
    opt = FusedAdamW(net, lr=1e-4)
    opt.load_state_dict(tsd)                                           # (differing counts used to raise)
    _expect_steps(net, late=2, early=4)
    assert int(eng.step_count.item()) == 4
    mine = dict(net.named_parameters())
    for n, r in zip(names, twin.params):                               # (the parameters of the twin, to the last bit)
        mine[n].data.copy_(r.detach())
    # the next step on fixed gradients, everything trainable: NEVER takes its first step, the others their third and fifth
    net.unfreeze(NEVER)
    _random_grads(net, torch.Generator(device=DEV).manual_seed(5))
    twin.step()
    opt.step()
    torch.cuda.synchronize()
    err = twin.worst()
    print("max |dp| vs torch on the step after the load: %.3g" % err)
    assert err < 1e-6
    _expect_steps(net, late=3, early=5, never=1)
    got, want = _steps(net), twin.steps()
    assert all(got[n] == want[n] for n in got)


# ------------------------------------------------------------------------------------------------ data-parallel broadcast
class _Wire(object):
    """torch.distributed stand-in that carries rank 0's broadcasts to rank 1 inside one process: rank 0 records every tensor it
    broadcasts, rank 1 receives them in the same order."""

    def __init__(self, rank, sent):
        self.rank, self.sent = rank, sent

    def get_world_size(self):
        return 2

    def get_rank(self):
        return self.rank

    def broadcast(self, t, src):
        if self.rank == src:
            self.sent.append(t.detach().clone())
        else:
            t.copy_(self.sent.pop(0))


def test_broadcast_parameters_carries_the_per_tensor_counts(schedule):
    from mmfn_amd.parallel import DataParallel
    src = schedule[0]
    dst = _net()
    sent = []
    want = src._engine_for().tensor_steps()
    assert len(set(want.tolist())) >= 2
    DataParallel(src, _Wire(0, sent)).broadcast_parameters()
    DataParallel(dst, _Wire(1, sent)).broadcast_parameters()
    torch.cuda.synchronize()
    assert not sent
    assert torch.equal(dst._engine_for().tensor_steps(), want) and torch.equal(src._engine_for().tensor_steps(), want)
    assert torch.equal(dst._engine_for().step_count, src._engine_for().step_count)
    for a, b in zip(_state(src)[:3], _state(dst)[:3]):
        assert torch.equal(a, b)
    assert not dst._engine_for().classes.uniform()


# ------------------------------------------------------------------------------------------------ 7. the trainer
@pytest.fixture(scope="module")
def store(tmp_path_factory):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from oracle import fixtures
    root = tmp_path_factory.mktemp("unfreeze_train")
    for i, s in enumerate(fixtures.synthetic_samples((5, 9, 3, 7), seed=3)):
        with open(root / ("%d.pkl" % i), "wb") as fd:
            pickle.dump(s, fd)
    return D.FrameStore(str(root), GlobalConfig(), "train")


def test_fit_unfreezes_at_the_epoch_and_a_resumed_run_follows_the_schedule(store, tmp_path):
    from mmfn_amd import data as D
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import fit
    loader = D.make_loader(store, batch_size=2, num_workers=0)       # 4 samples: two optimizer steps per epoch
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    trunk = lambda net: torch.cat([p.detach().flatten() for n, p in net.named_parameters() if n.startswith(TRUNK)])

    def run(logdir, epochs, val=True):
        net = _net()
        net.freeze(TRUNK)                                            # the initial frozen set is the caller's
        init = trunk(net).clone()
        fit(net, FusedAdamW(net, lr=1e-4), loader, loader if val else None, cfg, logdir, epochs, unfreeze_at={1: [TRUNK]})
        torch.cuda.synchronize()
        return net, init

    def counts(net):
        return {(n.startswith(TRUNK), t) for n, t in _steps(net).items()}

    log_a, log_b = str(tmp_path / "a"), str(tmp_path / "b")
    net, init = run(log_a, 1)
    assert torch.equal(trunk(net), init)                             # epoch 0: frozen, bit-unchanged
    assert counts(net) == {(True, 0), (False, 2)} and net.trainable_names() != [n for n, _ in net.named_parameters()]
    resumed, init = run(log_a, 2)                                    # a fresh process resumes into epoch 1
    assert not torch.equal(trunk(resumed), init)                     # epoch 1: trained
    assert counts(resumed) == {(True, 2), (False, 4)}                  # the trunk's count is epoch 1's step count
    assert resumed.trainable_names() == [n for n, _ in resumed.named_parameters()]
    whole, _ = run(log_b, 2, val=False)                              # the same two epochs without the interruption (or a save)
    assert counts(whole) == {(True, 2), (False, 4)}
    sa, sb = whole.state_dict(), resumed.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    with pytest.raises(ValueError, match="no parameter name starts with"):
        fit(whole, None, loader, None, cfg, str(tmp_path / "c"), 2, unfreeze_at={1: ["encoder.no_such_module."]})
