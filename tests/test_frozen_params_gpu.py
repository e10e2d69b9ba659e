"""Frozen parameters (requires_grad = False) in the fused training step: the masked AdamW kernel and fill_ranges on flat arrays,
frozen tensors that keep their bits through every kind of step, gradients of the trainable tensors that keep theirs, backward
work that is really not issued, norm / clipping / accumulation / guard over trainable tensors only, the weight average,
graph replay, the readiness hooks, the autograd path and the optimizer's checkpoint.

Every step case runs B = 2 synthetic inputs (bench.synth_inputs(2, DEV, seed=42, variant=...)) with dropout 0; the oracle and
autograd cases need the reference's forward() arguments and take the oracle's synthetic batch of the same size."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRUNKS = ("encoder.image_encoder.", "encoder.lidar_encoder.", "encoder.img_map_encoder.", "encoder.vectornet_encoder.")
HEAD = ("join.", "decoder.", "output.")
SCATTER = ("encoder.transformer1.blocks.0.attn.key.weight", "encoder.transformer1.blocks.0.ln1.weight",
           "encoder.transformer4.blocks.0.mlp.0.bias", "encoder.transformer2.pos_emb",
           "encoder.image_encoder.features.layer2.0.bn1.weight", "encoder.lidar_encoder._model.layer3.1.conv2.weight")


# ------------------------------------------------------------------------------------------------ 1. the kernels on flat arrays
def _flat_case(n, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(1000 + n + seed)
    mk = lambda: torch.randn(n, device=DEV, generator=gen)
    p, g, m, v, a = mk(), mk(), mk() * 0.1, mk().abs() * 0.01, mk()
    hyper = torch.zeros(16, 8, device=DEV)
    for i in range(2):   # lr, beta1, beta2, eps, weight decay, grad_scale
        hyper[i, :6] = torch.tensor([1e-3 * (i + 1), 0.9, 0.999, 1e-8, 1e-2 * (i + 1), 0.5], device=DEV)
    return p, g, m, v, a, hyper


@pytest.mark.parametrize("variant", ["plain", "coef", "avg", "coef_avg", "coef_guard", "coef_avg_guard"])
@pytest.mark.parametrize("n,table", [(4096, "mixed"), (4, "frozen"), (4, "live")])
def test_masked_adamw_leaves_frozen_float4s_alone_and_steps_the_others_bitwise(n, table, variant):
    from mmfn_amd import ops
    p, g, m, v, a, hyper = _flat_case(n)
    n4 = n // 4
    if table == "mixed":      # 0, 1, 255, 0, 1, 255, ...: every float4 differs from both neighbours
        gid = torch.tensor([0, 1, 255], dtype=torch.uint8, device=DEV).repeat((n4 + 2) // 3)[:n4].contiguous()
    else:
        gid = torch.full((n4,), 255 if table == "frozen" else 1, dtype=torch.uint8, device=DEV)
    ref_gid = torch.where(gid == 255, torch.zeros_like(gid), gid)   # the launch without MASK needs a legal id everywhere
    frozen = (gid == 255).repeat_interleave(4)
    step = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    coef = torch.tensor([0.37], device=DEV) if "coef" in variant else None
    w = torch.tensor([0.1], device=DEV)
    flags = [torch.full((1,), x, dtype=torch.int32, device=DEV) for x in (1, 0)] if "guard" in variant else [None]
    cases = [(mode, k) for mode in (ops.AVG_EMA, ops.AVG_SWA) for k in (0, 2)] if "avg" in variant else [(None, None)]
    for mode, k in cases:
        cnt = None if mode is None else torch.tensor([k], dtype=torch.int64, device=DEV)
        for ok in flags:
            def run(table, mask):
                q, mm, vv, aa = p.clone(), m.clone(), v.clone(), a.clone()
                ops.adamw_groups(q, g, mm, vv, step, hyper, 2, group_of=table, coef=coef,
                                 avg=None if mode is None else (aa, cnt, w, mode), ok=ok, mask=mask)
                return q, mm, vv, aa
            got, ref = run(gid, True), run(ref_gid, False)
            lerped = a.clone()
            if mode is not None:
                ops.weight_average(lerped, p, cnt, w, mode)   # the standalone launch over the OLD parameters
            torch.cuda.synchronize()
            what = (variant, mode, k, None if ok is None else int(ok.item()))
            if ok is not None and int(ok.item()) == 0:   # a skipped step touches nothing, frozen or not
                for x, y in zip(got, (p, m, v, a)):
                    assert torch.equal(x, y), what
                continue
            if table != "frozen":
                assert not torch.equal(ref[0], p), what
            for x, y, init in zip(got[:3], ref[:3], (p, m, v)):
                assert torch.equal(x[frozen], init[frozen]), what          # parameter and moments keep their bits
                assert torch.equal(x[~frozen], y[~frozen]), what           # everything else: the launch without MASK
            if mode is None:
                assert torch.equal(got[3], a), what
            else:
                assert torch.equal(got[3][frozen], lerped[frozen]), what   # the average still follows a frozen parameter
                assert torch.equal(got[3][~frozen], ref[3][~frozen]), what


def test_masked_adamw_needs_a_table():
    from mmfn_amd import ops
    from mmfn_amd._lib import lib
    p, g, m, v, a, hyper = _flat_case(64)
    step = torch.ones(1, dtype=torch.int64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert (ops.ADAMW_MASK, ops.ADAMW_FROZEN) == (8, 255)
    gid = torch.zeros(16, dtype=torch.uint8, device=DEV)
    call = lambda variant, table: lib().mmfn_adamw_groups_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 64, table,
                                                              hyper.data_ptr(), 1, step.data_ptr(), variant, None, None, None, None,
                                                              0, None, s)
    assert call(ops.ADAMW_MASK, None) == -1 and call(ops.ADAMW_MASK | ops.ADAMW_GUARD, gid.data_ptr()) == -1 and call(16, gid.data_ptr()) == -1
    assert call(ops.ADAMW_MASK, gid.data_ptr()) == 0
    with pytest.raises(ValueError):
        ops.adamw_groups(p, g, m, v, step, hyper, 1, group_of=None, mask=True)
    with pytest.raises(ValueError):
        ops.adamw_groups(p, g, m, v, step, hyper, 1, group_of=gid[:8], mask=True)
    torch.cuda.synchronize()


def test_fill_ranges_writes_exactly_its_ranges():
    from mmfn_amd import ops
    # a range of 4 floats, two adjacent ranges (the second longer than one chunk of 4096), a range that ends one chunk exactly
    ranges = [(4, 4), (16, 8), (24, 4100), (4200, 4096), (8300, 12)]
    total = 8320
    gen = torch.Generator(device=DEV).manual_seed(5)
    flat = torch.randn(total, device=DEV, generator=gen) + 3.0
    init = flat.clone()
    tab = ops.fill_ranges_table(ranges, DEV)
    assert tab["n_chunks"] == 1 + 1 + 2 + 1 + 1 and tab["limit"] == 8312
    inside = torch.zeros(total, dtype=torch.bool, device=DEV)
    for off, n in ranges:
        inside[off:off + n] = True
    for off, n in ((4, 4), (16, 4108), (4200, 4096), (8300, 12)):   # a guard float on each side of each (merged) range
        assert not inside[off - 1] and not inside[off + n]
    ops.fill_ranges(flat, tab, 0.0)
    torch.cuda.synchronize()
    assert not flat[inside].any() and not torch.signbit(flat[inside]).any()    # +0.0
    assert torch.equal(flat[~inside], init[~inside])
    ops.fill_ranges(flat, tab, 2.5)
    torch.cuda.synchronize()
    assert bool((flat[inside] == 2.5).all()) and torch.equal(flat[~inside], init[~inside])
    with pytest.raises(ValueError):
        ops.fill_ranges_table([(0, 6)], DEV)              # not whole float4s
    with pytest.raises(ValueError):
        ops.fill_ranges_table([(0, 8), (4, 8)], DEV)      # overlap
    with pytest.raises(ValueError):
        ops.fill_ranges(flat[:8000], tab)                 # the table reaches past the buffer


# ------------------------------------------------------------------------------------------------ engine helpers
@functools.lru_cache(maxsize=None)
def _weights(variant):
    from oracle import harness
    return harness.build_oracle(variant, dropout=0.0).state_dict()


def _net(variant="vec", act_dtype="f32"):
    from mmfn_amd.config import GlobalConfig
    import mmfn_amd.model as M
    cls = {"vec": M.MMFN, "img": M.MMFNImg, "rad": M.MMFNRad}[variant]
    net = cls(GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0, act_dtype=act_dtype), DEV)
    net.load_state_dict(_weights(variant), strict=True)
    net.train()
    return net


@functools.lru_cache(maxsize=None)
def _inputs(variant="vec"):
    sys.path.insert(0, ROOT)
    import bench
    return bench.synth_inputs(2, torch.device(DEV), seed=42, variant=variant)


def _freeze(net, which):
    if which == "HEAD_ONLY":
        names = [n for n, _ in net.named_parameters() if not n.startswith(HEAD)]
        for n, p in net.named_parameters():
            if not n.startswith(HEAD):
                p.requires_grad_(False)
    elif which == "SCATTER":
        names = net.freeze(*SCATTER)
        assert sorted(names) == sorted(SCATTER)
    else:
        have = [n for n, _ in net.named_parameters()]
        prefixes = TRUNKS if which == "TRUNKS" else which
        names = net.freeze(*[p for p in prefixes if any(n.startswith(p) for n in have)])   # (img: there is no VectorNet)
    L = net._layout
    return [n for n in names if n not in L.unused]


def _frozen_floats(net, names):
    """bool [tail]: the floats of the named tensors (their float4 padding included)."""
    L = net._layout
    return (L.group_table(names) == 255).repeat_interleave(4)[:L.tail].to(DEV)


def _bare_backward(net, inp, gt):
    from mmfn_amd import ops
    eng = net._engine_for()
    ops.rng_advance(eng.rng_state)
    eng.forward(inp, True, gt)
    eng.backward()
    torch.cuda.synchronize()


def _pmv(net):
    L = net._layout
    return [t[:L.tail] for t in (L.params, L.exp_avg, L.exp_avg_sq)]


def _state(net):
    L, eng = net._layout, net._engine_for()
    return [L.params, L.exp_avg, L.exp_avg_sq, L.buffers_flat, L.counters_flat, eng.step_count, eng.rng_state]


# ------------------------------------------------------------------------------------------------ 2. the step
STEP_CASES = [(mask, variant, dt) for mask in ("TRUNKS", "HEAD_ONLY", "SCATTER")
              for variant, dt in (("vec", "f32"), ("img", "f32"), ("vec", "bf16"))] + [("TRUNKS+RADAR", "rad", "f32")]


@pytest.mark.parametrize("mask,variant,act_dtype", STEP_CASES)
def test_frozen_tensors_keep_their_bits_and_trainable_ones_their_gradients(mask, variant, act_dtype):
    which = TRUNKS + ("encoder.radar_encoder.",) if mask == "TRUNKS+RADAR" else mask
    inp, gt = _inputs(variant)
    frozen_net, plain_net = _net(variant, act_dtype), _net(variant, act_dtype)
    names = _freeze(frozen_net, which)
    assert names and len(names) < len(list(frozen_net.parameters()))
    frozen = _frozen_floats(frozen_net, names)
    init = [t.clone() for t in _pmv(frozen_net)]
    # a bare forward + backward: trainable gradients keep their bits, frozen ranges hold zeros
    _bare_backward(frozen_net, inp, gt)
    _bare_backward(plain_net, inp, gt)
    gf, gp = frozen_net._layout.grads[:frozen.numel()], plain_net._layout.grads[:frozen.numel()]
    assert torch.equal(gf[~frozen], gp[~frozen])
    assert not gf[frozen].any() and gp[frozen].any()
    assert frozen_net._engine_for().frozen == frozenset(names)
    # three steps, default weight decay on
    for i in range(3):
        frozen_net.train_step(inp, gt, lr=1e-3)
        plain_net.train_step(inp, gt, lr=1e-3)
        if i == 0:
            torch.cuda.synchronize()
            for a, b in zip(_pmv(frozen_net), _pmv(plain_net)):
                assert torch.equal(a[~frozen], b[~frozen])          # the masked launch steps the others as the plain one does
            assert not torch.equal(_pmv(frozen_net)[0][~frozen], init[0][~frozen])
    torch.cuda.synchronize()
    for now, was in zip(_pmv(frozen_net), init):
        assert torch.equal(now[frozen], was[frozen])                # parameter, exp_avg, exp_avg_sq: no step, no decay
    assert not torch.equal(_pmv(plain_net)[0][frozen], init[0][frozen])   # (what the flags were ignored for: decay alone moves them)
    assert not frozen_net._layout.grads[:frozen.numel()][frozen].any()
    assert int(frozen_net._engine_for().step_count.item()) == 3


def test_trunks_frozen_step_agrees_with_the_oracle_under_the_same_flags():
    """The CPU oracle with the four encoders frozen: the same loss (1e-4, the bar of test_frames_gpu.py), frozen tensors
    unchanged on both sides.  Inputs: the oracle's synthetic batch, as in smoke()."""
    from oracle import fixtures, harness
    oracle = harness.build_oracle("vec")
    net = _net("vec")
    net.load_state_dict(oracle.state_dict(), strict=True)
    for n, p in oracle.named_parameters():
        if n.startswith(TRUNKS):
            p.requires_grad_(False)
    names = _freeze(net, "TRUNKS")
    before = {n: p.detach().clone() for n, p in oracle.named_parameters()}
    batch = fixtures.synthetic_batch(2, "vec", seed=42, lanes=9)
    args = harness.forward_args(batch, "vec")
    _, loss_ref, grads_ref = harness.train_step(oracle, args, batch["gt_wp"])
    to = lambda t: t.to(DEV)
    vm = [[to(args[3][0][0])], [to(args[3][1][0])], args[3][2]]
    inp = net._pack([to(args[0][0])], [to(args[1][0])], None, vm, None, None, to(args[6]), to(args[7]))
    init = net._layout.params.clone()
    loss = net.train_step(inp, to(batch["gt_wp"]))
    torch.cuda.synchronize()
    assert abs(float(loss.item()) - float(loss_ref.item())) <= 1e-4
    frozen = _frozen_floats(net, names)
    assert torch.equal(net._layout.params[:frozen.numel()][frozen], init[:frozen.numel()][frozen])
    for n, p in oracle.named_parameters():
        if n.startswith(TRUNKS):
            assert grads_ref[n] is None and torch.equal(p.detach(), before[n]), n
    assert any(not torch.equal(p.detach(), before[n]) for n, p in oracle.named_parameters() if n.startswith("encoder.transformer"))


def test_one_row_step_ignores_an_installed_group_table_frozen_or_not():
    """A two-group FusedAdamW was constructed (its group table is installed in the engine), then the step runs with ONE hyper
    row (net.train_step(lr=...)): everything is group 0, as without frozen parameters - the masked launch must not read the
    second group's scalars, which nobody wrote."""
    from mmfn_amd.optim import FusedAdamW, configure_optimizers
    inp, gt = _inputs("vec")
    frozen_net, plain_net = _net(), _net()
    for net in (frozen_net, plain_net):
        FusedAdamW(net, param_groups=configure_optimizers(net))
        assert net._engine_for().opt_group_of is not None
    names = _freeze(frozen_net, "SCATTER")
    frozen = _frozen_floats(frozen_net, names)
    init = [t.clone() for t in _pmv(frozen_net)]
    for _ in range(2):
        frozen_net.train_step(inp, gt, lr=1e-3)
    plain_net.train_step(inp, gt, lr=1e-3)
    torch.cuda.synchronize()
    for now, was in zip(_pmv(frozen_net), init):
        assert torch.equal(now[frozen], was[frozen])
    # the first step against the unmasked launch: redo it on a fresh twin and compare every live float
    twin = _net()
    FusedAdamW(twin, param_groups=configure_optimizers(twin))
    _freeze(twin, "SCATTER")
    twin.train_step(inp, gt, lr=1e-3)
    torch.cuda.synchronize()
    for a, b in zip(_pmv(twin), _pmv(plain_net)):
        assert torch.equal(a[~frozen], b[~frozen])
    # ... and with the optimizer's own two rows the table's ids are used again
    opt = FusedAdamW(twin, lr=1e-3, param_groups=configure_optimizers(twin))
    opt2 = FusedAdamW(plain_net, lr=1e-3, param_groups=configure_optimizers(plain_net))
    for net, o in ((twin, opt), (plain_net, opt2)):
        net._engine_for().train_step(inp, gt, lr=1e-3, groups=o.hyper_rows())
    torch.cuda.synchronize()
    assert torch.equal(_pmv(twin)[0][frozen], init[0][frozen])


# ------------------------------------------------------------------------------------------------ 3. work really skipped
def _count_calls(monkeypatch):
    from mmfn_amd import engine as E, ops, ops16
    calls = {}

    def wrap(owner, attr, key):
        real = getattr(owner, attr)

        def counted(*a, **k):
            calls[key] = calls.get(key, 0) + 1
            return real(*a, **k)
        monkeypatch.setattr(owner, attr, counted)

    wrap(ops, "conv2d_wgrad", "ops.conv2d_wgrad")
    wrap(ops16, "conv2d_wgrad", "ops16.conv2d_wgrad")
    wrap(ops, "conv2d_wgrad_winograd", "ops.conv2d_wgrad_winograd")
    wrap(E.ConvBN, "stem_wgrad", "stem_wgrad")
    wrap(E.VectorNet, "bwd", "VectorNet.bwd")
    wrap(E.GPT, "bwd", "GPT.bwd")
    wrap(E.ResNetTrunk, "layer_bwd", "layer_bwd")
    real_bwd_wino = ops.conv2d_bwd_winograd

    def bwd_wino(dy, x, u, dw_out, *a, **k):
        if dw_out is not None:
            calls["winograd dw"] = calls.get("winograd dw", 0) + 1
        return real_bwd_wino(dy, x, u, dw_out, *a, **k)
    monkeypatch.setattr(ops, "conv2d_bwd_winograd", bwd_wino)
    return calls


@pytest.mark.parametrize("act_dtype", ["f32", "bf16"])
def test_pruned_launches_are_not_issued(act_dtype, monkeypatch):
    inp, gt = _inputs("vec")
    nets = {k: _net("vec", act_dtype) for k in ("none", "TRUNKS", "HEAD_ONLY")}
    _freeze(nets["TRUNKS"], "TRUNKS")
    _freeze(nets["HEAD_ONLY"], "HEAD_ONLY")
    calls = _count_calls(monkeypatch)
    seen = {}
    for k, net in nets.items():
        calls.clear()
        net.train_step(inp, gt)
        torch.cuda.synchronize()
        seen[k] = dict(calls)
    wgrads = ("ops.conv2d_wgrad", "ops16.conv2d_wgrad", "winograd dw")
    # nothing frozen: the weight-gradient launches are there (which ones depends on the mode), the stems', VectorNet's too
    assert sum(seen["none"].get(k, 0) for k in wgrads) >= 60
    assert seen["none"].get("ops16.conv2d_wgrad" if act_dtype == "bf16" else "winograd dw", 0) > 0
    assert seen["none"]["stem_wgrad"] == 2 and seen["none"]["VectorNet.bwd"] == 1 and seen["none"]["GPT.bwd"] == 4
    assert seen["none"]["layer_bwd"] == 3 * 3 + 2
    t = seen["TRUNKS"]
    for k in wgrads + ("ops.conv2d_wgrad_winograd", "stem_wgrad", "VectorNet.bwd"):
        assert t.get(k, 0) == 0, (k, t)
    assert t["GPT.bwd"] == 4 and t["layer_bwd"] == 3 * 3      # the data gradient still flows through layers 2-4 into the transformers
    h = seen["HEAD_ONLY"]
    for k in wgrads + ("stem_wgrad", "VectorNet.bwd", "GPT.bwd", "layer_bwd"):
        assert h.get(k, 0) == 0, (k, h)


# ------------------------------------------------------------------------------------------------ 4. norm, clipping, accumulation, guard
@pytest.mark.parametrize("mask", ["TRUNKS", "SCATTER"])
def test_norm_clipping_accumulation_and_guard_range_over_trainable_tensors(mask):
    inp, gt = _inputs("vec")
    # the per-tensor norms of one bare backward ...
    probe = _net()
    names = _freeze(probe, mask)
    _bare_backward(probe, inp, gt)
    tnames, table = probe.tensor_stats("grads")
    table = table.cpu()
    torch.cuda.synchronize()
    norms = dict(zip(tnames, table[:, 0].tolist()))
    assert all(norms[n] == 0.0 for n in names)                       # frozen tensors report 0
    live = [n for n in tnames if n not in set(names)]
    assert sum(norms[n] > 0.0 for n in live) >= len(live) - 1        # (VectorNet's pos_emb.0.weight sees a zero input)
    want = sum(norms[n] ** 2 for n in live) ** 0.5
    # ... against the norm the clipped step measures on a copy, after a bare backward of its own
    net = _net()
    assert _freeze(net, mask) == names
    _bare_backward(net, inp, gt)
    frozen = _frozen_floats(net, names)
    init = [t.clone() for t in _pmv(net)]
    net.train_step(inp, gt, lr=1e-3, clip_grad_norm=0.5)
    torch.cuda.synchronize()
    got = float(net._engine_for().last_grad_norm.item())
    print("\n[%s] last_grad_norm %.9g, from tensor_stats %.9g" % (mask, got, want))
    assert abs(got - want) <= 1e-6 * want
    # accumulation, then the clipped final step: frozen bits stay, the others move
    net.accumulate_step(inp, gt)
    assert not net._engine_for().grad_acc[:frozen.numel()][frozen].any()
    net.train_step(inp, gt, lr=1e-3, clip_grad_norm=0.5)
    torch.cuda.synchronize()
    for now, was in zip(_pmv(net), init):
        assert torch.equal(now[frozen], was[frozen])
        assert not torch.equal(now[~frozen], was[~frozen])
    _, table2 = net.tensor_stats("grads")
    assert all(v == 0.0 for n, v in zip(tnames, table2[:, 0].tolist()) if n in set(names))
    # the guard: a NaN in the input image skips the step; every tensor, frozen or not, keeps its bits
    net.guard_nonfinite(True)
    before = [t.clone() for t in _state(net)]
    image = torch.rand(2, 3, 256, 256, device=DEV) * 255.0
    image[1, 2, 100, 7] = float("nan")
    bad = {k: v for k, v in inp.items() if k != "rgb_u8"}
    bad["image"] = image
    net.train_step(bad, gt, lr=1e-3)
    torch.cuda.synchronize()
    assert int(net._engine_for().skipped_steps.item()) == 1
    for now, was in zip(_state(net)[:-1], before[:-1]):              # (rng_state advances either way)
        assert torch.equal(now, was)
    net.train_step(inp, gt, lr=1e-3)                                 # and a finite step is taken again, frozen bits in place
    torch.cuda.synchronize()
    assert int(net._engine_for().skipped_steps.item()) == 1
    for now, was in zip(_pmv(net), init):
        assert torch.equal(now[frozen], was[frozen])
    assert not torch.equal(_pmv(net)[0][~frozen], before[0][:frozen.numel()][~frozen])


# ------------------------------------------------------------------------------------------------ 5. the weight average
def test_attached_average_follows_frozen_parameters_too():
    from mmfn_amd.averaging import AveragedMMFN
    inp, gt = _inputs("vec")
    net = _net()
    names = _freeze(net, "SCATTER")
    net.train_step(inp, gt, lr=1e-3)          # warm: buffers, filter tables
    torch.cuda.synchronize()
    avg = AveragedMMFN(net, "ema", decay=0.9)
    net.attach_average(avg)
    pnames = [n for n, _ in net.named_parameters()]
    ref = None
    for i in range(3):
        net.train_step(inp, gt, lr=1e-3)
        torch.cuda.synchronize()
        cur = [p.detach().clone() for p in net.parameters()]
        if ref is None:
            ref = cur                              # the first update copies
        else:
            torch._foreach_lerp_(ref, cur, 1 - 0.9)   # torch.optim.swa_utils.get_ema_multi_avg_fn
    net.attach_average(None)
    torch.cuda.synchronize()
    got = dict(avg.module.named_parameters())
    model = dict(net.named_parameters())
    for n, r in zip(pnames, ref):
        assert torch.equal(got[n].detach(), r), n
    for n in names:
        assert torch.equal(got[n].detach(), model[n].detach()), n
    assert int(avg.n_averaged.item()) == 3


# ------------------------------------------------------------------------------------------------ 6. graphs and hooks
def test_graph_replay_equals_eager_and_refuses_a_changed_mask():
    from mmfn_amd.parallel import GraphedStep
    inp, gt = _inputs("vec")
    eager, graphed = _net(), _net()
    _freeze(eager, "TRUNKS")
    names = _freeze(graphed, "TRUNKS")
    frozen = _frozen_floats(graphed, names)
    init = [t.clone() for t in _pmv(graphed)]
    eng = graphed._engine_for()
    step = GraphedStep(eng, None, inp, gt, lr=1e-3, warm=1)
    for _ in range(2):
        step()
    for _ in range(3):
        eager.train_step(inp, gt, lr=1e-3)
    torch.cuda.synchronize()
    for a, b in zip(_state(eager), _state(graphed)):
        assert torch.equal(a, b)
    for now, was in zip(_pmv(graphed), init):
        assert torch.equal(now[frozen], was[frozen]) and not torch.equal(now[~frozen], was[~frozen])
    graphed.unfreeze("encoder.vectornet_encoder.")
    with pytest.raises(RuntimeError, match="requires_grad"):
        step()
    again = GraphedStep(eng, None, inp, gt, lr=1e-3, warm=1)    # a new capture for the new flags works
    again()
    torch.cuda.synchronize()
    assert torch.isfinite(again.loss).all()
    vec = _frozen_floats(graphed, [n for n in names if "vectornet_encoder" in n])
    assert not torch.equal(_pmv(graphed)[0][vec], init[0][vec])       # VectorNet trains again
    still = _frozen_floats(graphed, [n for n in names if "vectornet_encoder" not in n])
    assert torch.equal(_pmv(graphed)[0][still], init[0][still])


@pytest.mark.parametrize("mask", ["TRUNKS", "HEAD_ONLY"])    # HEAD_ONLY: every scale takes the branch that launches nothing
def test_readiness_hooks_fire_as_always_over_zeroed_frozen_ranges(mask):
    inp, gt = _inputs("vec")
    plain, frozen_net = _net(), _net()
    names = _freeze(frozen_net, mask)
    frozen = _frozen_floats(frozen_net, names)
    seen = {}
    for key, net in (("plain", plain), ("frozen", frozen_net)):
        from mmfn_amd import ops
        eng, L = net._engine_for(), net._layout
        order, clones = [], {}

        def hook(k, L=L, order=order, clones=clones):
            order.append(k)
            b, e = L.group_ranges[k]
            clones[k] = L.grads[b:e].clone()      # on the stream that reports the group
        ops.rng_advance(eng.rng_state)
        eng.forward(inp, True, gt)
        eng.backward(on_ready=hook)
        torch.cuda.synchronize()
        seen[key] = (order, clones)
    assert seen["plain"][0] == seen["frozen"][0] and set(seen["plain"][0]) == set(plain._layout.group_ranges)
    for k, (b, e) in plain._layout.group_ranges.items():
        f = frozen[b:e]
        assert not seen["frozen"][1][k][f].any(), k
        assert torch.equal(seen["frozen"][1][k][~f], seen["plain"][1][k][~f]), k


# ------------------------------------------------------------------------------------------------ 7. autograd path, optimizer state
def test_autograd_path_optimizer_state_and_pending_micro_steps():
    from oracle import fixtures, harness
    from mmfn_amd.optim import FusedAdamW
    net = _net()
    L = net._layout
    names = set(_freeze(net, TRUNKS[:1] + ("encoder.transformer2.pos_emb", "join.0.bias")))
    batch = fixtures.synthetic_batch(2, "vec", seed=42, lanes=9)
    args = harness.forward_args(batch, "vec")
    to = lambda t: t.to(DEV)
    dargs = ([to(args[0][0])], [to(args[1][0])], None, [[to(args[3][0][0])], [to(args[3][1][0])], args[3][2]], None, None,
             to(args[6]), to(args[7]))
    gt = to(batch["gt_wp"])
    opt = FusedAdamW(net, lr=1e-3, param_groups=[{"params": [p for p in net.parameters() if p.requires_grad]}])
    init = L.params.clone()
    for i in range(2):
        opt.zero_grad()
        loss = torch.nn.functional.l1_loss(net(*dargs), gt)
        loss.backward()
        for n, p in net.named_parameters():
            assert (p.grad is None) == (n in names or n in L.unused), n
        opt.step()
    torch.cuda.synchronize()
    frozen = _frozen_floats(net, names)
    assert torch.equal(L.params[:frozen.numel()][frozen], init[:frozen.numel()][frozen])
    assert not torch.equal(L.params[:frozen.numel()][~frozen], init[:frozen.numel()][~frozen])
    # the checkpoint: no state for what was frozen at every step - in the filtered groups they do not even have an id
    sd = opt.state_dict()
    grouped = [n for n, p in net.named_parameters() if p.requires_grad]
    assert len(sd["param_groups"][0]["params"]) == len(grouped)
    assert sorted(sd["state"]) == [i for i, n in enumerate(grouped) if n not in L.unused]
    torch.optim.AdamW([{"params": [p for p in net.parameters() if p.requires_grad]}], lr=1e-3).load_state_dict(sd)
    # ... and with every parameter in the group, the frozen ones have an id and no entry, as in torch
    full = FusedAdamW(net, lr=1e-3)
    sd = full.state_dict()
    all_names = [n for n, _ in net.named_parameters()]
    assert sorted(sd["state"]) == [i for i, n in enumerate(all_names) if n not in names and n not in L.unused]
    torch.optim.AdamW(net.parameters(), lr=1e-3).load_state_dict(sd)
    # a parameter unfrozen outside every group raises at the next step
    net.unfreeze("join.0.bias")
    with pytest.raises(ValueError, match="must cover every parameter"):
        opt.step()
    net.freeze("join.0.bias")
    # a mask change with a micro-step pending raises, and the pending sum can still be used under the old flags
    inp, gtb = _inputs("vec")
    net.accumulate_step(inp, gtb)
    net.unfreeze(TRUNKS[0])
    with pytest.raises(RuntimeError, match="pending"):
        net.train_step(inp, gtb)
    with pytest.raises(RuntimeError, match="pending"):
        net.accumulate_step(inp, gtb)
    net.freeze(TRUNKS[0])
    net.train_step(inp, gtb)
    torch.cuda.synchronize()
    assert net._engine_for().accum_pending == 0
