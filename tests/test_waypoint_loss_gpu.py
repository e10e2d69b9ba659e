"""Waypoint objectives on the fused step (losses.WaypointLoss, Engine.set_loss): the head launches with the objective as a parameter
against float64 autograd, their L1 case against the original launches bit for bit, their refusals, the whole step against the
autograd entry fed with torch's own gradient of the loss, graph replay, the defaults, and the trainer."""
import functools
import os
import pickle
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("l1", "smooth_l1", "huber", "mse")
PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out")


def _close(got, ref, tol=2e-5, what=""):
    got = got.detach().cpu().double()
    ref = ref.detach().double()
    scale = ref.abs().max().item() + 1e-6
    err = (got - ref).abs().max().item()
    print("%s: max err %.3g, scale %.3g, bar %.3g" % (what, err, scale, tol * scale))
    assert err <= tol * scale, "%s max err %g vs scale %g" % (what, err, scale)


# ------------------------------------------------------------------------------------------------ 1: the kernels against float64
@functools.lru_cache(maxsize=None)
def _head_case(steps, B=3):
    """GRUCell(2, 64) + Linear(64, 2) and one batch, fp32-representable values held in float64 on the CPU; built once per `steps`
    and never changed (the tests clone what they differentiate)."""
    with torch.random.fork_rng():
        torch.manual_seed(1235 + steps)   # (chosen so that the conditions test 1 asserts on the float64 reference hold at B = 3)
        gru, out = torch.nn.GRUCell(2, 64), torch.nn.Linear(64, 2)
        z0 = torch.randn(B, 64)
        target = torch.randn(B, 2) * 5
        gt = torch.randn(B, steps, 2) * 3
        hw = torch.rand(steps) * 1.75 + 0.25
        sw = torch.rand(B) * 3
        sw[1] = 0.0
    P32 = dict(w_ih=gru.weight_ih, w_hh=gru.weight_hh, b_ih=gru.bias_ih, b_hh=gru.bias_hh, w_out=out.weight, b_out=out.bias)
    P32 = {k: v.detach().clone() for k, v in P32.items()}
    return {"P": P32, "z0": z0, "target": target, "gt": gt, "hw": hw, "sw": sw, "B": B, "steps": steps}


def _head_reference(case, loss, sw):
    """float64 autograd through the recurrence and loss.reference: pred, loss, per-sample terms, l1 terms, dz0, parameter grads."""
    P = {k: v.double().requires_grad_(True) for k, v in case["P"].items()}
    z0 = case["z0"].double().requires_grad_(True)
    target, gt = case["target"].double(), case["gt"].double()
    x, h, wps = torch.zeros(case["B"], 2, dtype=torch.float64), z0, []
    for _ in range(case["steps"]):
        xi = x + target
        gi = xi @ P["w_ih"].t() + P["b_ih"]
        gh = h @ P["w_hh"].t() + P["b_hh"]
        r = torch.sigmoid(gi[:, :64] + gh[:, :64])
        z = torch.sigmoid(gi[:, 64:128] + gh[:, 64:128])
        n = torch.tanh(gi[:, 128:] + r * gh[:, 128:])
        h = n + z * (h - n)
        x = x + h @ P["w_out"].t() + P["b_out"]
        wps.append(x)
    pred = torch.stack(wps, 1)
    sw64 = None if sw is None else sw.double()
    value = loss.reference(pred, gt, sw64)
    value.backward()
    term = loss.terms(pred.detach(), gt)
    if loss.step_weights is not None:
        term = term * torch.tensor(loss.step_weights, dtype=torch.float64)[None, :, None]
    if sw64 is not None:
        term = term * sw64[:, None, None]
    return {"pred": pred.detach(), "loss": value.item(), "terms": term.sum((1, 2)), "l1": (pred.detach() - gt).abs().sum((1, 2)),
            "dz0": z0.grad, "grads": [P[k].grad for k in PARAMS], "e": pred.detach() - gt}


def test_float64_recurrence_is_torchs_grucell():
    """The yardstick restates GRUCell by hand (to run it in float64 with gradients to every parameter): check it against the module."""
    case = _head_case(4)
    gru, out = torch.nn.GRUCell(2, 64).double(), torch.nn.Linear(64, 2).double()
    with torch.no_grad():
        for dst, k in ((gru.weight_ih, "w_ih"), (gru.weight_hh, "w_hh"), (gru.bias_ih, "b_ih"), (gru.bias_hh, "b_hh"),
                       (out.weight, "w_out"), (out.bias, "b_out")):
            dst.copy_(case["P"][k].double())
    x, h, wps = torch.zeros(3, 2, dtype=torch.float64), case["z0"].double(), []
    for _ in range(4):
        h = gru(x + case["target"].double(), h)
        x = x + out(h)
        wps.append(x)
    from mmfn_amd.losses import WaypointLoss
    ref = _head_reference(case, WaypointLoss("l1"), None)
    assert (torch.stack(wps, 1).detach() - ref["pred"]).abs().max().item() <= 1e-12


def _run_head(case, kind_code, table, sw, old=False):
    from mmfn_amd import ops
    from mmfn_amd._lib import lib
    B, steps = case["B"], case["steps"]
    P = {k: v.to(DEV).contiguous() for k, v in case["P"].items()}
    z0, target, gt = case["z0"].to(DEV), case["target"].to(DEV), case["gt"].to(DEV)
    o = {"pred": torch.empty(B, steps, 2, device=DEV), "hs": torch.empty(B, steps + 1, 64, device=DEV),
         "gates": torch.empty(B, steps, 4, 64, device=DEV), "xin": torch.empty(B, steps, 2, device=DEV),
         "lt": torch.empty(B, device=DEV), "loss": torch.empty(1, device=DEV), "l1": torch.empty(B, device=DEV),
         "dz0": torch.empty(B, 64, device=DEV), "part": torch.empty(B, lib().mmfn_gru_head_part_floats(), device=DEV)}
    gscale = 1.0 / (B * steps * 2)
    if old:
        ops.gru_head_fwd(z0, target, P["w_ih"], P["w_hh"], P["b_ih"], P["b_hh"], P["w_out"], P["b_out"], gt, o["pred"], o["hs"],
                         o["gates"], o["xin"], o["lt"], o["loss"], steps)
        ops.gru_head_bwd(o["pred"], gt, None, gscale, P["w_ih"], P["w_hh"], P["w_out"], o["hs"], o["gates"], o["xin"], o["dz0"],
                         o["part"], steps)
    else:
        swd = None if sw is None else sw.to(DEV)
        ops.gru_head_fwd_loss(z0, target, P["w_ih"], P["w_hh"], P["b_ih"], P["b_hh"], P["w_out"], P["b_out"], gt, o["pred"], o["hs"],
                              o["gates"], o["xin"], o["lt"], o["loss"], kind_code, table, swd, o["l1"], steps)
        ops.gru_head_bwd_loss(o["pred"], gt, gscale, P["w_ih"], P["w_hh"], P["w_out"], o["hs"], o["gates"], o["xin"], o["dz0"],
                              o["part"], kind_code, table, swd, steps)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("steps", [1, 4, 8])
@pytest.mark.parametrize("weights", ["both", "horizon", "sample", "neither"])
@pytest.mark.parametrize("kind", KINDS)
def test_head_loss_kernels_match_float64_autograd(kind, weights, steps):
    """Bars: test_kernels_gpu.py::test_gru_head's, relative to the reference's largest magnitude - 1e-5 pred, 2e-5 dz0, 5e-5 the
    parameter sums - and 1e-6 * max(1, |loss|) for the scalar.  The per-sample outputs have no bar there: l1_terms is a sum of |e|
    over the sample, each |e| as good as pred, so pred's 1e-5; loss_terms squares e in two of the kinds (d(e^2) / e^2 = 2 de / e), so
    2e-5."""
    from mmfn_amd.losses import WaypointLoss
    case = _head_case(steps)
    hw = case["hw"].tolist() if weights in ("both", "horizon") else None
    sw = case["sw"] if weights in ("both", "sample") else None
    loss = WaypointLoss(kind, beta=2.0, delta=2.0, step_weights=hw)
    ref = _head_reference(case, loss, sw)
    a = ref["e"].abs()
    # conditions on the inputs (a failing one asks for another seed in _head_case, never a wider bar)
    assert a.min().item() >= 1e-4, "an element sits on L1's kink"
    if kind in ("smooth_l1", "huber"):
        inner = (a < 2.0).double().mean().item()
        assert 0.25 <= inner <= 0.75, "each branch must hold a quarter of the elements, quadratic: %.2f" % inner
    if sw is not None:
        assert sw[1].item() == 0.0 and not ref["dz0"][1].any()
    table = torch.tensor(loss.table(steps), dtype=torch.float32, device=DEV)
    o = _run_head(case, loss.kind_code, table, sw)
    _close(o["pred"], ref["pred"], 1e-5, "pred")
    got = o["loss"].item()
    print("loss %.9g ref %.9g" % (got, ref["loss"]))
    assert abs(got - ref["loss"]) <= 1e-6 * max(1.0, abs(ref["loss"]))
    _close(o["lt"], ref["terms"], 2e-5, "loss_terms")
    _close(o["l1"], ref["l1"], 1e-5, "l1_terms")
    _close(o["dz0"], ref["dz0"], 2e-5, "dz0")
    if sw is not None:
        assert not o["dz0"][1].any()
    tot = o["part"].sum(0).cpu()
    off = 0
    for name, g in zip(PARAMS, ref["grads"]):
        _close(tot[off:off + g.numel()], g.flatten(), 5e-5, name)
        off += g.numel()
    assert off == tot.numel()


# ------------------------------------------------------------------------------------------------ 2: L1 restates the old launches
@pytest.mark.parametrize("steps", [4, 8])
@pytest.mark.parametrize("ones", [False, True])
def test_l1_with_unit_weights_is_the_original_pair_bit_for_bit(steps, ones):
    from mmfn_amd.losses import WaypointLoss
    case = _head_case(steps, B=5)
    loss = WaypointLoss("l1", step_weights=(1.0,) * steps)
    table = torch.tensor(loss.table(steps), dtype=torch.float32, device=DEV)
    old = _run_head(case, None, None, None, old=True)
    new = _run_head(case, loss.kind_code, table, torch.ones(5) if ones else None)
    for k in ("pred", "hs", "gates", "xin", "lt", "loss", "dz0", "part"):
        assert torch.equal(old[k], new[k]), k   # (x * 1.0f is exact: a difference means the arithmetic order changed)
    assert torch.equal(new["l1"], old["lt"])


# ------------------------------------------------------------------------------------------------ 3: refusals
def test_loss_entry_points_refuse_bad_arguments_without_launching():
    from mmfn_amd._lib import lib
    L = lib()
    B, S = 2, 4
    s = torch.cuda.current_stream().cuda_stream
    f = lambda *shape: torch.full(shape, 7.0, device=DEV)
    z0, target, gt = f(B, 64), f(B, 2), f(B, S, 2)
    w_ih, w_hh, b_ih, b_hh, w_out, b_out = f(192, 2), f(192, 64), f(192), f(192), f(2, 64), f(2)
    pred, hs, gates, xin, lt, loss, l1 = f(B, 9, 2), f(B, 10, 64), f(B, 9, 4, 64), f(B, 9, 2), f(B), f(1), f(B)
    dz0, part = f(B, 64), f(B, L.mmfn_gru_head_part_floats())
    table = torch.ones(16, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()

    def fwd(kind=1, tab=table, steps=S, batch=B, hs_=hs, gt_=gt, lt_=lt):
        return L.mmfn_gru_head_fwd_loss_f32(p(z0), p(target), p(w_ih), p(w_hh), p(b_ih), p(b_hh), p(w_out), p(b_out), p(gt_), p(pred),
                                            p(hs_), p(gates), p(xin), p(lt_), p(loss), kind, p(tab), None, p(l1), batch, steps, s)

    def bwd(kind=1, tab=table, steps=S, batch=B, gt_=gt):
        return L.mmfn_gru_head_bwd_loss_f32(p(pred), p(gt_), 0.125, p(w_ih), p(w_hh), p(w_out), p(hs), p(gates), p(xin), p(dz0), p(part),
                                            kind, p(tab), None, batch, steps, s)

    for call in (fwd, bwd):
        assert call(kind=4) == -1 and call(kind=-1) == -1
        assert call(tab=None) == -1
        assert call(steps=9) == -1 and call(steps=0) == -1
        assert call(batch=0) == -1
        assert call(gt_=None) == -1
    assert fwd(hs_=None) == -1 and fwd(lt_=None) == -1
    torch.cuda.synchronize()
    for t in (pred, hs, gates, xin, lt, loss, l1, dz0, part):   # nothing was launched: no output was touched
        assert bool((t == 7.0).all())
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not bool((pred[:, :S] == 7.0).all()) and not bool((dz0 == 7.0).all())


# ------------------------------------------------------------------------------------------------ engine helpers
@functools.lru_cache(maxsize=None)
def _oracle_weights():
    from oracle import harness
    return harness.build_oracle("vec", dropout=0.0).state_dict()


def _net(act_dtype="f32"):
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    net = MMFN(GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0, act_dtype=act_dtype), DEV)
    net.load_state_dict(_oracle_weights(), strict=True)
    net.train()
    return net


def _inputs(B, seed):
    sys.path.insert(0, ROOT)
    import bench
    return bench.synth_inputs(B, torch.device(DEV), seed=seed, lanes=16, n_lidar=4096)


def _state(net):
    L, eng = net._layout, net._engine_for()
    return [L.params, L.exp_avg, L.exp_avg_sq, L.buffers_flat, L.counters_flat, eng.step_count, eng.rng_state]


def _snapshot(net):
    return [t.clone() for t in _state(net)]


def _restore(net, snap):
    for dst, src in zip(_state(net), snap):
        dst.copy_(src)
    torch.cuda.synchronize()


HW = (2.0, 1.0, 0.5, 0.25)
SW = (1.0, 0.5)


def _loss(name, hw=HW):
    from mmfn_amd.losses import WaypointLoss
    return {"mse": WaypointLoss("mse", step_weights=hw), "huber": WaypointLoss("huber", delta=2.0, step_weights=hw),
            "smooth_l1": WaypointLoss("smooth_l1", beta=2.0, step_weights=hw), "l1": WaypointLoss("l1", step_weights=hw)}[name]


@pytest.fixture(scope="module")
def shared_nets():
    """One network per activation dtype for the tests that take no optimizer step (gradients depend on weights and inputs only)."""
    nets = {}

    def get(act_dtype):
        if act_dtype not in nets:
            nets[act_dtype] = _net(act_dtype)
        return nets[act_dtype]
    return get


# ------------------------------------------------------------------------------------------------ 4: the whole step
@pytest.mark.parametrize("act_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["mse", "huber", "smooth_l1", "l1"])
def test_step_gradient_equals_the_autograd_entry_fed_with_torchs_loss_gradient(name, act_dtype, shared_nets):
    """B = 2, pred_len = 4: 1 / (B S 2) = 1 / 16, horizon weights (2, 1, .5, .25), sample weights (1, .5), beta = delta = 2 - every
    factor of dpred but rho'(e) is a power of two, so the kernel's dpred and torch's fp32 dpred carry the same bits in any order."""
    net = shared_nets(act_dtype)
    eng, L = net._engine_for(), net._layout
    loss = _loss(name)
    inp, gt = _inputs(2, 71)
    sw = torch.tensor(SW, device=DEV)
    eng.set_loss(None)
    pred0 = eng.forward(inp, True, gt)[0].clone()
    if name in ("smooth_l1", "huber"):   # scale gt (by a power of two) until both branches occur
        for c in (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
            inner = ((pred0 - gt * c).abs() < 2.0).float().mean().item()
            if 0.2 <= inner <= 0.8:
                break
        gt = gt * c
        inner = (pred0 - gt).abs() <= 2.0
        assert inner.any() and not inner.all(), "both branches of the loss must occur"

    def comparator():
        pred, _ = eng.forward(inp, True, gt)
        p = pred.clone().requires_grad_()
        value = loss.reference(p, gt, sw)
        value.backward()
        eng.backward(p.grad.contiguous(), 1.0)
        torch.cuda.synchronize()
        return L.grads[:L.tail].clone(), value.detach()

    first, value = comparator()
    again, _ = comparator()
    assert torch.equal(first, again), "the comparator itself is not deterministic"
    eng.set_loss(loss)
    try:
        pred, got = eng.forward(dict(inp, sample_weight=sw), True, gt)
        eng.backward()
        torch.cuda.synchronize()
        assert torch.equal(pred, pred0)
        assert torch.equal(L.grads[:L.tail], first)
        ref = loss.reference(pred.double(), gt.double(), sw.double()).item()
        print("loss %.9g, float64 of the same pred %.9g, torch fp32 %.9g" % (got.item(), ref, value.item()))
        assert abs(got.item() - ref) <= 1e-6 * max(1.0, abs(ref))
        terms = eng.sample_losses()
        assert abs(terms.mean().item() - ref) <= 1e-6 * max(1.0, abs(ref))
        l1 = eng.sample_l1()
        assert abs(l1.mean().item() - F.l1_loss(pred, gt).item()) <= 1e-6 * max(1.0, l1.mean().item())
    finally:
        eng.set_loss(None)


def test_replay_equals_eager_and_follows_a_rewritten_table():
    from mmfn_amd.losses import WaypointLoss
    from mmfn_amd.parallel import StaticBatchStep
    data = []
    for i in range(4):
        inp, gt = _inputs(2, 80 + i)
        inp["sample_weight"] = torch.tensor(SW, device=DEV) * (i + 1)
        data.append((inp, gt))
    nets = [_net(), _net()]
    first = WaypointLoss("smooth_l1", beta=2.0, step_weights=HW)
    for net in nets:                           # one eager step sizes the buffers for the capture
        net.set_loss(first)
        net.train_step(*data[0])
    snap = _snapshot(nets[0])
    for net in nets:
        _restore(net, snap)
    ea, eb = nets[0]._engine_for(), nets[1]._engine_for()
    step = StaticBatchStep(eb, None, data[0][0], data[0][1], 1e-4)
    n_graphs = step.seg.recorder.n_graphs
    for inp, gt in data[:2]:
        la = nets[0].train_step(inp, gt).clone()
        lb = step(inp, gt).clone()
        assert torch.equal(la, lb)
    # beta and the horizon weights are device memory: a loss of the same kind rewrites the table, the capture stays
    second = WaypointLoss("smooth_l1", beta=0.5, step_weights=(0.25, 0.5, 1.0, 3.0))
    for net in nets:
        net.set_loss(second)
    for inp, gt in data[2:]:
        la = nets[0].train_step(inp, gt).clone()
        lb = step(inp, gt).clone()
        assert torch.equal(la, lb)
    torch.cuda.synchronize()
    assert step.seg.recorder.n_graphs == n_graphs
    for a, b in zip(_state(nets[0]), _state(nets[1])):
        assert torch.equal(a, b)
    assert int(eb.step_count.item()) == int(snap[5].item()) + 4
    # ... and it did matter: the eager twin under the first loss ends elsewhere
    third = _net()
    third.set_loss(first)
    third.train_step(*data[0])
    _restore(third, snap)
    for inp, gt in data:
        third.train_step(inp, gt)
    torch.cuda.synchronize()
    assert not torch.equal(third._layout.params, nets[0]._layout.params)
    # the kind is a launch argument: another kind, or the plain loss, needs a new capture
    before = _snapshot(nets[1])
    for other in (WaypointLoss("huber", delta=0.5, step_weights=(0.25, 0.5, 1.0, 3.0)), None, WaypointLoss("l1")):
        eb.set_loss(other)
        with pytest.raises(RuntimeError, match="captured with the smooth_l1 loss"):
            step(*data[0])
    torch.cuda.synchronize()
    for a, b in zip(_state(nets[1]), before):
        assert torch.equal(a, b)
    eb.set_loss(second)
    step(*data[0])
    # set_loss refuses while micro-steps are pending
    ea.accumulate_step(*data[0])
    with pytest.raises(RuntimeError, match="pending"):
        ea.set_loss(None)
    ea.discard_accumulated()
    ea.set_loss(None)
    with pytest.raises(ValueError, match="pred_len"):
        ea.set_loss(WaypointLoss("mse", step_weights=(1.0, 2.0)))
    with pytest.raises(TypeError):
        ea.set_loss("mse")
    assert ea.loss is None


# ------------------------------------------------------------------------------------------------ 5: nothing changes by default
def test_default_and_plain_losses_leave_the_step_as_it_was(monkeypatch):
    from mmfn_amd import ops
    from mmfn_amd.losses import WaypointLoss
    data = [_inputs(2, 90), _inputs(2, 91)]
    nets = [_net() for _ in range(4)]
    nets[1].set_loss(None)
    nets[2].set_loss(WaypointLoss("l1"))
    nets[3].set_loss(WaypointLoss("huber", delta=2.0, step_weights=HW))
    nets[3].set_loss(None)

    def refuse(*a, **k):
        raise AssertionError("the plain path must not reach the launches with the objective as a parameter")
    monkeypatch.setattr(ops, "gru_head_fwd_loss", refuse)
    monkeypatch.setattr(ops, "gru_head_bwd_loss", refuse)
    losses = []
    for net in nets:
        losses.append([net.train_step(inp, gt).clone() for inp, gt in data])
        assert net._engine_for().sample_l1() is None
    torch.cuda.synchronize()
    for net, ls in zip(nets[1:], losses[1:]):
        for a, b in zip(_state(nets[0]), _state(net)):
            assert torch.equal(a, b)
        for a, b in zip(losses[0], ls):
            assert torch.equal(a, b)
    monkeypatch.undo()
    # an eval forward's loss stays the mean L1 while another objective is set
    net = nets[0]
    eng = net._engine_for()
    inp, gt = data[0]
    net.eval()
    pred, plain = eng.forward(inp, False, gt)
    plain = plain.clone()
    eng.set_loss(WaypointLoss("huber", delta=0.5))
    pred2, held = eng.forward(dict(inp, sample_weight=torch.tensor(SW, device=DEV)), False, gt)
    torch.cuda.synchronize()
    assert torch.equal(plain, held)
    assert abs(held.item() - F.l1_loss(pred2, gt).item()) <= 1e-6 * max(1.0, held.item())
    net.train()
    _, huber = eng.forward(inp, True, gt)
    assert eng.sample_l1() is not None and not torch.equal(huber, plain)


# ------------------------------------------------------------------------------------------------ 6: trainer
@pytest.fixture(scope="module")
def store(tmp_path_factory):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from oracle import fixtures
    root = tmp_path_factory.mktemp("loss_train")
    samples = fixtures.synthetic_samples((5, 9, 3, 7, 4, 6, 8, 2), seed=5, radar_counts=(50, 81, 81, 20, 60, 81, 33, 70))
    for i, s in enumerate(samples):
        with open(root / ("%d.pkl" % i), "wb") as fd:
            pickle.dump(s, fd)
    return D.FrameStore(str(root), GlobalConfig(), "train")


def _lateral_weight(inp, gt):
    """Sample weights from the label's lateral extent (a power of two each, so that no test depends on their rounding)."""
    return torch.where(gt[:, :, 0].abs().amax(1) > 1.0, 2.0, 0.5).to(torch.float32)


def test_trainer_sets_the_loss_for_the_epoch_and_logs_the_plain_l1(store, monkeypatch):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.losses import WaypointLoss
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import Trainer, _bucket_lanes
    cfg = GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    loader = D.make_loader(store, batch_size=2, num_workers=0)      # 4 batches
    loss = WaypointLoss("smooth_l1", beta=2.0, step_weights=HW)
    net = _net()
    eng = net._engine_for()
    outer = WaypointLoss("mse")
    eng.set_loss(outer)
    tr = Trainer(DEV, None)
    logs = []
    tr.train(net, loader, cfg, FusedAdamW(net, lr=1e-4), accum_steps=2, clip_grad_norm=float("inf"), log_every=4, on_log=logs.append,
             graph=True, loss=loss, sample_weight=_lateral_weight)
    torch.cuda.synchronize()
    assert eng.loss is outer and eng.loss_key() == "mse"   # restored
    assert tr.cur_iter == 4 and int(eng.step_count.item()) == 2 and eng.accum_pending == 0
    captured = [k for k, v in tr._static_steps.items() if not isinstance(v, str)]
    assert len(captured) == 2 and all(("loss", "smooth_l1") in k for k in captured)   # the micro and the final step replayed
    # the same epoch by hand
    staged = [D.stage_batch(b, DEV, cfg) for b in loader]
    assert len(staged) == 4
    twin = _net()
    te = twin._engine_for()
    te.set_loss(loss)
    objective, l1 = [], []
    for i, (a, gt) in enumerate(staged):
        inp = _bucket_lanes(twin._pack(*a), 16)
        inp["sample_weight"] = _lateral_weight(inp, gt)
        if i % 2 == 0:
            objective.append(te.accumulate_step(inp, gt).item())
        else:
            objective.append(te.train_step(inp, gt, clip_grad_norm=float("inf")).item())
        pred = te._bufs_for(2).get("head.pred", (2, 4, 2))
        l1.append(F.l1_loss(pred, gt).item())
    torch.cuda.synchronize()
    for x, y in zip(_state(net), _state(twin)):
        assert torch.equal(x, y)
    assert len(logs) == 1 and set(logs[0]) >= {"loss", "l1", "iter", "grad_norm"}
    want = sum(l1) / 4
    print("l1 %.9g, by hand %.9g; objective %.9g, by hand %.9g" % (logs[0]["l1"], want, logs[0]["loss"], sum(objective) / 4))
    assert abs(logs[0]["l1"] - want) <= 1e-6 * want
    assert abs(logs[0]["loss"] - sum(objective) / 4) <= 1e-6 * abs(sum(objective) / 4)
    assert abs(tr.train_loss[-1] - sum(objective) / 4) <= 1e-6 * abs(sum(objective) / 4)

    # fused=False: the autograd loop calls loss.reference in the place of the L1 loss
    calls = []
    real = loss.reference
    monkeypatch.setattr(loss, "reference", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ref = _net()
    logs2 = []
    Trainer(DEV, None).train(ref, loader, cfg, torch.optim.AdamW(ref.parameters(), lr=1e-4), fused=False, log_every=4,
                             on_log=logs2.append, loss=loss, sample_weight=_lateral_weight)
    assert len(calls) == 4 and len(logs2) == 1 and "l1" in logs2[0]
    assert ref._engine_for().loss is None
