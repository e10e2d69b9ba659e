"""EMA / SWA weight averages (mmfn_amd.averaging) against torch.optim.swa_utils: the averaging kernel, the AVG instances of the
grouped AdamW, eager fused steps, graph replay, accumulation, evaluation on the average and the trainer's files.

"Bit-identical" is the expectation against torch's _foreach_lerp_ on the same device with the same weight; at most 1 ulp per
element is accepted, and each comparison prints which of the two it saw."""
import json
import os
import pickle
import sys

import pytest
import torch
from torch.optim.swa_utils import get_ema_multi_avg_fn, get_swa_multi_avg_fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ordered(t):
    i = t.detach().float().contiguous().view(torch.int32).long()
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _lerp_match(got, want, what):
    """got == want to at most 1 ulp per element (fp32); reports which."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype != torch.float32:
        assert torch.equal(got, want), what
        return
    ulps = int((_ordered(got) - _ordered(want)).abs().max().item()) if got.numel() else 0
    assert ulps <= 1, (what, ulps)
    print("%s: %s" % (what, "bit-identical" if ulps == 0 else "within 1 ulp"))


def _torch_fn(mode, decay):
    return get_ema_multi_avg_fn(decay) if mode == "ema" else get_swa_multi_avg_fn()


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("mode,decay", [("ema", 0.9), ("ema", 0.3), ("swa", None)])
@pytest.mark.parametrize("n", [4, 4 * 1021, (1 << 25) + 8, "full"])
def test_standalone_kernel_matches_foreach_lerp(mode, decay, n, full_size):
    from mmfn_amd import ops
    n = full_size if n == "full" else n
    gen = torch.Generator(device=DEV).manual_seed(n % 1000)
    avg = torch.randn(n, device=DEV, generator=gen)
    cnt = torch.zeros((), dtype=torch.int64, device=DEV)
    w = torch.zeros(1, device=DEV).fill_(1.0 - (decay or 0.0))
    code = ops.AVG_EMA if mode == "ema" else ops.AVG_SWA
    src = torch.randn(n, device=DEV, generator=gen)
    ops.weight_average(avg, src, cnt, w, code)               # n_averaged == 0: the first update copies
    torch.cuda.synchronize()
    assert torch.equal(avg, src) and int(cnt.item()) == 0     # (the count is advanced by the caller)
    fn = _torch_fn(mode, decay)
    for k in (1, 2, 5):
        cnt.fill_(k)
        src = torch.randn(n, device=DEV, generator=gen)
        ref = [avg.clone()]
        fn(ref, [src], cnt)
        ops.weight_average(avg, src, cnt, w, code)
        torch.cuda.synchronize()
        _lerp_match(avg, ref[0], "%s n=%d k=%d" % (mode, n, k))


def test_kernels_refuse_misaligned_ragged_or_null_arguments():
    from mmfn_amd import ops
    from mmfn_amd._lib import lib
    a, b = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    w = torch.zeros(1, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    L = lib()
    f = L.mmfn_weight_average_f32
    E, S = ops.AVG_EMA, ops.AVG_SWA
    assert f(a.data_ptr(), b.data_ptr(), 6, cnt.data_ptr(), w.data_ptr(), E, s) == -1          # ragged
    assert f(a[1:].data_ptr(), b.data_ptr(), 60, cnt.data_ptr(), w.data_ptr(), E, s) == -1     # misaligned average
    assert f(a.data_ptr(), b[1:].data_ptr(), 60, cnt.data_ptr(), w.data_ptr(), E, s) == -1     # misaligned source
    assert f(None, b.data_ptr(), 64, cnt.data_ptr(), w.data_ptr(), E, s) == -1
    assert f(a.data_ptr(), None, 64, cnt.data_ptr(), w.data_ptr(), E, s) == -1
    assert f(a.data_ptr(), b.data_ptr(), 64, None, w.data_ptr(), E, s) == -1
    assert f(a.data_ptr(), b.data_ptr(), 64, cnt.data_ptr(), None, E, s) == -1                 # EMA needs its weight
    assert f(a.data_ptr(), b.data_ptr(), 64, cnt.data_ptr(), w.data_ptr(), 7, s) == -1         # unknown mode
    assert f(a.data_ptr(), b.data_ptr(), 64, cnt.data_ptr(), None, S, s) == 0                  # SWA reads no weight
    m, v, g = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    hyper = torch.zeros(16, 8, device=DEV)
    step = torch.ones(1, dtype=torch.int64, device=DEV)
    coef = torch.ones(1, device=DEV)
    args = (b.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 64, None, hyper.data_ptr(), 1, step.data_ptr())
    adam = L.mmfn_adamw_groups_f32   # (..., variant, coef, avg, n_averaged, ema_w, avg_mode, ok, stream)
    AVG, COEF_AVG = ops.ADAMW_AVG, ops.ADAMW_COEF | ops.ADAMW_AVG
    assert adam(*args, AVG, None, a[1:].data_ptr(), cnt.data_ptr(), w.data_ptr(), E, None, s) == -1
    assert adam(*args, AVG, None, a.data_ptr(), None, w.data_ptr(), E, None, s) == -1
    assert adam(*args, COEF_AVG, None, a.data_ptr(), cnt.data_ptr(), w.data_ptr(), E, None, s) == -1
    assert adam(*args, COEF_AVG, coef.data_ptr(), a.data_ptr(), cnt.data_ptr(), w.data_ptr(), 3, None, s) == -1
    assert adam(*args, AVG, None, a.data_ptr(), cnt.data_ptr(), w.data_ptr(), E, None, s) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["ema", "swa"])
def test_fused_average_adamw_equals_plain_step_then_standalone_average(mode):
    from mmfn_amd import ops
    n = 4 * 300007
    gen = torch.Generator(device=DEV).manual_seed(7)
    p0 = torch.randn(n, device=DEV, generator=gen)
    g = torch.randn(n, device=DEV, generator=gen)
    m0 = torch.randn(n, device=DEV, generator=gen) * 1e-2
    v0 = torch.rand(n, device=DEV, generator=gen) * 1e-3
    a0 = torch.randn(n, device=DEV, generator=gen)
    hyper = torch.zeros(16, 8, device=DEV)
    hyper[0, :6] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5])
    hyper[1, :6] = torch.tensor([3e-4, 0.8, 0.99, 1e-6, 0.0, 0.5])
    group_of = torch.randint(0, 2, (n // 4,), dtype=torch.uint8, device=DEV, generator=gen)
    step = torch.tensor([3], dtype=torch.int64, device=DEV)
    coef = torch.tensor([0.37], device=DEV)
    w = torch.zeros(1, device=DEV).fill_(1.0 - 0.9)
    code = ops.AVG_EMA if mode == "ema" else ops.AVG_SWA
    for clip in (None, coef):
        for k in (0, 2):
            cnt = torch.tensor(k, dtype=torch.int64, device=DEV)
            p1, m1, v1, a1 = p0.clone(), m0.clone(), v0.clone(), a0.clone()
            ops.adamw_groups(p1, g, m1, v1, step, hyper, 2, group_of=group_of, coef=clip)
            ops.weight_average(a1, p1, cnt, w, code)
            p2, m2, v2, a2 = p0.clone(), m0.clone(), v0.clone(), a0.clone()
            ops.adamw_groups(p2, g, m2, v2, step, hyper, 2, group_of=group_of, coef=clip, avg=(a2, cnt, w, code))
            torch.cuda.synchronize()
            for x, y in ((p1, p2), (m1, m2), (v1, v2), (a1, a2)):
                assert torch.equal(x, y), (clip is not None, k)
            assert not torch.equal(p1, p0) and (torch.equal(a2, p2) if k == 0 else not torch.equal(a2, p2))


# ------------------------------------------------------------------------------------------------ engine helpers
def _net(act_dtype="f32"):
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    from oracle import harness
    net = MMFN(GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0, act_dtype=act_dtype), DEV)
    net.load_state_dict(harness.build_oracle("vec", dropout=0.0).state_dict(), strict=True)
    net.train()
    return net


@pytest.fixture(scope="module")
def full_size():
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    return MMFN(GlobalConfig(), DEV)._layout.total


def _inputs(B, seed):
    sys.path.insert(0, ROOT)
    import bench
    return bench.synth_inputs(B, torch.device(DEV), seed=seed, lanes=16, n_lidar=4096)


def _state(net):
    L, eng = net._layout, net._engine_for()
    return [L.params, L.exp_avg, L.exp_avg_sq, L.buffers_flat, L.counters_flat, eng.step_count, eng.rng_state]


def _avg_state(avg):
    A = avg.module._layout
    return [A.params, A.buffers_flat, A.counters_flat, avg.n_averaged]


def _snapshot(net):
    return [t.clone() for t in _state(net)]


def _restore(net, snap):
    for dst, src in zip(_state(net), snap):
        dst.copy_(src)
    torch.cuda.synchronize()


class _TorchAverage(object):
    """AveragedModel.update_parameters written out over state_dict clones: parameters through torch's multi_avg_fn, buffers
    copied (use_buffers=False) or the fp32 ones through the same fn and the counters copied (use_buffers=True)."""

    def __init__(self, net, mode, decay, use_buffers):
        self.fn, self.use_buffers, self.n = _torch_fn(mode, decay), use_buffers, 0
        self.pnames = [k for k, _ in net.named_parameters()]
        self.bnames = [k for k, _ in net.named_buffers()]
        self.sd = None

    def update(self, net):
        cur = {k: v.detach().clone() for k, v in net.state_dict().items()}
        if self.n == 0:
            self.sd = cur
        else:
            floats = self.pnames + ([k for k in self.bnames if cur[k].dtype == torch.float32] if self.use_buffers else [])
            self.fn([self.sd[k] for k in floats], [cur[k] for k in floats], torch.tensor(self.n, device=DEV))
            for k in self.bnames:
                if k not in floats:
                    self.sd[k] = cur[k]
        self.n += 1


def _compare(avg, ref, what):
    sd = avg.module.state_dict()
    assert list(sd) == list(ref.sd)
    got =torch.cat([sd[k].float().flatten() for k in sd if sd[k].dtype == torch.float32])
    want = torch.cat([ref.sd[k].float().flatten() for k in sd if sd[k].dtype == torch.float32])
    _lerp_match(got, want, what)
    for k in sd:
        if sd[k].dtype != torch.float32:
            assert torch.equal(sd[k], ref.sd[k]), (what, k)
    assert int(avg.n_averaged.item()) == ref.n


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("act_dtype", ["f32", "bf16"])
def test_attached_average_of_five_steps_matches_torch(act_dtype):
    from mmfn_amd.averaging import AveragedMMFN
    net = _net(act_dtype)
    eng = net._engine_for()
    data = [_inputs(2, 60 + i) for i in range(5)]
    eng.train_step(*data[0])                  # warm: buffers, filter tables
    torch.cuda.synchronize()
    snap = _snapshot(net)
    refs = {}
    for case in [(m, ub) for m in ("ema", "swa") for ub in (False, True)]:
        refs[case] = _TorchAverage(net, case[0], 0.9, case[1])
    for inp, gt in data:                      # the yardstick: nothing attached, torch's averaging over each step's state_dict
        eng.train_step(inp, gt)
        torch.cuda.synchronize()
        for r in refs.values():
            r.update(net)
    live = [t.clone() for t in _state(net)]
    for (mode, ub), ref in refs.items():
        _restore(net, snap)
        avg = AveragedMMFN(net, mode, decay=0.9, use_buffers=ub)
        net.attach_average(avg)
        for inp, gt in data:
            eng.train_step(inp, gt)
        net.attach_average(None)
        torch.cuda.synchronize()
        for a, b in zip(_state(net), live):
            assert torch.equal(a, b), (mode, ub)     # the AVG instance leaves the step itself bit-identical
        _compare(avg, ref, "%s %s use_buffers=%s" % (act_dtype, mode, ub))
        del avg


def test_update_parameters_equals_torch_and_refreshes_the_version():
    from mmfn_amd.averaging import AveragedMMFN
    net = _net()
    eng = net._engine_for()
    avg = AveragedMMFN(net, "swa")
    ref = _TorchAverage(net, "swa", None, False)
    v0 = avg.module._weights_version
    for i in range(3):
        eng.train_step(*_inputs(2, 70 + i))
        avg.update_parameters(net)
        ref.update(net)
    torch.cuda.synchronize()
    assert avg.module._weights_version > v0
    _compare(avg, ref, "update_parameters swa")


# ------------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_with_an_average_equals_eager_and_refuses_a_changed_attachment():
    from mmfn_amd.averaging import AveragedMMFN
    from mmfn_amd.parallel import GraphedStep, StaticBatchStep
    data = [_inputs(2, 80 + i) for i in range(3)]
    nets = [_net(), _net()]
    for net in nets:
        net._engine_for().train_step(*data[0])
    torch.cuda.synchronize()
    ea, eb = nets[0]._engine_for(), nets[1]._engine_for()
    avgs = [AveragedMMFN(n, "ema", decay=0.9) for n in nets]
    ea.attach_average(avgs[0])
    eb.attach_average(avgs[1])
    static = StaticBatchStep(eb, None, data[0][0], data[0][1], 1e-4)
    for inp, gt in data:
        ea.train_step(inp, gt, lr=1e-4)
        static(inp, gt, lr=1e-4)
    graphed = GraphedStep(eb, None, data[1][0], data[1][1], lr=1e-4, warm=1)
    ea.train_step(*data[1], lr=1e-4)          # the warm-up step
    for _ in range(2):
        graphed()
        ea.train_step(*data[1], lr=1e-4)
    torch.cuda.synchronize()
    for a, b in zip(_state(nets[0]) + _avg_state(avgs[0]), _state(nets[1]) + _avg_state(avgs[1])):
        assert torch.equal(a, b)
    assert int(avgs[1].n_averaged.item()) == 6
    eb.detach_average()
    with pytest.raises(RuntimeError):
        static(*data[0])
    with pytest.raises(RuntimeError):
        graphed()
    plain = StaticBatchStep(eb, None, data[0][0], data[0][1], 1e-4)
    eb.attach_average(avgs[1])
    with pytest.raises(RuntimeError):
        plain(*data[0])


# ------------------------------------------------------------------------------------------------ accumulation
def test_average_moves_once_per_accumulation_group():
    from mmfn_amd.averaging import AveragedMMFN
    data = [_inputs(2, 90 + i) for i in range(8)]
    a, b = _net(), _net()
    for net in (a, b):
        net._engine_for().accumulate_step(*data[0])
        net._engine_for().discard_accumulated()
    ref = _TorchAverage(a, "ema", 0.9, False)
    avg = AveragedMMFN(b, "ema", decay=0.9)
    b.attach_average(avg)
    for net, hook in ((a, ref.update), (b, None)):
        eng = net._engine_for()
        for grp in (data[:4], data[4:]):
            for inp, gt in grp[:-1]:
                eng.accumulate_step(inp, gt)
            eng.train_step(*grp[-1], clip_grad_norm=1.0)
            torch.cuda.synchronize()
            if hook is not None:
                hook(net)
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert int(avg.n_averaged.item()) == 2
    _compare(avg, ref, "accumulation k=4 + clipping")


# ------------------------------------------------------------------------------------------------ evaluation on the average
@pytest.fixture(scope="module")
def store(tmp_path_factory):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from oracle import fixtures
    root = tmp_path_factory.mktemp("avg_train")
    samples = fixtures.synthetic_samples((5, 9, 3, 7), seed=3, radar_counts=(50, 81, 81, 20))
    for i, s in enumerate(samples):
        with open(root / ("%d.pkl" % i), "wb") as fd:
            pickle.dump(s, fd)
    return D.FrameStore(str(root), GlobalConfig(), "train")


@pytest.mark.parametrize("act_dtype", ["f32", "bf16"])
def test_validate_and_driving_session_on_the_average_equal_a_loaded_model(act_dtype, store):
    import numpy as np
    from mmfn_amd import data as D
    from mmfn_amd.averaging import AveragedMMFN
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.inference import DrivingSession
    from mmfn_amd.model import MMFN
    from mmfn_amd.trainer import Trainer
    net = _net(act_dtype)
    avg = AveragedMMFN(net, "ema", decay=0.9)
    net.attach_average(avg)
    for i in range(3):
        net.train_step(*_inputs(2, 100 + i))
    net.attach_average(None)
    torch.cuda.synchronize()
    fresh = MMFN(GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0, act_dtype=act_dtype), DEV)
    fresh.load_state_dict(avg.module.state_dict(), strict=True)
    cfg = GlobalConfig()
    loader = D.make_loader(store, batch_size=2, num_workers=0)
    va = Trainer(DEV, None).validate(avg.module, loader, cfg)
    vb = Trainer(DEV, None).validate(fresh, loader, cfg)
    assert va == vb, (va, vb)
    rng = np.random.RandomState(0)
    rgb = rng.randint(0, 256, (300, 400, 3)).astype(np.uint8)
    pts = np.stack([rng.uniform(-20, 20, 6000), rng.uniform(-12, 28, 6000), rng.uniform(-3, 1, 6000),
                    rng.uniform(0, 1, 6000)], 1).astype(np.float32)
    lanes = rng.randn(7, 10, 5).astype(np.float32)
    outs = [DrivingSession(m, max_points=1 << 15, max_lanes=32).predict(rgb, pts, lanes, (3.0, -1.0), 4.0) for m in (avg.module, fresh)]
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ trainer
def test_trainer_resume_with_average_equals_a_straight_run(store, tmp_path):
    from mmfn_amd import data as D
    from mmfn_amd.averaging import AveragedMMFN
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.model import MMFN
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import Trainer
    cfg = GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    loader = D.make_loader(store, batch_size=2, num_workers=0)
    logdir = str(tmp_path / "log")

    def epoch(tr, net, opt, avg):
        tr.train(net, loader, cfg, opt, average=avg)
        tr.validate(net, loader, cfg)
        tr.validate_average(avg, loader, cfg)

    net = _net()
    opt = FusedAdamW(net, lr=1e-4)
    avg = AveragedMMFN(net, "ema", decay=0.9)
    tr = Trainer(DEV, logdir)
    for _ in range(2):
        epoch(tr, net, opt, avg)
    tr.save(net, opt, average=avg)
    table = json.load(open(os.path.join(logdir, "recent.log")))
    assert table["average"]["n_averaged"] == 4 and table["val_loss_average"] == tr.val_loss_average
    assert {"averaged_model.pth", "best_averaged_model.pth"} <= set(table["files"])
    plain = MMFN(cfg, DEV)
    plain.load_state_dict(torch.load(os.path.join(logdir, "averaged_model.pth")), strict=True)
    epoch(tr, net, opt, avg)                  # the straight run's third epoch

    net2 = _net()
    opt2 = FusedAdamW(net2, lr=5e-4)
    avg2 = AveragedMMFN(net2, "ema", decay=0.5)
    tr2 = Trainer(DEV, logdir)
    assert tr2.resume(net2, opt2, which="recent", average=avg2) is True
    assert int(avg2.n_averaged.item()) == 4 and avg2.decay == 0.9
    epoch(tr2, net2, opt2, avg2)
    torch.cuda.synchronize()
    s1, s2 = avg.module.state_dict(), avg2.module.state_dict()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    assert int(avg2.n_averaged.item()) == int(avg.n_averaged.item()) == 6
    assert tr2.val_loss_average == tr.val_loss_average and tr2.val_loss == tr.val_loss

    # without an average: the same files and recent.log keys as before
    plain_dir = str(tmp_path / "plain")
    tr3 = Trainer(DEV, plain_dir)
    net3 = _net()
    opt3 = FusedAdamW(net3, lr=1e-4)
    tr3.train(net3, loader, cfg, opt3)
    tr3.validate(net3, loader, cfg)
    tr3.save(net3, opt3)
    assert sorted(os.listdir(plain_dir)) == ["best_model.pth", "best_optim.pth", "model.pth", "recent.log", "recent_optim.pth"]
    table = json.load(open(os.path.join(plain_dir, "recent.log")))
    assert set(table) == {"epoch", "iter", "bestval", "bestval_epoch", "train_loss", "val_loss", "files"}


# ------------------------------------------------------------------------------------------------ data parallel
def test_two_ranks_keep_their_averages_in_lock_step():
    import subprocess
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29543", os.path.join(ROOT, "tools", "average_dp_check.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "average: lock step True, matches torch True" in r.stdout, tail
