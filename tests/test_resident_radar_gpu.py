"""Radar dropout and noise, speed noise inside the resident gather, on the GPU: mmfn_gather_radar_speed against
data.radar_noise_reference and data.speed_noise_reference (float64), the adjacency it rebuilds against the rows it wrote, guard
floats at every 4-byte phase, determinism, capture, refusals, and ResidentLoader(augment=Augment(radar=, speed=)) batch by batch,
sharded and under Trainer.train.

Tolerance of the value checks (absolute, rtol 0), per column: 5.3e-6 * std_c + 1.6e-5.  The first term is the bound of the noise
stage derived in tests/test_resident_degrade_gpu.py (|dz| <= 4.9e-6 from logf, sqrtf, the rounded 2 pi and cosf, plus std's own
rounding); the second is the one rounding of fmaf's result, below 256 (2^-17 = 7.6e-6, rounded up to 2^-16) - the test data keeps
depths in (0.5, 100), angles within +/-0.6, velocities within +/-40 and speeds within +/-64, so |x + std z| < 100 + 4 * 5.77.
A kept set, its order, the flag column, a column whose std is 0, a dropped speed and the adjacency are checked exactly: the
adjacency is one f32 subtraction of two values the kernel itself wrote, so it is compared in np.float32 over the kernel's own rows
and the sign the GAT reads needs no tolerance.  A wrong row, column or draw is an error of order std or larger.
The largest |kernel - reference| measured on an MI355X: depth 4.6e-6 at std 4 (bound 3.7e-5), angles 7.4e-8 at std 0.1 (1.7e-5),
velocity 3.7e-6 at std 4 (3.7e-5), speed 4.3e-6 at std 4 (3.7e-5)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUDGET = 64 << 20
PAD = 16          # guard floats on both sides of a destination
R = 81
COUNTS = (64, 0, 17, 81, 1, 65, 40, 63, 80)          # real rows of the nine stored samples
INDEX = [3, 7, 1, 8, 0, 5, 4]                        # the batch: 81, 63, 0, 80, 64, 65, 1 real rows
IDS = [20, 3, 11, 1 << 33, 7, 0, 5, 16, 9]           # global sample id of resident row i
SETTINGS = {"drop": dict(point_drop=0.5), "noise": dict(depth_std=2.0, angle_std=0.05, velocity_std=1.5),
            "both": dict(point_drop=0.3, depth_std=4.0, angle_std=0.1, velocity_std=4.0)}


def _atol(std):
    return 5.3e-6 * std + 1.6e-5


# ---------------------------------------------------------------------------------------------- helpers
def _radar(counts, seed=0):
    """f32 [len(counts), 81, 5]: counts[b] real rows - depth in (0.5, 100), angles within +/-0.6, velocity within +/-40, and in
    the flag column 1 + the row's number, so that a row written is known by it (the kernel copies the column whatever it holds) -
    and zero rows after them."""
    rng = np.random.RandomState(seed)
    out = np.zeros((len(counts), R, 5), dtype=np.float32)
    for b, m in enumerate(counts):
        out[b, :m, 0] = rng.uniform(0.5, 100.0, m)
        out[b, :m, 1:3] = rng.uniform(-0.6, 0.6, (m, 2))
        out[b, :m, 3] = rng.uniform(-40.0, 40.0, m)
        out[b, :m, 4] = 1.0 + np.arange(m)
    return out


def _speeds(n, seed=0):
    """f32 [n] within +/-64: standing, slow, reversing and fast samples."""
    rng = np.random.RandomState(seed)
    v = rng.uniform(-64.0, 64.0, n).astype(np.float32)
    v[::4] = 0.0
    v[1::8] = rng.uniform(0.0, 0.5, len(v[1::8]))
    return v


def _guarded(shape, skew=0):
    numel = int(np.prod(shape))
    full = torch.full((numel + 2 * PAD + skew,), -7.0, device=DEV)
    return full, full[PAD + skew:PAD + skew + numel].view(shape)


def _guards_intact(full, numel, skew=0):
    return bool((full[:PAD + skew] == -7.0).all()) and bool((full[PAD + skew + numel:] == -7.0).all())


def _state(seed, epoch):
    return torch.tensor([seed, epoch], dtype=torch.int64, device=DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _radar_part(aug, src, dst, adj, state):
    depth, angle, _, velocity = aug.column_std
    return dict(src=src, dst=dst, adj=adj, state=state, point_thresh=aug.point_thresh, depth_std=depth, angle_std=angle, velocity_std=velocity)


def _speed_part(aug, src, dst, state):
    return dict(src=src, dst=dst, state=state, drop_thresh=aug.drop_thresh, std=aug.std)


def _launch(index, epoch, radar=None, speed=None, sample_id=None, skew=0):
    """One launch for the batch `index` (a list).  radar = (RadarNoise, src [n, 81, 5] device), speed = (SpeedNoise, src [n] device);
    returns {"radar": (guard buffer, dst), "adj": ..., "speed": ...} of the parts carried."""
    from mmfn_amd import ops
    B = len(index)
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    out, parts = {}, {}
    n = (radar or speed)[1].shape[0]
    if radar is not None:
        out["radar"], out["adj"] = _guarded((B, R, 5), skew), _guarded((B, R, R), skew)
        parts["radar"] = _radar_part(radar[0], radar[1], out["radar"][1], out["adj"][1], _state(radar[0].seed, epoch))
    if speed is not None:
        out["speed"] = _guarded((B,), skew)
        parts["speed"] = _speed_part(speed[0], speed[1], out["speed"][1], _state(speed[0].seed, epoch))
    ops.gather_radar_speed(idx, n, sample_id=sample_id, **parts)
    return out


def _check_radar(got, adj, stored, ids, aug, epoch, what=""):
    """The radar rows `got` [B, 81, 5] and adjacency `adj` [B, 81, 81] of a launch (numpy f32) against the float64 reference over
    the stored rows `stored` [B, 81, 5] of the samples `ids`; returns the kept counts."""
    from mmfn_amd import data as D
    want, _ = D.radar_noise_reference(stored, ids, aug, epoch)
    keep = D.radar_keep_mask(stored, ids, aug, epoch)
    assert got.dtype == np.float32 and adj.dtype == np.float32 and got.shape == want.shape
    kept = keep.sum(axis=1)
    for b in range(got.shape[0]):                                               # the kept set and its order, exactly
        assert np.array_equal(_bits(got[b, :, 4]), _bits(want[b, :, 4])), (what, b)
        assert not _bits(got[b, kept[b]:]).any(), (what, b)                     # +0.0 after them
    worst = []
    for c, std in enumerate(aug.column_std):
        if std == 0.0:
            assert np.array_equal(_bits(got[..., c]), _bits(want[..., c])), (what, c)    # copied: the stored bits
            worst.append(0.0)
        else:
            err = float(np.abs(got[..., c].astype(np.float64) - want[..., c]).max())
            worst.append(err)
            assert err <= _atol(std), (what, c, err, _atol(std))
    if aug.column_std[0]:
        assert (got[..., 0] >= 0.0).all()
    print("%s: kept %s, max |kernel - float64 reference| per column %s (atol %s)" % (
        what, kept.tolist(), ["%.2e" % e for e in worst], ["%.2e" % (_atol(s) if s else 0.0) for s in aug.column_std]))
    assert np.array_equal(adj, got[:, None, :, 1] - got[:, :, None, 1]), what       # in np.float32, over the kernel's own rows
    return kept


def _check_speed(got, stored, ids, aug, epoch, what=""):
    from mmfn_amd import data as D
    want = D.speed_noise_reference(stored, ids, aug, epoch)
    dropped = D.speed_draws(aug.seed, epoch, ids)[:, 0] < aug.drop_thresh
    assert got.dtype == np.float32 and got.shape == want.shape
    assert not _bits(got[dropped]).any()                                           # exactly +0.0
    if aug.std == 0.0:
        assert np.array_equal(_bits(got[~dropped]), _bits(np.asarray(stored)[~dropped]))
        err = 0.0
    else:
        err = float(np.abs(got.astype(np.float64) - want).max())
        assert err <= _atol(float(np.float32(aug.std))), (what, err)
        assert (got >= np.minimum(np.asarray(stored), 0.0)).all()
    print("%s: %d of %d dropped, max |kernel - float64 reference| = %.2e (atol %.2e)" % (what, dropped.sum(), len(dropped), err, _atol(aug.std)))
    return dropped


@pytest.fixture(scope="module")
def store():
    """(radar f32 [9, 81, 5] host, the same on the device, sample ids on the device)"""
    radar = _radar(COUNTS, seed=4)
    return radar, torch.from_numpy(radar).to(DEV), torch.tensor(IDS, dtype=torch.int64, device=DEV)


# ---------------------------------------------------------------------------------------------- 5. the kernel against the reference
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_kernel_matches_the_float64_reference(store, setting):
    from mmfn_amd.data import RadarNoise
    radar, dev, sid = store
    aug = RadarNoise(seed=5, **SETTINGS[setting])
    ids = [IDS[i] for i in INDEX]
    for epoch in (0, 3):
        out = _launch(INDEX, epoch, radar=(aug, dev), sample_id=sid)
        kept = _check_radar(out["radar"][1].cpu().numpy(), out["adj"][1].cpu().numpy(), radar[INDEX], ids, aug, epoch, "%s epoch %d" % (setting, epoch))
        real = np.array([COUNTS[i] for i in INDEX])
        assert kept[2] == 0 and (kept <= real).all()
        if aug.point_thresh == 0:
            assert kept.tolist() == real.tolist()
        else:
            assert kept[0] < 81 and kept.sum() < real.sum()
    # without a sample_id table the row is the id
    out = _launch(INDEX, 1, radar=(aug, dev))
    _check_radar(out["radar"][1].cpu().numpy(), out["adj"][1].cpu().numpy(), radar[INDEX], INDEX, aug, 1, "%s, id = row" % setting)


def test_everything_dropped_nothing_dropped_and_holes(store):
    from mmfn_amd.data import RadarNoise
    radar, dev, sid = store
    ids = [IDS[i] for i in INDEX]
    out = _launch(INDEX, 0, radar=(RadarNoise(point_drop=1.0), dev), sample_id=sid)
    assert not _bits(out["radar"][1].cpu().numpy()).any() and not _bits(out["adj"][1].cpu().numpy()).any()
    # nothing dropped, nothing moved: the stored rows bit for bit, and the adjacency of their f32 values
    aug = RadarNoise(velocity_std=0.0, seed=3)
    out = _launch(INDEX, 0, radar=(aug, dev), sample_id=sid)
    got = out["radar"][1].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(radar[INDEX]))
    _check_radar(got, out["adj"][1].cpu().numpy(), radar[INDEX], ids, aug, 0, "inactive")
    # zero rows between real ones are padding too: they never land among the kept rows
    holes = radar.copy()
    holes[3, 10:13] = 0.0
    holes[3, 70] = -0.0
    aug = RadarNoise(depth_std=1.0, seed=3)
    out = _launch([3], 0, radar=(aug, torch.from_numpy(holes).to(DEV)), sample_id=sid)
    kept = _check_radar(out["radar"][1].cpu().numpy(), out["adj"][1].cpu().numpy(), holes[[3]], [IDS[3]], aug, 0, "holes")
    assert kept.tolist() == [77]


# ---------------------------------------------------------------------------------------------- 6. guard floats, every 4-byte phase
def test_guard_floats_are_untouched_and_every_phase_gives_the_same_bits(store):
    from mmfn_amd.data import RadarNoise, SpeedNoise
    radar, dev, sid = store
    vel = torch.from_numpy(_speeds(9, seed=1)).to(DEV)
    r_aug, s_aug = RadarNoise(seed=5, **SETTINGS["both"]), SpeedNoise(std=2.0, drop_prob=0.3, seed=6)
    first = None
    for skew in (0, 1, 2, 3):
        out = _launch(INDEX, 2, radar=(r_aug, dev), speed=(s_aug, vel), sample_id=sid, skew=skew)
        torch.cuda.synchronize()
        for k, (full, dst) in out.items():
            assert _guards_intact(full, dst.numel(), skew), (k, skew)
            assert not bool((dst == -7.0).any()), (k, skew)
        mine = {k: dst.clone() for k, (_, dst) in out.items()}
        if first is None:
            first = mine
        else:
            assert all(torch.equal(mine[k], first[k]) for k in first), skew
    # one part alone leaves the other's destinations alone
    lone = _launch(INDEX, 2, radar=(r_aug, dev), sample_id=sid)
    assert torch.equal(lone["radar"][1], first["radar"]) and torch.equal(lone["adj"][1], first["adj"]) and "speed" not in lone
    lone = _launch(INDEX, 2, speed=(s_aug, vel), sample_id=sid)
    assert torch.equal(lone["speed"][1], first["speed"]) and _guards_intact(lone["speed"][0], len(INDEX))


# ---------------------------------------------------------------------------------------------- 7. the speed
def test_speed_matches_the_float64_reference():
    from mmfn_amd.data import SpeedNoise
    n = 64
    v = _speeds(n, seed=2)
    dev = torch.from_numpy(v).to(DEV)
    sid = torch.arange(100, 100 + n, dtype=torch.int64, device=DEV)
    index = list(np.random.RandomState(3).permutation(n))
    stored, ids = v[index], [100 + i for i in index]
    for name, aug in (("noise", SpeedNoise(std=4.0, seed=8)), ("both", SpeedNoise(std=1.5, drop_prob=0.5, seed=9)),
                      ("drop", SpeedNoise(std=0.0, drop_prob=0.5, seed=10))):
        for epoch in (0, 1):
            out = _launch(index, epoch, speed=(aug, dev), sample_id=sid)
            dropped = _check_speed(out["speed"][1].cpu().numpy(), stored, ids, aug, epoch, "speed %s epoch %d" % (name, epoch))
            assert _guards_intact(out["speed"][0], n)
            assert (0 < dropped.sum() < n) if aug.drop_thresh else not dropped.any()
    out = _launch(index, 0, speed=(SpeedNoise(drop_prob=1.0), dev), sample_id=sid)
    assert not _bits(out["speed"][1].cpu().numpy()).any()
    got = _launch(index, 0, speed=(SpeedNoise(std=4.0, seed=8), dev), sample_id=sid)["speed"][1].cpu().numpy()
    assert (got[stored == 0.0] >= 0.0).all() and (got[stored == 0.0] > 0.0).any() and (got[stored == 0.0] == 0.0).any()


# ---------------------------------------------------------------------------------------------- 8. determinism
def test_the_result_depends_on_the_seed_the_epoch_and_the_sample_id_only(store):
    from mmfn_amd.data import RadarNoise, SpeedNoise
    radar, dev, sid = store
    vel = torch.from_numpy(np.abs(_speeds(9, seed=1)) + 30.0).to(DEV)                # (far from the floor: every draw shows)
    r_aug, s_aug = RadarNoise(seed=5, **SETTINGS["both"]), SpeedNoise(std=2.0, seed=6)
    run = lambda index, epoch=2, r=r_aug, s=s_aug, table=sid: {k: v[1] for k, v in _launch(index, epoch, radar=(r, dev), speed=(s, vel), sample_id=table).items()}
    base = run(INDEX)
    for index in ([3], [0, 3], [8, 8, 3, 3, 1], list(reversed(INDEX)) + [2, 6]):         # another position, another B, other neighbours
        got = run(index)
        for b, i in enumerate(index):
            if i in INDEX:
                p = INDEX.index(i)
                assert all(torch.equal(got[k][b], base[k][p]) for k in base), (index, i)
    for other in (run(INDEX, epoch=3), run(INDEX, r=RadarNoise(seed=6, **SETTINGS["both"]), s=SpeedNoise(std=2.0, seed=7))):
        for k in base:
            assert not torch.equal(other[k], base[k]), k
            assert not any(torch.equal(other[k][p], base[k][p]) for p in (0, 1, 3, 4, 5)), k     # (samples with many rows)
    # the speed part's seed is its own: another radar seed leaves the speeds alone, and the other way round
    mixed = run(INDEX, r=RadarNoise(seed=6, **SETTINGS["both"]))
    assert torch.equal(mixed["speed"], base["speed"]) and not torch.equal(mixed["radar"], base["radar"])
    mixed = run(INDEX, s=SpeedNoise(std=2.0, seed=7))
    assert torch.equal(mixed["radar"], base["radar"]) and torch.equal(mixed["adj"], base["adj"]) and not torch.equal(mixed["speed"], base["speed"])
    # the id, not the row: another table gives other draws for the same stored rows
    moved = run(INDEX, table=sid + 1)
    assert not torch.equal(moved["radar"], base["radar"]) and not torch.equal(moved["speed"], base["speed"])


# ---------------------------------------------------------------------------------------------- 9. capture
def test_a_captured_launch_follows_the_index_buffer_and_both_states(store):
    from mmfn_amd import ops
    from mmfn_amd.data import RadarNoise, SpeedNoise
    radar, dev, sid = store
    vel = torch.from_numpy(np.abs(_speeds(9, seed=1)) + 30.0).to(DEV)                # (far from the floor: every draw shows)
    r_aug, s_aug = RadarNoise(seed=5, **SETTINGS["both"]), SpeedNoise(std=2.0, drop_prob=0.3, seed=6)
    eager = lambda index, epoch, r=r_aug, s=s_aug: {k: v[1] for k, v in _launch(index, epoch, radar=(r, dev), speed=(s, vel), sample_id=sid).items()}
    first = eager([0, 1, 2], 0)                                        # eager (also loads the library outside the capture)
    index = torch.tensor([0, 1, 2], dtype=torch.int64, device=DEV)
    rstate, sstate = _state(5, 0), _state(6, 0)
    dst = {"radar": torch.empty(3, R, 5, device=DEV), "adj": torch.empty(3, R, R, device=DEV), "speed": torch.empty(3, device=DEV)}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # one launch on the capture stream: no branches
        ops.gather_radar_speed(index, 9, sample_id=sid, radar=_radar_part(r_aug, dev, dst["radar"], dst["adj"], rstate),
                               speed=_speed_part(s_aug, vel, dst["speed"], sstate))
    graph.replay()
    assert all(torch.equal(dst[k], first[k]) for k in dst)
    index.copy_(torch.tensor([8, 3, 5], dtype=torch.int64, device=DEV))
    rstate.copy_(_state(9, 4))
    sstate.copy_(_state(10, 4))
    graph.replay()
    want = eager([8, 3, 5], 4, RadarNoise(seed=9, **SETTINGS["both"]), SpeedNoise(std=2.0, drop_prob=0.3, seed=10))
    assert all(torch.equal(dst[k], want[k]) for k in dst) and not any(torch.equal(dst[k], first[k]) for k in dst)
    sstate.copy_(_state(6, 0))                                         # two buffers: the radar still reads {9, 4}
    graph.replay()
    assert torch.equal(dst["radar"], want["radar"]) and torch.equal(dst["speed"], eager([8, 3, 5], 0)["speed"])


# ---------------------------------------------------------------------------------------------- 10. refusals
def test_bad_descriptors_are_refused_and_nothing_is_launched(store):
    from mmfn_amd import _lib
    radar, dev, sid = store
    n, B = 9, 2
    vel = torch.from_numpy(_speeds(n, seed=1)).to(DEV)
    rstate, sstate = _state(1, 0), _state(2, 0)
    index = torch.tensor([1, 3, 0, 0], dtype=torch.int64, device=DEV)   # (longer than B: the +4-byte pointer below stays inside)
    fulls = {k: _guarded(shape) for k, shape in (("radar", (B, R, 5)), ("adj", (B, R, R)), ("speed", (B,)))}
    fn = _lib.lib().mmfn_gather_radar_speed
    assert _lib.lib().mmfn_sizeof_radar_speed_desc() == ctypes.sizeof(_lib.RadarSpeedDesc)
    EINVAL = -1
    nan = float("nan")
    BOTH = _lib.SIGNAL_RADAR | _lib.SIGNAL_SPEED

    def desc(**over):
        d = _lib.RadarSpeedDesc()
        d.sample_id, d.radar_src, d.radar_dst, d.adj_dst = sid.data_ptr(), dev.data_ptr(), fulls["radar"][1].data_ptr(), fulls["adj"][1].data_ptr()
        d.radar_state, d.speed_src, d.speed_dst, d.speed_state = rstate.data_ptr(), vel.data_ptr(), fulls["speed"][1].data_ptr(), sstate.data_ptr()
        d.parts, d.rows, d.point_thresh, d.depth_std, d.angle_std, d.velocity_std = BOTH, R, 1 << 23, 1.0, 0.05, 1.0
        d.speed_drop_thresh, d.speed_std = 1 << 23, 1.0
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def call(d, idx=index.data_ptr(), b=B, rows=n):
        return fn(ctypes.byref(d) if d is not None else None, idx, b, rows, _lib.stream())

    bad = {
        "d NULL": lambda: call(None),
        "index NULL": lambda: call(desc(), idx=None),
        "index misaligned": lambda: call(desc(), idx=index.data_ptr() + 4),
        "sample_id misaligned": lambda: call(desc(sample_id=sid.data_ptr() + 4)),
        "parts 0": lambda: call(desc(parts=0)),
        "parts 4": lambda: call(desc(parts=4)),
        "parts 7": lambda: call(desc(parts=7)),
        "parts -1": lambda: call(desc(parts=-1)),
        "rows 80": lambda: call(desc(rows=80)),
        "rows 82": lambda: call(desc(rows=82)),
        "rows 0": lambda: call(desc(rows=0)),
        "point_thresh 2^24 + 1": lambda: call(desc(point_thresh=(1 << 24) + 1)),
        "speed_drop_thresh 2^24 + 1": lambda: call(desc(speed_drop_thresh=(1 << 24) + 1)),
        "B -1": lambda: call(desc(), b=-1),
        "B 65536": lambda: call(desc(), b=65536),
        "n 0": lambda: call(desc(), rows=0),
        "n -1": lambda: call(desc(), rows=-1),
    }
    for name in ("radar_src", "radar_dst", "adj_dst", "radar_state", "speed_src", "speed_dst", "speed_state"):
        bad["%s NULL" % name] = lambda name=name: call(desc(**{name: None}))
        bad["%s misaligned" % name] = lambda name=name: call(desc(**{name: getattr(desc(), name) + 2}))
    for name in ("radar_state", "speed_state"):
        bad["%s at 4 bytes" % name] = lambda name=name: call(desc(**{name: getattr(desc(), name) + 4}))
    for name, top in (("depth_std", 4.0), ("angle_std", 0.1), ("velocity_std", 4.0), ("speed_std", 4.0)):
        for v in (-0.01, top * 1.01, nan):
            bad["%s %r" % (name, v)] = lambda name=name, v=v: call(desc(**{name: v}))
    for what, run in bad.items():
        assert run() == EINVAL, what
    assert call(desc(), b=0) == 0 and call(desc(), b=0, rows=0) == 0                  # an empty batch: nothing to do
    torch.cuda.synchronize()
    assert all(bool((full == -7.0).all()) for full, _ in fulls.values())
    # a part that is not carried is not read; thresholds of 2^24 and the stds at their bounds are inside
    assert call(desc(parts=_lib.SIGNAL_SPEED, radar_src=None, radar_dst=None, adj_dst=None, radar_state=None, rows=0, depth_std=nan,
                     point_thresh=(1 << 24) + 1, speed_drop_thresh=1 << 24, speed_std=4.0)) == 0
    torch.cuda.synchronize()
    assert not bool((fulls["speed"][1] == -7.0).any()) and bool((fulls["radar"][0] == -7.0).all()) and bool((fulls["adj"][0] == -7.0).all())
    assert call(desc(parts=_lib.SIGNAL_RADAR, speed_src=None, speed_dst=None, speed_state=None, speed_std=-1.0, speed_drop_thresh=(1 << 24) + 1,
                     point_thresh=1 << 24, depth_std=4.0, angle_std=float(np.float32(0.1)), velocity_std=4.0)) == 0
    assert call(desc(sample_id=None, point_thresh=0, depth_std=0.0, angle_std=0.0, velocity_std=0.0, speed_drop_thresh=0, speed_std=0.0)) == 0
    torch.cuda.synchronize()
    for k, (full, dst) in fulls.items():
        assert not bool((dst == -7.0).any()) and _guards_intact(full, dst.numel()), k


# ---------------------------------------------------------------------------------------------- 11. the loader
RADAR = dict(point_drop=0.3, depth_std=0.5, angle_std=0.02, velocity_std=0.8)
SPEED = dict(std=0.5, drop_prob=0.4)
AUGMENTED = ("radar", "radar_adj", "velocity")


def _pack_store(tmp, samples):
    from mmfn_amd import data as D
    for s in samples:
        s["radar_adj"] = D.radar_adjacency(s["radar"][0])
    return D.PackedFrames(D.pack_frames(samples, str(tmp / "packed")))


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    from oracle import fixtures
    return _pack_store(tmp_path_factory.mktemp("radar"), fixtures.synthetic_samples((5, 9, 3, 7, 1), seed=5, radar_counts=(50, 100, 81, 3, 90)))


def _same_except(got, want, fields):
    (ginp, ggt), (winp, wgt) = got, want
    assert list(ginp) == list(winp) and torch.equal(ggt, wgt)
    for k in winp:
        assert ginp[k].dtype == winp[k].dtype and ginp[k].shape == winp[k].shape and ginp[k].is_contiguous(), k
        if k not in fields:
            assert torch.equal(ginp[k], winp[k]), k


def _check_batch(got, want, idx, radar, speed, epoch, what):
    """The augmented fields of a batch against the references applied to the plain loader's batch of the samples idx."""
    ginp, winp = got[0], want[0]
    if radar is not None:
        _check_radar(ginp["radar"].cpu().numpy(), ginp["radar_adj"].cpu().numpy(), winp["radar"].cpu().numpy(), idx, radar, epoch, what)
    if speed is not None:
        _check_speed(ginp["velocity"].cpu().numpy(), winp["velocity"].cpu().numpy(), idx, speed, epoch, what)


def test_an_augmented_epoch_changes_radar_adjacency_and_speed_only(packed):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    n = len(packed)
    res = D.ResidentFrames(packed, DEV, cfg, "rad", max_bytes=BUDGET)
    plan, nbytes = D.ResidentFrames.plan(packed, cfg, "rad"), res.nbytes()
    radar, speed = D.RadarNoise(seed=11, **RADAR), D.SpeedNoise(seed=12, **SPEED)
    kw = dict(shuffle=True, seed=3, lane_bucket=4)
    aug = D.ResidentLoader(res, 2, augment=D.Augment(radar=radar, speed=speed), **kw)
    plain = D.ResidentLoader(res, 2, **kw)
    assert res.nbytes() == nbytes == plan["bytes"] and set(res.tensors) == set(plan["fields"])      # the store is as it was
    assert set(vars(aug)) - set(vars(plain)) == {"radar_state", "speed_state", "sample_id"} and aug.sample_id.tolist() == list(range(n))
    first, changed = {}, {k: 0 for k in AUGMENTED}
    for epoch in range(2):
        chunks = D._chunks(D._epoch_order(n, True, None, 3, epoch), 2, False)
        got, want = list(aug), list(plain)
        assert len(got) == len(want) == len(chunks)
        for g, w, idx in zip(got, want, chunks):
            _same_except(g, w, AUGMENTED)
            _check_batch(g, w, idx, radar, speed, epoch, "epoch %d batch %s" % (epoch, list(idx)))
            for b, i in enumerate(idx):
                mine = {k: g[0][k][b].clone() for k in AUGMENTED}
                if epoch == 0:
                    first[i] = mine
                else:                                                      # the second epoch: other draws
                    for k in AUGMENTED:
                        changed[k] += int(not torch.equal(mine[k], first[i][k]))
    assert changed["radar"] == changed["radar_adj"] == n and changed["velocity"] >= 2      # (a speed dropped twice is 0.0 twice)
    assert aug.epoch == plain.epoch == 2 and aug.radar_state.tolist() == [11, 1] and aug.speed_state.tolist() == [12, 1]


def test_inactive_parts_are_the_plain_loader_bit_for_bit_stored_adjacency_included(packed):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    res = D.ResidentFrames(packed, DEV, GlobalConfig(), "rad", max_bytes=BUDGET)
    kw = dict(shuffle=True, seed=1, lane_bucket=16)
    plain = list(D.ResidentLoader(res, 2, **kw))
    for aug in (D.Augment(radar=D.RadarNoise(), speed=D.SpeedNoise()), D.Augment(radar=D.RadarNoise(seed=3), speed=D.SpeedNoise(seed=4))):
        loader = D.ResidentLoader(res, 2, augment=aug, **kw)
        assert not any(isinstance(v, torch.Tensor) for v in vars(loader).values()) and loader._states() == {}
        got = list(loader)
        assert len(got) == len(plain)
        for g, w in zip(got, plain):
            _same_except(g, w, ())
    # the stored adjacency is the host's, rounded once: the bits a 'rad' batch has always had
    adj = torch.from_numpy(np.asarray(packed.arrays[res.plan_["arrays"][-1]]).astype(np.float32)).to(DEV)
    order = D._epoch_order(len(packed), True, None, 1, 0)
    assert torch.equal(torch.cat([w[0]["radar_adj"] for w in plain]), adj[list(order)])


def test_speed_alone_on_a_vec_store_changes_velocity_only_and_radar_is_refused_there(packed):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    res = D.ResidentFrames(packed, DEV, GlobalConfig(), "vec", max_bytes=BUDGET)
    with pytest.raises(ValueError):
        D.ResidentLoader(res, 2, augment=D.Augment(radar=D.RadarNoise(point_drop=0.5)))
    with pytest.raises(ValueError):
        res.radar_field()
    speed = D.SpeedNoise(seed=12, **SPEED)
    kw = dict(shuffle=True, seed=3, lane_bucket=4)
    aug, plain = D.ResidentLoader(res, 2, augment=D.Augment(speed=speed), **kw), D.ResidentLoader(res, 2, **kw)
    assert set(vars(aug)) - set(vars(plain)) == {"speed_state", "sample_id"}
    for epoch in range(2):
        chunks = D._chunks(D._epoch_order(len(packed), True, None, 3, epoch), 2, False)
        for g, w, idx in zip(list(aug), list(plain), chunks):
            _same_except(g, w, ("velocity",))
            assert "radar" not in g[0]
            _check_batch(g, w, idx, None, speed, epoch, "vec epoch %d batch %s" % (epoch, list(idx)))
    assert aug.speed_state.tolist() == [12, 1]


def test_together_with_the_other_parts_every_field_matches_its_own_reference(packed):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    res = D.ResidentFrames(packed, DEV, GlobalConfig(), "rad", max_bytes=BUDGET)
    jitter = D.CameraJitter(0.4, 0.4, 0.4, erase_prob=0.5, seed=1)
    lidar, noise = D.LidarDropout(cell_prob=0.1, erase_prob=0.5, seed=2), D.MapNoise(shift=0.5, yaw_deg=2.0, lane_drop=0.5, target_shift=0.5, seed=3)
    radar, speed = D.RadarNoise(seed=4, **RADAR), D.SpeedNoise(seed=5, **SPEED)
    kw = dict(shuffle=True, seed=2, lane_bucket=4)
    every = D.ResidentLoader(res, 2, augment=D.Augment(camera=jitter, lidar=lidar, map=noise, radar=radar, speed=speed), **kw)
    others = D.ResidentLoader(res, 2, augment=D.Augment(camera=jitter, lidar=lidar, map=noise), **kw)     # held to their references elsewhere
    plain = D.ResidentLoader(res, 2, **kw)
    for epoch in range(2):
        chunks = D._chunks(D._epoch_order(len(packed), True, None, 2, epoch), 2, False)
        for g, o, w, idx in zip(list(every), list(others), list(plain), chunks):
            _same_except(g, o, AUGMENTED)                                   # camera, LiDAR, lanes, target point: the other launches' bits
            _same_except(o, w, ("image", "lidar", "lane", "lane_num", "target_point"))
            assert not any(torch.equal(o[0][k], w[0][k]) for k in ("image", "lidar", "target_point"))
            _check_batch(g, w, idx, radar, speed, epoch, "all parts, epoch %d batch %s" % (epoch, list(idx)))
            # the lane reference once more here, on the exact part: which lanes are left
            keep = D.lane_keep_mask(idx, np.minimum(w[0]["lane_num"].cpu().numpy(), w[0]["lane"].shape[1]), noise, epoch)
            assert g[0]["lane_num"].tolist() == keep.sum(axis=1).tolist()
            ref = D.lidar_dropout_reference(w[0]["lidar"].cpu().numpy(), idx, lidar, epoch)
            assert np.array_equal(_bits(g[0]["lidar"].cpu().numpy()), _bits(ref))


def test_a_shard_draws_what_the_full_store_draws(packed):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    aug = D.Augment(radar=D.RadarNoise(seed=4, **RADAR), speed=D.SpeedNoise(std=0.5, seed=6))
    full = D.ResidentFrames(packed, DEV, cfg, "rad", max_bytes=BUDGET)
    shard = D.ResidentFrames(packed, DEV, cfg, "rad", indices=[1, 3], max_bytes=BUDGET)
    a, b = D.ResidentLoader(full, 5, augment=aug), D.ResidentLoader(shard, 2, augment=aug)
    assert b.sample_id.tolist() == [1, 3]
    for epoch in range(2):
        (fa, _), = list(a)
        (fb, _), = list(b)
        for row, i in ((0, 1), (1, 3)):
            assert all(torch.equal(fb[k][row], fa[k][i]) for k in AUGMENTED), (epoch, i)
        assert not torch.equal(fb["radar"][1], fa["radar"][1]) and not torch.equal(fb["velocity"][1], fa["velocity"][1])
    (fs, _), = list(D.ResidentLoader(shard, 2, sampler=[3], augment=aug))             # through a sampler of global ids as well
    a.epoch = 0
    (fa, _), = list(a)
    assert all(torch.equal(fs[k][0], fa[k][3]) for k in AUGMENTED)


# ---------------------------------------------------------------------------------------------- 12. the trainer
def test_two_epochs_of_trainer_train_over_the_augmented_rad_loader(tmp_path):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd import model as M
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import Trainer
    from oracle import fixtures, harness
    oracle = harness.build_oracle("rad", dropout=0.1)
    cfg = GlobalConfig()
    packed = _pack_store(tmp_path, fixtures.synthetic_samples((5, 9, 3, 7), seed=3, radar_counts=(50, 81, 81, 20)))
    res = D.ResidentFrames(packed, DEV, cfg, "rad", max_bytes=BUDGET)
    loader = D.ResidentLoader(res, 2, shuffle=True, seed=2, lane_bucket=16,
                              augment=D.Augment(radar=D.RadarNoise(seed=1, **RADAR), speed=D.SpeedNoise(seed=2, **SPEED)))
    net = M.MMFN(cfg, DEV, "rad")
    net.load_state_dict(oracle.state_dict(), strict=True)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    tr = Trainer(DEV, None)
    opt = FusedAdamW(net, lr=1e-4)
    for _ in range(2):
        tr.train(net, loader, cfg, opt, graph=True, lane_bucket=16)
    assert len(tr.train_loss) == 2 and all(np.isfinite(v) for v in tr.train_loss) and tr.cur_iter == 4
    assert len(tr._static_steps) == 1 and not isinstance(next(iter(tr._static_steps.values())), str)    # one 16-lane bucket, captured
    after = net.state_dict()
    changed = [k for k in before if before[k].dtype == torch.float32 and not torch.equal(before[k], after[k])]
    assert len(changed) > len(before) // 2 and all(bool(torch.isfinite(after[k]).all()) for k in changed)
    assert loader.epoch == 2 and loader.radar_state.tolist() == [1, 1] and loader.speed_state.tolist() == [2, 1]
