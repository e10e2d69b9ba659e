"""Radar dropout and noise, speed noise of the resident loader, host side: the settings objects, the integer draws and the float64
numpy references the GPU tests hold mmfn_gather_radar_speed to (data.radar_noise_reference, data.speed_noise_reference), each
against an independent statement of what it promises.  No GPU."""
import numpy as np
import pytest
import torch

NAN = float("nan")


def _radar(counts, seed=0):
    """f32 [len(counts), 81, 5]: counts[b] real rows (depth in (0.5, 100), angles within +/-0.6, velocity within +/-40, a 0 / 1
    flag - the first real row's flag is 1 so that no real row is all zero), zero rows after them."""
    rng = np.random.RandomState(seed)
    out = np.zeros((len(counts), 81, 5), dtype=np.float32)
    for b, m in enumerate(counts):
        out[b, :m, 0] = rng.uniform(0.5, 100.0, m)
        out[b, :m, 1:3] = rng.uniform(-0.6, 0.6, (m, 2))
        out[b, :m, 3] = rng.uniform(-40.0, 40.0, m)
        out[b, :m, 4] = rng.randint(0, 2, m)
    return out


# ---------------------------------------------------------------------------------------------- 1. settings
def test_radar_noise_validates_its_settings():
    from mmfn_amd.data import RadarNoise
    r = RadarNoise()
    assert (r.point_drop, r.depth_std, r.angle_std, r.velocity_std, r.seed) == (0.0, 0.0, 0.0, 0.0, 0)
    assert r.point_thresh == 0 and not r.active and r.column_std == (0.0, 0.0, 0.0, 0.0)
    assert RadarNoise(point_drop=0.5).point_thresh == 1 << 23 and RadarNoise(point_drop=1.0).point_thresh == 1 << 24
    assert RadarNoise(point_drop=0.25).point_thresh == 0.25 * (1 << 24)
    for cfg in (dict(point_drop=0.1), dict(depth_std=0.1), dict(angle_std=0.01), dict(velocity_std=0.1)):
        assert RadarNoise(**cfg).active
    assert not RadarNoise(seed=9).active and isinstance(RadarNoise(seed=7.0).seed, int)
    f32 = lambda v: float(np.float32(v))
    assert RadarNoise(depth_std=0.3, angle_std=0.02, velocity_std=0.7).column_std == (f32(0.3), f32(0.02), f32(0.02), f32(0.7))
    for name, top in (("point_drop", 1.0), ("depth_std", 4.0), ("angle_std", 0.1), ("velocity_std", 4.0)):
        for bad in (-0.01, top * 1.01, NAN):
            with pytest.raises(ValueError):
                RadarNoise(**{name: bad})
        RadarNoise(**{name: 0.0}), RadarNoise(**{name: top})


def test_speed_noise_validates_its_settings():
    from mmfn_amd.data import SpeedNoise
    s = SpeedNoise()
    assert (s.std, s.drop_prob, s.seed) == (0.0, 0.0, 0) and s.drop_thresh == 0 and not s.active
    assert SpeedNoise(drop_prob=0.5).drop_thresh == 1 << 23 and SpeedNoise(drop_prob=1.0).drop_thresh == 1 << 24
    assert SpeedNoise(std=0.1).active and SpeedNoise(drop_prob=0.1).active and not SpeedNoise(seed=3).active
    for name, top in (("std", 4.0), ("drop_prob", 1.0)):
        for bad in (-0.01, top * 1.01, NAN):
            with pytest.raises(ValueError):
                SpeedNoise(**{name: bad})
        SpeedNoise(**{name: 0.0}), SpeedNoise(**{name: top})


def test_augment_takes_the_radar_and_speed_parts_by_type():
    from mmfn_amd.data import Augment, CameraJitter, MapNoise, RadarNoise, SpeedNoise
    a = Augment()
    assert a.radar is None and a.speed is None and a.camera is None and a.lidar is None and a.map is None and a.degrade is None
    r, s = RadarNoise(0.1), SpeedNoise(0.5)
    a = Augment(radar=r, speed=s)
    assert a.radar is r and a.speed is s and a.map is None
    for bad in (dict(radar=s), dict(speed=r), dict(radar=MapNoise(0.5)), dict(speed=CameraJitter(0.4)), dict(radar={"point_drop": 0.1}),
                dict(speed=0.5), dict(camera=r), dict(map=s)):
        with pytest.raises(TypeError):
            Augment(**bad)


class _Store(object):
    """Stands in for a ResidentFrames: a loader whose parts are all inactive touches nothing of it at construction."""
    device = torch.device("cpu")
    n = 4
    indices = np.arange(4)

    def __len__(self):
        return self.n


class _VecStore(_Store):
    """A store without a radar field, with the real store's own check."""
    variant = "vec"

    def radar_field(self):
        from mmfn_amd.data import ResidentFrames
        return ResidentFrames.radar_field(self)


def test_inactive_parts_are_the_plain_loader_and_radar_on_a_vec_store_is_refused():
    from mmfn_amd.data import Augment, RadarNoise, ResidentLoader, SpeedNoise
    plain = set(vars(ResidentLoader(_Store(), 2)))
    for aug in (Augment(radar=RadarNoise(), speed=SpeedNoise()), Augment(radar=RadarNoise(seed=3)), Augment(speed=SpeedNoise(seed=4))):
        loader = ResidentLoader(_Store(), 2, augment=aug)
        assert loader.augment is aug and set(vars(loader)) == plain and loader._states() == {}
        assert not any(isinstance(v, (torch.Tensor, np.ndarray)) for v in vars(loader).values())
    for bad in (RadarNoise(0.1), SpeedNoise(0.1), {"radar": RadarNoise(0.1)}):
        with pytest.raises(TypeError):
            ResidentLoader(_Store(), 2, augment=bad)
    for part in (dict(point_drop=0.1), dict(depth_std=0.1), dict(angle_std=0.01), dict(velocity_std=0.1)):
        with pytest.raises(ValueError):
            ResidentLoader(_VecStore(), 2, augment=Augment(radar=RadarNoise(**part)))
    # the speed part works on every variant: the loader holds its state and the sample ids, nothing else
    loader = ResidentLoader(_VecStore(), 2, augment=Augment(speed=SpeedNoise(std=0.5, seed=6)))
    assert set(vars(loader)) - plain == {"speed_state", "sample_id"} and loader.sample_id.tolist() == [0, 1, 2, 3]
    extra = loader._states()["augment"]
    assert set(extra) == {"speed", "sample_id"} and loader.speed_state.tolist() == [6, 0]


def test_radar_on_a_vec_plan_is_refused(tmp_path):
    """The real store's own check, on a plan built without a device."""
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from oracle import fixtures
    samples = fixtures.synthetic_samples((3, 2), seed=1, radar_counts=(5, 81))
    for s in samples:
        s["radar_adj"] = D.radar_adjacency(s["radar"][0])
    packed = D.PackedFrames(D.pack_frames(samples, str(tmp_path / "packed")))
    for variant in ("vec", "rad"):
        res = D.ResidentFrames.__new__(D.ResidentFrames)
        plan = D.ResidentFrames.plan(packed, GlobalConfig(), variant)
        res.variant, res.seq_len, res.plan_, res.device, res.indices = variant, 1, plan, torch.device("cpu"), plan["rows"]
        res.shapes = {nm: tuple(packed.arrays[nm].shape[1:]) for nm in plan["arrays"]}
        res.tensors = {nm: torch.zeros((2,) + res.shapes[nm]).flatten(1) for nm in plan["arrays"] if "radar" in nm}
        if variant == "vec":
            with pytest.raises(ValueError):
                res.radar_field()
            with pytest.raises(ValueError):
                D.ResidentLoader(res, 2, augment=D.Augment(radar=D.RadarNoise(point_drop=0.5)))
        else:
            assert tuple(res.radar_field().shape) == (2, 405)
            loader = D.ResidentLoader(res, 2, augment=D.Augment(radar=D.RadarNoise(point_drop=0.5, seed=8)))
            assert loader.radar_state.tolist() == [0, 0] and loader._states()["augment"]["radar"][1].tolist() == [8, 0]


# ---------------------------------------------------------------------------------------------- 2. draws
def test_the_draws_are_24_bit_deterministic_and_streams_of_their_own():
    from mmfn_amd import data as D
    ids = [0, 1, 5, 1 << 40]
    k = D.radar_draws(3, 2, ids)
    assert k.shape == (4, 81) and k.dtype == np.int64 and k.min() >= 0 and k.max() < 1 << 24
    assert np.array_equal(k, D.radar_draws(3, 2, ids)) and np.array_equal(k[2], D.radar_draws(3, 2, [5])[0])
    assert not np.array_equal(k, D.radar_draws(4, 2, ids)) and not np.array_equal(k, D.radar_draws(3, 3, ids))
    want = D.rng_u32(3, 2, D.RNG_STREAM_RADAR, np.uint64(5 * 128) + np.arange(81, dtype=np.uint64)) >> np.uint64(8)
    assert np.array_equal(k[2], want.astype(np.int64))
    s = D.speed_draws(3, 2, ids)
    assert s.shape == (4, 8) and s.min() >= 0 and s.max() < 1 << 24 and np.array_equal(s, D.speed_draws(3, 2, ids))
    streams = [D.RNG_STREAM_RADAR, D.RNG_STREAM_RADAR_NOISE, D.RNG_STREAM_SPEED, D.RNG_STREAM_JITTER, D.RNG_STREAM_DEGRADE,
               D.RNG_STREAM_PIXEL_NOISE, D.RNG_STREAM_LIDAR, D.RNG_STREAM_LIDAR_CELL, D.RNG_STREAM_MAP, D.RNG_STREAM_LANE]
    assert len(set(streams)) == len(streams)
    # the same (seed, epoch, id): the radar, speed, map and LiDAR draws all differ
    eight = [k[:, :8], s, D.map_draws(3, 2, ids), D.lidar_draws(3, 2, ids)]
    for a in range(4):
        for b in range(a + 1, 4):
            assert not (eight[a] == eight[b]).any(axis=1).all()
    z = D.radar_normals(3, 2, ids)
    assert z.shape == (4, 81, 4) and np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(48 * np.log(2.0)) + 1e-12
    q = (np.uint64(5 * 128 + 7) * np.uint64(4) + np.uint64(2)) * np.uint64(2)
    k0, k1 = (int(D.rng_u32(3, 2, D.RNG_STREAM_RADAR_NOISE, [q + np.uint64(j)])[0]) >> 8 for j in (0, 1))
    assert z[2, 7, 2] == np.sqrt(-2.0 * np.log((k0 + 1) / 16777216.0)) * np.cos(2.0 * np.pi * (k1 / 16777216.0))


def test_the_keep_mask_never_drops_or_counts_a_padding_row():
    from mmfn_amd import data as D
    counts = (0, 1, 63, 64, 65, 80, 81)
    radar, ids = _radar(counts, seed=1), [10, 11, 12, 13, 14, 15, 16]
    real = np.arange(81)[None, :] < np.array(counts)[:, None]
    for epoch in range(2):
        keep = D.radar_keep_mask(radar, ids, D.RadarNoise(point_drop=0.5, seed=2), epoch)
        assert keep.shape == (7, 81) and keep.dtype == bool and not keep[~real].any()
        assert np.array_equal(keep, real & (D.radar_draws(2, epoch, ids) >= 1 << 23))
        assert 0 < keep[6].sum() < 81
    assert not D.radar_keep_mask(radar, ids, D.RadarNoise(point_drop=1.0), 0).any()
    assert np.array_equal(D.radar_keep_mask(radar, ids, D.RadarNoise(point_drop=0.0, depth_std=1.0), 0), real)
    # a zero row between real ones is padding as well, and -0.0 is zero
    holes = radar.copy()
    holes[6, 40] = 0.0
    holes[6, 41] = -0.0
    keep = D.radar_keep_mask(holes, ids, D.RadarNoise(), 0)
    assert not keep[6, 40] and not keep[6, 41] and keep[6].sum() == 79


# ---------------------------------------------------------------------------------------------- 3. reference semantics
def test_kept_rows_close_up_and_a_rows_noise_does_not_depend_on_the_other_rows():
    from mmfn_amd import data as D
    counts = (0, 1, 63, 64, 65, 80, 81)
    radar, ids = _radar(counts, seed=2), [3, 1, 4, 1 << 33, 5, 9, 2]
    stds = dict(depth_std=0.5, angle_std=0.02, velocity_std=0.8)
    full, _ = D.radar_noise_reference(radar, ids, D.RadarNoise(point_drop=0.0, seed=6, **stds), 1)
    half_aug = D.RadarNoise(point_drop=0.5, seed=6, **stds)
    half, adj = D.radar_noise_reference(radar, ids, half_aug, 1)
    keep = D.radar_keep_mask(radar, ids, half_aug, 1)
    assert full.dtype == half.dtype == adj.dtype == np.float64 and half.shape == (7, 81, 5) and adj.shape == (7, 81, 81)
    for b, m in enumerate(counts):
        rows = np.flatnonzero(keep[b])
        assert np.array_equal(half[b, :len(rows)], full[b, rows])              # stored order, the noise of the STORED row
        assert not half[b, len(rows):].any() and not np.signbit(half[b, len(rows):]).any()
        assert not full[b, m:].any()
        assert np.array_equal(half[b, :len(rows), 4], radar[b, rows, 4].astype(np.float64))      # the flag
        assert np.array_equal(full[b, :m, 4], radar[b, :m, 4].astype(np.float64))
        if m:
            assert (full[b, :m, :4] != radar[b, :m, :4]).all() and (full[b, :m, 0] >= 0.0).all()
        # the adjacency: antisymmetric, zero diagonal, the column-1 differences on the kept block, zero between padding rows
        a, col, n_k = adj[b], half[b, :, 1], len(rows)
        assert np.array_equal(a, -a.T) and not np.diagonal(a).any()
        assert np.array_equal(a[:n_k, :n_k], col[None, :n_k] - col[:n_k, None]) and not a[n_k:, n_k:].any()
        assert np.array_equal(a[n_k:, :n_k], np.broadcast_to(col[None, :n_k], (81 - n_k, n_k)))
        assert np.array_equal(a, D.radar_adjacency(half[b]))
    assert 0 < keep[6].sum() < 81


def test_zero_stds_copy_the_bits_and_the_depth_is_clamped():
    from mmfn_amd import data as D
    radar, ids = _radar((81, 40), seed=3), [7, 8]
    out, adj = D.radar_noise_reference(radar, ids, D.RadarNoise(seed=1), 0)
    assert np.array_equal(out.astype(np.float32).view(np.uint32), radar.view(np.uint32))
    assert np.array_equal(adj, radar[:, None, :, 1].astype(np.float64) - radar[:, :, None, 1].astype(np.float64))
    only = D.radar_noise_reference(radar, ids, D.RadarNoise(velocity_std=1.0, seed=1), 0)[0]
    assert np.array_equal(only[..., (0, 1, 2, 4)], radar[..., (0, 1, 2, 4)].astype(np.float64)) and (only[0, :, 3] != radar[0, :, 3]).all()
    near = radar.copy()
    near[:, :, 0] = np.where(near[:, :, 0] > 0, 0.01, 0.0)
    depth = D.radar_noise_reference(near, ids, D.RadarNoise(depth_std=4.0, seed=1), 0)[0][..., 0]
    assert depth.min() == 0.0 and (depth[0] == 0.0).sum() > 20 and (depth[0] > 0.0).sum() > 20
    z = D.radar_normals(1, 0, ids)
    f32 = float(np.float32(0.01))
    assert np.array_equal(depth[0], np.maximum(f32 + 4.0 * z[0, :, 0], 0.0))


# ---------------------------------------------------------------------------------------------- 4. moments
def test_moments_of_the_radar_noise_over_20000_fixed_draws():
    from mmfn_amd import data as D
    ids = np.arange(250) + 1000                                   # 250 samples x 81 rows = 20 250 draws per column
    radar = np.zeros((250, 81, 5), dtype=np.float32)
    radar[:] = np.array([50.0, 0.1, -0.2, 3.0, 1.0], dtype=np.float32)
    aug = D.RadarNoise(depth_std=2.0, angle_std=0.05, velocity_std=1.5, seed=12)
    out, _ = D.radar_noise_reference(radar, ids, aug, 3)
    for c, std in enumerate(aug.column_std):
        noise = (out[..., c] - float(radar[0, 0, c])).reshape(-1)
        assert noise.size >= 20000
        print("column %d: mean %.4f std, std %.4f of the one asked for" % (c, noise.mean() / std, noise.std() / std))
        assert abs(noise.mean()) <= 0.03 * std and abs(noise.std() / std - 1.0) <= 0.02
    assert np.array_equal(out[..., 4], radar[..., 4].astype(np.float64))


def test_moments_of_the_speed_noise_and_its_floor():
    from mmfn_amd import data as D
    ids = np.arange(20000)
    v = np.full(20000, 30.0, dtype=np.float32)
    noise = D.speed_noise_reference(v, ids, D.SpeedNoise(std=2.0, seed=5), 1) - 30.0
    print("speed: mean %.4f std, std %.4f of the one asked for" % (noise.mean() / 2.0, noise.std() / 2.0))
    assert abs(noise.mean()) <= 0.03 * 2.0 and abs(noise.std() / 2.0 - 1.0) <= 0.02
    # never below min(v, 0): a standing car stays standing or moves forward, a negative stored speed is not clamped above itself
    rng = np.random.RandomState(2)
    v = np.concatenate([np.zeros(5000), rng.uniform(0.0, 1.0, 5000), rng.uniform(-3.0, 0.0, 5000), rng.uniform(1.0, 60.0, 5000)]).astype(np.float32)
    aug = D.SpeedNoise(std=4.0, seed=6)
    out = D.speed_noise_reference(v, ids, aug, 0)
    k = D.speed_draws(6, 0, ids)
    z = np.sqrt(-2.0 * np.log((k[:, 1] + 1.0) / 16777216.0)) * np.cos(2.0 * np.pi * (k[:, 2] / 16777216.0))
    assert (out >= np.minimum(v, 0.0)).all() and (out[:10000] >= 0.0).all()
    assert np.array_equal(out, np.maximum(v.astype(np.float64) + 4.0 * z, np.minimum(v.astype(np.float64), 0.0)))
    assert (out[:5000] == 0.0).sum() > 2000 and (out[:5000] > 0.0).sum() > 2000
    neg = slice(10000, 15000)
    assert (out[neg] < v[neg]).sum() == 0 and (out[neg] == v[neg]).sum() > 2000 and (out[neg] > 0.0).any()
    # the dropped share, and what is not dropped keeps its bits while std is 0
    aug = D.SpeedNoise(drop_prob=0.5, seed=7)
    out = D.speed_noise_reference(v, ids, aug, 2)
    dropped = D.speed_draws(7, 2, ids)[:, 0] < aug.drop_thresh
    print("dropped share %.4f" % dropped.mean())
    assert abs(dropped.mean() - 0.5) <= 0.02
    assert not out[dropped].any() and not np.signbit(out[dropped]).any()
    assert np.array_equal(out[~dropped].astype(np.float32).view(np.uint32), v[~dropped].view(np.uint32))
    assert not D.speed_noise_reference(v, ids, D.SpeedNoise(drop_prob=1.0), 0).any()
    assert np.array_equal(D.speed_noise_reference(v, ids, D.SpeedNoise(), 0), v.astype(np.float64))
