"""LiDAR dropout, lane dropout and map noise of the resident loader, host side: the settings objects, the integer draws and the
numpy references the GPU tests hold the kernel to.  No GPU."""
import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------- settings
def test_lidar_dropout_validates_its_settings():
    from mmfn_amd.data import CameraJitter, LidarDropout
    a = LidarDropout()
    assert (a.cell_prob, a.erase_prob, a.erase_scale, a.seed) == (0.0, 0.0, (0.1, 0.3), 0)
    assert a.cell_thresh == 0 and a.erase_thresh == 0
    assert LidarDropout(cell_prob=0.5).cell_thresh == 1 << 23 and LidarDropout(cell_prob=1.0).cell_thresh == 1 << 24
    assert LidarDropout(erase_prob=0.5).erase_thresh == 1 << 23 and LidarDropout(erase_prob=1.0).erase_thresh == 1 << 24
    for name in ("cell_prob", "erase_prob"):
        for bad in (-0.01, 1.01, float("nan")):
            with pytest.raises(ValueError):
                LidarDropout(**{name: bad})
        LidarDropout(**{name: 0.0}), LidarDropout(**{name: 1.0})
    for bad in ((0.3, 0.1), (0.0, 0.3), (0.1, 1.5), 0.2, ("a", "b")):
        with pytest.raises(ValueError):
            LidarDropout(erase_scale=bad)
    # the rectangle's bounds are the camera jitter's: one piece of code
    for side in (1, 5, 8, 256):
        assert LidarDropout(erase_scale=(0.1, 0.3)).erase_bounds(side) == CameraJitter(erase_scale=(0.1, 0.3)).erase_bounds(side)
    assert LidarDropout.erase_bounds is CameraJitter.erase_bounds
    assert isinstance(LidarDropout(seed=7).seed, int)


def test_map_noise_validates_its_settings():
    from mmfn_amd.data import MapNoise
    m = MapNoise()
    assert (m.shift, m.yaw_deg, m.lane_drop, m.target_shift, m.seed) == (0.0, 0.0, 0.0, 0.0, 0)
    assert m.lane_thresh == 0 and MapNoise(lane_drop=0.5).lane_thresh == 1 << 23 and MapNoise(lane_drop=1.0).lane_thresh == 1 << 24
    for name, top in (("shift", 64.0), ("target_shift", 64.0), ("yaw_deg", 45.0), ("lane_drop", 1.0)):
        for bad in (-0.01, top * 1.01, float("nan")):
            with pytest.raises(ValueError):
                MapNoise(**{name: bad})
        MapNoise(**{name: 0.0}), MapNoise(**{name: top})
    y = MapNoise(yaw_deg=45.0).yaw_rad
    assert isinstance(y, np.float32) and y == np.float32(np.pi / 4) and MapNoise(yaw_deg=2.0).yaw_rad == np.float32(2.0 * np.pi / 180.0)
    assert float(y) <= np.pi / 4 + 1e-6                                       # inside the bound the C entry checks


def test_augment_takes_the_three_parts_by_type():
    from mmfn_amd.data import Augment, CameraJitter, LidarDropout, MapNoise
    a = Augment()
    assert a.camera is None and a.lidar is None and a.map is None
    j, l, m = CameraJitter(0.4), LidarDropout(0.1), MapNoise(0.5)
    a = Augment(camera=j, lidar=l, map=m)
    assert a.camera is j and a.lidar is l and a.map is m
    for bad in (dict(camera=l), dict(lidar=j), dict(map=l), dict(camera={"brightness": 0.4}), dict(map=0.5)):
        with pytest.raises(TypeError):
            Augment(**bad)


class _Store(object):
    """Stands in for a ResidentFrames: a loader whose parts are all inactive touches nothing of it at construction."""
    device = torch.device("cpu")
    n = 4
    indices = np.arange(4)

    def __len__(self):
        return self.n


def test_the_loaders_type_checks_and_inactive_parts():
    from mmfn_amd.data import Augment, LidarDropout, MapNoise, ResidentLoader
    plain = set(vars(ResidentLoader(_Store(), 2)))
    for aug in (Augment(), Augment(lidar=LidarDropout(), map=MapNoise())):
        loader = ResidentLoader(_Store(), 2, augment=aug)
        assert loader.augment is aug and set(vars(loader)) == plain            # no state, no sample ids: the plain launch
        assert not any(isinstance(v, (torch.Tensor, np.ndarray)) for v in vars(loader).values())
        assert loader._states() == {}
    for bad in ({"lidar": LidarDropout(0.1)}, LidarDropout(0.1), MapNoise(0.5), "all"):
        with pytest.raises(TypeError):
            ResidentLoader(_Store(), 2, augment=bad)


# ---------------------------------------------------------------------------------------------- draws
def test_draws_are_deterministic_24_bit_and_keyed_by_seed_epoch_id_and_stream():
    from mmfn_amd.data import jitter_draws, lidar_draws, map_draws
    ids = np.arange(64)
    for draws in (lidar_draws, map_draws):
        a = draws(3, 5, ids)
        assert a.dtype == np.int64 and a.shape == (64, 8)
        assert np.array_equal(a, draws(3, 5, ids)) and np.array_equal(a[[7, 2]], draws(3, 5, [7, 2]))
        assert a.min() >= 0 and a.max() < 1 << 24 and a.max() > 1 << 23 and a.min() < 1 << 21
        for other in (draws(4, 5, ids), draws(3, 6, ids), draws(3, 5, ids + 64), jitter_draws(3, 5, ids)):
            assert (other != a).mean() > 0.99
        big = draws(2 ** 63 + 11, 2 ** 40, [2 ** 40 + 3, 0])      # ids past 2^32 / 8: still 24 bits, the high index word folded in
        assert big.min() >= 0 and big.max() < 1 << 24 and not np.array_equal(big[0], draws(2 ** 63 + 11, 2 ** 40, [3])[0])
    assert (lidar_draws(3, 5, ids) != map_draws(3, 5, ids)).mean() > 0.99


def test_cell_and_lane_indices_past_32_bits_do_not_overflow():
    from mmfn_amd.data import LidarDropout, MapNoise, lane_keep_mask, lidar_dropout_reference
    x = np.ones((2, 2, 4, 8), dtype=np.float32)
    aug = LidarDropout(cell_prob=0.5, seed=3)
    big = 2 ** 32 // 64 + 5                                       # id * (C * H * W) passes 2^32
    out = lidar_dropout_reference(x, [big, 5], aug, 5)
    assert 16 <= (out[0] == 0).sum() <= 48 and not np.array_equal(out[0], out[1])
    huge = lidar_dropout_reference(x, [2 ** 62, 2 ** 62 + 1], aug, 5)          # id * 64 wraps mod 2^64, as the kernel's uint64 does
    assert np.array_equal(huge[0], lidar_dropout_reference(x[:1], [0], aug, 5)[0])
    m = MapNoise(lane_drop=0.5, seed=3)
    keep = lane_keep_mask([2 ** 20, 4], [12, 12], m, 5)           # id * 65536 passes 2^32
    assert keep.shape == (2, 12) and keep[:, 0].all() and not np.array_equal(keep[0], keep[1])


# ---------------------------------------------------------------------------------------------- identity
def test_zero_strengths_return_the_inputs_bits():
    from mmfn_amd.data import LidarDropout, MapNoise, lidar_dropout_reference, map_noise_reference
    odd = np.array([0x80000000, 0x7FC12345, 0x00000001, 0x3F800000], dtype=np.uint32).view(np.float32)      # -0.0, a NaN payload, ...
    frames = np.resize(odd, (3, 2, 5, 7)).astype(np.float32)
    out = lidar_dropout_reference(frames, [0, 1, 2], LidarDropout(seed=9), 4)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), frames.view(np.uint32)) and out is not frames
    lanes = np.resize(odd, (3, 4, 10, 5)).astype(np.float32)
    tp = np.resize(odd, (3, 2)).astype(np.float32)
    got, counts, tps = map_noise_reference(lanes, [4, 2, 6], tp, [0, 1, 2], MapNoise(seed=9), 4)
    want = lanes.copy()
    want[1, 2:] = 0.0                                                          # rows past the count are +0.0 padding
    assert np.array_equal(got.astype(np.float32).view(np.uint32), want.view(np.uint32))
    assert counts.tolist() == [4, 2, 6] and np.array_equal(tps.astype(np.float32).view(np.uint32), tp.view(np.uint32))


# ---------------------------------------------------------------------------------------------- LiDAR
def test_the_cell_mask_has_the_rate_it_was_asked_for():
    """A cap so the statistics cannot hide a dead mask: seed 3, epoch 5, [2, 64, 64], ids 0..3."""
    from mmfn_amd.data import LidarDropout, lidar_dropout_reference
    x = np.full((4, 2, 64, 64), 3.0, dtype=np.float32)
    for p in (0.25, 0.5):
        out = lidar_dropout_reference(x, np.arange(4), LidarDropout(cell_prob=p, seed=3), 5)
        assert set(np.unique(out)) == {0.0, 3.0}
        for i in range(4):
            assert abs((out[i] == 0).mean() - p) <= 0.03, (p, i)
    small = lidar_dropout_reference(np.ones((6, 2, 4, 8), np.float32), np.arange(6), LidarDropout(cell_prob=0.5, seed=3), 5)
    assert all(31 <= int((small[i] == 0).sum()) <= 40 for i in range(6))
    one = np.ones((1, 2, 64, 64), np.float32)
    e5 = lidar_dropout_reference(one, [0], LidarDropout(cell_prob=0.5, seed=3), 5) == 0
    e6 = lidar_dropout_reference(one, [0], LidarDropout(cell_prob=0.5, seed=3), 6) == 0
    assert 0.47 <= (e5 == e6).mean() <= 0.53                                   # two epochs: independent masks (49.5 % agree)
    assert np.array_equal(lidar_dropout_reference(one, [0], LidarDropout(cell_prob=1.0), 0), np.zeros_like(one))


def test_the_erased_rectangle_takes_every_channel_and_nothing_else():
    from mmfn_amd.data import LidarDropout, erase_rectangle, lidar_draws, lidar_dropout_reference
    aug = LidarDropout(erase_prob=1.0, erase_scale=(0.2, 0.5), seed=2)
    x = np.full((5, 2, 12, 9), 2.0, dtype=np.float32)
    ids = [0, 1, 2, 3, 2 ** 33]
    out = lidar_dropout_reference(x, ids, aug, 1)
    rects = set()
    for i, k in enumerate(lidar_draws(2, 1, ids)):
        y0, x0, h, w = erase_rectangle(k, aug, 12, 9)
        rects.add((y0, x0, h, w))
        inside = np.zeros((12, 9), dtype=bool)
        inside[y0:y0 + h, x0:x0 + w] = True
        assert np.array_equal(out[i] == 0, np.broadcast_to(inside, (2, 12, 9)))
    assert len(rects) > 1
    never = lidar_dropout_reference(x, ids, LidarDropout(erase_prob=0.0, seed=2), 1)
    assert np.array_equal(never, x)


# ---------------------------------------------------------------------------------------------- lanes
def _lanes(rng, counts, lmax, nodes=10):
    lanes = np.zeros((len(counts), lmax, nodes, 5), dtype=np.float32)
    for b, c in enumerate(counts):
        lanes[b, :min(c, lmax)] = rng.uniform(-64, 64, (min(c, lmax), nodes, 5)).astype(np.float32)
    return lanes


def test_lane_dropout_keeps_lane_0_and_the_order_and_counts_what_it_dropped():
    from mmfn_amd.data import MapNoise, lane_keep_mask, map_noise_reference
    m = MapNoise(lane_drop=0.5, seed=3)
    keep = lane_keep_mask(np.arange(6), [12] * 6, m, 5)
    assert keep.dtype == bool and keep.shape == (6, 12) and keep[:, 0].all()
    dropped = (~keep[:, 1:]).sum(axis=1)
    assert all(4 <= d <= 7 for d in dropped)                       # at least one dropped and one kept in every sample
    rng = np.random.RandomState(1)
    counts = [12, 0, 1, 12, 14, 5]                                 # 14 > lmax: only the first 12 stored lanes take part
    lanes = _lanes(rng, counts, 12)
    tp = rng.randn(6, 2).astype(np.float32)
    got, out_counts, tps = map_noise_reference(lanes, counts, tp, np.arange(6), m, 5)
    keep = lane_keep_mask(np.arange(6), np.minimum(counts, 12), m, 5)
    assert not keep[1].any() and keep[2].tolist() == [True] + [False] * 11 and not keep[5, 5:].any()
    for b, c in enumerate(counts):
        rows = np.flatnonzero(keep[b])
        assert out_counts[b] == c - (min(c, 12) - len(rows))
        assert np.array_equal(got[b, :len(rows)], lanes[b, rows].astype(np.float64))          # stored order, values untouched
        assert not got[b, len(rows):].any() and not np.signbit(got[b, len(rows):]).any()       # +0.0 from there on
    assert out_counts[4] == 14 - (12 - keep[4].sum()) and np.array_equal(tps, tp.astype(np.float64))
    all_gone = lane_keep_mask([0, 1], [5, 3], MapNoise(lane_drop=1.0), 0)
    assert all_gone[:, 0].all() and not all_gone[:, 1:].any()
    assert lane_keep_mask([], [], m, 0).shape == (0, 0)


def _id_with_w(j, lo, hi, seed, epoch):
    """The first sample id whose map draw w_j lies in [lo, hi)."""
    from mmfn_amd.data import map_draws
    ids = np.arange(4096)
    w = 2.0 * map_draws(seed, epoch, ids)[:, j] / 16777216.0 - 1.0
    return int(ids[(w >= lo) & (w < hi)][0])


def test_the_rigid_transform_of_a_hand_computed_node():
    """yaw_deg = 45 and an id whose w_2 is close to +1: the node (1, 0) turns towards (cos, sin) of almost 45 degrees and then
    moves by shift * (w_0, w_1); f2..f4 stay; an all-zero node does not move."""
    from mmfn_amd.data import MapNoise, map_draws, map_noise_reference
    m = MapNoise(shift=2.0, yaw_deg=45.0, target_shift=3.0, seed=6)
    i = _id_with_w(2, 0.9, 1.0, 6, 2)
    k = map_draws(6, 2, [i])[0]
    w = [2.0 * int(v) / 2.0 ** 24 - 1.0 for v in k]
    assert 0.9 <= w[2] < 1.0
    lanes = np.zeros((1, 2, 3, 5), dtype=np.float32)
    lanes[0, 0, 0] = [1.0, 0.0, 7.0, 8.0, 9.0]
    lanes[0, 0, 1] = [0.0, 2.0, 0.0, 0.0, 0.0]
    lanes[0, 1, 0] = [0.0, 0.0, 0.0, 0.0, 1.0]                                 # x = y = 0 but not padding: it moves
    got, counts, tp = map_noise_reference(lanes, [2], [[10.0, -20.0]], [i], m, 2)
    theta = float(np.float32(45.0 * np.pi / 180.0)) * w[2]
    c, s = np.cos(theta), np.sin(theta)
    assert 0.63 < s < 0.7072 and 0.7071 < c < 0.78
    tx, ty = 2.0 * w[0], 2.0 * w[1]
    assert np.allclose(got[0, 0, 0], [c + tx, s + ty, 7.0, 8.0, 9.0], rtol=0, atol=1e-12)
    assert np.allclose(got[0, 0, 1], [-2.0 * s + tx, 2.0 * c + ty, 0.0, 0.0, 0.0], rtol=0, atol=1e-12)
    assert np.allclose(got[0, 1, 0], [tx, ty, 0.0, 0.0, 1.0], rtol=0, atol=1e-12)
    assert not got[0, 0, 2].any() and not got[0, 1, 1:].any()                   # all-zero nodes stay where they are
    assert counts.tolist() == [2]
    assert np.allclose(tp, [[10.0 + 3.0 * w[3], -20.0 + 3.0 * w[4]]], rtol=0, atol=1e-12)
    # the opposite sign of w_2 turns the other way
    j = _id_with_w(2, -1.0, -0.9, 6, 2)
    back, _, _ = map_noise_reference(lanes, [2], [[0.0, 0.0]], [j], MapNoise(yaw_deg=45.0, seed=6), 2)
    assert back[0, 0, 0, 1] < -0.63 and back[0, 0, 0, 0] > 0.7
