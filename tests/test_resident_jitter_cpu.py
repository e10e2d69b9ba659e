"""Camera jitter of the resident loader, host side: the settings object, the integer draws restated in numpy, the float64
reference of the kernel's arithmetic and the erased rectangle's bounds.  No GPU."""
import numpy as np
import pytest
import torch


def test_camera_jitter_validates_its_settings():
    from mmfn_amd.data import CameraJitter
    j = CameraJitter()
    assert (j.brightness, j.contrast, j.saturation, j.erase_prob, j.erase_scale, j.seed) == (0.0, 0.0, 0.0, 0.0, (0.1, 0.3), 0)
    assert j.erase_thresh == 0 and CameraJitter(erase_prob=1.0).erase_thresh == 1 << 24 and CameraJitter(erase_prob=0.5).erase_thresh == 1 << 23
    for name in ("brightness", "contrast", "saturation", "erase_prob"):
        for bad in (-0.01, 1.01, float("nan")):
            with pytest.raises(ValueError):
                CameraJitter(**{name: bad})
        CameraJitter(**{name: 0.0}), CameraJitter(**{name: 1.0})
    for bad in ((0.3, 0.1), (0.0, 0.3), (0.1, 1.5), (-0.1, 0.2), 0.2, (0.1, 0.2, 0.3), ("a", "b")):
        with pytest.raises(ValueError):
            CameraJitter(erase_scale=bad)
    # fractions of a side become integer bounds: max(1, round(f * side))
    j = CameraJitter(erase_scale=(0.1, 0.3))
    assert j.erase_bounds(256) == (26, 77) and j.erase_bounds(8) == (1, 2) and j.erase_bounds(1) == (1, 1) and j.erase_bounds(5) == (1, 2)
    assert CameraJitter(erase_scale=(1.0, 1.0)).erase_bounds(7) == (7, 7)


def test_hash_restatement_against_known_values():
    """lowbias32 written out by hand for two inputs (32-bit wrap-around at each multiply)."""
    from mmfn_amd import data as D

    def by_hand(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) % (1 << 32)
        x ^= x >> 15
        x = (x * 0x846CA68B) % (1 << 32)
        return x ^ (x >> 16)

    vals = [0, 1, 0xFFFFFFFF, 0x12345678, 0x80000000]
    got = D._hash32(np.asarray(vals, dtype=np.uint64))
    assert [int(v) for v in got] == [by_hand(v) for v in vals] and by_hand(0) == 0 and by_hand(1) != 1


def test_draws_are_deterministic_24_bit_and_keyed_by_seed_epoch_and_id():
    from mmfn_amd.data import jitter_draws
    ids = np.arange(64)
    a = jitter_draws(3, 5, ids)
    assert a.dtype == np.int64 and a.shape == (64, 8)
    assert np.array_equal(a, jitter_draws(3, 5, ids)) and np.array_equal(a[[7, 2]], jitter_draws(3, 5, [7, 2]))
    assert a.min() >= 0 and a.max() < 1 << 24
    assert a.max() > 1 << 23 and a.min() < 1 << 21              # (512 draws: not stuck in a corner of the range)
    for other in (jitter_draws(4, 5, ids), jitter_draws(3, 6, ids), jitter_draws(3, 5, ids + 64)):
        assert (other != a).mean() > 0.99
    assert len({tuple(r) for r in a}) == 64                        # every id its own draws
    big = jitter_draws(2 ** 63 + 11, 2 ** 40, [2 ** 40 + 3, 0])    # ids past 2^32 / 8 and a seed past 2^63: still 24 bits, no overflow
    assert big.shape == (2, 8) and big.min() >= 0 and big.max() < 1 << 24
    assert not np.array_equal(big[0], jitter_draws(2 ** 63 + 11, 2 ** 40, [3])[0])     # the high index word is folded in


def test_reference_with_zero_strengths_returns_its_input():
    from mmfn_amd.data import CameraJitter, camera_jitter_reference, jitter_draws
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, (3, 3, 5, 7)).astype(np.uint8)
    out = camera_jitter_reference(frames, [10.0, 20.0, 30.0], jitter_draws(1, 2, [0, 1, 2]), CameraJitter())
    assert out.dtype == np.float64 and np.array_equal(out, frames.astype(np.float64))


def test_reference_blends_as_written():
    """One pixel by hand: contrast, brightness, saturation with clamping, draws chosen so that the factors are 1.2, 0.8, 1.4."""
    from mmfn_amd.data import CameraJitter, camera_jitter_reference
    j = CameraJitter(0.4, 0.4, 0.4)
    k = np.zeros((1, 8), dtype=np.int64)
    k[0, 0], k[0, 1], k[0, 2] = 1 << 22, 3 << 22, (1 << 24) - 1          # u = 0.25, 0.75, ~1: f_b = 0.8, f_c = 1.2, f_s ~ 1.4
    px = np.array([200.0, 100.0, 250.0]).reshape(1, 3, 1, 1)
    out = camera_jitter_reference(px, [120.0], k, j).reshape(3)
    s = float(np.float32(0.4))
    f_b, f_c, f_s = 1 + s * -0.5, 1 + s * 0.5, 1 + s * (2 * ((1 << 24) - 1) / 2.0 ** 24 - 1)
    x = np.clip(f_c * px.reshape(3) + (1 - f_c) * 120.0, 0, 255)           # [216, 96, 255 (clamped from 276)]
    assert x[2] == 255.0
    x = np.clip(f_b * x, 0, 255)
    g = 0.299 * x[0] + 0.587 * x[1] + 0.114 * x[2]
    x = np.clip(f_s * x + (1 - f_s) * g, 0, 255)
    assert np.allclose(out, x, rtol=0, atol=1e-12)


@pytest.mark.parametrize("H,W", [(5, 7), (48, 96), (256, 256), (1, 1)])
def test_erased_rectangle_stays_inside_the_frame_at_the_extreme_draws(H, W):
    from mmfn_amd.data import CameraJitter, camera_jitter_reference, erase_rectangle
    top = (1 << 24) - 1
    for scale in ((0.1, 0.3), (1.0, 1.0), (0.01, 1.0)):
        j = CameraJitter(erase_prob=1.0, erase_scale=scale)
        (h_min, h_max), (w_min, w_max) = j.erase_bounds(H), j.erase_bounds(W)
        assert 1 <= h_min <= h_max <= H and 1 <= w_min <= w_max <= W
        for k4 in (0, top):
            for k5 in (0, top):
                for k6 in (0, top):
                    for k7 in (0, top):
                        y0, x0, h, w = erase_rectangle([0, 0, 0, top, k4, k5, k6, k7], j, H, W)
                        assert h == (h_max if k4 else h_min) and w == (w_max if k5 else w_min)
                        assert 0 <= y0 and y0 + h <= H and 0 <= x0 and x0 + w <= W
                        assert y0 == (H - h if k7 else 0) and x0 == (W - w if k6 else 0)
    full = CameraJitter(erase_prob=1.0, erase_scale=(1.0, 1.0))             # h_min = h_max = H: the whole frame, at (0, 0)
    assert erase_rectangle([0, 0, 0, top, top, top, top, top], full, H, W) == (0, 0, H, W)
    out = camera_jitter_reference(np.full((1, 3, H, W), 9.0), [4.5], [[0, 0, 0, top, top, top, top, top]], full)
    assert np.array_equal(out, np.full((1, 3, H, W), 4.5))
    # draw 3 decides: at the threshold the sample keeps its pixels
    half = CameraJitter(erase_prob=0.5)
    assert erase_rectangle([0, 0, 0, (1 << 23) - 1, 0, 0, 0, 0], half, H, W) is not None
    assert erase_rectangle([0, 0, 0, 1 << 23, 0, 0, 0, 0], half, H, W) is None
    assert erase_rectangle([0, 0, 0, 0, 0, 0, 0, 0], CameraJitter(), H, W) is None


class _Store(object):
    """Stands in for a ResidentFrames: the plain loader touches nothing of it at construction."""
    device = torch.device("cpu")
    n = 4
    indices = np.arange(4)

    def __len__(self):
        return self.n


def test_the_plain_loader_holds_no_new_tensors():
    from mmfn_amd.data import CameraJitter, ResidentLoader
    plain, default = ResidentLoader(_Store(), 2, augment=None), ResidentLoader(_Store(), 2)
    assert plain.augment is None and default.augment is None
    for loader in (plain, default):
        assert set(vars(loader)) == {"resident", "batch_size", "shuffle", "sampler", "seed", "drop_last", "lane_bucket", "epoch", "augment"}
        assert not any(isinstance(v, (torch.Tensor, np.ndarray)) for v in vars(loader).values())
    with pytest.raises(TypeError):
        ResidentLoader(_Store(), 2, augment={"brightness": 0.4})
    assert isinstance(CameraJitter(seed=7).seed, int)
