"""Camera hue shift, Gaussian blur and sensor noise of the resident loader, host side: the settings object, the integer draws and
the float64 numpy reference the GPU tests hold the kernel to, each stage against an independent statement of it (the standard
library's colorsys, torch's reflect padding and conv2d, the moments of the fixed noise draws).  No GPU."""
import colorsys

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------- settings
def test_camera_degrade_validates_its_settings_and_derives_the_radius():
    from mmfn_amd.data import CameraDegrade
    d = CameraDegrade()
    assert (d.hue, d.blur_prob, d.blur_sigma, d.noise_prob, d.noise_std, d.seed) == (0.0, 0.0, (0.5, 2.0), 0.0, (2.0, 12.0), 0)
    assert d.blur_thresh == 0 and d.noise_thresh == 0 and not d.active and d.radius == 6
    assert CameraDegrade(blur_sigma=(0.1, 0.5)).radius == 2 and CameraDegrade(blur_sigma=(1.0, 8.0 / 3.0)).radius == 8
    assert CameraDegrade(blur_sigma=(1.0, 1.0)).radius == 3 and CameraDegrade(blur_sigma=(0.2, 0.2)).radius == 1
    assert CameraDegrade(blur_prob=0.5).blur_thresh == 1 << 23 and CameraDegrade(blur_prob=1.0).blur_thresh == 1 << 24
    assert CameraDegrade(noise_prob=0.5).noise_thresh == 1 << 23 and CameraDegrade(noise_prob=1.0).noise_thresh == 1 << 24
    for cfg in (dict(hue=0.1), dict(blur_prob=0.1), dict(noise_prob=0.1)):
        assert CameraDegrade(**cfg).active
    assert not CameraDegrade(blur_sigma=(1.0, 2.0), noise_std=(0.0, 64.0), seed=4).active
    for name, top in (("hue", 0.5), ("blur_prob", 1.0), ("noise_prob", 1.0)):
        for bad in (-0.01, top * 1.01, float("nan")):
            with pytest.raises(ValueError):
                CameraDegrade(**{name: bad})
        CameraDegrade(**{name: 0.0}), CameraDegrade(**{name: top})
    for bad in ((0.0, 1.0), (2.0, 1.0), (1.0, 2.7), (-1.0, 1.0), (float("nan"), 1.0), (1.0, float("nan")), 1.0, ("a", "b"), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            CameraDegrade(blur_sigma=bad)
    for bad in ((-0.1, 1.0), (2.0, 1.0), (1.0, 64.5), (float("nan"), 1.0), (1.0, float("nan")), 3.0, ("a", "b")):
        with pytest.raises(ValueError):
            CameraDegrade(noise_std=bad)
    CameraDegrade(noise_std=(0.0, 0.0)), CameraDegrade(noise_std=(64.0, 64.0)), CameraDegrade(blur_sigma=(8.0 / 3.0, 8.0 / 3.0))
    assert isinstance(CameraDegrade(seed=7).seed, int)


def test_augment_takes_the_degrade_part_by_type():
    from mmfn_amd.data import Augment, CameraDegrade, CameraJitter, LidarDropout
    a = Augment()
    assert a.camera is None and a.lidar is None and a.map is None and a.degrade is None
    j, d = CameraJitter(0.4), CameraDegrade(0.1)
    a = Augment(camera=j, degrade=d)
    assert a.camera is j and a.degrade is d and a.lidar is None
    for bad in (dict(degrade=j), dict(camera=d), dict(degrade=LidarDropout(0.1)), dict(degrade={"hue": 0.1}), dict(degrade=0.1)):
        with pytest.raises(TypeError):
            Augment(**bad)


class _Store(object):
    """Stands in for a ResidentFrames: a loader whose parts are all inactive touches nothing of it at construction."""
    device = torch.device("cpu")
    n = 4
    indices = np.arange(4)

    def __len__(self):
        return self.n


def test_an_inactive_degrade_part_is_the_plain_loader_and_a_bare_one_is_refused():
    from mmfn_amd.data import Augment, CameraDegrade, ResidentLoader
    plain = set(vars(ResidentLoader(_Store(), 2)))
    for aug in (Augment(degrade=CameraDegrade()), Augment(degrade=CameraDegrade(blur_sigma=(1.0, 2.0), seed=3))):
        loader = ResidentLoader(_Store(), 2, augment=aug)
        assert loader.augment is aug and set(vars(loader)) == plain
        assert not any(isinstance(v, (torch.Tensor, np.ndarray)) for v in vars(loader).values())
        assert loader._states() == {}
    for bad in (CameraDegrade(0.1), CameraDegrade(), {"degrade": CameraDegrade(0.1)}):
        with pytest.raises(TypeError):
            ResidentLoader(_Store(), 2, augment=bad)


# ---------------------------------------------------------------------------------------------- draws
def test_degrade_draws_are_deterministic_24_bit_and_a_stream_of_their_own():
    from mmfn_amd.data import degrade_draws, jitter_draws, lidar_draws, map_draws
    ids = np.arange(64)
    a = degrade_draws(3, 5, ids)
    assert a.dtype == np.int64 and a.shape == (64, 8)
    assert np.array_equal(a, degrade_draws(3, 5, ids)) and np.array_equal(a[[7, 2]], degrade_draws(3, 5, [7, 2]))
    assert a.min() >= 0 and a.max() < 1 << 24 and a.max() > 1 << 23 and a.min() < 1 << 21
    for other in (degrade_draws(4, 5, ids), degrade_draws(3, 6, ids), degrade_draws(3, 5, ids + 64), jitter_draws(3, 5, ids),
                  lidar_draws(3, 5, ids), map_draws(3, 5, ids)):
        assert (other != a).mean() > 0.99
    big = degrade_draws(2 ** 63 + 11, 2 ** 40, [2 ** 40 + 3, 0])
    assert big.min() >= 0 and big.max() < 1 << 24 and not np.array_equal(big[0], degrade_draws(2 ** 63 + 11, 2 ** 40, [3])[0])


# ---------------------------------------------------------------------------------------------- hue
def _hue_pixels():
    """A few hundred pixels in 0..255 as [1, 3, 1, P]: random ones, grays, pure primaries and secondaries, two-channel ties."""
    rng = np.random.RandomState(5)
    px = [rng.uniform(0.0, 255.0, (300, 3))]
    px.append(np.repeat(np.array([0.0, 1.0, 17.5, 128.0, 255.0])[:, None], 3, axis=1))                       # grays, black and white
    px.append(255.0 * np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=np.float64))
    t = rng.uniform(1.0, 254.0, (30, 2))
    hi, lo = t.max(axis=1), t.min(axis=1) * 0.5
    for a, b, c in ((hi, hi, lo), (hi, lo, hi), (lo, hi, hi), (lo, lo, hi), (lo, hi, lo), (hi, lo, lo)):     # max ties, min ties
        px.append(np.stack([a, b, c], axis=1))
    px = np.concatenate(px)
    return px.T.reshape(1, 3, 1, -1), px


def test_the_hue_stage_is_colorsys_round_trip():
    from mmfn_amd.data import hue_shift_reference
    x, px = _hue_pixels()
    assert px.shape[0] > 400
    for shift in (0.0, 0.25, -0.37, 0.5, -0.5, 1.0 / 6.0, 0.049):
        got = hue_shift_reference(x, shift)[0, :, 0, :].T
        want = np.empty_like(px)
        for i, (r, g, b) in enumerate(px / 255.0):
            h, s, v = colorsys.rgb_to_hsv(r, g, b)
            want[i] = 255.0 * np.array(colorsys.hsv_to_rgb((h + shift) % 1.0, s, v))
        assert np.abs(got - want).max() <= 1e-9 * 255.0, shift
        if shift == 0.0:
            assert np.abs(got - px).max() <= 1e-9 * 255.0
    # scale-free: the same pixels as fractions of 1 give the same colours
    assert np.abs(hue_shift_reference(x / 255.0, 0.3) * 255.0 - hue_shift_reference(x, 0.3)).max() <= 1e-9 * 255.0
    # per-sample shifts broadcast: [2, 3, 1, P] with shifts [2, 1, 1]
    both = hue_shift_reference(np.concatenate([x, x]), np.array([0.1, -0.2])[:, None, None])
    assert np.array_equal(both[0], hue_shift_reference(x, 0.1)[0]) and np.array_equal(both[1], hue_shift_reference(x, -0.2)[0])


def test_half_a_turn_twice_returns_the_input():
    from mmfn_amd.data import hue_shift_reference
    x, _ = _hue_pixels()
    once = hue_shift_reference(x, 0.5)
    assert np.abs(once - x).max() > 50.0
    assert np.abs(hue_shift_reference(once, 0.5) - x).max() <= 1e-9 * 255.0
    # saturation and value survive any turn
    for shift in (0.1, 0.5):
        y = hue_shift_reference(x, shift)
        assert np.abs(y.max(axis=1) - x.max(axis=1)).max() <= 1e-9 * 255.0 and np.abs(y.min(axis=1) - x.min(axis=1)).max() <= 1e-9 * 255.0


# ---------------------------------------------------------------------------------------------- blur
def _torch_blur(x, sigma, R):
    """torch's statement of the stage: reflect padding, then a float64 conv2d along x and one along y."""
    t = torch.from_numpy(np.ascontiguousarray(x))[None]                       # [1, C, H, W]
    C = t.shape[1]
    d = torch.arange(-R, R + 1, dtype=torch.float64)
    w = torch.exp(-d * d / (2.0 * sigma * sigma))
    w = w / w.sum()
    t = torch.nn.functional.pad(t, (R, R, R, R), mode="reflect")
    t = torch.nn.functional.conv2d(t, w.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)
    t = torch.nn.functional.conv2d(t, w.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
    return t[0].numpy()


@pytest.mark.parametrize("H,W,R,sigma", [(9, 9, 8, 2.5), (9, 9, 3, 1.0), (12, 20, 6, 1.7), (12, 20, 2, 0.4)])
def test_the_blur_is_reflect_padding_and_two_convolutions(H, W, R, sigma):
    from mmfn_amd.data import gaussian_blur_reference
    x = np.random.RandomState(H * W + R).uniform(0.0, 255.0, (3, H, W))
    got = gaussian_blur_reference(x, sigma, R)
    assert got.shape == x.shape and got.dtype == np.float64
    assert np.abs(got - _torch_blur(x, sigma, R)).max() <= 1e-9 * 255.0
    assert np.abs(gaussian_blur_reference(x, sigma, 0) - x).max() == 0.0      # one tap: the frame itself


def test_a_constant_frame_stays_constant_and_an_impulse_spreads_symmetrically():
    from mmfn_amd.data import gaussian_blur_reference
    flat = np.full((3, 9, 9), 93.25)
    assert np.abs(gaussian_blur_reference(flat, 2.0, 8) - 93.25).max() <= 1e-9
    imp = np.zeros((1, 21, 25))
    imp[0, 10, 12] = 1.0
    out = gaussian_blur_reference(imp, 1.5, 5)[0]
    assert abs(out.sum() - 1.0) <= 1e-12 and out.min() >= 0.0
    assert np.abs(out - out[::-1]).max() <= 1e-15 and np.abs(out - out[:, ::-1]).max() <= 1e-15
    assert np.abs(out[5:16, 7:18] - out[5:16, 7:18].T).max() <= 1e-15          # the same taps along both axes
    assert out[10, 12] == out.max() and out[10, 12] > out[10, 13] > out[10, 14] > out[10, 17] > 0.0
    assert out[10, 18] == 0.0 and out[4, 12] == 0.0                            # nothing past the radius
    # an impulse at the border: the mirrored half comes back in, the sum over the frame is what the border pixel's column says
    edge = np.zeros((1, 9, 9))
    edge[0, 0, 4] = 1.0
    e = gaussian_blur_reference(edge, 1.0, 3)[0]
    assert np.abs(e - e[:, ::-1]).max() <= 1e-15 and e[0, 4] == e.max()


# ---------------------------------------------------------------------------------------------- noise
def test_the_noise_of_a_mid_gray_frame_has_the_moments_it_was_asked_for():
    """Properties of the FIXED draws of (seed 3, epoch 5, sample 0), not of a retried experiment: the seed was picked once so that
    the sample mean is below 4 sigma / sqrt(N), the sample std within 3 % and the lag-1 autocorrelation along x below 4 / sqrt(N);
    a dead, shifted, correlated or mis-scaled generator misses them by far more than any seed does."""
    from mmfn_amd.data import CameraDegrade, CameraJitter, camera_degrade_reference, camera_jitter_reference
    frame = np.full((1, 3, 48, 96), 128.0)
    deg = CameraDegrade(noise_prob=1.0, noise_std=(8.0, 8.0), seed=3)
    out = camera_degrade_reference(frame, [128.0], [0], 5, None, deg)
    assert out.shape == frame.shape and out.min() >= 0.0 and out.max() <= 255.0
    e = (out - 128.0)[0]
    N = e.size
    mean, std = e.mean(), e.std()
    c = e - mean
    lag1 = (c[:, :, 1:] * c[:, :, :-1]).sum() / (c * c).sum()
    print("N = %d: mean %.4f (bound %.4f), std %.4f, lag-1 autocorrelation %.5f (bound %.5f)" % (
        N, mean, 4 * 8 / np.sqrt(N), std, lag1, 4 / np.sqrt(N)))
    assert abs(mean) < 4 * 8 / np.sqrt(N)
    assert abs(std / 8.0 - 1.0) < 0.03
    assert abs(lag1) < 4 / np.sqrt(N)
    assert abs(np.abs(e).max() - 8.0 * 4.0) < 8.0 * 1.5                         # the tail of 13824 normal draws: 2.5 .. 5.5 sigma
    # the frames of a sample share the sample's draws but not the noise; another epoch, another noise
    two = camera_degrade_reference(np.full((1, 2, 3, 48, 96), 128.0), [[128.0, 128.0]], [0], 5, None, deg)
    assert two.shape == (1, 2, 3, 48, 96) and not np.array_equal(two[0, 0], two[0, 1])
    a, b = (two[0, 0] - 128.0).ravel(), (two[0, 1] - 128.0).ravel()
    assert abs(np.corrcoef(a, b)[0, 1]) < 4 / np.sqrt(N)
    assert not np.array_equal(camera_degrade_reference(frame, [128.0], [0], 6, None, deg), out)
    # noise_prob 0: nothing
    never = camera_degrade_reference(frame, [128.0], [0], 5, None, CameraDegrade(noise_std=(8.0, 8.0), seed=3))
    assert np.array_equal(never, camera_jitter_reference(frame, [128.0], np.zeros((1, 8), np.int64), CameraJitter()))


def test_noise_indices_past_64_bits_wrap_as_the_kernels_do():
    from mmfn_amd.data import pixel_noise_reference
    a = pixel_noise_reference(3, 5, 2 ** 62, 4, 1, (3, 4, 8))                   # id * 4 wraps to 0: frame 1 of sample 0
    assert np.array_equal(a, pixel_noise_reference(3, 5, 0, 4, 1, (3, 4, 8)))
    assert not np.array_equal(a, pixel_noise_reference(3, 5, 0, 4, 2, (3, 4, 8)))
    big = pixel_noise_reference(3, 5, 2 ** 33, 2, 0, (3, 4, 8))                 # 2 q passes 2^32
    assert np.isfinite(big).all() and not np.array_equal(big, pixel_noise_reference(3, 5, 0, 2, 0, (3, 4, 8)))


# ---------------------------------------------------------------------------------------------- the whole reference
def test_zero_strengths_give_the_jitter_references_bits():
    from mmfn_amd.data import CameraDegrade, CameraJitter, camera_degrade_reference, camera_jitter_reference, jitter_draws
    rng = np.random.RandomState(2)
    frames = rng.randint(0, 256, (4, 3, 12, 20)).astype(np.uint8)
    m = rng.uniform(60.0, 190.0, 4)
    ids = [3, 0, 2 ** 33, 7]
    jitter = CameraJitter(0.4, 0.4, 0.4, erase_prob=1.0, seed=6)
    want = camera_jitter_reference(frames, m, jitter_draws(6, 2, ids), jitter)
    for deg in (None, CameraDegrade(), CameraDegrade(blur_sigma=(1.0, 2.0), noise_std=(0.0, 64.0), seed=9)):
        got = camera_degrade_reference(frames, m, ids, 2, jitter, deg)
        assert got.dtype == np.float64 and np.array_equal(got, want)
    plain = camera_degrade_reference(frames, m, ids, 2, None, None)
    assert np.array_equal(plain, frames.astype(np.float64))


def test_the_stages_run_in_the_documented_order():
    """Blur sees hue-shifted neighbours, noise lands on the blurred image, and the rectangle comes last: an erased pixel is exactly
    the gray mean with every stage on."""
    from mmfn_amd import data as D
    rng = np.random.RandomState(4)
    frames = rng.uniform(0.0, 255.0, (1, 3, 12, 20))
    m, ids, epoch = [101.5], [5], 1
    jitter = D.CameraJitter(0.4, 0.4, 0.4, erase_prob=1.0, erase_scale=(0.3, 0.5), seed=2)
    deg = D.CameraDegrade(hue=0.5, blur_prob=1.0, blur_sigma=(1.0, 1.0), noise_prob=1.0, noise_std=(5.0, 5.0), seed=8)
    got = D.camera_degrade_reference(frames, m, ids, epoch, jitter, deg)
    k, q = D.jitter_draws(2, epoch, ids), D.degrade_draws(8, epoch, ids)
    x = D._camera_blends(frames.copy(), np.array(m), k, jitter)
    x = D.hue_shift_reference(x, 0.5 * (2.0 * q[0, 0] / 2.0 ** 24 - 1.0))
    x = D.gaussian_blur_reference(x, 1.0, 3)
    x = np.clip(x + 5.0 * D.pixel_noise_reference(8, epoch, 5, 1, 0, (3, 12, 20)), 0.0, 255.0)
    y0, x0, h, w = D.erase_rectangle(k[0], jitter, 12, 20)
    inside = np.zeros((12, 20), dtype=bool)
    inside[y0:y0 + h, x0:x0 + w] = True
    assert np.abs(got[0][:, ~inside] - x[0][:, ~inside]).max() <= 1e-9
    assert (got[0][:, inside] == 101.5).all() and not (got[0][:, ~inside] == 101.5).any()
