"""Camera hue shift, Gaussian blur and sensor noise inside the resident gather, on the GPU: mmfn_gather_camera_degrade against
data.camera_degrade_reference (float64), the bit-for-bit identities with the jitter launch and the plain gather, the erased
rectangle, misaligned planes, determinism, capture, refusals, and ResidentLoader(augment=Augment(camera=, degrade=)) batch by
batch, sharded and under Trainer.train.

Tolerance of the value checks (absolute, rtol 0), stage by stage; the stages' errors add, none amplifies an earlier one:
  blends  3e-3, the jitter test's bound (nine fp32 roundings below 1024, amplified by at most 4, plus the factors' own).
  hue     the divisions by the pixel's chroma do not give a bound by counting roundings (h's error is amplified by M s, s's by M
          f), so, with hue on, stages 1 and 2 together are allowed FOUR times what a float32 numpy restatement of the same
          formulas (_stages_1_2_f32, no fma) misses the float64 reference by on the same frames: the kernel may contract
          multiplies into fma and rounds in another order.  Measured on an MI355X: the restatement's error was 6.3e-5 ..
          2.5e-4 over the cases below (four times that: 2.5e-4 .. 9.8e-4), the kernel's own error with hue alone 6.3e-5 ..
          1.9e-4 - with the blends off it is the restatement's, digit for digit.
  blur    a convex combination (positive taps of sum 1), so an input error passes at most once.  Its own error per pass: the pair
          sums x[-d] + x[d] < 512 round by 2^-15 each, weighted by w_d with sum <= 1/2: 1.5e-5; R + 1 <= 9 roundings of partial
          sums below 256: 9 * 2^-17 = 6.9e-5; the taps: sigma (1 rounding), 2 sigma^2 and the quotient (3) move the exponent by
          |arg| * 3e-7, expf by 1.2e-7, the sum and the division by 2.4e-7, and sum w_d |arg_d| = E[d^2] / (2 sigma^2) <= 1/2, so
          255 * (2 * 1.5e-7 + 3.6e-7) = 1.7e-4.  Two passes: 5.1e-4 -> 6e-4.
  noise   z = sqrtf(-2 logf(u1)) * cosf(c u2), |z| <= sqrt(48 ln 2) = 5.77: logf 1 ulp and sqrtf 1/2 ulp give 1.2e-7 relative;
          c = 6.2831855f is 2 pi (1 + 2.8e-8) and the product rounds once: the angle is off by 6.3 * 8.8e-8 = 5.5e-7, cosf adds
          1.2e-7; the product 6e-8 relative: |dz| <= 5.77 * (6.7e-7 + 1.2e-7 + 6e-8) = 4.9e-6.  Times std_hi, plus std's own
          rounding (6e-8 * 5.77 * std_hi) and the last fma's rounding below 1024 (2^-15 = 3.1e-5): 5.3e-6 * std_hi + 3.1e-5.
The largest |kernel - reference| measured: blur alone 7.2e-5 (bound 3.6e-3), noise alone 2.2e-5 (3.1e-3), every stage on 1.9e-4
(bounds 9.9e-4 .. 1.7e-3).  A wrong neighbour, tap, draw or channel is an error of order 1 to 100."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL_BLENDS, ATOL_BLUR = 3e-3, 6e-4
BUDGET = 64 << 20
PAD = 16          # guard floats on both sides of a destination (64 bytes keep the allocator's alignment)


def _atol_noise(degrade):
    return 5.3e-6 * degrade.noise_std[1] + 3.1e-5


# ---------------------------------------------------------------------------------------------- helpers
def _sources(kind, n, S, H, W, seed):
    """S tensors [n, 3, H, W] on the device, u8 or f32 with values in [0, 255]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(S):
        numel = n * 3 * H * W
        full = torch.randint(0, 256, (numel,), generator=g).to(torch.uint8) if kind == "u8" else torch.rand(numel, generator=g) * 255.0
        out.append(full.to(DEV).view(n, 3, H, W))
    return out


def _skewed(t, skew):
    """The same values, starting `skew` ELEMENTS past an allocation boundary."""
    full = torch.empty(t.numel() + skew, dtype=t.dtype, device=t.device)
    full[skew:] = t.reshape(-1)
    return full[skew:].view(t.shape)


def _gray_mean(srcs):
    """f32 [n, S] device, float64 [n, S] host: mean of 0.299 R + 0.587 G + 0.114 B over every frame, in float64 on the host."""
    gm = np.stack([(s.cpu().numpy().astype(np.float64).mean(axis=(2, 3)) * np.array([0.299, 0.587, 0.114])).sum(axis=1) for s in srcs], axis=1)
    dev = torch.from_numpy(gm.astype(np.float32)).to(DEV)
    return dev, dev.cpu().numpy().astype(np.float64)


def _guarded(shape, skew=0):
    numel = int(np.prod(shape))
    full = torch.full((numel + 2 * PAD + skew,), -7.0, device=DEV)
    return full, full[PAD + skew:PAD + skew + numel].view(shape)


def _guards_intact(full, numel, skew=0):
    return bool((full[:PAD + skew] == -7.0).all()) and bool((full[PAD + skew + numel:] == -7.0).all())


def _state(seed, epoch):
    return torch.tensor([seed, epoch], dtype=torch.int64, device=DEV)


def _args(jitter, degrade, H, W):
    return dict(brightness=jitter.brightness, contrast=jitter.contrast, saturation=jitter.saturation, erase_thresh=jitter.erase_thresh,
                erase_h=jitter.erase_bounds(H), erase_w=jitter.erase_bounds(W), hue=degrade.hue, blur_thresh=degrade.blur_thresh,
                blur_sigma=degrade.blur_sigma, blur_radius=degrade.radius, noise_thresh=degrade.noise_thresh, noise_std=degrade.noise_std)


def _launch(srcs, gm, index, jitter, degrade, epoch, sample_id=None, dst_skew=0):
    """(guard buffer, dst [B * S, 3, H, W]) of one launch for the batch `index` (a list)."""
    from mmfn_amd import ops
    n, _, H, W = srcs[0].shape
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    full, dst = _guarded((len(index) * len(srcs), 3, H, W), dst_skew)
    ops.gather_camera_degrade(srcs, dst, gm, _state(jitter.seed, epoch), _state(degrade.seed, epoch), idx, n, sample_id=sample_id,
                              **_args(jitter, degrade, H, W))
    return full, dst


def _stages_1_2_f32(frames, m, k, q, jitter, hue):
    """The blends and the hue stage of include/mmfn_hip.h in float32 numpy (every operation rounds, no fma): frames [N, 3, H, W],
    gray means m [N], jitter draws k [N, 8], degrade draws q [N, 8] -> float32 [N, 3, H, W]."""
    f = np.float32
    x = np.asarray(frames).astype(f)
    mm = np.asarray(m).astype(f)[:, None, None, None]
    pm1 = lambda col: f(2) * (col.astype(f) * f(2.0 ** -24)) - f(1)
    fac = lambda s, col: (f(s) * pm1(col) + f(1))[:, None, None, None]
    fb, fc, fs = fac(jitter.brightness, k[:, 0]), fac(jitter.contrast, k[:, 1]), fac(jitter.saturation, k[:, 2])
    clamp = lambda v: np.clip(v, f(0), f(255))
    x = clamp(fc * x + (f(1) - fc) * mm)
    x = clamp(fb * x)
    gray = f(0.299) * x[:, 0:1] + f(0.587) * x[:, 1:2] + f(0.114) * x[:, 2:3]
    x = clamp(fs * x + (f(1) - fs) * gray)
    if hue:
        shift = (f(hue) * pm1(q[:, 0]))[:, None, None]
        r, g, b = x[:, 0], x[:, 1], x[:, 2]
        mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
        c = mx - mn
        isgray = mx == mn
        s = c / np.where(isgray, f(1), mx)
        inv = f(1) / np.where(isgray, f(1), c)
        rc, gc, bc = (mx - r) * inv, (mx - g) * inv, (mx - b) * inv
        h6 = np.where(mx == r, bc - gc, np.where(mx == g, f(2) + rc - bc, f(4) + gc - rc))
        h = h6 * f(1.0 / 6.0) + shift
        h = h - np.floor(h)
        hs = h * f(6)
        fl = np.floor(hs)
        fr = hs - fl
        sector = fl.astype(np.int64) % 6
        p, qq, t = clamp(mx * (f(1) - s)), clamp(mx * (f(1) - s * fr)), clamp(mx * (f(1) - s * (f(1) - fr)))
        x = np.stack([np.choose(sector, [mx, qq, p, p, t, mx]), np.choose(sector, [t, mx, mx, qq, p, p]),
                      np.choose(sector, [p, p, t, mx, mx, qq])], axis=1)
    assert x.dtype == f
    return x


def _tolerance(frames, m, ids, epoch, jitter, degrade):
    """(atol of a launch over frames [B, S, 3, H, W] with gray means m [B, S], the float32 restatement's error or None)."""
    from mmfn_amd import data as D
    S = frames.shape[1]
    atol, restated = ATOL_BLENDS, None
    if degrade.hue:
        no_rect = D.CameraJitter(jitter.brightness, jitter.contrast, jitter.saturation, seed=jitter.seed)
        want = D.camera_degrade_reference(frames, m, ids, epoch, no_rect, D.CameraDegrade(hue=degrade.hue, seed=degrade.seed))
        k = np.repeat(D.jitter_draws(jitter.seed, epoch, ids), S, axis=0)
        q = np.repeat(D.degrade_draws(degrade.seed, epoch, ids), S, axis=0)
        got = _stages_1_2_f32(frames.reshape((-1,) + frames.shape[2:]), m.reshape(-1), k, q, jitter, degrade.hue)
        restated = float(np.abs(got.astype(np.float64) - want.reshape(got.shape)).max())
        atol = 4.0 * restated
    if degrade.blur_thresh:
        atol += ATOL_BLUR
    if degrade.noise_thresh:
        atol += _atol_noise(degrade)
    return atol, restated


def _check(dst, srcs, gm64, index, jitter, degrade, epoch, ids, what=""):
    """The launch's result against the float64 reference; returns (erased frames, blurred frames)."""
    from mmfn_amd import data as D
    S = len(srcs)
    host = [s.cpu().numpy() for s in srcs]
    frames = np.stack([np.stack([host[s][i] for s in range(S)]) for i in index])               # [B, S, 3, H, W]
    m = np.array([[gm64[i, s] for s in range(S)] for i in index])
    sample = [ids[i] for i in index]
    want = D.camera_degrade_reference(frames, m, sample, epoch, jitter, degrade).reshape((-1,) + frames.shape[2:])
    atol, restated = _tolerance(frames, m, sample, epoch, jitter, degrade)
    got = dst.cpu().numpy()
    H, W = got.shape[2:]
    err = np.abs(got.astype(np.float64) - want).max()
    print("%s %dx%d: max |kernel - float64 reference| = %.3e (atol %.2e%s)" % (
        what, H, W, err, atol, "" if restated is None else ", float32 restatement of stages 1-2: %.3e" % restated))
    assert got.dtype == np.float32 and err <= atol
    draws = np.repeat(D.jitter_draws(jitter.seed, epoch, sample), S, axis=0)
    erased = 0
    for f in range(got.shape[0]):
        inside = np.zeros((H, W), dtype=bool)
        rect = D.erase_rectangle(draws[f], jitter, H, W)
        if rect is not None:
            y0, x0, h, w = rect
            inside[y0:y0 + h, x0:x0 + w] = True
            erased += 1
        if jitter.erase_thresh:
            is_m = (got[f] == np.float32(m.reshape(-1)[f])).all(axis=0)    # every channel exactly the gray mean, and nowhere else
            assert np.array_equal(is_m, inside), (f, rect)
    blurred = int((np.repeat(D.degrade_draws(degrade.seed, epoch, sample)[:, 1], S) < degrade.blur_thresh).sum())
    return erased, blurred


def _tile():
    from mmfn_amd import _lib
    return _lib.lib().mmfn_camera_degrade_tile_h(), _lib.lib().mmfn_camera_degrade_tile_w()


JIT = dict(brightness=0.4, contrast=0.4, saturation=0.4)
PERM = [4, 0, 5, 1, 3, 2]           # sample id of resident row i in the "permuted table" case
# frame shape -> blur_sigma: 9x9 with R = 8 (the mirror image reaches the far edge), 5x7 with R = 2, 48x96 with the default R = 6
# (one tile and a half), and two tiles plus a ragged rest each way with the widest halo (filled in from the kernel's constants)
SHAPES = {"9x9": ((9, 9), (1.0, 8.0 / 3.0)), "5x7": ((5, 7), (0.1, 0.5)), "48x96": ((48, 96), (0.5, 2.0)), "tiles": (None, (0.5, 8.0 / 3.0))}


# ---------------------------------------------------------------------------------------------- 1. values against float64
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_kernel_matches_the_float64_reference(kind, S, shape):
    from mmfn_amd.data import CameraDegrade, CameraJitter
    (H, W), sigma = SHAPES[shape][0] or (2 * _tile()[0] + 5, 2 * _tile()[1] + 7), SHAPES[shape][1]
    n = 6
    srcs = _sources(kind, n, S, H, W, seed=H * W + S)
    gm, gm64 = _gray_mean(srcs)
    perm = torch.tensor(PERM, dtype=torch.int64, device=DEV)
    none = CameraJitter(seed=1)
    cases = [("hue", none, CameraDegrade(hue=0.5, seed=3)),
             ("blur", none, CameraDegrade(blur_prob=1.0, blur_sigma=sigma, seed=4)),
             ("noise", none, CameraDegrade(noise_prob=1.0, seed=5)),
             ("all", CameraJitter(erase_prob=1.0, seed=6, **JIT), CameraDegrade(hue=0.5, blur_prob=0.5, blur_sigma=sigma, noise_prob=0.5, seed=7)),
             ("all, blurred", CameraJitter(erase_prob=1.0, erase_scale=(0.2, 0.6), seed=8, **JIT),
              CameraDegrade(hue=0.3, blur_prob=1.0, blur_sigma=sigma, noise_prob=1.0, seed=9))]
    assert cases[1][2].radius == {"9x9": 8, "5x7": 2, "48x96": 6, "tiles": 8}[shape]
    mixed = [0, 0]
    for index, sample_id, ids in (([5], None, list(range(n))), ([0, 5, 2, 2, 0, 1, 3, 4], perm, PERM)):
        for what, jitter, degrade in cases:
            full, dst = _launch(srcs, gm, index, jitter, degrade, epoch=2, sample_id=sample_id)
            erased, blurred = _check(dst, srcs, gm64, index, jitter, degrade, 2, ids, "%s S=%d %s:" % (kind, S, what))
            assert _guards_intact(full, dst.numel())
            assert erased == (len(index) * S if jitter.erase_thresh else 0)
            if what == "all":
                mixed[0] += blurred
                mixed[1] += len(index) * S - blurred
            elif degrade.blur_thresh:
                assert blurred == len(index) * S
    assert mixed[0] > 0 and mixed[1] > 0                               # the mixed case ran both paths


# ---------------------------------------------------------------------------------------------- 2. bit for bit
def _jitter_launch(srcs, gm, index, jitter, epoch, dst_skew=0):
    from mmfn_amd import ops
    n, _, H, W = srcs[0].shape
    _, dst = _guarded((len(index) * len(srcs), 3, H, W), dst_skew)
    ops.gather_camera_jitter(srcs, dst, gm, _state(jitter.seed, epoch), torch.tensor(index, dtype=torch.int64, device=DEV), n,
                             brightness=jitter.brightness, contrast=jitter.contrast, saturation=jitter.saturation,
                             erase_thresh=jitter.erase_thresh, erase_h=jitter.erase_bounds(H), erase_w=jitter.erase_bounds(W))
    return dst


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("H,W", [(5, 7), (48, 96)], ids=["5x7", "48x96"])
def test_zero_degrade_strengths_give_the_jitter_launchs_bits_and_the_plain_gathers(kind, H, W):
    from mmfn_amd import ops
    from mmfn_amd.data import CameraDegrade, CameraJitter
    n, S, index = 6, 2, [0, 5, 2, 2, 0]
    srcs = _sources(kind, n, S, H, W, seed=4)
    gm, _ = _gray_mean(srcs)
    jitter = CameraJitter(erase_prob=0.5, seed=8, **JIT)
    for degrade in (CameraDegrade(seed=2), CameraDegrade(blur_sigma=(0.1, 0.5), noise_std=(0.0, 64.0), seed=3)):
        _, dst = _launch(srcs, gm, index, jitter, degrade, epoch=3)
        assert torch.equal(dst, _jitter_launch(srcs, gm, index, jitter, 3))
    _, dst = _launch(srcs, gm, index, CameraJitter(seed=8), CameraDegrade(seed=2), epoch=3)
    plain = torch.full_like(dst, -7.0)
    row = 3 * H * W
    ops.gather_batch([ops.gather_field(srcs[s].view(n, row), plain, row_elems=row, dst_stride=S * row, dst_offset=s * row) for s in range(S)],
                     torch.tensor(index, dtype=torch.int64, device=DEV), n)
    assert torch.equal(dst, plain)


@pytest.mark.parametrize("H,W", [(48, 96), (37, 50)], ids=["48x96", "37x50"])
@pytest.mark.parametrize("kind,src_skew,dst_skew", [("f32", 1, 1), ("u8", 3, 3), ("u8", 4, 0), ("u8", 3, 0), ("f32", 0, 2)],
                         ids=["f32-head3", "u8-head1", "u8-skew4", "u8-misaligned", "f32-misaligned"])
def test_misaligned_planes_give_the_aligned_results_bits(kind, src_skew, dst_skew, H, W):
    """The skews of the jitter test's heads-and-misaligned-planes case: a scalar head and then vector accesses, or element accesses
    (37 x 50: H W is no multiple of 4, element accesses whatever the skew) - and in a blurred frame 16-byte or element stores.
    Same arithmetic either way: the aligned launch's bits, erased rectangle included."""
    from mmfn_amd.data import CameraDegrade, CameraJitter
    n, S = 4, 2
    srcs = _sources(kind, n, S, H, W, seed=9)
    gm, gm64 = _gray_mean(srcs)
    jitter = CameraJitter(erase_prob=1.0, erase_scale=(0.2, 0.9), seed=5, **JIT)
    degrade = CameraDegrade(hue=0.4, blur_prob=0.5, noise_prob=0.5, seed=1)
    index = [2, 0, 1, 3, 2]
    _, aligned = _launch(srcs, gm, index, jitter, degrade, epoch=1)
    erased, blurred = _check(aligned, srcs, gm64, index, jitter, degrade, 1, list(range(n)), "%s aligned:" % kind)
    assert erased == len(index) * S and 0 < blurred < len(index) * S
    full, dst = _launch([_skewed(s, src_skew) for s in srcs], gm, index, jitter, degrade, epoch=1, dst_skew=dst_skew)
    assert torch.equal(dst, aligned)
    assert _guards_intact(full, dst.numel(), dst_skew)


# ---------------------------------------------------------------------------------------------- 3. a function of (seed, epoch, id) only
def test_the_result_depends_on_the_seeds_the_epoch_and_the_sample_id_only():
    from mmfn_amd.data import CameraDegrade, CameraJitter
    n, S, H, W = 6, 2, 48, 96
    srcs = _sources("u8", n, S, H, W, seed=12)
    gm, _ = _gray_mean(srcs)
    jitter = CameraJitter(erase_prob=0.5, seed=21, **JIT)
    cfg = dict(hue=0.3, blur_prob=0.5, noise_prob=0.5)
    degrade = CameraDegrade(seed=31, **cfg)
    _, batch = _launch(srcs, gm, [0, 5, 2, 2, 0], jitter, degrade, epoch=4)
    batch = batch.view(5, S, 3, H, W)
    assert torch.equal(batch[2], batch[3]) and torch.equal(batch[0], batch[4])        # the two copies of sample 2, of sample 0
    for i, b in ((5, 1), (2, 2), (0, 0)):                                             # alone (B = 1) = inside the batch
        _, alone = _launch(srcs, gm, [i], jitter, degrade, epoch=4)
        assert torch.equal(alone.view(S, 3, H, W), batch[b])
    _, other = _launch(srcs, gm, [1, 2, 3, 4, 5, 0, 5], jitter, degrade, epoch=4)     # another composition, B and position
    assert torch.equal(other.view(7, S, 3, H, W)[4], batch[1]) and torch.equal(other.view(7, S, 3, H, W)[6], batch[1])
    _, alone = _launch(srcs, gm, [5], jitter, degrade, epoch=4)
    _, other_epoch = _launch(srcs, gm, [5], jitter, degrade, epoch=5)
    _, other_seed = _launch(srcs, gm, [5], jitter, CameraDegrade(seed=32, **cfg), epoch=4)
    _, other_jitter = _launch(srcs, gm, [5], CameraJitter(erase_prob=0.5, seed=22, **JIT), degrade, epoch=4)
    for o in (other_epoch, other_seed, other_jitter):
        assert not torch.equal(o, alone)
    assert not torch.equal(other_seed, other_epoch)
    # the frames of a sample share the sample's draws, not the noise
    same = [srcs[0], srcs[0]]
    gm_same = gm[:, [0, 0]].contiguous()
    noisy = CameraDegrade(noise_prob=1.0, seed=31)
    _, twice = _launch(same, gm_same, [3], CameraJitter(seed=1), noisy, epoch=4)
    assert not torch.equal(twice[0], twice[1])
    _, twice = _launch(same, gm_same, [3], jitter, CameraDegrade(hue=0.3, blur_prob=1.0, seed=31), epoch=4)
    assert torch.equal(twice[0], twice[1])
    # a table of sample ids: row 2 named 5 draws what row 5 draws without a table (on its own pixels)
    ids = torch.tensor([0, 1, 5, 3, 4, 2], dtype=torch.int64, device=DEV)
    moved = [s[[0, 1, 5, 3, 4, 2]].contiguous() for s in srcs]                        # row 2 now also HOLDS sample 5's frames
    _, renamed = _launch(moved, gm[[0, 1, 5, 3, 4, 2]].contiguous(), [2], jitter, degrade, epoch=4, sample_id=ids)
    assert torch.equal(renamed, alone)


# ---------------------------------------------------------------------------------------------- 4. capture
def test_a_captured_launch_follows_the_index_buffer_and_both_states():
    from mmfn_amd import ops
    from mmfn_amd.data import CameraDegrade, CameraJitter
    n, S, H, W = 6, 2, 48, 96
    srcs = _sources("u8", n, S, H, W, seed=13)
    gm, _ = _gray_mean(srcs)
    cfg = dict(hue=0.3, blur_prob=0.5, noise_prob=0.5)
    jitter, degrade = CameraJitter(erase_prob=1.0, seed=2, **JIT), CameraDegrade(seed=3, **cfg)
    _, first = _launch(srcs, gm, [0, 1, 2], jitter, degrade, epoch=0)      # eager (also loads the library outside the capture)
    index = torch.tensor([0, 1, 2], dtype=torch.int64, device=DEV)
    jstate, dstate = _state(2, 0), _state(3, 0)
    dst = torch.empty(3 * S, 3, H, W, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # one launch on the capture stream: no branches
        ops.gather_camera_degrade(srcs, dst, gm, jstate, dstate, index, n, **_args(jitter, degrade, H, W))
    graph.replay()
    assert torch.equal(dst, first)
    index.copy_(torch.tensor([4, 3, 5], dtype=torch.int64, device=DEV))
    graph.replay()
    _, want = _launch(srcs, gm, [4, 3, 5], jitter, degrade, epoch=0)
    assert torch.equal(dst, want) and not torch.equal(dst, first)
    dstate.copy_(_state(9, 6))                                         # two buffers: the jitter still reads {2, 0}
    graph.replay()
    ref = torch.empty_like(dst)
    ops.gather_camera_degrade(srcs, ref, gm, _state(2, 0), _state(9, 6), index, n, **_args(jitter, degrade, H, W))
    assert torch.equal(dst, ref) and not torch.equal(dst, want)
    jstate.copy_(_state(7, 6))
    graph.replay()
    _, both = _launch(srcs, gm, [4, 3, 5], CameraJitter(erase_prob=1.0, seed=7, **JIT), CameraDegrade(seed=9, **cfg), epoch=6)
    assert torch.equal(dst, both) and not torch.equal(dst, ref)


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_bad_descriptors_are_refused_and_nothing_is_launched():
    from mmfn_amd import _lib
    n, S, H, W, B = 3, 2, 12, 16, 2
    u8 = _sources("u8", n, S, H, W, seed=1)
    f32 = _sources("f32", n, S, H, W, seed=2)
    gm, _ = _gray_mean(u8)
    state, dstate = _state(1, 0), _state(2, 0)
    index = torch.tensor([1, 2, 0, 0], dtype=torch.int64, device=DEV)   # (longer than B: the +4-byte pointer below stays inside)
    dst = torch.full((B * S, 3, H, W), -7.0, device=DEV)
    fn = _lib.lib().mmfn_gather_camera_degrade
    assert _lib.lib().mmfn_sizeof_camera_degrade_desc() == ctypes.sizeof(_lib.CameraDegradeDesc)
    EINVAL = -1
    nan = float("nan")

    def desc(srcs=u8, **over):
        d = _lib.CameraDegradeDesc()
        for s, t in enumerate(srcs):
            d.src[s] = t.data_ptr()
        d.dst, d.gray_mean, d.sample_id, d.state, d.degrade_state = dst.data_ptr(), gm.data_ptr(), None, state.data_ptr(), dstate.data_ptr()
        d.n_frames, d.src_type, d.H, d.W = len(srcs), _lib.GATHER_U8 if srcs[0].dtype == torch.uint8 else _lib.GATHER_F32, H, W
        d.brightness = d.contrast = d.saturation = 0.4
        d.erase_thresh = 1 << 23
        d.erase_h_min, d.erase_h_max, d.erase_w_min, d.erase_w_max = 1, H, 1, W
        d.hue, d.blur_thresh, d.blur_sigma_lo, d.blur_sigma_hi, d.blur_radius = 0.3, 1 << 23, 0.5, 2.0, 6
        d.noise_thresh, d.noise_std_lo, d.noise_std_hi = 1 << 23, 2.0, 12.0
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def call(d, idx=index.data_ptr(), b=B, rows=n):
        return fn(ctypes.byref(d) if d is not None else None, idx, b, rows, _lib.stream())

    def src_at(s, ptr, srcs=u8):
        d = desc(srcs)
        d.src[s] = ptr
        return d

    bad = {
        # what the jitter entry refuses
        "d NULL": lambda: call(None),
        "index NULL": lambda: call(desc(), idx=None),
        "index misaligned": lambda: call(desc(), idx=index.data_ptr() + 4),
        "n_frames 0": lambda: call(desc(n_frames=0)),
        "n_frames 5": lambda: call(desc(n_frames=5)),
        "src[0] NULL": lambda: call(src_at(0, None)),
        "src[1] NULL": lambda: call(src_at(1, None)),
        "f32 src misaligned": lambda: call(src_at(1, f32[1].data_ptr() + 2, f32)),
        "dst NULL": lambda: call(desc(dst=None)),
        "dst misaligned": lambda: call(desc(dst=dst.data_ptr() + 2)),
        "gray_mean NULL": lambda: call(desc(gray_mean=None)),
        "gray_mean misaligned": lambda: call(desc(gray_mean=gm.data_ptr() + 2)),
        "state NULL": lambda: call(desc(state=None)),
        "state misaligned": lambda: call(desc(state=state.data_ptr() + 4)),
        "sample_id misaligned": lambda: call(desc(sample_id=index.data_ptr() + 4)),
        "src_type PAL4": lambda: call(desc(src_type=_lib.GATHER_PAL4)),
        "src_type 7": lambda: call(desc(src_type=7)),
        "H 0": lambda: call(desc(H=0)),
        "W 0": lambda: call(desc(W=0)),
        "H -1": lambda: call(desc(H=-1)),
        "erase_thresh 2^24 + 1": lambda: call(desc(erase_thresh=(1 << 24) + 1)),
        "h_min 0": lambda: call(desc(erase_h_min=0)),
        "h_min > h_max": lambda: call(desc(erase_h_min=3, erase_h_max=2)),
        "h_max > H": lambda: call(desc(erase_h_max=H + 1)),
        "w_min 0": lambda: call(desc(erase_w_min=0)),
        "w_min > w_max": lambda: call(desc(erase_w_min=3, erase_w_max=2)),
        "w_max > W": lambda: call(desc(erase_w_max=W + 1)),
        "B -1": lambda: call(desc(), b=-1),
        "B 65536": lambda: call(desc(), b=65536),
        "n 0": lambda: call(desc(), rows=0),
        # and the new members
        "degrade_state NULL": lambda: call(desc(degrade_state=None)),
        "degrade_state misaligned": lambda: call(desc(degrade_state=dstate.data_ptr() + 4)),
        "R -1": lambda: call(desc(blur_radius=-1)),
        "R 9": lambda: call(desc(blur_radius=9)),
        "R 9 without blur": lambda: call(desc(blur_radius=9, blur_thresh=0)),
        "H <= R": lambda: call(desc(H=6, erase_h_max=6)),
        "W <= R": lambda: call(desc(W=6, erase_w_max=6)),
        "H < R": lambda: call(desc(H=5, erase_h_max=5, blur_radius=8)),
        "blur_thresh 2^24 + 1": lambda: call(desc(blur_thresh=(1 << 24) + 1)),
        "noise_thresh 2^24 + 1": lambda: call(desc(noise_thresh=(1 << 24) + 1)),
        "sigma lo 0": lambda: call(desc(blur_sigma_lo=0.0)),
        "sigma lo < 0": lambda: call(desc(blur_sigma_lo=-1.0)),
        "sigma lo > hi": lambda: call(desc(blur_sigma_lo=2.5)),
        "sigma hi 2.7": lambda: call(desc(blur_sigma_hi=2.7)),
        "sigma lo NaN": lambda: call(desc(blur_sigma_lo=nan)),
        "sigma hi NaN": lambda: call(desc(blur_sigma_hi=nan)),
        "std lo < 0": lambda: call(desc(noise_std_lo=-0.5)),
        "std lo > hi": lambda: call(desc(noise_std_lo=13.0)),
        "std hi 64.5": lambda: call(desc(noise_std_hi=64.5)),
        "std lo NaN": lambda: call(desc(noise_std_lo=nan)),
        "std hi NaN": lambda: call(desc(noise_std_hi=nan)),
    }
    for name in ("brightness", "contrast", "saturation"):
        for v in (-0.1, 1.5, nan):
            bad["%s %r" % (name, v)] = lambda name=name, v=v: call(desc(**{name: v}))
    for v in (-0.1, 0.51, nan):
        bad["hue %r" % v] = lambda v=v: call(desc(hue=v))
    for what, run in bad.items():
        assert run() == EINVAL, what
    assert call(desc(), b=0) == 0 and call(desc(), b=0, rows=0) == 0                  # an empty batch: nothing to do
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())
    # a part's bounds are ignored while it is off; thresholds 0 and 2^24, hue 0 and 0.5, sigma 8/3 and std 0 and 64 are inside
    assert call(desc(blur_thresh=0, blur_sigma_lo=0.0, blur_sigma_hi=-1.0, noise_thresh=0, noise_std_lo=nan, noise_std_hi=99.0, hue=0.0,
                     blur_radius=8, H=3, erase_h_max=3)) == 0
    assert call(desc(blur_thresh=1 << 24, noise_thresh=1 << 24, hue=0.5, blur_sigma_hi=float(np.float32(8.0 / 3.0)), blur_radius=8,
                     noise_std_lo=0.0, noise_std_hi=64.0)) == 0
    assert call(desc(f32, blur_radius=0)) == 0
    torch.cuda.synchronize()
    assert not bool((dst == -7.0).any())


# ---------------------------------------------------------------------------------------------- 6. the loader
AUG = dict(erase_prob=0.5, **JIT)
DEG = dict(hue=0.3, blur_prob=0.5, noise_prob=0.5)


def _pack_store(tmp, samples):
    from mmfn_amd import data as D
    for s in samples:
        s["radar_adj"] = D.radar_adjacency(s["radar"][0])
    return D.PackedFrames(D.pack_frames(samples, str(tmp / "packed")))


@pytest.fixture(scope="module")
def packed_vec(tmp_path_factory):
    from oracle import fixtures
    return _pack_store(tmp_path_factory.mktemp("degrade_vec"), fixtures.synthetic_samples((5, 9, 3, 7, 1), seed=5, radar_counts=(50, 100, 81, 3, 90)))


@pytest.fixture(scope="module")
def packed_img(tmp_path_factory):
    """seq_len = 2 samples for the image-map model."""
    rng = np.random.RandomState(17)
    samples = []
    for n_lane in (4, 2, 6, 3):
        samples.append({
            "fronts": [torch.from_numpy(rng.randint(0, 256, (3, 256, 256)).astype(np.uint8)) for _ in range(2)],
            "lidars": [(rng.randint(0, 6, (2, 256, 256)) / 5.0).astype(np.float32) for _ in range(2)],
            "vectormaps": [torch.from_numpy(rng.randn(n_lane, 10, 5)) for _ in range(2)],
            "radar": [rng.randn(81, 5) for _ in range(2)],
            "maps": [torch.from_numpy(rng.randint(0, 256, (3, 256, 256)).astype(np.uint8)) for _ in range(2)],
            "waypoints": [tuple(rng.randn(2)) for _ in range(6)], "target_point": tuple(rng.randn(2) * 10.0),
            "steer": 0.1, "throttle": 0.5, "brake": False, "command": 2, "velocity": float(rng.uniform(0, 8))})
    return _pack_store(tmp_path_factory.mktemp("degrade_img"), samples)


def _same_but_image(got, want):
    (ginp, ggt), (winp, wgt) = got, want
    assert list(ginp) == list(winp)
    for k in winp:
        assert ginp[k].dtype == winp[k].dtype and ginp[k].shape == winp[k].shape and ginp[k].is_contiguous(), k
        if k != "image":
            assert torch.equal(ginp[k], winp[k]), k
    assert torch.equal(ggt, wgt)


@pytest.mark.parametrize("variant", ["vec", "img"])
def test_a_degraded_epoch_changes_the_camera_field_only(packed_vec, packed_img, variant):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    packed, S = (packed_vec, 1) if variant == "vec" else (packed_img, 2)
    cfg = GlobalConfig(seq_len=S)
    n = len(packed)
    res = D.ResidentFrames(packed, DEV, cfg, variant, max_bytes=BUDGET)
    plan, nbytes = D.ResidentFrames.plan(packed, cfg, variant), res.nbytes()
    jitter, degrade = D.CameraJitter(seed=11, **AUG), D.CameraDegrade(seed=12, **DEG)
    aug = D.ResidentLoader(res, 2, shuffle=True, seed=3, augment=D.Augment(camera=jitter, degrade=degrade))
    plain = D.ResidentLoader(res, 2, shuffle=True, seed=3)
    assert res.nbytes() == nbytes == plan["bytes"] and set(res.tensors) == set(plan["fields"])      # the store is as it was
    assert set(vars(aug)) - set(vars(plain)) == {"gray_mean", "jitter_state", "degrade_state", "sample_id"}
    # without a CameraJitter the loader still holds what the launch reads, and no jitter state
    alone = D.ResidentLoader(res, 2, shuffle=True, seed=3, augment=D.Augment(degrade=degrade))
    assert set(vars(alone)) - set(vars(plain)) == {"gray_mean", "degrade_state", "sample_id"}
    assert torch.equal(alone.gray_mean, aug.gray_mean) and alone.sample_id.tolist() == list(range(n))
    cams = [np.asarray(packed.arrays["fronts.%d" % s]) for s in range(S)]
    gm64 = aug.gray_mean.cpu().numpy().astype(np.float64)
    first = None
    for epoch in range(2):
        chunks = D._chunks(D._epoch_order(n, True, None, 3, epoch), 2, False)
        got, want, lone = list(aug), list(plain), list(alone)
        assert len(got) == len(want) == len(lone) == len(chunks)
        for g, w, a, idx in zip(got, want, lone, chunks):
            _same_but_image(g, w)
            _same_but_image(a, w)
            assert not torch.equal(g[0]["image"], w[0]["image"]) and not torch.equal(a[0]["image"], g[0]["image"])
            if epoch == 0:
                frames = np.stack([np.stack([cams[s][i] for s in range(S)]) for i in idx])
                m = np.array([[gm64[i, s] for s in range(S)] for i in idx])
                for batch, j in ((g, jitter), (a, D.CameraJitter())):
                    ref = D.camera_degrade_reference(frames, m, idx, epoch, j, degrade).reshape((-1,) + frames.shape[2:])
                    atol, restated = _tolerance(frames, m, idx, epoch, j, degrade)
                    err = np.abs(batch[0]["image"].cpu().numpy().astype(np.float64) - ref).max()
                    print("epoch %d batch %s: max |image - reference| = %.3e (atol %.2e, float32 restatement %.3e)" % (epoch, idx, err, atol, restated))
                    assert err <= atol
        if epoch == 0:
            first = {i: g[0]["image"][b * S:(b + 1) * S].clone() for g, idx in zip(got, chunks) for b, i in enumerate(idx)}
        else:   # the second epoch: other draws for every sample
            for g, idx in zip(got, chunks):
                for b, i in enumerate(idx):
                    assert not torch.equal(g[0]["image"][b * S:(b + 1) * S], first[i]), i
    assert aug.epoch == plain.epoch == 2 and aug.jitter_state.tolist() == [11, 1] and aug.degrade_state.tolist() == [12, 1]
    assert alone.degrade_state.tolist() == [12, 1]


def test_no_degrade_part_is_the_jitter_loader_bit_for_bit(packed_vec):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    res = D.ResidentFrames(packed_vec, DEV, GlobalConfig(), "vec", max_bytes=BUDGET)
    jitter = D.CameraJitter(seed=4, **AUG)
    want = D.ResidentLoader(res, 2, shuffle=True, seed=1, lane_bucket=16, augment=jitter)
    for aug in (D.Augment(camera=jitter, degrade=None), D.Augment(camera=jitter, degrade=D.CameraDegrade(seed=5))):
        got = D.ResidentLoader(res, 2, shuffle=True, seed=1, lane_bucket=16, augment=aug)
        assert set(vars(got)) == set(vars(want)) and "degrade" not in got._states()["augment"]
        want.epoch = 0
        for (ia, ga), (ib, gb) in zip(list(got), list(want)):
            assert list(ia) == list(ib) and all(torch.equal(ia[k], ib[k]) for k in ia) and torch.equal(ga, gb)


def test_a_shard_draws_what_the_full_store_draws(packed_vec):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    aug = D.Augment(camera=D.CameraJitter(seed=4, **AUG), degrade=D.CameraDegrade(seed=6, **DEG))
    full = D.ResidentFrames(packed_vec, DEV, cfg, "vec", max_bytes=BUDGET)
    shard = D.ResidentFrames(packed_vec, DEV, cfg, "vec", indices=[1, 3], max_bytes=BUDGET)
    a, b = D.ResidentLoader(full, 5, augment=aug), D.ResidentLoader(shard, 2, augment=aug)
    assert b.sample_id.tolist() == [1, 3]
    for epoch in range(2):
        (fa, _), = list(a)
        (fb, _), = list(b)
        assert torch.equal(fb["image"][1], fa["image"][3]) and torch.equal(fb["image"][0], fa["image"][1])
        assert not torch.equal(fb["image"][1], fa["image"][1])
    (fs, _), = list(D.ResidentLoader(shard, 2, sampler=[3], augment=aug))             # through a sampler of global ids as well
    a.epoch = 0
    (fa, _), = list(a)
    assert torch.equal(fs["image"][0], fa["image"][3])


def test_frames_no_larger_than_the_radius_are_refused_by_the_loader(packed_vec):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    res = D.ResidentFrames(packed_vec, DEV, GlobalConfig(), "vec", max_bytes=BUDGET)
    res.shapes = dict(res.shapes, **{"fronts.0": (3, 6, 32768)})
    with pytest.raises(ValueError):
        D.ResidentLoader(res, 2, augment=D.Augment(degrade=D.CameraDegrade(blur_prob=0.5)))
    D.ResidentLoader(res, 2, augment=D.Augment(degrade=D.CameraDegrade(blur_prob=0.5, blur_sigma=(0.5, 1.0))))      # R = 3


def test_two_epochs_of_trainer_train_over_the_degraded_loader(tmp_path):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd import model as M
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import Trainer
    from oracle import fixtures, harness
    oracle = harness.build_oracle("vec", dropout=0.1)
    cfg = GlobalConfig()
    packed = _pack_store(tmp_path, fixtures.synthetic_samples((5, 9, 3, 7), seed=3, radar_counts=(50, 81, 81, 20)))
    res = D.ResidentFrames(packed, DEV, cfg, "vec", max_bytes=BUDGET)
    loader = D.ResidentLoader(res, 2, shuffle=True, seed=2, lane_bucket=16,
                              augment=D.Augment(camera=D.CameraJitter(seed=1, **AUG), degrade=D.CameraDegrade(seed=2, **DEG)))
    net = M.MMFN(cfg, DEV)
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
    assert loader.epoch == 2 and loader.jitter_state.tolist() == [1, 1] and loader.degrade_state.tolist() == [2, 1]
