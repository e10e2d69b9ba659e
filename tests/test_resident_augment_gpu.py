"""LiDAR dropout, lane dropout and map noise inside the resident gather, on the GPU: mmfn_gather_augment against the numpy
references of mmfn_amd.data (the LiDAR field and the lane dropout bit for bit, the rigid transform within a derived bound),
capture, refusals, and ResidentLoader(augment=Augment(...)) batch by batch, sharded, compact and under Trainer.train.

Tolerance of the moved lane coordinates: atol = 16 * 2^-24 * M with M the largest of |x|, |y| and shift in the test's data - one
rounding each for the translation, the angle and the two fmaf of a coordinate, and 2 ulp for sinf and cosf as the HIP math API
documents them, sum to 12 * 2^-24 * M.  A wrong sign, feature or sample is an error of order `shift` or more.  Target point:
2^-23 * (|tp| + target_shift), one fmaf."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUDGET = 64 << 20
PAD = 16          # guard floats on both sides of a destination (64 bytes keep the allocator's alignment)
PERM = [4, 0, 5, 1, 3, 2]           # sample id of resident row i in the "permuted table" case
VALUES = np.array([0.2, 0.4, 0.6, 0.8, 1.0, 1.2], dtype=np.float32)     # no 0.0: code 0 of the palette is 0.2, and a 0 is a drop


def _guarded(shape, skew=0):
    numel = int(np.prod(shape))
    full = torch.full((numel + 2 * PAD + skew,), -7.0, device=DEV)
    return full, full[PAD + skew:PAD + skew + numel].view(shape)


def _guards_intact(full, numel, skew=0):
    return bool((full[:PAD + skew] == -7.0).all()) and bool((full[PAD + skew + numel:] == -7.0).all())


def _state(seed, epoch):
    return torch.tensor([seed, epoch], dtype=torch.int64, device=DEV)


def _skewed(host, skew):
    """The host array on the device, starting `skew` ELEMENTS past an allocation boundary."""
    flat = torch.from_numpy(np.ascontiguousarray(host)).reshape(-1)
    full = torch.zeros(flat.numel() + skew, dtype=flat.dtype)
    full[skew:] = flat
    return full.to(DEV)[skew:].view(host.shape)


# ---------------------------------------------------------------------------------------------- 1. LiDAR, bit for bit
def _lidar_sources(kind, n, S, C, H, W, seed, skew=0):
    """(host f32 [S][n, C, H, W], device tensors [S] [n, row] f32 or [n, row / 2] codes, palettes [S] or None)"""
    from mmfn_amd import data as D
    rng = np.random.RandomState(seed)
    host = [VALUES[rng.randint(0, len(VALUES), (n, C, H, W))] for _ in range(S)]
    if kind == "f32":
        return host, [_skewed(h.reshape(n, -1), skew) for h in host], None
    coded = [D.palette_encode(h) for h in host]
    assert all(c is not None and c[1][0] != 0.0 for c in coded)                # a non-zero entry at code 0
    return host, [_skewed(c[0], skew) for c in coded], [torch.from_numpy(c[1]).to(DEV) for c in coded]


def _lidar_launch(srcs, pals, shape, index, aug, epoch, sample_id=None, dst_skew=0):
    from mmfn_amd import ops
    C, H, W = shape
    n = srcs[0].shape[0]
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    full, dst = _guarded((len(index) * len(srcs), C, H, W), dst_skew)
    ops.gather_augment(idx, n, sample_id=sample_id, lidar=dict(
        srcs=srcs, palettes=pals, dst=dst, state=_state(aug.seed, epoch), cell_thresh=aug.cell_thresh, erase_thresh=aug.erase_thresh,
        erase_h=aug.erase_bounds(H), erase_w=aug.erase_bounds(W)))
    return full, dst


def _lidar_expected(host, index, aug, epoch, ids):
    from mmfn_amd import data as D
    n, S = host[0].shape[0], len(host)
    rows = [min(max(i, 0), n - 1) for i in index]
    frames = np.stack([host[s][i] for i in rows for s in range(S)])
    return D.lidar_dropout_reference(frames, np.repeat([ids[i] for i in rows], S), aug, epoch)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


LIDAR_CONFIGS = [dict(cell_prob=0.3), dict(erase_prob=1.0, erase_scale=(0.2, 0.6)), dict(cell_prob=0.3, erase_prob=1.0, erase_scale=(0.2, 0.6)), dict()]
INDEX = [0, 5, 2, 2, -3, 9]          # a repeat, and entries out of range on both sides (clamped to rows 0 and 5)


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("kind,C,H,W", [("f32", 2, 4, 8), ("f32", 2, 5, 7), ("f32", 2, 48, 96), ("f32", 1, 5, 7), ("pal4", 2, 4, 8), ("pal4", 2, 5, 7),
                                        ("pal4", 2, 48, 96)])
def test_lidar_dropout_matches_the_reference_bit_for_bit(kind, C, H, W, S):
    """(2, 4, 8): a few vector accesses; (2, 5, 7): planes shorter than a piece, rows that end off a vector; (2, 48, 96) = 9216
    elements: more than one workgroup piece (4096 floats, 8192 codes), a plane longer than an f32 piece and shorter than a coded
    one; (1, 5, 7): an odd row, f32 only."""
    from mmfn_amd import ops
    from mmfn_amd.data import LidarDropout
    n = 6
    host, srcs, pals = _lidar_sources(kind, n, S, C, H, W, seed=C * H * W + S)
    perm = torch.tensor(PERM, dtype=torch.int64, device=DEV)
    for index in ([5], INDEX):
        for sample_id, ids in ((None, list(range(n))), (perm, PERM)):
            for c, cfg in enumerate(LIDAR_CONFIGS):
                aug = LidarDropout(seed=3 + c, **cfg)
                full, dst = _lidar_launch(srcs, pals, (C, H, W), index, aug, 2, sample_id)
                want = _lidar_expected(host, index, aug, 2, ids)
                got = dst.cpu().numpy()
                assert np.array_equal(_bits(got), _bits(want)), (index, ids, cfg, int((_bits(got) != _bits(want)).sum()))
                assert _guards_intact(full, dst.numel())
                if cfg:
                    assert (got == 0).any() and (got != 0).any()
                else:                                                           # all zero: what the plain gather writes
                    plain = torch.full_like(dst, -7.0)
                    row = C * H * W
                    ops.gather_batch([ops.gather_field(srcs[s], plain, row_elems=row, dst_stride=S * row, dst_offset=s * row,
                                                       palette=pals[s] if pals else None) for s in range(S)],
                                     torch.tensor(index, dtype=torch.int64, device=DEV), n)
                    assert torch.equal(dst.view(torch.int32), plain.view(torch.int32))


@pytest.mark.parametrize("kind,src_skew,dst_skew", [("f32", 1, 1), ("f32", 3, 3), ("f32", 2, 1), ("f32", 0, 2), ("pal4", 1, 2), ("pal4", 3, 2),
                                                    ("pal4", 2, 1), ("pal4", 0, 3)])
@pytest.mark.parametrize("C,H,W", [(2, 5, 7), (2, 48, 96)], ids=["2x5x7", "2x48x96"])
def test_lidar_heads_and_misaligned_rows(kind, src_skew, dst_skew, C, H, W):
    """A source that starts 1-3 elements (bytes of codes) off a 16-byte boundary: with the destination misaligned alike ((f32, 1, 1):
    a 3-float head; (pal4, 1, 2): 15 bytes = 30 floats) a scalar head and then vector accesses, the rectangle and the cell draws
    still where the element's index puts them; otherwise element accesses."""
    from mmfn_amd.data import LidarDropout
    n, S = 3, 2
    host, srcs, pals = _lidar_sources(kind, n, S, C, H, W, seed=9, skew=src_skew)
    aug = LidarDropout(cell_prob=0.3, erase_prob=1.0, erase_scale=(0.2, 0.9), seed=5)
    index = [2, 0, 1, 2]
    full, dst = _lidar_launch(srcs, pals, (C, H, W), index, aug, 1, dst_skew=dst_skew)
    assert np.array_equal(_bits(dst.cpu().numpy()), _bits(_lidar_expected(host, index, aug, 1, list(range(n)))))
    assert _guards_intact(full, dst.numel(), dst_skew)


def test_lidar_u8_frames_are_widened_and_masked():
    from mmfn_amd.data import LidarDropout
    n, S, C, H, W = 4, 1, 2, 48, 96
    rng = np.random.RandomState(3)
    host = [rng.randint(1, 256, (n, C, H, W)).astype(np.uint8)]
    for skew, dst_skew in ((0, 0), (3, 3), (5, 0)):
        srcs = [_skewed(host[0].reshape(n, -1), skew)]
        aug = LidarDropout(cell_prob=0.3, erase_prob=1.0, seed=8)
        full, dst = _lidar_launch(srcs, None, (C, H, W), [3, 0, 1], aug, 0, dst_skew=dst_skew)
        want = _lidar_expected([host[0].astype(np.float32)], [3, 0, 1], aug, 0, list(range(n)))
        assert np.array_equal(_bits(dst.cpu().numpy()), _bits(want)) and _guards_intact(full, dst.numel(), dst_skew)


# ---------------------------------------------------------------------------------------------- 2. lanes and target point
COUNTS, LMAX, NODES = [0, 1, 3, 8, 10], 8, 10


@pytest.fixture(scope="module")
def lane_store():
    """(host rows [sum(COUNTS), NODES, 5] f32, row_off, target points [n, 2] f32) - coordinates within +-64, some lanes with
    trailing all-zero nodes (the reference's padding), one node that is -0.0 throughout."""
    rng = np.random.RandomState(7)
    rows = rng.uniform(-64, 64, (sum(COUNTS), NODES, 5)).astype(np.float32)
    rows[1, 6:] = 0.0
    rows[4, 3:] = 0.0
    rows[13, 9:] = 0.0
    rows[2, 5] = -0.0
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    tp = (rng.randn(len(COUNTS), 2) * 20.0).astype(np.float32)
    return rows, off, tp


def _map_launch(store, index, noise, epoch, sample_id=None, lanes=True, target=True, lmax=LMAX):
    from mmfn_amd import ops
    rows, off, tp = store
    n, B = len(COUNTS), len(index)
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    out = {}
    parts = {}
    if lanes:
        out["lane_full"], out["lane"] = _guarded((B, lmax, NODES, 5))
        out["count_full"] = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
        out["count"] = out["count_full"][1:B + 1]
        parts["lanes"] = dict(src=torch.from_numpy(rows).to(DEV).view(-1, NODES * 5), row_off=torch.from_numpy(off).to(DEV), dst=out["lane"],
                              count_out=out["count"], lane_thresh=noise.lane_thresh, shift=noise.shift, yaw_rad=noise.yaw_rad)
    if target:
        out["tp_full"], out["tp"] = _guarded((B, 2))
        parts["target"] = dict(src=torch.from_numpy(tp).to(DEV), dst=out["tp"], shift=noise.target_shift)
    ops.gather_augment(idx, n, sample_id=sample_id, map_state=_state(noise.seed, epoch), **parts)
    return out


def _map_expected(store, index, noise, epoch, ids, lmax=LMAX):
    """(plain padded lanes [B, lmax, NODES, 5], reference lanes, counts, target points) of that launch"""
    from mmfn_amd import data as D
    rows, off, tp = store
    n = len(COUNTS)
    take = [min(max(i, 0), n - 1) for i in index]
    plain = np.zeros((len(take), lmax, NODES, 5), dtype=np.float32)
    for b, i in enumerate(take):
        c = min(COUNTS[i], lmax)
        plain[b, :c] = rows[off[i]:off[i] + c]
    lanes, counts, tps = D.map_noise_reference(plain, [COUNTS[i] for i in take], tp[take], [ids[i] for i in take], noise, epoch)
    return plain, lanes, counts, tps


MAP_INDEX = [4, 0, 3, 2, 1, 3, -1, 7]        # every count, a repeat, both ends out of range
MAP_PERM = [3, 0, 4, 1, 2]


def test_lane_dropout_alone_is_bit_exact(lane_store):
    from mmfn_amd.data import MapNoise
    perm = torch.tensor(MAP_PERM, dtype=torch.int64, device=DEV)
    dropped = 0
    for sample_id, ids in ((None, list(range(5))), (perm, MAP_PERM)):
        for seed, p in ((3, 0.5), (4, 0.5), (5, 1.0)):
            noise = MapNoise(lane_drop=p, seed=seed)
            out = _map_launch(lane_store, MAP_INDEX, noise, 5, sample_id, target=False)
            plain, lanes, counts, _ = _map_expected(lane_store, MAP_INDEX, noise, 5, ids)
            assert np.array_equal(_bits(out["lane"].cpu().numpy()), _bits(lanes))              # values, order and the +0.0 padding rows
            assert out["count"].cpu().tolist() == counts.tolist()
            assert _guards_intact(out["lane_full"], out["lane"].numel()) and out["count_full"][[0, -1]].tolist() == [-7, -7]
            dropped += sum(COUNTS[min(max(i, 0), 4)] for i in MAP_INDEX) - int(counts.sum())
    assert dropped > 20                                                     # (the cases above do drop lanes)


def test_lane_transform_and_target_shift_stay_inside_the_derived_bounds(lane_store):
    from mmfn_amd.data import MapNoise
    rows, _, tp = lane_store
    perm = torch.tensor(MAP_PERM, dtype=torch.int64, device=DEV)
    worst = worst_tp = 0.0
    for sample_id, ids in ((None, list(range(5))), (perm, MAP_PERM)):
        for noise in (MapNoise(shift=0.5, yaw_deg=2.0, target_shift=0.5, seed=6), MapNoise(shift=0.5, yaw_deg=2.0, lane_drop=0.5, seed=7),
                      MapNoise(yaw_deg=45.0, target_shift=64.0, seed=8), MapNoise(shift=64.0, seed=9)):
            out = _map_launch(lane_store, MAP_INDEX, noise, 3, sample_id)
            plain, lanes, counts, tps = _map_expected(lane_store, MAP_INDEX, noise, 3, ids)
            got = out["lane"].cpu().numpy()
            assert out["count"].cpu().tolist() == counts.tolist()
            assert np.array_equal(_bits(got[..., 2:]), _bits(lanes[..., 2:]))                  # f2..f4, bit for bit
            padding = (lanes == 0.0).all(axis=-1)                                              # all-zero nodes and rows: untouched
            assert padding.any() and np.array_equal(_bits(got[padding]), _bits(lanes[padding]))
            M = max(float(np.abs(rows[..., :2]).max()), noise.shift)
            err = float(np.abs(got[..., :2].astype(np.float64) - lanes[..., :2]).max())
            worst = max(worst, err / (2.0 ** -24 * M))
            assert err <= 16 * 2.0 ** -24 * M, (noise.shift, noise.yaw_deg, err)
            still = _map_expected(lane_store, MAP_INDEX, MapNoise(lane_drop=noise.lane_drop, seed=noise.seed), 3, ids)[1]
            assert np.abs(got[..., :2] - still[..., :2])[~padding].max() > 0.05                # (the same lanes, and they did move)
            got_tp = out["tp"].cpu().numpy().astype(np.float64)
            bound = 2.0 ** -23 * (np.abs(tps) + noise.target_shift)
            worst_tp = max(worst_tp, float((np.abs(got_tp - tps) / np.maximum(bound, 1e-30)).max()))
            assert (np.abs(got_tp - tps) <= bound).all()
            if noise.target_shift == 0.0:
                assert np.array_equal(_bits(got_tp), _bits(tps))
            assert _guards_intact(out["lane_full"], out["lane"].numel()) and _guards_intact(out["tp_full"], out["tp"].numel())
    print("max |x', y' - float64 reference| = %.2f * 2^-24 * M (bound 16); target point: %.2f of its bound" % (worst, worst_tp))


def test_the_target_point_alone_and_a_launch_without_lanes(lane_store):
    """The form an 'img' store takes: no lane field, the target point only."""
    from mmfn_amd.data import MapNoise
    noise = MapNoise(target_shift=2.0, seed=12)
    out = _map_launch(lane_store, [1, 4, 4, 0], noise, 9, lanes=False)
    _, _, _, tps = _map_expected(lane_store, [1, 4, 4, 0], noise, 9, list(range(5)))
    got = out["tp"].cpu().numpy().astype(np.float64)
    assert (np.abs(got - tps) <= 2.0 ** -23 * (np.abs(tps) + 2.0)).all() and np.abs(got - lane_store[2][[1, 4, 4, 0]]).max() > 0.1
    assert np.array_equal(got[1], got[2]) and _guards_intact(out["tp_full"], 8)


def test_more_lanes_than_one_round_of_the_prefix_sum():
    """600 stored lanes: three rounds of 256 keep bits, and a sample cut at lmax."""
    from mmfn_amd import data as D, ops
    rng = np.random.RandomState(2)
    counts, lmax, nodes = [600, 257, 300], 512, 2
    rows = rng.uniform(-64, 64, (sum(counts), nodes, 5)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    noise = D.MapNoise(lane_drop=0.3, seed=1)
    full, dst = _guarded((3, lmax, nodes, 5))
    count = torch.empty(3, dtype=torch.int32, device=DEV)
    ops.gather_augment(torch.tensor([2, 0, 1], dtype=torch.int64, device=DEV), 3, map_state=_state(1, 4), lanes=dict(
        src=torch.from_numpy(rows).to(DEV).view(-1, nodes * 5), row_off=torch.from_numpy(off).to(DEV), dst=dst, count_out=count,
        lane_thresh=noise.lane_thresh))
    plain = np.zeros((3, lmax, nodes, 5), dtype=np.float32)
    for b, i in enumerate([2, 0, 1]):
        c = min(counts[i], lmax)
        plain[b, :c] = rows[off[i]:off[i] + c]
    want, want_counts, _ = D.map_noise_reference(plain, [counts[i] for i in [2, 0, 1]], np.zeros((3, 2)), [2, 0, 1], noise, 4)
    assert np.array_equal(_bits(dst.cpu().numpy()), _bits(want)) and count.cpu().tolist() == want_counts.tolist()
    assert _guards_intact(full, dst.numel()) and want_counts[1] < 600 - 100


# ---------------------------------------------------------------------------------------------- 3. capture
def test_a_captured_launch_follows_the_index_buffer_and_the_states(lane_store):
    from mmfn_amd import data as D, ops
    rows, off, tp = lane_store
    n, S, C, H, W = 5, 1, 2, 48, 96
    host, srcs, pals = _lidar_sources("pal4", n, S, C, H, W, seed=13)
    lid, noise = D.LidarDropout(cell_prob=0.3, erase_prob=1.0, seed=2), D.MapNoise(shift=0.5, yaw_deg=2.0, lane_drop=0.5, target_shift=0.5, seed=3)
    src, row_off, tps = torch.from_numpy(rows).to(DEV).view(-1, NODES * 5), torch.from_numpy(off).to(DEV), torch.from_numpy(tp).to(DEV)

    def launch(index, lidar_state, map_state, dst, lane, count, tpo):
        ops.gather_augment(index, n, map_state=map_state,
                           lidar=dict(srcs=srcs, palettes=pals, dst=dst, state=lidar_state, cell_thresh=lid.cell_thresh,
                                      erase_thresh=lid.erase_thresh, erase_h=lid.erase_bounds(H), erase_w=lid.erase_bounds(W)),
                           lanes=dict(src=src, row_off=row_off, dst=lane, count_out=count, lane_thresh=noise.lane_thresh, shift=noise.shift,
                                      yaw_rad=noise.yaw_rad),
                           target=dict(src=tps, dst=tpo, shift=noise.target_shift))

    def buffers():
        return (torch.full((2, C, H, W), -7.0, device=DEV), torch.full((2, LMAX, NODES, 5), -7.0, device=DEV),
                torch.full((2,), -7, dtype=torch.int32, device=DEV), torch.full((2, 2), -7.0, device=DEV))

    first = buffers()
    launch(torch.tensor([4, 3], dtype=torch.int64, device=DEV), _state(2, 0), _state(3, 0), *first)   # eager (loads the library too)
    index, lidar_state, map_state = torch.tensor([4, 3], dtype=torch.int64, device=DEV), _state(2, 0), _state(3, 0)
    out = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # one launch on the capture stream: no branches
        launch(index, lidar_state, map_state, *out)
    graph.replay()
    assert all(torch.equal(a, b) for a, b in zip(out, first))
    index.copy_(torch.tensor([2, 4], dtype=torch.int64, device=DEV))
    lidar_state.copy_(_state(9, 6))
    map_state.copy_(_state(8, 7))
    graph.replay()
    want = buffers()
    launch(torch.tensor([2, 4], dtype=torch.int64, device=DEV), _state(9, 6), _state(8, 7), *want)
    assert all(torch.equal(a, b) for a, b in zip(out, want)) and not any(torch.equal(a, b) for a, b in zip(out, first))
    ref = D.lidar_dropout_reference(np.stack([host[0][2], host[0][4]]), [2, 4], D.LidarDropout(cell_prob=0.3, erase_prob=1.0, seed=9), 6)
    assert np.array_equal(_bits(out[0].cpu().numpy()), _bits(ref))


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_bad_descriptors_raise_and_nothing_is_launched(lane_store):
    from mmfn_amd import _lib, ops
    from mmfn_amd.data import LidarDropout
    rows, off, tp = lane_store
    n, S, C, H, W, B = 5, 2, 2, 4, 8, 2
    _, f32, _ = _lidar_sources("f32", n, S, C, H, W, seed=1)
    _, codes, pals = _lidar_sources("pal4", n, S, C, H, W, seed=2)
    lidar_state, map_state = _state(1, 0), _state(2, 0)
    index = torch.tensor([1, 2, 0, 0], dtype=torch.int64, device=DEV)   # (longer than B: the +4-byte pointer below stays inside)
    src, row_off, tps = torch.from_numpy(rows).to(DEV).view(-1, NODES * 5), torch.from_numpy(off).to(DEV), torch.from_numpy(tp).to(DEV)
    dsts = [torch.full((B * S, C, H, W), -7.0, device=DEV), torch.full((B, LMAX, NODES, 5), -7.0, device=DEV),
            torch.full((B, 2), -7.0, device=DEV)]
    count = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ALL = _lib.AUGMENT_LIDAR | _lib.AUGMENT_LANES | _lib.AUGMENT_TARGET

    def desc(srcs=f32, palettes=None, **over):
        d = _lib.GatherAugmentDesc()
        for s, t in enumerate(srcs):
            d.lidar_src[s] = t.data_ptr()
            if palettes:
                d.lidar_palette[s] = palettes[s].data_ptr()
        d.parts, d.sample_id = ALL, None
        d.lidar_dst, d.lidar_state = dsts[0].data_ptr(), lidar_state.data_ptr()
        d.n_frames, d.src_type, d.C, d.H, d.W = len(srcs), _lib.GATHER_PAL4 if palettes else _lib.GATHER_F32, C, H, W
        d.cell_thresh = d.erase_thresh = d.lane_thresh = 1 << 23
        d.erase_h_min, d.erase_h_max, d.erase_w_min, d.erase_w_max = 1, H, 1, W
        d.lane_src, d.lane_row_off, d.lane_dst, d.lane_count_out = src.data_ptr(), row_off.data_ptr(), dsts[1].data_ptr(), count.data_ptr()
        d.lane_nodes, d.lmax, d.shift, d.yaw_rad = NODES, LMAX, 0.5, 0.03
        d.target_src, d.target_dst, d.target_shift, d.map_state = tps.data_ptr(), dsts[2].data_ptr(), 0.5, map_state.data_ptr()
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def call(d, idx=index.data_ptr(), b=B, rows=n):
        ops._call("mmfn_gather_augment", ctypes.byref(d) if d is not None else None, idx, b, rows, _lib.stream())

    def at(member, s, ptr, **kw):
        d = desc(**kw)
        getattr(d, member)[s] = ptr
        return d

    bad = {
        "d NULL": lambda: call(None),
        "index NULL": lambda: call(desc(), idx=None),
        "index misaligned": lambda: call(desc(), idx=index.data_ptr() + 4),
        "parts 0": lambda: call(desc(parts=0)),
        "parts 8": lambda: call(desc(parts=8)),
        "sample_id misaligned": lambda: call(desc(sample_id=index.data_ptr() + 4)),
        "n_frames 0": lambda: call(desc(n_frames=0)),
        "n_frames 5": lambda: call(desc(n_frames=5)),
        "lidar_src[0] NULL": lambda: call(at("lidar_src", 0, None)),
        "lidar_src[1] NULL": lambda: call(at("lidar_src", 1, None)),
        "f32 lidar_src misaligned": lambda: call(at("lidar_src", 1, f32[1].data_ptr() + 2)),
        "lidar_dst NULL": lambda: call(desc(lidar_dst=None)),
        "lidar_dst misaligned": lambda: call(desc(lidar_dst=dsts[0].data_ptr() + 2)),
        "lidar_state NULL": lambda: call(desc(lidar_state=None)),
        "lidar_state misaligned": lambda: call(desc(lidar_state=lidar_state.data_ptr() + 4)),
        "src_type 7": lambda: call(desc(src_type=7)),
        "src_type -1": lambda: call(desc(src_type=-1)),
        "PAL4 without a palette": lambda: call(desc(codes, None, src_type=_lib.GATHER_PAL4)),
        "PAL4 palette[1] NULL": lambda: call(at("lidar_palette", 1, None, srcs=codes, palettes=pals)),
        "PAL4 odd row": lambda: call(desc(codes, pals, C=1, H=5, W=3, erase_thresh=0)),
        "C 0": lambda: call(desc(C=0)),
        "H 0": lambda: call(desc(H=0)),
        "W -1": lambda: call(desc(W=-1)),
        "cell_thresh 2^24 + 1": lambda: call(desc(cell_thresh=(1 << 24) + 1)),
        "erase_thresh 2^24 + 1": lambda: call(desc(erase_thresh=(1 << 24) + 1)),
        "lane_thresh 2^24 + 1": lambda: call(desc(lane_thresh=(1 << 24) + 1)),
        "h_min 0": lambda: call(desc(erase_h_min=0)),
        "h_min > h_max": lambda: call(desc(erase_h_min=3, erase_h_max=2)),
        "h_max > H": lambda: call(desc(erase_h_max=H + 1)),
        "w_min 0": lambda: call(desc(erase_w_min=0)),
        "w_min > w_max": lambda: call(desc(erase_w_min=3, erase_w_max=2)),
        "w_max > W": lambda: call(desc(erase_w_max=W + 1)),
        "lane_src NULL": lambda: call(desc(lane_src=None)),
        "lane_src misaligned": lambda: call(desc(lane_src=src.data_ptr() + 2)),
        "lane_row_off NULL": lambda: call(desc(lane_row_off=None)),
        "lane_row_off misaligned": lambda: call(desc(lane_row_off=row_off.data_ptr() + 4)),
        "lane_dst NULL": lambda: call(desc(lane_dst=None)),
        "lane_dst misaligned": lambda: call(desc(lane_dst=dsts[1].data_ptr() + 2)),
        "lane_count_out misaligned": lambda: call(desc(lane_count_out=count.data_ptr() + 2)),
        "lane_nodes 0": lambda: call(desc(lane_nodes=0)),
        "lmax -1": lambda: call(desc(lmax=-1)),
        "lmax 4097": lambda: call(desc(lmax=4097)),
        "map_state NULL": lambda: call(desc(map_state=None)),
        "map_state misaligned": lambda: call(desc(map_state=map_state.data_ptr() + 4)),
        "map_state NULL, target only": lambda: call(desc(map_state=None, parts=_lib.AUGMENT_TARGET)),
        "target_src NULL": lambda: call(desc(target_src=None)),
        "target_src misaligned": lambda: call(desc(target_src=tps.data_ptr() + 2)),
        "target_dst NULL": lambda: call(desc(target_dst=None)),
        "target_dst misaligned": lambda: call(desc(target_dst=dsts[2].data_ptr() + 2)),
        "yaw_rad above pi / 4": lambda: call(desc(yaw_rad=0.7854 + 1e-4)),
        "B -1": lambda: call(desc(), b=-1),
        "B 65536": lambda: call(desc(), b=65536),
        "n 0": lambda: call(desc(), rows=0),
    }
    for name in ("shift", "target_shift"):
        for v in (-0.1, 64.5, float("nan")):
            bad["%s %r" % (name, v)] = lambda name=name, v=v: call(desc(**{name: v}))
    for v in (-0.01, float("nan")):
        bad["yaw_rad %r" % v] = lambda v=v: call(desc(yaw_rad=v))
    for what, run in bad.items():
        with pytest.raises(_lib.MMFNLibraryError):
            run()
            pytest.fail("accepted: " + what)
    # the wrapper's own refusals: a lane-augmented launch of more than 4096 lanes, frames of another form
    with pytest.raises(ValueError):
        ops.gather_augment(index[:B], n, map_state=map_state, lanes=dict(src=src, row_off=row_off, dst=torch.empty(B, 4097, NODES, 5, device=DEV),
                                                                         lane_thresh=1 << 23))
    with pytest.raises(ValueError):
        ops.gather_augment(index[:B], n, lidar=dict(srcs=f32 * 3, dst=dsts[0], state=lidar_state))
    call(desc(), b=0)                                                       # an empty batch: nothing to do
    call(desc(), b=0, rows=0)
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in dsts) and count.tolist() == [-7, -7]
    # a part that is not named is not read; bounds are ignored while nothing is erased; the largest values are inside
    call(desc(parts=_lib.AUGMENT_LIDAR, lane_src=None, target_dst=None, map_state=None, shift=99.0, lmax=-1))
    call(desc(parts=_lib.AUGMENT_LANES, n_frames=0, lidar_dst=None, target_shift=float("nan"), lane_count_out=None))
    call(desc(erase_thresh=0, erase_h_min=0, erase_h_max=99, erase_w_min=-3, erase_w_max=0, shift=64.0, target_shift=64.0,
              yaw_rad=float(np.float32(np.pi / 4)), cell_thresh=1 << 24, lane_thresh=1 << 24))
    call(desc(codes, pals, erase_thresh=1 << 24))
    torch.cuda.synchronize()
    assert not any(bool((t == -7.0).any()) for t in dsts) and -7 not in count.tolist()
    assert LidarDropout(cell_prob=1.0).cell_thresh == 1 << 24


# ---------------------------------------------------------------------------------------------- 5. the loader
def _pack_store(tmp, samples):
    from mmfn_amd import data as D
    for s in samples:
        s["radar_adj"] = D.radar_adjacency(s["radar"][0])
    return D.PackedFrames(D.pack_frames(samples, str(tmp / "packed")))


@pytest.fixture(scope="module")
def packed_vec(tmp_path_factory):
    from oracle import fixtures
    return _pack_store(tmp_path_factory.mktemp("augment_vec"), fixtures.synthetic_samples((5, 9, 3, 7, 1), seed=5, radar_counts=(50, 100, 81, 3, 90)))


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
    return _pack_store(tmp_path_factory.mktemp("augment_img"), samples)


LIDAR = dict(cell_prob=0.1, erase_prob=0.5)
NOISE = dict(shift=0.5, yaw_deg=2.0, lane_drop=0.5, target_shift=0.5)


def _check_batch(got, want, idx, S, lidar, noise, epoch, lanes=True):
    """An augmented batch `got` against the references applied to the plain loader's batch `want` of the samples idx."""
    from mmfn_amd import data as D
    (ginp, ggt), (winp, wgt) = got, want
    assert list(ginp) == list(winp) and torch.equal(ggt, wgt)
    for k in winp:
        assert ginp[k].dtype == winp[k].dtype and ginp[k].shape == winp[k].shape and ginp[k].is_contiguous(), k
        if k not in ("lidar", "lane", "lane_num", "target_point"):
            assert torch.equal(ginp[k], winp[k]), k                                            # camera, velocity, radar, map: plain
    ref = D.lidar_dropout_reference(winp["lidar"].cpu().numpy(), np.repeat(idx, S), lidar, epoch)
    assert np.array_equal(_bits(ginp["lidar"].cpu().numpy()), _bits(ref)) and not torch.equal(ginp["lidar"], winp["lidar"])
    tp = winp["target_point"].cpu().numpy()
    if lanes:
        plain = winp["lane"].cpu().numpy()
        ref_lane, ref_count, ref_tp = D.map_noise_reference(plain, winp["lane_num"].cpu().numpy(), tp, idx, noise, epoch)
        got_lane = ginp["lane"].cpu().numpy()
        assert ginp["lane_num"].cpu().tolist() == ref_count.tolist()
        assert np.array_equal(_bits(got_lane[..., 2:]), _bits(ref_lane[..., 2:]))
        M = max(float(np.abs(plain[..., :2]).max()), noise.shift)
        assert np.abs(got_lane[..., :2].astype(np.float64) - ref_lane[..., :2]).max() <= 16 * 2.0 ** -24 * M
    else:
        ref_tp = D.map_noise_reference(np.zeros((len(idx), 0, 1, 5)), [0] * len(idx), tp, idx, noise, epoch)[2]
    got_tp = ginp["target_point"].cpu().numpy().astype(np.float64)
    assert (np.abs(got_tp - ref_tp) <= 2.0 ** -23 * (np.abs(ref_tp) + noise.target_shift)).all() and np.abs(got_tp - tp).max() > 1e-3


@pytest.mark.parametrize("variant", ["vec", "rad", "img"])
def test_an_augmented_epoch_equals_the_references_on_the_plain_batches(packed_vec, packed_img, variant):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    packed, S = (packed_img, 2) if variant == "img" else (packed_vec, 1)
    cfg = GlobalConfig(seq_len=S)
    n = len(packed)
    res = D.ResidentFrames(packed, DEV, cfg, variant, max_bytes=BUDGET)
    plan, nbytes = D.ResidentFrames.plan(packed, cfg, variant), res.nbytes()
    lidar = D.LidarDropout(seed=11, **LIDAR)
    noise = D.MapNoise(seed=12, **NOISE) if variant != "img" else D.MapNoise(seed=12, target_shift=0.5)
    if variant == "img":                                                   # no lane field to move or thin out
        for part in (dict(shift=0.5), dict(yaw_deg=2.0), dict(lane_drop=0.5)):
            with pytest.raises(ValueError):
                D.ResidentLoader(res, 2, augment=D.Augment(map=D.MapNoise(**part)))
    aug = D.ResidentLoader(res, 2, shuffle=True, seed=3, lane_bucket=4, augment=D.Augment(lidar=lidar, map=noise))
    plain = D.ResidentLoader(res, 2, shuffle=True, seed=3, lane_bucket=4)
    assert res.nbytes() == nbytes == plan["bytes"] and set(res.tensors) == set(plan["fields"])      # the store is as it was
    assert not hasattr(aug, "gray_mean") and not hasattr(aug, "jitter_state") and aug.sample_id.tolist() == list(range(n))
    first = {}
    for epoch in range(2):
        chunks = D._chunks(D._epoch_order(n, True, None, 3, epoch), 2, False)
        got, want = list(aug), list(plain)
        assert len(got) == len(want) == len(chunks)
        for g, w, idx in zip(got, want, chunks):
            _check_batch(g, w, idx, S, lidar, noise, epoch, lanes=variant != "img")
            for b, i in enumerate(idx):
                mine = (g[0]["lidar"][b * S:(b + 1) * S].clone(), g[0]["target_point"][b].clone())
                if epoch == 0:
                    first[i] = mine
                else:                                                      # the second epoch: other draws for every sample
                    assert not torch.equal(mine[0], first[i][0]) and not torch.equal(mine[1], first[i][1]), i
    assert aug.epoch == plain.epoch == 2 and aug.lidar_state.tolist() == [11, 1] and aug.map_state.tolist() == [12, 1]


def test_a_shard_draws_what_the_full_store_draws(packed_vec):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    aug = D.Augment(lidar=D.LidarDropout(seed=4, **LIDAR), map=D.MapNoise(seed=5, **NOISE))
    full = D.ResidentFrames(packed_vec, DEV, cfg, "vec", max_bytes=BUDGET)
    shard = D.ResidentFrames(packed_vec, DEV, cfg, "vec", indices=[1, 3], max_bytes=BUDGET)
    a, b = D.ResidentLoader(full, 5, augment=aug), D.ResidentLoader(shard, 2, augment=aug)
    assert b.sample_id.tolist() == [1, 3]
    for epoch in range(2):
        (fa, _), = list(a)
        (fb, _), = list(b)
        for row, i in ((0, 1), (1, 3)):
            assert torch.equal(fb["lidar"][row], fa["lidar"][i]) and torch.equal(fb["target_point"][row], fa["target_point"][i])
            assert fb["lane_num"][row] == fa["lane_num"][i]
            kept = int(fb["lane_num"][row])
            assert torch.equal(fb["lane"][row, :kept], fa["lane"][i, :kept])
        assert not torch.equal(fb["lidar"][1], fa["lidar"][1])


def test_inactive_parts_and_the_compact_store(packed_vec):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    res = D.ResidentFrames(packed_vec, DEV, cfg, "vec", max_bytes=BUDGET)
    small = D.ResidentFrames(packed_vec, DEV, cfg, "vec", max_bytes=BUDGET, compact=True)
    assert small.plan_["compact"] == ["lidars.0"]
    kw = dict(shuffle=True, seed=1, lane_bucket=16)
    plain = list(D.ResidentLoader(res, 2, **kw))
    same = lambda x, y: all(list(a[0]) == list(b[0]) and all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and torch.equal(a[1], b[1])
                            for a, b in zip(x, y)) and len(x) == len(y)
    for aug in (D.Augment(), D.Augment(camera=D.CameraJitter(), lidar=D.LidarDropout(seed=3), map=D.MapNoise(seed=4))):
        loader = D.ResidentLoader(res, 2, augment=aug, **kw)
        assert not any(isinstance(v, torch.Tensor) for v in vars(loader).values())              # nothing to hold: the plain launch
        assert same(list(loader), plain)
    # Augment(camera=j) is augment=j
    j = D.CameraJitter(0.4, 0.4, 0.4, erase_prob=0.5, seed=6)
    assert same(list(D.ResidentLoader(res, 2, augment=D.Augment(camera=j), **kw)), list(D.ResidentLoader(res, 2, augment=j, **kw)))
    # the coded store: the same augmented bits as the f32 store, all three launches on
    everything = D.Augment(camera=j, lidar=D.LidarDropout(seed=7, **LIDAR), map=D.MapNoise(seed=8, **NOISE))
    a, b = list(D.ResidentLoader(res, 2, augment=everything, **kw)), list(D.ResidentLoader(small, 2, augment=everything, **kw))
    assert same(a, b) and not same(a, plain)
    assert not any(torch.equal(x[0][k], y[0][k]) for x, y in zip(a, plain) for k in ("image", "lidar", "lane", "target_point"))
    assert all(torch.equal(x[0][k], y[0][k]) for x, y in zip(a, plain) for k in ("velocity",))


def test_a_field_the_kernel_cannot_take_is_refused(packed_vec):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    res = D.ResidentFrames(packed_vec, DEV, GlobalConfig(), "vec", max_bytes=BUDGET)
    assert len(res.lidar_frames()[0]) == 1 and res.lidar_frames()[1] is None
    res.shapes = dict(res.shapes, **{"lidars.0": (2 * 256 * 256,)})
    with pytest.raises(ValueError):
        res.lidar_frames()
    with pytest.raises(ValueError):
        D.ResidentLoader(res, 2, augment=D.Augment(lidar=D.LidarDropout(0.1)))
    D.ResidentLoader(res, 2, augment=D.Augment(lidar=D.LidarDropout()))      # an inactive part does not care
    with pytest.raises(TypeError):
        D.ResidentLoader(res, 2, augment={"lidar": D.LidarDropout(0.1)})


def test_one_epoch_of_trainer_train_with_everything_on(tmp_path):
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
    everything = D.Augment(camera=D.CameraJitter(0.4, 0.4, 0.4, erase_prob=0.5, seed=1), lidar=D.LidarDropout(seed=2, **LIDAR),
                           map=D.MapNoise(seed=3, **NOISE))
    shapes = {}
    for name, augment in (("plain", None), ("augmented", everything)):
        loader = D.ResidentLoader(res, 2, shuffle=True, seed=2, lane_bucket=16, augment=augment)
        net = M.MMFN(cfg, DEV)
        net.load_state_dict(oracle.state_dict(), strict=True)
        tr = Trainer(DEV, None)
        tr.train(net, loader, cfg, FusedAdamW(net, lr=1e-4), graph=True, lane_bucket=16)
        assert len(tr.train_loss) == 1 and np.isfinite(tr.train_loss[0]) and tr.cur_iter == 2
        assert not any(isinstance(v, str) for v in tr._static_steps.values())                   # captured, not refused
        shapes[name] = len(tr._static_steps)
    assert shapes["augmented"] <= shapes["plain"] == 1
    assert loader.lidar_state.tolist() == [2, 0] and loader.map_state.tolist() == [3, 0] and loader.jitter_state.tolist() == [1, 0]
