"""Compact device-resident store on the GPU: the gather kernel's 4-bit palette source type against torch indexing, and the batches
of ResidentFrames(..., compact=True) against the plain store and the PackedFrames.batch -> stage_batch -> MMFN._pack chain, bit
for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUDGET = 64 << 20   # max_bytes of the stores here (3-5 samples of ~0.9 MB)


# ---------------------------------------------------------------------------------------------- 1. the ABI against torch
def _palette(count, seed):
    """f32 [16] on the device: `count` distinct entries, the rest +0.0.  The 16-entry one holds -0.0, a NaN and an infinity."""
    g = torch.Generator().manual_seed(100 + seed)
    pal = torch.zeros(16)
    pal[:count] = torch.randn(count, generator=g) + torch.arange(count) * 4.0        # distinct
    if count == 16:
        pal[3], pal[7], pal[11] = -0.0, float("nan"), float("inf")
    return pal.to(DEV)


def _coded(n, row, count, seed, skew=0):
    """Codes u8 [n, row / 2] on the device, every nibble < count; skew > 0 starts the buffer that many BYTES past an allocation
    boundary."""
    g = torch.Generator().manual_seed(seed)
    nib = torch.randint(0, count, (n * row + 2 * skew,), generator=g)
    full = (nib[0::2] | (nib[1::2] << 4)).to(torch.uint8)
    return full.to(DEV)[skew:].view(n, row // 2)


def _decoded(codes, pal):
    """f32 [n, row]: element 2j from the low nibble of byte j, element 2j + 1 from the high one."""
    c = codes.long()
    return torch.stack([pal[c & 15], pal[c >> 4]], dim=-1).view(codes.shape[0], -1)


def _source(kind, n, row, seed):
    g = torch.Generator().manual_seed(seed)
    full = torch.randint(0, 256, (n * row,), generator=g).to(torch.uint8) if kind == "u8" else torch.randn(n * row, generator=g)
    return full.to(DEV).view(n, row)


def _guarded(numel, pad=16):
    """f32 destination of `numel` elements between two sentinel zones (pad floats = 64 bytes keep the allocator's alignment)."""
    full = torch.full((numel + 2 * pad,), -7.0, device=DEV)
    return full, full[pad:pad + numel]


def _guards_intact(full, numel, pad=16):
    return bool((full[:pad] == -7.0).all()) and bool((full[pad + numel:] == -7.0).all())


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("index", [[5], [0, 5, 2, 2, 0]], ids=["B1", "B5"])
@pytest.mark.parametrize("count", [1, 6, 16])
@pytest.mark.parametrize("row", [2, 26, 8198, 131072])      # 1 byte; 13 bytes (every alignment); 4099 bytes = 2 pieces; 16 pieces
def test_coded_gather_equals_index_select_of_the_decoded_source(row, count, index):
    from mmfn_amd import ops
    n, B = 6, len(index)
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    pal = _palette(count, seed=count)
    for skew in (0, 1):
        src = _coded(n, row, count, seed=row + skew, skew=skew)
        assert src.data_ptr() % 16 == skew
        full, dst = _guarded(B * row)
        ops.gather_batch([ops.gather_field(src, dst, palette=pal)], idx, n)
        want = _decoded(src, pal).index_select(0, idx)
        assert _same_bits(dst.view(B, row), want), (row, count, skew)
        if count < 16:                                   # (no NaN in these palettes)
            assert torch.equal(dst.view(B, row), want)
        assert _guards_intact(full, B * row)


@pytest.mark.parametrize("row", [26, 8198])
def test_an_odd_destination_offset_takes_the_element_path(row):
    """dst_offset = 1 with a 16-byte aligned code row: source and destination are misaligned differently, so nothing is moved
    16 bytes at a time; the floats around each destination row stay untouched."""
    from mmfn_amd import ops
    n, index, stride = 6, [0, 5, 2, 2, 0], row + 4
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    pal = _palette(6, seed=1)
    src = _coded(n, row, 6, seed=row)
    full, dst = _guarded(len(index) * stride)
    ops.gather_batch([ops.gather_field(src, dst, dst_stride=stride, dst_offset=1, palette=pal)], idx, n)
    got = dst.view(len(index), stride)
    assert torch.equal(got[:, 1:1 + row], _decoded(src, pal).index_select(0, idx))
    assert bool((got[:, 0] == -7.0).all()) and bool((got[:, 1 + row:] == -7.0).all()) and _guards_intact(full, dst.numel())


def test_coded_u8_f32_and_ragged_fields_in_one_launch():
    from mmfn_amd import ops
    counts = [0, 1, 9, 3]
    n = len(counts)
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=DEV)
    lanes = _source("f32", sum(counts), 50, seed=1)
    pal = _palette(16, seed=2)
    coded, pixels, floats = _coded(n, 8198, 16, seed=3), _source("u8", n, 4099, seed=4), _source("f32", n, 405, seed=5)
    for index in ([2], [2, 0, 1, 3, 2]):
        B, lmax = len(index), 9
        idx = torch.tensor(index, dtype=torch.int64, device=DEV)
        outs = [_guarded(B * r) for r in (8198, 4099, 405)]
        lane_full, lane = _guarded(B * lmax * 50)
        lane_num = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        ops.gather_batch([ops.gather_field(pixels, outs[1][1]), ops.gather_field(coded, outs[0][1], palette=pal),
                          ops.gather_field(lanes, lane, row_off=off, count_out=lane_num, lmax=lmax),
                          ops.gather_field(floats, outs[2][1])], idx, n)
        assert _same_bits(outs[0][1].view(B, -1), _decoded(coded, pal).index_select(0, idx))
        assert torch.equal(outs[1][1].view(B, -1), pixels.index_select(0, idx).float())
        assert torch.equal(outs[2][1].view(B, -1), floats.index_select(0, idx))
        want = torch.zeros(B, lmax, 50, device=DEV)
        for b, i in enumerate(index):
            want[b, :counts[i]] = lanes[int(off[i]):int(off[i + 1])]
        assert _same_bits(lane, want.view(-1)) and lane_num.tolist() == [counts[i] for i in index]
        assert all(_guards_intact(full, o.numel()) for full, o in outs) and _guards_intact(lane_full, lane.numel())


def test_two_coded_frames_per_sample_land_interleaved():
    from mmfn_amd import ops
    n, row, index = 4, 8198, [3, 0, 3]
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    pa, pb = _palette(6, seed=1), _palette(6, seed=2)
    a, b = _coded(n, row, 6, seed=7), _coded(n, row, 6, seed=8)
    full, dst = _guarded(len(index) * 2 * row)
    ops.gather_batch([ops.gather_field(a, dst, dst_stride=2 * row, palette=pa),
                      ops.gather_field(b, dst, dst_stride=2 * row, dst_offset=row, palette=pb)], idx, n)
    want = torch.stack([_decoded(a, pa).index_select(0, idx), _decoded(b, pb).index_select(0, idx)], dim=1).flatten(0, 1)
    assert torch.equal(dst.view(-1, row), want) and _guards_intact(full, dst.numel())


def test_a_bad_coded_descriptor_is_refused_and_nothing_is_launched():
    from mmfn_amd import ops
    from mmfn_amd._lib import MMFNLibraryError
    n, row = 3, 8
    pal = _palette(6, seed=1)
    src = _coded(n, row, 6, seed=1)
    idx = torch.tensor([1, 2], dtype=torch.int64, device=DEV)
    dst = torch.full((2, row), -7.0, device=DEV)
    off = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device=DEV)
    good = ops.gather_field(src, dst, palette=pal)
    no_palette = ops.gather_field(src, dst, palette=pal)
    no_palette.palette = None
    for bad in (no_palette,                                                        # NULL palette
                ops.gather_field(src, dst, row_elems=7, palette=pal),              # odd row_elems
                ops.gather_field(src, dst, row_off=off, lmax=1, palette=pal)):     # a coded ragged field
        with pytest.raises(MMFNLibraryError):
            ops.gather_batch([good, bad], idx, n)
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())
    ops.gather_batch([good], idx, n)
    assert torch.equal(dst, _decoded(src, pal)[1:3])


# ---------------------------------------------------------------------------------------------- 2. batches against the host chain
LANES = (5, 9, 3, 7, 1)


def _pack_store(tmp, samples):
    from mmfn_amd import data as D
    for s in samples:
        s["radar_adj"] = D.radar_adjacency(s["radar"][0])
    return D.PackedFrames(D.pack_frames(samples, str(tmp / "packed")))


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    from oracle import fixtures
    return _pack_store(tmp_path_factory.mktemp("compact"), fixtures.synthetic_samples(LANES, seed=5, radar_counts=(50, 100, 81, 3, 90)))


@pytest.fixture(scope="module")
def nets():
    """One MMFN per variant: only its _pack (the reference forward's argument packing) is used."""
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd import model as M
    return {v: M.MMFN(GlobalConfig(), DEV, v) for v in ("vec", "img", "rad")}


def _chain(net, packed, idx, cfg):
    from mmfn_amd import data as D
    args, gt = D.stage_batch(packed.batch(idx), DEV, cfg, non_blocking=False)
    return net._pack(*args), gt


def _same_batch(got, want):
    (ginp, ggt), (winp, wgt) = got, want
    assert list(ginp) == list(winp)
    for k in winp:
        g, w = ginp[k], winp[k]
        assert g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous() and g.device == w.device, k
        assert torch.equal(g, w), k
    assert ggt.dtype == wgt.dtype and ggt.shape == wgt.shape and ggt.is_contiguous() and torch.equal(ggt, wgt)


def _epochs_agree(packed, net, cfg, variant, n, indices=None, epochs=2, coded=("lidars.0",)):
    """Every batch of `epochs` shuffled epochs (batch 2, the last one partial when n is odd): compact store == plain store == host
    chain.  Returns the compact store."""
    from mmfn_amd import data as D
    plain = D.ResidentFrames(packed, DEV, cfg, variant, indices=indices, max_bytes=BUDGET)
    small = D.ResidentFrames(packed, DEV, cfg, variant, indices=indices, max_bytes=BUDGET, compact=True)
    assert small.plan_["compact"] == list(coded) and plain.plan_["compact"] == []
    ids = list(range(len(packed))) if indices is None else list(indices)
    a, b = D.ResidentLoader(plain, 2, shuffle=True, seed=3), D.ResidentLoader(small, 2, shuffle=True, seed=3)
    for epoch in range(epochs):
        chunks = D._chunks(D._epoch_order(n, True, None, 3, epoch), 2, False)
        ba, bb = list(a), list(b)
        assert len(ba) == len(bb) == len(chunks) == (n + 1) // 2 and bb[-1][1].shape[0] == (n % 2 or 2)
        for x, y, rows in zip(ba, bb, chunks):
            _same_batch(y, x)
            _same_batch(y, _chain(net, packed, [ids[r] for r in rows], cfg))
    return small


@pytest.mark.parametrize("variant", ["vec", "img", "rad"])
def test_every_batch_of_the_compact_store_equals_the_plain_store_and_the_host_chain(packed, nets, variant):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    small = _epochs_agree(packed, nets[variant], cfg, variant, 5)
    assert small.tensors["lidars.0"].dtype == torch.uint8 and small.tensors["lidars.0"].shape == (5, 65536)
    assert small.tensors["lidars.0.palette"].shape == (16,)
    assert small.nbytes() == D.ResidentFrames.plan(packed, cfg, variant, compact=True)["bytes"] < D.ResidentFrames.plan(packed, cfg, variant)["bytes"]


def test_a_compact_shard_serves_its_rows(packed, nets):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    small = _epochs_agree(packed, nets["vec"], cfg, "vec", 2, indices=[1, 3], epochs=1)
    assert len(small) == 2 and small.nbytes() == D.ResidentFrames.plan(packed, cfg, "vec", indices=[1, 3], compact=True)["bytes"]


def test_two_coded_lidar_frames_per_sample_with_the_image_map_model(tmp_path):
    """seq_len = 2: both LiDAR frames are coded, each with its own palette, and frame s of sample b is batch entry 2 b + s."""
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd import model as M
    rng = np.random.RandomState(17)
    samples = []
    for n_lane in (4, 2, 6):
        samples.append({
            "fronts": [torch.from_numpy(rng.randint(0, 256, (3, 256, 256)).astype(np.uint8)) for _ in range(2)],
            "lidars": [(rng.randint(0, 6, (2, 256, 256)) / 5.0).astype(np.float32) + np.float32(s) for s in range(2)],
            "vectormaps": [torch.from_numpy(rng.randn(n_lane, 10, 5)) for _ in range(2)],
            "radar": [rng.randn(81, 5) for _ in range(2)],
            "maps": [torch.from_numpy(rng.randint(0, 256, (3, 256, 256)).astype(np.uint8)) for _ in range(2)],
            "waypoints": [tuple(rng.randn(2)) for _ in range(6)], "target_point": tuple(rng.randn(2) * 10.0),
            "steer": 0.1, "throttle": 0.5, "brake": False, "command": 2, "velocity": float(rng.uniform(0, 8))})
    packed = _pack_store(tmp_path, samples)
    cfg = GlobalConfig(seq_len=2)
    small = _epochs_agree(packed, M.MMFN(cfg, DEV, "img"), cfg, "img", 3, epochs=1, coded=("lidars.0", "lidars.1"))
    assert not torch.equal(small.tensors["lidars.0.palette"], small.tensors["lidars.1.palette"])
    inp, _ = small.gather(torch.tensor([2, 0], dtype=torch.int64, device=DEV), np.array([2, 0]))
    for b, i in enumerate((2, 0)):
        for s in range(2):
            assert torch.equal(inp["lidar"][2 * b + s].cpu(), torch.from_numpy(samples[i]["lidars"][s]))


def _lidar_samples(make):
    from oracle import fixtures
    samples = fixtures.synthetic_samples(LANES[:3], seed=9)
    rng = np.random.RandomState(4)
    for s in samples:
        s["lidars"] = [make(rng)]
    return samples


def test_a_seventeenth_value_keeps_the_field_f32(tmp_path, nets):
    """16 LiDAR values are coded; one element of one sample with a 17th keeps the whole field f32, with the plain store's bytes -
    and the same batches either way."""
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    samples = _lidar_samples(lambda rng: (rng.randint(0, 16, (2, 256, 256)) / 15.0).astype(np.float32))
    _epochs_agree(_pack_store(tmp_path / "a", samples), nets["vec"], cfg, "vec", 3, epochs=1)
    samples[1]["lidars"][0][1, 200, 77] = 7.0
    packed = _pack_store(tmp_path / "b", samples)
    small = _epochs_agree(packed, nets["vec"], cfg, "vec", 3, epochs=1, coded=())
    assert small.tensors["lidars.0"].dtype == torch.float32 and "lidars.0.palette" not in small.tensors
    assert small.nbytes() == small.plan_["bytes"] == D.ResidentFrames.plan(packed, cfg, "vec")["bytes"]


def test_a_float64_lidar_source_is_coded_after_its_rounding(tmp_path, nets):
    from mmfn_amd.config import GlobalConfig
    samples = _lidar_samples(lambda rng: rng.randint(0, 6, (2, 256, 256)) / 5.0)          # f64, as PRE_Data pickles hold it
    assert samples[0]["lidars"][0].dtype == np.float64
    small = _epochs_agree(_pack_store(tmp_path, samples), nets["vec"], GlobalConfig(), "vec", 3, epochs=1)
    assert small.tensors["lidars.0"].dtype == torch.uint8


# ---------------------------------------------------------------------------------------------- 3. capture and training
def test_a_captured_coded_gather_follows_the_index_buffer(packed):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    res = D.ResidentFrames(packed, DEV, GlobalConfig(), "vec", max_bytes=BUDGET, compact=True)
    index = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    rows = np.array([0, 1])
    first = res.gather(index.clone(), rows, lane_bucket=16)       # eager (also loads the library outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # one launch on the capture stream: no branches
        inp, gt = res.gather(index, rows, lane_bucket=16)
    graph.replay()
    _same_batch((inp, gt), first)
    index.copy_(torch.tensor([3, 2], dtype=torch.int64, device=DEV))
    graph.replay()
    want = res.gather(torch.tensor([3, 2], dtype=torch.int64, device=DEV), np.array([3, 2]), lane_bucket=16)
    _same_batch((inp, gt), want)
    assert not torch.equal(inp["lidar"], first[0]["lidar"])


def test_a_training_epoch_from_the_compact_store_gives_the_same_loss_bits(packed):
    """Trainer.train, 5 samples at batch 2, vec model, dropout 0.1: the loss of the epoch from the compact loader == from the plain
    one."""
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd import model as M
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import Trainer
    from oracle import harness
    oracle = harness.build_oracle("vec", dropout=0.1)
    cfg = GlobalConfig()
    losses = []
    for compact in (False, True):
        loader = D.ResidentLoader(D.ResidentFrames(packed, DEV, cfg, "vec", max_bytes=BUDGET, compact=compact), batch_size=2)
        net = M.MMFN(cfg, DEV)
        net.load_state_dict(oracle.state_dict(), strict=True)
        tr = Trainer(DEV, None)
        tr.train(net, loader, cfg, FusedAdamW(net, lr=1e-4))
        losses.append(tr.train_loss)
    assert losses[0] == losses[1] and np.isfinite(np.asarray(losses[0], dtype=np.float64)).all()
