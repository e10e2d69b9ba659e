"""Device-resident dataset on the GPU: the gather kernel's ABI against torch indexing, ResidentLoader's batches against the
PackedFrames.batch -> stage_batch -> MMFN._pack chain (bit for bit), a training epoch, graph capture and rank shards."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUDGET = 64 << 20   # max_bytes of the stores here (4-7 samples of ~0.9 MB)


# ---------------------------------------------------------------------------------------------- 1. the ABI against torch
def _source(kind, n, row, seed, skew=0):
    """[n, row] u8 / f32 on the device; skew > 0 starts it that many ELEMENTS past an allocation boundary."""
    g = torch.Generator().manual_seed(seed)
    full = torch.randint(0, 256, (n * row + skew,), generator=g).to(torch.uint8) if kind == "u8" else torch.randn(n * row + skew, generator=g)
    return full.to(DEV)[skew:].view(n, row)


def _guarded(numel, pad=16):
    """f32 destination of `numel` elements between two sentinel zones (pad floats = 64 bytes keep the allocator's alignment)."""
    full = torch.full((numel + 2 * pad,), -7.0, device=DEV)
    return full, full[pad:pad + numel]


def _guards_intact(full, numel, pad=16):
    return bool((full[:pad] == -7.0).all()) and bool((full[pad + numel:] == -7.0).all())


@pytest.mark.parametrize("index", [[5], [0, 5, 2, 2, 0]], ids=["B1", "B5"])
@pytest.mark.parametrize("kind,row", [("u8", 1), ("u8", 13), ("u8", 4099), ("u8", 196608),
                                      ("f32", 1), ("f32", 50), ("f32", 405), ("f32", 131072)])
def test_dense_gather_equals_index_select(kind, row, index):
    from mmfn_amd import ops
    n, B = 6, len(index)
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    for skew in (0, 1):       # rows of 13 / 4099 / 405 elements already start at every alignment; skew moves the base too
        src = _source(kind, n, row, seed=row + skew, skew=skew)
        full, dst = _guarded(B * row)
        ops.gather_batch([ops.gather_field(src, dst)], idx, n)
        want = src.index_select(0, idx).float()
        assert dst.dtype == torch.float32 and torch.equal(dst.view(B, row), want), (kind, row, skew)
        assert _guards_intact(full, B * row)


def test_several_fields_in_one_launch_ragged_padding_and_lane_counts():
    """Four dense fields and a ragged one per launch; lane sets of 0 / 1 / 9 / 3 rows of 50 floats padded to Lmax = 9 and 16 with
    +0.0 (bits compared), counts as int32."""
    from mmfn_amd import ops
    counts = [0, 1, 9, 3]
    n = len(counts)
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=DEV)
    lanes = _source("f32", sum(counts), 50, seed=1)
    dense = [_source("u8", n, 13, seed=2), _source("f32", n, 405, seed=3), _source("u8", n, 4099, seed=4), _source("f32", n, 1, seed=5)]
    for index in ([2], [2, 0, 1, 3, 2]):
        B = len(index)
        idx = torch.tensor(index, dtype=torch.int64, device=DEV)
        for lmax in (9, 16):
            outs = [_guarded(B * s.shape[1]) for s in dense]
            lane_full, lane = _guarded(B * lmax * 50)
            lane_full.fill_(float("nan"))          # padding must be WRITTEN, and as +0.0
            lane_num = torch.full((B,), -1, dtype=torch.int32, device=DEV)
            fields = [ops.gather_field(s, o[1]) for s, o in zip(dense, outs)]
            fields.insert(2, ops.gather_field(lanes, lane, row_off=off, count_out=lane_num, lmax=lmax))
            ops.gather_batch(fields, idx, n)
            for s, (full, o) in zip(dense, outs):
                assert torch.equal(o.view(B, -1), s.index_select(0, idx).float())
                assert _guards_intact(full, o.numel())
            want = torch.zeros(B, lmax, 50, device=DEV)
            for b, i in enumerate(index):
                want[b, :counts[i]] = lanes[int(off[i]):int(off[i + 1])]
            assert torch.equal(lane.view(torch.int32), want.view(-1).view(torch.int32))       # bits: padding is +0.0, not -0.0
            assert bool(torch.isnan(lane_full[:16]).all()) and bool(torch.isnan(lane_full[16 + lane.numel():]).all())
            assert lane_num.dtype == torch.int32 and lane_num.tolist() == [counts[i] for i in index]


def test_two_frames_per_sample_land_interleaved():
    from mmfn_amd import ops
    n, row, index = 4, 4099, [3, 0, 3]
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    a, b = _source("u8", n, row, seed=7), _source("u8", n, row, seed=8)
    fa, fb = _source("f32", n, 50, seed=9), _source("f32", n, 50, seed=10)
    full, dst = _guarded(len(index) * 2 * row)
    fdst = torch.empty(len(index) * 2, 50, device=DEV)
    ops.gather_batch([ops.gather_field(a, dst, dst_stride=2 * row), ops.gather_field(b, dst, dst_stride=2 * row, dst_offset=row),
                      ops.gather_field(fa, fdst, dst_stride=100), ops.gather_field(fb, fdst, dst_stride=100, dst_offset=50)], idx, n)
    want = torch.stack([a.index_select(0, idx).float(), b.index_select(0, idx).float()], dim=1).flatten(0, 1)   # model_vec.py:506-508
    assert torch.equal(dst.view(-1, row), want) and _guards_intact(full, dst.numel())
    assert torch.equal(fdst, torch.stack([fa.index_select(0, idx), fb.index_select(0, idx)], dim=1).flatten(0, 1))


def test_a_bad_descriptor_is_refused_and_nothing_is_launched():
    from mmfn_amd import ops
    from mmfn_amd._lib import MMFNLibraryError
    n = 3
    src = _source("f32", n, 8, seed=1)
    idx = torch.tensor([1, 2], dtype=torch.int64, device=DEV)
    dst = torch.full((2, 8), -7.0, device=DEV)
    good = ops.gather_field(src, dst)
    for fields in ([good, ops.gather_field(None, dst, row_elems=8)],     # NULL source
                   [good] * 17,                                           # n_fields = 17
                   []):
        with pytest.raises(MMFNLibraryError):
            ops.gather_batch(fields, idx, n)
    with pytest.raises(MMFNLibraryError):
        ops.gather_batch([ops.gather_field(src, dst, row_elems=-1)], idx, n)
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())
    ops.gather_batch([good], idx, n)
    assert torch.equal(dst, src[1:3])


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
    return _pack_store(tmp_path_factory.mktemp("resident"), fixtures.synthetic_samples(LANES, seed=5, radar_counts=(50, 100, 81, 3, 90)))


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


@pytest.mark.parametrize("variant", ["vec", "img", "rad"])
def test_every_batch_of_a_shuffled_epoch_equals_the_host_chain(packed, nets, variant):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    res = D.ResidentFrames(packed, DEV, cfg, variant, max_bytes=BUDGET)
    assert res.nbytes() == D.ResidentFrames.plan(packed, cfg, variant)["bytes"] and len(res) == 5
    loader = D.ResidentLoader(res, 2, shuffle=True, seed=3)
    for epoch in range(2):
        chunks = D._chunks(D._epoch_order(5, True, None, 3, epoch), 2, False)
        batches = list(D.DevicePrefetcher(loader, DEV, cfg, variant=variant))      # passed straight through
        assert len(batches) == len(loader) == 3 and [b[1].shape[0] for b in batches] == [2, 2, 1]
        for got, idx in zip(batches, chunks):
            _same_batch(got, _chain(nets[variant], packed, idx, cfg))
    assert D.DevicePrefetcher(loader, DEV, cfg, variant=variant).stream is None


def test_lane_bucket_pads_as_the_trainer_would(packed, nets):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd.trainer import _bucket_lanes
    cfg = GlobalConfig()
    res = D.ResidentFrames(packed, DEV, cfg, "vec", max_bytes=BUDGET)
    for bucket, lmax in ((16, [16, 16, 16]), (4, [12, 8, 4])):      # batches [0, 1], [2, 3], [4]: 9 / 7 / 1 lanes
        got = list(D.ResidentLoader(res, 2, lane_bucket=bucket))
        assert [g[0]["lane"].shape[1] for g in got] == lmax
        for (inp, gt), idx in zip(got, ([0, 1], [2, 3], [4])):
            winp, wgt = _chain(nets["vec"], packed, idx, cfg)
            _same_batch((inp, gt), (_bucket_lanes(winp, bucket), wgt))
            assert _bucket_lanes(inp, bucket) is inp                 # nothing left for the trainer to pad


def test_two_frames_per_sample_with_the_image_map_model(tmp_path):
    """seq_len = 2: frame s of sample b is batch entry 2 b + s of image / lidar / map, six waypoints of which the last four are gt."""
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd import model as M
    rng = np.random.RandomState(17)
    samples = []
    for n_lane in (4, 2, 6, 3):
        radar = [rng.randn(81, 5) for _ in range(2)]
        samples.append({
            "fronts": [torch.from_numpy(rng.randint(0, 256, (3, 256, 256)).astype(np.uint8)) for _ in range(2)],
            "lidars": [(rng.randint(0, 6, (2, 256, 256)) / 5.0).astype(np.float32) for _ in range(2)],
            "vectormaps": [torch.from_numpy(rng.randn(n_lane, 10, 5)) for _ in range(2)],
            "radar": radar,
            "maps": [torch.from_numpy(rng.randint(0, 256, (3, 256, 256)).astype(np.uint8)) for _ in range(2)],
            "waypoints": [tuple(rng.randn(2)) for _ in range(6)], "target_point": tuple(rng.randn(2) * 10.0),
            "steer": 0.1, "throttle": 0.5, "brake": False, "command": 2, "velocity": float(rng.uniform(0, 8))})
    packed = _pack_store(tmp_path, samples)
    cfg = GlobalConfig(seq_len=2)
    net = M.MMFN(cfg, DEV, "img")
    res = D.ResidentFrames(packed, DEV, cfg, "img", max_bytes=BUDGET)
    assert set(res.plan_["arrays"]) == {"fronts.0", "fronts.1", "lidars.0", "lidars.1", "maps.0", "maps.1"}
    loader = D.ResidentLoader(res, 3, shuffle=True, seed=1)
    chunks = D._chunks(D._epoch_order(4, True, None, 1, 0), 3, False)
    got = list(loader)
    assert [g[0]["image"].shape[0] for g in got] == [6, 2] and got[0][1].shape == (3, 4, 2)
    for g, idx in zip(got, chunks):
        _same_batch(g, _chain(net, packed, idx, cfg))
    with pytest.raises(NotImplementedError):
        D.ResidentFrames.plan(packed, cfg, "vec")


# ---------------------------------------------------------------------------------------------- 3. a training epoch
def test_epoch_from_resident_frames_equals_epoch_from_packed_frames(tmp_path):
    """Trainer.train over ResidentLoader == over PackedLoader: two epochs, dropout 0.1, graph replay - losses and every state_dict
    tensor bit-equal; one validate() over both loaders gives the same number."""
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    from mmfn_amd import model as M
    from mmfn_amd.optim import FusedAdamW
    from mmfn_amd.trainer import Trainer
    from oracle import fixtures, harness
    oracle = harness.build_oracle("vec", dropout=0.1)
    cfg = GlobalConfig()
    packed = _pack_store(tmp_path, fixtures.synthetic_samples((5, 9, 3, 7), seed=3, radar_counts=(50, 81, 81, 20)))
    loaders = (D.PackedLoader(packed, batch_size=2), D.ResidentLoader(D.ResidentFrames(packed, DEV, cfg, "vec", max_bytes=BUDGET), batch_size=2))
    out = []
    for loader in loaders:
        net = M.MMFN(cfg, DEV)
        net.load_state_dict(oracle.state_dict(), strict=True)
        tr = Trainer(DEV, None)
        opt = FusedAdamW(net, lr=1e-4)
        tr.train(net, loader, cfg, opt)
        tr.train(net, loader, cfg, opt)
        assert not any(isinstance(s, str) and s == "eager" for s in tr._static_steps.values())    # replayed, not fallen back
        val = [tr.validate(net, ld, cfg) for ld in loaders]
        assert val[0] == val[1]
        out.append((tr.train_loss, net.state_dict(), val[0]))
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2]
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k


# ---------------------------------------------------------------------------------------------- 4. capture
def test_a_captured_gather_follows_the_index_buffer(packed):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    res = D.ResidentFrames(packed, DEV, cfg, "rad", max_bytes=BUDGET)
    index = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    rows = np.array([0, 1])
    first = res.gather(index.clone(), rows, lane_bucket=16)       # eager (also loads the library outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # one launch on the capture stream: no branches
        inp, gt = res.gather(index, rows, lane_bucket=16)          # 16 lanes hold every sample's set, whatever the indices
    graph.replay()
    _same_batch((inp, gt), first)
    index.copy_(torch.tensor([3, 2], dtype=torch.int64, device=DEV))
    graph.replay()
    want = res.gather(torch.tensor([3, 2], dtype=torch.int64, device=DEV), np.array([3, 2]), lane_bucket=16)
    _same_batch((inp, gt), want)
    assert inp["lane_num"].tolist() == [7, 3]
    assert not torch.equal(inp["image"], first[0]["image"])


# ---------------------------------------------------------------------------------------------- 5. a rank's shard
def test_a_shard_serves_its_global_sample_ids_only(packed, nets):
    from mmfn_amd import data as D
    from mmfn_amd.config import GlobalConfig
    cfg = GlobalConfig()
    res = D.ResidentFrames(packed, DEV, cfg, "vec", indices=[4, 0, 2])      # default budget: free memory less the reserve
    assert len(res) == 3 and res.nbytes() == D.ResidentFrames.plan(packed, cfg, "vec", indices=[4, 0, 2])["bytes"]
    sampler = [2, 4, 0, 4, 2]                                               # global ids, in the sampler's order
    got = list(D.ResidentLoader(res, 2, sampler=sampler))
    assert len(got) == 3
    for g, idx in zip(got, ([2, 4], [0, 4], [2])):
        _same_batch(g, _chain(nets["vec"], packed, idx, cfg))
    # without a sampler the order runs over the shard's rows: row r is sample indices[r]
    for g, idx in zip(D.ResidentLoader(res, 2), ([4, 0], [2])):
        _same_batch(g, _chain(nets["vec"], packed, idx, cfg))
    with pytest.raises(IndexError):
        list(D.ResidentLoader(res, 2, sampler=[2, 1]))
    with pytest.raises(IndexError):
        list(D.ResidentLoader(res, 2, sampler=[5]))
