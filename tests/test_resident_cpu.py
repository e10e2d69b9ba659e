"""Host side of the device-resident dataset (data.ResidentFrames.plan, ResidentLoader's epoch order): no GPU needed."""
import numpy as np
import pytest
import torch

from mmfn_amd import data as D
from mmfn_amd.config import GlobalConfig
from oracle import fixtures

LANES = (5, 9, 3, 7, 1)
IMG = 3 * 256 * 256          # u8 camera frame / raster map
BEV = 2 * 256 * 256 * 4      # f32 LiDAR histogram
LANE_ROW = 10 * 5 * 4        # one lane, rounded to f32
RADAR, RADAR_ADJ = 81 * 5 * 4, 81 * 81 * 4
LABELS = 2 * 4 + 4 + 4 * 2 * 4   # target point, velocity, pred_len = 4 waypoints


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    samples = fixtures.synthetic_samples(lane_counts=LANES, seed=5, radar_counts=(50, 100, 81, 3, 90))
    for s in samples:
        s["radar_adj"] = D.radar_adjacency(s["radar"][0])
    return D.PackedFrames(D.pack_frames(samples, str(tmp_path_factory.mktemp("resident") / "packed")))


@pytest.mark.parametrize("variant", ["vec", "img", "rad"])
def test_plan_keeps_the_engine_inputs_and_counts_their_bytes(packed, variant):
    cfg = GlobalConfig()
    plan = D.ResidentFrames.plan(packed, cfg, variant)
    n, lanes = 5, sum(LANES)
    want = {"fronts.0": n * IMG, "lidars.0": n * BEV, "target_point": n * 8, "velocity": n * 4, "waypoints": n * 32}
    if variant == "img":
        want["maps.0"] = n * IMG
    else:
        want.update({"vectormaps.0": lanes * LANE_ROW, "vectormaps.0.row_off": (n + 1) * 8})
    if variant == "rad":
        want.update({"radar.0": n * RADAR, "radar_adj": n * RADAR_ADJ})
    assert plan["fields"] == want                       # nothing else: no steer / throttle / brake / command, one map form
    assert plan["bytes"] == sum(want.values())
    assert plan["bytes"] == {"vec": 3609748, "img": 4587740, "rad": 3749068}[variant]
    assert plan["rows"].tolist() == [0, 1, 2, 3, 4]


def test_plan_of_a_shard_changes_only_the_counts(packed):
    cfg = GlobalConfig()
    full, part = D.ResidentFrames.plan(packed, cfg, "rad"), D.ResidentFrames.plan(packed, cfg, "rad", indices=[4, 0, 2])
    assert list(part["fields"]) == list(full["fields"]) and part["arrays"] == full["arrays"]
    lanes = LANES[4] + LANES[0] + LANES[2]
    assert part["bytes"] == 3 * (IMG + BEV + RADAR + RADAR_ADJ + LABELS) + lanes * LANE_ROW + 4 * 8
    assert part["rows"].tolist() == [4, 0, 2]
    with pytest.raises(IndexError):
        D.ResidentFrames.plan(packed, cfg, "vec", indices=[5])
    with pytest.raises(ValueError):
        D.ResidentFrames.plan(packed, cfg, "lidar")


def test_a_plan_over_the_budget_is_refused_before_any_allocation(packed, monkeypatch):
    def no_alloc(*a, **k):
        raise AssertionError("allocated before the budget check")
    monkeypatch.setattr(torch, "empty", no_alloc)
    with pytest.raises(ValueError) as exc:
        D.ResidentFrames(packed, "cuda:0", GlobalConfig(), "vec", max_bytes=1)
    assert "3609748" in str(exc.value) and " 1 " in str(exc.value)     # needed and available bytes


class _Rows(object):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [False, True])
def test_resident_loader_orders_an_epoch_as_packed_loader_does(packed, shuffle, drop_last):
    a = D.PackedLoader(packed, 2, shuffle=shuffle, seed=3, drop_last=drop_last, pin_memory=False)
    b = D.ResidentLoader(_Rows(5), 2, shuffle=shuffle, seed=3, drop_last=drop_last)
    assert len(a) == len(b) == (2 if drop_last else 3)
    for epoch in (0, 1, 7):
        a.epoch = b.epoch = epoch
        assert a._order() == b._order()
        chunks = D._chunks(b._order(), 2, drop_last)
        assert len(chunks) == len(b) and [len(c) for c in chunks] == [2, 2, 1][:len(b)]
    if shuffle:
        a.epoch, b.epoch = 0, 1
        assert a._order() != b._order() and sorted(a._order()) == sorted(b._order()) == list(range(5))


def test_resident_loader_takes_a_sampler_and_exposes_what_fit_uses(packed):
    sampler = D.shard_sampler(packed, rank=1, world=2, shuffle=True, seed=4)
    a, b = D.PackedLoader(packed, 2, sampler=sampler, pin_memory=False), D.ResidentLoader(_Rows(5), 2, sampler=sampler)
    for epoch in (0, 1):
        sampler.set_epoch(epoch)
        assert a._order() == b._order() == [int(i) for i in sampler]
    assert len(a) == len(b) == 2 and b.sampler is sampler and b.epoch == 0 and b.device_resident is True
    assert len(D.ResidentLoader(_Rows(5), 2, sampler=sampler, drop_last=True)) == len(D.PackedLoader(packed, 2, sampler=sampler, drop_last=True)) == 1
