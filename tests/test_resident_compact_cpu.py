"""Host side of the compact device-resident store: the 4-bit palette encoder (data.palette_encode / palette_decode) and what
ResidentFrames.plan(..., compact=True) counts.  No GPU needed."""
import numpy as np
import pytest
import torch

from mmfn_amd import data as D
from mmfn_amd.config import GlobalConfig
from oracle import fixtures

LANES = (5, 9, 3, 7, 1)
IMG = 3 * 256 * 256          # u8 camera frame / raster map
BEV = 2 * 256 * 256          # elements of the LiDAR histogram: 4 bytes each as f32, half a byte each as codes


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).reshape(len(x), -1).view(np.uint32)


def _field(values, n, row, seed):
    """f32 [n, row] drawn from `values` (f32 bit patterns kept as given), every value present."""
    values = np.asarray(values, dtype=np.float32)
    rng = np.random.RandomState(seed)
    pick = rng.randint(0, len(values), n * row)
    pick[:len(values)] = np.arange(len(values))
    return values[pick].reshape(n, row)


NAN_A, NAN_B = np.array([0x7fc00000, 0x7fc00001], dtype=np.uint32).view(np.float32)
SETS = {"six": np.arange(6, dtype=np.float32) / np.float32(5.0),
        "sixteen": np.linspace(-3.0, 4.5, 16).astype(np.float32),
        "zeros_and_nans": np.array([0.0, -0.0, NAN_A, NAN_B, 1.5], dtype=np.float32)}


@pytest.mark.parametrize("name", sorted(SETS))
def test_decode_of_encode_is_the_input_bit_for_bit(name):
    x = _field(SETS[name], 7, 26, seed=len(name))
    codes, palette, count = D.palette_encode(x)
    assert codes.dtype == np.uint8 and codes.shape == (7, 13)
    assert palette.dtype == np.float32 and palette.shape == (16,) and count == len(SETS[name])
    back = D.palette_decode(codes, palette)
    assert back.dtype == np.float32 and back.shape == x.shape
    assert np.array_equal(_bits(back), _bits(x))       # as uint32: -0.0 stays -0.0, each NaN keeps its payload


def test_a_float64_field_is_coded_as_its_float32_rounding():
    x = _field(SETS["six"], 4, 10, seed=2).astype(np.float64) + 1e-12       # not representable in f32: rounds back
    x64 = D.palette_encode(x)
    x32 = D.palette_encode(x.astype(np.float32))
    assert x64[2] == x32[2] == 6
    assert np.array_equal(x64[0], x32[0]) and np.array_equal(_bits(x64[1][None]), _bits(x32[1][None]))
    assert np.array_equal(_bits(D.palette_decode(*x64[:2])), _bits(x.astype(np.float32)))


def test_a_field_with_more_values_an_odd_row_or_another_dtype_is_not_coded():
    assert D.palette_encode(_field(np.arange(17, dtype=np.float32), 3, 20, seed=1)) is None
    assert D.palette_encode(_field(SETS["six"], 3, 13, seed=1)) is None
    assert D.palette_encode(np.zeros((3, 8), dtype=np.uint8)) is None
    # +0.0 and -0.0 count twice: 15 values and both zeros are 17 patterns
    both = np.concatenate([np.arange(1, 16, dtype=np.float32), np.array([0.0, -0.0], dtype=np.float32)])
    assert D.palette_encode(_field(both, 2, 20, seed=3)) is None
    assert D.palette_encode(_field(both[:-1], 2, 20, seed=3))[2] == 16


def test_nibble_order_and_palette_order():
    """Element 2j is the low nibble of byte j; the palette is the patterns in ascending uint32 order (so the negative values, sign
    bit set, come last), unused slots +0.0."""
    x = np.array([[2.0, -1.0, 0.5, 0.5], [-1.0, -0.0, 2.0, 0.5]], dtype=np.float32)
    codes, palette, count = D.palette_encode(x)
    order = np.array([0.5, 2.0, -0.0, -1.0], dtype=np.float32)               # 0x3f000000 < 0x40000000 < 0x80000000 < 0xbf800000
    assert count == 4 and np.array_equal(_bits(palette[None])[0, :4], _bits(order[None])[0])
    assert not _bits(palette[None])[0, 4:].any()
    assert codes.tolist() == [[1 | 3 << 4, 0 | 0 << 4], [3 | 2 << 4, 1 | 0 << 4]]


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    samples = fixtures.synthetic_samples(lane_counts=LANES, seed=5, radar_counts=(50, 100, 81, 3, 90))
    for s in samples:
        s["radar_adj"] = D.radar_adjacency(s["radar"][0])
    return D.PackedFrames(D.pack_frames(samples, str(tmp_path_factory.mktemp("compact") / "packed")))


@pytest.mark.parametrize("variant", ["vec", "img", "rad"])
def test_compact_plan_counts_the_lidar_codes_and_their_palette(packed, variant, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("plan() touched the device")
    for name in ("is_available", "mem_get_info", "_lazy_init", "current_device", "device_count"):
        monkeypatch.setattr(torch.cuda, name, no_device)
    cfg, n = GlobalConfig(), 5
    plain = D.ResidentFrames.plan(packed, cfg, variant)
    plan = D.ResidentFrames.plan(packed, cfg, variant, compact=True)
    assert plan["compact"] == ["lidars.0"]              # radar rows (405, 6561 elements) are odd, lanes ragged, the rest u8
    assert plan["fields"]["lidars.0"] == n * 65536 == n * BEV // 2 and plan["fields"]["lidars.0.palette"] == 64
    want = dict(plain["fields"], **{"lidars.0": n * 65536, "lidars.0.palette": 64})
    assert plan["fields"] == want and plan["fields"]["fronts.0"] == n * IMG
    assert plan["bytes"] == sum(plan["fields"].values()) == plain["bytes"] - n * (BEV * 4 - BEV // 2) + 64
    assert plan["arrays"] == plain["arrays"] and plan["rows"].tolist() == plain["rows"].tolist()


def test_plan_without_the_argument_is_the_plain_plan(packed):
    cfg = GlobalConfig()
    a, b = D.ResidentFrames.plan(packed, cfg, "vec"), D.ResidentFrames.plan(packed, cfg, "vec", compact=False)
    assert sorted(a) == sorted(b) == ["arrays", "bytes", "compact", "fields", "rows"]
    assert a["compact"] == b["compact"] == []
    assert a["fields"] == b["fields"] and a["bytes"] == b["bytes"] == 3609748 and a["arrays"] == b["arrays"]
    assert a["rows"].tolist() == b["rows"].tolist() == [0, 1, 2, 3, 4]
    assert a["fields"]["lidars.0"] == 5 * BEV * 4 and "lidars.0.palette" not in a["fields"]


def test_values_are_counted_over_the_kept_rows_only(packed, tmp_path):
    """A 17th LiDAR value in sample 2 keeps the whole field f32 - unless the shard leaves sample 2 out."""
    samples = fixtures.synthetic_samples(lane_counts=LANES[:3], seed=5)
    for s in samples:
        s["radar_adj"] = D.radar_adjacency(s["radar"][0])
    extra = np.arange(6, 17, dtype=np.float32)          # 11 more values: 17 in all
    samples[2]["lidars"][0].reshape(-1)[:11] = extra
    store = D.PackedFrames(D.pack_frames(samples, str(tmp_path / "packed")))
    cfg = GlobalConfig()
    full = D.ResidentFrames.plan(store, cfg, "vec", compact=True)
    assert full["compact"] == [] and full["fields"] == D.ResidentFrames.plan(store, cfg, "vec")["fields"]
    part = D.ResidentFrames.plan(store, cfg, "vec", indices=[1, 0], compact=True)
    assert part["compact"] == ["lidars.0"] and part["fields"]["lidars.0"] == 2 * 65536


def test_the_capacity_error_names_compact_only_when_it_was_not_asked_for(packed):
    cfg = GlobalConfig()
    with pytest.raises(ValueError) as exc:
        D.ResidentFrames(packed, "cuda:0", cfg, "vec", max_bytes=1)
    assert "compact=True" in str(exc.value)
    with pytest.raises(ValueError) as exc:
        D.ResidentFrames(packed, "cuda:0", cfg, "vec", max_bytes=1, compact=True)
    assert "compact=True" not in str(exc.value) and str(D.ResidentFrames.plan(packed, cfg, "vec", compact=True)["bytes"]) in str(exc.value)
