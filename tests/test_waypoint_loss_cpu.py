"""losses.WaypointLoss on the CPU: its reference expression against torch's own loss functions in float64, and its validation."""
import math

import pytest
import torch
import torch.nn.functional as F

CASES = [("l1", {}), ("smooth_l1", {"beta": 2.0}), ("smooth_l1", {"beta": 0.0}), ("smooth_l1", {"beta": 0.3}),
         ("huber", {"delta": 2.0}), ("huber", {"delta": 0.4}), ("mse", {})]


def _torch_terms(kind, kw, pred, gt):
    if kind == "l1":
        return F.l1_loss(pred, gt, reduction="none")
    if kind == "smooth_l1":
        return F.smooth_l1_loss(pred, gt, reduction="none", beta=kw["beta"])
    if kind == "huber":
        return F.huber_loss(pred, gt, reduction="none", delta=kw["delta"])
    return F.mse_loss(pred, gt, reduction="none")


@pytest.mark.parametrize("kind,kw", CASES)
@pytest.mark.parametrize("weights", ["both", "horizon", "sample", "neither"])
def test_reference_is_torchs_loss_times_the_broadcast_weights(kind, kw, weights):
    from mmfn_amd.losses import WaypointLoss
    g = torch.Generator().manual_seed(7)
    B, S = 5, 4
    pred = torch.randn(B, S, 2, generator=g, dtype=torch.float64) * 2
    gt = torch.randn(B, S, 2, generator=g, dtype=torch.float64) * 2
    hw = (torch.rand(S, generator=g, dtype=torch.float64) * 1.75 + 0.25) if weights in ("both", "horizon") else None
    sw = (torch.rand(B, generator=g, dtype=torch.float64) * 3) if weights in ("both", "sample") else None
    loss = WaypointLoss(kind, step_weights=None if hw is None else hw.tolist(), **kw)
    want = _torch_terms(kind, kw, pred, gt)
    if hw is not None:
        want = want * hw[None, :, None]
    if sw is not None:
        want = want * sw[:, None, None]
    got = loss.reference(pred, gt, sw)
    assert got.dtype == torch.float64 and got.dim() == 0
    assert abs(got.item() - want.mean().item()) <= 1e-12
    # the closed forms of the table in include/mmfn_hip.h (what the kernels restate)
    e = pred - gt
    a = e.abs()
    if kind == "l1" or (kind == "smooth_l1" and kw["beta"] == 0):
        rho = a
    elif kind == "smooth_l1":
        rho = torch.where(a < kw["beta"], 0.5 * e * e / kw["beta"], a - 0.5 * kw["beta"])
    elif kind == "huber":
        rho = torch.where(a <= kw["delta"], 0.5 * e * e, kw["delta"] * (a - 0.5 * kw["delta"]))
    else:
        rho = e * e
    assert (loss.terms(pred, gt) - rho).abs().max().item() <= 1e-12


def test_reference_follows_the_dtype_of_its_arguments_and_is_differentiable():
    from mmfn_amd.losses import WaypointLoss
    loss = WaypointLoss("huber", delta=0.5, step_weights=(2, 1, 0.5, 0.25))
    pred = torch.randn(3, 4, 2, requires_grad=True)
    gt = torch.randn(3, 4, 2)
    out = loss.reference(pred, gt, torch.tensor([1.0, 0.0, 2.0]))
    assert out.dtype == torch.float32
    out.backward()
    assert pred.grad is not None and not pred.grad[1].any() and pred.grad[0].any()


def test_plain_means_l1_without_step_weights():
    from mmfn_amd.losses import WaypointLoss
    assert WaypointLoss().is_plain() and WaypointLoss("l1", beta=3.0, delta=2.0).is_plain()
    assert not WaypointLoss("l1", step_weights=(1, 1, 1, 1)).is_plain()
    assert not WaypointLoss("smooth_l1", beta=0.0).is_plain()
    assert not WaypointLoss("mse").is_plain() and not WaypointLoss("huber").is_plain()


def test_table_layout():
    from mmfn_amd.losses import WaypointLoss
    tab = WaypointLoss("smooth_l1", beta=0.75, delta=9.0, step_weights=(2, 1, 0.5, 0.25)).table(4)
    assert len(tab) == 16 and tab[0] == 0.75 and tab[8:12] == [2.0, 1.0, 0.5, 0.25] and tab[12:] == [1.0] * 4
    assert WaypointLoss("huber", beta=0.75, delta=9.0).table(4)[0] == 9.0
    assert WaypointLoss("mse").table(8)[8:] == [1.0] * 8


def test_validation_errors():
    from mmfn_amd.losses import WaypointLoss
    with pytest.raises(ValueError, match="does not support negative values for beta"):
        WaypointLoss("smooth_l1", beta=-0.1)
    with pytest.raises(ValueError, match="negative values for beta"):
        WaypointLoss("l1", beta=float("nan"))
    with pytest.raises(ValueError, match="non-positive values for delta"):
        WaypointLoss("huber", delta=0.0)
    with pytest.raises(ValueError, match="loss kind must be one of l1 / smooth_l1 / huber / mse"):
        WaypointLoss("l2")
    with pytest.raises(ValueError, match="step_weights must be finite"):
        WaypointLoss("l1", step_weights=(1.0, math.inf, 1.0, 1.0))
    with pytest.raises(ValueError, match="one weight per predicted waypoint"):
        WaypointLoss("l1", step_weights=())
    with pytest.raises(ValueError, match="one weight per predicted waypoint"):
        WaypointLoss("l1", step_weights=(1.0,) * 9)
    loss = WaypointLoss("mse", step_weights=(1, 2, 3))
    with pytest.raises(ValueError, match=r"holds 3 weight\(s\), the model predicts 4 waypoints"):
        loss.check_steps(4)
    with pytest.raises(ValueError, match=r"holds 3 weight\(s\)"):
        loss.reference(torch.zeros(2, 4, 2), torch.zeros(2, 4, 2))
    assert WaypointLoss("smooth_l1", beta=0.0).beta == 0.0   # torch's definition: L1


def test_header_declares_the_loss_entry_points_and_kind_codes():
    import re
    from mmfn_amd import _lib, losses
    for name, n_args in (("mmfn_gru_head_fwd_loss_f32", 22), ("mmfn_gru_head_bwd_loss_f32", 17)):
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name][1]) == n_args
    text = open(_lib.HEADER_PATH).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define MMFN_LOSS_(L1|SMOOTH_L1|HUBER|MSE) (\d+)", text)}
    assert codes == losses.KIND_CODES
    assert "#define MMFN_LOSS_TABLE_FLOATS %d" % losses.TABLE_FLOATS in text
    assert "#define MMFN_LOSS_TABLE_HORIZON %d" % losses.TABLE_HORIZON in text
