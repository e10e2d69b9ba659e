"""Waypoint objectives of the fused training step (Engine.set_loss, Trainer.train(loss=...)).

The reference trains on `F.l1_loss(pred, gt, reduction="none").mean()` (run_steps/phase2_train_net.py:104), and that is the fused
step's default.  A WaypointLoss replaces the per-element term - L1, smooth-L1(beta), Huber(delta) or MSE, torch's definitions - and
may weight the prediction horizon; a batch may carry per-sample weights beside it (inp["sample_weight"]).  The objective is

    (sample_weight[:, None, None] * step_weights[None, :, None] * rho(pred - gt)).mean()

with no normalisation by the weights: a user who wants a weighted mean normalises the weights.  `reference` is that expression
in torch - what the tests compare the kernels with and what the autograd path (Trainer.train(fused=False)) calls; the fused step
forms it inside the head launches (csrc/head.hip: mmfn_gru_head_fwd_loss_f32 / mmfn_gru_head_bwd_loss_f32).
"""
import math

import torch
import torch.nn.functional as F

KINDS = ("l1", "smooth_l1", "huber", "mse")
# MMFN_LOSS_* of include/mmfn_hip.h
KIND_CODES = {"l1": 0, "smooth_l1": 1, "huber": 2, "mse": 3}
TABLE_FLOATS = 16    # MMFN_LOSS_TABLE_FLOATS: [0] = beta or delta, [8 + t] = the horizon weight of GRU step t
TABLE_HORIZON = 8    # MMFN_LOSS_TABLE_HORIZON
MAX_STEPS = TABLE_FLOATS - TABLE_HORIZON


class WaypointLoss(object):
    """kind: "l1" | "smooth_l1" | "huber" | "mse".  beta: smooth-L1's threshold (>= 0; 0 is L1, as torch defines it); delta: Huber's
    (> 0).  step_weights: one finite weight per predicted waypoint (None: all 1); the length is checked against the model's pred_len
    when the loss is set (Engine.set_loss)."""

    def __init__(self, kind="l1", beta=1.0, delta=1.0, step_weights=None):
        if kind not in KINDS:
            raise ValueError("loss kind must be one of %s, got %r" % (" / ".join(KINDS), kind))
        beta, delta = float(beta), float(delta)
        if not beta >= 0.0 or math.isinf(beta):
            raise ValueError("smooth_l1_loss does not support negative values for beta (got %r)" % (beta,))
        if not delta > 0.0 or math.isinf(delta):
            raise ValueError("huber_loss does not support non-positive values for delta (got %r)" % (delta,))
        if step_weights is not None:
            step_weights = tuple(float(w) for w in step_weights)
            if not step_weights or len(step_weights) > MAX_STEPS:
                raise ValueError("step_weights holds one weight per predicted waypoint (1 to %d), got %d" % (MAX_STEPS, len(step_weights)))
            if not all(math.isfinite(w) for w in step_weights):
                raise ValueError("step_weights must be finite, got %r" % (step_weights,))
        self.kind, self.beta, self.delta, self.step_weights = kind, beta, delta, step_weights

    def __repr__(self):
        return "WaypointLoss(kind=%r, beta=%r, delta=%r, step_weights=%r)" % (self.kind, self.beta, self.delta, self.step_weights)

    @property
    def kind_code(self):
        return KIND_CODES[self.kind]

    def is_plain(self):
        """L1 without step weights: the reference's loss, which the fused step forms in its original launches."""
        return self.kind == "l1" and self.step_weights is None

    def check_steps(self, pred_len):
        if self.step_weights is not None and len(self.step_weights) != int(pred_len):
            raise ValueError("step_weights holds %d weight(s), the model predicts %d waypoints (pred_len)" % (
                len(self.step_weights), int(pred_len)))

    def table(self, pred_len):
        """The 16 floats the head launches read from device memory."""
        self.check_steps(pred_len)
        if int(pred_len) > MAX_STEPS:
            raise ValueError("at most %d predicted waypoints, got %d" % (MAX_STEPS, int(pred_len)))
        tab = [0.0] * TABLE_FLOATS
        tab[0] = self.beta if self.kind == "smooth_l1" else (self.delta if self.kind == "huber" else 0.0)
        hw = self.step_weights if self.step_weights is not None else (1.0,) * int(pred_len)
        for t in range(TABLE_HORIZON, TABLE_FLOATS):
            tab[t] = 1.0
        tab[TABLE_HORIZON:TABLE_HORIZON + len(hw)] = hw
        return tab

    def terms(self, pred, gt):
        """rho(pred - gt) per element, torch's own functions."""
        if self.kind == "l1":
            return F.l1_loss(pred, gt, reduction="none")
        if self.kind == "smooth_l1":
            return F.smooth_l1_loss(pred, gt, reduction="none", beta=self.beta)
        if self.kind == "huber":
            return F.huber_loss(pred, gt, reduction="none", delta=self.delta)
        return F.mse_loss(pred, gt, reduction="none")

    def reference(self, pred, gt, sample_weight=None):
        """(sample_weight[:, None, None] * step_weights[None, :, None] * rho(pred - gt)).mean() in the dtype of pred / gt.
        pred, gt: [B, pred_len, 2]; sample_weight: [B] or None."""
        term = self.terms(pred, gt)
        if self.step_weights is not None:
            self.check_steps(term.shape[1])
            term = torch.tensor(self.step_weights, dtype=term.dtype, device=term.device)[None, :, None] * term
        if sample_weight is not None:
            term = sample_weight.to(term.dtype)[:, None, None] * term
        return term.mean()


PLAIN = WaypointLoss("l1")
