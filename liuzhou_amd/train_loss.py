"""Fused policy + bucketed-value training loss on the HIP library.

`fused_policy_value_loss(...)` is the drop-in for the loss assembly of `v1/python/train_bridge.py:330-375`
(`build_combined_logits` -> `masked_log_softmax` -> `batched_policy_loss`, two-hot bucket cross entropy): one kernel
computes the per-sample terms and the gradients with respect to the four head outputs; autograd only multiplies
them by the incoming scalar gradient (which carries the AMP loss scale).  No CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import _lib as L


def _forward(ctx, lp1, lp2, lpm, vlogits, legal_mask, policy_target, value_target, soft_target, alpha, anti_draw,
             draw_weight, row_weights=None, dist=None):
    """The forward of the three autograd functions; `row_weights` None: the unweighted entry point; `dist` = (value_dist
    float32 [D,101], value_dist_row int32 [B]): the distributional entry point, weighted or not."""
    dev = lp1.device
    if dev.type != "cuda":
        L.require_hip(lp1, "fused_policy_value_loss")
    B = int(lp1.shape[0])
    f32 = lambda t: t.detach().reshape(B, -1).to(torch.float32).contiguous()
    a1, a2, a3, av = f32(lp1), f32(lp2), f32(lpm), f32(vlogits)
    mask = legal_mask.reshape(B, -1).contiguous()
    mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)
    tgt = policy_target.reshape(B, -1).to(torch.float32).contiguous()
    val = value_target.reshape(B).to(torch.float32).contiguous()
    soft = soft_target.reshape(B).to(torch.float32).contiguous()
    if a1.shape[1] != 36 or av.shape[1] != 101 or mask.shape[1] != 220 or tgt.shape[1] != 220:
        raise RuntimeError("fused loss expects 6x6 heads [B,36], 101 value bins and 220 actions")
    wsum = torch.where(val.abs() < 1e-8, float(draw_weight), 1.0).to(torch.float32).sum().reshape(1)
    terms = torch.empty((B, 4), dtype=torch.float32, device=dev)
    g1, g2, g3 = (torch.empty((B, 36), dtype=torch.float32, device=dev) for _ in range(3))
    gv = torch.empty((B, 101), dtype=torch.float32, device=dev)
    tail = (L.i64(B), C.c_float(float(alpha)), C.c_float(float(anti_draw)), C.c_float(float(draw_weight)),
            L.ptr(wsum), C.c_float(1.0), L.ptr(terms), L.ptr(g1), L.ptr(g2), L.ptr(g3), L.ptr(gv), L.stream_ptr(dev))
    with torch.cuda.device(dev):
        if dist is not None:
            rw = None if row_weights is None else row_weights.contiguous()
            table, rows = dist[0].contiguous(), dist[1].contiguous()
            L.check(L.lib().lz_policy_value_loss_dist_fwd_bwd(
                L.ptr(a1), L.ptr(a2), L.ptr(a3), L.ptr(av), L.ptr(mask), L.ptr(tgt), L.ptr(val), L.ptr(soft),
                L.ptr(rw), *tail, L.ptr(rows), L.ptr(table), L.i64(int(table.shape[0]))),
                "policy_value_loss_dist_fwd_bwd")
        elif row_weights is None:
            L.check(L.lib().lz_policy_value_loss_fwd_bwd(
                L.ptr(a1), L.ptr(a2), L.ptr(a3), L.ptr(av), L.ptr(mask), L.ptr(tgt), L.ptr(val), L.ptr(soft), *tail),
                "policy_value_loss_fwd_bwd")
        else:
            rw = row_weights.contiguous()
            L.check(L.lib().lz_policy_value_loss_weighted_fwd_bwd(
                L.ptr(a1), L.ptr(a2), L.ptr(a3), L.ptr(av), L.ptr(mask), L.ptr(tgt), L.ptr(val), L.ptr(soft),
                L.ptr(rw), *tail), "policy_value_loss_weighted_fwd_bwd")
    policy_loss = (terms[:, 0] * terms[:, 1]).sum() / (wsum[0] + 1e-8)     # terms[:, 1] = draw weight * row weight
    if row_weights is None:
        bucket_loss = terms[:, 2].mean()
        wdl_aux = terms[:, 3].mean()
    else:
        bucket_loss = (terms[:, 2] * rw).sum() / B
        wdl_aux = (terms[:, 3] * rw).sum() / B
    ctx.save_for_backward(g1, g2, g3, gv)
    ctx.shapes = (lp1.shape, lp2.shape, lpm.shape, vlogits.shape)
    ctx.dtypes = (lp1.dtype, lp2.dtype, lpm.dtype, vlogits.dtype)
    ctx.mark_non_differentiable(policy_loss, bucket_loss, wdl_aux)
    return policy_loss + bucket_loss, policy_loss, bucket_loss, wdl_aux


def _backward(ctx, grad_loss):
    g1, g2, g3, gv = ctx.saved_tensors
    outs = []
    for g, shape, dt in zip((g1, g2, g3, gv), ctx.shapes, ctx.dtypes):
        outs.append((g * grad_loss).to(dt).reshape(shape))
    return outs


class _FusedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp1, lp2, lpm, vlogits, legal_mask, policy_target, value_target, soft_target, alpha, anti_draw,
                draw_weight):
        return _forward(ctx, lp1, lp2, lpm, vlogits, legal_mask, policy_target, value_target, soft_target, alpha,
                        anti_draw, draw_weight)

    @staticmethod
    def backward(ctx, grad_loss, _gp, _gb, _ga):
        return (*_backward(ctx, grad_loss), None, None, None, None, None, None, None)


class _FusedLossWeighted(torch.autograd.Function):
    """`_FusedLoss` through the weighted instantiation of the kernel (`row_weights` float32 [B], no gradient)."""

    @staticmethod
    def forward(ctx, lp1, lp2, lpm, vlogits, legal_mask, policy_target, value_target, soft_target, row_weights, alpha,
                anti_draw, draw_weight):
        return _forward(ctx, lp1, lp2, lpm, vlogits, legal_mask, policy_target, value_target, soft_target, alpha,
                        anti_draw, draw_weight, row_weights)

    @staticmethod
    def backward(ctx, grad_loss, _gp, _gb, _ga):
        return (*_backward(ctx, grad_loss), None, None, None, None, None, None, None, None)


class _FusedLossDist(torch.autograd.Function):
    """`_FusedLoss` / `_FusedLossWeighted` through the distributional instantiations of the kernel: `value_dist` float32
    [D,101] and `value_dist_row` int32 [B] (no gradient); `row_weights` may be None."""

    @staticmethod
    def forward(ctx, lp1, lp2, lpm, vlogits, legal_mask, policy_target, value_target, soft_target, row_weights, value_dist,
                value_dist_row, alpha, anti_draw, draw_weight):
        return _forward(ctx, lp1, lp2, lpm, vlogits, legal_mask, policy_target, value_target, soft_target, alpha,
                        anti_draw, draw_weight, row_weights, (value_dist, value_dist_row))

    @staticmethod
    def backward(ctx, grad_loss, _gp, _gb, _ga):
        return (*_backward(ctx, grad_loss), None, None, None, None, None, None, None, None, None, None)


def _check_value_dist(value_dist, value_dist_row, B: int, device, anti_draw_penalty: float) -> None:
    if value_dist is None or value_dist_row is None:
        raise ValueError("value_dist and value_dist_row must be given together")
    if not isinstance(value_dist, torch.Tensor) or value_dist.dtype != torch.float32:
        raise TypeError("value_dist must be a float32 tensor")
    if not isinstance(value_dist_row, torch.Tensor) or value_dist_row.dtype != torch.int32:
        raise TypeError("value_dist_row must be an int32 tensor")
    if value_dist.dim() != 2 or int(value_dist.shape[1]) != 101:
        raise ValueError(f"value_dist must have shape [D,101], got {tuple(value_dist.shape)}")
    if tuple(value_dist_row.shape) != (B,):
        raise ValueError(f"value_dist_row must have shape [{B}], got {tuple(value_dist_row.shape)}")
    if value_dist.device != device or value_dist_row.device != device:
        raise ValueError(f"value_dist and value_dist_row must live on {device}")
    if abs(float(anti_draw_penalty)) > 1e-9:
        raise ValueError(f"value_dist cannot be combined with anti_draw_penalty={anti_draw_penalty!r}: the table was built "
                         "from the members' own values, without the penalty")


def fused_policy_value_loss(log_p1: torch.Tensor, log_p2: torch.Tensor, log_pmc: torch.Tensor,
                            value_logits: torch.Tensor, legal_mask: torch.Tensor, policy_target: torch.Tensor,
                            value_target: torch.Tensor, soft_value_target: torch.Tensor, *,
                            soft_label_alpha: float = 0.0, anti_draw_penalty: float = 0.0,
                            policy_draw_weight: float = 1.0, row_weights: Optional[torch.Tensor] = None,
                            value_dist: Optional[torch.Tensor] = None, value_dist_row: Optional[torch.Tensor] = None
                            ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """loss = weighted policy KL + mean two-hot bucket cross entropy; parts = policy_loss, bucket_value_loss,
    wdl_aux_loss (reported only: its weight is 0 in the reference, train_bridge.py:25).

    `row_weights` (float32 [B] on the heads' device; finite, >= 0, checked by the trainers -- nothing is read back
    here) multiplies every row as an absolute factor: policy_loss = sum(kl * draw weight * rw) /
    (sum(draw weight) + 1e-8), bucket_value_loss = sum(ce * rw) / B, wdl_aux_loss = sum(aux * rw) / B.  None: the
    unweighted kernel.

    `value_dist` (float32 [D,101]) and `value_dist_row` (int32 [B]), both or neither: a row b
    with 0 <= value_dist_row[b] < D is trained against row value_dist_row[b] of the table -- the mean of the two-hot
    distributions of the rows it was merged from -- in place of the two-hot of its value; every other row is untouched.
    Refused with a non-zero `anti_draw_penalty`.  None: the kernels without a table."""
    L.require_hip(log_p1, "fused_policy_value_loss")
    alpha = float(max(0.0, min(1.0, soft_label_alpha)))
    if value_dist is not None or value_dist_row is not None:
        _check_value_dist(value_dist, value_dist_row, int(log_p1.shape[0]), log_p1.device, anti_draw_penalty)
    if row_weights is not None:
        B = int(log_p1.shape[0])
        if not isinstance(row_weights, torch.Tensor) or row_weights.dtype != torch.float32:
            raise TypeError("row_weights must be a float32 tensor")
        if tuple(row_weights.shape) != (B,):
            raise ValueError(f"row_weights must have shape [{B}], got {tuple(row_weights.shape)}")
        if row_weights.device != log_p1.device:
            raise ValueError(f"row_weights must live on {log_p1.device}, got {row_weights.device}")
    if value_dist is not None:
        loss, pol, bucket, aux = _FusedLossDist.apply(
            log_p1, log_p2, log_pmc, value_logits, legal_mask, policy_target, value_target, soft_value_target,
            None if row_weights is None else row_weights.detach(), value_dist.detach(), value_dist_row, alpha,
            float(anti_draw_penalty), float(max(0.0, policy_draw_weight)))
        return loss, {"policy_loss": pol, "bucket_value_loss": bucket, "wdl_aux_loss": aux}
    if row_weights is not None:
        loss, pol, bucket, aux = _FusedLossWeighted.apply(
            log_p1, log_p2, log_pmc, value_logits, legal_mask, policy_target, value_target, soft_value_target,
            row_weights.detach(), alpha, float(anti_draw_penalty), float(max(0.0, policy_draw_weight)))
        return loss, {"policy_loss": pol, "bucket_value_loss": bucket, "wdl_aux_loss": aux}
    loss, pol, bucket, aux = _FusedLoss.apply(log_p1, log_p2, log_pmc, value_logits, legal_mask, policy_target,
                                              value_target, soft_value_target, alpha, float(anti_draw_penalty),
                                              float(max(0.0, policy_draw_weight)))
    return loss, {"policy_loss": pol, "bucket_value_loss": bucket, "wdl_aux_loss": aux}
