"""Laplace chunk loss on the device: what `train_driver.batch_loss` does between the stack and the spectral terms - the
data-driven LP mean, the scale floor, the per-segment Laplace NLL, the reparameterised sample rows, the sample error and
the figures of the LaplaceLoss log line - as one HIP operator (`torch.ops.swn.laplace_loss`, csrc/swn_laplace_loss.hip)
on the raw output of the stack instead of a few hundred element-wise torch ops and their autograd nodes.

    loss = LaplaceChunkLoss(model.seg, model.lpc)
    raw = model.forward_raw(aux, audio, do=True)                              # (B, 2 seg + lpc, Tp)
    nll, err, samples, targets, stats = loss(raw, x_prob, target, eps, skip)

nll (B, seg) and err (B, seg) are the per-segment means over the Tp - skip kept positions, samples / targets the
(B seg, N) rows `spectral.MultiResolutionSTFTLoss` takes, stats (7,) min / mean / max / unbiased variance of mu and min /
mean / max of 2 b^2 of segment 0.  Gradient flows to `raw` from nll and samples only.  eps: (B, seg, N) deviates of
U(-0.4999, 0.5).  There is no torch fall-back: without the library the call raises.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .config import NetConfig


class LaplaceChunkLoss:
    """the operator for one (seg, lpc) head geometry."""

    def __init__(self, seg: int, lpc: int) -> None:
        if not 1 <= int(seg) <= 10 or not 0 <= int(lpc) <= 16:
            raise ValueError(f"seg in [1, 10] and lpc in [0, 16], got seg {seg} / lpc {lpc}")
        self.seg, self.lpc = int(seg), int(lpc)
        self.n_out = 2 * self.seg + self.lpc
        self._desc = ops.desc_list(NetConfig(kind="laplace", seg=self.seg, lpc=self.lpc))

    def check(self, raw, x_prob, target, eps, skip: int) -> Tuple[int, int, int]:
        """shape rules of the call -> (B, Tp, N)"""
        seg, lpc = self.seg, self.lpc
        if raw.dim() != 3 or raw.shape[1] != self.n_out:
            raise ValueError(f"raw must be (B, {self.n_out}, Tp) for seg {seg} / lpc {lpc}, got {tuple(raw.shape)}")
        B, _, tp = raw.shape
        skip = int(skip)
        if skip < 0 or tp - skip < 1:
            raise ValueError(f"skip {skip} leaves no position of the {tp} the stack produced")
        N = tp - skip
        if lpc > 0:
            if x_prob is None:
                raise ValueError(f"lpc {lpc} needs the LP context x_prob")
            if tuple(x_prob.shape) != (B, tp + seg + lpc - 1):
                raise ValueError(f"x_prob must be ({B}, {tp + seg + lpc - 1}) = (B, Tp + seg + lpc - 1), got "
                                 f"{tuple(x_prob.shape)}")
        if tuple(target.shape) != (B, tp + seg - 1):
            raise ValueError(f"target must be ({B}, {tp + seg - 1}) = (B, Tp + seg - 1), got {tuple(target.shape)}")
        if tuple(eps.shape) != (B, seg, N):
            raise ValueError(f"eps must be ({B}, {seg}, {N}) = (B, seg, Tp - skip), got {tuple(eps.shape)}")
        if target.requires_grad or eps.requires_grad or (x_prob is not None and x_prob.requires_grad):
            raise ValueError("the Laplace chunk loss gives gradient to raw only: detach the context, target and deviates")
        return B, tp, N

    def __call__(self, raw: torch.Tensor, x_prob: Optional[torch.Tensor], target: torch.Tensor, eps: torch.Tensor,
                 skip: int = 0):
        """-> (nll (B, seg), err (B, seg), samples (B seg, N), targets (B seg, N), stats (7,)); a 1-D target of a
        one-utterance chunk (as `slice_chunk` returns it) is taken as (1, Tp + seg - 1)."""
        if target.dim() == 1:
            target = target.unsqueeze(0)
        if self.lpc == 0:
            x_prob = None
        self.check(raw, x_prob, target, eps, skip)
        if torch.is_grad_enabled() and raw.requires_grad:
            return ops.LaplaceLossFunction.apply(raw, x_prob, target, eps, self._desc, int(skip))
        return ops.laplace_loss_impl(raw.detach(), x_prob, target, eps, self._desc, int(skip))
