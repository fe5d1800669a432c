"""Multi-resolution STFT loss on the device: the spectral terms of `train_driver.batch_loss` as one HIP operator
(`torch.ops.swn.spectral_loss`, csrc/swn_spectral.hip) instead of one `torch.stft` and its autograd per FFT size.

    loss = MultiResolutionSTFTLoss(train_driver.fft_sizes(17), "cuda:0")
    l1, lsd = loss(samples, targets, feat_len)         # (R, K') each, K' = the sizes with feat_len > n // 2

`l1[r, k]` is `LSDloss(LSD=False, L2=False)` and `lsd[r, k]` is `LSDloss()` of the reference on
`torch.stft(x, n, window=hann_window(n))` of row r (hop n // 4, reflect-centred, one-sided); l1 is differentiable in the
samples, lsd is a reported figure.  The values are raw per pair - non-finite terms included; the selection of the finite
ones stays with the caller, as in `batch_loss`.  There is no torch fall-back: without the library the call raises.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops


def frame_count(length: int, n_fft: int) -> int:
    """frames of torch.stft(x, n_fft) with its defaults (hop n_fft // 4, center=True)"""
    return 1 + length // (n_fft // 4)


def bin_count(n_fft: int) -> int:
    """one-sided bins"""
    return n_fft // 2 + 1


def check_size(n_fft: int) -> None:
    if n_fft % 32 != 0 or not 32 <= n_fft <= _lib.SPECTRAL_MAX_FFT:
        raise ValueError(f"FFT size {n_fft} is not a multiple of 32 in [32, {_lib.SPECTRAL_MAX_FFT}]")


def size_tables(n_fft: int) -> np.ndarray:
    """cos(2 pi m / n) for m < n, then the periodic Hann window: 2 n floats, evaluated in float64"""
    check_size(n_fft)
    m = np.arange(n_fft, dtype=np.float64)
    # exact zeros and ones at the quarter points (cos of a float64 multiple of pi / 2 is not exactly 0)
    c = np.cos(2.0 * np.pi * m / n_fft)
    c[n_fft // 4] = c[3 * n_fft // 4] = 0.0
    return np.concatenate([c, 0.5 - 0.5 * c]).astype(np.float32)


class MultiResolutionSTFTLoss:
    """holds the per-size tables on `device`; a call evaluates the sizes that fit the signal length."""

    def __init__(self, fft_sizes: Sequence[int], device) -> None:
        self.fft_sizes: List[int] = [int(n) for n in fft_sizes]
        if not 1 <= len(self.fft_sizes) <= _lib.SPECTRAL_MAX_SIZES:
            raise ValueError(f"1 to {_lib.SPECTRAL_MAX_SIZES} FFT sizes, got {len(self.fft_sizes)}")
        self.device = torch.device(device)
        self._tables = {n: torch.from_numpy(size_tables(n)).to(self.device) for n in self.fft_sizes}
        self._joined: Dict[Tuple[int, ...], torch.Tensor] = {}

    def sizes_for(self, feat_len: int) -> List[int]:
        """the sizes `batch_loss` keeps for a chunk of feat_len samples"""
        return [n for n in self.fft_sizes if feat_len > n // 2]

    def tables_for(self, sizes: Sequence[int]) -> torch.Tensor:
        key = tuple(sizes)
        t = self._joined.get(key)
        if t is None:
            t = self._joined[key] = torch.cat([self._tables[n] for n in key])
        return t

    def __call__(self, samples, targets, feat_len: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """samples / targets: (R, T) tensors or lists of R equally long signals -> (l1 (R, K'), lsd (R, K'))"""
        if not torch.is_tensor(samples):
            samples = torch.stack(list(samples))
        if not torch.is_tensor(targets):
            targets = torch.stack(list(targets))
        if targets.requires_grad:
            raise ValueError("the spectral loss gives no gradient to its targets: detach them")
        if samples.dim() != 2 or samples.shape != targets.shape:
            raise ValueError(f"samples and targets must share one shape (R, T), got {tuple(samples.shape)} and "
                             f"{tuple(targets.shape)}")
        T = samples.shape[1]
        sizes = self.sizes_for(feat_len)
        if not sizes:
            raise ValueError(f"no FFT size of {self.fft_sizes} fits a chunk of {feat_len} samples")
        for n in sizes:
            if T <= n // 2:
                raise ValueError(f"FFT size {n} needs signals longer than {n // 2} samples (reflect padding), got {T}")
        tables = self.tables_for(sizes)
        if torch.is_grad_enabled() and samples.requires_grad:
            return ops.SpectralLossFunction.apply(samples, targets, tables, sizes)
        l1, lsd, _ = ops.spectral_loss_impl(samples.detach(), targets, tables, sizes, False)
        return l1, lsd
