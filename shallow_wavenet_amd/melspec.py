"""Log-mel conditioning features from waveforms on the device (`torch.ops.swn.logmel`, csrc/swn_melspec.hip): a second,
fully pinned feature type next to the WORLD / SPTK features of run.sh stage 1 (which stay with pyworld / pysptk, dsp.py).

    ext = LogMelExtractor(fs=22050, n_fft=1024, hop=110, n_mels=80, device="cuda:0")
    feats = ext(wavs, lengths)                 # (R, F_max, n_mels), time-major like the feature files; zero past a row's frames
    stream = LogMelStream(ext)                 # the same frames, as the samples arrive
    new = stream.push(chunk); ...; last = stream.finish()

Definition (the contract; include/swn_hip.h and csrc/swn_melspec.hip restate it).  Parameters: `fs` sample rate; `n_fft` a
multiple of 32 in [32, SWN_SPECTRAL_MAX_FFT]; `hop` in 1 .. n_fft, which need not divide n_fft (the 22.05 kHz nets use 110,
the 16 kHz nets 80); `n_mels` in 1 .. 128; 0 <= fmin < fmax <= fs / 2; floor > 0 (default 1e-5).  For a signal of `len`
samples, len > n_fft / 2:
  * Frames: F = 1 + len // hop.  Frame f reads the padded positions p = f * hop - n_fft / 2 + j, j < n_fft, with reflect
    padding that does not repeat the edge sample: p < 0 -> -p and p >= len -> 2 (len - 1) - p.  This is
    `torch.stft(center=True, pad_mode="reflect")`.
  * Window: periodic Hann, w[j] = 0.5 - 0.5 cos(2 pi j / n_fft).
  * Amplitude: A[f][b] = | sum_j x[p] w[j] e^(-2 pi i j b / n_fft) |, b = 0 .. n_fft / 2 - the amplitude, not the power.
  * Filter bank: HTK mel, no area normalisation.  mel(h) = 2595 log10(1 + h / 700); points P_k = mel^-1 of n_mels + 2
    equally spaced values from mel(fmin) to mel(fmax); W[m][b] = max(0, min((h_b - P_m) / (P_m+1 - P_m),
    (P_m+2 - h_b) / (P_m+2 - P_m+1))) with h_b = b fs / n_fft.  The tables are evaluated in float64 on the host and stored as
    fp32, like `spectral.size_tables`.  A filter that covers no bin is a ValueError when the extractor is built.
  * Mel amplitudes: M[f][m] = sum_b W[m][b] A[f][b] over the filter's support in ascending b.  The order is fixed.
  * Output: ln(max(M, floor)) as fp32, laid out (rows, F_max, n_mels); `linear=True` returns M itself.

F = 1 + len // hop is NOT WORLD's frame count when 5 ms is not an integer number of samples (22 050 Hz: 110.25 samples;
`dsp.world_frame_count` is unchanged); the training drivers' `validate_length` trims features and waveform to each other.
A frame's values do not depend on the batch, the frame range or the buffer window it is computed from, so the stream's
concatenated output is bit-identical to the one-shot call.  There is no torch fall-back: without the library the call raises.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, ops
from .spectral import check_size, size_tables


def frame_count(length: int, hop: int) -> int:
    """F = 1 + len // hop"""
    return 1 + int(length) // int(hop)


def hz_to_mel(h):
    return 2595.0 * np.log10(1.0 + np.asarray(h, dtype=np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def _check_band(fs: float, n_mels: int, fmin: float, fmax: float) -> None:
    if not 1 <= n_mels <= _lib.LOGMEL_MAX_MELS:
        raise ValueError(f"n_mels {n_mels} outside [1, {_lib.LOGMEL_MAX_MELS}]")
    if not 0.0 <= fmin < fmax <= fs / 2.0:
        raise ValueError(f"need 0 <= fmin < fmax <= fs / 2, got fmin {fmin}, fmax {fmax}, fs {fs}")


def mel_filterbank(fs: float, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None) -> np.ndarray:
    """W (n_mels, n_fft // 2 + 1) in float64: HTK mel triangles of height 1, no area normalisation"""
    fmax = fs / 2.0 if fmax is None else float(fmax)
    check_size(n_fft)
    _check_band(fs, n_mels, fmin, fmax)
    pts = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    h = np.arange(n_fft // 2 + 1, dtype=np.float64) * fs / n_fft
    up = (h[None, :] - pts[:-2, None]) / (pts[1:-1] - pts[:-2])[:, None]
    down = (pts[2:, None] - h[None, :]) / (pts[2:] - pts[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(up, down))


def tables(fs: float, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None
           ) -> Tuple[np.ndarray, List[int]]:
    """(table, bank) as swn_logmel takes them: cos(2 pi m / n_fft), the periodic Hann window, then every filter's run of
    non-zero weights back to back, zero-filled to 2 (n_fft / 2 + 1) floats - fp32 roundings of float64 values; bank[m] is
    the run of filter m as first bin | bins << 16.  ValueError for a filter that covers no bin."""
    W = mel_filterbank(fs, n_fft, n_mels, fmin, fmax)
    bins = n_fft // 2 + 1
    runs, bank = [], []
    for m in range(n_mels):
        nz = np.flatnonzero(W[m] > 0.0)
        if nz.size == 0:
            raise ValueError(f"mel filter {m} of {n_mels} covers no bin of a {n_fft}-point transform at fs {fs} "
                             f"(fmin {fmin}, fmax {fs / 2.0 if fmax is None else fmax}): fewer filters or a longer transform")
        assert nz[-1] - nz[0] + 1 == nz.size          # a triangle: one run
        runs.append(W[m, nz[0]:nz[-1] + 1])
        bank.append(int(nz[0]) | (int(nz.size) << 16))
    w = np.concatenate(runs)
    assert w.size <= 2 * bins                         # at most two filters overlap a bin
    table = np.zeros(2 * n_fft + 2 * bins, dtype=np.float32)
    table[:2 * n_fft] = size_tables(n_fft)
    table[2 * n_fft:2 * n_fft + w.size] = w.astype(np.float32)
    return table, bank


class LogMelExtractor:
    """holds the tables on `device`; a call computes the features of a batch of waveforms."""

    def __init__(self, fs: float, n_fft: int, hop: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None,
                 floor: float = 1e-5, device="cuda") -> None:
        self.fs, self.n_fft, self.hop, self.n_mels = fs, int(n_fft), int(hop), int(n_mels)
        self.fmin, self.fmax, self.floor = float(fmin), (fs / 2.0 if fmax is None else float(fmax)), float(floor)
        check_size(self.n_fft)
        if not 1 <= self.hop <= self.n_fft:
            raise ValueError(f"hop {hop} outside [1, n_fft = {n_fft}]")
        if not self.floor > 0.0:
            raise ValueError(f"floor {floor} must be > 0")
        table, self.bank = tables(fs, self.n_fft, self.n_mels, self.fmin, self.fmax)
        self.device = torch.device(device)
        self._table = torch.from_numpy(table).to(self.device)
        self._op = ops.logmel_impl

    def frame_count(self, length: int) -> int:
        return frame_count(length, self.hop)

    def _check_len(self, length: int) -> None:
        if length <= self.n_fft // 2:
            raise ValueError(f"n_fft {self.n_fft} needs signals longer than {self.n_fft // 2} samples (reflect padding), "
                             f"got {length}")

    def __call__(self, wavs, lengths: Optional[Sequence[int]] = None, linear: bool = False) -> torch.Tensor:
        """wavs: a padded (R, S) batch with `lengths` (default: S for every row), one 1-D signal, or a list of R 1-D signals
        of their own lengths -> (R, F_max, n_mels), row r holding frame_count(lengths[r]) frames and zeros after them."""
        if torch.is_tensor(wavs) or isinstance(wavs, np.ndarray):
            batch = torch.as_tensor(wavs)
            if batch.dim() == 1:
                batch = batch[None]
            if batch.dim() != 2:
                raise ValueError(f"wavs must be (R, S) or a list of 1-D signals, got shape {tuple(batch.shape)}")
            lens = [batch.shape[1]] * batch.shape[0] if lengths is None else [int(n) for n in lengths]
            batch = batch.to(self.device, torch.float32).contiguous()
        else:
            rows = [torch.as_tensor(w).reshape(-1) for w in wavs]
            if lengths is not None:
                raise ValueError("a list of signals carries its own lengths")
            lens = [int(r.numel()) for r in rows]
            batch = torch.zeros((len(rows), max(lens + [1])), dtype=torch.float32, device=self.device)
            for i, r in enumerate(rows):
                batch[i, :lens[i]] = r.to(self.device, torch.float32)
        if len(lens) != batch.shape[0] or batch.shape[0] < 1:
            raise ValueError(f"{batch.shape[0]} rows, {len(lens)} lengths")
        for n in lens:
            self._check_len(n)
            if n > batch.shape[1]:
                raise ValueError(f"length {n} exceeds the batch's {batch.shape[1]} columns")
        R = len(lens)
        return self._op(batch, self._table, self.bank, [0] * R, lens, lens, [0] * R, [self.frame_count(n) for n in lens],
                        self.n_fft, self.hop, self.floor, bool(linear))

    def frames(self, wav: torch.Tensor, t0: Union[int, Sequence[int]], n_avail: Union[int, Sequence[int]],
               length: Union[int, Sequence[int]], f0: Union[int, Sequence[int]], f1: Union[int, Sequence[int]],
               linear: bool = False) -> torch.Tensor:
        """frames [f0, f1) from a partial buffer: `wav` (S,) or (R, S) holds the samples [t0, t0 + n_avail) of each signal,
        whose total length is `length` or -1 while it is not known -> (f1 - f0, n_mels) or (R, max(f1 - f0), n_mels).  A
        range whose samples (the reflected ones included) are not all in the buffer is refused."""
        one = wav.dim() == 1
        buf = (wav[None] if one else wav).to(self.device, torch.float32).contiguous()
        lst = lambda v: [int(v)] * buf.shape[0] if isinstance(v, (int, np.integer)) else [int(x) for x in v]
        out = self._op(buf, self._table, self.bank, lst(t0), lst(n_avail), lst(length), lst(f0), lst(f1), self.n_fft, self.hop,
                       self.floor, bool(linear))
        return out[0] if one else out


class LogMelStream:
    """one signal's features as its samples arrive: `push` returns the frames that became computable, `finish` the rest
    (those that read the reflected end).  Only the tail of the signal that later frames still read is kept.  The
    concatenation of everything returned is bit-identical to the extractor's one-shot call on the whole signal."""

    def __init__(self, extractor: LogMelExtractor, linear: bool = False) -> None:
        self.ext, self.linear = extractor, bool(linear)
        self._buf = torch.zeros(0, dtype=torch.float32, device=extractor.device)
        self.t0 = 0                 # absolute index of _buf[0]
        self.n_received = 0
        self.n_frames = 0           # frames returned so far
        self.finished = False

    def computable(self, n_received: int) -> int:
        """frames whose samples have all arrived: frame 0 reads up to sample n_fft / 2 (the left reflection), frame
        f >= 1 up to f hop + n_fft / 2 - 1"""
        half = self.ext.n_fft // 2
        return 0 if n_received <= half else 1 + (n_received - half) // self.ext.hop

    def _drop_consumed(self) -> None:
        # the next frame starts at n_frames hop - n_fft / 2; the reflected end of the last frame comes back to one sample
        # before the start of a frame that begins exactly at the signal's end
        keep = max(self.t0, self.n_frames * self.ext.hop - self.ext.n_fft // 2 - 1)
        if keep > self.t0:
            self._buf = self._buf[keep - self.t0:]
            self.t0 = keep

    def _range(self, f1: int, length: int) -> torch.Tensor:
        f0 = self.n_frames
        if f1 <= f0:
            return torch.zeros((0, self.ext.n_mels), dtype=torch.float32, device=self.ext.device)
        out = self.ext.frames(self._buf, self.t0, int(self._buf.numel()), length, f0, f1, self.linear)
        self.n_frames = f1
        self._drop_consumed()
        return out

    def push(self, samples) -> torch.Tensor:
        """append 1-D samples -> (k, n_mels) new frames, k >= 0"""
        if self.finished:
            raise RuntimeError("the stream is finished")
        s = torch.as_tensor(samples).reshape(-1).to(self.ext.device, torch.float32)
        self._buf = torch.cat([self._buf, s])
        self.n_received += int(s.numel())
        return self._range(self.computable(self.n_received), -1)

    def finish(self) -> torch.Tensor:
        """the signal ends here -> the remaining frames up to F = 1 + n_received // hop"""
        if self.finished:
            raise RuntimeError("the stream is finished")
        self.ext._check_len(self.n_received)
        self.finished = True
        return self._range(self.ext.frame_count(self.n_received), self.n_received)
