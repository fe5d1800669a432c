"""Log-mel conditioning features from waveforms on the device (`torch.ops.swn.logmel`, csrc/swn_melspec.hip): a second,
fully pinned feature type next to the WORLD / SPTK features of run.sh stage 1 (which stay with pyworld / pysptk, dsp.py).

    ext = LogMelExtractor(fs=22050, n_fft=1024, hop=110, n_mels=80, device="cuda:0")
    feats = ext(wavs, lengths)                 # (R, F_max, n_mels), time-major like the feature files; zero past a row's frames
    stream = LogMelStream(ext)                 # the same frames, as the samples arrive
    new = stream.push(chunk); ...; last = stream.finish()
    mels = LogMelPool(ext, capacity=64, max_chunk=4096)        # ... for many signals at once, one call per tick
    m = mels.open(); new = mels.push_many({m: chunk, ...}, finish=[...])       # {session: (1, n_mels, k)}: what the decode pools take
    mc = MelCepstrumExtractor(fs=22050, n_fft=1024, hop=110, order=49, alpha=0.455, device="cuda:0")(wavs, lengths)
                                               # (R, F_max, order + 1): the mel-cepstrum of the same short-time spectra
                                               # (`torch.ops.swn.mcep`), for the statistics the noise-shaping stages need;
                                               # its definition is in the class's docstring
    env = SpectralEnvelopeExtractor(fs=22050, n_fft=1024, hop=110, order=49, alpha=0.455, device="cuda:0")
    mc = env(wavs, lengths, f0)                # (R, F_max, order + 1): the mel-cepstrum of the F0-adaptive spectral envelope
                                               # (`torch.ops.swn.envelope`) at the per-frame F0 of pitch.F0Extractor - without the
                                               # pitch harmonics the short-time spectrum carries; definition in the class's docstring
    cut = LowCut(fs=22050, cutoff=70.0, device="cuda:0")       # the stage-1 low cut (`torch.ops.swn.lowcut_chunk`): what the
    y = cut(wavs, lengths)                                     # training features were taken from; LogMelStream(ext, low_cut=cut)
                                                               # and LogMelPool(..., low_cut=cut) take RAW samples and filter them
    res = Resampler(fs_in=48000, fs_out=22050, device="cuda:0")    # the rational resampler (`torch.ops.swn.resample_chunk`) in
    y = res(wavs, lengths)                                     # front of it: LogMelStream(ext, resample=res, low_cut=cut) and
                                                               # LogMelPool(..., resample=res, low_cut=cut) take samples at fs_in

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

The low cut (the contract; include/swn_hip.h states it, csrc/swn_lowcut.hpp is its arithmetic).  Taps h[0 .. n_taps - 1] in fp64,
1 <= n_taps <= SWN_LOWCUT_MAX_TAPS (256); input samples x in fp32, x[t] = 0 for t < 0.  Output sample t:
    acc = 0.0;  for q = 0 .. n_taps - 1 ascending: acc = fma(h[q], (double)x[t - q], acc);  y[t] = (float)acc
Every output sample depends only on its absolute index and the signal - not on the chunking, the entry, the batch, the tile or
the call - so any partition of a signal into chunks gives the bits of the one-shot call, and a stream's or a pool's frames are
the extractor's on the one-shot filtered signal.  A session's state is its last n_taps - 1 raw input samples in fp32 (exact: the
inputs are fp32).  `dsp.low_cut_filter` (scipy's lfilter, float64 out) sums the same products in another order and is not
rounded to fp32: the two differ by the rounding above, at most one step of a PCM16 file.

The resampler (the contract; include/swn_hip.h states it, tests/resample_ref.py pins it).  fs_in and fs_out are integers,
L = fs_out / g and M = fs_in / g with g = gcd(fs_in, fs_out).  Prototype filter h[0 .. N - 1] in fp64, N odd, from
`resample_taps(L, M, half_len=10, beta=5.0)`: N = 2 * 10 * max(L, M) + 1 and h = L * scipy.signal.firwin(N, 1 / max(L, M),
window=("kaiser", 5.0)), the filter of `scipy.signal.resample_poly`; D = (N - 1) / 2.  Polyphase table P[r][q], r < L,
q < Q = ceil(N / L): P[r][q] = h[r + q L], and 0.0 where r + q L >= N (`resample_table`), fp64 on the device, row by row.  Output
sample n (absolute index) of a signal of `len` input samples, x[t] = 0 outside [0, len):
    p = n M + D (64-bit),  r = p mod L,  i0 = p div L
    acc = +0.0;  for q = 0 .. Q - 1 ascending: acc = fma(P[r][q], (double)x[i0 - q], acc);  y[n] = (float)acc
and there are ceil(len L / M) outputs.  One fp64 fma chain in a fixed order, rounded once to fp32: a sample's bits depend only on
its absolute index and the signal, not on the chunking, the entry, the batch, the tile or the call.  Streaming rule
(`resample_ready`, the one place it is written): while the signal goes on and T inputs have arrived, the computable outputs are
those with i0 <= T - 1 - none if T L - 1 - D < 0, else (T L - 1 - D) div M + 1 of them; when the signal ends at T, all
ceil(T L / M).  A session's state is its last Q - 1 raw inputs in fp32 (exact), so a call is parallel over time.
"""
from __future__ import annotations

import math
from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple, Union

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


def _padded_batch(ext, wavs, lengths: Optional[Sequence[int]]) -> Tuple[torch.Tensor, List[int]]:
    """the waveforms of a call as one padded fp32 (R, S) batch on the extractor's device, and the rows' lengths"""
    if torch.is_tensor(wavs) or isinstance(wavs, np.ndarray):
        batch = torch.as_tensor(wavs)
        if batch.dim() == 1:
            batch = batch[None]
        if batch.dim() != 2:
            raise ValueError(f"wavs must be (R, S) or a list of 1-D signals, got shape {tuple(batch.shape)}")
        lens = [batch.shape[1]] * batch.shape[0] if lengths is None else [int(n) for n in lengths]
        batch = batch.to(ext.device, torch.float32).contiguous()
    else:
        rows = [torch.as_tensor(w).reshape(-1) for w in wavs]
        if lengths is not None:
            raise ValueError("a list of signals carries its own lengths")
        lens = [int(r.numel()) for r in rows]
        batch = torch.zeros((len(rows), max(lens + [1])), dtype=torch.float32, device=ext.device)
        for i, r in enumerate(rows):
            batch[i, :lens[i]] = r.to(ext.device, torch.float32)
    if len(lens) != batch.shape[0] or batch.shape[0] < 1:
        raise ValueError(f"{batch.shape[0]} rows, {len(lens)} lengths")
    for n in lens:
        ext._check_len(n)
        if n > batch.shape[1]:
            raise ValueError(f"length {n} exceeds the batch's {batch.shape[1]} columns")
    return batch, lens


def _check_reflect_len(n_fft: int, length: int) -> None:
    if length <= n_fft // 2:
        raise ValueError(f"n_fft {n_fft} needs signals longer than {n_fft // 2} samples (reflect padding), got {length}")


def _per_row(v, rows: int) -> List[int]:
    return [int(v)] * rows if isinstance(v, (int, np.integer)) else [int(x) for x in v]


class _FrameExtractor:
    """what LogMelExtractor, MelCepstrumExtractor, SpectralEnvelopeExtractor and pitch.F0Extractor share: the one-shot call and the frames of a partial
    buffer, both as one call of the frame-range contract ops._frame_entries states.  A subclass's constructor sets `hop`, `device`
    and `_op`; it supplies `_check_len(length)` (ValueError for a signal too short) and `_run(buf, t0s, n_avails, lens, f0s,
    f1s, *more)`, which hands `self._op` the contract's lists with the subclass's own arguments around them."""

    def frame_count(self, length: int) -> int:
        return frame_count(length, self.hop)

    def _whole(self, wavs, lengths, *more) -> torch.Tensor:
        batch, lens = _padded_batch(self, wavs, lengths)
        R = len(lens)
        return self._run(batch, [0] * R, lens, lens, [0] * R, [self.frame_count(n) for n in lens], *more)

    def _partial(self, wav, t0, n_avail, length, f0, f1, *more) -> torch.Tensor:
        one = wav.dim() == 1
        buf = (wav[None] if one else wav).to(self.device, torch.float32).contiguous()
        out = self._run(buf, *[_per_row(v, buf.shape[0]) for v in (t0, n_avail, length, f0, f1)], *more)
        return out[0] if one else out

    def __call__(self, wavs, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
        """wavs: a padded (R, S) batch with `lengths` (default: S for every row), one 1-D signal, or a list of R 1-D signals
        of their own lengths -> (R, F_max, columns), row r holding frame_count(lengths[r]) frames and zeros after them."""
        return self._whole(wavs, lengths)

    def frames(self, wav: torch.Tensor, t0: Union[int, Sequence[int]], n_avail: Union[int, Sequence[int]],
               length: Union[int, Sequence[int]], f0: Union[int, Sequence[int]], f1: Union[int, Sequence[int]]) -> torch.Tensor:
        """frames [f0, f1) from a partial buffer: `wav` (S,) or (R, S) holds the samples [t0, t0 + n_avail) of each signal,
        whose total length is `length` or -1 while it is not known -> (f1 - f0, columns) or (R, max(f1 - f0), columns).  A
        range whose in-signal samples (for log-mel and mel-cepstrum the reflected ones included) are not all in the buffer is
        refused."""
        return self._partial(wav, t0, n_avail, length, f0, f1)


class LogMelExtractor(_FrameExtractor):
    """holds the tables on `device`; a call computes the features of a batch of waveforms: n_mels columns."""

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

    def _check_len(self, length: int) -> None:
        _check_reflect_len(self.n_fft, length)

    def _run(self, buf, t0s, n_avails, lens, f0s, f1s, linear=False) -> torch.Tensor:
        return self._op(buf, self._table, self.bank, t0s, n_avails, lens, f0s, f1s, self.n_fft, self.hop, self.floor, bool(linear))

    def __call__(self, wavs, lengths: Optional[Sequence[int]] = None, linear: bool = False) -> torch.Tensor:
        """as _FrameExtractor.__call__ -> (R, F_max, n_mels); `linear`: the mel amplitudes themselves, not their logarithms"""
        return self._whole(wavs, lengths, linear)

    def frames(self, wav: torch.Tensor, t0: Union[int, Sequence[int]], n_avail: Union[int, Sequence[int]],
               length: Union[int, Sequence[int]], f0: Union[int, Sequence[int]], f1: Union[int, Sequence[int]],
               linear: bool = False) -> torch.Tensor:
        """as _FrameExtractor.frames -> (f1 - f0, n_mels) or (R, max(f1 - f0), n_mels)"""
        return self._partial(wav, t0, n_avail, length, f0, f1, linear)


# ---- mel-cepstrum --------------------------------------------------------------------------------------------------------
def _check_order(n_fft: int, order: int, alpha: float) -> None:
    if not 0 <= order <= min(_lib.MCEP_MAX_ORDER, n_fft // 2):
        raise ValueError(f"order {order} outside [0, min({_lib.MCEP_MAX_ORDER}, n_fft / 2 = {n_fft // 2})]")
    if not abs(float(alpha)) < 1.0:
        raise ValueError(f"|alpha| must be < 1, not {alpha!r}")


def mcep_matrix(n_fft: int, order: int, alpha: float) -> np.ndarray:
    """G (order + 1, n_fft // 2 + 1) in float64 with mc = G L: steps 2 - 4 of the definition as one matrix, G = T C.
    C (bins, bins) takes L to the one-sided cepstrum: irfft of a real even spectrum is a cosine sum,
    c[k] = e_k / n_fft * sum_b e_b L[b] cos(2 pi k b / n_fft) with e = 1 at 0 and n_fft / 2 and 2 between.
    T (order + 1, bins) is the frequency transform: sum_m mc(m) w^m = sum_k c(k) ((w + alpha) / (1 + alpha w))^k, so column k
    of T is the power series of the k-th power of the all-pass, truncated at w^order, each column from the one before:
    times (w + alpha), then divided by (1 + alpha w)."""
    n_fft, order = int(n_fft), int(order)
    check_size(n_fft)
    _check_order(n_fft, order, alpha)
    bins, a = n_fft // 2 + 1, float(alpha)
    e = np.full(bins, 2.0)
    e[0] = e[-1] = 1.0
    kb = (np.arange(bins)[:, None] * np.arange(bins)[None, :]) % n_fft         # the argument reduced exactly
    C = e[:, None] * e[None, :] * np.cos(2.0 * np.pi * kb.astype(np.float64) / n_fft) / n_fft
    T = np.zeros((order + 1, bins), dtype=np.float64)
    p = np.zeros(order + 1, dtype=np.float64)
    p[0] = 1.0                                                                  # the 0-th power
    T[:, 0] = p
    for k in range(1, bins):
        q = a * p
        q[1:] += p[:-1]                                                         # times (w + alpha)
        r = np.empty_like(q)
        r[0] = q[0]
        for m in range(1, order + 1):
            r[m] = q[m] - a * r[m - 1]                                          # divided by (1 + alpha w)
        T[:, k] = p = r
    return T @ C


def mcep_tables(n_fft: int, order: int, alpha: float) -> np.ndarray:
    """the table swn_mcep takes: cos(2 pi m / n_fft), the periodic Hann window, then G row by row as fp32 roundings of
    mcep_matrix, every row zero-padded to the next multiple of 4 columns"""
    G = mcep_matrix(n_fft, order, alpha)
    bins = n_fft // 2 + 1
    kp = (bins + 3) & ~3
    table = np.zeros(2 * n_fft + (order + 1) * kp, dtype=np.float32)
    table[:2 * n_fft] = size_tables(n_fft)
    table[2 * n_fft:].reshape(order + 1, kp)[:, :bins] = G.astype(np.float32)
    return table


class MelCepstrumExtractor(_FrameExtractor):
    """Mel-cepstra of the short-time spectra the log-mel features are computed from, on the device (`torch.ops.swn.mcep`,
    swn_mcep): for corpus statistics - the mean over a corpus is what the noise-shaping stages and `post_filter=` build their
    MLSA filter from - and as a conditioning feature type.

        ext = MelCepstrumExtractor(fs=22050, n_fft=1024, hop=110, order=49, alpha=0.455, device="cuda:0")
        mc = ext(wavs, lengths)                # (R, F_max, order + 1), time-major; zero past a row's frames

    Definition (the contract; include/swn_hip.h and csrc/swn_melspec.hip restate it).  Frames (F = 1 + len // hop), reflect
    padding, periodic Hann window and amplitude A[f][b] = |DFT|, b = 0 .. n_fft / 2, are exactly those of the log-mel features
    (the module docstring).  Then, with 0 <= order <= min(63, n_fft / 2), |alpha| < 1 and floor > 0 (default 1e-5):
      1. L[f][b] = ln(max(A[f][b], floor)), evaluated in double and rounded once to fp32, as the log-mel output is.
      2. The real cepstrum v = irfft(L) of length n_fft.
      3. The one-sided cepstrum c[0] = v[0], c[k] = 2 v[k] for 0 < k < n_fft / 2, c[n_fft / 2] = v[n_fft / 2].  With this
         convention |exp(sum_k c(k) z^-k)| = A: the one `dsp.py` and the MLSA filter use.
      4. The frequency transform with all-pass constant alpha to order M (SPTK `freqt`): mc[f][0 .. M].
      5. Steps 2 - 4 are linear: mc[f] = G L[f] with G = mcep_matrix(n_fft, M, alpha) of shape (M + 1, n_fft / 2 + 1),
         evaluated in float64 on the host and stored as fp32, its columns zero-padded to a multiple of 4.
      6. Output fp32, time-major out[frame][coefficient].  Each coefficient is one chain over the bins in ascending order (the
         k order of the matrix instruction), so a frame's values do not depend on the tile, the row of the tile, the entry,
         the batch, the frame range or the window they are computed from: any partition of the frames gives the same bits.
    On the first n_fft / 2 + 1 cepstral coefficients this is what `pysptk.sp2mc(A**2, M, alpha)` computes; parity with pysptk
    is NOT pinned (the library is absent), as for the MLSA filter.  It is the cepstrum of the short-time spectrum, not of
    WORLD's cheaptrick envelope: pitch harmonics are in it.  How audio shaped with its mean sounds is not measured here.
    There is no torch fall-back: without the library the call raises."""

    def __init__(self, fs: float, n_fft: int, hop: int, order: int, alpha: float, floor: float = 1e-5, device="cuda") -> None:
        self.fs, self.n_fft, self.hop, self.order = fs, int(n_fft), int(hop), int(order)
        self.alpha, self.floor = float(alpha), float(floor)
        check_size(self.n_fft)
        if not 1 <= self.hop <= self.n_fft:
            raise ValueError(f"hop {hop} outside [1, n_fft = {n_fft}]")
        if not self.floor > 0.0:
            raise ValueError(f"floor {floor} must be > 0")
        table = mcep_tables(self.n_fft, self.order, self.alpha)
        self.device = torch.device(device)
        self._table = torch.from_numpy(table).to(self.device)
        self._op = ops.mcep_impl

    def _check_len(self, length: int) -> None:
        _check_reflect_len(self.n_fft, length)

    def _run(self, buf, t0s, n_avails, lens, f0s, f1s) -> torch.Tensor:
        return self._op(buf, self._table, t0s, n_avails, lens, f0s, f1s, self.n_fft, self.hop, self.order, self.floor)


# ---- spectral envelope by F0-adaptive smoothing ----------------------------------------------------------------------------
ENVELOPE_OUTPUTS = {"mcep": _lib.ENVELOPE_MCEP, "logamp": _lib.ENVELOPE_LOGAMP}


def envelope_f0_floor(fs: float, n_fft: int) -> float:
    """the lowest F0 a transform of n_fft points can analyse: 3 fs / (n_fft - 3), so that three periods fit the frame"""
    return 3.0 * float(fs) / (float(n_fft) - 3.0)


def _check_envelope(fs: float, n_fft: int, hop: int, order: int, alpha: float, floor: float, q1: float, default_f0: float) -> None:
    check_size(n_fft)
    if not (fs > 0.0 and math.isfinite(fs)):
        raise ValueError(f"fs {fs!r} must be a finite number > 0")
    if not 1 <= hop <= _lib.F0_MAX_HOP:
        raise ValueError(f"hop {hop} outside [1, {_lib.F0_MAX_HOP}]")
    _check_order(n_fft, order, alpha)
    if not (floor > 0.0 and math.isfinite(floor) and float(np.float32(floor)) > 0.0 and math.isfinite(float(np.float32(floor)))):
        raise ValueError(f"floor {floor!r} must be a finite fp32 number > 0")
    if not math.isfinite(q1):
        raise ValueError(f"q1 {q1!r} must be finite")
    lo = envelope_f0_floor(fs, n_fft)
    if not lo < default_f0 <= fs / 4.0:
        raise ValueError(f"default_f0 {default_f0!r} outside (3 fs / (n_fft - 3) = {lo:g}, fs / 4 = {fs / 4.0:g}]: n_fft {n_fft} "
                         f"is too short for fs {fs} (8 000 Hz needs 64, 22 050 Hz needs 160)")


def envelope_matrix(n_fft: int, order: int, alpha: float) -> np.ndarray:
    """G (order + 1, n_fft // 2 + 1) in float64 with mc = G c: SPTK's `freqt` recursion run on the unit vectors, coefficient by
    coefficient (for every input coefficient from the last to the first: g[0] = c + alpha d[0]; g[1] = (1 - alpha^2) d[0] +
    alpha d[1]; g[j] = d[j - 1] + alpha (d[j] - g[j - 1]), d the g of the step before)."""
    n_fft, order = int(n_fft), int(order)
    check_size(n_fft)
    _check_order(n_fft, order, alpha)
    bins = n_fft // 2 + 1
    a = np.float64(alpha)
    b = np.float64(1.0) - a * a
    c = np.eye(bins, dtype=np.float64)
    g = np.zeros((bins, order + 1), dtype=np.float64)
    for i in range(bins - 1, -1, -1):
        d = g.copy()
        g[:, 0] = c[:, i] + a * d[:, 0]
        if order >= 1:
            g[:, 1] = b * d[:, 0] + a * d[:, 1]
        for j in range(2, order + 1):
            g[:, j] = d[:, j - 1] + a * (d[:, j] - g[:, j - 1])
    return np.ascontiguousarray(g.T)


def envelope_tables(n_fft: int, order: int, alpha: float) -> np.ndarray:
    """the float64 table swn_envelope takes: cos(2 pi m / n_fft) for m < n_fft, then envelope_matrix row by row"""
    G = envelope_matrix(n_fft, order, alpha)
    return np.concatenate([np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft), G.reshape(-1)])


def envelope_frames_ready(n_fft: int, hop: int, n_received: int, final: bool = False) -> int:
    """the streaming rule of the spectral envelope, the one place it is written: frame f spans [f hop - (n_fft / 2 - 1),
    f hop + n_fft / 2) whatever its F0, so while the signal goes on it is computable iff f hop + n_fft / 2 <= n_received; when the
    signal ends there (`final`), all F = 1 + n_received // hop are.  Not `frames_ready`: there frame 0 reads the reflected sample
    n_fft / 2 and needs one sample more."""
    if final:
        return frame_count(n_received, hop)
    half = n_fft // 2
    return 0 if n_received < half else 1 + (n_received - half) // hop


class SpectralEnvelopeExtractor(_FrameExtractor):
    """The spectral envelope by F0-adaptive smoothing, and its mel-cepstrum, on the device (`torch.ops.swn.envelope`,
    swn_envelope): what `MelCepstrumExtractor` is not - its fixed 1 024-sample frame resolves the harmonics, so the pitch is in
    its coefficients; here a frame is analysed under a window of three pitch periods and smoothed over 2 f0 / 3.

        f0 = F0Extractor(fs=22050, hop=110, device="cuda:0")(wavs, lengths)[..., 0]        # (R, F_max) Hz, 0.0 when unvoiced
        ext = SpectralEnvelopeExtractor(fs=22050, n_fft=1024, hop=110, order=49, alpha=0.455, device="cuda:0")
        mc = ext(wavs, lengths, f0)            # (R, F_max, order + 1), time-major; zero past a row's frames
        part = ext.frames(buf, t0, n_avail, length, f0, f1, f0_values)      # frames [f0, f1) from a partial buffer
        E = SpectralEnvelopeExtractor(..., output="logamp")(wavs, lengths, f0)             # (R, F_max, n_fft / 2 + 1): ln amplitude

    It is CheapTrick's procedure (Morise 2015) in a fixed arithmetic.  It omits WORLD's added noise and its eps and has a floor
    instead.  Parity with pyworld / pysptk is neither claimed nor pinned, as for F0 and the aperiodicity.

    Definition (the contract; include/swn_hip.h restates it, tests/envelope_ref.py pins it).  Parameters: fs > 0; n_fft a
    multiple of 32 in [32, SWN_SPECTRAL_MAX_FFT]; 1 <= hop <= SWN_F0_MAX_HOP; 0 <= order <= min(63, n_fft / 2) with |alpha| < 1;
    floor > 0, an amplitude, given as fp32 (default 1e-5); q1 (default -0.15); default_f0 (default 500.0).  With D = fs / n_fft
    and f0_floor = 3 fs / (n_fft - 3) the geometry is refused unless f0_floor < default_f0 <= fs / 4: fs 8 000 needs n_fft >= 64,
    22 050 needs 160.  Input: len >= 1 finite fp32 samples, x[t] = 0 outside [0, len) (zero padding, as F0Extractor); F = 1 +
    len // hop frames, the grid of the other extractors; one fp32 value f0[f] per frame, any number - F0Extractor's column 0 is
    the intended source.  Everything below is IEEE double in the order written, every sum one chain in ascending index from +0.0
    with fma, each output value rounded once to fp32.
      1. Effective F0: f0e = (double)f0[f] if f0_floor < f0[f] <= fs / 4, else default_f0.  Unvoiced 0.0, NaN, values under the
         floor and values over fs / 4 all take the default.
      2. Window: hl = floor(1.5 fs / f0e + 0.5), so 2 hl + 1 <= n_fft - 1 always.  For k = -hl .. hl: w[k] = 0.5 cos(pi k f0e /
         (1.5 fs)) + 0.5; w /= sqrt(sum w^2); xw[k] = x[f hop + k] w[k]; then xw[k] -= w[k] (sum xw / sum w), w already normalised.
      3. Power: P[b] = |sum_k xw[k] e^(-2 pi i b (k + hl) / n_fft)|^2 = re^2 + im^2 for b = 0 .. n_fft / 2; with j = k + hl the
         twiddles are T[(b j) mod n_fft] (re) and T[(b j + n_fft / 4) mod n_fft] (im), T[m] = cos(2 pi m / n_fft) the fp64 table
         evaluated on the host.
      4. DC correction, from the uncorrected P: for b = 0 .. floor(f0e / D): u = f0e / D - b, i = floor(u), P'[b] = (P[b] + P[i])
         + (u - i)(P[i + 1] - P[i]); P' = P elsewhere.
      5. Box smoothing of width wd = 2 f0e / 3 over the spectrum taken as one rectangle of width D per bin, mirrored at 0 and at
         Nyquist: S[b] = (1 / wd) sum_n ov(n) P'[mir(n)], n ascending from floor((b D - wd / 2) / D + 0.5) to floor((b D + wd / 2)
         / D + 0.5), ov(n) = min(b D + wd / 2, (n + 0.5) D) - max(b D - wd / 2, (n - 0.5) D), terms with ov <= 0 skipped,
         mir(n) = -n for n < 0, n_fft - n for n > n_fft / 2, else n.
      6. Log: L[b] = ln max(S[b], floor^2).
      7. Liftering: v[k] = (1 / n_fft) sum_b e_b L[b] T[(k b) mod n_fft] for k = 0 .. n_fft / 2, e = 1 at 0 and n_fft / 2 and 2
         between (irfft as a cosine sum); l_s[0] = 1, l_s[k] = sin(pi f0e k / fs) / (pi f0e k / fs); l_c[k] = (1 - 2 q1) + 2 q1
         cos(2 pi k f0e / fs); ct[k] = v[k] l_s[k] l_c[k].
      8. Outputs.  "mcep": the one-sided cepstrum of the log AMPLITUDE envelope, c[0] = ct[0] / 2, c[k] = ct[k] for 0 < k <
         n_fft / 2, c[n_fft / 2] = ct[n_fft / 2] / 2, then mc[0 .. order] = freqt(c, order, alpha) as the fp64 matrix
         `envelope_matrix` (order + 1, n_fft / 2 + 1), built on the host from unit vectors.  "logamp": E[b] = 0.5 (ct[0] + 2
         sum_{0<k<n/2} ct[k] cos(2 pi k b / n_fft) + ct[n/2] (-1)^b), ln of the amplitude envelope, n_fft / 2 + 1 values.
    A frame's values depend on the signal, the frame index and that frame's F0 value alone, not on the batch, the entry, the
    frame range, the buffer window or the call: any partition gives the same bits, as for the other extractors.  Streaming rule
    (`envelope_frames_ready`): frame f is computable iff f hop + n_fft / 2 <= n_received, or when the signal has ended.
    There is no torch fall-back: without the library the call raises.

    Not covered: an EnvelopeStream or a pool variant (`frames` serves ranges; the rule above is for it); `low_cut=` /
    `resample=` (filter and resample first, as for F0Stream); parity with WORLD; time-varying noise shaping; `swn_mcep` and
    MelCepstrumExtractor are unchanged."""

    def __init__(self, fs: float, n_fft: int, hop: int, order: int, alpha: float, floor: float = 1e-5, q1: float = -0.15,
                 default_f0: float = 500.0, output: str = "mcep", device="cuda") -> None:
        self.fs, self.n_fft, self.hop, self.order = float(fs), int(n_fft), int(hop), int(order)
        self.alpha, self.floor, self.q1, self.default_f0 = float(alpha), float(floor), float(q1), float(default_f0)
        if output not in ENVELOPE_OUTPUTS:
            raise ValueError(f"output must be one of {sorted(ENVELOPE_OUTPUTS)}, not {output!r}")
        self.output, self._what = output, ENVELOPE_OUTPUTS[output]
        _check_envelope(self.fs, self.n_fft, self.hop, self.order, self.alpha, self.floor, self.q1, self.default_f0)
        self.cols = self.order + 1 if output == "mcep" else self.n_fft // 2 + 1
        table = envelope_tables(self.n_fft, self.order, self.alpha)
        self.device = torch.device(device)
        self._table = torch.from_numpy(table).to(self.device)
        self._op = ops.envelope_impl

    def _check_len(self, length: int) -> None:
        if length < 1:
            raise ValueError(f"a signal needs at least one sample, got {length}")

    def _check_ranges(self, t0s, n_avails, lens, f0s, f1s) -> None:
        """the entry rules of swn_envelope, as ValueErrors before anything is launched"""
        half = self.n_fft // 2
        for r, (t0, na, n, f0, f1) in enumerate(zip(t0s, n_avails, lens, f0s, f1s)):
            if f0 < 0 or f1 < f0:
                raise ValueError(f"row {r}: frame range [{f0}, {f1})")
            if n != -1 and not 1 <= n <= 1 << 30:
                raise ValueError(f"row {r}: length {n}, need 1 <= len <= 2^30 (or -1 while unknown)")
            if t0 < 0 or na < 0 or t0 + na > 1 << 30 or (n != -1 and t0 + na > n):
                raise ValueError(f"row {r}: window [{t0}, {t0} + {na}) is not inside the signal")
            if f1 == f0:
                continue
            if n != -1 and f1 > self.frame_count(n):
                raise ValueError(f"row {r}: f1 = {f1}, a signal of {n} samples has {self.frame_count(n)} frames")
            lo, hi = max(0, f0 * self.hop - (half - 1)), (f1 - 1) * self.hop + half - 1
            if n == -1:
                if hi >= t0 + na:
                    raise ValueError(f"row {r}: frames [{f0}, {f1}) need sample {hi}, the window ends at {t0 + na} and the total "
                                     f"length is unknown")
            else:
                hi = min(hi, n - 1)
            if lo <= hi and (lo < t0 or hi >= t0 + na):
                raise ValueError(f"row {r}: frames [{f0}, {f1}) read samples [{lo}, {hi}], the window holds [{t0}, {t0 + na})")

    def _run(self, buf, t0s, n_avails, lens, f0s, f1s, f0_values) -> torch.Tensor:
        self._check_ranges(t0s, n_avails, lens, f0s, f1s)
        if f0_values is None:
            raise ValueError("the spectral envelope needs one F0 value per frame (F0Extractor's column 0)")
        f0v = torch.as_tensor(f0_values)
        if f0v.dim() == 1:
            f0v = f0v[None]
        need = max([b - a for a, b in zip(f0s, f1s)] + [0])
        if f0v.dim() != 2 or f0v.shape[0] != buf.shape[0] or f0v.shape[1] < need:
            raise ValueError(f"f0 must hold one value per frame, ({buf.shape[0]}, >= {need}), got {tuple(f0v.shape)}")
        f0v = f0v.to(self.device, torch.float32).contiguous()
        return self._op(buf, f0v, self._table, t0s, n_avails, lens, f0s, f1s, self.fs, self.n_fft, self.hop, self.order,
                        self.floor, self.q1, self.default_f0, self._what)

    def __call__(self, wavs, lengths: Optional[Sequence[int]] = None, f0=None) -> torch.Tensor:
        """wavs, lengths: as _FrameExtractor.__call__; f0: (R, >= F_max) fp32, row r holding the F0 in Hz of its frames (what
        lies past a row's frames is not read) -> (R, F_max, order + 1) or, with output="logamp", (R, F_max, n_fft / 2 + 1)"""
        return self._whole(wavs, lengths, f0)

    def frames(self, wav: torch.Tensor, t0: Union[int, Sequence[int]], n_avail: Union[int, Sequence[int]],
               length: Union[int, Sequence[int]], f0: Union[int, Sequence[int]], f1: Union[int, Sequence[int]],
               f0_values=None) -> torch.Tensor:
        """as _FrameExtractor.frames; f0_values: (f1 - f0,) or (R, >= max(f1 - f0)), the F0 of the frames f0, f0 + 1, ... of each
        row -> (f1 - f0, columns) or (R, max(f1 - f0), columns)"""
        return self._partial(wav, t0, n_avail, length, f0, f1, f0_values)


# ---- stage-1 low cut -----------------------------------------------------------------------------------------------------
class _Slots:
    """the session slots of a LowCut or a Resampler: which of the `capacity` are free (`free`, sorted); `noun` is what the
    "the ... is full" message names"""

    def __init__(self, capacity: int, noun: str) -> None:
        self.capacity, self.noun, self.free = capacity, noun, list(range(capacity))

    def open(self, slot: Optional[int] = None) -> int:
        if slot is None:
            if not self.free:
                raise RuntimeError(f"the {self.noun} is full: all {self.capacity} slots are open")
            slot = self.free[0]
        slot = int(slot)
        if slot not in self.free:
            raise RuntimeError(f"slot {slot} is not free (capacity {self.capacity})")
        self.free.remove(slot)
        return slot

    def need_open(self, slot: int) -> None:
        if slot in self.free or not 0 <= slot < self.capacity:
            raise RuntimeError(f"slot {slot} is not open")

    def close(self, slot: int) -> int:
        slot = int(slot)
        self.need_open(slot)
        self.free.append(slot)
        self.free.sort()
        return slot


class LowCut:
    """the causal FIR high-pass of run.sh stage 1 (`dsp.low_cut_taps(fs, cutoff)`: 255 taps) on the device, with the taps held
    there as fp64 and `capacity` session slots; the definition is in the module docstring.

        cut = LowCut(22050, cutoff=70.0, capacity=8, device="cuda:0")
        y = cut(wavs, lengths)                   # one-shot: (rows, n_max) fp32, every row filtered from zero state
        s = cut.open()                           # a free slot (or open(slot) for a given one); starts from zero history
        out = cut.run({s: chunk})                # {slot: filtered chunk}; one device call for all slots
        cut.close(s)
    """

    def __init__(self, fs: int, cutoff: float = 70.0, capacity: int = 1, device="cuda") -> None:
        if not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer, not {capacity!r}")
        if not 0.0 < float(cutoff) < int(fs) // 2:
            raise ValueError(f"cutoff {cutoff!r} outside (0, fs / 2 = {int(fs) // 2})")
        from . import dsp
        self.fs, self.cutoff, self.capacity = int(fs), float(cutoff), capacity
        self.taps = np.ascontiguousarray(dsp.low_cut_taps(self.fs, self.cutoff), dtype=np.float64)
        self.n_taps = int(self.taps.size)
        if not 1 <= self.n_taps <= _lib.LOWCUT_MAX_TAPS:
            raise ValueError(f"{self.n_taps} taps, the device low cut takes 1 .. {_lib.LOWCUT_MAX_TAPS}")
        self.device = torch.device(device)
        self.state_floats = self.n_taps - 1
        self._taps = torch.from_numpy(self.taps).to(self.device)
        self._state = torch.zeros(max(1, capacity * self.state_floats), dtype=torch.float32, device=self.device)
        self._slots = _Slots(capacity, "low cut")
        self._free = self._slots.free
        self._reset = set()                                   # opened slots that have not run yet
        self._op = ops.lowcut_chunk_impl

    def _check_len(self, length: int) -> None:
        if length < 0:
            raise ValueError(f"length {length}")

    # ------------------------------------------------------------------ one shot
    def __call__(self, wavs, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
        """wavs as LogMelExtractor takes them (a padded (R, S) batch with `lengths`, one 1-D signal, or a list of 1-D signals)
        -> (R, max(lengths)) fp32 on the device: every row filtered from zero state, valid up to its length (the floats past
        it are not written).  One device call; the open sessions' slots are not touched."""
        batch, lens = _padded_batch(self, wavs, lengths)
        R = len(lens)
        state = torch.empty(max(1, R * self.state_floats), dtype=torch.float32, device=self.device)
        return self._op(self._taps, state, [batch[r, :lens[r]] for r in range(R)], list(range(R)), [True] * R, R)

    # ------------------------------------------------------------------ sessions
    def open(self, slot: Optional[int] = None) -> int:
        """claim a slot (the lowest free one when slot is None); its session starts from zero history."""
        slot = self._slots.open(slot)
        self._reset.add(slot)
        return slot

    def close(self, slot: int) -> None:
        """free the slot; a session opened in it later starts from zero history."""
        self._reset.discard(self._slots.close(slot))

    def run(self, chunks: Mapping[int, torch.Tensor]) -> Dict[int, torch.Tensor]:
        """the next chunk (1-D samples, host or device, any length) of each open slot's session, all in one device call ->
        {slot: filtered fp32 chunk (1-D, views of one dense output)}."""
        slots = [int(s) for s in chunks]
        for s in slots:
            self._slots.need_open(s)
        if not slots:
            return {}
        xs = [torch.as_tensor(chunks[s]) for s in chunks]
        for x in xs:
            if x.dim() != 1:
                raise ValueError(f"samples must be a 1-D tensor, got shape {tuple(x.shape)}")
        xs = [x.to(self.device, torch.float32) for x in xs]
        out = self._op(self._taps, self._state, xs, slots, [s in self._reset for s in slots], self.capacity)
        self._reset.difference_update(slots)
        return {s: out[e, :x.numel()] for e, (s, x) in enumerate(zip(slots, xs))}


def _check_low_cut(low_cut, extractor: "LogMelExtractor") -> None:
    if not isinstance(low_cut, LowCut):
        raise ValueError(f"low_cut must be a LowCut or None, not {low_cut!r}")
    if low_cut.device != extractor.device:
        raise ValueError(f"the low cut is on {low_cut.device}, the extractor on {extractor.device}")
    if low_cut.fs != int(extractor.fs):
        raise ValueError(f"the low cut was built for fs {low_cut.fs}, the extractor for {extractor.fs}")


# ---- rational resampler --------------------------------------------------------------------------------------------------
def resample_ratio(fs_in: int, fs_out: int) -> Tuple[int, int]:
    """(L, M) = (fs_out / g, fs_in / g), g = gcd(fs_in, fs_out): 48 000 -> 24 000 Hz is 1 / 2"""
    for name, fs in (("fs_in", fs_in), ("fs_out", fs_out)):
        if isinstance(fs, bool) or not isinstance(fs, (int, np.integer)) or fs < 1:
            raise ValueError(f"{name} must be a positive integer number of Hz, not {fs!r}")
    g = math.gcd(int(fs_in), int(fs_out))
    return int(fs_out) // g, int(fs_in) // g


def resample_taps(L: int, M: int, half_len: int = 10, beta: float = 5.0) -> np.ndarray:
    """the prototype filter in fp64: N = 2 * half_len * max(L, M) + 1 taps, L * firwin(N, 1 / max(L, M), ("kaiser", beta)) -
    with the defaults the filter `scipy.signal.resample_poly(x, L, M)` designs for itself"""
    from scipy.signal import firwin
    L, M, half_len = int(L), int(M), int(half_len)
    if L < 1 or M < 1 or half_len < 1:
        raise ValueError(f"L, M and half_len must be positive, got {L}, {M}, {half_len}")
    top = max(L, M)
    return L * firwin(2 * half_len * top + 1, 1.0 / top, window=("kaiser", float(beta)))


def resample_table(h, L: int) -> np.ndarray:
    """the polyphase table (L, Q = ceil(N / L)) in fp64: P[r][q] = h[r + q L], and 0.0 where r + q L >= N"""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    L = int(L)
    Q = -(-h.size // L)
    flat = np.zeros(Q * L, dtype=np.float64)
    flat[:h.size] = h
    return np.ascontiguousarray(flat.reshape(Q, L).T)


def resample_ready(L: int, M: int, n_taps: int, n_received: int, final: bool = False) -> int:
    """the streaming rule: outputs of a signal that can be computed once n_received inputs are there.  While it goes on, those
    whose newest input i0 = (n M + D) div L has arrived, D = (n_taps - 1) / 2; when it ends there (`final`), all
    ceil(n_received L / M): the last ones read the zeros past the end."""
    T = int(n_received)
    if final:
        return -(-T * L // M)
    a = T * L - 1 - (int(n_taps) - 1) // 2
    return 0 if a < 0 else a // M + 1


class Resampler:
    """the rational resampler fs_in -> fs_out on the device, with the polyphase table held there as fp64 and `capacity` session
    slots; the definition is in the module docstring.

        res = Resampler(48000, 22050, capacity=8, device="cuda:0")
        y = res(wavs, lengths)                   # one-shot: (rows, max outputs) fp32; row r holds res.out_count(lengths[r]) values
        s = res.open()                           # a free slot (or open(slot) for a given one); starts from zero history
        out = res.run({s: chunk})                # {slot: the outputs that became computable}; one device call for all slots
        out = res.run({}, finish=[s])            # ... the signal ends: the rest (a last chunk may come in the same call)
        res.close(s)
    """

    def __init__(self, fs_in: int, fs_out: int, capacity: int = 1, device="cuda", half_len: int = 10, beta: float = 5.0) -> None:
        if not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer, not {capacity!r}")
        self.L, self.M = resample_ratio(fs_in, fs_out)
        if fs_in == fs_out:
            raise ValueError(f"fs_in == fs_out == {fs_in}: there is nothing to resample (leave resample=None)")
        self.fs_in, self.fs_out, self.capacity = int(fs_in), int(fs_out), capacity
        self.taps = np.ascontiguousarray(resample_taps(self.L, self.M, half_len, beta), dtype=np.float64)
        self.n_taps = int(self.taps.size)
        self.delay = (self.n_taps - 1) // 2
        self.table = resample_table(self.taps, self.L)
        self.Q = int(self.table.shape[1])
        if int(_lib.lib().swn_resample_table_doubles(self.L, self.M, self.n_taps)) != self.table.size:
            raise ValueError(f"{fs_in} -> {fs_out} Hz is {self.L} / {self.M} with {self.n_taps} taps (Q = {self.Q}): the device "
                             f"resampler takes up <= {_lib.RESAMPLE_MAX_UP}, Q <= {_lib.RESAMPLE_MAX_Q}, n_taps <= "
                             f"{_lib.RESAMPLE_MAX_TAPS} and ceil({_lib.RESAMPLE_TILE} down / up) + Q <= {_lib.RESAMPLE_MAX_SPAN}")
        self.device = torch.device(device)
        self.state_floats = self.Q - 1
        self._table = torch.from_numpy(self.table.reshape(-1)).to(self.device)
        self._state = torch.zeros(max(1, capacity * self.state_floats), dtype=torch.float32, device=self.device)
        self._slots = _Slots(capacity, "resampler")
        self._free = self._slots.free
        self._at: Dict[int, List[int]] = {}                   # open slot -> [inputs received, outputs returned, ended]
        self._op = ops.resample_chunk_impl

    def _check_len(self, length: int) -> None:
        if length < 0:
            raise ValueError(f"length {length}")

    def ready(self, n_received: int, final: bool = False) -> int:
        """the streaming rule (resample_ready) of this resampler"""
        return resample_ready(self.L, self.M, self.n_taps, n_received, final)

    def out_count(self, length: int) -> int:
        """ceil(length L / M): the outputs of a signal of `length` inputs"""
        return self.ready(length, True)

    # ------------------------------------------------------------------ one shot
    def __call__(self, wavs, lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
        """wavs as LogMelExtractor takes them (a padded (R, S) batch with `lengths`, one 1-D signal, or a list of 1-D signals)
        -> (R, out_count(max(lengths))) fp32 on the device: every row resampled from zero state, valid up to out_count of its
        length (the floats past it are not written).  One device call; the open sessions' slots are not touched."""
        batch, lens = _padded_batch(self, wavs, lengths)
        R = len(lens)
        state = torch.empty(max(1, R * self.state_floats), dtype=torch.float32, device=self.device)
        return self._op(self._table, state, [batch[r, :lens[r]] for r in range(R)], list(range(R)), [0] * R, [0] * R,
                        [self.out_count(n) for n in lens], lens, self.L, self.M, self.n_taps, R, False)

    # ------------------------------------------------------------------ sessions
    def open(self, slot: Optional[int] = None) -> int:
        """claim a slot (the lowest free one when slot is None); its session starts from zero history."""
        slot = self._slots.open(slot)
        self._at[slot] = [0, 0, False]
        return slot

    def close(self, slot: int) -> None:
        """free the slot; a session opened in it later starts from zero history."""
        del self._at[self._slots.close(slot)]

    def run(self, chunks: Mapping[int, torch.Tensor], finish: Sequence[int] = ()) -> Dict[int, torch.Tensor]:
        """the next chunk (1-D samples at fs_in, host or device, any length) of each open slot's session, all in one device call
        -> {slot: the fp32 outputs at fs_out that became computable (1-D, views of one dense buffer), possibly none}.  The
        signals of the slots in `finish` end here (after their chunk of this call, if they have one): they receive all their
        remaining outputs, and take no samples afterwards."""
        ending = [int(s) for s in finish]
        if len(set(ending)) != len(ending):
            raise ValueError("a slot is named twice in finish")
        slots = [int(s) for s in chunks] + [s for s in ending if s not in {int(k) for k in chunks}]
        for s in slots:
            self._slots.need_open(s)
            if self._at[s][2]:
                raise RuntimeError(f"the signal of slot {s} has ended: no samples can be run after it finished")
        if not slots:
            return {}
        xs = [torch.as_tensor(c) for c in chunks.values()]
        for x in xs:
            if x.dim() != 1:
                raise ValueError(f"samples must be a 1-D tensor, got shape {tuple(x.shape)}")
        xs = [x.to(self.device, torch.float32) for x in xs]
        xs += [torch.zeros(0, dtype=torch.float32, device=self.device)] * (len(slots) - len(xs))
        in0s, out0s, n_outs, lens = [], [], [], []
        for s, x in zip(slots, xs):
            got, given, _ = self._at[s]
            end = got + int(x.numel())
            in0s.append(got)
            out0s.append(given)
            n_outs.append(self.ready(end, s in ending) - given)
            lens.append(end if s in ending else -1)
        out = self._op(self._table, self._state, xs, slots, in0s, out0s, n_outs, lens, self.L, self.M, self.n_taps, self.capacity,
                       True)
        res, at = {}, 0
        for s, x, k in zip(slots, xs, n_outs):
            self._at[s] = [self._at[s][0] + int(x.numel()), self._at[s][1] + k, s in ending]
            res[s] = out[at:at + k]
            at += k
        return res


def _check_resample(resample, low_cut, extractor: "LogMelExtractor") -> None:
    if not isinstance(resample, Resampler):
        raise ValueError(f"resample must be a Resampler or None, not {resample!r}")
    if resample.device != extractor.device:
        raise ValueError(f"the resampler is on {resample.device}, the extractor on {extractor.device}")
    if resample.fs_out != int(extractor.fs):
        raise ValueError(f"the resampler delivers fs {resample.fs_out}, the extractor was built for {extractor.fs}")
    if low_cut is not None and isinstance(low_cut, LowCut) and low_cut.fs != resample.fs_out:
        raise ValueError(f"the resampler delivers fs {resample.fs_out}, the low cut was built for {low_cut.fs}")


# ---- the streaming rule: the one place LogMelStream and LogMelPool take it from ------------------------------------------
def frames_ready(n_fft: int, hop: int, n_received: int, final: bool = False) -> int:
    """frames of a signal that can be computed once n_received samples are there.  While it goes on, those whose samples have
    all arrived: frame 0 reads up to sample n_fft / 2 (the left reflection), frame f >= 1 up to f hop + n_fft / 2 - 1.  When
    it ends there (`final`), all F = 1 + n_received // hop: the last ones read the reflected end."""
    if final:
        return frame_count(n_received, hop)
    half = n_fft // 2
    return 0 if n_received <= half else 1 + (n_received - half) // hop


def keep_from(n_fft: int, hop: int, t0: int, n_frames: int) -> int:
    """absolute index of the first sample a signal still needs after n_frames frames, when its buffer starts at t0: the next
    frame starts at n_frames hop - n_fft / 2; the reflected end of the last frame comes back to one sample before the start
    of a frame that begins exactly at the signal's end"""
    return max(t0, n_frames * hop - n_fft // 2 - 1)


class _FrameStream:
    """what LogMelStream, pitch.F0Stream and pitch.BapStream share: one signal's frames as its samples arrive.  `push` returns
    the frames that became computable, `finish` the rest; `_buf` holds the samples from the absolute index `t0` on, and after
    every call only the tail that later frames still read.  A subclass supplies `computable(n_received, final=False)`, its
    streaming rule, and `_keep()`, the absolute index of the first sample it still needs; `cols` is a frame's width and `more`
    what the extractor's `frames` takes after the range."""

    def __init__(self, extractor: _FrameExtractor, cols: int, *more) -> None:
        self.ext, self._cols, self._more = extractor, cols, more
        self._buf = torch.zeros(0, dtype=torch.float32, device=extractor.device)
        self.t0 = 0                 # absolute index of _buf[0]
        self.n_received = 0
        self.n_frames = 0           # frames returned so far
        self.finished = False

    def _take(self, s: torch.Tensor) -> None:
        self._buf = torch.cat([self._buf, s])
        self.n_received += int(s.numel())

    def _end(self) -> None:
        """what `finish` does before the last frames: the signal must be long enough"""
        self.ext._check_len(self.n_received)

    def _range(self, f1: int, length: int) -> torch.Tensor:
        f0 = self.n_frames
        if f1 > f0:
            out = self.ext.frames(self._buf, self.t0, int(self._buf.numel()), length, f0, f1, *self._more)
            self.n_frames = f1
        else:
            out = torch.zeros((0, self._cols), dtype=torch.float32, device=self.ext.device)
        keep = self._keep()
        if keep > self.t0:
            self._buf = self._buf[keep - self.t0:]
            self.t0 = keep
        return out

    def push(self, samples) -> torch.Tensor:
        """append 1-D samples -> (k, columns) new frames, k >= 0"""
        if self.finished:
            raise RuntimeError("the stream is finished")
        self._take(torch.as_tensor(samples).reshape(-1).to(self.ext.device, torch.float32))
        return self._range(self.computable(self.n_received), -1)

    def finish(self) -> torch.Tensor:
        """the signal ends here -> the remaining frames up to F = 1 + n_received // hop"""
        if self.finished:
            raise RuntimeError("the stream is finished")
        self._end()
        self.finished = True
        return self._range(self.computable(self.n_received, True), self.n_received)


class LogMelStream(_FrameStream):
    """one signal's features as its samples arrive: `push` returns the frames that became computable, `finish` the rest
    (those that read the reflected end).  Only the tail of the signal that later frames still read is kept.  The
    concatenation of everything returned is bit-identical to the extractor's one-shot call on the whole signal.  With
    `low_cut` (a LowCut) the pushed samples are RAW and every push filters them first, in a slot of the low cut that the
    stream opens for itself and frees when it finishes: the frames are the extractor's on low_cut(whole signal).  With
    `resample` (a Resampler whose fs_out is the extractor's fs) the pushed samples are at its fs_in and every push resamples
    them first, likewise in a slot of its own - resample, then low cut, then frames; `finish` flushes the resampler's last
    outputs through the low cut before the last frames: the frames are the extractor's on low_cut(resample(whole signal))."""

    def __init__(self, extractor: LogMelExtractor, linear: bool = False, low_cut: Optional[LowCut] = None,
                 resample: Optional[Resampler] = None) -> None:
        self.linear = bool(linear)
        self.low_cut, self._cut_slot = low_cut, None
        self.resample, self._res_slot = resample, None
        if low_cut is not None:
            _check_low_cut(low_cut, extractor)
        if resample is not None:
            _check_resample(resample, low_cut, extractor)
            self._res_slot = resample.open()
        if low_cut is not None:
            try:
                self._cut_slot = low_cut.open()
            except RuntimeError:
                if resample is not None:
                    resample.close(self._res_slot)
                raise
        super().__init__(extractor, extractor.n_mels, self.linear)

    def computable(self, n_received: int, final: bool = False) -> int:
        """frames whose samples have all arrived: frame 0 reads up to sample n_fft / 2 (the left reflection), frame
        f >= 1 up to f hop + n_fft / 2 - 1; with `final`, all of a signal that ends there"""
        return frames_ready(self.ext.n_fft, self.ext.hop, n_received, final)

    def _keep(self) -> int:
        return keep_from(self.ext.n_fft, self.ext.hop, self.t0, self.n_frames)

    def _take(self, s: torch.Tensor, resampled: bool = False) -> None:
        """pushed samples: through the resampler (unless they are its own last outputs) and the low cut, into the buffer"""
        if self.resample is not None and not resampled:
            s = self.resample.run({self._res_slot: s})[self._res_slot]
        if self.low_cut is not None:
            s = self.low_cut.run({self._cut_slot: s})[self._cut_slot]
        super()._take(s)

    def _end(self) -> None:
        if self.resample is not None:
            got, given, _ = self.resample._at[self._res_slot]
            self.ext._check_len(self.n_received + self.resample.ready(got, True) - given)
            self._take(self.resample.run({}, finish=[self._res_slot])[self._res_slot], resampled=True)
            self.resample.close(self._res_slot)
        super()._end()
        if self.low_cut is not None:
            self.low_cut.close(self._cut_slot)


# ---- many signals at once ------------------------------------------------------------------------------------------------
class MelPlanEntry(NamedTuple):
    """one session's share of a pool call, as swn_logmel_pool_entry states it (offsets are those of the call's buffers)"""
    key: object
    t0: int             # absolute index of the window's first sample before the call
    n_held: int         # samples in the window before the call
    n_drop: int         # of which the call discards this many from the front
    new_off: int
    n_new: int
    len: int            # the total length, or -1 while the signal goes on
    f0: int
    f1: int
    out_off: int
    out_stride: int


def plan_mel_push(sessions: Sequence[Tuple[object, int, int, int, int, int, bool]], n_fft: int, hop: int, n_mels: int,
                  limit: int = _lib.LOGMEL_POOL_MAX_ENTRIES) -> List[List[MelPlanEntry]]:
    """the calls of one batched push.  sessions: (key, t0, n_held, n_frames, n_received, n_new, finishing) of every session that
    is handed samples or ended, in the caller's order, where [t0, t0 + n_held) is what the session's window holds.  Each
    one's entry first drops what the frames returned so far no longer need (keep_from; LogMelStream drops it right after
    those frames, the window drops it at the start of its next call), appends the n_new samples, and computes the frames
    [n_frames, frames_ready(n_received + n_new, finishing)).  After the call the session stands at t0 + n_drop,
    n_held - n_drop + n_new, f1 and n_received + n_new.  The entries are split into calls of at most `limit`, offsets
    counted per call.  Pure host arithmetic: nothing here touches a device."""
    n_fft, hop, n_mels, limit = int(n_fft), int(hop), int(n_mels), int(limit)
    if limit < 1:
        raise ValueError(f"limit must be a positive integer, not {limit}")
    calls: List[List[MelPlanEntry]] = []
    for i in range(0, len(sessions), limit):
        entries, new_off, out_off = [], 0, 0
        for key, t0, n_held, n_frames, n_received, n_new, finishing in sessions[i:i + limit]:
            t0, n_held, n_frames, n_received, n_new = int(t0), int(n_held), int(n_frames), int(n_received), int(n_new)
            if min(t0, n_held, n_frames, n_received, n_new) < 0 or t0 + n_held != n_received:
                raise ValueError(f"session {key!r}: a window [{t0}, {t0} + {n_held}) does not end at the {n_received} samples received")
            after = n_received + n_new
            if finishing and after <= n_fft // 2:
                raise ValueError(f"session {key!r}: n_fft {n_fft} needs signals longer than {n_fft // 2} samples (reflect padding), "
                                 f"got {after}")
            n_drop = min(keep_from(n_fft, hop, t0, n_frames) - t0, n_held)
            f1 = max(n_frames, frames_ready(n_fft, hop, after, bool(finishing)))
            k = f1 - n_frames
            entries.append(MelPlanEntry(key, t0, n_held, n_drop, new_off, n_new, after if finishing else -1, n_frames, f1,
                                        out_off, k))
            new_off += n_new
            out_off += k * n_mels
        calls.append(entries)
    return calls


class MelSession:
    """one signal of a LogMelPool: `slot` is its window, n_received / n_frames / finished tell where it stands (as
    LogMelStream's do).  Made by LogMelPool.open."""

    def __init__(self, pool: "LogMelPool", slot: int) -> None:
        self._pool, self.slot = pool, slot
        self.t0 = 0                 # absolute index of the window's first sample
        self.n_held = 0             # samples in the window (what the next call no longer needs is dropped by that call)
        self.n_received = 0
        self.n_frames = 0           # frames returned so far
        self.n_in = 0               # with a resampler: samples at fs_in received so far (n_received counts those at the extractor's fs)
        self.finished = False
        self.closed = False


class LogMelPool:
    """many signals' features as their samples arrive, one call per tick: push_many gives every session what
    LogMelStream.push / finish would, bit for bit, with at most two launches and one staging copy per 64 sessions whatever
    their number.  The sessions' tails live in `windows` (capacity, n_fft + max_chunk) on the device: there is no
    per-session cat or slice, and the frames come back channel-major, (1, n_mels, k), as DecodePool.push_many,
    SteppedDecodePool.push_many and DecodeStream.push take them.  With `low_cut` (a LowCut) the chunks are RAW samples: the
    window update filters them (`torch.ops.swn.logmel_pool_lowcut`, still two launches per call) and every session's frames are
    the extractor's on low_cut(whole signal).  The pool owns `hist` (capacity, n_taps - 1), each window slot's last raw samples;
    a session opened in a freed slot starts from zero history.  The LowCut's own slots are not used.  With `resample` (a
    Resampler whose fs_out is the extractor's fs) the chunks are samples at its fs_in: one `torch.ops.swn.resample_staged` call
    per 64 sessions writes every session's newly computable samples straight into the buffer the pool call then takes as its
    staged new samples, and that call (with or without a low cut) follows unchanged - resample, then low cut, then frames.
    `max_chunk` stays in samples at the extractor's fs: a chunk that yields more is refused before any launch.  The pool owns
    `res_state` (capacity, Q - 1), each slot's last raw inputs; the Resampler's own slots are not used."""

    def __init__(self, extractor: LogMelExtractor, capacity: int, max_chunk: int, linear: bool = False,
                 low_cut: Optional[LowCut] = None, resample: Optional[Resampler] = None) -> None:
        if not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer, not {capacity!r}")
        if not isinstance(max_chunk, int) or max_chunk < 1:
            raise ValueError(f"max_chunk must be a positive integer, not {max_chunk!r}")
        self.ext, self.capacity, self.max_chunk, self.linear = extractor, capacity, max_chunk, bool(linear)
        floats = int(_lib.lib().swn_logmel_pool_window_floats(extractor.n_fft, max_chunk))
        if floats == 0:
            raise ValueError(f"no window for n_fft {extractor.n_fft} and chunks of {max_chunk} samples")
        self.windows = torch.zeros((capacity, floats), dtype=torch.float32, device=extractor.device)
        self._free = list(range(capacity))
        self._open: Dict[int, MelSession] = {}
        self._op = ops.logmel_pool_impl
        self.low_cut, self.hist = low_cut, None
        if low_cut is not None:
            _check_low_cut(low_cut, extractor)
            self.hist = torch.zeros((capacity, max(1, low_cut.n_taps - 1)), dtype=torch.float32, device=extractor.device)
            self._cut_op = ops.logmel_pool_lowcut_impl
        self.resample, self.res_state = resample, None
        if resample is not None:
            _check_resample(resample, low_cut, extractor)
            self.res_state = torch.zeros((capacity, max(1, resample.state_floats)), dtype=torch.float32, device=extractor.device)
            self._res_op = ops.resample_staged_impl

    def open(self) -> MelSession:
        """claim a free slot for a new signal (whatever the slot held before is never read)"""
        if not self._free:
            raise RuntimeError(f"the pool is full: all {self.capacity} slots hold open sessions")
        s = MelSession(self, self._free.pop(0))
        self._open[s.slot] = s
        return s

    def close(self, s: MelSession) -> None:
        """free the session's slot (finished or not)"""
        if not isinstance(s, MelSession) or s.closed or self._open.get(s.slot) is not s:
            raise RuntimeError("this session is not open in this pool")
        s.closed = True
        del self._open[s.slot]
        self._free.append(s.slot)
        self._free.sort()

    def _check(self, chunks, finish) -> List[Tuple[MelSession, Optional[torch.Tensor], bool]]:
        """(session, flat fp32 chunk or None, finishing) of a push_many call in its order; nothing is changed"""
        if not isinstance(chunks, dict):
            raise ValueError("chunks must map mel sessions to 1-D sample tensors")
        finish = list(finish)
        if len(set(map(id, finish))) != len(finish):
            raise ValueError("a session is named twice in finish")
        ending = set(map(id, finish))
        order = [(s, c, id(s) in ending) for s, c in chunks.items()] + [(s, None, True) for s in finish if s not in chunks]
        out = []
        for s, c, fin in order:
            if not isinstance(s, MelSession) or s.closed or self._open.get(s.slot) is not s:
                if isinstance(s, MelSession) and s._pool is self and s.closed:
                    raise RuntimeError(f"mel session of slot {s.slot} is closed")
                raise RuntimeError("this session is not open in this pool")
            if s.finished:
                raise RuntimeError(f"mel session of slot {s.slot} is finished: no samples can be pushed after it ended")
            if c is not None:
                c = torch.as_tensor(c)
                if c.dim() != 1:
                    raise ValueError(f"samples must be a 1-D tensor, got shape {tuple(c.shape)}")
                if self.resample is not None:
                    n = self._yield(s, c, fin)
                    if n > self.max_chunk:
                        raise ValueError(f"a chunk of {c.numel()} samples at {self.resample.fs_in} Hz yields {n} at "
                                         f"{self.resample.fs_out} Hz, the pool was built for at most {self.max_chunk}")
                elif c.numel() > self.max_chunk:
                    raise ValueError(f"a chunk of {c.numel()} samples, the pool was built for at most {self.max_chunk}")
                if c.dtype != torch.float32:
                    c = c.to(torch.float32)
            if fin:
                self.ext._check_len(s.n_received + (self._yield(s, c, fin) if self.resample is not None else
                                                    0 if c is None else c.numel()))
            out.append((s, c, fin))
        return out

    def _yield(self, s: MelSession, c: Optional[torch.Tensor], fin: bool) -> int:
        """with a resampler: the samples at the extractor's fs that chunk c (or the end of the signal) makes computable"""
        return self.resample.ready(s.n_in + (0 if c is None else c.numel()), fin) - s.n_received

    def _resampled(self, entries: List[MelPlanEntry], order) -> Optional[torch.Tensor]:
        """one resampler call for the sessions of a pool call: their chunks at fs_in, staged as usual, become the pool call's
        staged new samples - every entry's n_new outputs back to back in entry order, written there by the kernel"""
        res = self.resample
        raw = [order[e.key][1] for e in entries]
        counts = [0 if c is None else c.numel() for c in raw]
        if not any(counts) and not any(e.n_new for e in entries):
            return None
        sess = [order[e.key][0] for e in entries]
        out = self._res_op(res._table, self.res_state, self._stage([c for c in raw if c is not None]), counts,
                           [s.slot for s in sess], [s.n_in for s in sess], [s.n_received for s in sess],
                           [e.n_new for e in entries],
                           [s.n_in + n if order[e.key][2] else -1 for s, n, e in zip(sess, counts, entries)], res.L, res.M,
                           res.n_taps, self.capacity)
        return out if out.numel() else None

    def _stage(self, pieces: List[torch.Tensor]) -> Optional[torch.Tensor]:
        """the chunks of one call back to back in entry order, on the device: one host-to-device copy for the host chunks,
        one cat for the device chunks (as DecodePool._stage)"""
        flat = [c for c in pieces if c.numel() > 0]
        if not flat:
            return None
        dev = self.ext.device
        host = [i for i, c in enumerate(flat) if not c.is_cuda]
        if host:
            up = (flat[host[0]] if len(host) == 1 else torch.cat([flat[i] for i in host])).to(dev)
            if len(host) == len(flat):
                return up.contiguous()
            at = 0
            for i in host:
                n = flat[i].numel()
                flat[i] = up[at:at + n]
                at += n
        return flat[0].contiguous() if len(flat) == 1 else torch.cat(flat)

    def push_many(self, chunks: dict, finish: Sequence[MelSession] = ()) -> Dict[MelSession, torch.Tensor]:
        """one call for a whole tick of audio: push(chunk) for every session of `chunks` ({session: 1-D samples on the host or
        the device, 0 .. max_chunk of them}) and finish for every session of `finish` (which may also have a last chunk in
        `chunks`) -> {session: (1, n_mels, k) fp32 new frames on the device, k >= 0}, contiguous views of the calls' output
        buffers.  Per 64 sessions: one staging copy, one swn_logmel_pool (with a low cut: swn_logmel_pool_lowcut) call (two launches),
        with a resampler one swn_resample_chunk call (two launches) in front of it, whose chunks are at fs_in.  Everything is checked first and
        the counters move only after every call is enqueued: a call that raises leaves every session as it was."""
        order = self._check(chunks, finish)
        ext = self.ext
        if self.resample is not None:
            calls = plan_mel_push([(i, s.t0, s.n_held, s.n_frames, s.n_received, self._yield(s, c, fin), fin)
                                   for i, (s, c, fin) in enumerate(order)], ext.n_fft, ext.hop, ext.n_mels)
        else:
            calls = plan_mel_push([(i, s.t0, s.n_held, s.n_frames, s.n_received, 0 if c is None else c.numel(), fin)
                                   for i, (s, c, fin) in enumerate(order)], ext.n_fft, ext.hop, ext.n_mels)
        results: Dict[MelSession, torch.Tensor] = {}
        for entries in calls:
            if self.resample is not None:
                staged = self._resampled(entries, order)
            else:
                staged = self._stage([order[e.key][1] for e in entries if e.n_new > 0])
            if self.low_cut is None:
                out = self._op(self.windows, staged, ext._table, ext.bank, [order[e.key][0].slot for e in entries],
                               [e.t0 for e in entries], [e.n_held for e in entries], [e.n_drop for e in entries],
                               [e.n_new for e in entries], [e.len for e in entries], [e.f0 for e in entries],
                               [e.f1 for e in entries], ext.n_fft, ext.hop, ext.floor, self.linear)
            else:
                out = self._cut_op(self.windows, self.hist, staged, ext._table, ext.bank, self.low_cut._taps,
                                   [order[e.key][0].slot for e in entries], [e.t0 for e in entries],
                                   [e.n_held for e in entries], [e.n_drop for e in entries], [e.n_new for e in entries],
                                   [e.len for e in entries], [e.f0 for e in entries], [e.f1 for e in entries], ext.n_fft,
                                   ext.hop, ext.floor, self.linear)
            for e in entries:
                k = e.f1 - e.f0
                results[order[e.key][0]] = out[e.out_off:e.out_off + k * ext.n_mels].view(1, ext.n_mels, k)
        # every call has been enqueued: only now do the sessions move
        for entries in calls:
            for e in entries:
                s = order[e.key][0]
                s.t0, s.n_held = e.t0 + e.n_drop, e.n_held - e.n_drop + e.n_new
                s.n_received, s.n_frames = s.n_received + e.n_new, e.f1
        for s, c, fin in order:
            if self.resample is not None and c is not None:
                s.n_in += int(c.numel())
            if fin:
                s.finished = True
        return results
