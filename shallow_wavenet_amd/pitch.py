"""F0 and voicing from waveforms on the device (`torch.ops.swn.f0`, csrc/swn_f0.hip): the contour the reference's features start
with - `[uv, log F0 (continuous, smoothed), ...]` - without WORLD, by a fully pinned definition of its own.

    ext = F0Extractor(fs=22050, hop=110, minf0=40, maxf0=700, device="cuda:0")
    f0ap = ext(wavs, lengths)                  # (R, F_max, 2): [F0 in Hz or 0.0 when unvoiced, aperiodicity]; zero past a row's frames
    stream = F0Stream(ext)                     # the same frames, as the samples arrive
    new = stream.push(chunk); ...; last = stream.finish()
    cond = uv_lf0(f0ap[0, :F, 0].cpu().numpy(), frame_rate=200)     # (F, 2): [uv, log of the bridged, smoothed F0] on the host

Definition (the contract; include/swn_hip.h and csrc/swn_f0.hip restate it, tests/f0_ref.py pins it).  Parameters: `fs` > 0;
`hop` in 1 .. 4096; `win` = W in 16 .. 2048, any integer; lags 2 <= lag_lo <= lag_hi <= 1535, which `f0_lags` derives from Hz as
lag_lo = floor(fs / maxf0), lag_hi = ceil(fs / minf0); `threshold` in (0, 1].  With L1 = lag_hi + 1 a frame spans S = W + L1
samples.  Input samples are fp32 and finite, len >= 1 of them; outside [0, len) x[t] = 0: the padding is zeros, not reflection.
  * Frames: F = 1 + len // hop, the grid of the log-mel features.  Frame f reads x[s .. s + S) with s = f * hop - S // 2.
  * Difference function: for tau = 1 .. L1, in fp64, one chain over j = 0 .. W - 1 ascending from acc = +0.0:
    diff = (double)x[s + j] - (double)x[s + j + tau]; acc = fma(diff, diff, acc); d(tau) = acc.
  * Cumulative mean normalisation: c(0) = 0, c(tau) = c(tau - 1) + d(tau) strictly in this order; d'(tau) = (d(tau) * tau) / c(tau)
    if c(tau) > 0, else 1.0; d'(0) = 1.
  * Decision: scan tau = lag_lo .. lag_hi ascending; at the first tau with d'(tau) < threshold walk to the local minimum (while
    tau < lag_hi and d'(tau + 1) < d'(tau): tau += 1); the frame is voiced with lag tau*.  If no tau is below the threshold the frame
    is unvoiced and tau* is the first arg-min of d' over [lag_lo, lag_hi].
  * Refinement (voiced frames): ym, y0, yp = d'(tau* - 1), d'(tau*), d'(tau* + 1); den = ym - 2 y0 + yp; shift = 0.5 (ym - yp) / den
    if den > 0 and y0 <= ym and y0 <= yp, else 0; f0 = fs / (tau* + shift).
  * Output, fp32, each value rounded once: [0] = F0 in Hz, exactly 0.0 when unvoiced; [1] = d'(tau*), the aperiodicity (1.0 on
    silence).
A frame's two values depend on the signal and the frame index alone - not on the batch, the frame range, the buffer window or
the call - so the stream's concatenated output is bit-identical to the one-shot call.  Streaming rule (`f0_frames_ready`, the one
place it is written): while the signal goes on, frame f is computable iff f * hop - S // 2 + S <= n_received; when it ends, all
1 + n_received // hop frames are.  The latency is S - S // 2 samples (n_fft / 2 for the log-mel features): 789 samples, 36 ms, at
the shipped geometry (22 050 Hz, win 1024, 40 Hz).  There is no torch fall-back: without the library the call raises.

This is the difference-function estimator of de Cheveigne and Kawahara (YIN, 2002) in a fixed arithmetic, not WORLD's Harvest:
parity with Harvest is not claimed and not pinned.  Out of scope here: a pool variant (one call per tick for many sessions),
`low_cut=` and `resample=` arguments on the streams (compose them with `Resampler.run` / `LowCut.run`), and any smoothing or
octave correction of the contour on the device (`uv_lf0` bridges and smooths on the host, with dsp.py's helpers).

Band aperiodicity (`torch.ops.swn.bap`, swn_bap in the same file) adds the reference's `codeap` columns to those two:

    ext = BandAperiodicityExtractor(fs=22050, hop=110, device="cuda:0")       # bands bap_bands(fs), 255 taps, band_win 256
    f = ext(wavs, lengths)                     # (R, F_max, 2 + B): [F0, aperiodicity, coded aperiodicity of band 0 .. B - 1 in dB]
    stream = BapStream(ext)                    # the same frames as the samples arrive, (n_taps - 1) / 2 samples later than F0Stream's

Its definition, limits and streaming rule (`bap_frames_ready`) are in BandAperiodicityExtractor's docstring; it is this project's
own measure, not WORLD's D4C / `code_aperiodicity`, and parity with them is neither claimed nor pinned."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, dsp, ops
from .melspec import _FrameExtractor, _FrameStream, frame_count


def f0_lags(fs: float, minf0: float, maxf0: float) -> Tuple[int, int]:
    """(lag_lo, lag_hi) = (floor(fs / maxf0), ceil(fs / minf0)); ValueError where swn_f0 would refuse them"""
    if not (fs > 0 and 0 < minf0 <= maxf0):
        raise ValueError(f"need fs > 0 and 0 < minf0 <= maxf0, got fs {fs}, minf0 {minf0}, maxf0 {maxf0}")
    lo, hi = int(math.floor(fs / maxf0)), int(math.ceil(fs / minf0))
    if not 2 <= lo <= hi <= _lib.F0_MAX_LAG - 1:
        raise ValueError(f"fs {fs}, minf0 {minf0}, maxf0 {maxf0} give the lags [{lo}, {hi}]: need 2 <= lag_lo <= lag_hi <= "
                         f"{_lib.F0_MAX_LAG - 1}")
    return lo, hi


def f0_span(win: int, lag_hi: int) -> int:
    """S = win + lag_hi + 1, the samples a frame reads"""
    return int(win) + int(lag_hi) + 1


def f0_frames_ready(hop: int, win: int, lag_hi: int, n_received: int, final: bool = False) -> int:
    """frames of a signal that can be computed once n_received samples are there.  While it goes on, frame f is computable iff
    f * hop - S // 2 + S <= n_received; when it ends there (`final`), all F = 1 + n_received // hop (the rest is zeros)."""
    if final:
        return frame_count(n_received, hop)
    S = f0_span(win, lag_hi)
    ahead = S - S // 2
    return 0 if n_received < ahead else 1 + (n_received - ahead) // hop


class F0Extractor(_FrameExtractor):
    """holds the geometry; a call computes [F0, aperiodicity] of every frame of a batch of waveforms on `device`: (R, F_max, 2),
    and `frames` those of a range from a partial buffer."""

    def __init__(self, fs: float, hop: int, minf0: float = 40.0, maxf0: float = 700.0, win: int = 1024, threshold: float = 0.1,
                 device="cuda") -> None:
        self.fs, self.hop, self.win, self.threshold = float(fs), int(hop), int(win), float(threshold)
        self.minf0, self.maxf0 = float(minf0), float(maxf0)
        self.lag_lo, self.lag_hi = f0_lags(self.fs, self.minf0, self.maxf0)
        if not 1 <= self.hop <= _lib.F0_MAX_HOP:
            raise ValueError(f"hop {hop} outside [1, {_lib.F0_MAX_HOP}]")
        if not _lib.F0_MIN_WIN <= self.win <= _lib.F0_MAX_WIN:
            raise ValueError(f"win {win} outside [{_lib.F0_MIN_WIN}, {_lib.F0_MAX_WIN}]")
        if not 0.0 < self.threshold <= 1.0:
            raise ValueError(f"threshold {threshold} outside (0, 1]")
        self.span = f0_span(self.win, self.lag_hi)
        self.device = torch.device(device)
        self._op = ops.f0_impl

    def _check_len(self, length: int) -> None:
        if length < 1:
            raise ValueError(f"a signal needs at least one sample, got {length}")

    def _run(self, buf, t0s, n_avails, lens, f0s, f1s) -> torch.Tensor:
        return self._op(buf, t0s, n_avails, lens, f0s, f1s, self.fs, self.hop, self.win, self.lag_lo, self.lag_hi, self.threshold)


class F0Stream(_FrameStream):
    """one signal's [F0, aperiodicity] frames as its samples arrive: `push` returns the frames that became computable, `finish`
    the rest (those that read the zeros past the end).  Only the tail of the signal that later frames still read is kept.  The
    concatenation of everything returned is bit-identical to the extractor's one-shot call on the whole signal.  The samples are
    at the extractor's rate, already filtered: a caller that has raw audio at another rate runs `Resampler.run` and `LowCut.run`
    on each chunk first."""

    def __init__(self, extractor: F0Extractor) -> None:
        super().__init__(extractor, 2)
        self._behind = extractor.span // 2      # samples a frame reads before f * hop

    def computable(self, n_received: int, final: bool = False) -> int:
        return f0_frames_ready(self.ext.hop, self.ext.win, self.ext.lag_hi, n_received, final)

    def _keep(self) -> int:
        # the next frame's first sample; with hop > S it may not have arrived yet
        return min(self.n_received, max(self.t0, self.n_frames * self.ext.hop - self._behind))


# ---- band aperiodicity: the reference's `codeap` columns ------------------------------------------------------------------------
BAP_FLOOR = 1e-6


def bap_bands(fs: float) -> List[Tuple[float, float]]:
    """the band edges in Hz, one band per coded aperiodicity of the reference at this rate: B = floor(min(15000, fs / 2 - 3000) /
    3000) bands (2 at 22.05 kHz, 1 at 16 kHz, 3 at 24 kHz, 5 at 44.1 / 48 kHz, none at 8 kHz - so 2 + B is run.sh's `stdim`), band
    b spanning 3000 b + 1500 .. 3000 b + 4500 Hz around the reference's coding frequencies 3000 (b + 1)"""
    n = int(math.floor(min(15000.0, fs / 2.0 - 3000.0) / 3000.0))
    return [(3000.0 * b + 1500.0, 3000.0 * b + 4500.0) for b in range(max(n, 0))]


def bap_taps(fs: float, bands: Sequence[Tuple[float, float]], n_taps: int = 255) -> np.ndarray:
    """(B, n_taps) float64: one linear-phase band-pass (scipy.signal.firwin, Hamming) per (lo, hi) band in Hz"""
    from scipy.signal import firwin
    if n_taps < 1 or n_taps > _lib.BAP_MAX_TAPS or n_taps % 2 == 0:
        raise ValueError(f"n_taps {n_taps}: need an odd count in 1 .. {_lib.BAP_MAX_TAPS}")
    rows = []
    for lo, hi in bands:
        if not 0.0 < lo < hi < fs / 2.0:
            raise ValueError(f"band ({lo}, {hi}) Hz: need 0 < lo < hi < fs / 2 = {fs / 2.0}")
        rows.append(firwin(n_taps, [lo, hi], pass_zero=False, fs=fs))
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(len(rows), n_taps))


def bap_reach(win: int, lag_hi: int, n_taps: int) -> int:
    """S + 2 c, the samples a frame reads"""
    return f0_span(win, lag_hi) + int(n_taps) - 1


def bap_frames_ready(hop: int, win: int, lag_hi: int, n_taps: int, n_received: int, final: bool = False) -> int:
    """frames of a signal that can be computed once n_received samples are there.  While it goes on, frame f is computable iff
    f * hop - S // 2 + S + c <= n_received, c = (n_taps - 1) // 2; when it ends there (`final`), all F = 1 + n_received // hop."""
    if final:
        return frame_count(n_received, hop)
    S = f0_span(win, lag_hi)
    ahead = S - S // 2 + (int(n_taps) - 1) // 2
    return 0 if n_received < ahead else 1 + (n_received - ahead) // hop


class BandAperiodicityExtractor(F0Extractor):
    """[F0, aperiodicity, coded aperiodicity of B bands in dB] of every frame (`torch.ops.swn.bap`, swn_bap): the F0 columns have
    F0Extractor's bits, column 2 + b is 10 log10 of how far band b is from periodic at the frame's decided lag, clamped to
    [floor, 1] (<= 0 dB), exactly 0.0 on unvoiced frames - the counterpart of the reference's `codeap` columns.

    Definition (the contract; include/swn_hip.h states it in full, tests/bap_ref.py pins it).  With F0's W, L1, S, s = f hop -
    S // 2 and the frame's decided lag tau*: B filters of T odd fp64 taps h_b, c = (T - 1) / 2; y_b[t] = sum_k h_b[k] x[t + c - k]
    (one fp64 fma chain, k ascending; x = 0 outside the signal); s_b = f hop - (Wb + tau*) // 2; over j < Wb: d = sum (y_b[s_b + j]
    - y_b[s_b + j + tau*])^2, e0 = sum y_b[s_b + j]^2, e1 = sum y_b[s_b + j + tau*]^2, each as 64 interleaved fma chains added in
    order; ap = d / (e0 + e1), or 1.0 when that is 0; coded 10 log10(min(max(ap, floor), 1)).  A frame reads x[s - c .. s + S + c).
    Frames are bit-identical under any batch, frame range, window or chunking.  The latency is S - S // 2 + c samples: 916
    samples, 41.5 ms, at the shipped geometry with 255 taps.

    This is not WORLD's D4C nor its `code_aperiodicity`: parity with them is neither claimed nor pinned.  Known limits: tau* is
    an integer lag, so a band around frequency nu cannot go below about 1 - cos(pi nu / fs) for a period that falls between two
    lags, and vibrato inside the window raises the value further (a shorter `band_win` recovers some of that: the default is 256).

    `bands`: (lo, hi) edges in Hz, default `bap_bands(fs)` (ValueError when that is empty: below 12 kHz the reference codes no
    band); `taps`: an explicit (B, T) float64 table instead of `bands` / `n_taps`; `band_win` is clipped to `win`."""

    def __init__(self, fs: float, hop: int, minf0: float = 40.0, maxf0: float = 700.0, win: int = 1024, threshold: float = 0.1,
                 bands: Optional[Sequence[Tuple[float, float]]] = None, n_taps: int = 255, band_win: int = 256,
                 floor: float = BAP_FLOOR, device="cuda", taps=None) -> None:
        super().__init__(fs, hop, minf0, maxf0, win, threshold, device)
        if taps is None:
            self.bands = list(bap_bands(self.fs) if bands is None else bands)
            if not self.bands:
                raise ValueError(f"no aperiodicity band at fs {fs}: pass `bands`")
            taps = bap_taps(self.fs, self.bands, n_taps)
        else:
            self.bands = None
        table = np.ascontiguousarray(np.asarray(taps, dtype=np.float64))
        if table.ndim != 2 or not 1 <= table.shape[0] <= _lib.BAP_MAX_BANDS:
            raise ValueError(f"taps of shape {table.shape}: need (B, T) with 1 <= B <= {_lib.BAP_MAX_BANDS}")
        if not (1 <= table.shape[1] <= _lib.BAP_MAX_TAPS and table.shape[1] % 2 == 1):
            raise ValueError(f"{table.shape[1]} taps: need an odd count in 1 .. {_lib.BAP_MAX_TAPS}")
        if not 0.0 < float(floor) < 1.0:
            raise ValueError(f"floor {floor} outside (0, 1)")
        if int(band_win) < _lib.F0_MIN_WIN:
            raise ValueError(f"band_win {band_win} below {_lib.F0_MIN_WIN}")
        self.n_bands, self.n_taps = int(table.shape[0]), int(table.shape[1])
        self.band_win, self.floor = min(int(band_win), self.win), float(floor)
        self.reach = bap_reach(self.win, self.lag_hi, self.n_taps)
        self.taps = torch.from_numpy(table).to(self.device)
        self._op = ops.bap_impl

    def _run(self, buf, t0s, n_avails, lens, f0s, f1s) -> torch.Tensor:
        return self._op(buf, self.taps, t0s, n_avails, lens, f0s, f1s, self.fs, self.hop, self.win, self.lag_lo, self.lag_hi,
                        self.threshold, self.band_win, self.floor)


class BapStream(F0Stream):
    """F0Stream for a BandAperiodicityExtractor: frames of 2 + B values, each c = (n_taps - 1) // 2 samples later than F0's, and
    a tail that starts c samples earlier: at n_frames * hop - S // 2 - c."""

    def __init__(self, extractor: BandAperiodicityExtractor) -> None:
        super().__init__(extractor)
        self._behind = extractor.span // 2 + (extractor.n_taps - 1) // 2
        self._cols = 2 + extractor.n_bands

    def computable(self, n_received: int, final: bool = False) -> int:
        return bap_frames_ready(self.ext.hop, self.ext.win, self.ext.lag_hi, self.ext.n_taps, n_received, final)


def uv_lf0(f0_column, frame_rate: int) -> np.ndarray:
    """(F,) F0 in Hz with 0.0 on unvoiced frames -> (F, 2) float64 [uv, log(low_pass_filter(continuous_f0(f0), frame_rate, 20))]:
    the first two columns of the reference's feature layout, by the helpers of dsp.py (feature_extract.py:296-305).  ValueError
    when no frame is voiced."""
    f0 = np.asarray(f0_column, dtype=np.float64).reshape(-1)
    uv, cont = dsp.continuous_f0(f0)
    lf0 = np.log(dsp.low_pass_filter(cont, int(frame_rate), cutoff=20))
    return np.stack([uv.astype(np.float64), lf0], axis=1)
