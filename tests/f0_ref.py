"""numpy float64 reference of the F0 / voicing definition (swn_f0; include/swn_hip.h and pitch.py state it), and the cases the
tests of it share.  With W = win, L1 = lag_hi + 1, S = W + L1, x = 0 outside [0, len), frame f of F = 1 + len // hop reads
x[s .. s + S), s = f hop - S // 2:

    d(tau)  = sum_{j < W} (x[s + j] - x[s + j + tau])^2,  tau = 1 .. L1                 (the device: one fp64 fma chain, j ascending)
    c(tau)  = c(tau - 1) + d(tau), c(0) = 0;   d'(tau) = d(tau) tau / c(tau) if c(tau) > 0 else 1;   d'(0) = 1
    scan tau = lag_lo .. lag_hi; at the first d'(tau) < threshold walk while tau < lag_hi and d'(tau + 1) < d'(tau): voiced, lag tau*;
    else unvoiced, tau* = first arg-min of d' over [lag_lo, lag_hi]
    voiced: ym, y0, yp = d'(tau* - 1), d'(tau*), d'(tau* + 1); den = ym - 2 y0 + yp;
            shift = 0.5 (ym - yp) / den if den > 0 and y0 <= ym and y0 <= yp else 0;   f0 = fs / (tau* + shift)
    output [f0 or 0.0, d'(tau*)]

Here d is summed by numpy (pairwise, another order than the device's chain) and c by np.cumsum (the sequential order).  What the
comparison with the device needs comes back per frame: tau*, den, max(ym, y0, yp), whether the refinement was taken, and
whether the frame is DECISIVE.  The error scale of d' is

    eta(y) = (2 win + lag_hi + 8) 2^-53 y

derived, not fitted, as the distance of one evaluation from the exact value: d(tau) is a sum of W non-negative terms, each with
the rounding of its difference (twice, squared), of its square and of its addition - relative error at most (W + 2) 2^-53 in either
summation order; c(tau) adds at most lag_hi + 1 such values, all non-negative: (W + 2 + lag_hi) 2^-53; the product and the
quotient add one rounding each: (2 W + lag_hi + 6) 2^-53 y, which eta covers.  A comparison of a with b is decisive
when |a - b| > 4 eta(max(|a|, |b|)); a frame is decisive when every comparison the procedure made on it is: the threshold tests
up to the first hit (all of them on an unvoiced frame), every step of the walk and the test that ended it, the two guards of the
refinement, and den > 0 (|den| against 4 eta of the largest of ym, y0, yp).  On a decisive frame every evaluation within the
error scale takes the same branches, so the outputs can be compared value by value:

    |f0 - ref| <= 2^-24 ref (1 + 2^-20) + ref 6 eta(ymax) / (den tau_hat)         (the second term where the refinement is taken)
    |ap - ref| <= 2^-24 ref (1 + 2^-20) + 2 eta(ref)

  - of one evaluation, the numerator 0.5 (ym - yp) lies within eta(ymax) of the exact one and den within 4 eta(ymax); with
    |shift| <= 1/2 (the guards) its shift lies within (eta + 0.5 * 4 eta) / den = 3 eta(ymax) / den, to first order; the two sides
    being compared are each that far from the exact value, and f0 = fs / tau_hat moves by f0 / tau_hat times the shift's change;
  - the one rounding to fp32 is 2^-24 of the device's value, which is within (1 + 2^-20) of the reference's;
  - either side's aperiodicity lies within eta of the exact one; on an unvoiced frame it is the minimum of d' over the range, which
    moves by at most eta whichever lag attains it, so there the bound holds on non-decisive frames too."""
import functools

import numpy as np

MAX_HOP, MIN_WIN, MAX_WIN, MAX_LAG = 4096, 16, 2048, 1536


def lags(fs, minf0, maxf0):
    return int(np.floor(fs / maxf0)), int(np.ceil(fs / minf0))


def span(win, lag_hi):
    return win + lag_hi + 1


def frame_count(n, hop):
    return 1 + n // hop


def frames_ready_brute(hop, win, lag_hi, n_received, final):
    """the streaming rule, frame by frame"""
    if final:
        return 1 + n_received // hop
    S, f = span(win, lag_hi), 0
    while f * hop - S // 2 + S <= n_received:
        f += 1
    return f


def eta(win, lag_hi, y):
    return (2 * win + lag_hi + 8) * 2.0 ** -53 * np.abs(y)


def normalised_difference(x, hop, win, lag_hi, frames=None):
    """d' (n_frames, L1 + 1) in float64 for the frames `frames` (default: all) of the fp32 signal x"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, L1 = x.shape[0], lag_hi + 1
    S = win + L1
    frames = range(frame_count(n, hop)) if frames is None else frames
    out = np.ones((len(frames), L1 + 1), dtype=np.float64)
    taus = np.arange(1, L1 + 1, dtype=np.float64)
    for i, f in enumerate(frames):
        s = f * hop - S // 2
        seg = np.zeros(S, dtype=np.float64)
        lo, hi = max(s, 0), min(s + S, n)
        if hi > lo:
            seg[lo - s:hi - s] = x[lo:hi]
        w = np.lib.stride_tricks.sliding_window_view(seg, win)      # w[tau] = seg[tau : tau + W], tau = 0 .. L1
        diff = w[0][None, :] - w[1:]
        d = (diff * diff).sum(axis=1)
        c = np.cumsum(d)
        pos = c > 0
        out[i, 1:][pos] = d[pos] * taus[pos] / c[pos]
    return out


def decide(dp, fs, win, lag_lo, lag_hi, threshold):
    """one frame's d' (L1 + 1,) -> dict(f0, ap, voiced, tau, den, ymax, refined, decisive)"""
    e4 = lambda a, b: 4.0 * eta(win, lag_hi, max(abs(a), abs(b)))
    sure = lambda a, b: abs(a - b) > e4(a, b)
    decisive = True
    tau = None
    for t in range(lag_lo, lag_hi + 1):
        decisive &= sure(dp[t], threshold)
        if dp[t] < threshold:
            tau = t
            break
    if tau is None:
        seg = dp[lag_lo:lag_hi + 1]
        t = lag_lo + int(np.argmin(seg))
        return dict(f0=0.0, ap=float(dp[t]), voiced=False, tau=t, den=0.0, ymax=float(dp[t]), refined=False, decisive=bool(decisive))
    while tau < lag_hi:
        decisive &= sure(dp[tau + 1], dp[tau])
        if not dp[tau + 1] < dp[tau]:
            break
        tau += 1
    ym, y0, yp = float(dp[tau - 1]), float(dp[tau]), float(dp[tau + 1])
    den, ymax = ym - 2.0 * y0 + yp, max(ym, y0, yp)
    decisive &= sure(y0, ym) and sure(y0, yp) and abs(den) > 4.0 * eta(win, lag_hi, ymax)
    refined = den > 0.0 and y0 <= ym and y0 <= yp
    shift = 0.5 * (ym - yp) / den if refined else 0.0
    return dict(f0=fs / (tau + shift), ap=y0, voiced=True, tau=tau, den=den, ymax=ymax, refined=bool(refined), decisive=bool(decisive))


def analyse(x, fs, hop, win, lag_lo, lag_hi, threshold, frames=None):
    """the whole signal -> dict of per-frame arrays: f0, ap (float64), voiced, tau, den, ymax, refined, decisive"""
    dp = normalised_difference(x, hop, win, lag_hi, frames)
    rows = [decide(r, fs, win, lag_lo, lag_hi, threshold) for r in dp]
    keys = ("f0", "ap", "voiced", "tau", "den", "ymax", "refined", "decisive")
    return {k: np.array([r[k] for r in rows]) for k in keys}


def tau_hat_of(ref, fs):
    """tau* + shift of the voiced frames (fs / f0), 1 elsewhere"""
    return np.where(ref["voiced"], fs / np.where(ref["voiced"], ref["f0"], 1.0), 1.0)


def bounds(ref, fs, win, lag_hi):
    """(bound on |f0 - ref|, bound on |ap - ref|) per frame, as derived above"""
    f0, ap = ref["f0"], ref["ap"]
    bf = 2.0 ** -24 * f0 * (1.0 + 2.0 ** -20)
    r = ref["refined"] & ref["voiced"]
    th = tau_hat_of(ref, fs)
    bf[r] = bf[r] + f0[r] * 6.0 * eta(win, lag_hi, ref["ymax"][r]) / (ref["den"][r] * th[r])
    ba = 2.0 ** -24 * ap * (1.0 + 2.0 ** -20) + 2.0 * eta(win, lag_hi, ap)
    return bf, ba


# ---- the cases of tests/test_gpu_f0.py, which tests/test_f0_reference.py proves decisive ---------------------------------------
# (fs, hop, win, minf0, maxf0, n_long)
GEOMETRIES = [
    (8000, 40, 256, 60.0, 500.0, 3000),
    (8000, 37, 97, 100.0, 1000.0, 3000),         # odd window, a hop that divides nothing
    (16000, 80, 512, 50.0, 600.0, 3000),
    (22050, 110, 1024, 40.0, 700.0, 8000),       # the shipped one
    (8000, 1, 64, 200.0, 1000.0, 300),           # hop 1; S // 2 < win, as in every geometry here: a frame that holds any
                                                 # sample of the signal holds one in x[s .. s + W), so no d(tau) is exactly 0
                                                 # and no two d' tie exactly on signals of a few samples
    (8000, 600, 128, 80.0, 500.0, 3000),         # hop > S: the frames do not overlap
]
THRESHOLD = 0.1
SIGNALS = ("tone", "half-silent", "noise", "zeros", "glide")
# through the op with explicit lags: (fs, hop, win, lag_lo, lag_hi, n) - the edges of a lanes-over-lags loop and the limits
LAG_CASES = [(8000, 50, 128, 20, L1 - 1, 700) for L1 in (63, 64, 65, 255, 256, 257)] + [
    (22050, 512, 2048, 30, 1535, 6000),          # both limits
    (8000, 50, 128, 2, 100, 700),                # lag_lo = 2
    (8000, 50, 128, 66, 66, 700),                # lag_lo = lag_hi, near the tone's period
    (8000, 50, 16, 20, 100, 700),                # the smallest window
]


def lengths(hop, win, lag_hi, n_long):
    S = span(win, lag_hi)
    return [1, S // 2, S // 2 + 1, S - 1, S, S + 1, 15 * hop - 1, 16 * hop, 17 * hop + 3, n_long]


def signal(kind, n, fs, maxf0=700.0, seed=0):
    """float32 test signals: a harmonic tone (11 partials, 120 Hz, slow vibrato, weak noise), the same with its first half
    silent, white noise, zeros, and a two-partial glide that leaves the lag range at the top (0.5 maxf0 -> 1.5 maxf0)"""
    g = np.random.Generator(np.random.PCG64(4000 + seed))
    t = np.arange(n, dtype=np.float64) / fs
    if kind in ("tone", "half-silent"):
        phase = 2 * np.pi * (120.0 * t + 3.0 / (2 * np.pi * 4.0) * (1.0 - np.cos(2 * np.pi * 4.0 * t)))     # 120 Hz +- 3 Hz at 4 Hz
        x = sum(np.sin(k * phase + 0.3 * k) / k for k in range(1, 12)) * 0.2 + 0.002 * g.standard_normal(n)
        if kind == "half-silent":
            x[:n // 2] = 0.0
    elif kind == "noise":
        x = 0.3 * g.standard_normal(n)
    elif kind == "zeros":
        x = np.zeros(n)
    elif kind == "glide":
        f = maxf0 * (0.5 + np.arange(n) / max(n, 1))
        phase = 2 * np.pi * np.cumsum(f) / fs
        x = 0.4 * np.sin(phase) + 0.2 * np.sin(2 * phase + 0.5)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def geometry_case(gi):
    """geometry GEOMETRIES[gi] -> (params dict, list of (kind, n, signal, reference)): computed once per process"""
    fs, hop, win, minf0, maxf0, n_long = GEOMETRIES[gi]
    lo, hi = lags(fs, minf0, maxf0)
    rows = []
    for k, kind in enumerate(SIGNALS):
        for n in lengths(hop, win, hi, n_long):
            x = signal(kind, n, fs, maxf0, seed=10 * gi + k)
            rows.append((kind, n, x, analyse(x, fs, hop, win, lo, hi, THRESHOLD)))
    return dict(fs=fs, hop=hop, win=win, minf0=minf0, maxf0=maxf0, lag_lo=lo, lag_hi=hi), rows


@functools.lru_cache(maxsize=None)
def lag_case(ci):
    """LAG_CASES[ci] -> (params dict, list of (kind, n, signal, reference)) on the tone, the noise and the half-silent tone"""
    fs, hop, win, lo, hi, n = LAG_CASES[ci]
    rows = []
    for k, kind in enumerate(("tone", "noise", "half-silent")):
        x = signal(kind, n, fs, seed=100 + 10 * ci + k)
        rows.append((kind, n, x, analyse(x, fs, hop, win, lo, hi, THRESHOLD)))
    return dict(fs=fs, hop=hop, win=win, lag_lo=lo, lag_hi=hi), rows
