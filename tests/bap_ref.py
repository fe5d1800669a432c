"""numpy float64 reference of the band aperiodicity definition (swn_bap; include/swn_hip.h and pitch.py state it), and the cases
the tests of it share.  Everything about F0 is f0_ref's: W = win, L1 = lag_hi + 1, S = W + L1, x = 0 outside [0, len), frame f of
F = 1 + len // hop at s = f hop - S // 2, its decided lag tau*, its voicing decision and whether it is decisive come from
f0_ref.analyse.  With B filters of T odd taps h_b, c = (T - 1) / 2, a sum window Wb and a floor:

    y_b[t]  = sum_k h_b[k] x[t + c - k]                                        (the device: one fp64 fma chain, k ascending)
    s_b     = f hop - (Wb + tau*) // 2
    d       = sum_{j < Wb} (y_b[s_b + j] - y_b[s_b + j + tau*])^2,   e0 = sum y_b[s_b + j]^2,   e1 = sum y_b[s_b + j + tau*]^2
                                                                               (the device: 64 interleaved fma chains, added in order)
    ap      = d / (e0 + e1) if e0 + e1 > 0 else 1.0
    coded   = 10 log10(min(max(ap, floor), 1.0)) on voiced frames, exactly 0.0 on unvoiced ones

Here y_b is a direct convolution (np.convolve: one dot product per sample, no FFT) and the sums are numpy's (pairwise).

The bound on |coded - ref| is derived, not fitted.  Take either side (the device or this file) and call `exact` the value in real
arithmetic on the fp32 samples and the fp64 taps.
  - y: a sum of T products in any order is within (T + 1) 2^-53 sum_k |h_b[k]| |x[t + c - k]| = eps_y[t] of the exact one (one
    rounding per product, at most T - 1 per partial sum, first order; an fma chain has fewer).
  - the sums: the vector of the Wb differences is off by at most eps_y[j] + eps_y[j + tau*] per element, so by at most
    r = 2 sqrt(Wb) max eps_y in norm (the maximum over the samples the frame reads); d is its squared norm, so it moves by at most
    2 sqrt(d) r + r^2, and summing Wb non-negative terms, each with the roundings of its difference (twice, squared), its square
    and its addition, adds at most (Wb + 3) 2^-53 d in either order:  |delta d| <= 2 sqrt(d) r + r^2 + (Wb + 3) 2^-53 d.
    e0 and e1 are squared norms of vectors that are off by at most r / 2 < r: the same form bounds them, and e = e0 + e1 adds one
    rounding:  |delta e| <= |delta e0| + |delta e1| + 2^-53 e.
  - the ratio: |delta ap| <= (|delta d| + ap |delta e|) / (e - |delta e|) + 2^-53 ap  (infinite when e <= |delta e|).
  - both sides are that far from the exact value, so they are at most gap = 2 |delta ap| apart.
  - the code: x -> 10 log10(min(max(x, floor), 1)) is monotone, so both sides' coded values lie between lo = code(ap - gap) and
    hi = code(ap + gap) - the two clamps need no cases -; the fp64 log10 is within a few units of its last place: 4 2^-53 |value|
    on either side; the one rounding to fp32 is 2^-24 |value| (1 + 2^-20).  With |value| <= |lo| (the values are <= 0):
        bound = max(hi - ref, ref - lo) + |lo| (8 2^-53 + 2^-24 (1 + 2^-20))
The comparison applies on frames that are decisive for F0 (there both sides have the same tau* and the same voicing); e > 0 needs
no decisiveness: e is exactly 0 on both sides iff every sample the frame reaches is 0 (then ap = 1.0 and the code is 0.0).  At
most 1 % of a case's frames may be non-decisive; tests/test_bap_reference.py shows on the CPU that none of the cases below has
any."""
import functools

import numpy as np
from scipy.signal import firwin

import f0_ref

MAX_BANDS, MAX_TAPS, TILE = 5, 255, 1280
FLOOR = 1e-6
U = 2.0 ** -53


def bands(fs):
    """the reference's band count, floor(min(15000, fs / 2 - 3000) / 3000), as (lo, hi) edges in Hz"""
    n = int(np.floor(min(15000.0, fs / 2.0 - 3000.0) / 3000.0))
    return [(3000.0 * b + 1500.0, 3000.0 * b + 4500.0) for b in range(max(n, 0))]


def taps(fs, edges, n_taps):
    return np.stack([firwin(n_taps, [lo, hi], pass_zero=False, fs=fs) for lo, hi in edges]).astype(np.float64)


def reach(win, lag_hi, n_taps):
    return f0_ref.span(win, lag_hi) + n_taps - 1


def frames_ready_brute(hop, win, lag_hi, n_taps, n_received, final):
    """the streaming rule, frame by frame"""
    if final:
        return 1 + n_received // hop
    S, c, f = f0_ref.span(win, lag_hi), (n_taps - 1) // 2, 0
    while f * hop - S // 2 + S + c <= n_received:
        f += 1
    return f


def band_signals(x, h, lo, hi):
    """(y, eps_y) of shape (B, hi - lo): y_b[t] and its error scale for t = lo .. hi - 1, x (fp32) zero outside [0, len)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    B, T = h.shape
    c = (T - 1) // 2
    xp = np.zeros(hi - lo + 2 * c, dtype=np.float64)            # x[lo - c .. hi + c)
    a, b = max(lo - c, 0), min(hi + c, x.shape[0])
    if b > a:
        xp[a - (lo - c):b - (lo - c)] = x[a:b]
    y = np.stack([np.convolve(xp, h[k], mode="valid") for k in range(B)])
    eps = np.stack([np.convolve(np.abs(xp), np.abs(h[k]), mode="valid") for k in range(B)]) * ((T + 1) * U)
    return y, eps


def code(ap, floor):
    return 10.0 * np.log10(np.minimum(np.maximum(ap, floor), 1.0))


def analyse(x, h, fs, hop, win, lag_lo, lag_hi, threshold, band_win, floor=FLOOR, frames=None):
    """the whole signal -> f0_ref.analyse's dict plus, per frame and band (F, B): d, e0, e1, ap, coded and bound"""
    ref = dict(f0_ref.analyse(x, fs, hop, win, lag_lo, lag_hi, threshold, frames))
    n, S, Wb = len(x), f0_ref.span(win, lag_hi), band_win
    B = h.shape[0]
    fl = float(np.float32(floor))
    frames = list(range(f0_ref.frame_count(n, hop)) if frames is None else frames)
    lo, hi = frames[0] * hop - S // 2, frames[-1] * hop - S // 2 + S
    y, eps = band_signals(x, h, lo, hi)
    F = len(frames)
    out = {k: np.zeros((F, B)) for k in ("d", "e0", "e1", "ap", "coded", "bound")}
    for i, f in enumerate(frames):
        tau = int(ref["tau"][i])
        at = f * hop - (Wb + tau) // 2 - lo
        assert 0 <= f * hop - S // 2 - lo <= at and at + tau + Wb <= f * hop - S // 2 + S - lo
        y0, y1 = y[:, at:at + Wb], y[:, at + tau:at + tau + Wb]
        diff = y0 - y1
        d, e0, e1 = (diff * diff).sum(axis=1), (y0 * y0).sum(axis=1), (y1 * y1).sum(axis=1)
        e = e0 + e1
        pos = e > 0
        ap = np.where(pos, d / np.where(pos, e, 1.0), 1.0)
        r = 2.0 * np.sqrt(Wb) * eps[:, at:at + tau + Wb].max(axis=1)
        dd, de0, de1 = (2.0 * np.sqrt(v) * r + r * r + (Wb + 3) * U * v for v in (d, e0, e1))
        de = de0 + de1 + U * e
        with np.errstate(divide="ignore", invalid="ignore"):
            dap = np.where(e > de, (dd + ap * de) / np.where(e > de, e - de, 1.0) + U * ap, np.inf)
        dap = np.where(pos, dap, 0.0)                               # e is exactly 0 on both sides
        gap = 2.0 * dap
        if ref["voiced"][i]:
            coded, c_lo, c_hi = code(ap, fl), code(ap - gap, fl), code(ap + gap, fl)
        else:
            coded = c_lo = c_hi = np.zeros(B)
        bound = np.maximum(c_hi - coded, coded - c_lo) + np.abs(c_lo) * (8.0 * U + 2.0 ** -24 * (1.0 + 2.0 ** -20))
        for k, v in (("d", d), ("e0", e0), ("e1", e1), ("ap", ap), ("coded", coded), ("bound", bound)):
            out[k][i] = v
    ref.update(out)
    return ref


# ---- the cases of tests/test_gpu_bap.py, which tests/test_bap_reference.py proves decisive ---------------------------------------
THRESHOLD = f0_ref.THRESHOLD
# (fs, hop, win, minf0, maxf0, n_long) as f0_ref.GEOMETRIES, then the band edges in Hz (None: one identity tap), T, Wb
GEOMETRIES = [
    ((8000, 37, 97, 100.0, 1000.0, 3000), [(500.0, 1500.0), (1500.0, 3000.0)], 31, 97),
    ((8000, 40, 256, 60.0, 500.0, 3000), None, 1, 16),
    ((16000, 80, 512, 50.0, 600.0, 3000), bands(16000), 255, 255),          # Wb odd, no multiple of 64
    ((22050, 110, 1024, 40.0, 700.0, 8000), bands(22050), 255, 256),        # the shipped one, the defaults
    ((8000, 600, 128, 80.0, 500.0, 3000), [(300.0, 900.0), (900.0, 1500.0), (1500.0, 2100.0), (2100.0, 2700.0), (2700.0, 3500.0)],
     63, 64),                                                               # hop > reach: the frames do not overlap
    ((8000, 1, 64, 200.0, 1000.0, 300), [(1000.0, 3000.0)], 3, 64),
]
SIGNALS = f0_ref.SIGNALS + ("rich", "rich-noisy", "rich-steady")
# the edges of the 64 partial chains: Wb on one geometry - (geometry index, edges, T, Wb values, n)
WB_GEOMETRY, WB_EDGES, WB_TAPS, WB_VALUES, WB_N = 1, [(500.0, 1500.0), (1500.0, 3000.0)], 31, (63, 64, 65, 129), 2000


def geometry_taps(gi):
    (fs, *_), edges, T, _ = GEOMETRIES[gi]
    return np.ones((1, 1)) if edges is None else taps(fs, edges, T)


def lengths(hop, win, lag_hi, n_long, n_taps):
    """f0_ref's lengths, the first length whose frame 0 is inside the signal with its halo, and - where the hop allows it - the
    lengths whose band-pass region (F - 1) hop + S is TILE - 1, TILE and TILE + 1 samples"""
    S, c = f0_ref.span(win, lag_hi), (n_taps - 1) // 2
    out = f0_ref.lengths(hop, win, lag_hi, n_long) + [S // 2 + c]
    for region in (TILE - 1, TILE, TILE + 1):
        if region > S and (region - S) % hop == 0:
            out.append(region - S)
    return out


def signal(kind, n, fs, maxf0=700.0, seed=0):
    """f0_ref's signals, and a "rich" tone: 120 Hz with 4 Hz vibrato, partials 1 / k up to 0.45 fs and weak noise; "rich-noisy" the
    same with noise 0.05, "rich-steady" the same without vibrato"""
    if not kind.startswith("rich"):
        return f0_ref.signal(kind, n, fs, maxf0, seed)
    g = np.random.Generator(np.random.PCG64(5000 + seed))
    t = np.arange(n, dtype=np.float64) / fs
    vib = 0.0 if kind == "rich-steady" else 3.0 / (2 * np.pi * 4.0) * (1.0 - np.cos(2 * np.pi * 4.0 * t))
    phase = 2 * np.pi * (120.0 * t + vib)
    x = sum(np.sin(k * phase + 0.3 * k) / k for k in range(1, int(0.45 * fs / 120.0) + 1)) * 0.2
    x = x + (0.05 if kind == "rich-noisy" else 0.002) * g.standard_normal(n)
    return x.astype(np.float32)


def params(gi):
    (fs, hop, win, minf0, maxf0, n_long), edges, T, Wb = GEOMETRIES[gi]
    lo, hi = f0_ref.lags(fs, minf0, maxf0)
    return dict(fs=fs, hop=hop, win=win, minf0=minf0, maxf0=maxf0, lag_lo=lo, lag_hi=hi, n_long=n_long, n_taps=T, band_win=Wb,
                edges=edges)


@functools.lru_cache(maxsize=None)
def geometry_case(gi):
    """geometry GEOMETRIES[gi] -> (params dict, taps, list of (kind, n, signal, reference)): computed once per process"""
    p, h = params(gi), geometry_taps(gi)
    rows = []
    for k, kind in enumerate(SIGNALS):
        for n in lengths(p["hop"], p["win"], p["lag_hi"], p["n_long"], p["n_taps"]):
            x = signal(kind, n, p["fs"], p["maxf0"], seed=10 * gi + k)
            rows.append((kind, n, x, analyse(x, h, p["fs"], p["hop"], p["win"], p["lag_lo"], p["lag_hi"], THRESHOLD, p["band_win"])))
    return p, h, rows


@functools.lru_cache(maxsize=None)
def band_win_case(Wb):
    """the geometry WB_GEOMETRY with WB_EDGES / WB_TAPS and the sum window Wb, on the tone, the rich tone and the noise"""
    p = dict(params(WB_GEOMETRY), n_taps=WB_TAPS, band_win=Wb, edges=WB_EDGES)
    h = taps(p["fs"], WB_EDGES, WB_TAPS)
    rows = []
    for k, kind in enumerate(("tone", "rich", "noise")):
        x = signal(kind, WB_N, p["fs"], p["maxf0"], seed=200 + k)
        rows.append((kind, WB_N, x, analyse(x, h, p["fs"], p["hop"], p["win"], p["lag_lo"], p["lag_hi"], THRESHOLD, Wb)))
    return p, h, rows
