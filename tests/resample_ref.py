"""numpy references of the rational resampler (swn_resample_chunk; the definition is in include/swn_hip.h and melspec.py).
With L = up, M = down, taps h[0 .. N - 1] (N odd), D = (N - 1) / 2, P[r][q] = h[r + q L] (0.0 past N), Q = ceil(N / L), output n
of a signal x of T samples (x = 0 outside [0, T)), n < ceil(T L / M):

    p = n M + D,  r = p mod L,  i0 = p div L
    acc = +0.0;  for q = 0 .. Q - 1 ascending: acc = fma(P[r][q], (double)x[i0 - q], acc);  y[n] = (float)acc

(a) `value64`: the float64 value, np.convolve(h, zero-stuffed x)[n M + D] - what scipy.signal.resample_poly(x, L, M) computes
    with the default design.
(b) `exact_chain`: the device bits for signals whose samples are 0 or +-2^k.  There P[r][q] * x is exact (a power-of-two
    scaling, away from under- and overflow), so fma(P, x, acc) is the ordinary fp64 add acc + P x, and a loop over q of vectorised
    adds reproduces the chain of every output at once.
(c) `emulated_chain`: the definition itself with libm's fma: slow, for short signals.
`bound`: for general signals, derived and not fitted:

    |y - r| <= 2^-24 (1 + 2^-20) |r| + Q 2^-53 (|P_r| * |x|)[n] + 2^-149

  - the chain and the reference each sum the same (at most Q non-zero) products of output n; either one's rounding error is at
    most gamma(Q) (|P_r| * |x|)[n] with gamma(k) ~ k 2^-53 and (|P_r| * |x|)[n] = sum_q |P[r][q]| |x[i0 - q]|, and the second term
    covers what separates the two sums
  - the one rounding to fp32 is at most 2^-24 |acc|, and |acc| <= |r| (1 + 2^-20) once the second term (relative to |r| it is far
    below 2^-20 wherever the first term matters) is folded in
  - 2^-149, the spacing of the fp32 subnormals, covers a result that rounds into them, where the relative term no longer holds.
Checked on the CPU with the 147 / 320 table (6 401 taps, Q = 44; 0.3-sigma noise, a +-1 signal and a 50 Hz tone on DC, 700 inputs
= 322 outputs each, general_signal(kind, 700, 48000, seed=1)): the emulated chain reaches 0.99, 0.96 and 0.90 of the bound (the
fp32 rounding alone comes that close to half a unit in the last place somewhere in a few hundred samples) and never exceeds it.
The bound leaves no entry out."""
import numpy as np

RATIOS = [(1, 2), (2, 1), (3, 2), (147, 160), (147, 320), (441, 320), (80, 147), (441, 160)]       # (L, M)


def taps(L, M, half_len=10, beta=5.0):
    """the scipy recipe itself, written out: the prototype filter of scipy.signal.resample_poly(x, L, M)"""
    from scipy.signal import firwin
    top = max(L, M)
    return L * firwin(2 * half_len * top + 1, 1.0 / top, window=("kaiser", beta))


def table(h, L):
    """P (L, Q): P[r][q] = h[r + q L], 0.0 past the taps"""
    h = np.asarray(h, dtype=np.float64)
    Q = -(-h.shape[0] // L)
    P = np.zeros((L, Q), dtype=np.float64)
    for r in range(L):
        col = h[r::L]
        P[r, :col.shape[0]] = col
    return P


def out_count(T, L, M):
    return -(-T * L // M)


def ready_brute(T, L, M, n_taps):
    """outputs whose newest input i0 = (n M + D) div L has arrived when T have: counted one by one"""
    D, n = (n_taps - 1) // 2, 0
    while (n * M + D) // L <= T - 1:
        n += 1
    return n


def value64(h, x, L, M):
    """(a): r[n] = sum_k h[n M + D - k L] x[k] in float64"""
    h, x = np.asarray(h, dtype=np.float64), np.asarray(x, dtype=np.float64)
    T, D = x.shape[0], (h.shape[0] - 1) // 2
    n_out = out_count(T, L, M)
    if n_out == 0:
        return np.zeros(0)
    u = np.zeros(T * L, dtype=np.float64)
    u[::L] = x
    c = np.convolve(h, u)
    at = np.arange(n_out, dtype=np.int64) * M + D
    return np.where(at < c.shape[0], c[np.minimum(at, c.shape[0] - 1)], 0.0)


def is_exact_signal(x):
    """every sample is 0 or +-2^k with a modest k: the products with fp64 taps are exact"""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    return bool(np.all((x == 0) | ((np.abs(m) == 0.5) & (np.abs(e) <= 64))))


def _gather(x64, i0, q):
    """x[i0 - q] with zeros outside the signal"""
    i = i0 - q
    ok = (i >= 0) & (i < x64.shape[0])
    return np.where(ok, x64[np.clip(i, 0, max(x64.shape[0] - 1, 0))], 0.0) if x64.shape[0] else np.zeros(i.shape[0])


def exact_chain(h, x, L, M):
    """(b): the bits of the fma chain for a signal of zeros and +-2^k, as float32"""
    h = np.asarray(h, dtype=np.float64)
    x32 = np.asarray(x, dtype=np.float32)
    assert is_exact_signal(x32), "reference (b) holds only for samples that are 0 or +-2^k"
    P = table(h, L)
    x64 = x32.astype(np.float64)
    n_out = out_count(x32.shape[0], L, M)
    p = np.arange(n_out, dtype=np.int64) * M + (h.shape[0] - 1) // 2
    r, i0 = p % L, p // L
    acc = np.zeros(n_out, dtype=np.float64)
    for q in range(P.shape[1]):
        acc = acc + P[r, q] * _gather(x64, i0, q)   # exact product, one rounding: the fma
    return acc.astype(np.float32)


def emulated_chain(h, x, L, M):
    """(c): the definition itself, output by output with libm's fma: slow (n_out Q calls), for short signals on the CPU"""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    h = np.asarray(h, dtype=np.float64)
    P = table(h, L).tolist()
    xs = [float(v) for v in np.asarray(x, dtype=np.float32)]
    T, D, Q = len(xs), (h.shape[0] - 1) // 2, len(P[0])
    out = np.zeros(out_count(T, L, M), dtype=np.float64)
    for n in range(out.shape[0]):
        p = n * M + D
        row, i0, acc = P[p % L], p // L, 0.0
        for q in range(Q):
            i = i0 - q
            acc = libm.fma(row[q], xs[i] if 0 <= i < T else 0.0, acc)
        out[n] = acc
    return out.astype(np.float32)


def bound(h, x, L, M, r=None):
    """the derived bound on |y - value64| per output (r: value64(h, x, L, M), where the caller has it already)"""
    h, x = np.asarray(h, dtype=np.float64), np.asarray(x, dtype=np.float64)
    Q = -(-h.shape[0] // L)
    r = value64(h, x, L, M) if r is None else r
    return 2.0 ** -24 * (1.0 + 2.0 ** -20) * np.abs(r) + Q * 2.0 ** -53 * value64(np.abs(h), np.abs(x), L, M) + 2.0 ** -149


def exact_signal(kind, n, seed=0, at=0):
    """float32 signals for reference (b): impulse (a one at sample `at`), ones, ternary (-1, 0, +1), pow2 (0 or +-2^k, |k| <= 8)"""
    g = np.random.Generator(np.random.PCG64(2000 + seed))
    if kind == "impulse":
        x = np.zeros(n, dtype=np.float32)
        x[at] = 1.0
    elif kind == "ones":
        x = np.ones(n, dtype=np.float32)
    elif kind == "ternary":
        x = g.integers(-1, 2, n).astype(np.float32)
    elif kind == "pow2":
        x = (g.choice([-1.0, 0.0, 1.0], n) * 2.0 ** g.integers(-8, 9, n)).astype(np.float32)
    else:
        raise ValueError(kind)
    return x


def general_signal(kind, n, fs, seed=0):
    """float32 signals for the bound: broadband noise, a +-1 signal, a 50 Hz tone on a DC offset, half-silence"""
    g = np.random.Generator(np.random.PCG64(3000 + seed))
    t = np.arange(n, dtype=np.float64) / fs
    if kind == "noise":
        x = 0.3 * g.standard_normal(n)
    elif kind == "signs":
        x = g.choice([-1.0, 1.0], n)
    elif kind == "hum":
        x = 0.25 * np.sin(2 * np.pi * 50.0 * t + 0.4) + 0.125
    elif kind == "half-silence":
        x = 0.1 * g.standard_normal(n)
        x[:n // 2] = 0.0
    else:
        raise ValueError(kind)
    return x.astype(np.float32)
