"""numpy references of the stage-1 low cut (swn_lowcut_chunk; the definition is in include/swn_hip.h and melspec.py):

    acc = 0.0;  for q = 0 .. n_taps - 1 ascending: acc = fma(h[q], (double)x[t - q], acc);  y[t] = (float)acc,  x[t < 0] = 0

(a) `value64`: the float64 value r = np.convolve(h, x64)[:n].
(b) `exact_chain`: the device bits for signals whose samples are 0 or +-2^k.  There h[q] * x is exact (a power-of-two scaling,
    away from under- and overflow), so fma(h[q], x, acc) is the ordinary fp64 add acc + h[q] x, and a loop over q of vectorised
    adds reproduces the chain of every sample at once.
`bound`: for general signals, derived and not fitted:

    |y - r| <= 2^-24 (1 + 2^-20) |r| + n_taps 2^-53 (|h| * |x|)[t] + 2^-149

  - the chain and the reference each sum the same n_taps products; either one's rounding error is at most
    gamma(n_taps) (|h| * |x|)[t] with gamma(k) ~ k 2^-53, and the second term covers what separates the two sums
  - the one rounding to fp32 is at most 2^-24 |acc|, and |acc| <= |r| (1 + 2^-20) once the second term (relative to |r| it is far
    below 2^-20 wherever the first term matters) is folded in
  - 2^-149, the spacing of the fp32 subnormals, covers a result that rounds into them, where the relative term no longer holds.
Checked on the CPU with the 255 taps at 22 050 Hz (a +-1 signal, 0.3-sigma noise and DC, 3 000 samples each): the emulated
chain reaches 0.99 of the bound and never exceeds it.  The bound leaves no entry out."""
import numpy as np


def value64(h, x):
    """(a): r[t] = sum_q h[q] x[t - q] in float64"""
    h, x = np.asarray(h, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return np.convolve(h, x)[:x.shape[0]] if x.shape[0] else np.zeros(0)


def is_exact_signal(x):
    """every sample is 0 or +-2^k with a modest k: the products with fp64 taps are exact"""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    return bool(np.all((x == 0) | ((np.abs(m) == 0.5) & (np.abs(e) <= 64))))


def exact_chain(h, x):
    """(b): the bits of the fma chain for a signal of zeros and +-2^k, as float32"""
    h = np.asarray(h, dtype=np.float64)
    x32 = np.asarray(x, dtype=np.float32)
    assert is_exact_signal(x32), "reference (b) holds only for samples that are 0 or +-2^k"
    n = x32.shape[0]
    x64 = x32.astype(np.float64)
    acc = np.zeros(n, dtype=np.float64)
    for q in range(min(h.shape[0], n)):             # taps past the signal's length meet x[t < 0] = 0 only
        acc[q:] = acc[q:] + h[q] * x64[:n - q]      # exact product, one rounding: the fma
    return acc.astype(np.float32)


def emulated_chain(h, x):
    """the definition itself, sample by sample with libm's fma: slow (n n_taps calls), for short signals on the CPU"""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    h = [float(v) for v in np.asarray(h, dtype=np.float64)]
    x = [float(v) for v in np.asarray(x, dtype=np.float32)]
    out = np.zeros(len(x), dtype=np.float64)
    for t in range(len(x)):
        acc = 0.0
        for q in range(min(len(h), t + 1)):         # fma(h, 0, acc) = acc: the taps that meet x[t < 0] change nothing
            acc = libm.fma(h[q], x[t - q], acc)
        out[t] = acc
    return out.astype(np.float32)


def bound(h, x):
    """the derived bound on |y - value64| per sample"""
    h, x = np.asarray(h, dtype=np.float64), np.asarray(x, dtype=np.float64)
    r = value64(h, x)
    spread = np.convolve(np.abs(h), np.abs(x))[:x.shape[0]] if x.shape[0] else np.zeros(0)
    return 2.0 ** -24 * (1.0 + 2.0 ** -20) * np.abs(r) + h.shape[0] * 2.0 ** -53 * spread + 2.0 ** -149


def taps(n_taps, seed=0):
    """n_taps fp64 taps with full mantissas: a decaying seeded sequence with both signs"""
    g = np.random.Generator(np.random.PCG64(1000 + 7 * n_taps + seed))
    return g.standard_normal(n_taps) * np.exp(-np.arange(n_taps) / 97.0)


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
    """float32 signals for the bound: broadband noise, a 50 Hz tone on a DC offset, half-silence"""
    g = np.random.Generator(np.random.PCG64(3000 + seed))
    t = np.arange(n, dtype=np.float64) / fs
    if kind == "noise":
        x = 0.3 * g.standard_normal(n)
    elif kind == "hum":
        x = 0.25 * np.sin(2 * np.pi * 50.0 * t + 0.4) + 0.125
    elif kind == "half-silence":
        x = 0.1 * g.standard_normal(n)
        x[:n // 2] = 0.0
    else:
        raise ValueError(kind)
    return x.astype(np.float32)
