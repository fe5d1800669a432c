"""The mel-cepstrum definition (shallow_wavenet_amd/melspec.py MelCepstrumExtractor, include/swn_hip.h) in plain numpy, for the
tests: the yardstick of the operator.  Written from the definition alone - it imports nothing of the package and does not
go through a matrix: per frame it pads (np.pad, reflect), windows, takes np.fft.rfft, the log of the floored amplitude,
np.fft.irfft, doubles the one-sided cepstrum and runs the SPTK `freqt` recursion coefficient by coefficient.
test_mcep_reference.py checks the package's matrix against it on the CPU.

float64 is the reference.  `mcep32` evaluates the same formulas in fp32 numpy (dense DFT and dense cosine sum as matrix
products, so that it really runs in fp32 whatever the FFT library does); its distance from float64 is reported next to the
operator's.  `fma_chain` is the exact arithmetic of one coefficient on the device: one fmaf chain over the bins in ascending
order."""
import functools

import numpy as np

import melspec_ref as MR

# (fs, n_fft, hop, order, alpha) of the GPU tests: fewer coefficients than one column tile of 16; 49 bins (K padded to 52);
# exactly one tile with hop 1; one coefficient into the second tile; run.sh's; both maxima
GEOMETRIES = [(8000, 32, 8, 7, 0.31), (8000, 96, 37, 12, 0.31), (8000, 64, 1, 15, 0.31), (16000, 512, 80, 16, 0.41),
              (22050, 1024, 110, 49, 0.455), (22050, 2048, 2048, 63, 0.455)]
FLOOR = 1e-5


def geom_id(g):
    return f"fs{g[0]}-n{g[1]}-hop{g[2]}-M{g[3]}-a{g[4]}"


def log_floor32(floor=FLOOR):
    """fl32(ln floor) as the operator evaluates it: the fp32 floor, its log in double, rounded once"""
    return np.float32(np.log(np.float64(np.float32(floor))))


def amplitudes(x, n_fft, hop):
    """A (F, n_fft // 2 + 1) in float64: np.pad(reflect), periodic Hann, np.fft.rfft"""
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 1 and x.shape[0] > n_fft // 2
    xp = np.pad(x, n_fft // 2, mode="reflect")
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    F = 1 + x.shape[0] // hop
    return np.stack([np.abs(np.fft.rfft(xp[f * hop:f * hop + n_fft] * w)) for f in range(F)])


def log_amplitudes(x, n_fft, hop, floor=FLOOR):
    """L (F, bins) in float64; the floor is the fp32 number the operator is given"""
    return np.log(np.maximum(amplitudes(x, n_fft, hop), np.float64(np.float32(floor))))


def one_sided_cepstrum(L, n_fft):
    """c (.., n_fft // 2 + 1) from L (.., n_fft // 2 + 1): irfft, then c[0] = v[0], c[k] = 2 v[k], c[n_fft / 2] = v[n_fft / 2]"""
    v = np.fft.irfft(L, n_fft, axis=-1)
    c = 2.0 * v[..., :n_fft // 2 + 1]
    c[..., 0] = v[..., 0]
    c[..., n_fft // 2] = v[..., n_fft // 2]
    return c


def freqt(c, order, alpha):
    """SPTK freqt: c (.., m1 + 1) -> (.., order + 1), the recursion coefficient by coefficient (the leading axes are only
    batched); in the dtype of c"""
    c = np.asarray(c)
    m1 = c.shape[-1] - 1
    a = c.dtype.type(alpha)
    b = c.dtype.type(1.0) - a * a
    g = np.zeros(c.shape[:-1] + (order + 1,), dtype=c.dtype)
    for i in range(m1, -1, -1):
        d = g.copy()
        g[..., 0] = c[..., i] + a * d[..., 0]
        if order >= 1:
            g[..., 1] = b * d[..., 0] + a * d[..., 1]
        for j in range(2, order + 1):
            g[..., j] = d[..., j - 1] + a * (d[..., j] - g[..., j - 1])
    return g


def mcep(x, n_fft, hop, order, alpha, floor=FLOOR):
    """mc (F, order + 1) in float64: the reference"""
    return freqt(one_sided_cepstrum(log_amplitudes(x, n_fft, hop, floor), n_fft), order, alpha)


@functools.lru_cache(maxsize=None)
def matrix(n_fft, order, alpha):
    """G (order + 1, bins) in float64 by pushing the unit vectors through the reference chain (read-only, shared)"""
    G = freqt(one_sided_cepstrum(np.eye(n_fft // 2 + 1), n_fft), order, alpha).T.copy()
    G.setflags(write=False)
    return G


def mcep32(x, n_fft, hop, order, alpha, floor=FLOOR):
    """the same formulas in fp32 numpy: amplitudes by the dense DFT (melspec_ref), the log, the cepstrum as a dense cosine sum,
    the recursion - every intermediate is fp32"""
    f32 = np.float32
    A = MR.amplitudes(x, n_fft, hop, dtype=f32)
    L = np.log(np.maximum(A, f32(floor)))
    assert L.dtype == f32
    bins = n_fft // 2 + 1
    e = np.full(bins, 2.0)
    e[0] = e[-1] = 1.0
    kb = (np.arange(bins)[:, None] * np.arange(bins)[None, :]) % n_fft
    C = (e[:, None] * e[None, :] * np.cos(2.0 * np.pi * kb / n_fft) / n_fft).astype(f32)
    out = freqt(L @ C.T, order, alpha)
    assert out.dtype == f32
    return out


def fma32(a, b, c):
    """fl32(a b + c) with one rounding, element by element, for fp32 arrays: the product of two fp32 numbers is exact in
    double; the sum is rounded to odd in double (TwoSum tells whether it was exact), and 53 bits rounded to odd round to the
    24 bits of fp32 as the exact sum would"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    nudged = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, nudged, s).astype(np.float32)


def fma_chain(L32, G32):
    """(order + 1,) fp32: acc <- fmaf(L[b], G[m][b], acc) over b ascending from 0, for every row m of G32 (order + 1, bins)"""
    L32, G32 = np.asarray(L32, dtype=np.float32), np.asarray(G32, dtype=np.float32)
    acc = np.zeros(G32.shape[0], dtype=np.float32)
    for b in range(G32.shape[1]):
        acc = fma32(np.broadcast_to(L32[b], acc.shape), G32[:, b], acc)
    return acc


def tolerance(x, n_fft, hop, order, alpha, floor=FLOOR):
    """(tol (F, order + 1), e32 of the amplitudes, B): the bound of the GPU tests, derived.  With A the float64 amplitudes,
    top the row's largest, e32 = max |A32 - A| / top from the fp32 numpy evaluation and B = max(4 e32, 1e-6) top (the linear
    bound of the log-mel tests), an amplitude within B of a moves the log by at most
        dL[b] = ln max(a + B, floor) - ln max(a - B, floor);
    the log itself is rounded to fp32 (2^-24 |L|, taken as 2^-23), and a chain of bins + 2 fp32 fused multiply-adds on fp32
    roundings of G adds at most (bins + 2) 2^-24 sum_b |G[m][b]| |L[b]| to first order:
        tol[m] = sum_b |G[m][b]| (dL[b] + 2^-23 |L[b]|) + (bins + 2) 2^-24 sum_b |G[m][b]| |L[b]|."""
    A = amplitudes(x, n_fft, hop)
    top = A.max()
    e32 = float(np.abs(MR.amplitudes(x, n_fft, hop, dtype=np.float32) - A).max() / top) if top > 0 else 0.0
    B = max(4.0 * e32, 1e-6) * top
    fl = np.float64(np.float32(floor))
    dL = np.log(np.maximum(A + B, fl)) - np.log(np.maximum(A - B, fl))
    L = np.log(np.maximum(A, fl))
    Ga = np.abs(matrix(n_fft, order, alpha))
    bins = n_fft // 2 + 1
    tol = (dL + 2.0 ** -23 * np.abs(L)) @ Ga.T + (bins + 2) * 2.0 ** -24 * (np.abs(L) @ Ga.T)
    return tol, e32, B
