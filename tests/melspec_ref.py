"""The log-mel definition (shallow_wavenet_amd/melspec.py, include/swn_hip.h) in plain numpy, for the tests: the yardstick of
the operator.  Written from the definition alone - it imports nothing of the package - and checked on the CPU by
test_melspec_reference.py (amplitudes against torch.stft in float64, the filter bank's properties).

Every function takes `dtype`: float64 is the reference, float32 the same formulas evaluated in fp32 numpy, whose distance
from float64 (e32) is what the GPU tests scale their bound with.  The transform is the dense DFT as a matrix product, so the
fp32 evaluation really runs in fp32 whatever the FFT library does, and the float64 one shares no code with torch.stft.
"""
import functools

import numpy as np

# (fs, n_fft, hop, n_mels) of the GPU tests
GEOMETRIES = [(8000, 32, 8, 4), (8000, 96, 37, 8), (16000, 512, 80, 40), (22050, 1024, 110, 80), (22050, 2048, 2048, 128),
              (8000, 64, 1, 8)]
FRAME_TILE = 16          # frames per block of the kernel (LM_FR, csrc/swn_melspec.hip)
FLOOR = 1e-5


def frame_count(length, hop):
    return 1 + length // hop


def frame_indices(length, n_fft, hop):
    """(F, n_fft) sample index of every frame position: reflect padding without repeating the edge sample"""
    p = np.arange(frame_count(length, hop))[:, None] * hop - n_fft // 2 + np.arange(n_fft)[None, :]
    p = np.where(p < 0, -p, p)
    return np.where(p >= length, 2 * (length - 1) - p, p)


def window(n_fft, dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)).astype(dtype)


@functools.lru_cache(maxsize=4)
def basis(n_fft, dtype=np.float64):
    """cos and sin (n_fft, n_fft // 2 + 1) of 2 pi j b / n_fft, the argument reduced exactly: (j b) mod n_fft (shared between
    the calls: read-only)"""
    jb = (np.arange(n_fft)[:, None] * np.arange(n_fft // 2 + 1)[None, :]) % n_fft
    ang = 2.0 * np.pi * jb.astype(np.float64) / n_fft
    return np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)


def stft_parts(x, n_fft, hop, dtype=np.float64):
    """Re, Im (F, n_fft // 2 + 1) of sum_j x[p] w[j] e^(-2 pi i j b / n_fft)"""
    x = np.asarray(x).astype(dtype)
    assert x.ndim == 1 and x.shape[0] > n_fft // 2
    fr = x[frame_indices(x.shape[0], n_fft, hop)] * window(n_fft, dtype)[None, :]
    c, s = basis(n_fft, dtype)
    re, im = fr @ c, -(fr @ s)
    assert re.dtype == dtype
    return re, im


def amplitudes(x, n_fft, hop, dtype=np.float64):
    re, im = stft_parts(x, n_fft, hop, dtype)
    return np.sqrt(re * re + im * im)


def hz_to_mel(h):
    return 2595.0 * np.log10(1.0 + h / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (m / 2595.0) - 1.0)


def mel_points(n_mels, fmin, fmax):
    """P_0 .. P_(n_mels + 1) in Hz"""
    lo, hi = hz_to_mel(np.float64(fmin)), hz_to_mel(np.float64(fmax))
    return mel_to_hz(lo + (hi - lo) * np.arange(n_mels + 2, dtype=np.float64) / (n_mels + 1))


def filterbank(fs, n_fft, n_mels, fmin=0.0, fmax=None):
    """W (n_mels, n_fft // 2 + 1), float64, element by element from the definition"""
    fmax = fs / 2.0 if fmax is None else fmax
    P = mel_points(n_mels, fmin, fmax)
    W = np.zeros((n_mels, n_fft // 2 + 1), dtype=np.float64)
    for m in range(n_mels):
        for b in range(n_fft // 2 + 1):
            h = b * float(fs) / n_fft
            W[m, b] = max(0.0, min((h - P[m]) / (P[m + 1] - P[m]), (P[m + 2] - h) / (P[m + 2] - P[m + 1])))
    return W


def mel(x, fs, n_fft, hop, n_mels, fmin=0.0, fmax=None, dtype=np.float64):
    """M (F, n_mels): the fp32-rounded filter bank (what the operator is given) applied to the amplitudes, in `dtype`"""
    W = filterbank(fs, n_fft, n_mels, fmin, fmax).astype(np.float32).astype(dtype)
    return amplitudes(x, n_fft, hop, dtype) @ W.T


def logmel(x, fs, n_fft, hop, n_mels, fmin=0.0, fmax=None, floor=FLOOR, dtype=np.float64):
    return np.log(np.maximum(mel(x, fs, n_fft, hop, n_mels, fmin, fmax, dtype), dtype(floor)))


# ---- the signals of the GPU tests (fp32 values: what the operator is given) ----------------------------------------------
def signal(kind, length, fs, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(length, dtype=np.float64) / fs
    if kind == "broadband":          # two sinusoids plus Gaussian noise, |x| <= 0.5
        x = 0.2 * np.sin(2 * np.pi * 0.031 * fs * t) + 0.15 * np.sin(2 * np.pi * 0.173 * fs * t + 0.7) + 0.04 * g.standard_normal(length)
        x = np.clip(x, -0.5, 0.5)
    elif kind == "tone":
        x = 0.4 * np.sin(2 * np.pi * 0.0917 * fs * t + 0.3)
    elif kind == "half-silence":
        x = 0.1 * g.standard_normal(length)
        x[:length // 2] = 0.0
    elif kind == "zeros":
        x = np.zeros(length)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


KINDS = ("broadband", "tone", "half-silence", "zeros")


def lengths(n_fft, hop):
    """the shortest signal; F one below, on and one above a multiple of the kernel's frame tile (the first multiple whose
    signals are long enough); about 3 000 samples"""
    k = 1
    while (FRAME_TILE * k - 2) * hop < n_fft // 2 + 1:
        k += 1
    out = [n_fft // 2 + 1, max(3001, n_fft // 2 + 1)]
    for F in (FRAME_TILE * k - 1, FRAME_TILE * k, FRAME_TILE * k + 1):
        out.append((F - 1) * hop + hop // 2)                 # 1 + len // hop == F
        assert frame_count(out[-1], hop) == F and out[-1] > n_fft // 2
    return sorted(set(out))
