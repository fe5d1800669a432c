"""CPU: the float64 yardstick of the log-mel operator (tests/melspec_ref.py) is the definition - its amplitudes are
torch.stft's in float64 (periodic Hann, centre, reflect) for hops that do and do not divide n_fft, its filter bank has the
properties of HTK triangles - and the tables melspec.py hands to the kernel are that yardstick's after fp32 rounding."""
import numpy as np
import pytest
import torch

import melspec_ref as MR
from shallow_wavenet_amd import melspec


@pytest.mark.parametrize("n_fft,hop,length", [(32, 8, 17), (32, 8, 131), (96, 37, 500), (96, 96, 49), (512, 80, 1201),
                                              (512, 128, 1024), (1024, 110, 3001), (64, 1, 200), (2048, 2048, 4099)])
def test_amplitudes_equal_torch_stft_in_float64(n_fft, hop, length):
    x = MR.signal("broadband", length, 16000, seed=length).astype(np.float64)
    got = MR.amplitudes(x, n_fft, hop)
    want = torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64),
                      center=True, pad_mode="reflect", return_complex=True).abs().numpy().T
    assert got.shape == want.shape == (MR.frame_count(length, hop), n_fft // 2 + 1)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, want.max())
    re, im = MR.stft_parts(x, n_fft, hop)
    full = torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, window=torch.hann_window(n_fft, dtype=torch.float64),
                      return_complex=True).numpy().T
    assert np.abs(re - full.real).max() <= 1e-12 * max(1.0, want.max()) and np.abs(im - full.imag).max() <= 1e-12 * max(1.0, want.max())


@pytest.mark.parametrize("length,hop", [(17, 8), (16, 8), (15, 8), (1, 1), (3001, 110), (66000, 110), (110, 110), (109, 110)])
def test_frame_count(length, hop):
    assert MR.frame_count(length, hop) == 1 + length // hop == melspec.frame_count(length, hop)
    if length > 16:
        assert MR.frame_indices(length, 32, hop).shape == (1 + length // hop, 32)


def test_reflection_does_not_repeat_the_edge_sample():
    idx = MR.frame_indices(20, 32, 8)
    assert idx[0].tolist()[:18] == list(range(16, 0, -1)) + [0, 1]
    assert idx[2].tolist() == list(range(0, 20)) + list(range(18, 6, -1))      # frame 2 starts at sample 0, runs off the end
    assert idx.min() == 0 and idx.max() == 19


BANKS = [(fs, n, m, 0.0, None) for fs, n, _, m in MR.GEOMETRIES] + [(22050, 1024, 80, 80.0, 7600.0), (16000, 512, 40, 55.0, 7000.0)]


@pytest.mark.parametrize("fs,n_fft,n_mels,fmin,fmax", BANKS)
def test_filter_bank_properties(fs, n_fft, n_mels, fmin, fmax):
    W = MR.filterbank(fs, n_fft, n_mels, fmin, fmax)
    P = MR.mel_points(n_mels, fmin, fs / 2.0 if fmax is None else fmax)
    h = np.arange(n_fft // 2 + 1) * fs / n_fft
    assert W.shape == (n_mels, n_fft // 2 + 1) and W.min() >= 0.0 and W.max() <= 1.0
    assert ((W > 0).sum(0) <= 2).all()                                  # at most two filters overlap a bin
    inside = (h >= P[1]) & (h <= P[-2])                                 # between the first and the last centre
    assert np.abs(W.sum(0)[inside] - 1.0).max() <= 1e-12
    assert (W.sum(0)[~inside] < 1.0 + 1e-12).all()
    for m in range(n_mels):
        nz = np.flatnonzero(W[m])
        if nz.size:                                                      # one run, inside (P_m, P_m+2)
            assert nz[-1] - nz[0] + 1 == nz.size and h[nz[0]] > P[m] and h[nz[-1]] < P[m + 2]
        # the peak lies at one of the two bins nearest the centre P_m+1, the one below or the one above it: the one with the
        # larger value of the triangle (the slopes differ, so the nearer of the two in Hz need not be the higher one)
        if nz.size:
            below = int(np.floor(P[m + 1] * n_fft / fs))
            above = min(below + 1, n_fft // 2)
            tri = lambda b: max(0.0, min((h[b] - P[m]) / (P[m + 1] - P[m]), (P[m + 2] - h[b]) / (P[m + 2] - P[m + 1])))
            assert np.argmax(W[m]) == (below if tri(below) >= tri(above) else above)
            assert W[m].max() == max(tri(below), tri(above))
    # equally spaced in mel, end points exact
    mel = MR.hz_to_mel(P)
    assert np.abs(np.diff(mel) - np.diff(mel)[0]).max() <= 1e-9 and abs(P[0] - fmin) <= 1e-9
    assert abs(MR.mel_to_hz(MR.hz_to_mel(1000.0)) - 1000.0) <= 1e-9 and abs(MR.hz_to_mel(1000.0) - 999.9855) <= 1e-3


@pytest.mark.parametrize("fs,n_fft,n_mels,fmin,fmax", BANKS)
def test_package_tables_equal_the_yardstick_after_fp32_rounding(fs, n_fft, n_mels, fmin, fmax):
    W = MR.filterbank(fs, n_fft, n_mels, fmin, fmax)
    Wp = melspec.mel_filterbank(fs, n_fft, n_mels, fmin, fmax)
    assert Wp.dtype == np.float64 and np.array_equal(Wp.astype(np.float32), W.astype(np.float32))
    table, bank = melspec.tables(fs, n_fft, n_mels, fmin, fmax)
    bins = n_fft // 2 + 1
    assert table.dtype == np.float32 and table.shape == (2 * n_fft + 2 * bins,) and len(bank) == n_mels
    c, _ = MR.basis(n_fft)
    assert np.abs(table[:n_fft] - c[:, 1].astype(np.float32)).max() <= 2.0 ** -24      # cos(2 pi m / n): column b = 1
    assert np.array_equal(table[n_fft:2 * n_fft], MR.window(n_fft, np.float32))
    # the runs, unpacked, are the bank
    dense, at = np.zeros((n_mels, bins), dtype=np.float32), 2 * n_fft
    for m, code in enumerate(bank):
        start, cnt = code & 0xffff, code >> 16
        assert cnt >= 1 and start + cnt <= bins
        dense[m, start:start + cnt] = table[at:at + cnt]
        at += cnt
    assert at <= table.shape[0] and not table[at:].any()
    assert np.array_equal(dense, W.astype(np.float32))


def test_yardstick_fp32_evaluation_is_close_but_not_equal():
    """e32 of the GPU tests' bound: the same formulas in fp32 numpy land within a few 1e-7 of float64"""
    fs, n_fft, hop, n_mels = 22050, 1024, 110, 80
    x = MR.signal("broadband", 3001, fs, seed=1)
    m64 = MR.mel(x, fs, n_fft, hop, n_mels)
    m32 = MR.mel(x, fs, n_fft, hop, n_mels, dtype=np.float32)
    assert m32.dtype == np.float32
    e32 = np.abs(m32 - m64).max() / m64.max()
    assert 1e-9 < e32 < 2e-6
    assert m64.min() > 0.01 and np.abs(MR.logmel(x, fs, n_fft, hop, n_mels) - np.log(m64)).max() == 0.0
