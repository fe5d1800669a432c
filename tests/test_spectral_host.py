"""CPU: the host side of the multi-resolution STFT loss (spectral.py, the swn_spectral_* entry points, the driver flag):
geometry against torch.stft, argument checks, symbols.  No device call behind any of these."""
import ctypes

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, ops, spectral
from shallow_wavenet_amd import train_driver as T

SIZES = T.fft_sizes(17)


def _sz(sizes):
    return (ctypes.c_int * len(sizes))(*sizes)


def test_frame_and_bin_counts_equal_torch_stft():
    for length in (65, 277, 601, 1025, 4999, 8114, 8800):
        x = torch.zeros(length)
        for n in SIZES + [32, 64, 96]:
            if length > n // 2:
                sp = torch.stft(x, n, window=torch.hann_window(n), return_complex=True)
                assert tuple(sp.shape) == (spectral.bin_count(n), spectral.frame_count(length, n)), (length, n)


def test_state_size_is_one_byte_per_row_frame_and_bin():
    lib = _lib.lib()
    for rows, length in ((1, 601), (5, 8114)):
        sizes = [n for n in SIZES if length > n // 2]
        want = sum(rows * spectral.frame_count(length, n) * spectral.bin_count(n) for n in sizes)
        assert lib.swn_spectral_state_bytes(rows, length, _sz(sizes), len(sizes)) == want
        frames_floats = 4 * sum(rows * spectral.frame_count(length, n) * n for n in sizes)
        assert lib.swn_spectral_work_bytes(rows, length, _sz(sizes), len(sizes)) >= frames_floats


def test_tables_are_the_cos_and_periodic_hann_tables():
    for n in (32, 160, 2048):
        t = spectral.size_tables(n)
        assert t.shape == (2 * n,) and t.dtype == np.float32
        m = np.arange(n)
        assert np.abs(t[:n] - np.cos(2 * np.pi * m / n)).max() < 1e-7
        assert np.abs(t[n:] - torch.hann_window(n, dtype=torch.float64).numpy()).max() < 1e-7
        assert t[n // 4] == 0.0 and t[0] == 1.0 and t[n // 2] == -1.0 and t[n] == 0.0


def test_bad_sizes_and_lengths_are_rejected():
    lib = _lib.lib()
    null = ctypes.c_void_p(None)
    for rows, length, sizes in ((1, 64, [128]), (1, 600, [128, 1280]), (1, 8114, [100]), (1, 8114, [48]), (1, 8114, [4096]),
                                (0, 8114, [128]), (1, 8114, []), (1, 8114, [128] * 33)):
        assert lib.swn_spectral_work_bytes(rows, length, _sz(sizes), len(sizes)) == 0
        assert lib.swn_spectral_state_bytes(rows, length, _sz(sizes), len(sizes)) == 0
        assert lib.swn_spectral_forward(null, null, rows, length, _sz(sizes), len(sizes), null, null, null, null, null, null) == -2
        assert lib.swn_spectral_backward(null, null, rows, length, _sz(sizes), len(sizes), null, null, null, null) == -2
    # valid geometry, null pointers
    assert lib.swn_spectral_forward(null, null, 1, 8114, _sz([128]), 1, null, null, null, null, null, null) == -2
    with pytest.raises(ValueError, match="multiple of 32"):
        spectral.MultiResolutionSTFTLoss([128, 100], "cpu")
    with pytest.raises(ValueError, match="multiple of 32"):
        spectral.MultiResolutionSTFTLoss([4096], "cpu")
    loss = spectral.MultiResolutionSTFTLoss(SIZES, "cpu")
    assert loss.sizes_for(601) == [n for n in SIZES if n <= 1024] and loss.sizes_for(64) == []
    x = torch.zeros(2, 100)
    with pytest.raises(ValueError, match="FFT size 224 needs signals longer than 112"):
        loss(x, x, 601)                       # the filter passes 224, the signals are too short for its reflect padding
    with pytest.raises(ValueError, match="no FFT size"):
        loss(x, x, 64)
    with pytest.raises(ValueError, match="targets"):
        loss(torch.zeros(2, 700), torch.zeros(2, 700, requires_grad=True), 700)
    with pytest.raises(ValueError, match="one shape"):
        loss(torch.zeros(2, 700), torch.zeros(3, 700), 700)
    with pytest.raises(RuntimeError, match="HIP device"):          # no CPU path behind the op
        torch.ops.swn.spectral_loss(torch.zeros(2, 700), torch.zeros(2, 700), loss.tables_for([128]), [128], False)


def test_fake_implementations_give_the_shapes_and_the_checks():
    from torch._subclasses.fake_tensor import FakeTensorMode
    sizes = [128, 160, 2048]
    with FakeTensorMode():
        s, t, tab = torch.empty(5, 8114), torch.empty(5, 8114), torch.empty(2 * sum(sizes))
        l1, lsd, state = torch.ops.swn.spectral_loss(s, t, tab, sizes, True)
        assert tuple(l1.shape) == (5, 3) and tuple(lsd.shape) == (5, 3) and state.dtype == torch.uint8
        assert state.numel() == sum(5 * spectral.frame_count(8114, n) * spectral.bin_count(n) for n in sizes)
        assert torch.ops.swn.spectral_loss(s, t, tab, sizes, False)[2].numel() == 0
        grad = torch.ops.swn.spectral_loss_backward(l1, state, tab, sizes, 8114)
        assert tuple(grad.shape) == (5, 8114)
        with pytest.raises(RuntimeError, match="multiple of 32"):
            torch.ops.swn.spectral_loss(s, t, tab, [100], False)
        with pytest.raises(RuntimeError, match="longer than"):
            torch.ops.swn.spectral_loss(torch.empty(5, 64), torch.empty(5, 64), tab, [128], False)


def test_parser_takes_the_flag_and_defaults_to_torch():
    p = T.build_parser()
    assert p.parse_args(["--expdir", "x"]).spectral_loss == "torch"
    assert p.parse_args(["--expdir", "x", "--spectral_loss", "hip"]).spectral_loss == "hip"
    with pytest.raises(SystemExit):
        p.parse_args(["--expdir", "x", "--spectral_loss", "rocfft"])


def test_symbols_are_exported_and_bound():
    lib = _lib.lib()
    for name in ("swn_spectral_work_bytes", "swn_spectral_state_bytes", "swn_spectral_forward", "swn_spectral_backward"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "spectral_loss" in ops.OP_NAMES and "spectral_loss_backward" in ops.OP_NAMES
    assert lib.swn_abi_version() == 3
