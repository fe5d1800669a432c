"""CPU: the definition of the F0-adaptive spectral envelope (tests/envelope_ref.py, numpy float64) has the properties it claims,
the package's host tables are the reference's, and the host refuses what the contract refuses - no GPU call behind any of it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import envelope_ref as R
from shallow_wavenet_amd import _lib, melspec, ops
from shallow_wavenet_amd import feature_extract_driver as FD

RUN_SH = (22050, 1024, 110, 49, 0.455)


@pytest.mark.parametrize("g", R.GEOMETRIES + [(22050, 2048, 256, 63, 0.455), (8000, 64, 8, 0, 0.31)], ids=R.geom_id)
def test_matrix_is_the_freqt_recursion_on_unit_vectors(g):
    fs, n_fft, hop, order, alpha = g
    bins = n_fft // 2 + 1
    G = melspec.envelope_matrix(n_fft, order, alpha)
    assert G.shape == (order + 1, bins) and G.dtype == np.float64
    want = R.freqt(np.eye(bins), order, alpha).T             # row k of the identity is the unit vector e_k
    assert np.abs(G - want).max() <= 1e-12
    assert np.array_equal(want, R.matrix(n_fft, order, alpha))
    for k in (0, 1, bins // 3, bins - 1):                    # ... and one vector at a time gives the same column
        assert np.array_equal(R.freqt(np.eye(bins)[k], order, alpha), want[:, k])
    # c[0] reaches mc[0] alone, with weight 1: a gain moves nothing else
    assert G[0, 0] == 1.0 and not G[1:, 0].any()
    table = melspec.envelope_tables(n_fft, order, alpha)
    assert table.dtype == np.float64 and table.size == int(_lib.lib().swn_envelope_table_doubles(n_fft, order))
    assert np.array_equal(table[:n_fft], R.cos_table(n_fft)) and np.array_equal(table[n_fft:].reshape(order + 1, bins), G)


@pytest.mark.parametrize("fs,n_fft", [(8000, 64), (8000, 96), (16000, 512), (22050, 1024), (22050, 2048)])
def test_a_constant_spectrum_is_smoothed_to_itself(fs, n_fft):
    """the mirror at 0 and Nyquist and the overlaps: every bin's weights add up to wd"""
    P = np.full(n_fft // 2 + 1, 3.7)
    lo, hi = R.f0_floor(fs, n_fft), fs / 4.0
    for f0e in [np.nextafter(lo, np.inf), hi, 500.0, 0.5 * (lo + hi)] + list(np.random.default_rng(0).uniform(lo, hi, 6)):
        S = R.smooth(P, float(f0e), fs / n_fft, n_fft)
        assert np.abs(S / 3.7 - 1.0).max() <= 1e-12, f0e


def test_a_gain_moves_c0_and_the_level_alone():
    fs, n_fft, hop, order, alpha = RUN_SH
    x = (0.1 * np.random.default_rng(1).standard_normal(2000)).astype(np.float32)
    f0 = np.where(np.arange(R.frame_count(2000, hop)) % 2 == 0, 140.0, 0.0).astype(np.float32)
    a = R.envelope(x, f0, fs, n_fft, hop, order, alpha)
    for g in (0.25, 8.0):                                    # exact in fp32
        b = R.envelope(g * x, f0, fs, n_fft, hop, order, alpha)
        assert (a["S"] > 1e-8).all() and (b["S"] > 1e-8).all()          # everything above the floor^2 = 1e-10
        assert np.abs(b["E"] - a["E"] - np.log(g)).max() <= 1e-9
        assert np.abs(b["mc"][:, 0] - a["mc"][:, 0] - np.log(g)).max() <= 1e-9
        assert np.abs(b["mc"][:, 1:] - a["mc"][:, 1:]).max() <= 1e-9


def test_zeros_give_the_log_of_the_floor():
    for g in (R.GEOMETRIES[0], RUN_SH):
        fs, n_fft, hop, order, alpha = g
        F = R.frame_count(700, hop)
        r = R.envelope(np.zeros(700, np.float32), np.full(F, 0.3 * fs / 4.0, np.float32), fs, n_fft, hop, order, alpha)
        ln = np.log(np.float64(np.float32(R.FLOOR)))
        assert np.array_equal(r["L"], np.full_like(r["L"], 2.0 * ln))
        assert np.array_equal(r["E"].astype(np.float32), np.full(r["E"].shape, R.log_floor32()))        # the output, rounded once
        assert np.abs(r["E"] - ln).max() <= 1e-12 and not r["near_floor"].any()
        assert np.abs(r["mc"][:, 0] - ln).max() <= 1e-12 and np.abs(r["mc"][:, 1:]).max() <= 1e-12
        assert (r["tol_E"] < 2.0 ** -23 * abs(ln)).all()


def test_effective_f0_takes_the_branch_the_definition_says():
    fs, n_fft = 6100, 64                                     # f0_floor = 3 * 6100 / 61 = 300 and fs / 4 = 1525, exact in fp32
    assert R.f0_floor(fs, n_fft) == 300.0 and R.geometry_ok(fs, n_fft)
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    f0 = np.array([0.0, np.nan, 300.0, up(300.0), 1525.0, up(1525.0), -400.0, np.inf, 400.0], dtype=np.float32)
    want = [500.0, 500.0, 500.0, float(up(300.0)), 1525.0, 500.0, 500.0, 500.0, 400.0]
    assert R.effective_f0(f0, fs, n_fft).tolist() == want
    # the geometry rule: f0_floor < default_f0 <= fs / 4
    assert R.geometry_ok(8000, 64) and not R.geometry_ok(8000, 32) and R.geometry_ok(22050, 160) and not R.geometry_ok(22050, 128)
    assert not R.geometry_ok(1600, 64) and R.geometry_ok(2000, 64)
    # the window always fits: 2 hl + 1 <= n_fft - 1 just above the floor, hl = 6 at fs / 4
    for fs, n_fft in [(8000, 64), (22050, 1024), (22050, 2048), (6100, 64)]:
        lo = R.effective_f0(np.float32(R.f0_floor(fs, n_fft)) * np.float32(1.0001), fs, n_fft)
        assert 2 * R.half_len(fs, float(lo)) + 1 <= n_fft - 1 and R.half_len(fs, fs / 4.0) == 6


def test_the_rounding_tie_of_the_window_length():
    assert 1.5 * 8000 / 960.0 == 12.5 and R.half_len(8000, 960.0) == 13
    hl, w_raw, w = R.window(8000, 960.0)
    assert w.size == 27 and abs(np.sum(w * w) - 1.0) <= 1e-15 and w_raw[13] == 1.0


@pytest.mark.parametrize("f0", [120.0, 300.0, 600.0])
def test_the_envelope_follows_a_resonator_where_the_short_time_spectrum_shows_the_pitch(f0):
    """a pulse train through a two-pole resonator (1 500 Hz, r = 0.97) at fs 22 050, n_fft 1 024, hop 110: ln amplitude over the
    bins 10 .. 400, mean removed, true response subtracted, pooled over twenty frames of the steady state.  The envelope's std
    must be at least 5 times smaller than the raw short-time log amplitude's (the reference gave 16x - 150x here)."""
    fs, n_fft, hop, order, alpha = RUN_SH
    x, H = R.resonator_signal(fs, f0, 11025)
    F = R.frame_count(x.size, hop)
    r = R.envelope(x, np.full(F, f0, np.float32), fs, n_fft, hop, order, alpha)
    b = np.arange(10, 401)
    true = np.log(H(b * fs / n_fft))
    env, raw = [], []
    for f in range(40, 60):
        d = r["E"][f, b] - true
        q = R.short_time_logamp(x.astype(np.float32), f, n_fft, hop)[b] - true
        env.append(d - d.mean())
        raw.append(q - q.mean())
    env, raw = np.array(env), np.array(raw)
    print(f"F0 {f0}: envelope std {env.std():.3f} max {np.abs(env).max():.2f}; raw std {raw.std():.2f} max {np.abs(raw).max():.1f}; "
          f"ratio {raw.std() / env.std():.0f}x")
    assert raw.std() >= 5.0 * env.std()
    assert env.std() < 0.2


def test_streaming_rule():
    for n_fft, hop in [(64, 8), (96, 37), (64, 1), (1024, 110)]:
        half = n_fft // 2
        for n in list(range(0, 3 * n_fft)) + [5000]:
            want = sum(1 for f in range(0, n // hop + 2) if f * hop + half <= n)
            assert melspec.envelope_frames_ready(n_fft, hop, n) == want
            assert melspec.envelope_frames_ready(n_fft, hop, n, final=True) == 1 + n // hop
        # frame 0 of the envelope needs no reflected sample: one sample earlier than the log-mel rule
        assert melspec.envelope_frames_ready(n_fft, hop, half) == 1 and melspec.frames_ready(n_fft, hop, half) == 0


def test_the_extractor_refuses_on_the_host():
    E = melspec.SpectralEnvelopeExtractor
    ok = dict(fs=22050, n_fft=1024, hop=110, order=49, alpha=0.455)
    for bad in (dict(n_fft=1000), dict(n_fft=4096), dict(hop=0), dict(hop=_lib.F0_MAX_HOP + 1), dict(order=-1), dict(order=64),
                dict(n_fft=64, order=33), dict(alpha=1.0), dict(floor=0.0), dict(floor=float("inf")), dict(floor=1e-60),
                dict(q1=float("nan")), dict(n_fft=128), dict(default_f0=64.0), dict(default_f0=5600.0), dict(fs=0.0),
                dict(fs=8000, n_fft=32), dict(output="power")):
        with pytest.raises(ValueError):
            E(**{**ok, **bad}, device="cuda:0")
    with pytest.raises(ValueError):
        melspec.envelope_matrix(1024, 64, 0.455)
    with pytest.raises(RuntimeError):                        # the op itself, for callers that go past the class
        ops.envelope_impl(torch.zeros(1, 100), torch.zeros(1, 4), torch.zeros(4, dtype=torch.float64), [0], [100], [100], [0], [1],
                          22050.0, 1024, 110, 49, 1e-5, -0.15, 500.0, 0)
    assert "envelope" in ops.OP_NAMES
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        args = ([0, 0], [900, 700], [900, 700], [0, 2], [9, 7], 22050.0, 1024, 110, 49, 1e-5, -0.15, 500.0)
        wav, f0, tab = torch.empty(2, 900), torch.empty(2, 9), torch.empty(10, dtype=torch.float64)
        assert tuple(torch.ops.swn.envelope(wav, f0, tab, *args, 0).shape) == (2, 9, 50)
        assert tuple(torch.ops.swn.envelope(wav, f0, tab, *args, 1).shape) == (2, 9, 513)
        with pytest.raises(RuntimeError):
            torch.ops.swn.envelope(wav, f0, tab, *args, 2)


def test_the_driver_refuses_its_flag_without_a_device(tmp_path):
    from scipy.io import wavfile
    wavdir = str(tmp_path / "wav")
    os.makedirs(wavdir)
    wavfile.write(os.path.join(wavdir, "a.wav"), 22050, np.zeros(4000, dtype=np.int16))
    base = ["--waveforms", wavdir, "--hdf5dir", str(tmp_path / "h5"), "--verbose", "0", "--mcep_envelope", "true"]
    assert FD.build_parser().parse_args([]).mcep_envelope is False
    assert FD.main(base) == 2                                                        # needs --mcep_dim > 0
    assert FD.main(base + ["--mcep_dim", "0", "--feature_type", "mcep"]) == 2
    assert FD.main(base + ["--mcep_dim", "24", "--feature_type", "world"]) == 2      # a device flag, as the others
    assert FD.main(base + ["--mcep_dim", "24", "--feature_type", "mcep", "--fftl", "128"]) == 2     # 22 050 Hz needs n_fft >= 160
    assert not os.listdir(str(tmp_path / "h5"))


def test_symbols_are_bound_and_null_pointers_are_refused():
    lib = _lib.lib()
    for name in ("swn_envelope", "swn_envelope_table_doubles", "swn_envelope_work_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.EnvelopeEntry) == 48
    assert lib.swn_abi_version() == 3
    null = ctypes.c_void_p(None)
    call = lambda **kw: lib.swn_envelope(*[{**dict(fs=22050.0, n_fft=1024, hop=110, order=49, floor=1e-5, q1=-0.15, default_f0=500.0,
                                                   what=0, tables=null, entries=None, n=1, work=null, stream=null), **kw}[k]
                                           for k in ("fs", "n_fft", "hop", "order", "floor", "q1", "default_f0", "what", "tables",
                                                     "entries", "n", "work", "stream")])
    assert call() == -2 and b"NULL" in lib.swn_last_error_detail()
    assert lib.swn_envelope_table_doubles(1024, 49) == 1024 + 50 * 513
    assert lib.swn_envelope_table_doubles(1000, 49) == 0 and lib.swn_envelope_table_doubles(1024, 64) == 0
    assert lib.swn_envelope_table_doubles(64, 33) == 0 and lib.swn_envelope_table_doubles(4096, 10) == 0
    assert lib.swn_envelope_work_bytes(1024, 110, None, 1) == 0
    # pointers that are never followed: every refusal comes before a launch
    fake = ctypes.c_void_p(4096)
    entry = lambda **kw: (_lib.EnvelopeEntry * 1)(_lib.EnvelopeEntry(**{**dict(wav_dev=4096, out_dev=4096, f0_dev=4096, t0=0,
                                                                                n_avail=3000, len=3000, f0=0, f1=28, reserved=0,
                                                                                reserved2=0), **kw}))
    good = entry()
    assert lib.swn_envelope_work_bytes(1024, 110, good, 1) > 0
    assert lib.swn_envelope_work_bytes(1000, 110, good, 1) == 0 and lib.swn_envelope_work_bytes(1024, 0, good, 1) == 0
    assert lib.swn_envelope_work_bytes(1024, 110, good, 65) == 0 and lib.swn_envelope_work_bytes(1024, 110, entry(f1=-1), 1) == 0
    full = dict(tables=fake, work=fake, entries=good)
    for bad in (dict(fs=0.0), dict(n_fft=1000), dict(hop=0), dict(hop=4097), dict(order=64), dict(order=-1), dict(floor=0.0),
                dict(q1=float("nan")), dict(default_f0=64.0), dict(default_f0=5513.0), dict(n_fft=128), dict(what=2), dict(what=-1),
                dict(n=0), dict(n=65), dict(tables=null), dict(work=null), dict(entries=None),
                dict(entries=entry(reserved=1)), dict(entries=entry(reserved2=1)), dict(entries=entry(f0_dev=None)),
                dict(entries=entry(wav_dev=None)), dict(entries=entry(out_dev=None)), dict(entries=entry(f1=29)),
                dict(entries=entry(f0=-1)), dict(entries=entry(f0=3, f1=2)), dict(entries=entry(len=0, n_avail=0)),
                dict(entries=entry(n_avail=3001)), dict(entries=entry(n_avail=2999)), dict(entries=entry(t0=1, n_avail=2999)),
                dict(entries=entry(len=-1, f1=24)), dict(entries=entry(t0=2, n_avail=2998, f0=4))):
        assert call(**{**full, **bad}) == -2, bad
        assert lib.swn_last_error_detail().startswith(b"swn_envelope"), bad
    # entries without frames launch nothing and may carry null pointers
    assert call(**{**full, "entries": entry(wav_dev=None, out_dev=None, f0_dev=None, f0=4, f1=4)}) == 0
