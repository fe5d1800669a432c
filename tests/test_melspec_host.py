"""CPU: the log-mel entry points of the C ABI and every refusal that is decided before a device is touched (fake pointers:
nothing is launched), the empty-filter ValueError, the bookkeeping of LogMelStream with a fake operator, and the stage-1
driver's argument parsing and output naming."""
import ctypes
import os

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, melspec, ops
from shallow_wavenet_amd import feature_extract_driver as FD

NEW_SYMBOLS = ("swn_logmel", "swn_logmel_table_floats", "swn_logmel_work_bytes")


def test_symbols_are_exported_bound_and_registered():
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.swn_abi_version() == 3
    assert "logmel" in ops.OP_NAMES
    assert str(torch.ops.swn.logmel.default._schema).startswith("swn::logmel(")
    assert ctypes.sizeof(_lib.LogMelEntry) == 40
    assert _lib.LOGMEL_MAX_MELS == 128 and _lib.LOGMEL_MAX_ENTRIES == 64


def test_size_queries():
    lib = _lib.lib()
    assert lib.swn_logmel_table_floats(1024, 80) == 2 * 1024 + 2 * 513
    assert lib.swn_logmel_table_floats(32, 1) == 2 * 32 + 2 * 17
    for n, m in ((0, 8), (16, 8), (48, 8), (2080, 8), (1024, 0), (1024, 129)):
        assert lib.swn_logmel_table_floats(n, m) == 0
    en = (_lib.LogMelEntry * 2)(_entry(length=3001, f1=28), _entry(length=600, n_avail=600, f1=5))
    # 2 + 1 tiles of 16 frames x (513 bins padded to 516) floats
    assert lib.swn_logmel_work_bytes(1024, 110, en, 2) == 3 * 16 * 516 * 4
    assert lib.swn_logmel_work_bytes(1024, 110, en, 0) == 0 and lib.swn_logmel_work_bytes(1024, 0, en, 2) == 0
    assert lib.swn_logmel_work_bytes(1024, 110, None, 2) == 0


def _entry(wav=1, out=1, t0=0, n_avail=3001, length=3001, f0=0, f1=28, reserved=0):
    return _lib.LogMelEntry(wav_dev=wav or None, out_dev=out or None, t0=t0, n_avail=n_avail, len=length, f0=f0, f1=f1,
                            reserved=reserved)


def _call(n_fft=1024, hop=110, n_mels=4, floor=1e-5, linear=0, tables=1, bank=True, entries=True, n_entries=None, work=1,
          bank_codes=None, **kw):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    codes = bank_codes if bank_codes is not None else [(10 * m + 1) | (12 << 16) for m in range(max(n_mels, 1))]
    bank_c = (ctypes.c_int32 * len(codes))(*codes) if bank else None
    if entries is True:
        entries = [_entry(**kw)]
    table = (_lib.LogMelEntry * len(entries))(*entries) if entries else None
    return lib.swn_logmel(n_fft, hop, n_mels, floor, linear, p(tables), bank_c, table,
                          len(entries or []) if n_entries is None else n_entries, p(work), None)


def test_call_checks_its_arguments_before_any_launch():
    """fake non-null addresses: every one of these is refused before the library touches them"""
    detail = lambda: _lib.lib().swn_last_error_detail().decode()
    BAD = -2
    # sizes
    for n in (0, 16, 48, 1000, 2080):
        assert _call(n_fft=n) == BAD and "n_fft" in detail()
    assert _call(hop=0) == BAD and "hop" in detail()
    assert _call(hop=1025) == BAD and "hop" in detail()
    assert _call(n_mels=0) == BAD and "n_mels" in detail()
    assert _call(n_mels=129) == BAD and "n_mels" in detail()
    for fl in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(floor=fl) == BAD and "floor" in detail()
    assert _call(linear=2) == BAD and "linear" in detail()
    # pointers
    assert _call(tables=0) == BAD and _call(work=0) == BAD and _call(bank=False) == BAD and _call(entries=None, n_entries=1) == BAD
    assert _call(wav=0) == BAD and "null" in detail()
    assert _call(out=0) == BAD and "null" in detail()
    assert _call(n_entries=0) == BAD and "n_entries" in detail()
    assert _call(entries=[_entry()] * 65) == BAD and "n_entries" in detail()
    assert _call(reserved=1) == BAD and "reserved" in detail()
    # the bank
    assert _call(bank_codes=[500 | (14 << 16)] * 4) == BAD and "filter 0" in detail()        # 500 + 14 > 513 bins
    assert _call(bank_codes=[5] * 4) == BAD and "filter 0" in detail()                       # a run of no bin
    assert _call(n_mels=128, bank_codes=[0 | (9 << 16)] * 128) == BAD and "weights" in detail()      # 1 152 > 2 x 513
    # lengths
    assert _call(length=512, n_avail=512, f1=1) == BAD and "length" in detail()              # len <= n_fft / 2
    assert _call(length=-2) == BAD
    assert _call(n_avail=3002) == BAD and "window" in detail()                               # the window leaves the signal
    assert _call(t0=-1) == BAD and _call(n_avail=-1) == BAD
    # frame ranges
    assert _call(f0=-1) == BAD and _call(f0=3, f1=2) == BAD
    assert _call(f1=29) == BAD and "28 frames" in detail()                                   # 1 + 3001 // 110 = 28
    # a frame whose span leaves the available window: frame 5 starts at 550 - 512 = 38
    assert _call(t0=39, n_avail=2962, f0=5, f1=6) == BAD and "window" in detail()
    assert _call(t0=38, n_avail=1023, f0=5, f1=6) == BAD and "window" in detail()            # ... and ends at 1061
    # frame 0 reads sample 512 through the left reflection
    assert _call(n_avail=512, length=-1, f0=0, f1=1) == BAD and "unknown" in detail()
    # the reflected end: frame 27 spans 2458 .. 3481, back to sample 2519 - it needs the total length ...
    assert _call(t0=2458, n_avail=543, length=-1, f0=27, f1=28) == BAD and "unknown" in detail()
    # ... and with it, a window from 2458 on is enough, one from 2459 on is not
    assert _call(t0=2459, n_avail=542, f0=27, f1=28) == BAD and "window" in detail()
    # a second entry is checked like the first
    assert _call(entries=[_entry(), _entry(f1=29)]) == BAD and "entry 1" in detail()


def test_empty_ranges_launch_nothing():
    """entries without frames may carry null pointers; a call without any frame returns before the launch"""
    assert _call(tables=0, work=0, wav=0, out=0, f0=7, f1=7) == 0
    assert _call(tables=0, work=0, entries=[_entry(wav=0, out=0, f1=0), _entry(wav=0, out=0, length=-1, n_avail=5, f0=0, f1=0)]) == 0
    # a window that holds what the range reads passes every check of the work-size query (no launch behind it)
    lib = _lib.lib()
    ok = (_lib.LogMelEntry * 1)(_entry(t0=38, n_avail=1024, length=-1, f0=5, f1=6))
    assert lib.swn_logmel_work_bytes(1024, 110, ok, 1) == 16 * 516 * 4
    ok = (_lib.LogMelEntry * 1)(_entry(t0=2458, n_avail=543, f0=27, f1=28))
    assert lib.swn_logmel_work_bytes(1024, 110, ok, 1) == 16 * 516 * 4
    ok = (_lib.LogMelEntry * 1)(_entry(n_avail=513, length=-1, f0=0, f1=1))
    assert lib.swn_logmel_work_bytes(1024, 110, ok, 1) == 16 * 516 * 4


def test_a_filter_without_a_bin_is_a_value_error():
    with pytest.raises(ValueError, match="covers no bin"):
        melspec.tables(22050, 64, 80)
    with pytest.raises(ValueError, match="covers no bin"):
        melspec.LogMelExtractor(22050, 64, 16, 80, device="cpu")
    melspec.tables(22050, 1024, 80)
    for bad in (dict(n_mels=0), dict(n_mels=129), dict(fmin=-1.0), dict(fmin=4000.0, fmax=4000.0), dict(fmax=12000.0)):
        with pytest.raises(ValueError):
            melspec.tables(**{**dict(fs=22050, n_fft=1024, n_mels=80), **bad})
    with pytest.raises(ValueError):
        melspec.LogMelExtractor(22050, 1000, 110, 80, device="cpu")
    with pytest.raises(ValueError, match="hop"):
        melspec.LogMelExtractor(22050, 1024, 1025, 80, device="cpu")
    with pytest.raises(ValueError, match="floor"):
        melspec.LogMelExtractor(22050, 1024, 110, 80, floor=0.0, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):                 # no torch fall-back
        melspec.LogMelExtractor(22050, 1024, 110, 80, device="cpu")(torch.zeros(1, 3000))
    with pytest.raises(ValueError, match="longer than"):
        melspec.LogMelExtractor(22050, 1024, 110, 80, device="cpu")(torch.zeros(1, 512))


class _FakeOp:
    """stands in for ops.logmel_impl: records every call, checks it against the rules of the C call, returns frame indices"""

    def __init__(self):
        self.calls = []

    def __call__(self, wav, table, bank, t0s, n_avails, lens, f0s, f1s, n_fft, hop, floor, linear):
        (t0,), (na,), (ln,), (f0,), (f1,) = t0s, n_avails, lens, f0s, f1s
        assert wav.shape == (1, na)
        en = (_lib.LogMelEntry * 1)(_entry(t0=t0, n_avail=na, length=ln, f0=f0, f1=f1))
        assert _lib.lib().swn_logmel_work_bytes(n_fft, hop, en, 1) > 0, _lib.lib().swn_last_error_detail().decode()
        self.calls.append(dict(t0=t0, n_avail=na, len=ln, f0=f0, f1=f1, first=float(wav[0, 0])))
        return torch.arange(f0, f1, dtype=torch.float32)[None, :, None].expand(1, f1 - f0, len(bank)).clone()


@pytest.mark.parametrize("n_fft,hop,chunks", [(1024, 110, [1103] * 4), (1024, 110, [1] * 520 + [37] * 30), (64, 1, [37] * 5),
                                              (96, 37, [160] * 7 + [5]), (2048, 2048, [1103] * 5), (32, 8, [16, 1, 7, 8, 8, 1, 160])])
def test_stream_bookkeeping(n_fft, hop, chunks):
    ext = melspec.LogMelExtractor(22050, n_fft, hop, 4, device="cpu")
    fake = ext._op = _FakeOp()
    st = melspec.LogMelStream(ext)
    total, got, half = 0, [], n_fft // 2
    for n in chunks:
        out = st.push(torch.arange(total, total + n, dtype=torch.float32))        # sample value = its absolute index
        total += n
        # frame 0 needs sample n_fft / 2, frame f >= 1 needs f hop + n_fft / 2 - 1
        want = 0 if total <= half else 1 + (total - half) // hop
        assert st.n_frames == want == st.computable(total) and st.n_received == total
        got.append(out)
        # only the tail later frames still read is kept: from the start of the next frame, less the one sample the
        # reflected end can reach back
        assert st.t0 == max(0, st.n_frames * hop - half - 1)
        assert st._buf.numel() == total - st.t0 and (st._buf.numel() == 0 or float(st._buf[0]) == st.t0)
        assert st._buf.numel() <= n_fft + hop + 1 + n
    for c in fake.calls:
        assert c["len"] == -1 and c["first"] == c["t0"]
    n_push_calls, before = len(fake.calls), st.n_frames
    got.append(st.finish())
    F = 1 + total // hop
    assert st.n_frames == F and st.finished
    if F > before:                                                       # the rest in one call that knows the length
        assert len(fake.calls) == n_push_calls + 1
        assert fake.calls[-1]["len"] == total and (fake.calls[-1]["f0"], fake.calls[-1]["f1"]) == (before, F)
    else:
        assert len(fake.calls) == n_push_calls
    frames = torch.cat(got)
    assert frames.shape == (F, 4) and torch.equal(frames[:, 0], torch.arange(F, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="finished"):
        st.push(torch.zeros(3))
    with pytest.raises(RuntimeError, match="finished"):
        st.finish()


def test_stream_too_short_to_finish():
    ext = melspec.LogMelExtractor(8000, 32, 8, 4, device="cpu")
    ext._op = _FakeOp()
    st = melspec.LogMelStream(ext)
    assert st.push(torch.zeros(16)).shape == (0, 4)
    with pytest.raises(ValueError, match="longer than"):
        st.finish()


def test_driver_arguments_and_output_naming(tmp_path):
    p = FD.build_parser()
    a = p.parse_args([])
    assert (a.fs, a.shiftms, a.fftl, a.highpass_cutoff, a.n_jobs, a.verbose) == (22050, 5.0, 1024, 70, 1, 1)
    assert (a.feature_type, a.n_mels, a.fmin, a.fmax, a.hop, a.floor, a.string_path) == ("logmel", 80, 0.0, None, None, 1e-5,
                                                                                           "/feat_logmel")
    assert FD.hop_of(a) == 110                                           # round(110.25)
    a = p.parse_args(["--expdir", "e", "--waveforms", "w", "--hdf5dir", "h", "--wavdir", "v", "--fs", "16000", "--shiftms", "5",
                      "--fftl", "512", "--highpass_cutoff", "0", "--n_jobs", "3", "--verbose", "0", "--n_mels", "40", "--fmin",
                      "55", "--fmax", "7600", "--floor", "1e-4", "--string_path", "/mel"])
    assert FD.hop_of(a) == 80 and (a.expdir, a.waveforms, a.hdf5dir, a.wavdir) == ("e", "w", "h", "v")
    assert (a.n_mels, a.fmin, a.fmax, a.floor, a.string_path, a.highpass_cutoff) == (40, 55.0, 7600.0, 1e-4, "/mel", 0)
    assert FD.hop_of(p.parse_args(["--hop", "128"])) == 128
    with pytest.raises(SystemExit):
        p.parse_args(["--feature_type", "lpc"])
    for flag in ("feature_type", "n_mels", "fmin", "fmax", "hop", "floor", "string_path"):
        assert "not a reference flag" in next(x.help for x in p._actions if x.dest == flag)
    # <hdf5dir>/<name>.h5 with h5py, the .npz side format without
    try:
        import h5py  # noqa: F401
        ext = ".h5"
    except ImportError:
        ext = ".npz"
    assert FD.feature_path("/data/hdf5", "/corpus/spk/utt_001.wav") == "/data/hdf5/utt_001" + ext
    assert FD.main([]) == 2                                              # --waveforms and --hdf5dir are required
    # WORLD / SPTK features keep needing pyworld / pysptk
    try:
        import pyworld  # noqa: F401
        import pysptk  # noqa: F401
    except ImportError:
        from scipy.io import wavfile
        wav = tmp_path / "a.wav"
        wavfile.write(str(wav), 22050, (np.sin(np.arange(4000) * 0.1) * 8000).astype(np.int16))
        with pytest.raises(ImportError, match="is required for WORLD / SPTK analysis"):
            FD.main(["--waveforms", str(tmp_path), "--hdf5dir", str(tmp_path / "h5"), "--feature_type", "world", "--verbose", "0"])
        assert not os.path.exists(FD.feature_path(str(tmp_path / "h5"), str(wav)))


def _write_wav(path, fs, n=4000):
    from scipy.io import wavfile
    wavfile.write(str(path), fs, (np.sin(np.arange(n) * 0.1) * 8000).astype(np.int16))


def test_driver_refuses_a_wav_of_another_sampling_frequency(tmp_path):
    _write_wav(tmp_path / "a.wav", 16000)
    args = FD.build_parser().parse_args(["--highpass_cutoff", "0"])
    with pytest.raises(ValueError, match="sampling frequency 16000 does not match --fs 22050"):
        FD.load_waveform(str(tmp_path / "a.wav"), args)
    args = FD.build_parser().parse_args(["--highpass_cutoff", "0", "--fs", "16000"])
    assert FD.load_waveform(str(tmp_path / "a.wav"), args).shape == (4000,)


def test_driver_with_workers_returns_when_a_worker_dies(tmp_path):
    """--n_jobs 2: workers that raise (here: WORLD features without pyworld) give a non-zero return, not a parent that waits"""
    try:
        import pyworld  # noqa: F401
        pytest.skip("pyworld is importable: the workers would not fail")
    except ImportError:
        pass
    for name in ("a.wav", "b.wav"):
        _write_wav(tmp_path / name, 22050)
    rc = FD.main(["--waveforms", str(tmp_path), "--hdf5dir", str(tmp_path / "h5"), "--feature_type", "world", "--n_jobs", "2",
                  "--verbose", "0"])
    assert rc != 0
