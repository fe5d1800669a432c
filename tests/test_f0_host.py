"""CPU: the F0 entry points of the C ABI and every refusal that is decided before a device is touched (fake pointers: nothing is
launched), the lags and the streaming rule of pitch.py, the bookkeeping of F0Stream with a fake operator, uv_lf0, and the stage-1
driver's new arguments."""
import ctypes
import os

import numpy as np
import pytest
import torch

import f0_ref as R
from shallow_wavenet_amd import _lib, dsp, ops, pitch
from shallow_wavenet_amd import feature_extract_driver as FD

NEW_SYMBOLS = ("swn_f0", "swn_f0_span")


def test_symbols_are_exported_bound_and_registered():
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.swn_abi_version() == 3
    assert "f0" in ops.OP_NAMES
    assert str(torch.ops.swn.f0.default._schema).startswith("swn::f0(")
    assert (_lib.F0_MAX_HOP, _lib.F0_MIN_WIN, _lib.F0_MAX_WIN, _lib.F0_MAX_LAG) == (4096, 16, 2048, 1536)
    assert (R.MAX_HOP, R.MIN_WIN, R.MAX_WIN, R.MAX_LAG) == (4096, 16, 2048, 1536)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "swn_hip.h")).read()
    for name, v in (("SWN_F0_MAX_HOP", 4096), ("SWN_F0_MIN_WIN", 16), ("SWN_F0_MAX_WIN", 2048), ("SWN_F0_MAX_LAG", 1536)):
        assert f"#define {name} {v}\n" in header


def test_lags_from_hz():
    assert pitch.f0_lags(22050, 40, 700) == (31, 552) == R.lags(22050, 40, 700)
    assert pitch.f0_lags(8000, 100, 1000) == (8, 80)
    assert pitch.f0_lags(16000, 50, 600) == (26, 320)
    assert pitch.f0_lags(8000, 125, 125) == (64, 64)
    for bad in ((22050, 10, 700), (8000, 100, 5000), (8000, 0, 100), (8000, 300, 200), (0, 40, 700)):
        with pytest.raises(ValueError):
            pitch.f0_lags(*bad)
    assert pitch.f0_lags(22050, 14.4, 700)[1] == 1532
    with pytest.raises(ValueError):
        pitch.f0_lags(22050, 14.3, 700)                                   # ceil(1541.96) > 1535


def test_span():
    lib = _lib.lib()
    assert lib.swn_f0_span(1024, 552) == 1577 == pitch.f0_span(1024, 552) == R.span(1024, 552)
    assert lib.swn_f0_span(16, 2) == 19 and lib.swn_f0_span(2048, 1535) == 3584 and lib.swn_f0_span(97, 80) == 178
    for win, hi in ((15, 100), (2049, 100), (0, 100), (-1, 100), (1024, 1), (1024, 1536), (1024, -5)):
        assert lib.swn_f0_span(win, hi) == 0


def test_frames_ready_is_the_brute_force_rule():
    for hop, win, hi in ((110, 1024, 552), (37, 97, 80), (1, 64, 40), (600, 128, 100), (80, 512, 320), (4096, 16, 2)):
        S = R.span(win, hi)
        for n in sorted(set(list(range(0, 40)) + [S // 2 - 1, S // 2, S - S // 2 - 1, S - S // 2, S - S // 2 + 1, S - 1, S, S + 1,
                                                   S + hop - 1, S + hop, 5 * hop, 5 * hop + S, 7777])):
            for final in (False, True):
                assert pitch.f0_frames_ready(hop, win, hi, n, final) == R.frames_ready_brute(hop, win, hi, n, final), (hop, win, hi, n)
        # the latency: frame f appears with sample f hop + (S - S // 2) - 1
        assert pitch.f0_frames_ready(hop, win, hi, S - S // 2 - 1) == 0 and pitch.f0_frames_ready(hop, win, hi, S - S // 2) == 1


def _entry(wav=1, out=1, t0=0, n_avail=3001, length=3001, f0=0, f1=28, reserved=0):
    return _lib.LogMelEntry(wav_dev=wav or None, out_dev=out or None, t0=t0, n_avail=n_avail, len=length, f0=f0, f1=f1,
                            reserved=reserved)


def _call(fs=22050.0, hop=110, win=1024, lag_lo=31, lag_hi=552, threshold=0.1, entries=True, n_entries=None, **kw):
    lib = _lib.lib()
    if entries is True:
        entries = [_entry(**kw)]
    table = (_lib.LogMelEntry * len(entries))(*entries) if entries else None
    return lib.swn_f0(fs, hop, win, lag_lo, lag_hi, threshold, table, len(entries or []) if n_entries is None else n_entries, None)


def test_call_checks_its_arguments_before_any_launch():
    """fake non-null addresses: every one of these is refused before the library touches them.  S = 1577, S // 2 = 788."""
    detail = lambda: _lib.lib().swn_last_error_detail().decode()
    BAD = -2
    # ranges
    for fs in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(fs=fs) == BAD and "fs" in detail() and detail().startswith("swn_f0")
    for hop in (0, -3, 4097):
        assert _call(hop=hop) == BAD and "hop" in detail()
    for win in (0, 15, 2049):
        assert _call(win=win) == BAD and "win" in detail()
    for lo, hi in ((1, 552), (0, 552), (553, 552), (31, 1536), (31, 4000)):
        assert _call(lag_lo=lo, lag_hi=hi) == BAD and "lag" in detail()
    for th in (0.0, -0.1, 1.0000001, float("nan")):
        assert _call(threshold=th) == BAD and "threshold" in detail()
    # pointers, counts, the reserved field
    assert _call(entries=None, n_entries=1) == BAD and "entries_host" in detail()
    assert _call(wav=0) == BAD and "null" in detail()
    assert _call(out=0) == BAD and "null" in detail()
    assert _call(n_entries=0) == BAD and "n_entries" in detail()
    assert _call(entries=[_entry()] * 65) == BAD and "n_entries" in detail()
    assert _call(reserved=1) == BAD and "reserved" in detail()
    # lengths and windows
    assert _call(length=0, n_avail=0, f1=1) == BAD and "length" in detail()
    assert _call(length=-2) == BAD and "length" in detail()
    assert _call(length=2 ** 30 + 1) == BAD and "length" in detail()
    assert _call(n_avail=3002) == BAD and "window" in detail()                               # the window leaves the signal
    assert _call(t0=-1) == BAD and "window" in detail()
    assert _call(n_avail=-1) == BAD and "window" in detail()
    assert _call(t0=2 ** 30, n_avail=1, length=-1) == BAD and "window" in detail()
    # frame ranges
    assert _call(f0=-1) == BAD and "frame range" in detail()
    assert _call(f0=3, f1=2) == BAD and "frame range" in detail()
    assert _call(f1=29) == BAD and "28 frames" in detail()                                   # 1 + 3001 // 110 = 28
    # a frame whose in-signal samples are not all in the window: frame 10 reads 1100 - 788 = 312 .. 1888
    assert _call(t0=313, n_avail=2688, f0=10, f1=11) == BAD and "window holds" in detail()
    assert _call(t0=312, n_avail=1576, f0=10, f1=11) == BAD and "window holds" in detail()
    # the last frame, 27, reads 2182 .. 3758: its in-signal samples end at 3000
    assert _call(t0=2183, n_avail=818, f0=27, f1=28) == BAD and "window holds" in detail()
    # a frame that needs samples past the window while the length is unknown
    assert _call(n_avail=788, length=-1, f0=0, f1=1) == BAD and "unknown" in detail()        # frame 0 reads up to sample 788
    assert _call(t0=312, n_avail=1576, length=-1, f0=10, f1=11) == BAD and "unknown" in detail()
    # a second entry is checked like the first
    assert _call(entries=[_entry(), _entry(f1=29)]) == BAD and "entry 1" in detail()
    # more frames than one call takes
    assert _call(hop=1, length=2 ** 25, n_avail=2 ** 25, f1=2 ** 24 + 1) == BAD and "2^24" in detail()


def test_empty_ranges_launch_nothing():
    """entries without frames may carry null pointers; a call without any frame returns before the launch - so these calls, which
    pass every check, show what the checks accept"""
    assert _call(wav=0, out=0, f0=7, f1=7) == 0
    assert _call(entries=[_entry(wav=0, out=0, f1=0), _entry(wav=0, out=0, length=-1, n_avail=5, f0=0, f1=0)]) == 0
    assert _call(wav=0, out=0, length=1, n_avail=1, f0=1, f1=1) == 0
    assert _call(threshold=1.0, win=16, lag_lo=2, lag_hi=2, hop=4096, wav=0, out=0, f1=0) == 0
    assert _call(win=2048, lag_lo=1535, lag_hi=1535, wav=0, out=0, f1=0) == 0


class _FakeOp:
    """stands in for ops.f0_impl: records every call, checks it against the rules of the C call (the same entry with an empty
    range passes them; the range's own rule is restated here), returns frame indices"""

    def __init__(self):
        self.calls = []

    def __call__(self, wav, t0s, n_avails, lens, f0s, f1s, fs, hop, win, lag_lo, lag_hi, threshold):
        (t0,), (na,), (ln,), (f0,), (f1,) = t0s, n_avails, lens, f0s, f1s
        assert wav.shape == (1, na) and f1 > f0
        assert _call(fs, hop, win, lag_lo, lag_hi, threshold, t0=t0, n_avail=na, length=ln, f0=f0, f1=f0, wav=0, out=0) == 0
        S = win + lag_hi + 1
        lo, hi = max(0, f0 * hop - S // 2), (f1 - 1) * hop - S // 2 + S - 1
        if ln == -1:
            assert hi < t0 + na
        else:
            assert f1 <= 1 + ln // hop
            hi = min(hi, ln - 1)
        assert t0 <= lo and hi < t0 + na
        self.calls.append(dict(t0=t0, n_avail=na, len=ln, f0=f0, f1=f1, first=float(wav[0, 0]) if na else None))
        return torch.arange(f0, f1, dtype=torch.float32)[None, :, None].expand(1, f1 - f0, 2).clone()


@pytest.mark.parametrize("hop,win,minf0,chunks", [(110, 1024, 40.0, [1103] * 4), (110, 1024, 40.0, [1] * 900 + [37] * 30),
                                                  (1, 64, 200.0, [37] * 5), (37, 97, 100.0, [160] * 7 + [5]),
                                                  (600, 128, 80.0, [1000, 1, 7, 250, 1500]), (40, 256, 60.0, [16, 1, 391, 8, 1, 160])])
def test_stream_bookkeeping(hop, win, minf0, chunks):
    fs = 22050 if win == 1024 else 8000
    ext = pitch.F0Extractor(fs, hop, minf0, 700.0 if fs == 22050 else 1000.0, win, device="cpu")
    fake = ext._op = _FakeOp()
    st = pitch.F0Stream(ext)
    S = ext.span
    assert S == win + ext.lag_hi + 1
    total, got = 0, []
    for n in chunks:
        out = st.push(torch.arange(total, total + n, dtype=torch.float32))        # sample value = its absolute index
        total += n
        want = R.frames_ready_brute(hop, win, ext.lag_hi, total, False)
        assert st.n_frames == want == st.computable(total) and st.n_received == total
        got.append(out)
        # only the tail later frames still read is kept: from the start of the next frame
        assert st.t0 == min(total, max(0, st.n_frames * hop - S // 2))
        assert st._buf.numel() == total - st.t0 and (st._buf.numel() == 0 or float(st._buf[0]) == st.t0)
        assert st._buf.numel() <= S + hop + n
    for c in fake.calls:
        assert c["len"] == -1 and c["first"] == c["t0"]
    n_push_calls, before = len(fake.calls), st.n_frames
    got.append(st.finish())
    F = 1 + total // hop
    assert st.n_frames == F and st.finished
    assert len(fake.calls) == n_push_calls + (1 if F > before else 0)
    if F > before:
        assert fake.calls[-1]["len"] == total and (fake.calls[-1]["f0"], fake.calls[-1]["f1"]) == (before, F)
    frames = torch.cat(got)
    assert frames.shape == (F, 2) and torch.equal(frames[:, 0], torch.arange(F, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="finished"):
        st.push(torch.zeros(3))
    with pytest.raises(RuntimeError, match="finished"):
        st.finish()


def test_extractor_arguments():
    ext = pitch.F0Extractor(22050, 110, device="cpu")
    assert (ext.minf0, ext.maxf0, ext.win, ext.threshold, ext.lag_lo, ext.lag_hi, ext.span) == (40.0, 700.0, 1024, 0.1, 31, 552, 1577)
    assert ext.frame_count(66000) == 601
    for bad in (dict(hop=0), dict(hop=4097), dict(win=15), dict(win=2049), dict(threshold=0.0), dict(threshold=1.5),
                dict(minf0=10.0), dict(maxf0=20000.0)):
        with pytest.raises(ValueError):
            pitch.F0Extractor(**{**dict(fs=22050, hop=110, device="cpu"), **bad})
    with pytest.raises(RuntimeError, match="HIP device"):                 # no torch fall-back
        ext(torch.zeros(1, 3000))
    with pytest.raises(ValueError, match="at least one sample"):
        ext([torch.zeros(0)])
    st = pitch.F0Stream(ext)
    with pytest.raises(ValueError, match="at least one sample"):
        st.finish()
    # the op's shape inference runs without a device and refuses what the library refuses
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        wav = torch.empty(3, 5000)
        out = torch.ops.swn.f0(wav, [0] * 3, [5000] * 3, [5000] * 3, [0, 2, 7], [46, 30, 7], 22050.0, 110, 1024, 31, 552, 0.1)
        assert tuple(out.shape) == (3, 46, 2) and out.dtype == torch.float32
        for bad, what in ((dict(lag_lo=1), "lags"), (dict(lag_hi=1536), "lags"), (dict(hop=0), "hop"), (dict(win=2049), "win"),
                          (dict(threshold=0.0), "threshold"), (dict(fs=0.0), "fs")):
            a = {**dict(fs=22050.0, hop=110, win=1024, lag_lo=31, lag_hi=552, threshold=0.1), **bad}
            with pytest.raises(RuntimeError, match=what):
                torch.ops.swn.f0(wav, [0] * 3, [5000] * 3, [5000] * 3, [0] * 3, [46] * 3, *a.values())


def test_uv_lf0_uses_the_helpers_of_dsp():
    f0 = np.array([0, 0, 100, 110, 0, 0, 120, 130, 0], dtype=np.float32)
    out = pitch.uv_lf0(f0, 200)
    assert out.shape == (9, 2) and out.dtype == np.float64
    uv, cont = dsp.continuous_f0(f0)
    assert np.array_equal(out[:, 0], uv) and np.array_equal(out[:, 0], [0, 0, 1, 1, 0, 0, 1, 1, 0])
    assert np.array_equal(out[:, 1], np.log(dsp.low_pass_filter(cont, 200, cutoff=20)))
    assert np.all(np.abs(np.exp(out[:, 1]) - 115.0) < 20.0)
    with pytest.raises(ValueError, match="no voiced frame"):
        pitch.uv_lf0(np.zeros(5), 200)


def test_driver_arguments():
    p = FD.build_parser()
    a = p.parse_args([])
    assert (a.minf0, a.maxf0, a.f0, a.f0_cond, a.f0_string_path, a.f0_win, a.f0_threshold) == (40, 700, False, False, "/feat_f0",
                                                                                              1024, 0.1)
    a = p.parse_args(["--minf0", "70", "--maxf0", "340", "--f0", "true", "--f0_cond", "true", "--f0_string_path", "/f0",
                      "--f0_win", "512", "--f0_threshold", "0.15"])
    assert (a.minf0, a.maxf0, a.f0, a.f0_cond, a.f0_string_path, a.f0_win, a.f0_threshold) == (70, 340, True, True, "/f0", 512, 0.15)
    for flag in ("f0", "f0_cond", "f0_string_path", "f0_win", "f0_threshold"):
        assert "not a reference flag" in next(x.help for x in p._actions if x.dest == flag)
    for flag in ("minf0", "maxf0"):
        assert "not a reference flag" not in next(x.help for x in p._actions if x.dest == flag)
