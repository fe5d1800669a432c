"""CPU: the band aperiodicity entry points of the C ABI and every refusal that is decided before a device is touched (fake
pointers: nothing is launched), the bands, taps and streaming rule of pitch.py, the bookkeeping of BapStream with a fake operator,
and the extractor's and the stage-1 driver's new arguments."""
import os

import numpy as np
import pytest
import torch

import bap_ref as R
import f0_ref
from shallow_wavenet_amd import _lib, ops, pitch
from shallow_wavenet_amd import feature_extract_driver as FD

NEW_SYMBOLS = ("swn_bap", "swn_bap_reach", "swn_bap_work_bytes")
BAD = -2


def test_symbols_are_exported_bound_and_registered():
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.swn_abi_version() == 3
    assert "bap" in ops.OP_NAMES
    assert str(torch.ops.swn.bap.default._schema).startswith("swn::bap(")
    assert (_lib.BAP_MAX_BANDS, _lib.BAP_MAX_TAPS, _lib.BAP_TILE) == (5, 255, 1280) == (R.MAX_BANDS, R.MAX_TAPS, R.TILE)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "swn_hip.h")).read()
    for name, v in (("SWN_BAP_MAX_BANDS", 5), ("SWN_BAP_MAX_TAPS", 255), ("SWN_BAP_TILE", 1280)):
        assert f"#define {name} {v}\n" in header
    assert "code_aperiodicity" in header and "neither claimed nor pinned" in header      # no claim about WORLD


def test_bands_match_the_stdim_of_run_sh():
    # run.sh: fs 8000 -> stdim 2, 12000 / 16000 -> 3, 22050 -> 4, 24000 -> 5, 44100 / 48000 -> 7 (uv, lf0 and the coded bands)
    for fs, stdim in ((8000, 2), (16000, 3), (22050, 4), (24000, 5), (44100, 7), (48000, 7)):
        assert 2 + len(pitch.bap_bands(fs)) == stdim, fs
        assert pitch.bap_bands(fs) == R.bands(fs)
    assert pitch.bap_bands(22050) == [(1500.0, 4500.0), (4500.0, 7500.0)]
    assert pitch.bap_bands(4000) == []


def test_taps_are_firwin_band_passes():
    h = pitch.bap_taps(22050, pitch.bap_bands(22050))
    assert h.shape == (2, 255) and h.dtype == np.float64 and h.flags["C_CONTIGUOUS"]
    assert np.array_equal(h, R.taps(22050, R.bands(22050), 255))
    assert np.allclose(h, h[:, ::-1], rtol=0, atol=1e-15)                 # linear phase: centred, no group delay left
    # the response: about 1 in the band's middle, small outside
    w = lambda f: np.abs(np.exp(-2j * np.pi * f / 22050 * np.arange(255)) @ h.T)
    assert np.all(np.abs(w(3000.0)[0] - 1.0) < 0.01) and w(6000.0)[0] < 0.01 and w(500.0)[0] < 0.01
    assert np.abs(w(6000.0)[1] - 1.0) < 0.01 and w(3000.0)[1] < 0.01
    assert pitch.bap_taps(8000, [(500.0, 1500.0)], 31).shape == (1, 31)
    for bad in (0, 2, 254, 257, -1):
        with pytest.raises(ValueError, match="n_taps"):
            pitch.bap_taps(22050, [(1500.0, 4500.0)], bad)
    for band in ((0.0, 100.0), (5000.0, 4000.0), (3000.0, 12000.0)):
        with pytest.raises(ValueError, match="band"):
            pitch.bap_taps(22050, [band])


def test_reach_and_frames_ready_are_the_brute_force_rule():
    lib = _lib.lib()
    assert lib.swn_bap_reach(1024, 552, 255) == 1831 == pitch.bap_reach(1024, 552, 255) == R.reach(1024, 552, 255)
    assert lib.swn_bap_reach(16, 2, 1) == 19 and lib.swn_bap_reach(2048, 1535, 255) == 3584 + 254
    for win, hi, T in ((15, 100, 31), (2049, 100, 31), (1024, 1, 31), (1024, 1536, 31), (1024, 552, 0), (1024, 552, 2),
                       (1024, 552, 254), (1024, 552, 257), (1024, 552, -1)):
        assert lib.swn_bap_reach(win, hi, T) == 0
    for hop, win, hi, T in ((110, 1024, 552, 255), (37, 97, 80, 31), (1, 64, 40, 3), (600, 128, 100, 63), (40, 256, 134, 1)):
        S, c = f0_ref.span(win, hi), (T - 1) // 2
        ahead = S - S // 2 + c
        for n in sorted(set(list(range(0, 40)) + [ahead - 1, ahead, ahead + 1, S, S + c, S + 2 * c, S + hop, 5 * hop + S, 7777])):
            for final in (False, True):
                assert pitch.bap_frames_ready(hop, win, hi, T, n, final) == R.frames_ready_brute(hop, win, hi, T, n, final), (hop, n)
        assert pitch.bap_frames_ready(hop, win, hi, T, ahead - 1) == 0 and pitch.bap_frames_ready(hop, win, hi, T, ahead) == 1
    assert 1577 - 1577 // 2 + 127 == 916                                   # the latency the docs quote


def _entry(wav=1, out=1, t0=0, n_avail=3001, length=3001, f0=0, f1=28, reserved=0):
    return _lib.LogMelEntry(wav_dev=wav or None, out_dev=out or None, t0=t0, n_avail=n_avail, len=length, f0=f0, f1=f1,
                            reserved=reserved)


def _call(fs=22050.0, hop=110, win=1024, lag_lo=31, lag_hi=552, threshold=0.1, band_win=256, n_bands=2, n_taps=255, taps=8,
          floor=1e-6, entries=True, n_entries=None, work=8, **kw):
    lib = _lib.lib()
    if entries is True:
        entries = [_entry(**kw)]
    table = (_lib.LogMelEntry * len(entries))(*entries) if entries else None
    return lib.swn_bap(fs, hop, win, lag_lo, lag_hi, threshold, band_win, n_bands, n_taps, taps or None, floor, table,
                       len(entries or []) if n_entries is None else n_entries, work or None, None)


def test_call_checks_its_arguments_before_any_launch():
    """fake non-null addresses: every one of these is refused before the library touches them.  S = 1577, S // 2 = 788, c = 127."""
    detail = lambda: _lib.lib().swn_last_error_detail().decode()
    # everything swn_f0 refuses
    for fs in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(fs=fs) == BAD and "fs" in detail() and detail().startswith("swn_bap")
    for hop in (0, -3, 4097):
        assert _call(hop=hop) == BAD and "hop" in detail()
    for win in (0, 15, 2049):
        assert _call(win=win, band_win=16) == BAD and "win" in detail()
    for lo, hi in ((1, 552), (0, 552), (553, 552), (31, 1536), (31, 4000)):
        assert _call(lag_lo=lo, lag_hi=hi) == BAD and "lag" in detail()
    for th in (0.0, -0.1, 1.0000001, float("nan")):
        assert _call(threshold=th) == BAD and "threshold" in detail()
    assert _call(entries=None, n_entries=1) == BAD and "entries_host" in detail()
    assert _call(wav=0) == BAD and "null" in detail()
    assert _call(out=0) == BAD and "null" in detail()
    assert _call(n_entries=0) == BAD and "n_entries" in detail()
    assert _call(entries=[_entry()] * 65) == BAD and "n_entries" in detail()
    assert _call(reserved=1) == BAD and "reserved" in detail()
    assert _call(length=0, n_avail=0, f1=1) == BAD and "length" in detail()
    assert _call(length=2 ** 30 + 1) == BAD and "length" in detail()
    assert _call(n_avail=3002) == BAD and "window" in detail()
    assert _call(t0=-1) == BAD and "window" in detail()
    assert _call(f0=-1) == BAD and "frame range" in detail()
    assert _call(f0=3, f1=2) == BAD and "frame range" in detail()
    assert _call(f1=29) == BAD and "28 frames" in detail()
    assert _call(entries=[_entry(), _entry(f1=29)]) == BAD and "entry 1" in detail()
    assert _call(hop=1, length=2 ** 25, n_avail=2 ** 25, f1=2 ** 24 + 1) == BAD and "2^24" in detail()
    # the new parameters
    for nb in (0, -1, 6):
        assert _call(n_bands=nb) == BAD and "n_bands" in detail() and detail().startswith("swn_bap")
    for nt in (0, -1, 2, 254, 256, 257):
        assert _call(n_taps=nt) == BAD and "n_taps" in detail()
    for bw in (0, 15, 1025, -1):
        assert _call(band_win=bw) == BAD and "band_win" in detail()
    for fl in (0.0, -1e-6, 1.0, 2.0, float("nan")):
        assert _call(floor=fl) == BAD and "floor" in detail()
    assert _call(taps=0) == BAD and "taps_dev" in detail()
    assert _call(work=0) == BAD and "work_dev" in detail()
    assert _call(work=12) == BAD and "work_dev" in detail()               # doubles need 8-byte alignment


def test_the_window_must_hold_the_halo_on_either_side():
    """frame 10 reads 1100 - 788 - 127 = 185 .. 185 + 1577 + 254 = 2016 (exclusive)"""
    detail = lambda: _lib.lib().swn_last_error_detail().decode()
    ok = dict(t0=185, n_avail=1831, f0=10, f1=10)                        # passes every check that does not need frames
    assert _call(wav=0, out=0, **ok) == 0
    assert _call(t0=186, n_avail=1830, f0=10, f1=11) == BAD and "window holds" in detail()
    assert _call(t0=185, n_avail=1830, f0=10, f1=11) == BAD and "window holds" in detail()
    # what swn_f0 accepts - the frame's own span without the halo - is refused here on either side
    assert _call(t0=312, n_avail=1577 + 127, f0=10, f1=11) == BAD and "window holds" in detail()
    assert _call(t0=185, n_avail=1577 + 127, f0=10, f1=11) == BAD and "window holds" in detail()
    # the last frame, 27, reads 2970 - 915 = 2055 ..: its in-signal samples end at 3000
    assert _call(t0=2056, n_avail=945, f0=27, f1=28) == BAD and "window holds" in detail()
    assert _call(wav=0, out=0, t0=2055, n_avail=946, f0=27, f1=27) == 0
    # with fewer taps the halo shrinks: 31 taps, c = 15
    assert _call(n_taps=31, t0=298, n_avail=1606, f0=10, f1=11) == BAD and "window holds" in detail()
    # a frame that needs samples past the window while the length is unknown: frame 0 reads up to sample 789 + 127 - 1
    assert _call(n_avail=915, length=-1, f0=0, f1=1) == BAD and "unknown" in detail()
    assert _call(t0=185, n_avail=1830, length=-1, f0=10, f1=11) == BAD and "unknown" in detail()


def test_empty_ranges_launch_nothing_and_the_scratch_size():
    assert _call(wav=0, out=0, f0=7, f1=7) == 0
    assert _call(entries=[_entry(wav=0, out=0, f1=0), _entry(wav=0, out=0, length=-1, n_avail=5, f0=0, f1=0)]) == 0
    assert _call(win=2048, band_win=2048, lag_lo=1535, lag_hi=1535, n_bands=5, n_taps=1, wav=0, out=0, f1=0) == 0
    assert _call(win=16, band_win=16, lag_lo=2, lag_hi=2, hop=4096, n_bands=1, floor=0.5, threshold=1.0, wav=0, out=0, f1=0) == 0
    lib = _lib.lib()
    size = lambda entries, hop=110, win=1024, hi=552, nb=2: lib.swn_bap_work_bytes(
        hop, win, hi, nb, (_lib.LogMelEntry * len(entries))(*entries), len(entries))
    assert size([_entry()]) == 2 * (27 * 110 + 1577) * 8                   # the samples frames 0 .. 27 span, per band
    assert size([_entry(f0=10, f1=11)]) == 2 * 1577 * 8
    assert size([_entry(), _entry(f1=0), _entry(f0=3, f1=5)], nb=5) == 5 * ((27 * 110 + 1577) + (110 + 1577)) * 8
    assert size([_entry(f1=0)]) == 0
    for bad in (dict(hop=0), dict(win=15), dict(hi=1536), dict(nb=0), dict(nb=6)):
        assert size([_entry()], **bad) == 0
    assert size([_entry(f0=3, f1=2)]) == 0
    assert lib.swn_bap_work_bytes(110, 1024, 552, 2, None, 1) == 0


class _FakeOp:
    """stands in for ops.bap_impl: records every call, checks it against the rules of the C call (the same entry with an empty
    range passes them; the range's own rule, with the halo, is restated here), returns frame indices"""

    def __init__(self):
        self.calls = []

    def __call__(self, wav, taps, t0s, n_avails, lens, f0s, f1s, fs, hop, win, lag_lo, lag_hi, threshold, band_win, floor):
        (t0,), (na,), (ln,), (f0,), (f1,) = t0s, n_avails, lens, f0s, f1s
        B, T = taps.shape
        assert wav.shape == (1, na) and f1 > f0 and taps.dtype == torch.float64
        assert _call(fs, hop, win, lag_lo, lag_hi, threshold, band_win, B, T, floor=floor, t0=t0, n_avail=na, length=ln, f0=f0, f1=f0,
                     wav=0, out=0) == 0
        S, c = win + lag_hi + 1, (T - 1) // 2
        lo, hi = max(0, f0 * hop - S // 2 - c), (f1 - 1) * hop - S // 2 + S - 1 + c
        if ln == -1:
            assert hi < t0 + na
        else:
            assert f1 <= 1 + ln // hop
            hi = min(hi, ln - 1)
        assert t0 <= lo and hi < t0 + na
        self.calls.append(dict(t0=t0, n_avail=na, len=ln, f0=f0, f1=f1, first=float(wav[0, 0]) if na else None))
        return torch.arange(f0, f1, dtype=torch.float32)[None, :, None].expand(1, f1 - f0, 2 + B).clone()


@pytest.mark.parametrize("hop,win,minf0,T,chunks", [(110, 1024, 40.0, 255, [1103] * 4), (110, 1024, 40.0, 255, [1] * 1000 + [37] * 30),
                                                    (1, 64, 200.0, 3, [37] * 5), (37, 97, 100.0, 31, [160] * 7 + [5]),
                                                    (600, 128, 80.0, 63, [1000, 1, 7, 250, 1500]),
                                                    (40, 256, 60.0, 1, [16, 1, 391, 8, 1, 160])])
def test_stream_bookkeeping(hop, win, minf0, T, chunks):
    fs = 22050 if win == 1024 else 8000
    taps = np.ones((2, T)) / T
    ext = pitch.BandAperiodicityExtractor(fs, hop, minf0, 700.0 if fs == 22050 else 1000.0, win, taps=taps, band_win=64, device="cpu")
    fake = ext._op = _FakeOp()
    st = pitch.BapStream(ext)
    S, c = ext.span, (T - 1) // 2
    assert ext.reach == S + 2 * c == R.reach(win, ext.lag_hi, T)
    total, got = 0, []
    for n in chunks:
        out = st.push(torch.arange(total, total + n, dtype=torch.float32))        # sample value = its absolute index
        total += n
        want = R.frames_ready_brute(hop, win, ext.lag_hi, T, total, False)
        assert st.n_frames == want == st.computable(total) and st.n_received == total
        assert out.shape[1] == 4
        got.append(out)
        # only the tail later frames still read is kept: from the halo before the start of the next frame
        assert st.t0 == min(total, max(0, st.n_frames * hop - S // 2 - c))
        assert st._buf.numel() == total - st.t0 and (st._buf.numel() == 0 or float(st._buf[0]) == st.t0)
        assert st._buf.numel() <= ext.reach + hop + n
    for call in fake.calls:
        assert call["len"] == -1 and call["first"] == call["t0"]
    n_push_calls, before = len(fake.calls), st.n_frames
    got.append(st.finish())
    F = 1 + total // hop
    assert st.n_frames == F and st.finished
    assert len(fake.calls) == n_push_calls + (1 if F > before else 0)
    if F > before:
        assert fake.calls[-1]["len"] == total and (fake.calls[-1]["f0"], fake.calls[-1]["f1"]) == (before, F)
    frames = torch.cat(got)
    assert frames.shape == (F, 4) and torch.equal(frames[:, 3], torch.arange(F, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="finished"):
        st.push(torch.zeros(3))


def test_extractor_arguments():
    ext = pitch.BandAperiodicityExtractor(22050, 110, device="cpu")
    assert (ext.minf0, ext.maxf0, ext.win, ext.threshold, ext.lag_lo, ext.lag_hi, ext.span) == (40.0, 700.0, 1024, 0.1, 31, 552, 1577)
    assert (ext.n_bands, ext.n_taps, ext.band_win, ext.floor, ext.reach) == (2, 255, 256, 1e-6, 1831)
    assert ext.bands == pitch.bap_bands(22050) and ext.frame_count(66000) == 601
    assert ext.taps.dtype == torch.float64 and tuple(ext.taps.shape) == (2, 255) and ext.taps.is_contiguous()
    assert np.array_equal(ext.taps.numpy(), pitch.bap_taps(22050, pitch.bap_bands(22050)))
    assert isinstance(ext, pitch.F0Extractor)
    assert pitch.BandAperiodicityExtractor(22050, 110, win=128, band_win=256, device="cpu").band_win == 128    # clipped to win
    assert pitch.BandAperiodicityExtractor(8000, 40, bands=[(500, 1500)], n_taps=31, device="cpu").n_bands == 1
    with pytest.raises(ValueError, match="no aperiodicity band"):
        pitch.BandAperiodicityExtractor(8000, 40, device="cpu")
    for bad in (dict(hop=0), dict(win=15), dict(threshold=0.0), dict(minf0=10.0), dict(n_taps=254), dict(n_taps=257),
                dict(band_win=15), dict(floor=0.0), dict(floor=1.0), dict(bands=[(1500, 4500)] * 6), dict(bands=[(4500, 1500)]),
                dict(taps=np.ones((2, 4))), dict(taps=np.ones((6, 3))), dict(taps=np.ones(5))):
        with pytest.raises(ValueError):
            pitch.BandAperiodicityExtractor(**{**dict(fs=22050, hop=110, device="cpu"), **bad})
    with pytest.raises(RuntimeError, match="HIP device"):                 # no torch fall-back
        ext(torch.zeros(1, 3000))
    with pytest.raises(ValueError, match="at least one sample"):
        pitch.BapStream(ext).finish()
    assert "aperiodicity coding" not in pitch.__doc__ and "pool variant" in pitch.__doc__
    assert "neither claimed nor pinned" in pitch.__doc__
    # the op's shape inference runs without a device and refuses what the library refuses
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        wav, taps = torch.empty(3, 5000), torch.empty(2, 255, dtype=torch.float64)
        geom = dict(fs=22050.0, hop=110, win=1024, lag_lo=31, lag_hi=552, threshold=0.1, band_win=256, floor=1e-6)
        out = torch.ops.swn.bap(wav, taps, [0] * 3, [5000] * 3, [5000] * 3, [0, 2, 7], [46, 30, 7], *geom.values())
        assert tuple(out.shape) == (3, 46, 4) and out.dtype == torch.float32
        for bad, what in ((dict(lag_lo=1), "lags"), (dict(hop=0), "hop"), (dict(band_win=15), "band_win"), (dict(band_win=1025), "band_win"),
                          (dict(floor=0.0), "floor"), (dict(floor=1.0), "floor")):
            with pytest.raises(RuntimeError, match=what):
                torch.ops.swn.bap(wav, taps, [0] * 3, [5000] * 3, [5000] * 3, [0] * 3, [46] * 3, *{**geom, **bad}.values())
        for bad_taps, what in ((torch.empty(2, 254, dtype=torch.float64), "taps"), (torch.empty(6, 255, dtype=torch.float64), "bands"),
                               (torch.empty(2, 255), "float64")):
            with pytest.raises(RuntimeError, match=what):
                torch.ops.swn.bap(wav, bad_taps, [0] * 3, [5000] * 3, [5000] * 3, [0] * 3, [46] * 3, *geom.values())


def test_driver_arguments():
    p = FD.build_parser()
    a = p.parse_args([])
    assert (a.bap, a.bap_string_path, a.bap_taps, a.bap_win) == (False, "/feat_bap", 255, 256)
    a = p.parse_args(["--bap", "true", "--bap_string_path", "/bap", "--bap_taps", "127", "--bap_win", "512"])
    assert (a.bap, a.bap_string_path, a.bap_taps, a.bap_win) == (True, "/bap", 127, 512)
    for flag in ("bap", "bap_string_path", "bap_taps", "bap_win"):
        assert "not a reference flag" in next(x.help for x in p._actions if x.dest == flag)


def test_driver_refuses_bap_with_world_and_without_bands(tmp_path, caplog):
    p = FD.build_parser()
    a = p.parse_args(["--feature_type", "world", "--bap", "true", "--hdf5dir", str(tmp_path)])
    with caplog.at_level("ERROR"):
        assert FD.extract_files([], a, device="cpu") == 2
    assert any("--bap" in r.getMessage() for r in caplog.records)
    caplog.clear()
    a = p.parse_args(["--fs", "8000", "--bap", "true", "--hdf5dir", str(tmp_path)])       # no band below 12 kHz
    with caplog.at_level("ERROR"):
        assert FD.extract_files([], a, device="cpu") == 2
    assert any("no aperiodicity band" in r.getMessage() for r in caplog.records)
