"""CPU: the stage-1 low cut on the device (swn_lowcut_chunk, swn_logmel_pool_lowcut, melspec.LowCut) - its symbols are exported,
bound and registered, the state query follows the definition, every refusal of both calls is decided before a device is touched
(fake pointers: nothing is launched), the Python classes refuse what they must, the stage-1 driver parses its new flag, and the
references of lowcut_ref.py agree with the definition evaluated by libm's fma."""
import ctypes

import numpy as np
import pytest
import torch

import lowcut_ref as LR
from shallow_wavenet_amd import _lib, dsp, melspec, ops
from shallow_wavenet_amd import feature_extract_driver as FD

BAD = -2
WINDOW = 1024 + 4096


def _detail():
    return _lib.lib().swn_last_error_detail().decode()


def test_symbols_are_exported_bound_and_registered():
    lib = _lib.lib()
    for n in ("swn_lowcut_state_floats", "swn_lowcut_chunk", "swn_logmel_pool_lowcut"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.swn_abi_version() == 3
    assert "lowcut_chunk" in ops.OP_NAMES and "logmel_pool_lowcut" in ops.OP_NAMES
    assert str(torch.ops.swn.lowcut_chunk.default._schema).startswith("swn::lowcut_chunk(Tensor taps, Tensor(a1!) state, ")
    schema = str(torch.ops.swn.logmel_pool_lowcut.default._schema)
    assert schema.startswith("swn::logmel_pool_lowcut(Tensor(a0!) win, Tensor(a1!) hist, ") and schema.endswith("-> Tensor")
    assert ctypes.sizeof(_lib.LowcutEntry) == 32
    assert [f[0] for f in _lib.LowcutEntry._fields_] == ["in_dev", "out_dev", "slot", "n", "flags", "reserved"]
    assert (_lib.LOWCUT_MAX_TAPS, _lib.LOWCUT_TILE, _lib.LOWCUT_MAX_ENTRIES, _lib.LOWCUT_RESET) == (256, 1024, 64, 1)
    assert _lib.LOWCUT_TILE >= _lib.LOWCUT_MAX_TAPS         # only an entry's first tile reads the slot's state


def test_state_query():
    lib = _lib.lib()
    for n in (1, 2, 31, 255, 256):
        assert lib.swn_lowcut_state_floats(n) == n - 1
    for n in (0, -1, 257, 1 << 20):
        assert lib.swn_lowcut_state_floats(n) == 0


# ------------------------------------------------------------------------------------------------------ swn_lowcut_chunk
def _entry(**kw):
    e = dict(in_dev=1 << 20, out_dev=1 << 21, slot=0, n=16, flags=_lib.LOWCUT_RESET, reserved=0)
    e.update(kw)
    return e


def _chunk(n_taps=255, taps=1 << 12, state=1 << 14, capacity=2, entries=None, n_entries=None, table=True):
    """the C entry point with fake (never dereferenced) device addresses: every case here must fail before a device call"""
    entries = [_entry()] if entries is None else entries
    tab = (_lib.LowcutEntry * max(1, len(entries)))(*[_lib.LowcutEntry(**e) for e in entries]) if table else None
    n = len(entries) if n_entries is None else n_entries
    vp = ctypes.c_void_p
    return _lib.lib().swn_lowcut_chunk(n_taps, vp(taps), vp(state), capacity, tab, n, vp(None))


@pytest.mark.parametrize("kw,text", [
    (dict(n_taps=0), "n_taps"), (dict(n_taps=-3), "n_taps"), (dict(n_taps=257), "n_taps"),
    (dict(taps=None), "null"), (dict(state=None), "null"), (dict(table=False), "entries_host"),
    (dict(capacity=0), "capacity"), (dict(capacity=-1), "capacity"), (dict(n_entries=-1), "n_entries"),
    (dict(entries=[_entry(slot=2)]), "slot 2"), (dict(entries=[_entry(slot=-1)]), "slot -1"),
    (dict(entries=[_entry(), _entry(in_dev=1 << 22, out_dev=1 << 23)]), "twice"),
    (dict(entries=[_entry(n=-1)]), "n = -1"),
    (dict(entries=[_entry(flags=2)]), "flag"), (dict(entries=[_entry(flags=3)]), "flag"),
    (dict(entries=[_entry(reserved=1)]), "reserved"),
    (dict(entries=[_entry(in_dev=None)]), "null"), (dict(entries=[_entry(out_dev=None)]), "null"),
    # the ranges of one entry: in place, out one float into in, in one float into out; 16 floats = 64 bytes
    (dict(entries=[_entry(out_dev=1 << 20)]), "overlap"),
    (dict(entries=[_entry(out_dev=(1 << 20) + 60)]), "overlap"),
    (dict(entries=[_entry(out_dev=(1 << 20) - 60)]), "overlap"),
    (dict(entries=[_entry(slot=1), _entry(n=-1)]), "entry 1"),
])
def test_chunk_refusals_come_before_any_launch(kw, text):
    assert _chunk(**kw) == BAD and text in _detail(), _detail()


def test_chunk_calls_that_launch_nothing_succeed():
    assert _chunk(entries=[], n_entries=0) == 0
    assert _chunk(entries=[], n_entries=0, table=False) == 0
    # n == 0 without RESET touches nothing, and carries no pointers
    assert _chunk(entries=[_entry(n=0, flags=0, in_dev=None, out_dev=None)]) == 0
    # n_taps == 1 has no state: RESET of an empty entry is no launch either
    assert _chunk(n_taps=1, entries=[_entry(n=0, in_dev=None, out_dev=None)]) == 0


# ------------------------------------------------------------------------------------------------ swn_logmel_pool_lowcut
def _pool_entry(slot=0, t0=0, n_held=0, n_drop=0, new_off=0, n_new=3001, length=3001, f0=0, f1=28, out_off=0, out_stride=None,
                reserved=0):
    return _lib.LogMelPoolEntry(slot=slot, t0=t0, n_held=n_held, n_drop=n_drop, new_off=new_off, n_new=n_new, len=length, f0=f0,
                                f1=f1, out_off=out_off, out_stride=f1 - f0 if out_stride is None else out_stride,
                                reserved=reserved)


def _pool(n_fft=1024, hop=110, n_mels=4, floor=1e-5, linear=0, tables=1, bank=True, win=1, window=WINDOW, new=1, out=1,
          entries=True, n_entries=None, work=1, n_taps=255, taps=1, hist=1, **kw):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    codes = [(10 * m + 1) | (12 << 16) for m in range(max(n_mels, 1))]
    bank_c = (ctypes.c_int32 * len(codes))(*codes) if bank else None
    if entries is True:
        entries = [_pool_entry(**kw)]
    table = (_lib.LogMelPoolEntry * len(entries))(*entries) if entries else None
    return lib.swn_logmel_pool_lowcut(n_fft, hop, n_mels, floor, linear, p(tables), bank_c, p(win), window, p(new), p(out), table,
                                      len(entries or []) if n_entries is None else n_entries, p(work), n_taps, p(taps), p(hist),
                                      None)


def test_pool_refusals_come_before_any_launch():
    """fake non-null addresses: every one of these is refused before the library touches them"""
    # the new arguments
    for n in (0, -1, 257):
        assert _pool(n_taps=n) == BAD and "n_taps" in _detail()
    assert _pool(taps=0) == BAD and "null" in _detail()
    assert _pool(hist=0) == BAD and "null" in _detail()
    assert "swn_logmel_pool_lowcut" in _detail()                                  # the text names the call that refused
    # ... and every rule of swn_logmel_pool
    for n in (0, 16, 48, 1000, 2080):
        assert _pool(n_fft=n) == BAD and "n_fft" in _detail()
    assert _pool(hop=0) == BAD and "hop" in _detail()
    assert _pool(hop=1025) == BAD and "hop" in _detail()
    assert _pool(n_mels=0) == BAD and "n_mels" in _detail()
    assert _pool(n_mels=129) == BAD and "n_mels" in _detail()
    for fl in (0.0, -1.0, float("nan"), float("inf")):
        assert _pool(floor=fl) == BAD and "floor" in _detail()
    assert _pool(linear=2) == BAD and "linear" in _detail()
    assert _pool(length=512, n_new=512, f1=1) == BAD and "length" in _detail()
    assert _pool(length=3000) == BAD and "window" in _detail()
    for name in ("tables", "work", "win", "new", "out"):
        assert _pool(**{name: 0}) == BAD and "null" in _detail(), name
    assert _pool(bank=False) == BAD and "bank" in _detail()
    assert _pool(entries=None, n_entries=1) == BAD and "entries_host" in _detail()
    assert _pool(n_entries=0) == BAD and "n_entries" in _detail()
    assert _pool(entries=[_pool_entry(slot=i, f1=0, n_new=0, length=-1) for i in range(65)]) == BAD and "n_entries" in _detail()
    assert _pool(reserved=1) == BAD and "reserved" in _detail()
    assert _pool(window=0) == BAD and "window_floats" in _detail()
    two = lambda **kw: [_pool_entry(), _pool_entry(**{**dict(slot=1, new_off=3001, out_off=4 * 28), **kw})]
    assert _pool(entries=two(slot=0)) == BAD and "slot 0" in _detail()
    for name in ("slot", "t0", "n_held", "n_drop", "new_off", "n_new", "out_off", "out_stride"):
        assert _pool(**{name: -1}) == BAD, name
    assert _pool(f0=-1) == BAD and _pool(f0=3, f1=2) == BAD and _pool(length=-2) == BAD
    assert _pool(n_held=10, n_drop=11, t0=0, n_new=3001 - 10) == BAD and "n_drop" in _detail()
    assert _pool(n_new=WINDOW + 1, length=WINDOW + 1) == BAD and "fit the window" in _detail()
    assert _pool(n_held=100, n_drop=50, n_new=2901) == BAD and "window" in _detail()
    assert _pool(length=-1) == BAD and "unknown" in _detail()
    assert _pool(f1=29) == BAD and "28 frames" in _detail()
    assert _pool(out_stride=27) == BAD and "overlap" in _detail()
    assert _pool(entries=two(out_off=0)) == BAD and "overlap" in _detail()
    assert _pool(entries=two(f1=29)) == BAD and "entry 1" in _detail()
    # a call in which nothing moves and no frame is due launches nothing
    assert _pool(entries=[_pool_entry(n_new=0, length=-1, f1=0)], new=0, out=0, tables=0, work=0) == 0


# ------------------------------------------------------------------------------------------------------ the Python classes
def test_lowcut_holds_the_taps_of_the_host_filter():
    cut = melspec.LowCut(22050, device="meta")
    assert cut.n_taps == 255 and cut.state_floats == 254 == _lib.lib().swn_lowcut_state_floats(255)
    assert np.array_equal(cut.taps, dsp.low_cut_taps(22050, 70.0)) and cut.taps.dtype == np.float64
    assert cut._taps.dtype == torch.float64 and cut._taps.shape == (255,)
    assert cut._state.shape == (254,) and cut._state.dtype == torch.float32
    assert melspec.LowCut(16000, cutoff=50.0, capacity=3, device="meta")._state.shape == (3 * 254,)
    assert np.array_equal(melspec.LowCut(16000, cutoff=50.0, device="meta").taps, dsp.low_cut_taps(16000, 50.0))


def test_lowcut_argument_errors():
    for cap in (0, -1, 1.5, None):
        with pytest.raises(ValueError, match="capacity"):
            melspec.LowCut(22050, capacity=cap, device="meta")
    for cutoff in (0.0, -70.0, 11025.0, 20000.0):
        with pytest.raises(ValueError, match="cutoff"):
            melspec.LowCut(22050, cutoff=cutoff, device="meta")
    cut = melspec.LowCut(22050, capacity=3, device="meta")
    assert [cut.open(), cut.open()] == [0, 1]
    assert cut.open(2) == 2
    with pytest.raises(RuntimeError, match="full"):
        cut.open()
    cut.close(1)
    assert cut.open() == 1 and 1 in cut._reset
    with pytest.raises(RuntimeError, match="not free"):
        cut.open(1)
    cut.close(0)
    with pytest.raises(RuntimeError, match="not open"):
        cut.close(0)
    with pytest.raises(RuntimeError, match="not open"):
        cut.run({0: torch.zeros(4)})
    with pytest.raises(RuntimeError, match="not open"):
        cut.run({7: torch.zeros(4)})
    with pytest.raises(ValueError, match="1-D"):
        cut.run({1: torch.zeros(2, 4)})
    assert cut.run({}) == {}
    # the ops refuse host tensors: there is no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.lowcut_chunk_impl(torch.zeros(255, dtype=torch.float64), torch.zeros(254), [torch.zeros(4)], [0], [True], 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        melspec.LowCut(22050, device="cpu")(torch.zeros(1, 600))


def test_streams_and_pools_check_their_low_cut():
    ext = melspec.LogMelExtractor(22050, 1024, 110, 80, device="cpu")
    with pytest.raises(ValueError, match="LowCut"):
        melspec.LogMelStream(ext, low_cut="70 Hz")
    with pytest.raises(ValueError, match="LowCut"):
        melspec.LogMelPool(ext, 2, 400, low_cut=70.0)
    with pytest.raises(ValueError, match="fs"):
        melspec.LogMelStream(ext, low_cut=melspec.LowCut(16000, device="cpu"))
    with pytest.raises(ValueError, match="extractor on"):
        melspec.LogMelPool(ext, 2, 400, low_cut=melspec.LowCut(22050, device="meta"))
    cut = melspec.LowCut(22050, capacity=1, device="cpu")
    # the default takes today's path and owns no history
    pool = melspec.LogMelPool(ext, 2, 400)
    assert pool.low_cut is None and pool.hist is None and pool._op is ops.logmel_pool_impl
    assert melspec.LogMelStream(ext).low_cut is None
    # a pool owns its history and leaves the LowCut's slots alone; a stream takes a slot of its own
    pool = melspec.LogMelPool(ext, 3, 400, low_cut=cut)
    assert pool.hist.shape == (3, 254) and pool.hist.dtype == torch.float32 and cut._free == [0]
    stream = melspec.LogMelStream(ext, low_cut=cut)
    assert stream._cut_slot == 0 and cut._free == []
    with pytest.raises(RuntimeError, match="full"):
        melspec.LogMelStream(ext, low_cut=cut)


class _FakePoolCutOp:
    """stands in for ops.logmel_pool_lowcut_impl: records what a push hands the call"""

    def __init__(self):
        self.calls = []

    def __call__(self, win, hist, staged, table, bank, taps, slots, t0s, n_helds, n_drops, n_news, lens, f0s, f1s, n_fft, hop, floor,
                 linear):
        self.calls.append(dict(hist=hist, taps=taps, slots=list(slots), t0s=list(t0s), n_helds=list(n_helds), n_news=list(n_news),
                               staged=None if staged is None else staged.clone()))
        return torch.zeros(len(bank) * sum(f1 - f0 for f0, f1 in zip(f0s, f1s)))


def test_pool_with_a_low_cut_goes_through_the_fused_call():
    ext = melspec.LogMelExtractor(8000, 32, 8, 4, device="cpu")
    cut = melspec.LowCut(8000, device="cpu")
    pool = melspec.LogMelPool(ext, 2, 64, low_cut=cut)
    pool._op = None                                     # the plain call must not be reached
    pool._cut_op = fake = _FakePoolCutOp()
    a, b = pool.open(), pool.open()
    new = pool.push_many({a: torch.arange(40.0), b: torch.arange(10.0)})
    assert new[a].shape == (1, 4, 4) and new[b].shape == (1, 4, 0)
    call = fake.calls[0]
    assert call["hist"] is pool.hist and call["taps"] is cut._taps
    assert call["slots"] == [0, 1] and call["t0s"] == [0, 0] and call["n_helds"] == [0, 0] and call["n_news"] == [40, 10]
    assert torch.equal(call["staged"], torch.cat([torch.arange(40.0), torch.arange(10.0)]))        # RAW samples
    # a reopened slot presents itself as fresh (t0 == 0, n_held == 0): the call starts it from zero history
    pool.close(a)
    c = pool.open()
    assert c.slot == a.slot
    pool.push_many({c: torch.arange(5.0), b: torch.arange(10.0, 13.0)})
    call = fake.calls[1]
    assert call["slots"] == [0, 1] and call["t0s"] == [0, 0] and call["n_helds"] == [0, 10] and call["n_news"] == [5, 3]


# ------------------------------------------------------------------------------------------------------ the driver's flag
def test_driver_flag_parsing_and_default():
    p = FD.build_parser()
    args = p.parse_args([])
    assert args.highpass_on == "host" and not FD.on_device(args)
    args = p.parse_args(["--highpass_on", "device"])
    assert args.highpass_on == "device" and FD.on_device(args)
    assert not FD.on_device(p.parse_args(["--highpass_on", "device", "--highpass_cutoff", "0"]))      # 0 still means no filter
    with pytest.raises(SystemExit):
        p.parse_args(["--highpass_on", "gpu"])
    helptext = p.format_help()
    assert "--highpass_on" in helptext and "one" in helptext and "step" in helptext
    # WORLD features are analysed on the host: the device filter does not serve them
    args = p.parse_args(["--highpass_on", "device", "--feature_type", "world", "--hdf5dir", "unused"])
    assert FD.extract_files([], args) == 2


def test_host_setting_loads_the_waveform_as_before(tmp_path):
    from scipy.io import wavfile
    fs = 8000
    pcm = np.round(8000.0 * np.sin(np.arange(900) / 7.0) + 3000.0).astype(np.int16)
    wavfile.write(str(tmp_path / "a.wav"), fs, pcm)
    p = FD.build_parser()
    x = pcm.astype(np.float64) / 32768.0
    host = FD.load_waveform(str(tmp_path / "a.wav"), p.parse_args(["--fs", str(fs)]))
    assert np.array_equal(host, dsp.low_cut_filter(x, fs, cutoff=70))
    raw = FD.load_waveform(str(tmp_path / "a.wav"), p.parse_args(["--fs", str(fs), "--highpass_on", "device"]))
    assert np.array_equal(raw, x)                       # the device filters the batch: the loader hands it the raw samples


# ------------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("n_taps", [1, 2, 255, 256])
def test_reference_b_is_the_definition_on_exact_signals(n_taps):
    h = LR.taps(n_taps)
    for kind, at in (("impulse", 0), ("impulse", 3), ("ones", 0), ("ternary", 0), ("pow2", 0)):
        x = LR.exact_signal(kind, 300, seed=n_taps, at=at)
        y = LR.exact_chain(h, x)
        assert y.dtype == np.float32 and np.array_equal(y, LR.emulated_chain(h, x)), (n_taps, kind)
        if kind == "impulse":
            want = np.zeros(300, dtype=np.float32)
            want[at:at + n_taps] = h.astype(np.float32)[:300 - at]
            assert np.array_equal(y, want)
    with pytest.raises(AssertionError):
        LR.exact_chain(h, np.array([0.3], dtype=np.float32))


@pytest.mark.parametrize("kind", ["noise", "hum", "half-silence"])
def test_the_definition_stays_inside_the_derived_bound(kind):
    h = dsp.low_cut_taps(22050, 70.0)
    x = LR.general_signal(kind, 600, 22050, seed=1)
    y = LR.emulated_chain(h, x).astype(np.float64)
    err, lim = np.abs(y - LR.value64(h, x)), LR.bound(h, x)
    assert np.all(err <= lim), float((err / lim).max())
    assert np.all(lim[np.abs(x) > 0][:1] > 0) and float(lim.max()) < 1e-6         # a bound of rounding size, not a tolerance
