"""CPU: the rational resampler (swn_resample_chunk, melspec.Resampler, LogMelStream / LogMelPool(resample=), feature_extract
--resample) - its symbols are exported, bound and registered, the filter is scipy's bit for bit, the table has the stated layout,
the references of resample_ref.py agree with scipy.signal.resample_poly and with the definition evaluated by libm's fma, the
streaming rule equals a brute-force count, every refusal of the C call is decided before a device is touched (fake pointers:
nothing is launched), and the Python classes and the stage-1 driver refuse what they must."""
import ctypes

import numpy as np
import pytest
import torch

import resample_ref as RR
from shallow_wavenet_amd import _lib, melspec, ops
from shallow_wavenet_amd import feature_extract_driver as FD

BAD = -2
FS_PAIRS = [(2, 1), (1, 2), (2, 3), (48000, 44100), (48000, 22050), (16000, 22050), (44100, 24000), (16000, 44100)]   # (fs_in, fs_out)


def _detail():
    return _lib.lib().swn_last_error_detail().decode()


def test_symbols_are_exported_bound_and_registered():
    lib = _lib.lib()
    for n in ("swn_resample_table_doubles", "swn_resample_state_floats", "swn_resample_chunk"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.swn_abi_version() == 3
    assert "resample_chunk" in ops.OP_NAMES and "resample_staged" in ops.OP_NAMES
    schema = str(torch.ops.swn.resample_chunk.default._schema)
    assert schema.startswith("swn::resample_chunk(Tensor table, Tensor(a1!) state, Tensor[] inputs, ") and schema.endswith("-> Tensor")
    schema = str(torch.ops.swn.resample_staged.default._schema)
    assert schema.startswith("swn::resample_staged(Tensor table, Tensor(a1!) state, Tensor? staged, ") and schema.endswith("-> Tensor")
    assert ctypes.sizeof(_lib.ResampleEntry) == 56
    assert [f[0] for f in _lib.ResampleEntry._fields_] == ["in_dev", "out_dev", "in0", "out0", "len", "n_in", "n_out", "slot",
                                                           "reserved"]
    assert (_lib.RESAMPLE_MAX_UP, _lib.RESAMPLE_MAX_Q, _lib.RESAMPLE_MAX_TAPS) == (1024, 256, 65535)
    assert (_lib.RESAMPLE_MAX_ENTRIES, _lib.RESAMPLE_TILE, _lib.RESAMPLE_MAX_SPAN) == (64, 1024, 8192)
    assert _lib.RESAMPLE_MAX_Q - 1 <= 256                  # one thread per float of a slot's state


def test_the_ratios_of_run_sh_reduce_and_fit_the_limits():
    assert melspec.resample_ratio(48000, 24000) == (1, 2)              # gcd reduction
    assert melspec.resample_ratio(16000, 48000) == (3, 1)
    assert melspec.resample_ratio(48000, 22050) == (147, 320) and melspec.resample_ratio(44100, 48000) == (160, 147)
    assert sorted(melspec.resample_ratio(a, b) for a, b in FS_PAIRS) == sorted(RR.RATIOS)
    lib = _lib.lib()
    for L, M in RR.RATIOS:
        N = 20 * max(L, M) + 1
        Q = -(-N // L)
        assert lib.swn_resample_table_doubles(L, M, N) == L * Q and lib.swn_resample_state_floats(L, N) == Q - 1, (L, M)
    assert max(20 * max(L, M) + 1 for L, M in RR.RATIOS) == 8821
    for bad in (0, -8000, 22050.0, "16000", True, None):
        with pytest.raises(ValueError, match="positive integer"):
            melspec.resample_ratio(bad, 8000)
        with pytest.raises(ValueError, match="positive integer"):
            melspec.resample_ratio(8000, bad)


def test_size_queries_return_zero_for_refused_arguments():
    lib = _lib.lib()
    assert lib.swn_resample_table_doubles(1, 2, 41) == 41 and lib.swn_resample_state_floats(1, 41) == 40
    assert lib.swn_resample_table_doubles(3, 2, 61) == 63 and lib.swn_resample_state_floats(3, 61) == 20
    assert lib.swn_resample_table_doubles(5, 3, 1) == 5 and lib.swn_resample_state_floats(5, 1) == 0          # Q == 1: no state
    for up, down, n in ((0, 1, 41), (1, 0, 41), (-1, 2, 41), (2, 4, 41), (6, 9, 181), (1, 2, 40), (1, 2, 0), (1, 2, -1),
                        (1, 2, 65537), (1025, 1, 20501), (1, 2, 513), (1, 9, 181)):
        assert lib.swn_resample_table_doubles(up, down, n) == 0, (up, down, n)
    for up, n in ((0, 41), (-1, 41), (1, 40), (1, 0), (1, 65537), (1025, 20501), (1, 513)):
        assert lib.swn_resample_state_floats(up, n) == 0, (up, n)


# ------------------------------------------------------------------------------------------------------ filter and table
@pytest.mark.parametrize("L,M", RR.RATIOS)
def test_taps_are_the_scipy_recipe_bit_for_bit(L, M):
    from scipy.signal import firwin
    h = melspec.resample_taps(L, M)
    N = 2 * 10 * max(L, M) + 1
    assert h.dtype == np.float64 and h.shape == (N,) and N % 2 == 1
    assert np.array_equal(h, L * firwin(N, 1.0 / max(L, M), window=("kaiser", 5.0)))
    assert np.array_equal(h, RR.taps(L, M))
    assert np.array_equal(melspec.resample_taps(L, M, half_len=3, beta=8.0), RR.taps(L, M, 3, 8.0))
    assert melspec.resample_taps(L, M, half_len=3).shape == (6 * max(L, M) + 1,)


@pytest.mark.parametrize("L,M", RR.RATIOS)
def test_table_layout_and_zero_padding(L, M):
    h = melspec.resample_taps(L, M)
    P = melspec.resample_table(h, L)
    N, Q = h.shape[0], -(-h.shape[0] // L)
    assert P.shape == (L, Q) and P.dtype == np.float64 and P.flags["C_CONTIGUOUS"]
    assert np.array_equal(P, RR.table(h, L))
    for r in {0, 1 % L, L // 2, L - 1}:
        for q in {0, 1, Q // 2, Q - 1}:
            assert P[r, q] == (h[r + q * L] if r + q * L < N else 0.0), (r, q)
    pad = np.array([[r + q * L >= N for q in range(Q)] for r in range(L)])
    assert pad.sum() == L * Q - N and np.all(P[pad] == 0.0) and not np.signbit(P[pad]).any()
    res = melspec.Resampler(M * 100, L * 100, device="meta")
    assert (res.L, res.M, res.n_taps, res.Q, res.delay) == (L, M, N, Q, (N - 1) // 2)
    assert np.array_equal(res.table, P) and res._table.shape == (L * Q,) and res._table.dtype == torch.float64
    assert res.state_floats == Q - 1 and res._state.shape == (max(1, Q - 1),)


# ------------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("L,M", RR.RATIOS)
def test_value64_is_scipy_resample_poly(L, M):
    from scipy.signal import resample_poly
    h = RR.taps(L, M)
    g = np.random.Generator(np.random.PCG64(L * 1000 + M))
    for T in (1, 2, 333, 1000):
        x = g.standard_normal(T)
        want = resample_poly(x, L, M)
        got = RR.value64(h, x, L, M)
        assert got.shape == want.shape == (RR.out_count(T, L, M),), T                                # the output count is scipy's
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (T, float(np.abs(got - want).max()))
    assert RR.value64(h, np.zeros(0), L, M).shape == (0,)


@pytest.mark.parametrize("L,M", [(1, 2), (2, 1), (3, 2), (147, 320), (441, 320)])
def test_reference_b_is_the_definition_on_exact_signals(L, M):
    h = RR.taps(L, M)
    Q, D = -(-h.shape[0] // L), (h.shape[0] - 1) // 2
    n = Q + 7
    for kind, at in (("impulse", 0), ("impulse", Q - 1), ("impulse", n - 1), ("ones", 0), ("ternary", 0), ("pow2", 0)):
        x = RR.exact_signal(kind, n, seed=L + M, at=at)
        y = RR.exact_chain(h, x, L, M)
        assert y.dtype == np.float32 and y.shape == (RR.out_count(n, L, M),)
        assert np.array_equal(y, RR.emulated_chain(h, x, L, M)), (kind, at)
        if kind == "impulse":                       # y[n] = fl32(h[n M + D - at L])
            k = np.arange(y.shape[0]) * M + D - at * L
            direct = np.where((k >= 0) & (k < h.shape[0]), h[np.clip(k, 0, h.shape[0] - 1)], 0.0).astype(np.float32)
            assert np.array_equal(y, direct), at
    with pytest.raises(AssertionError):
        RR.exact_chain(h, np.array([0.3], dtype=np.float32), L, M)


@pytest.mark.parametrize("kind", ["noise", "signs", "hum"])
def test_the_definition_stays_inside_the_derived_bound(kind):
    L, M = 147, 320
    h = RR.taps(L, M)
    x = RR.general_signal(kind, 400, 48000, seed=1)
    y = RR.emulated_chain(h, x, L, M).astype(np.float64)
    err, lim = np.abs(y - RR.value64(h, x, L, M)), RR.bound(h, x, L, M)
    assert np.all(err <= lim), float((err / lim).max())
    assert float(lim.max()) < 2e-7 and np.all(lim > 0)                 # a bound of rounding size, not a tolerance


@pytest.mark.parametrize("L,M", RR.RATIOS)
def test_ready_rule_against_brute_force(L, M):
    N = 20 * max(L, M) + 1
    Q = -(-N // L)
    res = melspec.Resampler(M * 50, L * 50, device="meta")
    for T in (0, 1, 5, Q - 1, Q, Q + 1, 100, 1001):
        want = RR.ready_brute(T, L, M, N)
        assert melspec.resample_ready(L, M, N, T) == res.ready(T) == want, T
        assert melspec.resample_ready(L, M, N, T, True) == res.ready(T, True) == res.out_count(T) == RR.out_count(T, L, M)
        assert want <= RR.out_count(T, L, M)
        if want:                                    # the last ready output has all its inputs, the next one does not
            assert ((want - 1) * M + res.delay) // L <= T - 1 < (want * M + res.delay) // L
    assert melspec.resample_ready(1, 2, 41, 1 << 40) == ((1 << 40) - 21) // 2 + 1          # plain Python integers: no 2^31 edge


# ------------------------------------------------------------------------------------------------------ swn_resample_chunk
def _entry(**kw):
    """up 1, down 2, 41 taps (Q 41, D 20): 100 inputs make outputs 0 .. 39 computable"""
    e = dict(in_dev=1 << 20, out_dev=1 << 21, in0=0, out0=0, len=-1, n_in=100, n_out=40, slot=0, reserved=0)
    e.update(kw)
    return e


def _chunk(up=1, down=2, n_taps=41, table=1 << 12, state=1 << 14, capacity=2, entries=None, n_entries=None, tab=True):
    """the C entry point with fake (never dereferenced) device addresses: every case here must fail before a device call"""
    entries = [_entry()] if entries is None else entries
    t = (_lib.ResampleEntry * max(1, len(entries)))(*[_lib.ResampleEntry(**e) for e in entries]) if tab else None
    n = len(entries) if n_entries is None else n_entries
    vp = ctypes.c_void_p
    return _lib.lib().swn_resample_chunk(up, down, n_taps, vp(table), vp(state), capacity, t, n, vp(None))


@pytest.mark.parametrize("kw,text", [
    (dict(up=0), "up < 1"), (dict(up=-2), "up < 1"), (dict(down=0), "down < 1"), (dict(down=-1), "down < 1"),
    (dict(up=2, down=4), "coprime"), (dict(up=6, down=9, n_taps=181), "coprime"),
    (dict(n_taps=40), "even"), (dict(n_taps=0), "n_taps"), (dict(n_taps=-41), "n_taps"), (dict(n_taps=65537), "n_taps"),
    (dict(up=1025, down=1, n_taps=20501), "SWN_RESAMPLE_MAX_UP"), (dict(n_taps=513), "SWN_RESAMPLE_MAX_Q"),
    (dict(down=9, n_taps=181), "SWN_RESAMPLE_MAX_SPAN"),
    (dict(table=None), "null"), (dict(state=None), "null"), (dict(tab=False), "entries_host"),
    (dict(capacity=0), "capacity"), (dict(capacity=-1), "capacity"), (dict(n_entries=-1), "n_entries"),
    (dict(entries=[_entry(slot=2)]), "slot 2"), (dict(entries=[_entry(slot=-1)]), "slot -1"),
    (dict(entries=[_entry(), _entry(in_dev=1 << 22, out_dev=1 << 23)]), "twice"),
    (dict(entries=[_entry(n_in=-1)]), "negative"), (dict(entries=[_entry(n_out=-1)]), "negative"),
    (dict(entries=[_entry(in0=-1)]), "negative"), (dict(entries=[_entry(out0=-1)]), "negative"),
    (dict(entries=[_entry(len=-2)]), "negative"),
    (dict(entries=[_entry(out0=1 << 62, in0=1 << 62)]), "too large"), (dict(entries=[_entry(in0=(1 << 63) - 50)]), "too large"),
    (dict(entries=[_entry(reserved=1)]), "reserved"),
    (dict(entries=[_entry(in_dev=None)]), "null"), (dict(entries=[_entry(out_dev=None)]), "null"),
    # the ranges of one entry: 100 floats in, 40 out; in place, out inside in, in's first float on out's last
    (dict(entries=[_entry(out_dev=1 << 20)]), "overlap"),
    (dict(entries=[_entry(out_dev=(1 << 20) + 396)]), "overlap"),
    (dict(entries=[_entry(out_dev=(1 << 20) - 156)]), "overlap"),
    # not computable: output 40 reads input 100; a signal of 100 inputs has 50 outputs; len is the end of the chunk that gives it
    (dict(entries=[_entry(n_out=41)]), "not computable"),
    (dict(entries=[_entry(len=100, n_out=51)]), "not computable"),
    (dict(entries=[_entry(in0=100, out0=40, n_in=0, n_out=11, len=100, in_dev=None)]), "not computable"),
    (dict(entries=[_entry(len=99)]), "len 99"), (dict(entries=[_entry(len=101, n_out=0)]), "len 101"),
    # below the state: output 0 reads inputs 10 .. -30, the chunk starts at 50 and the state holds 10 .. 49
    (dict(entries=[_entry(in0=50, n_in=50, n_out=10)]), "below the state"),
    (dict(entries=[_entry(in0=100, out0=39, n_in=2, n_out=2)]), "below the state"),
    (dict(entries=[_entry(slot=1), _entry(n_out=41)]), "entry 1"),
])
def test_chunk_refusals_come_before_any_launch(kw, text):
    assert _chunk(**kw) == BAD and text in _detail() and "swn_resample_chunk" in _detail(), _detail()


def test_chunk_calls_that_launch_nothing_succeed():
    assert _chunk(entries=[], n_entries=0) == 0
    assert _chunk(entries=[], n_entries=0, tab=False) == 0
    # nothing in, nothing out: the slot is untouched, and the entry carries no pointers - at the start, mid-way and at an end
    # that has no outputs left
    none = dict(n_in=0, n_out=0, in_dev=None, out_dev=None)
    assert _chunk(entries=[_entry(**none)]) == 0
    assert _chunk(entries=[_entry(in0=100, out0=40, **none)]) == 0
    assert _chunk(entries=[_entry(in0=0, out0=0, len=0, **none), _entry(slot=1, in0=100, out0=50, len=100, **none)]) == 0


# ------------------------------------------------------------------------------------------------------ the Python classes
def test_resampler_argument_errors():
    with pytest.raises(ValueError, match="nothing to resample"):
        melspec.Resampler(22050, 22050, device="meta")
    for cap in (0, -1, 1.5, None):
        with pytest.raises(ValueError, match="capacity"):
            melspec.Resampler(48000, 22050, capacity=cap, device="meta")
    for fs in (0, -1, 22050.0, None):
        with pytest.raises(ValueError, match="positive integer"):
            melspec.Resampler(fs, 22050, device="meta")
    with pytest.raises(ValueError, match="device resampler takes"):
        melspec.Resampler(9000, 1000, device="meta")                   # 1 / 9: a tile's input span does not fit
    with pytest.raises(ValueError, match="device resampler takes"):
        melspec.Resampler(48000, 22050, half_len=200, device="meta")   # n_taps beyond the limit
    res = melspec.Resampler(48000, 22050, capacity=3, device="meta")
    assert (res.fs_in, res.fs_out, res.L, res.M, res.Q) == (48000, 22050, 147, 320, 44) and res._state.shape == (3 * 43,)
    assert [res.open(), res.open()] == [0, 1]
    assert res.open(2) == 2
    with pytest.raises(RuntimeError, match="full"):
        res.open()
    res.close(1)
    assert res.open() == 1 and res._at[1] == [0, 0, False]
    with pytest.raises(RuntimeError, match="not free"):
        res.open(1)
    res.close(0)
    with pytest.raises(RuntimeError, match="not open"):
        res.close(0)
    with pytest.raises(RuntimeError, match="not open"):
        res.run({0: torch.zeros(4)})
    with pytest.raises(RuntimeError, match="not open"):
        res.run({}, finish=[7])
    with pytest.raises(ValueError, match="twice"):
        res.run({}, finish=[1, 1])
    with pytest.raises(ValueError, match="1-D"):
        res.run({1: torch.zeros(2, 4)})
    assert res.run({}) == {}
    res._at[2][2] = True                                # as after run(..., finish=[2])
    with pytest.raises(RuntimeError, match="has ended"):
        res.run({2: torch.zeros(4)})
    # the op refuses host tensors (there is no CPU path) and a table that is not the ratio's
    cpu = melspec.Resampler(16000, 8000, device="cpu")
    args = ([torch.zeros(100)], [0], [0], [0], [40], [-1], 1, 2, 41, 1, True)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.resample_chunk_impl(cpu._table, cpu._state, *args)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.resample_staged_impl(cpu._table, cpu._state, torch.zeros(100), [100], [0], [0], [0], [40], [-1], 1, 2, 41, 1)
    with pytest.raises(RuntimeError, match="at least 100 samples"):
        ops.resample_staged_impl(cpu._table, cpu._state, torch.zeros(99), [100], [0], [0], [0], [40], [-1], 1, 2, 41, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        cpu(torch.zeros(1, 600))
    with pytest.raises(RuntimeError, match="HIP device"):
        cpu.run({cpu.open(): torch.zeros(100)})


def test_streams_and_pools_check_their_resampler():
    ext = melspec.LogMelExtractor(22050, 1024, 110, 80, device="cpu")
    with pytest.raises(ValueError, match="Resampler"):
        melspec.LogMelStream(ext, resample="48 kHz")
    with pytest.raises(ValueError, match="Resampler"):
        melspec.LogMelPool(ext, 2, 400, resample=48000)
    with pytest.raises(ValueError, match="delivers fs 16000"):
        melspec.LogMelStream(ext, resample=melspec.Resampler(48000, 16000, device="cpu"))
    with pytest.raises(ValueError, match="delivers fs 48000"):
        melspec.LogMelPool(ext, 2, 400, resample=melspec.Resampler(22050, 48000, device="cpu"))           # the wrong way round
    with pytest.raises(ValueError, match="extractor on"):
        melspec.LogMelPool(ext, 2, 400, resample=melspec.Resampler(48000, 22050, device="meta"))
    res = melspec.Resampler(48000, 22050, capacity=1, device="cpu")
    with pytest.raises(ValueError, match="fs"):         # resample.fs_out, low_cut.fs and extractor.fs must be one number
        melspec.LogMelStream(ext, resample=res, low_cut=melspec.LowCut(16000, device="cpu"))
    with pytest.raises(ValueError, match="fs"):
        melspec.LogMelPool(ext, 2, 400, resample=res, low_cut=melspec.LowCut(48000, device="cpu"))
    assert res._free == [0]                             # a refused stream claimed nothing
    # the default takes today's path and owns no state
    pool = melspec.LogMelPool(ext, 2, 400)
    assert pool.resample is None and pool.res_state is None and pool._op is ops.logmel_pool_impl
    stream = melspec.LogMelStream(ext)
    assert stream.resample is None and stream._res_slot is None
    # a pool owns its state and leaves the Resampler's slots alone; a stream takes a slot of its own and gives it back if the
    # low cut has none left
    cut = melspec.LowCut(22050, capacity=1, device="cpu")
    pool = melspec.LogMelPool(ext, 3, 400, low_cut=cut, resample=res)
    assert pool.res_state.shape == (3, 43) and pool.res_state.dtype == torch.float32 and res._free == [0] and cut._free == [0]
    stream = melspec.LogMelStream(ext, resample=res, low_cut=cut)
    assert stream._res_slot == 0 and stream._cut_slot == 0 and res._free == [] and cut._free == []
    with pytest.raises(RuntimeError, match="full"):
        melspec.LogMelStream(ext, resample=res)
    res2 = melspec.Resampler(48000, 22050, capacity=1, device="cpu")
    with pytest.raises(RuntimeError, match="full"):
        melspec.LogMelStream(ext, resample=res2, low_cut=cut)
    assert res2._free == [0]


class _FakeOps:
    """stand in for ops.resample_staged_impl and ops.logmel_pool_impl: record what a push hands the two calls"""

    def __init__(self):
        self.res, self.mel = [], []

    def resample(self, table, state, staged, n_ins, slots, in0s, out0s, n_outs, lens, up, down, n_taps, capacity):
        self.res.append(dict(table=table, state=state, staged=None if staged is None else staged.clone(), n_ins=list(n_ins),
                             slots=list(slots), in0s=list(in0s), out0s=list(out0s), n_outs=list(n_outs), lens=list(lens),
                             ratio=(up, down, n_taps), capacity=capacity))
        return torch.arange(float(sum(n_outs))) + 1000.0 * len(self.res)

    def logmel(self, win, staged, table, bank, slots, t0s, n_helds, n_drops, n_news, lens, f0s, f1s, n_fft, hop, floor, linear):
        self.mel.append(dict(staged=staged, slots=list(slots), n_news=list(n_news), lens=list(lens)))
        return torch.zeros(len(bank) * sum(f1 - f0 for f0, f1 in zip(f0s, f1s)))


def test_pool_with_a_resampler_stages_its_outputs_for_the_pool_call():
    ext = melspec.LogMelExtractor(8000, 32, 8, 4, device="cpu")
    res = melspec.Resampler(16000, 8000, device="cpu")                 # 1 / 2, 41 taps: T inputs make (T - 21) // 2 + 1 outputs
    pool = melspec.LogMelPool(ext, 3, 64, resample=res)
    fake = _FakeOps()
    pool._res_op, pool._op = fake.resample, fake.logmel
    a, b, c = pool.open(), pool.open(), pool.open()
    new = pool.push_many({a: torch.arange(100.0), b: torch.arange(10.0), c: torch.zeros(0)})
    call = fake.res[0]
    assert call["table"] is res._table and call["state"] is pool.res_state and call["capacity"] == 3
    assert call["ratio"] == (1, 2, 41) and call["slots"] == [0, 1, 2]
    assert call["in0s"] == [0, 0, 0] and call["out0s"] == [0, 0, 0] and call["n_outs"] == [40, 0, 0] and call["lens"] == [-1] * 3
    assert call["n_ins"] == [100, 10, 0]              # the chunks at fs_in, staged back to back in one buffer
    assert torch.equal(call["staged"], torch.cat([torch.arange(100.0), torch.arange(10.0)]))
    mel = fake.mel[0]
    assert torch.equal(mel["staged"], torch.arange(40.0) + 1000.0)     # the resampler's output is the pool call's staging buffer
    assert mel["n_news"] == [40, 0, 0] and mel["lens"] == [-1] * 3
    assert new[a].shape == (1, 4, 4) and new[b].shape == (1, 4, 0)
    assert (a.n_in, a.n_received, b.n_in, b.n_received) == (100, 40, 10, 0)
    # max_chunk counts samples at the extractor's fs: 140 more inputs would yield 70 - refused before any call, nothing moves
    with pytest.raises(ValueError, match="yields 70 at 8000 Hz"):
        pool.push_many({b: torch.arange(5.0), a: torch.zeros(140)})
    assert len(fake.res) == 1 and (a.n_in, a.n_received, b.n_in) == (100, 40, 10)
    # b goes on (10 + 33 inputs: 12 outputs), a ends without a chunk: the flush yields outputs 40 .. 49 of its 50
    pool.push_many({b: torch.arange(33.0)}, finish=[a])
    call = fake.res[1]
    assert call["slots"] == [1, 0] and call["in0s"] == [10, 100] and call["out0s"] == [0, 40]
    assert call["n_outs"] == [12, 10] and call["lens"] == [-1, 100] and call["n_ins"] == [33, 0]
    assert fake.mel[1]["n_news"] == [12, 10] and fake.mel[1]["lens"] == [-1, 50]
    assert a.finished and (a.n_in, a.n_received, b.n_in, b.n_received) == (100, 50, 43, 12)
    # a tick in which nobody receives or yields anything makes no resampler call
    pool.push_many({c: torch.zeros(0)})
    assert len(fake.res) == 2 and fake.mel[2]["staged"] is None
    # a reopened slot presents itself as fresh (in0 == 0): the call starts it from zero history
    pool.close(a)
    d = pool.open()
    assert d.slot == a.slot and d.n_in == 0
    pool.push_many({d: torch.arange(30.0)})
    assert fake.res[2]["slots"] == [0] and fake.res[2]["in0s"] == [0] and fake.res[2]["n_outs"] == [5]


# ------------------------------------------------------------------------------------------------------ the driver's flag
def test_driver_flag_parsing_and_default(tmp_path):
    from scipy.io import wavfile
    p = FD.build_parser()
    assert p.parse_args([]).resample is False
    assert p.parse_args(["--resample", "true"]).resample is True and p.parse_args(["--resample", "false"]).resample is False
    with pytest.raises(SystemExit):
        p.parse_args(["--resample", "maybe"])
    assert "--resample" in p.format_help()
    # without the flag a file of another rate keeps raising; at --fs the flag changes nothing and touches no device
    wavfile.write(str(tmp_path / "a.wav"), 16000, (np.sin(np.arange(900) * 0.1) * 8000).astype(np.int16))
    with pytest.raises(ValueError, match="sampling frequency 16000 does not match --fs 8000"):
        FD.load_waveform(str(tmp_path / "a.wav"), p.parse_args(["--fs", "8000", "--highpass_cutoff", "0"]))
    plain = FD.load_waveform(str(tmp_path / "a.wav"), p.parse_args(["--fs", "16000"]))
    same = FD.load_waveform(str(tmp_path / "a.wav"), p.parse_args(["--fs", "16000", "--resample", "true"]), device="cpu")
    assert np.array_equal(plain, same)
    with pytest.raises(RuntimeError, match="HIP device"):      # there is no host resampler behind the flag
        FD.load_waveform(str(tmp_path / "a.wav"), p.parse_args(["--fs", "8000", "--resample", "true"]), device="cpu")
