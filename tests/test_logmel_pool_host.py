"""CPU: the log-mel pool's entry points of the C ABI and every refusal that is decided before a device is touched (fake
pointers: nothing is launched), and the bookkeeping of melspec.LogMelPool with a fake operator that keeps the windows on the
host: the planner against a LogMelStream over seeded random chunkings, the window bound, the all-or-nothing rule and the
split of a tick into calls."""
import ctypes
import random

import pytest
import torch

from shallow_wavenet_amd import _lib, melspec, ops

NEW_SYMBOLS = ("swn_logmel_pool", "swn_logmel_pool_window_floats", "swn_logmel_pool_work_bytes")
PAIRS = [(32, 8), (96, 37), (512, 80), (1024, 110), (64, 1), (2048, 2048), (32, 32), (32, 1)]      # (n_fft, hop)
WINDOW = 1024 + 4096


def test_symbols_are_exported_bound_and_registered():
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.swn_abi_version() == 3
    assert "logmel_pool" in ops.OP_NAMES
    schema = str(torch.ops.swn.logmel_pool.default._schema)
    assert schema.startswith("swn::logmel_pool(Tensor(a0!) win, ") and schema.endswith("-> Tensor")
    assert ctypes.sizeof(_lib.LogMelPoolEntry) == 48
    assert _lib.LOGMEL_POOL_MAX_ENTRIES == 64
    assert [f[0] for f in _lib.LogMelPoolEntry._fields_] == ["slot", "t0", "n_held", "n_drop", "new_off", "n_new", "len", "f0", "f1",
                                                             "out_off", "out_stride", "reserved"]


def _entry(slot=0, t0=0, n_held=0, n_drop=0, new_off=0, n_new=3001, length=3001, f0=0, f1=28, out_off=0, out_stride=None,
           reserved=0):
    return _lib.LogMelPoolEntry(slot=slot, t0=t0, n_held=n_held, n_drop=n_drop, new_off=new_off, n_new=n_new, len=length, f0=f0,
                                f1=f1, out_off=out_off, out_stride=f1 - f0 if out_stride is None else out_stride,
                                reserved=reserved)


def _table(entries):
    return (_lib.LogMelPoolEntry * len(entries))(*entries) if entries else None


def test_size_queries():
    lib = _lib.lib()
    assert lib.swn_logmel_pool_window_floats(1024, 4096) == WINDOW
    assert lib.swn_logmel_pool_window_floats(32, 1) == 33
    for n, c in ((1000, 10), (16, 10), (2080, 10), (1024, 0), (1024, -1), (1024, 1 << 24)):
        assert lib.swn_logmel_pool_window_floats(n, c) == 0
    en = _table([_entry(), _entry(slot=3, n_new=600, length=600, f1=5, new_off=3001, out_off=4 * 28)])
    # 2 + 1 tiles of 16 frames x (513 bins padded to 516) floats
    assert lib.swn_logmel_pool_work_bytes(1024, 110, 4, WINDOW, en, 2) == 3 * 16 * 516 * 4
    assert lib.swn_logmel_pool_work_bytes(1024, 110, 4, WINDOW, en, 0) == 0
    assert lib.swn_logmel_pool_work_bytes(1024, 110, 4, WINDOW, None, 2) == 0
    assert lib.swn_logmel_pool_work_bytes(1024, 0, 4, WINDOW, en, 2) == 0
    assert lib.swn_logmel_pool_work_bytes(1000, 110, 4, WINDOW, en, 2) == 0
    assert lib.swn_logmel_pool_work_bytes(1024, 110, 0, WINDOW, en, 2) == 0
    assert lib.swn_logmel_pool_work_bytes(1024, 110, 4, 3000, en, 2) == 0                   # 3 001 samples do not fit
    assert lib.swn_logmel_pool_work_bytes(1024, 110, 4, 0, en, 2) == 0
    # an entry without frames needs no scratch, and is no refusal of the call
    en = _table([_entry(n_new=100, length=-1, f1=0)])
    assert lib.swn_logmel_pool_work_bytes(1024, 110, 4, WINDOW, en, 1) == 0
    assert _call(entries=[_entry(n_new=100, length=-1, f1=0)], out=0, tables=0, work=0, win=0) == -2      # ... the window is needed


def _call(n_fft=1024, hop=110, n_mels=4, floor=1e-5, linear=0, tables=1, bank=True, win=1, window=WINDOW, new=1, out=1,
          entries=True, n_entries=None, work=1, **kw):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    codes = [(10 * m + 1) | (12 << 16) for m in range(max(n_mels, 1))]
    bank_c = (ctypes.c_int32 * len(codes))(*codes) if bank else None
    if entries is True:
        entries = [_entry(**kw)]
    return lib.swn_logmel_pool(n_fft, hop, n_mels, floor, linear, p(tables), bank_c, p(win), window, p(new), p(out),
                               _table(entries), len(entries or []) if n_entries is None else n_entries, p(work), None)


def test_call_checks_its_arguments_before_any_launch():
    """fake non-null addresses: every one of these is refused before the library touches them"""
    detail = lambda: _lib.lib().swn_last_error_detail().decode()
    BAD = -2
    # the size rules of swn_logmel
    for n in (0, 16, 48, 1000, 2080):
        assert _call(n_fft=n) == BAD and "n_fft" in detail()
    assert _call(hop=0) == BAD and "hop" in detail()
    assert _call(hop=1025) == BAD and "hop" in detail()
    assert _call(n_mels=0) == BAD and "n_mels" in detail()
    assert _call(n_mels=129) == BAD and "n_mels" in detail()
    for fl in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(floor=fl) == BAD and "floor" in detail()
    assert _call(linear=2) == BAD and "linear" in detail()
    assert _call(length=512, n_new=512, f1=1) == BAD and "length" in detail()               # len <= n_fft / 2
    assert _call(length=3000) == BAD and "window" in detail()                               # the window leaves the signal
    # pointers
    for name in ("tables", "work", "win", "new", "out"):
        assert _call(**{name: 0}) == BAD and "null" in detail(), name
    assert _call(bank=False) == BAD and "bank" in detail()
    assert _call(entries=None, n_entries=1) == BAD and "entries_host" in detail()
    # the table
    assert _call(n_entries=0) == BAD and "n_entries" in detail()
    assert _call(entries=[_entry(slot=i, f1=0, n_new=0, length=-1) for i in range(65)]) == BAD and "n_entries" in detail()
    assert _call(reserved=1) == BAD and "reserved" in detail()
    assert _call(window=0) == BAD and "window_floats" in detail()
    two = lambda **kw: [_entry(), _entry(**{**dict(slot=1, new_off=3001, out_off=4 * 28), **kw})]
    assert _lib.lib().swn_logmel_pool_work_bytes(1024, 110, 4, WINDOW, _table(two()), 2) == 4 * 16 * 516 * 4
    assert _call(entries=two(slot=0)) == BAD and "slot 0" in detail()                       # a slot twice in one call
    # negative counts
    for name in ("slot", "t0", "n_held", "n_drop", "new_off", "n_new", "out_off", "out_stride"):
        assert _call(**{name: -1}) == BAD, name
    assert _call(f0=-1) == BAD and _call(f0=3, f1=2) == BAD and _call(length=-2) == BAD
    # the window's arithmetic
    assert _call(n_held=10, n_drop=11, t0=0, n_new=3001 - 10) == BAD and "n_drop" in detail()
    assert _call(n_new=WINDOW + 1, length=WINDOW + 1) == BAD and "fit the window" in detail()
    assert _call(n_held=2120, n_new=3001, length=5121) == BAD and "fit the window" in detail()            # 5 121 > 5 120
    assert _call(n_held=WINDOW + 1, n_drop=WINDOW + 1, t0=0, n_new=0, length=-1, f1=0) == BAD and "fit the window" in detail()
    # frame ranges against the UPDATED window: 100 held, 50 of them dropped - the window starts at sample 50, frame 0 reads 0
    assert _call(n_held=100, n_drop=50, n_new=2901) == BAD and "window" in detail()
    ok = _table([_entry(n_held=100, n_drop=0, n_new=2901)])                                 # (without the drop it passes)
    assert _lib.lib().swn_logmel_pool_work_bytes(1024, 110, 4, WINDOW, ok, 1) == 2 * 16 * 516 * 4
    # frame 5 spans 38 .. 1061: held from 38 on it is there, from 39 on it is not; one sample short at the end it is not
    ok = _table([_entry(t0=30, n_held=100, n_drop=8, n_new=932, length=-1, f0=5, f1=6)])
    assert _lib.lib().swn_logmel_pool_work_bytes(1024, 110, 4, WINDOW, ok, 1) == 16 * 516 * 4
    assert _call(t0=30, n_held=100, n_drop=9, n_new=932, length=-1, f0=5, f1=6) == BAD and "window" in detail()
    assert _call(t0=30, n_held=100, n_drop=8, n_new=931, length=-1, f0=5, f1=6) == BAD and "unknown" in detail()
    # the reflected end needs the total length
    assert _call(length=-1) == BAD and "unknown" in detail()
    assert _call(t0=2458, n_held=0, n_new=543, length=-1, f0=27, f1=28) == BAD and "unknown" in detail()
    ok = _table([_entry(t0=2000, n_held=500, n_drop=458, n_new=501, f0=27, f1=28)])
    assert _lib.lib().swn_logmel_pool_work_bytes(1024, 110, 4, WINDOW, ok, 1) == 16 * 516 * 4
    assert _call(t0=2000, n_held=500, n_drop=459, n_new=501, f0=27, f1=28) == BAD and "window" in detail()
    # f1 beyond 1 + len / hop
    assert _call(f1=29) == BAD and "28 frames" in detail()
    # output ranges: a stride below the frame count folds an entry's rows onto each other; two entries on the same floats
    assert _call(out_stride=27) == BAD and "overlap" in detail()
    assert _call(entries=two(out_off=4 * 28 - 1)) == BAD and "overlap" in detail()
    assert _call(entries=two(out_off=0)) == BAD and "overlap" in detail()
    # interleaved rows of one (n_mels, 56) matrix do not overlap
    inter = [_entry(out_stride=56), _entry(slot=1, new_off=3001, out_off=28, out_stride=56)]
    assert _lib.lib().swn_logmel_pool_work_bytes(1024, 110, 4, WINDOW, _table(inter), 2) == 4 * 16 * 516 * 4
    # a second entry is checked like the first
    assert _call(entries=two(f1=29)) == BAD and "entry 1" in detail()


# ------------------------------------------------------------------------------------------------------ the host class
class _FakeStreamOp:
    """stands in for ops.logmel_impl under a LogMelStream: returns frame indices"""

    def __call__(self, wav, table, bank, t0s, n_avails, lens, f0s, f1s, n_fft, hop, floor, linear):
        (f0,), (f1,) = f0s, f1s
        return torch.arange(f0, f1, dtype=torch.float32)[None, :, None].expand(1, f1 - f0, len(bank)).clone()


class _FakePoolOp:
    """stands in for ops.logmel_pool_impl: checks every call against the rules of the C call (the size query runs them all),
    applies the window update on the host, and returns 1000 m + f for frame f, filter m in the call's layout"""

    def __init__(self):
        self.calls = []

    def __call__(self, win, staged, table, bank, slots, t0s, n_helds, n_drops, n_news, lens, f0s, f1s, n_fft, hop, floor, linear):
        E, n_mels = len(slots), len(bank)
        assert staged is None or (staged.dim() == 1 and staged.numel() == sum(n_news))
        en, new_off, out_off = [], 0, 0
        for e in range(E):
            k = f1s[e] - f0s[e]
            en.append(_lib.LogMelPoolEntry(slot=slots[e], t0=t0s[e], n_held=n_helds[e], n_drop=n_drops[e], new_off=new_off,
                                           n_new=n_news[e], len=lens[e], f0=f0s[e], f1=f1s[e], out_off=out_off, out_stride=k))
            new_off += n_news[e]
            out_off += k * n_mels
        lib = _lib.lib()
        if any(e.f1 > e.f0 for e in en):                        # (a call without frames needs no scratch: 0 is no refusal)
            assert lib.swn_logmel_pool_work_bytes(n_fft, hop, n_mels, win.shape[1], _table(en), E) > 0, \
                lib.swn_last_error_detail().decode()
        out = torch.empty(out_off)
        for e in en:
            w = win[e.slot]
            kept = w[e.n_drop:e.n_held].clone()
            w[:kept.numel()] = kept
            if e.n_new:
                w[kept.numel():kept.numel() + e.n_new] = staged[e.new_off:e.new_off + e.n_new]
            held = kept.numel() + e.n_new
            w[held:] = float("nan")                             # what the window does not hold is nobody's
            # sample value = its absolute index: the window holds [t0 + n_drop, ...) from its first float
            assert torch.equal(w[:held], torch.arange(e.t0 + e.n_drop, e.t0 + e.n_drop + held, dtype=torch.float32))
            k = e.f1 - e.f0
            out[e.out_off:e.out_off + k * n_mels] = (1000.0 * torch.arange(n_mels)[:, None] + torch.arange(e.f0, e.f1)[None, :]
                                                     ).reshape(-1)
        self.calls.append([dict(slot=e.slot, t0=e.t0, n_held=e.n_held, n_drop=e.n_drop, n_new=e.n_new, len=e.len, f0=e.f0,
                                f1=e.f1) for e in en])
        return out


def _pool(n_fft, hop, capacity, max_chunk, n_mels=4):
    ext = melspec.LogMelExtractor(22050, n_fft, hop, n_mels, device="cpu")
    ext._op = _FakeStreamOp()
    pool = melspec.LogMelPool(ext, capacity=capacity, max_chunk=max_chunk)
    pool._op = _FakePoolOp()
    return ext, pool


@pytest.mark.parametrize("n_fft,hop", PAIRS)
def test_planner_reproduces_the_stream_counters(n_fft, hop):
    """three sessions over seeded random chunkings (sizes 0, 1, hop - 1, hop, hop + 1, n_fft, 3 n_fft), ticks in which a
    session gets nothing, one finished with a last chunk and one without: after every tick each session stands where a
    LogMelStream fed the same chunks stands, returns the frames it returns, and holds at most n_fft samples"""
    sizes = [0, 1, hop - 1, hop, hop + 1, n_fft, 3 * n_fft]
    ext, pool = _pool(n_fft, hop, 3, 3 * n_fft)
    assert pool.windows.shape == (3, 4 * n_fft)
    for seed in range(4):
        rng = random.Random(1000 * n_fft + 10 * hop + seed)
        sess = [pool.open() for _ in range(3)]
        assert [s.slot for s in sess] == [0, 1, 2]
        streams = [melspec.LogMelStream(ext) for _ in sess]
        got = [[] for _ in sess]
        want = [[] for _ in sess]
        n_ticks = 14
        for tick in range(n_ticks):
            chunks, fin = {}, []
            for i, (s, st) in enumerate(zip(sess, streams)):
                if s.finished or rng.random() < 0.25:
                    continue                                    # nothing for this session in this tick
                n = rng.choice(sizes)
                last = tick >= n_ticks - 2 and s.n_received + (0 if i == 1 else n) > n_fft // 2
                x = torch.arange(s.n_received, s.n_received + n, dtype=torch.float32)
                if last and i == 1:
                    fin.append(s)                               # finished without a last chunk
                    want[i].append(st.finish())
                else:
                    chunks[s] = x
                    want[i].append(st.push(x))
                    if last:
                        fin.append(s)
                        want[i].append(st.finish())
            if not chunks and not fin:
                continue
            new = pool.push_many(chunks, finish=fin)
            assert set(new) == set(chunks) | set(fin)
            for i, (s, st) in enumerate(zip(sess, streams)):
                if s in new:
                    assert new[s].shape[:2] == (1, 4) and new[s].is_contiguous()
                    got[i].append(new[s])
                assert (s.n_received, s.n_frames, s.finished) == (st.n_received, st.n_frames, st.finished)
                # the stream has dropped what the pool's window drops at the start of its next call
                keep = melspec.keep_from(n_fft, hop, s.t0, s.n_frames)
                assert s.t0 + s.n_held == s.n_received
                if not s.finished:
                    assert keep == st.t0 and s.n_received - keep == st._buf.numel()
                    assert s.n_received - keep <= n_fft, (n_fft, hop, s.n_received, keep)
                assert s.n_held <= pool.windows.shape[1]
        for i, s in enumerate(sess):
            a = torch.cat(got[i], 2) if got[i] else torch.zeros(1, 4, 0)
            b = torch.cat(want[i]) if want[i] else torch.zeros(0, 4)
            assert a.shape[2] == b.shape[0] == s.n_frames
            # frame f, filter m came back as 1000 m + f, in order and once each
            assert torch.equal(a[0], 1000.0 * torch.arange(4)[:, None] + torch.arange(s.n_frames)[None, :])
            if s.finished:
                assert s.n_frames == 1 + s.n_received // hop
            pool.close(s)
    for call in pool._op.calls:
        for e in call:
            assert e["n_held"] - e["n_drop"] <= n_fft               # what a session holds between calls


def test_plan_mel_push_is_pure_arithmetic():
    calls = melspec.plan_mel_push([("a", 0, 0, 0, 0, 600, False), ("b", 38, 1000, 5, 1038, 0, True), ("c", 0, 10, 0, 10, 0, False)],
                                  1024, 110, 80, limit=2)
    assert [len(c) for c in calls] == [2, 1]
    a, b = calls[0]
    assert a == melspec.MelPlanEntry("a", 0, 0, 0, 0, 600, -1, 0, 1, 0, 1)                  # 600 > 512: frame 0
    # b: 5 frames returned -> keep from 5 * 110 - 512 - 1 = 37 (the window starts later: nothing to drop); the end: 10 frames
    assert b == melspec.MelPlanEntry("b", 38, 1000, 0, 600, 0, 1038, 5, 10, 80, 5)
    assert calls[1][0] == melspec.MelPlanEntry("c", 0, 10, 0, 0, 0, -1, 0, 0, 0, 0)         # offsets count per call
    with pytest.raises(ValueError, match="longer than"):
        melspec.plan_mel_push([("a", 0, 0, 0, 0, 512, True)], 1024, 110, 80)
    with pytest.raises(ValueError, match="does not end"):
        melspec.plan_mel_push([("a", 1, 5, 0, 7, 1, False)], 1024, 110, 80)
    with pytest.raises(ValueError, match="limit"):
        melspec.plan_mel_push([], 1024, 110, 80, limit=0)
    assert melspec.frames_ready(1024, 110, 512) == 0 and melspec.frames_ready(1024, 110, 513) == 1
    assert melspec.frames_ready(1024, 110, 621) == 1 and melspec.frames_ready(1024, 110, 622) == 2
    assert melspec.frames_ready(1024, 110, 622, True) == 6
    assert melspec.keep_from(1024, 110, 0, 4) == 0 and melspec.keep_from(1024, 110, 0, 6) == 147


def _state(sessions):
    return [(s.slot, s.t0, s.n_held, s.n_received, s.n_frames, s.finished, s.closed) for s in sessions]


def test_a_raising_call_changes_nothing():
    ext, pool = _pool(32, 8, 4, 64)
    _, other = _pool(32, 8, 2, 64)
    a, b, c, d = (pool.open() for _ in range(4))
    with pytest.raises(RuntimeError, match="full"):
        pool.open()
    x = lambda s, n: torch.arange(s.n_received, s.n_received + n, dtype=torch.float32)
    pool.push_many({a: x(a, 40), b: x(b, 10), c: x(c, 20), d: x(d, 30)})
    pool.push_many({d: x(d, 3)}, finish=[d])
    pool.close(c)
    stranger = other.open()
    sess = [a, b, c, d, stranger]
    before, windows, n_calls = _state(sess), pool.windows.clone(), len(pool._op.calls)
    good = {a: x(a, 9)}
    bad_calls = [
        (RuntimeError, "closed", lambda: pool.push_many({**good, c: x(c, 1)})),
        (RuntimeError, "finished", lambda: pool.push_many({**good, d: x(d, 1)})),
        (RuntimeError, "finished", lambda: pool.push_many(good, finish=[d])),
        (RuntimeError, "not open in this pool", lambda: pool.push_many({**good, stranger: torch.zeros(4)})),
        (RuntimeError, "not open in this pool", lambda: pool.push_many({**good, "a": torch.zeros(4)})),
        (ValueError, "twice", lambda: pool.push_many(good, finish=[a, a])),
        (ValueError, "at most 64", lambda: pool.push_many({**good, b: torch.zeros(65)})),
        (ValueError, "1-D", lambda: pool.push_many({**good, b: torch.zeros(1, 8)})),
        (ValueError, "longer than", lambda: pool.push_many({**good, b: x(b, 6)}, finish=[b])),      # 16 samples: n_fft / 2
        (ValueError, "longer than", lambda: pool.push_many(good, finish=[b])),
        (ValueError, "must map", lambda: pool.push_many([a])),
        (RuntimeError, "not open in this pool", lambda: pool.close(c)),
        (RuntimeError, "not open in this pool", lambda: pool.close(stranger)),
    ]
    for exc, match, call in bad_calls:
        with pytest.raises(exc, match=match):
            call()
        assert _state(sess) == before and len(pool._op.calls) == n_calls
        assert torch.equal(pool.windows.nan_to_num(-1.0), windows.nan_to_num(-1.0))
    # ... and every session goes on: b ends with one more sample than the refusal had
    new = pool.push_many({**good, b: x(b, 7)}, finish=[b])
    assert b.finished and b.n_received == 17 and b.n_frames == 3 and new[b].shape == (1, 4, 3)
    assert a.n_received == 49 and a.n_frames == 1 + (49 - 16) // 8 and not a.finished
    # other dtypes are converted, host lists are taken, the freed slot goes to the next session
    e = pool.open()
    assert e.slot == c.slot
    new = pool.push_many({e: torch.arange(20, dtype=torch.int16), a: torch.arange(49, 52, dtype=torch.float64)})
    assert new[e].shape == (1, 4, 1) and e.n_received == 20 and a.n_received == 52
    with pytest.raises(ValueError):
        melspec.LogMelPool(ext, capacity=0, max_chunk=8)
    with pytest.raises(ValueError):
        melspec.LogMelPool(ext, capacity=1, max_chunk=0)


def test_a_tick_of_65_sessions_is_two_calls():
    ext, pool = _pool(32, 8, 65, 40)
    sess = [pool.open() for _ in range(65)]
    new = pool.push_many({s: torch.arange(20 + (i % 7), dtype=torch.float32) for i, s in enumerate(sess)})
    assert [len(c) for c in pool._op.calls] == [64, 1]
    assert [e["slot"] for e in pool._op.calls[0]] == list(range(64)) and pool._op.calls[1][0]["slot"] == 64
    assert list(new) == sess                                    # entry order
    for i, s in enumerate(sess):
        assert s.n_received == 20 + (i % 7) and s.n_frames == 1 + (4 + i % 7) // 8 and new[s].shape == (1, 4, s.n_frames)
    # sessions that get nothing cost no entry; finishing ones without a chunk come after the chunks
    pool._op.calls.clear()
    new = pool.push_many({sess[3]: torch.arange(23, 30, dtype=torch.float32)}, finish=[sess[64], sess[3]])
    assert [[e["slot"] for e in c] for c in pool._op.calls] == [[3, 64]]
    assert pool._op.calls[0][0]["len"] == 30 and pool._op.calls[0][1]["len"] == 21
    assert sess[64].finished and sess[64].n_frames == 1 + 21 // 8 and new[sess[64]].shape == (1, 4, 2)       # frames 1 and 2
    assert sess[3].finished and sess[3].n_frames == 1 + 30 // 8
