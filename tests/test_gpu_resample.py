"""GPU: the rational resampler on the device (swn_resample_chunk / torch.ops.swn.resample_chunk / melspec.Resampler),
LogMelStream(resample=), LogMelPool(resample=) and `feature_extract_driver --resample true`.

The yardsticks are resample_ref.py: (b) the exact chain, bit for bit, on signals of zeros and +-2^k; (a) the float64 value with
the derived bound on general signals.  Everything about chunking, batching, slots, streams and pools is exact (torch.equal):
an output sample depends only on its absolute index and the signal.

Shapes: the ratios 1/2, 2/1, 3/2, 147/160, 147/320 and 441/320 with the default design (Q = 41, 21, 21, 22, 44, 21); input
lengths 1, Q - 1, Q, those that give one output less and more than tile - 1, tile, tile + 1 (the kernel's tile is
_lib.RESAMPLE_TILE = 1 024 outputs per block) and about three tiles; every case of one ratio is one device call.  Batches of 65
entries (a launch group takes 64).  The bound's signals are as long as np.convolve on the zero-stuffed signal stays near a
second (3 001 inputs at 1/2, 200 at 441/320).  Streams and pools at fs8000-n32-hop8-m4 behind 16 kHz and 4 kHz audio."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import resample_ref as RR
from shallow_wavenet_amd import _lib, featio, melspec, ops
from shallow_wavenet_amd import feature_extract_driver as FD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = _lib.RESAMPLE_TILE
NAN = float("nan")
RATIOS = [(1, 2), (2, 1), (3, 2), (147, 160), (147, 320), (441, 320)]          # (L, M)
RATIO_IDS = [f"{L}-{M}" for L, M in RATIOS]
GEOM = (8000, 32, 8, 4)


@functools.lru_cache(maxsize=None)
def _res(L, M, capacity=4):
    return melspec.Resampler(M * 100, L * 100, capacity=capacity, device=DEV)


def _one_shot(res, signals):
    """torch.ops.swn.resample_chunk on a list of host signals, every slot's state NaN -> list of host fp32 arrays"""
    E = len(signals)
    state = torch.full((max(1, E * res.state_floats),), NAN, dtype=torch.float32, device=DEV)
    ins = [torch.from_numpy(np.asarray(x, dtype=np.float32)).to(DEV) for x in signals]
    counts = [res.out_count(len(x)) for x in signals]
    out = torch.ops.swn.resample_chunk(res._table, state, ins, list(range(E)), [0] * E, [0] * E, counts, [len(x) for x in signals],
                                       res.L, res.M, res.n_taps, E, False)
    return [out[e, :k].cpu().numpy() for e, k in enumerate(counts)]


def _lengths(L, M, Q):
    lens = {1, Q - 1, Q, -(-(3 * TILE + 5) * M // L)}
    for target in (TILE - 1, TILE, TILE + 1):
        lens |= {target * M // L, -(-target * M // L)}
    return sorted(lens)


# ------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("L,M", RATIOS, ids=RATIO_IDS)
def test_bit_exact_against_the_exact_chain(gpu_ok, L, M):
    """all ones, random signals over {-1, 0, +1} and over powers of two at every length; impulses at sample 0, at Q - 1, at the
    last sample and at the input the first output of the second tile reads (y[n] = fl32(h[n M + D - at L])): the bits of (b)"""
    res = _res(L, M)
    h, Q, D = res.taps, res.Q, res.delay
    lens = _lengths(L, M, Q)
    counts = sorted({RR.out_count(n, L, M) for n in lens})
    # output counts on both sides of a tile's edge (2/1 and 3/2 cannot give every count), and more than three tiles
    assert any(TILE - 3 <= c <= TILE for c in counts) and any(TILE < c <= TILE + 3 for c in counts) and counts[-1] > 3 * TILE
    cases = []
    for n in lens:
        for kind in ("ones", "ternary", "pow2"):
            cases.append((kind, 0, RR.exact_signal(kind, n, seed=n)))
        if n >= Q:
            edge = (TILE * M + D) // L
            for at in sorted({0, Q - 1, n - 1} | ({edge} if edge < n else set())):
                cases.append(("impulse", at, RR.exact_signal("impulse", n, at=at)))
    got = _one_shot(res, [x for _, _, x in cases])
    for (kind, at, x), y in zip(cases, got):
        want = RR.exact_chain(h, x, L, M)
        assert y.dtype == np.float32 and y.shape == want.shape == (RR.out_count(len(x), L, M),)
        assert np.array_equal(y, want), (kind, at, len(x), int((y != want).sum()))
        if kind == "impulse":
            k = np.arange(y.shape[0]) * M + D - at * L
            direct = np.where((k >= 0) & (k < h.shape[0]), h[np.clip(k, 0, h.shape[0] - 1)], 0.0).astype(np.float32)
            assert np.array_equal(y, direct) and np.any(y != 0), (at, len(x))


@pytest.mark.parametrize("L,M", RATIOS, ids=RATIO_IDS)
def test_general_signals_stay_inside_the_derived_bound(gpu_ok, L, M):
    res = _res(L, M)
    T = int(min(3001, max(200, 6e8 / (L * res.n_taps))))
    kinds = ("noise", "hum", "half-silence")
    signals = [RR.general_signal(kind, T, M * 100, seed=i) for i, kind in enumerate(kinds)]
    outs = _one_shot(res, signals)
    for kind, x, y in zip(kinds, signals, outs):
        r = RR.value64(res.taps, x, L, M)
        err, lim = np.abs(y.astype(np.float64) - r), RR.bound(res.taps, x, L, M, r)
        print(f"{kind} {L}/{M}, {T} inputs: max |y - r| / bound = {float((err / lim).max()):.3f}")
        assert err.shape == lim.shape == (RR.out_count(T, L, M),)
        assert np.all(err <= lim), (kind, float((err / lim).max()))
    quiet = ((T // 2 - 1) * L - res.delay) // M        # the last output that reads the silent half only
    assert quiet > 0 and np.all(outs[2][:quiet] == 0) and np.any(outs[2] != 0)          # silence in, exact zeros out


# ------------------------------------------------------------------------------------------------------ chunking
@functools.lru_cache(maxsize=None)
def _signal(n, seed, fs=16000):
    """a general fp32 signal on the host; shared, never written to"""
    return torch.from_numpy(RR.general_signal("noise", n, fs, seed=seed))


def _chunked(res, x, sizes, flush_alone):
    """x through one session in chunks of `sizes` (cycled) -> (the concatenated outputs, the outputs' counts per call)"""
    s = res.open()
    got, at, i = [], 0, 0
    while at < x.numel():
        n = sizes[i % len(sizes)]
        last = at + n >= x.numel()
        c = x[at:at + n]
        got.append(res.run({s: c.to(DEV) if i % 2 else c}, finish=[s] if last and not flush_alone else [])[s])
        assert got[-1].shape == (res.ready(min(at + n, x.numel()), last and not flush_alone) - res.ready(at),)
        at, i = at + n, i + 1
    if flush_alone:
        got.append(res.run({}, finish=[s])[s])          # the flush with no new input
        assert got[-1].numel() == res.out_count(x.numel()) - res.ready(x.numel()) > 0
    res.close(s)
    return torch.cat(got), [int(g.numel()) for g in got]


@pytest.mark.parametrize("L,M", RATIOS, ids=RATIO_IDS)
def test_any_chunking_gives_the_one_shot_bits(gpu_ok, L, M):
    res = _res(L, M)
    n_in = -(-(2 * TILE + 300) * M // L) + 777          # one chunk below yields more than two tiles of outputs
    x = _signal(n_in, 11)
    want = res(x)[0]
    assert want.shape == (res.out_count(n_in),) and want.dtype == torch.float32
    primes = [2, 3, 5, 7, 11, 13, 101, 211, 0, 401]
    for sizes, alone in ((primes, True), (primes[::-1], False), ([7, n_in - 777, 1000], True), ([n_in], True)):
        got, counts = _chunked(res, x, sizes, alone)
        assert torch.equal(got, want), (sizes[:3], alone)
        if sizes[0] in (2, 7):
            assert counts[0] == 0                       # a chunk that yields no output
        if sizes[0] == 7:
            assert counts[1] > 2 * TILE                 # a chunk that spans more than one tile
    # chunks of one sample, on a shorter signal
    short = x[:res.Q + 150]
    got, counts = _chunked(res, short, [1], True)
    assert torch.equal(got, res(short)[0]) and 0 in counts and max(counts[:-1]) == -(-L // M)
    assert res._free == list(range(res.capacity))


def test_a_row_alone_equals_the_row_inside_a_ragged_batch(gpu_ok):
    """65 entries: more than one launch group"""
    res = _res(147, 320)
    lens = [9001, 1, 2500, 0] + [200 + 37 * (i % 9) for i in range(61)]
    signals = [_signal(n, 100 + i) for i, n in enumerate(lens)]
    out = res(signals)
    assert out.shape == (65, res.out_count(9001)) and res.out_count(9001) > 4 * TILE
    for r in (0, 1, 2, 4, 63, 64):
        assert torch.equal(out[r, :res.out_count(lens[r])], res(signals[r])[0]), r
    # the padded form with lengths reads no float past a row's length
    batch = torch.full((65, 9001), NAN)
    for r, s in enumerate(signals):
        batch[r, :lens[r]] = s
    again = res(batch, lens)
    for r in range(65):
        k = res.out_count(lens[r])
        assert torch.equal(again[r, :k], out[r, :k]) and not torch.isnan(again[r, :k]).any(), r


def test_staged_chunks_give_the_bits_of_the_entries_one_by_one(gpu_ok):
    """torch.ops.swn.resample_staged, the form LogMelPool uses: the chunks back to back in one buffer, no tensor per entry"""
    res = _res(147, 320)
    n_ins = [2400, 0, 481, 3000]
    xs = [_signal(n, 300 + i).to(DEV) for i, n in enumerate(n_ins)]
    H = res.state_floats
    outs, states = [], []
    for staged in (False, True):
        state = torch.full((4 * H,), NAN, dtype=torch.float32, device=DEV)
        first = [res.ready(n) for n in n_ins]
        rest = [res.out_count(2 * n) - res.ready(n) for n in n_ins]
        if staged:
            a = torch.ops.swn.resample_staged(res._table, state, torch.cat(xs), n_ins, [3, 2, 1, 0], [0] * 4, [0] * 4, first,
                                              [-1] * 4, res.L, res.M, res.n_taps, 4)
            b = torch.ops.swn.resample_staged(res._table, state, torch.cat(xs), n_ins, [3, 2, 1, 0], n_ins, first, rest,
                                              [2 * n for n in n_ins], res.L, res.M, res.n_taps, 4)
        else:
            a = torch.ops.swn.resample_chunk(res._table, state, xs, [3, 2, 1, 0], [0] * 4, [0] * 4, first, [-1] * 4, res.L, res.M,
                                             res.n_taps, 4, True)
            b = torch.ops.swn.resample_chunk(res._table, state, xs, [3, 2, 1, 0], n_ins, first, rest, [2 * n for n in n_ins],
                                             res.L, res.M, res.n_taps, 4, True)
        assert a.shape == (sum(first),) and b.shape == (sum(rest),)
        outs.append((a, b))
        states.append(state)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(states[0].view(4, H)[[0, 1, 3]], states[1].view(4, H)[[0, 1, 3]]) and torch.isnan(states[1].view(4, H)[2]).all()
    # ... and those are the one-shot bits of every signal played twice
    at_a = at_b = 0
    for x, n, k, m in zip(xs, n_ins, first, rest):
        want = res(torch.cat([x, x]))[0] if n else torch.zeros(0, device=DEV)
        assert torch.equal(torch.cat([outs[1][0][at_a:at_a + k], outs[1][1][at_b:at_b + m]]), want[:k + m]), n
        at_a, at_b = at_a + k, at_b + m


# ------------------------------------------------------------------------------------------------------ slots, C ABI
def _abi_call(res, state, capacity, entries):
    """swn_resample_chunk itself on caller-owned buffers: entries (in tensor, out tensor, slot, in0, n_in, out0, n_out, len)"""
    table = (_lib.ResampleEntry * len(entries))(*[
        _lib.ResampleEntry(in_dev=i.data_ptr() if n_in else None, out_dev=o.data_ptr() if n_out else None, in0=in0, out0=out0,
                           len=length, n_in=n_in, n_out=n_out, slot=slot, reserved=0)
        for i, o, slot, in0, n_in, out0, n_out, length in entries])
    vp = ctypes.c_void_p
    rc = _lib.lib().swn_resample_chunk(res.L, res.M, res.n_taps, vp(res._table.data_ptr()), vp(state.data_ptr()), capacity, table,
                                       len(entries), vp(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "resample_chunk")
    torch.cuda.synchronize()


@pytest.mark.parametrize("L,M", [(3, 2), (147, 320)], ids=["3-2", "147-320"])
def test_slots_fresh_starts_untouched_state_and_nan_around_the_buffers(gpu_ok, L, M):
    res = _res(L, M)
    H, cap = res.state_floats, 4
    x = _signal(2000, 21).to(DEV)
    want = res(x)[0]
    want1500 = res(x[:1500])[0]
    rdy = res.ready
    state = torch.full((cap * H,), NAN, dtype=torch.float32, device=DEV)
    # outputs live inside a NaN buffer with a margin on both sides; rows are longer than what the entries write
    pad, row = 64, res.out_count(1000) + 100
    out = torch.full((pad + 3 * row + pad,), NAN, dtype=torch.float32, device=DEV)
    o = [out[pad + k * row: pad + (k + 1) * row] for k in range(3)]

    def untouched(written):
        for k, n in enumerate(written):
            assert torch.isnan(o[k][n:]).all(), k
        assert torch.isnan(out[:pad]).all() and torch.isnan(out[-pad:]).all()

    _abi_call(res, state, cap, [(x, o[0], 0, 0, 1000, 0, rdy(1000), -1), (x, o[1], 2, 0, 300, 0, rdy(300), -1),
                                (x, o[2], 3, 0, 0, 0, 0, -1)])
    assert rdy(1000) > TILE or L < M
    assert torch.equal(o[0][:rdy(1000)], want[:rdy(1000)]) and torch.equal(o[1][:rdy(300)], want[:rdy(300)])
    untouched([rdy(1000), rdy(300), 0])
    st = state.view(cap, H)
    assert torch.isnan(st[1]).all()                                     # a slot no entry names keeps its floats
    assert torch.isnan(st[3]).all()                                     # nothing in, nothing out: untouched
    assert torch.equal(st[0], x[1000 - H:1000]) and torch.equal(st[2], x[300 - H:300])          # the last Q - 1 RAW inputs
    # slot 0 goes on where it stood; slot 2 starts again at in0 == 0, from zero history whatever it holds; slot 3 receives a
    # chunk shorter than the state, which yields nothing
    out.fill_(NAN)
    k0 = rdy(1500) - rdy(1000)
    _abi_call(res, state, cap, [(x[1000:], o[0], 0, 1000, 500, rdy(1000), k0, -1), (x, o[1], 2, 0, 300, 0, rdy(300), -1),
                                (x, o[2], 3, 0, 10, 0, rdy(10), -1)])
    assert rdy(10) == 0
    assert torch.equal(o[0][:k0], want[rdy(1000):rdy(1500)]) and torch.equal(o[1][:rdy(300)], want[:rdy(300)])
    untouched([k0, rdy(300), 0])
    assert torch.isnan(st[1]).all() and torch.equal(st[0], x[1500 - H:1500]) and torch.equal(st[2], x[300 - H:300])
    assert torch.equal(st[3], torch.cat([torch.zeros(H - 10, device=DEV), x[:10]]))
    # slot 0 ends: the flush with no new input gives the outputs that read the zeros past the end; slot 3's next chunk shifts
    # its state
    out.fill_(NAN)
    k0, k3 = res.out_count(1500) - rdy(1500), rdy(H + 3)
    assert k0 > 0 and k3 > 0
    _abi_call(res, state, cap, [(x, o[0], 0, 1500, 0, rdy(1500), k0, 1500), (x[10:], o[2], 3, 10, H - 7, 0, k3, -1)])
    assert torch.equal(o[0][:k0], want1500[rdy(1500):]) and torch.equal(o[2][:k3], want[:k3])
    untouched([k0, 0, k3])
    assert torch.equal(st[0], x[1500 - H:1500])                         # a flush receives nothing: the state stays
    assert torch.equal(st[3], x[3:H + 3])                               # a shift of the old one


def test_a_slot_reused_after_close_starts_from_zero(gpu_ok):
    res = melspec.Resampler(16000, 8000, capacity=1, device=DEV)
    x, y = _signal(900, 31), _signal(700, 32)
    s = res.open()
    res.run({s: x[:500]})                               # mid-way: its inputs stay in the slot's floats
    res.close(s)
    s2 = res.open()
    assert s2 == s
    got = torch.cat([res.run({s2: y[:333]})[s2], res.run({s2: y[333:]}, finish=[s2])[s2]])
    assert torch.equal(got, res(y)[0])
    with pytest.raises(RuntimeError, match="has ended"):
        res.run({s2: y[:5]})
    res.close(s2)


# ------------------------------------------------------------------------------------------------------ streams and pools
@functools.lru_cache(maxsize=None)
def _ext():
    fs, n_fft, hop, n_mels = GEOM
    return melspec.LogMelExtractor(fs, n_fft, hop, n_mels, device=DEV)


@functools.lru_cache(maxsize=None)
def _cut():
    return melspec.LowCut(GEOM[0], capacity=4, device=DEV)


@functools.lru_cache(maxsize=None)
def _front(fs_in):
    return melspec.Resampler(fs_in, GEOM[0], capacity=4, device=DEV)


@functools.lru_cache(maxsize=None)
def _composed(fs_in, n, seed, low_cut=True):
    """(signal at fs_in on the host, LogMelExtractor(LowCut(Resampler(signal))) as (F, n_mels)): computed once, shared"""
    x = _signal(n, seed, fs_in)
    y = _front(fs_in)(x)
    return x, _ext()(_cut()(y) if low_cut else y)[0]


@pytest.mark.parametrize("low_cut", [True, False], ids=["lowcut", "plain"])
@pytest.mark.parametrize("fs_in", [16000, 4000])
def test_stream_with_a_resampler_equals_the_one_shot_composition(gpu_ok, fs_in, low_cut):
    x, want = _composed(fs_in, 3001 * fs_in // 8000, 41, low_cut)
    res, cut = _front(fs_in), _cut() if low_cut else None
    free, cut_free = list(res._free), list(_cut()._free)
    stream = melspec.LogMelStream(_ext(), low_cut=cut, resample=res)
    assert res._free == free[1:]                                        # a slot of its own
    sizes = [1, 77, 0, 333, 5, 1023, fs_in // 100]
    got, at, i = [], 0, 0
    while at < x.numel():
        n = sizes[i % len(sizes)]
        got.append(stream.push(x[at:at + n]))
        at, i = at + n, i + 1
    got.append(stream.finish())
    assert res._free == free and _cut()._free == cut_free                # ... given back when the stream ends
    assert stream.n_received == res.out_count(x.numel())
    assert torch.equal(torch.cat(got), want)


@pytest.mark.parametrize("low_cut", [True, False], ids=["lowcut", "plain"])
def test_pool_with_a_resampler_equals_the_one_shot_composition(gpu_ok, low_cut):
    """three sessions behind 16 kHz audio with ragged chunks from the host and the device; the second is the shortest and ends
    mid-way in the call of its last chunk, the others are flushed in a call that brings them nothing"""
    fs_in, max_chunk = 16000, 450
    res = _front(fs_in)
    pool = melspec.LogMelPool(_ext(), capacity=3, max_chunk=max_chunk, low_cut=_cut() if low_cut else None, resample=res)
    pool.res_state.fill_(NAN)
    pool.windows.fill_(NAN)
    if low_cut:
        pool.hist.fill_(NAN)
    plans = []
    for i, n in enumerate((3000, 1700, 2333)):
        x, want = _composed(fs_in, n, 60 + i, low_cut)
        plans.append(dict(x=x, want=want, at=0, sess=pool.open(), got=[], sizes=[160, 37 + i, 0, 401, 800 + i, 3]))
    tick = 0
    while any(not p["sess"].finished for p in plans):
        chunks, fin = {}, []
        for i, p in enumerate(plans):
            if p["sess"].finished:
                continue
            if p["at"] >= p["x"].numel():
                fin.append(p["sess"])                                   # the flush with no new input
                continue
            c = p["x"][p["at"]:p["at"] + p["sizes"][tick % 6]]
            p["at"] += c.numel()
            chunks[p["sess"]] = c.to(DEV) if (tick + i) % 2 else c
            if i == 1 and p["at"] >= p["x"].numel():
                fin.append(p["sess"])
        new = pool.push_many(chunks, finish=fin)
        for p in plans:
            if p["sess"] in new:
                assert new[p["sess"]].shape[:2] == (1, GEOM[3]) and new[p["sess"]].is_contiguous()
                p["got"].append(new[p["sess"]])
        tick += 1
    assert res._free == list(range(res.capacity))                       # the Resampler's own slots are not used
    for i, p in enumerate(plans):
        got = torch.cat(p["got"], 2)[0].t()
        assert p["sess"].n_in == p["x"].numel() and p["sess"].n_received == res.out_count(p["x"].numel())
        assert got.shape == p["want"].shape and torch.equal(got, p["want"]), i
    # a chunk that would yield more than max_chunk is refused before any launch; a slot reused after close starts from zero
    pool.close(plans[0]["sess"])
    s = pool.open()
    state = pool.res_state.clone()
    with pytest.raises(ValueError, match="yields"):
        pool.push_many({s: torch.zeros(2 * max_chunk + 100)})
    assert torch.equal(pool.res_state, state) and s.n_in == 0
    x, want = _composed(fs_in, 1700, 61, low_cut)
    got = [pool.push_many({s: x[:850]})[s], pool.push_many({s: x[850:]}, finish=[s])[s]]
    assert torch.equal(torch.cat(got, 2)[0].t(), want)


# ------------------------------------------------------------------------------------------------------ the driver
def test_driver_resamples_on_the_device(gpu_ok, tmp_path):
    from scipy.io import wavfile
    fs_in, fs = 16000, 8000
    g = np.random.Generator(np.random.PCG64(5))
    t = np.arange(4800) / fs_in
    waves = {"utt_a": 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 + 0.05 * g.standard_normal(4800),
             "utt_b": (0.25 * np.sin(2 * np.pi * 50.0 * t) + 0.1 * np.sin(2 * np.pi * 1234.0 * t))[:3555]}
    wavdir = tmp_path / "wav"
    os.makedirs(wavdir)
    pcm = {}
    for name, x in waves.items():
        pcm[name] = np.round(x * 32767.0).astype(np.int16)
        wavfile.write(str(wavdir / (name + ".wav")), fs_in, pcm[name])
    argv = ["--waveforms", str(wavdir), "--fs", str(fs), "--fftl", "256", "--n_mels", "20", "--verbose", "0"]
    # without the flag the files are refused, as before
    assert FD.main(argv + ["--hdf5dir", str(tmp_path / "h5_refused")]) == 1
    assert not os.path.exists(FD.feature_path(str(tmp_path / "h5_refused"), "utt_a.wav"))
    h5d, h5h, h5n = tmp_path / "h5_device", tmp_path / "h5_host", tmp_path / "h5_none"
    on = argv + ["--resample", "true"]
    assert FD.main(on + ["--hdf5dir", str(h5d), "--wavdir", str(tmp_path / "wav_device"), "--highpass_on", "device"]) == 0
    assert FD.main(on + ["--hdf5dir", str(h5h), "--wavdir", str(tmp_path / "wav_host")]) == 0
    assert FD.main(on + ["--hdf5dir", str(h5n), "--highpass_cutoff", "0"]) == 0
    from shallow_wavenet_amd import dsp
    ext = melspec.LogMelExtractor(fs, 256, 40, 20, device=DEV)
    res = melspec.Resampler(fs_in, fs, device=DEV)
    cut = melspec.LowCut(fs, 70.0, device=DEV)
    for name in waves:
        raw = torch.from_numpy((pcm[name].astype(np.float64) / 32768.0).astype(np.float32))      # what the driver reads
        y = res(raw)
        assert y.shape == (1, (len(pcm[name]) + 1) // 2)
        read = lambda d: featio.read_dataset(FD.feature_path(str(d), name + ".wav"), "/feat_logmel")
        assert read(h5n).dtype == np.float32 and np.array_equal(read(h5n), ext(y)[0].cpu().numpy()), name
        assert np.array_equal(read(h5d), ext(cut(y))[0].cpu().numpy()), name
        host = dsp.low_cut_filter(y[0].cpu().numpy().astype(np.float64), fs, cutoff=70)
        assert np.array_equal(read(h5h), ext(torch.from_numpy(host.astype(np.float32)))[0].cpu().numpy()), name
        # --wavdir receives audio at --fs
        rate, dev_wav = wavfile.read(str(tmp_path / "wav_device" / (name + ".wav")))
        want = np.rint(np.clip(cut(y)[0].cpu().numpy(), -1.0, 1.0).astype(np.float64) * 32767.0).astype(np.int16)
        assert rate == fs and np.array_equal(dev_wav, want), name
        rate, host_wav = wavfile.read(str(tmp_path / "wav_host" / (name + ".wav")))
        assert rate == fs and host_wav.shape == dev_wav.shape
        assert np.abs(dev_wav.astype(np.int32)).max() > 1000            # the files hold a signal
