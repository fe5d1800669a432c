"""GPU: the stage-1 low cut on the device (swn_lowcut_chunk / torch.ops.swn.lowcut_chunk / melspec.LowCut), its fused form in
the log-mel pool (swn_logmel_pool_lowcut / LogMelPool(low_cut=)), LogMelStream(low_cut=) and `feature_extract_driver
--highpass_on device`.

The yardsticks are lowcut_ref.py: (b) the exact chain, bit for bit, on signals of zeros and +-2^k; (a) the float64 value with
the derived bound on general signals.  Everything about chunking, batching, slots, streams and pools is exact (torch.equal):
an output sample depends only on its absolute index and the signal.

Shapes: n_taps 1, 2, 255 and 256; lengths 1, n_taps - 2, n_taps - 1, n_taps, tile - 1, tile, tile + 1 (the kernel's tile is
_lib.LOWCUT_TILE = 1 024 outputs per block) and 3 001; every case of one tap count is one device call.  Batches of 3 and of 65
entries (a launch group takes 64).  Streams and pools at fs8000-n32-hop8-m4 and fs22050-n1024-hop110-m80 with signals of at
most 3 001 samples."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import lowcut_ref as LR
from shallow_wavenet_amd import _lib, dsp, featio, melspec, ops
from shallow_wavenet_amd import feature_extract_driver as FD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = _lib.LOWCUT_TILE
NAN = float("nan")
GEOMS = [(8000, 32, 8, 4), (22050, 1024, 110, 80)]
GEOM_IDS = [f"fs{fs}-n{n}-hop{hop}-m{m}" for fs, n, hop, m in GEOMS]


def _taps(n_taps):
    return dsp.low_cut_taps(22050, 70.0) if n_taps == 255 else LR.taps(n_taps)


def _filter(h, signals, state=None, slots=None, resets=None, capacity=None):
    """torch.ops.swn.lowcut_chunk on a list of host signals -> list of host fp32 arrays (one-shot from zero state by default)"""
    E = len(signals)
    taps = torch.from_numpy(np.ascontiguousarray(h, dtype=np.float64)).to(DEV)
    capacity = E if capacity is None else capacity
    if state is None:
        state = torch.full((max(1, capacity * (len(h) - 1)),), NAN, dtype=torch.float32, device=DEV)
    ins = [torch.from_numpy(np.asarray(x, dtype=np.float32)).to(DEV) for x in signals]
    out = torch.ops.swn.lowcut_chunk(taps, state, ins, list(range(E)) if slots is None else slots,
                                     [True] * E if resets is None else resets, capacity)
    return [out[e, :len(x)].cpu().numpy() for e, x in enumerate(signals)]


def _lengths(n_taps):
    return sorted({n for n in (1, n_taps - 2, n_taps - 1, n_taps, TILE - 1, TILE, TILE + 1, 3001) if n >= 1})


# ------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("n_taps", [1, 2, 255, 256])
def test_bit_exact_against_the_exact_chain(gpu_ok, n_taps):
    """impulses at 0 and at an odd index (y[t] = fl32(h[t - p])), all ones, random signals over {-1, 0, +1} and over powers of
    two, at every length: the bits of reference (b)"""
    h = _taps(n_taps)
    cases = []
    for n in _lengths(n_taps):
        cases.append(("impulse", 0, LR.exact_signal("impulse", n, at=0)))
        odd = min(n - 1, 301 if n > 301 else 3)
        if odd % 2 == 1:
            cases.append(("impulse", odd, LR.exact_signal("impulse", n, at=odd)))
        for kind in ("ones", "ternary", "pow2"):
            cases.append((kind, 0, LR.exact_signal(kind, n, seed=n)))
    got = _filter(h, [x for _, _, x in cases])
    h32 = h.astype(np.float32)
    for (kind, at, x), y in zip(cases, got):
        want = LR.exact_chain(h, x)
        assert y.dtype == np.float32 and np.array_equal(y, want), (n_taps, kind, at, len(x), int((y != want).sum()))
        if kind == "impulse":
            direct = np.zeros(len(x), dtype=np.float32)
            direct[at:at + n_taps] = h32[:len(x) - at]
            assert np.array_equal(y, direct), (n_taps, at, len(x))


@pytest.mark.parametrize("fs", [22050, 8000])
def test_general_signals_stay_inside_the_derived_bound(gpu_ok, fs):
    h = dsp.low_cut_taps(fs, 70.0)
    signals = [LR.general_signal(kind, 3001, fs, seed=i) for i, kind in enumerate(("noise", "hum", "half-silence"))]
    outs = _filter(h, signals)
    for kind, x, y in zip(("noise", "hum", "half-silence"), signals, outs):
        err, lim = np.abs(y.astype(np.float64) - LR.value64(h, x)), LR.bound(h, x)
        print(f"{kind} fs {fs}: max |y - r| / bound = {float((err / lim).max()):.3f}")
        assert np.all(err <= lim), (kind, float((err / lim).max()))
    assert np.all(outs[2][:3001 // 2] == 0) and np.any(outs[2] != 0)            # silence in, exact zeros out


# ------------------------------------------------------------------------------------------------------ invariances
@functools.lru_cache(maxsize=None)
def _signal(n, seed, fs=22050):
    """a general fp32 signal on the host; shared, never written to"""
    return torch.from_numpy(LR.general_signal("noise", n, fs, seed=seed))


@functools.lru_cache(maxsize=None)
def _cut(fs=22050, capacity=4):
    return melspec.LowCut(fs, capacity=capacity, device=DEV)


CHUNKS = [1, 0, 7, 0, 0, 254, 255, 0, 256, 1000, 0, 1228]          # 3 001 samples


def test_any_chunking_gives_the_one_shot_bits(gpu_ok):
    cut = _cut()
    x = _signal(sum(CHUNKS), 11)
    want = cut(x)[0]
    assert want.shape == (sum(CHUNKS),) and want.dtype == torch.float32
    for order in (CHUNKS, CHUNKS[::-1], [0] + CHUNKS):       # ... also when a session's first chunk is empty
        s = cut.open()
        got, at = [], 0
        for n in order:
            y = cut.run({s: x[at:at + n]})[s]
            assert y.shape == (n,)
            got.append(y)
            at += n
        cut.close(s)
        assert torch.equal(torch.cat(got), want)
    # other tap counts, through the operator: the state is n_taps - 1 floats, down to one and to none
    for n_taps in (256, 2, 1):
        h = LR.taps(n_taps)
        xs = x.numpy()
        want = _filter(h, [xs])[0]
        state = torch.full((max(1, n_taps - 1),), NAN, dtype=torch.float32, device=DEV)
        got, at = [], 0
        for i, n in enumerate(CHUNKS):
            got.append(_filter(h, [xs[at:at + n]], state=state, slots=[0], resets=[i == 0], capacity=1)[0])
            at += n
        assert np.array_equal(np.concatenate(got), want), n_taps


@pytest.mark.parametrize("rows", [3, 65])
def test_a_row_alone_equals_the_row_inside_a_ragged_batch(gpu_ok, rows):
    cut = _cut()
    lens = [3001, 1, 1500] + [200 + 37 * (i % 9) for i in range(rows - 3)]
    signals = [_signal(n, 100 + i) for i, n in enumerate(lens)]
    out = cut(signals)
    assert out.shape == (rows, 3001)
    for r in (0, 1, 2, rows - 1):
        assert torch.equal(out[r, :lens[r]], cut(signals[r])[0]), r
    # the padded form with lengths reads no float past a row's length
    batch = torch.full((rows, 3001), NAN)
    for r, s in enumerate(signals):
        batch[r, :lens[r]] = s
    again = cut(batch, lens)
    for r in range(rows):
        assert torch.equal(again[r, :lens[r]], out[r, :lens[r]]), r


# ------------------------------------------------------------------------------------------------------ slots, C ABI
def _abi_call(taps, state, capacity, entries):
    """swn_lowcut_chunk itself on caller-owned buffers: entries (in tensor, out tensor, slot, n, flags)"""
    table = (_lib.LowcutEntry * len(entries))(*[
        _lib.LowcutEntry(in_dev=i.data_ptr() if n else None, out_dev=o.data_ptr() if n else None, slot=slot, n=n, flags=flags,
                         reserved=0) for i, o, slot, n, flags in entries])
    rc = _lib.lib().swn_lowcut_chunk(taps.numel(), ctypes.c_void_p(taps.data_ptr()), ctypes.c_void_p(state.data_ptr()), capacity,
                                     table, len(entries), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "lowcut_chunk")
    torch.cuda.synchronize()


def test_slots_reset_untouched_state_and_nan_around_the_buffers(gpu_ok):
    cut = _cut()
    H, cap = cut.n_taps - 1, 4
    x = _signal(1500, 21).to(DEV)
    want = cut(x)[0]
    state = torch.full((cap * H,), NAN, dtype=torch.float32, device=DEV)
    # outputs live inside a NaN buffer with a margin on both sides; rows are longer than what the entries write
    pad, row = 64, 1100
    out = torch.full((pad + 3 * row + pad,), NAN, dtype=torch.float32, device=DEV)
    o = [out[pad + k * row: pad + (k + 1) * row] for k in range(3)]
    R = _lib.LOWCUT_RESET
    _abi_call(cut._taps, state, cap, [(x, o[0], 0, 1000, R), (x, o[1], 2, 300, R), (x, o[2], 3, 0, 0)])
    assert torch.equal(o[0][:1000], want[:1000]) and torch.equal(o[1][:300], want[:300])
    assert torch.isnan(o[0][1000:]).all() and torch.isnan(o[1][300:]).all() and torch.isnan(o[2]).all()
    assert torch.isnan(out[:pad]).all() and torch.isnan(out[-pad:]).all()
    st = state.view(cap, H)
    assert torch.isnan(st[1]).all()                                     # a slot no entry names keeps its floats
    assert torch.isnan(st[3]).all()                                     # n == 0 without RESET leaves its slot untouched
    assert torch.equal(st[0], x[1000 - H:1000]) and torch.equal(st[2], x[300 - H:300])      # the last n_taps - 1 RAW samples
    # slot 0 goes on where it stood; slot 2 restarts from zero history; slot 3 is cleared by an empty RESET
    out.fill_(NAN)
    _abi_call(cut._taps, state, cap, [(x[1000:], o[0], 0, 500, 0), (x, o[1], 2, 300, R), (x, o[2], 3, 0, R)])
    assert torch.equal(o[0][:500], want[1000:1500]) and torch.equal(o[1][:300], want[:300])
    assert torch.isnan(o[0][500:]).all() and torch.isnan(o[1][300:]).all() and torch.isnan(o[2]).all()
    assert torch.isnan(st[1]).all() and torch.equal(st[3], torch.zeros(H, device=DEV))
    # a chunk shorter than the state shifts it: 10 samples into slot 3
    _abi_call(cut._taps, state, cap, [(x, o[2], 3, 10, 0)])
    assert torch.equal(o[2][:10], want[:10]) and torch.isnan(o[2][10:]).all()
    assert torch.equal(st[3], torch.cat([torch.zeros(H - 10, device=DEV), x[:10]]))


# ------------------------------------------------------------------------------------------------------ streams
@functools.lru_cache(maxsize=None)
def _ext(geom):
    fs, n_fft, hop, n_mels = geom
    return melspec.LogMelExtractor(fs, n_fft, hop, n_mels, device=DEV)


@functools.lru_cache(maxsize=None)
def _composed(geom, n, seed):
    """(raw signal on the host, LogMelExtractor(LowCut(signal)) as (F, n_mels)): computed once, shared, never written to"""
    x = _signal(n, seed, geom[0])
    return x, _ext(geom)(_cut(geom[0])(x))[0]


@pytest.mark.parametrize("chunk", ["10ms", "odd"])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_stream_with_a_low_cut_equals_the_one_shot_composition(gpu_ok, geom, chunk):
    x, want = _composed(geom, 3001, 31)
    cut = _cut(geom[0])
    free = list(cut._free)
    stream = melspec.LogMelStream(_ext(geom), low_cut=cut)
    assert cut._free == free[1:]                                        # a slot of its own
    sizes = [geom[0] // 100] if chunk == "10ms" else [1, 77, 0, 333, 5, 1023]
    got, at, i = [], 0, 0
    while at < x.numel():
        n = sizes[i % len(sizes)]
        got.append(stream.push(x[at:at + n]))
        at, i = at + n, i + 1
    got.append(stream.finish())
    assert cut._free == free                                            # ... given back when the stream ends
    assert torch.equal(torch.cat(got), want)


# ------------------------------------------------------------------------------------------------------ pools
def _drive_pool(pool, geom, n_sessions, max_chunk, reopen=None):
    """sessions at different phases: session i opens at tick i % 3 and is fed chunks of its own sizes until its signal ends.
    `reopen`: that session (0: it sits in slot 0, the first a pool hands out again) is closed after tick 3, mid-way, and a new
    signal opened in its slot.  -> [(frames, want)]"""
    pool.hist.fill_(NAN)
    pool.windows.fill_(NAN)
    plans = []
    for i in range(n_sessions):
        n = geom[1] // 2 + 1 + (i * 53) % 700 + (1500 if i < 3 else 0)
        x, want = _composed(geom, n, 200 + i)
        plans.append(dict(x=x, want=want, at=0, opens=i % 3, sess=None, got=[], sizes=[max_chunk, 1 + (i * 7) % max_chunk, 0,
                                                                                         max_chunk // 3 + i % 5]))
    done, tick = [], 0
    while any(p["at"] < p["x"].numel() or p["sess"] is None for p in plans):
        chunks, fin = {}, []
        for i, p in enumerate(plans):
            if tick < p["opens"]:
                continue
            if p["sess"] is None:
                p["sess"] = pool.open()
            if p["at"] >= p["x"].numel():
                continue
            n = p["sizes"][tick % 4]
            c = p["x"][p["at"]:p["at"] + n]
            p["at"] += c.numel()
            chunks[p["sess"]] = c.to(DEV) if (tick + i) % 2 else c          # from the host and from the device in turn
            if p["at"] >= p["x"].numel():
                fin.append(p["sess"])
        new = pool.push_many(chunks, finish=fin)
        for p in plans:
            if p["sess"] in new:
                p["got"].append(new[p["sess"]])
        for s in fin:
            pool.close(s)
        if reopen is not None and tick == 3 and plans[reopen]["at"] < plans[reopen]["x"].numel():
            old = plans[reopen]
            slot = old["sess"].slot
            pool.close(old["sess"])                                     # mid-way: its history stays in the slot's floats
            x, want = _composed(geom, geom[1] + 999, 777)
            fresh = dict(x=x, want=want, at=0, opens=0, sess=pool.open(), got=[], sizes=[5, max_chunk, 1, 0])
            assert fresh["sess"].slot == slot
            # what the closed session returned so far is a prefix of its frames
            part = torch.cat(old["got"], 2)[0].t()
            assert torch.equal(part, old["want"][:part.shape[0]])
            plans[reopen] = fresh
            reopen = None
        tick += 1
    for p in plans:
        done.append((torch.cat(p["got"], 2)[0].t(), p["want"]))
    return done


@pytest.mark.parametrize("geom,n_sessions", [(GEOMS[0], 3), (GEOMS[0], 65), (GEOMS[1], 3)],
                         ids=[GEOM_IDS[0] + "-3", GEOM_IDS[0] + "-65", GEOM_IDS[1] + "-3"])
def test_pool_with_a_low_cut_equals_the_one_shot_composition(gpu_ok, geom, n_sessions):
    max_chunk = 400
    pool = melspec.LogMelPool(_ext(geom), capacity=n_sessions, max_chunk=max_chunk, low_cut=_cut(geom[0]))
    for i, (got, want) in enumerate(_drive_pool(pool, geom, n_sessions, max_chunk, reopen=0)):
        assert got.shape == want.shape and torch.equal(got, want), i


def test_pool_history_holds_the_last_raw_samples(gpu_ok):
    geom = GEOMS[0]
    cut = _cut(geom[0])
    H = cut.n_taps - 1
    pool = melspec.LogMelPool(_ext(geom), capacity=2, max_chunk=400, low_cut=cut)
    pool.hist.fill_(NAN)
    x = _signal(700, 41, geom[0]).to(DEV)
    a, b = pool.open(), pool.open()
    pool.push_many({a: x[:100]})
    assert torch.equal(pool.hist[0], torch.cat([torch.zeros(H - 100, device=DEV), x[:100]]))        # shorter than the history
    assert torch.isnan(pool.hist[1]).all()                              # a slot no entry names keeps its floats
    pool.push_many({a: x[100:103], b: x[:0]})
    assert torch.equal(pool.hist[0], torch.cat([torch.zeros(H - 103, device=DEV), x[:103]]))        # a shift of the old one
    assert torch.isnan(pool.hist[1]).all()                              # nothing received: untouched
    pool.push_many({a: x[103:503]})
    assert torch.equal(pool.hist[0], x[503 - H:503])
    # the window holds the FILTERED samples
    assert torch.equal(pool.windows[0, :a.n_held], cut(x[:503])[0][a.t0:a.t0 + a.n_held])


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_without_a_low_cut_the_pool_gives_the_bits_it_gave(gpu_ok, geom):
    ext = _ext(geom)
    x = _signal(3001, 51, geom[0])
    want = ext(x)[0]                                                    # the RAW signal's features
    pools = [melspec.LogMelPool(ext, 2, 400), melspec.LogMelPool(ext, 2, 400, low_cut=None),
             melspec.LogMelPool(ext, capacity=2, max_chunk=400, linear=False, low_cut=None)]
    stream = melspec.LogMelStream(ext, low_cut=None)
    sess = [p.open() for p in pools]
    got, ref = [[] for _ in pools], []
    for at in range(0, 3001, 333):
        c = x[at:at + 333]
        last = at + 333 >= 3001
        for k, (p, s) in enumerate(zip(pools, sess)):
            got[k].append(p.push_many({s: c}, finish=[s] if last else [])[s])
        ref.append(stream.push(c))
    ref.append(stream.finish())
    for p, g in zip(pools, got):
        assert p.hist is None and p._op is ops.logmel_pool_impl
        assert torch.equal(torch.cat(g, 2)[0].t(), want)
    assert torch.equal(torch.cat(ref), want)


# ------------------------------------------------------------------------------------------------------ the driver
def test_driver_with_the_filter_on_the_device(gpu_ok, tmp_path):
    from scipy.io import wavfile
    fs = 16000
    g = np.random.Generator(np.random.PCG64(5))
    t = np.arange(2400) / fs
    waves = {"utt_a": 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 + 0.05 * g.standard_normal(2400),
             "utt_b": (0.25 * np.sin(2 * np.pi * 50.0 * t) + 0.1 * np.sin(2 * np.pi * 1234.0 * t))[:1777],
             "utt_c": 0.2 * g.standard_normal(900)}
    wavdir = tmp_path / "wav"
    os.makedirs(wavdir)
    pcm = {}
    for name, x in waves.items():
        pcm[name] = np.round(x * 32767.0).astype(np.int16)
        wavfile.write(str(wavdir / (name + ".wav")), fs, pcm[name])
    argv = ["--waveforms", str(wavdir), "--fs", str(fs), "--fftl", "512", "--n_mels", "40", "--verbose", "0"]
    h5d, h5h = tmp_path / "h5_device", tmp_path / "h5_host"
    assert FD.main(argv + ["--hdf5dir", str(h5d), "--wavdir", str(tmp_path / "wav_device"), "--highpass_on", "device"]) == 0
    assert FD.main(argv + ["--hdf5dir", str(h5h), "--wavdir", str(tmp_path / "wav_host")]) == 0
    ext = melspec.LogMelExtractor(fs, 512, 80, 40, device=DEV)
    cut = melspec.LowCut(fs, 70.0, device=DEV)
    for name in waves:
        raw = torch.from_numpy((pcm[name].astype(np.float64) / 32768.0).astype(np.float32))      # what the driver reads
        y = cut(raw)
        got = featio.read_dataset(FD.feature_path(str(h5d), name + ".wav"), "/feat_logmel")
        assert got.dtype == np.float32 and np.array_equal(got, ext(y)[0].cpu().numpy()), name
        _, dev_wav = wavfile.read(str(tmp_path / "wav_device" / (name + ".wav")))
        _, host_wav = wavfile.read(str(tmp_path / "wav_host" / (name + ".wav")))
        want = np.rint(np.clip(y[0].cpu().numpy(), -1.0, 1.0).astype(np.float64) * 32767.0).astype(np.int16)
        assert np.array_equal(dev_wav, want), name                      # written from the device result
        step = np.abs(dev_wav.astype(np.int32) - host_wav.astype(np.int32))
        print(f"{name}: {int((step > 0).sum())} of {step.size} PCM samples differ from the host filter's, max {int(step.max())}")
        assert step.max() <= 1, name
        assert np.abs(dev_wav.astype(np.int32)).max() > 1000            # the files hold a signal
    # --highpass_cutoff 0 still means no filter, wherever it would have run
    h5n = tmp_path / "h5_none"
    assert FD.main(argv + ["--hdf5dir", str(h5n), "--wavdir", str(tmp_path / "wav_none"), "--highpass_on", "device",
                           "--highpass_cutoff", "0"]) == 0
    assert not (tmp_path / "wav_none").exists()
    raw = torch.from_numpy((pcm["utt_c"].astype(np.float64) / 32768.0).astype(np.float32))
    assert np.array_equal(featio.read_dataset(FD.feature_path(str(h5n), "utt_c.wav"), "/feat_logmel"), ext(raw)[0].cpu().numpy())
