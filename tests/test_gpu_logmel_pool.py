"""GPU: the log-mel pool (swn_logmel_pool / torch.ops.swn.logmel_pool / melspec.LogMelPool).  One call per tick hands every
session its new frames; each session's frames, concatenated, are the one-shot features of its whole signal bit for bit -
whatever the chunking, whoever shares its calls, whichever slot it sits in and whatever that slot or the rest of the window
memory held before.  All comparisons are exact (torch.equal against LogMelExtractor.__call__, which test_gpu_melspec.py pins
to the float64 yardstick).

Shapes: the geometries of melspec_ref.GEOMETRIES; three sessions of 3 001, 1 703 and n_fft / 2 + 1 samples that open at
ticks 0, 2 and 5 and are fed seeded schedules with 0-sample, 1-sample and max_chunk-sample chunks (max_chunk 400) and ticks
without anything, from the host and from the device in turn; 65 sessions of about 200 samples at the smallest geometry (the
per-call entry limit is 64)."""
import dataclasses
import functools
import random

import pytest
import torch

import melspec_ref as MR
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import melspec
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodePool
from shallow_wavenet_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOM_IDS = [f"fs{fs}-n{n}-hop{hop}-m{m}" for fs, n, hop, m in MR.GEOMETRIES]
MAX_CHUNK = 400
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _ext(geom):
    fs, n_fft, hop, n_mels = geom
    return melspec.LogMelExtractor(fs, n_fft, hop, n_mels, floor=MR.FLOOR, device=DEV)


@functools.lru_cache(maxsize=None)
def _signal(geom, length, seed, kind="broadband"):
    """(x on the host, one-shot log features (n_mels, F), one-shot linear features) - computed once, shared, never written to"""
    x = torch.from_numpy(MR.signal(kind, length, geom[0], seed=seed))
    ext = _ext(geom)
    return x, ext(x)[0].t().contiguous(), ext(x, linear=True)[0].t().contiguous()


def _schedule(rng, length, max_chunk):
    """chunk sizes that sum to `length`: None is a tick without anything; 0, 1 and max_chunk come first (in a seeded order,
    as far as the signal reaches), then sizes drawn from 0 .. max_chunk"""
    head = [0, 1, max_chunk, None, max_chunk // 3]
    rng.shuffle(head)
    out, left = [], length
    while left > 0:
        n = head.pop() if head else rng.choice([None, 0, 1, rng.randint(0, max_chunk), rng.randint(0, max_chunk), max_chunk])
        if n is not None:
            n = min(n, left)
            left -= n
        out.append(n)
    return out


class _Run:
    """one signal on its way through a pool"""

    def __init__(self, geom, length, seed, opens_at, ends_with_chunk, rng):
        self.x, self.want, self.want_linear = _signal(geom, length, seed)
        self.opens_at, self.ends_with_chunk = opens_at, ends_with_chunk
        self.plan = _schedule(rng, length, MAX_CHUNK)
        self.at, self.session, self.got = 0, None, []


def _poison(pool):
    """NaN in every window float that no open session holds"""
    held = {s.slot: s.n_held for s in pool._open.values()}
    for slot in range(pool.capacity):
        pool.windows[slot, held.get(slot, 0):] = NAN


def _drive(pool, runs, poison=False, raise_at=None):
    """tick by tick until every run has ended; chunks alternate between the host and the device"""
    tick, n_dev = 0, 0
    if poison:
        pool.windows.fill_(NAN)
    while any(r.session is None or not r.session.finished for r in runs):
        chunks, fin = {}, []
        for r in runs:
            if tick < r.opens_at or (r.session is not None and r.session.finished):
                continue
            if r.session is None:
                r.session = pool.open()
            if not r.plan:                                      # everything pushed: the end comes in a tick of its own
                fin.append(r.session)
                continue
            n = r.plan.pop(0)
            if n is None:
                continue
            c = r.x[r.at:r.at + n]
            n_dev += 1
            chunks[r.session] = c.to(DEV) if n_dev % 2 else c
            r.at += n
            if not r.plan and r.ends_with_chunk:
                fin.append(r.session)
        if raise_at is not None and tick == raise_at:
            # a session that cannot end yet beside the valid chunks of the tick: the call raises and nothing moves
            short = pool.open()
            before = [(r.session.n_received, r.session.n_frames, r.session.t0, r.session.n_held) for r in runs if r.session]
            with pytest.raises(ValueError, match="longer than"):
                pool.push_many({**chunks, short: torch.zeros(3)}, finish=fin + [short])
            assert before == [(r.session.n_received, r.session.n_frames, r.session.t0, r.session.n_held) for r in runs if r.session]
            assert short.n_received == 0 and not short.finished
            pool.close(short)
        new = pool.push_many(chunks, finish=fin)
        assert set(new) == set(chunks) | set(fin)
        for r in runs:
            if r.session in new:
                v = new[r.session]
                assert v.shape[:2] == (1, r.want.shape[0]) and v.is_contiguous() and v.dtype == torch.float32 and v.is_cuda
                r.got.append(v)
        if poison:
            _poison(pool)
        tick += 1
        assert tick < 400
    return tick


def _three(geom, seed):
    n_fft = geom[1]
    rng = random.Random(seed)
    return [_Run(geom, 3001, seed + 1, 0, True, rng), _Run(geom, 1703, seed + 2, 2, False, rng),
            _Run(geom, n_fft // 2 + 1, seed + 3, 5, True, rng)]


def _check(runs, linear=False):
    for i, r in enumerate(runs):
        got = torch.cat(r.got, 2)[0]
        want = r.want_linear if linear else r.want
        assert r.session.finished and r.session.n_received == r.x.numel() and r.session.n_frames == want.shape[1]
        assert got.shape == want.shape and torch.isfinite(got).all(), (i, got.shape, want.shape)
        assert torch.equal(got, want), (i, int((got != want).sum()))


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "poisoned"])
@pytest.mark.parametrize("geom", MR.GEOMETRIES, ids=GEOM_IDS)
def test_every_session_equals_the_one_shot_call(gpu_ok, geom, poison):
    """poisoned: NaN in the whole window memory before the first push, and again after every tick wherever no session holds a
    sample - the outputs are those of the clean run: finite, and the one-shot features"""
    runs = _three(geom, 100 + geom[1])
    sizes = [n for r in runs for n in r.plan]
    assert 0 in sizes and 1 in sizes and MAX_CHUNK in sizes and None in sizes
    pool = melspec.LogMelPool(_ext(geom), capacity=4, max_chunk=MAX_CHUNK)
    assert pool.windows.shape == (4, geom[1] + MAX_CHUNK) and pool.windows.device.type == "cuda"
    _drive(pool, runs, poison=poison)
    _check(runs)
    assert sorted(r.session.slot for r in runs) == [0, 1, 2]
    for r in runs:
        assert r.session.n_held <= geom[1] + MAX_CHUNK


def test_linear_amplitudes(gpu_ok):
    geom = MR.GEOMETRIES[1]
    runs = _three(geom, 7)
    _drive(melspec.LogMelPool(_ext(geom), capacity=3, max_chunk=MAX_CHUNK, linear=True), runs)
    _check(runs, linear=True)


def test_on_a_side_stream(gpu_ok):
    geom = MR.GEOMETRIES[3]
    runs = _three(geom, 11)
    pool = melspec.LogMelPool(_ext(geom), capacity=3, max_chunk=MAX_CHUNK)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _drive(pool, runs, poison=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _check(runs)


def test_a_reused_slot_knows_nothing_of_its_past(gpu_ok):
    geom = MR.GEOMETRIES[2]
    ext = _ext(geom)
    pool = melspec.LogMelPool(ext, capacity=2, max_chunk=MAX_CHUNK)
    xa, _, _ = _signal(geom, 3001, 31)
    xb, want_b, _ = _signal(geom, 1703, 32, "tone")
    xc, want_c, _ = _signal(geom, 3001, 33)
    a, c = pool.open(), pool.open()
    got_b, got_c = [], []
    for i in range(0, 1200, 300):                               # a is closed in the middle of its signal
        new = pool.push_many({a: xa[i:i + 300], c: xc[i:i + 300].to(DEV)})
        got_c.append(new[c])
    assert a.n_frames > 0 and a.n_held > 0
    pool.close(a)
    b = pool.open()
    assert b.slot == a.slot and (b.n_received, b.n_frames, b.n_held, b.t0) == (0, 0, 0, 0)
    for i in range(0, 1800, 300):
        new = pool.push_many({b: xb[i:i + 300].to(DEV), c: xc[1200 + i:1200 + i + 300]}, finish=[b] if i == 1500 else [])
        got_b.append(new[b])
        got_c.append(new[c])
    got_c.append(pool.push_many({c: xc[3000:]}, finish=[c])[c])
    assert torch.equal(torch.cat(got_b, 2)[0], want_b) and torch.equal(torch.cat(got_c, 2)[0], want_c)
    with pytest.raises(RuntimeError, match="closed"):
        pool.push_many({a: xa[:10]})


def test_65_sessions_cross_the_entry_limit(gpu_ok):
    geom = MR.GEOMETRIES[0]
    ext = _ext(geom)
    base, _, _ = _signal(geom, 3001, 41)
    rows = [base[7 * i:7 * i + 190 + i % 23] for i in range(65)]
    want = ext(rows)                                            # (65, F_max, n_mels), zeros past a row's frames
    pool = melspec.LogMelPool(ext, capacity=65, max_chunk=128)
    sess = [pool.open() for _ in rows]
    got = [[] for _ in rows]
    for tick in range(2):
        new = pool.push_many({s: (r[:100] if tick == 0 else r[100:]) for s, r in zip(sess, rows)})
        assert list(new) == sess
        for g, s in zip(got, sess):
            g.append(new[s])
    new = pool.push_many({}, finish=sess)
    for i, (g, s, r) in enumerate(zip(got, sess, rows)):
        g.append(new[s])
        F = 1 + r.numel() // geom[2]
        assert torch.equal(torch.cat(g, 2)[0], want[i, :F].t()), i
        assert s.finished and s.n_frames == F


def test_a_raising_call_leaves_every_session_able_to_go_on(gpu_ok):
    geom = MR.GEOMETRIES[1]
    runs = _three(geom, 23)
    pool = melspec.LogMelPool(_ext(geom), capacity=4, max_chunk=MAX_CHUNK)
    assert _drive(pool, runs, raise_at=6) > 6
    _check(runs)


def test_mel_pool_into_decode_pool(gpu_ok):
    """audio in, mel, vocoder out for three sessions of different lengths: LogMelPool.push_many -> DecodePool.push_many ->
    step gives each the samples of net.decode on its one-shot features (same rng_seed and utterance id)"""
    cfg = dataclasses.replace(C.tiny(), n_aux=8)
    net = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=5, flavor="trained"), DEV)
    fs, n_fft, hop = 8000, 64, cfg.upsampling_factor
    ext = melspec.LogMelExtractor(fs, n_fft, hop, cfg.n_aux, device=DEV)
    lengths, uids = [1203, 805, 451], [4, 9, 2]
    xs = [torch.from_numpy(MR.signal("broadband", L, fs, seed=9 + i)).to(DEV) for i, L in enumerate(lengths)]
    mels = melspec.LogMelPool(ext, capacity=3, max_chunk=160)
    pool = DecodePool(net, 3, rng_seed=77)
    ms = [mels.open() for _ in xs]
    ds = [pool.open(utt_id=u) for u in uids]
    outs = [[] for _ in xs]
    for i in range(0, max(lengths), 160):                       # 20 ms of audio at a time
        live = [k for k, L in enumerate(lengths) if i < L]
        ending = [k for k in live if i + 160 >= lengths[k]]
        new = mels.push_many({ms[k]: xs[k][i:i + 160] for k in live}, finish=[ms[k] for k in ending])
        pool.push_many({ds[k]: new[ms[k]] for k in live}, finish=[ds[k] for k in ending])
        for s, res in pool.step().items():
            outs[ds.index(s)].append(res[0])
    while not all(s.done for s in ds):
        for s, res in pool.step().items():
            outs[ds.index(s)].append(res[0])
    for k, x in enumerate(xs):
        aux = ext(x).transpose(1, 2).contiguous()               # (1, n_aux, F)
        N = aux.shape[2] * cfg.upsampling_factor // cfg.seg
        want = net.decode(aux, N, rng_seed=77, utt_ids=[uids[k]], variant=pool.resolved_variant)[0]
        got = torch.cat(outs[k], 1)
        assert got.shape == want.shape == (1, N * cfg.seg) and torch.equal(got, want), k
