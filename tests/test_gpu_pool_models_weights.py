"""GPU: one decode pool launch over several models with bf16 / E4M3 head weights (DecodeModelPool,
swn_decode_pool_chunk_models_w16 / _w8).  The workgroup of a session reads its model's packed parameters AND its model's image -
the three streamed sections, the resident out_1 slices, the FP8 codes kept in LDS and the row scales - so every session equals,
bit for bit, the solo DecodeStream of its model in that format, whatever shares its launch.  All comparisons are exact
(torch.equal); every decode runs at most 300 steps."""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import streaming
from shallow_wavenet_amd.nets import dswnv as md
from shallow_wavenet_amd.postfilter import NoiseShapingRestorer
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodeModelPool, DecodePool, DecodeStream
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RNG = 0x5EED0123456789AB
MAX_STEPS = 300
FORMATS = [("bf16", "w16"), ("e4m3", "w8")]
# 10 .. 15 frames = 200 .. 300 steps per session on every net (across the 64-step noise staging of the Laplace kernels)
SMX = replace(C.bl6_softmax(), upsampling_factor=20)
S5L4 = replace(C.bl6_laplace(5, 4), upsampling_factor=100)
S1L4 = replace(C.bl6_laplace(1, 4), upsampling_factor=20)        # out_1 slices resident in LDS; e4m3: codes and scales there too
NETS = {"smx": SMX, "s5l4": S5L4, "s1l4": S1L4}
CASES = [("smx", 0), ("smx", 6), ("s5l4", 0), ("s5l4", 6), ("s1l4", 6)]
FRAMES, MODELS, IDS = [10, 13, 15, 12], [2, 0, 2, 1], [4, 9, 2, 7]


def _seg(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


def _sd(cfg, seed):
    return synth_state_dict(cfg, seed=seed, flavor="trained" if cfg.kind == "laplace" else "xavier")


@functools.lru_cache(maxsize=None)
def _net(key, seed):
    """model `seed` of geometry `key`, built once and never changed (the repack test builds its own)"""
    return HipNet.from_state_dict(NETS[key], _sd(NETS[key], seed), DEV)


@functools.lru_cache(maxsize=None)
def _aux(key, frames, seed):
    return torch.from_numpy(synth_aux(NETS[key], 1, frames, seed=seed)).to(DEV)


@functools.lru_cache(maxsize=None)
def _solo(key, seed, fmt, variant, frames, aux_seed, utt_id):
    """(out, heads) of the utterance alone on model `seed`: DecodeStream of batch 1 in format `fmt` (or "fp32")"""
    s = DecodeStream(_net(key, seed), 1, variant=variant, rng_seed=RNG, utt_ids=[utt_id], want_heads=True, weights=fmt)
    out, heads = s.finish(_aux(key, frames, aux_seed))
    assert out.shape[1] == frames * NETS[key].U <= MAX_STEPS * _seg(NETS[key])
    return out, heads


def _pool(key, fmt, variant, seeds, capacity, **kw):
    pool = DecodeModelPool(_net(key, seeds[0]), capacity, variant=variant, rng_seed=RNG, want_heads=True, weights=fmt, **kw)
    assert [pool.add_model(_net(key, s)) for s in seeds[1:]] == list(range(1, len(seeds)))
    return pool


def _run_to_end(pool, sess):
    """tick until every session is done -> {session: (out, heads)}"""
    got = {s: [] for s in sess}
    ticks = 0
    while not all(s.done for s in sess):
        for s, r in pool.step().items():
            got[s].append(r)
        ticks += 1
        assert ticks < 8
    return {s: (torch.cat([p[0] for p in got[s]], 1), torch.cat([p[1] for p in got[s]], 1)) for s in sess}


class _Counting:
    """torch.ops.swn with the name of every call noted"""

    def __init__(self):
        self.real, self.names = torch.ops.swn, []

    def __getattr__(self, name):
        op = getattr(self.real, name)

        def call(*a, **k):
            self.names.append(name)
            return op(*a, **k)
        return call


@pytest.fixture
def counted(monkeypatch):
    c = _Counting()
    monkeypatch.setattr(streaming, "_O", c)
    return c


# ------------------------------------------------------------------------------------------ 1, 2: sessions and their solos
@functools.lru_cache(maxsize=None)
def _mixed_run(key, variant, fmt):
    """capacity 5, three models (seeds 5, 6, 7), four sessions of models [2, 0, 2, 1]: push_many in pieces of 3 and 7 frames, one
    tick after each -> per session (out, heads), and the ops the pool issued"""
    c = _Counting()
    saved, streaming._O = streaming._O, c
    try:
        pool = _pool(key, fmt, variant, (5, 6, 7), 5)
        sess = [pool.open(utt_id=u, model=m) for u, m in zip(IDS, MODELS)]
        assert [s.slot for s in sess] == [0, 1, 2, 3]
        got = {s: [] for s in sess}
        at, tick = [0] * len(sess), 0
        while not all(s.done for s in sess):
            n = (3, 7)[tick % 2]
            tick += 1
            chunks, fin = {}, []
            for i, s in enumerate(sess):
                if s.finished:
                    continue
                chunks[s] = _aux(key, FRAMES[i], 20 + i)[:, :, at[i]:at[i] + n]
                at[i] += n
                if at[i] >= FRAMES[i]:
                    fin.append(s)
            pool.push_many(chunks, finish=fin)
            for s, r in pool.step().items():
                got[s].append(r)
            assert tick < 16
    finally:
        streaming._O = saved
    return [(torch.cat([p[0] for p in got[s]], 1), torch.cat([p[1] for p in got[s]], 1)) for s in sess], c.names


@pytest.mark.parametrize("fmt,sfx", FORMATS)
@pytest.mark.parametrize("key,variant", CASES, ids=[f"{k}_v{v}" for k, v in CASES])
def test_each_session_equals_its_solo_stream(gpu_ok, key, variant, fmt, sfx):
    runs, names = _mixed_run(key, variant, fmt)
    assert f"decode_pool_chunk_models_{sfx}" in names and "decode_pool_chunk_models" not in names
    for i, (out, heads) in enumerate(runs):
        want_out, want_heads = _solo(key, 5 + MODELS[i], fmt, variant, FRAMES[i], 20 + i, IDS[i])
        assert out.shape == want_out.shape and torch.equal(out, want_out), (key, variant, fmt, i, "out")
        assert heads.shape == want_heads.shape and torch.equal(heads, want_heads), (key, variant, fmt, i, "heads")


@pytest.mark.parametrize("fmt,sfx", FORMATS)
@pytest.mark.parametrize("key,variant", [("smx", 0), ("s5l4", 0), ("s1l4", 6)], ids=["smx", "s5l4", "s1l4"])
def test_no_silent_fallback_to_fp32_or_to_another_models_image(gpu_ok, key, variant, fmt, sfx):
    runs, _ = _mixed_run(key, variant, fmt)
    for i, (_, heads) in enumerate(runs):
        fp32 = _solo(key, 5 + MODELS[i], "fp32", variant, FRAMES[i], 20 + i, IDS[i])[1]
        other = _solo(key, 5 + (MODELS[i] + 1) % 3, fmt, variant, FRAMES[i], 20 + i, IDS[i])[1]
        assert heads.shape == fp32.shape == other.shape
        assert not torch.equal(heads, fp32), (key, fmt, i)
        assert not torch.equal(heads, other), (key, fmt, i)
        # the first step reads nothing but weights, conditioning and the seed: it differs already
        assert not torch.equal(heads[:, 0], fp32[:, 0]) and not torch.equal(heads[:, 0], other[:, 0]), (key, fmt, i)


# --------------------------------------------------------------------------------------------- 3: the cap of 16 models
@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_sixteen_models_share_a_launch_and_seventeen_take_two(gpu_ok, counted, fmt, sfx):
    """sixteen sessions of sixteen models: one launch.  Seventeen models (and an eighteenth session, of model 0 again, so that
    the second call is a mixed one too, with a local table [16, 0]): two calls, cut where the 17th model would enter"""
    key, n = "smx", _lib.POOL_MAX_MODELS + 1
    pool = _pool(key, fmt, 0, tuple(range(5, 5 + n)), n + 1)
    for count in (n - 1, n + 1):
        models = [k % n for k in range(count)]
        frames = [2 + k % 2 for k in range(count)]
        sess = [pool.open(utt_id=100 + k, model=m) for k, m in enumerate(models)]
        pool.push_many({s: _aux(key, frames[k], 40 + k) for k, s in enumerate(sess)}, finish=sess)
        del counted.names[:]
        got = _run_to_end(pool, sess)
        assert counted.names == [f"decode_pool_chunk_models_{sfx}"] * (1 if count < n else 2), count
        for k, s in enumerate(sess):
            want = _solo(key, 5 + models[k], fmt, 0, frames[k], 40 + k, 100 + k)
            assert torch.equal(got[s][0], want[0]) and torch.equal(got[s][1], want[1]), (count, k)
            pool.close(s)


# --------------------------------------------------------------------------------------------------------- 4: control
@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_a_pool_that_does_not_mix_issues_the_single_model_op(gpu_ok, counted, fmt, sfx):
    key = "smx"
    pool = _pool(key, fmt, 0, (5, 6, 7), 4)
    sess = [pool.open(utt_id=30 + k, model=1) for k in range(2)]
    pool.push_many({s: _aux(key, 2, 60 + k) for k, s in enumerate(sess)}, finish=sess)
    got = _run_to_end(pool, sess)
    assert counted.names == ["frontend_pool", f"decode_pool_chunk_{sfx}"]
    for k, s in enumerate(sess):
        want = _solo(key, 6, fmt, 0, 2, 60 + k, 30 + k)
        assert torch.equal(got[s][0], want[0]) and torch.equal(got[s][1], want[1]), k
        pool.close(s)
    del counted.names[:]
    sess = [pool.open(utt_id=30 + k, model=m) for k, m in enumerate((1, 2))]
    pool.push_many({s: _aux(key, 2, 60 + k) for k, s in enumerate(sess)}, finish=sess)
    got = _run_to_end(pool, sess)
    assert counted.names == ["frontend_pool_models", f"decode_pool_chunk_models_{sfx}"]
    for k, s in enumerate(sess):
        want = _solo(key, 6 + k, fmt, 0, 2, 60 + k, 30 + k)
        assert torch.equal(got[s][0], want[0]) and torch.equal(got[s][1], want[1]), k


# ------------------------------------------------------------------------------------------- 5: a slot changes its model
@pytest.mark.parametrize("fmt,sfx", FORMATS)
@pytest.mark.parametrize("key,variant", [("smx", 0), ("s1l4", 6)], ids=["smx", "s1l4"])
def test_a_slot_passes_from_one_model_to_another(gpu_ok, key, variant, fmt, sfx):
    """slot 0 runs half a session of model 0, is closed and reopened under model 1 (BEGIN) in a launch shared with a resumed
    session of model 0: the new session is model 1's stream, the other one is unaffected"""
    pool = _pool(key, fmt, variant, (5, 6), 2)
    first, stay = pool.open(utt_id=1, model=0), pool.open(utt_id=2, model=0)
    pool.push_many({first: _aux(key, 4, 70), stay: _aux(key, 6, 71)}, finish=[first, stay])
    half = first.steps_ready // 2
    res = pool.step(half)
    stay_parts = [res[stay]]
    assert torch.equal(res[first][1], _solo(key, 5, fmt, variant, 4, 70, 1)[1][:, :half])
    pool.close(first)
    late = pool.open(utt_id=3, model=1)
    assert late.slot == first.slot == 0 and stay.slot == 1
    pool.push_many({late: _aux(key, 3, 72)}, finish=[late])
    late_parts = []
    while not (late.done and stay.done):
        res = pool.step(50)
        if late in res:
            late_parts.append(res[late])
        if stay in res:
            stay_parts.append(res[stay])
    for parts, want in ((late_parts, _solo(key, 6, fmt, variant, 3, 72, 3)), (stay_parts, _solo(key, 5, fmt, variant, 6, 71, 2))):
        assert torch.equal(torch.cat([p[0] for p in parts], 1), want[0])
        assert torch.equal(torch.cat([p[1] for p in parts], 1), want[1])
    assert not torch.equal(torch.cat([p[1] for p in late_parts], 1), _solo(key, 5, fmt, variant, 3, 72, 3)[1])


# ---------------------------------------------------------------------------------------------------------- 6: repack
@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_a_repacked_model_brings_its_new_image(gpu_ok, fmt, sfx):
    key, cfg = "s1l4", S1L4
    nets = [HipNet.from_state_dict(cfg, _sd(cfg, s), DEV) for s in (5, 6)]          # this test's own: one is repacked
    pool = DecodeModelPool(nets[0], 4, variant=6, rng_seed=RNG, want_heads=True, weights=fmt)
    pool.add_model(nets[1])

    def tick(base):
        sess = [pool.open(utt_id=base + m, model=m) for m in (0, 1)]
        pool.push_many({s: _aux(key, 3, 80 + m) for m, s in enumerate(sess)}, finish=sess)
        got = _run_to_end(pool, sess)
        for s in sess:
            pool.close(s)
        return [got[s] for s in sess]

    before = tick(0)
    for m in (0, 1):
        want = _solo(key, 5 + m, fmt, 6, 3, 80 + m, m)
        assert torch.equal(before[m][0], want[0]) and torch.equal(before[m][1], want[1]), m
    new = _sd(cfg, 9)
    nets[1].repack([torch.from_numpy(new[k]).to(DEV) for k, _ in cfg.param_shapes()])
    after = tick(0)
    fresh = _solo(key, 9, fmt, 6, 3, 81, 1)                                     # a fresh net of the new weights, in the format
    assert torch.equal(after[1][0], fresh[0]) and torch.equal(after[1][1], fresh[1])
    assert not torch.equal(after[1][1], before[1][1])
    assert torch.equal(after[0][0], before[0][0]) and torch.equal(after[0][1], before[0][1])   # the other model: unchanged


# --------------------------------------------------------------------------------------------- 7: open_pool, post_filter
ALPHA = 0.455
MEAN = np.concatenate([[0.9, 5.0, -3.0, -4.0, 0.1], 1.5 * np.exp(-0.15 * np.arange(50)) * np.cos(0.7 * np.arange(50))])


@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_open_pool_returns_the_model_pool_and_its_post_filter_restores_as_the_solo_stream(gpu_ok, counted, fmt, sfx):
    key, cfg = "smx", SMX
    m = md.DSWNV(**cfg.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(cfg, 5).items()})
    m.cuda().eval()
    m.noise_rng_seed = RNG
    plain = m.open_pool(4, multi_model=True, weights=fmt)
    assert type(plain) is DecodeModelPool and plain.weights == fmt
    assert type(m.open_pool(4, multi_model=True)) is DecodePool and type(m.open_pool(4, weights=fmt)) is DecodePool
    pool = m.open_pool(4, multi_model=True, weights=fmt, post_filter=NoiseShapingRestorer(MEAN, 16000, ALPHA, capacity=4, device=DEV))
    assert type(pool) is DecodeModelPool and pool.add_model(_net(key, 6)) == 1
    frames, models = [3, 2, 3], [1, 0, 1]
    sess = [pool.open(utt_id=50 + k, model=mm) for k, mm in enumerate(models)]
    pool.push_many({s: _aux(key, frames[k], 90 + k) for k, s in enumerate(sess)}, finish=sess)
    got = {s: [] for s in sess}
    while not all(s.done for s in sess):
        for s, r in pool.step(25).items():
            assert len(r) == 3
            got[s].append(r)
    assert f"decode_pool_chunk_models_{sfx}" in counted.names
    for k, s in enumerate(sess):
        net = pool.net if models[k] == 0 else _net(key, 6)
        solo = DecodeStream(net, 1, rng_seed=RNG, utt_ids=[50 + k], weights=fmt,
                            post_filter=NoiseShapingRestorer(MEAN, 16000, ALPHA, capacity=1, device=DEV))
        out, _, restored = solo.finish(_aux(key, frames[k], 90 + k))
        assert torch.equal(torch.cat([p[0] for p in got[s]], 1), out), k
        mine = torch.cat([p[2] for p in got[s]], 1)
        assert mine.shape == restored.shape and torch.equal(mine, restored), k
        assert float(restored.abs().max()) > 0
