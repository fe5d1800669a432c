"""GPU: the stepped decode pool over several models of one geometry (swn_decode_pool_stepped_chunk_models /
SteppedModelPool).  Sessions of different models share ONE launch chain, and every session's out, heads and noise stay
bit-identical to HipNet.decode(variant=3) of that utterance alone with ITS model - whether the per-entry or the tile kernels
serve it, across the 16-model cap of a call, through a slot passing from one model to another while its prologue is spread
over ticks, fed by push_many and with a post-filter.  A tick over one model issues the single-model op, and the models op
with one model equals it bit for bit.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, ops
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import streaming
from shallow_wavenet_amd.postfilter import NoiseShapingRestorer
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import SteppedModelPool
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RNG_SEED = 4242
_NETS = {}


def _net(cfg, seed):
    """the model of synth_state_dict(cfg, seed), built once"""
    if (cfg, seed) not in _NETS:
        flavor = "trained" if cfg.kind == "laplace" else "xavier"
        _NETS[(cfg, seed)] = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=seed, flavor=flavor), DEV)
    return _NETS[(cfg, seed)]


def _models(cfg, n):
    nets = [_net(cfg, 5 + k) for k in range(n)]
    for i in range(min(n, 4)):
        for j in range(i):
            assert not torch.equal(nets[i].packed, nets[j].packed)
    return nets


def _seg(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


def _seed_of(cfg, rng):
    if rng.random() < 0.3:
        return None
    if cfg.kind == "softmax":
        return torch.tensor([int(rng.integers(0, cfg.n_quantize))], dtype=torch.int32)
    return torch.from_numpy(rng.uniform(-0.9, 0.9, (1, cfg.seg)).astype(np.float32))


def _solo(net, aux, n_steps, seed, utt_id):
    """HipNet.decode of the utterance alone: batch 1, variant 3, the pool's key, utterance id and seed"""
    return net.decode(aux.to(DEV), n_steps, want_heads=True, variant=3, rng_seed=RNG_SEED, want_noise=True,
                      seed=None if seed is None else seed.to(DEV), utt_ids=[utt_id])


class _Run:
    """one session of a pool run: features, seed, id, model and the pieces the pool returned"""

    def __init__(self, cfg, F, seed, utt_id, start, aux_seed, model):
        self.aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=aux_seed))
        self.F, self.seed, self.utt_id, self.start, self.model = F, seed, utt_id, start, model
        self.pushed, self.s = 0, None
        self.out, self.heads, self.noise, self.rest = [], [], [], []

    def collect(self, r):
        self.out.append(r[0]), self.heads.append(r[1]), self.noise.append(r[2])
        if len(r) > 3:
            self.rest.append(r[3])

    def cat(self):
        return torch.cat(self.out, 1), torch.cat(self.heads, 1), torch.cat(self.noise, 1)


def _check(net, r):
    n = r.s.steps_done
    ref_out, ref_heads, ref_used = _solo(net, r.aux, n, r.seed, r.utt_id)
    out, heads, used = r.cat()
    assert out.shape[1] == n * _seg(net.cfg)
    assert torch.equal(out, ref_out), (net.cfg, r.utt_id, r.model)
    assert torch.equal(heads, ref_heads), (net.cfg, r.utt_id, r.model)
    assert torch.equal(used, ref_used), (net.cfg, r.utt_id, r.model)


class _Counting:
    """torch.ops.swn with every call noted: (op name, address of a leading packed buffer or None, models of the call, entries
    of a stepped pool call that run at least one iteration)"""

    def __init__(self):
        self.real, self.calls = torch.ops.swn, []

    def __getattr__(self, name):
        op = getattr(self.real, name)

        def call(*a, **k):
            first = a[0].data_ptr() if isinstance(a[0], torch.Tensor) else None
            n_models, active = 1, None
            if name == "decode_pool_stepped_chunk_models":
                n_models, active = len(a[0]), sum(1 for n in a[6] if n > 0)
                assert len(set(a[1])) == n_models                        # the pool passes the models the call names
            elif name == "decode_pool_stepped_chunk":
                active = sum(1 for n in a[5] if n > 0)
            self.calls.append((name, first, n_models, active))
            return op(*a, **k)
        return call

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def counted(monkeypatch):
    c = _Counting()
    monkeypatch.setattr(streaming, "_O", c)
    return c


def _drive(pool, runs, rng, batched=False):
    """tick until every session is done: admit at its start tick, push 1-3 frames per tick (then finish) - per session or,
    batched, by one push_many per tick - a random step budget and, in some ticks, a prologue budget.  Ticks 0 .. 3 run one
    step and 100 prologue iterations at most: the sessions admitted at tick 0 (at most 4 frames) have all their features by
    tick 3 and none is through by then, so that tick's call holds every one of them."""
    tick, live = 0, []
    while any(r.s is None for r in runs) or live:
        for r in runs:
            if r.s is None and r.start <= tick:
                r.s = pool.open(seed=r.seed, utt_id=r.utt_id, model=r.model)
                assert r.s.model == r.model
                live.append(r)
        chunks, ending = {}, []
        for r in live:
            if not r.s.finished:
                piece = r.aux[:, :, r.pushed:r.pushed + int(rng.integers(1, 4))]
                r.pushed += piece.shape[2]
                if batched:
                    chunks[r.s] = piece if rng.random() < 0.5 else piece.to(DEV)
                    if r.pushed >= r.F:
                        ending.append(r.s)
                else:
                    (r.s.finish if r.pushed >= r.F else r.s.push)(piece.to(DEV))
        if batched and chunks:
            pool.push_many(chunks, finish=ending)
        steps = [None, 1, 7, 64, 150][int(rng.integers(0, 5))]
        pro = [None, None, 100, 300][int(rng.integers(0, 4))]
        res = pool.step(1 if tick < 4 else steps, max_prologue=100 if tick < 4 else pro)
        for r in live:
            if r.s in res:
                r.collect(res[r.s])
        for r in [r for r in live if r.s.done]:
            pool.close(r.s)
            live.remove(r)
        tick += 1
        assert tick < 2000


# NI = 6 | 5 positions per tile pass | NI = 8, out_2 as a mat-vec launch, rowvec_tile_kernel<9> | NI = 1
NETS = [("ref6_s1l4", C.ref6_laplace(1, 4)), ("ref6_s5l4", C.ref6_laplace(5, 4)), ("ref6_smx", C.ref6_softmax()),
        ("bl6_lap", C.bl6_laplace())]
SPLIT = {27: [0] * 16 + [1] * 8 + [2] * 3,     # two full tiles, one full tile, one partial tile
         5: [0, 0, 1, 1, 2]}                   # the per-entry kernels


@pytest.mark.parametrize("n_sess", [5, 27])
@pytest.mark.parametrize("name,cfg", NETS, ids=[n[0] for n in NETS])
def test_mixed_stepped_sessions_equal_their_solo_decodes(gpu_ok, counted, name, cfg, n_sess):
    """three models and a fourth that no session names; models interleaved over the slots.  Sessions 0 and 1 are the same
    utterance (features, seed, id) on models 0 and 1."""
    nets = _models(cfg, 4)
    rng = np.random.default_rng(len(name) + n_sess)
    rest = list(SPLIT[n_sess])
    rest.remove(0), rest.remove(1)                                       # sessions 0 and 1: the twins on models 0 and 1
    models = [0, 1] + [rest[i] for i in rng.permutation(len(rest))]
    assert sorted(models) == SPLIT[n_sess]
    twin_seed = _seed_of(cfg, rng)
    runs = []
    for i in range(n_sess):
        start = 0 if n_sess > 8 and i < 26 else int(rng.integers(0, 4))
        if i < 2:
            runs.append(_Run(cfg, 3, twin_seed, 31337, 0, aux_seed=99, model=models[i]))
        else:
            runs.append(_Run(cfg, int(rng.integers(1, 5)), _seed_of(cfg, rng), int(rng.integers(0, 100000)), start,
                             aux_seed=100 + i, model=models[i]))
    pool = SteppedModelPool(nets[0], 32, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    assert [pool.add_model(n) for n in nets[1:]] == [1, 2, 3]
    _drive(pool, runs, rng)
    for r in runs:
        assert r.s.steps_done == r.F * cfg.U // _seg(cfg)
        _check(nets[r.model], r)
    # not "every session ran model 0": the twins differ in their samples, not in their draws
    assert not torch.equal(runs[0].cat()[0], runs[1].cat()[0])
    assert torch.equal(runs[0].cat()[2], runs[1].cat()[2])
    mixed = [c for c in counted.calls if c[0] == "decode_pool_stepped_chunk_models"]
    assert mixed and all(2 <= c[2] <= 3 for c in mixed)
    if n_sess == 27:
        assert any(c[2] == 3 and c[3] >= 24 for c in mixed)             # the tile kernels ran over three models
    else:
        assert all(c[3] < 24 for c in mixed)


def test_seventeen_models_are_split_into_calls_of_sixteen(gpu_ok, counted):
    """34 sessions over 17 models in a pool of 40 slots: every tick is cut into calls of at most 16 models, and every session
    still equals its solo decode"""
    cfg = C.bl6_laplace()
    nets = _models(cfg, 17)
    rng = np.random.default_rng(17)
    pool = SteppedModelPool(nets[0], 40, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    assert [pool.add_model(n) for n in nets[1:]] == list(range(1, 17))
    runs = [_Run(cfg, int(rng.integers(1, 4)), _seed_of(cfg, rng), 900 + i, 0, aux_seed=700 + i, model=i % 17)
            for i in range(34)]
    for r in runs:
        r.s = pool.open(seed=r.seed, utt_id=r.utt_id, model=r.model)
    pool.push_many({r.s: r.aux for r in runs}, finish=[r.s for r in runs])
    assert counted.names() == ["frontend_pool_models"] * 3
    full = 0
    while not all(r.s.done for r in runs):
        before = len(counted.calls)
        n_open = sum(1 for r in runs if not r.s.done)
        res = pool.step(int(rng.integers(7, 40)), max_prologue=[None, 200][int(rng.integers(0, 2))])
        for r in runs:
            if r.s in res:
                r.collect(res[r.s])
        calls = counted.calls[before:]
        assert all(c[0].startswith("decode_pool_stepped_chunk") and c[2] <= 16 for c in calls)
        if n_open == 34:
            # sessions 0 .. 15 (16 models); the 17th model and, behind it, models 0 .. 14; models 15 and 16
            assert [(c[0], c[2]) for c in calls] == [("decode_pool_stepped_chunk_models", 16)] * 2 + \
                [("decode_pool_stepped_chunk_models", 2)]
            full += 1
    assert full >= 1
    for r in runs:
        _check(nets[r.model], r)


def test_a_freed_slot_passes_to_another_model_with_a_split_prologue(gpu_ok):
    """a model-0 session closed part-way frees its slot; a model-1 session BEGINs there and spreads its prologue over ticks of
    100 iterations while sessions of models 0 and 2 generate; a slot that no entry names stays byte-identical"""
    cfg = C.ref6_laplace(1, 4)
    nets = _models(cfg, 3)
    rng = np.random.default_rng(21)
    pool = SteppedModelPool(nets[0], 4, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    pool.add_model(nets[1]), pool.add_model(nets[2])
    runs = [_Run(cfg, 3, _seed_of(cfg, rng), 10 + i, 0, aux_seed=200 + i, model=m) for i, m in enumerate((0, 0, 2))]
    for r in runs:
        r.s = pool.open(seed=r.seed, utt_id=r.utt_id, model=r.model)
        r.s.finish(r.aux.to(DEV))
    idle = pool.open(utt_id=55, model=1)                                 # slot 3: opened, no features yet
    res = pool.step(40)
    for r in runs:
        r.collect(res[r.s])
    cut = runs[1]
    pool.close(cut.s)
    late = _Run(cfg, 2, _seed_of(cfg, rng), 77, 0, aux_seed=299, model=1)
    late.s = pool.open(seed=late.seed, utt_id=late.utt_id, model=late.model)
    assert late.s.slot == cut.s.slot and cut.model == 0 and late.s.model == 1 and idle.slot == 3
    late.s.finish(late.aux.to(DEV))
    stride = int(_lib.lib().swn_decode_session_floats(ctypes.byref(ops._desc(nets[0].dlist)), 1, 3))
    torch.cuda.synchronize()
    before = pool._session[3 * stride:4 * stride].clone()
    live, pro_ticks = [runs[0], runs[2], late], 0
    while live:
        res = pool.step(int(rng.integers(1, 90)), max_prologue=100)
        if late.s.steps_done == 0:
            pro_ticks += 1
            assert late.s not in res and all(r.s in res for r in live if r is not late)
        for r in live:
            if r.s in res:
                r.collect(res[r.s])
        live = [r for r in live if not r.s.done]
    torch.cuda.synchronize()
    assert pro_ticks >= 6                                                # 690 prologue iterations, 100 per tick
    assert torch.equal(pool._session[3 * stride:4 * stride].view(torch.int32), before.view(torch.int32))
    for r in (runs[0], runs[2], late):
        _check(nets[r.model], r)
    assert 0 < cut.s.steps_done < cut.s.steps_ready
    _check(nets[0], cut)


def test_single_model_ticks_issue_the_single_model_op(gpu_ok, monkeypatch):
    """control: a SteppedModelPool that never saw add_model, and one with two more models whose sessions all run model 2,
    issue decode_pool_stepped_chunk only - the latter with model 2's packed buffer; a mixed tick issues the models op"""
    cfg = C.bl6_laplace()
    nets = _models(cfg, 3)
    for extra, model in ((0, 0), (2, 2)):
        c = _Counting()
        monkeypatch.setattr(streaming, "_O", c)
        rng = np.random.default_rng(77)
        runs = [_Run(cfg, int(rng.integers(1, 4)), _seed_of(cfg, rng), 40 + i, int(rng.integers(0, 3)), aux_seed=500 + i,
                     model=model) for i in range(5)]
        pool = SteppedModelPool(nets[0], 8, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
        for n in nets[1:1 + extra]:
            pool.add_model(n)
        _drive(pool, runs, rng)
        for r in runs:
            _check(nets[model], r)
        assert {n for n in c.names()} == {"frontend", "decode_pool_stepped_chunk"}
        assert {x[1] for x in c.calls if x[0] == "decode_pool_stepped_chunk"} == {nets[model].packed.data_ptr()}
    # the second pool, now with a session of model 0 beside one of model 2
    c = _Counting()
    monkeypatch.setattr(streaming, "_O", c)
    pair = [_Run(cfg, 2, None, 60 + m, 0, aux_seed=600 + m, model=m) for m in (0, 2)]
    for r in pair:
        r.s = pool.open(seed=r.seed, utt_id=r.utt_id, model=r.model)
        r.s.finish(r.aux.to(DEV))
    while not all(r.s.done for r in pair):
        res = pool.step(50)
        for r in pair:
            if r.s in res:
                r.collect(res[r.s])
    assert {n for n in c.names()} == {"frontend", "decode_pool_stepped_chunk_models"}
    for r in pair:
        _check(nets[r.model], r)


def test_the_models_op_with_one_model_equals_the_single_model_op(gpu_ok):
    """the same tables through both ops, 27 entries (the tile kernels), then a resumed call in which entries run out at
    different iterations: out, heads, noise and the slot region of the session buffer are bit-equal"""
    cfg = C.ref6_laplace(1, 4)
    net = _models(cfg, 1)[0]
    d = ops._desc(net.dlist)
    E, cap = 27, 32
    rng = np.random.default_rng(5)
    feeder = SteppedModelPool(net, cap, rng_seed=RNG_SEED)               # only to finalise the conditioning
    conds = []
    for e in range(E):
        s = feeder.open(utt_id=e)
        s.finish(torch.from_numpy(synth_aux(cfg, 1, 2, seed=300 + e)).to(DEV))
        conds.append(s._stream._cond[0])
    slots = [int(x) for x in rng.permutation(cap)[:E]]
    n_pro = int(_lib.lib().swn_decode_stepped_prologue_iterations(ctypes.byref(d)))
    seeds = torch.from_numpy(rng.uniform(-0.9, 0.9, (E, cfg.seg)).astype(np.float32))
    ids = [int(x) for x in rng.integers(0, 1000, E)]
    first = [n_pro + int(x) for x in rng.integers(1, 20, E)]
    second = [int(x) for x in rng.integers(0, 16, E)]
    second[3] = second[11] = 0                                           # idle entries in the resumed call
    slot_floats = int(_lib.lib().swn_decode_session_floats(ctypes.byref(d), cap, 3))
    n_sess = ops.stepped_pool_models_session_floats(d, cap)
    got = []
    for several in (False, True):
        session = torch.zeros(n_sess, dtype=torch.float32, device=DEV)
        outs = []
        for it0s, n_its, begins, sd in (([0] * E, first, [True] * E, seeds), (first, second, [False] * E, None)):
            args = (session, conds, slots, it0s, n_its, begins, sd, ids, net.dlist, cap, RNG_SEED, True, True)
            if several:
                outs.append(torch.ops.swn.decode_pool_stepped_chunk_models([net.packed], [0] * E, *args))
            else:
                outs.append(torch.ops.swn.decode_pool_stepped_chunk(net.packed, *args))
        torch.cuda.synchronize()
        got.append((outs, session[:slot_floats].clone()))
    (one, sess_one), (many, sess_many) = got
    n_gen = [[n - n_pro for n in first], second]
    for c in range(2):
        for e in range(E):
            n = n_gen[c][e]
            assert torch.equal(one[c][0][e, :n * cfg.seg], many[c][0][e, :n * cfg.seg]), (c, e)
            assert torch.equal(one[c][1][e, :n], many[c][1][e, :n]), (c, e)
            assert torch.equal(one[c][2][e, :n], many[c][2][e, :n]), (c, e)
    assert float(one[0][0].abs().max()) > 0
    assert torch.equal(sess_one.view(torch.int32), sess_many.view(torch.int32))


ALPHA = 0.455
MEAN = np.concatenate([[0.9, 5.0, -3.0, -4.0, 0.1], 1.5 * np.exp(-0.15 * np.arange(50)) * np.cos(0.7 * np.arange(50))])


def test_push_many_and_post_filter_on_a_mixed_stepped_pool(gpu_ok, counted):
    """6 sessions over three models: one push_many per tick equals the per-session pushes, and the restored chunks
    concatenate to the restore of the whole output"""
    cfg = C.ref6_laplace(1, 4)
    nets = _models(cfg, 3)
    cat = []
    for batched in (False, True):
        rng = np.random.default_rng(91)
        runs = [_Run(cfg, int(rng.integers(1, 4)), _seed_of(cfg, rng), 70 + i, int(rng.integers(0, 2)), aux_seed=800 + i,
                     model=i % 3) for i in range(6)]
        restorer = NoiseShapingRestorer(MEAN, 22050, ALPHA, capacity=6, device=DEV)
        pool = SteppedModelPool(nets[0], 6, rng_seed=RNG_SEED, want_heads=True, want_noise=True, post_filter=restorer)
        pool.add_model(nets[1]), pool.add_model(nets[2])
        counted.calls.clear()
        _drive(pool, runs, rng, batched)
        names = set(counted.names())
        assert "decode_pool_stepped_chunk_models" in names
        if batched:
            assert "frontend_pool_models" in names and "frontend" not in names
        else:
            assert "frontend" in names and "frontend_pool_models" not in names
        for r in runs:
            _check(nets[r.model], r)
            whole = r.cat()[0]
            rest = torch.cat(r.rest, 1)
            assert rest.shape == whole.shape and float(rest.abs().max()) > 0
            assert torch.equal(rest[0], restorer.restore([whole[0]])[0]), r.utt_id
        cat.append([r.cat() for r in runs])
    for x, y in zip(*cat):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
