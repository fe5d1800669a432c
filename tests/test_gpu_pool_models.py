"""GPU: a decode pool over several models of one geometry (swn_decode_pool_chunk_models / swn_frontend_pool_models /
DecodePool.add_model).  Sessions of different models share launches and front end calls, and every session's out, heads and
noise stay bit-identical to HipNet.decode of that utterance alone with ITS model - fed by per-session pushes or by push_many,
across the 16-model cap of a call, through slot reuse from one model to another and with a post-filter.  A pool that never
saw add_model issues exactly the single-model ops.  All comparisons are exact."""
import numpy as np
import pytest
import torch

from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import streaming
from shallow_wavenet_amd.postfilter import NoiseShapingRestorer
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodePool, lookahead_frames
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


def _three(cfg):
    nets = [_net(cfg, s) for s in (5, 6, 7)]
    for i in range(3):
        for j in range(i):
            assert not torch.equal(nets[i].packed, nets[j].packed)
    return nets


def _seg(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


def _seed_of(cfg, rng):
    """a random seed waveform for one session, or None (zeros / Q/2)"""
    if rng.random() < 0.3:
        return None
    if cfg.kind == "softmax":
        return torch.tensor([int(rng.integers(0, cfg.n_quantize))], dtype=torch.int32)
    return torch.from_numpy(rng.uniform(-0.9, 0.9, (1, cfg.seg)).astype(np.float32))


def _solo(net, aux, n_steps, variant, seed, utt_id):
    """HipNet.decode of the utterance alone: batch 1, the pool's variant, key, utterance id and seed"""
    return net.decode(aux.to(DEV), n_steps, want_heads=True, variant=variant, rng_seed=RNG_SEED, want_noise=True,
                      seed=None if seed is None else seed.to(DEV), utt_ids=[utt_id])


class _Run:
    """one session of a pool run: features, seed, id, model and the pieces the pool returned"""

    def __init__(self, cfg, F, seed, utt_id, start, aux_seed, model):
        self.aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=aux_seed))
        self.F, self.seed, self.utt_id, self.start, self.model = F, seed, utt_id, start, model
        self.pushed, self.s = 0, None
        self.out, self.heads, self.noise = [], [], []

    def collect(self, r):
        self.out.append(r[0]), self.heads.append(r[1]), self.noise.append(r[2])

    def cat(self):
        return torch.cat(self.out, 1), torch.cat(self.heads, 1), torch.cat(self.noise, 1)


def _budget(rng):
    return [None, 1, 2, 3, 63, 64, 65, 127, int(rng.integers(1, 200))][int(rng.integers(0, 9))]


def _drive(pool, runs, rng, batched):
    """tick until every session is done: admit at its start tick (or when a slot frees up), 0-7 frames per tick and session after
    tick 0 (then finish) - through
    PoolSession.push / finish or, batched, one push_many per tick - and a random step budget per tick"""
    tick, live = 0, []
    while any(r.s is None for r in runs) or live:
        for r in runs:
            if r.s is None and r.start <= tick and len(live) < pool.capacity:
                r.s = pool.open(seed=r.seed, utt_id=r.utt_id, model=r.model)
                assert r.s.model == r.model
                live.append(r)
        chunks, ending = {}, []
        for r in live:
            if not r.s.finished:
                k = r.F if tick == 0 else int(rng.integers(0, 8))          # tick 0: whole utterances, see below
                piece = r.aux[:, :, r.pushed:r.pushed + k]
                r.pushed += piece.shape[2]
                if batched:
                    chunks[r.s] = piece if rng.random() < 0.5 else piece.to(DEV)
                    if r.pushed >= r.F:
                        ending.append(r.s)
                elif r.pushed >= r.F:
                    r.s.finish(piece.to(DEV))
                else:
                    r.s.push(piece.to(DEV))
        if batched and chunks:
            pool.push_many(chunks, finish=ending)
        # the sessions admitted at tick 0 (one per model at least, _runs) end their features there and run one step: that
        # tick's front end call and launch name every model, and these sessions then resume beside whatever comes later
        res = pool.step(1 if tick == 0 else _budget(rng))
        for r in live:
            if r.s in res:
                r.collect(res[r.s])
        for r in [r for r in live if r.s.done]:
            pool.close(r.s)
            live.remove(r)
        tick += 1
        assert tick < 5000


def _check(net, r, variant):
    n = r.s.steps_done
    ref_out, ref_heads, ref_used = _solo(net, r.aux, n, variant, r.seed, r.utt_id)
    out, heads, used = r.cat()
    assert out.shape[1] == n * _seg(net.cfg)
    assert torch.equal(out, ref_out), (net.cfg, variant, r.utt_id, r.model)
    assert torch.equal(heads, ref_heads), (net.cfg, variant, r.utt_id, r.model)
    assert torch.equal(used, ref_used), (net.cfg, variant, r.utt_id, r.model)


class _Counting:
    """torch.ops.swn with every call noted: (op name, address of a leading packed buffer or None)"""

    def __init__(self):
        self.real, self.calls = torch.ops.swn, []

    def __getattr__(self, name):
        op = getattr(self.real, name)

        def call(*a, **k):
            self.calls.append((name, a[0].data_ptr() if isinstance(a[0], torch.Tensor) else None))
            return op(*a, **k)
        return call

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def counted(monkeypatch):
    c = _Counting()
    monkeypatch.setattr(streaming, "_O", c)
    return c


def _runs(cfg, rng, n_models, frames=(2, 7)):
    """5 to 9 runs; the first n_models, one per model, are admitted at tick 0, so that tick's calls name every model"""
    n = int(rng.integers(5, 10))
    return [_Run(cfg, int(rng.integers(frames[0], frames[1] + 1)), _seed_of(cfg, rng), int(rng.integers(0, 100000)),
                 int(rng.integers(0, 6)) if i >= n_models else 0, aux_seed=100 + i,
                 model=int(rng.integers(0, n_models)) if i >= n_models else i)
            for i in range(n)]


POOL_NETS = [
    ("bl6w", C.bl6_laplace(), 2), ("bl6_sym", C.bl6_laplace(), 6), ("bl6w_lpc4", C.bl6_laplace(1, 4), 0),
    ("bl6_s5l4", C.bl6_laplace(5, 4), 0), ("bl6_smx", C.bl6_softmax(), 0),
    ("tiny_lap", C.tiny("laplace", 2, 4), 1), ("tiny_smx", C.tiny("softmax"), 1),
]


@pytest.mark.parametrize("batched", [False, True], ids=["push", "push_many"])
@pytest.mark.parametrize("name,cfg,variant", POOL_NETS, ids=[n[0] for n in POOL_NETS])
def test_mixed_model_sessions_equal_their_solo_decodes(gpu_ok, counted, name, cfg, variant, batched):
    """5 to 9 sessions of 2 to 7 frames over three models in a pool of 8 slots, models interleaved"""
    nets = _three(cfg)
    rng = np.random.default_rng(len(name) + 50 * batched)
    runs = _runs(cfg, rng, 3)
    assert {r.model for r in runs} == {0, 1, 2}
    pool = DecodePool(nets[0], 8, variant=variant, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    assert [pool.add_model(n) for n in nets[1:]] == [1, 2]
    _drive(pool, runs, rng, batched)
    for r in runs:
        assert r.s.steps_done == r.F * cfg.U // _seg(cfg)
        _check(nets[r.model], r, variant)
    names = counted.names()
    assert "decode_pool_chunk_models" in names                   # the launches were shared across models
    if batched:
        assert "frontend_pool_models" in names and "frontend" not in names


def test_a_session_runs_its_own_model_not_the_pools(gpu_ok):
    """control: the same utterance, id and seed in model 1 and in model 0 give different samples, and the pool's session of
    model 1 is model 1's"""
    cfg = C.bl6_laplace()
    nets = _three(cfg)
    pool = DecodePool(nets[0], 2, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    pool.add_model(nets[1])
    a = _Run(cfg, 3, None, 11, 0, aux_seed=400, model=0)
    b = _Run(cfg, 3, None, 11, 0, aux_seed=400, model=1)
    for r in (a, b):
        r.s = pool.open(seed=r.seed, utt_id=r.utt_id, model=r.model)
        r.s.finish(r.aux.to(DEV))
    res = pool.step()
    for r in (a, b):
        r.collect(res[r.s])
        _check(nets[r.model], r, 0)
    assert not torch.equal(b.cat()[0], a.cat()[0])
    assert not torch.equal(b.cat()[0], _solo(nets[0], b.aux, b.s.steps_done, 0, None, 11)[0])
    assert torch.equal(b.cat()[2], a.cat()[2])                    # the same draws: the key and the utterance id are shared


@pytest.mark.parametrize("batched", [False, True], ids=["push", "push_many"])
def test_pool_without_add_model_issues_the_single_model_ops(gpu_ok, monkeypatch, batched):
    """control: a pool that never saw add_model, and a pool with two more models whose sessions all run model 0, issue the
    same single-model ops with the pool's packed buffer, call for call, and return the same outputs"""
    cfg = C.bl6_laplace()
    nets = _three(cfg)
    logs, outs = [], []
    for extra in (0, 2):
        c = _Counting()
        monkeypatch.setattr(streaming, "_O", c)
        rng = np.random.default_rng(77)
        runs = _runs(cfg, rng, 1)
        pool = DecodePool(nets[0], 8, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
        for n in nets[1:1 + extra]:
            pool.add_model(n)
        _drive(pool, runs, rng, batched)
        for r in runs:
            _check(nets[0], r, 0)
        logs.append(c.calls)
        outs.append([r.cat() for r in runs])
    assert logs[0] == logs[1]
    allowed = {"frontend_pool", "decode_pool_chunk"} if batched else {"frontend", "decode_pool_chunk"}
    assert {n for n, _ in logs[0]} == allowed
    assert {p for _, p in logs[0]} == {nets[0].packed.data_ptr()}
    for x, y in zip(*outs):
        assert all(torch.equal(u, v) for u, v in zip(x, y))


# -------------------------------------------------------------------------------------------------- the front end alone
SENTINEL = -7.5


class _Utt:
    """one session driven through frontend_pool_models directly: its features, its buffers and where it stands"""

    def __init__(self, cfg, F, seed, model, N):
        self.full = torch.from_numpy(synth_aux(cfg, 1, F, seed=seed)).to(DEV)
        self.F, self.model = F, model
        self.aux = torch.zeros((cfg.n_aux, F + 3), dtype=torch.float32, device=DEV)
        self.cond = torch.full((F + 2, N), SENTINEL, dtype=torch.float32, device=DEV)
        self.received = self.final = 0

    def entry(self, upto, f1, fin):
        """the entry that appends frames [received, upto) and finalises [final, f1)"""
        return self.full[0, :, self.received:upto].contiguous().reshape(-1), upto, self.final, f1, fin


def _call(nets, utts, entries, model_of=None):
    pieces = [e[0] for e in entries if e[0].numel()]
    torch.ops.swn.frontend_pool_models(
        [n.packed for n in nets], [u.model for u in utts] if model_of is None else model_of, [u.aux for u in utts],
        [u.cond for u in utts], torch.cat(pieces) if pieces else None, [e[1] - u.received for u, e in zip(utts, entries)],
        [e[1] for e in entries], [e[2] for e in entries], [e[3] for e in entries], [e[4] for e in entries], nets[0].dlist)
    for u, e in zip(utts, entries):
        u.received, u.final = e[1], e[3]


def _rows_ok(nets, u):
    """rows [0, final) are the one-shot front end's with the session's model, every other row still holds the sentinel"""
    want = torch.ops.swn.frontend(nets[u.model].packed, u.full, nets[0].dlist)[0][0]
    assert torch.equal(u.cond[:u.final], want[:u.final]), (u.model, u.F, u.final)
    assert bool((u.cond[u.final:] == SENTINEL).all()), (u.model, u.F, u.final)
    assert torch.equal(u.aux[:, :u.received], u.full[0, :, :u.received])
    assert int(torch.count_nonzero(u.aux[:, u.received:])) == 0


@pytest.mark.parametrize("name,cfg", [("bl6_lap", C.bl6_laplace()), ("tiny_lap", C.tiny("laplace", 2, 4))],
                         ids=["bl6_lap", "tiny_lap"])
def test_front_end_rows_equal_each_models_one_shot_front_end(gpu_ok, name, cfg):
    """models interleaved a, b, a, c, b; a 70-frame entry of b between 2-frame entries of a and c, so that b's columns cross a
    64-column tile and every model's first column is padded up to a multiple of 64 in every stage; an entry of a that only
    appends; a model d whose only entry only appends (no columns at all) and a model e that no entry names; non-final and
    FINAL entries.  A second call resumes the non-final ones at f0 > 0 in another interleaving."""
    la = lookahead_frames(cfg)
    N = cfg.L * _seg(cfg) * 2 * cfg.H
    nets = [_net(cfg, s) for s in (5, 6, 7, 8, 9)]                 # a, b, c, d, e
    a, b, c, d = 0, 1, 2, 3
    utts = [_Utt(cfg, 2, 500, a, N), _Utt(cfg, 70, 501, b, N), _Utt(cfg, 2, 502, a, N), _Utt(cfg, 2, 503, c, N),
            _Utt(cfg, 12, 504, b, N), _Utt(cfg, 9, 505, a, N), _Utt(cfg, 8, 506, d, N)]
    assert [u.model for u in utts[:5]] == [a, b, a, c, b]
    first = [utts[0].entry(2, 2, True), utts[1].entry(70, 70, True), utts[2].entry(2, 2, True), utts[3].entry(2, 2, True),
             utts[4].entry(12, 12 - la, False),                    # non-final: the last `la` frames wait for their context
             utts[5].entry(3, 0, False),                           # only appends: f1 == f0
             utts[6].entry(la, 0, False)]                          # model d: no columns at all
    assert first[5][2] == first[5][3] and first[6][2] == first[6][3]
    _call(nets, utts, first)
    for u in utts:
        _rows_ok(nets, u)
    assert utts[4].final == 12 - la and utts[5].final == 0 and utts[6].final == 0
    # second call: d, b, a in this order; b ends without new frames (f0 = 12 - la > 0), a appends and ends, d stays open
    again = [utts[6], utts[4], utts[5]]
    _call(nets, again, [utts[6].entry(8, 8 - la, False), utts[4].entry(12, 12, True), utts[5].entry(9, 9, True)])
    for u in utts:
        _rows_ok(nets, u)
    assert utts[4].final == 12 and utts[5].final == 9 and utts[6].final == 8 - la > 0
    # one model named by every entry of a *_models call: the rows of the single-model call
    solo = _Utt(cfg, 70, 501, 0, N)
    _call(nets[1:2], [solo], [solo.entry(70, 70, True)])
    assert torch.equal(solo.cond[:70], utts[1].cond[:70])


def test_rejected_models_call_changes_nothing(gpu_ok):
    cfg = C.bl6_laplace()
    nets = _three(cfg)
    N = cfg.L * 2 * cfg.H
    u = [_Utt(cfg, 6, 600 + i, i, N) for i in range(2)]
    ent = [x.entry(6, 6, True) for x in u]
    with pytest.raises(RuntimeError, match="names model 2"):
        _call(nets[:2], u, ent, model_of=[0, 2])
    with pytest.raises(RuntimeError, match="model 1 must be"):
        torch.ops.swn.frontend_pool_models([nets[0].packed, nets[1].packed[:-1]], [0, 1], [x.aux for x in u],
                                           [x.cond for x in u], torch.cat([e[0] for e in ent]), [6, 6], [6, 6], [0, 0], [6, 6],
                                           [True, True], nets[0].dlist)
    with pytest.raises(RuntimeError, match="17 models"):
        _call([nets[0]] * 17, u, ent, model_of=[0, 16])
    torch.cuda.synchronize()
    for x in u:
        assert bool((x.cond == SENTINEL).all()) and int(torch.count_nonzero(x.aux)) == 0


# ------------------------------------------------------------------------------------------------- more than 16 models
def test_seventeen_models_are_split_into_calls_of_sixteen(gpu_ok, counted):
    """20 sessions over 17 models in a pool of 24 slots: every tick's front end call and launch are cut at the 16-model cap,
    and every session still equals its solo decode"""
    cfg = C.tiny("laplace", 2, 4)
    nets = [_net(cfg, 5 + k) for k in range(17)]
    rng = np.random.default_rng(17)
    pool = DecodePool(nets[0], 24, variant=1, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    assert [pool.add_model(n) for n in nets[1:]] == list(range(1, 17))
    runs = [_Run(cfg, int(rng.integers(2, 4)), _seed_of(cfg, rng), 900 + i, 0, aux_seed=700 + i, model=i % 17) for i in range(20)]
    for r in runs:
        r.s = pool.open(seed=r.seed, utt_id=r.utt_id, model=r.model)
    pool.push_many({r.s: r.aux for r in runs}, finish=[r.s for r in runs])
    assert counted.names() == ["frontend_pool_models", "frontend_pool_models"]
    ticks = 0
    while not all(r.s.done for r in runs):
        before = len(counted.calls)
        res = pool.step(int(rng.integers(7, 40)))
        for r in runs:
            if r.s in res:
                r.collect(res[r.s])
        if len(res) == 20:
            # sessions 0 .. 15 (16 models) in the first launch; the 17th model and, behind it, models 0, 1, 2 in the second
            assert counted.names()[before:] == ["decode_pool_chunk_models", "decode_pool_chunk_models"]
            ticks += 1
    assert ticks >= 1
    for r in runs:
        _check(nets[r.model], r, 1)


# ------------------------------------------------------------------------------------------ slot reuse across models
@pytest.mark.parametrize("name,cfg,variant", [("bl6w", C.bl6_laplace(), 0), ("tiny_lap", C.tiny("laplace", 2, 4), 1),
                                              ("tiny_smx", C.tiny("softmax"), 1)], ids=["bl6w", "tiny_lap", "tiny_smx"])
def test_a_freed_slot_passes_to_another_model(gpu_ok, name, cfg, variant):
    """a model-0 session closed part-way frees its slot; a model-2 session BEGINs there in the same launch as resumed sessions
    of models 0 and 1 and equals its solo decode, the others are unaffected"""
    nets = _three(cfg)
    rng = np.random.default_rng(21)
    runs = [_Run(cfg, 4, _seed_of(cfg, rng), 10 + i, 0, aux_seed=200 + i, model=m) for i, m in enumerate((1, 0, 0))]
    late = _Run(cfg, 3, _seed_of(cfg, rng), 77, 0, aux_seed=299, model=2)
    pool = DecodePool(nets[0], 3, variant=variant, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    pool.add_model(nets[1]), pool.add_model(nets[2])
    for r in runs:
        r.s = pool.open(seed=r.seed, utt_id=r.utt_id, model=r.model)
        r.s.finish(r.aux.to(DEV))
    res = pool.step(runs[1].s.steps_ready // 2)
    for r in runs:
        r.collect(res[r.s])
    cut = runs[1]
    pool.close(cut.s)
    late.s = pool.open(seed=late.seed, utt_id=late.utt_id, model=late.model)
    assert late.s.slot == cut.s.slot and cut.model == 0 and late.s.model == 2
    late.s.finish(late.aux.to(DEV))
    live = [runs[0], runs[2], late]
    while live:
        res = pool.step(int(rng.integers(1, 90)))
        assert len(res) == len(live)
        for r in live:
            r.collect(res[r.s])
        live = [r for r in live if not r.s.done]
    for r in (runs[0], runs[2], late, cut):
        _check(nets[r.model], r, variant)
    assert 0 < cut.s.steps_done < cut.s.steps_ready


# ------------------------------------------------------------------------------------------------------- post-filter
ALPHA = 0.455
MEAN = np.concatenate([[0.9, 5.0, -3.0, -4.0, 0.1], 1.5 * np.exp(-0.15 * np.arange(50)) * np.cos(0.7 * np.arange(50))])


def test_post_filter_on_a_two_model_pool(gpu_ok):
    """the noise-shaping statistics are shared across speakers: the restored rows of a two-model pool are those of the same
    sessions run in two single-model pools"""
    cfg = C.bl6_laplace()
    nets = _three(cfg)[:2]
    models, frames = [0, 1, 1, 0], [3, 2, 4, 3]
    auxs = [torch.from_numpy(synth_aux(cfg, 1, f, seed=800 + i)).to(DEV) for i, f in enumerate(frames)]

    def run(pool, which, mixed):
        sess = {i: pool.open(utt_id=i, model=models[i] if mixed else 0) for i in which}
        for i, s in sess.items():
            s.finish(auxs[i])
        raw, rest = {i: [] for i in which}, {i: [] for i in which}
        while not all(s.done for s in sess.values()):
            res = pool.step(150)
            for i, s in sess.items():
                if s in res:
                    assert len(res[s]) == 3
                    raw[i].append(res[s][0]), rest[i].append(res[s][2])
        return {i: (torch.cat(raw[i], 1), torch.cat(rest[i], 1)) for i in which}

    mixed = DecodePool(nets[0], 4, rng_seed=RNG_SEED,
                       post_filter=NoiseShapingRestorer(MEAN, 22050, ALPHA, capacity=4, device=DEV))
    mixed.add_model(nets[1])
    got = run(mixed, range(4), True)
    for m in (0, 1):
        single = DecodePool(nets[m], 2, rng_seed=RNG_SEED,
                            post_filter=NoiseShapingRestorer(MEAN, 22050, ALPHA, capacity=2, device=DEV))
        want = run(single, [i for i in range(4) if models[i] == m], False)
        for i, (raw, rest) in want.items():
            assert torch.equal(got[i][0], raw) and torch.equal(got[i][1], rest), i
            assert rest.shape == raw.shape and float(rest.abs().max()) > 0
