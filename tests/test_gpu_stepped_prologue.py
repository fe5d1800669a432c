"""GPU: the parallel prologue of the stepped decode (swn_decode_stepped_prologue, prologue="parallel").  The oracle is the
stepped prologue of the same build: after the new call every float of every named slot's state block is the one a BEGIN
entry with it0 = 0, n_it = n_pro of the stepped pool call leaves, a slot no entry names keeps its bytes, and pools and streams
that fill their sessions this way return what HipNet.decode(variant=3) returns for each utterance alone."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, ops
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodeStream, SteppedDecodePool, SteppedModelPool
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RNG_SEED = 4242
PATTERN = 0x5A5A5A5A                           # what an untouched float of a session buffer holds in these tests

_NETS = {}


def _net(cfg, seed=5):
    key = (cfg, seed)
    if key not in _NETS:
        flavor = "trained" if cfg.kind == "laplace" else "xavier"
        _NETS[key] = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=seed, flavor=flavor), DEV)
    return _NETS[key]


def _seg(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


def _stride(net):
    return int(_lib.lib().swn_decode_session_floats(ctypes.byref(ops._desc(net.dlist)), 1, 3))


def _n_pro(net):
    return int(_lib.lib().swn_decode_stepped_prologue_iterations(ctypes.byref(ops._desc(net.dlist))))


def _patterned(floats):
    return torch.full((floats,), PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)


def _entries(cfg, E, capacity, seeded, rng):
    """E entries with distinct conditioning of 1 - 3 frames, slots not in table order, seed rows or None"""
    width = cfg.L * _seg(cfg) * 2 * cfg.H
    conds = [torch.from_numpy(rng.standard_normal((1 + e % 3, width)).astype(np.float32)).to(DEV) for e in range(E)]
    slots = [int(s) for s in rng.permutation(capacity)[:E]]
    if E > 1 and slots == sorted(slots):
        slots.reverse()
    seeds = None
    if seeded:
        if cfg.kind == "softmax":
            seeds = torch.from_numpy(rng.integers(0, cfg.n_quantize, (E,)).astype(np.int32))
        else:
            seeds = torch.from_numpy(rng.uniform(-0.9, 0.9, (E, cfg.seg)).astype(np.float32))
    return conds, slots, seeds


def _compare_slots(a, b, stride, slots, capacity):
    torch.cuda.synchronize()
    ai, bi = a.view(torch.int32), b.view(torch.int32)
    for s in range(capacity):
        blk_a, blk_b = ai[s * stride:(s + 1) * stride], bi[s * stride:(s + 1) * stride]
        if s in slots:
            assert not bool((blk_a == PATTERN).any()), s             # the oracle wrote the whole block
            assert torch.equal(blk_a, blk_b), (s, int((blk_a != blk_b).sum()))
        else:
            assert bool((blk_a == PATTERN).all()) and bool((blk_b == PATTERN).all()), s


STATE_NETS = [
    ("tiny_s1l0", C.tiny("laplace", 1, 0)),                          # rf 54, K Hp = 96: one partial piece, n_pro = 6 x 8 + 6
    ("tiny_s5l4", C.tiny("laplace", 5, 4)),                          # n_pro 50, the seg conditioning loop, a wider window
    ("tiny_smx_audioin", C.tiny("softmax", audio_in_flag=True)),     # the audio_in row of every layer
    ("tiny_h30", dataclasses.replace(C.tiny("laplace", 1, 0), hid_chn=30)),   # Hp = 32 != H, H no multiple of 8 pairs
    ("ref6_s1l4", C.ref6_laplace(1, 4)),                             # NI 6 with a 64-float last piece, n_pro = 86 x 8 + 2
    ("ref6_smx", C.ref6_softmax()),                                  # NI 7 exact
]


@pytest.mark.parametrize("E,seeded", [(1, False), (1, True), (9, False), (9, True)])
@pytest.mark.parametrize("name,cfg", STATE_NETS, ids=[n[0] for n in STATE_NETS])
def test_parallel_prologue_leaves_the_state_of_the_stepped_one(gpu_ok, name, cfg, E, seeded):
    net = _net(cfg)
    capacity = 12
    rng = np.random.default_rng(len(name) * 31 + E * 2 + seeded)
    conds, slots, seeds = _entries(cfg, E, capacity, seeded, rng)
    d = ops._desc(net.dlist)
    floats = ops.stepped_pool_session_floats(d, capacity)
    stride, n_pro = _stride(net), _n_pro(net)
    a, b = _patterned(floats), _patterned(floats)
    # (A) the stepped prologue: BEGIN entries that run the n_pro prologue iterations and no generation step
    torch.ops.swn.decode_pool_stepped_chunk(net.packed, a, conds, slots, [0] * E, [n_pro] * E, [True] * E, seeds,
                                            list(range(E)), net.dlist, capacity, RNG_SEED, False, False)
    # (B) the parallel prologue over the same entries
    torch.ops.swn.decode_stepped_prologue([net.packed], [], b, conds, slots, seeds, net.dlist, capacity)
    _compare_slots(a, b, stride, slots, capacity)


def test_parallel_prologue_over_several_models(gpu_ok):
    cfg = C.tiny("laplace", 2, 4)
    nets = [_net(cfg, seed=5 + k) for k in range(3)]
    capacity, E = 8, 5
    model_of = [0, 2, 1, 0, 2]
    rng = np.random.default_rng(77)
    conds, slots, seeds = _entries(cfg, E, capacity, True, rng)
    d = ops._desc(nets[0].dlist)
    floats = ops.stepped_pool_models_session_floats(d, capacity)
    stride, n_pro = _stride(nets[0]), _n_pro(nets[0])
    a, b = _patterned(floats), _patterned(floats)
    packed = [n.packed for n in nets]
    torch.ops.swn.decode_pool_stepped_chunk_models(packed, model_of, a, conds, slots, [0] * E, [n_pro] * E, [True] * E, seeds,
                                                   list(range(E)), nets[0].dlist, capacity, RNG_SEED, False, False)
    torch.ops.swn.decode_stepped_prologue(packed, model_of, b, conds, slots, seeds, nets[0].dlist, capacity)
    _compare_slots(a, b, stride, slots, capacity)
    # the models differ: entries 0 and 1 (models 0 and 2) would not agree on one model's weights
    c = _patterned(floats)
    torch.ops.swn.decode_stepped_prologue([packed[0]], [], c, conds, slots, seeds, nets[0].dlist, capacity)
    torch.cuda.synchronize()
    s0, s1 = slots[0], slots[1]
    assert torch.equal(c[s0 * stride:(s0 + 1) * stride].view(torch.int32), b[s0 * stride:(s0 + 1) * stride].view(torch.int32))
    assert not torch.equal(c[s1 * stride:(s1 + 1) * stride].view(torch.int32), b[s1 * stride:(s1 + 1) * stride].view(torch.int32))


# ---------------------------------------------------------------------------------------------------- end to end: pools
def _seed_of(cfg, rng):
    if rng.random() < 0.3:
        return None
    if cfg.kind == "softmax":
        return torch.tensor([int(rng.integers(0, cfg.n_quantize))], dtype=torch.int32)
    return torch.from_numpy(rng.uniform(-0.9, 0.9, (1, cfg.seg)).astype(np.float32))


class _Run:
    def __init__(self, cfg, F, seed, utt_id, start, aux_seed, model=0):
        self.aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=aux_seed))
        self.F, self.seed, self.utt_id, self.start, self.model = F, seed, utt_id, start, model
        self.pushed, self.s = 0, None
        self.out, self.heads, self.noise = [], [], []

    def collect(self, r):
        self.out.append(r[0]), self.heads.append(r[1]), self.noise.append(r[2])


def _check(net, r):
    n = r.s.steps_done
    ref_out, ref_heads, ref_used = net.decode(r.aux.to(DEV), n, want_heads=True, variant=3, rng_seed=RNG_SEED,
                                              want_noise=True, seed=None if r.seed is None else r.seed.to(DEV),
                                              utt_ids=[r.utt_id])
    out, heads, used = torch.cat(r.out, 1), torch.cat(r.heads, 1), torch.cat(r.noise, 1)
    assert out.shape[1] == n * _seg(net.cfg)
    assert torch.equal(out, ref_out), (net.cfg, r.utt_id)
    assert torch.equal(heads, ref_heads), (net.cfg, r.utt_id)
    assert torch.equal(used, ref_used), (net.cfg, r.utt_id)


def _drive(pool, runs, rng, several=False):
    """tick until every session is done: admit at its start tick, push 1-3 frames per tick (then finish), a random step
    budget"""
    tick, live = 0, []
    while any(r.s is None for r in runs) or live:
        for r in runs:
            if r.s is None and r.start <= tick:
                kw = dict(model=r.model) if several else {}
                r.s = pool.open(seed=r.seed, utt_id=r.utt_id, **kw)
                live.append(r)
        for r in live:
            if not r.s.finished:
                piece = r.aux[:, :, r.pushed:r.pushed + int(rng.integers(1, 4))]
                r.pushed += piece.shape[2]
                (r.s.finish if r.pushed >= r.F else r.s.push)(piece.to(DEV))
        steps = [None, 1, 7, 64, 150][int(rng.integers(0, 5))]
        began = [r for r in live if r.s._it_done == 0 and r.s.steps_ready > 0]
        res = pool.step(steps, max_prologue=[None, 100][int(rng.integers(0, 2))])
        assert all(r.s in res for r in began)                        # a session generates in the tick it begins in
        for r in live:
            if r.s in res:
                r.collect(res[r.s])
        for r in [r for r in live if r.s.done]:
            pool.close(r.s)
            live.remove(r)
        tick += 1
        assert tick < 2000


POOL_NETS = [("ref6_s1l4", C.ref6_laplace(1, 4)), ("tiny_s5l4", C.tiny("laplace", 5, 4))]


@pytest.mark.parametrize("n_sess", [5, 27])
@pytest.mark.parametrize("name,cfg", POOL_NETS, ids=[n[0] for n in POOL_NETS])
def test_parallel_pool_sessions_equal_solo_decodes(gpu_ok, name, cfg, n_sess):
    """5 sessions: the per-entry kernels generate; 27: the tile kernels while 24 or more are active"""
    net = _net(cfg)
    rng = np.random.default_rng(len(name) + n_sess)
    runs = [_Run(cfg, int(rng.integers(2, 5)), _seed_of(cfg, rng), int(rng.integers(0, 100000)),
                 0 if n_sess > 8 and i < 26 else int(rng.integers(0, 4)), aux_seed=100 + i) for i in range(n_sess)]
    pool = SteppedDecodePool(net, 32, rng_seed=RNG_SEED, want_heads=True, want_noise=True, prologue="parallel")
    _drive(pool, runs, rng)
    for r in runs:
        assert r.s.steps_done == r.F * cfg.U // _seg(cfg)
        _check(net, r)


@pytest.mark.parametrize("name,cfg", POOL_NETS, ids=[n[0] for n in POOL_NETS])
def test_parallel_model_pool_sessions_equal_solo_decodes(gpu_ok, name, cfg):
    nets = [_net(cfg, seed=5 + k) for k in range(3)]
    rng = np.random.default_rng(len(name) + 3)
    runs = [_Run(cfg, int(rng.integers(2, 4)), _seed_of(cfg, rng), int(rng.integers(0, 100000)), int(rng.integers(0, 3)),
                 aux_seed=300 + i, model=(2 * i + 1) % 3) for i in range(7)]
    pool = SteppedModelPool(nets[0], 8, rng_seed=RNG_SEED, want_heads=True, want_noise=True, prologue="parallel")
    for n in nets[1:]:
        pool.add_model(n)
    _drive(pool, runs, rng, several=True)
    for r in runs:
        assert r.s.steps_done == r.F * cfg.U // _seg(cfg)
        _check(nets[r.model], r)


# -------------------------------------------------------------------------------------------------- end to end: streams
STREAM_NETS = [("ref6_s1l4", C.ref6_laplace(1, 4)), ("tiny_smx_audioin", C.tiny("softmax", audio_in_flag=True))]


@pytest.mark.parametrize("name,cfg", STREAM_NETS, ids=[n[0] for n in STREAM_NETS])
def test_parallel_stream_chunks_equal_the_stepped_stream(gpu_ok, name, cfg):
    net = _net(cfg)
    B, F = 3, 4
    rng = np.random.default_rng(9)
    aux = torch.from_numpy(synth_aux(cfg, B, F, seed=12)).to(DEV)
    if cfg.kind == "softmax":
        seed = torch.from_numpy(rng.integers(0, cfg.n_quantize, (B,)).astype(np.int32))
    else:
        seed = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, cfg.seg)).astype(np.float32))
    kw = dict(variant=3, seed=seed, rng_seed=RNG_SEED, utt_ids=[7, 3, 11], want_heads=True, want_noise=True)
    ref, par = DecodeStream(net, B, **kw), DecodeStream(net, B, prologue="parallel", **kw)
    total = 0
    for f0, f1 in ((0, 1), (1, 3), (3, 4)):
        got = [(s.finish if f1 == F else s.push)(aux[:, :, f0:f1]) for s in (ref, par)]
        assert got[0][0].shape == got[1][0].shape
        total += got[0][0].shape[1]
        for x, y in zip(*got):
            assert torch.equal(x, y), (name, f0)
    assert total == F * cfg.U and par.steps_done == ref.steps_done == F * cfg.U // _seg(cfg)
    torch.cuda.synchronize()
    n = int(_lib.lib().swn_decode_session_floats(ctypes.byref(ops._desc(net.dlist)), B, 3))
    assert torch.equal(ref._session[:n].view(torch.int32), par._session[:n].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ late begin
def test_a_late_parallel_begin_leaves_the_generating_sessions_alone(gpu_ok):
    cfg = C.ref6_laplace(1, 4)
    net = _net(cfg)

    def run(with_late):
        pool = SteppedDecodePool(net, 4, rng_seed=RNG_SEED, want_heads=True, want_noise=True, prologue="parallel")
        runs = [_Run(cfg, 3, None if i else torch.tensor([[0.5]]), 10 + i, 0, aux_seed=200 + i) for i in range(2)]
        for r in runs:
            r.s = pool.open(seed=r.seed, utt_id=r.utt_id)
            r.s.finish(r.aux.to(DEV))
        late = _Run(cfg, 2, torch.tensor([[-0.25]]), 77, 0, aux_seed=299)
        for tick in range(40):
            if tick == 2 and with_late:
                late.s = pool.open(seed=late.seed, utt_id=late.utt_id)
                late.s.finish(late.aux.to(DEV))
            res = pool.step(60)
            if tick == 2 and with_late:
                assert late.s in res and all(r.s in res for r in runs)   # mid-generation neighbours, same tick
            for r in runs + ([late] if late.s is not None else []):
                if r.s in res:
                    r.collect(res[r.s])
            if all(r.s.done for r in runs) and (late.s is None or late.s.done):
                break
        return runs, late

    alone, _ = run(False)
    mixed, late = run(True)
    for x, y in zip(alone, mixed):
        assert x.s.steps_done == y.s.steps_done == 3 * cfg.U
        for p, q in ((x.out, y.out), (x.heads, y.heads), (x.noise, y.noise)):
            assert torch.equal(torch.cat(p, 1), torch.cat(q, 1))
    assert late.s.steps_done == 2 * cfg.U
    _check(net, late)
    _check(net, mixed[0])
