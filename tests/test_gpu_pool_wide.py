"""GPU: the wide decode pool launch (swn_decode_pool_chunk_wide, DecodePool(launch_width=256)): up to 256 sessions per launch,
the entry table in device memory.  Every session's out, heads and noise are bit-identical to those of a pool that runs the
64-entry launches (launch_width=64, same key and utterance ids) and to its solo DecodeStream - on the generic kernel, the
wave-specialised and the symmetric BL6 kernels, fp32 / bf16 / E4M3 head weights, one model and three.  The direct calls check
that rows past an entry's own steps stay unwritten and that a refused call writes nothing.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import streaming
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodeModelPool, DecodePool, DecodeStream
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RNG_SEED = 777
BADARG = -2
_NETS = {}


def _net(cfg, seed):
    """the model of synth_state_dict(cfg, seed), built once (as tests/test_gpu_pool_models.py builds its nets)"""
    if (cfg, seed) not in _NETS:
        flavor = "trained" if cfg.kind == "laplace" else "xavier"
        _NETS[(cfg, seed)] = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=seed, flavor=flavor), DEV)
    return _NETS[(cfg, seed)]


def _seg(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


def _seed_of(cfg, rng):
    if rng.random() < 0.3:
        return None
    if cfg.kind == "softmax":
        return torch.tensor([int(rng.integers(0, cfg.n_quantize))], dtype=torch.int32)
    return torch.from_numpy(rng.uniform(-0.9, 0.9, (1, cfg.seg)).astype(np.float32))


class _Counting:
    """torch.ops.swn with every decode launch noted: (op name, entries)"""

    def __init__(self):
        self.real, self.calls = torch.ops.swn, []

    def __getattr__(self, name):
        op = getattr(self.real, name)

        def call(*a, **k):
            if name.startswith("decode_pool_chunk"):
                self.calls.append((name, len(next(x for x in a if isinstance(x, list) and x and isinstance(x[0], bool)))))
            return op(*a, **k)
        return call


class _Plan:
    """one session of the schedule: F frames, a seed, an id, a model, the tick it is opened in, whether it is closed after tick
    0, and its step quota in each of the three ticks"""

    def __init__(self, cfg, i, rng, n_models, late):
        self.F = int(rng.integers(2, 5))
        self.aux = torch.from_numpy(synth_aux(cfg, 1, self.F, seed=300 + i))
        self.seed, self.utt_id, self.model = _seed_of(cfg, rng), 1000 + 3 * i, int(rng.integers(0, n_models))
        self.late = late
        per_frame = cfg.U // _seg(cfg)
        total = self.F * per_frame
        # ragged: nothing, one step, up to two frames' worth.  Tick 0 leaves at least one step and tick 1 runs at least one, so
        # the launch of tick 1 holds every open session - resumed ones and those that begin there
        q = lambda lo: int(rng.choice([lo, 1, int(rng.integers(lo, 2 * per_frame + 1)), 2 * per_frame]))
        self.quota = [0 if late else min(q(0), total - 1), max(1, q(1)), q(0)]
        self.close_early = (not late) and rng.random() < 0.1


def _schedule(cfg, E, n_models):
    rng = np.random.default_rng(E + 7 * n_models + cfg.U)
    n_late = max(1, E // 8)
    plans = [_Plan(cfg, i, rng, n_models, late=i >= E - n_late) for i in range(E)]
    # every session that is closed after tick 0 makes room for one more late one
    n_early = sum(p.close_early for p in plans)
    plans += [_Plan(cfg, E + j, rng, n_models, late=True) for j in range(n_early)]
    return plans


def _run_pool(monkeypatch, nets, variant, weights, E, width, plans):
    """the schedule through a pool of capacity E and `launch_width` width -> (per plan: (out, heads, noise, steps_done), the
    decode launches as (op, entries), the sessions in entry order at tick 1 as plan indices)"""
    cfg = nets[0].cfg
    counted = _Counting()
    monkeypatch.setattr(streaming, "_O", counted)
    quota = {}
    real_plan = streaming.plan_tick.__wrapped__ if hasattr(streaming.plan_tick, "__wrapped__") else streaming.plan_tick

    def plan_tick(sessions, max_steps=None, limit=_lib.DECODE_POOL_MAX_ENTRIES):
        return real_plan([(s, min(ready, done + quota[s]), done) for s, ready, done in sessions], max_steps, limit)
    plan_tick.__wrapped__ = real_plan
    monkeypatch.setattr(streaming, "plan_tick", plan_tick)

    cls = DecodeModelPool if len(nets) > 1 and weights != "fp32" else DecodePool
    pool = cls(nets[0], E, variant=variant, rng_seed=RNG_SEED, want_heads=True, want_noise=True, weights=weights,
               launch_width=width)
    for n in nets[1:]:
        pool.add_model(n)
    pool._free = [(37 * e) % E for e in range(E)]        # slots permuted against the admission (= entry) order
    pieces = {i: [] for i in range(len(plans))}
    sess, order = {}, None

    def admit(idx):
        chunks = {}
        for i in idx:
            p = plans[i]
            sess[i] = pool.open(seed=p.seed, utt_id=p.utt_id, model=p.model)
            chunks[sess[i]] = p.aux
        pool.push_many(chunks, finish=list(chunks))

    for tick in range(3):
        if tick == 0:
            admit([i for i, p in enumerate(plans) if not p.late])
        if tick == 1:
            for i, p in enumerate(plans):
                if p.close_early:
                    pool.close(sess[i])
            admit([i for i, p in enumerate(plans) if p.late])
            assert len(pool.sessions) == E
            back = {s: i for i, s in sess.items()}
            order = [back[s] for s in pool.sessions]
        quota.clear()
        quota.update({sess[i]: plans[i].quota[tick] for i in sess if not sess[i].closed})
        res = pool.step()
        for i, s in sess.items():
            if s in res:
                pieces[i].append(res[s])
    done = {}
    for i, p in enumerate(plans):
        if pieces[i]:
            done[i] = tuple(torch.cat([r[k] for r in pieces[i]], 1) for k in range(3)) + (sess[i].steps_done,)
        else:
            done[i] = (None, None, None, 0)
    slots = [sess[i].slot for i in order]
    assert slots != sorted(slots)
    return done, counted.calls, order


# name, cfg, variant, weights, models
CASES = [
    ("tiny_generic", C.tiny("laplace", 2, 4), 1, "fp32", 1),
    ("bl6w", C.bl6_laplace(1, 0), 0, "fp32", 1),
    ("bl6_s5l4", C.bl6_laplace(5, 4), 0, "fp32", 1),
    ("smx_fp32", C.bl6_softmax(), 0, "fp32", 1),
    ("smx_bf16", C.bl6_softmax(), 0, "bf16", 1),
    ("smx_e4m3", C.bl6_softmax(), 0, "e4m3", 1),
    ("smx_m3_fp32", C.bl6_softmax(), 0, "fp32", 3),
    ("smx_m3_bf16", C.bl6_softmax(), 0, "bf16", 3),
]


@pytest.mark.parametrize("E", [65, 256])
@pytest.mark.parametrize("name,cfg,variant,weights,n_models", CASES, ids=[c[0] for c in CASES])
def test_wide_tick_equals_the_narrow_tick_and_the_solo_streams(gpu_ok, monkeypatch, name, cfg, variant, weights, n_models, E):
    nets = [_net(cfg, 5 + m) for m in range(n_models)]
    plans = _schedule(cfg, E, n_models)
    if n_models > 1:
        assert {p.model for p in plans} == set(range(n_models))
    wide, wide_calls, order = _run_pool(monkeypatch, nets, variant, weights, E, 256, plans)
    narrow, narrow_calls, order64 = _run_pool(monkeypatch, nets, variant, weights, E, 64, plans)
    assert order == order64
    # the wide pool made wide launches only, one per tick, and tick 1 held all E sessions - beginning and resumed ones;
    # the narrow pool made today's launches of at most 64
    assert {c[0] for c in wide_calls} == {"decode_pool_chunk_wide"} and len(wide_calls) == 3
    assert wide_calls[1][1] == E
    assert "decode_pool_chunk_wide" not in {c[0] for c in narrow_calls} and max(c[1] for c in narrow_calls) <= 64
    assert any(p.quota[0] == 0 and not p.late for p in plans) and any(p.close_early for p in plans)
    ran = 0
    for i in range(len(plans)):
        w, n = wide[i], narrow[i]
        assert w[3] == n[3], (name, E, i)
        if w[0] is None:
            assert n[0] is None
            continue
        ran += 1
        for k, what in enumerate(("out", "heads", "noise")):
            assert torch.equal(w[k], n[k]), (name, E, i, what)
    assert ran >= E
    # the sessions at the edges of the 64-entry groups of tick 1's launch against their solo streams
    for e in sorted({0, 63, 64, 65, E - 1}):
        if e >= E:
            continue
        i = order[e]
        p = plans[i]
        st = DecodeStream(nets[p.model], 1, variant=variant, seed=p.seed, rng_seed=RNG_SEED, utt_ids=[p.utt_id],
                          want_heads=True, want_noise=True, weights=weights)
        ref = st.finish(p.aux.to(DEV))
        out, heads, noise, n = wide[i]
        assert n > 0
        assert torch.equal(out, ref[0][:, :n * _seg(cfg)]), (name, E, e)
        assert torch.equal(heads, ref[1][:, :n]) and torch.equal(noise, ref[2][:, :n]), (name, E, e)


# ------------------------------------------------------------------------------------------------- the call itself
SENT = 12345.5


def _io(seeds, used, ids):
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return _lib.DecodeIO(noise_dev=None, forced_dev=None, seed_dev=p(seeds), noise_out_dev=p(used), rng_seed=RNG_SEED,
                         rng_utt0=0, reserved=0, rng_utt_ids_dev=p(ids))


class _Direct:
    """the buffers of direct pool calls over E sessions of `net`, full of a sentinel"""

    def __init__(self, net, E, variant, n_max, cap):
        cfg = net.cfg
        soft = cfg.kind == "softmax"
        self.seg, self.width = _seg(cfg), cfg.n_quantize if soft else cfg.seg
        floats = _lib.lib().swn_decode_session_floats(ctypes.byref(net.desc), cap, variant)
        full = lambda *shape: torch.full(shape, SENT, dtype=torch.float32, device=DEV)
        self.session = full(floats)
        self.out = torch.full((E, n_max * self.seg), 77777, dtype=torch.int32, device=DEV) if soft else full(E, n_max * self.seg)
        self.heads, self.used = full(E, n_max, cfg.n_out), full(E, n_max, self.width)
        self.ids = torch.arange(50, 50 + E, dtype=torch.int32, device=DEV)

    def tensors(self):
        return self.session, self.out, self.heads, self.used


DIRECT = [("tiny_generic", C.tiny("laplace", 2, 4), 1, "fp32"), ("bl6w", C.bl6_laplace(1, 0), 0, "fp32"),
          ("smx_bf16", C.bl6_softmax(), 0, "bf16")]


@pytest.mark.parametrize("E", [1, 64])
@pytest.mark.parametrize("name,cfg,variant,weights", DIRECT, ids=[c[0] for c in DIRECT])
def test_direct_wide_call_writes_what_the_narrow_call_writes_and_nothing_else(gpu_ok, name, cfg, variant, weights, E):
    """two calls (BEGIN, then resumed) of ragged step counts through swn_decode_pool_chunk_wide and through the 64-entry call on
    buffers full of a sentinel: session, out, heads and noise are equal byte for byte, rows past an entry's own steps still hold
    the sentinel, and a refused call (one slot in two entries) leaves everything as it was"""
    L = _lib.lib()
    net = _net(cfg, 5)
    d = ctypes.byref(net.desc)
    Tf, cap = 2, 70
    per_frame = cfg.U // _seg(cfg)
    rng = np.random.default_rng(E)
    cond = net.frontend(torch.from_numpy(synth_aux(cfg, E, Tf, seed=9)).to(DEV)).contiguous()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    first = [int(rng.integers(0, per_frame + 1)) for _ in range(E)]
    second = [int(rng.integers(0, per_frame + 1)) for _ in range(E)]
    first[0] = 0                                                         # (E = 64: entry 0 runs its prologue alone)
    # the rows of a call are n_max = max(n_steps) of THAT call apart: the last entry runs a whole frame in both calls, so both
    # share one layout and one set of buffers
    first[E - 1] = second[E - 1] = n_max = per_frame
    slots = [(37 * e + 3) % cap for e in range(E)]
    image = None
    if weights != "fp32":
        image = net.decode_w16_image()
    models = (ctypes.c_void_p * 1)(net.packed.data_ptr())
    images = None if image is None else (ctypes.c_void_p * 1)(image.data_ptr())
    fmt = {"fp32": _lib.WEIGHTS_FP32, "bf16": _lib.WEIGHTS_BF16}[weights]
    of = (ctypes.c_int32 * E)(*([0] * E))
    table = torch.empty(L.swn_decode_pool_wide_table_bytes(E), dtype=torch.uint8, device=DEV)
    w, n = _Direct(net, E, variant, n_max, cap), _Direct(net, E, variant, n_max, cap)

    def entries(steps, step0s, begin):
        return (_lib.DecodePoolEntry * E)(*[
            _lib.DecodePoolEntry(cond_dev=cond[e].data_ptr(), n_frames=Tf, slot=slots[e], step0=step0s[e], n_steps=steps[e],
                                 flags=_lib.CHUNK_BEGIN if begin else 0, reserved=0) for e in range(E)])

    def wide_call(tab, b):
        return L.swn_decode_pool_chunk_wide(d, models, 1, of, cap, tab, E, ctypes.byref(_io(None, b.used, b.ids)), p(b.session),
                                            p(b.out), p(b.heads), variant, images, fmt, p(table), st)

    def narrow_call(tab, b):
        args = (d, p(net.packed), cap, tab, E, ctypes.byref(_io(None, b.used, b.ids)), p(b.session), p(b.out), p(b.heads), variant)
        if image is None:
            return L.swn_decode_pool_chunk(*args, st)
        return L.swn_decode_pool_chunk_w16(*args, p(image), st)

    if E > 1:                                                            # refused before anything is launched
        bad = entries(first, [0] * E, True)
        bad[E - 1].slot = bad[1].slot
        assert wide_call(bad, w) == BADARG
        torch.cuda.synchronize()
        for t in w.tensors():
            assert bool((t == (77777 if t.dtype == torch.int32 else SENT)).all())
    for steps, step0s, begin in ((first, [0] * E, True), (second, first, False)):
        tab = entries(steps, step0s, begin)
        assert wide_call(tab, w) == 0 and narrow_call(tab, n) == 0
        torch.cuda.synchronize()
        for a, b, what in zip(w.tensors(), n.tensors(), ("session", "out", "heads", "noise")):
            assert torch.equal(a, b), (name, E, what, begin)
        for e in range(E):
            top = steps[e] if begin else max(first[e], second[e])        # (the second call reuses the first one's buffers)
            assert bool((w.heads[e, top:] == SENT).all()) and bool((w.used[e, top:] == SENT).all()), (name, e)
            assert bool((w.out[e, top * w.seg:] == (77777 if w.out.dtype == torch.int32 else SENT)).all()), (name, e)
            if steps[e] > 0:
                assert not bool((w.heads[e, :steps[e]] == SENT).any())
        used_slots = set(slots)
        per_slot = w.session.numel() // cap
        for s in range(cap if variant != 1 else 0):                       # (the BL6 sessions lie slot by slot)
            if s not in used_slots:
                assert bool((w.session[s * per_slot:(s + 1) * per_slot] == SENT).all()), (name, s)


@pytest.mark.parametrize("E", [1, 64])
def test_wide_op_called_directly_equals_the_narrow_op(gpu_ok, E):
    cfg = C.bl6_softmax()
    net = _net(cfg, 5)
    Tf = 2
    cond = net.frontend(torch.from_numpy(synth_aux(cfg, E, Tf, seed=11)).to(DEV)).contiguous()
    rng = np.random.default_rng(100 + E)
    steps = [int(rng.integers(0, cfg.U + 1)) for _ in range(E)]
    steps[E - 1] = cfg.U
    floats = _lib.lib().swn_decode_session_floats(ctypes.byref(net.desc), E, 0)
    sw, sn = torch.zeros(floats, device=DEV), torch.zeros(floats, device=DEV)
    args = ([cond[e] for e in range(E)], [(37 * e) % E for e in range(E)], [0] * E, steps, [True] * E, None,
            list(range(200, 200 + E)), net.dlist, E, 0, RNG_SEED, True, True)
    ow, hw, uw = torch.ops.swn.decode_pool_chunk_wide([net.packed], [], "fp32", [0] * E, sw, *args)
    on, hn, un = torch.ops.swn.decode_pool_chunk(net.packed, sn, *args)
    assert torch.equal(sw, sn)
    for e in range(E):
        k = steps[e]
        assert torch.equal(ow[e, :k], on[e, :k]) and torch.equal(hw[e, :k], hn[e, :k]) and torch.equal(uw[e, :k], un[e, :k])
