"""GPU: the pool front end (swn_frontend_pool / torch.ops.swn.frontend_pool / DecodePool.push_many).  One call finalises the
conditioning of many sessions, each at its own frame position; every cond row it writes is bit-identical to the one-shot
front end over the whole utterance, and a pool fed through push_many is, tick by tick, the pool fed through the separate
PoolSession.push / finish calls.  All comparisons are exact."""
import json

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import decode_driver as DD
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodePool, SteppedDecodePool, lookahead_frames
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RNG_SEED = 4242
_NETS = {}


def _net(name, cfg):
    if name not in _NETS:
        flavor = "trained" if cfg.kind == "laplace" else "xavier"
        _NETS[name] = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=5, flavor=flavor), DEV)
    return _NETS[name]


def _seg(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


# ------------------------------------------------------------------------------------------------------------ op level
class _Utt:
    """one utterance driven through frontend_pool: its features, its session buffers and where it stands"""

    def __init__(self, cfg, F, seed, N, rng, one_piece=False, pieces=(0, 8)):
        self.full = torch.from_numpy(synth_aux(cfg, 1, F, seed=seed)).to(DEV)
        self.F, self.one_piece, self.pieces = F, one_piece, pieces
        self.aux = torch.zeros((cfg.n_aux, F + int(rng.integers(0, 9))), dtype=torch.float32, device=DEV)
        self.cond = torch.zeros((F + int(rng.integers(0, 3)), N), dtype=torch.float32, device=DEV)
        self.received = self.final = 0
        self.ended = False

    def next_entry(self, rng, la):
        """(piece, n_received, f0, f1, final) of this utterance's next call: 0 to 7 new frames (pieces[0] to pieces[1] - 1);
        the features end with the last piece or, as often, with an empty call after it"""
        k = self.F if self.one_piece else int(rng.integers(*self.pieces))
        a, b = self.received, min(self.F, self.received + k)
        fin = b == self.F and (a == b or self.one_piece or rng.random() < 0.5)
        f1 = b if fin else max(0, b - la)
        return self.full[0, :, a:b].contiguous().reshape(-1), b, self.final, max(self.final, f1), fin


def _drive_op(net, utts, rng, la, name):
    """every utterance an entry at its own position of every frontend_pool call (64 entries per call) until it has ended; then
    every cond row against the one-shot front end over the whole utterance"""
    dirty = torch.zeros((), dtype=torch.int64, device=DEV)
    calls = 0
    while any(not u.ended for u in utts):
        live = [u for u in utts if not u.ended]
        for at in range(0, len(live), 64):
            part = live[at:at + 64]
            ent = [u.next_entry(rng, la) for u in part]
            pieces = [e[0] for e in ent if e[0].numel()]
            torch.ops.swn.frontend_pool(net.packed, [u.aux for u in part], [u.cond for u in part],
                                        torch.cat(pieces) if pieces else None,
                                        [e[1] - u.received for u, e in zip(part, ent)], [e[1] for e in ent],
                                        [e[2] for e in ent], [e[3] for e in ent], [e[4] for e in ent], net.dlist)
            calls += 1
            for u, e in zip(part, ent):
                u.received, u.final, u.ended = e[1], e[3], e[4]
                dirty += torch.count_nonzero(u.cond[u.final:])          # rows past f1 are still zeros after every call
    assert calls > 1
    assert int(dirty) == 0
    for i, u in enumerate(utts):
        want = torch.ops.swn.frontend(net.packed, u.full, net.dlist)[0][0]
        assert u.final == u.F and torch.equal(u.cond[:u.F], want), (name, i, u.F)
        assert torch.equal(u.aux[:, :u.F], u.full[0]), (name, i)
        assert int(torch.count_nonzero(u.aux[:, u.F:])) == 0
    return calls


OP_NETS = [("tiny_lap", C.tiny("laplace", 2, 4)), ("bl6_lap", C.bl6_laplace()), ("bl6_s5l4", C.bl6_laplace(5, 4)),
           ("bl6_smx", C.bl6_softmax()), ("ref6_lap", C.ref6_laplace()), ("ref6_smx", C.ref6_softmax())]


@pytest.mark.parametrize("n_utt", [1, 7, 64])
@pytest.mark.parametrize("name,cfg", OP_NETS, ids=[n[0] for n in OP_NETS])
def test_op_rows_equal_the_one_shot_front_end(gpu_ok, name, cfg, n_utt):
    """n_utt utterances of 5 to 40 frames, one of 600 frames in pushes of 0 to 7 and one of 600 frames in one piece, every one
    an entry at its own position of every call until it has ended"""
    net = _net(name, cfg)
    rng = np.random.default_rng(1000 + n_utt + len(name))
    la = lookahead_frames(cfg)
    N = cfg.L * _seg(cfg) * 2 * cfg.H
    utts = [_Utt(cfg, int(rng.integers(5, 41)), 300 + i, N, rng) for i in range(n_utt)]
    utts += [_Utt(cfg, 600, 298, N, rng), _Utt(cfg, 600, 299, N, rng, one_piece=True)]
    _drive_op(net, utts, rng, la, name)


def test_rejected_op_call_changes_nothing(gpu_ok):
    cfg = C.bl6_laplace()
    net = _net("bl6_lap", cfg)
    N = cfg.L * 2 * cfg.H
    aux = [torch.zeros((cfg.n_aux, 16), device=DEV) for _ in range(2)]
    cond = torch.zeros((8, N), device=DEV)
    new = torch.ones(cfg.n_aux * 12 * 2, device=DEV)
    with pytest.raises(RuntimeError):                                      # one cond buffer in two entries
        torch.ops.swn.frontend_pool(net.packed, aux, [cond, cond], new, [12, 12], [12, 12], [0, 0], [8, 8], [False, False],
                                    net.dlist)
    with pytest.raises(RuntimeError):                                      # past the frames whose context has arrived
        torch.ops.swn.frontend_pool(net.packed, aux[:1], [cond], new[:cfg.n_aux * 12], [12], [12], [0], [9], [False], net.dlist)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(cond)) == 0 and all(int(torch.count_nonzero(a)) == 0 for a in aux)


# ---------------------------------------------------------------------------------------------------------- pool level
def _seed_of(cfg, rng):
    if rng.random() < 0.3:
        return None
    if cfg.kind == "softmax":
        return torch.tensor([int(rng.integers(0, cfg.n_quantize))], dtype=torch.int32)
    return torch.from_numpy(rng.uniform(-0.9, 0.9, (1, cfg.seg)).astype(np.float32))


class _Run:
    """one utterance in both pools: a = fed by PoolSession.push / finish, b = fed by push_many"""

    def __init__(self, cfg, F, seed, utt_id, start, aux_seed):
        self.aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=aux_seed))
        self.F, self.seed, self.utt_id, self.start = F, seed, utt_id, start
        self.pushed, self.a, self.b = 0, None, None
        self.out, self.heads, self.noise = [], [], []


def _budget(rng):
    return [None, 1, 2, 3, 63, 64, 65, 127, int(rng.integers(1, 200))][int(rng.integers(0, 9))]


def _same_cond(x, y):
    return (x is None and y is None) or (x is not None and y is not None and torch.equal(x, y))


def _drive_pair(pa, pb, runs, rng, capacity, cut_tick, stepped):
    """the two pools through one schedule: staggered admission as slots free up (a run with start < 0 is admitted when a
    session is closed part-way, into its slot), 0 to 7 frames per tick and session (host and device chunks mixed for
    push_many; the features end with the last chunk or with an empty finish one tick later), random step budgets, one
    session closed part-way.  After every tick the two pools must stand exactly alike."""
    tick, live, most, cut, reused = 0, [], 0, None, False
    while any(r.a is None for r in runs) or live:
        for r in runs:
            if r.a is None and 0 <= r.start <= tick and len(live) < capacity:
                r.a, r.b = pa.open(seed=r.seed, utt_id=r.utt_id), pb.open(seed=r.seed, utt_id=r.utt_id)
                assert r.a.slot == r.b.slot
                live.append(r)
        most = max(most, len(live))
        chunks, finish = {}, []
        for r in live:
            if r.a.finished:
                continue
            if r.pushed >= r.F:                                    # all features pushed last tick: an empty finish
                r.a.finish()
                finish.append(r.b)
                continue
            piece = r.aux[:, :, r.pushed:r.pushed + int(rng.integers(0, 8))]
            r.pushed += piece.shape[2]
            ends = r.pushed >= r.F and rng.random() < 0.6
            (r.a.finish if ends else r.a.push)(piece.to(DEV))
            chunks[r.b] = piece.to(DEV) if rng.random() < 0.5 else piece
            if ends:
                finish.append(r.b)
        pb.push_many(chunks, finish=finish)
        for r in live:
            sa, sb = r.a._stream, r.b._stream
            assert (sa.frames_received, sa.frames_final, r.a.steps_ready, r.a.finished) == \
                   (sb.frames_received, sb.frames_final, r.b.steps_ready, r.b.finished), (tick, r.utt_id)
            assert _same_cond(sa.cond, sb.cond), (tick, r.utt_id)
        budget = [1, 2, 3, 50][int(rng.integers(0, 4))] if cut is None else _budget(rng)    # nobody is done before the cut
        kw = dict(max_prologue=[None, None, 100, 300][int(rng.integers(0, 4))]) if stepped else {}
        ra, rb = pa.step(budget, **kw), pb.step(budget, **kw)
        for r in live:
            assert (r.a in ra) == (r.b in rb) and r.a.steps_done == r.b.steps_done, (tick, r.utt_id)
            if r.b in rb:
                for x, y in zip(ra[r.a], rb[r.b]):
                    assert torch.equal(x, y), (tick, r.utt_id)
                r.out.append(rb[r.b][0]), r.heads.append(rb[r.b][1]), r.noise.append(rb[r.b][2])
        part_way = [r for r in live if not r.b.done and r.b.steps_done > 0]
        if cut is None and tick >= cut_tick and part_way:
            cut = part_way[0]                                      # closed part-way: its slot goes to the next session
            pa.close(cut.a), pb.close(cut.b)
            live.remove(cut)
            for r in [r for r in runs if r.start < 0]:
                r.a, r.b = pa.open(seed=r.seed, utt_id=r.utt_id), pb.open(seed=r.seed, utt_id=r.utt_id)
                assert r.a.slot == r.b.slot
                reused = reused or r.b.slot == cut.b.slot
                live.append(r)
        for r in [r for r in live if r.b.done]:
            pa.close(r.a), pb.close(r.b)
            live.remove(r)
        tick += 1
        assert tick < 5000
    return most, cut, reused


def _check_solo(net, r, variant):
    """tests/test_gpu_decode_pool.py::_check: the session's pieces against HipNet.decode of the utterance alone"""
    n = r.b.steps_done
    ref_out, ref_heads, ref_used = net.decode(r.aux.to(DEV), n, want_heads=True, variant=variant, rng_seed=RNG_SEED,
                                              want_noise=True, seed=None if r.seed is None else r.seed.to(DEV),
                                              utt_ids=[r.utt_id])
    out, heads, used = torch.cat(r.out, 1), torch.cat(r.heads, 1), torch.cat(r.noise, 1)
    assert out.shape[1] == n * _seg(net.cfg)
    assert torch.equal(out, ref_out), (net.cfg, variant, r.utt_id)
    assert torch.equal(heads, ref_heads), (net.cfg, variant, r.utt_id)
    assert torch.equal(used, ref_used), (net.cfg, variant, r.utt_id)


POOL_NETS = [("bl6_lap", C.bl6_laplace(), False), ("bl6_smx", C.bl6_softmax(), False), ("ref6_lap", C.ref6_laplace(), True)]


@pytest.mark.parametrize("name,cfg,stepped", POOL_NETS, ids=[n[0] for n in POOL_NETS])
def test_push_many_pool_equals_the_pool_of_separate_pushes(gpu_ok, name, cfg, stepped):
    net = _net(name, cfg)
    rng = np.random.default_rng(77 + len(name))
    capacity, n_runs = 70, 76
    runs = [_Run(cfg, int(rng.integers(2, 6 if stepped else 8)), _seed_of(cfg, rng), int(rng.integers(0, 100000)),
                 0 if i < 68 else (int(rng.integers(1, 6)) if i < 75 else -1), aux_seed=100 + i) for i in range(n_runs)]
    mk = (lambda: SteppedDecodePool(net, capacity, rng_seed=RNG_SEED, want_heads=True, want_noise=True)) if stepped else \
         (lambda: DecodePool(net, capacity, rng_seed=RNG_SEED, want_heads=True, want_noise=True))
    pa, pb = mk(), mk()
    most, cut, reused = _drive_pair(pa, pb, runs, rng, capacity, cut_tick=3, stepped=stepped)
    assert most > 64                                # push_many split its sessions over two front end calls
    assert cut is not None and reused and 0 < cut.b.steps_done < cut.F * cfg.U // _seg(cfg)
    variant = pb.resolved_variant
    for r in runs:
        if r is not cut:
            assert r.b.steps_done == r.F * cfg.U // _seg(cfg)
        _check_solo(net, r, variant)


def test_rejected_push_many_changes_nothing(gpu_ok):
    cfg = C.bl6_laplace()
    net = _net("bl6_lap", cfg)
    pool = DecodePool(net, 4, rng_seed=RNG_SEED)
    sess = [pool.open() for _ in range(4)]
    feats = [torch.from_numpy(synth_aux(cfg, 1, 12, seed=40 + i)) for i in range(4)]
    pool.push_many({s: f[:, :, :9] for s, f in zip(sess[:3], feats)})          # the fourth has nothing yet
    torch.cuda.synchronize()

    def state():
        return [(s._stream.frames_received, s._stream.frames_final, s.steps_ready, s.finished,
                 None if s._stream._aux is None else s._stream._aux.clone(),
                 None if s._stream._cond is None else s._stream._cond.clone()) for s in sess]

    before = state()
    assert [b[:2] for b in before] == [(9, 5), (9, 5), (9, 5), (0, 0)]
    good = {s: f[:, :, 9:] for s, f in zip(sess, feats)}
    for bad, exc, fin in ((torch.zeros(1, cfg.n_aux + 1, 3), ValueError, ()), (torch.zeros(cfg.n_aux, 3), ValueError, ()),
                          (torch.zeros(2, cfg.n_aux, 3), ValueError, ()), (None, RuntimeError, (sess[3],))):
        chunks = dict(good)
        if bad is None:
            del chunks[sess[3]]                                                # named in finish, never any features
        else:
            chunks[sess[2]] = bad.to(DEV)
        with pytest.raises(exc):
            pool.push_many(chunks, finish=fin)
        torch.cuda.synchronize()
        for b, a in zip(before, state()):
            assert b[:4] == a[:4] and _same_cond(b[4], a[4]) and _same_cond(b[5], a[5])
    pool.push_many(good, finish=sess)
    for s, f in zip(sess, feats):
        assert s.finished and s._stream.frames_final == f.shape[2] - (9 if s is sess[3] else 0)
    want = torch.ops.swn.frontend(net.packed, feats[0].to(DEV), net.dlist)[0]
    assert torch.equal(sess[0]._stream.cond, want)


# -------------------------------------------------------------------------------------------------------------- driver
def _tiny_run(tmp_path, kind, frames):
    """the synthetic-checkpoint run of tests/test_decode_driver.py"""
    cfg = C.tiny(kind, 2, 4) if kind == "laplace" else C.tiny("softmax", wav_conv_flag=False)
    feats = tmp_path / "feats"
    feats.mkdir()
    rng = np.random.default_rng(3)
    for i, f in enumerate(frames):
        np.save(str(feats / f"utt{i:02d}.npy"), rng.standard_normal((f, cfg.n_aux)).astype(np.float32))
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, seed=7, flavor="trained" if kind == "laplace" else "xavier").items()}
    torch.save({"model": sd}, str(tmp_path / "checkpoint-1.pkl"))
    (tmp_path / "model.json").write_text(json.dumps(dict(cfg.to_dict(), string_path="/feat_org_lf0", audio_in=cfg.audio_in_flag)))
    return cfg, ["--feats", str(feats), "--checkpoint", str(tmp_path / "checkpoint-1.pkl"), "--config", str(tmp_path / "model.json"),
                 "--fs", "22050", "--verbose", "0"]


@pytest.mark.parametrize("kind", ["laplace", "softmax"])
def test_driver_pool_slots_admits_through_push_many(gpu_ok, tmp_path, monkeypatch, kind):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        monkeypatch.delenv(k, raising=False)
    calls = []
    real = DecodePool.push_many
    monkeypatch.setattr(DecodePool, "push_many", lambda self, chunks, finish=(): (calls.append(len(chunks)), real(self, chunks, finish))[1])
    frames = [9, 5, 16, 12, 7, 3]
    cfg, argv = _tiny_run(tmp_path, kind, frames)
    outs = []
    for extra in ([], ["--pool_slots", "4"]):
        out = tmp_path / f"wav{len(extra)}"
        rc = DD.main(kind, argv + ["--outdir", str(out), "--seed", "5", "--noise_source", "device"] + extra)
        assert rc == 0
        outs.append(out)
    assert calls and calls[0] == 4 and sum(calls) == len(frames)           # the first tick admits four sessions in one call
    for i, f in enumerate(frames):
        a, b = (open(o / f"utt{i:02d}.wav", "rb").read() for o in outs)
        assert len(a) == 44 + 2 * f * cfg.U and a == b, (kind, i)
