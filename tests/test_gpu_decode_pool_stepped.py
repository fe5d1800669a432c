"""GPU: the stepped decode pool (swn_decode_pool_stepped_chunk / SteppedDecodePool) on the run.sh geometry (REF6) advances
independent sessions in shared launches, and each session's out, heads and noise are bit-identical to HipNet.decode of that
utterance alone with variant 3 - whatever its start tick, its feature pushes, the per-tick step budgets, a prologue split
over ticks while others generate, slot reuse in the middle of a run, and whether the per-entry or the tile kernels serve
it.  A slot no entry names is left byte for byte, the modules and the decode driver route REF6 nets to it, and a pooled run
replays in the CPU oracle."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from shallow_wavenet_amd import _lib, ops
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import decode_driver as DD
from shallow_wavenet_amd.nets import cswnv_shift1 as mc
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import SteppedDecodePool
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RNG_SEED = 4242
TOL_FREE = 1e-5                                # the free-running REF6 decode tolerance of the parity tests


def _net(cfg, seed=5):
    flavor = "trained" if cfg.kind == "laplace" else "xavier"
    return HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=seed, flavor=flavor), DEV)


def _seg(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


def _seed_of(cfg, rng):
    if rng.random() < 0.3:
        return None
    if cfg.kind == "softmax":
        return torch.tensor([int(rng.integers(0, cfg.n_quantize))], dtype=torch.int32)
    return torch.from_numpy(rng.uniform(-0.9, 0.9, (1, cfg.seg)).astype(np.float32))


class _Run:
    def __init__(self, cfg, F, seed, utt_id, start, aux_seed):
        self.aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=aux_seed))
        self.F, self.seed, self.utt_id, self.start = F, seed, utt_id, start
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


def _drive(pool, runs, rng):
    """tick until every session is done: admit at its start tick, push 1-3 frames per tick (then finish), a random step
    budget and, in some ticks, a prologue budget"""
    tick, live = 0, []
    while any(r.s is None for r in runs) or live:
        for r in runs:
            if r.s is None and r.start <= tick:
                r.s = pool.open(seed=r.seed, utt_id=r.utt_id)
                live.append(r)
        for r in live:
            if not r.s.finished:
                piece = r.aux[:, :, r.pushed:r.pushed + int(rng.integers(1, 4))]
                r.pushed += piece.shape[2]
                (r.s.finish if r.pushed >= r.F else r.s.push)(piece.to(DEV))
        steps = [None, 1, 7, 64, 150][int(rng.integers(0, 5))]
        pro = [None, None, 100, 300][int(rng.integers(0, 4))]
        res = pool.step(steps, max_prologue=pro)
        for r in live:
            if r.s in res:
                r.collect(res[r.s])
        for r in [r for r in live if r.s.done]:
            pool.close(r.s)
            live.remove(r)
        tick += 1
        assert tick < 2000


NETS = [("ref6_s1l4", C.ref6_laplace(1, 4)), ("ref6_s5l4", C.ref6_laplace(5, 4)), ("ref6_smx", C.ref6_softmax())]


@pytest.mark.parametrize("n_sess", [5, 27])
@pytest.mark.parametrize("name,cfg", NETS, ids=[n[0] for n in NETS])
def test_stepped_pool_sessions_equal_solo_decodes(gpu_ok, name, cfg, n_sess):
    """5 sessions: the per-entry kernels; 27 (not a multiple of 8): the tile kernels while 24 or more are active"""
    net = _net(cfg)
    rng = np.random.default_rng(len(name) + n_sess)
    runs = [_Run(cfg, int(rng.integers(2, 7)), _seed_of(cfg, rng), int(rng.integers(0, 100000)),
                 0 if n_sess > 8 and i < 26 else int(rng.integers(0, 4)), aux_seed=100 + i) for i in range(n_sess)]
    pool = SteppedDecodePool(net, 32, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    _drive(pool, runs, rng)
    for r in runs:
        assert r.s.steps_done == r.F * cfg.U // _seg(cfg)
        _check(net, r)


def test_split_prologue_slot_reuse_and_untouched_slot(gpu_ok):
    """a session closed part-way frees its slot; the next one BEGINs there and spreads its prologue over ticks of 100
    iterations while the others generate; a slot that no entry names stays byte-identical"""
    cfg = C.ref6_laplace(1, 4)
    net = _net(cfg)
    rng = np.random.default_rng(21)
    pool = SteppedDecodePool(net, 4, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    runs = [_Run(cfg, 3, _seed_of(cfg, rng), 10 + i, 0, aux_seed=200 + i) for i in range(3)]
    for r in runs:
        r.s = pool.open(seed=r.seed, utt_id=r.utt_id)
        r.s.finish(r.aux.to(DEV))
    idle = _Run(cfg, 2, None, 55, 0, aux_seed=250)                    # slot 3: opened, no features yet
    idle.s = pool.open(utt_id=idle.utt_id)
    res = pool.step(40)
    for r in runs:
        r.collect(res[r.s])
    cut = runs[1]
    pool.close(cut.s)
    late = _Run(cfg, 2, _seed_of(cfg, rng), 77, 0, aux_seed=299)
    late.s = pool.open(seed=late.seed, utt_id=late.utt_id)
    assert late.s.slot == cut.s.slot
    late.s.finish(late.aux.to(DEV))
    stride = int(_lib.lib().swn_decode_session_floats(ctypes.byref(ops._desc(net.dlist)), 1, 3))
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
    assert pro_ticks >= 6                                             # 690 prologue iterations, 100 per tick
    assert torch.equal(pool._session[3 * stride:4 * stride].view(torch.int32), before.view(torch.int32))
    for r in (runs[0], runs[2], late):
        _check(net, r)
    assert 0 < cut.s.steps_done < cut.s.steps_ready
    _check(net, cut)


def test_pooled_ref6_run_replays_in_the_cpu_oracle(gpu_ok):
    cfg = C.ref6_laplace(1, 4)
    sd = synth_state_dict(cfg, seed=5, flavor="trained")
    net, P = HipNet.from_state_dict(cfg, sd, DEV), cpu_ref.as_params(sd)
    F = 2
    aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=2))
    pool = SteppedDecodePool(net, 2, rng_seed=99, want_noise=True)
    other = pool.open(utt_id=3)
    other.finish(torch.from_numpy(synth_aux(cfg, 1, 1, seed=8)).to(DEV))
    s = pool.open()
    outs, used = [], []
    s.push(aux[:, :, :1].to(DEV))
    s.finish(aux[:, :, 1:].to(DEV))
    while not s.done:
        res = pool.step(50, max_prologue=300)
        if s in res:
            outs.append(res[s][0]), used.append(res[s][2])
    out = torch.cat(outs, 1).cpu().numpy()[0]
    noise = torch.cat(used, 1).permute(1, 0, 2).contiguous().cpu().numpy()
    ref = cpu_ref.laplace_generate(cfg, P, aux, [F * cfg.U], noise)[0]
    assert out.shape[0] == F * cfg.U
    assert float(np.abs(out - ref).max()) <= TOL_FREE


def test_module_open_pool_on_ref6_equals_batch_fast_generate(gpu_ok):
    cfg = C.ref6_laplace(1, 4)
    sd = synth_state_dict(cfg, seed=7, flavor="trained")
    m = mc.CSWNV(**cfg.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.cuda().eval()
    ids = [5, 2]
    m.noise_source, m.noise_rng_seed, m.noise_utterance_ids = "device", 31337, ids
    F = 4
    aux = torch.from_numpy(synth_aux(cfg, 2, F, seed=6)).cuda()
    n = [F * cfg.U, (F - 2) * cfg.U]
    audio = torch.tensor([[0.25], [-0.5]]).cuda()
    want = m.batch_fast_generate(audio, aux, n)
    pool = m.open_pool(2)
    assert isinstance(pool, SteppedDecodePool)
    sess = [pool.open(seed=audio[b:b + 1, -cfg.seg:], utt_id=ids[b]) for b in range(2)]
    got = [[], []]
    for f in range(0, F + 2, 2):
        for b, s in enumerate(sess):
            if f < F:
                s.push(aux[b:b + 1, :, f:f + 2])
            else:
                s.finish()
        res = pool.step()
        for b, s in enumerate(sess):
            if s in res:
                got[b].append(res[s][0])
    assert all(s.done for s in sess)
    for b in range(2):
        g = torch.cat(got[b], 1).cpu().numpy()[0]
        assert np.array_equal(g[:n[b]].astype(want[b].dtype), want[b]), b


def test_driver_pool_slots_on_a_ref6_checkpoint(gpu_ok, tmp_path, monkeypatch):
    """--pool_slots on a run.sh-geometry checkpoint writes the WAVs of the default path"""
    import json
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        monkeypatch.delenv(k, raising=False)
    cfg = C.ref6_laplace(1, 4)
    frames = [3, 2, 4]
    feats = tmp_path / "feats"
    feats.mkdir()
    rng = np.random.default_rng(3)
    for i, f in enumerate(frames):
        np.save(str(feats / f"utt{i:02d}.npy"), rng.standard_normal((f, cfg.n_aux)).astype(np.float32))
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, seed=7, flavor="trained").items()}
    torch.save({"model": sd}, str(tmp_path / "checkpoint-1.pkl"))
    (tmp_path / "model.json").write_text(json.dumps(dict(cfg.to_dict(), string_path="/feat_org_lf0", audio_in=False)))
    argv = ["--feats", str(feats), "--checkpoint", str(tmp_path / "checkpoint-1.pkl"), "--config",
            str(tmp_path / "model.json"), "--fs", "22050", "--verbose", "0", "--seed", "5", "--noise_source", "device"]
    outs = []
    for extra in ([], ["--pool_slots", "2"]):
        out = tmp_path / f"wav{len(extra)}"
        assert DD.main("laplace", argv + ["--outdir", str(out)] + extra) == 0
        outs.append(out)
    for i, f in enumerate(frames):
        a, b = (open(o / f"utt{i:02d}.wav", "rb").read() for o in outs)
        assert len(a) == 44 + 2 * f * cfg.U and a == b, i
