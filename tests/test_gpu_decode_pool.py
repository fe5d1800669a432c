"""GPU: a decode pool (swn_decode_pool_chunk / DecodePool) advances independent sessions in shared launches, and each
session's out, heads and noise are bit-identical to HipNet.decode of that utterance alone - whatever its start tick, its
feature pushes, the per-tick step budgets (across the 64-step noise staging and the frame boundaries, at different phases
per entry), slot reuse in the middle of a run (in-kernel ring zeroing of the generic kernel included), the modules and the
decode driver.  A rejected call changes nothing, and a pooled run replays in the CPU oracle."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import decode_driver as DD
from shallow_wavenet_amd.nets import cswnv_shift1 as mc
from shallow_wavenet_amd.nets import dswnv as md
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodePool
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RNG_SEED = 4242


def _net(cfg, seed=5):
    flavor = "trained" if cfg.kind == "laplace" else "xavier"
    return HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=seed, flavor=flavor), DEV)


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
    """sessions of a pool run: features, seed, id and the pieces the pool returned"""

    def __init__(self, cfg, F, seed, utt_id, start, aux_seed):
        self.aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=aux_seed))
        self.F, self.seed, self.utt_id, self.start = F, seed, utt_id, start
        self.pushed, self.s = 0, None
        self.out, self.heads, self.noise = [], [], []

    def collect(self, r):
        self.out.append(r[0]), self.heads.append(r[1]), self.noise.append(r[2])


def _budget(rng):
    return [None, 1, 2, 3, 63, 64, 65, 127, int(rng.integers(1, 200))][int(rng.integers(0, 9))]


def _drive(pool, runs, rng):
    """tick until every session is done: admit at its start tick, push 0-7 frames per tick (then finish), a random step
    budget per tick"""
    tick, live = 0, []
    while any(r.s is None for r in runs) or live:
        for r in runs:
            if r.s is None and r.start <= tick:
                r.s = pool.open(seed=r.seed, utt_id=r.utt_id)
                live.append(r)
        for r in live:
            if not r.s.finished:
                k = int(rng.integers(0, 8))
                piece = r.aux[:, :, r.pushed:r.pushed + k]
                r.pushed += piece.shape[2]
                if r.pushed >= r.F:
                    r.s.finish(piece.to(DEV))
                else:
                    r.s.push(piece.to(DEV))
        res = pool.step(_budget(rng))
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
    seg = _seg(net.cfg)
    out, heads, used = torch.cat(r.out, 1), torch.cat(r.heads, 1), torch.cat(r.noise, 1)
    assert out.shape[1] == n * seg
    assert torch.equal(out, ref_out), (net.cfg, variant, r.utt_id)
    assert torch.equal(heads, ref_heads), (net.cfg, variant, r.utt_id)
    assert torch.equal(used, ref_used), (net.cfg, variant, r.utt_id)


def _scenario(cfg, variant, seed, frames=(2, 7), n_sess=None):
    net = _net(cfg)
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 10)) if n_sess is None else n_sess
    runs = [_Run(cfg, int(rng.integers(frames[0], frames[1] + 1)), _seed_of(cfg, rng), int(rng.integers(0, 100000)),
                 int(rng.integers(0, 6)), aux_seed=100 + i) for i in range(n)]
    pool = DecodePool(net, 8, variant=variant, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    _drive(pool, runs, rng)
    for r in runs:
        assert r.s.steps_done == r.F * cfg.U // _seg(cfg)
        _check(net, r, variant)


POOL_NETS = [
    ("bl6w", C.bl6_laplace(), 2), ("bl6_sym", C.bl6_laplace(), 6), ("bl6w_lpc4", C.bl6_laplace(1, 4), 0),
    ("bl6_s5l4", C.bl6_laplace(5, 4), 0), ("bl6_smx", C.bl6_softmax(), 0),
    ("tiny_lap", C.tiny("laplace", 2, 4), 1), ("tiny_smx", C.tiny("softmax"), 1),
]


@pytest.mark.parametrize("name,cfg,variant", POOL_NETS, ids=[n[0] for n in POOL_NETS])
def test_pool_sessions_equal_solo_decodes(gpu_ok, name, cfg, variant):
    _scenario(cfg, variant, seed=len(name))


def test_pool_ref6_on_the_generic_kernel(gpu_ok):
    _scenario(C.ref6_laplace(), 1, seed=3, frames=(1, 1), n_sess=3)


@pytest.mark.parametrize("name,cfg,variant", [("bl6w", C.bl6_laplace(), 0), ("tiny_lap", C.tiny("laplace", 2, 4), 1),
                                              ("tiny_smx", C.tiny("softmax"), 1)], ids=["bl6w", "tiny_lap", "tiny_smx"])
def test_slot_reuse_in_the_middle_of_a_run(gpu_ok, name, cfg, variant):
    """a session closed part-way frees its slot; the next session BEGINs there in the same launch as resumed ones (the
    generic kernel zeroes that slot's rings itself) and matches its solo decode, the others are unaffected"""
    net = _net(cfg)
    rng = np.random.default_rng(21)
    runs = [_Run(cfg, 4, _seed_of(cfg, rng), 10 + i, 0, aux_seed=200 + i) for i in range(3)]
    late = _Run(cfg, 3, _seed_of(cfg, rng), 77, 0, aux_seed=299)
    pool = DecodePool(net, 3, variant=variant, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    for r in runs:
        r.s = pool.open(seed=r.seed, utt_id=r.utt_id)
        r.s.finish(r.aux.to(DEV))
    res = pool.step(runs[1].s.steps_ready // 2)
    for r in runs:
        r.collect(res[r.s])
    cut = runs[1]
    pool.close(cut.s)
    late.s = pool.open(seed=late.seed, utt_id=late.utt_id)
    assert late.s.slot == cut.s.slot
    late.s.finish(late.aux.to(DEV))
    live = [runs[0], runs[2], late]
    while live:
        res = pool.step(int(rng.integers(1, 90)))
        assert len(res) == len(live)
        for r in live:
            r.collect(res[r.s])
        live = [r for r in live if not r.s.done]
    for r in (runs[0], runs[2], late):
        _check(net, r, variant)
    assert 0 < cut.s.steps_done < cut.s.steps_ready
    _check(net, cut, variant)


def test_rejected_call_changes_nothing(gpu_ok):
    cfg = C.bl6_laplace()
    net = _net(cfg)
    pool = DecodePool(net, 2, rng_seed=RNG_SEED)
    a, b = pool.open(), pool.open()
    for i, s in enumerate((a, b)):
        s.finish(torch.from_numpy(synth_aux(cfg, 1, 2, seed=i)).to(DEV))
    pool.step(30)
    torch.cuda.synchronize()
    before = pool._session.clone()
    with pytest.raises(RuntimeError):
        torch.ops.swn.decode_pool_chunk(net.packed, pool._session, [a._stream._cond[0], b._stream._cond[0]], [0, 0], [30, 30],
                                        [5, 5], [False, False], None, [0, 1], net.dlist, 2, 0, RNG_SEED, False, False)
    torch.cuda.synchronize()
    assert torch.equal(pool._session.view(torch.int32), before.view(torch.int32))


def test_pooled_run_replays_in_the_cpu_oracle(gpu_ok):
    cfg = C.tiny("laplace", 2, 4)
    sd = synth_state_dict(cfg, seed=5, flavor="trained")
    net, P = HipNet.from_state_dict(cfg, sd, DEV), cpu_ref.as_params(sd)
    F = 6
    n = F * cfg.U
    aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=2))
    other = torch.from_numpy(synth_aux(cfg, 1, 4, seed=8))
    pool = DecodePool(net, 2, rng_seed=99, want_noise=True)
    s, t = pool.open(), pool.open(utt_id=3)
    t.finish(other.to(DEV))
    outs, used = [], []
    for f in range(F + 1):
        if f < F:
            s.push(aux[:, :, f:f + 1].to(DEV))
        else:
            s.finish()
        res = pool.step(7)
        if s in res:
            outs.append(res[s][0]), used.append(res[s][2])
    while not s.done:
        res = pool.step()
        outs.append(res[s][0]), used.append(res[s][2])
    out = torch.cat(outs, 1).cpu().numpy()[0]
    noise = torch.cat(used, 1).permute(1, 0, 2).contiguous().cpu().numpy()          # (n_steps, B, seg): the oracle's layout
    ref = cpu_ref.laplace_generate(cfg, P, aux, [n], noise)[0]
    assert out.shape[0] == n
    assert float(np.abs(out - ref).max()) <= 1e-5


def test_modules_open_pool_equal_batch_fast_generate(gpu_ok):
    for kind in ("laplace", "softmax"):
        cfg = C.bl6_laplace() if kind == "laplace" else C.bl6_softmax()
        sd = synth_state_dict(cfg, seed=7, flavor="trained" if kind == "laplace" else "xavier")
        m = (mc.CSWNV if kind == "laplace" else md.DSWNV)(**cfg.ctor_kwargs())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.cuda().eval()
        ids = [5, 2]
        m.noise_source, m.noise_rng_seed, m.noise_utterance_ids = "device", 31337, ids
        F = 12
        aux = torch.from_numpy(synth_aux(cfg, 2, F, seed=6)).cuda()
        n = [F * cfg.U, (F - 3) * cfg.U]
        if kind == "laplace":
            audio = torch.tensor([[0.25], [-0.5]]).cuda()
        else:
            audio = torch.tensor([[17], [250]]).cuda()
        want = m.batch_fast_generate(audio, aux, n)
        pool = m.open_pool(2)
        sess = []
        for b in range(2):
            seed = audio[b, -1:].to(torch.int32) if kind == "softmax" else audio[b:b + 1, -cfg.seg:]
            sess.append(pool.open(seed=seed, utt_id=ids[b]))
        got = [[], []]
        for f in range(0, F + 3, 3):
            for b, s in enumerate(sess):
                if f < F:
                    s.push(aux[b:b + 1, :, f:f + 3])
                else:
                    s.finish()
            res = pool.step()
            for b, s in enumerate(sess):
                if s in res:
                    got[b].append(res[s][0])
        assert all(s.done for s in sess)
        for b in range(2):
            g = torch.cat(got[b], 1).cpu().numpy()[0]
            assert np.array_equal(g[:n[b]].astype(want[b].dtype), want[b]), (kind, b)


def _tiny_run(tmp_path, kind, frames):
    """the synthetic-checkpoint run of tests/test_decode_driver.py"""
    import json
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
def test_driver_pool_slots_writes_the_default_wavs(gpu_ok, tmp_path, monkeypatch, kind):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        monkeypatch.delenv(k, raising=False)
    frames = [9, 5, 16, 12]
    cfg, argv = _tiny_run(tmp_path, kind, frames)
    outs = []
    for extra in ([], ["--pool_slots", "2"]):
        out = tmp_path / f"wav{len(extra)}"
        rc = DD.main(kind, argv + ["--outdir", str(out), "--seed", "5", "--noise_source", "device"] + extra)
        assert rc == 0
        outs.append(out)
    for i, f in enumerate(frames):
        a, b = (open(o / f"utt{i:02d}.wav", "rb").read() for o in outs)
        assert len(a) == 44 + 2 * f * cfg.U and a == b, (kind, i)
    # host noise is drawn for the whole run up front: not for a pool
    assert DD.main("laplace", argv + ["--outdir", str(tmp_path / "h"), "--pool_slots", "2"]) != 0
