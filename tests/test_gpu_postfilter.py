"""GPU: noise-shaping restoration on the device (swn_postfilter_chunk, postfilter.NoiseShapingRestorer) computes what the host
dsp.noise_shaping computes, chunk by chunk bit for bit as in one shot, and rides along decode streams, both pools and the
decode driver without changing what they return otherwise."""
import os

import numpy as np
import pytest
import torch

import postfilter_ref as R
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import decode_driver as DD
from shallow_wavenet_amd import dsp, featio
from shallow_wavenet_amd.nets.dswnv import decode_mu_law
from shallow_wavenet_amd.noise_shaping_driver import read_wav_fs
from shallow_wavenet_amd.postfilter import NoiseShapingRestorer
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream, SteppedDecodePool
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RNG_SEED = 4242
ALPHA = 0.455
# a smooth synthetic statistics vector: [uv, lf0, 3 x codeap, mcep 0..49] (m = 49, as run.sh)
MEAN = np.concatenate([[0.9, 5.0, -3.0, -4.0, 0.1], 1.5 * np.exp(-0.15 * np.arange(50)) * np.cos(0.7 * np.arange(50))])


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.5 * np.sin(2 * np.pi * 220 * t / 22050) + 0.45 * rng.uniform(-1, 1, n)
    return torch.from_numpy(x.astype(np.float32))


def _host(x, fs, inv, pade, mean=MEAN, alpha=ALPHA):
    """dsp.noise_shaping, with the Pade order as a parameter (noise_shaping itself uses 4)"""
    x = np.asarray(x, dtype=np.float64)
    if pade == 4:
        return dsp.noise_shaping(x, mean, fs, alpha, inv=inv)
    coef = dsp.shaping_mcep(mean, 0.5, 5, inv)
    b = dsp.mc2b(coef, alpha)
    y = dsp.MLSAFilter(coef.size - 1, alpha, int(fs / 1000 * 5.0), pade=5).synthesis(x, b[None])
    return dsp.low_cut_filter(y, fs)


@pytest.mark.parametrize("pade", [4, 5])
@pytest.mark.parametrize("inv", [True, False])
def test_one_shot_matches_host_noise_shaping(gpu_ok, pade, inv):
    fs = 22050
    r = NoiseShapingRestorer(MEAN, fs, ALPHA, inv=inv, pade=pade, device=DEV)
    xs = [_signal(n, i) for i, n in enumerate([1, 4410, 66000])]
    ys = r.restore([x.to(DEV) for x in xs])
    # the exact reference (tests/postfilter_ref.py) of each signal's first 4 410 samples, one batched run; from zero state the
    # reference of a prefix is the prefix of the reference
    n_ref = 4410
    xr = np.zeros((len(xs), n_ref))
    for i, x in enumerate(xs):
        xr[i, :min(n_ref, x.numel())] = x.numpy()[:n_ref]
    ref, _ = R.restore_ref(xr, r.b, ALPHA, pade, r.taps)
    l1, tail = R.impulse_l1(r.b, ALPHA, pade, r.taps)
    assert tail < 1e-20
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert y.dtype == torch.float32 and y.numel() == x.numel()
        got = y.cpu().numpy().astype(np.float64)
        want = _host(x.numpy(), fs, inv, pade)
        err = float(np.abs(got - want).max())
        assert err <= 1e-6, (pade, inv, x.numel(), err)
        k = min(n_ref, x.numel())
        bound = R.output_bound(ref[i, :k], R.e64(r.order, pade, r.n_taps, l1, float(np.abs(xr[i]).max())))
        share = float((np.abs(got[:k] - ref[i, :k]) / bound).max())
        print(f"pade {pade} inv {inv} n {x.numel()}: share of the bound {share:.3f}")
        assert share <= 1.0, (pade, inv, x.numel(), share)
    assert float(np.abs(want).max()) > 0.1                                        # it filtered something


def test_chunked_equals_one_shot_bitwise(gpu_ok):
    r = NoiseShapingRestorer(MEAN, 22050, ALPHA, capacity=6, device=DEV)
    x = _signal(6000, 7).to(DEV)
    whole = r.restore([x])[0]
    rng = np.random.default_rng(3)
    cuts = np.sort(rng.choice(np.arange(1, 6000), 40, replace=False))
    splits = {c: list(range(0, 6000, c)) + [6000] for c in (1, 7, 441, 1102)}
    splits["random"] = [0] + cuts.tolist() + [6000]
    slots = {k: r.open() for k in splits}
    got = {k: [] for k in splits}
    pos = {k: 0 for k in splits}
    # every split advances in the same calls (other sessions sharing a call must not matter)
    while any(pos[k] < len(splits[k]) - 1 for k in splits):
        chunks = {}
        for k, b in splits.items():
            if pos[k] < len(b) - 1:
                chunks[slots[k]] = x[b[pos[k]]:b[pos[k] + 1]]
                pos[k] += 1
        out = r.run(chunks)
        for k in splits:
            if slots[k] in out:
                got[k].append(out[slots[k]])
    for k in splits:
        assert torch.equal(torch.cat(got[k]), whole), k
    # slot reuse: a session opened in a closed slot starts from zero state
    r.close(slots[7])
    s = r.open()
    assert s == slots[7]
    assert torch.equal(torch.cat([r.run({s: x[:3000]})[s], r.run({s: x[3000:]})[s]]), whole)


def test_many_entries_in_one_call(gpu_ok):
    """more than 64 sessions (several launches) and mu-law classes: each row is its own one-shot restore"""
    r = NoiseShapingRestorer(MEAN, 16000, ALPHA, device=DEV)
    rng = np.random.default_rng(1)
    xs = [torch.from_numpy(rng.integers(0, 256, int(n)).astype(np.int32)).to(DEV) for n in rng.integers(1, 900, 70)]
    ys = r.restore(xs, n_quantize=256)
    for i in (0, 33, 64, 69):
        assert torch.equal(ys[i], r.restore([xs[i]], n_quantize=256)[0])
        want = dsp.noise_shaping(decode_mu_law(xs[i].cpu().numpy().astype(np.float64), 256), MEAN, 16000, ALPHA)
        assert float(np.abs(ys[i].cpu().numpy() - want).max()) <= 1e-6


def _net(cfg, seed=5):
    flavor = "trained" if cfg.kind == "laplace" else "xavier"
    return HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=seed, flavor=flavor), DEV)


def test_stream_restores_its_chunks(gpu_ok):
    cfg = C.bl6_laplace()
    net = _net(cfg)
    F = 40
    aux = torch.from_numpy(synth_aux(cfg, 2, F, seed=4)).to(DEV)
    r = NoiseShapingRestorer(MEAN, 22050, ALPHA, capacity=2, device=DEV)
    plain = DecodeStream(net, 2, rng_seed=RNG_SEED)
    post = DecodeStream(net, 2, rng_seed=RNG_SEED, post_filter=r)
    raw, restored = [], []
    for f in range(0, F, 2):                                    # 10 ms of features per push (U = 110 at 22.05 kHz)
        a, b = plain.push(aux[:, :, f:f + 2]), post.push(aux[:, :, f:f + 2])
        assert len(a) == 2 and len(b) == 3 and torch.equal(a[0], b[0])
        assert b[2].shape == b[0].shape and b[2].dtype == torch.float32
        raw.append(b[0]), restored.append(b[2])
    a, b = plain.finish(), post.finish()
    assert torch.equal(a[0], b[0])
    raw.append(b[0]), restored.append(b[2])
    post.close()
    out = torch.cat(raw, 1)
    one_shot, _ = net.decode(aux, F * cfg.U, rng_seed=RNG_SEED)
    assert torch.equal(out, one_shot)
    want = r.restore([one_shot[0], one_shot[1]])
    got = torch.cat(restored, 1)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _pool_run(pool, r, cfg, lengths, starts, chunk_frames, aux_seed=10):
    """staggered sessions fed chunk_frames of features per tick; -> per session (raw pieces, restored pieces, utt id, aux)"""
    runs = []
    tick = 0
    todo = list(range(len(lengths)))
    live = {}
    done = []
    while todo or live:
        for i in [i for i in todo if starts[i] <= tick and len(live) < pool.capacity]:
            todo.remove(i)
            aux = torch.from_numpy(synth_aux(cfg, 1, lengths[i], seed=aux_seed + i)).to(DEV)
            live[pool.open(utt_id=i)] = [aux, 0, [], [], i]
        for s, st in live.items():
            aux, f = st[0], st[1]
            if f < aux.shape[2]:
                s.push(aux[:, :, f:f + chunk_frames])
                st[1] = f + chunk_frames
                if st[1] >= aux.shape[2]:
                    s.finish()
        for s, res in pool.step().items():
            live[s][2].append(res[0]), live[s][3].append(res[-1])
            assert res[-1].shape == res[0].shape
        for s in [s for s in live if s.done]:
            done.append(live.pop(s))
            pool.close(s)
        tick += 1
    return done


def test_decode_pool_sessions_equal_their_solo_restore(gpu_ok):
    cfg = C.bl6_laplace()
    net = _net(cfg)
    r = NoiseShapingRestorer(MEAN, 22050, ALPHA, capacity=3, device=DEV)
    pool = DecodePool(net, 3, rng_seed=RNG_SEED, post_filter=r)
    lengths, starts = [12, 7, 15, 9, 11], [0, 1, 1, 4, 6]         # 5 sessions over 3 slots: slots are reused after close
    done = _pool_run(pool, r, cfg, lengths, starts, 2)
    assert len(done) == 5
    for aux, _, raw, rest, i in done:
        out = torch.cat(raw, 1)
        solo, _ = net.decode(aux, lengths[i] * cfg.U, rng_seed=RNG_SEED, utt_ids=[i])
        assert torch.equal(out, solo), i
        assert torch.equal(torch.cat(rest, 1)[0], r.restore([solo[0]])[0]), i
    # without a post_filter nothing changes: same tuples
    plain = DecodePool(net, 1, rng_seed=RNG_SEED)
    s = plain.open(utt_id=0)
    s.finish(torch.from_numpy(synth_aux(cfg, 1, 3, seed=10)).to(DEV))
    assert all(len(v) == 2 for v in plain.step().values())


def test_softmax_pool_matches_host_restore(gpu_ok):
    cfg = C.bl6_softmax()
    net = _net(cfg)
    r = NoiseShapingRestorer(MEAN, 16000, ALPHA, capacity=2, device=DEV)
    pool = DecodePool(net, 2, rng_seed=RNG_SEED, post_filter=r)
    done = _pool_run(pool, r, cfg, [10, 6, 8], [0, 0, 2], 3)
    for aux, _, raw, rest, i in done:
        classes = torch.cat(raw, 1)[0].cpu().numpy().astype(np.int64)
        want = dsp.noise_shaping(decode_mu_law(classes, cfg.n_quantize), MEAN, 16000, ALPHA)
        got = torch.cat(rest, 1)[0].cpu().numpy().astype(np.float64)
        assert float(np.abs(got - want).max()) <= 1e-6, i


def test_stepped_pool_sessions_equal_their_solo_restore(gpu_ok):
    cfg = C.ref6_laplace()
    net = _net(cfg)
    r = NoiseShapingRestorer(MEAN, 22050, ALPHA, capacity=2, device=DEV)
    pool = SteppedDecodePool(net, 2, rng_seed=RNG_SEED, post_filter=r)
    runs = []
    for i, F in enumerate([3, 2]):                               # a few hundred steps each (U = 110)
        s = pool.open(utt_id=i)
        aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=20 + i)).to(DEV)
        s.finish(aux)
        runs.append((s, aux, F, [], []))
    while not all(s.done for s, *_ in runs):
        res = pool.step(max_steps=64)
        for s, aux, F, raw, rest in runs:
            if s in res:
                raw.append(res[s][0]), rest.append(res[s][-1])
    for i, (s, aux, F, raw, rest) in enumerate(runs):
        solo, _ = net.decode(aux, F * cfg.U, rng_seed=RNG_SEED, utt_ids=[i], variant=3)
        out = torch.cat(raw, 1)
        assert torch.equal(out, solo[:, :out.shape[1]]) and out.shape[1] == F * cfg.U
        assert torch.equal(torch.cat(rest, 1)[0], r.restore([out[0]])[0]), i


def _tiny_run(tmp_path, frames):
    import json
    cfg = C.tiny("laplace", 2, 4)
    feats = tmp_path / "feats"
    feats.mkdir()
    rng = np.random.default_rng(3)
    for i, f in enumerate(frames):
        np.save(str(feats / f"utt{i:02d}.npy"), rng.standard_normal((f, cfg.n_aux)).astype(np.float32))
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, seed=7, flavor="trained").items()}
    torch.save({"model": sd}, str(tmp_path / "checkpoint-1.pkl"))
    (tmp_path / "model.json").write_text(json.dumps(dict(cfg.to_dict(), string_path="/feat_org_lf0", audio_in=False)))
    stats = str(tmp_path / "stats.npz")
    featio.write_stats(stats, "/feat_org_lf0", MEAN, np.ones_like(MEAN))
    return cfg, stats, ["--feats", str(feats), "--checkpoint", str(tmp_path / "checkpoint-1.pkl"), "--config",
                        str(tmp_path / "model.json"), "--fs", "22050", "--verbose", "0", "--seed", "5",
                        "--noise_source", "device", "--pool_slots", "2"]


def test_driver_writes_restored_wavs(gpu_ok, tmp_path, monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        monkeypatch.delenv(k, raising=False)
    frames = [9, 5, 16, 12]
    cfg, stats, argv = _tiny_run(tmp_path, frames)
    assert DD.main("laplace", argv + ["--outdir", str(tmp_path / "plain")]) == 0
    assert DD.main("laplace", argv + ["--outdir", str(tmp_path / "raw"), "--restore_stats", stats, "--restore_writedir",
                                      str(tmp_path / "restored"), "--mcep_alpha", str(ALPHA)]) == 0
    # the bound rounding the unrestored file to pcm16 can cause: 0.5 LSB through the combined impulse response, + 1 LSB
    imp = np.zeros(4096)
    imp[0] = 1.0
    h = dsp.noise_shaping(imp, MEAN, 22050, ALPHA)
    bound = 0.5 * float(np.abs(h).sum()) + 1.0
    for i, f in enumerate(frames):
        name = f"utt{i:02d}.wav"
        assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "raw" / name, "rb").read()
        raw, fs = read_wav_fs(str(tmp_path / "raw" / name))
        pcm = np.frombuffer(open(tmp_path / "raw" / name, "rb").read()[44:], dtype="<i2")
        assert np.abs(pcm).max() < 32767                                          # no clipping in play
        got = np.frombuffer(open(tmp_path / "restored" / name, "rb").read()[44:], dtype="<i2").astype(np.int64)
        want = np.rint(np.clip(dsp.noise_shaping(pcm / 32767.0, MEAN, 22050, ALPHA), -1, 1) * 32767.0).astype(np.int64)
        assert got.size == f * cfg.U == want.size
        assert int(np.abs(got - want).max()) <= bound, (name, int(np.abs(got - want).max()), bound)
    assert DD.main("laplace", argv + ["--outdir", str(tmp_path / "x"), "--restore_stats", stats]) == 2
