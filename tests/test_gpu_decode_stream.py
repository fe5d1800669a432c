"""GPU: the streamed decode (swn_decode_chunk / DecodeStream) is bit-identical to the one-shot decode - for every kernel
variant, any partition of the steps into chunks (0- and 1-step chunks, chunks across the 64-step noise staging), device
and host noise, forced input, seed waveforms and utterance indices; features pushed in pieces give the one-shot cond and
samples; the modules and the decode driver stream to the same results; and a streamed run replays in the CPU oracle."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import decode_driver as DD
from shallow_wavenet_amd import noise as _noise
from shallow_wavenet_amd.nets import cswnv_shift1 as mc
from shallow_wavenet_amd.nets import dswnv as md
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodeStream
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _net(cfg, seed=5):
    flavor = "trained" if cfg.kind == "laplace" else "xavier"
    return HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=seed, flavor=flavor), DEV)


def _seg(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


def _frames_for(cfg, min_steps):
    return -(-min_steps * _seg(cfg) // cfg.U) + 1


def _partitions(N):
    fixed = [0, 1, 1, 1, 61, 64, 65]
    parts = [[N], fixed + [N - sum(fixed)]]
    for s in (11, 12):
        rng = np.random.default_rng(s)
        p, left = [], N
        while left > 0:
            n = int(min(left, rng.integers(0, 97)))
            p.append(n)
            left -= n
        parts.append(p)
    return parts


def _stream(net, aux, parts, variant=0, noise=None, forced=None, seed=None, utt_ids=None, rng_seed=77):
    cfg = net.cfg
    B = aux.shape[0]
    s = DecodeStream(net, B, variant=variant, seed=seed, rng_seed=rng_seed, utt_ids=utt_ids, want_heads=True, want_noise=True)
    s.push(aux, generate=False)
    s.finish(generate=False)
    outs, heads, used = [], [], []
    k, seg = 0, _seg(cfg)
    for n in parts:
        nz = None if noise is None else noise[:, k:k + n]
        fc = None if forced is None else forced[:, k * seg:(k + n) * seg]
        o, h, u = s.advance(n, noise=nz, forced=fc)
        outs.append(o), heads.append(h), used.append(u)
        k += n
    assert s.steps_done == sum(parts)
    return torch.cat(outs, 1), torch.cat(heads, 1), torch.cat(used, 1), s


def _check_partitions(cfg, B, variant, min_steps, **kw):
    net = _net(cfg)
    F = _frames_for(cfg, min_steps)
    aux = torch.from_numpy(synth_aux(cfg, B, F, seed=3)).to(DEV)
    N = F * cfg.U // _seg(cfg)
    ref_out, ref_heads, ref_used = net.decode(aux, N, kw.get("noise"), kw.get("forced"), want_heads=True, variant=variant,
                                              seed=kw.get("seed"), rng_seed=77, want_noise=True, utt_ids=kw.get("utt_ids"))
    for parts in _partitions(N):
        out, heads, used, s = _stream(net, aux, parts, variant=variant, **kw)
        assert torch.equal(s.cond, net.frontend(aux))
        assert torch.equal(out, ref_out), (cfg, B, variant, parts)
        assert torch.equal(heads, ref_heads), (cfg, B, variant, parts)
        assert torch.equal(used, ref_used), (cfg, B, variant, parts)


NETS = [
    ("bl6_lap", C.bl6_laplace(), 2, 300), ("bl6_lap_lpc4", C.bl6_laplace(1, 4), 2, 300), ("bl6_lap_s5l4", C.bl6_laplace(5, 4), 2, 300),
    ("bl6_smx", C.bl6_softmax(), 2, 300), ("ref6_lap_b2", C.ref6_laplace(), 2, 200), ("ref6_lap_b27", C.ref6_laplace(), 27, 200),
    ("ref6_smx_b1", C.ref6_softmax(), 1, 200), ("tiny_lap", C.tiny("laplace", 2, 4), 2, 300), ("tiny_smx", C.tiny("softmax"), 2, 300),
]


@pytest.mark.parametrize("name,cfg,B,min_steps", NETS, ids=[n[0] for n in NETS])
def test_partitions_equal_one_shot_auto_variant(gpu_ok, name, cfg, B, min_steps):
    _check_partitions(cfg, B, 0, min_steps)


@pytest.mark.parametrize("variant", [1, 6, 3])
def test_partitions_equal_one_shot_forced_variants(gpu_ok, variant):
    _check_partitions(C.bl6_laplace(), 2, variant, 300)


INPUT_NETS = [("bl6w", C.bl6_laplace()), ("bl6_smx", C.bl6_softmax()), ("bl6_s5l4", C.bl6_laplace(5, 4)),
              ("ref6", C.ref6_laplace()), ("tiny_lap", C.tiny("laplace", 2, 4)), ("tiny_smx", C.tiny("softmax"))]


@pytest.mark.parametrize("name,cfg", INPUT_NETS, ids=[n[0] for n in INPUT_NETS])
def test_inputs_host_noise_forced_seed_and_ids(gpu_ok, name, cfg):
    B, seg = 2, _seg(cfg)
    F = _frames_for(cfg, 200)
    N = F * cfg.U // seg
    g = torch.Generator().manual_seed(9)
    if cfg.kind == "softmax":
        noise = _noise.softmax_exponential(cfg, N, B).to(DEV)
        forced = torch.randint(0, cfg.n_quantize, (B, N), generator=g, dtype=torch.int32).to(DEV)
        seed = torch.tensor([3, 200], dtype=torch.int32, device=DEV)
    else:
        noise = _noise.laplace_uniform(cfg, N, B).to(DEV)
        forced = (torch.rand((B, N * seg), generator=g) * 1.8 - 0.9).to(DEV)
        seed = (torch.rand((B, seg), generator=g) - 0.5).to(DEV)
    ids = [41, 7]
    rng = np.random.default_rng(5)
    for kw in (dict(noise=noise), dict(forced=forced), dict(seed=seed), dict(utt_ids=ids),
               dict(noise=noise, forced=forced, seed=seed)):
        net = _net(cfg)
        aux = torch.from_numpy(synth_aux(cfg, B, F, seed=4)).to(DEV)
        ref = net.decode(aux, N, kw.get("noise"), kw.get("forced"), want_heads=True, seed=kw.get("seed"), rng_seed=77,
                         want_noise=True, utt_ids=kw.get("utt_ids"))
        parts, left = [], N
        while left > 0:
            n = int(min(left, rng.integers(0, 70)))
            parts.append(n)
            left -= n
        got = _stream(net, aux, parts, **kw)
        for a, b in zip(got[:3], ref):
            assert torch.equal(a, b), (name, sorted(kw))


PIECE_NETS = [("bl6w", C.bl6_laplace()), ("bl6_smx", C.bl6_softmax()), ("bl6_s5l4", C.bl6_laplace(5, 4)),
              ("ref6", C.ref6_laplace()), ("tiny_smx", C.tiny("softmax"))]


@pytest.mark.parametrize("name,cfg", PIECE_NETS, ids=[n[0] for n in PIECE_NETS])
def test_features_in_pieces_equal_one_shot(gpu_ok, name, cfg):
    """features pushed 1, 2, 5, 17, rest frames at a time then finish(): the assembled cond is frontend(full_aux) and the
    samples are HipNet.decode(full_aux, frames * U // seg), at B = 3 with different utterances"""
    B, F = 3, 40
    net = _net(cfg)
    aux = torch.from_numpy(synth_aux(cfg, B, F, seed=8)).to(DEV)
    N = F * cfg.U // _seg(cfg)
    ref, _ = net.decode(aux, N, rng_seed=1234)
    s = DecodeStream(net, B, rng_seed=1234)
    outs, f0 = [], 0
    for n in (1, 2, 5, 17, F - 25):
        o, _ = s.push(aux[:, :, f0:f0 + n])
        f0 += n
        assert s.frames_received == f0 and s.frames_final == max(0, f0 - s.lookahead_frames)
        assert s.steps_done == s.frames_final * cfg.U // _seg(cfg) and o.shape[1] == s.steps_done * _seg(cfg) - sum(x.shape[1] for x in outs)
        outs.append(o)
    outs.append(s.finish()[0])
    assert s.finished and s.steps_done == N
    assert torch.equal(s.cond, net.frontend(aux))
    assert torch.equal(torch.cat(outs, 1), ref)
    with pytest.raises(RuntimeError):
        s.push(aux[:, :, :1])
    with pytest.raises(RuntimeError):
        s.advance(1)


def test_modules_open_stream_equal_batch_fast_generate(gpu_ok):
    for kind in ("laplace", "softmax"):
        cfg = C.bl6_laplace() if kind == "laplace" else C.bl6_softmax()
        sd = synth_state_dict(cfg, seed=7, flavor="trained" if kind == "laplace" else "xavier")
        m = (mc.CSWNV if kind == "laplace" else md.DSWNV)(**cfg.ctor_kwargs())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.cuda().eval()
        m.noise_source, m.noise_rng_seed, m.noise_utterance_ids = "device", 31337, [5, 2]
        F = 12
        aux = torch.from_numpy(synth_aux(cfg, 2, F, seed=6)).cuda()
        n = [F * cfg.U, (F - 3) * cfg.U]
        if kind == "laplace":
            audio = torch.tensor([[0.25], [-0.5]]).cuda()
        else:
            audio = torch.tensor([[17], [250]]).cuda()
        want = m.batch_fast_generate(audio, aux, n)
        s = m.open_stream(2, audio)
        pieces = [s.push(aux[:, :, f:f + 3])[0] for f in range(0, F, 3)] + [s.finish()[0]]
        got = torch.cat(pieces, 1).cpu().numpy()
        for b in range(2):
            assert np.array_equal(got[b, :n[b]].astype(want[b].dtype), want[b]), (kind, b)


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
def test_driver_stream_frames_writes_the_one_shot_wavs(gpu_ok, tmp_path, monkeypatch, kind):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        monkeypatch.delenv(k, raising=False)
    frames = [9, 5, 16, 12]
    cfg, argv = _tiny_run(tmp_path, kind, frames)
    outs = []
    for sf in (0, 7):
        out = tmp_path / f"wav{sf}"
        rc = DD.main(kind, argv + ["--outdir", str(out), "--batch_size", "2", "--seed", "5", "--noise_source", "device",
                                   "--stream_frames", str(sf)])
        assert rc == 0
        outs.append(out)
    for i, f in enumerate(frames):
        a, b = (open(o / f"utt{i:02d}.wav", "rb").read() for o in outs)
        assert len(a) == 44 + 2 * f * cfg.U and a == b, (kind, i)
    # host noise is drawn for the whole run up front: not streamable
    assert DD.main("laplace", argv + ["--outdir", str(tmp_path / "h"), "--stream_frames", "7"]) != 0


def test_streamed_run_replays_in_the_cpu_oracle(gpu_ok):
    cfg = C.tiny("laplace", 2, 4)
    sd = synth_state_dict(cfg, seed=5, flavor="trained")
    net, P = HipNet.from_state_dict(cfg, sd, DEV), cpu_ref.as_params(sd)
    F = 6
    n = F * cfg.U
    aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=2))
    s = DecodeStream(net, 1, rng_seed=99, want_noise=True)
    outs, used = [], []
    for f in range(F):
        o, _, u = s.push(aux[:, :, f:f + 1])
        outs.append(o), used.append(u)
    o, _, u = s.finish()
    outs.append(o), used.append(u)
    out = torch.cat(outs, 1).cpu().numpy()[0]
    noise = torch.cat(used, 1).permute(1, 0, 2).contiguous().cpu().numpy()          # (n_steps, B, seg): the oracle's layout
    ref = cpu_ref.laplace_generate(cfg, P, aux, [n], noise)[0]
    assert out.shape[0] == n
    assert float(np.abs(out - ref).max()) <= 1e-5
