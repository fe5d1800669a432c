"""GPU: decode with bf16 storage of the streamed head matrices (weights="bf16").

bf16 -> fp32 is exact and the bf16 instantiations of the symmetric BL6 kernel run the fp32 kernel's FMAs in its order, so the
mode is pinned WITHOUT a tolerance: weights="bf16" on a model W equals, bit for bit, the fp32 symmetric kernel on
bf16_weight_state_dict(W).  The other tests show that the mode really reads rounded weights (no silent fp32 fallback), that
the CPU oracle on the rounded state dict agrees at the tolerances of tests/test_gpu_decode_parity.py, and that streams, pools,
repack and the decode driver carry the mode.  Every decode here runs at most 300 steps at B <= 3."""
import functools
import json
from dataclasses import replace

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import cpu_ref
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import decode_driver as DD
from shallow_wavenet_amd import noise as _noise
from shallow_wavenet_amd.nets import dswnv as md
from shallow_wavenet_amd.runtime import HipNet, bf16_weight_state_dict
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_STEPS = 300
SMX = ["g1_bl6_softmax_b1", "g1_bl6_softmax_b3", "g8_seed_smx_bl6"]
LAP = ["g1_bl6_lap_s5l4_b1_trained", "g1_bl6_lap_s5l4_b3_xavier", "g8_seed_laplace_bl6_s2l4",
       "g1_bl6_lap_s1l4_u240_b2_trained", "g1_bl6_lap_s1l0_b1_trained"]
RNG = 0x5EED0123456789AB


def _seg(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


def _variants(cfg):
    """the variants that reach the symmetric kernel: 6 for the single-sample Laplace nets, 0 and 6 otherwise"""
    return (6,) if cfg.kind == "laplace" and cfg.seg == 1 else (0, 6)


@functools.lru_cache(maxsize=None)
def _case(name):
    """fixture -> everything the tests share: the model W with the mode on, the fp32 model on the rounded weights, the
    fixture's inputs cut to MAX_STEPS steps (host noise in the kernels' layout, the seed where the fixture has one)"""
    cfg, d = load_golden(name)
    sd = synth_state_dict(cfg, seed=int(d["wseed"]), flavor=str(d["flavor"]))
    sd16 = bf16_weight_state_dict(cfg, sd)
    aux = torch.from_numpy(d["aux"])
    B, seg = aux.shape[0], _seg(cfg)
    n_all = int(d["n_samples"].max()) // seg
    n_steps = min(n_all, MAX_STEPS)
    if cfg.kind == "softmax":
        q = d["q"] if "q" in d else cpu_ref.softmax_noise(cfg, n_all, B, generator=torch.Generator().manual_seed(int(d["noise_seed"])))
        noise = q[:n_steps]
    else:
        noise = d["noise"][:n_steps]
    seed = None
    if "seed" in d:
        seed = torch.from_numpy(d["seed"]).reshape(B, -1)
        seed = seed[:, 0] if cfg.kind == "softmax" else seed
    return dict(cfg=cfg, sd=sd, sd16=sd16, aux=aux, B=B, n_steps=n_steps, noise_sbw=noise,
                noise=torch.from_numpy(np.ascontiguousarray(noise)).permute(1, 0, 2).contiguous(), seed=seed,
                net=HipNet.from_state_dict(cfg, sd, DEV), net16=HipNet.from_state_dict(cfg, sd16, DEV))


def _np(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


# ---------------------------------------------------------------------------------------------------------------- image
@pytest.mark.parametrize("cfg", [C.bl6_laplace(5, 4), C.bl6_softmax()], ids=["lap_s5l4", "softmax"])
def test_device_built_image_equals_numpy(gpu_ok, cfg):
    """section [NS / 2][rows][4 lanes][4 words]: word j of lane p of row r in slice pair g holds bf16(W[r, 32 g + 4 p + j]) in
    its low half and bf16(W[r, 32 g + 16 + 4 p + j]) in its high half; sections out_skip (per layer), out_1, softmax out_2"""
    sd = synth_state_dict(cfg, seed=11, flavor="trained" if cfg.kind == "laplace" else "xavier")
    net = HipNet.from_state_dict(cfg, sd, DEV)
    got = net.decode_w16_image().cpu().numpy().view(np.uint32)

    def bits(w):
        t = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(torch.bfloat16)
        return t.view(torch.int16).numpy().astype(np.uint16).astype(np.uint32)

    def section(w):                                          # w (rows, n_in)
        rows, n_in = w.shape
        b = bits(w).reshape(rows, n_in // 32, 2, 4, 4)      # row, pair g, half, lane, j
        return (b[:, :, 0] | (b[:, :, 1] << 16)).transpose(1, 0, 2, 3).reshape(-1)

    want = [section(sd[f"out_skip.{l}.weight"][:, :, 0]) for l in range(cfg.L)] + [section(sd["out_1.weight"][:, :, 0])]
    if cfg.kind == "softmax":
        want.append(section(sd["out_2.weight"][:, :, 0]))
    want = np.concatenate(want)
    assert got.shape == want.shape
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------------------------------------- bit-identity
@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("name", SMX + LAP)
def test_bf16_equals_fp32_kernel_on_rounded_weights(gpu_ok, name, source):
    c = _case(name)
    noise = c["noise"] if source == "host" else None
    for v in _variants(c["cfg"]):
        kw = dict(want_heads=True, variant=v, seed=c["seed"], rng_seed=RNG, rng_utt0=3, want_noise=True)
        got = _np(c["net"].decode(c["aux"], c["n_steps"], noise, weights="bf16", **kw))
        want = _np(c["net16"].decode(c["aux"], c["n_steps"], noise, **kw))
        for g, w, what in zip(got, want, ("out", "heads", "noise")):
            assert g.shape == w.shape and np.array_equal(g, w), (name, source, v, what)
        if source == "host":
            assert np.array_equal(got[2], c["noise"].numpy())


@pytest.mark.parametrize("name", ["g1_bl6_softmax_b1", "g1_bl6_lap_s5l4_b1_trained"])
def test_bf16_equals_fp32_kernel_teacher_forced(gpu_ok, name):
    c = _case(name)
    cfg, B, n = c["cfg"], c["B"], c["n_steps"]
    rng = np.random.default_rng(5)
    if cfg.kind == "softmax":
        forced = torch.from_numpy(rng.integers(0, cfg.n_quantize, (B, n)).astype(np.int32))
    else:
        forced = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, n * cfg.seg)).astype(np.float32))
    for v in _variants(cfg):
        got = _np(c["net"].decode(c["aux"], n, c["noise"], forced=forced, want_heads=True, variant=v, weights="bf16"))
        want = _np(c["net16"].decode(c["aux"], n, c["noise"], forced=forced, want_heads=True, variant=v))
        free = _np(c["net16"].decode(c["aux"], n, c["noise"], want_heads=True, variant=v))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, v)
        assert not np.array_equal(want[1], free[1])         # the forced input was read


# ------------------------------------------------------------------------------------------------- no silent fp32 fallback
@pytest.mark.parametrize("name", SMX)
def test_bf16_logits_differ_from_fp32_logits(gpu_ok, name):
    """rounding the three matrices moves the logits by about 4e-4 (CPU oracle): far outside the 2e-5 logits tolerance, so a
    mode that silently ran the fp32 weights would show here"""
    c = _case(name)
    forced = torch.full((c["B"], c["n_steps"]), c["cfg"].n_quantize // 2, dtype=torch.int32)    # same inputs for both
    _, h16 = c["net"].decode(c["aux"], c["n_steps"], c["noise"], forced=forced, want_heads=True, weights="bf16")
    _, h32 = c["net"].decode(c["aux"], c["n_steps"], c["noise"], forced=forced, want_heads=True)
    assert float((h16 - h32).abs().max()) > 2e-5, name


# ----------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("name", SMX + LAP)
def test_bf16_matches_the_cpu_oracle_on_rounded_weights(gpu_ok, name):
    """tolerances of tests/test_gpu_decode_parity.py: Laplace samples and heads <= 1e-5, softmax logits <= 2e-5 and
    indices equal (the oracle's top-2 margins on the rounded weights are >= 1.1e-3 over these steps)"""
    c = _case(name)
    cfg, B, n = c["cfg"], c["B"], c["n_steps"]
    P = cpu_ref.as_params(c["sd16"])
    v = _variants(cfg)[-1]
    out, heads = _np(c["net"].decode(c["aux"], n, c["noise"], want_heads=True, variant=v, seed=c["seed"], weights="bf16"))
    if cfg.kind == "softmax":
        want, ref_heads, _ = cpu_ref.softmax_generate(cfg, P, c["aux"], [n] * B, c["noise_sbw"], return_heads=True,
                                                      seed=c["seed"])
        ref_heads = np.transpose(np.asarray(ref_heads), (1, 0, 2))
        print(name, "max |logit - oracle|", np.abs(heads - ref_heads).max())
        assert np.abs(heads - ref_heads).max() <= 2e-5, name
        for b in range(B):
            assert np.array_equal(out[b], np.asarray(want[b])[:n]), (name, b)
    else:
        want, ref_heads = cpu_ref.laplace_generate(cfg, P, c["aux"], [n * cfg.seg] * B, c["noise_sbw"], return_heads=True,
                                                   seed=c["seed"])
        ref_heads = np.transpose(np.asarray(ref_heads), (1, 0, 2))
        print(name, "max |head - oracle|", np.abs(heads - ref_heads).max(), "max |sample - oracle|",
              max(np.abs(out[b] - want[b]).max() for b in range(B)))
        assert np.abs(heads - ref_heads).max() <= 1e-5, name
        for b in range(B):
            assert np.abs(out[b] - want[b]).max() <= 1e-5, (name, b)


# ---------------------------------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize("cfg,F", [(C.bl6_softmax(), 3), (C.bl6_laplace(5, 4), 10)], ids=["softmax", "lap_s5l4"])
def test_stream_chunks_concatenate_to_the_one_shot_decode(gpu_ok, cfg, F):
    """features in uneven pushes, then chunks of 37, 64, 100 steps and the remainder (across the 64-step noise staging)"""
    B = 2
    net = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=5, flavor="trained" if cfg.kind == "laplace" else "xavier"), DEV)
    aux = torch.from_numpy(synth_aux(cfg, B, F, seed=3)).to(DEV)
    N = F * cfg.U // _seg(cfg)
    assert 201 < N <= MAX_STEPS
    ref = net.decode(aux, N, want_heads=True, rng_seed=77, want_noise=True, weights="bf16")
    fp32 = net.decode(aux, N, want_heads=True, rng_seed=77, want_noise=True)
    assert not torch.equal(ref[1], fp32[1])
    s = DecodeStream(net, B, rng_seed=77, want_heads=True, want_noise=True, weights="bf16")
    cut = [1, F - 2] if F > 3 else [1, 1]
    f0 = 0
    for n in cut:
        s.push(aux[:, :, f0:f0 + n], generate=False)
        f0 += n
    s.finish(aux[:, :, f0:], generate=False)
    parts = [s.advance(n) for n in (37, 64, 100, N - 201)]
    assert s.steps_done == N
    for k, what in enumerate(("out", "heads", "noise")):
        assert torch.equal(torch.cat([p[k] for p in parts], 1), ref[k]), what


# ------------------------------------------------------------------------------------------------------------------- pool
def test_pool_sessions_equal_their_solo_streams(gpu_ok):
    """capacity 4, three sessions of different lengths, features in pushes of 3 and 7 frames, one tick after every push"""
    cfg = replace(C.bl6_softmax(), upsampling_factor=20)     # 10 .. 15 frames = 200 .. 300 steps per session
    sd = synth_state_dict(cfg, seed=5, flavor="xavier")
    net = HipNet.from_state_dict(cfg, sd, DEV)
    frames, ids = [10, 13, 15], [4, 9, 2]
    auxs = [torch.from_numpy(synth_aux(cfg, 1, f, seed=20 + i)).to(DEV) for i, f in enumerate(frames)]
    pool = DecodePool(net, 4, rng_seed=99, want_heads=True, weights="bf16")
    sess = [pool.open(utt_id=u) for u in ids]
    got = {s: [] for s in sess}
    at = [0, 0, 0]
    tick = 0
    while not all(s.done for s in sess):
        n = (3, 7)[tick % 2]
        tick += 1
        chunks, fin = {}, []
        for i, s in enumerate(sess):
            if s.finished:
                continue
            chunks[s] = auxs[i][:, :, at[i]:at[i] + n]
            at[i] += n
            if at[i] >= frames[i]:
                fin.append(s)
        pool.push_many(chunks, finish=fin)
        for s, r in pool.step().items():
            got[s].append((r[0], r[1]))
        assert tick < 16
    for i, s in enumerate(sess):
        solo = DecodeStream(net, 1, rng_seed=99, utt_ids=[ids[i]], want_heads=True, weights="bf16")
        o, h = solo.finish(auxs[i])
        assert o.shape[1] == frames[i] * cfg.U <= MAX_STEPS
        assert torch.equal(torch.cat([p[0] for p in got[s]], 1), o), i
        assert torch.equal(torch.cat([p[1] for p in got[s]], 1), h), i
    fp32 = DecodeStream(net, 1, rng_seed=99, utt_ids=[ids[0]], want_heads=True)
    assert not torch.equal(fp32.finish(auxs[0])[1], torch.cat([p[1] for p in got[sess[0]]], 1))
    with pytest.raises(ValueError, match="one model"):
        pool.add_model(HipNet.from_state_dict(cfg, sd, DEV))


# ----------------------------------------------------------------------------------------------------------------- repack
def test_image_follows_repack(gpu_ok):
    cfg = C.bl6_softmax()
    sd1 = synth_state_dict(cfg, seed=5, flavor="xavier")
    sd2 = synth_state_dict(cfg, seed=6, flavor="xavier")
    aux = torch.from_numpy(synth_aux(cfg, 1, 2, seed=3)).to(DEV)
    N = 2 * cfg.U
    net = HipNet.from_state_dict(cfg, sd1, DEV)
    first = net.decode(aux, N, want_heads=True, rng_seed=7, weights="bf16")
    net.repack([torch.from_numpy(sd2[k]).to(DEV) for k, _ in cfg.param_shapes()])
    again = net.decode(aux, N, want_heads=True, rng_seed=7, weights="bf16")
    fresh = HipNet.from_state_dict(cfg, sd2, DEV).decode(aux, N, want_heads=True, rng_seed=7, weights="bf16")
    assert torch.equal(again[0], fresh[0]) and torch.equal(again[1], fresh[1])
    assert not torch.equal(again[1], first[1])


# ----------------------------------------------------------------------------------------------------------------- driver
def test_driver_weights_flag_writes_the_wav_of_the_api_call(gpu_ok, tmp_path, monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        monkeypatch.delenv(k, raising=False)
    cfg = C.bl6_softmax()
    F = 3
    feats = tmp_path / "feats"
    feats.mkdir()
    h = np.random.default_rng(3).standard_normal((F, cfg.n_aux)).astype(np.float32)
    np.save(str(feats / "utt00.npy"), h)
    sd = synth_state_dict(cfg, seed=7, flavor="xavier")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, str(tmp_path / "checkpoint-1.pkl"))
    (tmp_path / "model.json").write_text(json.dumps(dict(cfg.to_dict(), string_path="/feat_org_lf0", audio_in=cfg.audio_in_flag)))
    argv = ["--feats", str(feats), "--checkpoint", str(tmp_path / "checkpoint-1.pkl"), "--config", str(tmp_path / "model.json"),
            "--fs", "22050", "--verbose", "0", "--seed", "5"]
    wavs, images = {}, []
    build_image = HipNet.decode_w16_image
    monkeypatch.setattr(HipNet, "decode_w16_image", lambda self: (images.append(1), build_image(self))[1])
    for tag, extra in (("bf16", ["--weights", "bf16"]), ("fp32", []), ("stream", ["--weights", "bf16", "--stream_frames", "2"]),
                       ("pool", ["--weights", "bf16", "--pool_slots", "2"])):
        del images[:]
        assert DD.main("softmax", argv + ["--outdir", str(tmp_path / tag)] + extra) == 0
        wavs[tag] = open(tmp_path / tag / "utt00.wav", "rb").read()
        assert bool(images) == (tag != "fp32"), tag        # the flag reached the decode calls of this path, and only with bf16
    # the API call the flag stands for: device noise keyed as the driver keys it, utterance 0 of the list
    key = _noise.draw_rng_seed(torch.Generator().manual_seed(5))
    net = HipNet.from_state_dict(cfg, sd, DEV)
    out, _ = net.decode(torch.from_numpy(h.T[None].copy()), F * cfg.U, rng_seed=key, utt_ids=[0], variant=6, weights="bf16")
    want = tmp_path / "want.wav"
    DD.write_wav_pcm16(str(want), np.clip(md.decode_mu_law(out[0].cpu().numpy().astype(np.int64), cfg.n_quantize), -1, 1), 22050)
    assert wavs["bf16"] == open(want, "rb").read()
    assert wavs["stream"] == wavs["bf16"] and wavs["pool"] == wavs["bf16"]
    # (the fp32 WAV may well be the same bytes: 240 sampled classes rarely notice logits that moved by 4e-4 - that the
    # mode reads rounded weights is shown on the logits above)
