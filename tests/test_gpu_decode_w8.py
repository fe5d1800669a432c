"""GPU: decode with FP8 (OCP E4M3) storage of the streamed head matrices (weights="e4m3").

The W8 instantiations of the symmetric BL6 kernel widen every streamed code to exactly code x 2^-e_row in fp32 and run the
fp32 kernel's FMAs in its order, so the mode is pinned WITHOUT a tolerance: weights="e4m3" on a model W equals, bit for bit,
the fp32 symmetric kernel on e4m3_weight_state_dict(W).  The code-table test pins the conversion itself (OCP, not FNUZ; the
scaled conversion exact for power-of-two scales); the other tests show that the mode really reads quantised weights (no silent
fp32 or bf16 fallback), that the CPU oracle on the dequantised state dict agrees at the tolerances of
tests/test_gpu_decode_parity.py, and that streams, pools, repack and the decode driver carry the mode.  Every decode here runs
at most 300 steps at B <= 3."""
import ctypes
import functools
import json
from dataclasses import replace

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import cpu_ref
from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import decode_driver as DD
from shallow_wavenet_amd import noise as _noise
from shallow_wavenet_amd.nets import dswnv as md
from shallow_wavenet_amd.runtime import HipNet, e4m3_quantise, e4m3_values, e4m3_weight_state_dict
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
    """fixture -> everything the tests share: the model W with the mode on, the fp32 model on the dequantised weights, the
    fixture's inputs cut to MAX_STEPS steps (host noise in the kernels' layout, the seed where the fixture has one)"""
    cfg, d = load_golden(name)
    sd = synth_state_dict(cfg, seed=int(d["wseed"]), flavor=str(d["flavor"]))
    sd8 = e4m3_weight_state_dict(cfg, sd)
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
    return dict(cfg=cfg, sd=sd, sd8=sd8, aux=aux, B=B, n_steps=n_steps, noise_sbw=noise,
                noise=torch.from_numpy(np.ascontiguousarray(noise)).permute(1, 0, 2).contiguous(), seed=seed,
                net=HipNet.from_state_dict(cfg, sd, DEV), net8=HipNet.from_state_dict(cfg, sd8, DEV))


def _np(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


# ----------------------------------------------------------------------------------------------------------- code table
@pytest.mark.parametrize("log2_scale", [0, -9, 7, -100])
def test_e4m3_table_equals_the_host_table_bit_for_bit(gpu_ok, log2_scale):
    """all 256 codes through the kernels' own conversion helper at a power-of-two scale: the host table (the format's
    definition) times the scale, exact in fp32; NaN codes compared as NaN.  FNUZ would read code 0x80 as NaN and every exponent
    one binade lower."""
    scale = float(np.ldexp(np.float32(1), log2_scale))
    got = torch.ops.swn.e4m3_table(torch.empty(1, device=DEV), scale).cpu().numpy()
    want = (e4m3_values().astype(np.float64) * 2.0 ** log2_scale).astype(np.float32)
    nan = np.isnan(want)
    assert nan.sum() == 2 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32)).ravel()[:8]
    assert got.view(np.uint32)[0x80] == 0x80000000 and got[0] == 0 and got.view(np.uint32)[0] == 0    # the zeros keep their signs


# ---------------------------------------------------------------------------------------------------------------- image
def _numpy_image(cfg, sd):
    """code sections [NS / 4][rows][4 lanes][4 words], byte s of word j of lane p of row r in slice group g =
    code(W[r, 64 g + 16 s + 4 p + j]): out_skip (per layer), out_1, softmax out_2; then the fp32 2^-e of every row, in that order"""
    mats = [sd[f"out_skip.{l}.weight"][:, :, 0] for l in range(cfg.L)] + [sd["out_1.weight"][:, :, 0]]
    if cfg.kind == "softmax":
        mats.append(sd["out_2.weight"][:, :, 0])
    words, scales = [], []
    for w in mats:
        codes, e = e4m3_quantise(w)
        rows, n_in = codes.shape
        b = codes.reshape(rows, n_in // 64, 4, 4, 4).astype(np.uint32)           # row, group g, slice s, lane, j
        word = b[:, :, 0] | (b[:, :, 1] << 8) | (b[:, :, 2] << 16) | (b[:, :, 3] << 24)
        words.append(word.transpose(1, 0, 2, 3).reshape(-1))
        scales.append(np.ldexp(np.float32(1), -e).astype(np.float32))
    return np.concatenate([np.concatenate(words).view(np.uint8), np.concatenate(scales).view(np.uint8)])


@pytest.mark.parametrize("cfg", [C.bl6_laplace(5, 4), C.bl6_laplace(2, 4), C.bl6_softmax()], ids=["lap_s5l4", "lap_s2l4", "softmax"])
def test_device_built_image_equals_numpy(gpu_ok, cfg):
    sd = {k: v.copy() for k, v in synth_state_dict(cfg, seed=11, flavor="trained" if cfg.kind == "laplace" else "xavier").items()}
    # rows the synthetic weights do not have: all zero, tiny enough for the clamp, amax on the 0.875 boundary, exact ties
    w = sd["out_1.weight"]
    w[3] = 0.0
    w[4] *= np.float32(2.0 ** -110)
    w[5, :4, 0] = [0.875 * 2.0 ** -5, -0.0, 17 * 2.0 ** -14, 1.5 * 2.0 ** -23]
    w[5, 4:] = 0.0
    net = HipNet.from_state_dict(cfg, sd, DEV)
    got = net.decode_w8_image().cpu().numpy()
    want = _numpy_image(cfg, sd)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert got.size == _lib.lib().swn_decode_w8_bytes(ctypes.byref(_lib.desc_from_cfg(cfg)))
    assert np.array_equal(got, want), np.argwhere(got != want).ravel()[:8]


def test_packer_refuses_a_weight_that_is_not_finite(gpu_ok):
    cfg = C.bl6_laplace(5, 4)
    sd = {k: v.copy() for k, v in synth_state_dict(cfg, seed=11, flavor="trained").items()}
    sd["out_skip.2.weight"][7, 3, 0] = np.inf
    net = HipNet.from_state_dict(cfg, sd, DEV)
    with pytest.raises(RuntimeError, match="pack_decode_w8"):
        net.decode_w8_image()
    with pytest.raises(ValueError, match="not finite"):
        e4m3_weight_state_dict(cfg, sd)


# ----------------------------------------------------------------------------------------------------------- bit-identity
@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("name", SMX + LAP)
def test_e4m3_equals_fp32_kernel_on_dequantised_weights(gpu_ok, name, source):
    c = _case(name)
    noise = c["noise"] if source == "host" else None
    for v in _variants(c["cfg"]):
        kw = dict(want_heads=True, variant=v, seed=c["seed"], rng_seed=RNG, rng_utt0=3, want_noise=True)
        got = _np(c["net"].decode(c["aux"], c["n_steps"], noise, weights="e4m3", **kw))
        want = _np(c["net8"].decode(c["aux"], c["n_steps"], noise, **kw))
        for g, w, what in zip(got, want, ("out", "heads", "noise")):
            assert g.shape == w.shape and np.array_equal(g, w), (name, source, v, what)
        if source == "host":
            assert np.array_equal(got[2], c["noise"].numpy())


@pytest.mark.parametrize("name", ["g1_bl6_softmax_b1", "g1_bl6_lap_s5l4_b1_trained"])
def test_e4m3_equals_fp32_kernel_teacher_forced(gpu_ok, name):
    c = _case(name)
    cfg, B, n = c["cfg"], c["B"], c["n_steps"]
    rng = np.random.default_rng(5)
    if cfg.kind == "softmax":
        forced = torch.from_numpy(rng.integers(0, cfg.n_quantize, (B, n)).astype(np.int32))
    else:
        forced = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, n * cfg.seg)).astype(np.float32))
    for v in _variants(cfg):
        got = _np(c["net"].decode(c["aux"], n, c["noise"], forced=forced, want_heads=True, variant=v, weights="e4m3"))
        want = _np(c["net8"].decode(c["aux"], n, c["noise"], forced=forced, want_heads=True, variant=v))
        free = _np(c["net8"].decode(c["aux"], n, c["noise"], want_heads=True, variant=v))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, v)
        assert not np.array_equal(want[1], free[1])         # the forced input was read


# ------------------------------------------------------------------------------------------ no silent fp32 / bf16 fallback
@pytest.mark.parametrize("name", SMX)
def test_e4m3_logits_differ_from_fp32_and_bf16_logits(gpu_ok, name):
    """three fraction bits move a weight by up to 2^-4 of itself, 2^4 times what bf16 rounding moves it: the logits leave the
    fp32 model's and the bf16 mode's by far more than the 2e-5 logits tolerance, so a mode that silently ran either would show"""
    c = _case(name)
    forced = torch.full((c["B"], c["n_steps"]), c["cfg"].n_quantize // 2, dtype=torch.int32)    # same inputs for all
    _, h8 = c["net"].decode(c["aux"], c["n_steps"], c["noise"], forced=forced, want_heads=True, weights="e4m3")
    _, h16 = c["net"].decode(c["aux"], c["n_steps"], c["noise"], forced=forced, want_heads=True, weights="bf16")
    _, h32 = c["net"].decode(c["aux"], c["n_steps"], c["noise"], forced=forced, want_heads=True)
    print(name, "max |e4m3 - fp32|", float((h8 - h32).abs().max()), "max |e4m3 - bf16|", float((h8 - h16).abs().max()))
    assert float((h8 - h32).abs().max()) > 2e-5, name
    assert float((h8 - h16).abs().max()) > 2e-5, name


# ----------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("name", SMX + LAP)
def test_e4m3_matches_the_cpu_oracle_on_dequantised_weights(gpu_ok, name):
    """tolerances of tests/test_gpu_decode_parity.py: Laplace samples and heads <= 1e-5, softmax logits <= 2e-5 and
    indices equal"""
    c = _case(name)
    cfg, B, n = c["cfg"], c["B"], c["n_steps"]
    P = cpu_ref.as_params(c["sd8"])
    v = _variants(cfg)[-1]
    out, heads = _np(c["net"].decode(c["aux"], n, c["noise"], want_heads=True, variant=v, seed=c["seed"], weights="e4m3"))
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
    ref = net.decode(aux, N, want_heads=True, rng_seed=77, want_noise=True, weights="e4m3")
    fp32 = net.decode(aux, N, want_heads=True, rng_seed=77, want_noise=True)
    assert not torch.equal(ref[1], fp32[1])
    s = DecodeStream(net, B, rng_seed=77, want_heads=True, want_noise=True, weights="e4m3")
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
    pool = DecodePool(net, 4, rng_seed=99, want_heads=True, weights="e4m3")
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
        solo = DecodeStream(net, 1, rng_seed=99, utt_ids=[ids[i]], want_heads=True, weights="e4m3")
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
    first = net.decode(aux, N, want_heads=True, rng_seed=7, weights="e4m3")
    net.repack([torch.from_numpy(sd2[k]).to(DEV) for k, _ in cfg.param_shapes()])
    again = net.decode(aux, N, want_heads=True, rng_seed=7, weights="e4m3")
    fresh = HipNet.from_state_dict(cfg, sd2, DEV).decode(aux, N, want_heads=True, rng_seed=7, weights="e4m3")
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
    build_image = HipNet.decode_w8_image
    monkeypatch.setattr(HipNet, "decode_w8_image", lambda self: (images.append(1), build_image(self))[1])
    for tag, extra in (("e4m3", ["--weights", "e4m3"]), ("fp32", []), ("stream", ["--weights", "e4m3", "--stream_frames", "2"]),
                       ("pool", ["--weights", "e4m3", "--pool_slots", "2"])):
        del images[:]
        assert DD.main("softmax", argv + ["--outdir", str(tmp_path / tag)] + extra) == 0
        wavs[tag] = open(tmp_path / tag / "utt00.wav", "rb").read()
        assert bool(images) == (tag != "fp32"), tag        # the flag reached the decode calls of this path, and only with e4m3
    # the API call the flag stands for: device noise keyed as the driver keys it, utterance 0 of the list
    key = _noise.draw_rng_seed(torch.Generator().manual_seed(5))
    net = HipNet.from_state_dict(cfg, sd, DEV)
    out, _ = net.decode(torch.from_numpy(h.T[None].copy()), F * cfg.U, rng_seed=key, utt_ids=[0], variant=6, weights="e4m3")
    want = tmp_path / "want.wav"
    DD.write_wav_pcm16(str(want), np.clip(md.decode_mu_law(out[0].cpu().numpy().astype(np.int64), cfg.n_quantize), -1, 1), 22050)
    assert wavs["e4m3"] == open(want, "rb").read()
    assert wavs["stream"] == wavs["e4m3"] and wavs["pool"] == wavs["e4m3"]
