"""GPU: the wave-specialised decode (csrc/swn_decode_bl6w.hip, variant 2) stages the classic mode's deviates in 64-step chunks
(one wave of group A, lane = step, an LDS ring of four chunks written two chunks ahead of its reader), and group A forms layer 5's
older-tap product of position q + 1 in the skip-fin phase while group B forms the other five.  Pinned here: the chunk edges of the
noise ring (1, 63, 64, 65, 127, 128, 129 and 193 steps) against the symmetric kernel (variant 6) at 1e-5, the project's bar for the
two kernels; the prefix property of the classic decode, bit for bit; classic against extended on one noise stream, bit for bit; and
a stream and a pool advanced across dilation 32, the wrap of layer 5's 64-slot ring and a frame crossing, bit-identical to the
one-shot decode.  Two utterances of two frames (U = 110: 220 steps), lpc 0 and 4, synthetic weights and features."""
import functools

import pytest
import torch

from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-5      # variant 2 against variant 6: same arithmetic per element up to the order of the partial sums
EDGES = (1, 63, 64, 65, 127, 128, 129, 193)     # around every edge of the 64-step chunks, and into the ring's fourth chunk
N_MAX = EDGES[-1]
CHUNKS = (31, 1, 32, 33, 64, 59)                # across dilation 32, the 64-slot ring wrap and the frame crossing at 110


@functools.lru_cache(maxsize=None)
def _setup(lpc, B=2, Tf=2, seed=41):
    cfg = C.bl6_laplace(1, lpc)
    sd = synth_state_dict(cfg, seed=seed, flavor="trained")
    net = HipNet.from_state_dict(cfg, sd, DEV)
    aux = torch.from_numpy(synth_aux(cfg, B, Tf, seed=seed + 1)).to(DEV)
    assert cfg.U == 110 and sum(CHUNKS) == Tf * cfg.U
    return cfg, net, aux


def _streams(teacher_forced, seed):
    """the host-drawn noise of N_MAX steps (and the teacher-forced inputs); a decode of n steps takes their first n"""
    g = torch.Generator().manual_seed(seed)
    noise = torch.empty(2, N_MAX, 1).uniform_(-0.4999, 0.5, generator=g)
    forced = torch.empty(2, N_MAX).uniform_(-0.8, 0.8, generator=g) if teacher_forced else None
    return noise, forced


def _decode(net, aux, n, noise, forced, variant, **kw):
    if forced is not None:
        kw["forced"] = forced[:, :n].contiguous()
    return net.decode(aux, n, noise[:, :n].contiguous(), want_heads=True, variant=variant, **kw)


@pytest.mark.parametrize("teacher_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_noise_ring_chunk_edges_against_the_symmetric_kernel(gpu_ok, lpc, teacher_forced):
    """classic mode (host-drawn noise), free-running and teacher-forced; samples and heads"""
    cfg, net, aux = _setup(lpc)
    noise, forced = _streams(teacher_forced, 300 + lpc)
    for n in EDGES:
        o2, h2 = _decode(net, aux, n, noise, forced, 2)
        o6, h6 = _decode(net, aux, n, noise, forced, 6)
        assert o2.shape == o6.shape == (2, n) and h2.shape == h6.shape == (2, n, cfg.n_out)
        eo, eh = float((o2 - o6).abs().max()), float((h2 - h6).abs().max())
        print(f"lpc {lpc} forced {teacher_forced} n_steps {n}: samples {eo:.3g} heads {eh:.3g}")
        assert bool(torch.isfinite(o2).all()) and bool(torch.isfinite(h2).all())
        assert eo <= BAR, (lpc, teacher_forced, n, eo)
        assert eh <= BAR, (lpc, teacher_forced, n, eh)


@pytest.mark.parametrize("teacher_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_classic_decode_prefix_property_bit_for_bit(gpu_ok, lpc, teacher_forced):
    """the classic decode of n steps over the first n deviates equals the first n samples and heads of the 193-step decode:
    a slip of the staging ring (a deviate of another step, a chunk read before it is written) shows here even inside 1e-5"""
    cfg, net, aux = _setup(lpc)
    noise, forced = _streams(teacher_forced, 310 + lpc)
    ref, ref_h = _decode(net, aux, N_MAX, noise, forced, 2)
    for n in EDGES:
        o, h = _decode(net, aux, n, noise, forced, 2)
        assert torch.equal(o, ref[:, :n]), (lpc, teacher_forced, n)
        assert torch.equal(h, ref_h[:, :n]), (lpc, teacher_forced, n)


@pytest.mark.parametrize("lpc", [0, 4])
def test_classic_and_extended_agree_on_one_stream_bit_for_bit(gpu_ok, lpc):
    """the extended instantiation replays a host-drawn stream when the caller also asks for the noise dump (or gives a seed
    waveform): over 129 steps both modes decode the same samples and heads, and the dump is the stream"""
    cfg, net, aux = _setup(lpc)
    noise, _ = _streams(False, 320 + lpc)
    n = 129
    oc, hc = _decode(net, aux, n, noise, None, 2)
    oe, he, used = _decode(net, aux, n, noise, None, 2, want_noise=True)
    assert torch.equal(used.cpu(), noise[:, :n])
    assert torch.equal(oc, oe) and torch.equal(hc, he)
    os_, hs = _decode(net, aux, n, noise, None, 2, seed=torch.zeros(2, 1))
    assert torch.equal(oc, os_) and torch.equal(hc, hs)


@pytest.mark.parametrize("lpc", [0, 4])
def test_stream_across_ring_and_frame_edges_bit_identical(gpu_ok, lpc):
    """a stream advanced by 31, 1, 32, 33, 64 and 59 steps: every chunk's first step takes layer 5's older-tap product from
    the session, where group A left it in the last step of the chunk before"""
    cfg, net, aux = _setup(lpc)
    N = sum(CHUNKS)
    ref, ref_h = net.decode(aux, N, None, want_heads=True, variant=2, rng_seed=53)
    s = DecodeStream(net, 2, variant=2, rng_seed=53, want_heads=True)
    s.push(aux, generate=False)
    s.finish(generate=False)
    outs, heads = [], []
    for k in CHUNKS:
        o, h = s.advance(k)
        outs.append(o), heads.append(h)
    assert torch.equal(torch.cat(outs, 1), ref)
    assert torch.equal(torch.cat(heads, 1), ref_h)


@pytest.mark.parametrize("lpc", [0, 4])
def test_pool_across_ring_and_frame_edges_bit_identical(gpu_ok, lpc):
    """three sessions admitted one tick apart, budgets of 31, 1, 32, 33, 64, 59, ... steps per tick: the entries of a launch sit
    at different phases of the ring and the frame; each session bit-identical to the decode of its utterance alone"""
    cfg, net, _ = _setup(lpc)
    F, n_sess, key = 2, 3, 5153
    N = F * cfg.U
    auxs = [torch.from_numpy(synth_aux(cfg, 1, F, seed=700 + i)).to(DEV) for i in range(n_sess)]
    pool = DecodePool(net, n_sess, variant=2, rng_seed=key, want_heads=True)
    sess, got = [], {}
    tick = 0
    while len(sess) < n_sess or any(not s.done for s in sess):
        if len(sess) < n_sess:
            s = pool.open(utt_id=900 + len(sess))
            s.finish(auxs[len(sess)])
            sess.append(s)
            got[s] = ([], [])
        for s, r in pool.step(CHUNKS[tick % len(CHUNKS)]).items():
            got[s][0].append(r[0]), got[s][1].append(r[1])
        tick += 1
        assert tick < 4 * len(CHUNKS)
    assert tick == len(CHUNKS) + 2              # the last session ends two ticks after the first
    for i, s in enumerate(sess):
        assert s.steps_done == N
        ref, ref_h = net.decode(auxs[i], N, want_heads=True, variant=2, rng_seed=key, utt_ids=[900 + i])
        assert torch.equal(torch.cat(got[s][0], 1), ref), (lpc, i)
        assert torch.equal(torch.cat(got[s][1], 1), ref_h), (lpc, i)
