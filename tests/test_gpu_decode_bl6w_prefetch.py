"""GPU: the wave-specialised decode (csrc/swn_decode_bl6w.hip, variant 2) requests LDS rows that do not depend on a barrier in
front of it (lds_barrier_keep): in skip-fin, behind its hand-off write, group B asks for the operand rows of the three older-tap
products it forms in the out_1 phase, and group A (lpc 0) for the first out_1 weights, which it then reads rolled, one block
ahead.  A row read before its writer, or a hand-off write not retired at the barrier, changes a sample.  Pinned here, where an
early read can go wrong: one-shot decodes of 1, 2, 3, 109, 110, 111 and 193 steps (the first steps behind the prologue, the
frame crossing at U = 110) against the symmetric kernel (variant 6) at 1e-5, the project's bar for the two kernels,
samples and heads; the prefix property of those lengths, bit for bit (a check, not a proof: the hazard table in
DESIGN.md 3.1 is the argument); a stream in chunks of 1, 1, 2, 31, 32, 33, 64 and 56 steps and a pool whose two entries start one
step apart, both bit-identical to the one-shot decode, the session they leave included (a resume in front of every early read,
across dilation 32, the wrap of layer 5's 64-slot ring and the frame edge); classic against extended mode on one noise stream,
bit for bit.  Two utterances of two frames (U = 110: 220 steps), lpc 0 and 4, synthetic weights and features."""
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
LENGTHS = (1, 2, 3, 109, 110, 111, 193)         # the first steps behind the prologue, around the frame edge, into the second frame
N_MAX = LENGTHS[-1]
CHUNKS = (1, 1, 2, 31, 32, 33, 64, 56)          # a resume in front of every early read; dilation 32, the 64-slot wrap, the frame edge
SESS_RINGS = (2 + 4 + 8 + 16 + 32 + 64) * 64    # Tw::sess_old: the six history rings
SESS_WIN = SESS_RINGS + 2 * 6 * 128             # Tw::sess_win: behind both parities of the older-tap products


@functools.lru_cache(maxsize=None)
def _setup(lpc, B=2, Tf=2, seed=61):
    cfg = C.bl6_laplace(1, lpc)
    sd = synth_state_dict(cfg, seed=seed, flavor="trained")
    net = HipNet.from_state_dict(cfg, sd, DEV)
    aux = torch.from_numpy(synth_aux(cfg, B, Tf, seed=seed + 1)).to(DEV)
    assert cfg.U == 110 and sum(CHUNKS) == Tf * cfg.U
    return cfg, net, aux


@functools.lru_cache(maxsize=None)
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


@functools.lru_cache(maxsize=None)
def _decode2(lpc, teacher_forced, n):
    """the classic variant-2 decode of n steps (computed once, shared by the two tests below, left unchanged)"""
    cfg, net, aux = _setup(lpc)
    noise, forced = _streams(teacher_forced, 400 + lpc)
    return _decode(net, aux, n, noise, forced, 2)


def _session_words(sess, n_utt, lpc):
    """what the kernel writes of each utterance's session: rings, older-tap products, the sample window (its padding is not)"""
    wn = max(1, lpc) + 1
    return sess.view(n_utt, -1)[:, :SESS_WIN + wn]


@pytest.mark.parametrize("teacher_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_first_steps_and_frame_edge_against_the_symmetric_kernel(gpu_ok, lpc, teacher_forced):
    """classic mode (host-drawn noise), free-running and teacher-forced; samples and heads"""
    cfg, net, aux = _setup(lpc)
    noise, forced = _streams(teacher_forced, 400 + lpc)
    for n in LENGTHS:
        o2, h2 = _decode2(lpc, teacher_forced, n)
        o6, h6 = _decode(net, aux, n, noise, forced, 6)
        assert o2.shape == o6.shape == (2, n) and h2.shape == h6.shape == (2, n, cfg.n_out)
        eo, eh = float((o2 - o6).abs().max()), float((h2 - h6).abs().max())
        print(f"lpc {lpc} forced {teacher_forced} n_steps {n}: samples {eo:.3g} heads {eh:.3g}")
        assert bool(torch.isfinite(o2).all()) and bool(torch.isfinite(h2).all())
        assert eo <= BAR, (lpc, teacher_forced, n, eo)
        assert eh <= BAR, (lpc, teacher_forced, n, eh)


@pytest.mark.parametrize("teacher_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_prefix_property_bit_for_bit(gpu_ok, lpc, teacher_forced):
    """the decode of n steps equals the first n samples and heads of the 193-step decode: a row requested before its writer
    has stored it depends on what a longer decode leaves there later"""
    ref, ref_h = _decode2(lpc, teacher_forced, N_MAX)
    for n in LENGTHS:
        o, h = _decode2(lpc, teacher_forced, n)
        assert torch.equal(o, ref[:, :n]), (lpc, teacher_forced, n)
        assert torch.equal(h, ref_h[:, :n]), (lpc, teacher_forced, n)


@pytest.mark.parametrize("lpc", [0, 4])
def test_classic_and_extended_agree_on_one_stream_bit_for_bit(gpu_ok, lpc):
    """the extended instantiation replays a host-drawn stream when the caller also asks for the noise dump: over 111 steps
    (one past the frame edge) both modes decode the same samples and heads"""
    cfg, net, aux = _setup(lpc)
    noise, _ = _streams(False, 400 + lpc)
    n = 111
    oc, hc = _decode2(lpc, False, n)
    oe, he, used = _decode(net, aux, n, noise, None, 2, want_noise=True)
    assert torch.equal(used.cpu(), noise[:, :n])
    assert torch.equal(oc, oe) and torch.equal(hc, he)


@pytest.mark.parametrize("lpc", [0, 4])
def test_stream_in_chunks_bit_identical_session_included(gpu_ok, lpc):
    """a stream advanced by 1, 1, 2, 31, 32, 33, 64 and 56 steps against the one-shot decode, and the session it leaves against
    that of a stream advanced by all 220 steps at once"""
    cfg, net, aux = _setup(lpc)
    N = sum(CHUNKS)
    ref, ref_h = net.decode(aux, N, None, want_heads=True, variant=2, rng_seed=67)

    def stream(chunks):
        s = DecodeStream(net, 2, variant=2, rng_seed=67, want_heads=True)
        s.push(aux, generate=False)
        s.finish(generate=False)
        res = [s.advance(k) for k in chunks]
        return torch.cat([r[0] for r in res], 1), torch.cat([r[1] for r in res], 1), s._session

    o1, h1, sess1 = stream((N,))
    assert torch.equal(o1, ref) and torch.equal(h1, ref_h)
    o, h, sess = stream(CHUNKS)
    assert torch.equal(o, ref)
    assert torch.equal(h, ref_h)
    assert torch.equal(_session_words(sess, 2, lpc), _session_words(sess1, 2, lpc))


@pytest.mark.parametrize("lpc", [0, 4])
def test_pool_entries_one_step_apart_bit_identical_session_included(gpu_ok, lpc):
    """two sessions admitted one tick - one step - apart, budgets of 1, 1, 2, 31, 32, 33, 64, 56, 1 steps per tick: the entries of
    every launch sit one step apart; each session equals the decode of its utterance alone, and its slot of the pool's session
    buffer that of a one-chunk stream over the utterance"""
    cfg, net, _ = _setup(lpc)
    F, n_sess, key = 2, 2, 6173
    N = F * cfg.U
    auxs = [torch.from_numpy(synth_aux(cfg, 1, F, seed=800 + i)).to(DEV) for i in range(n_sess)]
    pool = DecodePool(net, n_sess, variant=2, rng_seed=key, want_heads=True)
    sess, got = [], {}
    tick = 0
    while len(sess) < n_sess or any(not s.done for s in sess):
        if len(sess) < n_sess:
            s = pool.open(utt_id=950 + len(sess))
            s.finish(auxs[len(sess)])
            sess.append(s)
            got[s] = ([], [])
        for s, r in pool.step(CHUNKS[tick % len(CHUNKS)]).items():
            got[s][0].append(r[0]), got[s][1].append(r[1])
        tick += 1
        if tick == 2:
            assert [s.steps_done for s in sess] == [2, 1]
        assert tick < 2 * len(CHUNKS)
    assert tick == len(CHUNKS) + 1              # the second session ends one tick after the first
    slots = _session_words(pool._session, n_sess, lpc)
    for i, s in enumerate(sess):
        assert s.steps_done == N
        ref, ref_h = net.decode(auxs[i], N, want_heads=True, variant=2, rng_seed=key, utt_ids=[950 + i])
        assert torch.equal(torch.cat(got[s][0], 1), ref), (lpc, i)
        assert torch.equal(torch.cat(got[s][1], 1), ref_h), (lpc, i)
        one = DecodeStream(net, 1, variant=2, rng_seed=key, utt_ids=[950 + i], want_heads=True)
        one.push(auxs[i], generate=False)
        one.finish(generate=False)
        o1, _ = one.advance(N)
        assert torch.equal(o1, ref), (lpc, i)
        assert torch.equal(slots[s.slot], _session_words(one._session, 1, lpc)[0]), (lpc, i)
