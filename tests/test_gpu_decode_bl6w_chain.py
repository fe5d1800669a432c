"""GPU: the wave-specialised decode (csrc/swn_decode_bl6w.hip, variant 2) forms a step's conditioning taps, its parity offset and
layer 0's row one step AHEAD (in the previous step's tail, primed in front of the step loop - also of a resumed chunk and of a
pool entry), hands h0 to layer 0 inside a wave without a wait, stores the sample and the heads behind the next input layer,
and refills the conditioning frame of a crossing at the head of the new frame's first step behind a flag that look-ahead
left.  A tap of the wrong frame, a refill into a buffer still read, a primed value that does not match the step a chunk
resumes at, or a look-ahead that reads what it may not changes a sample.  Pinned here with FOUR frames (U = 110: 440 steps; with
two frames the refill never runs behind the one-time loads): one-shot decodes whose lengths end one step before, at and one step
behind every frame edge, and at 1, 2 and 440 steps, against the symmetric kernel (variant 6) at 1e-5, the project's bar for the
two kernels, samples and heads, free-running and teacher-forced; the prefix property of those lengths against the 440-step
decode, bit for bit; streams in chunks that end one step before, at and one step behind each crossing, and one of single steps
across a crossing (steps 108-112), bit-identical to the one-shot decode and to a one-chunk stream, the session they leave
included; a pool of two sessions admitted one step apart, run across all three crossings, each equal to its one-shot decode;
classic against extended mode on one host-drawn noise stream over 221 steps, bit for bit.  Two utterances, lpc 0 and 4,
synthetic weights and features."""
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
TF = 4          # frames: the refill of a crossing runs for frames 2 and 3 (both buffers), and is suppressed in the last frame
LENGTHS = (1, 2, 109, 110, 111, 219, 220, 221, 329, 330, 331, 440)
N_MAX = LENGTHS[-1]
# chunks ending one step before, at and one step behind each crossing (110, 220, 330); single steps 108 .. 112
STREAMS = ((109, 1, 1, 109, 110, 1, 109), (110, 110, 110, 110), (111, 108, 2, 109, 110), (329, 1, 1, 109),
           (108, 1, 1, 1, 1, 1, 327))
POOL_TICKS = (1, 108, 1, 1, 109, 110, 1, 109)   # the first session stands at 1, 109, 110, 111, 220, 330, 331, 440 steps
SESS_RINGS = (2 + 4 + 8 + 16 + 32 + 64) * 64    # Tw::sess_old: the six history rings
SESS_WIN = SESS_RINGS + 2 * 6 * 128             # Tw::sess_win: behind both parities of the older-tap products


@functools.lru_cache(maxsize=None)
def _setup(lpc, B=2, seed=71):
    cfg = C.bl6_laplace(1, lpc)
    sd = synth_state_dict(cfg, seed=seed, flavor="trained")
    net = HipNet.from_state_dict(cfg, sd, DEV)
    aux = torch.from_numpy(synth_aux(cfg, B, TF, seed=seed + 1)).to(DEV)
    assert cfg.U == 110 and TF * cfg.U == N_MAX
    assert all(sum(c) == N_MAX for c in STREAMS) and sum(POOL_TICKS) == N_MAX
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
    """the classic variant-2 decode of n steps (computed once, shared by the tests below, left unchanged)"""
    cfg, net, aux = _setup(lpc)
    noise, forced = _streams(teacher_forced, 500 + lpc)
    return _decode(net, aux, n, noise, forced, 2)


@functools.lru_cache(maxsize=None)
def _oneshot_ext(lpc):
    """the extended-mode one-shot decode the streams are compared with, and a one-chunk stream over the same utterances"""
    cfg, net, aux = _setup(lpc)
    ref = net.decode(aux, N_MAX, None, want_heads=True, variant=2, rng_seed=73)
    return ref, _stream(lpc, (N_MAX,))


def _stream(lpc, chunks):
    cfg, net, aux = _setup(lpc)
    s = DecodeStream(net, 2, variant=2, rng_seed=73, want_heads=True)
    s.push(aux, generate=False)
    s.finish(generate=False)
    res = [s.advance(k) for k in chunks]
    return torch.cat([r[0] for r in res], 1), torch.cat([r[1] for r in res], 1), s._session


def _session_words(sess, n_utt, lpc):
    """what the kernel writes of each utterance's session: rings, older-tap products, the sample window (its padding is not)"""
    wn = max(1, lpc) + 1
    return sess.view(n_utt, -1)[:, :SESS_WIN + wn]


@pytest.mark.parametrize("teacher_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_frame_edges_against_the_symmetric_kernel(gpu_ok, lpc, teacher_forced):
    """classic mode (host-drawn noise), free-running and teacher-forced; samples and heads"""
    cfg, net, aux = _setup(lpc)
    noise, forced = _streams(teacher_forced, 500 + lpc)
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
    """the decode of n steps equals the first n samples and heads of the 440-step decode: the look-ahead of the step behind the
    last one - at 109, 219 and 329 steps a crossing - changes nothing that was decoded"""
    ref, ref_h = _decode2(lpc, teacher_forced, N_MAX)
    for n in LENGTHS:
        o, h = _decode2(lpc, teacher_forced, n)
        assert torch.equal(o, ref[:, :n]), (lpc, teacher_forced, n)
        assert torch.equal(h, ref_h[:, :n]), (lpc, teacher_forced, n)


@pytest.mark.parametrize("chunks", STREAMS, ids=["-".join(map(str, c)) for c in STREAMS])
@pytest.mark.parametrize("lpc", [0, 4])
def test_stream_chunks_around_the_crossings_bit_identical_session_included(gpu_ok, lpc, chunks):
    """a resumed chunk primes its first step's taps, row and frame counters from its own step0: every chunking equals the
    one-shot decode and the one-chunk stream, and leaves the one-chunk stream's session"""
    (ref, ref_h), (o1, h1, sess1) = _oneshot_ext(lpc)
    assert torch.equal(o1, ref) and torch.equal(h1, ref_h)
    o, h, sess = _stream(lpc, chunks)
    assert torch.equal(o, ref), (lpc, chunks)
    assert torch.equal(h, ref_h), (lpc, chunks)
    assert torch.equal(_session_words(sess, 2, lpc), _session_words(sess1, 2, lpc)), (lpc, chunks)


@pytest.mark.parametrize("lpc", [0, 4])
def test_pool_entries_one_step_apart_across_the_crossings(gpu_ok, lpc):
    """two sessions admitted one tick - one step - apart: the entries of every launch sit one step apart, on either side of
    each crossing; each session equals the decode of its utterance alone, and its slot of the pool's session buffer that of a
    one-chunk stream over the utterance (decode_bl6w_pool_kernel)"""
    cfg, net, _ = _setup(lpc)
    n_sess, key = 2, 7193
    auxs = [torch.from_numpy(synth_aux(cfg, 1, TF, seed=900 + i)).to(DEV) for i in range(n_sess)]
    pool = DecodePool(net, n_sess, variant=2, rng_seed=key, want_heads=True)
    sess, got = [], {}
    tick = 0
    while len(sess) < n_sess or any(not s.done for s in sess):
        if len(sess) < n_sess:
            s = pool.open(utt_id=970 + len(sess))
            s.finish(auxs[len(sess)])
            sess.append(s)
            got[s] = ([], [])
        for s, r in pool.step(POOL_TICKS[tick % len(POOL_TICKS)]).items():
            got[s][0].append(r[0]), got[s][1].append(r[1])
        tick += 1
        if tick == 2:
            assert [s.steps_done for s in sess] == [109, 108]
        if tick == 3:
            assert [s.steps_done for s in sess] == [110, 109]      # on either side of the first crossing
        assert tick < 2 * len(POOL_TICKS)
    assert tick == len(POOL_TICKS) + 1          # the second session ends one tick after the first
    slots = _session_words(pool._session, n_sess, lpc)
    for i, s in enumerate(sess):
        assert s.steps_done == N_MAX
        ref, ref_h = net.decode(auxs[i], N_MAX, want_heads=True, variant=2, rng_seed=key, utt_ids=[970 + i])
        assert torch.equal(torch.cat(got[s][0], 1), ref), (lpc, i)
        assert torch.equal(torch.cat(got[s][1], 1), ref_h), (lpc, i)
        one = DecodeStream(net, 1, variant=2, rng_seed=key, utt_ids=[970 + i], want_heads=True)
        one.push(auxs[i], generate=False)
        one.finish(generate=False)
        o1, _ = one.advance(N_MAX)
        assert torch.equal(o1, ref), (lpc, i)
        assert torch.equal(slots[s.slot], _session_words(one._session, 1, lpc)[0]), (lpc, i)


@pytest.mark.parametrize("lpc", [0, 4])
def test_classic_and_extended_agree_on_one_stream_bit_for_bit(gpu_ok, lpc):
    """the extended instantiation replays a host-drawn stream when the caller also asks for the noise dump: over 221 steps
    (one past the second crossing) both modes decode the same samples and heads"""
    cfg, net, aux = _setup(lpc)
    noise, _ = _streams(False, 500 + lpc)
    n = 221
    oc, hc = _decode2(lpc, False, n)
    oe, he, used = _decode(net, aux, n, noise, None, 2, want_noise=True)
    assert torch.equal(used.cpu(), noise[:, :n])
    assert torch.equal(oc, oe) and torch.equal(hc, he)
