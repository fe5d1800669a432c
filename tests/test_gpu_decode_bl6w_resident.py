"""GPU: the wave-specialised decode (csrc/swn_decode_bl6w.hip, variant 2) keeps slice 0 of out_skip RESIDENT in group B's
registers - loaded once in front of the step loop, of a pool entry's own model - and runs group A's step loop ROTATED by the
stores: the sample and the heads of a step are stored in the next step, behind layer 0's LDS reads, together with the refill
test and the noise staging; the last step's stores follow the loop.  A resident slice of the wrong model, a slice consumed
in the wrong phase, a store of the wrong step or a store lost at the end of a launch or of a chunk changes a sample.  Pinned here
on BL6 Laplace seg 1 (U = 110), lpc 0 and 4, classic and extended mode, two utterances, synthetic weights and features:
one-shot decodes of 1, 2, 3, U - 1, U, U + 1, U + 2 and 2U + 1 steps against the CPU oracle (samples) and the symmetric
kernel, variant 6 (samples and heads), at 1e-5, the bar of the existing tests of this kernel - the store behind the loop, the
first and the last rotated step, a refill on a launch's last step and on the step before it; the same lengths teacher-forced,
against variant 6; streams in chunks of 1 and 2 steps and in chunks that end on and one step past a frame crossing, bit-identical
to the one-shot decode and, session included, to the one-chunk stream; a pool of three sessions one step apart, of one model
and of two models with different weights, each session bit-identical to its own solo stream, session slot included.
The classic lpc 0 kernel is the one built in this form (it alone is faster with it); the extended kernels and lpc 4 keep the
earlier loop, and the same cases pin them, so the form can be switched on for them without a new test.
(FOUR conditioning frames: a decode of 2U + 1 steps needs three - the library rejects more steps than the conditioning
holds - and with four the refill of a crossing runs at steps U and 2U.)"""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-5      # variant 2 against variant 6 and the oracle: the bar of the existing tests of the wave-specialised kernel
U = 110
TF = 4
LENGTHS = (1, 2, 3, U - 1, U, U + 1, U + 2, 2 * U + 1)
N_MAX = LENGTHS[-1]
# chunks of 1 and 2 steps at the start and at the crossing; a chunk ending on the crossing (U) and one step past it (U + 1)
STREAMS = ((1, 2, 1, U - 4, U + 1), (2, 1, U - 3, 1, 2, 1, U - 3), (U + 1, 1, 2, U - 3), (U - 1, 1, 1, 1, U - 1))
POOL_TICKS = (1, 1, U - 3, 1, 1, 1, U - 2, 1, 1, 2 * U - 2)   # the first session stands at 1, 2, 109, 110, 111, 112, 220, 221, 222, 440
SESS_RINGS = (2 + 4 + 8 + 16 + 32 + 64) * 64    # Tw::sess_old: the six history rings
SESS_WIN = SESS_RINGS + 2 * 6 * 128             # Tw::sess_win: behind both parities of the older-tap products


@functools.lru_cache(maxsize=None)
def _net(lpc, seed=83):
    cfg = C.bl6_laplace(1, lpc)
    assert cfg.U == U and all(sum(c) == N_MAX for c in STREAMS) and sum(POOL_TICKS) == TF * U
    sd = synth_state_dict(cfg, seed=seed, flavor="trained")
    return cfg, sd, HipNet.from_state_dict(cfg, sd, DEV)


@functools.lru_cache(maxsize=None)
def _inputs(lpc):
    """features, the host-drawn noise of N_MAX steps in the oracle's draw order, and teacher-forced inputs (a decode of n steps
    takes their first n)"""
    cfg, _, _ = _net(lpc)
    aux = torch.from_numpy(synth_aux(cfg, 2, TF, seed=84))
    g = torch.Generator().manual_seed(600 + lpc)
    noise_o = cpu_ref.laplace_noise(cfg, N_MAX, 2, generator=g)                    # (steps, B, seg)
    noise = torch.from_numpy(noise_o).permute(1, 0, 2).contiguous()                # (B, steps, seg)
    forced = torch.empty(2, N_MAX).uniform_(-0.8, 0.8, generator=g)
    return aux, noise_o, noise, forced


@functools.lru_cache(maxsize=None)
def _oracle(lpc):
    """the CPU oracle's N_MAX samples of both utterances (generation is causal: a decode of n steps is their first n)"""
    cfg, sd, _ = _net(lpc)
    aux, noise_o, _, _ = _inputs(lpc)
    ref = cpu_ref.laplace_generate(cfg, cpu_ref.as_params(sd), aux, [N_MAX, N_MAX], noise_o)
    return torch.from_numpy(np.stack([np.asarray(ref[b])[:N_MAX] for b in range(2)]).astype(np.float32))


def _decode(lpc, n, variant, extended, teacher_forced):
    _, _, net = _net(lpc)
    aux, _, noise, forced = _inputs(lpc)
    kw = {"forced": forced[:, :n].contiguous()} if teacher_forced else {}
    if extended:        # the extended instantiation replays a host-drawn stream when the caller also asks for the noise dump
        o, h, used = net.decode(aux.to(DEV), n, noise[:, :n].contiguous(), want_heads=True, variant=variant, want_noise=True, **kw)
        assert torch.equal(used.cpu(), noise[:, :n])
        return o.cpu(), h.cpu()
    o, h = net.decode(aux.to(DEV), n, noise[:, :n].contiguous(), want_heads=True, variant=variant, **kw)
    return o.cpu(), h.cpu()


@pytest.mark.parametrize("extended", [False, True], ids=["classic", "extended"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_oneshot_lengths_against_the_oracle_and_the_symmetric_kernel(gpu_ok, lpc, extended):
    cfg, _, _ = _net(lpc)
    ref = _oracle(lpc)
    for n in LENGTHS:
        o2, h2 = _decode(lpc, n, 2, extended, False)
        o6, h6 = _decode(lpc, n, 6, extended, False)
        assert o2.shape == o6.shape == (2, n) and h2.shape == h6.shape == (2, n, cfg.n_out)
        assert bool(torch.isfinite(o2).all()) and bool(torch.isfinite(h2).all())
        er, eo, eh = float((o2 - ref[:, :n]).abs().max()), float((o2 - o6).abs().max()), float((h2 - h6).abs().max())
        print(f"lpc {lpc} extended {extended} n_steps {n}: oracle {er:.3g} variant 6 samples {eo:.3g} heads {eh:.3g}")
        assert er <= BAR, (lpc, extended, n, er)
        assert eo <= BAR, (lpc, extended, n, eo)
        assert eh <= BAR, (lpc, extended, n, eh)


@pytest.mark.parametrize("extended", [False, True], ids=["classic", "extended"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_forced_lengths_with_heads_against_the_symmetric_kernel(gpu_ok, lpc, extended):
    """teacher-forced: the forced load of a step is older than that step's stores, which now leave one step later; the free
    samples and the heads are stored as before"""
    cfg, _, _ = _net(lpc)
    full, full_h = _decode(lpc, N_MAX, 2, extended, True)
    for n in LENGTHS:
        o2, h2 = _decode(lpc, n, 2, extended, True)
        o6, h6 = _decode(lpc, n, 6, extended, True)
        assert o2.shape == o6.shape == (2, n) and h2.shape == h6.shape == (2, n, cfg.n_out)
        eo, eh = float((o2 - o6).abs().max()), float((h2 - h6).abs().max())
        print(f"lpc {lpc} extended {extended} forced n_steps {n}: samples {eo:.3g} heads {eh:.3g}")
        assert bool(torch.isfinite(o2).all()) and bool(torch.isfinite(h2).all())
        assert eo <= BAR, (lpc, extended, n, eo)
        assert eh <= BAR, (lpc, extended, n, eh)
        # every step's stores arrive, the last one's from behind the loop: a shorter decode is the longer one's prefix
        assert torch.equal(o2, full[:, :n]) and torch.equal(h2, full_h[:, :n]), (lpc, extended, n)


@functools.lru_cache(maxsize=None)
def _oneshot_ext(lpc):
    """the one-shot decode on the device generator the streams are compared with, and a one-chunk stream over the same utterances"""
    _, _, net = _net(lpc)
    aux = _inputs(lpc)[0].to(DEV)
    ref = net.decode(aux, N_MAX, None, want_heads=True, variant=2, rng_seed=91)
    return ref, _stream(lpc, (N_MAX,))


def _stream(lpc, chunks):
    _, _, net = _net(lpc)
    s = DecodeStream(net, 2, variant=2, rng_seed=91, want_heads=True)
    s.push(_inputs(lpc)[0].to(DEV), generate=False)
    s.finish(generate=False)
    res = [s.advance(k) for k in chunks]
    return torch.cat([r[0] for r in res], 1), torch.cat([r[1] for r in res], 1), s._session


def _session_words(sess, n_utt, lpc):
    """what the kernel writes of each utterance's session: rings, older-tap products, the sample window (its padding is not)"""
    wn = max(1, lpc) + 1
    return sess.view(n_utt, -1)[:, :SESS_WIN + wn]


@pytest.mark.parametrize("chunks", STREAMS, ids=["-".join(map(str, c)) for c in STREAMS])
@pytest.mark.parametrize("lpc", [0, 4])
def test_stream_chunks_bit_identical_session_included(gpu_ok, lpc, chunks):
    """a chunk's last step stores behind the loop and in front of the session copy; a resumed chunk reloads the resident slice"""
    (ref, ref_h), (o1, h1, sess1) = _oneshot_ext(lpc)
    assert torch.equal(o1, ref) and torch.equal(h1, ref_h)
    o, h, sess = _stream(lpc, chunks)
    assert torch.equal(o, ref), (lpc, chunks)
    assert torch.equal(h, ref_h), (lpc, chunks)
    assert torch.equal(_session_words(sess, 2, lpc), _session_words(sess1, 2, lpc)), (lpc, chunks)


@pytest.mark.parametrize("two_models", [False, True], ids=["one_model", "two_models"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_pool_of_three_entries_one_step_apart(gpu_ok, lpc, two_models):
    """three sessions admitted one tick - one step - apart; with two models the middle one runs a model whose weights - slice 0 of
    out_skip among them - differ from the pool's own, in the same launches.  Each session equals its own solo stream bit for
    bit, samples, heads and session slot: a workgroup that kept the wrong model's slice fails here"""
    cfg, _, net0 = _net(lpc)
    nets = [net0, _net(lpc, seed=97)[2]] if two_models else [net0]
    if two_models:
        a, b = (n.packed.cpu() for n in nets)
        assert a.shape == b.shape and not torch.equal(a, b)
    n_sess, key, n_all = 3, 8117, TF * U
    model_of = [0, len(nets) - 1, 0]
    auxs = [torch.from_numpy(synth_aux(cfg, 1, TF, seed=910 + i)).to(DEV) for i in range(n_sess)]
    pool = DecodePool(nets[0], n_sess, variant=2, rng_seed=key, want_heads=True)
    if two_models:
        assert pool.add_model(nets[1]) == 1
    sess, got = [], {}
    tick = 0
    while len(sess) < n_sess or any(not s.done for s in sess):
        if len(sess) < n_sess:
            s = pool.open(utt_id=930 + len(sess), model=model_of[len(sess)])
            s.finish(auxs[len(sess)])
            sess.append(s)
            got[s] = ([], [])
        for s, r in pool.step(POOL_TICKS[tick % len(POOL_TICKS)]).items():
            got[s][0].append(r[0].clone()), got[s][1].append(r[1].clone())
        tick += 1
        if tick == 3:
            assert [s.steps_done for s in sess] == [U - 1, U - 2, U - 3]
        if tick == 5:
            assert [s.steps_done for s in sess] == [U + 1, U, U - 1]     # on either side of the first crossing
        assert tick < 2 * len(POOL_TICKS)
    slots = _session_words(pool._session, n_sess, lpc)
    for i, s in enumerate(sess):
        assert s.steps_done == n_all
        one = DecodeStream(nets[model_of[i]], 1, variant=2, rng_seed=key, utt_ids=[930 + i], want_heads=True)
        one.push(auxs[i], generate=False)
        one.finish(generate=False)
        o1, h1 = one.advance(n_all)
        assert torch.equal(torch.cat(got[s][0], 1), o1), (lpc, two_models, i)
        assert torch.equal(torch.cat(got[s][1], 1), h1), (lpc, two_models, i)
        assert torch.equal(slots[s.slot], _session_words(one._session, 1, lpc)[0]), (lpc, two_models, i)
