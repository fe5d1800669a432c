"""GPU: group B of the wave-specialised decode (csrc/swn_decode_bl6w.hip, variant 2) requests the out_skip weights as a rolling
stream - half a slice at a time, into the registers the multiply-adds of the slice before have just freed.  The pipeline starts
and drains inside every step, so the short decodes are pinned: 1, 2, 3, U - 1, U and U + 1 steps against the symmetric kernel
(variant 6) at 1e-5, the project's bar for the two kernels; chunks of one and two steps and a pool whose entries sit one step
apart, both bit-identical to the one-shot decode."""
import pytest
import torch

from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-5      # variant 2 against variant 6: same arithmetic per element up to the order of the partial sums


def _setup(lpc, B, Tf, seed=41):
    cfg = C.bl6_laplace(1, lpc)
    sd = synth_state_dict(cfg, seed=seed, flavor="trained")
    net = HipNet.from_state_dict(cfg, sd, DEV)
    aux = torch.from_numpy(synth_aux(cfg, B, Tf, seed=seed + 1))
    return cfg, net, aux


@pytest.mark.parametrize("teacher_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("extended", [False, True], ids=["classic", "extended"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_short_decodes_against_the_symmetric_kernel(gpu_ok, lpc, extended, teacher_forced):
    """two utterances; host-drawn noise (classic mode) or the in-kernel generator (extended mode); samples and heads"""
    cfg, net, aux = _setup(lpc, 2, 3)
    U = cfg.U
    for n in (1, 2, 3, U - 1, U, U + 1):
        g = torch.Generator().manual_seed(100 + n)
        kw = dict(noise=None, rng_seed=23) if extended else dict(noise=torch.empty(2, n, 1).uniform_(-0.4999, 0.5, generator=g))
        if teacher_forced:
            kw["forced"] = torch.empty(2, n).uniform_(-0.8, 0.8, generator=g)
        o2, h2 = net.decode(aux, n, want_heads=True, variant=2, **kw)
        o6, h6 = net.decode(aux, n, want_heads=True, variant=6, **kw)
        assert o2.shape == o6.shape == (2, n) and h2.shape == h6.shape == (2, n, cfg.n_out)
        eo, eh = float((o2 - o6).abs().max()), float((h2 - h6).abs().max())
        print(f"lpc {lpc} extended {extended} forced {teacher_forced} n_steps {n}: samples {eo:.3g} heads {eh:.3g}")
        assert bool(torch.isfinite(o2).all()) and bool(torch.isfinite(h2).all())
        assert eo <= BAR, (lpc, extended, teacher_forced, n, eo)
        assert eh <= BAR, (lpc, extended, teacher_forced, n, eh)


@pytest.mark.parametrize("lpc", [0, 4])
def test_chunks_of_one_and_two_steps_bit_identical(gpu_ok, lpc):
    """free-running chunks of 1, 2, 1, 2, ... steps from the first step across a frame crossing: every chunk edge resumes
    the slice pipeline from the session; samples and heads bit-identical to the one-shot decode"""
    cfg, net, aux = _setup(lpc, 2, 3)
    aux = aux.to(DEV)
    parts = [1, 2] * (cfg.U // 3 + 6)
    N = sum(parts)
    assert cfg.U + 12 < N <= 3 * cfg.U
    ref, ref_h = net.decode(aux, N, None, want_heads=True, variant=2, rng_seed=37)
    s = DecodeStream(net, 2, variant=2, rng_seed=37, want_heads=True)
    s.push(aux, generate=False)
    s.finish(generate=False)
    outs, heads = [], []
    for k in parts:
        o, h = s.advance(k)
        outs.append(o), heads.append(h)
    assert torch.equal(torch.cat(outs, 1), ref)
    assert torch.equal(torch.cat(heads, 1), ref_h)


@pytest.mark.parametrize("lpc", [0, 4])
def test_pool_entries_one_step_apart_bit_identical(gpu_ok, lpc):
    """four sessions admitted on successive ticks of one step each, then budgets of 1, 2, 3 steps in turn: the entries of
    every launch sit one step apart; each session bit-identical to the decode of its utterance alone"""
    cfg, net, _ = _setup(lpc, 1, 2)
    F, n_sess, key = 2, 4, 4243
    N = F * cfg.U
    auxs = [torch.from_numpy(synth_aux(cfg, 1, F, seed=200 + i)) for i in range(n_sess)]
    pool = DecodePool(net, n_sess, variant=2, rng_seed=key, want_heads=True)
    sess, got = [], {}
    tick = 0
    while len(sess) < n_sess or any(not s.done for s in sess):
        if len(sess) < n_sess:
            s = pool.open(utt_id=500 + len(sess))
            s.finish(auxs[len(sess)].to(DEV))
            sess.append(s)
            got[s] = ([], [])
        res = pool.step(1 if tick < 2 * n_sess else 1 + tick % 3)
        for s, r in res.items():
            got[s][0].append(r[0]), got[s][1].append(r[1])
        if tick == n_sess:
            assert [s.steps_done for s in sess] == [n_sess + 1 - i for i in range(n_sess)]
        tick += 1
        assert tick < 4 * N
    for i, s in enumerate(sess):
        assert s.steps_done == N
        ref, ref_h = net.decode(auxs[i].to(DEV), N, want_heads=True, variant=2, rng_seed=key, utt_ids=[500 + i])
        assert torch.equal(torch.cat(got[s][0], 1), ref), (lpc, i)
        assert torch.equal(torch.cat(got[s][1], 1), ref_h), (lpc, i)
