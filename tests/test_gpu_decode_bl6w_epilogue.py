"""GPU: the wave-specialised decode (csrc/swn_decode_bl6w.hip, variant 2) finishes a layer's gate in one straight-line
epilogue - no branch around the transcendentals for a saturated tanh lane -, group B reads all four input quads of an
out_skip slice at the head of its phase, and group A (lpc 0) requests half the operands of layer 5's older-tap product in
front of barrier 5.  Pinned here with FOUR frames (U = 110: 440 steps), two utterances, lpc 0 and 4, synthetic weights and
features:
* saturating gates: the candidate rows (64 .. 127) of every dil_h conv and their biases scaled up (SCALE), so that tanh lanes
  saturate in fp32 (|v| > 9.02, where the parent's branch returned +-1) while others stay in the curved part (1 < |v| < 9.02).
  The candidate pre-activations of the teacher-forced inputs are formed on the host with the oracle's layer arithmetic; all
  are finite and at least 5 % lie in either range.  Variant 2 against the symmetric kernel (variant 6, which keeps the
  branch) and against the CPU oracle at 1e-5, samples and heads, free-running and teacher-forced;
* unscaled weights: variant 2 against variant 6 at 1e-5 for lengths 1, 2, 63, 64, 65 and 440 (the noise chunk pass of every
  64th step shares the step with the early reads) and 32, 33, 34 (the early operand row h_4(q - 31) is the prologue's
  until step 31);
* streams in chunks of (1, 1, 438), (31, 1, 1, 407) and (64, 64, 312) and a pool of two sessions admitted one step apart,
  bit-identical to the one-shot extended decode, the session included;
* classic against extended mode on one host-drawn noise stream, bit for bit.

SCALE = (weights, biases) is chosen on the CPU alone, from the shares and from the reference's own error (the fp32 oracle
against the same oracle in float64, which bounds what a 1e-5 comparison against it can mean).  ONE factor for rows and
biases cannot serve: the saturated share needs it above 32 (4.7 % at 32, 6.5 % at 36), and from 16 on it turns the recurrent
net into an amplifier of rounding errors - the oracle's own free-running samples are 4.6e-7 from float64 at 8, 1.1e-5 at
16, 0.39 at 24 and 0.78 at 36, its teacher-forced heads 1.3e-5 at 36 - so no implementation, the oracle itself included,
compares at 1e-5 there.  What saturates a lane is the size of the pre-activation, not its gain on the hidden state, so the
rows are scaled by 2 and the biases by 500: v is then dominated by bias x conditioning, which moves with the frame and the
channel.  Shares on the host (lpc 0 and 4 alike): 12 % saturated (11 - 16 % in every layer), 60 % curved, max |v| 46;
3 % / 7.6 % / 21 % saturated at biases x 300 / 400 / 700.  The oracle's own error at (2, 500) is what it is at the unscaled
weights: teacher-forced heads 3.5e-6 (unscaled 3.4e-6), free-running heads 3.7e-6 (4.6e-6), samples below 1e-6."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-5      # the project's bar: variant 2 against variant 6 and against the oracle
TF = 4
N_MAX = 440
SCALE = (2.0, 500.0)   # candidate rows, candidate biases of every dil_h conv
SAT = 9.02      # above it tanh is +-1 in fp32: exp(-2 |v|) < 2^-25
LENGTHS = (1, 2, 32, 33, 34, 63, 64, 65, N_MAX)
STREAMS = ((1, 1, 438), (31, 1, 1, 407), (64, 64, 312))
POOL_TICKS = (1, 30, 1, 1, 1, 406)              # the first session stands at 1, 31, 32, 33, 34 and 440 steps
SESS_RINGS = (2 + 4 + 8 + 16 + 32 + 64) * 64    # Tw::sess_old: the six history rings
SESS_WIN = SESS_RINGS + 2 * 6 * 128             # Tw::sess_win: behind both parities of the older-tap products


def _state_dict(cfg, scale, seed=71):
    sd = {k: np.array(v, copy=True) for k, v in synth_state_dict(cfg, seed=seed, flavor="trained").items()}
    if scale is not None:
        for l in range(cfg.L):
            sd[f"dil_h.{l}.conv.weight"][cfg.H:] *= np.float32(scale[0])
            sd[f"dil_h.{l}.conv.bias"][cfg.H:] *= np.float32(scale[1])
    return sd


@functools.lru_cache(maxsize=None)
def _setup(lpc, scale=None, seed=71):
    cfg = C.bl6_laplace(1, lpc)
    sd = _state_dict(cfg, scale, seed)
    net = HipNet.from_state_dict(cfg, sd, DEV)
    aux = torch.from_numpy(synth_aux(cfg, 2, TF, seed=seed + 1))
    assert cfg.U == 110 and TF * cfg.U == N_MAX and cfg.receptive_field == 64
    assert all(sum(c) == N_MAX for c in STREAMS) and sum(POOL_TICKS) == N_MAX
    return cfg, net, aux.to(DEV), cpu_ref.as_params(sd), aux


@functools.lru_cache(maxsize=None)
def _inputs(lpc):
    """the host-drawn noise of N_MAX steps and the teacher-forced inputs; a decode of n steps takes their first n"""
    g = torch.Generator().manual_seed(500 + lpc)
    noise = torch.empty(2, N_MAX, 1).uniform_(-0.4999, 0.5, generator=g)
    forced = torch.empty(2, N_MAX).uniform_(-0.8, 0.8, generator=g)
    return noise, forced


def _decode(net, aux, n, noise, forced, variant, **kw):
    if forced is not None:
        kw["forced"] = forced[:, :n].contiguous()
    return net.decode(aux, n, noise[:, :n].contiguous(), want_heads=True, variant=variant, **kw)


@functools.lru_cache(maxsize=None)
def _decode2(lpc, teacher_forced, n, scale=None):
    """the classic variant-2 decode of n steps (computed once, shared by the tests below, left unchanged)"""
    cfg, net, aux, _, _ = _setup(lpc, scale)
    noise, forced = _inputs(lpc)
    return _decode(net, aux, n, noise, forced if teacher_forced else None, 2)


def _forced_on_host(cfg, P, aux, forced, noise):
    """the teacher-forced decode on the host with the oracle's layer arithmetic: step i of the decode is position rf + i of
    the stack over [rf + 1 zeros, the forced samples] and the replicate-padded conditioning (cpu_ref.laplace_generate).
    Returns the candidate pre-activations (B, L, H, n), the heads (B, n, n_out) and the samples (B, n)."""
    rf, (B, n), lpc = cfg.receptive_field, forced.shape, cfg.lpc
    with torch.no_grad():
        x = cpu_ref.upsample(cfg, P, cpu_ref.frontend(cfg, P, aux))
        x = F.pad(x, (rf, 0), "replicate")[:, :, :rf + n]
        fed = torch.cat((torch.zeros(B, rf + 1), forced), 1)        # what the input layer and the LP window see
        h = F.softsign(cpu_ref.causal_conv(cpu_ref._lift(cfg, P, fed[:, None, :rf + n]), P["causal.conv.weight"],
                                           P["causal.conv.bias"], 1))
        pre, tot = [], None
        for l in range(cfg.L):
            a = cpu_ref.causal_conv(h, P[f"dil_h.{l}.conv.weight"], P[f"dil_h.{l}.conv.bias"], cfg.dilations[l])
            g = F.conv1d(x, P[f"in_x.{l}.weight"], P[f"in_x.{l}.bias"]) * a
            pre.append(g[:, cfg.H:, rf:])
            sk, h = cpu_ref.gated_layer(cfg, P, l, x, h)
            tot = sk if tot is None else tot + sk
        o = cpu_ref.head(cfg, P, tot)[:, :, rf:].transpose(1, 2)     # B, n, n_out
        mu, b = o[:, :, 0], torch.exp(F.logsigmoid(o[:, :, 1]))
        e = noise[:, :n, 0]
        s = mu - b * e.sign() * torch.log1p(-2 * e.abs())
        if lpc > 0:
            win = fed[:, rf + 1 - lpc: rf + n].unfold(1, lpc, 1)      # B, n, lpc: the lpc samples in front of step i
            s = (o[:, :, 2:].flip(-1) * win).sum(-1) + mu - b * e.sign() * torch.log1p(-2 * e.abs())
        return torch.stack(pre, 1), o.contiguous(), torch.clamp(s, min=-1, max=1)


@functools.lru_cache(maxsize=None)
def _oracle_forced(lpc, scale):
    cfg, _, _, P, aux = _setup(lpc, scale)
    noise, forced = _inputs(lpc)
    return _forced_on_host(cfg, P, aux, forced, noise)


@functools.lru_cache(maxsize=None)
def _oracle_free(lpc, scale):
    cfg, _, _, P, aux = _setup(lpc, scale)
    noise, _ = _inputs(lpc)
    out, heads = cpu_ref.laplace_generate(cfg, P, aux, [N_MAX, N_MAX], noise.permute(1, 0, 2).contiguous().numpy(),
                                          return_heads=True)
    return torch.from_numpy(np.stack(out)), torch.from_numpy(heads).permute(1, 0, 2).contiguous()


@pytest.mark.parametrize("lpc", [0, 4])
def test_scaled_weights_saturate_and_curve_on_the_host(gpu_ok, lpc):
    """the oracle alone: every candidate pre-activation of the teacher-forced inputs is finite, at least 5 % of (layer,
    channel, step) are saturated in fp32 and at least 5 % lie in the curved part of tanh"""
    pre, _, _ = _oracle_forced(lpc, SCALE)
    assert pre.shape == (2, 6, 64, N_MAX)
    assert bool(torch.isfinite(pre).all())
    av = pre.abs()
    sat, mid = float((av > SAT).float().mean()), float(((av > 1.0) & (av < SAT)).float().mean())
    print(f"lpc {lpc} scale {SCALE}: |v| > {SAT}: {sat:.4f}, 1 < |v| < {SAT}: {mid:.4f}, max |v| {float(av.max()):.3g}")
    assert sat >= 0.05 and mid >= 0.05, f"saturated share {sat:.4f}, curved share {mid:.4f} (both >= 0.05 wanted)"


@pytest.mark.parametrize("teacher_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_saturating_gates_against_the_symmetric_kernel_and_the_oracle(gpu_ok, lpc, teacher_forced):
    cfg, net, aux, _, _ = _setup(lpc, SCALE)
    noise, forced = _inputs(lpc)
    o2, h2 = _decode2(lpc, teacher_forced, N_MAX, SCALE)
    o6, h6 = _decode(net, aux, N_MAX, noise, forced if teacher_forced else None, 6)
    if teacher_forced:
        _, hr, orf = _oracle_forced(lpc, SCALE)
    else:
        orf, hr = _oracle_free(lpc, SCALE)
    assert o2.shape == o6.shape == orf.shape == (2, N_MAX) and h2.shape == h6.shape == hr.shape == (2, N_MAX, cfg.n_out)
    assert bool(torch.isfinite(o2).all()) and bool(torch.isfinite(h2).all())
    e6 = float((o2 - o6).abs().max()), float((h2 - h6).abs().max())
    er = float((o2.cpu() - orf).abs().max()), float((h2.cpu() - hr).abs().max())
    print(f"lpc {lpc} forced {teacher_forced}: against variant 6 samples {e6[0]:.3g} heads {e6[1]:.3g}; "
          f"against the oracle samples {er[0]:.3g} heads {er[1]:.3g}")
    assert max(e6) <= BAR, (lpc, teacher_forced, e6)
    assert max(er) <= BAR, (lpc, teacher_forced, er)


@pytest.mark.parametrize("teacher_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("lpc", [0, 4])
def test_unscaled_lengths_against_the_symmetric_kernel(gpu_ok, lpc, teacher_forced):
    """classic mode (host-drawn noise); samples and heads"""
    cfg, net, aux, _, _ = _setup(lpc)
    noise, forced = _inputs(lpc)
    for n in LENGTHS:
        o2, h2 = _decode2(lpc, teacher_forced, n)
        o6, h6 = _decode(net, aux, n, noise, forced if teacher_forced else None, 6)
        assert o2.shape == o6.shape == (2, n) and h2.shape == h6.shape == (2, n, cfg.n_out)
        eo, eh = float((o2 - o6).abs().max()), float((h2 - h6).abs().max())
        print(f"lpc {lpc} forced {teacher_forced} n_steps {n}: samples {eo:.3g} heads {eh:.3g}")
        assert bool(torch.isfinite(o2).all()) and bool(torch.isfinite(h2).all())
        assert eo <= BAR, (lpc, teacher_forced, n, eo)
        assert eh <= BAR, (lpc, teacher_forced, n, eh)


@functools.lru_cache(maxsize=None)
def _oneshot_ext(lpc):
    """the extended-mode one-shot decode the streams are compared with, and a one-chunk stream over the same utterances"""
    cfg, net, aux, _, _ = _setup(lpc)
    ref = net.decode(aux, N_MAX, None, want_heads=True, variant=2, rng_seed=73)
    return ref, _stream(lpc, (N_MAX,))


def _stream(lpc, chunks):
    cfg, net, aux, _, _ = _setup(lpc)
    s = DecodeStream(net, 2, variant=2, rng_seed=73, want_heads=True)
    s.push(aux, generate=False)
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
    """every early read is issued and used inside one step: a chunk that ends after 1, 2, 31, 32, 33, 64 or 128 steps leaves
    nothing outstanding, and the next one primes nothing - samples, heads and the session equal the one-shot decode's"""
    (ref, ref_h), (o1, h1, sess1) = _oneshot_ext(lpc)
    assert torch.equal(o1, ref) and torch.equal(h1, ref_h)
    o, h, sess = _stream(lpc, chunks)
    assert torch.equal(o, ref), (lpc, chunks)
    assert torch.equal(h, ref_h), (lpc, chunks)
    assert torch.equal(_session_words(sess, 2, lpc), _session_words(sess1, 2, lpc)), (lpc, chunks)


@pytest.mark.parametrize("lpc", [0, 4])
def test_pool_entries_one_step_apart(gpu_ok, lpc):
    """two sessions admitted one tick - one step - apart (decode_bl6w_pool_kernel): each equals the decode of its utterance
    alone, and its slot of the pool's session buffer that of a one-chunk stream over the utterance"""
    cfg, net, _, _, _ = _setup(lpc)
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
            assert [s.steps_done for s in sess] == [31, 30]
        if tick == 3:
            assert [s.steps_done for s in sess] == [32, 31]      # on either side of the last step the prologue's row serves
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
    """the extended instantiation replays a host-drawn stream when the caller also asks for the noise dump: both modes
    decode the same samples and heads"""
    cfg, net, aux, _, _ = _setup(lpc)
    noise, _ = _inputs(lpc)
    oc, hc = _decode2(lpc, False, N_MAX)
    oe, he, used = _decode(net, aux, N_MAX, noise, None, 2, want_noise=True)
    assert torch.equal(used.cpu(), noise)
    assert torch.equal(oc, oe) and torch.equal(hc, he)
