"""GPU: the wave-specialised decode (csrc/swn_decode_bl6w.hip, variant 2) forms out_2 as per-wave partial sums in the out_1
phase, which the tail of every wave of group A adds in one fixed order, and starts the out_skip sums from their bias.  Both
change the order of partial sums: the samples and the heads against the symmetric kernel (variant 6) at 1e-5 over more than
three frames, free and teacher-forced, and streamed chunks of one and two steps bit-identical to the one-shot decode."""
import pytest
import torch

from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodeStream
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _setup(lpc, B, Tf, seed=31):
    cfg = C.bl6_laplace(1, lpc)
    sd = synth_state_dict(cfg, seed=seed, flavor="trained")
    net = HipNet.from_state_dict(cfg, sd, DEV)
    aux = torch.from_numpy(synth_aux(cfg, B, Tf, seed=seed + 1))
    return cfg, net, aux


@pytest.mark.parametrize("lpc", [0, 4])
def test_samples_and_heads_against_the_symmetric_kernel(gpu_ok, lpc):
    """3 U + 7 steps cross three conditioning frames; host-drawn noise (classic mode) and the in-kernel generator (extended
    mode), each free and teacher-forced"""
    cfg, net, aux = _setup(lpc, 2, 4)
    n = 3 * cfg.U + 7
    g = torch.Generator().manual_seed(11)
    forced = torch.empty(2, n).uniform_(-0.8, 0.8, generator=g)
    nz = torch.empty(2, n, 1).uniform_(-0.4999, 0.5, generator=g)
    for kw in (dict(noise=nz), dict(noise=nz, forced=forced), dict(noise=None, rng_seed=17),
               dict(noise=None, rng_seed=17, forced=forced)):
        o2, h2 = net.decode(aux, n, want_heads=True, variant=2, **kw)
        o6, h6 = net.decode(aux, n, want_heads=True, variant=6, **kw)
        assert o2.shape == o6.shape == (2, n) and h2.shape == h6.shape == (2, n, cfg.n_out)
        assert float((o2 - o6).abs().max()) <= 1e-5, (lpc, sorted(kw))
        assert float((h2 - h6).abs().max()) <= 1e-5, (lpc, sorted(kw))


@pytest.mark.parametrize("lpc", [0, 4])
def test_one_and_two_step_chunks_bit_identical(gpu_ok, lpc):
    """teacher-forced chunks of 1 and 2 steps across a frame crossing, then the rest in one piece: samples and heads
    bit-identical to the one-shot decode"""
    cfg, net, aux = _setup(lpc, 2, 3)
    aux = aux.to(DEV)
    N = 3 * cfg.U
    g = torch.Generator().manual_seed(12)
    forced = torch.empty(2, N).uniform_(-0.8, 0.8, generator=g).to(DEV)
    ref, ref_h = net.decode(aux, N, None, forced=forced, want_heads=True, variant=2, rng_seed=29)
    parts = [1, 2] * (cfg.U // 3 + 4)
    parts.append(N - sum(parts))
    assert parts[-1] > 0 and sum(parts[:-1]) > cfg.U
    s = DecodeStream(net, 2, variant=2, rng_seed=29, want_heads=True)
    s.push(aux, generate=False)
    s.finish(generate=False)
    outs, heads, k0 = [], [], 0
    for k in parts:
        o, h = s.advance(k, forced=forced[:, k0:k0 + k].contiguous())
        outs.append(o), heads.append(h)
        k0 += k
    assert torch.equal(torch.cat(outs, 1), ref)
    assert torch.equal(torch.cat(heads, 1), ref_h)
