"""GPU: the wave-specialised decode (csrc/swn_decode_bl6w.hip, variant 0 / 2) forms the next input layer in every wave of
group A and starts layer 0 without a barrier.  The places where that is delicate, against the symmetric kernel (variant 6)
and the CPU oracle: forced input, the in-kernel noise across its 64-step staging chunks, conditioning frame crossings, and
streamed chunks of one and two steps (each resumes from the session and forms h0 before its first layer 0)."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodeStream
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _setup(lpc, B, Tf, seed=21):
    cfg = C.bl6_laplace(1, lpc)
    sd = synth_state_dict(cfg, seed=seed, flavor="trained")
    net, P = HipNet.from_state_dict(cfg, sd, DEV), cpu_ref.as_params(sd)
    aux = torch.from_numpy(synth_aux(cfg, B, Tf, seed=seed + 1))
    return cfg, net, P, aux


@pytest.mark.parametrize("lpc", [0, 4])
def test_device_noise_across_chunks_and_frames(gpu_ok, lpc):
    """extended mode (in-kernel generator): three frames = 3 U steps cross two conditioning frames and five 64-step noise
    chunks; the noise the kernel used, replayed in the oracle and in the symmetric kernel, gives the same samples"""
    cfg, net, P, aux = _setup(lpc, 2, 3)
    n = 3 * cfg.U
    out, heads, used = net.decode(aux, n, None, want_heads=True, variant=2, rng_seed=123, want_noise=True)
    sym, hsym, used6 = net.decode(aux, n, None, want_heads=True, variant=6, rng_seed=123, want_noise=True)
    assert torch.equal(used, used6)
    assert float((out - sym).abs().max()) <= 1e-5 and float((heads - hsym).abs().max()) <= 1e-5
    want = cpu_ref.laplace_generate(cfg, P, aux, [n, n], used.permute(1, 0, 2).contiguous().cpu().numpy())
    for b in range(2):
        assert np.abs(out[b].cpu().numpy() - want[b][:n]).max() <= 1e-5, (lpc, b)


@pytest.mark.parametrize("lpc", [0, 4])
def test_forced_input_extended_and_classic(gpu_ok, lpc):
    """teacher-forced samples feed every wave's sample window: against the symmetric kernel in both noise modes (a seed
    waveform selects the extended instantiation) and the forced run's first step against the free run's"""
    cfg, net, P, aux = _setup(lpc, 2, 2)
    n = 2 * cfg.U
    g = torch.Generator().manual_seed(4)
    forced = torch.empty(2, n).uniform_(-0.8, 0.8, generator=g)
    nz = torch.empty(2, n, 1).uniform_(-0.4999, 0.5, generator=g)
    seed = torch.tensor([[0.25], [-0.5]])
    for kw in (dict(noise=nz), dict(noise=None, seed=seed, rng_seed=9)):
        f2, h2 = net.decode(aux, n, forced=forced, want_heads=True, variant=2, **kw)
        f6, h6 = net.decode(aux, n, forced=forced, want_heads=True, variant=6, **kw)
        assert float((f2 - f6).abs().max()) <= 1e-5 and float((h2 - h6).abs().max()) <= 1e-5
        free, _ = net.decode(aux, n, want_heads=True, variant=2, **kw)
        assert torch.equal(free[:, 0], f2[:, 0])
        assert float((free - f2).abs().max()) > 0.0             # the forced samples did reach the input layer


@pytest.mark.parametrize("lpc", [0, 4])
def test_stream_chunks_of_one_and_two_steps(gpu_ok, lpc):
    """chunks of 1 and 2 steps (a resume and the h0 formed from the restored window before each chunk's first layer 0),
    across a 64-step noise chunk and a frame crossing, then the rest in one piece: bit-identical to the one-shot decode"""
    cfg, net, _, aux = _setup(lpc, 2, 2)
    aux = aux.to(DEV)
    N = 2 * cfg.U
    ref, ref_h, ref_used = net.decode(aux, N, None, want_heads=True, variant=2, rng_seed=5, want_noise=True)
    parts = [1, 2] * 25 + [1] * 20
    parts.append(N - sum(parts))
    assert parts[-1] > 0 and sum(parts[:-1]) > 64
    s = DecodeStream(net, 2, variant=2, rng_seed=5, want_heads=True, want_noise=True)
    s.push(aux, generate=False)
    s.finish(generate=False)
    outs, heads, used = [], [], []
    for k in parts:
        o, h, u = s.advance(k)
        outs.append(o), heads.append(h), used.append(u)
    assert torch.equal(torch.cat(outs, 1), ref)
    assert torch.equal(torch.cat(heads, 1), ref_h)
    assert torch.equal(torch.cat(used, 1), ref_used)
