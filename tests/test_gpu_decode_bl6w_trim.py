"""GPU: group A's trimmed chain in the wave-specialised decode (csrc/swn_decode_bl6w.hip, variant 2), classic lpc 0 kernel.
The changes take instructions off the chain without touching a multiply-add, an operand or a summation order.  Built:
  * lanes of odd position in their quad load the gate and the candidate row swapped at launch, so the quad reduction takes the
    partial sums without a select;
  * the gate epilogue runs on all four lanes of the quad with no exec mask, and the lanes that own no channel store to a dump
    word of their own in a 1 KB tail of the LDS carve.
Behind build switches that are off (measured slower), and covered by the same cases when they are on:
  * layer l + 1 takes its highway operand - the `hn` the same thread wrote to ring l + 1 one phase earlier - from a register,
    not back from LDS (layers 1 - 5, the prologue too);
  * a launch without forced inputs runs a copy of the kernel whose tail has no forced load, wait or select and which forms the
    next input layer behind the last step too.
A highway operand from the wrong layer, rows left unswapped in the odd lanes, a dump word outside the carve or over a live one,
or a forced sample ignored, changes every sample from the first steps on.
Pinned here through the C entry point on caller-owned buffers pre-filled with NaN, on the BL6 Laplace seg 1 net (U = 110) with the
`trained` synthetic weights, four conditioning frames, three utterances per call:
  * one-shot decodes of 1, 2, 3, 4, 5, 9, 17, 33 (every ring's wrap: the first step sits at position 63, the last slot of
    every ring), 63, 64, 65, 66, 129, 130 (the 64-step noise pass), U - 1, U, U + 1, 2U + 1, 3U + 1 steps (the frame
    crossings) - each length also ends on the last step;
  * variant 2 against the CPU oracle (samples, free-running) and against the symmetric kernel, variant 6 (samples and heads),
    at 1e-5 - the bar the existing tests of this kernel hold on these shapes -, free-running and teacher-forced with heads;
  * no NaN left in `out` or `heads`, and the guard words on either side of both buffers untouched;
  * the dynamic LDS the launch asks for, through swn_decode_bl6w_lds_bytes: the classic lpc 0 carve is the 39 308 floats it was
    and 256 dump words behind them, inside 160 KB; the extended and the lpc 4 kernels keep their carves;
  * the first n samples and heads of a decode of n + 5 steps equal the decode of n steps bit for bit;
  * without a heads buffer the samples are the same and nothing but `out` is written.
lpc 0 classic is the changed kernel; lpc 0 extended (the caller asks for the noise dump) and lpc 4 keep the earlier code and
run the same cases as controls."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-5      # variant 2 against variant 6 and the oracle: the bar of the existing tests of the wave-specialised kernel
U = 110
TF = 4
B = 3
LENGTHS = (1, 2, 3, 4, 5, 9, 17, 33, 63, 64, 65, 66, 129, 130, U - 1, U, U + 1, 2 * U + 1, 3 * U + 1)
MORE = 5                        # the prefix property compares a decode of n steps with one of n + MORE
N_MAX = LENGTHS[-1] + MORE
GUARD = 64                      # floats of NaN on either side of `out` and `heads`
KERNELS = {"lpc0_classic": (0, False), "lpc0_extended": (0, True), "lpc4_classic": (4, False)}
CARVE_LPC0_CLASSIC = 39308 + 256    # floats: the carve of the kernel before the dump words, and one dump word per thread of group A


@functools.lru_cache(maxsize=None)
def _net(lpc):
    cfg = C.bl6_laplace(1, lpc)
    assert cfg.U == U and N_MAX <= TF * U
    sd = synth_state_dict(cfg, seed=91, flavor="trained")
    return cfg, sd, HipNet.from_state_dict(cfg, sd, DEV)


@functools.lru_cache(maxsize=None)
def _inputs(lpc):
    """features and their conditioning, the host-drawn noise of N_MAX steps in the oracle's draw order, teacher-forced inputs"""
    cfg, _, net = _net(lpc)
    aux = torch.from_numpy(synth_aux(cfg, B, TF, seed=92))
    g = torch.Generator().manual_seed(900 + lpc)
    noise_o = cpu_ref.laplace_noise(cfg, N_MAX, B, generator=g)                     # (steps, B, seg)
    noise = torch.from_numpy(noise_o).permute(1, 0, 2).contiguous()                 # (B, steps, seg)
    forced = torch.empty(B, N_MAX).uniform_(-0.8, 0.8, generator=g)
    cond = net.frontend(aux.to(DEV)).contiguous()
    return aux, noise_o, noise, forced, cond


@functools.lru_cache(maxsize=None)
def _oracle(lpc):
    """the CPU oracle's free-running samples (generation is causal: a decode of n steps is their first n)"""
    cfg, sd, _ = _net(lpc)
    aux, noise_o = _inputs(lpc)[:2]
    n = LENGTHS[-1]
    ref = cpu_ref.laplace_generate(cfg, cpu_ref.as_params(sd), aux, [n] * B, noise_o[:n])
    return torch.from_numpy(np.stack([np.asarray(ref[b])[:n] for b in range(B)]).astype(np.float32))


def _guarded(*shape):
    """a NaN-filled buffer with GUARD floats in front of and behind the view the kernel gets"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def _guards_intact(whole):
    return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all())


@functools.lru_cache(maxsize=None)
def _decode(kernel, n, variant, teacher_forced, heads=True):
    """swn_decode on caller-owned, NaN-filled buffers: (samples, heads or None) on the host, guards checked"""
    lpc, extended = KERNELS[kernel]
    cfg, _, net = _net(lpc)
    _, _, noise, forced, cond = _inputs(lpc)
    nz = noise[:, :n].contiguous().to(DEV)
    fo = forced[:, :n].contiguous().to(DEV) if teacher_forced else None
    dump = torch.full((B, n, 1), float("nan"), device=DEV) if extended else None
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    io = _lib.DecodeIO(noise_dev=p(nz), forced_dev=p(fo), seed_dev=None, noise_out_dev=p(dump), rng_seed=0, rng_utt0=0,
                       reserved=0, rng_utt_ids_dev=None)
    lib = _lib.lib()
    state = torch.empty(max(1, lib.swn_decode_state_floats(ctypes.byref(net.desc), B)), device=DEV)
    out_w, out = _guarded(B, n)
    heads_w, hd = _guarded(B, n, cfg.n_out)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.swn_decode(ctypes.byref(net.desc), p(net.packed), p(cond), B, TF, n, ctypes.byref(io), p(state), p(out),
                        p(hd) if heads else None, variant, st)
    assert rc == 0, (kernel, n, variant, rc)
    torch.cuda.synchronize()
    assert _guards_intact(out_w) and _guards_intact(heads_w), (kernel, n, variant)
    if extended:
        assert torch.equal(dump.cpu(), noise[:, :n]), (kernel, n)
    if not heads:
        assert bool(torch.isnan(heads_w).all()), (kernel, n, "a head was written without a heads buffer")
        return out.cpu(), None
    return out.cpu(), hd.cpu()


def test_the_dump_words_lie_inside_the_carve(gpu_ok):
    """the launch asks for the carve the kernel addresses: the parent's 39 308 floats and one dump word per thread of group A
    for the classic lpc 0 kernel, the carves they had for the others - all within the 160 KB of a workgroup"""
    lib = _lib.lib()
    sizes = {}
    for lpc in (0, 4):
        d = ctypes.byref(_net(lpc)[2].desc)
        sizes[lpc] = (int(lib.swn_decode_bl6w_lds_bytes(d, 0)), int(lib.swn_decode_bl6w_lds_bytes(d, 1)))
    print("dynamic LDS bytes (classic, extended):", sizes)
    assert sizes[0][0] == 4 * CARVE_LPC0_CLASSIC, sizes
    for lpc in (0, 4):
        for n in sizes[lpc]:
            assert 0 < n <= 160 * 1024 and n % 16 == 0, sizes
    assert lib.swn_decode_bl6w_lds_bytes(None, 0) == 0


@pytest.mark.parametrize("teacher_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_lengths_against_the_oracle_and_the_symmetric_kernel(gpu_ok, kernel, teacher_forced):
    lpc = KERNELS[kernel][0]
    ref = None if teacher_forced else _oracle(lpc)
    for n in LENGTHS:
        o2, h2 = _decode(kernel, n, 2, teacher_forced)
        o6, h6 = _decode(kernel, n, 6, teacher_forced)
        assert not bool(torch.isnan(o2).any()) and not bool(torch.isnan(h2).any()), (kernel, n, "a step was not stored")
        assert bool(torch.isfinite(o2).all()) and bool(torch.isfinite(h2).all())
        eo, eh = float((o2 - o6).abs().max()), float((h2 - h6).abs().max())
        er = 0.0 if ref is None else float((o2 - ref[:, :n]).abs().max())
        print(f"{kernel} forced {teacher_forced} n_steps {n}: oracle {er:.3g} variant 6 samples {eo:.3g} heads {eh:.3g}")
        assert er <= BAR, (kernel, n, er)
        assert eo <= BAR, (kernel, n, eo)
        assert eh <= BAR, (kernel, n, eh)


@pytest.mark.parametrize("teacher_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_a_shorter_decode_is_the_prefix_of_a_longer_one(gpu_ok, kernel, teacher_forced):
    """a step depends on nothing a later step does: the highway operand carried in a register is formed and used inside one
    step, and the input layer formed behind the last step is read by nobody"""
    for n in LENGTHS:
        o, h = _decode(kernel, n, 2, teacher_forced)
        ol, hl = _decode(kernel, n + MORE, 2, teacher_forced)
        assert not bool(torch.isnan(ol).any()) and not bool(torch.isnan(hl).any()), (kernel, n + MORE)
        assert torch.equal(o, ol[:, :n]), (kernel, n)
        assert torch.equal(h, hl[:, :n]), (kernel, n)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_without_a_heads_buffer_no_head_is_written(gpu_ok, kernel):
    for n in LENGTHS:
        o, _ = _decode(kernel, n, 2, False, heads=False)
        assert not bool(torch.isnan(o).any()), (kernel, n)
        assert torch.equal(o, _decode(kernel, n, 2, False)[0]), (kernel, n)
