"""GPU: the fused multi-resolution STFT loss (torch.ops.swn.spectral_loss, spectral.MultiResolutionSTFTLoss) against
`torch.stft` in float64 on the CPU, the non-finite pattern of the fp32 torch path, the reference's training chunks
(g6_trainstep_* fixtures) with the HIP loss inside `batch_loss`, run-to-run determinism, the no-grad call and the driver flag.

Tolerances of the fp64 comparison: the test measures torch's own fp32 CPU error e32 against fp64 on the same inputs
(relative to the largest fp64 value) and requires the HIP result within max(4 e32, 1e-6) for l1 and the gradient and within
max(4 e32, 1e-4) for lsd: the factor 4 allows for another summation order over up to 2 048 terms, the floors keep a lucky
e32 from making the test flaky.  The measured figures are printed before each assertion (pytest -s).

Measured on an MI355X (relative to the largest fp64 value; e32 = torch fp32 on the CPU, same inputs):
    5 x 8 114, 17 sizes:  l1 9.9e-8 (e32 2.4e-7)   lsd 3.4e-5 (e32 2.6e-5)   grad 3.0e-7 (e32 6.8e-4)
    1 x 601, 13 sizes:    lsd 1.9e-5 (e32 3.2e-5)   grad 3.0e-7 (e32 9.9e-8)
    3 x 4 999, 17 sizes:  lsd 2.3e-5 (e32 5.7e-5)   grad 3.3e-7 (e32 7.7e-4)
    zero-target case:     lsd 2.9e-5 (e32 2.9e-5)   grad 8.2e-4 (e32 8.2e-4)
The factor 4 did not have to move.  Where e32 of the gradient is near 7e-4, one coefficient of |S - T| lies so close to zero
that rounding decides its sign (torch's fp32 path subtracts two nearly equal transforms; the op transforms sample - target and
flips about fifty times less often): a flipped sign moves a few gradient samples by 2 / count, it is no transform error.

The structural set (tests/spectral_ref.py): the imaginary parts of bins 0 and n / 2, and of every bin of a frame centred on
sample 0 or on sample T - 1 (reflect padding makes such a frame symmetric), are zero in exact arithmetic; what fp32 or float64
give there is rounding noise of random sign, and the fold of the backward cancels its contribution.  Measured on the GPU,
5 x 8 114 / 17 sizes: of the operator's 2 808 930 sign entries 46 125 are structural and 17 703 of those differ from float64;
of the 2 762 805 others none differs (3 018 of them lie below the worst-case fp32 rounding bound, none of those differs
either).  tests/test_gpu_spectral_edges.py takes that noise out of the yardstick and holds the gradient near 1e-6 per size,
edge length and upstream weight.
"""
import logging

import numpy as np
import pytest
import torch

from conftest import load_golden
from shallow_wavenet_amd import train_driver as T
from spectral_ref import signals as _signals, torch_path as _torch_path       # the fp64 / fp32 torch formulas on the CPU
from shallow_wavenet_amd.spectral import MultiResolutionSTFTLoss

pytestmark = pytest.mark.gpu

SIZES = T.fft_sizes(17)


def _hip_path(loss, smp, trg, length):
    s = smp.float().cuda().requires_grad_(True)
    l1, lsd = loss(s, trg.float().cuda(), length)
    l1.mean().backward()
    return l1.detach().double().cpu(), lsd.detach().double().cpu(), s.grad.double().cpu()


def _rel(a, ref, mask=None):
    if mask is not None:
        a, ref = a[mask], ref[mask]
    return float((a - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("R,length", [(5, 8114), (1, 601), (3, 4999)])
def test_op_matches_float64_stft(gpu_ok, R, length):
    """l1, lsd and d mean(l1) / d samples against torch.stft in float64: the recipe's chunk (5 rows of 8 114 samples, all 17
    sizes), one short row (601 samples: the sizes above 1 024 are filtered out, 2 to 19 frames) and a prime length that no
    hop divides."""
    smp, trg = _signals(R, length, seed=length)
    loss = MultiResolutionSTFTLoss(SIZES, "cuda")
    sizes = loss.sizes_for(length)
    assert sizes == [n for n in SIZES if length > n // 2] and (len(sizes) == 17) == (length > 1024)
    ref = _torch_path(smp, trg, sizes, torch.float64)
    f32 = _torch_path(smp, trg, sizes, torch.float32)
    hip = _hip_path(loss, smp, trg, length)
    assert hip[0].shape == (R, len(sizes)) and hip[1].shape == (R, len(sizes)) and hip[2].shape == (R, length)
    for what, i, floor in (("l1", 0, 1e-6), ("lsd", 1, 1e-4), ("grad", 2, 1e-6)):
        e32, ehip = _rel(f32[i], ref[i]), _rel(hip[i], ref[i])
        print(f"spectral R={R} T={length} {what}: torch fp32 {e32:.3e}  hip {ehip:.3e}  bound {max(4 * e32, floor):.3e}")
    for what, i, floor in (("l1", 0, 1e-6), ("lsd", 1, 1e-4), ("grad", 2, 1e-6)):
        e32, ehip = _rel(f32[i], ref[i]), _rel(hip[i], ref[i])
        assert ehip <= max(4 * e32, floor), (what, ehip, e32)


def test_non_finite_pattern_matches_the_torch_path(gpu_ok):
    """an all-zero target row: log10(0) = -inf makes that row's lsd non-finite in torch; the op must give the same isfinite
    masks (batch_loss selects by them) and meet the tolerances on the finite entries."""
    R, length = 4, 3000
    smp, trg = _signals(R, length, seed=7)
    trg[2] = 0.0
    loss = MultiResolutionSTFTLoss(SIZES, "cuda")
    sizes = loss.sizes_for(length)
    ref = _torch_path(smp, trg, sizes, torch.float64)
    f32 = _torch_path(smp, trg, sizes, torch.float32)
    hip = _hip_path(loss, smp, trg, length)
    assert not torch.isfinite(f32[1][2]).any() and torch.isfinite(f32[1][[0, 1, 3]]).all()
    assert torch.equal(torch.isfinite(hip[0]), torch.isfinite(f32[0]))
    assert torch.equal(torch.isfinite(hip[1]), torch.isfinite(f32[1]))
    assert torch.isfinite(hip[2]).all()
    for what, i, floor in (("l1", 0, 1e-6), ("lsd", 1, 1e-4), ("grad", 2, 1e-6)):
        ok = torch.isfinite(ref[i])
        e32, ehip = _rel(f32[i], ref[i], ok), _rel(hip[i], ref[i], ok)
        print(f"spectral zero-target {what}: torch fp32 {e32:.3e}  hip {ehip:.3e}")
        assert ehip <= max(4 * e32, floor), (what, ehip, e32)


@pytest.mark.parametrize("name", ["g6_trainstep_tiny_s5l4", "g6_trainstep_tiny_s1l0", "g6_trainstep_tiny_s1l4_tail"])
def test_training_chunk_with_hip_loss_matches_reference_modules(gpu_ok, name):
    """test_gpu_train_step.py::test_training_chunk_matches_reference_modules with the HIP loss inside batch_loss: the
    fixtures hold the losses and parameter gradients of the REFERENCE's modules, the spectral term adds 0.30-0.44 to the stored total."""
    from shallow_wavenet_amd.nets import cswnv_shift1 as mc
    from shallow_wavenet_amd.synth import synth_state_dict
    from test_gpu_backward_parity import _check
    cfg, d = load_golden(name)
    m = mc.CSWNV(**cfg.ctor_kwargs(), do_prob=float(d["drop_p"]))
    m.dropout_source = "host"
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, seed=int(d["wseed"]), flavor="trained").items()})
    m.cuda().train()
    for p in m.scale_in.parameters():
        p.requires_grad = False
    plan = [tuple(int(v) for v in r) for r in d["plan"]]
    h_bs, x_bs, h_ss, x_ss = plan[int(d["chunk_index"])]
    bh, bx, trg, xp, flen = T.slice_chunk(m, torch.from_numpy(d["x"]).cuda(), torch.from_numpy(d["h"]).cuda(), h_bs, x_bs, h_ss, x_ss)
    assert flen == int(d["feat_len"])
    fft = T.fft_sizes(int(d["n_fft_facts"]))
    spectral = MultiResolutionSTFTLoss(fft, "cuda")
    assert spectral.sizes_for(flen) == ([128, 256] if name.endswith("tail") else [128, 256, 512])
    torch.manual_seed(int(d["step_seed"]))
    loss, l_lap, l_lsd, l_err = T.batch_loss(m, mc.LaplaceLoss(), mc.LSDloss(), bh, bx, trg, xp, flen, h_ss, fft, [None] * len(fft),
                                             do=True, spectral_loss=spectral)
    rel = lambda a, b: abs(a - b) <= 2e-5 * max(1.0, abs(b))
    assert rel(l_lap.item(), float(d["loss_laplace"])), (l_lap.item(), float(d["loss_laplace"]))
    assert rel(l_err.item(), float(d["loss_err"]))
    assert 0.25 < float(d["loss"]) - float(d["loss_laplace"]) < 0.5        # the spectral term the fixture stores
    assert rel(loss.item(), float(d["loss"])), (loss.item(), float(d["loss"]))
    if not np.isnan(float(d["loss_lsd"])):
        assert abs(l_lsd.item() - float(d["loss_lsd"])) <= 1e-3 * max(1.0, abs(float(d["loss_lsd"])))
    loss.backward()
    for k, p in m.named_parameters():
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    _check(name, m, d)


def test_two_calls_are_bit_identical(gpu_ok):
    smp, trg = _signals(5, 8114, seed=11)
    loss = MultiResolutionSTFTLoss(SIZES, "cuda")
    g = torch.rand(5, 17, generator=torch.Generator().manual_seed(1)).cuda()
    outs = []
    for _ in range(2):
        s = smp.float().cuda().requires_grad_(True)
        l1, lsd = loss(s, trg.float().cuda(), 8114)
        (l1 * g).sum().backward()
        outs.append((l1.detach().clone(), lsd.detach().clone(), s.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_no_grad_call_gives_the_forward_values_and_keeps_no_state(gpu_ok):
    smp, trg = _signals(5, 8114, seed=13)
    loss = MultiResolutionSTFTLoss(SIZES, "cuda")
    s = smp.float().cuda().requires_grad_(True)
    t = trg.float().cuda()
    l1, lsd = loss(s, t, 8114)
    assert l1.requires_grad and not lsd.requires_grad
    with torch.no_grad():
        e1, elsd = loss(s, t, 8114)
    assert not e1.requires_grad and torch.equal(e1, l1.detach()) and torch.equal(elsd, lsd)
    tables = loss.tables_for(SIZES)
    assert torch.ops.swn.spectral_loss(s.detach(), t, tables, SIZES, False)[2].numel() == 0
    assert torch.ops.swn.spectral_loss(s.detach(), t, tables, SIZES, True)[2].numel() > 0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stage4_driver_runs_with_the_hip_spectral_loss(gpu_ok, tmp_path, caplog, precision):
    exp = tmp_path / precision
    caplog.set_level(logging.INFO)
    rc = T.main(["--expdir", str(exp), "--synthetic", "3", "--max_iters", "4", "--n_aux", "10", "--hid_chn", "32",
                 "--skip_chn", "48", "--dilation_depth", "3", "--dilation_repeat", "2", "--kernel_size", "3",
                 "--upsampling_factor", "20", "--seg", "1", "--lpc", "0", "--batch_size", "600", "--n_fft_facts", "5",
                 "--do_prob", "0.5", "--wav_conv_flag", "true", "--epoch_count", "1", "--verbose", "1",
                 "--precision", precision, "--spectral_loss", "hip"])
    assert rc == 0
    text = caplog.text.lower()
    assert "iteration" in text and "nan" not in text
