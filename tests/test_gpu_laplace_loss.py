"""GPU: the fused Laplace chunk loss (torch.ops.swn.laplace_loss, laplace_loss.LaplaceChunkLoss) against its formulas in
float64 on the CPU (tests/laplace_loss_ref.py), the scale floor, exact ties, the reference's training chunks (g6_trainstep_*
fixtures) with the operator inside `batch_loss`, run-to-run determinism, the no-grad call, `CSWNV.forward_raw` and the
driver flag.

Tolerances of the fp64 comparison, as in test_gpu_spectral_loss.py: the test measures the error e32 of the same formulas in
fp32 torch on the CPU against fp64 on the same inputs (relative to the largest fp64 value of the tensor) and requires the HIP
result within max(4 e32, 1e-6) for nll, err, samples, stats and the gradient with respect to raw, under an upstream of random
g_nll plus random g_samples.  The target rows are copies and must be equal.  The measured figures are printed before the
assertions (pytest -s).

Measured on an MI355X (hip error / e32, relative to the largest fp64 value), cases (seg, lpc, B, tp, skip):
    (1, 0, 1, 300, 0):    nll 5.1e-8 / 4.5e-8   err 2.0e-8 / 7.5e-8   samples 6.1e-8 / 4.1e-8   stats 4.6e-8 / 4.6e-8   graw 1.3e-7 / 1.6e-7
    (1, 4, 1, 257, 37):   nll 3.8e-8 / 3.8e-8   err 4.8e-9 / 4.8e-9   samples 5.2e-8 / 6.6e-8   stats 5.0e-8 / 5.0e-8   graw 1.6e-7 / 1.1e-7
    (5, 4, 1, 1000, 100): nll 7.1e-8 / 8.2e-8   err 3.6e-8 / 1.1e-7   samples 7.6e-8 / 1.4e-7   stats 3.1e-8 / 3.0e-8   graw 5.0e-8 / 8.4e-8
    (2, 4, 3, 513, 0):    nll 1.0e-7 / 1.1e-7   err 2.6e-8 / 8.8e-8   samples 8.2e-8 / 8.2e-8   stats 4.7e-8 / 4.7e-8   graw 3.5e-7 / 3.5e-7
    (10, 4, 2, 255, 254): nll 1.9e-7 / 7.8e-8   err 5.5e-8 / 5.5e-8   samples 8.9e-8 / 8.9e-8   stats 6.5e-8 / 6.5e-8   graw 1.7e-7 / 1.3e-7
    floor case:           nll 8.3e-8 / 9.4e-8   err 2.9e-8 / 8.0e-8   samples 4.7e-8 / 5.9e-8   stats 2.0e-8 / 2.0e-8   graw 1.5e-7 / 1.5e-7
    ties case:            nll 3.4e-8 / 3.4e-8   err 4.3e-8 / 4.5e-8   samples 8.7e-8 / 8.7e-8   stats 2.2e-8 / 2.2e-8   graw 2.4e-7 / 2.4e-7
(the sums run in float64 on the device, so what is left of nll, err and stats is the rounding of the fp32 result.)
The factor 4 did not have to move: every figure lies under the 1e-6 floor of the bound, 3.5e-7 at the most.
"""
import logging
import re

import numpy as np
import pytest
import torch

import laplace_loss_ref as R
from conftest import golden_names, load_golden
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import train_driver as T
from shallow_wavenet_amd.laplace_loss import LaplaceChunkLoss
from shallow_wavenet_amd.nets import cswnv_shift1 as mc
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

CASES = [(1, 0, 1, 300, 0), (1, 4, 1, 257, 37), (5, 4, 1, 1000, 100), (2, 4, 3, 513, 0), (10, 4, 2, 255, 254)]
KEYS = ("nll", "err", "samples", "stats", "graw")


def _upstream(seg, B, N, seed, samples=True):
    g = torch.Generator().manual_seed(seed)
    g_nll = torch.randn(B, seg, generator=g, dtype=torch.float32).double()
    g_smp = 0.01 * torch.randn(B * seg, N, generator=g, dtype=torch.float32).double() if samples else None
    return g_nll, g_smp


def _hip(seg, lpc, skip, raw, ctx, target, eps, g_nll=None, g_smp=None):
    """the operator and its backward -> dict of float64 CPU tensors, the keys of laplace_loss_ref.reference"""
    cu = lambda t: None if t is None else t.float().cuda()
    r = cu(raw).requires_grad_(True)
    nll, err, samples, targets, stats = LaplaceChunkLoss(seg, lpc)(r, cu(ctx), cu(target), cu(eps), skip)
    assert nll.requires_grad and samples.requires_grad
    assert not (err.requires_grad or targets.requires_grad or stats.requires_grad)
    out = dict(nll=nll, err=err, samples=samples, targets=targets, stats=stats)
    if g_nll is not None:
        up = (cu(g_nll) * nll).sum()
        if g_smp is not None:
            up = up + (cu(g_smp) * samples).sum()
        up.backward()
        out["graw"] = r.grad
    return {k: v.detach().double().cpu() for k, v in out.items()}


def _rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


def _hold_to_float64(tag, hip, f32, ref):
    figs = {k: (_rel(hip[k], ref[k]), _rel(f32[k].double(), ref[k])) for k in KEYS}
    for k, (ehip, e32) in figs.items():
        print(f"laplace_loss {tag} {k}: torch fp32 {e32:.3e}  hip {ehip:.3e}  bound {max(4 * e32, 1e-6):.3e}")
    assert torch.equal(hip["targets"], ref["targets"])
    for k in KEYS:
        assert hip[k].shape == ref[k].shape and bool(torch.isfinite(hip[k]).all()), k
    for k, (ehip, e32) in figs.items():
        assert ehip <= max(4 * e32, 1e-6), (tag, k, ehip, e32)


@pytest.mark.parametrize("seg,lpc,B,tp,skip", CASES)
def test_op_matches_float64_reference(gpu_ok, seg, lpc, B, tp, skip):
    """one block and several, a ragged last block, skip inside a block and across blocks, N = 1, B > 1"""
    raw, ctx, target, eps = R.inputs(seg, lpc, B, tp, skip, seed=tp)
    g_nll, g_smp = _upstream(seg, B, tp - skip, seed=tp + 1)
    ref = R.reference(raw, ctx, target, eps, seg, lpc, skip, torch.float64, g_nll, g_smp)
    f32 = R.reference(raw, ctx, target, eps, seg, lpc, skip, torch.float32, g_nll, g_smp)
    hip = _hip(seg, lpc, skip, raw, ctx, target, eps, g_nll, g_smp)
    _hold_to_float64(f"{(seg, lpc, B, tp, skip)}", hip, f32, ref)
    assert float(hip["graw"][:, :, :skip].abs().max()) == 0.0 if skip else True


def test_scale_floor(gpu_ok):
    """scale logits of -15.5 and -20 at some positions put lb below the floor there: b is floored in the NLL, b_noclip is not
    in the samples, and the NLL gives the logit exactly no gradient where the floor acts"""
    seg, lpc, B, tp, skip = 2, 4, 2, 300, 10
    raw, ctx, target, eps = R.inputs(seg, lpc, B, tp, skip, seed=3)
    raw[:, seg, ::7] = -20.0
    raw[:, seg + 1, 3::11] = -15.5
    g_nll, g_smp = _upstream(seg, B, tp - skip, seed=4)
    ref = R.reference(raw, ctx, target, eps, seg, lpc, skip, torch.float64, g_nll, g_smp)
    below = ref["lb"] < R.FLOOR                                                   # (B, seg, N)
    assert 20 < int(below.sum()) < below.numel() // 4
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    f32 = R.reference(raw, ctx, target, eps, seg, lpc, skip, torch.float32, g_nll, g_smp)
    hip = _hip(seg, lpc, skip, raw, ctx, target, eps, g_nll, g_smp)
    _hold_to_float64("floor", hip, f32, ref)
    nll_only = _hip(seg, lpc, skip, raw, ctx, target, eps, g_nll, None)["graw"][:, seg:2 * seg, skip:]
    assert bool((nll_only[below] == 0.0).all()) and bool((nll_only[~below] != 0.0).all())


def test_exact_ties_take_sign_zero(gpu_ok):
    """|trg - mu| at trg == mu and sign(eps) at eps == 0: the gradient is 0 there, as torch's abs and sign give it"""
    seg, lpc, B, tp, skip = 2, 0, 1, 300, 0
    raw, ctx, target, eps = R.inputs(seg, lpc, B, tp, skip, seed=9)
    ties = [(0, 5), (1, 70), (0, 255), (1, 256), (0, 299)]                        # (segment, position), distinct t + j
    zeros = [(0, 6), (1, 71), (1, 299)]
    for j, t in ties:
        target[0, t + j] = raw[0, j, t]
    for j, t in zeros:
        eps[0, j, t] = 0.0
    r32, t32 = raw.float(), target.float()
    assert all(float(t32[0, t + j]) == float(r32[0, j, t]) for j, t in ties)      # the ties are exact in fp32 too
    assert all(float(eps.float()[0, j, t]) == 0.0 for j, t in zeros)
    g_nll, g_smp = _upstream(seg, B, tp, seed=10)
    ref = R.reference(raw, ctx, target, eps, seg, lpc, skip, torch.float64, g_nll, g_smp)
    f32 = R.reference(raw, ctx, target, eps, seg, lpc, skip, torch.float32, g_nll, g_smp)
    _hold_to_float64("ties", _hip(seg, lpc, skip, raw, ctx, target, eps, g_nll, g_smp), f32, ref)
    by_nll = _hip(seg, lpc, skip, raw, ctx, target, eps, g_nll, None)["graw"]
    for j, t in ties:
        assert float(by_nll[0, j, t]) == 0.0 and float(by_nll[0, seg + j, t]) != 0.0
    assert int((by_nll[0, :seg] == 0.0).sum()) == len(ties)
    by_smp = _hip(seg, lpc, skip, raw, ctx, target, eps, torch.zeros_like(g_nll), g_smp)["graw"]
    for j, t in zeros:
        assert float(by_smp[0, seg + j, t]) == 0.0 and float(by_smp[0, j, t]) == float(g_smp.float()[j, t])
    assert int((by_smp[0, seg:] == 0.0).sum()) == len(zeros)


@pytest.mark.parametrize("spectral", ["torch", "hip"])
@pytest.mark.parametrize("name", [n for n in golden_names() if n.startswith("g6_trainstep") and "softmax" not in n])
def test_training_chunk_with_hip_laplace_loss_matches_reference_modules(gpu_ok, name, spectral):
    """test_gpu_train_step.py::test_training_chunk_matches_reference_modules with the operator inside batch_loss: the
    fixtures hold the losses and parameter gradients of the REFERENCE's modules under the host draws of the torch path."""
    from shallow_wavenet_amd.spectral import MultiResolutionSTFTLoss
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
    win = [torch.hann_window(n).cuda() for n in fft]
    torch.manual_seed(int(d["step_seed"]))
    loss, l_lap, l_lsd, l_err = T.batch_loss(m, mc.LaplaceLoss(), mc.LSDloss(), bh, bx, trg, xp, flen, h_ss, fft, win, do=True,
                                             spectral_loss=MultiResolutionSTFTLoss(fft, "cuda") if spectral == "hip" else None,
                                             laplace_loss=LaplaceChunkLoss(m.seg, m.lpc))
    rel = lambda a, b: abs(a - b) <= 2e-5 * max(1.0, abs(b))
    assert rel(l_lap.item(), float(d["loss_laplace"])), (l_lap.item(), float(d["loss_laplace"]))
    assert rel(l_err.item(), float(d["loss_err"])), (l_err.item(), float(d["loss_err"]))
    assert rel(loss.item(), float(d["loss"])), (loss.item(), float(d["loss"]))
    if not np.isnan(float(d["loss_lsd"])):
        assert abs(l_lsd.item() - float(d["loss_lsd"])) <= 1e-3 * max(1.0, abs(float(d["loss_lsd"])))
    loss.backward()
    for k, p in m.named_parameters():
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    _check(name, m, d)


def test_two_calls_are_bit_identical(gpu_ok):
    seg, lpc, B, tp, skip = 5, 4, 2, 1000, 100
    raw, ctx, target, eps = (None if t is None else t.float().cuda() for t in R.inputs(seg, lpc, B, tp, skip, seed=21))
    g_nll, g_smp = (t.float().cuda() for t in _upstream(seg, B, tp - skip, seed=22))
    loss = LaplaceChunkLoss(seg, lpc)
    outs = []
    for _ in range(2):
        r = raw.clone().requires_grad_(True)
        o = loss(r, ctx, target, eps, skip)
        ((g_nll * o[0]).sum() + (g_smp * o[2]).sum()).backward()
        outs.append([t.detach().clone() for t in o] + [r.grad.clone()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_no_grad_call_and_the_ops(gpu_ok):
    seg, lpc, B, tp, skip = 2, 4, 1, 300, 10
    raw, ctx, target, eps = (None if t is None else t.float().cuda() for t in R.inputs(seg, lpc, B, tp, skip, seed=31))
    loss = LaplaceChunkLoss(seg, lpc)
    r = raw.clone().requires_grad_(True)
    with_grad = loss(r, ctx, target, eps, skip)
    with torch.no_grad():
        without = loss(r, ctx, target, eps, skip)
    for a, b in zip(with_grad, without):
        assert not b.requires_grad and torch.equal(a.detach(), b)
    one_d = loss(raw, ctx, target[0], eps, skip)                                   # the 1-D target slice_chunk returns
    assert all(torch.equal(a, b) for a, b in zip(one_d, without))
    desc = loss._desc
    by_op = torch.ops.swn.laplace_loss(raw, ctx, target, eps, desc, skip)
    assert all(torch.equal(a, b) for a, b in zip(by_op, without))
    g_nll = torch.ones(B, seg, device="cuda")
    (with_grad[0].sum()).backward()
    assert torch.equal(torch.ops.swn.laplace_loss_backward(raw, ctx, target, eps, g_nll, None, desc, skip), r.grad)
    with pytest.raises(RuntimeError):
        torch.ops.swn.laplace_loss(raw, None, target, eps, desc, skip)             # lpc > 0 needs the context


@pytest.mark.parametrize("seg,lpc", [(1, 0), (2, 4)])
def test_forward_raw_is_the_raw_behind_forward(gpu_ok, seg, lpc):
    """without dropout, in the evaluation path and behind autograd: forward's mu / a are rows of forward_raw, bit for bit"""
    cfg = C.tiny("laplace", seg, lpc)
    B, Tf = 2, 9
    m = mc.CSWNV(**cfg.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, seed=1, flavor="trained").items()})
    m.cuda().train()
    aux = torch.from_numpy(synth_aux(cfg, B, Tf)).cuda()
    audio = (torch.rand(B, 1, Tf * cfg.U - seg, generator=torch.Generator().manual_seed(2)) * 1.8 - 0.9).cuda()
    Tp = Tf * cfg.U - 2 * seg + 1
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            raw = m.forward_raw(aux, audio)
            res = m(aux, audio, clip=True)
        assert raw.shape == (B, 2 * seg + lpc, Tp) and raw.requires_grad == grad
        assert torch.equal(res[0].reshape(B, Tp, seg), raw[:, :seg].transpose(1, 2))
        if lpc > 0:
            assert torch.equal(res[-1], raw[:, 2 * seg:].transpose(1, 2))
    target = torch.zeros(B, Tp + seg - 1, device="cuda")
    ctx = torch.zeros(B, Tp + seg + lpc - 1, device="cuda") if lpc else None
    eps = torch.full((B, seg, Tp), 0.25, device="cuda")
    nll = LaplaceChunkLoss(seg, lpc)(raw, ctx, target, eps, 0)[0]
    nll.mean().backward()                                                          # the operator's gradient reaches the stack
    assert float(m.out_2.weight.grad.abs().max()) > 0.0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stage4_driver_runs_with_the_hip_laplace_loss(gpu_ok, tmp_path, caplog, precision):
    """two synthetic epochs (training and the no-grad evaluation loop) at seg 2 / lpc 4 with both HIP losses: the driver's log
    lines parse, the losses are finite, and every training and evaluation chunk logs one LaplaceLoss statistics line"""
    exp = tmp_path / precision
    caplog.set_level(logging.INFO)
    rc = T.main(["--expdir", str(exp), "--synthetic", "3", "--n_aux", "10", "--hid_chn", "32", "--skip_chn", "48",
                 "--dilation_depth", "3", "--dilation_repeat", "2", "--kernel_size", "3", "--upsampling_factor", "20",
                 "--seg", "2", "--lpc", "4", "--batch_size", "600", "--n_fft_facts", "5", "--do_prob", "0.5",
                 "--wav_conv_flag", "true", "--epoch_count", "2", "--verbose", "1", "--precision", precision,
                 "--spectral_loss", "hip", "--laplace_loss", "hip"])
    assert rc == 0
    text = caplog.text
    assert "nan" not in text.lower()
    evals = [float(v) for v in re.findall(r"\(EPOCH:\d+\) average evaluation loss = (-?[0-9.]+)", text)]
    assert len(evals) == 2 and all(np.isfinite(evals))
    batch = re.findall(r"batch loss \S+ \[\d+:\d+\] \d+ \d+ \d+ -?\d+ \d+ -?\d+ = (-?[0-9.]+) (-?[0-9.]+ dB|n/a) ([0-9.]+) \(", text)
    n_train = len(re.findall(r"\d+ iteration \[\d+\]", text))
    assert n_train >= 4 and len(batch) == n_train and all(np.isfinite(float(v.split()[0])) for row in batch for v in row if v != "n/a")
    stats = re.findall(r" (-?\d+\.\d{6}) (\S+E[+-]\d+) (-?\d+\.\d{6}) (\S+E[+-]\d+) (\S+E[+-]\d+) (\S+E[+-]\d+) (\S+E[+-]\d+)$", text, re.M)
    names, _, loader = T.synthetic_corpus(3, 10, 20, seed=1)
    rf = mc.CSWNV(n_aux=10, hid_chn=32, skip_chn=48, dilation_depth=3, dilation_repeat=2, kernel_size=3, upsampling_factor=20,
                  seg=2, lpc=4, wav_conv_flag=True).receptive_field
    n_eval = sum(len(T.chunk_plan(len(loader(n, n)[1]), rf, 600, 2, 20)) for n in names[:1])
    assert len(stats) == n_train + 2 * n_eval, (len(stats), n_train, n_eval)
    for row in stats:
        lo, mean, hi, var, vlo, vmean, vhi = (float(v) for v in row)
        assert lo <= mean <= hi and var >= 0.0 and 0.0 < vlo <= vmean <= vhi
