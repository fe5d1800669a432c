"""CPU: the formulas of the fused Laplace chunk loss (tests/laplace_loss_ref.py, the oracle of the GPU tests) equal the torch
assembly of `train_driver.batch_loss` they replace, the shape rules of `LaplaceChunkLoss` and the driver flag.

The assembly is driven with a stub model that returns the head tensors of a fixed `raw` the way `CSWNV.forward(clip=True)`
does, and a stub spectral loss that records the sample / target rows and returns a fixed linear functional of the samples,
so that the chunk's total loss carries gradient through the NLL and through the samples.  Both sides are fp32 on the CPU and
differ only in the order of a few operations (the LP sum over <= 4 taps, means over <= 300 positions): element-wise
results within 4 fp32 ulp of the largest value (5e-7), means and the gradient within 2e-6 of the largest value."""
import logging
import re

import pytest
import torch

import laplace_loss_ref as R
from shallow_wavenet_amd import train_driver as T
from shallow_wavenet_amd.laplace_loss import LaplaceChunkLoss
from shallow_wavenet_amd.nets.cswnv_shift1 import LaplaceLoss, LSDloss


class _StubModel:
    """seg / lpc / receptive_field and the tuples of CSWNV.forward(clip=True) (cswnv_shift1.py:228-267) from a fixed raw"""

    def __init__(self, raw, seg, lpc, rf):
        self.raw, self.seg, self.lpc, self.receptive_field = raw, seg, lpc, rf

    def __call__(self, aux, audio, do=False, clip=False):
        assert clip
        seg, lpc = self.seg, self.lpc
        tm = lambda x: x.transpose(1, 2)
        mu, lb = tm(self.raw[:, :seg]), torch.nn.functional.logsigmoid(tm(self.raw[:, seg:2 * seg]))
        b = torch.exp(lb)
        if lpc == 0 and seg == 1:
            mu, lb, b = (x.reshape(x.shape[0], -1) for x in (mu, lb, b))
        tail = (tm(self.raw[:, 2 * seg:]),) if lpc > 0 else ()
        if torch.min(lb) < R.FLOOR:
            lc = torch.clamp(lb, min=R.FLOOR)
            return (mu, b, torch.exp(lc), lc) + tail
        return (mu, b, b, lb) + tail


class _StubSpectral:
    """records the rows and returns l1[r] = sum_t w[r, t] samples[r, t] as the only 'FFT size'"""

    def __init__(self, w):
        self.w, self.samples, self.targets = w, None, None

    def sizes_for(self, feat_len):
        return [128]

    def __call__(self, samples, targets, feat_len):
        self.samples = torch.stack(list(samples)) if not torch.is_tensor(samples) else samples
        self.targets = torch.stack(list(targets)) if not torch.is_tensor(targets) else targets
        l1 = (self.samples * self.w).sum(1, keepdim=True)
        return l1, torch.ones_like(l1).detach()


def _close(a, b, tol):
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("floor", [False, True])
@pytest.mark.parametrize("h_ss", [0, 3])
@pytest.mark.parametrize("seg,lpc", [(1, 0), (1, 4), (5, 4)])
def test_fp32_reference_equals_the_torch_assembly_of_batch_loss(caplog, seg, lpc, h_ss, floor):
    tp, rf = 300, 41
    skip = rf if h_ss > 0 else 0
    N = tp - skip
    raw, ctx, target, _ = R.inputs(seg, lpc, 1, tp, skip, seed=seg * 10 + lpc + h_ss)
    if floor:
        raw[0, seg, ::17] = -20.0
        raw[0, 2 * seg - 1, 5::23] = -15.5
    raw32 = raw.float().requires_grad_(True)
    x_prob = None if ctx is None else ctx.float()
    w = torch.randn(seg, N, generator=torch.Generator().manual_seed(5))
    spec = _StubSpectral(w)
    caplog.set_level(logging.INFO)
    gen = torch.Generator().manual_seed(77)
    loss, l_lap, l_lsd, l_err = T.batch_loss(_StubModel(raw32, seg, lpc, rf), LaplaceLoss(), LSDloss(), None, None,
                                             target[0].float(), x_prob, N, h_ss, [128], [None], do=False,
                                             eps_generator=gen, spectral_loss=spec)
    loss.backward()
    # the deviates the assembly drew: per segment, in order, from the same generator
    gen = torch.Generator().manual_seed(77)
    eps = torch.stack([torch.empty(N).uniform_(-0.4999, 0.5, generator=gen) for _ in range(seg)]).unsqueeze(0)
    ref = R.reference(raw, ctx, target, eps, seg, lpc, skip, torch.float32,
                      g_nll=torch.full((1, seg), 1.0 / seg), g_samples=w / seg)
    assert bool((ref["lb"] < R.FLOOR).any()) == floor
    assert _close(spec.samples.detach(), ref["samples"], 5e-7)
    assert torch.equal(spec.targets, ref["targets"])
    assert _close(l_lap.detach(), ref["nll"].mean(), 2e-6)
    assert _close(l_err.detach(), ref["err"].mean(), 2e-6)
    assert _close(loss.detach(), ref["nll"].mean() + (ref["samples"] * w).sum(1).mean(), 2e-6)
    assert _close(raw32.grad, ref["graw"], 2e-6)
    assert float(raw32.grad[0, :, :skip].abs().max()) == 0.0 if skip else True
    # LaplaceLoss's log line of segment 0 is what `stats` holds
    lines = re.findall(r"(-?\d+\.\d{6}) (\S+E[+-]\d+) (-?\d+\.\d{6}) (\S+E[+-]\d+) (\S+E[+-]\d+) (\S+E[+-]\d+) (\S+E[+-]\d+)",
                       caplog.text)
    assert len(lines) == 1
    for got, want in zip(lines[0], ref["stats"].tolist()):
        assert abs(float(got) - want) <= 1e-6 + 1e-5 * abs(want), (lines[0], ref["stats"])


def test_shape_validation_errors():
    seg, lpc, tp, skip = 2, 4, 40, 7
    raw, ctx, target, eps = (None if t is None else t.float() for t in R.inputs(seg, lpc, 1, tp, skip))
    loss = LaplaceChunkLoss(seg, lpc)
    assert loss.check(raw, ctx, target, eps, skip) == (1, tp, tp - skip)
    bad = [(raw[:, :-1], ctx, target, eps, skip), (raw[0], ctx, target, eps, skip), (raw, None, target, eps, skip),
           (raw, ctx[:, :-1], target, eps, skip), (raw, ctx, target[:, 1:], eps, skip), (raw, ctx, target, eps[:, :1], skip),
           (raw, ctx, target, eps, skip + 1), (raw, ctx, target, eps, tp), (raw, ctx, target, eps, -1),
           (raw, ctx, target.clone().requires_grad_(True), eps, skip)]
    for args in bad:
        with pytest.raises(ValueError):
            loss.check(*args)
    for args in bad[:6]:
        with pytest.raises(ValueError):
            loss(*args)                                   # the call validates before it touches a device
    with pytest.raises(ValueError):
        LaplaceChunkLoss(0, 4)
    with pytest.raises(ValueError):
        LaplaceChunkLoss(5, 17)
    LaplaceChunkLoss(1, 0).check(raw[:, :2], None, target[:, :tp], eps[:, :1], skip)      # lpc 0 takes no context


def test_parser_takes_the_flag_and_defaults_to_torch():
    p = T.build_parser()
    assert p.parse_args(["--expdir", "x"]).laplace_loss == "torch"
    assert p.parse_args(["--expdir", "x", "--laplace_loss", "hip"]).laplace_loss == "hip"
    with pytest.raises(SystemExit):
        p.parse_args(["--expdir", "x", "--laplace_loss", "triton"])


def test_library_rejects_bad_arguments_without_a_device():
    """SWN_E_BADARG (-2) ahead of any launch: a softmax descriptor, N < 1, null pointers, a NULL context with lpc > 0"""
    import ctypes
    from shallow_wavenet_amd import _lib, config as C
    lib = _lib.lib()
    null, one = ctypes.c_void_p(None), ctypes.c_void_p(64)
    d = _lib.desc_from_cfg(C.tiny("laplace", 2, 4))
    r = ctypes.byref(d)
    assert lib.swn_laplace_loss_work_bytes(r, 3, 513, 0) == 8 * 3 * 3 * (2 * 2 + 7)
    assert lib.swn_laplace_loss_work_bytes(r, 1, 10, 10) == 0
    assert lib.swn_laplace_loss_forward(r, one, one, one, one, 1, 10, 10, one, one, one, one, one, one, null) == -2
    assert lib.swn_laplace_loss_forward(r, one, null, one, one, 1, 10, 0, one, one, one, one, one, one, null) == -2
    assert lib.swn_laplace_loss_forward(r, null, one, one, one, 1, 10, 0, one, one, one, one, one, one, null) == -2
    assert lib.swn_laplace_loss_backward(r, one, null, one, one, 1, 10, 0, one, null, one, null) == -2
    assert lib.swn_laplace_loss_backward(r, one, one, one, one, 1, 10, 0, null, null, one, null) == -2
    s = _lib.desc_from_cfg(C.tiny("softmax"))
    assert lib.swn_laplace_loss_work_bytes(ctypes.byref(s), 1, 10, 0) == 0
    assert lib.swn_laplace_loss_forward(ctypes.byref(s), one, one, one, one, 1, 10, 0, one, one, one, one, one, one, null) == -2


def test_fake_implementations_give_the_shapes_and_the_checks():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from shallow_wavenet_amd import ops
    seg, lpc, B, tp, skip = 5, 4, 2, 1000, 100
    desc = LaplaceChunkLoss(seg, lpc)._desc
    assert "laplace_loss" in ops.OP_NAMES and "laplace_loss_backward" in ops.OP_NAMES
    with FakeTensorMode():
        raw, ctx, trg = torch.empty(B, 2 * seg + lpc, tp), torch.empty(B, tp + seg + lpc - 1), torch.empty(B, tp + seg - 1)
        eps = torch.empty(B, seg, tp - skip)
        nll, err, samples, targets, stats = torch.ops.swn.laplace_loss(raw, ctx, trg, eps, desc, skip)
        assert tuple(nll.shape) == (B, seg) and tuple(err.shape) == (B, seg) and tuple(stats.shape) == (7,)
        assert tuple(samples.shape) == (B * seg, tp - skip) and tuple(targets.shape) == (B * seg, tp - skip)
        graw = torch.ops.swn.laplace_loss_backward(raw, ctx, trg, eps, nll, samples, desc, skip)
        assert tuple(graw.shape) == tuple(raw.shape)
        with pytest.raises(RuntimeError, match="LP context"):
            torch.ops.swn.laplace_loss(raw, None, trg, eps, desc, skip)
        with pytest.raises(RuntimeError, match="leaves no position"):
            torch.ops.swn.laplace_loss(raw, ctx, trg, eps, desc, tp)


def test_there_is_no_cpu_path_behind_the_op():
    seg, lpc, tp = 1, 0, 40
    raw, _, target, eps = (None if t is None else t.float() for t in R.inputs(seg, lpc, 1, tp, 0))
    with pytest.raises(RuntimeError, match="HIP device"):
        LaplaceChunkLoss(seg, lpc)(raw, None, target, eps, 0)
