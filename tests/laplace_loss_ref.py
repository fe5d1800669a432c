"""The Laplace chunk loss (include/swn_hip.h, swn_laplace_loss_*) as plain torch formulas on the CPU, in a chosen dtype:
the values and the autograd gradient with respect to `raw`.  Shared by test_laplace_loss_host.py (fp32, against the torch
assembly of train_driver.batch_loss) and test_gpu_laplace_loss.py (float64, the oracle of the HIP operator)."""
import numpy as np
import torch

FLOOR = float(np.float32(-14.162084148244246758816564788835))      # the fp32 constant of laplace_head_kernel
LN2 = 0.69314718055994530941723212145818


def inputs(seg, lpc, B, tp, skip, seed=0, logit_scale=2.0):
    """raw (B, 2 seg + lpc, tp), ctx (B, tp + seg + lpc - 1) or None, target (B, tp + seg - 1), eps (B, seg, tp - skip),
    float64 values that are exact in fp32"""
    g = torch.Generator().manual_seed(seed)
    r32 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    raw = r32(B, 2 * seg + lpc, tp)
    raw[:, :seg] *= 0.3
    raw[:, seg:2 * seg] = raw[:, seg:2 * seg] * logit_scale - 3.0
    raw[:, 2 * seg:] *= 0.4
    target = torch.tanh(r32(B, tp + seg - 1))
    ctx = torch.tanh(r32(B, tp + seg + lpc - 1)) if lpc > 0 else None
    eps = torch.empty(B, seg, tp - skip, dtype=torch.float32).uniform_(-0.4999, 0.5, generator=g)
    d = lambda t: None if t is None else t.double()
    return d(raw), d(ctx), d(target), d(eps)


def reference(raw, ctx, target, eps, seg, lpc, skip, dtype, g_nll=None, g_samples=None):
    """-> dict(nll (B, seg), err (B, seg), samples (B seg, N), targets (B seg, N), stats (7,), lb (B, seg, N) and, given
    the upstream gradients, graw (B, NO, tp) = d (sum g_nll nll + sum g_samples samples) / d raw), all in `dtype`"""
    c = lambda t: None if t is None else t.detach().to(dtype)
    raw, ctx, target, eps = c(raw).requires_grad_(True), c(ctx), c(target), c(eps)
    B, NO, tp = raw.shape
    assert NO == 2 * seg + lpc and eps.shape == (B, seg, tp - skip)
    mu, trg = [], []
    for j in range(seg):
        m = raw[:, j]
        for k in range(lpc):
            m = m + raw[:, 2 * seg + lpc - 1 - k] * ctx[:, j + k:j + k + tp]
        mu.append(m)
        trg.append(target[:, j:j + tp])
    mu, trg = torch.stack(mu, 1)[:, :, skip:], torch.stack(trg, 1)[:, :, skip:]          # (B, seg, N)
    lb = torch.nn.functional.logsigmoid(raw[:, seg:2 * seg, skip:])
    b_noclip = torch.exp(lb)
    lc = torch.clamp(lb, min=FLOOR)
    b = torch.exp(lc)
    nll = (LN2 + lc + torch.abs(trg - mu) / b).mean(2)
    samples = mu - b_noclip * torch.sign(eps) * torch.log1p(-2 * torch.abs(eps))
    err = torch.abs(samples - trg).mean(2)
    m0, v0 = mu[:, 0].reshape(-1), (2 * b[:, 0] ** 2).reshape(-1)
    stats = torch.stack([m0.min(), m0.mean(), m0.max(), m0.var(), v0.min(), v0.mean(), v0.max()])
    N = tp - skip
    out = dict(nll=nll.detach(), err=err.detach(), samples=samples.detach().reshape(B * seg, N),
               targets=trg.detach().reshape(B * seg, N), stats=stats.detach(), lb=lb.detach())
    if g_nll is not None:
        up = (c(g_nll) * nll).sum()
        if g_samples is not None:
            up = up + (c(g_samples).reshape(B, seg, N) * samples).sum()
        out["graw"], = torch.autograd.grad(up, raw)
    return out
