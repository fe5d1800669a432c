"""float64 yardstick for the backward of the mixed-precision training mode (`train_precision("bf16")`), with a model of
where that mode rounds to bf16.  Test helper (not collected): tests/test_mixed_reference.py verifies it on the CPU,
tests/test_gpu_mixed_backward_edges.py and tools/measure_mixed_deviation.py hold the HIP kernels against it.

  exact(cfg, sd, aux, audio, grad_raw, drop=None)      oracle/cpu_ref.py (laplace_stack / softmax_stack) with float64 parameters
        and inputs under torch autograd, raw.backward(grad_raw)  ->  (raw, {state-dict name: gradient})
  rounded(cfg, sd, aux, audio, grad_raw, drop=None, path=...)     the same graph, rounding to bf16 (through float32, round to
        nearest even) where the kernels do.  Forward rounding is straight-through: the value changes, the derivative is that
        of the identity.  path=None switches every rounding off and walks the oracle's own graph: bit for bit `exact`.
  yardstick(...)   D_k = ||g_rounded - g_exact|| per parameter tensor (and per row of its leading axis), D_fwd = max |raw_rounded
        - raw_exact|: the error inherent in the arithmetic for exactly this input and this upstream gradient, computed
        without the code under test.  Every bound of the GPU test is a multiple of it, so a sparse probe gets a small bound.

Where the mixed mode rounds (csrc/ = shallow_wavenet_amd/csrc/), and how the model restates it.  Every contraction that runs
on the matrix cores is one `_qconv`: operands rounded in the forward (F), and in the backward (B) the upstream gradient, the
stored input and the weights rounded before the weight- and the data-gradient products; sums are fp32 on the device, float64
here.

  forward (all paths)
    weights of dil_h, out_skip, out_1, out_2                F   swn_stack_bf16.hip:76 (pack_frag_kernel), :133 (pack_wd_kernel);
                                                                swn_stack_bf16g.hip (the GEMM stack's fragment images)
    h_0 = softsign(causal(lift(audio))), fp32 arithmetic,   F   swn_stack_bf16.hip:108-110 (bf16_input_kernel)
        stored bf16
    h_l of every gated layer, stored bf16; the next layer   F   swn_stack_bf16.hip:360 (bf16_layer_kernel) and the frame-unit
        takes its operand AND its highway term z * h from        variant :503; gates, conditioning, highway in fp32
        the stored value
    relu(skip), relu(out_1), stored bf16                    F   swn_stack_bf16.hip:918, :942 (bf16_head_kernel)
    in_x products of the conditioning: fp32 at frame rate   -   swn_frontend.hip (no rounding), w_up[j] * cond[f] + bx in fp32
        (hoisted: cond = W_inx . C)
  backward, path "fused" (BL6 class, swn_bwd_bl6.hip)
    d raw as the operand of W2^T . dY and of g W2, g b2     B   swn_bwd_bl6.hip:716, :721 (both orientations of dY)
    relu(skip), relu(out_1) recomputed from bf16 h          F   :741 via :748, :771 (put)
    d out_1, d skip, bf16 rows [t][128]                     B   :772, :802 (put); their row sums are g b1, g bsk (all-ones
                                                                fragment of bl6_wgrad_kernel :586: sums of the ROUNDED values)
    da_l = d a of the gate pre-activations, bf16 rows       B   :403-404 (pack2); operand of the data gradient of the layer
                                                                below (:305), of g dil_h and, summed, of g bd (:586)
    Wd, Wd^T, Wsk^T, W1, W1^T, W2^T fragment images         B   :115, :129, :620, :628
    d h (highway carry E, d h_0), d in_x products, d cond,  -   fp32 (:395, :399-400, :326-332)
        g w_up, g b_inx, the input layer
  backward, paths "chain" (BL6 class with fused_backward = False), "recompute" and "keep" (GEMM-stack class) - swn_train.hip
    every time / reduce GEMM rounds BOTH operands on the    B   swn_train.hip:229-231, :332-334 (time GEMMs), :685-687,
        way into LDS, whatever they are: d raw, d out_1,        :852-856 (reduce GEMMs); the head :1884-1907, the layers
        d skip, da, weights, stored activations                 :1969-1986
    bias gradients are fp32 row sums of the UNROUNDED       -   swn_train.hip:634-635
        gradient
    da also leaves as bf16 copies for those GEMMs           B   swn_train.hip:1027 (same values as rounding at the GEMM)
    "keep" only: the in_x-product gradient d gx is stored   B   swn_train.hip:1034 (read by cond_bwd_kernel :1137-1178): d cond,
        as bf16 rows                                            g b_inx and g w_up see the rounded value
  backward, every path: the frame-rate front end
    d C = W_inx^T . d cond, g W_inx = d cond . C^T, the     B   swn_train.hip:2062-2087 through launch_time / launch_reduce in
        conv_aux and scale_in weight and data gradients         the bf16 mode (:1371, :1413); their forward is fp32
  dropout mode (drop = (drop_x, [mask or None per layer]), both classes): in_x runs at sample rate on the masked conditioning
    xm = upsampled C * drop_x, stored bf16                  F   swn_stack_bf16.hip:987 (xm16_kernel)
    gx = W_inx . xm through the matrix cores; path "fused": F   swn_bwd_bl6.hip:99, :378-381 (gx16 rows; the GEMM-stack class
        stored bf16                                             keeps them fp32, swn_train.hip:989-991)
    the layer operand and the highway take h * mask         F   (mask values 0 and 1 / (1 - p) = 2 are exact in bf16)
    d gx as bf16 rows: operand of g W_inx and of d xm       B   swn_bwd_bl6.hip:406-407, swn_train.hip:1034
    d xm, stored bf16 (path "fused")                        B   swn_train.hip:1557-1566 (xm_bwd16_kernel reads bf16 rows)

With any rounding on, the conditioning is walked in the hoisted form the kernels use (cond = W_inx . C at frame rate, then
gx[o][t] = sum_s w_up[j(t+s)] cond_s[o][f(t+s)] + b_inx[o] + b_up sum_c W_inx[o][c]) because that is where the front end's
roundings sit; `rounded(..., path="hoisted")` is that form with no rounding, equal to `exact` to float64 accuracy
(test_mixed_reference.py).  aux_conv2d nets are not modelled (no mixed-precision case uses them).

ReLU kinks.  A ReLU unit whose pre-activation lies within the forward's bf16 error of zero (about 1e-3 here, against a spread
of 0.08-0.2) may sit on different sides in the two graphs, and then moves the gradient by its whole share.  At the synthetic
nets' own biases that is one unit in a thousand: 3-5 % of every tensor under a dense probe, more than half of what the old
tests allow, so no multiple of it fits below their bound.  `single` cases keep the nets' biases and use seeds at which no probed
unit changes side; `edges` and `dense` cases move out_skip.0.bias and out_1.bias so that the skip sum and the out_1
pre-activation are centred two standard deviations above zero (three at 8 x 38 frames; `inputs_of`), `edges` with such seeds too.
`Yardstick.flips` and `.pre_min` report both conditions; test_mixed_reference.py asserts them.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from shallow_wavenet_amd import config as C

PATHS = ("fused", "chain", "recompute", "keep")
ROW_TENSORS = ("dil_h.", "out_skip.", "out_1.weight", "in_x.", "wav_conv.weight", "aux_conv2d.weight")


def bf16(x: torch.Tensor) -> torch.Tensor:
    """round to bf16 through float32 (round to nearest even both times), keeping the dtype"""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


class _Ste(torch.autograd.Function):
    """y = bf16(x) with the derivative of the identity (a value stored as bf16 and read back)"""

    @staticmethod
    def forward(ctx, x):
        return bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _GradRound(torch.autograd.Function):
    """identity whose gradient is rounded to bf16 (a gradient stored as bf16 rows)"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


class _QConv(torch.autograd.Function):
    """conv1d (stride 1) as the matrix cores run it: qf rounds input and weight in the forward, qb rounds the upstream gradient,
    the input and the weight in the two backward products; the bias gradient sums the rounded gradient when qbias, else the
    exact one.  With every flag off this is aten's own convolution and convolution_backward: what autograd runs."""

    @staticmethod
    def forward(ctx, x, w, b, padding, dilation, qf, qb, qbias):
        xq, wq = (bf16(x), bf16(w)) if qf else (x, w)
        ctx.save_for_backward(xq, wq)
        ctx.cfg = (padding, dilation, qf, qb, qbias, b is not None)
        return F.conv1d(xq, wq, b, padding=padding, dilation=dilation)

    @staticmethod
    def backward(ctx, gy):
        xq, wq = ctx.saved_tensors
        padding, dilation, qf, qb, qbias, has_b = ctx.cfg
        gq = bf16(gy) if qb else gy
        if qb and not qf:
            xq, wq = bf16(xq), bf16(wq)
        gx, gw, gb = torch.ops.aten.convolution_backward(gq, xq, wq, [wq.shape[0]] if has_b else None, [1], [padding], [dilation],
                                                         False, [0], 1, [True, True, has_b])
        if has_b and qb and not qbias:
            gb = gy.sum((0, 2))
        return gx, gw, (gb if has_b else None), None, None, None, None, None


@dataclasses.dataclass(frozen=True)
class Model:
    """which roundings are on"""
    fwd: bool = False          # bf16 forward stack (weights, stored activations)
    bwd: bool = False          # backward contractions on bf16 operands
    qbias: bool = False        # bias gradients are sums of the ROUNDED gradient (fused path)
    dgx16: bool = False        # d gx stored as bf16 rows ("keep"; every path in dropout mode)
    dxm16: bool = False        # d xm stored as bf16 rows (fused dropout path)
    gx16: bool = False         # the sample-rate in_x products stored as bf16 rows (fused dropout path)
    hs16: bool = False         # hidden states stored as bf16: the highway term sees the rounded value (every bf16 stack, the
                               # dropout forwards included: swn_stack.hip:431-447 from 256 positions on - below that the
                               # GEMM-stack class runs an fp32-work chain that is not modelled)
    hoist: bool = False        # walk the conditioning in the hoisted form

    @staticmethod
    def of(path: Optional[str], drop: bool = False) -> "Model":
        if path is None:
            return Model()
        if path == "hoisted":
            return Model(hoist=True)
        if path not in PATHS:
            raise ValueError(f"path must be one of {PATHS}, 'hoisted' or None")
        return Model(fwd=True, bwd=True, qbias=path == "fused", dgx16=path == "keep" or drop, dxm16=path == "fused" and drop,
                     gx16=path == "fused" and drop, hs16=True, hoist=True)


def _conv(m: Model, x, w, b, padding=0, dilation=1, fwd=None):
    """one matrix-core contraction; fwd=False: a product whose forward stays fp32 (the frame-rate front end)"""
    return _QConv.apply(x, w, b, padding, dilation, m.fwd if fwd is None else fwd, m.bwd, m.qbias)


def _causal(m: Model, x, w, b, dil, fwd=None):
    k = w.shape[-1]
    return _conv(m, x, w, b, (k - 1) * dil, dil, fwd)[:, :, : x.shape[2]]


def _frontend(m: Model, cfg, P, aux):
    c = _conv(m, aux, P["scale_in.weight"], P["scale_in.bias"], fwd=False)
    k = cfg.aux_kernel_size
    for i in range(cfg.aux_dilation_size):
        c = _conv(m, c, P[f"conv_aux.conv.{i}.weight"], P[f"conv_aux.conv.{i}.bias"], (k ** (i + 1) - k ** i) // 2, k ** i, fwd=False)
    return c


def _in_x_products(m: Model, cfg, P, Cf, Tp: int, oh, drop):
    """[gx_l (B, 2H, Tp) without the dil_h factor, l = 0..L-1]"""
    soft = cfg.kind == "softmax"
    seg = 1 if soft else cfg.seg
    coff, U, A0 = seg, cfg.U, cfg.A0
    if cfg.kind == "laplace" and cfg.aux_conv2d_flag and seg > 1:
        raise NotImplementedError("aux_conv2d nets are not modelled")
    out = []
    if not m.hoist or drop is not None:
        # the oracle's own graph: x at sample rate, then in_x as a 1x1 conv (dropout mode: that is what the kernels do too)
        x = cpu_ref.upsample(cfg, P, Cf)[:, :, coff:]
        if drop is not None:
            x = x * drop[0]
            if m.fwd:
                x = _Ste.apply(x)
            if m.dxm16:
                x = _GradRound.apply(x)
        if not soft:
            x = cpu_ref._stack_seg(cfg, P, x)
        if drop is not None and m.hoist:
            for l in range(cfg.L):
                W, b = P[f"in_x.{l}.weight"], P[f"in_x.{l}.bias"]
                gx = _conv(m, x, W[:, : A0 * seg], None)
                if m.gx16:
                    gx = _Ste.apply(gx)
                gx = gx + b[None, :, None]
                if soft and cfg.audio_in_flag:
                    gx = gx + F.conv1d(oh, W[:, A0 * seg:])
                out.append(gx)
            return out
        if soft and cfg.audio_in_flag:
            x = torch.cat((x, oh), 1)
        return [F.conv1d(x, P[f"in_x.{l}.weight"], P[f"in_x.{l}.bias"]) for l in range(cfg.L)]
    B, Tf = Cf.shape[0], Cf.shape[2]
    w_up, b_up = P["upsampling.conv.weight"].reshape(U), P["upsampling.conv.bias"].reshape(())
    taps = w_up.repeat(Tf)
    for l in range(cfg.L):
        W, b = P[f"in_x.{l}.weight"], P[f"in_x.{l}.bias"]
        Wc = W[:, : A0 * seg]
        gx = (b + b_up * Wc[:, :, 0].sum(1))[None, :, None]
        for s in range(seg):
            cond = _conv(m, Cf, Wc[:, s::seg], None, fwd=False)                       # (B, 2H, Tf): W[o][c*seg+s] . C[c][f]
            lo = coff + s
            gx = gx + cond.repeat_interleave(U, dim=2)[:, :, lo: lo + Tp] * taps[lo: lo + Tp]
        if m.dgx16:
            gx = _GradRound.apply(gx)
        if soft and cfg.audio_in_flag:
            gx = gx + F.conv1d(oh, W[:, A0 * seg:])
        out.append(gx)
    return out


def _stack(m: Model, cfg, P, aux, audio, drop=None):
    """raw (B, n_out, Tp) and the pre-activations of the two ReLUs (skip sum, out_1) - the oracle's laplace_stack /
    softmax_stack op for op, with the roundings of `m`"""
    soft = cfg.kind == "softmax"
    H = cfg.H
    Cf = _frontend(m, cfg, P, aux)
    if soft:
        oh = cpu_ref.one_hot(audio, cfg.n_quantize, dtype=P["causal.conv.weight"].dtype).transpose(1, 2)
        h = F.softsign(cpu_ref.causal_conv(cpu_ref._lift(cfg, P, oh), P["causal.conv.weight"], P["causal.conv.bias"], 1))
    else:
        oh = None
        h = F.softsign(cpu_ref.causal_conv(cpu_ref._lift(cfg, P, audio), P["causal.conv.weight"], P["causal.conv.bias"], 1)[:, :, cfg.seg - 1:])
    Tp = h.shape[2]
    gxs = _in_x_products(m, cfg, P, Cf, Tp, oh, drop)
    if m.hs16:
        h = _Ste.apply(h)
    tot = None
    for l in range(cfg.L):
        a = _causal(m, h, P[f"dil_h.{l}.conv.weight"], P[f"dil_h.{l}.conv.bias"], cfg.dilations[l])
        g = gxs[l] * a
        z = torch.sigmoid(g[:, :H])
        hn = (1 - z) * torch.tanh(g[:, H:]) + z * h
        if m.hs16:
            hn = _Ste.apply(hn)
        sk = _conv(m, hn, P[f"out_skip.{l}.weight"], P[f"out_skip.{l}.bias"])
        h = hn
        if drop is not None and drop[1][l] is not None:
            h = h * drop[1][l]
        tot = sk if tot is None else tot + sk
    y = _conv(m, F.relu(tot), P["out_1.weight"], P["out_1.bias"])
    raw = _conv(m, F.relu(y), P["out_2.weight"], P["out_2.bias"])
    return raw, (tot, y)


def _inputs(cfg, sd, aux, audio, grad_raw, drop, dtype=torch.float64):
    P = cpu_ref.as_params(sd, dtype=dtype)
    for v in P.values():
        v.requires_grad_(True)
    aux = torch.as_tensor(np.asarray(aux), dtype=dtype)
    audio = torch.as_tensor(np.asarray(audio))
    audio = audio.to(torch.int64) if cfg.kind == "softmax" else audio.to(dtype)
    grad_raw = torch.as_tensor(np.asarray(grad_raw), dtype=dtype)
    if drop is not None:
        drop = (torch.as_tensor(drop[0], dtype=dtype), [None if q is None else torch.as_tensor(q, dtype=dtype) for q in drop[1]])
    return P, aux, audio, grad_raw, drop


def _grads(P) -> Dict[str, np.ndarray]:
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().double().numpy().copy() for k, v in P.items()}


def exact(cfg, sd, aux, audio, grad_raw, drop=None) -> Tuple[np.ndarray, Dict[str, np.ndarray]]:
    """the oracle in float64 under autograd: (raw, {name: d (raw . grad_raw).sum() / d parameter})"""
    P, aux, audio, grad_raw, drop = _inputs(cfg, sd, aux, audio, grad_raw, drop)
    if cfg.kind == "softmax":
        raw, _ = cpu_ref.softmax_stack(cfg, P, audio, aux, drop=drop)
    else:
        raw, _ = cpu_ref.laplace_stack(cfg, P, aux, audio, drop=drop)
    raw.backward(grad_raw)
    return raw.detach().numpy().copy(), _grads(P)


def rounded(cfg, sd, aux, audio, grad_raw, drop=None, path: Optional[str] = "fused", want_pre: bool = False, dtype=torch.float64):
    """the same graph with the roundings of `path` (module docstring); path=None: none, bit for bit `exact`.  dtype =
    torch.float32 evaluates everything between the roundings in fp32, as the device does"""
    P, aux, audio, grad_raw, drop = _inputs(cfg, sd, aux, audio, grad_raw, drop, dtype)
    raw, pre = _stack(Model.of(path, drop is not None), cfg, P, aux, audio, drop)
    raw.backward(grad_raw)
    out = (raw.detach().numpy().copy(), _grads(P))
    return out + (tuple(p.detach().numpy().copy() for p in pre),) if want_pre else out


def rows_of(name: str, g: np.ndarray) -> Optional[np.ndarray]:
    """2-D / 3-D weights the assertions also hold per row of the leading axis: (rows, -1) view, else None"""
    if g.ndim >= 2 and name.endswith("weight") and name.startswith(ROW_TENSORS):
        return g.reshape(g.shape[0], -1)
    return None


@dataclasses.dataclass
class Yardstick:
    raw: np.ndarray                       # exact raw (B, n_out, Tp)
    g: Dict[str, np.ndarray]              # exact gradients
    g_rounded: Dict[str, np.ndarray]
    D: Dict[str, float]                   # ||g_rounded - g_exact|| per tensor
    D_rows: Dict[str, np.ndarray]         # the same per row (ROW_TENSORS)
    D_fwd: float                          # max |raw_rounded - raw_exact|
    pre_min: float                        # smallest |pre-activation| of the two ReLUs at the probed positions (either graph)
    flips: int                            # ReLU units at probed positions on different sides of zero in the two graphs

    @property
    def D_max(self) -> float:
        return max(self.D.values())


def yardstick(cfg, sd, aux, audio, grad_raw, drop=None, path="fused") -> Yardstick:
    raw_e, g_e, pre_e = rounded(cfg, sd, aux, audio, grad_raw, drop, None, want_pre=True)     # = exact, bit for bit
    raw_r, g_r, pre_r = rounded(cfg, sd, aux, audio, grad_raw, drop, path, want_pre=True)
    probed = np.abs(np.asarray(grad_raw)).max(axis=1) > 0                              # (B, Tp)
    at = lambda p: p.transpose(0, 2, 1)[probed]
    pre_min = min(float(np.abs(at(p)).min()) for p in pre_e + pre_r) if probed.any() else float("inf")
    flips = sum(int(((at(a) > 0) != (at(b) > 0)).sum()) for a, b in zip(pre_e, pre_r))
    D = {k: float(np.linalg.norm((g_r[k] - g_e[k]).ravel())) for k in g_e}
    D_rows = {}
    for k in g_e:
        r = rows_of(k, g_e[k])
        if r is not None:
            D_rows[k] = np.linalg.norm(rows_of(k, g_r[k]) - r, axis=1)
    return Yardstick(raw_e, g_e, g_r, D, D_rows, float(np.abs(raw_r - raw_e).max()), pre_min, flips)


# ------------------------------------------------------------------------------------------------ probes and cases
def edge_positions(cfg, Tf: int) -> List[int]:
    """the positions at which an indexing slip of the backward kernels shows (sorted, inside [0, Tp))"""
    soft = cfg.kind == "softmax"
    coff = 1 if soft else cfg.seg
    U = cfg.U
    Tp = Tf * U - 1 if soft else Tf * U - 2 * cfg.seg + 1
    d, rf = max(cfg.dilations), cfg.receptive_field
    pos = {0, 1, Tp - 2, Tp - 1, d - 1, d, d + 1, rf - 1, rf}
    for tile in (16, 32, 64, 128, 192):            # layer chunk, bl6_wgrad tile, bl6_head_bwd tile, time / reduce GEMM and gate tiles
        pos |= {tile - 1, tile}
        last = (Tp - 1) // tile * tile                # the last whole tile boundary below Tp
        pos |= {last - 1, last}
    for k in (1, 2):                               # both sides of the first two conditioning-frame boundaries
        pos |= {k * U - coff - 1, k * U - coff}
    return sorted(p for p in pos if 0 <= p < Tp)


RELU_SIGMAS = 2.0
PRE_MIN = 1e-5           # (1e-4 in dropout mode)
DROP_SEEDS = (301, 527)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    geom: str                    # "bl6" | "ref6" | "ref6_s5" | "ref6_softmax" | "ref6_softmax_audio_in"
    path: str                    # one of PATHS: the backward the case must run
    probe: str                   # "dense" | "edges" | "single"
    B: int = 2
    Tf: int = 3
    U: Optional[int] = None      # upsampling factor (default: the geometry's)
    lpc: Optional[int] = None
    frames: Optional[Tuple[int, ...]] = None   # utterances zero-padded to these numbers of frames
    at: Optional[Tuple[int, int]] = None       # single probe: (utterance, position), negative = from the end
    drop: bool = False
    seed: int = 1

    @property
    def relu_sigmas(self) -> Optional[float]:
        """where the two ReLUs' pre-activations are centred, in standard deviations (None: where the synthetic net has them)"""
        if self.probe == "single":
            return None
        return 3.0 if self.B * self.Tf > 100 else RELU_SIGMAS      # 17 million units: one in 10 000 on the other side is too many

    def cfg(self):
        if self.geom == "bl6":
            cfg = C.bl6_laplace(1, 0 if self.lpc is None else self.lpc)
        elif self.geom == "ref6":
            cfg = C.ref6_laplace(1, 4)
        elif self.geom == "ref6_s5":
            cfg = C.ref6_laplace(5, 4)
        elif self.geom == "ref6_softmax":
            cfg = C.ref6_softmax()
        elif self.geom == "ref6_softmax_audio_in":
            cfg = dataclasses.replace(C.ref6_softmax(), audio_in_flag=True)
        else:
            raise ValueError(self.geom)
        return cfg if self.U is None else dataclasses.replace(cfg, upsampling_factor=self.U)

    @property
    def pre_min(self) -> float:
        """the gap around zero no ReLU pre-activation at a probed position may lie in: the device's fp32 sums differ from the
        float64 ones by about 1e-6 at these magnitudes"""
        return 1e-4 if self.drop else PRE_MIN

    @property
    def margin_group(self) -> str:
        """one margin per path (and arithmetic of the forward)"""
        return self.path + ("+drop" if self.drop else "")


def cases() -> List[Case]:
    """the seeds of the `edges` and `single` cases are the first (from the case's number, then 200 upwards) at which no ReLU
    unit at a probed position lies on different sides of zero in the exact and the rounded graph and none is within
    PRE_MIN of zero in either (test_mixed_reference.py asserts both)"""
    out = []
    # BL6 class, fused backward: both lpc settings, the covered range of upsampling factors (16 .. 112; 37 and 110 leave ragged
    # 16-chunks), one batch of utterances zero-padded to different lengths
    for U, lpc, Tf, probe, seed in ((110, 0, 3, "edges", 229), (110, 2, 3, "dense", 112), (37, 0, 5, "edges", 202), (37, 2, 5, "dense", 39),
                                    (16, 0, 5, "edges", 209), (112, 2, 2, "edges", 200)):
        out.append(Case(f"bl6-fused-U{U}-lpc{lpc}-{probe}", "bl6", "fused", probe, B=2, Tf=Tf, U=U, lpc=lpc, seed=seed))
    out.append(Case("bl6-fused-U110-ragged-edges", "bl6", "fused", "edges", B=3, Tf=4, frames=(4, 3, 2), seed=203))
    for i, (at, seed) in enumerate((((1, 0), 20), ((0, -1), 200), ((-1, -1), 201))):
        out.append(Case(f"bl6-fused-U110-single{i}", "bl6", "fused", "single", B=3, Tf=2, at=at, seed=seed))
    out.append(Case("bl6-fused-U37-single1", "bl6", "fused", "single", B=2, Tf=3, U=37, lpc=2, at=(0, -1), seed=200))
    # BL6 class through the generic chain
    for U, probe, seed in ((110, "edges", 229), (37, "edges", 202), (110, "dense", 140)):
        out.append(Case(f"bl6-chain-U{U}-{probe}", "bl6", "chain", probe, B=2, Tf=3 if U == 110 else 5, U=U, seed=seed))
    for i, at in enumerate(((1, 0), (0, -1), (-1, -1))):
        out.append(Case(f"bl6-chain-U37-single{i}", "bl6", "chain", "single", B=3, Tf=3, U=37, at=at, seed=40 + i))
    # run.sh geometry (H = 192, K = 7), seg 1 lpc 4: kept and recomputed pre-activations
    for path in ("keep", "recompute"):
        out.append(Case(f"ref6-{path}-edges", "ref6", path, "edges", B=2, Tf=3, seed=227))
        out.append(Case(f"ref6-{path}-dense", "ref6", path, "dense", B=2, Tf=3, seed=51))
        for i, (at, seed) in enumerate((((1, 0), 52), ((0, -1), 200), ((-1, -1), 201))):
            out.append(Case(f"ref6-{path}-single{i}", "ref6", path, "single", B=3, Tf=2, at=at, seed=seed))
    # the gate's 192-position tiles need 8 x 38 frames (33 000 positions: the only slow case, the oracle runs once)
    out.append(Case("ref6-keep-wide-edges", "ref6", "keep", "edges", B=8, Tf=38, seed=56))
    # seg 5: the conditioning through the reduce / time GEMMs
    out.append(Case("ref6s5-keep-edges", "ref6_s5", "keep", "edges", B=2, Tf=3, seed=207))
    out.append(Case("ref6s5-keep-single1", "ref6_s5", "keep", "single", B=2, Tf=2, at=(0, -1), seed=200))
    # softmax, H = 256
    out.append(Case("smx-keep-edges", "ref6_softmax", "keep", "edges", B=2, Tf=3, seed=70))
    out.append(Case("smx-keep-single0", "ref6_softmax", "keep", "single", B=2, Tf=2, at=(1, 0), seed=200))
    out.append(Case("smx-keep-single2", "ref6_softmax", "keep", "single", B=2, Tf=2, at=(-1, -1), seed=201))
    out.append(Case("smx-ai-keep-edges", "ref6_softmax_audio_in", "keep", "edges", B=2, Tf=3, seed=243))
    out.append(Case("smx-ai-keep-single0", "ref6_softmax_audio_in", "keep", "single", B=2, Tf=2, at=(1, 0), seed=71))
    out.append(Case("smx-ai-keep-single2", "ref6_softmax_audio_in", "keep", "single", B=2, Tf=2, at=(-1, -1), seed=72))
    # one step in dropout mode (host masks, p = 0.5)
    out.append(Case("bl6-fused-drop-edges", "bl6", "fused", "edges", B=2, Tf=3, drop=True, seed=DROP_SEEDS[0]))
    out.append(Case("ref6-keep-drop-edges", "ref6", "keep", "edges", B=2, Tf=3, drop=True, seed=DROP_SEEDS[1]))
    return out


def inputs_of(case: Case):
    """-> (cfg, sd, aux, audio, grad_raw, drop) as numpy / torch CPU tensors in the dtypes the HIP entry points take"""
    from shallow_wavenet_amd.synth import synth_aux, synth_state_dict
    cfg = case.cfg()
    soft = cfg.kind == "softmax"
    B, Tf = case.B, case.Tf
    sd = synth_state_dict(cfg, seed=3 + case.seed, flavor="trained", identity_scale_in=True)
    aux = synth_aux(cfg, B, Tf, seed=case.seed)
    if case.frames is not None:
        for b, f in enumerate(case.frames):
            aux[b, :, f:] = 0.0
    T = Tf * cfg.U
    g = torch.Generator().manual_seed(case.seed)
    if soft:
        audio = torch.randint(0, cfg.n_quantize, (B, T - 1), generator=g)
        Tp = T - 1
    else:
        audio = torch.rand(B, 1, T - cfg.seg, generator=g) * 1.8 - 0.9
        Tp = T - 2 * cfg.seg + 1
    noise = torch.randn(B, cfg.n_out, Tp, generator=g)
    if case.probe == "dense":
        grad_raw = noise / Tp
    elif case.probe == "edges":
        pos = edge_positions(cfg, Tf)
        grad_raw = torch.zeros_like(noise)
        grad_raw[:, :, pos] = noise[:, :, pos] / len(pos)
    elif case.probe == "single":
        b, t = case.at
        grad_raw = torch.zeros_like(noise)
        grad_raw[b % B, :, t % Tp] = noise[b % B, :, t % Tp]
    else:
        raise ValueError(case.probe)
    drop = None
    if case.drop:
        from shallow_wavenet_amd import noise as swn_noise
        drop = swn_noise.dropout_masks(cfg, B, Tf, 0.5, generator=torch.Generator().manual_seed(100 + case.seed))
    if case.relu_sigmas is not None:
        # centre the skip sum, then the out_1 pre-activation, at relu_sigmas standard deviations (module docstring, "ReLU kinks")
        for which, name in enumerate(("out_skip.0.bias", "out_1.bias")):
            with torch.no_grad():
                P, a64, au64, _, d64 = _inputs(cfg, sd, aux, audio, grad_raw, drop)
                pre = _stack(Model(), cfg, P, a64, au64, d64)[1][which]
            sd[name] = sd[name] + np.float32(case.relu_sigmas * float(pre.std()) - float(pre.mean()))
    return cfg, sd, aux, audio, grad_raw, drop


def gpu_run(case: Case, inp=None):
    """the case through HipNet.forward_train / HipNet.backward under train_precision("bf16") and the device-side unfold of the
    packed gradient (what the modules' autograd runs) -> (raw, {state-dict name: gradient}) as float64 numpy.  Asserts that
    the path the case names is the one that ran."""
    from shallow_wavenet_amd import _lib, ops
    from shallow_wavenet_amd.nets._autograd import unfold_packed_grads, unfold_packed_grads_device
    from shallow_wavenet_amd.runtime import HipNet, train_precision
    cfg, sd, aux, audio, grad_raw, drop = inp if inp is not None else inputs_of(case)
    net = HipNet.from_state_dict(cfg, sd, "cuda:0")
    net.fused_backward = case.path == "fused"
    net.keep_preactivations = case.path == "keep"
    with train_precision("bf16"):
        raw, saved = net.forward_train(torch.from_numpy(aux).cuda(), audio.cuda(), drop=drop)
        assert saved["precision"] == _lib.PRECISION_BF16
        if drop is None:
            assert saved.get("work_bf16") is not None, "the bf16 forward did not engage"
            assert (saved.get("a_keep") is not None) == (case.path == "keep"), "kept pre-activations: not as the case asks"
            fused = ops.backward_bf16_supported(net.dlist, case.B, case.Tf) and net.fused_backward
            assert fused == (case.path == "fused"), "fused backward: not as the case asks"
            assert (saved["work"] is None) == fused
        else:
            assert saved.get("drop") is not None
            import ctypes
            ptrs = (ctypes.c_void_p * cfg.L)(*[None if q is None else q.data_ptr() for q in saved["drop"][1]])
            took = net.lib.swn_drop_fused_path(ctypes.byref(net.desc), case.B, case.Tf, ctypes.cast(ptrs, ctypes.c_void_p))
            assert took == (1 if case.path == "fused" else 0), "fused dropout step: not as the case asks"
        gp = net.backward(saved, grad_raw.cuda())
    torch.cuda.synchronize()
    names = [k for k, _ in cfg.param_shapes()]
    params = [torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)).cuda() for k in names]
    out = unfold_packed_grads_device(net, gp, params, [True] * len(params))
    if out is None:
        g = unfold_packed_grads(cfg, gp, dict(zip(names, params)))
        out = [g[k].reshape(p.shape) for k, p in zip(names, params)]
    return raw.double().cpu().numpy(), {k: o.double().cpu().numpy() for k, o in zip(names, out)}


BF16_EPS = 2.0 ** -8          # largest relative error of one rounding to bf16 (8 significant bits, round to nearest)


def row_yardstick(case: Case, y: Yardstick, k: str) -> np.ndarray:
    """D_row plus the quantisation scale of the row.  D_row is ONE realisation of the row's rounding errors, and which one is
    decided by rounding decisions upstream: the same model evaluated in float32 instead of float64 between its roundings
    (`rounded(..., dtype=torch.float32)`, no device involved) lands 0.3-0.4 D_k from the float64 evaluation at tensor level - a
    handful of the thousands of stored values sit close enough to a bf16 tie for 1e-7 to decide them, and everything downstream
    of a flipped value moves by part of a step - and single rows of it stand at 2.5-2.7 D_row.  The device (fp32 sums in another
    order, the exp2 / rcp unit) is a third evaluation of that kind.  Where a row is a sum over many positions this averages
    out and the row follows D_row (measured 0.85-1.0); where it is ONE rounded scalar times a rounded vector - g in_x under a
    single-position probe: d cond[o][f], and d gx before it where that is stored as bf16 - its error is one draw of up to
    BF16_EPS ||g_row|| per rounding in series, of which D_row can be arbitrarily small (measured: device rows at 0.4-1.0 % of
    ||g_row|| next to D_row = 0.17 %).  So the yardstick of a row is D_row + n BF16_EPS ||g_row||, n = the roundings a scalar
    passes in series (2 where d gx is stored as bf16, else 1): the step of the number format, not a measured figure.
    test_mixed_reference.py holds the float32 evaluation of the model to the bounds of the GPU file, rows included.  Rows of
    wav_conv.weight are sums over ALL channels of the causal layer's gradient times causal.conv.weight - cancelling terms: their
    error follows the tensor's, D_k / sqrt(rows), not the row's own norm."""
    g = rows_of(k, y.g[k])
    n = 2 if (case.path == "keep" or case.drop) else 1
    yard = y.D_rows[k] + n * BF16_EPS * np.linalg.norm(g, axis=1)
    if k == "wav_conv.weight":
        yard = yard + y.D[k] / np.sqrt(g.shape[0])
    return yard + FLOOR * y.D_max / np.sqrt(g.shape[0])


def violations(case: Case, d: Dict) -> List:
    """what of `deviations` lies outside the bounds of the GPU file: one margin per path for tensors and rows, one for the forward"""
    m, mf = MARGIN[case.margin_group], MARGIN_FWD[case.margin_group]
    bad = [("exactly zero", n) for n in d["nonzero"]]
    if d["fwd_err"] > mf * d["D_fwd"]:
        bad.append(("forward", d["fwd_err"], d["D_fwd"]))
    for k, t in d["tensors"].items():
        if t["err"] > m * (t["D"] + FLOOR * d["D_max"]):
            bad.append((k, t["err"], t["D"]))
        if "rows_err" in t:
            rr = t["rows_err"] / t["rows_yard"]
            if rr.max() > m:
                bad.append((k, "row", int(rr.argmax()), float(rr.max())))
    return bad


def deviations(case: Case, y: Yardstick, raw: np.ndarray, g: Dict[str, np.ndarray]) -> Dict:
    """errors of a result against the exact gradients next to their yardsticks: per tensor (err, D), per row of the
    ROW_TENSORS (err_row, row_yardstick), the forward (max |raw - raw_exact|, D_fwd), and the slices that must be exactly
    zero and are not."""
    out = {"D_max": y.D_max, "D_fwd": y.D_fwd, "fwd_err": float(np.abs(raw - y.raw).max()), "tensors": {}, "nonzero": []}
    for k, ge in y.g.items():
        e = g[k] - ge
        t = {"err": float(np.linalg.norm(e.ravel())), "D": y.D[k], "norm": float(np.linalg.norm(ge.ravel())),
             "model": float(np.linalg.norm((g[k] - y.g_rounded[k]).ravel()))}
        r = rows_of(k, e)
        if r is not None:
            t["rows_err"] = np.linalg.norm(r, axis=1)
            t["rows_yard"] = row_yardstick(case, y, k)
        out["tensors"][k] = t
        # a slice (tensor, tap) whose exact gradient is zero - nothing of the probe reaches it - must be exactly zero
        parts = [(f"{k}[:, :, {j}]", ge[..., j], g[k][..., j]) for j in range(ge.shape[-1])] if ge.ndim == 3 and ge.shape[-1] > 1 else [(k, ge, g[k])]
        for name, a, b in parts:
            if not a.any() and b.any():
                out["nonzero"].append(name)
    return out


_YARD: Dict[str, Yardstick] = {}


def yardstick_of(case: Case) -> Yardstick:
    """computed once per process and case, shared by the tests that need it, never modified"""
    if case.name not in _YARD:
        cfg, sd, aux, audio, grad_raw, drop = inputs_of(case)
        _YARD[case.name] = yardstick(cfg, sd, aux, audio, grad_raw, drop, case.path)
    return _YARD[case.name]


# Margins: twice the worst ratio ||g_gpu - g_exact|| / (D_k + FLOOR D_max) tools/measure_mixed_deviation.py measured on an MI355X
# per path, over all its cases, two runs each (profiles/mixed_backward_deviation.json; measured worst in brackets).  One value
# per path; rows are held to the same m (their measured worst: 1.18, 1.00, 1.58, 1.11, 0.92, see the profile).  FLOOR: the fp32
# sums of the device against float64 - about 1e-6 of a tensor's norm, while D_max is some 5e-3 of the largest norm - for the
# tensors whose D_k is zero or tiny (out_2.bias outside the fused path: exact row sums of the upstream gradient; the scalar
# upsampler bias, a sum of cancelling terms): floor_k = m FLOOR D_max.
MARGIN: Dict[str, float] = {"fused": 2.1, "chain": 2.2, "keep": 2.3, "recompute": 2.1,          # (1.03, 1.08, 1.11, 1.04)
                            "fused+drop": 2.3, "keep+drop": 2.0}                                # (1.13, 1.00)
MARGIN_FWD: Dict[str, float] = {"fused": 2.0, "chain": 2.1, "keep": 2.3, "recompute": 2.1,      # (1.00, 1.05, 1.12, 1.01)
                                "fused+drop": 2.2, "keep+drop": 2.0}                            # (1.07, 1.00)
FLOOR = 1e-3


def old_bound(case: Case, y: Yardstick, k: str) -> float:
    """what test_gpu_train_bf16.py / test_gpu_fused_backward.py allow the tensor: 5e-2 ||g|| + 1e-3 of the largest tensor
    norm (1e-1 for the softmax nets)"""
    big = max(float(np.linalg.norm(v.ravel())) for v in y.g.values())
    tol = 1e-1 if case.geom.startswith("ref6_softmax") else 5e-2
    return tol * float(np.linalg.norm(y.g[k].ravel())) + 1e-3 * big
