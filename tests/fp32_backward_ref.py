"""float64 yardstick for the backward of the fp32 training mode (`train_precision("fp32")`, the default and the mode every
reference-parity claim rests on), the sibling of tests/mixed_ref.py.  Test helper (not collected):
tests/test_fp32_backward_reference.py verifies it on the CPU, tests/test_gpu_fp32_backward_edges.py and
tools/measure_fp32_backward_deviation.py hold the HIP kernels of csrc/swn_train.hip against it.

  evaluate(cfg, sd, aux, audio, grad_raw, drop, dtype)   oracle/cpu_ref.py (laplace_stack / softmax_stack) under torch autograd
        with parameters from as_params(sd, dtype), raw.backward(grad_raw) -> raw, {state-dict name: gradient}, the hidden states
        and the pre-activations of the two ReLUs (skip sum, out_1), restated from the hidden states op for op.
  yardstick(...)   the oracle once in float64 (g_exact, raw_exact) and once in float32 (g_32, raw_32):
        D_k = ||g_32 - g_exact|| per tensor, D_row the same per row of the leading axis of the ROW_TENSORS weights,
        D_fwd = max |raw_32 - raw_exact|, D_hs the same over the hidden states.  That is the error inherent in fp32 arithmetic
        for exactly this input and upstream gradient, computed without the code under test.  Going through cpu_ref itself
        (not mixed_ref.Model) brings the aux_conv2d and off-grid nets in.

Bounds (one margin m per path for tensors and rows, one m_f for the forward; MARGIN / MARGIN_FWD below, measured):
    per tensor     ||g_gpu - g_exact||  <=  m (D_k + FLOOR D_max / sqrt(n_k))          D_max the largest D_k of the case, n_k the
                                                                                   number of elements of the tensor
    per row        ||row of the error|| <=  m (D_row + N_SERIES 2^-24 ||g_row|| + FLOOR D_max / sqrt(n_k))
    forward        max |raw_gpu - raw_exact| <= m_f D_fwd   (hidden states: m_f D_hs where the entry returns them)
    exact zeros    a slice of a tensor (an index of any axis: a row, an input column, a tap) whose exact gradient is exactly zero
                   is exactly zero on the device: a `single` probe at t = 0 reaches no earlier tap, a tap that no probed
                   position reaches, rows of out_skip / out_1 (and columns of out_1 / out_2) behind a ReLU unit that is dead at
                   every probed position, classes of the one-hot input that do not occur.

N_SERIES = 16.  Under a single-position probe a row of a weight gradient is ONE product chain, and D_row is one draw of its
rounding errors, which can be arbitrarily small.  The chain from d raw to an element of g in_x / g dil_h passes, in series:
the out_2^T, out_1^T and out_skip^T products (3), dh (hprev - c) (2), z (1 - z) (2), the factor gz or sz (1), sigmoid as
exp, add, divide (3), tanh and 1 - c c (3), the product gz sz under them (1), the final product with the stored input (1):
16 roundings of at most 2^-24 relative each, so the row may stand 16 x 2^-24 ||g_row|| from float64 with none of them wrong.
This is the step of the number format, as BF16_EPS is in mixed_ref.row_yardstick; no measured figure enters it.
FLOOR = 2^-3, shrinking with the square root of the tensor's size.  D_k over n_k elements is the norm of n_k rounding draws: its
own relative spread is 1 / sqrt(2 n_k), so for a matrix it cannot be small by chance, and the floor it gets, at most
2^-3 D_max / sqrt(n_k), is below 1 % of D_max from 160 elements on (never above the FLOOR D_max of the plain form, and for the
rows never above FLOOR D_max / sqrt(rows)).  A tensor that is ONE number (upsampling.conv.bias) or a handful (out_2.bias) has a D_k
that is a single draw from a centred distribution of some width s, and the device's error is another draw of that width:
measured, the oracle's draw for the upsampler bias was 6e-10 of the value in one case - a hundredth of one fp32 rounding -
next to a device error of 4 roundings that moves by half of itself from run to run (float atomics).  Both tensors are sums
over every position of the terms the other gradients are made of, so s is of the order of the case's D_max; a normal draw
falls below an eighth of its width once in ten times, and then the floor holds the scalar to an eighth of D_max instead.
(out_2.bias under a `single` probe is the upstream gradient itself: D_k = 0 and the device's error is 0 as well.)

Where the device stands (profiles/fp32_backward_deviation.json).  Every tensor of the stack - dil_h, in_x, out_skip, out_1, out_2, the
input layer - sits at 0.6-1.2 D_k: the device is as close to float64 as the fp32 oracle is.  The frame-rate front end (conv_aux,
scale_in) stands at 1.4-2 D_k on the nets with N = L seg 2H = 384 in_x products per frame and at 3-5 on the seg 5 / seg 7 nets
(N = 1 920, 1 512): d C = W_inx^T d cond is ONE contraction over N on the device, accumulated in k order by the fp32 MFMA chain,
where the oracle sums per layer over 2H channels and then over layers and positions.  A serial fp32 sum of n products of random
sign stands sqrt(n) / 1.4 roundings from the exact one, a blocked one a few: restated in numpy (4 products per accumulate, as
the 16x16x4 MFMA; 200 draws) the serial sum's error is 2.0 times the blocked sum's at n = 384 and 3.4 times at n = 1 920 - the
measured ratios.  Its size is 1e-6 of the tensor's norm; no index or operand is wrong, so it gets its margin.  The forward
stands at 0.05-0.16 D_fwd on the Laplace nets (the device's FMA chains are closer to float64 than the CPU's fp32 convolutions) and at
0.6-1.2 on the softmax nets.

ReLU kinks.  fp32 and float64 decide a ReLU differently only within about 1e-6 of zero.  mixed_ref's rule is kept: every
case's seed is the first, from the case's number upwards, at which in BOTH evaluations no pre-activation of either ReLU at a
probed position lies within PRE_MIN = 1e-5 of zero, and none lies on different sides of zero.  `dense` / `edges` cases centre the
skip sum and the out_1 pre-activation two standard deviations above zero (`inputs_of`, as mixed_ref.inputs_of), `single` cases
keep the synthetic nets' own biases.  test_fp32_backward_reference.py asserts both properties for every case: no case runs
with a flip present.

Launch arithmetic (`launch_facts`): which kernel instantiation, how many tiles, segments and frames per workgroup a case
reaches, restated from launch_time, launch_reduce, BwdCall::cond_layer, BwdCall::frontend and swn_train_path
(csrc/swn_train.hip, csrc/swn_train_internal.hpp).  Each case carries the facts it exists for in `expect`; the CPU test
asserts them, so a case that silently stops reaching its edge fails without a GPU.
  time_gemm_kernel<false>   64(m) x 64(t) tiles, 1-D grid 8 ceil(ntt B / 8) mtl, each XCD walks ceil(ntt B / 8) (tile, utterance)
                            pairs; k loop 48 deep over Kd = taps x channels, the tail tiles read zeros.  (XMUL = true is never
                            launched: nothing sets TimeGemm::xmul, the masked input goes through mask_mul_kernel.)
  reduce_gemm_kernel        time segments of 512 positions, B x segments spread over the XCDs in groups of 8, float atomics
  gate_bwd_kernel           256 positions per workgroup
  cond_bwd_kernel<2 | 5>    ceil((U + seg - 1) / 64) column chunks <= 2 -> <2>, else <5>; FR = clamp(rb Tf B / 768, 1, 16) frames
                            per workgroup, rb = ceil(2H / 64)
  xm_bwd_kernel             dropout mode; FR = clamp(ceil(A0 / 32) Tf B / 1024, 1, 16)
  dropout mode, seg == 1: every layer's d gx kept (dgx_all), one in_x contraction pair behind the layers (inx_all);
  seg > 1: per layer (inx_layer), the accumulating time GEMM with XT = Tp and the reduce GEMM with QT = Tx.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import mixed_ref as M
from oracle import cpu_ref
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.config import NetConfig

PATHS = ("chain", "drop1", "dropN")
PRE_MIN = 1e-5
RELU_SIGMAS = 2.0
FP32_EPS = 2.0 ** -24         # largest relative error of one rounding to fp32 (round to nearest)
N_SERIES = 16                 # roundings a single-probe row passes in series (module docstring)
FLOOR = 2.0 ** -3             # (module docstring)


# ------------------------------------------------------------------------------------------------ nets
def _frontend_row(rid: str) -> NetConfig:
    import frontend_geometry as FG
    return FG.BY_ID[rid].cfg


NETS = {
    "tiny": lambda: C.tiny("laplace", 1, 0),
    "tiny_s2": lambda: C.tiny("laplace", 2, 0),
    "tiny_s5": lambda: C.tiny("laplace", 5, 4),
    "tiny_smx": lambda: C.tiny("softmax", wav_conv_flag=False),
    "tiny_smx_ai": lambda: C.tiny("softmax", wav_conv_flag=True, audio_in_flag=True),
    "bl6": lambda: C.bl6_laplace(1, 0),
    "ref6": lambda: C.ref6_laplace(1, 4),
    # the g10 geometries off the tiny / bl6 / ref6 grid that the backward serves (tests/test_gpu_offgrid_geometry.py)
    "h20k5": lambda: NetConfig(kind="laplace", n_aux=3, hid_chn=20, skip_chn=33, aux_kernel_size=5, aux_dilation_size=2, dilation_depth=2,
                               dilation_repeat=2, kernel_size=5, upsampling_factor=7, seg=1, lpc=1),
    "h36s7": lambda: NetConfig(kind="laplace", n_aux=6, hid_chn=36, skip_chn=20, aux_kernel_size=1, aux_dilation_size=1, dilation_depth=3,
                               dilation_repeat=1, kernel_size=2, upsampling_factor=21, seg=7, lpc=0, wav_conv_flag=True),
    "s4c2d": lambda: NetConfig(kind="laplace", n_aux=5, hid_chn=24, skip_chn=18, aux_kernel_size=3, aux_dilation_size=3, dilation_depth=1,
                               dilation_repeat=3, kernel_size=4, upsampling_factor=12, seg=4, lpc=5, wav_conv_flag=True,
                               aux_conv2d_flag=True),
    "q90": lambda: NetConfig(kind="softmax", n_aux=5, hid_chn=28, skip_chn=30, aux_kernel_size=3, aux_dilation_size=2, dilation_depth=4,
                             dilation_repeat=1, kernel_size=2, upsampling_factor=9, n_quantize=90, audio_in_flag=True),
    "q300": lambda: NetConfig(kind="softmax", n_aux=4, hid_chn=44, skip_chn=70, aux_kernel_size=3, aux_dilation_size=1, dilation_depth=2,
                              dilation_repeat=2, kernel_size=3, upsampling_factor=11, n_quantize=300, wav_conv_flag=True),
    # front end geometries (tests/frontend_geometry.py; the rows with H % 4 == 0, which the backward serves): aux kernel 1 / 3 / 5,
    # 1 and 3 layers (the tiny net has 2), the (seg, 1) Conv2d folded into in_x
    "fe_k1l1": lambda: _frontend_row("k1l1_a16"),
    "fe_k3l3": lambda: _frontend_row("k3l3_a12"),
    "fe_k5l3": lambda: _frontend_row("k5l3_a2"),
    "fe_k3l4": lambda: _frontend_row("k3l4_a9"),
}


def seg_of(cfg) -> int:
    return 1 if cfg.kind == "softmax" else cfg.seg


def tp_of(cfg, Tf: int) -> int:
    return Tf * cfg.U - 1 if cfg.kind == "softmax" else Tf * cfg.U - 2 * cfg.seg + 1


# ------------------------------------------------------------------------------------------------ oracle
def _pre_activations(cfg, P, hs) -> Tuple[torch.Tensor, torch.Tensor]:
    """the skip sum and the out_1 pre-activation, from the hidden states with the ops of cpu_ref.gated_layer / cpu_ref.head in
    their order (bit for bit what the graph holds)"""
    tot = None
    for l in range(cfg.L):
        sk = F.conv1d(hs[l + 1], P[f"out_skip.{l}.weight"], P[f"out_skip.{l}.bias"])
        tot = sk if tot is None else tot + sk
    return tot, F.conv1d(F.relu(tot), P["out_1.weight"], P["out_1.bias"])


def _forward(cfg, P, aux, audio, drop):
    if cfg.kind == "softmax":
        return cpu_ref.softmax_stack(cfg, P, audio, aux, drop=drop)
    return cpu_ref.laplace_stack(cfg, P, aux, audio, drop=drop)


@dataclasses.dataclass
class Evaluation:
    raw: np.ndarray                       # (B, n_out, Tp) float64
    g: Dict[str, np.ndarray]              # float64
    hs: np.ndarray                        # (B, L + 1, H, Tp)
    pre: Tuple[np.ndarray, np.ndarray]    # skip sum (B, S, Tp), out_1 pre-activation (B, O1, Tp)


def evaluate(cfg, sd, aux, audio, grad_raw, drop=None, dtype=torch.float64) -> Evaluation:
    P, aux, audio, grad_raw, drop = M._inputs(cfg, sd, aux, audio, grad_raw, drop, dtype)
    raw, hs = _forward(cfg, P, aux, audio, drop)
    with torch.no_grad():
        pre = _pre_activations(cfg, P, [h.detach() for h in hs])
    raw.backward(grad_raw)
    return Evaluation(raw.detach().double().numpy().copy(), M._grads(P), torch.stack([h.detach() for h in hs], 1).double().numpy(),
                      tuple(p.double().numpy() for p in pre))


rows_of = M.rows_of


@dataclasses.dataclass
class Yardstick:
    raw: np.ndarray
    hs: np.ndarray
    g: Dict[str, np.ndarray]              # exact gradients
    g32: Dict[str, np.ndarray]
    D: Dict[str, float]
    D_rows: Dict[str, np.ndarray]
    D_fwd: float
    D_hs: float
    pre_min: float                        # smallest |pre-activation| of the two ReLUs at the probed positions (either evaluation)
    flips: int                            # ReLU units at probed positions on different sides of zero in the two evaluations

    @property
    def D_max(self) -> float:
        return max(self.D.values())


def _kinks(grad_raw, e64: Evaluation, e32: Evaluation) -> Tuple[float, int]:
    probed = np.abs(np.asarray(grad_raw)).max(axis=1) > 0                              # (B, Tp)
    at = lambda p: p.transpose(0, 2, 1)[probed]
    pre_min = min(float(np.abs(at(p)).min()) for p in e64.pre + e32.pre) if probed.any() else float("inf")
    flips = sum(int(((at(a) > 0) != (at(b) > 0)).sum()) for a, b in zip(e64.pre, e32.pre))
    return pre_min, flips


def yardstick(cfg, sd, aux, audio, grad_raw, drop=None) -> Yardstick:
    e64 = evaluate(cfg, sd, aux, audio, grad_raw, drop, torch.float64)
    e32 = evaluate(cfg, sd, aux, audio, grad_raw, drop, torch.float32)
    pre_min, flips = _kinks(grad_raw, e64, e32)
    D = {k: float(np.linalg.norm((e32.g[k] - e64.g[k]).ravel())) for k in e64.g}
    D_rows = {}
    for k in e64.g:
        r = rows_of(k, e64.g[k])
        if r is not None:
            D_rows[k] = np.linalg.norm(rows_of(k, e32.g[k]) - r, axis=1)
    return Yardstick(e64.raw, e64.hs, e64.g, e32.g, D, D_rows, float(np.abs(e32.raw - e64.raw).max()),
                     float(np.abs(e32.hs - e64.hs).max()), pre_min, flips)


# ------------------------------------------------------------------------------------------------ probes and cases
TILES = (16, 64, 256, 512)       # 64: time tile of the GEMMs, column chunk of cond_bwd_kernel; 256: gate / input kernels; 512: reduce segment


def edge_positions(cfg, Tf: int) -> List[int]:
    """the positions at which an indexing slip of the fp32 backward kernels shows (sorted, inside [0, Tp))"""
    seg, U, Tp = seg_of(cfg), cfg.U, tp_of(cfg, Tf)
    coff = seg
    d, rf = max(cfg.dilations), cfg.receptive_field
    pos = {0, 1, Tp - 2, Tp - 1, d - 1, d, d + 1, rf - 1, rf}
    for tile in TILES:
        last = (Tp - 1) // tile * tile                # the last whole tile boundary below Tp
        pos |= {tile - 1, tile, last - 1, last}
    for k in (1, 2):                                  # both sides of the first two conditioning-frame boundaries, as the first and
        for s in {0, seg - 1}:                        # the last of a position's seg conditioning columns cross them
            pos |= {k * U - coff - s - 1, k * U - coff - s}
    return sorted(p for p in pos if 0 <= p < Tp)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    net: str                     # key of NETS
    path: str                    # one of PATHS
    probe: str                   # "dense" | "edges" | "single"
    B: int = 2
    Tf: int = 3
    U: Optional[int] = None      # upsampling factor (default: the geometry's)
    frames: Optional[Tuple[int, ...]] = None   # utterances zero-padded to these numbers of frames
    at: Optional[Tuple[int, int]] = None       # single probe: (utterance, position), negative = from the end
    unmasked: Tuple[int, ...] = ()             # dropout paths: layers whose drop_h is None (the last layer's always is)
    own_hs: bool = False                       # the caller's own hidden states (hs_opt), through the C ABI
    seed: int = 1
    expect: Tuple[Tuple[str, object], ...] = ()   # the launch facts the case exists for

    def cfg(self) -> NetConfig:
        cfg = NETS[self.net]()
        return cfg if self.U is None else dataclasses.replace(cfg, upsampling_factor=self.U)

    @property
    def drop(self) -> bool:
        return self.path != "chain"

    @property
    def relu_sigmas(self) -> Optional[float]:
        return None if self.probe == "single" else RELU_SIGMAS

    @property
    def Tp(self) -> int:
        return tp_of(self.cfg(), self.Tf)


def launch_facts(case: Case) -> Dict[str, object]:
    """the launch decisions of one fp32 backward call (module docstring), from the host arithmetic of csrc/swn_train.hip"""
    cfg = case.cfg()
    ceil = lambda a, b: -(-a // b)
    clamp = lambda v: 1 if v < 1 else 16 if v > 16 else v
    B, Tf, seg, H, U, K = case.B, case.Tf, seg_of(cfg), cfg.H, cfg.U, cfg.K
    Tp = tp_of(cfg, Tf)
    ntt, nseg = ceil(Tp, 64), ceil(Tp, 512)
    out = {"Tp": Tp, "route": "chain",                         # swn_train_path: fp32 precision never leaves the chain
           "time_tiles": ntt, "time_pairs": ntt * B, "xcd_chunk": ceil(ntt * B, 8),
           "segments": nseg, "segment_pairs": nseg * B, "segment_rounds": ceil(nseg * B, 8),
           "gate_tiles": ceil(Tp, 256),
           "Kd_layer": K * H, "k_tail": (K * H) % 48, "row_tiles": ceil(2 * H, 64), "taps": K}
    kernels = {"time_gemm", "reduce_gemm", "gate_bwd", "input_bwd"}
    if not case.drop:
        cch = ceil(U + seg - 1, 64)
        rb = ceil(2 * H, 64)
        FR = clamp(rb * Tf * B // 768)
        out.update(cond_columns=U + seg - 1, cond_chunks=cch, cond_nch=2 if cch <= 2 else 5, FR=FR, frame_groups=ceil(Tf, FR),
                   last_group=Tf - (ceil(Tf, FR) - 1) * FR)
        kernels |= {f"cond_bwd<{out['cond_nch']}>", "wup_fold"}
    else:
        out.update(xm_FR=clamp(ceil(cfg.A0, 32) * Tf * B // 1024), dgx_all=seg == 1, inx="inx_all" if seg == 1 else "inx_layer")
        kernels.add("xm_bwd")
        if any(l not in case.unmasked for l in range(cfg.L - 1)):
            kernels.add("mask_mul")                            # the masked input of layer l + 1
    out["kernels"] = frozenset(kernels)
    return out


def _c(name, net, path, probe, number, expect=(), **kw) -> Case:
    return Case(name, net, path, probe, seed=SEEDS.get(name, number), expect=tuple(dict(expect).items()), **kw)


# the first seed from the case's number upwards at which the ReLU conditions of the module docstring hold (cases absent here hold
# them at their number); found with tools/measure_fp32_backward_deviation.py --seeds, asserted by test_fp32_backward_reference.py
SEEDS: Dict[str, int] = {"tiny_smx_ai-dense": 18, "ref6-edges": 23, "cond129-tiny-edges": 47, "fr2-edges": 50}

SINGLES = ((1, 0), (0, -1), (-1, -1))


def cases() -> List[Case]:
    out: List[Case] = []
    n = lambda: len(out) + 1
    # ---- path chain: swn_forward + swn_backward, pre-activations recomputed
    for net in ("tiny", "tiny_s5", "tiny_smx", "tiny_smx_ai"):
        nch = {"cond_nch": 2, "FR": 1}
        out.append(_c(f"{net}-edges", net, "chain", "edges", n(), nch))
        out.append(_c(f"{net}-dense", net, "chain", "dense", n(), nch))
        for i, at in enumerate(SINGLES):
            out.append(_c(f"{net}-single{i}", net, "chain", "single", n(), nch, B=3, Tf=2, at=at))
    # BL6: Kd = 2 x 64 = 128 is no multiple of the 48-deep k loop (its third round holds one real tile and two of zeros);
    # REF6 at 1 x 2 frames: M = 2H = 384 is six row tiles, K = 7 taps
    out.append(_c("bl6-edges", "bl6", "chain", "edges", n(), {"Kd_layer": 128, "k_tail": 32, "row_tiles": 2, "cond_nch": 2}))
    out.append(_c("ref6-edges", "ref6", "chain", "edges", n(), {"row_tiles": 6, "taps": 7, "Kd_layer": 1344, "k_tail": 0}, B=1, Tf=2))
    # off the grid: H = 20, K = 5 (Kd = 100 is no multiple of 16), S = 33; H = 36, seg 7; the (seg, 1) Conv2d; class counts 90 / 300
    out.append(_c("h20k5-edges", "h20k5", "chain", "edges", n(), {"Kd_layer": 100, "k_tail": 4}, Tf=10))
    out.append(_c("h36s7-edges", "h36s7", "chain", "edges", n(), {"cond_columns": 27}))
    out.append(_c("s4c2d-edges", "s4c2d", "chain", "edges", n()))
    out.append(_c("q90-edges", "q90", "chain", "edges", n(), Tf=4))
    out.append(_c("q300-edges", "q300", "chain", "edges", n(), Tf=4))
    # Tp on both sides of one and of two 512-position reduce segments
    for Tp, net, U, Tf, nseg in ((511, "tiny", 16, 32, 1), (512, "tiny", 19, 27, 1), (513, "tiny_s2", 43, 12, 2),
                                 (1023, "tiny", 32, 32, 2), (1025, "tiny", 19, 54, 3)):
        out.append(_c(f"tp{Tp}-edges", net, "chain", "edges", n(), {"Tp": Tp, "segments": nseg, "time_tiles": -(-Tp // 64)}, B=1, U=U, Tf=Tf))
    # (64-position time tiles) x B and B x segments on both sides of 8, the XCD order of the two GEMM kernels: one tile and
    # one segment per utterance at B = 7, 8, 9; several tiles per utterance; two segments per utterance
    for B in (7, 8, 9):
        out.append(_c(f"pairs{B}-b{B}-edges", "tiny", "chain", "edges", n(), {"time_pairs": B, "segment_pairs": B, "xcd_chunk": -(-B // 8),
                                                                            "segment_rounds": -(-B // 8)}, B=B, Tf=2))
    for pairs, B, Tf in ((7, 1, 20), (8, 2, 12), (9, 3, 8)):
        out.append(_c(f"pairs{pairs}-b{B}-edges", "tiny", "chain", "edges", n(), {"time_pairs": pairs, "time_tiles": pairs // B}, B=B, Tf=Tf))
    for pairs, B, (net, U, Tf) in ((8, 4, ("tiny_s2", 43, 12)), (9, 3, ("tiny", 19, 54))):
        out.append(_c(f"segs{pairs}-b{B}-edges", net, "chain", "edges", n(), {"segment_pairs": pairs, "segment_rounds": -(-pairs // 8)},
                      B=B, U=U, Tf=Tf))
    # one batch of three utterances zero-padded to different frame counts
    out.append(_c("ragged-edges", "tiny", "chain", "edges", n(), B=3, Tf=4, frames=(4, 3, 2)))
    # a single frame: Tp = U - 2 seg + 1
    out.append(_c("tf1-edges", "tiny", "chain", "edges", n(), {"Tp": 19, "frame_groups": 1}, Tf=1))
    out.append(_c("tf1-s5-dense", "tiny_s5", "chain", "dense", n(), {"Tp": 11}, Tf=1))
    # cond_bwd_kernel<2> at U + seg - 1 = 128, <5> at 129 (three chunks) and at 256 + seg - 1 (five)
    for net, U, cols, cch, nch in (("tiny", 128, 128, 2, 2), ("tiny_s5", 124, 128, 2, 2), ("tiny", 129, 129, 3, 5), ("tiny_s5", 125, 129, 3, 5),
                                   ("tiny_s5", 256, 260, 5, 5)):
        out.append(_c(f"cond{cols}-{net}-edges", net, "chain", "edges", n(), {"cond_columns": cols, "cond_chunks": cch, "cond_nch": nch}, U=U))
    # two frames per workgroup of cond_bwd_kernel and an odd frame count (the last group holds one frame): on a net of one
    # row block that takes Tf B >= 1536
    out.append(_c("fr2-edges", "tiny", "chain", "edges", n(), {"FR": 2, "frame_groups": 25, "last_group": 1}, B=32, Tf=49, U=8))
    # front end backward: aux kernel 1 / 3 / 5, 1, 3 and 4 layers (dilations 9 and 27 reach past the two frames), the Conv2d net
    for net in ("fe_k1l1", "fe_k3l3", "fe_k5l3", "fe_k3l4"):
        out.append(_c(f"{net}-edges", net, "chain", "edges", n(), Tf=2))
    out.append(_c("fe_k5l3-tf7-edges", "fe_k5l3", "chain", "edges", n(), Tf=7))
    # the caller's own hidden states
    out.append(_c("ownhs-edges", "tiny", "chain", "edges", n(), own_hs=True))
    # ---- path drop1: swn_forward_drop + swn_backward_drop at seg 1 (dgx_all -> inx_all, xm_bwd_kernel), host masks p = 0.5
    for net in ("tiny", "tiny_smx"):
        d1 = {"dgx_all": True, "inx": "inx_all", "xm_FR": 1}
        out.append(_c(f"drop1-{net}-edges", net, "drop1", "edges", n(), d1))
        out.append(_c(f"drop1-{net}-dense", net, "drop1", "dense", n(), d1))
        out.append(_c(f"drop1-{net}-some-edges", net, "drop1", "edges", n(), d1, unmasked=(0, 3)))
    out.append(_c("drop1-ownhs-edges", "tiny", "drop1", "edges", n(), own_hs=True))
    # ---- path dropN: the same entries at seg 2 and seg 5 (inx_layer: the accumulating time GEMM with XT, the reduce GEMM with QT)
    for net in ("tiny_s2", "tiny_s5"):
        out.append(_c(f"dropN-{net}-edges", net, "dropN", "edges", n(), {"dgx_all": False, "inx": "inx_layer"}))
    return out


def inputs_of(case: Case):
    """-> (cfg, sd, aux, audio, grad_raw, drop) as numpy / torch CPU tensors in the dtypes the HIP entry points take (the recipe
    of mixed_ref.inputs_of with this module's edge positions)"""
    from shallow_wavenet_amd.synth import synth_aux, synth_state_dict
    cfg = case.cfg()
    soft = cfg.kind == "softmax"
    B, Tf = case.B, case.Tf
    sd = synth_state_dict(cfg, seed=3 + case.seed, flavor="trained", identity_scale_in=not case.net.startswith("fe_"))
    aux = synth_aux(cfg, B, Tf, seed=case.seed)
    if case.frames is not None:
        for b, f in enumerate(case.frames):
            aux[b, :, f:] = 0.0
    T = Tf * cfg.U
    g = torch.Generator().manual_seed(case.seed)
    Tp = tp_of(cfg, Tf)
    if soft:
        audio = torch.randint(0, cfg.n_quantize, (B, T - 1), generator=g)
    else:
        audio = torch.rand(B, 1, T - cfg.seg, generator=g) * 1.8 - 0.9
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
        drop_x, drop_h = swn_noise.dropout_masks(cfg, B, Tf, 0.5, generator=torch.Generator().manual_seed(100 + case.seed))
        drop = (drop_x, [None if l in case.unmasked else q for l, q in enumerate(drop_h)])
    if case.relu_sigmas is not None:
        for which, name in enumerate(("out_skip.0.bias", "out_1.bias")):
            with torch.no_grad():
                P, a64, au64, _, d64 = M._inputs(cfg, sd, aux, audio, grad_raw, drop)
                pre = _pre_activations(cfg, P, _forward(cfg, P, a64, au64, d64)[1])[which]
            sd[name] = sd[name] + np.float32(case.relu_sigmas * float(pre.std()) - float(pre.mean()))
    return cfg, sd, aux, audio, grad_raw, drop


def decisive(case: Case, inp=None) -> Tuple[float, int]:
    """(pre_min, flips) of the case from the two forwards alone (the seed search)"""
    cfg, sd, aux, audio, grad_raw, drop = inp if inp is not None else inputs_of(case)
    ev = []
    for dtype in (torch.float64, torch.float32):
        with torch.no_grad():
            P, a, au, _, d = M._inputs(cfg, sd, aux, audio, grad_raw, drop, dtype)
            pre = _pre_activations(cfg, P, _forward(cfg, P, a, au, d)[1])
        ev.append(Evaluation(None, None, None, tuple(p.double().numpy() for p in pre)))
    return _kinks(grad_raw, *ev)


_YARD: Dict[str, Yardstick] = {}


def yardstick_of(case: Case) -> Yardstick:
    """computed once per process and case, shared by the tests that need it, never modified"""
    if case.name not in _YARD:
        _YARD[case.name] = yardstick(*inputs_of(case))
    return _YARD[case.name]


# ------------------------------------------------------------------------------------------------ the device
def gpu_run(case: Case, inp=None):
    """the case through HipNet.forward_train / HipNet.backward under train_precision("fp32") and the device-side unfold of the
    packed gradient -> (raw, {state-dict name: gradient}, hidden states or None) as float64 numpy.  own_hs: the same pair of C
    entry points with the caller's hidden-state buffer (the Python runtime never passes one)."""
    from shallow_wavenet_amd import _lib, ops
    from shallow_wavenet_amd.nets._autograd import unfold_packed_grads, unfold_packed_grads_device
    from shallow_wavenet_amd.runtime import HipNet, _ptr, _stream_ptr, train_precision
    cfg, sd, aux, audio, grad_raw, drop = inp if inp is not None else inputs_of(case)
    net = HipNet.from_state_dict(cfg, sd, "cuda:0")
    dev = net.device
    B, Tf, Tp = case.B, case.Tf, tp_of(cfg, case.Tf)
    hs = None
    with train_precision("fp32"):
        if not case.own_hs:
            raw, saved = net.forward_train(torch.from_numpy(aux).cuda(), audio.cuda(), drop=drop)
            assert saved["precision"] == _lib.PRECISION_FP32
            assert saved.get("work_bf16") is None and saved.get("a_keep") is None, "a bf16 buffer in the fp32 mode"
            assert saved["work"].dtype == torch.float32 and (saved.get("drop") is not None) == case.drop
            gp = net.backward(saved, grad_raw.cuda())
        else:
            L, d, st = net.lib, ctypes.byref(net.desc), _stream_ptr(dev)
            nan = lambda n: torch.full((int(n),), float("nan"), dtype=torch.float32, device=dev)
            a = torch.from_numpy(aux).to(dev, torch.float32).contiguous()
            au = audio.to(dev, torch.int32 if cfg.kind == "softmax" else torch.float32).contiguous()
            gr = grad_raw.to(dev, torch.float32).contiguous()
            raw = torch.empty((B, cfg.n_out, Tp), dtype=torch.float32, device=dev)
            hs = nan(B * (cfg.L + 1) * cfg.H * Tp)
            gp = torch.empty_like(net.packed)
            with ops._on(dev):
                if not case.drop:
                    cond, fe_work = ops.frontend_impl(net.packed, a, net.dlist)
                    # the forward leaves the hs section of its work buffer alone when it is given one: full of NaN, a backward
                    # that read it instead of the caller's buffer could not pass
                    work = nan(L.swn_forward_work_floats(d, B, Tf))
                    _lib.check(L.swn_forward(d, _ptr(net.packed), _ptr(cond.contiguous()), _ptr(au), B, Tf, _ptr(work), _ptr(raw), _ptr(hs), st),
                               "forward")
                    bwork = torch.empty(L.swn_backward_work_floats(d, B, Tf), dtype=torch.float32, device=dev)
                    _lib.check(L.swn_backward(d, _ptr(net.packed), _ptr(a), _ptr(cond), _ptr(fe_work), _ptr(au), _ptr(work), _ptr(hs), _ptr(gr),
                                              B, Tf, _ptr(bwork), _ptr(gp), _lib.PRECISION_FP32, st), "backward")
                else:
                    fe_work = torch.empty(L.swn_frontend_work_floats(d, B, Tf), dtype=torch.float32, device=dev)
                    _lib.check(L.swn_frontend(d, _ptr(net.packed), _ptr(a), B, Tf, _ptr(fe_work), _ptr(None), st), "frontend")
                    drop_x, drop_h, ptrs = net._drop_args(drop)
                    hptr = ctypes.cast(ptrs, ctypes.c_void_p)
                    work = nan(L.swn_forward_drop_work_floats(d, B, Tf))
                    _lib.check(L.swn_forward_drop(d, _ptr(net.packed), _ptr(fe_work), _ptr(au), B, Tf, _ptr(drop_x), hptr, _ptr(work), _ptr(raw),
                                                  _ptr(hs), _lib.PRECISION_FP32, st), "forward_drop")
                    bwork = torch.empty(L.swn_backward_drop_work_floats(d, B, Tf), dtype=torch.float32, device=dev)
                    _lib.check(L.swn_backward_drop(d, _ptr(net.packed), _ptr(a), _ptr(fe_work), _ptr(au), _ptr(work), _ptr(hs), _ptr(drop_x), hptr,
                                                   _ptr(gr), B, Tf, _ptr(bwork), _ptr(gp), _lib.PRECISION_FP32, st), "backward_drop")
            hs = hs.view(B, cfg.L + 1, cfg.H, Tp)
    torch.cuda.synchronize()
    names = [k for k, _ in cfg.param_shapes()]
    params = [torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)).cuda() for k in names]
    out = unfold_packed_grads_device(net, gp, params, [True] * len(params))
    if out is None:
        g = unfold_packed_grads(cfg, gp, dict(zip(names, params)))
        out = [g[k].reshape(p.shape) for k, p in zip(names, params)]
    return (raw.double().cpu().numpy(), {k: o.double().cpu().numpy() for k, o in zip(names, out)},
            None if hs is None else hs.double().cpu().numpy())


# ------------------------------------------------------------------------------------------------ deviations and bounds
def floor_of(y: Yardstick, k: str) -> float:
    """FLOOR D_max / sqrt(elements of the tensor)  (module docstring)"""
    return FLOOR * y.D_max / np.sqrt(y.g[k].size)


def row_yardstick(y: Yardstick, k: str) -> np.ndarray:
    """D_row + N_SERIES 2^-24 ||g_row|| + FLOOR D_max / sqrt(elements)  (module docstring)"""
    g = rows_of(k, y.g[k])
    return y.D_rows[k] + N_SERIES * FP32_EPS * np.linalg.norm(g, axis=1) + floor_of(y, k)


def zero_slices(name: str, exact: np.ndarray, got: np.ndarray) -> List[str]:
    """slices (one index of one axis, or the whole tensor) whose exact gradient is exactly zero and whose `got` is not"""
    bad = []
    if not exact.any():
        return [name] if got.any() else []
    for ax in range(exact.ndim):
        if exact.shape[ax] == 1:
            continue
        other = tuple(i for i in range(exact.ndim) if i != ax)
        dead = ~np.abs(exact).max(axis=other).astype(bool) if other else exact == 0
        live = np.abs(got).max(axis=other).astype(bool) if other else got != 0
        bad += [f"{name}[axis {ax}, {int(i)}]" for i in np.nonzero(dead & live)[0]]
    return bad


def deviations(y: Yardstick, raw: np.ndarray, g: Dict[str, np.ndarray], hs: Optional[np.ndarray] = None) -> Dict:
    """errors of a result against the exact gradients next to their yardsticks"""
    out = {"D_max": y.D_max, "D_fwd": y.D_fwd, "fwd_err": float(np.abs(raw - y.raw).max()), "tensors": {}, "nonzero": []}
    if hs is not None:
        out["D_hs"], out["hs_err"] = y.D_hs, float(np.abs(hs - y.hs).max())
    for k, ge in y.g.items():
        e = g[k] - ge
        t = {"err": float(np.linalg.norm(e.ravel())), "D": y.D[k], "norm": float(np.linalg.norm(ge.ravel())), "floor": floor_of(y, k)}
        r = rows_of(k, e)
        if r is not None:
            t["rows_err"] = np.linalg.norm(r, axis=1)
            t["rows_yard"] = row_yardstick(y, k)
        out["tensors"][k] = t
        out["nonzero"] += zero_slices(k, ge, g[k])
    return out


def ratios(d: Dict) -> Dict[str, float]:
    """worst tensor ratio, worst row ratio and forward ratio of `deviations`"""
    fwd = d["fwd_err"] / d["D_fwd"] if d["D_fwd"] else 0.0
    if "hs_err" in d and d["D_hs"]:
        fwd = max(fwd, d["hs_err"] / d["D_hs"])
    return {"tensor": max(t["err"] / (t["D"] + t["floor"]) for t in d["tensors"].values()),
            "rows": max((float((t["rows_err"] / t["rows_yard"]).max()) for t in d["tensors"].values() if "rows_err" in t), default=0.0),
            "fwd": fwd}


def violations(case: Case, d: Dict) -> List:
    m, mf = MARGIN[case.path], MARGIN_FWD[case.path]
    bad = [("exactly zero", n) for n in d["nonzero"]]
    if d["fwd_err"] > mf * d["D_fwd"]:
        bad.append(("forward", d["fwd_err"], d["D_fwd"]))
    if "hs_err" in d and d["hs_err"] > mf * d["D_hs"]:
        bad.append(("hidden states", d["hs_err"], d["D_hs"]))
    for k, t in d["tensors"].items():
        if t["err"] > m * (t["D"] + t["floor"]):
            bad.append((k, t["err"], t["D"]))
        if "rows_err" in t:
            rr = t["rows_err"] / t["rows_yard"]
            if rr.max() > m:
                bad.append((k, "row", int(rr.argmax()), float(rr.max())))
    return bad


# Margins: twice the worst tensor ratio ||g_gpu - g_exact|| / (D_k + FLOOR D_max), and twice the worst forward ratio,
# tools/measure_fp32_backward_deviation.py measured on an MI355X per path over all its cases, two runs each
# (profiles/fp32_backward_deviation.json; measured worst in brackets); the rows are held to the same m (their measured worst:
# 4.15, 0.77, 0.63).  chain's 4.91 is the front end of the seg 5 nets (module docstring, "Where the device stands"); without
# the front end tensors every path sits at 0.6-1.2.  No margin goes below 2: two fp32 evaluations of one graph stand sqrt(2) D
# apart, and a margin under that would ask the device to be closer to float64 than an fp32 evaluation has to be (dropN's
# forward, 0.09 D_fwd, is the Laplace forward's FMA chains against the CPU's fp32 convolutions).
MARGIN: Dict[str, float] = {"chain": 9.9, "drop1": 4.1, "dropN": 2.6}          # (4.91, 2.05, 1.26)
MARGIN_FWD: Dict[str, float] = {"chain": 2.5, "drop1": 2.0, "dropN": 2.0}      # (1.22, 0.99, 0.09)


def old_bound(y: Yardstick, k: str) -> float:
    """the rule of test_gpu_backward_parity.py, max |g - ref| <= 2e-5 + 2e-4 max |ref| per parameter, as an L2 bound: the
    smallest L2 error that rule can refuse puts everything into one element, so an L2 error at or below this passes it
    whatever its shape"""
    return 2e-5 + 2e-4 * float(np.abs(y.g[k]).max())
