"""float64 yardstick for the FORWARD of the bf16 stack (`swn_forward_bf16`, BL6 class) on every kernel it dispatches to.  Test helper
(not collected): tests/test_mixed_reference.py verifies it on the CPU, tests/test_gpu_bf16_forward_paths.py and
tools/measure_bf16_forward_deviation.py hold the HIP kernels against it.

It reuses tests/mixed_ref.py: `exact` (oracle/cpu_ref.py in float64) and `rounded(..., path="fused")`, whose forward roundings
("forward (all paths)" in that module's docstring: bf16 weights of dil_h / out_skip / out_1 / out_2, h_0 .. h_L stored as bf16 and
read back for the operand and the highway term, relu(skip) and relu(out_1) as bf16, the conditioning in fp32 at frame rate) are
the same for every kernel of the dispatch table - the kernels differ in how they cut the work, not in where they round.  Per case:
    raw_exact, raw_rounded    float64 (rows, n_out, Tp) over the distinct utterances
    D_fwd = max |raw_rounded - raw_exact|,  D_rms = rms of the same over all positions and output rows
the error inherent in the arithmetic for exactly these inputs, computed without the code under test.

Inputs: K = 8 distinct utterances (aux, audio) of Tf frames, one of them zero-padded from its second frame on (utterances of
different lengths); row b of the batch is a copy of row b mod 8, so the float64 model runs on 8 rows whatever the batch.

Margins: MARGIN_FWD below, per path.  mixed_ref.MARGIN_FWD["fused"] = 2.0 (twice the measured worst of a kernel that rounds where
the model rounds) is the default; a path whose measured worst ratio does not fit carries twice that ratio, with the figure beside
it (tools/measure_bf16_forward_deviation.py -> profiles/bf16_forward_deviation.json) - the rule mixed_ref.MARGIN follows.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Tuple

import numpy as np
import torch

import mixed_ref as M
from shallow_wavenet_amd import config as C

K = 8                    # distinct utterances
PAD_ROW = 1              # the utterance that is zero-padded from its second frame on (row 0 where the batch is one row)
OLD_TOL = 3e-3           # test_gpu_bf16_stack.py: 3e-3 x max(1, |ref| max)


@dataclasses.dataclass(frozen=True)
class Case:
    path: str            # the kernel the case must run (shallow_wavenet_amd._lib.BF16_PATHS)
    U: int
    B: int
    Tf: int
    seg: int = 1
    lpc: int = 0

    @property
    def name(self) -> str:
        return f"{self.path}-U{self.U}-{self.B}x{self.Tf}" + (f"-seg{self.seg}lpc{self.lpc}" if self.seg > 1 else "")

    @property
    def rows(self) -> int:
        return min(K, self.B)

    def cfg(self):
        return dataclasses.replace(C.bl6_laplace(self.seg, self.lpc), upsampling_factor=self.U)

    @property
    def Tp(self) -> int:
        return self.Tf * self.U - 2 * self.seg + 1


def cases() -> List[Case]:
    """the smallest shapes that reach each kernel (each one forward of at most 350 k positions)"""
    out = []
    # units4 below the fused range: one and two chunks per frame, ragged and not
    for U in (16, 17, 31, 32):
        out += [Case("units4", U, 3, 7), Case("units4", U, 1, 2)]
    # units4 above 3 072 frames: a wave walks several units, the unit past the range is empty, the head loops over its tiles
    out += [Case("units4", U, 1537, 2) for U in (33, 48, 64)] + [Case("units4", 64, 3073, 1)]
    # units5: a last chunk of one position, and none ragged
    out += [Case("units5", U, 1537, 2) for U in (65, 80)]
    # units7: six chunks and an empty seventh (81, 96), seven (97, 110, 112); a frame strictly inside the utterance
    out += [Case("units7", U, 1537, 2) for U in (81, 96, 97, 110, 112)] + [Case("units7", 110, 1025, 3)]
    # the fused kernel at its upper limit
    out.append(Case("fused", 110, 1536, 2))
    # bf16_layer_kernel<0>: U outside 16 .. 112, seg 5; 24 x 7 x 113 positions are more than 4 x 256 chunks (a second round)
    out += [Case("layer0", 15, 3, 7), Case("layer0", 113, 3, 7), Case("layer0", 240, 2, 3), Case("layer0", 110, 3, 7, seg=5, lpc=4),
            Case("layer0", 113, 24, 7)]
    return out


TRAIN_CASE = Case("units7", 110, 1537, 2)       # the mixed-precision training entry (HipNet.forward_train)

# one margin per path: m_f of  max |raw_gpu - raw_exact| <= m_f D_fwd  and  rms(raw_gpu - raw_exact) <= m_f D_rms
MARGIN_FWD: Dict[str, float] = {p: M.MARGIN_FWD["fused"] for p in ("fused", "units4", "units5", "units7", "layer0")}


def inputs_of(case: Case):
    """-> (cfg, sd, aux (rows, n_aux, Tf) float32 numpy, audio (rows, 1, T - seg) float32 torch) of the distinct utterances"""
    from shallow_wavenet_amd.synth import synth_aux, synth_state_dict
    cfg = case.cfg()
    sd = synth_state_dict(cfg, seed=6, flavor="trained", identity_scale_in=True)
    aux = synth_aux(cfg, K, case.Tf, seed=7)
    audio = torch.rand(K, 1, case.Tf * cfg.U - cfg.seg, generator=torch.Generator().manual_seed(2)) * 1.8 - 0.9
    aux, audio = aux[: case.rows].copy(), audio[: case.rows].clone()
    aux[min(PAD_ROW, case.rows - 1), :, 1:] = 0.0
    return cfg, sd, aux, audio


@dataclasses.dataclass
class Yardstick:
    raw_exact: np.ndarray
    raw_rounded: np.ndarray
    D_fwd: float
    D_rms: float

    @property
    def old_bound(self) -> float:
        return OLD_TOL * max(1.0, float(np.abs(self.raw_exact).max()))


def yardstick(case: Case, inp=None) -> Yardstick:
    cfg, sd, aux, audio = inp if inp is not None else inputs_of(case)
    zero = np.zeros((case.rows, cfg.n_out, case.Tp))
    raw_e, _ = M.exact(cfg, sd, aux, audio, zero)
    raw_r, _ = M.rounded(cfg, sd, aux, audio, zero, path="fused")
    d = raw_r - raw_e
    return Yardstick(raw_e, raw_r, float(np.abs(d).max()), float(np.sqrt(np.mean(d * d))))


_YARD: Dict[str, Yardstick] = {}


def yardstick_of(case: Case) -> Yardstick:
    """computed once per process and case, shared by the tests that need it, never modified"""
    if case.name not in _YARD:
        _YARD[case.name] = yardstick(case)
    return _YARD[case.name]


def tile_rows(x: torch.Tensor, B: int) -> torch.Tensor:
    """(rows, ...) -> (B, ...) with row b a copy of row b mod rows"""
    reps = -(-B // x.shape[0])
    return x.repeat(reps, *([1] * (x.dim() - 1)))[:B].contiguous()


def where(case: Case, t: int) -> Tuple[int, int]:
    """position t of an utterance -> (conditioning frame, 16-position chunk inside the frame as the frame-unit kernels cut it)"""
    coff = case.seg
    f = (t + coff) // case.U
    return f, (t - max(f * case.U - coff, 0)) // 16


def gpu_run(case: Case, inp=None):
    """the case through torch.ops.swn.stack_forward_bf16 with the conditioning of the distinct utterances (net.frontend, once)
    tiled over the batch -> (path name the library reports, raw (B, n_out, Tp) fp32, hs (L + 1, B, Tp, 64) int16: the bit
    patterns of the seven stored bf16 hidden-state levels), all on the device"""
    import ctypes
    from shallow_wavenet_amd import _lib
    from shallow_wavenet_amd.runtime import HipNet
    cfg, sd, aux, audio = inp if inp is not None else inputs_of(case)
    net = HipNet.from_state_dict(cfg, sd, "cuda:0")
    rc = net.lib.swn_forward_bf16_path(ctypes.byref(net.desc), case.B, case.Tf)
    path = _lib.BF16_PATHS[rc] if rc >= 0 else str(rc)
    cond = tile_rows(net.frontend(torch.from_numpy(aux).cuda()), case.B)
    wbf = torch.ops.swn.pack_bf16(net.packed, net.dlist)
    raw, work = torch.ops.swn.stack_forward_bf16(net.packed, wbf, cond, tile_rows(audio.cuda(), case.B), net.dlist)
    n = (cfg.L + 1) * case.B * case.Tp * cfg.H * 2
    assert work.numel() == n, "the work buffer of the BL6 class is the hidden states alone"
    return path, raw, work.view(torch.int16).view(cfg.L + 1, case.B, case.Tp, cfg.H)


def copies_differ(case: Case, raw: torch.Tensor, hs: torch.Tensor) -> List[str]:
    """rows b >= 8 against row b mod 8, bit for bit: [] or a description of the first difference"""
    R = case.rows
    if case.B <= R:
        return []
    ref_raw, ref_hs = tile_rows(raw[:R], case.B), tile_rows(hs[:, :R].transpose(0, 1), case.B).transpose(0, 1)
    if torch.equal(raw, ref_raw) and torch.equal(hs, ref_hs):
        return []
    out = []
    bad_h = (hs != ref_hs).any(dim=3)                                  # (L + 1, B, Tp)
    rows = torch.nonzero(bad_h.any(dim=0).any(dim=1) | (raw != ref_raw).any(dim=1).any(dim=1)).flatten()
    b = int(rows[0])
    for l in range(hs.shape[0]):
        ts = torch.nonzero(bad_h[l, b]).flatten()
        if ts.numel():
            t = int(ts[0])
            f, c = where(case, t)
            out.append(f"row {b} (copy of {b % R}) level {l}: first of {ts.numel()} differing positions t = {t} (frame {f}, chunk {c})")
    ts = torch.nonzero((raw[b] != ref_raw[b]).any(dim=0)).flatten()
    if ts.numel():
        t = int(ts[0])
        f, c = where(case, t)
        out.append(f"row {b} (copy of {b % R}) raw: first of {ts.numel()} differing positions t = {t} (frame {f}, chunk {c}, head tile "
                   f"{b * (-(-case.Tp // 64)) + t // 64})")
    out.append(f"{int(rows.numel())} of {case.B} rows differ from their originals")
    return out


def deviations(case: Case, y: Yardstick, raw: np.ndarray) -> Dict:
    """raw (rows, n_out, Tp) float64 of the distinct utterances against the float64 oracle, next to the yardstick"""
    e = raw - y.raw_exact
    m = MARGIN_FWD[case.path]
    over = np.argwhere(np.abs(e).max(axis=1) > m * y.D_fwd)           # (row, t)
    return {"max": float(np.abs(e).max()), "rms": float(np.sqrt(np.mean(e * e))), "D_fwd": y.D_fwd, "D_rms": y.D_rms,
            "finite": bool(np.isfinite(raw).all()),
            "over": [(int(b), int(t)) + where(case, int(t)) for b, t in over[:40]], "n_over": int(len(over))}


def violations(case: Case, d: Dict) -> List:
    m = MARGIN_FWD[case.path]
    bad = []
    if not d["finite"]:
        bad.append("not finite")
    if not d["max"] <= m * d["D_fwd"]:
        bad.append(("max", d["max"], m * d["D_fwd"], f"{d['n_over']} positions above the bound, (row, t, frame, chunk in frame):", d["over"]))
    if not d["rms"] <= m * d["D_rms"]:
        bad.append(("rms", d["rms"], m * d["D_rms"]))
    return bad
