"""GPU: the backward of the fp32 training mode (`train_precision("fp32")`, the default) per tensor and per row at tile and
utterance edges against the float64 oracle, in units of the fp32 oracle's own distance to float64 (tests/fp32_backward_ref.py,
verified on the CPU by test_fp32_backward_reference.py).

Driven through HipNet.forward_train / HipNet.backward under train_precision("fp32") and the device-side unfold of the packed
gradient; every case asserts that the forward recorded PRECISION_FP32 and kept no bf16 buffer.  The 64 cases
(fp32_backward_ref.cases(), each with the launch decision it exists for, asserted on the CPU) run the kernels of
csrc/swn_train.hip that only this mode reaches or that it shares: time_gemm_kernel, reduce_gemm_kernel, gate_bwd_kernel,
cond_bwd_kernel<2 | 5>, wup_fold_kernel, input_bwd_kernel, mask_mul_kernel, xm_bwd_kernel.
  chain   swn_forward + swn_backward: the tiny Laplace (seg 1 lpc 0, seg 5 lpc 4) and softmax nets (with and without audio_in and
          wav_conv) under `edges`, `dense` and three `single` probes; BL6 (Kd = 128 ends the 48-deep k loop in zero tiles) and
          REF6 at 1 x 2 frames (six row tiles, 7 taps); the off-grid nets (H = 20 K = 5 S = 33, H = 36 seg 7, the (seg, 1)
          Conv2d, 90 / 300 classes); Tp = 511, 512, 513, 1 023, 1 025 around the 512-position reduce segments; (time tiles) x B
          and B x segments at 7, 8, 9 around the XCD order of both GEMMs; three utterances zero-padded to 4 / 3 / 2 frames; a
          single frame; cond_bwd_kernel<2> at 128 columns, <5> at 129 and 260; two frames per workgroup with an odd frame count
          (32 x 49 frames at U = 8); the front end at aux kernel 1 / 3 / 5 with 1, 3 and 4 layers and dilations past the frame
          count; the caller's own hidden states.
  drop1   swn_forward_drop + swn_backward_drop at seg 1 (every layer's d gx kept, one in_x contraction pair, xm_bwd_kernel):
          tiny Laplace and softmax, every layer masked and layers 0 and 3 unmasked, host masks p = 0.5; the caller's own hs.
  dropN   the same entries at seg 2 and seg 5 (per-layer in_x contractions: the accumulating time GEMM with XT, reduce with QT).
Probes: `dense` (noise / Tp), `edges` (fp32_backward_ref.edge_positions: both ends, around the largest dilation and the receptive
field, both sides of the 16 / 64 / 256 / 512 tile boundaries and of the last whole one below Tp, both sides of the first two
conditioning-frame boundaries - in every utterance, all channels), `single` ((b = 1, t = 0), (b = 0, t = Tp - 1), (b = B - 1, t = Tp - 1)).

Per case and tensor k, with D_k = ||g_32 - g_exact|| from the oracle in float32 and float64 on the CPU and ONE margin m per path:
    ||g_gpu - g_exact|| <= m (D_k + FLOOR D_max / sqrt(n_k))                 FLOOR = 2^-3, n_k the tensor's element count
    per row of the leading axis of the dil_h, out_skip, out_1, in_x, wav_conv, aux_conv2d weights:
        ||row of (g_gpu - g_exact)|| <= m (D_row + 16 x 2^-24 ||g_row|| + FLOOR D_max / sqrt(n_k))
    max |raw_gpu - raw_exact| <= m_f D_fwd, and the hidden states the same where the entry returns them
    a slice (an index of any axis) whose exact gradient is exactly zero is exactly zero
(fp32_backward_ref's docstring derives 16 and FLOOR and says why the floor shrinks with the tensor's size.)  No case has a ReLU
unit at a probed position within 1e-5 of zero or on different sides in the two evaluations (asserted on the CPU).

Margins: twice the worst tensor ratio and twice the worst forward ratio tools/measure_fp32_backward_deviation.py measured on an
MI355X per path over all its cases, two runs each (profiles/fp32_backward_deviation.json), none below 2:
    path     tensors  m      rows (measured)   forward  m_f    largest run-to-run spread of a tensor ratio
    chain     4.91    9.9       4.15            1.22    2.5       0.08
    drop1     2.05    4.1       0.77            0.99    2.0       0.00
    dropN     1.26    2.6       0.63            0.09    2.0       0.00
Every tensor of the stack sits at 0.6-1.2 in every case: the device is as close to float64 as the fp32 oracle.  What sets the
margins is the frame-rate front end (conv_aux, scale_in): 1.4-2.0 at N = L seg 2H = 384 products per frame, 2.7-4.9 on the
seg 5 / seg 7 nets (N = 1 920 / 1 512), where d C = W_inx^T d cond is one contraction over N accumulated in k order by the fp32
MFMA chain; a serial fp32 sum restated in numpy stands 2.0 x (n = 384) and 3.4 x (n = 1 920) further from float64 than a
blocked one.  It is 1e-6 of the tensor's norm and no operand is wrong.  The rows that stand apart (2.4-4.2) are single rows of
g in_x / g dil_h under a single-position probe, one product chain each.  Before the floor took its present form the two sum
tensors stood out: the oracle's draw for the scalar upsampler bias was 6e-10 of its value in tiny_smx-single1 (ratio 14.9, moving
by 5 between two runs) and 2e-8 for out_2.bias at Tp = 512 (6.2); nothing was wrong with either.  Every new bound, as an L2 norm over the
whole tensor, is below what the rule of test_gpu_backward_parity.py allows ONE element of it (asserted per case and tensor on the
CPU): 0.9 % of it in the median, 38 % at most (the 65 536 elements of the softmax nets' out_2.weight).
The file takes 7 s on the device (64 cases and 12 of the head; the float64 and float32 oracles of a case take 0.9 s at most,
17 s for the whole CPU file); no case is slower than a second - the FR = 2 case reaches 1 568 frames at U = 8.

Mutants (index / arithmetic only, inside their buffers; built outside the tree, never committed) against the old fp32 value
checks - test_gpu_backward_parity, test_gpu_train_step, test_gpu_dropout_parity, test_gpu_ref6_teacher_forced,
test_gpu_cond_bwd_wide and the gradient part of test_gpu_offgrid_geometry, 73 tests - and against the 64 cases of this file:
                                                                                        old files (of 73)   this file (of 64)
    1  time_gemm_kernel: the last k-tile dropped when Kd % 48 != 0                           47 fail            64
    2  time_gemm_kernel: the neighbouring tap for the first column of a 64-tile              44                 64
    3  reduce_gemm_kernel: the last position of every full 512-segment skipped               17                  7
    4  gate_bwd_kernel: position 255 of every 256-tile zeroed                                21                 15
    5  cond_bwd_kernel<5>: its third 64-column chunk ignored                                  6                  3
    6  cond_bwd_kernel at FR = 2: the second frame of a group skipped                         0                  1
    7  input_bwd_kernel: taps 0 and 1 of causal.conv swapped                                 51                 61
    8  xm_bwd_kernel: the first position of every frame dropped                              16                  9
    9  row 5 of layer 0's recomputed dil_h pre-activation x 1.001                             0                 61
Mutant 3 fails exactly the cases with Tp >= 512, 5 the three cases with more than two chunks, 8 the nine dropout cases, 4 the
cases with Tp >= 256.  Mutant 6 passes all 73 old tests - none of their shapes has 1 536 frames on one row block - and fails
fr2-edges alone (tensors at 1e6).  Mutant 9 passes all 73 old tests; here 61 cases fail on the row (27-725 against m; the
three that pass are two single probes that do not reach the channel and the front end net with H = 4, which has no channel 5).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp32_backward_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_backward_against_the_float64_oracle(gpu_ok, case):
    inp = R.inputs_of(case)
    y = R.yardstick_of(case)
    raw, g, hs = R.gpu_run(case, inp)
    d = R.deviations(y, raw, g, hs)
    print(f"{case.name}: forward {d['fwd_err']:.3e} / D_fwd {d['D_fwd']:.3e}" +
          (f"  hidden states {d['hs_err']:.3e} / D_hs {d['D_hs']:.3e}" if hs is not None else ""))
    for k, t in d["tensors"].items():
        line = f"  {k}: err {t['err']:.3e}  D {t['D']:.3e}  ratio {t['err'] / (t['D'] + t['floor']):.2f}"
        if "rows_err" in t:
            rr = t["rows_err"] / t["rows_yard"]
            line += f"  worst row {int(rr.argmax())}: {rr.max():.2f}"
        print(line)
    bad = R.violations(case, d)
    assert not bad, (R.MARGIN[case.path], bad)


# ------------------------------------------------------------------------------------------------ the Laplace head, directly
LOGB_FLOOR = -14.162084148244246758816564788835
OPTIONAL = ("gmu", "gb", "glogb", "ga", "gbc", "glc")
# every gradient given; each one missing in turn; only the clipped pair; only the mean; none
GIVEN = [set(OPTIONAL)] + [set(OPTIONAL) - {k} for k in OPTIONAL] + [{"gbc", "glc"}, {"gmu"}, set()]


def _head_reference(raw, seg, lpc, gr, dtype):
    """graw_mu = gmu, graw_y = (glogb + gb sigmoid(y) + [log_sigmoid(y) >= floor] (glc + gbc sigmoid(y))) (1 - sigmoid(y)),
    graw_a = ga, evaluated in `dtype`; a missing gradient is zero -> (mu part, y part, a part), each (B, rows, Tp) float64"""
    get = lambda k, w: (gr[k].to(dtype) if gr.get(k) is not None else torch.zeros(raw.shape[0], raw.shape[2], w, dtype=dtype)).transpose(1, 2)
    yv = raw[:, seg:2 * seg].to(dtype)
    s, lb = torch.sigmoid(yv), F.logsigmoid(yv)
    keep = (lb >= torch.tensor(LOGB_FLOOR, dtype=dtype)).to(dtype)
    gy = (get("glogb", seg) + get("gb", seg) * s + keep * (get("glc", seg) + get("gbc", seg) * s)) * (1 - s)
    return get("gmu", seg).double(), gy.double(), get("ga", lpc).double()


@pytest.mark.parametrize("lpc", [0, 4])
@pytest.mark.parametrize("seg", [1, 5])
@pytest.mark.parametrize("Tp", [255, 256, 257])
def test_laplace_head_backward_against_its_formula(gpu_ok, Tp, seg, lpc):
    from shallow_wavenet_amd import config as C
    from shallow_wavenet_amd.runtime import HipNet
    from shallow_wavenet_amd.synth import synth_state_dict
    cfg = C.tiny("laplace", seg, lpc)
    net = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=5, flavor="trained"), "cuda:0")
    B, NO = 3, 2 * seg + lpc
    gen = torch.Generator().manual_seed(1000 * Tp + 10 * seg + lpc)
    raw = torch.randn(B, NO, Tp, generator=gen)
    # the scale rows on both sides of the clip floor (log_sigmoid(y) = y - e^y there), none within 1e-3 of it
    u = torch.rand(B, seg, Tp, generator=gen)
    yv = torch.where(u < 0.4, LOGB_FLOOR - 2e-3 - 6.0 * u, torch.where(u < 0.8, LOGB_FLOOR + 2e-3 + 3.0 * (u - 0.4), 20.0 * (u - 0.9)))
    raw[:, seg:2 * seg] = yv
    lb = F.logsigmoid(yv.double())
    assert float((lb - LOGB_FLOOR).abs().min()) > 1e-3 and bool((lb < LOGB_FLOOR).any()) and bool((lb > LOGB_FLOOR).any())
    full = {k: torch.randn(B, Tp, lpc if k == "ga" else seg, generator=gen) for k in OPTIONAL}
    for given in GIVEN:
        gr = {k: (full[k] if k in given and (k != "ga" or lpc > 0) else None) for k in OPTIONAL}
        cu = lambda k: None if gr[k] is None else gr[k].cuda()
        got = net.laplace_head_backward(raw.cuda(), cu("gmu"), cu("gb"), cu("glogb"), cu("ga"), cu("gbc"), cu("glc")).double().cpu()
        assert got.shape == raw.shape
        parts = (got[:, :seg], got[:, seg:2 * seg], got[:, 2 * seg:])
        ref, r32 = _head_reference(raw, seg, lpc, gr, torch.float64), _head_reference(raw, seg, lpc, gr, torch.float32)
        for what, a, e, f, needs in zip(("mu", "y", "a"), parts, ref, r32, ({"gmu"}, {"gb", "glogb", "gbc", "glc"}, {"ga"})):
            if a.numel() == 0:
                continue
            err, d32 = float((a - e).abs().max()), float((f - e).abs().max())
            print(f"Tp {Tp} seg {seg} lpc {lpc} given {sorted(given)} {what}: error {err:.3e}, fp32 evaluation {d32:.3e}")
            if not (needs & given):
                assert not bool(a.any()), (what, sorted(given))
            assert err <= 4.0 * d32, (what, sorted(given), err, d32)
