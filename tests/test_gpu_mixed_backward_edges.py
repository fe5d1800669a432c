"""GPU: the backward of the mixed-precision training mode (`train_precision("bf16")`) at tile and utterance edges against the
float64 oracle, in units of the error inherent in its arithmetic (tests/mixed_ref.py, verified on the CPU by
test_mixed_reference.py).

Driven through HipNet.forward_train / HipNet.backward and the device-side unfold of the packed gradient; every case asserts
that the path it names ran (`work_bf16`, `a_keep`, `fused_backward`).  Cases (mixed_ref.cases()): the fused BL6 backward
(lpc 0 / 2, U = 16, 37, 110, 112, utterances zero-padded to different lengths), the generic chain at the BL6 class, the run.sh
geometry with kept and recomputed pre-activations (one case at 8 x 38 frames, the gate's 192-position tiles), seg 5, the
softmax net with and without audio_in, one dropout-mode step at each class.  Upstream gradients: `dense` (noise / Tp),
`edges` (mixed_ref.edge_positions: both ends, around the largest dilation, the receptive field, the 16 / 32 / 64 / 128 / 192
tiles and the last whole tile below Tp, the first two conditioning-frame boundaries - in every utterance, all channels),
`single` (one position: (b = 1, t = 0), (b = 0, t = Tp - 1), (b = B - 1, t = Tp - 1)).

Per case and reference tensor k, with D_k = ||g_rounded - g_exact|| computed on the CPU without the code under test, and ONE
margin m per path for tensors and rows alike:
    ||g_gpu - g_exact|| <= m (D_k + FLOOR D_max)            D_max the largest D_k of the case
    per row of the leading axis of the dil_h, out_skip, out_1, in_x, wav_conv weights:
        ||row of (g_gpu - g_exact)|| <= m (D_row + n BF16_EPS ||g_row|| + FLOOR D_max / sqrt(rows))     (mixed_ref.row_yardstick)
    max |raw_gpu - raw_exact| <= m_f D_fwd
    a (tensor, tap) slice whose exact gradient is zero is exactly zero (a `single` probe at t = 0 reaches no earlier tap)
The quantisation term of the rows (mixed_ref.row_yardstick has the whole argument): D_row is one realisation of the row's
rounding errors, decided by rounding decisions upstream.  The model itself, evaluated in float32 instead of float64 between its
roundings, lands 0.3-0.4 D_k from its float64 evaluation and shows single rows at 2.5-2.7 D_row (no device involved;
test_mixed_reference.py holds that evaluation to these same bounds); the device is a third evaluation of that kind.  Rows that
are sums over many positions follow D_row (0.85-1.0).  A row of g in_x under a single-position probe is ONE rounded scalar
times a rounded vector: its error is one draw of up to BF16_EPS = 2^-8 ||g_row|| per rounding in series (n = 2 where d gx is
stored as bf16), and D_row can be arbitrarily small (device rows at 0.4-1.0 % of ||g_row|| next to D_row = 0.17 %).  Held to
D_row alone 25 of some 250 000 rows stood at 2.3-3.3, all of this kind or rows of wav_conv.weight (sums over all channels:
D_k / sqrt(rows) added); with the format's step in the yardstick the rows sit at 0.8-1.6 and are held to the tensors' m.

ReLU kinks.  At the synthetic nets' own biases about one ReLU unit in a thousand lies within the forward's bf16 error of zero,
and a unit on the other side of zero moves the gradient by its whole share: with dense noise that IS the inherent error,
3-5 % per tensor (why the old tests needed 5e-2), and twice it is more than the old tests allow.  So the `single` cases run
at the net's own biases with seeds at which no probed unit changes side (256-512 units), and the `edges` / `dense` cases
centre the skip sum and the out_1 pre-activation two standard deviations above zero (2 % of the units stay dead), `edges`
with seeds at which no probed unit changes side.  D_k is then 0.3-1 % of ||g_k||, and every bound stays below the old one
(asserted on the CPU per case and tensor; a third of it or less at the small shapes).

Margins (mixed_ref.MARGIN, MARGIN_FWD, FLOOR): twice the worst tensor ratio ||g_gpu - g_exact|| / (D_k + FLOOR D_max)
tools/measure_mixed_deviation.py measured on an MI355X per path over all its cases, two runs each
(profiles/mixed_backward_deviation.json); the rows are held to the same m:
    path          tensors  m      rows (measured)    forward  m_f
    fused          1.03    2.1       1.18              1.00    2.0
    chain          1.08    2.2       1.00              1.05    2.1
    keep           1.11    2.3       1.58              1.12    2.3
    recompute      1.04    2.1       1.11              1.01    2.1
    fused+drop     1.13    2.3       0.92              1.07    2.2
    keep+drop      1.02    2.0       0.86              1.00    2.0
Every path sits at 1: the kernels round where the model rounds and none stands out.  What is left between device and model
(0.2-0.8 D_k where a probe reaches back in time, 0.000-0.006 where it does not) is the cascade of tie decisions: read back
from the device, 3 of 42 048 stored values of h_0 differ from the model's by one bf16 step, 31 of h_1, ... 972 of h_6 (fused,
2 x 110 frames; the float32 evaluation of the model differs from the float64 one in the same way).  FLOOR = 1e-3: the
device's fp32 sums where D_k is zero (out_2.bias outside the fused path) or tiny (the scalar upsampler bias); fp32 noise is
~1e-6 of a tensor's norm, D_max some 5e-3 of the largest norm.  The dropout step of the GEMM-stack class is taken at 3 frames
(Tp >= 256: the bf16 stack with bf16 in_x copies that run.sh trains on; below that the library runs an fp32-work chain the
model does not describe).  The file takes 34 s, 22 s of them the float64 oracle of the 8 x 38 case.

Mutants (index / arithmetic only, inside their buffers; built outside the tree, never committed) against
test_gpu_train_bf16.py + test_gpu_fused_backward.py (45 tests) and against this file's cases of the mutated path (18 BL6 cases
for 1-4 and 6, the 20 GEMM-stack-class cases less the 8 x 38 one for 5a / 5b), failing tests of each:
                                                                                 old files                       this file
    1   bl6_wgrad_kernel: the dil_h jobs read t - dil only for t - dil >= 1           6 (fused against chain only)    caught (9)
    2   bl6_layer_bwd_kernel: last position of a ragged 16-chunk loads zeros     13                              caught (11)
    3   bl6_layer_bwd_kernel: da(t + dil) read without the utterance-end guard    2 (fused against chain only)    caught (9)
    4   bl6_head_bwd_kernel: d skip of position 63 of every 64-tile zeroed       13                              caught (8)
    5a  reduce_gemm_bf16_kernel: last column of a ragged 32-tile dropped         28                              caught (19)
    5b  time_gemm_b16_kernel: last column of a ragged 8-piece dropped            16                              caught (15)
    6   pack_wrec_kernel: row 102 of layer 0's Wd image x 1.01                    0                              caught (2)
Mutants 1 and 3 pass every comparison of the old files with a reference; only the fused-against-chain self-comparison sees
them (6 and 2 of its 12 cases), and a slip common to both paths would pass it.  Mutant 6 passes all 45 old tests; here the
two single-position cases that reach the channel fail on its rows (in_x.0 row 102 at 2.66; in_x.0 row 38 at 3.50, dil_h.0
row 38 at 2.87 and upsampling.conv.weight at 8.1 D_k, against m = 2.1).  Its row is the one with the largest gradient: most
gate channels of the synthetic nets run in the linear middle of their sigmoid, where 1 % on the pre-activation moves every
gradient by 1e-5 to 2e-3 of its inherent error (float64, layer 2 row 37) - below anything the arithmetic lets a test see.
"""
import numpy as np
import pytest

import mixed_ref as M

pytestmark = pytest.mark.gpu

CASES = M.cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_backward_against_the_float64_oracle(gpu_ok, case):
    inp = M.inputs_of(case)
    y = M.yardstick_of(case)
    raw, g = M.gpu_run(case, inp)
    d = M.deviations(case, y, raw, g)
    floor = M.FLOOR * d["D_max"]
    print(f"{case.name}: forward {d['fwd_err']:.3e} / D_fwd {d['D_fwd']:.3e}")
    for k, t in d["tensors"].items():
        line = f"  {k}: err {t['err']:.3e}  D {t['D']:.3e}  ratio {t['err'] / (t['D'] + floor):.2f}"
        if "rows_err" in t:
            rr = t["rows_err"] / t["rows_yard"]
            line += f"  worst row {int(rr.argmax())}: {rr.max():.2f}"
        print(line)
    bad = M.violations(case, d)
    assert not bad, (M.MARGIN[case.margin_group], bad)
