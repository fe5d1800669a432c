"""GPU: torch.ops.swn.spectral_loss / spectral_loss_backward per FFT size, edge length and upstream weight against the
float64 reference of spectral_ref.py (verified on the CPU by test_spectral_reference.py), and `batch_loss` with the HIP loss
against its own torch formulas in float64.

Per case (table `spectral_ref.cases()`: the recipe chunk, all 64 admissible sizes in two 32-size calls, single-size calls,
descending / shuffled / repeated size lists, the shortest admissible signals, lengths around the forward tile of 8 and the
backward tile of 16 frames, 10 and 16 rows), in this order:

  state     the decoded sign state against sign(STFT64(sample - target)).  Outside the structural set (spectral_ref.py) and
            above the worst-case fp32 bound not one entry may differ; the imaginary parts of bins 0 and n / 2 must be code 0;
            at most 1 % of the non-structural entries may lie below the bound (they are the only thing left out).
  values    l1 within max(4 e32, 1e-6), lsd within max(4 e32, 1e-4) of float64, relative to the largest float64 value,
            e32 = torch's fp32 CPU path on the same inputs (the rule of test_gpu_spectral_loss.py).
  gradient  with a random upstream weight g (R, K) in [-1, 1] holding exact zeros, negative entries and an all-zero row,
            against the float64 gradient of the linear surrogate with the float64 signs (structural set zeroed, the
            operator's own code only at the entries the state check left out): within max(4 e32_lin, 1e-6) of the largest
            float64 value, e32_lin = the same surrogate evaluated by torch in fp32.  No sign flip is left in that
            yardstick, so the bound is the 1e-6 floor or close to it in every case; rows of g that are zero give rows of
            exact zeros.

Exact properties (bit for bit): row independence, size independence and order, sample == target, no hidden state between
interleaved calls (also on a side stream), views / float64 / list-of-rows inputs; and the non-finite pattern of lsd on a
partly silent target.

Measured on an MI355X (errors relative to the largest float64 value, the bound of the rule in brackets; state: entries
compared / left out below the bound (how many of those differ from float64) / structural entries (how many differ)):
    case                 state: compared / left out (differing) / structural (differing)     l1 (bound)         lsd (bound)        gradient (bound)
    recipe-5x8114         2759787 / 3018 (  0) /  46125 (17703)    9.5e-08 (1.0e-06)   3.3e-05 (1.1e-04)   1.9e-07 (1.0e-06)
    sizes-32-1024          280857 /  167 (  0) /  19124 ( 9410)    1.5e-07 (1.6e-06)   2.0e-05 (2.0e-04)   8.2e-07 (1.5e-06)
    sizes-1056-2048        284292 /  828 (  0) /  50044 (27711)    1.2e-07 (2.9e-06)   8.6e-05 (1.1e-04)   3.1e-07 (1.3e-06)
    single-2048             58141 /  230 (  0) /   3129 ( 1714)    6.4e-08 (1.0e-06)   1.4e-05 (1.0e-04)   1.8e-07 (1.0e-06)
    single-32               59955 /    0 (  0) /   3795 (   30)    1.2e-07 (1.0e-06)   1.0e-06 (1.0e-04)   1.6e-07 (1.0e-06)
    order-descending       148403 /  175 (  0) /  13394 ( 6987)    1.2e-07 (2.3e-06)   1.8e-05 (4.5e-04)   7.5e-07 (2.1e-06)
    order-shuffled         148403 /  175 (  0) /  13394 ( 6987)    1.2e-07 (2.3e-06)   1.8e-05 (4.5e-04)   3.2e-07 (1.2e-06)
    order-512-128-512       26232 /   14 (  0) /   1358 (  689)    1.3e-07 (1.0e-06)   1.4e-05 (6.8e-04)   2.3e-07 (1.0e-06)
    short-n32-T17             264 /    0 (  0) /    144 (   72)    6.7e-08 (1.8e-06)   4.8e-07 (1.0e-04)   8.8e-08 (1.0e-06)
    short-n32-T18             324 /    0 (  0) /     84 (   32)    4.5e-08 (2.3e-06)   9.7e-07 (1.0e-04)   1.2e-07 (1.0e-06)
    short-n96-T49             776 /    0 (  0) /    400 (  223)    7.2e-08 (6.8e-06)   1.3e-06 (1.0e-04)   1.8e-07 (1.0e-06)
    short-n96-T50             964 /    0 (  0) /    212 (  110)    8.0e-08 (1.5e-06)   1.4e-06 (1.0e-04)   1.3e-07 (1.0e-06)
    short-n160-T81           1288 /    0 (  0) /    656 (  352)    5.1e-08 (4.4e-06)   1.3e-05 (1.0e-04)   2.8e-07 (1.0e-06)
    short-n160-T82           1604 /    0 (  0) /    340 (  186)    9.3e-08 (2.1e-06)   1.1e-06 (1.0e-04)   1.9e-07 (1.0e-06)
    short-n1024-T513         8196 /    4 (  0) /   4112 ( 2328)    8.0e-08 (5.0e-06)   1.8e-05 (1.6e-04)   1.7e-07 (1.0e-06)
    short-n1024-T514        10219 /   25 (  0) /   2068 ( 1112)    4.9e-08 (2.7e-06)   1.8e-04 (4.8e-04)   1.8e-07 (1.0e-06)
    short-n2016-T1009       16080 /   56 (  0) /   8080 ( 4464)    7.9e-08 (5.9e-06)   5.7e-05 (3.3e-04)   1.7e-07 (1.3e-06)
    short-n2016-T1010       20023 /  141 (  0) /   4052 ( 2251)    6.8e-08 (2.4e-06)   4.3e-05 (1.0e-04)   1.6e-07 (1.0e-06)
    short-n2048-T1025       16331 /   61 (  0) /   8208 ( 4619)    1.3e-07 (5.2e-06)   3.1e-05 (1.7e-04)   1.7e-07 (1.0e-06)
    short-n2048-T1026       20334 /  150 (  0) /   4116 ( 2364)    1.7e-07 (2.7e-06)   9.9e-06 (1.0e-04)   1.8e-07 (1.0e-06)
    tile-n32-T55              836 /    0 (  0) /    116 (   31)    7.8e-08 (1.0e-06)   3.0e-06 (1.0e-04)   8.1e-08 (1.0e-06)
    tile-n32-T56              964 /    0 (  0) /    124 (   34)    9.1e-08 (1.0e-06)   2.8e-06 (1.0e-04)   7.7e-08 (1.0e-06)
    tile-n32-T64             1092 /    0 (  0) /    132 (   31)    1.0e-07 (1.0e-06)   2.1e-06 (1.0e-04)   1.6e-07 (1.0e-06)
    tile-n32-T120            1987 /    1 (  0) /    188 (   31)    9.9e-08 (1.5e-06)   9.9e-07 (1.0e-04)   1.1e-07 (1.0e-06)
    tile-n32-T128            2116 /    0 (  0) /    196 (   34)    4.0e-08 (1.0e-06)   1.4e-06 (1.0e-04)   7.8e-08 (1.0e-06)
    tile-n32-T129            2056 /    0 (  0) /    256 (   61)    1.3e-07 (1.0e-06)   1.7e-07 (1.0e-04)   1.1e-07 (1.0e-06)
    tile-n96-T167            2500 /    0 (  0) /    244 (  109)    5.3e-08 (1.0e-06)   2.1e-06 (1.0e-04)   1.9e-07 (1.0e-06)
    tile-n96-T168            2884 /    0 (  0) /    252 (   90)    9.0e-08 (1.0e-06)   2.0e-06 (1.0e-04)   1.8e-07 (1.0e-06)
    tile-n96-T192            3268 /    0 (  0) /    260 (  109)    7.3e-08 (1.1e-06)   1.6e-06 (1.0e-04)   1.0e-07 (1.0e-06)
    tile-n96-T360            5956 /    0 (  0) /    316 (   97)    5.5e-08 (1.0e-06)   3.3e-07 (1.0e-04)   1.4e-07 (1.0e-06)
    tile-n96-T384            6340 /    0 (  0) /    324 (   87)    8.2e-08 (1.0e-06)   7.1e-07 (1.0e-04)   2.1e-07 (1.0e-06)
    tile-n96-T385            6151 /    1 (  0) /    512 (  192)    7.1e-08 (1.0e-06)   1.7e-05 (1.0e-04)   2.2e-07 (1.0e-06)
    tile-n160-T279           4163 /    1 (  0) /    372 (  177)    1.1e-07 (1.0e-06)   1.6e-06 (1.0e-04)   2.0e-07 (1.0e-06)
    tile-n160-T280           4803 /    1 (  0) /    380 (  178)    7.1e-08 (1.0e-06)   1.9e-06 (1.0e-04)   2.0e-07 (1.0e-06)
    tile-n160-T320           5443 /    1 (  0) /    388 (  181)    8.1e-08 (1.2e-06)   6.7e-06 (1.0e-04)   2.3e-07 (1.0e-06)
    tile-n160-T600           9922 /    2 (  0) /    444 (  191)    5.6e-08 (1.0e-06)   3.4e-06 (1.0e-04)   2.2e-07 (1.0e-06)
    tile-n160-T640          10564 /    0 (  0) /    452 (  180)    2.1e-08 (1.0e-06)   2.0e-06 (1.0e-04)   2.9e-07 (1.0e-06)
    tile-n160-T641          10246 /    2 (  0) /    768 (  368)    7.7e-08 (1.0e-06)   6.0e-06 (1.0e-04)   2.1e-07 (1.0e-06)
    tile-n1024-T1791        26588 /   40 (  0) /   2100 ( 1159)    1.2e-07 (1.4e-06)   3.1e-06 (1.3e-04)   1.6e-07 (1.0e-06)
    tile-n1024-T1792        30668 /   56 (  0) /   2108 ( 1121)    5.5e-08 (1.0e-06)   1.1e-05 (1.0e-04)   1.5e-07 (1.0e-06)
    tile-n1024-T2048        34748 /   72 (  0) /   2116 ( 1159)    1.3e-07 (1.0e-06)   2.4e-05 (1.0e-04)   1.8e-07 (1.0e-06)
    tile-n1024-T3840        63399 /   93 (  0) /   2172 ( 1117)    4.9e-08 (1.0e-06)   1.3e-06 (1.0e-04)   1.6e-07 (1.0e-06)
    tile-n1024-T4096        67493 /   95 (  0) /   2180 ( 1132)    1.2e-07 (1.0e-06)   3.2e-06 (1.0e-04)   2.1e-07 (1.0e-06)
    tile-n1024-T4097        65447 /   97 (  0) /   4224 ( 2265)    9.1e-08 (1.0e-06)   5.8e-06 (1.0e-04)   2.2e-07 (1.0e-06)
    tile-n2016-T3527        52212 /  208 (  0) /   4084 ( 2253)    6.5e-08 (1.2e-06)   5.0e-05 (1.0e-04)   2.0e-07 (1.0e-06)
    tile-n2016-T3528        60206 /  278 (  0) /   4092 ( 2258)    7.9e-08 (1.0e-06)   4.9e-05 (5.9e-04)   1.5e-07 (1.0e-06)
    tile-n2016-T4032        68181 /  367 (  0) /   4100 ( 2220)    6.8e-08 (1.2e-06)   1.5e-04 (2.6e-04)   2.1e-07 (1.0e-06)
    tile-n2016-T7560       124436 /  560 (  0) /   4156 ( 2237)    9.9e-08 (1.0e-06)   1.6e-04 (3.0e-04)   2.2e-07 (1.0e-06)
    tile-n2016-T8064       132463 /  597 (  0) /   4164 ( 2216)    8.3e-08 (1.0e-06)   1.6e-05 (1.1e-04)   1.7e-07 (1.0e-06)
    tile-n2016-T8065       128522 /  510 (  0) /   8192 ( 4576)    1.4e-07 (1.0e-06)   2.6e-05 (1.0e-04)   2.6e-07 (1.0e-06)
    tile-n2048-T3583        53059 /  193 (  0) /   4148 ( 2273)    6.4e-08 (1.4e-06)   2.2e-05 (1.0e-04)   1.9e-07 (1.0e-06)
    tile-n2048-T3584        61147 /  297 (  0) /   4156 ( 2273)    1.1e-07 (1.0e-06)   3.2e-05 (1.0e-04)   1.9e-07 (1.0e-06)
    tile-n2048-T4096        69279 /  357 (  0) /   4164 ( 2244)    1.5e-07 (1.0e-06)   1.0e-04 (2.3e-04)   1.8e-07 (1.0e-06)
    tile-n2048-T7680       126388 /  592 (  0) /   4220 ( 2244)    9.1e-08 (1.0e-06)   4.4e-06 (1.0e-04)   1.6e-07 (1.0e-06)
    tile-n2048-T8192       134522 /  650 (  0) /   4228 ( 2327)    9.5e-08 (1.0e-06)   5.3e-06 (1.0e-04)   2.3e-07 (1.0e-06)
    tile-n2048-T8193       130559 /  521 (  0) /   8320 ( 4572)    1.1e-07 (1.1e-06)   6.7e-06 (1.0e-04)   2.0e-07 (1.0e-06)
    rows-16x2500          2709497 / 2839 (  0) / 115312 (56057)    1.2e-07 (1.9e-06)   2.6e-04 (2.2e-03)   2.3e-07 (1.0e-06)
    rows-10x8114          5519636 / 5974 (  0) /  92250 (35139)    1.2e-07 (1.0e-06)   1.6e-04 (9.3e-04)   2.5e-07 (1.0e-06)
    partly-silent         1655852 / 1831 (  0) /  27675 (10546)    9.0e-08 (1.0e-06)   2.4e-05 (1.0e-04)   3.6e-07 (1.0e-06)
Over all cases 15 258 066 state entries were compared and none differs; of the 21 280 entries below the bound none differs
either (torch's own fp32 transform: one, in rows-16x2500); inside the structural set 232 913 of 496 720 differ, as rounding
noise of random sign must.  The largest gradient bound is 2.1e-6 (order-descending), the largest share of a bound used 0.54
(sizes-32-1024).  batch_loss, gradient of the spectral term (hip / torch fp32 / bound):
    speech-like d mus: e32 5.823e-04  hip 2.334e-07  bound 2.329e-03
    speech-like d bs_noclip: e32 3.349e-04  hip 2.251e-07  bound 1.340e-03
    partly-silent d mus: e32 6.389e-04  hip 2.484e-07  bound 2.556e-03
    partly-silent d bs_noclip: e32 3.750e-04  hip 2.384e-07  bound 1.500e-03
    all-zero d mus: e32 1.671e-07  hip 2.256e-07  bound 1.000e-06
    all-zero d bs_noclip: e32 1.169e-07  hip 1.481e-07  bound 1.000e-06

What the gradient check found: with one accumulation chain over all 2 (n / 2 + 1) terms the backward was 1.0e-6 to 1.5e-6 off
at n = 2 016 / 2 048 (single-2048 1.2e-6, short-n2048-T1025 1.5e-6, seven more cases; bounds 1.0e-6 to 2.1e-6) while
test_gpu_spectral_loss.py, where those sizes are two of 17, saw 3e-7.  `spectral_bwd_kernel` now sums in runs of 64 bins
(single-2048 1.8e-7); the figures above are with that.

Mutants of swn_spectral.hip (arithmetic only, built outside the tree) against both files, failing tests of each:
                                                               test_gpu_spectral_loss.py   this file
    1  bwd reads g[r * nk + (nk - 1 - k)]                          not caught (0 of 12)    caught (8)
    2  coef x 1.001 for sizes above 1 024                          not caught (0 of 12)    caught (25)
    3  bwd reads g[k] (row 0's weights for every row)              not caught (0 of 12)    caught (61)
    4  sp_sign_code(0.f) returns 1                                 not caught (0 of 12)    caught (60)
"""
import numpy as np
import pytest
import torch

import spectral_ref as SR
from shallow_wavenet_amd import spectral
from shallow_wavenet_amd import train_driver as T

pytestmark = pytest.mark.gpu

CASES = SR.cases()
GRAD_BOUND_CEILING = 1e-5      # a gradient bound above this means the yardstick contains sign flips: the case is wrong


def _tables(sizes):
    return torch.from_numpy(np.concatenate([spectral.size_tables(n) for n in sizes])).cuda()


def _fwd(smp, trg, sizes, keep_state=True):
    """-> l1 (R, K), lsd (R, K) float32 on the CPU, state bytes on the CPU"""
    l1, lsd, state = torch.ops.swn.spectral_loss(smp.float().cuda(), trg.float().cuda(), _tables(sizes), list(sizes), keep_state)
    return l1.cpu(), lsd.cpu(), state.cpu()


def _bwd(g, state, sizes, length):
    return torch.ops.swn.spectral_loss_backward(g.float().cuda(), state.cuda(), _tables(sizes), list(sizes), length).cpu()


def _check_state(name, d, sizes, state):
    """the state assertion; returns the reference signs for the gradient (float64 signs, structural set zeroed, the
    operator's code at the entries below the bound)"""
    R, length = d.shape
    got = SR.decode_state(state, R, length, sizes)
    tot = dict(compared=0, left_out=0, nonstructural=0, bad=0, left_out_diff=0, structural=0, structural_diff=0)
    ref_signs = []
    for n, s in zip(sizes, got):
        rep = SR.sign_report(d, n, s)
        for key in tot:
            tot[key] += rep[key]
        assert not s[:, 0, :, 1].any() and not s[:, n // 2, :, 1].any(), f"{name}: Im of bin 0 or n/2 is not code 0 (n = {n})"
        ref_signs.append(torch.where(rep["below"], s, rep["ref"]))
    print(f"{name} state: compared {tot['compared']}  differing {tot['bad']}  left out {tot['left_out']} "
          f"({100.0 * tot['left_out'] / tot['nonstructural']:.3f} %), {tot['left_out_diff']} of them differ;  structural "
          f"{tot['structural']}, {tot['structural_diff']} differ")
    assert tot["left_out"] <= SR.BELOW_BOUND_CAP * tot["nonstructural"], (name, tot["left_out"], tot["nonstructural"])
    assert tot["bad"] == 0, (name, tot["bad"])
    return ref_signs


def _check_values(name, smp, trg, sizes, l1, lsd):
    ref = SR.loss64(smp, trg, sizes)
    f32 = SR.torch_path(smp, trg, sizes, torch.float32)
    assert l1.shape == ref[0].shape and lsd.shape == ref[1].shape
    assert torch.isfinite(ref[0]).all() and torch.isfinite(l1).all()
    fin = torch.isfinite(ref[1])
    assert torch.equal(torch.isfinite(lsd), fin), (name, "isfinite pattern of lsd")
    out = []
    for what, got, i, floor, ok in (("l1", l1, 0, 1e-6, None), ("lsd", lsd, 1, 1e-4, fin)):
        if ok is not None and not ok.any():
            continue
        assert torch.isfinite(f32[i] if ok is None else f32[i][ok]).all(), (name, what, "torch fp32 is no yardstick here")
        e32 = SR.rel(f32[i], ref[i], ok)
        ehip = SR.rel(got.double(), ref[i], ok)
        print(f"{name} {what}: torch fp32 {e32:.3e}  hip {ehip:.3e}  bound {max(4 * e32, floor):.3e}")
        out.append((what, ehip, e32, floor))
    for what, ehip, e32, floor in out:
        assert ehip <= max(4 * e32, floor), (name, what, ehip, e32)


def _check_grad(name, smp, sizes, ref_signs, g, grad):
    ref = SR.grad64_from_signs(smp, ref_signs, sizes, g)
    lin = SR.grad_from_signs(smp, ref_signs, sizes, g, torch.float32)
    top = float(ref.abs().max())
    assert top > 0
    e32, ehip = float((lin - ref).abs().max()) / top, float((grad.double() - ref).abs().max()) / top
    bound = max(4 * e32, 1e-6)
    print(f"{name} grad: torch fp32 surrogate {e32:.3e}  hip {ehip:.3e}  bound {bound:.3e}")
    assert bound <= GRAD_BOUND_CEILING, (name, bound)
    assert ehip <= bound, (name, ehip, e32)
    zero_rows = [r for r in range(g.shape[0]) if not g[r].any()]
    assert g.shape[0] == 1 or zero_rows
    for r in zero_rows:
        assert not grad[r].any(), (name, "row of zero weights", r)


def _check_case(name, smp, trg, sizes, gseed):
    d = smp - trg
    R, length = d.shape
    l1, lsd, state = _fwd(smp, trg, sizes)
    ref_signs = _check_state(name, d, sizes, state)
    _check_values(name, smp, trg, sizes, l1, lsd)
    g = SR.weights(R, len(sizes), gseed)
    assert (g == 0).any() and (g < 0).any() and g.abs().max() <= 1
    grad = _bwd(g, state, sizes, length)
    assert grad.shape == (R, length) and torch.isfinite(grad).all()
    _check_grad(name, smp, sizes, ref_signs, g.double(), grad)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_state_values_and_weighted_gradient_match_float64(gpu_ok, case):
    name, R, length, sizes, seed = case
    smp, trg, _ = SR.signals_f32(R, length, seed)
    _check_case(name, smp, trg, sizes, gseed=seed + 1)


def test_partly_silent_target(gpu_ok):
    """700 consecutive exact zeros in every target row: the small sizes have frames of silence (lsd not finite), the large
    ones do not.  A frame of exact zeros has power 0 in any precision, so the pattern is float64's."""
    smp, trg, _ = SR.signals_f32(3, 8114, 24)
    trg = SR.silence(trg)
    fin = torch.isfinite(SR.loss64(smp, trg, SR.FFT17)[1])
    assert not fin[:, :10].any() and fin[:, 10:].all()         # sizes up to 640 see a silent frame, 768 and above never do
    _check_case("partly-silent", smp, trg, SR.FFT17, gseed=25)


# ------------------------------------------------------------------------------------------------------- exact properties
def _state_slices(state, R, length, sizes):
    """per size the (R, frames * bins) bytes of the state"""
    out, at = [], 0
    for n in sizes:
        m = SR.frames_of(length, n) * SR.bins_of(n)
        out.append(state[at:at + R * m].reshape(R, m))
        at += R * m
    assert at == state.numel()
    return out


@pytest.mark.parametrize("length,seed", [(8114, 21), (1025, 22)])
def test_rows_are_independent(gpu_ok, length, seed):
    R, sizes = 5, [n for n in SR.FFT17 if length > n // 2]
    assert len(sizes) == 17
    smp, trg, _ = SR.signals_f32(R, length, seed)
    g = SR.weights(R, len(sizes), seed)
    g[R // 2] = g[0].flip(0)                                    # every row carries weights here
    l1, lsd, state = _fwd(smp, trg, sizes)
    grad = _bwd(g, state, sizes, length)
    whole = _state_slices(state, R, length, sizes)
    for r in range(R):
        a1, alsd, astate = _fwd(smp[r:r + 1], trg[r:r + 1], sizes)
        assert torch.equal(a1[0], l1[r]) and torch.equal(alsd[0], lsd[r]), r
        for k, s in enumerate(_state_slices(astate, 1, length, sizes)):
            assert torch.equal(s[0], whole[k][r]), (r, sizes[k])
        assert torch.equal(_bwd(g[r:r + 1], astate, sizes, length)[0], grad[r]), r


def test_sizes_are_independent_of_their_company_and_order(gpu_ok):
    R, length = 5, 8114
    smp, trg, _ = SR.signals_f32(R, length, 23)
    orders = {"ascending": SR.FFT17, "descending": SR.FFT17[::-1], "shuffled": SR.shuffled(SR.FFT17, 17)}
    alone = {}
    for n in SR.FFT17:
        l1, lsd, state = _fwd(smp, trg, [n])
        alone[n] = (l1[:, 0], lsd[:, 0], state.reshape(R, -1))
    for what, sizes in orders.items():
        l1, lsd, state = _fwd(smp, trg, sizes)
        for k, (n, s) in enumerate(zip(sizes, _state_slices(state, R, length, sizes))):
            assert torch.equal(l1[:, k], alone[n][0]) and torch.equal(lsd[:, k], alone[n][1]), (what, n)
            assert torch.equal(s, alone[n][2]), (what, n)


def test_sample_equal_to_target(gpu_ok):
    R, length = 3, 4999
    _, trg, _ = SR.signals_f32(R, length, 26)
    l1, lsd, state = _fwd(trg, trg, SR.FFT17)
    assert not l1.any() and not state.any()
    assert not lsd.any()                                         # the targets of the recipe have power in every frame
    grad = _bwd(SR.weights(R, 17, 26), state, SR.FFT17, length)
    assert not grad.any()


def _lone(smp, trg, sizes, g):
    l1, lsd, state = _fwd(smp, trg, sizes)
    return l1, lsd, _bwd(g, state, sizes, smp.shape[1])


@pytest.mark.parametrize("side_stream", [False, True])
def test_no_hidden_state_between_calls(gpu_ok, side_stream):
    """forward A, forward B (other shape, other sizes), backward B, backward A: each as from a lone forward + backward"""
    sa, sb = SR.FFT17, [96, 2016, 512, 32]
    A, B = SR.signals_f32(5, 8114, 21), SR.signals_f32(2, 1100, 27)
    ga, gb = SR.weights(5, len(sa), 28), SR.weights(2, len(sb), 29)
    lone_a, lone_b = _lone(A[0], A[1], sa, ga), _lone(B[0], B[1], sb, gb)
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        a1, alsd, astate = torch.ops.swn.spectral_loss(A[0].float().cuda(), A[1].float().cuda(), _tables(sa), sa, True)
        b1, blsd, bstate = torch.ops.swn.spectral_loss(B[0].float().cuda(), B[1].float().cuda(), _tables(sb), sb, True)
        gradb = torch.ops.swn.spectral_loss_backward(gb.cuda(), bstate, _tables(sb), sb, 1100)
        grada = torch.ops.swn.spectral_loss_backward(ga.cuda(), astate, _tables(sa), sa, 8114)
    stream.synchronize()
    for got, want in zip((a1, alsd, grada, b1, blsd, gradb), lone_a + lone_b):
        assert torch.equal(got.cpu(), want)


def test_views_float64_and_lists_of_rows_equal_the_contiguous_call(gpu_ok):
    R, length = 5, 8114
    smp, trg, _ = SR.signals_f32(R, length, 21)
    g = SR.weights(R, 17, 30)
    l1, lsd, state = _fwd(smp, trg, SR.FFT17)
    grad = _bwd(g, state, SR.FFT17, length)
    tab = _tables(SR.FFT17)
    wide_s, wide_t = torch.zeros(R, length + 37).cuda(), torch.zeros(R, length + 37).cuda()
    wide_s[:, 19:19 + length], wide_t[:, 19:19 + length] = smp.float().cuda(), trg.float().cuda()
    inputs = {"column slice": (wide_s[:, 19:19 + length], wide_t[:, 19:19 + length]), "float64": (smp.cuda(), trg.cuda())}
    for what, (s, t) in inputs.items():
        assert what == "float64" or not s.is_contiguous()
        b1, blsd, bstate = torch.ops.swn.spectral_loss(s, t, tab, SR.FFT17, True)
        assert torch.equal(b1.cpu(), l1) and torch.equal(blsd.cpu(), lsd) and torch.equal(bstate.cpu(), state), what
    # the way batch_loss calls it: lists of rows, through autograd
    loss = spectral.MultiResolutionSTFTLoss(SR.FFT17, "cuda")
    rows = [smp[r].float().cuda().requires_grad_(True) for r in range(R)]
    c1, clsd = loss(rows, [trg[r].float().cuda() for r in range(R)], length)
    (c1 * g.cuda()).sum().backward()
    assert torch.equal(c1.detach().cpu(), l1) and torch.equal(clsd.cpu(), lsd)
    assert torch.equal(torch.stack([r.grad for r in rows]).cpu(), grad)


# ---------------------------------------------------------------------------------------- the selection inside batch_loss
class _Stub:
    """what batch_loss needs of a model: seg, lpc, receptive_field and a call returning (mus, bs_noclip, bs, log_bs)"""
    seg, lpc, receptive_field = 5, 0, 0

    def __init__(self, mus, bs_noclip):
        self.mus, self.bs_noclip = mus, bs_noclip

    def __call__(self, batch_h, batch_x, do=True, clip=True):
        bs = self.bs_noclip.clamp(min=1e-3)
        return self.mus, self.bs_noclip, bs, torch.log(bs)


def _batch_loss_run(target64, mus64, bn64, dtype, device, hip):
    from shallow_wavenet_amd.nets import cswnv_shift1 as mc
    mus = mus64.detach().clone().to(device, dtype).requires_grad_(True)
    bn = bn64.detach().clone().to(device, dtype).requires_grad_(True)
    target = target64.to(device, dtype)
    feat_len = mus.shape[1]
    fft = SR.FFT17
    loss, l_lap, l_lsd, l_err = T.batch_loss(
        _Stub(mus, bn), mc.LaplaceLoss(), mc.LSDloss(), None, None, target, None, feat_len, 0, fft,
        [torch.hann_window(n, dtype=dtype, device=device) for n in fft], do=False,
        eps_generator=torch.Generator().manual_seed(5), spectral_loss=spectral.MultiResolutionSTFTLoss(fft, device) if hip else None)
    (loss - l_lap).backward()                                   # the spectral term alone: the NLL part would only dilute it
    return (float(loss), float(l_lap), None if l_lsd is None else float(l_lsd), float(l_err),
            mus.grad.double().cpu(), bn.grad.double().cpu())


@pytest.mark.parametrize("kind", ["speech-like", "partly-silent", "all-zero"])
def test_batch_loss_selection_matches_float64(gpu_ok, kind):
    """`batch_loss` on a stub model (seg 5, lpc 0, 8 800 positions) with the HIP loss on the GPU in fp32 against the torch
    formulas on the CPU in float64, same host noise.  partly-silent: some (row, size) lsd terms are dropped; all-zero: every
    lsd term is dropped (loss_lsd None) and l1 still counts.  Gradients of loss - loss_laplace (the spectral term) in mus and
    bs_noclip within max(4 e32, 1e-6) of the largest float64 value, e32 = the float64 run repeated in fp32 on the CPU: that
    yardstick holds torch's sign flips (near 3e-3), a term weighted wrongly or not dropped is an error of the order 1 / 17."""
    N, seg = 8800, 5
    smp, trg = SR.signals(1, N + seg - 1, seed=31)
    target = trg[0].float().double()
    if kind == "partly-silent":
        target[3001:3701] = 0.0
    elif kind == "all-zero":
        target[:] = 0.0
    gen = torch.Generator().manual_seed(32)
    mus = torch.stack([trg[0, i:i + N] for i in range(seg)], 1) + 0.01 * torch.randn(N, seg, generator=gen, dtype=torch.float64)
    mus = mus.float().double()[None]
    bn = (0.01 + 0.02 * torch.rand(N, seg, generator=gen, dtype=torch.float64)).float().double()[None]
    ref = _batch_loss_run(target, mus, bn, torch.float64, "cpu", False)
    f32 = _batch_loss_run(target, mus, bn, torch.float32, "cpu", False)
    hip = _batch_loss_run(target, mus, bn, torch.float32, "cuda", True)
    print(f"batch_loss {kind}: loss {hip[0]:.7f} / {ref[0]:.7f}  lsd {hip[2]} / {ref[2]}  err {hip[3]:.7f} / {ref[3]:.7f}")
    assert (ref[2] is None) == (kind == "all-zero")
    assert (hip[2] is None) == (ref[2] is None)
    for i in (0, 1, 3):
        assert abs(hip[i] - ref[i]) <= 2e-5 * max(1.0, abs(ref[i])), (i, hip[i], ref[i])
    assert ref[0] - ref[1] > 0.01                                # the l1 term counts, also where every lsd term is dropped
    if ref[2] is not None:
        assert abs(hip[2] - ref[2]) <= 1e-3 * max(1.0, abs(ref[2])), (hip[2], ref[2])
    for what, i in (("d mus", 4), ("d bs_noclip", 5)):
        top = float(ref[i].abs().max())
        e32, ehip = float((f32[i] - ref[i]).abs().max()) / top, float((hip[i] - ref[i]).abs().max()) / top
        print(f"batch_loss {kind} {what}: torch fp32 {e32:.3e}  hip {ehip:.3e}  bound {max(4 * e32, 1e-6):.3e}")
        assert top > 0 and ehip <= max(4 * e32, 1e-6), (what, ehip, e32)
