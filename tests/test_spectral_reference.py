"""CPU: the float64 reference of the STFT loss (spectral_ref.py) against itself, so that the GPU tests of
test_gpu_spectral_edges.py stand on something verified: the linear surrogate of the backward equals autograd of the true
loss, the structural set carries no gradient, torch's own fp32 transform of sample - target has the float64 signs outside
it, the 1 % cap on the entries below the worst-case bound is met by the inputs of every case, and the state decoder reads
the layout include/swn_hip.h documents."""
import pytest
import torch

import spectral_ref as SR

CASES = SR.cases()


def _fp64_signs(d, sizes, zero_structural):
    out = []
    for n in sizes:
        c = SR.stft64(d, n)
        s = torch.sign(c).to(torch.int8)
        if zero_structural:
            st = SR.structural_mask(n, d.shape[1], c.shape[1], c.shape[2])
            s = torch.where(st.expand_as(s), torch.zeros_like(s), s)
        out.append(s)
    return out


@pytest.mark.parametrize("R,T,sizes", [(5, 8114, SR.FFT17), (1, 601, [n for n in SR.FFT17 if n <= 1024]), (3, 1025, [2048]),
                                       (2, 17, [32])], ids=["5x8114", "1x601", "3x1025-n2048", "2x17-n32"])
def test_surrogate_gradient_is_the_true_gradient_and_the_structural_set_carries_none(R, T, sizes):
    smp, trg, d = SR.signals_f32(R, T, seed=T)
    g = SR.weights(R, len(sizes), seed=3).double()
    true = SR.true_grad64(smp, trg, sizes, g)
    with_all = SR.grad64_from_signs(smp, _fp64_signs(d, sizes, False), sizes, g)
    without = SR.grad64_from_signs(smp, _fp64_signs(d, sizes, True), sizes, g)
    top = float(true.abs().max())
    e_sur, e_struct = float((with_all - true).abs().max()) / top, float((without - with_all).abs().max()) / top
    print(f"{R} x {T}: surrogate vs autograd {e_sur:.2e}, structural set zeroed moves it by {e_struct:.2e}")
    assert top > 0 and e_sur < 1e-12 and e_struct < 1e-12
    if R > 1:
        assert not true[R // 2].any() and not without[R // 2].any()         # the all-zero row of g


def _check_inputs(d, sizes, what):
    """torch fp32 signs of STFT(d) against float64 + the cap, per size and over the case.  Above the bound a mismatch is
    impossible for any fp32 evaluation and the count must be zero.  Below it rounding may decide: over the 58 cases torch's
    fp32 transform differs from float64 at ONE such entry (rows-16x2500, n = 1 792; 4.6 M entries in that case), so that
    count is printed, not asserted."""
    left, non, diff_struct, diff_below = 0, 0, 0, 0
    for n in sizes:
        rep = SR.sign_report(d, n, torch.sign(SR.stft(d, n, torch.float32)))
        assert rep["bad"] == 0, (what, n, rep["bad"])
        assert rep["compared"] + rep["left_out"] == rep["nonstructural"]
        left, non, diff_struct = left + rep["left_out"], non + rep["nonstructural"], diff_struct + rep["structural_diff"]
        diff_below += rep["left_out_diff"]
    print(f"{what}: {non} entries outside the structural set, {left} below the bound ({100.0 * left / non:.3f} %), "
          f"torch fp32 differs at {diff_below} of those and at {diff_struct} structural entries")
    assert left <= SR.BELOW_BOUND_CAP * non, (what, left, non)
    return left / non


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fp32_signs_equal_float64_outside_the_structural_set_and_the_cap_holds(case):
    name, R, T, sizes, seed = case
    _check_inputs(SR.signals_f32(R, T, seed)[2], sizes, name)


def test_cap_holds_on_the_inputs_of_the_exact_property_tests():
    for R, T, seed in ((5, 8114, 21), (5, 1025, 22), (5, 8114, 23)):
        _check_inputs(SR.signals_f32(R, T, seed)[2], [n for n in SR.FFT17 if T > n // 2], f"{R} x {T} seed {seed}")
    smp, trg, _ = SR.signals_f32(3, 8114, 24)
    _check_inputs(smp - SR.silence(trg), SR.FFT17, "partly silent target")


def test_case_table_is_the_one_the_issue_lists():
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)) == 58
    by = {c[0]: c for c in CASES}
    assert by["sizes-32-1024"][3] == list(range(32, 1025, 32)) and len(by["sizes-32-1024"][3]) == 32
    assert by["sizes-1056-2048"][3][0] == 1056 and by["sizes-1056-2048"][3][-1] == 2048 and len(by["sizes-1056-2048"][3]) == 32
    assert sorted(by["order-shuffled"][3]) == SR.FFT17 and by["order-shuffled"][3] not in (SR.FFT17, SR.FFT17[::-1])
    assert by["order-descending"][3] == SR.FFT17[::-1]
    for n in SR.EDGE_SIZES:
        hop = n // 4
        assert [SR.frames_of(T, n) for T in (n // 2 + 1, n // 2 + 2)] == [3, 3]
        assert [SR.frames_of(T, n) for T in (7 * hop - 1, 7 * hop, 8 * hop, 15 * hop, 16 * hop, 16 * hop + 1)] == [7, 8, 9, 16, 17, 17]
    for _, R, T, sizes, _ in CASES:
        assert 1 <= len(sizes) <= 32 and all(n % 32 == 0 and 32 <= n <= 2048 and T > n // 2 for n in sizes)


def test_structural_mask_marks_the_symmetric_frames():
    m = SR.structural_mask(32, 17, 17, 3)              # hop 8: frames centred on 0, 8, 16 = T - 1
    assert m[:, 0, 1].all() and m[:, 2, 1].all() and not m[:, :, 0].any()
    assert m[0, 1, 1] and m[16, 1, 1] and not m[1:16, 1, 1].any()
    m = SR.structural_mask(32, 18, 17, 3)              # T - 1 = 17 is no frame centre
    assert m[:, 0, 1].all() and not m[1:16, 1:, 1].any()
    # the claim itself: those imaginary parts are rounding noise in float64
    x = SR.signals_f32(2, 17, seed=1)[2]
    c = SR.stft64(x, 32)
    st = SR.structural_mask(32, 17, 17, 3).expand_as(c)
    assert float(c[st].abs().max()) < 1e-15 * float(c.abs().max()) * 32 and float(c[~st].abs().min()) > 0


def test_worst_case_bound_is_the_weighted_absolute_sum():
    x = SR.signals_f32(2, 100, seed=2)[2]
    b = SR.worst_case_bound(x, 32)
    assert tuple(b.shape) == (2, 13)
    w = torch.hann_window(32, dtype=torch.float64)
    pad = torch.cat([x[:, 1:17].flip(1), x, x[:, -17:-1].flip(1)], 1).abs()
    for f in (0, 5, 12):
        want = 35 * 2.0 ** -24 * (pad[:, 8 * f:8 * f + 32] * w).sum(1)
        assert torch.allclose(b[:, f], want, rtol=1e-14, atol=0)
    # it bounds |fp32 - float64| of torch's own fp32 transform with room to spare
    err = (SR.stft(x, 32, torch.float32).double() - SR.stft64(x, 32)).abs()
    assert bool((err <= b[:, None, :, None]).all())


def test_decode_state_reads_the_documented_layout():
    sizes, R, T = [64, 32], 2, 40                      # frames 3 / 6, bins 33 / 17
    signs = [torch.randint(-1, 2, (R, SR.bins_of(n), SR.frames_of(T, n), 2), generator=torch.Generator().manual_seed(n),
                           dtype=torch.int8) for n in sizes]
    code = lambda s: torch.where(s > 0, 1, torch.where(s < 0, 2, 0))
    state = torch.cat([(code(s[..., 0]) | (code(s[..., 1]) << 2)).permute(0, 2, 1).reshape(-1) for s in signs]).to(torch.uint8)
    back = SR.decode_state(state, R, T, sizes)
    assert all(torch.equal(a, b) for a, b in zip(back, signs))
    state[5] = 3
    with pytest.raises(AssertionError, match="code 3"):
        SR.decode_state(state, R, T, sizes)
    with pytest.raises(AssertionError, match="state size"):
        SR.decode_state(state[:-1], R, T, sizes)
