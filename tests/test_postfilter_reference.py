"""CPU: the references of tests/postfilter_ref.py hold each other, and the host MLSA filter (csrc/swn_dsp.c) is held to them.

- restore_ref (the serial long-double definition) against transfer_function (the closed form) over the case grid of the device
  tests: max |rfft(h) - H| <= 1e-12 max|H|, the impulse response decayed below 1e-20 at the end of the window.  1e-12 is 250 times
  what fp64 C code reaches on this comparison (4e-15), and the reference is long double.
- dsp.MLSAFilter.synthesis with one constant frame against the same closed form (1e-12 of max|H|) and against restore_ref with
  the identity FIR (within E64, the fp64 term of the device bound): the host code held to what it implements, not to the exp()
  its Pade table approximates.
- restore_ref resumed from the state it returns equals its one-shot output exactly (the state taken unrounded, in long double;
  its float64 rounding, what the device tests compare and upload, is the same array rounded and resumes within E64)."""
import numpy as np
import pytest

import postfilter_ref as R
from shallow_wavenet_amd import dsp
from shallow_wavenet_amd.nets.dswnv import decode_mu_law


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_serial_reference_realises_the_transfer_function(name):
    c = R.case(name)
    H = R.transfer_function(*c.args, R.IMPULSE_N)
    assert H.dtype == np.complex128 and H.shape == (R.IMPULSE_N // 2 + 1,)
    err = float(np.abs(np.fft.rfft(c.h) - H).max())
    hmax = float(np.abs(H).max())
    print(f"{name}: max|H| {hmax:.3g}  err/max|H| {err / hmax:.3g}  tail {c.tail:.3g}  L1 {c.l1:.4g}")
    assert c.tail < 1e-20, (name, c.tail)
    assert err <= 1e-12 * hmax, (name, err, hmax)


def test_the_grid_contains_what_it_must():
    orders = {c[1] for c in R.CASES}
    assert {1, 2, 3, 31, 32, 33, 49, 61, 62} <= orders and max(orders) == 62
    assert {0.455, 0.466, 0.7, 0.0, -0.3} <= {c[2] for c in R.CASES}
    for m in (1, 33, 62):
        assert any(c[1] == m and c[2] <= 0 for c in R.CASES), m
    for m in (1, 2, 62):
        assert {c[3] for c in R.CASES if c[1] == m} == {4, 5}, m
    assert {R.case(n).n_taps for n in R.CASE_NAMES} == {1, 2, 64, 65, 255, 256}
    assert any(c[1:5] == (24, 0.41, 5, 2.0) for c in R.CASES)
    assert np.array_equal(R.low_cut_255(), dsp.low_cut_taps(22050))
    mc = np.random.default_rng(0).normal(size=50)
    assert np.array_equal(R.mc2b(mc, 0.455), dsp.mc2b(mc, 0.455))                 # the two-line recursion is the project's mc2b
    for n in R.CASE_NAMES:
        c = R.case(n)
        assert c.b[0] != 0.0 and float(np.abs(c.x).max()) < 1.0


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_host_mlsa_filter_against_the_exact_references(name):
    c = R.case(name)
    one = np.array([1.0])
    f = dsp.MLSAFilter(c.order, c.alpha, hopsize=110, pade=c.pade)
    imp = np.zeros(R.IMPULSE_N)
    imp[0] = 1.0
    h = f.synthesis(imp, c.b[None])
    H = R.transfer_function(c.b, c.alpha, c.pade, one, R.IMPULSE_N)
    err, hmax = float(np.abs(np.fft.rfft(h) - H).max()), float(np.abs(H).max())
    assert float(np.abs(h[-64:]).max()) < 1e-20
    assert err <= 1e-12 * hmax, (name, err, hmax)
    x = c.x[0, :R.N_LONG].astype(np.float64)
    want, _ = R.restore_ref(x, c.b, c.alpha, c.pade, one)
    l1, _ = R.impulse_l1(c.b, c.alpha, c.pade, one)
    e = R.e64(c.order, c.pade, 1, l1, float(np.abs(x).max()))
    dev = float(np.abs(f.synthesis(x, c.b[None]) - want).max())
    print(f"{name}: host rfft err/max|H| {err / hmax:.3g}  |host - ref| / E64 {dev / e:.3g}")
    assert dev <= e, (name, dev, e)


@pytest.mark.parametrize("name", ["m1-p4-one", "m2-p4-lowcut", "m33-p5-a0-r64", "m62-p5-r256"])
def test_reference_resumes_from_its_own_state_exactly(name):
    c = R.case(name)
    x = c.x[1, :700].astype(np.float64)
    whole, end = R.restore_ref(x, *c.args)
    assert end.dtype == np.float64 and end.shape == (R.state_doubles(c.order, c.pade, c.n_taps),)
    for cut in (1, 254, 255, 256, 512):
        y0, s0 = R.restore_ref(x[:cut], *c.args, state_dtype=np.longdouble)
        y1, s1 = R.restore_ref(x[cut:], *c.args, state=s0, state_dtype=np.longdouble)
        assert np.array_equal(np.concatenate([y0, y1]), whole), (name, cut)
        assert np.array_equal(s1.astype(np.float64), end), (name, cut)
        # the float64 state (what is compared with and uploaded to the device) is that state rounded, in the same layout, and
        # resuming from it moves the outputs by no more than its rounding through the filter
        y0r, s0r = R.restore_ref(x[:cut], *c.args)
        assert s0r.dtype == np.float64 and np.array_equal(s0r, s0.astype(np.float64))
        y1r, _ = R.restore_ref(x[cut:], *c.args, state=s0r)
        assert float(np.abs(y1r - whole[cut:]).max()) <= c.e64(), (name, cut)


def test_mulaw_table_is_the_decoder_of_the_nets():
    for q in (256, 90, 2):
        t = R.mulaw_table(q)
        assert np.array_equal(t[:q], decode_mu_law(np.arange(q, dtype=np.float64), q))
        assert np.all(t[q:] == t[q - 1])
    got = R.mulaw_decode([-1, -2 ** 31, 0, 89, 90, 255, 256, 1000, 2 ** 31 - 1], 90)
    t = R.mulaw_table(90)
    assert np.array_equal(got, t[[0, 0, 0, 89, 89, 89, 89, 89, 89]])
