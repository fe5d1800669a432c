"""CPU: the float64 restatement of the F0 / voicing definition (tests/f0_ref.py) gives the known answers, and on every case of
tests/test_gpu_f0.py it makes no comparison closer than four times the derived error scale - so the GPU test's cap on frames it
may leave out as non-decisive hides nothing."""
import numpy as np
import pytest

import f0_ref as R


def test_a_sine_of_integer_period_gives_fs_over_p():
    for fs, hop, win, minf0, maxf0, P in [(8000, 40, 256, 60.0, 500.0, 50), (16000, 80, 512, 50.0, 600.0, 123),
                                          (22050, 110, 1024, 40.0, 700.0, 200)]:
        lo, hi = R.lags(fs, minf0, maxf0)
        assert lo < P < hi
        n = 6 * R.span(win, hi)
        x = np.sin(2 * np.pi * np.arange(n) / P).astype(np.float32)
        ref = R.analyse(x, fs, hop, win, lo, hi, R.THRESHOLD)
        S = R.span(win, hi)
        f = np.arange(R.frame_count(n, hop))
        interior = (f * hop - S // 2 >= 0) & (f * hop - S // 2 + S <= n)
        assert interior.sum() > 10
        assert ref["voiced"][interior].all()
        assert np.all(np.abs(ref["f0"][interior] - fs / P) <= 0.005 * fs / P), (fs, P, ref["f0"][interior])
        assert np.all(ref["ap"][interior] < R.THRESHOLD)


def test_zeros_give_exactly_zero_and_one():
    ref = R.analyse(np.zeros(1000, dtype=np.float32), 8000, 40, 256, 16, 134, R.THRESHOLD)
    assert np.all(ref["f0"] == 0.0) and np.all(ref["ap"] == 1.0) and not ref["voiced"].any()


def test_white_noise_is_unvoiced_everywhere():
    for gi, (fs, hop, win, minf0, maxf0, n_long) in enumerate(R.GEOMETRIES):
        lo, hi = R.lags(fs, minf0, maxf0)
        ref = R.analyse(R.signal("noise", n_long, fs, seed=gi), fs, hop, win, lo, hi, 0.1)
        assert not ref["voiced"].any() and np.all(ref["f0"] == 0.0)


def test_the_decision_follows_the_definition_on_a_hand_made_curve():
    """first lag below the threshold, the walk, the refinement and its guards, the first arg-min of an unvoiced frame"""
    dp = np.ones(12)
    dp[[4, 5, 6, 7]] = [0.5, 0.08, 0.04, 0.06]      # first hit at 5, walk to 6
    dp[9] = 0.01                                     # a deeper dip further up is not reached
    r = R.decide(dp, 1200.0, 64, 2, 10, 0.1)
    den = 0.08 - 2 * 0.04 + 0.06
    assert r["voiced"] and r["tau"] == 6 and r["refined"] and r["decisive"]
    assert r["f0"] == 1200.0 / (6 + 0.5 * (0.08 - 0.06) / den) and r["ap"] == 0.04
    r = R.decide(dp, 1200.0, 64, 2, 6, 0.1)         # the walk stops at lag_hi; d'(lag_hi + 1) is above: still a minimum
    assert r["tau"] == 6 and r["refined"]
    r = R.decide(dp, 1200.0, 64, 2, 5, 0.1)         # ... and here it is below: a guard fails, no shift
    assert r["tau"] == 5 and not r["refined"] and r["f0"] == 240.0
    dp = np.array([1.0, 1.0, 0.7, 0.4, 0.9, 0.4, 0.8, 1.0])
    r = R.decide(dp, 1200.0, 64, 2, 6, 0.1)
    assert not r["voiced"] and r["f0"] == 0.0 and r["tau"] == 3 and r["ap"] == 0.4 and r["decisive"]
    dp[2] = 0.1 * (1 + 2.0 ** -50)                  # a threshold test inside the error scale
    assert not R.decide(dp, 1200.0, 64, 2, 6, 0.1)["decisive"]


def test_a_second_summation_order_and_longdouble_change_no_decision():
    fs, hop, win, minf0, maxf0, _ = R.GEOMETRIES[0]
    lo, hi = R.lags(fs, minf0, maxf0)
    x = R.signal("tone", 1200, fs, seed=77)
    ref = R.analyse(x, fs, hop, win, lo, hi, R.THRESHOLD)
    S, L1 = R.span(win, hi), hi + 1
    xl = x.astype(np.longdouble)
    for f in range(0, R.frame_count(x.shape[0], hop), 5):
        s = f * hop - S // 2
        seg = np.zeros(S, dtype=np.longdouble)
        a, b = max(s, 0), min(s + S, x.shape[0])
        seg[a - s:b - s] = xl[a:b]
        for dtype, order in ((np.longdouble, 1), (np.float64, -1)):
            g = seg.astype(dtype)
            d = np.array([np.sum(((g[:win] - g[t:t + win]) ** 2)[::order]) for t in range(1, L1 + 1)], dtype=dtype)
            dp = np.ones(L1 + 1)
            c = np.cumsum(d)
            dp[1:] = np.where(c > 0, d * np.arange(1, L1 + 1) / np.where(c > 0, c, 1), 1.0).astype(np.float64)
            r = R.decide(dp, fs, win, lo, hi, R.THRESHOLD)
            assert r["voiced"] == ref["voiced"][f] and r["tau"] == ref["tau"][f] and r["refined"] == ref["refined"][f]
            if r["voiced"]:
                assert abs(r["f0"] - ref["f0"][f]) <= 1e-12 * ref["f0"][f]


@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)))
def test_every_frame_of_the_gpu_cases_is_decisive(gi):
    p, rows = R.geometry_case(gi)
    assert len(rows) == len(R.SIGNALS) * 10
    for kind, n, x, ref in rows:
        assert ref["f0"].shape[0] == R.frame_count(n, p["hop"])
        assert ref["decisive"].all(), (p, kind, n, np.flatnonzero(~ref["decisive"]))
        assert np.all(ref["f0"][~ref["voiced"]] == 0.0)


def test_the_gpu_cases_hold_voiced_and_unvoiced_frames():
    voiced = unvoiced = 0
    for gi in range(len(R.GEOMETRIES)):
        for _, _, _, ref in R.geometry_case(gi)[1]:
            voiced += int(ref["voiced"].sum())
            unvoiced += int((~ref["voiced"]).sum())
    assert voiced > 100 and unvoiced > 100
    # the shipped geometry itself sees both on the tone
    tone = [ref for kind, n, _, ref in R.geometry_case(3)[1] if kind == "tone" and n == 8000][0]
    assert tone["voiced"].sum() > 30 and np.all(np.abs(tone["f0"][tone["voiced"]] - 120.0) < 6.0)


@pytest.mark.parametrize("ci", range(len(R.LAG_CASES)))
def test_every_frame_of_the_explicit_lag_cases_is_decisive(ci):
    p, rows = R.lag_case(ci)
    for kind, n, x, ref in rows:
        assert ref["decisive"].all(), (p, kind, np.flatnonzero(~ref["decisive"]))
