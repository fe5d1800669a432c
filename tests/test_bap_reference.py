"""CPU: the float64 reference of the band aperiodicity definition (tests/bap_ref.py) against a brute-force evaluation with Python
floats in the device's order of operations, its streaming rule against a frame-by-frame loop, the properties the definition
promises (d <= 2 e, zeros give exactly 0.0), and what tests/test_gpu_bap.py relies on: no case has a non-decisive frame, and the
derived bound is finite and far below anything audible on the rich tone - it pins the values, it is not vacuous."""
import numpy as np
import pytest

import bap_ref as R
import f0_ref


def _brute_frame(x, h, f, tau, hop, win, lag_hi, Wb):
    """frame f's (d, e0, e1) per band with Python floats, as the device orders them: y by one chain over k ascending, each sum as
    64 interleaved chains added in lane order (products and additions rounded separately: no fma here)"""
    n, S = len(x), f0_ref.span(win, lag_hi)
    B, T = h.shape
    c = (T - 1) // 2
    xs = lambda t: float(x[t]) if 0 <= t < n else 0.0
    s_b = f * hop - (Wb + tau) // 2
    assert f * hop - S // 2 <= s_b and s_b + tau + Wb <= f * hop - S // 2 + S
    out = []
    for b in range(B):
        y = {}
        for t in range(s_b, s_b + tau + Wb):
            acc = 0.0
            for k in range(T):
                acc = float(h[b, k]) * xs(t + c - k) + acc
            y[t] = acc
        part = [[0.0, 0.0, 0.0] for _ in range(64)]
        for j in range(Wb):
            y0, y1 = y[s_b + j], y[s_b + j + tau]
            p = part[j % 64]
            p[0] += (y0 - y1) * (y0 - y1)
            p[1] += y0 * y0
            p[2] += y1 * y1
        tot = [0.0, 0.0, 0.0]
        for p in part:
            for i in range(3):
                tot[i] = tot[i] + p[i]
        out.append(tot)
    return np.array(out)


@pytest.mark.parametrize("gi,kind", [(0, "rich"), (1, "tone"), (4, "rich-noisy"), (5, "half-silent")])
def test_one_frame_by_brute_force(gi, kind):
    p, h, rows = R.geometry_case(gi)
    kind_, n, x, ref = next(r for r in rows if r[0] == kind and r[1] == p["n_long"])
    F = f0_ref.frame_count(n, p["hop"])
    for f in (0, F // 2, F - 1):
        tau = int(ref["tau"][f])
        got = _brute_frame(x, h, f, tau, p["hop"], p["win"], p["lag_hi"], p["band_win"])
        for i, key in enumerate(("d", "e0", "e1")):
            assert np.allclose(got[:, i], ref[key][f], rtol=1e-9, atol=1e-24), (f, key)
        e = got[:, 1] + got[:, 2]
        ap = np.where(e > 0, got[:, 0] / np.where(e > 0, e, 1.0), 1.0)
        coded = R.code(ap, float(np.float32(R.FLOOR))) if ref["voiced"][f] else np.zeros(len(ap))
        assert np.all(np.abs(coded - ref["coded"][f]) <= ref["bound"][f]), (f, coded, ref["coded"][f], ref["bound"][f])


def test_band_signal_is_the_centred_convolution():
    g = np.random.Generator(np.random.PCG64(1))
    x = g.standard_normal(50).astype(np.float32)
    h = g.standard_normal((2, 7))
    y, eps = R.band_signals(x, h, -10, 70)
    for b in range(2):
        for t in (-10, -3, 0, 1, 25, 49, 52, 69):
            want = sum(h[b, k] * (float(x[t + 3 - k]) if 0 <= t + 3 - k < 50 else 0.0) for k in range(7))
            assert abs(y[b, t + 10] - want) <= eps[b, t + 10] + 1e-300
    assert np.all(y[:, :7] == 0.0) and np.all(y[:, 63:] == 0.0)          # out of the filter's reach of the signal
    # the identity tap returns the signal
    y1, _ = R.band_signals(x, np.ones((1, 1)), 0, 50)
    assert np.array_equal(y1[0], x.astype(np.float64))


def test_streaming_rule_and_reach():
    for hop, win, hi, T in ((110, 1024, 552, 255), (37, 97, 80, 31), (1, 64, 40, 3), (600, 128, 100, 63), (40, 256, 134, 1)):
        S, c = f0_ref.span(win, hi), (T - 1) // 2
        assert R.reach(win, hi, T) == S + 2 * c
        ahead = S - S // 2 + c
        for n in sorted({0, 1, ahead - 1, ahead, ahead + 1, ahead + hop - 1, ahead + hop, ahead + 7 * hop, 5000}):
            want = 0 if n < ahead else 1 + (n - ahead) // hop
            assert R.frames_ready_brute(hop, win, hi, T, n, False) == want, (hop, n)
            assert R.frames_ready_brute(hop, win, hi, T, n, True) == 1 + n // hop
    assert 1577 - 788 + 127 == 916                                       # the latency at the shipped geometry with 255 taps


def test_band_counts_follow_the_reference():
    assert [len(R.bands(fs)) for fs in (8000, 12000, 16000, 22050, 24000, 44100, 48000)] == [0, 1, 1, 2, 3, 5, 5]
    assert R.bands(22050) == [(1500.0, 4500.0), (4500.0, 7500.0)]


@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)))
def test_cases_are_decisive_and_the_ratio_is_bounded(gi):
    p, h, rows = R.geometry_case(gi)
    assert h.shape == (1 if p["edges"] is None else len(p["edges"]), p["n_taps"])
    kinds = set()
    for kind, n, x, ref in rows:
        kinds.add(kind)
        assert ref["decisive"].all(), (kind, n, np.flatnonzero(~ref["decisive"]))
        assert np.all(ref["d"] <= 2.0 * (ref["e0"] + ref["e1"]) * (1 + 1e-12))
        assert np.all(ref["ap"] >= 0.0) and np.all(ref["ap"] <= 2.0 * (1 + 1e-12))
        assert np.all(ref["coded"] <= 0.0) and np.all(ref["coded"] >= 10.0 * np.log10(np.float32(R.FLOOR)))
        assert np.all(ref["coded"][~ref["voiced"]] == 0.0) and np.all(ref["bound"][~ref["voiced"]] == 0.0)
        assert np.isfinite(ref["bound"]).all() and np.all(ref["bound"] >= 0.0)
        if kind == "zeros":
            assert not ref["coded"].any() and np.all(ref["ap"] == 1.0) and not ref["bound"].any()
        if kind.startswith("rich"):
            assert np.all(ref["bound"] < 1e-3), (kind, n, ref["bound"].max())
    assert kinds == set(R.SIGNALS)
    # the tile-edge lengths exist where the hop divides them
    if p["hop"] == 1:
        S = f0_ref.span(p["win"], p["lag_hi"])
        assert {R.TILE - 1 - S, R.TILE - S, R.TILE + 1 - S} <= {n for _, n, _, _ in rows}


@pytest.mark.parametrize("Wb", R.WB_VALUES)
def test_band_win_cases_are_decisive(Wb):
    p, h, rows = R.band_win_case(Wb)
    assert p["band_win"] == Wb and h.shape == (2, R.WB_TAPS)
    for kind, n, x, ref in rows:
        assert ref["decisive"].all(), (kind, Wb)
        assert np.isfinite(ref["bound"]).all()
        if kind == "rich":
            assert ref["voiced"].sum() > 10 and np.all(ref["bound"] < 1e-3)


def test_the_rich_tone_is_more_periodic_than_noise():
    """not a target, a sanity check of the measure: the steady rich tone's lower band is well below 0 dB, noise is near it"""
    p, h, rows = R.geometry_case(3)
    steady = next(r for r in rows if r[0] == "rich-steady" and r[1] == p["n_long"])[3]
    noisy = next(r for r in rows if r[0] == "rich-noisy" and r[1] == p["n_long"])[3]
    v = steady["voiced"]
    assert v.sum() > 20 and np.median(steady["coded"][v, 0]) < -8.0
    vn = noisy["voiced"]
    assert vn.sum() > 20 and np.median(noisy["coded"][vn, 0]) > np.median(steady["coded"][v, 0])
