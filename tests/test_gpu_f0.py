"""GPU: F0 and voicing on the device (swn_f0 / torch.ops.swn.f0 / pitch.F0Extractor / pitch.F0Stream) against the float64
restatement of the definition, tests/f0_ref.py, whose docstring derives the two bounds used here.

Values: six geometries (fs / hop / win / Hz range, f0_ref.GEOMETRIES: 8000/40/256, 8000/37/97 - an odd window and a hop that
divides nothing -, 16000/80/512, the shipped 22050/110/1024, hop 1, and a hop longer than the frame) x five signals (harmonic
tone with vibrato and weak noise, the same with a silent first half, white noise, zeros, a two-partial glide that leaves the lag
range at the top) x ten lengths (1, S // 2, S // 2 + 1, S - 1, S, S + 1, 15 hop - 1, 16 hop, 17 hop + 3 and a few thousand samples):
the fifty signals of a geometry are one ragged batch, one device call.  Explicit lags through the op (f0_ref.LAG_CASES): lag_hi + 1
on both sides of 64 and 256, lag_hi = 1535 with win = 2048, lag_lo = 2, lag_lo = lag_hi, win = 16.  tests/test_f0_reference.py
shows on the CPU that no frame of any of these is non-decisive, so the 1 % a case may leave out is never used.

Bits (torch.equal): a row alone against the row in ragged batches of 3 and of 70 (a launch group takes 64 entries), any split of
[0, F) into ranges, windows with t0 > 0 that hold exactly what a range reads, F0Stream in chunks of 1, 7, hop, S and 1000 samples."""
import functools

import numpy as np
import pytest
import torch

import f0_ref as R
from shallow_wavenet_amd import pitch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SMALL = (8000, 37, 97, 100.0, 1000.0)            # fs, hop, win, minf0, maxf0 of the bit-identity tests
SHIPPED = (22050, 110, 1024, 40.0, 700.0)


@functools.lru_cache(maxsize=None)
def _ext(fs, hop, win, minf0, maxf0):
    return pitch.F0Extractor(fs, hop, minf0, maxf0, win, R.THRESHOLD, device=DEV)


def _compare(tag, out, ref, fs, win, lag_hi):
    """one signal's device frames (F, 2) against the reference, by the rules of f0_ref.py; prints the figures before it asserts"""
    F = ref["f0"].shape[0]
    assert out.shape == (F, 2) and np.isfinite(out).all(), tag
    dec, voiced = ref["decisive"], ref["voiced"]
    assert (~dec).sum() <= 0.01 * F, (tag, "non-decisive frames", np.flatnonzero(~dec))
    dev_voiced = out[:, 0] != 0.0
    bf, ba = R.bounds(ref, fs, win, lag_hi)
    ef, ea = np.abs(out[:, 0].astype(np.float64) - ref["f0"]), np.abs(out[:, 1].astype(np.float64) - ref["ap"])
    mv = dec & voiced
    ma = dec | (~voiced & ~dev_voiced)
    worst_f = float((ef[mv] / bf[mv]).max()) if mv.any() else 0.0
    worst_a = float((ea[ma] / ba[ma]).max()) if ma.any() else 0.0
    print(f"{tag}: {F} frames, {int(voiced.sum())} voiced, {int((~dec).sum())} left out; |f0 - ref| / bound <= {worst_f:.3f}, "
          f"|ap - ref| / bound <= {worst_a:.3f}")
    assert np.array_equal(dev_voiced[dec], voiced[dec]), (tag, np.flatnonzero(dec & (dev_voiced != voiced)))
    assert np.all(ref["f0"][~voiced] == 0.0) and np.all(out[~dev_voiced, 0] == 0.0)
    assert np.all(ef[mv] <= bf[mv]), (tag, np.flatnonzero(mv & (ef > bf)), worst_f)
    assert np.all(ea[ma] <= ba[ma]), (tag, np.flatnonzero(ma & (ea > ba)), worst_a)


# ------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=[f"fs{g[0]}-hop{g[1]}-win{g[2]}" for g in R.GEOMETRIES])
def test_values_against_the_float64_reference(gpu_ok, gi):
    p, rows = R.geometry_case(gi)
    ext = _ext(p["fs"], p["hop"], p["win"], p["minf0"], p["maxf0"])
    assert (ext.lag_lo, ext.lag_hi) == (p["lag_lo"], p["lag_hi"])
    out = ext([torch.from_numpy(x) for _, _, x, _ in rows]).cpu().numpy()
    assert out.shape == (len(rows), max(R.frame_count(n, p["hop"]) for _, n, _, _ in rows), 2)
    for r, (kind, n, x, ref) in enumerate(rows):
        F = R.frame_count(n, p["hop"])
        _compare(f"{kind} n={n}", out[r, :F], ref, p["fs"], p["win"], p["lag_hi"])
        assert not out[r, F:].any()                                     # zeros past a row's frames
        if kind == "zeros":
            assert np.all(out[r, :F, 0] == 0.0) and np.all(out[r, :F, 1] == 1.0)


@pytest.mark.parametrize("ci", range(len(R.LAG_CASES)),
                         ids=[f"win{c[2]}-lags{c[3]}-{c[4]}" for c in R.LAG_CASES])
def test_explicit_lags_through_the_op(gpu_ok, ci):
    p, rows = R.lag_case(ci)
    n = rows[0][1]
    wav = torch.from_numpy(np.stack([x for _, _, x, _ in rows])).to(DEV)
    F = R.frame_count(n, p["hop"])
    E = len(rows)
    out = torch.ops.swn.f0(wav, [0] * E, [n] * E, [n] * E, [0] * E, [F] * E, float(p["fs"]), p["hop"], p["win"], p["lag_lo"],
                           p["lag_hi"], R.THRESHOLD).cpu().numpy()
    for r, (kind, _, x, ref) in enumerate(rows):
        _compare(f"{kind} lags {p['lag_lo']}..{p['lag_hi']}", out[r], ref, p["fs"], p["win"], p["lag_hi"])


# ------------------------------------------------------------------------------------------------------ bits
def _mixed(n, fs, seed):
    """a signal with voiced and unvoiced stretches: tone, silence, noise"""
    x = R.signal("tone", n, fs, seed=seed)
    x[n // 3:n // 2] = 0.0
    x[n // 2:2 * n // 3] = R.signal("noise", 2 * n // 3 - n // 2, fs, seed=seed + 1)
    return x


@pytest.mark.parametrize("geom,n", [(SMALL, 1500), (SHIPPED, 5000)], ids=["fs8000-hop37-win97", "shipped"])
def test_a_row_alone_and_in_ragged_batches(gpu_ok, geom, n):
    ext = _ext(*geom)
    fs, hop = geom[0], geom[1]
    x = torch.from_numpy(_mixed(n, fs, 5))
    F = ext.frame_count(n)
    alone = ext(x)
    assert alone.shape == (1, F, 2)
    assert (alone[0, :, 0] != 0).any() and (alone[0, :, 0] == 0).any()          # voiced and unvoiced frames
    for rows_n, at in ((3, 1), (70, 67)):
        g = np.random.Generator(np.random.PCG64(rows_n))
        lens = [int(v) for v in g.integers(1, 2 * n if rows_n == 3 else 600, rows_n)]
        rows = [torch.from_numpy(_mixed(m, fs, 100 + i)) for i, m in enumerate(lens)]
        rows[at] = x
        out = ext(rows)
        assert torch.equal(out[at, :F], alone[0]) and not out[at, F:].any()
        # ... as a padded batch whose padding is NaN: nothing outside a row's samples is read
        S = max(r.numel() for r in rows)
        batch = torch.full((rows_n, S), NAN)
        for i, r in enumerate(rows):
            batch[i, :r.numel()] = r
        assert torch.equal(ext(batch, [r.numel() for r in rows]), out)
        for i in (0, rows_n - 1):                                       # and the others are their own one-shot results
            Fi = ext.frame_count(rows[i].numel())
            assert torch.equal(out[i, :Fi], ext(rows[i])[0]) and not out[i, Fi:].any()


@pytest.mark.parametrize("geom,n", [(SMALL, 1500), (SHIPPED, 5000), ((8000, 600, 128, 80.0, 500.0), 4000)],
                         ids=["fs8000-hop37-win97", "shipped", "hop600"])
def test_frame_ranges_and_windows(gpu_ok, geom, n):
    ext = _ext(*geom)
    fs, hop, S = geom[0], geom[1], ext.span
    x = torch.from_numpy(_mixed(n, fs, 9)).to(DEV)
    F = ext.frame_count(n)
    whole = ext(x)[0]
    g = np.random.Generator(np.random.PCG64(11))
    for cuts in ([0, F], [0, 1, F], [0, F - 1, F], [0, F // 2, F // 2, F], sorted({0, F, *[int(v) for v in g.integers(0, F, 5)]})):
        parts = [ext.frames(x, 0, n, n, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        assert torch.equal(torch.cat(parts), whole), cuts
    # windows that hold exactly what a range reads, in a buffer that is NaN everywhere else
    for a, b in ((0, 1), (F - 1, F), (F // 2, F // 2 + 3), (1, F), (0, F), (F // 3, F // 3 + 1)):
        lo, hi = max(0, a * hop - S // 2), min(n, (b - 1) * hop - S // 2 + S)
        buf = torch.full((1, hi - lo + 13), NAN, device=DEV)
        buf[0, :hi - lo] = x[lo:hi]
        got = ext.frames(buf, [lo], [hi - lo], [n], [a], [b])[0]
        assert torch.equal(got, whole[a:b]), (a, b)
        if (b - 1) * hop - S // 2 + S <= n:                             # every sample is there: the length need not be known
            assert torch.equal(ext.frames(buf, [lo], [hi - lo], [-1], [a], [b])[0], whole[a:b]), (a, b)
    # one sample less on either side is refused, not read
    a = F // 2
    lo, hi = a * hop - S // 2, a * hop - S // 2 + S
    assert 0 < lo and hi < n
    for t0, t1 in ((lo + 1, hi), (lo, hi - 1)):
        with pytest.raises(RuntimeError, match="window"):
            ext.frames(x[t0:t1], t0, t1 - t0, n, a, a + 1)


@pytest.mark.parametrize("chunk", ["1", "7", "hop", "S", "1000"])
def test_stream_is_bit_identical_to_the_one_shot_call(gpu_ok, chunk):
    geom = (8000, 40, 256, 60.0, 500.0)
    ext = _ext(*geom)
    n = 2500
    x = torch.from_numpy(_mixed(n, geom[0], 21)).to(DEV)
    whole = ext(x)[0]
    size = {"hop": ext.hop, "S": ext.span}.get(chunk) or int(chunk)
    st = pitch.F0Stream(ext)
    got, k = [], 0
    for at in range(0, n, size):
        out = st.push(x[at:at + size])
        k += out.shape[0]
        assert k == pitch.f0_frames_ready(ext.hop, ext.win, ext.lag_hi, min(n, at + size))
        assert st._buf.numel() <= ext.span + ext.hop + size
        got.append(out)
    last = st.finish()
    assert last.shape[0] == ext.frame_count(n) - k and last.shape[0] > 0
    assert torch.equal(torch.cat(got + [last]), whole)


def test_stream_of_a_signal_shorter_than_a_frame(gpu_ok):
    ext = _ext(*SHIPPED)
    x = torch.from_numpy(R.signal("tone", 700, 22050, seed=3)).to(DEV)
    st = pitch.F0Stream(ext)
    assert st.push(x[:300]).shape == (0, 2) and st.push(x[300:]).shape == (0, 2)
    assert torch.equal(st.finish(), ext(x)[0])


def test_zeros_and_the_rows_past_their_frames(gpu_ok):
    ext = _ext(*SHIPPED)
    out = ext(torch.zeros(2, 3000), [3000, 500])
    assert out.shape == (2, 28, 2)
    assert torch.equal(out[0], torch.tensor([0.0, 1.0], device=out.device).expand(28, 2))
    assert torch.equal(out[1, :5], out[0, :5]) and not out[1, 5:].any()
    # a row without frames in a call with others: its output stays zero
    x = torch.from_numpy(_mixed(3000, 22050, 4))
    two = ext.frames(torch.stack([x, x]), [0, 0], [3000, 3000], [3000, 3000], [0, 7], [28, 7])
    assert torch.equal(two[0], ext(x)[0]) and not two[1].any()
