"""GPU: band aperiodicity on the device (swn_bap / torch.ops.swn.bap / pitch.BandAperiodicityExtractor / pitch.BapStream) against
the float64 restatement of the definition, tests/bap_ref.py, whose docstring derives the bound used here.

Values: six geometries (bap_ref.GEOMETRIES: two bands of 31 taps on an odd window, one identity tap with a 16-sample sum, 255
taps with a 255-sample sum, the shipped defaults, five bands with a hop longer than the reach, hop 1) x eight signals (f0_ref's
five, and a rich 120 Hz tone with vibrato, with 5 % noise, and without vibrato) x f0_ref's lengths, the first length that holds
frame 0's halo and - at hop 1 - the lengths whose band-pass region is one tile - 1, one tile and one tile + 1: a geometry's signals
are one ragged batch, one device call.  The sum windows 63, 64, 65 and 129 (the edges of the 64 partial chains) on one geometry.
tests/test_bap_reference.py shows on the CPU that no frame of any of these is non-decisive, so the 1 % a case may leave out is
never used.  Columns 0 - 1 are compared with torch.ops.swn.f0, bit for bit.

Bits (torch.equal): a row alone against the row in ragged batches of 3 and of 70 (a launch group takes 64 entries), a NaN-padded
batch, any split of [0, F) into ranges, NaN-surrounded windows that hold exactly the halo-extended reach, BapStream in chunks of
1, 7, hop, reach and 1000 samples."""
import functools

import numpy as np
import pytest
import torch

import bap_ref as R
import f0_ref
from shallow_wavenet_amd import pitch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
# fs, hop, win, minf0, maxf0, band edges, taps, band_win of the bit-identity tests
SMALL = (8000, 37, 97, 100.0, 1000.0, ((500.0, 1500.0), (1500.0, 3000.0)), 31, 97)
SHIPPED = (22050, 110, 1024, 40.0, 700.0, None, 255, 256)
HOP600 = (8000, 600, 128, 80.0, 500.0, ((300.0, 900.0), (900.0, 1500.0), (1500.0, 2100.0)), 63, 64)
STREAM = (8000, 40, 256, 60.0, 500.0, ((500.0, 1500.0), (1500.0, 3000.0)), 31, 64)


@functools.lru_cache(maxsize=None)
def _ext(fs, hop, win, minf0, maxf0, edges, n_taps, band_win):
    return pitch.BandAperiodicityExtractor(fs, hop, minf0, maxf0, win, R.THRESHOLD, None if edges is None else list(edges), n_taps,
                                           band_win, device=DEV)


@functools.lru_cache(maxsize=None)
def _f0_ext(fs, hop, win, minf0, maxf0):
    return pitch.F0Extractor(fs, hop, minf0, maxf0, win, R.THRESHOLD, device=DEV)


def _case_ext(p, h):
    return pitch.BandAperiodicityExtractor(p["fs"], p["hop"], p["minf0"], p["maxf0"], p["win"], R.THRESHOLD, taps=h,
                                           band_win=p["band_win"], device=DEV)


def _compare(tag, out, ref):
    """one signal's device frames (F, 2 + B) against the reference's coded values, by the rules of bap_ref.py; returns the
    worst share of the bound"""
    F, B = ref["coded"].shape
    assert out.shape == (F, 2 + B) and np.isfinite(out).all(), tag
    dec, voiced = ref["decisive"], ref["voiced"]
    assert (~dec).sum() <= 0.01 * F, (tag, "non-decisive frames", np.flatnonzero(~dec))
    dev_voiced = out[:, 0] != 0.0
    assert np.array_equal(dev_voiced[dec], voiced[dec]), tag
    assert np.all(out[~dev_voiced, 2:] == 0.0), tag                     # exactly 0.0 on unvoiced frames
    assert np.all(out[:, 2:] <= 0.0), tag
    err = np.abs(out[:, 2:].astype(np.float64) - ref["coded"])[dec]
    bound = ref["bound"][dec]
    share = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(share.max()) if share.size else 0.0
    assert np.all(err <= bound), (tag, worst, np.argwhere(err > bound)[:5])
    return worst


def _run_case(name, p, h, rows):
    ext = _case_ext(p, h)
    assert (ext.lag_lo, ext.lag_hi, ext.n_bands, ext.n_taps, ext.band_win) == (p["lag_lo"], p["lag_hi"], h.shape[0], h.shape[1],
                                                                               p["band_win"])
    wavs = [torch.from_numpy(x) for _, _, x, _ in rows]
    out_t = ext(wavs)
    f0_t = _f0_ext(p["fs"], p["hop"], p["win"], p["minf0"], p["maxf0"])(wavs)
    assert torch.equal(out_t[..., :2], f0_t)                            # swn_f0's bits
    out = out_t.cpu().numpy()
    assert out.shape == (len(rows), max(f0_ref.frame_count(n, p["hop"]) for _, n, _, _ in rows), 2 + h.shape[0])
    worst, n_voiced = {}, 0
    for r, (kind, n, x, ref) in enumerate(rows):
        F = f0_ref.frame_count(n, p["hop"])
        worst[kind] = max(worst.get(kind, 0.0), _compare(f"{kind} n={n}", out[r, :F], ref))
        n_voiced += int(ref["voiced"].sum())
        assert not out[r, F:].any()                                     # zeros past a row's frames
        if kind == "zeros":
            assert np.all(out[r, :F, 0] == 0.0) and np.all(out[r, :F, 1] == 1.0) and not out[r, :F, 2:].any()
    print(f"{name}: {len(rows)} signals, {n_voiced} voiced frames; worst |coded - ref| / bound per signal kind: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert n_voiced > 0


# ------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=[f"fs{g[0][0]}-hop{g[0][1]}-win{g[0][2]}" for g in R.GEOMETRIES])
def test_values_against_the_float64_reference(gpu_ok, gi):
    p, h, rows = R.geometry_case(gi)
    _run_case(f"fs {p['fs']} hop {p['hop']} win {p['win']} T {p['n_taps']} Wb {p['band_win']}", p, h, rows)


@pytest.mark.parametrize("Wb", R.WB_VALUES)
def test_band_win_at_the_edges_of_the_partial_chains(gpu_ok, Wb):
    p, h, rows = R.band_win_case(Wb)
    _run_case(f"Wb {Wb}", p, h, rows)


# ------------------------------------------------------------------------------------------------------ bits
def _mixed(n, fs, seed):
    """a signal with voiced and unvoiced stretches: rich tone, silence, noise"""
    x = R.signal("rich", n, fs, seed=seed)
    x[n // 3:n // 2] = 0.0
    x[n // 2:2 * n // 3] = f0_ref.signal("noise", 2 * n // 3 - n // 2, fs, seed=seed + 1)
    return x


@pytest.mark.parametrize("geom,n", [(SMALL, 1500), (SHIPPED, 5000)], ids=["fs8000-hop37-win97", "shipped"])
def test_a_row_alone_and_in_ragged_batches(gpu_ok, geom, n):
    ext = _ext(*geom)
    fs = geom[0]
    x = torch.from_numpy(_mixed(n, fs, 5))
    F = ext.frame_count(n)
    alone = ext(x)
    assert alone.shape == (1, F, 2 + ext.n_bands)
    assert (alone[0, :, 0] != 0).any() and (alone[0, :, 0] == 0).any()          # voiced and unvoiced frames
    assert (alone[0, :, 2:] < 0).any()
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


@pytest.mark.parametrize("geom,n", [(SMALL, 1500), (SHIPPED, 5000), (HOP600, 4000)], ids=["fs8000-hop37-win97", "shipped", "hop600"])
def test_frame_ranges_and_windows(gpu_ok, geom, n):
    ext = _ext(*geom)
    fs, hop, S, c = geom[0], geom[1], ext.span, (ext.n_taps - 1) // 2
    x = torch.from_numpy(_mixed(n, fs, 9)).to(DEV)
    F = ext.frame_count(n)
    whole = ext(x)[0]
    g = np.random.Generator(np.random.PCG64(11))
    for cuts in ([0, F], [0, 1, F], [0, F - 1, F], [0, F // 2, F // 2, F], sorted({0, F, *[int(v) for v in g.integers(0, F, 5)]})):
        parts = [ext.frames(x, 0, n, n, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        assert torch.equal(torch.cat(parts), whole), cuts
    # windows that hold exactly what a range reads with its halo, in a buffer that is NaN everywhere else
    for a, b in ((0, 1), (F - 1, F), (F // 2, F // 2 + 3), (1, F), (0, F), (F // 3, F // 3 + 1)):
        lo, hi = max(0, a * hop - S // 2 - c), min(n, (b - 1) * hop - S // 2 + S + c)
        buf = torch.full((1, hi - lo + 13), NAN, device=DEV)
        buf[0, :hi - lo] = x[lo:hi]
        got = ext.frames(buf, [lo], [hi - lo], [n], [a], [b])[0]
        assert torch.equal(got, whole[a:b]), (a, b)
        if (b - 1) * hop - S // 2 + S + c <= n:                         # every sample is there: the length need not be known
            assert torch.equal(ext.frames(buf, [lo], [hi - lo], [-1], [a], [b])[0], whole[a:b]), (a, b)
    # one sample less on either side is refused, not read
    a = F // 2
    lo, hi = a * hop - S // 2 - c, a * hop - S // 2 + S + c
    assert 0 < lo and hi < n
    for t0, t1 in ((lo + 1, hi), (lo, hi - 1)):
        with pytest.raises(RuntimeError, match="window"):
            ext.frames(x[t0:t1], t0, t1 - t0, n, a, a + 1)


@pytest.mark.parametrize("chunk", ["1", "7", "hop", "reach", "1000"])
def test_stream_is_bit_identical_to_the_one_shot_call(gpu_ok, chunk):
    ext = _ext(*STREAM)
    n = 2500
    x = torch.from_numpy(_mixed(n, STREAM[0], 21)).to(DEV)
    whole = ext(x)[0]
    size = {"hop": ext.hop, "reach": ext.reach}.get(chunk) or int(chunk)
    st = pitch.BapStream(ext)
    got, k = [], 0
    for at in range(0, n, size):
        out = st.push(x[at:at + size])
        k += out.shape[0]
        assert k == pitch.bap_frames_ready(ext.hop, ext.win, ext.lag_hi, ext.n_taps, min(n, at + size))
        assert st._buf.numel() <= ext.reach + ext.hop + size
        got.append(out)
    last = st.finish()
    assert last.shape[0] == ext.frame_count(n) - k and last.shape[0] > 0
    assert torch.equal(torch.cat(got + [last]), whole)


def test_stream_of_a_signal_shorter_than_a_frame(gpu_ok):
    ext = _ext(*SHIPPED)
    x = torch.from_numpy(R.signal("rich", 700, 22050, seed=3)).to(DEV)
    st = pitch.BapStream(ext)
    assert st.push(x[:300]).shape == (0, 4) and st.push(x[300:]).shape == (0, 4)
    assert torch.equal(st.finish(), ext(x)[0])


def test_zeros_and_the_rows_past_their_frames(gpu_ok):
    ext = _ext(*SHIPPED)
    out = ext(torch.zeros(2, 3000), [3000, 500])
    assert out.shape == (2, 28, 4)
    assert torch.equal(out[0], torch.tensor([0.0, 1.0, 0.0, 0.0], device=out.device).expand(28, 4))
    assert torch.equal(out[1, :5], out[0, :5]) and not out[1, 5:].any()
    # a row without frames in a call with others: its output stays zero
    x = torch.from_numpy(_mixed(3000, 22050, 4))
    two = ext.frames(torch.stack([x, x]), [0, 0], [3000, 3000], [3000, 3000], [0, 7], [28, 7])
    assert torch.equal(two[0], ext(x)[0]) and not two[1].any()
