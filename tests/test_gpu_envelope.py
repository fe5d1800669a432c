"""GPU: the spectral envelope by F0-adaptive smoothing (melspec.SpectralEnvelopeExtractor, swn_envelope) against the float64
reference of tests/envelope_ref.py.  Both outputs are held to the per-entry bound `envelope_ref.tolerance` derives; the worst
share of it per geometry and signal is printed (the README's table).  Then: entries left to the floor are counted (none on the
broadband rows), a row alone against the same row inside a ragged batch, the whole call against `frames()` over a partition from
buffer windows that hold exactly what a range reads, zeros, and the stage-1 driver's `--mcep_envelope`."""
import functools
import os

import numpy as np
import pytest
import torch

import envelope_ref as R
from shallow_wavenet_amd import featio, melspec, pitch
from shallow_wavenet_amd import feature_extract_driver as FD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (signal, F0 track, samples) of the rows of one ragged batch per geometry
ROWS = [("broadband", "voiced", 3001), ("broadband", "unvoiced", 2950), ("broadband", "sweep", 3100), ("broadband", "limits", 2903),
        ("tone", "sweep", 3000), ("half-silence", "sweep", 2977), ("zeros", "voiced", 2800)]


def signal(kind, n, fs, seed):
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros(n, dtype=np.float32)
    if kind == "tone":
        return (0.5 * np.sin(2.0 * np.pi * 0.11 * np.arange(n))).astype(np.float32)
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    if kind == "half-silence":
        x[n // 2:] = 0.0
    return x


def limits(fs, n_fft):
    """fp32 F0 values on both sides of each validity limit, and the values that are not frequencies"""
    lo, hi = np.float32(R.f0_floor(fs, n_fft)), np.float32(fs / 4.0)
    below = lo if np.float64(lo) <= R.f0_floor(fs, n_fft) else np.nextafter(lo, np.float32(0))
    above = np.nextafter(below, np.float32(np.inf))
    while np.float64(above) <= R.f0_floor(fs, n_fft):
        above = np.nextafter(above, np.float32(np.inf))
    return np.array([0.0, np.nan, below, above, hi, np.nextafter(hi, np.float32(np.inf)), -120.0, np.inf, 1e-30, 0.6 * hi],
                    dtype=np.float32)


def track(kind, F, fs, n_fft):
    lim = limits(fs, n_fft)
    if kind == "voiced":
        return np.full(F, min(fs / 4.0, max(2.0 * R.f0_floor(fs, n_fft), 150.0)), dtype=np.float32)
    if kind == "unvoiced":
        return np.zeros(F, dtype=np.float32)
    if kind == "limits":
        return lim[np.arange(F) % lim.size]
    # a sweep from just above f0_floor (the longest window) to fs / 4 (the shortest), another value every frame; at most 48
    # distinct values, so that the reference can evaluate the frames of one value together
    vals = np.geomspace(np.float64(lim[3]), np.float64(lim[4]), min(F, 48)).astype(np.float32)
    vals[0], vals[-1] = lim[3], lim[4]
    return vals[np.arange(F) % vals.size]


@functools.lru_cache(maxsize=None)
def batch(gi):
    """(waves, F0 tracks, references) of geometry gi's ragged batch: computed once, shared, read-only"""
    fs, n_fft, hop, order, alpha = R.GEOMETRIES[gi]
    dG = float(np.abs(melspec.envelope_matrix(n_fft, order, alpha) - R.matrix(n_fft, order, alpha)).max())
    waves, tracks, refs = [], [], []
    for i, (sk, tk, n) in enumerate(ROWS):
        x = signal(sk, n, fs, seed=100 * gi + i)
        f0 = track(tk, R.frame_count(n, hop), fs, n_fft)
        waves.append(x)
        tracks.append(f0)
        refs.append(R.envelope(x, f0, fs, n_fft, hop, order, alpha, dG=dG))
    return waves, tracks, refs


def extractor(gi, output):
    fs, n_fft, hop, order, alpha = R.GEOMETRIES[gi]
    return melspec.SpectralEnvelopeExtractor(fs, n_fft, hop, order, alpha, output=output, device=DEV)


def f0_batch(tracks):
    out = np.zeros((len(tracks), max(t.size for t in tracks)), dtype=np.float32)
    for i, t in enumerate(tracks):
        out[i, :t.size] = t
    return torch.from_numpy(out).to(DEV)


@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=[R.geom_id(g) for g in R.GEOMETRIES])
def test_values_against_the_float64_reference(gpu_ok, gi):
    """checks 1 and 2: every entry of both outputs within the derived bound; the entries the floor decides are counted"""
    waves, tracks, refs = batch(gi)
    hop = R.GEOMETRIES[gi][2]
    got = {o: extractor(gi, o)([torch.from_numpy(w) for w in waves], None, f0_batch(tracks)).cpu().numpy()
           for o in ("mcep", "logamp")}
    worst = 0.0
    for r, (sk, tk, n) in enumerate(ROWS):
        F = R.frame_count(n, hop)
        ref = refs[r]
        shares = {}
        for o, val, tol in (("mcep", "mc", "tol_mc"), ("logamp", "E", "tol_E")):
            out = got[o][r]
            assert np.isfinite(out).all() and not out[F:].any(), (sk, tk, o)
            err = np.abs(out[:F].astype(np.float64) - ref[val])
            with np.errstate(divide="ignore", invalid="ignore"):
                share = np.where(ref[tol] > 0.0, err / ref[tol], np.where(err > 0.0, np.inf, 0.0))
            shares[o] = float(share.max())
        near = int(ref["near_floor"].sum())
        print(f"{R.geom_id(R.GEOMETRIES[gi])} {sk}/{tk}: worst share of the bound mcep {shares['mcep']:.3f} logamp "
              f"{shares['logamp']:.3f}; largest bound mcep {ref['tol_mc'].max():.3g} logamp {ref['tol_E'].max():.3g}; "
              f"entries within dS of the floor {near}")
        if sk == "broadband":
            assert near == 0, (sk, tk, near)
        worst = max(worst, shares["mcep"], shares["logamp"])
        assert shares["mcep"] <= 1.0 and shares["logamp"] <= 1.0, (sk, tk, shares)
    assert worst > 0.0


@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=[R.geom_id(g) for g in R.GEOMETRIES])
def test_lengths_around_a_tile_edge_alone_and_in_a_ragged_batch(gpu_ok, gi):
    """15, 16 and 17 frames: each row against the reference, and alone against the same row inside the ragged batch of 3
    (check 3, first half): torch.equal"""
    fs, n_fft, hop, order, alpha = R.GEOMETRIES[gi]
    lens = [14 * hop + hop // 2, 15 * hop, 16 * hop + (1 if hop > 1 else 0)]
    waves = [signal("broadband", n, fs, seed=7 + i) for i, n in enumerate(lens)]
    tracks = [track("sweep", R.frame_count(n, hop), fs, n_fft) for n in lens]
    assert [t.size for t in tracks] == [15, 16, 17]
    for o, val, tol in (("mcep", "mc", "tol_mc"), ("logamp", "E", "tol_E")):
        ext = extractor(gi, o)
        both = ext([torch.from_numpy(w) for w in waves], None, f0_batch(tracks))
        for r, (w, t) in enumerate(zip(waves, tracks)):
            alone = ext(torch.from_numpy(w), None, torch.from_numpy(t).to(DEV))
            assert tuple(alone.shape) == (1, t.size, ext.cols)
            assert torch.equal(alone[0], both[r, :t.size]) and not both[r, t.size:].any(), (o, r)
            ref = R.envelope(w, t, fs, n_fft, hop, order, alpha)
            assert (np.abs(alone[0].cpu().numpy().astype(np.float64) - ref[val]) <= ref[tol]).all(), (o, r)


@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=[R.geom_id(g) for g in R.GEOMETRIES])
def test_frame_ranges_from_exact_windows(gpu_ok, gi):
    """check 3, second half: the whole call against frames() over a partition into a head, ranges of 1 and 7 frames and the rest,
    each from a buffer that holds exactly the samples the range reads, with t0 > 0 after the head; and two rows with different
    ranges in one call"""
    fs, n_fft, hop, order, alpha = R.GEOMETRIES[gi]
    waves, tracks, _ = batch(gi)
    x, f0 = torch.from_numpy(waves[2]).to(DEV), torch.from_numpy(tracks[2]).to(DEV)
    n, F, half = x.numel(), tracks[2].size, n_fft // 2
    s = -(-half // hop) + 1
    cuts = [0, s, s + 1, s + 8, F]
    assert cuts[-2] < F
    for o in ("mcep", "logamp"):
        ext = extractor(gi, o)
        whole = ext(x, None, f0)[0]
        parts, windows = [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            lo, hi = max(0, a * hop - (half - 1)), min(n - 1, (b - 1) * hop + half - 1)
            windows.append((lo, hi))
            parts.append(ext.frames(x[lo:hi + 1].clone(), lo, hi + 1 - lo, n, a, b, f0[a:b].clone()))
            assert tuple(parts[-1].shape) == (b - a, ext.cols)
        assert all(lo > 0 for lo, _ in windows[1:])
        assert torch.equal(torch.cat(parts), whole), o
        # while the length is unknown, the frames the streaming rule allows from the samples received so far
        got = (cuts[2] - 1) * hop + half
        ready = melspec.envelope_frames_ready(n_fft, hop, got)
        assert ready == cuts[2]
        assert torch.equal(ext.frames(x[:got].clone(), 0, got, -1, 0, ready, f0[:ready].clone()), whole[:ready])
        with pytest.raises(ValueError):
            ext.frames(x[:got].clone(), 0, got, -1, 0, ready + 1, f0[:ready + 1].clone())
        # two rows, two ranges, one call
        x2, f02 = torch.from_numpy(waves[0]).to(DEV), torch.from_numpy(tracks[0]).to(DEV)
        buf = torch.zeros((2, max(n, x2.numel())), device=DEV)
        buf[0, :n], buf[1, :x2.numel()] = x, x2
        fv = torch.zeros((2, 9), device=DEV)
        fv[0, :9], fv[1, :3] = f0[4:13], f02[10:13]
        two = ext.frames(buf, [0, 0], [n, x2.numel()], [n, x2.numel()], [4, 10], [13, 13], fv)
        assert torch.equal(two[0], whole[4:13]) and torch.equal(two[1, :3], ext(x2, None, f02)[0, 10:13]) and not two[1, 3:].any()


def test_zeros_give_the_log_of_the_floor(gpu_ok):
    """check 4: an all-zero signal gives fl32(ln floor) in every bin of every frame, bit for bit, whatever the F0"""
    for gi in (0, 4):
        fs, n_fft, hop, order, alpha = R.GEOMETRIES[gi]
        n = 1500
        F = R.frame_count(n, hop)
        ext = extractor(gi, "logamp")
        for tk in ("voiced", "sweep", "limits"):
            out = ext(torch.zeros(n), None, torch.from_numpy(track(tk, F, fs, n_fft)).to(DEV))[0]
            assert tuple(out.shape) == (F, n_fft // 2 + 1)
            assert torch.equal(out, torch.full_like(out, float(R.log_floor32()))), (gi, tk)
        other = melspec.SpectralEnvelopeExtractor(fs, n_fft, hop, order, alpha, floor=3e-4, output="logamp", device=DEV)
        out = other(torch.zeros(n), None, torch.zeros(F, device=DEV))[0]
        assert torch.equal(out, torch.full_like(out, float(R.log_floor32(3e-4))))


# ---- the stage-1 driver --------------------------------------------------------------------------------------------------------
FS, FFTL, HOP, M = 16000, 512, 80, 12
ARGS = ["--fs", str(FS), "--fftl", str(FFTL), "--hop", str(HOP), "--n_mels", "20", "--verbose", "0", "--minf0", "50", "--maxf0", "600",
        "--f0_win", "512", "--highpass_cutoff", "0", "--mcep_dim", str(M), "--mcep_alpha", "0.41"]


def _write(wavdir):
    from scipy.io import wavfile
    os.makedirs(wavdir, exist_ok=True)
    raw = {}
    for i, (name, n, f0) in enumerate((("utt_a", 4800, 110.0), ("utt_b", 6100, 240.0), ("utt_c", 3777, 0.0))):
        t = np.arange(n, dtype=np.float64)
        x = 0.05 * np.random.default_rng(i).standard_normal(n)
        if f0 > 0.0:
            x += 0.2 * sum(np.cos(2.0 * np.pi * h * f0 * t / FS) / h for h in range(1, 12))
        pcm = np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
        wavfile.write(os.path.join(wavdir, name + ".wav"), FS, pcm)
        raw[name] = torch.from_numpy((pcm.astype(np.float64) / 32768.0).astype(np.float32))     # what the driver reads
    return raw


def test_driver_writes_the_envelope_cepstra_at_the_f0_of_the_batch(gpu_ok, tmp_path):
    """check 5: with --mcep_envelope true /feat_mcep is the extractor's output at F0Extractor's column 0, and /feat_f0 is written
    only when asked; without the flag the dataset is MelCepstrumExtractor's, as before"""
    raw = _write(str(tmp_path / "wav"))
    on, off, both = str(tmp_path / "h5_on"), str(tmp_path / "h5_off"), str(tmp_path / "h5_both")
    base = ARGS + ["--waveforms", str(tmp_path / "wav")]
    assert FD.main(base + ["--hdf5dir", on, "--mcep_envelope", "true"]) == 0
    assert FD.main(base + ["--hdf5dir", off]) == 0
    assert FD.main(base + ["--hdf5dir", both, "--mcep_envelope", "true", "--f0", "true", "--feature_type", "mcep"]) == 0
    f0_ext = pitch.F0Extractor(FS, HOP, 50, 600, 512, device=DEV)
    env = melspec.SpectralEnvelopeExtractor(FS, FFTL, HOP, M, 0.41, device=DEV)
    old = melspec.MelCepstrumExtractor(FS, FFTL, HOP, M, 0.41, device=DEV)
    voiced = 0
    for name, x in raw.items():
        F = 1 + x.numel() // HOP
        f0 = f0_ext(x)
        want = env(x, None, f0[..., 0].contiguous())[0].cpu().numpy()
        a = featio.read_dataset(FD.feature_path(on, name + ".wav"), "/feat_mcep")
        assert a.dtype == np.float32 and a.shape == (F, M + 1) and np.array_equal(a, want), name
        assert not featio.check_dataset(FD.feature_path(on, name + ".wav"), "/feat_f0")
        assert np.array_equal(featio.read_dataset(FD.feature_path(on, name + ".wav"), "/feat_logmel"),
                              featio.read_dataset(FD.feature_path(off, name + ".wav"), "/feat_logmel"))
        b = featio.read_dataset(FD.feature_path(off, name + ".wav"), "/feat_mcep")
        assert np.array_equal(b, old(x)[0].cpu().numpy()) and not np.array_equal(a, b), name
        c = FD.feature_path(both, name + ".wav")
        assert np.array_equal(featio.read_dataset(c, "/feat_mcep"), want)
        assert np.array_equal(featio.read_dataset(c, "/feat_f0"), f0[0].cpu().numpy())
        voiced += int((f0[0, :, 0] > 0).sum())
    assert voiced > 20                                      # the envelope really ran at measured pitches
