"""GPU: the mel-cepstrum operator (csrc/swn_melspec.hip mcep_kernel, melspec.MelCepstrumExtractor, torch.ops.swn.mcep) against
the float64 yardstick of tests/mcep_ref.py, its exact properties, and the loop it closes (wav files -> /feat_mcep ->
statistics -> the device post-filter).

Shapes: (fs, n_fft, hop, order, alpha) from mcep_ref.GEOMETRIES - fewer coefficients than one 16-coefficient column tile; 49
bins, K padded to 52; exactly one tile with hop 1; one coefficient into the second tile; run.sh's; both maxima, where L reuses
the LDS of the frame image - at the lengths of melspec_ref.lengths (n_fft / 2 + 1, F one below, on and one above the 16-frame
tile, about 3 000 samples); one row alone and three rows of ragged lengths; broadband, pure tone, half silence, all zeros.

Bound per entry (mcep_ref.tolerance; derived, not taken from what the kernel gives).  With A the float64 amplitudes, top the
row's largest, e32 the distance of their fp32 numpy evaluation relative to top and B = max(4 e32, 1e-6) top (the linear bound
of test_gpu_melspec.py):
    dL[b]  = ln max(a + B, floor) - ln max(a - B, floor)
    tol[m] = sum_b |G[m][b]| (dL[b] + 2^-23 |L[b]|) + (bins + 2) 2^-24 sum_b |G[m][b]| |L[b]|
All-zero input: every coefficient equals, exactly, the fp32 fused-multiply-add chain of fl32(ln floor) over its row of the
fp32 G in ascending bins (mcep_ref.fma_chain).  The figures are printed before each assertion (pytest -s).

Measured on an MI355X: see the table in README.md (worst share of the bound, worst absolute error and e32 per geometry and
signal)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import mcep_ref as MC
import melspec_ref as MR
from shallow_wavenet_amd import _lib, dsp, featio, melspec
from shallow_wavenet_amd import feature_extract_driver as FD
from shallow_wavenet_amd.postfilter import NoiseShapingRestorer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOM_IDS = [MC.geom_id(g) for g in MC.GEOMETRIES]


@functools.lru_cache(maxsize=None)
def _ext(geom, floor=MC.FLOOR):
    fs, n_fft, hop, order, alpha = geom
    return melspec.MelCepstrumExtractor(fs, n_fft, hop, order, alpha, floor=floor, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(geom, kind, length):
    """(x fp32, ref64 (F, order + 1), tol (F, order + 1), e32 of the amplitudes) - computed once, shared, never written to"""
    fs, n_fft, hop, order, alpha = geom
    x = MR.signal(kind, length, fs, seed=length + n_fft)
    tol, e32, _ = MC.tolerance(x, n_fft, hop, order, alpha)
    return x, MC.mcep(x, n_fft, hop, order, alpha), tol, e32


def _g32(ext):
    """the fp32 G the operator multiplies with, (order + 1, bins), from the extractor's own table"""
    bins = ext.n_fft // 2 + 1
    return ext._table.cpu().numpy()[2 * ext.n_fft:].reshape(ext.order + 1, -1)[:, :bins]


def _zeros_row(ext):
    return MC.fma_chain(np.full(ext.n_fft // 2 + 1, MC.log_floor32(ext.floor), dtype=np.float32), _g32(ext))


def _check_values(tag, kind, got, ref, tol, e32, ext):
    got32 = got.cpu().numpy()
    got = got32.astype(np.float64)
    assert got.shape == ref.shape == tol.shape, (tag, got.shape, ref.shape)
    err = np.abs(got - ref)
    share = float((err / tol).max())
    print(f"{tag}: worst share of the bound {share:.3f}, worst error {err.max():.2e}, smallest bound {tol.min():.2e}, "
          f"largest bound {tol.max():.2e}, e32 of the amplitudes {e32:.2e}, largest |mc| {np.abs(ref).max():.2f}")
    assert np.isfinite(got).all()
    assert (err <= tol).all(), (tag, share)
    if kind == "zeros":
        want = _zeros_row(ext)
        assert np.array_equal(got32, np.broadcast_to(want, got32.shape)), tag
        assert abs(float(want[0]) - float(MC.log_floor32(ext.floor))) <= 1e-5 and np.abs(want[1:]).max(initial=0.0) <= 1e-5


@pytest.mark.parametrize("kind", MR.KINDS)
@pytest.mark.parametrize("geom", MC.GEOMETRIES, ids=GEOM_IDS)
def test_values_one_row_and_ragged_batches(gpu_ok, geom, kind):
    fs, n_fft, hop, order, alpha = geom
    ext = _ext(geom)
    lens = MR.lengths(n_fft, hop)
    gid = MC.geom_id(geom)
    alone = {}
    for L in lens:
        x, ref, tol, e32 = _case(geom, kind, L)
        got = ext(torch.from_numpy(x))
        assert got.shape == (1, MR.frame_count(L, hop), order + 1) and got.dtype == torch.float32
        _check_values(f"{gid} {kind} len {L} alone", kind, got[0], ref, tol, e32, ext)
        alone[L] = got[0]
    # three rows of ragged lengths: as a list, and as a padded batch whose padding is NaN (never read); every row equals the
    # row alone bit for bit
    for trio in (lens[:3], lens[-3:][::-1]):
        rows = [torch.from_numpy(_case(geom, kind, L)[0]) for L in trio]
        padded = torch.full((3, max(trio) + 5), float("nan"))
        for i, r in enumerate(rows):
            padded[i, :trio[i]] = r
        got = ext(rows)
        assert got.shape == (3, max(MR.frame_count(L, hop) for L in trio), order + 1)
        assert torch.equal(got, ext(padded, lengths=trio))
        for i, L in enumerate(trio):
            F = MR.frame_count(L, hop)
            assert torch.equal(got[i, :F], alone[L]), (geom, kind, trio, i)
            assert not got[i, F:].any()
        x, ref, tol, e32 = _case(geom, kind, trio[1])
        _check_values(f"{gid} {kind} len {trio[1]} in a batch", kind, got[1, :ref.shape[0]], ref, tol, e32, ext)


def _long(geom, kind="broadband"):
    n_fft, hop = geom[1], geom[2]
    L = MR.lengths(n_fft, hop)[-1]                           # 3 001 samples; 17 frames of the 2 048-point transform
    return L, torch.from_numpy(_case(geom, kind, L)[0]).to(DEV)


@pytest.mark.parametrize("geom", MC.GEOMETRIES, ids=GEOM_IDS)
def test_any_partition_of_the_frames_equals_the_one_shot_call(gpu_ok, geom):
    fs, n_fft, hop, order, alpha = geom
    ext = _ext(geom)
    L, x = _long(geom)
    F = MR.frame_count(L, hop)
    whole = ext(x)[0]
    assert whole.shape == (F, order + 1)
    # ranges that cross the 16-frame tile boundaries, and ranges of 7
    for cuts in ([0, F], [0, 1, F], sorted({0, 1, 5, 16, 17, 33, F - 1, F} & set(range(F + 1))), list(range(0, F, 7)) + [F]):
        parts = [ext.frames(x, 0, L, L, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        assert torch.equal(torch.cat(parts), whole), (geom, cuts)
    # single frames: as calls of their own and as the rows of one call
    singles = sorted({0, 1, 15, 16, 17, F // 2, F - 2, F - 1} & set(range(F)))
    for f in singles:
        assert torch.equal(ext.frames(x, 0, L, L, f, f + 1)[0], whole[f]), (geom, f)
    got = ext.frames(x[None].expand(len(singles), L).contiguous(), 0, L, L, singles, [f + 1 for f in singles])
    assert got.shape == (len(singles), 1, order + 1) and torch.equal(got[:, 0], whole[singles])
    # several ranges of one signal as the rows of one call
    cuts = [0, F // 3, F // 3, F]
    got = ext.frames(x[None].expand(3, L).contiguous(), 0, L, L, cuts[:3], cuts[1:])
    assert torch.equal(torch.cat([got[i, :cuts[i + 1] - cuts[i]] for i in range(3)]), whole)


@pytest.mark.parametrize("geom", MC.GEOMETRIES, ids=GEOM_IDS)
def test_explicit_windows_with_unknown_length_and_nan_around_them(gpu_ok, geom):
    """frames from a window [t0, t0 + n_avail) of the signal, total length -1, equal the same frames of the whole signal; NaN
    before the window, after it and past the signal changes nothing"""
    fs, n_fft, hop, order, alpha = geom
    ext = _ext(geom)
    L, x = _long(geom)
    F = MR.frame_count(L, hop)
    whole = ext(x)[0]
    assert torch.isfinite(whole).all()
    inner = [f for f in range(F) if f * hop - n_fft // 2 >= 1 and f * hop + n_fft // 2 <= L - 1]
    if inner:
        f0, f1 = inner[0], inner[-1] + 1
        if f1 - f0 > 20:
            f0, f1 = f0 + 3, f0 + 3 + 18                    # across a tile boundary, away from the ends
        t0, t1 = f0 * hop - n_fft // 2, (f1 - 1) * hop + n_fft // 2
        big = torch.full((L + 64,), float("nan"), device=DEV)
        big[32 + t0:32 + t1] = x[t0:t1]
        assert torch.equal(ext.frames(big[32 + t0:], t0, t1 - t0, -1, f0, f1), whole[f0:f1]), (geom, f0, f1)
        assert torch.equal(ext.frames(big[32 + t0:], t0, t1 - t0, L, f0, f1), whole[f0:f1])
    # the last frames read the reflected end: a window from their first sample on, NaN before it and after the signal
    f0 = max(0, F - 3)
    t0 = max(0, min(f0 * hop - n_fft // 2, 2 * (L - 1) - ((F - 1) * hop + n_fft // 2 - 1)))
    big = torch.full((L + 64,), float("nan"), device=DEV)
    big[32 + t0:32 + L] = x[t0:]
    assert torch.equal(ext.frames(big[32 + t0:], t0, L - t0, L, f0, F), whole[f0:])
    # the first two frames read the reflected start: a window that ends with the last sample of frame 1, length unknown
    t1 = hop + n_fft // 2
    assert F >= 2 and t1 <= L
    big = torch.full((L + 64,), float("nan"), device=DEV)
    big[32:32 + t1] = x[:t1]
    assert torch.equal(ext.frames(big[32:], 0, t1, -1, 0, 2), whole[:2])


@pytest.mark.parametrize("geom", MC.GEOMETRIES, ids=GEOM_IDS)
def test_a_row_has_the_same_bits_alone_in_3_rows_and_in_65_rows(gpu_ok, geom):
    fs, n_fft, hop, order, alpha = geom
    ext = _ext(geom)
    base = n_fft // 2 + 1 + 16 * hop                         # more than one tile of frames
    x = torch.from_numpy(MR.signal("broadband", base + 80, fs, seed=11))
    rows = [x[i:i + base - (i % 5)] for i in range(65)]       # 65 rows > 64 entries of a launch
    got65 = ext(rows)
    got3 = ext([rows[64], rows[1], rows[63]])
    for i, j in ((64, 0), (1, 1), (63, 2)):
        F = MR.frame_count(rows[i].numel(), hop)
        solo = ext(rows[i])[0]
        assert solo.shape == (F, order + 1) and F > 16
        assert torch.equal(got65[i, :F], solo) and torch.equal(got3[j, :F], solo), (geom, i)
        assert not got65[i, F:].any() and not got3[j, F:].any()
    assert torch.equal(got65[0, :MR.frame_count(rows[0].numel(), hop)], ext(rows[0])[0])


def test_order_edges(gpu_ok):
    fs, n_fft, hop = 8000, 32, 8
    x = MR.signal("broadband", 301, fs, seed=5)
    A = MC.amplitudes(x, n_fft, hop)
    # order 0: one coefficient, the chain of G's only row - with alpha 0 the mean log amplitude over the full spectrum
    for alpha in (0.0, 0.31):
        ext = melspec.MelCepstrumExtractor(fs, n_fft, hop, 0, alpha, device=DEV)
        got = ext(torch.from_numpy(x))[0]
        tol, e32, _ = MC.tolerance(x, n_fft, hop, 0, alpha)
        ref = MC.mcep(x, n_fft, hop, 0, alpha)
        assert got.shape == ref.shape == (38, 1)
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        print(f"order 0 alpha {alpha}: worst share of the bound {(err / tol).max():.3f}, worst error {err.max():.2e}")
        assert (err <= tol).all()
        if alpha == 0.0:
            Lg = np.log(np.maximum(A, np.float64(np.float32(MC.FLOOR))))
            mean = (Lg[:, 0] + Lg[:, -1] + 2.0 * Lg[:, 1:-1].sum(axis=1)) / n_fft
            assert np.abs(ref[:, 0] - mean).max() <= 1e-13
        zero = ext(torch.zeros(301))[0].cpu().numpy()
        assert np.array_equal(zero, np.broadcast_to(_zeros_row(ext), zero.shape))
    # order n_fft / 2: every coefficient of the one-sided cepstrum is kept
    ext = melspec.MelCepstrumExtractor(fs, n_fft, hop, n_fft // 2, 0.31, device=DEV)
    got = ext(torch.from_numpy(x))[0]
    tol, e32, _ = MC.tolerance(x, n_fft, hop, n_fft // 2, 0.31)
    err = np.abs(got.cpu().numpy().astype(np.float64) - MC.mcep(x, n_fft, hop, n_fft // 2, 0.31))
    print(f"order n_fft / 2: worst share of the bound {(err / tol).max():.3f}, worst error {err.max():.2e}")
    assert got.shape == (38, 17) and (err <= tol).all()


def test_refused_calls_leave_the_output_untouched(gpu_ok):
    lib = _lib.lib()
    n_fft, hop, L = 32, 8, 301
    wav = torch.from_numpy(MR.signal("broadband", L, 8000, seed=5)).to(DEV)
    F = MR.frame_count(L, hop)
    out = torch.full((F, 80), -7.25, device=DEV)
    work = torch.zeros(3 * 16 * 20, device=DEV)
    tables = torch.from_numpy(melspec.mcep_tables(n_fft, 16, 0.31)).to(DEV)
    entry = (_lib.LogMelEntry * 1)(_lib.LogMelEntry(wav_dev=wav.data_ptr(), out_dev=out.data_ptr(), t0=0, n_avail=L, len=L, f0=0,
                                                     f1=F, reserved=0))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.swn_mcep_work_bytes(n_fft, hop, entry, 1) == work.numel() * 4
    for order, floor, text in ((64, 1e-5, "order outside"), (17, 1e-5, "n_fft / 2"), (-1, 1e-5, "order outside"), (16, 0.0, "floor")):
        assert lib.swn_mcep(n_fft, hop, order, floor, p(tables), entry, 1, p(work), stream) == -2
        assert text in lib.swn_last_error_detail().decode()
        torch.cuda.synchronize()
        assert bool((out == -7.25).all()), (order, floor)
    for kw in (dict(order=64), dict(order=17), dict(floor=0.0)):
        args = dict(fs=8000, n_fft=n_fft, hop=hop, order=16, alpha=0.31, floor=1e-5, device=DEV)
        args.update(kw)
        with pytest.raises(ValueError):
            melspec.MelCepstrumExtractor(**args)
    with pytest.raises(RuntimeError, match="order 64"):
        torch.ops.swn.mcep(wav[None], tables, [0], [L], [L], [0], [F], n_fft, hop, 64, 1e-5)
    # the same call with arguments it accepts writes its 17 columns and nothing else
    assert lib.swn_mcep(n_fft, hop, 16, 1e-5, p(tables), entry, 1, p(work), stream) == 0
    torch.cuda.synchronize()
    want = melspec.MelCepstrumExtractor(8000, n_fft, hop, 16, 0.31, device=DEV)(wav)[0]
    assert torch.equal(out.view(-1)[:F * 17].view(F, 17), want) and bool((out.view(-1)[F * 17:] == -7.25).all())


@pytest.mark.parametrize("gi", [1, 4, 5], ids=[GEOM_IDS[i] for i in (1, 4, 5)])
def test_logmel_is_unchanged_by_interleaved_mcep_calls(gpu_ok, gi):
    """no shared state: the log-mel output after mel-cepstrum calls on the same stream has the bits it had before them"""
    geom = MC.GEOMETRIES[gi]
    fs, n_fft, hop, order, alpha = geom
    n_mels = {96: 8, 1024: 80, 2048: 128}[n_fft]
    lm, mc = melspec.LogMelExtractor(fs, n_fft, hop, n_mels, floor=MR.FLOOR, device=DEV), _ext(geom)
    L, x = _long(geom)
    before, before_lin, mc_before = lm(x), lm(x, linear=True), mc(x)
    for _ in range(2):
        got_mc = mc(x)
        part = mc.frames(x, 0, L, L, 1, min(19, MR.frame_count(L, hop)))
        assert torch.equal(lm(x), before) and torch.equal(got_mc, mc_before)
        assert torch.equal(part, mc_before[0, 1:min(19, MR.frame_count(L, hop))])
        assert torch.equal(lm(x, linear=True), before_lin)
    torch.cuda.synchronize()
    assert torch.equal(lm(x), before)


def test_driver_writes_both_datasets_and_the_statistics_drive_the_post_filter(gpu_ok, tmp_path):
    from scipy.io import wavfile
    fs, order, alpha = 16000, 12, 0.41
    waves = {"utt_a": MR.signal("broadband", 2400, fs, seed=1), "utt_b": MR.signal("tone", 1777, fs, seed=2)}
    wavdir = tmp_path / "wav"
    os.makedirs(wavdir)
    for name, x in waves.items():
        wavfile.write(str(wavdir / (name + ".wav")), fs, np.round(x * 32767.0).astype(np.int16))
    h5 = tmp_path / "hdf5"
    argv = ["--waveforms", str(wavdir), "--hdf5dir", str(h5), "--fs", str(fs), "--fftl", "512", "--n_mels", "40", "--verbose", "0",
            "--highpass_cutoff", "0", "--mcep_alpha", str(alpha)]
    assert FD.main(argv + ["--mcep_dim", str(order)]) == 0
    ext = melspec.MelCepstrumExtractor(fs, 512, 80, order, alpha, device=DEV)
    lm = melspec.LogMelExtractor(fs, 512, 80, 40, device=DEV)
    files = []
    for name, x in waves.items():
        path = FD.feature_path(str(h5), name + ".wav")
        files.append(path)
        pcm = (np.round(x * 32767.0).astype(np.int16).astype(np.float64) / 32768.0).astype(np.float32)     # what read_wav returns
        mc, mel = featio.read_dataset(path, "/feat_mcep"), featio.read_dataset(path, "/feat_logmel")
        assert mc.shape == (1 + x.shape[0] // 80, order + 1) and mel.shape == (mc.shape[0], 40) and mc.dtype == np.float32
        assert np.array_equal(mc, ext(torch.from_numpy(pcm))[0].cpu().numpy())
        assert np.array_equal(mel, lm(torch.from_numpy(pcm))[0].cpu().numpy())
    # --feature_type mcep: the mel-cepstra are the conditioning dataset, and nothing else is written
    h5c = tmp_path / "hdf5_mcep"
    argv_c = [a if a != str(h5) else str(h5c) for a in argv] + ["--feature_type", "mcep", "--mcep_dim", str(order)]
    assert FD.main(argv_c + ["--string_path", "/feat_cond"]) == 0
    for name in waves:
        path = FD.feature_path(str(h5c), name + ".wav")
        assert np.array_equal(featio.read_dataset(path, "/feat_cond"),
                              featio.read_dataset(FD.feature_path(str(h5), name + ".wav"), "/feat_mcep"))
        assert not featio.check_dataset(path, "/feat_logmel") and not featio.check_dataset(path, "/feat_mcep")
    assert FD.main([a if a != str(h5) else str(tmp_path / "none") for a in argv] + ["--feature_type", "mcep"]) == 2
    # calc_stats of the second dataset -> the device post-filter at mcep_dim_start 0, against the host filter
    from shallow_wavenet_amd.noise_shaping_driver import mean_mcep_vector
    mean, scale = featio.calc_stats(files, "/feat_mcep")
    stats = str(tmp_path / "stats.npz")
    featio.write_stats(stats, "/feat_mcep", mean, scale)
    mean = mean_mcep_vector(stats, "/feat_mcep")
    assert mean.shape == (order + 1,) and np.isfinite(mean).all() and np.abs(mean[1:]).max() > 0.05
    y = torch.from_numpy(MR.signal("broadband", 4000, fs, seed=3))
    r = NoiseShapingRestorer(mean, fs, alpha, mcep_dim_start=0, device=DEV)
    got = r.restore([y.to(DEV)])[0].cpu().numpy().astype(np.float64)
    want = dsp.noise_shaping(y.numpy().astype(np.float64), mean, fs, alpha, mcep_dim_start=0, inv=False)
    err = float(np.abs(got - want).max())
    print(f"post-filter from /feat_mcep statistics: |device - host| {err:.2e}, largest output {np.abs(want).max():.2f}")
    assert err <= 1e-6 and np.abs(want - y.numpy()).max() > 1e-2
