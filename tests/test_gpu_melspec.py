"""GPU: the log-mel operator (csrc/swn_melspec.hip, melspec.LogMelExtractor / LogMelStream) against the float64 yardstick of
tests/melspec_ref.py, its exact properties, and the two loops it closes (audio -> mel -> vocoder, wav files -> feature files).

Shapes: (fs, n_fft, hop, n_mels) from melspec_ref.GEOMETRIES - the smallest transform, a hop that does not divide n_fft, the
16 kHz and 22.05 kHz recipes, the largest transform with hop = n_fft and 128 filters, and hop 1 - at the lengths of
melspec_ref.lengths: n_fft / 2 + 1, F one below, on and one above the kernel's 16-frame tile, and about 3 000 samples; one
row alone and three rows of ragged lengths; broadband, pure tone, half silence, all zeros.

Bounds (set by the issue, not by what the kernel gives).  With ref64 the yardstick in float64 and e32 the distance of its fp32
numpy evaluation from it, relative to the row's largest float64 value:
    linear   |got - ref64| <= B = max(4 e32, 1e-6) x the row's largest float64 value   (the rule of test_gpu_spectral_loss.py)
    log      |got - ln a| <= 1.01 B / a + 1e-6 max(1, |ln a|), a = max(ref64, floor), wherever B / a <= 1e-2: the linear bound
             propagated to first order plus the fp32 rounding of the log.  Entries with B / a > 1e-2 (amplitudes within 100 B
             of nothing) are left to the linear check; on the broadband signals there must be none.
    zeros    exactly 0, and float32(log(floor)) to 1e-6.
The figures are printed before each assertion (pytest -s).

Measured on an MI355X, worst over the lengths, one row alone and inside the ragged batches:
    geometry                     signal        linear: worst error (largest e32, smallest bound)   log: worst share of its bound   left to the linear check
    fs8000-n32-hop8-m4           broadband       2.0e-07 (2.2e-07, 1.0e-06)                        0.11                                 0 / 1836
    fs8000-n32-hop8-m4           tone            1.8e-07 (2.7e-07, 1.0e-06)                        0.07                                 0 / 1824
    fs8000-n32-hop8-m4           half-silence    1.3e-07 (2.0e-07, 1.0e-06)                        0.07                               872 / 1824
    fs8000-n32-hop8-m4           zeros           exactly 0                                            |log - ln floor| 0.0e+00
    fs8000-n96-hop37-m8          broadband       2.2e-07 (2.6e-07, 1.0e-06)                        0.09                                 0 / 1296
    fs8000-n96-hop37-m8          tone            1.5e-07 (1.8e-07, 1.0e-06)                        0.08                               143 / 1296
    fs8000-n96-hop37-m8          half-silence    1.8e-07 (1.5e-07, 1.0e-06)                        0.10                               584 / 1296
    fs8000-n96-hop37-m8          zeros           exactly 0                                            |log - ln floor| 0.0e+00
    fs16000-n512-hop80-m40       broadband       4.1e-07 (3.0e-07, 1.0e-06)                        0.10                                 0 / 4720
    fs16000-n512-hop80-m40       tone            2.0e-07 (1.9e-07, 1.0e-06)                        0.07                              2660 / 4720
    fs16000-n512-hop80-m40       half-silence    2.8e-07 (1.9e-07, 1.0e-06)                        0.11                              1720 / 4720
    fs16000-n512-hop80-m40       zeros           exactly 0                                            |log - ln floor| 0.0e+00
    fs22050-n1024-hop110-m80     broadband       3.9e-07 (3.5e-07, 1.0e-06)                        0.13                                 0 / 8640
    fs22050-n1024-hop110-m80     tone            6.1e-07 (3.1e-07, 1.0e-06)                        0.14                              3935 / 8640
    fs22050-n1024-hop110-m80     half-silence    3.4e-07 (2.8e-07, 1.0e-06)                        0.11                              2268 / 8640
    fs22050-n1024-hop110-m80     zeros           exactly 0                                            |log - ln floor| 0.0e+00
    fs22050-n2048-hop2048-m128   broadband       5.8e-07 (2.5e-07, 1.0e-06)                        0.14                                 0 / 8704
    fs22050-n2048-hop2048-m128   tone            4.9e-07 (2.7e-07, 1.0e-06)                        0.08                              7428 / 8704
    fs22050-n2048-hop2048-m128   half-silence    3.2e-07 (2.6e-07, 1.0e-06)                        0.11                              4224 / 8704
    fs22050-n2048-hop2048-m128   zeros           exactly 0                                            |log - ln floor| 0.0e+00
    fs8000-n64-hop1-m8           broadband       2.7e-07 (3.1e-07, 1.0e-06)                        0.14                                 0 / 25936
    fs8000-n64-hop1-m8           tone            2.0e-07 (2.7e-07, 1.0e-06)                        0.09                              2939 / 25936
    fs8000-n64-hop1-m8           half-silence    2.1e-07 (2.7e-07, 1.0e-06)                        0.10                             11752 / 25936
    fs8000-n64-hop1-m8           zeros           exactly 0                                            |log - ln floor| 0.0e+00
Every exact property held bit for bit.  The slowest case is the copy-synthesis loop (1.6 s).
"""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

import melspec_ref as MR
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import feature_extract_driver as FD
from shallow_wavenet_amd import featio, melspec
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodeStream
from shallow_wavenet_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOM_IDS = [f"fs{fs}-n{n}-hop{hop}-m{m}" for fs, n, hop, m in MR.GEOMETRIES]


@functools.lru_cache(maxsize=None)
def _ext(geom):
    fs, n_fft, hop, n_mels = geom
    return melspec.LogMelExtractor(fs, n_fft, hop, n_mels, floor=MR.FLOOR, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(geom, kind, length):
    """(x fp32, ref64 (F, n_mels), e32) - computed once, shared, never written to"""
    fs, n_fft, hop, n_mels = geom
    x = MR.signal(kind, length, fs, seed=length + n_fft)
    ref = MR.mel(x, fs, n_fft, hop, n_mels)
    r32 = MR.mel(x, fs, n_fft, hop, n_mels, dtype=np.float32)
    top = ref.max()
    e32 = float(np.abs(r32 - ref).max() / top) if top > 0 else 0.0
    return x, ref, e32


def _check_values(tag, kind, lin, log, ref, e32):
    lin, log = lin.double().cpu().numpy(), log.double().cpu().numpy()
    assert lin.shape == log.shape == ref.shape, (tag, lin.shape, ref.shape)
    top = ref.max()
    B = max(4 * e32, 1e-6) * top
    err = np.abs(lin - ref).max()
    a = np.maximum(ref, MR.FLOOR)
    if kind == "zeros":
        print(f"{tag}: zeros, linear max {np.abs(lin).max():.1e}, log - ln floor {np.abs(log - np.float32(np.log(MR.FLOOR))).max():.1e}")
        assert top == 0.0 and not lin.any()
        assert np.abs(log - np.float64(np.float32(np.log(MR.FLOOR)))).max() <= 1e-6
        return
    checked = B / a <= 1e-2
    lerr = np.abs(log - np.log(a))
    lbound = 1.01 * B / a + 1e-6 * np.maximum(1.0, np.abs(np.log(a)))
    worst = float((lerr[checked] / lbound[checked]).max()) if checked.any() else 0.0
    print(f"{tag}: linear {err / top:.2e} of the largest value (e32 {e32:.2e}, bound {B / top:.2e}); log: worst share of its "
          f"bound {worst:.2f}, {int((~checked).sum())} of {checked.size} entries left to the linear check")
    assert np.isfinite(lin).all() and np.isfinite(log).all()
    assert err <= B, (tag, err / top, e32)
    assert (lerr[checked] <= lbound[checked]).all(), (tag, worst)
    if kind == "broadband":
        assert checked.all(), tag


@pytest.mark.parametrize("kind", MR.KINDS)
@pytest.mark.parametrize("geom", MR.GEOMETRIES, ids=GEOM_IDS)
def test_values_one_row_and_ragged_batches(gpu_ok, geom, kind):
    fs, n_fft, hop, n_mels = geom
    ext = _ext(geom)
    lens = MR.lengths(n_fft, hop)
    alone = {}
    for L in lens:
        x, ref, e32 = _case(geom, kind, L)
        lin, log = ext(torch.from_numpy(x), linear=True), ext(torch.from_numpy(x))
        assert lin.shape == (1, MR.frame_count(L, hop), n_mels)
        _check_values(f"{GEOM_IDS[MR.GEOMETRIES.index(geom)]} {kind} len {L} alone", kind, lin[0], log[0], ref, e32)
        alone[L] = (lin[0], log[0])
    # three rows of ragged lengths: as a list, and as a padded batch whose padding is NaN (never read); every row equals the
    # row alone bit for bit
    for trio in (lens[:3], lens[-3:][::-1]):
        rows = [torch.from_numpy(_case(geom, kind, L)[0]) for L in trio]
        padded = torch.full((3, max(trio) + 5), float("nan"))
        for i, r in enumerate(rows):
            padded[i, :trio[i]] = r
        for linear in (True, False):
            got = ext(rows, linear=linear)
            got_p = ext(padded, lengths=trio, linear=linear)
            assert got.shape == (3, max(MR.frame_count(L, hop) for L in trio), n_mels) and torch.equal(got, got_p)
            for i, L in enumerate(trio):
                F = MR.frame_count(L, hop)
                assert torch.equal(got[i, :F], alone[L][0 if linear else 1]), (geom, kind, trio, i)
                assert not got[i, F:].any()
        x, ref, e32 = _case(geom, kind, trio[1])
        _check_values(f"{GEOM_IDS[MR.GEOMETRIES.index(geom)]} {kind} len {trio[1]} in a batch", kind,
                      ext(rows, linear=True)[1, :ref.shape[0]], ext(rows)[1, :ref.shape[0]], ref, e32)


def _long(geom, kind="broadband"):
    n_fft, hop = geom[1], geom[2]
    L = MR.lengths(n_fft, hop)[-1]                           # 3 001 samples; 17 frames of the 2 048-point transform
    return L, torch.from_numpy(_case(geom, kind, L)[0]).to(DEV)


@pytest.mark.parametrize("geom", MR.GEOMETRIES, ids=GEOM_IDS)
def test_any_partition_of_the_frames_equals_the_one_shot_call(gpu_ok, geom):
    fs, n_fft, hop, n_mels = geom
    ext = _ext(geom)
    L, x = _long(geom)
    F = MR.frame_count(L, hop)
    for linear in (False, True):
        whole = ext(x, linear=linear)[0]
        for cuts in ([0, F], [0, 1, F], sorted({0, 1, 5, 16, 17, 33, F - 1, F} & set(range(F + 1))), list(range(0, F, 7)) + [F]):
            parts = [ext.frames(x, 0, L, L, a, b, linear) for a, b in zip(cuts[:-1], cuts[1:])]
            assert torch.equal(torch.cat(parts), whole), (geom, cuts)
    # several ranges of one signal as the rows of one call
    cuts = [0, F // 3, F // 3, F]
    got = ext.frames(x[None].expand(3, L).contiguous(), 0, L, L, cuts[:3], cuts[1:])
    whole = ext(x)[0]
    assert torch.equal(torch.cat([got[i, :cuts[i + 1] - cuts[i]] for i in range(3)]), whole)


@pytest.mark.parametrize("geom", MR.GEOMETRIES, ids=GEOM_IDS)
def test_partial_window_with_unknown_length_and_nan_around_it(gpu_ok, geom):
    """frames from a window [t0, t0 + n_avail) of the signal, total length unknown, equal the same frames of the whole signal;
    NaN before the window, after it and past each row's length changes nothing"""
    fs, n_fft, hop, n_mels = geom
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
        got = ext.frames(big[32 + t0:], t0, t1 - t0, -1, f0, f1)
        assert torch.equal(got, whole[f0:f1]), (geom, f0, f1)
        # the same window with the length known
        assert torch.equal(ext.frames(big[32 + t0:], t0, t1 - t0, L, f0, f1), whole[f0:f1])
    # the last frames read the reflected end: a window from their first sample on, NaN before it and after the signal
    f0 = max(0, F - 3)
    t0 = max(0, min(f0 * hop - n_fft // 2, 2 * (L - 1) - ((F - 1) * hop + n_fft // 2 - 1)))
    big = torch.full((L + 64,), float("nan"), device=DEV)
    big[32 + t0:32 + L] = x[t0:]
    assert torch.equal(ext.frames(big[32 + t0:], t0, L - t0, L, f0, F), whole[f0:])
    # the first two frames read the reflected start: a window that ends with the last sample of frame 1
    t1 = hop + n_fft // 2
    assert F >= 2 and t1 <= L
    big = torch.full((L + 64,), float("nan"), device=DEV)
    big[32:32 + t1] = x[:t1]
    assert torch.equal(ext.frames(big[32:], 0, t1, -1, 0, 2), whole[:2])


@pytest.mark.parametrize("chunk", [1, 37, 160, 1103])
@pytest.mark.parametrize("geom", MR.GEOMETRIES, ids=GEOM_IDS)
def test_stream_in_chunks_equals_the_one_shot_call(gpu_ok, geom, chunk):
    fs, n_fft, hop, n_mels = geom
    ext = _ext(geom)
    L, x = _long(geom)
    if chunk == 1:
        L = min(L, max(n_fft // 2 + 1 + 3 * hop, 700))      # sample by sample: a shorter signal, still several frames
        x = x[:L]
    whole = ext(x)[0]
    st = melspec.LogMelStream(ext)
    got, most = [], 0
    for i in range(0, L, chunk):
        got.append(st.push(x[i:i + chunk]))
        most = max(most, int(st._buf.numel()))
    got.append(st.finish())
    assert torch.equal(torch.cat(got), whole), (geom, chunk)
    assert most <= n_fft + hop + 1 + chunk                   # only the tail is kept
    lin = melspec.LogMelStream(ext, linear=True)
    assert torch.equal(torch.cat([lin.push(x), lin.finish()]), ext(x, linear=True)[0])


@pytest.mark.parametrize("side_stream", [False, True])
def test_no_hidden_state_between_interleaved_calls(gpu_ok, side_stream):
    ga, gb = MR.GEOMETRIES[3], MR.GEOMETRIES[1]
    ea, eb = _ext(ga), _ext(gb)
    (La, xa), (Lb, xb) = _long(ga), _long(gb, "tone")
    want_a, want_b = ea(xa), eb(xb)
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(3):
            got_b = eb(xb)
            got_a = ea(xa)
            part = ea.frames(xa, 0, La, La, 3, 9)
            assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b) and torch.equal(part, want_a[0, 3:9])
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    assert torch.equal(ea(xa), want_a)


def test_more_rows_than_one_launch_takes(gpu_ok):
    geom = MR.GEOMETRIES[0]
    ext = _ext(geom)
    L = 131
    x = torch.from_numpy(_case(geom, "broadband", 3001)[0])[:L + 69]
    rows = [x[i:i + L - (i % 5)] for i in range(70)]         # 70 rows > 64 entries of a call
    got = ext(rows)
    for i in (0, 1, 63, 64, 69):
        F = MR.frame_count(rows[i].numel(), geom[2])
        assert torch.equal(got[i, :F], ext(rows[i])[0]) and not got[i, F:].any()


def test_copy_synthesis_stream_into_decode_stream(gpu_ok):
    """audio in, mel, vocoder out: a LogMelStream pushing into DecodeStream.push gives the samples of net.decode on the
    one-shot features (same noise key)"""
    cfg = dataclasses.replace(C.tiny(), n_aux=8)
    net = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=5, flavor="trained"), DEV)
    fs, n_fft, hop = 8000, 64, cfg.upsampling_factor
    ext = melspec.LogMelExtractor(fs, n_fft, hop, cfg.n_aux, device=DEV)
    L = 1203
    x = torch.from_numpy(MR.signal("broadband", L, fs, seed=9)).to(DEV)
    feats = ext(x)                                           # (1, F, n_aux)
    F = feats.shape[1]
    aux = feats.transpose(1, 2).contiguous()                 # (1, n_aux, F): what the networks take
    N = F * cfg.upsampling_factor // cfg.seg
    want = net.decode(aux, N, rng_seed=77)[0]
    mel, dec = melspec.LogMelStream(ext), DecodeStream(net, 1, rng_seed=77)
    outs = []
    for i in range(0, L, 160):                               # 20 ms of audio at a time
        new = mel.push(x[i:i + 160])
        outs.append(dec.push(new.t()[None].contiguous())[0])
    outs.append(dec.finish(mel.finish().t()[None].contiguous())[0])
    got = torch.cat(outs, 1)
    assert got.shape == want.shape == (1, N * cfg.seg) and torch.equal(got, want)


def test_driver_writes_feature_files(gpu_ok, tmp_path):
    from scipy.io import wavfile
    fs = 16000
    waves = {"utt_a": MR.signal("broadband", 2400, fs, seed=1), "utt_b": MR.signal("tone", 1777, fs, seed=2)}
    wavdir = tmp_path / "wav"
    os.makedirs(wavdir)
    for name, x in waves.items():
        wavfile.write(str(wavdir / (name + ".wav")), fs, np.round(x * 32767.0).astype(np.int16))
    h5, filt = tmp_path / "hdf5", tmp_path / "wav_filtered"
    argv = ["--expdir", str(tmp_path / "exp"), "--waveforms", str(wavdir), "--hdf5dir", str(h5), "--wavdir", str(filt), "--fs",
            str(fs), "--fftl", "512", "--n_mels", "40", "--verbose", "0"]
    assert FD.main(argv + ["--highpass_cutoff", "0"]) == 0
    ext = melspec.LogMelExtractor(fs, 512, 80, 40, device=DEV)
    files = []
    for name, x in waves.items():
        path = FD.feature_path(str(h5), name + ".wav")
        files.append(path)
        got = featio.read_dataset(path, "/feat_logmel")
        pcm = (np.round(x * 32767.0).astype(np.int16).astype(np.float64) / 32768.0).astype(np.float32)     # what read_wav returns
        want = ext(torch.from_numpy(pcm))[0].cpu().numpy()
        assert got.shape == (1 + x.shape[0] // 80, 40) and got.dtype == np.float32 and np.array_equal(got, want)
    mean, scale = featio.calc_stats(files, "/feat_logmel")
    assert mean.shape == scale.shape == (40,) and np.isfinite(mean).all() and np.isfinite(scale).all() and (scale > 0).all()
    assert not filt.exists()                                 # no filter, no filtered wav
    # with the high-pass filter: the filtered wav is written and the features are those of the filtered signal
    assert FD.main(argv + ["--highpass_cutoff", "70", "--string_path", "/feat_hp"]) == 0
    from shallow_wavenet_amd import dsp
    from shallow_wavenet_amd.train_driver import read_wav
    for name, x in waves.items():
        assert (filt / (name + ".wav")).exists()
        y = dsp.low_cut_filter(read_wav(str(wavdir / (name + ".wav"))), fs, cutoff=70).astype(np.float32)
        got = featio.read_dataset(FD.feature_path(str(h5), name + ".wav"), "/feat_hp")
        assert np.array_equal(got, ext(torch.from_numpy(y))[0].cpu().numpy())
        assert featio.read_dataset(FD.feature_path(str(h5), name + ".wav"), "/feat_logmel").shape == got.shape     # both kept
