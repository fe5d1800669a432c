"""GPU: the stage-1 driver's band aperiodicity on three short synthetic wav files at 16 kHz (one coded band, as the reference has
there): `--bap true` writes the extractor's own columns, `/feat_f0` from the same call equals its columns 0 - 1, `--f0_cond true`
puts the band columns between [uv, lf0] and the features - the reference's order - and leaves the old columns bit-identical, and
the noise-shaping driver reads the same mel-cepstrum mean at `--mcep_dim_start 2 + B` of that dataset as at 0 of `/feat_mcep`."""
import os

import numpy as np
import pytest
import torch

import bap_ref as R
from shallow_wavenet_amd import featio, pitch
from shallow_wavenet_amd import feature_extract_driver as FD
from shallow_wavenet_amd import noise_shaping_driver as ND

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS, FFTL, HOP, B, M = 16000, 512, 80, 1, 12
ARGS = ["--fs", str(FS), "--fftl", str(FFTL), "--hop", str(HOP), "--n_mels", "20", "--verbose", "0", "--minf0", "50", "--maxf0", "600",
        "--f0_win", "512", "--highpass_cutoff", "0"]


def _write(wavdir):
    from scipy.io import wavfile
    waves = {"utt_a": R.signal("rich", 4800, FS, seed=1), "utt_b": R.signal("rich-noisy", 6100, FS, seed=2),
             "utt_c": R.signal("half-silent", 3777, FS, seed=3)}
    os.makedirs(wavdir, exist_ok=True)
    raw = {}
    for name, x in waves.items():
        pcm = np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
        wavfile.write(os.path.join(wavdir, name + ".wav"), FS, pcm)
        raw[name] = torch.from_numpy((pcm.astype(np.float64) / 32768.0).astype(np.float32))     # what the driver reads
    return raw


def test_bap_and_f0_datasets_are_the_extractors_output(gpu_ok, tmp_path):
    assert len(pitch.bap_bands(FS)) == B
    raw = _write(str(tmp_path / "wav"))
    h5 = str(tmp_path / "h5")
    assert FD.main(ARGS + ["--waveforms", str(tmp_path / "wav"), "--hdf5dir", h5, "--bap", "true", "--f0", "true"]) == 0
    ext = pitch.BandAperiodicityExtractor(FS, HOP, 50, 600, 512, device=DEV)
    f0_ext = pitch.F0Extractor(FS, HOP, 50, 600, 512, device=DEV)
    for name, x in raw.items():
        path = FD.feature_path(h5, name + ".wav")
        want = ext(x)[0].cpu().numpy()
        F = 1 + x.numel() // HOP
        bap, f0 = featio.read_dataset(path, "/feat_bap"), featio.read_dataset(path, "/feat_f0")
        assert bap.dtype == np.float32 and bap.shape == (F, B) and f0.shape == (F, 2)
        assert np.array_equal(bap, want[:, 2:]) and np.array_equal(f0, want[:, :2]), name
        assert np.array_equal(f0, f0_ext(x)[0].cpu().numpy())
        voiced = f0[:, 0] > 0
        assert voiced.sum() > F // 4 and np.all(bap[~voiced] == 0.0) and (bap[voiced] < 0.0).any() and np.all(bap <= 0.0)
    # other names and parameters; without --f0 there is no F0 dataset
    h5n = str(tmp_path / "h5_other")
    assert FD.main(ARGS + ["--waveforms", str(tmp_path / "wav"), "--hdf5dir", h5n, "--bap", "true", "--bap_string_path", "/bap",
                           "--bap_taps", "127", "--bap_win", "128"]) == 0
    ext2 = pitch.BandAperiodicityExtractor(FS, HOP, 50, 600, 512, n_taps=127, band_win=128, device=DEV)
    path = FD.feature_path(h5n, "utt_a.wav")
    assert np.array_equal(featio.read_dataset(path, "/bap"), ext2(raw["utt_a"])[0].cpu().numpy()[:, 2:])
    assert not featio.check_dataset(path, "/feat_bap") and not featio.check_dataset(path, "/feat_f0")


def test_f0_cond_with_bap_writes_the_reference_column_order(gpu_ok, tmp_path):
    raw = _write(str(tmp_path / "wav"))
    base = ARGS + ["--waveforms", str(tmp_path / "wav"), "--feature_type", "mcep", "--mcep_dim", str(M)]
    plain, old, cond = str(tmp_path / "h5_plain"), str(tmp_path / "h5_f0cond"), str(tmp_path / "h5_cond")
    assert FD.main(base + ["--hdf5dir", plain]) == 0
    assert FD.main(base + ["--hdf5dir", old, "--f0_cond", "true"]) == 0
    assert FD.main(base + ["--hdf5dir", cond, "--f0_cond", "true", "--bap", "true"]) == 0
    ext = pitch.BandAperiodicityExtractor(FS, HOP, 50, 600, 512, device=DEV)
    files_plain, files_cond = [], []
    for name, x in raw.items():
        a = featio.read_dataset(FD.feature_path(plain, name + ".wav"), "/feat_mcep")
        b = featio.read_dataset(FD.feature_path(old, name + ".wav"), "/feat_mcep")
        c = featio.read_dataset(FD.feature_path(cond, name + ".wav"), "/feat_mcep")
        files_plain.append(FD.feature_path(plain, name + ".wav"))
        files_cond.append(FD.feature_path(cond, name + ".wav"))
        assert c.dtype == np.float32 and c.shape == (a.shape[0], 2 + B + M + 1)
        assert np.array_equal(c[:, 2 + B:], a) and np.array_equal(c[:, :2], b[:, :2]) and np.array_equal(b[:, 2:], a), name
        frames = ext(x)[0].cpu().numpy()
        assert np.array_equal(c[:, 2:2 + B], frames[:, 2:]), name
        assert np.array_equal(c[:, :2], pitch.uv_lf0(frames[:, 0], round(FS / HOP)).astype(np.float32))
        assert np.array_equal(featio.read_dataset(FD.feature_path(cond, name + ".wav"), "/feat_bap"), frames[:, 2:])
    # stage 3: noise shaping reads the mel-cepstrum mean at 2 + B = run.sh's stdim of the conditioning dataset
    s_plain, s_cond = str(tmp_path / "stats_plain.npz"), str(tmp_path / "stats_cond.npz")
    for stats, files in ((s_plain, files_plain), (s_cond, files_cond)):
        mean, scale = featio.calc_stats(files, "/feat_mcep")
        featio.write_stats(stats, "/feat_mcep", mean, scale)
    m_plain, m_cond = ND.mean_mcep_vector(s_plain, "/feat_mcep"), ND.mean_mcep_vector(s_cond, "/feat_mcep")
    assert m_cond.shape == (2 + B + M + 1,) and np.allclose(m_cond[2 + B:], m_plain, rtol=1e-12, atol=0)
    common = ["--waveforms", str(tmp_path / "wav"), "--fs", str(FS), "--mcep_alpha", "0.41", "--verbose", "0", "--inv", "true",
              "--stats_string_path", "/feat_mcep"]
    assert ND.main(common + ["--stats", s_plain, "--writedir", str(tmp_path / "ns_plain"), "--mcep_dim_start", "0"]) == 0
    assert ND.main(common + ["--stats", s_cond, "--writedir", str(tmp_path / "ns_cond"), "--mcep_dim_start", str(2 + B)]) == 0
    from scipy.io import wavfile
    for name in raw:
        _, ya = wavfile.read(str(tmp_path / "ns_plain" / (name + ".wav")))
        _, yb = wavfile.read(str(tmp_path / "ns_cond" / (name + ".wav")))
        _, x = wavfile.read(str(tmp_path / "wav" / (name + ".wav")))
        assert np.abs(ya.astype(np.int64) - yb.astype(np.int64)).max() <= 1 and np.abs(ya.astype(np.int64) - x).max() > 30
