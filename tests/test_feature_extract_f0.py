"""GPU: the stage-1 driver's F0 datasets on three short synthetic wav files: `--f0 true` writes the extractor's own frames (from
the device-filtered batch under `--highpass_on device`), `--f0_cond true` prepends pitch.uv_lf0 to the conditioning dataset and
leaves the old columns bit-identical, and a file without a voiced frame is reported, skipped and turns the return value to 1."""
import os

import numpy as np
import pytest
import torch

import f0_ref as R
from shallow_wavenet_amd import featio, melspec, pitch
from shallow_wavenet_amd import feature_extract_driver as FD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS, FFTL, HOP = 8000, 256, 40


def _write(wavdir, waves):
    from scipy.io import wavfile
    os.makedirs(wavdir, exist_ok=True)
    pcm = {}
    for name, x in waves.items():
        pcm[name] = np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
        wavfile.write(os.path.join(wavdir, name + ".wav"), FS, pcm[name])
    # what the driver reads
    return {name: torch.from_numpy((v.astype(np.float64) / 32768.0).astype(np.float32)) for name, v in pcm.items()}


def _waves():
    return {"utt_a": R.signal("tone", 2400, FS, seed=1), "utt_b": R.signal("half-silent", 3100, FS, seed=2),
            "utt_c": R.signal("tone", 1777, FS, seed=3)}


ARGS = ["--fs", str(FS), "--fftl", str(FFTL), "--hop", str(HOP), "--n_mels", "20", "--verbose", "0", "--minf0", "60", "--maxf0", "500",
        "--f0_win", "256"]


def test_f0_dataset_is_the_extractors_output(gpu_ok, tmp_path):
    raw = _write(str(tmp_path / "wav"), _waves())
    h5 = str(tmp_path / "h5")
    assert FD.main(ARGS + ["--waveforms", str(tmp_path / "wav"), "--hdf5dir", h5, "--highpass_on", "device", "--f0", "true"]) == 0
    ext = pitch.F0Extractor(FS, HOP, 60, 500, 256, device=DEV)
    mel = melspec.LogMelExtractor(FS, FFTL, HOP, 20, device=DEV)
    cut = melspec.LowCut(FS, 70.0, device=DEV)
    for name, x in raw.items():
        y = cut(x)
        path = FD.feature_path(h5, name + ".wav")
        got = featio.read_dataset(path, "/feat_f0")
        F = 1 + x.numel() // HOP
        assert got.dtype == np.float32 and got.shape == (F, 2)
        assert np.array_equal(got, ext(y)[0].cpu().numpy()), name
        assert (got[:, 0] > 0).sum() > F // 3 and np.all(np.abs(got[got[:, 0] > 0, 0] - 120.0) < 8.0)      # the tone's 120 Hz
        assert np.array_equal(featio.read_dataset(path, "/feat_logmel"), mel(y)[0].cpu().numpy())       # the others are as before
    # another dataset name, raw samples
    h5n = str(tmp_path / "h5_raw")
    assert FD.main(ARGS + ["--waveforms", str(tmp_path / "wav"), "--hdf5dir", h5n, "--highpass_cutoff", "0", "--f0", "true",
                           "--f0_string_path", "/f0", "--f0_threshold", "0.2"]) == 0
    ext2 = pitch.F0Extractor(FS, HOP, 60, 500, 256, threshold=0.2, device=DEV)
    got = featio.read_dataset(FD.feature_path(h5n, "utt_c.wav"), "/f0")
    assert np.array_equal(got, ext2(raw["utt_c"])[0].cpu().numpy())
    assert not featio.check_dataset(FD.feature_path(h5n, "utt_c.wav"), "/feat_f0")


@pytest.mark.parametrize("feature_type", ["logmel", "mcep"])
def test_f0_cond_prepends_uv_lf0_and_keeps_the_old_columns(gpu_ok, tmp_path, feature_type):
    raw = _write(str(tmp_path / "wav"), _waves())
    base = ARGS + ["--waveforms", str(tmp_path / "wav"), "--highpass_cutoff", "0", "--feature_type", feature_type, "--mcep_dim", "12"]
    plain, cond = str(tmp_path / "h5_plain"), str(tmp_path / "h5_cond")
    assert FD.main(base + ["--hdf5dir", plain]) == 0
    assert FD.main(base + ["--hdf5dir", cond, "--f0_cond", "true", "--f0", "true"]) == 0
    dataset = "/feat_logmel" if feature_type == "logmel" else "/feat_mcep"
    ext = pitch.F0Extractor(FS, HOP, 60, 500, 256, device=DEV)
    for name, x in raw.items():
        old = featio.read_dataset(FD.feature_path(plain, name + ".wav"), dataset)
        new = featio.read_dataset(FD.feature_path(cond, name + ".wav"), dataset)
        assert new.dtype == np.float32 and new.shape == (old.shape[0], old.shape[1] + 2)
        assert np.array_equal(new[:, 2:], old), name                    # bit-identical to the run without the flag
        f0 = ext(x)[0].cpu().numpy()
        lead = pitch.uv_lf0(f0[:, 0], round(FS / HOP)).astype(np.float32)
        assert np.array_equal(new[:, :2], lead), name
        assert set(np.unique(new[:, 0])) <= {0.0, 1.0} and np.all(np.abs(np.exp(new[:, 1]) - 120.0) < 8.0)
        assert np.array_equal(featio.read_dataset(FD.feature_path(cond, name + ".wav"), "/feat_f0"), f0)
        if feature_type == "logmel":                                    # the second dataset is not the conditioning one
            assert np.array_equal(featio.read_dataset(FD.feature_path(cond, name + ".wav"), "/feat_mcep"),
                                  featio.read_dataset(FD.feature_path(plain, name + ".wav"), "/feat_mcep"))


def test_a_file_without_a_voiced_frame_is_reported_and_skipped(gpu_ok, tmp_path, caplog):
    waves = _waves()
    waves["utt_silent"] = np.zeros(2000, dtype=np.float32)
    _write(str(tmp_path / "wav"), waves)
    h5 = str(tmp_path / "h5")
    with caplog.at_level("ERROR"):
        rc = FD.main(ARGS + ["--waveforms", str(tmp_path / "wav"), "--hdf5dir", h5, "--highpass_cutoff", "0", "--f0_cond", "true",
                             "--f0", "true"])
    assert rc == 1
    assert any("utt_silent" in r.getMessage() and "no voiced frame" in r.getMessage() for r in caplog.records)
    assert not os.path.exists(FD.feature_path(h5, "utt_silent.wav"))
    for name in ("utt_a", "utt_b", "utt_c"):
        assert featio.read_dataset(FD.feature_path(h5, name + ".wav"), "/feat_logmel").shape[1] == 22
    # without --f0_cond a silent file is no error: its F0 frames are [0, 1]
    h5f = str(tmp_path / "h5_f0")
    assert FD.main(ARGS + ["--waveforms", str(tmp_path / "wav"), "--hdf5dir", h5f, "--highpass_cutoff", "0", "--f0", "true"]) == 0
    got = featio.read_dataset(FD.feature_path(h5f, "utt_silent.wav"), "/feat_f0")
    assert got.shape == (51, 2) and np.all(got[:, 0] == 0.0) and np.all(got[:, 1] == 1.0)
