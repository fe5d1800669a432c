"""Stage 1 of run.sh for the feature types computed on the device: every waveform of a directory or list is read, optionally
high-pass filtered (`dsp.low_cut_filter`, the filtered wav written under `--wavdir`), turned into log-mel features in batches
(`melspec.LogMelExtractor`, csrc/swn_melspec.hip; the definition is in melspec.py) and written as dataset `--string_path` of
`<hdf5dir>/<name>.h5` - or `<name>.npz`, the side format of featio.py, where h5py is absent.  The flag names are those of the
reference's stage-1 command that make sense here; `--feature_type world` is the WORLD / SPTK analysis, which needs pyworld and
pysptk (dsp.extract_features raises the ImportError that says so).

With `--mcep_dim M` (> 0) each batch also goes through `melspec.MelCepstrumExtractor` (order M, `--mcep_alpha`, `--mcep_floor`)
and the mel-cepstra of the same frames are written as a second dataset `--mcep_string_path` (default `/feat_mcep`, M + 1
columns, as the reference's mcep_dim counts) of the same file; `--feature_type mcep` writes them as the conditioning dataset
instead (`--string_path` when it is given, else `--mcep_string_path`).  It is the mel-cepstrum of the short-time spectrum, not
of WORLD's envelope, and parity with pysptk is not pinned (melspec.py).

Frames: F = 1 + len // hop with hop = round(fs * shiftms / 1000) unless `--hop` is given - not WORLD's count when 5 ms is not an
integer number of samples; the training drivers' validate_length trims features and waveform to each other.  The statistics
of these features (`calc_stats --string_path /feat_logmel`) initialise scale_in as usual.  The noise-shaping stages take the
corpus-mean mel-cepstrum from the second dataset: `calc_stats --string_path /feat_mcep`, then `noise_shaping.py --stats ...
--stats_string_path /feat_mcep --mcep_dim_start 0` (stages 3 / 6 / 9) and `decode_driver --restore_stats ...
--stats_string_path /feat_mcep --mcep_dim_start 0` (stage 6 on the device); INTEGRATION.md has the recipe.

`--highpass_on device` moves the high-pass filter to the device (`melspec.LowCut`, csrc/swn_lowcut.hip): a batch of raw
waveforms is filtered there, the features are taken from that device tensor with no host round trip, and the `--wavdir` files
are written from it.  These are the bits `LogMelStream(low_cut=)` and `LogMelPool(low_cut=)` give a live session, so features
taken this way and features taken while serving agree exactly.  The default `host` is `dsp.low_cut_filter` as before; the two
settings differ by at most the rounding of the device definition (melspec.py): both sum the same products in fp64, in
different orders, and the device rounds once to fp32, so a sample of a PCM16 file can differ by one step.

`--resample true` takes files of any sampling frequency: a file whose own rate is not --fs is resampled to --fs on the device
(`melspec.Resampler`, csrc/swn_resample.hip: the filter of scipy's resample_poly as one fp64 fma chain per sample, rounded once
to fp32) before the high-pass filter, wherever that runs; `--wavdir` then receives audio at --fs.  These are the bits
`LogMelStream(resample=)` and `LogMelPool(resample=)` give a live session fed at the file's rate.  Without the flag such a file
is refused, as before.

`--f0 true` adds F0 and voicing (`pitch.F0Extractor`, csrc/swn_f0.hip; the definition is in pitch.py - a difference-function
estimator in a fixed arithmetic, not WORLD's Harvest): dataset `--f0_string_path` (default `/feat_f0`) of shape (F, 2), raw
`[F0 in Hz or 0.0 when unvoiced, aperiodicity]` of the same frames, taken from the same batch as the other features (the
device-filtered one under `--highpass_on device`).  `--minf0` / `--maxf0` are the reference's flags, `--f0_win` / `--f0_threshold`
the estimator's window and threshold.  `--f0_cond true` prepends `pitch.uv_lf0` - `[uv, log of the bridged, 20 Hz low-passed F0]`,
the first two columns of the reference's layout, at the frame rate round(fs / hop) - to the conditioning dataset: with
`--feature_type mcep` the file holds `[uv, lf0, c(0 .. M)]`, which `noise_shaping.py --mcep_dim_start 2` reads.  A file without a
voiced frame has no continuous F0: it is logged and skipped, and the driver returns 1.

`--bap true` adds the band aperiodicity (`pitch.BandAperiodicityExtractor`, the same file's swn_bap; the definition is in
pitch.py - this project's own measure, not WORLD's D4C / code_aperiodicity): dataset `--bap_string_path` (default `/feat_bap`) of
shape (F, B), the coded aperiodicity in dB of the B = `pitch.bap_bands(fs)` bands the reference codes at this rate (2 at 22.05
kHz; a rate below 12 kHz has none and is refused), with `--bap_taps` taps per band-pass and the sum window `--bap_win`.  One call
serves `--f0` / `--f0_cond` too: `/feat_f0` is its columns 0 - 1.  With `--f0_cond true` the conditioning dataset becomes `[uv,
lf0, bap_0 .. bap_{B-1}, features]`, the reference's column order, so `noise_shaping.py --mcep_dim_start` is 2 + B - run.sh's
`stdim`.

`--mcep_envelope true` (with `--mcep_dim M` > 0) takes the mel-cepstra from the F0-adaptive spectral envelope
(`melspec.SpectralEnvelopeExtractor`, csrc/swn_envelope.hip; the definition is in melspec.py - CheapTrick's procedure in a fixed
arithmetic, parity with WORLD neither claimed nor pinned) instead of the short-time spectrum: the pitch harmonics are not in
them.  The F0 is column 0 of the batch's one `F0Extractor` / `BandAperiodicityExtractor` call, with `--minf0` / `--maxf0` /
`--f0_win` / `--f0_threshold` as for `--f0`; that call is issued even without `--f0`, and `/feat_f0` is still written only when
asked.  Datasets, columns and the noise-shaping recipe stay as above.  Without the flag the files are what they were."""
from __future__ import annotations

import argparse
import functools
import logging
import multiprocessing as mp
import os
import sys
from typing import List, Optional, Sequence

import numpy as np

from . import dsp, featio
from .decode_driver import write_wav_pcm16
from .noise_shaping_driver import _strtobool, list_waveforms, read_wav_fs

FS, SHIFTMS, FFTL, HIGHPASS_CUTOFF, MCEP_ALPHA = 22050, 5.0, 1024, 70, 0.455      # the reference's stage-1 defaults
MINF0, MAXF0 = 40, 700
STRING_PATH = "/feat_logmel"
BATCH = 16                                                     # utterances per device call
MAX_JOBS = 16                                                  # worker processes that open the device


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="conditioning features from waveforms (log-mel on the device)")
    p.add_argument("--expdir", default=None, help="experiment directory: the log goes to <expdir>/feature_extract.log")
    p.add_argument("--waveforms", default=None, help="directory or list file of the input wav files")
    p.add_argument("--hdf5dir", default=None, help="directory of the feature files")
    p.add_argument("--wavdir", default=None, help="directory of the high-pass filtered wav files (none: not written)")
    p.add_argument("--fs", default=FS, type=int, help="sampling frequency")
    p.add_argument("--shiftms", default=SHIFTMS, type=float, help="frame shift in msec (the hop, unless --hop is given)")
    p.add_argument("--fftl", default=FFTL, type=int, help="FFT length: a multiple of 32")
    p.add_argument("--highpass_cutoff", default=HIGHPASS_CUTOFF, type=int, help="cut-off of the high-pass filter, 0: none")
    p.add_argument("--highpass_on", default="host", choices=("host", "device"),
                   help="where the high-pass filter runs: host (dsp.low_cut_filter, scipy in float64) or device (melspec.LowCut: "
                        "the bits of the live streams and pools).  The two differ by at most the rounding of the device "
                        "definition - fp64 sums in different orders, rounded once to fp32 - so a PCM16 sample can differ by one "
                        "step (not a reference flag)")
    p.add_argument("--resample", default=False, type=_strtobool,
                   help="true: a file whose sampling frequency is not --fs is resampled to --fs on the device (melspec.Resampler) "
                        "before the high-pass filter; false: it is refused (not a reference flag)")
    p.add_argument("--n_jobs", default=1, type=int, help=f"number of worker processes (at most {MAX_JOBS})")
    p.add_argument("--verbose", default=1, type=int, help="log level")
    p.add_argument("--feature_type", default="logmel", choices=("logmel", "mcep", "world"), help="not a reference flag")
    p.add_argument("--n_mels", default=80, type=int, help="mel filters (logmel; not a reference flag)")
    p.add_argument("--fmin", default=0.0, type=float, help="lowest filter edge in Hz (logmel; not a reference flag)")
    p.add_argument("--fmax", default=None, type=float, help="highest filter edge in Hz, default fs / 2 (logmel; not a reference flag)")
    p.add_argument("--hop", default=None, type=int, help="hop in samples, default round(fs * shiftms / 1000) (logmel; not a reference flag)")
    p.add_argument("--floor", default=1e-5, type=float, help="floor of the mel amplitude under the log (logmel; not a reference flag)")
    p.add_argument("--string_path", default=STRING_PATH, help="dataset name in the feature files (not a reference flag)")
    p.add_argument("--mcep_dim", default=0, type=int,
                   help="order of the mel-cepstrum, 0: none; the dataset has mcep_dim + 1 columns (as the reference counts)")
    p.add_argument("--mcep_alpha", default=MCEP_ALPHA, type=float, help="all-pass constant of the mel-cepstrum")
    p.add_argument("--mcep_floor", default=1e-5, type=float, help="floor of the amplitude under the log (mel-cepstrum; not a reference flag)")
    p.add_argument("--mcep_string_path", default="/feat_mcep", help="dataset name of the mel-cepstra (not a reference flag)")
    p.add_argument("--mcep_envelope", default=False, type=_strtobool,
                   help="true: the mel-cepstra are those of the F0-adaptive spectral envelope (melspec.SpectralEnvelopeExtractor) at "
                        "the F0 of the batch's F0 / band aperiodicity call, not of the short-time spectrum; needs --mcep_dim > 0 "
                        "(not a reference flag)")
    p.add_argument("--minf0", default=MINF0, type=int, help="minimum f0")
    p.add_argument("--maxf0", default=MAXF0, type=int, help="maximum f0")
    p.add_argument("--f0", default=False, type=_strtobool,
                   help="true: write [F0 in Hz, aperiodicity] per frame (pitch.F0Extractor) as dataset --f0_string_path "
                        "(not a reference flag)")
    p.add_argument("--f0_string_path", default="/feat_f0", help="dataset name of the F0 frames (not a reference flag)")
    p.add_argument("--f0_cond", default=False, type=_strtobool,
                   help="true: prepend [uv, log F0 (continuous, smoothed)] (pitch.uv_lf0) to the conditioning dataset of "
                        "--feature_type logmel / mcep (not a reference flag)")
    p.add_argument("--f0_win", default=1024, type=int, help="window of the F0 estimator in samples (not a reference flag)")
    p.add_argument("--f0_threshold", default=0.1, type=float,
                   help="voicing threshold of the F0 estimator on the normalised difference function (not a reference flag)")
    p.add_argument("--bap", default=False, type=_strtobool,
                   help="true: write the coded band aperiodicity in dB per frame (pitch.BandAperiodicityExtractor) as dataset "
                        "--bap_string_path, and with --f0_cond true put it behind [uv, lf0] (not a reference flag)")
    p.add_argument("--bap_string_path", default="/feat_bap", help="dataset name of the band aperiodicity (not a reference flag)")
    p.add_argument("--bap_taps", default=255, type=int, help="taps of each band-pass filter, odd (not a reference flag)")
    p.add_argument("--bap_win", default=256, type=int,
                   help="sum window of the band aperiodicity in samples, clipped to --f0_win (not a reference flag)")
    return p


def hop_of(args) -> int:
    return int(args.hop) if args.hop is not None else int(round(args.fs * args.shiftms / 1000.0))


def feature_path(hdf5dir: str, wav_name: str) -> str:
    """<hdf5dir>/<name>.h5 where h5py is importable, else the .npz side format"""
    try:
        import h5py  # noqa: F401
        ext = ".h5"
    except ImportError:
        ext = ".npz"
    return os.path.join(hdf5dir, os.path.splitext(os.path.basename(wav_name))[0] + ext)


def on_device(args) -> bool:
    """the high-pass filter runs on the device (--highpass_on device with a cut-off)"""
    return getattr(args, "highpass_on", "host") == "device" and args.highpass_cutoff != 0


@functools.lru_cache(maxsize=8)
def _resampler(fs_in: int, fs_out: int, device: str):
    from .melspec import Resampler
    return Resampler(fs_in, fs_out, device=device)


def load_waveform(name: str, args, device="cuda") -> np.ndarray:
    """the utterance as the features see it: mono float64, high-pass filtered (and written to --wavdir) when the cut-off is not 0
    - or raw when the filter runs on the device (extract_files filters the batch and writes --wavdir from the result).
    ValueError when the file's sampling frequency is not --fs (the mel scale, the hop and the filter would all be wrong) - unless
    --resample is true: then the file is resampled to --fs on `device` first (fp32 values, which float64 holds exactly)."""
    x, fs = read_wav_fs(name)
    if fs != args.fs and not getattr(args, "resample", False):
        raise ValueError(f"{name}: sampling frequency {fs} does not match --fs {args.fs}")
    if x.ndim > 1:
        x = x[:, 0]
    if fs != args.fs:
        x = _resampler(int(fs), int(args.fs), str(device))(x.astype(np.float32))[0].cpu().numpy().astype(np.float64)
    if args.highpass_cutoff != 0 and not on_device(args):
        x = dsp.low_cut_filter(x, args.fs, cutoff=args.highpass_cutoff)
        if args.wavdir:
            os.makedirs(args.wavdir, exist_ok=True)
            write_wav_pcm16(os.path.join(args.wavdir, os.path.basename(name)), np.clip(x, -1.0, 1.0), args.fs)
    return x


def extract_files(files: Sequence[str], args, device="cuda") -> int:
    want_f0, f0_cond = bool(getattr(args, "f0", False)), bool(getattr(args, "f0_cond", False))
    want_bap = bool(getattr(args, "bap", False))
    want_env = bool(getattr(args, "mcep_envelope", False))
    if args.feature_type == "world":
        if want_env:
            logging.error("--mcep_envelope serves the features computed on the device, not --feature_type world")
            return 2
        if want_f0 or f0_cond or want_bap:
            logging.error("--f0 / --f0_cond / --bap serve the features computed on the device; --feature_type world has its own "
                          "F0 and aperiodicity")
            return 2
        if on_device(args):
            logging.error("--highpass_on device serves the features computed on the device, not --feature_type world")
            return 2
        for name in files:
            feats = dsp.extract_features(load_waveform(name, args, device), args.fs, shiftms=args.shiftms, fftl=args.fftl)
            featio.write_dataset(feature_path(args.hdf5dir, name), args.string_path, feats)
        return 0
    from .melspec import LogMelExtractor, LowCut, MelCepstrumExtractor, SpectralEnvelopeExtractor
    as_cond = args.feature_type == "mcep"
    if want_env and args.mcep_dim <= 0:
        logging.error("--mcep_envelope needs --mcep_dim > 0")
        return 2
    if as_cond and args.mcep_dim <= 0:
        logging.error("--feature_type mcep needs --mcep_dim > 0")
        return 2
    # (extractor, dataset) of every feature the files receive; all share the frames F = 1 + len // hop
    jobs = []
    if not as_cond:
        jobs.append((LogMelExtractor(args.fs, args.fftl, hop_of(args), args.n_mels, args.fmin, args.fmax, args.floor, device),
                     args.string_path))
    if args.mcep_dim > 0:
        dataset = args.string_path if as_cond and args.string_path != STRING_PATH else args.mcep_string_path
        if want_env:
            try:
                env_ext = SpectralEnvelopeExtractor(args.fs, args.fftl, hop_of(args), args.mcep_dim, args.mcep_alpha,
                                                    args.mcep_floor, device=device)
            except ValueError as e:
                logging.error("--mcep_envelope: %s", e)
                return 2
            jobs.append((env_ext, dataset))
        else:
            jobs.append((MelCepstrumExtractor(args.fs, args.fftl, hop_of(args), args.mcep_dim, args.mcep_alpha, args.mcep_floor,
                                              device), dataset))
    ext = jobs[0][0]
    f0_ext = None
    if want_bap:                                                    # one call serves the F0 columns too
        from .pitch import BandAperiodicityExtractor, uv_lf0
        try:
            f0_ext = BandAperiodicityExtractor(args.fs, hop_of(args), args.minf0, args.maxf0, args.f0_win, args.f0_threshold,
                                               n_taps=args.bap_taps, band_win=args.bap_win, device=device)
        except ValueError as e:
            logging.error("--bap: %s", e)
            return 2
    elif want_f0 or f0_cond or want_env:                            # the envelope takes its F0 from this call
        from .pitch import F0Extractor, uv_lf0
        f0_ext = F0Extractor(args.fs, hop_of(args), args.minf0, args.maxf0, args.f0_win, args.f0_threshold, device)
    cut = LowCut(args.fs, args.highpass_cutoff, device=device) if on_device(args) else None
    rc = 0
    for i in range(0, len(files), BATCH):
        names: List[str] = []
        waves: List[np.ndarray] = []
        for name in files[i:i + BATCH]:
            try:
                x = load_waveform(name, args, device)
            except ValueError as e:
                logging.error("%s", e)
                rc = 1
                continue
            if x.shape[0] <= args.fftl // 2:
                logging.error("%s: %d samples, --fftl %d needs more than %d", name, x.shape[0], args.fftl, args.fftl // 2)
                rc = 1
                continue
            names.append(name)
            waves.append(x.astype(np.float32))
        if not names:
            continue
        batch, lengths = waves, None
        if cut is not None:
            # raw samples up, filtered on the device; the features read that tensor, the wav files are written from it
            lengths = [x.shape[0] for x in waves]
            batch = cut(waves)
            if args.wavdir:
                os.makedirs(args.wavdir, exist_ok=True)
                for name, n, y in zip(names, lengths, batch.cpu().numpy()):
                    write_wav_pcm16(os.path.join(args.wavdir, os.path.basename(name)), np.clip(y[:n], -1.0, 1.0), args.fs)
        lead: List[Optional[np.ndarray]] = [None] * len(names)     # --f0_cond: the [uv, lf0 (, bap)] columns of each file
        skip = [False] * len(names)
        f0_dev = None                                               # --mcep_envelope: the batch's F0 column, on the device
        if f0_ext is not None:
            f0ap = f0_ext(batch, lengths)
            if want_env:
                f0_dev = f0ap[..., 0].contiguous()
            f0ap = f0ap.cpu().numpy()
            for k, (name, x) in enumerate(zip(names, waves)):
                frames = f0ap[k, :ext.frame_count(x.shape[0])]
                contour, bap = np.ascontiguousarray(frames[:, :2]), np.ascontiguousarray(frames[:, 2:])
                if f0_cond:
                    try:
                        lead[k] = np.concatenate([uv_lf0(contour[:, 0], int(round(args.fs / hop_of(args)))).astype(np.float32),
                                                  bap], axis=1)
                    except ValueError as e:
                        logging.error("%s: %s (--f0_cond needs one for the continuous F0): skipped", name, e)
                        rc, skip[k] = 1, True
                        continue
                if want_f0:
                    out = feature_path(args.hdf5dir, name)
                    featio.write_dataset(out, args.f0_string_path, contour)
                    logging.info("%s -> %s %s %s", name, out, args.f0_string_path, contour.shape)
                if want_bap:
                    out = feature_path(args.hdf5dir, name)
                    featio.write_dataset(out, args.bap_string_path, bap)
                    logging.info("%s -> %s %s %s", name, out, args.bap_string_path, bap.shape)
        for j, (extractor, dataset) in enumerate(jobs):
            feats = (extractor(batch, lengths, f0_dev) if isinstance(extractor, SpectralEnvelopeExtractor) else
                     extractor(batch, lengths)).cpu().numpy()
            for k, (name, x, f) in enumerate(zip(names, waves, feats)):
                if skip[k]:
                    continue
                out = feature_path(args.hdf5dir, name)
                f = f[:ext.frame_count(x.shape[0])]
                if j == 0 and lead[k] is not None:                  # the conditioning dataset
                    f = np.concatenate([lead[k], f], axis=1)
                featio.write_dataset(out, dataset, f)
                logging.info("%s -> %s %s %s", name, out, dataset, f.shape)
    return rc


def _job(files, args) -> None:
    sys.exit(extract_files(files, args))


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose > 0 else logging.WARN, format="%(asctime)s %(message)s")
    if not args.waveforms or not args.hdf5dir:
        logging.error("--waveforms and --hdf5dir are required")
        return 2
    log_file = None
    if args.expdir:
        os.makedirs(args.expdir, exist_ok=True)
        log_file = logging.FileHandler(os.path.join(args.expdir, "feature_extract.log"))
        logging.getLogger().addHandler(log_file)
    try:
        return _run(args)
    finally:
        if log_file is not None:
            logging.getLogger().removeHandler(log_file)
            log_file.close()


def _run(args) -> int:
    files = list_waveforms(args.waveforms)
    os.makedirs(args.hdf5dir, exist_ok=True)
    n_jobs = min(args.n_jobs, MAX_JOBS)
    if n_jobs <= 1 or len(files) <= 1:
        return extract_files(files, args)
    ctx = mp.get_context("spawn")
    parts = [list(p) for p in np.array_split(np.asarray(files, dtype=object), n_jobs) if len(p)]
    procs = [ctx.Process(target=_job, args=(p, args)) for p in parts]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join()
    # a worker that raised or was killed has a non-zero exit code too
    return max(abs(pr.exitcode) for pr in procs)


if __name__ == "__main__":
    sys.exit(main())
