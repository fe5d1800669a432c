"""dev tool: what the F0-adaptive spectral envelope costs on the device (csrc/swn_envelope.hip, swn_envelope) next to its two
neighbours at the run.sh geometry - fs 22 050, n_fft 1 024, hop 110, order 49, alpha 0.455: the mel-cepstrum of the short-time
spectrum (swn_mcep) and the F0 estimator whose column 0 it consumes (swn_f0, 40 - 700 Hz, win 1 024).

SpectralEnvelopeExtractor, MelCepstrumExtractor and F0Extractor alternate, call by call, on a (64, 66 000) batch and on a
(1, 66 000) batch (3 s each, 601 frames a row) that is on the device; the envelope runs at the F0 the estimator gave for the same
batch.  Per call: device time (events around the work).  Reported as median [min - max] over the measured repetitions after the
warm-up ones, the ratios of the medians, and the envelope's fp64 fma per second against the 3.93e13 of the data sheet.  A frame
with window half length hl runs (2 hl + 1) x 2 x bins fma for the transform, bins^2 for the cepstrum and (order + 1) x bins for the
frequency transform; hl follows the frame's F0, so the count is summed over the batch's frames.

Every shape runs in a process of its own under a time limit (`--step_timeout` seconds); a step that fails or runs out of time ends
the tool, and no later step is started.

  python tools/time_envelope.py [--out profiles/envelope_timing.json] [--reps 20] [--warm 3] [--step_timeout 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_f0 import FS, HOP, MAXF0, MINF0, SAMPLES, THRESHOLD, WIN, signals, spread, timed  # noqa: E402

N_FFT, ORDER, ALPHA = 1024, 49, 0.455
SHAPES = (64, 1)
PEAK_FP64_FMA = 3.93e13                                 # vector fp64 fma per second, MI355X data sheet (78.6 TFLOP/s)


def fma_count(env, f0):
    """fp64 fma of the three dense products over the frames of an (R, F) F0 tensor"""
    import numpy as np
    v = f0.double().cpu().numpy()
    lo, hi = 3.0 * env.fs / (env.n_fft - 3.0), env.fs / 4.0
    f0e = np.where((v > lo) & (v <= hi), v, env.default_f0)
    hl = np.floor(1.5 * env.fs / f0e + 0.5)
    bins = env.n_fft // 2 + 1
    return int(((2 * hl + 1) * 2 * bins + bins * bins + (env.order + 1) * bins).sum()), float(hl.mean()), int(hl.max())


def one_shape(rows, reps, warm):
    import torch
    from shallow_wavenet_amd import melspec, pitch
    assert torch.cuda.is_available(), "needs a HIP device"
    env = melspec.SpectralEnvelopeExtractor(FS, N_FFT, HOP, ORDER, ALPHA, device="cuda")
    mcep = melspec.MelCepstrumExtractor(FS, N_FFT, HOP, ORDER, ALPHA, device="cuda")
    f0_ext = pitch.F0Extractor(FS, HOP, MINF0, MAXF0, WIN, THRESHOLD, device="cuda")
    x = signals(torch, rows, SAMPLES).cuda()
    f0 = f0_ext(x)[..., 0].contiguous()
    calls = {"envelope": lambda: env(x, None, f0), "mcep": lambda: mcep(x), "f0": lambda: f0_ext(x)}
    t = {name: [] for name in calls}
    for r in range(warm + reps):
        for name, fn in calls.items():
            d, _, _ = timed(torch, fn)
            if r >= warm:
                t[name].append(d)
    frames = rows * env.frame_count(SAMPLES)
    fma, hl_mean, hl_max = fma_count(env, f0)
    med = {name: statistics.median(v) for name, v in t.items()}
    rate = fma / (med["envelope"] * 1e-3)
    row = {"rows": rows, "samples": SAMPLES, "frames": frames, "voiced_frames": int((f0 != 0).sum()), "reps_measured": reps,
           "warm_reps": warm, "device": torch.cuda.get_device_name(0), "half_window_mean": round(hl_mean, 1), "half_window_max": hl_max,
           "envelope_fp64_fma": fma, "envelope_fp64_fma_per_second": round(rate, 0),
           "envelope_share_of_fp64_vector_peak": round(rate / PEAK_FP64_FMA, 4)}
    for name in calls:
        row[name] = {"device": spread(t[name]), "device_us_per_frame": round(med[name] * 1e3 / frames, 4)}
    row["envelope_over_mcep_device"] = round(med["envelope"] / med["mcep"], 3)
    row["envelope_over_f0_device"] = round(med["envelope"] / med["f0"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "envelope_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--step_timeout", type=int, default=240, help="seconds a shape's process may run")
    ap.add_argument("--rows", type=int, default=None, help="(internal) measure this one shape in this process and write it to --out")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 measured repetitions")
    if a.rows is not None:
        row = one_shape(a.rows, a.reps, a.warm)
        with open(a.out, "w") as f:
            json.dump(row, f)
        return 0
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for shape in SHAPES:                            # this process never opens the device
            part = os.path.join(tmp, f"rows{shape}.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(shape), "--reps", str(a.reps), "--warm", str(a.warm),
                   "--out", part]
            try:
                rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
            except subprocess.TimeoutExpired:
                print(f"rows {shape}: no result inside {a.step_timeout} s; nothing further is started", file=sys.stderr)
                return 124
            if rc != 0:
                print(f"rows {shape}: the step ended with status {rc}; nothing further is started", file=sys.stderr)
                return rc if rc > 0 else 128 - rc
            rows.append(json.load(open(part)))
            print(json.dumps(rows[-1]), flush=True)
    out = {"geometry": {"fs": FS, "n_fft": N_FFT, "hop": HOP, "order": ORDER, "alpha": ALPHA, "f0": {"minf0": MINF0, "maxf0": MAXF0,
                                                                                                   "win": WIN, "threshold": THRESHOLD}},
           "peak_fp64_fma_per_second": PEAK_FP64_FMA, "one_shot": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
