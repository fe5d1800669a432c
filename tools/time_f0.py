"""dev tool: what F0 and voicing cost on the device (csrc/swn_f0.hip, swn_f0) at the shipped geometry: fs 22 050, hop 110, win
1 024, 40 - 700 Hz (lags 31 .. 552, S = 1 577, 566 272 fp64 multiply-adds per frame).

(1) One-shot: F0Extractor on a (64, 66 000) batch and on a (1, 66 000) batch (3 s each, 601 frames a row) that is on the device.
(2) Stream: one `F0Stream.push` of 50 ms (1 102 samples, 10 or 11 new frames) in the middle of a signal, the chunk on the device.

Per call: device time (events around the work) and host wall clock from before the call to the end of a synchronise.  Reported as
median [min - max] over the measured repetitions (at least 7) after the warm-up ones.  There is no host competitor to time: the
float64 numpy restatement of tests/f0_ref.py is a test reference, and pyworld's Harvest is absent.

  python tools/time_f0.py [--out profiles/f0_timing.json] [--reps 20] [--warm 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)

FS, HOP, WIN, MINF0, MAXF0, THRESHOLD = 22050, 110, 1024, 40.0, 700.0, 0.1
SAMPLES, CHUNK = 66000, 1102


def timed(torch, fn, *a):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    ev0.record()
    out = fn(*a)
    ev1.record()
    torch.cuda.synchronize()
    w1 = time.perf_counter()
    return ev0.elapsed_time(ev1), (w1 - w0) * 1e3, out


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def signals(torch, rows, n):
    """a 120 Hz harmonic tone with noise, silent in its last fifth: voiced and unvoiced frames"""
    g = torch.Generator().manual_seed(rows + n)
    t = torch.arange(n, dtype=torch.float64) / FS
    tone = sum(torch.sin(2 * torch.pi * 120.0 * k * t + 0.3 * k) / k for k in range(1, 12)) * 0.2
    x = tone.float()[None] + 0.01 * torch.randn(rows, n, generator=g)
    x[:, 4 * n // 5:] = 0.0
    return x


def one_shot(ext, rows, reps, warm):
    import torch
    x = signals(torch, rows, SAMPLES).cuda()
    dev, wall = [], []
    out = None
    for r in range(warm + reps):
        d, w, out = timed(torch, ext, x)
        if r >= warm:
            dev.append(d)
            wall.append(w)
    frames = rows * ext.frame_count(SAMPLES)
    row = {"rows": rows, "samples": SAMPLES, "frames": frames, "voiced_frames": int((out[..., 0] != 0).sum()),
           "reps_measured": reps, "device": spread(dev), "wall": spread(wall),
           "device_us_per_frame": round(statistics.median(dev) * 1e3 / frames, 4),
           "fp64_fma_per_second": round(frames * WIN * (ext.lag_hi + 1) / (statistics.median(dev) * 1e-3), 0)}
    print(json.dumps(row), flush=True)
    return row


def stream_push(ext, reps, warm):
    import torch
    from shallow_wavenet_amd import pitch
    x = signals(torch, 1, (warm + reps + 4) * CHUNK)[0].cuda()
    st = pitch.F0Stream(ext)
    st.push(x[:2 * CHUNK])                                          # past the first frames' latency
    dev, wall, got = [], [], []
    for r in range(warm + reps):
        at = (2 + r) * CHUNK
        d, w, out = timed(torch, st.push, x[at:at + CHUNK])
        if r >= warm:
            dev.append(d)
            wall.append(w)
            got.append(int(out.shape[0]))
    row = {"chunk_ms": 50, "chunk_samples": CHUNK, "frames_per_push": sorted(set(got)), "chunk_on": "device",
           "reps_measured": reps, "device": spread(dev), "wall": spread(wall)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "f0_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 measured repetitions")
    import torch
    from shallow_wavenet_amd import pitch
    assert torch.cuda.is_available(), "needs a HIP device"
    ext = pitch.F0Extractor(FS, HOP, MINF0, MAXF0, WIN, THRESHOLD, device="cuda")
    out = {"geometry": {"fs": FS, "hop": HOP, "win": WIN, "minf0": MINF0, "maxf0": MAXF0, "lag_lo": ext.lag_lo, "lag_hi": ext.lag_hi,
                        "span": ext.span, "threshold": THRESHOLD, "fp64_fma_per_frame": WIN * (ext.lag_hi + 1)},
           "warm_reps": a.warm, "device": torch.cuda.get_device_name(0),
           "one_shot": [one_shot(ext, 64, a.reps, a.warm), one_shot(ext, 1, a.reps, a.warm)],
           "stream_push": stream_push(ext, a.reps, a.warm)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
