"""dev tool: what the rational resampler costs on the device (csrc/swn_resample.hip, swn_resample_chunk).  48 000 -> 22 050 Hz
(147 / 320, 6 401 taps, Q = 44) in front of fs 22 050, n_fft 1 024, hop 110, 80 mels.

(1) A tick of `LogMelPool.push_many` for E = 1 and 64 sessions with 10 ms and 50 ms chunks that arrive on the host, two settings
    alternating tick by tick in one run:
      plain     LogMelPool(resample=None), fed the model-rate audio (the resampler's one-shot output, 220 / 1 102 samples)
      resample  LogMelPool(resample=Resampler), fed the same audio at 48 kHz (480 / 2 400 samples)
(2) One-shot: Resampler on a (16, 144 000) batch (3 s each) that is on the device, against 16 calls of
    scipy.signal.resample_poly(x, 147, 320) on one core, alternating.
(3) `--profile-pass`: 10 ticks of the `resample` setting at E = 64, 50 ms and nothing else, for
    `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/time_resample.py --profile-pass` (a run of its own).

Within a tick the settings take turns at going first.  Per tick and setting: device time (events around the work) and host wall
clock from before the first call to the end of a synchronise.  Reported as median [min - max] over the measured ticks (at least
7) after the warm-up ticks.

  python tools/time_resample.py [--out profiles/resample_timing.json] [--ticks 40] [--warm 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)

FS_IN, FS, N_FFT, HOP, N_MELS, FLOOR = 48000, 22050, 1024, 110, 80, 1e-5
CHUNKS = {10: 480, 50: 2400}            # ms -> samples at FS_IN
ONE_SHOT = (16, 144000)


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


def signals(torch, sessions, n):
    g = torch.Generator().manual_seed(sessions + n)
    return 0.3 * torch.tanh(torch.randn(sessions, n, generator=g)) + 0.05


def pool_setup(torch, melspec, ext, res, sessions, chunk, n_ticks):
    """-> {setting: tick function}; both settings see the same audio, `plain` at the model's rate"""
    x = signals(torch, sessions, n_ticks * chunk)
    y = res(x.cuda()).cpu()                                 # the same audio at the model's rate
    step = y.shape[1] // n_ticks
    fns = {}
    pool = melspec.LogMelPool(ext, capacity=sessions, max_chunk=step + 2)
    sess = [pool.open() for _ in range(sessions)]
    fns["plain"] = lambda t: pool.push_many({s: y[e, t * step:(t + 1) * step] for e, s in enumerate(sess)})
    rpool = melspec.LogMelPool(ext, capacity=sessions, max_chunk=step + 2, resample=res)
    rsess = [rpool.open() for _ in range(sessions)]
    fns["resample"] = lambda t: rpool.push_many({s: x[e, t * chunk:(t + 1) * chunk] for e, s in enumerate(rsess)})
    return fns, step


def pool_ticks(ticks, warm):
    import torch
    from shallow_wavenet_amd import melspec
    assert torch.cuda.is_available(), "needs a HIP device"
    ext = melspec.LogMelExtractor(FS, N_FFT, HOP, N_MELS, floor=FLOOR, device="cuda")
    res = melspec.Resampler(FS_IN, FS, device="cuda")
    rows = []
    for sessions in (1, 64):
        for chunk_ms, chunk in CHUNKS.items():
            fns, step = pool_setup(torch, melspec, ext, res, sessions, chunk, warm + ticks)
            dev = {k: [] for k in fns}
            wall = {k: [] for k in fns}
            for t in range(warm + ticks):
                names = list(fns)
                for name in names[t % len(names):] + names[:t % len(names)]:      # the settings take turns at going first
                    d, w, _ = timed(torch, fns[name], t)
                    if t >= warm:
                        dev[name].append(d)
                        wall[name].append(w)
            row = {"sessions": sessions, "chunk_ms": chunk_ms, "chunk_samples_in": chunk, "chunk_samples_model_rate": step,
                   "chunks_on": "host", "ticks_measured": ticks}
            for name in fns:
                row[name + "_device"] = spread(dev[name])
                row[name + "_wall"] = spread(wall[name])
            m = lambda d, k: statistics.median(d[k])
            row["resample_adds_device_ms"] = round(m(dev, "resample") - m(dev, "plain"), 4)
            row["resample_adds_wall_ms"] = round(m(wall, "resample") - m(wall, "plain"), 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def one_shot(reps, warm):
    import numpy as np
    import torch
    from scipy.signal import resample_poly
    from shallow_wavenet_amd import melspec
    rows_n, n = ONE_SHOT
    x = signals(torch, rows_n, n)
    xd, xn = x.cuda(), x.numpy().astype(np.float64)
    res = melspec.Resampler(FS_IN, FS, device="cuda")
    dev, wall, host = [], [], []
    y = h = None
    for r in range(warm + reps):
        d, w, y = timed(torch, res, xd)
        t0 = time.perf_counter()
        h = [resample_poly(row, res.L, res.M) for row in xn]
        t1 = time.perf_counter()
        if r >= warm:
            dev.append(d)
            wall.append(w)
            host.append((t1 - t0) * 1e3)
    apart = float(np.abs(y.cpu().numpy().astype(np.float64) - np.stack(h)).max())
    row = {"rows": rows_n, "samples_in": n, "samples_out": int(y.shape[1]), "reps_measured": reps, "device": spread(dev),
           "device_wall": spread(wall), "scipy_resample_poly_one_core_wall": spread(host),
           "device_us_per_output_sample": round(statistics.median(dev) * 1e3 / (rows_n * int(y.shape[1])), 6),
           "wall_speedup_over_host": round(statistics.median(host) / statistics.median(wall), 1),
           "max_abs_difference_device_vs_scipy": apart}
    print(json.dumps(row), flush=True)
    return row


def profile_pass():
    import torch
    from shallow_wavenet_amd import melspec
    ext = melspec.LogMelExtractor(FS, N_FFT, HOP, N_MELS, floor=FLOOR, device="cuda")
    res = melspec.Resampler(FS_IN, FS, device="cuda")
    fns, _ = pool_setup(torch, melspec, ext, res, 64, CHUNKS[50], 10)
    for t in range(10):
        fns["resample"](t)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "resample_timing.json"))
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--profile-pass", action="store_true", help="only 10 pooled ticks with the resampler, for a kernel trace")
    a = ap.parse_args()
    if a.profile_pass:
        profile_pass()
        return
    if a.ticks < 7:
        ap.error("at least 7 measured ticks")
    import torch
    from shallow_wavenet_amd import melspec
    r = melspec.Resampler(FS_IN, FS, device="meta")
    out = {"geometry": {"fs_in": FS_IN, "fs": FS, "up": r.L, "down": r.M, "n_taps": r.n_taps, "Q": r.Q, "n_fft": N_FFT, "hop": HOP,
                        "n_mels": N_MELS},
           "warm_ticks": a.warm, "device": torch.cuda.get_device_name(0), "pool_tick": pool_ticks(a.ticks, a.warm),
           "one_shot": one_shot(max(7, a.ticks // 4), 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
