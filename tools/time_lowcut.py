"""dev tool: what the stage-1 low cut costs on the device (csrc/swn_lowcut.hip, swn_lowcut_chunk; the fused window update of
swn_logmel_pool_lowcut in csrc/swn_melspec.hip).  fs 22 050, n_fft 1 024, hop 110, 80 mels, the 255 taps at 70 Hz.

(1) A tick of `LogMelPool.push_many` for E = 1 and 64 sessions with 10 ms (220 samples) and 50 ms (1 102 samples) chunks that
    arrive on the host, three settings alternating tick by tick in one run on identical chunks:
      plain        LogMelPool(low_cut=None): raw samples, no filter - what the pool did before
      lowcut       LogMelPool(low_cut=LowCut): raw samples, filtered inside the window-update launch
      host_filter  every session's chunk through scipy.signal.lfilter with a carried zi (float64), rounded to fp32, then the
                   plain pool: what a caller had to do to serve low-cut features
(2) One-shot: LowCut on a (16, 66 000) batch that is on the device, against 16 calls of dsp.low_cut_filter on one core,
    alternating.
(3) `--plain-runs parent=a.json this=b.json ...`: the plain tick of several processes of two builds (see --plain-only), so that
    the unchanged path can be set against the parent commit's run-to-run spread.

Within a tick the settings take turns at going first (the one behind the host filter's CPU work finds an idle device).
Per tick and setting: device time (events around the work) and host wall clock from before the first call to the end of a
synchronise.  Reported as median [min - max] over the measured ticks (at least 7) after the warm-up ticks.

  python tools/time_lowcut.py [--out profiles/lowcut_timing.json] [--ticks 12] [--warm 4] [--plain-runs LABEL=FILE ...]
  python tools/time_lowcut.py --plain-only --out FILE [--package-root DIR]      (DIR: another checkout with a built library,
                                                                                 the parent commit's for instance)
"""
import argparse
import json
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FS, N_FFT, HOP, N_MELS, FLOOR, CUTOFF = 22050, 1024, 110, 80, 1e-5, 70.0
CHUNKS = {10: 220, 50: 1102}            # ms -> samples
ONE_SHOT = (16, 66000)


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
    return 0.3 * torch.tanh(torch.randn(sessions, n, generator=g)) + 0.05      # a DC offset for the filter to remove


def pool_ticks(ticks, warm, plain_only):
    import numpy as np
    import torch
    from scipy.signal import lfilter
    from shallow_wavenet_amd import dsp, melspec
    assert torch.cuda.is_available(), "needs a HIP device"
    ext = melspec.LogMelExtractor(FS, N_FFT, HOP, N_MELS, floor=FLOOR, device="cuda")
    rows = []
    for sessions in (1, 64):
        for chunk_ms, chunk in CHUNKS.items():
            x = signals(torch, sessions, (warm + ticks) * chunk)
            pools, fns = {}, {}

            def opened(**kw):
                pool = melspec.LogMelPool(ext, capacity=sessions, max_chunk=chunk, **kw)
                return pool, [pool.open() for _ in range(sessions)]

            pools["plain"] = opened()
            fns["plain"] = lambda t, p=pools["plain"]: p[0].push_many(
                {s: x[e, t * chunk:(t + 1) * chunk] for e, s in enumerate(p[1])})
            if not plain_only:
                cut = melspec.LowCut(FS, CUTOFF, device="cuda")
                pools["lowcut"] = opened(low_cut=cut)
                fns["lowcut"] = lambda t, p=pools["lowcut"]: p[0].push_many(
                    {s: x[e, t * chunk:(t + 1) * chunk] for e, s in enumerate(p[1])})
                pools["host_filter"] = opened()
                taps = dsp.low_cut_taps(FS, CUTOFF)
                zi = [np.zeros(taps.size - 1) for _ in range(sessions)]
                xn = x.numpy()

                def host_filter(t, p=pools["host_filter"]):
                    chunks = {}
                    for e, s in enumerate(p[1]):
                        y, zi[e] = lfilter(taps, 1.0, xn[e, t * chunk:(t + 1) * chunk].astype(np.float64), zi=zi[e])
                        chunks[s] = torch.from_numpy(y.astype(np.float32))
                    return p[0].push_many(chunks)

                fns["host_filter"] = host_filter
            dev = {k: [] for k in fns}
            wall = {k: [] for k in fns}
            apart = 0.0
            for t in range(warm + ticks):
                outs = {}
                names = list(fns)
                for name in names[t % len(names):] + names[:t % len(names)]:      # the settings take turns at going first
                    d, w, outs[name] = timed(torch, fns[name], t)
                    if t >= warm:
                        dev[name].append(d)
                        wall[name].append(w)
                if not plain_only:      # the two filters round differently; how far apart that leaves the log-mel frames
                    for a, b in zip(outs["lowcut"].values(), outs["host_filter"].values()):
                        if a.numel():
                            apart = max(apart, float((a - b).abs().max()))
            row = {"sessions": sessions, "chunk_ms": chunk_ms, "chunk_samples": chunk, "chunks_on": "host", "ticks_measured": ticks}
            for name in fns:
                row[name + "_device"] = spread(dev[name])
                row[name + "_wall"] = spread(wall[name])
            if not plain_only:
                m = lambda d, k: statistics.median(d[k])
                row["lowcut_adds_device_ms"] = round(m(dev, "lowcut") - m(dev, "plain"), 4)
                row["lowcut_adds_wall_ms"] = round(m(wall, "lowcut") - m(wall, "plain"), 4)
                row["host_filter_adds_wall_ms"] = round(m(wall, "host_filter") - m(wall, "plain"), 4)
                row["logmel_max_abs_difference_lowcut_vs_host_filter"] = apart
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def one_shot(reps, warm):
    import numpy as np
    import torch
    from shallow_wavenet_amd import dsp, melspec
    rows_n, n = ONE_SHOT
    x = signals(torch, rows_n, n)
    xd, xn = x.cuda(), x.numpy().astype(np.float64)
    cut = melspec.LowCut(FS, CUTOFF, device="cuda")
    dev, wall, host = [], [], []
    y = h = None
    for r in range(warm + reps):
        d, w, y = timed(torch, cut, xd)
        t0 = time.perf_counter()
        h = [dsp.low_cut_filter(row, FS, cutoff=CUTOFF) for row in xn]
        t1 = time.perf_counter()
        if r >= warm:
            dev.append(d)
            wall.append(w)
            host.append((t1 - t0) * 1e3)
    step = float(np.abs(np.rint(y.cpu().numpy().astype(np.float64) * 32767.0) - np.rint(np.stack(h) * 32767.0)).max())
    row = {"rows": rows_n, "samples": n, "reps_measured": reps, "device": spread(dev), "device_wall": spread(wall),
           "host_low_cut_filter_one_core_wall": spread(host),
           "device_us_per_sample": round(statistics.median(dev) * 1e3 / (rows_n * n), 6),
           "wall_speedup_over_host": round(statistics.median(host) / statistics.median(wall), 1),
           "max_pcm16_steps_between_device_and_host": step}
    print(json.dumps(row), flush=True)
    return row


def plain_vs_parent(specs):
    """LABEL=FILE of --plain-only runs -> per (E, chunk) each build's per-process medians, and whether this build's tick sits
    inside (or below) the parent's run-to-run spread"""
    runs = {}
    for spec in specs:
        label, path = spec.split("=", 1)
        with open(path) as f:
            runs.setdefault(label, []).append(json.load(f)["pool_tick"])
    out = []
    first = next(iter(runs.values()))[0]
    for i, ref in enumerate(first):
        row = {"sessions": ref["sessions"], "chunk_ms": ref["chunk_ms"]}
        for clock in ("device", "wall"):
            med = {label: [r[i]["plain_" + clock]["median_ms"] for r in rs] for label, rs in runs.items()}
            for label, v in med.items():
                row[f"{label}_{clock}_medians_ms"] = v
            if "parent" in med and "this" in med:
                lo, hi, mine = min(med["parent"]), max(med["parent"]), statistics.median(med["this"])
                row[f"this_{clock}_median_of_medians_ms"] = round(mine, 4)
                row[f"parent_{clock}_spread_ms"] = [lo, hi]
                row[f"this_{clock}_not_above_parent_spread"] = mine <= hi
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "lowcut_timing.json"))
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--plain-only", action="store_true", help="only the low_cut=None tick (also runs on a build without the low cut)")
    ap.add_argument("--package-root", default=_R, help="the checkout whose shallow_wavenet_amd package is measured")
    ap.add_argument("--plain-runs", nargs="*", default=[], metavar="LABEL=FILE",
                    help="--plain-only results of the labels `parent` and `this`, merged into the output")
    a = ap.parse_args()
    if a.ticks < 7:
        ap.error("at least 7 measured ticks")
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    import shallow_wavenet_amd
    res = {"geometry": {"fs": FS, "n_fft": N_FFT, "hop": HOP, "n_mels": N_MELS, "low_cut_hz": CUTOFF, "n_taps": 255},
           "warm_ticks": a.warm, "device": torch.cuda.get_device_name(0),
           "package": os.path.relpath(os.path.dirname(shallow_wavenet_amd.__file__), _R),
           "pool_tick": pool_ticks(a.ticks, a.warm, a.plain_only)}
    if not a.plain_only:
        res["one_shot"] = one_shot(max(7, a.ticks), 2)
    if a.plain_runs:
        res["plain_tick_vs_parent"] = plain_vs_parent(a.plain_runs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
