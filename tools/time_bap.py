"""dev tool: what the band aperiodicity costs on the device (csrc/swn_f0.hip, swn_bap) next to F0 alone (swn_f0) at the shipped
geometry: fs 22 050, hop 110, win 1 024, 40 - 700 Hz (lags 31 .. 552, S = 1 577), the two bands of `pitch.bap_bands`, 255 taps,
band_win 256.  By operation counts the band-pass adds 255 x 2 x 110 = 56 100 fp64 multiply-adds per frame to the 566 272 of the
difference function, about 10 %; the frame sums add two short wave tasks.  That is an expectation, not a gate.

(1) One-shot: F0Extractor and BandAperiodicityExtractor alternate, call by call, on a (64, 66 000) batch and on a (1, 66 000)
    batch (3 s each, 601 frames a row) that is on the device.
(2) Stream: one `F0Stream.push` and one `BapStream.push` of 50 ms (1 102 samples, 10 or 11 new frames) alternate in the middle of
    a signal, the chunk on the device.

Per call: device time (events around the work) and host wall clock from before the call to the end of a synchronise.  Reported as
median [min - max] over the measured repetitions (at least 7) after the warm-up ones, and the ratio of the medians bap / f0.
`--f0_parent FILE ..` records the medians and ranges of `tools/time_f0.py` runs of the parent commit, taken in the same session
in turn with runs of this build (`--f0_this FILE ..`, as many), and whether each of this build's medians lies inside the range
of the parent's run before it.

  python tools/time_bap.py [--out profiles/bap_timing.json] [--reps 20] [--warm 3] [--f0_this A.json B.json --f0_parent PA.json PB.json]
"""
import argparse
import json
import os
import statistics
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_f0 import CHUNK, FS, HOP, MAXF0, MINF0, SAMPLES, THRESHOLD, WIN, signals, spread, timed  # noqa: E402

N_TAPS, BAND_WIN = 255, 256


def one_shot(f0_ext, bap_ext, rows, reps, warm):
    import torch
    x = signals(torch, rows, SAMPLES).cuda()
    t = {"f0": ([], []), "bap": ([], [])}
    out = {}
    for r in range(warm + reps):
        for name, ext in (("f0", f0_ext), ("bap", bap_ext)):
            d, w, out[name] = timed(torch, ext, x)
            if r >= warm:
                t[name][0].append(d)
                t[name][1].append(w)
    assert torch.equal(out["bap"][..., :2], out["f0"])                  # the F0 columns are swn_f0's
    frames = rows * f0_ext.frame_count(SAMPLES)
    voiced = out["f0"][..., 0] != 0
    row = {"rows": rows, "samples": SAMPLES, "frames": frames, "voiced_frames": int(voiced.sum()), "reps_measured": reps,
           "median_coded_db_voiced": [round(float(out["bap"][..., 2 + b][voiced].median()), 3) for b in range(bap_ext.n_bands)]}
    for name in ("f0", "bap"):
        row[name] = {"device": spread(t[name][0]), "wall": spread(t[name][1]),
                     "device_us_per_frame": round(statistics.median(t[name][0]) * 1e3 / frames, 4)}
    row["bap_over_f0_device"] = round(statistics.median(t["bap"][0]) / statistics.median(t["f0"][0]), 4)
    print(json.dumps(row), flush=True)
    return row


def stream_push(f0_ext, bap_ext, reps, warm):
    import torch
    from shallow_wavenet_amd import pitch
    x = signals(torch, 1, (warm + reps + 4) * CHUNK)[0].cuda()
    streams = {"f0": pitch.F0Stream(f0_ext), "bap": pitch.BapStream(bap_ext)}
    t = {"f0": ([], [], []), "bap": ([], [], [])}
    for st in streams.values():
        st.push(x[:2 * CHUNK])                                          # past the first frames' latency
    for r in range(warm + reps):
        at = (2 + r) * CHUNK
        for name, st in streams.items():
            d, w, out = timed(torch, st.push, x[at:at + CHUNK])
            if r >= warm:
                t[name][0].append(d)
                t[name][1].append(w)
                t[name][2].append(int(out.shape[0]))
    row = {"chunk_ms": 50, "chunk_samples": CHUNK, "chunk_on": "device", "reps_measured": reps}
    for name in ("f0", "bap"):
        row[name] = {"frames_per_push": sorted(set(t[name][2])), "device": spread(t[name][0]), "wall": spread(t[name][1])}
    row["bap_over_f0_device"] = round(statistics.median(t["bap"][0]) / statistics.median(t["f0"][0]), 4)
    print(json.dumps(row), flush=True)
    return row


def f0_against_parent(this_paths, parent_paths):
    """this build's `tools/time_f0.py` medians against the parent commit's [min - max], run by run in the order of the session"""
    rows = []
    for run, (this_path, parent_path) in enumerate(zip(this_paths, parent_paths)):
        this, parent = json.load(open(this_path)), json.load(open(parent_path))
        pairs = [(f"one_shot rows {a['rows']}", a["device"], b["device"]) for a, b in zip(this["one_shot"], parent["one_shot"])]
        pairs.append(("stream_push", this["stream_push"]["device"], parent["stream_push"]["device"]))
        for what, a, b in pairs:
            rows.append({"run": run, "what": what, "this_build_device": a, "parent_device": b,
                         "this_median_inside_parent_range": bool(b["min_ms"] <= a["median_ms"] <= b["max_ms"])})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "bap_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--f0_this", nargs="+", default=[], help="outputs of tools/time_f0.py on this build")
    ap.add_argument("--f0_parent", nargs="+", default=[], help="outputs of tools/time_f0.py on the parent commit, same session")
    ap.add_argument("--f0_kernel_note", default=None, help="a sentence on f0_kernel's device assembly against the parent's")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 measured repetitions")
    import torch
    from shallow_wavenet_amd import pitch
    assert torch.cuda.is_available(), "needs a HIP device"
    f0_ext = pitch.F0Extractor(FS, HOP, MINF0, MAXF0, WIN, THRESHOLD, device="cuda")
    bap_ext = pitch.BandAperiodicityExtractor(FS, HOP, MINF0, MAXF0, WIN, THRESHOLD, n_taps=N_TAPS, band_win=BAND_WIN, device="cuda")
    per_frame = {"difference_function": WIN * (f0_ext.lag_hi + 1), "band_pass": N_TAPS * bap_ext.n_bands * HOP}
    out = {"geometry": {"fs": FS, "hop": HOP, "win": WIN, "minf0": MINF0, "maxf0": MAXF0, "lag_lo": f0_ext.lag_lo,
                        "lag_hi": f0_ext.lag_hi, "span": f0_ext.span, "threshold": THRESHOLD, "bands_hz": bap_ext.bands,
                        "n_taps": N_TAPS, "band_win": bap_ext.band_win, "reach": bap_ext.reach, "fp64_fma_per_frame": per_frame,
                        "expected_bap_over_f0_by_operation_count": round(1.0 + per_frame["band_pass"] / per_frame["difference_function"], 3)},
           "warm_reps": a.warm, "device": torch.cuda.get_device_name(0),
           "one_shot": [one_shot(f0_ext, bap_ext, 64, a.reps, a.warm), one_shot(f0_ext, bap_ext, 1, a.reps, a.warm)],
           "stream_push": stream_push(f0_ext, bap_ext, a.reps, a.warm)}
    if a.f0_this and len(a.f0_this) == len(a.f0_parent):
        out["swn_f0_against_parent"] = f0_against_parent(a.f0_this, a.f0_parent)
    if a.f0_kernel_note:
        out["f0_kernel_assembly"] = a.f0_kernel_note
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
