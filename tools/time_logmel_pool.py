"""dev tool: what the mel front end of a tick costs for E sessions, through one `LogMelPool.push_many` (csrc/swn_melspec.hip,
swn_logmel_pool: two launches and one staging copy per 64 sessions) and through what the pool replaces: E times
`LogMelStream.push` plus the `.t()[None].contiguous()` its consumer needs (`DecodeStream.push` / `DecodePool.push_many` take
(1, n_aux, f)).  fs 22 050, n_fft 1 024, hop 110, 80 mels; E = 1 and 64; chunks of 10 ms (220 samples) and 50 ms
(1 102 samples); chunks on the device and on the host.

The two paths alternate tick by tick in one run on identical chunks.  Per tick and path: device time (events around the
path's work) and host wall clock from before the first call to the end of a synchronise.  Reported as median [min - max] over
the measured ticks (at least 7) after the warm-up ticks.  The outputs of the two paths are compared on every tick (after the
clocks have stopped): `identical` says whether all were equal bit for bit.  Where profiles/pool_frontend_timing.json has the
same E and chunk size (BL6 cfg2 Laplace, DecodePool), its `push_many` front end and decode tick are copied beside the
figures, so the mel front end's share of a whole tick can be read off.

  python tools/time_logmel_pool.py [--out profiles/logmel_pool_timing.json] [--ticks 12] [--warm 4]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_logmel_pool.py --profile-pass    (a run of its own:
      10 ticks of 50 ms device chunks through the pool at E = 1 and at E = 64, then the same ticks through the streams)
"""
import argparse
import json
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)

FS, N_FFT, HOP, N_MELS, FLOOR = 22050, 1024, 110, 80, 1e-5
CHUNKS = {10: 220, 50: 1102}            # ms -> samples


def setup(sessions, ticks, chunk):
    import torch
    from shallow_wavenet_amd import melspec
    assert torch.cuda.is_available(), "needs a HIP device"
    ext = melspec.LogMelExtractor(FS, N_FFT, HOP, N_MELS, floor=FLOOR, device="cuda")
    g = torch.Generator().manual_seed(sessions + chunk)
    x = 0.3 * torch.tanh(torch.randn(sessions, ticks * chunk, generator=g))
    return torch, melspec, ext, x


def tick_fns(torch, melspec, ext, x, chunk, on_device):
    """(pool_tick(t), separate_tick(t)) -> list of the sessions' (1, n_mels, k) frames of tick t"""
    E = x.shape[0]
    src = x.cuda() if on_device else x
    pool = melspec.LogMelPool(ext, capacity=E, max_chunk=chunk)
    sess = [pool.open() for _ in range(E)]
    streams = [melspec.LogMelStream(ext) for _ in range(E)]

    def pool_tick(t):
        new = pool.push_many({s: src[e, t * chunk:(t + 1) * chunk] for e, s in enumerate(sess)})
        return [new[s] for s in sess]

    def separate_tick(t):
        return [st.push(src[e, t * chunk:(t + 1) * chunk]).t()[None].contiguous() for e, st in enumerate(streams)]

    return pool_tick, separate_tick


def timed(torch, fn, t):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    ev0.record()
    out = fn(t)
    ev1.record()
    torch.cuda.synchronize()
    w1 = time.perf_counter()
    return ev0.elapsed_time(ev1), (w1 - w0) * 1e3, out


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def decode_side(sessions, chunk_ms, on):
    """the push_many front end and the decode tick of the same E and chunk size, as profiles/pool_frontend_timing.json has them"""
    path = os.path.join(_R, "profiles", "pool_frontend_timing.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        rows = json.load(f).get("rows", [])
    for r in rows:
        if (r.get("config"), r.get("pool"), r.get("sessions"), r.get("chunk_ms"), r.get("chunks_on")) == \
                ("bl6_laplace_cfg2", "DecodePool", sessions, chunk_ms, on):
            return {"push_many_ms": r["push_many_ms"], "decode_tick_ms": r["decode_tick_ms"]}
    return None


def measure(ticks, warm):
    rows = []
    for sessions in (1, 64):
        for chunk_ms, chunk in CHUNKS.items():
            for on in ("device", "host"):
                torch, melspec, ext, x = setup(sessions, warm + ticks, chunk)
                pool_tick, separate_tick = tick_fns(torch, melspec, ext, x, chunk, on == "device")
                dev = {"pool": [], "separate": []}
                wall = {"pool": [], "separate": []}
                identical = True
                for t in range(warm + ticks):
                    outs = {}
                    for name, fn in (("pool", pool_tick), ("separate", separate_tick)):
                        d, w, outs[name] = timed(torch, fn, t)
                        if t >= warm:
                            dev[name].append(d)
                            wall[name].append(w)
                    identical = identical and all(torch.equal(a, b) for a, b in zip(outs["pool"], outs["separate"]))
                p, s = statistics.median(dev["pool"]), statistics.median(dev["separate"])
                pw, sw = statistics.median(wall["pool"]), statistics.median(wall["separate"])
                row = {"sessions": sessions, "chunk_ms": chunk_ms, "chunk_samples": chunk, "chunks_on": on, "ticks_measured": ticks,
                       "pool_device": spread(dev["pool"]), "separate_device": spread(dev["separate"]),
                       "pool_wall": spread(wall["pool"]), "separate_wall": spread(wall["separate"]),
                       "device_speedup": round(s / p, 2), "wall_speedup": round(sw / pw, 2),
                       "pool_below_separate_device": p < s, "pool_below_separate_wall": pw < sw, "identical": identical}
                side = decode_side(sessions, chunk_ms, on)
                if side is not None:
                    row["decode_side_bl6_cfg2"] = side
                    row["mel_pool_share_of_tick"] = round(p / (p + side["push_many_ms"] + side["decode_tick_ms"]), 3)
                    row["separate_share_of_tick"] = round(s / (s + side["push_many_ms"] + side["decode_tick_ms"]), 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
    import torch
    return {"geometry": {"fs": FS, "n_fft": N_FFT, "hop": HOP, "n_mels": N_MELS}, "warm_ticks": warm,
            "device": torch.cuda.get_device_name(0), "rows": rows}


def profile_pass(ticks):
    """untimed, for a kernel trace: `ticks` ticks of 50 ms device chunks through the pool at E = 1 and E = 64 (two launches
    per tick: logmel_pool_update_kernel and logmel_kernel<true>), then through the streams (E launches of logmel_kernel<false>
    per tick)"""
    chunk = CHUNKS[50]
    fns = []
    for sessions in (1, 64):
        torch, melspec, ext, x = setup(sessions, ticks, chunk)
        fns.append(tick_fns(torch, melspec, ext, x, chunk, True))
    for which in (0, 1):
        for pair in fns:
            for t in range(ticks):
                pair[which](t)
            torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "logmel_pool_timing.json"))
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    if a.profile_pass:
        profile_pass(10)
        return
    if a.ticks < 7:
        ap.error("at least 7 measured ticks")
    res = measure(a.ticks, a.warm)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
