"""What the wide decode pool launch (DecodePool(launch_width=256), swn_decode_pool_chunk_wide) costs and buys on one MI355X: E
sessions of 1 s each, one chunk (10 ms / 50 ms) of features and of samples per session and tick, through push_many + step.

  narrow   launch_width = 64: the tick's decode is ceil(E / 64) launches of swn_decode_pool_chunk[_w16 / _w8], one after another
  wide     launch_width = 256: ONE swn_decode_pool_chunk_wide call (ceil(E / 64) setup launches of 64 table rows, one decode
           launch of E workgroups).  At E = 64 the same 64 workgroups run either way, so wide - narrow prices the setup launch

Both pools live in one process and are fed the same features; the settings ALTERNATE tick by tick (narrow first in even ticks,
wide first in odd ones), each tick between device events with a device synchronisation in front.  Per setting, over the ticks
in which every session runs a whole chunk (the first --skip ticks, which hold the prologues, and the last one are left out),
median [min - max] of

  decode_ms   the decode launches alone (pool.step)       tick_ms   push_many + step: the front end stays in calls of 64
  host_ms     wall clock the host spends issuing the tick (no synchronisation inside)

Claims, per net, weights and chunk (written next to the rows by --claims):
  a   wide against narrow at E = 256, same run: "faster" only if the wide [min - max] lies below the narrow one's, "slower"
      only if above, else "overlap"
  b   this build's narrow ticks against the parent commit's ([min - max] of --parent): "inside" = unchanged
  c   wide E = 256 over wide E = 64, medians: what 32 workgroups per XCD sharing one L2 cost against 8

    python tools/time_pool_wide.py --out profiles/pool_wide_timing.json
    python tools/time_pool_wide.py --tree <checkout of the parent commit> --narrow-only --out profiles/pool_wide_timing_parent.json
    python tools/time_pool_wide.py --claims profiles/pool_wide_timing.json --parent profiles/pool_wide_timing_parent.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (64, 128, 192, 256)
_NETS: dict = {}


def _stat(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def _configs():
    from shallow_wavenet_amd import config as C
    # (name, cfg, sample rate, weights): variant 0 = the wave-specialised kernel for cfg2, the symmetric one for the softmax net
    return [("bl6_laplace_cfg2", C.bl6_laplace(), 22050, ("fp32",)),
            ("bl6_softmax", C.bl6_softmax(), 16000, ("fp32", "bf16", "e4m3"))]


def _net(name, cfg):
    from shallow_wavenet_amd.runtime import HipNet
    from shallow_wavenet_amd.synth import synth_state_dict
    if name not in _NETS:
        sd = synth_state_dict(cfg, seed=5, flavor="trained" if cfg.kind == "laplace" else "xavier")
        _NETS[name] = HipNet.from_state_dict(cfg, sd, "cuda:0")
    return _NETS[name]


def measure(name, cfg, fs, weights, seconds, chunk_ms, E, widths, skip):
    import torch
    from shallow_wavenet_amd.streaming import DecodePool
    from shallow_wavenet_amd.synth import synth_aux
    seg = 1 if cfg.kind == "softmax" else cfg.seg
    net = _net(name, cfg)
    frames = max(1, int(round(chunk_ms * 1e-3 * fs / cfg.U)))
    F = max(4 * frames, int(round(seconds * fs / cfg.U)))
    steps = frames * cfg.U // seg
    auxs = [torch.from_numpy(synth_aux(cfg, 1, F, seed=10 + i)).cuda() for i in range(16)]
    pools, sess = {}, {}
    for w in widths:
        kw = {} if w == 64 else dict(launch_width=w)             # (the parent commit's pool has no such keyword)
        pools[w] = DecodePool(net, E, rng_seed=1, weights=weights, **kw)
        sess[w] = [pools[w].open(utt_id=i) for i in range(E)]
    rows = {w: [] for w in widths}
    tick, f0 = 0, 0
    while f0 < F:
        f1 = min(F, f0 + frames)
        for w in (widths if tick % 2 == 0 else widths[::-1]):
            pool, ss = pools[w], sess[w]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            pool.push_many({s: auxs[i % 16][:, :, f0:f1] for i, s in enumerate(ss)}, finish=ss if f1 == F else ())
            ev[1].record()
            res = pool.step(steps)
            ev[2].record()
            host = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            rows[w].append((ev[1].elapsed_time(ev[2]), ev[0].elapsed_time(ev[2]), ev[0].elapsed_time(ev[1]), host, len(res)))
        f0, tick = f1, tick + 1
    out = dict(config=name, weights=weights, chunk_ms=chunk_ms, chunk_frames=frames, chunk_steps=steps, sessions=E,
               seconds=seconds, variant=pools[widths[0]].resolved_variant)
    for w in widths:
        kept = rows[w][skip:-1] if len(rows[w]) > skip + 1 else rows[w]
        assert all(r[4] == E for r in kept), "a measured tick did not run every session"
        out["narrow" if w == 64 else "wide"] = dict(
            launch_width=w, decode_launches=-(-E // w), decode_ms=_stat([r[0] for r in kept]), tick_ms=_stat([r[1] for r in kept]),
            frontend_ms=_stat([r[2] for r in kept]), host_ms=_stat([r[3] for r in kept]), ticks_measured=len(kept))
    return out


def _key(r):
    return (r["config"], r["weights"], r["chunk_ms"])


def _against(x, y):
    """x's [min - max] against y's"""
    return "below" if x["max"] < y["min"] else "above" if x["min"] > y["max"] else "overlap"


def claims(rows, parent_rows):
    by = {(_key(r), r["sessions"]): r for r in rows}
    par = {(_key(r), r["sessions"]): r for r in parent_rows or []}
    out = []
    for k in sorted({_key(r) for r in rows}):
        c = dict(config=k[0], weights=k[1], chunk_ms=k[2])
        big, small = by.get((k, 256)), by.get((k, 64))
        if big and "wide" in big:
            for what in ("decode_ms", "tick_ms"):
                rel = _against(big["wide"][what], big["narrow"][what])
                c[f"a_{what}"] = dict(wide=big["wide"][what], narrow=big["narrow"][what],
                                      verdict={"below": "faster", "above": "slower"}.get(rel, rel),
                                      ratio_of_medians=round(big["narrow"][what]["median"] / big["wide"][what]["median"], 3))
        if par:
            c["b_narrow_vs_parent"] = {}
            for E in SIZES:
                if (k, E) in by and (k, E) in par:
                    m, p = by[(k, E)]["narrow"]["decode_ms"], par[(k, E)]["narrow"]["decode_ms"]
                    c["b_narrow_vs_parent"][str(E)] = dict(
                        median=m["median"], parent=p, verdict="inside" if p["min"] <= m["median"] <= p["max"] else
                        ("below" if m["median"] < p["min"] else "above"))
        if big and small and "wide" in big and "wide" in small:
            c["c_wide_256_over_wide_64"] = round(big["wide"]["decode_ms"]["median"] / small["wide"]["decode_ms"]["median"], 3)
            c["setup_cost_ms_at_64"] = round(small["wide"]["decode_ms"]["median"] - small["narrow"]["decode_ms"]["median"], 4)
        out.append(c)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="audio per session")
    ap.add_argument("--chunks", default="10,50", help="chunk lengths in ms")
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES), help="sessions per pool")
    ap.add_argument("--only", default=None, help="one configuration name")
    ap.add_argument("--weights", default=None, help="one weight format")
    ap.add_argument("--skip", type=int, default=3, help="leading ticks left out")
    ap.add_argument("--narrow-only", action="store_true", help="launch_width = 64 alone (the parent commit's run)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose shallow_wavenet_amd is measured")
    ap.add_argument("--out", default=None)
    ap.add_argument("--claims", default=None, help="a result file: (re)write its claims, no device needed")
    ap.add_argument("--parent", default=None, help="with --claims: the parent commit's result file")
    a = ap.parse_args()
    if a.claims:
        with open(a.claims) as f:
            doc = json.load(f)
        parent = None
        if a.parent:
            with open(a.parent) as f:
                parent = json.load(f)["rows"]
        doc["claims"] = claims(doc["rows"], parent)
        with open(a.claims, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    widths = (64,) if a.narrow_only else (64, 256)
    rows = []
    for name, cfg, fs, formats in _configs():
        if a.only and a.only != name:
            continue
        for weights in formats:
            if a.weights and a.weights != weights:
                continue
            for chunk_ms in [int(x) for x in a.chunks.split(",")]:
                for E in [int(x) for x in a.sizes.split(",")]:
                    r = measure(name, cfg, fs, weights, a.seconds, chunk_ms, E, widths, a.skip)
                    print(json.dumps(r), flush=True)
                    rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), narrow_only=a.narrow_only,
                           rows=rows, claims=claims(rows, None)), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
