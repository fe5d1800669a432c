"""The front end of a decode pool's tick on one MI355X: E sessions receive one chunk of features (10 ms / 50 ms of audio) per
tick, session i starting at tick i % 4.  Two pools on one net get identical chunks, alternating tick by tick in one process:

  pool A   E PoolSession.push calls (one swn_frontend and its copies per session): the baseline
  pool B   one DecodePool.push_many (one staging copy, one swn_frontend_pool), then the tick's decode launch pool.step

Per configuration, chunk length, E and where the chunks lie (device / host), medians over the measured ticks in which every
session pushes:

  separate_ms / push_many_ms                 device events around the calls of one tick
  separate_wall_ms / push_many_wall_ms       host wall clock of the calls and a trailing synchronise
  separate_enqueue_ms / push_many_enqueue_ms host wall clock of the calls alone
  decode_tick_ms                             device events around pool B's pool.step of the same tick
  push_many_over_decode                      push_many_ms / decode_tick_ms (< 1: the front end is under half of the tick)
  frontend_share                             push_many_ms / (push_many_ms + decode_tick_ms)
  speedup, wall_speedup                      separate / push_many
  push_many_vs_e1                            push_many_ms / the E = 1 push_many_ms of the same configuration, chunk and place

    python tools/time_pool_frontend.py [--seconds 2] [--out profiles/pool_frontend_timing.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/time_pool_frontend.py --trace 64      # pool B alone, buffers pre-sized
    python tools/time_pool_frontend.py --merge_stats 1=a_kernel_stats.csv 64=b_kernel_stats.csv --out profiles/...csv
    python tools/time_pool_frontend.py --launches 1=a_kernel_trace.csv 64=b_kernel_trace.csv --out profiles/...json
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from shallow_wavenet_amd import _lib, config as C, ops  # noqa: E402
from shallow_wavenet_amd.runtime import HipNet  # noqa: E402
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream, SteppedDecodePool  # noqa: E402
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict  # noqa: E402

# the configurations of tools/time_pool.py and REF6 Laplace (the stepped pool)
CONFIGS = [("bl6_laplace_cfg2", C.bl6_laplace(), 22050), ("bl6_softmax", C.bl6_softmax(), 16000),
           ("ref6_laplace", C.ref6_laplace(), 22050)]
STAGGER = 4
WARM = 3                                       # unmeasured ticks after the last admission
NETS: dict = {}


def _net(name, cfg):
    if name not in NETS:
        sd = synth_state_dict(cfg, seed=5, flavor="trained" if cfg.kind == "laplace" else "xavier")
        NETS[name] = HipNet.from_state_dict(cfg, sd, "cuda:0")
    return NETS[name]


def _pool(net, capacity):
    """what open_pool of the modules gives: the stepped pool where the decode resolves to the stepped chain"""
    if _lib.lib().swn_decode_resolve_variant(ops._desc(net.dlist), capacity, 0) == 3:
        return SteppedDecodePool(net, capacity, rng_seed=1)
    return DecodePool(net, capacity, rng_seed=1)


def _timed(fn):
    """fn under device events and the host clock: (events, enqueue ms, ms with a trailing synchronise)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return a.elapsed_time(b), (t1 - t0) * 1e3, (t2 - t0) * 1e3


def _chunks(cfg, E, F, frames, where):
    """per session, its features cut into contiguous chunks (what a server receives), on the device or the host"""
    out = []
    for i in range(E):
        a = torch.from_numpy(synth_aux(cfg, 1, F, seed=10 + i))
        if where == "device":
            a = a.cuda()
        out.append([a[:, :, f:f + frames].contiguous() for f in range(0, F, frames)])
    return out


def measure(name, cfg, fs, seconds, chunk_ms, E, where, ticks):
    seg = 1 if cfg.kind == "softmax" else cfg.seg
    net = _net(name, cfg)
    F = max(4, int(round(seconds * fs / cfg.U)))
    frames = max(1, int(round(chunk_ms * 1e-3 * fs / cfg.U)))
    steps = frames * cfg.U // seg
    chunks = _chunks(cfg, E, F, frames, where)
    n_chunks = len(chunks[0])
    pa, pb = _pool(net, E), _pool(net, E)
    sa, sb = [None] * E, [None] * E
    sent = [0] * E
    rows = []
    for t in range(min(n_chunks + STAGGER, STAGGER + WARM + ticks)):
        for i in range(E):
            if sa[i] is None and i % STAGGER == t:
                sa[i], sb[i] = pa.open(), pb.open()
        todo = [(i, chunks[i][sent[i]], sent[i] == n_chunks - 1) for i in range(E) if sa[i] is not None and sent[i] < n_chunks]
        full = len(todo) == E

        def separate():
            for i, c, last in todo:
                (sa[i].finish if last else sa[i].push)(c)

        def batched():
            pb.push_many({sb[i]: c for i, c, _ in todo}, finish=[sb[i] for i, _, last in todo if last])

        r = (_timed(separate), _timed(batched), _timed(lambda: pb.step(steps)))
        for i, _, _ in todo:
            sent[i] += 1
        if full and t >= STAGGER + WARM:
            rows.append(r)
    for i in range(E):                                       # the two pools stand alike
        assert sa[i]._stream.frames_final == sb[i]._stream.frames_final
        assert torch.equal(sa[i]._stream.cond, sb[i]._stream.cond)
    med = lambda k, j: statistics.median(r[k][j] for r in rows)
    sep, many, dec = med(0, 0), med(1, 0), med(2, 0)
    row = dict(config=name, chunk_ms=chunk_ms, chunk_frames=frames, sessions=E, chunks_on=where, seconds=seconds,
               ticks_measured=len(rows), pool=type(pb).__name__,
               separate_ms=round(sep, 4), push_many_ms=round(many, 4), decode_tick_ms=round(dec, 4),
               separate_wall_ms=round(med(0, 2), 4), push_many_wall_ms=round(med(1, 2), 4),
               separate_enqueue_ms=round(med(0, 1), 4), push_many_enqueue_ms=round(med(1, 1), 4),
               push_many_over_decode=round(many / dec, 4), frontend_share=round(many / (many + dec), 4),
               separate_share=round(sep / (sep + dec), 4), speedup=round(sep / many, 3),
               wall_speedup=round(med(0, 2) / med(1, 2), 3))
    print(json.dumps(row), flush=True)
    return row


def trace(E, calls):
    """pool B alone for a kernel trace: BL6 Laplace, 10 ms chunks on the device, `calls` push_many calls of E sessions each with
    the session buffers sized up front (no growth copies), one pool.step per call"""
    name, cfg, fs = CONFIGS[0]
    net = _net(name, cfg)
    frames = max(1, int(round(10e-3 * fs / cfg.U)))
    F = frames * (calls + 2)
    chunks = _chunks(cfg, E, F, frames, "device")
    pool = _pool(net, E)
    sess = [pool.open() for _ in range(E)]
    N = cfg.L * 2 * cfg.H
    for s in sess:
        s._stream._aux = DecodeStream._grow(None, 2, F, (1, cfg.n_aux, 0), net.device)
        s._stream._cond = DecodeStream._grow(None, 1, F, (1, 0, N), net.device)
    torch.cuda.synchronize()
    for t in range(calls):
        pool.push_many({s: chunks[i][t] for i, s in enumerate(sess)})
        pool.step(frames * cfg.U)
    torch.cuda.synchronize()
    print(json.dumps(dict(trace_sessions=E, push_many_calls=calls)), flush=True)


def merge_stats(parts, out):
    """kernel-stats CSVs of separate traced runs -> one CSV with the run's session count in front"""
    with open(out, "w", newline="") as f:
        w = None
        for part in parts:
            E, path = part.split("=", 1)
            with open(path, newline="") as g:
                for k, line in enumerate(csv.reader(g)):
                    if k == 0:
                        if w is None:
                            w = csv.writer(f)
                            w.writerow(["sessions"] + line)
                        continue
                    w.writerow([E] + line)


def _short(name):
    """a kernel's name without its arguments, namespaces and at::native wrappers' template text"""
    name = name.replace("(anonymous namespace)::", "").replace("void ", "").strip()
    return name.split("(")[0].split("<")[0].split("::")[-1] or "?"


def launches(parts, out):
    """kernel-trace CSVs (E=path) of --trace runs -> JSON: per run, the kernels launched between two decode launches of
    consecutive ticks (one push_many each), in launch order, as distinct sequences with the number of ticks that show each"""
    res = {}
    for part in parts:
        E, path = part.split("=", 1)
        with open(path, newline="") as g:
            rows = sorted(csv.DictReader(g), key=lambda r: int(r["Start_Timestamp"]))
        names = [_short(r["Kernel_Name"]) for r in rows]
        dec = [i for i, n in enumerate(names) if n.startswith("decode_") and "pool" in n]
        seqs = {}
        for a, b in zip(dec, dec[1:]):
            seq = names[a + 1:b]
            if any(n.startswith("fp_") for n in seq):
                key = " ".join(seq)
                seqs[key] = seqs.get(key, 0) + 1
        res[E] = dict(sessions=int(E), decode_launches=len(dec),
                      between_decode_launches=[dict(ticks=v, launches=len(k.split()),
                                                    front_end_launches=sum(n.startswith("fp_") for n in k.split()),
                                                    kernels=k.split()) for k, v in sorted(seqs.items(), key=lambda x: -x[1])])
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="audio per session")
    ap.add_argument("--sessions", default="1,8,32,64")
    ap.add_argument("--chunks", default="10,50", help="chunk lengths in ms")
    ap.add_argument("--ticks", type=int, default=40, help="measured ticks per case")
    ap.add_argument("--only", default=None, help="one configuration name")
    ap.add_argument("--trace", type=int, default=0, help="E: only pool B's ticks at E sessions, for rocprofv3")
    ap.add_argument("--trace_calls", type=int, default=50)
    ap.add_argument("--merge_stats", nargs="*", default=None, help="E=path of kernel-stats CSVs to merge into --out")
    ap.add_argument("--launches", nargs="*", default=None, help="E=path of kernel-trace CSVs: launches per push_many into --out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge_stats:
        return merge_stats(a.merge_stats, a.out)
    if a.launches:
        return launches(a.launches, a.out)
    if a.trace:
        return trace(a.trace, a.trace_calls)
    rows = []
    for name, cfg, fs in CONFIGS:
        if a.only and a.only != name:
            continue
        for where in ("device", "host"):
            for chunk_ms in [int(x) for x in a.chunks.split(",")]:
                base = None
                for E in [int(x) for x in a.sessions.split(",")]:
                    r = measure(name, cfg, fs, a.seconds, chunk_ms, E, where, a.ticks)
                    base = r["push_many_ms"] if E == 1 else base
                    r["push_many_vs_e1"] = round(r["push_many_ms"] / base, 4) if base else None
                    rows.append(r)
    pick = [r for r in rows if r["config"] == CONFIGS[0][0] and r["sessions"] == 64 and r["chunk_ms"] == 10]
    conditions = [dict(chunks_on=r["chunks_on"],
                       push_many_device_below_decode_tick=r["push_many_ms"] < r["decode_tick_ms"],
                       push_many_wall_below_separate_wall=r["push_many_wall_ms"] < r["separate_wall_ms"]) for r in pick]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), stagger_ticks=STAGGER, warm_ticks=WARM,
                           conditions_bl6_laplace_e64_10ms=conditions, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
