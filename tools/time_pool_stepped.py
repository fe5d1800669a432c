"""Stepped decode pool on one MI355X (REF6, the run.sh geometry): E sessions advanced one chunk (10 ms / 50 ms of audio)
per tick, conditioning final up front.  Per configuration, chunk length and E:

  pool_tick_ms          SteppedDecodePool.step of one tick in which every session generates a chunk (prologues already
                        run), device events, median over --ticks ticks;  us_per_step = pool_tick_ms / chunk steps
  tick_ratio_vs_e1      pool_tick_ms / the E = 1 pool_tick_ms of the same configuration and chunk
  stream_tick_ms        one batch-1 DecodeStream.advance of the same chunk (variant 3);  e1_vs_stream = the E = 1 pool tick
                        over it
  streams_tick_ms       the tick as E DecodeStream.advance calls one after another on one stream;  pool_speedup =
                        streams_tick_ms / pool_tick_ms
  generic_pool_ms_per_step  (E = 8) DecodePool(variant=1), the generic persistent kernel, at --generic_steps steps per tick
  begin_tick_ms         a tick in which one session begins (its whole prologue) while E - 1 generate a chunk;
  begin_tick_ms_maxpro  the same with max_prologue = --max_prologue (the first of the ticks that spread it)

    python tools/time_pool_stepped.py [--out profiles/pool_stepped_timing.json]
    python tools/time_pool_stepped.py --pool_only --only ref6_laplace_s1 --sessions 64 --chunks 10   (for a kernel trace)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from shallow_wavenet_amd import config as C  # noqa: E402
from shallow_wavenet_amd.runtime import HipNet  # noqa: E402
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream, SteppedDecodePool  # noqa: E402
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict  # noqa: E402

CONFIGS = [("ref6_laplace_s1", C.ref6_laplace(1, 4), 22050), ("ref6_softmax", C.ref6_softmax(), 22050)]


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def _ms(evs):
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def _net(name, cfg):
    net = _net.cache.get(name)
    if net is None:
        sd = synth_state_dict(cfg, seed=5, flavor="trained" if cfg.kind == "laplace" else "xavier")
        net = _net.cache[name] = HipNet.from_state_dict(cfg, sd, "cuda:0")
    return net


_net.cache = {}


def measure(name, cfg, fs, chunk_ms, E, a):
    seg = 1 if cfg.kind == "softmax" else cfg.seg
    net = _net(name, cfg)
    frames = max(1, int(round(chunk_ms * 1e-3 * fs / cfg.U)))
    steps = frames * cfg.U // seg
    F = frames * (a.ticks + 4) + 1
    auxs = [torch.from_numpy(synth_aux(cfg, 1, F, seed=10 + i)).cuda() for i in range(E + 2)]

    pool = SteppedDecodePool(net, E, rng_seed=1)
    sess = []
    for i in range(E):
        s = pool.open()
        s.finish(auxs[i])
        sess.append(s)
    pool.step(steps)                                           # every prologue and the first chunk
    torch.cuda.synchronize()
    evs = [_timed(lambda: pool.step(steps)) for _ in range(a.ticks)]
    pool_ms = statistics.median(_ms(evs))
    row = dict(config=name, chunk_ms=chunk_ms, chunk_frames=frames, chunk_steps=steps, sessions=E, ticks=a.ticks,
               pool_tick_ms=round(pool_ms, 4), us_per_step=round(pool_ms * 1e3 / steps, 2),
               pool_samples_per_s=round(E * steps * seg / (pool_ms * 1e-3)))
    if a.pool_only:
        print(json.dumps(row), flush=True)
        return row

    # a session begins: its whole prologue in the tick, then (a new one again) spread by max_prologue
    pool.close(sess[0])
    s = pool.open()
    s.finish(auxs[E])
    torch.cuda.synchronize()
    row["begin_tick_ms"] = round(_ms([_timed(lambda: pool.step(steps))])[0], 4)
    pool.close(sess[1] if E > 1 else s)
    s = pool.open()
    s.finish(auxs[E + 1])
    torch.cuda.synchronize()
    row["begin_tick_ms_maxpro"] = round(_ms([_timed(lambda: pool.step(steps, max_prologue=a.max_prologue))])[0], 4)
    row["max_prologue"] = a.max_prologue
    del pool

    # the same load as E separate batch-1 DecodeStreams, one after another on one stream
    streams = []
    for i in range(E):
        st = DecodeStream(net, 1, variant=3, rng_seed=1, utt_ids=[i])
        st.push(auxs[i], generate=False)
        st.finish(generate=False)
        st.advance(steps)
        streams.append(st)
    torch.cuda.synchronize()
    evs = [_timed(lambda: [st.advance(steps) for st in streams]) for _ in range(a.stream_ticks)]
    st_ms = statistics.median(_ms(evs))
    one = statistics.median(_ms([_timed(lambda: streams[0].advance(steps)) for _ in range(a.stream_ticks)]))
    del streams
    row.update(streams_tick_ms=round(st_ms, 4), pool_speedup=round(st_ms / pool_ms, 3), stream_tick_ms=round(one, 4))

    if E == 8:
        gp = DecodePool(net, E, variant=1, rng_seed=1)
        for i in range(E):
            gs = gp.open()
            gs.finish(auxs[i])
        gp.step(1)
        torch.cuda.synchronize()
        g_ms = statistics.median(_ms([_timed(lambda: gp.step(a.generic_steps)) for _ in range(2)]))
        row.update(generic_pool_tick_ms=round(g_ms, 4), generic_pool_steps=a.generic_steps,
                   generic_pool_ms_per_step=round(g_ms / a.generic_steps, 4),
                   generic_vs_stepped_per_step=round((g_ms / a.generic_steps) / (pool_ms / steps), 2))
        del gp
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,8,24,64")
    ap.add_argument("--chunks", default="10,50", help="chunk lengths in ms")
    ap.add_argument("--ticks", type=int, default=5, help="pool ticks measured")
    ap.add_argument("--stream_ticks", type=int, default=2, help="ticks measured for the separate-streams comparison")
    ap.add_argument("--generic_steps", type=int, default=20)
    ap.add_argument("--max_prologue", type=int, default=100)
    ap.add_argument("--only", default=None, help="one configuration name")
    ap.add_argument("--pool_only", action="store_true", help="only the pool ticks (a kernel trace of the pool alone)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name, cfg, fs in CONFIGS:
        if a.only and a.only != name:
            continue
        for chunk_ms in [int(x) for x in a.chunks.split(",")]:
            base = None
            for E in [int(x) for x in a.sessions.split(",")]:
                r = measure(name, cfg, fs, chunk_ms, E, a)
                base = r["pool_tick_ms"] if E == 1 else base
                r["tick_ratio_vs_e1"] = round(r["pool_tick_ms"] / base, 4) if base else None
                if E == 1 and "stream_tick_ms" in r:
                    r["e1_vs_stream"] = round(r["pool_tick_ms"] / r["stream_tick_ms"], 4)
                rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
