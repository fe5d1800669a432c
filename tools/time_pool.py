"""Decode pool against separate streams on one MI355X: E sessions of `--seconds` of audio each, advanced one chunk
(10 ms / 50 ms of audio) per tick, session i starting at tick i % 4.  Per configuration, chunk length and E:

  pool_tick_ms          DecodePool.step of one tick (conditioning already final), device events, median over the ticks in
                        which every session runs
  pool_samples_per_s    E * chunk samples / pool_tick_ms
  rtf_per_session       pool_tick_ms / chunk duration: < 1 keeps every session ahead of real time
  tick_ratio_vs_e1      pool_tick_ms / the E = 1 pool_tick_ms of the same configuration and chunk
  streams_tick_ms       the same tick as E DecodeStream.advance calls one after another on one stream (first --stream_ticks
                        ticks), and streams_samples_per_s;  pool_speedup = streams_tick_ms / pool_tick_ms
  frontend_ms_per_tick  the E PoolSession.push calls of one chunk of features each (one swn_frontend per session), device
                        events, median; frontend_share = frontend / (frontend + pool tick)

    python tools/time_pool.py [--seconds 2] [--out profiles/pool_timing.json]
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
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream  # noqa: E402
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict  # noqa: E402

CONFIGS = [("bl6_laplace_cfg2", C.bl6_laplace(), 22050), ("bl6_softmax", C.bl6_softmax(), 16000)]
STAGGER = 4


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def _ms(evs):
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def measure(name, cfg, fs, seconds, chunk_ms, E, stream_ticks, pool_only=False):
    seg = 1 if cfg.kind == "softmax" else cfg.seg
    net = measure.nets.get(name)
    if net is None:
        sd = synth_state_dict(cfg, seed=5, flavor="trained" if cfg.kind == "laplace" else "xavier")
        net = measure.nets[name] = HipNet.from_state_dict(cfg, sd, "cuda:0")
    F = max(4, int(round(seconds * fs / cfg.U)))
    frames = max(1, int(round(chunk_ms * 1e-3 * fs / cfg.U)))
    steps = frames * cfg.U // seg
    auxs = [torch.from_numpy(synth_aux(cfg, 1, F, seed=10 + i)).cuda() for i in range(E)]
    n_ticks = -(-F // frames) + STAGGER

    # pool, conditioning final up front: the decode launches alone
    pool = DecodePool(net, E, rng_seed=1)
    sess = [None] * E
    evs, full = [], []
    for t in range(n_ticks):
        for i in range(E):
            if sess[i] is None and i % STAGGER == t:
                sess[i] = pool.open()
                sess[i].finish(auxs[i])
        torch.cuda.synchronize()
        evs.append(_timed(lambda: pool.step(steps)))
        full.append(all(s is not None and s.steps_done < s.steps_ready for s in sess))
    ticks = _ms(evs)
    pool_ms = statistics.median([x for x, f in zip(ticks, full) if f] or ticks)
    chunk_samples = steps * seg
    row = dict(config=name, chunk_ms=chunk_ms, chunk_frames=frames, chunk_steps=steps, sessions=E, seconds=seconds,
               ticks=n_ticks, variant=pool.resolved_variant,
               pool_tick_ms=round(pool_ms, 4), pool_samples_per_s=round(E * chunk_samples / (pool_ms * 1e-3)),
               rtf_per_session=round(pool_ms / (chunk_samples / fs * 1e3), 4))
    if pool_only:
        print(json.dumps(row), flush=True)
        return row

    # pool with the features pushed one chunk per tick: the front end's share
    pool = DecodePool(net, E, rng_seed=1)
    sess = [None] * E
    fe = []
    for t in range(min(n_ticks, stream_ticks + STAGGER)):
        for i in range(E):
            if sess[i] is None and i % STAGGER == t:
                sess[i] = pool.open()

        def pushes():
            for i, s in enumerate(sess):
                if s is not None and not s.finished:
                    f0 = s._stream.frames_received
                    if f0 + frames >= F:
                        s.finish(auxs[i][:, :, f0:])
                    else:
                        s.push(auxs[i][:, :, f0:f0 + frames])
        torch.cuda.synchronize()
        if t >= STAGGER:
            fe.append(_timed(pushes))
        else:
            pushes()
        pool.step(steps)
    fe_ms = statistics.median(_ms(fe))

    # the same load as E separate DecodeStreams, one after another on one stream
    streams = []
    for i in range(E):
        s = DecodeStream(net, 1, rng_seed=1, utt_ids=[i])
        s.push(auxs[i], generate=False)
        s.finish(generate=False)
        streams.append(s)
    evs = []
    for t in range(stream_ticks):
        torch.cuda.synchronize()
        evs.append(_timed(lambda: [s.advance(min(steps, s.steps_ready - s.steps_done)) for s in streams]))
    st_ms = statistics.median(_ms(evs))

    row.update(streams_tick_ms=round(st_ms, 4), streams_samples_per_s=round(E * chunk_samples / (st_ms * 1e-3)),
               pool_speedup=round(st_ms / pool_ms, 3), streams_ticks_measured=stream_ticks,
               frontend_ms_per_tick=round(fe_ms, 4), frontend_share=round(fe_ms / (fe_ms + pool_ms), 4))
    print(json.dumps(row), flush=True)
    return row


measure.nets = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="audio per session")
    ap.add_argument("--sessions", default="1,8,32,64")
    ap.add_argument("--stream_ticks", type=int, default=40, help="ticks measured for the separate-streams comparison")
    ap.add_argument("--only", default=None, help="one configuration name")
    ap.add_argument("--chunks", default="10,50", help="chunk lengths in ms")
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
                r = measure(name, cfg, fs, a.seconds, chunk_ms, E, a.stream_ticks, a.pool_only)
                base = r["pool_tick_ms"] if E == 1 else base
                r["tick_ratio_vs_e1"] = round(r["pool_tick_ms"] / base, 4) if base else None
                rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), stagger_ticks=STAGGER, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
