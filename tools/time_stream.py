"""Streamed decode against the one-shot decode on one MI355X: per configuration and chunk length (10 ms / 50 ms of audio)

  oneshot_us_per_step   HipNet.decode over the whole utterance (device noise), µs per generation step
  stream_us_per_step    the same steps as DecodeStream.advance chunks over final conditioning, µs per step
  ratio                 stream / one-shot
  chunk_overhead_us     (stream - one-shot) time per chunk: launch(es), weight reload, state load and save
  push_to_ready_us      DecodeStream.push of one chunk of features (front end + steps) until its samples are on the
                        device, stream idle before the push (median over the pushes)

    python tools/time_stream.py [--seconds 2] [--out profiles/stream.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from shallow_wavenet_amd import config as C  # noqa: E402
from shallow_wavenet_amd.runtime import HipNet  # noqa: E402
from shallow_wavenet_amd.streaming import DecodeStream  # noqa: E402
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict  # noqa: E402

CONFIGS = [("bl6_laplace_cfg2", C.bl6_laplace(), 22050), ("bl6_softmax", C.bl6_softmax(), 16000),
           ("ref6_laplace", C.ref6_laplace(), 22050)]


def _events_ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def measure(name, cfg, fs, seconds, reps):
    seg = 1 if cfg.kind == "softmax" else cfg.seg
    sd = synth_state_dict(cfg, seed=5, flavor="trained" if cfg.kind == "laplace" else "xavier")
    net = HipNet.from_state_dict(cfg, sd, "cuda:0")
    F = max(4, int(round(seconds * fs / cfg.U)))
    aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=3)).cuda()
    N = F * cfg.U // seg
    cond = net.frontend(aux)
    net.decode(aux, N, cond=cond, rng_seed=1)                                    # warm-up (code objects, allocator)
    one_ms = _events_ms(lambda: net.decode(aux, N, cond=cond, rng_seed=1), reps)
    rows = []
    for chunk_ms in (10, 50):
        frames = max(1, int(round(chunk_ms * 1e-3 * fs / cfg.U)))
        steps = frames * cfg.U // seg

        def streamed():
            s = DecodeStream(net, 1, rng_seed=1)
            s.push(aux, generate=False)
            s.finish(generate=False)
            for k in range(0, N, steps):
                s.advance(min(steps, N - k))
        streamed()
        st_ms = _events_ms(streamed, reps)
        # the part of `streamed` that is not decode: the front end of the two pushes (measured alone)
        def fe_only():
            s = DecodeStream(net, 1, rng_seed=1)
            s.push(aux, generate=False)
            s.finish(generate=False)
        fe_ms = _events_ms(fe_only, reps)
        n_chunks = -(-N // steps)
        dec_ms = st_ms - fe_ms
        # push -> samples ready: features of one chunk at a time, the device idle before each push
        s = DecodeStream(net, 1, rng_seed=1)
        lat = []
        for f0 in range(0, F, frames):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.push(aux[:, :, f0:f0 + frames])
            torch.cuda.synchronize()
            lat.append((time.perf_counter() - t0) * 1e6)
        s.finish()
        torch.cuda.synchronize()
        rows.append(dict(config=name, chunk_ms=chunk_ms, chunk_frames=frames, chunk_steps=steps, n_steps=N, n_chunks=n_chunks,
                         oneshot_us_per_step=round(one_ms * 1e3 / N, 4), stream_us_per_step=round(dec_ms * 1e3 / N, 4),
                         ratio=round(dec_ms / one_ms, 4), chunk_overhead_us=round((dec_ms - one_ms) * 1e3 / n_chunks, 2),
                         push_to_ready_us=round(statistics.median(lat[2:] or lat), 1),
                         variant=s.resolved_variant))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="audio per utterance")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="one configuration name")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name, cfg, fs in CONFIGS:
        if a.only and a.only != name:
            continue
        rows += measure(name, cfg, fs, a.seconds if not name.startswith("ref6") else min(a.seconds, 1.0), a.reps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
