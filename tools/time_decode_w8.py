"""fp32, bf16 and e4m3 storage of the streamed head matrices (HipNet.decode(weights=...)) on one MI355X, same process,
settings alternating inside every repetition, medians with every repetition listed.

  one-shot   us per generation step = (t(N steps) - t(N / 2 steps)) / (N / 2) of one utterance at the shapes of the bf16 row
             (BL6 softmax Tf = 600: 48 000 steps; BL6 Laplace seg 5 lpc 4 Tf = 600: 13 200 steps; seg 1 lpc 4 Tf = 600:
             66 000 steps), device events.  Settings: fp32_host (host-drawn noise: the classic instantiation the bench legs
             time), fp32, bf16 and e4m3 (device noise: the extended instantiations, which is what the two modes have); the
             single-sample net also lists the wave-specialised fp32 kernel (variant 0), the one to use there.
  pool       one tick of a 64-session softmax DecodePool at 10 ms and 50 ms chunks (conditioning final, every session
             running), the pools of the modes ticking in turn.

    python tools/time_decode_w8.py [--reps 7] [--modes fp32,bf16,e4m3] [--only NAME] [--tree DIR]
                                   [--out profiles/decode_w8_timing.json]

--modes never names a mode it was not given, and --tree imports the package from another checkout, so
`--modes fp32,bf16 --tree <parent checkout>` times the parent commit's kernels with this tool (to show they did not move).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--seconds", type=float, default=1.0, help="audio per pool session")
ap.add_argument("--sessions", type=int, default=64)
ap.add_argument("--modes", default="fp32,bf16,e4m3")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--only", default="", help="run the workloads whose name contains this (pool: bl6_softmax_pool)")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args() if __name__ == "__main__" else ap.parse_args([])
sys.path.insert(0, os.path.abspath(ARGS.tree))

import torch  # noqa: E402

from shallow_wavenet_amd import config as C  # noqa: E402
from shallow_wavenet_amd import noise as NZ  # noqa: E402
from shallow_wavenet_amd.runtime import HipNet  # noqa: E402
from shallow_wavenet_amd.streaming import DecodePool  # noqa: E402
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict  # noqa: E402

# (label, weights, variant, host noise)
ONE_SHOT = [
    ("cfg1_bl6_softmax", C.bl6_softmax(), 600,
     [("fp32_host", "fp32", 0, True), ("fp32", "fp32", 0, False), ("bf16", "bf16", 0, False), ("e4m3", "e4m3", 0, False)]),
    ("cfg3_bl6_laplace_s5l4", C.bl6_laplace(5, 4), 600,
     [("fp32_host", "fp32", 0, True), ("fp32", "fp32", 0, False), ("bf16", "bf16", 0, False), ("e4m3", "e4m3", 0, False)]),
    ("bl6_laplace_s1l4", C.bl6_laplace(1, 4), 600,
     [("fp32_symmetric", "fp32", 6, False), ("bf16_symmetric", "bf16", 6, False), ("e4m3_symmetric", "e4m3", 6, False),
      ("fp32_wave_specialised", "fp32", 0, False)]),
]


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _summary(xs, nd=3):
    return dict(median=round(statistics.median(xs), nd), min=round(min(xs), nd), max=round(max(xs), nd),
                reps=[round(x, nd) for x in xs])


def one_shot(name, cfg, Tf, settings, reps, modes):
    seg = 1 if cfg.kind == "softmax" else cfg.seg
    flavor = "trained" if cfg.kind == "laplace" else "xavier"
    net = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=5, flavor=flavor), "cuda:0")
    aux = torch.from_numpy(synth_aux(cfg, 1, Tf, seed=3)).cuda()
    cond = net.frontend(aux)
    N = Tf * cfg.U // seg
    half = N // 2
    g = torch.Generator().manual_seed(1)
    host = (NZ.softmax_exponential(cfg, N, 1, generator=g) if cfg.kind == "softmax" else NZ.laplace_uniform(cfg, N, 1, generator=g)).cuda()
    settings = [s for s in settings if s[1] in modes]

    def run(weights, variant, host_noise, n):
        kw = dict(cond=cond, variant=variant, rng_seed=9)
        if weights != "fp32":
            kw["weights"] = weights
        net.decode(aux, n, host[:, :n].contiguous() if host_noise else None, **kw)

    us = {s[0]: [] for s in settings}
    for label, w, v, hn in settings:                         # warm-up: code objects, the images
        run(w, v, hn, 256)
    torch.cuda.synchronize()
    for _ in range(reps):
        for label, w, v, hn in settings:
            full = _event_ms(lambda: run(w, v, hn, N))
            part = _event_ms(lambda: run(w, v, hn, half))
            us[label].append((full - part) * 1e3 / (N - half))
    row = dict(workload=name, steps=N, frames=Tf, us_per_step={k: _summary(v) for k, v in us.items()})
    print(json.dumps(row), flush=True)
    return row


def pool_ticks(chunk_ms, E, seconds, modes, fs=16000):
    cfg = C.bl6_softmax()
    net = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=5, flavor="xavier"), "cuda:0")
    F = max(4, int(round(seconds * fs / cfg.U)))
    frames = max(1, int(round(chunk_ms * 1e-3 * fs / cfg.U)))
    steps = frames * cfg.U
    auxs = [torch.from_numpy(synth_aux(cfg, 1, F, seed=10 + i)).cuda() for i in range(E)]
    pools = {}
    for m in modes:
        pools[m] = DecodePool(net, E, rng_seed=1, **({"weights": m} if m != "fp32" else {}))
        for i in range(E):
            pools[m].open().finish(auxs[i])
        pools[m].step(1)                                     # the prologue tick (and the image) stays out of the figures
    n_ticks = (F * cfg.U - 1) // steps
    ms = {m: [] for m in modes}
    for t in range(n_ticks):
        order = modes[t % len(modes):] + modes[:t % len(modes)]          # every mode takes every place in turn
        for m in order:
            torch.cuda.synchronize()
            ms[m].append(_event_ms(lambda: pools[m].step(steps)))
    row = dict(workload="bl6_softmax_pool", sessions=E, chunk_ms=chunk_ms, chunk_steps=steps, ticks=n_ticks,
               tick_ms={m: dict(median=round(statistics.median(v), 4), p10=round(sorted(v)[len(v) // 10], 4),
                                p90=round(sorted(v)[(9 * len(v)) // 10], 4), min=round(min(v), 4), max=round(max(v), 4))
                        for m, v in ms.items()})
    print(json.dumps(row), flush=True)
    return row


def main():
    a = ARGS
    modes = [m for m in a.modes.split(",") if m]
    rows = [one_shot(n, cfg, Tf, st, a.reps, modes) for n, cfg, Tf, st in ONE_SHOT if a.only in n]
    if a.only in "bl6_softmax_pool":
        rows += [pool_ticks(ms, a.sessions, a.seconds, modes) for ms in (10, 50)]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, modes=modes, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
