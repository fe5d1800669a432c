"""What a multi-model decode pool buys on one MI355X: 64 sessions over M models of one geometry, one chunk (10 ms / 50 ms of
audio) of features and of samples per session and tick, through push_many + step.

  mixed     ONE DecodePool of 64 slots holding the M models (add_model), session i running model i % M: per tick one
            swn_frontend_pool[_models] call and one swn_decode_pool_chunk[_models] launch
  separate  the baseline without the feature: M single-model pools of 64 / M sessions each, ticked back to back

Per configuration, chunk length and M, medians over the ticks in which every session runs (the first --skip ticks, which hold
the prologues, and the last one are left out):

  device_ms    push_many + step of one tick between two device events;  frontend_ms / decode_ms: its two parts
  host_ms      wall clock the host spends issuing the tick (no synchronisation inside)
  speedup      separate device_ms / mixed device_ms;  vs_m1 = mixed device_ms / the M = 1 mixed device_ms

    python tools/time_pool_models.py [--seconds 1] [--out profiles/pool_models_timing.json]
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
from shallow_wavenet_amd.streaming import DecodePool  # noqa: E402
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict  # noqa: E402

CONFIGS = [("bl6_laplace_cfg2", C.bl6_laplace(), 22050), ("bl6_softmax", C.bl6_softmax(), 16000)]
SESSIONS = 64
_NETS: dict = {}


def _net(name, cfg, k):
    if (name, k) not in _NETS:
        sd = synth_state_dict(cfg, seed=5 + k, flavor="trained" if cfg.kind == "laplace" else "xavier")
        _NETS[(name, k)] = HipNet.from_state_dict(cfg, sd, "cuda:0")
    return _NETS[(name, k)]


def _ticks(pools, groups, auxs, F, frames, steps, skip):
    """drive the pools (pools[p] serves the sessions groups[p] = [(session index, model)]) tick by tick -> the medians"""
    sess = [[pool.open(utt_id=i, model=m) for i, m in group] for pool, group in zip(pools, groups)]
    rows = []
    f0 = 0
    while f0 < F:
        f1 = min(F, f0 + frames)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        # the separate pools run back to back: all their front end calls, then all their launches, as one tick
        t0 = time.perf_counter()
        ev[0].record()
        for pool, group, ss in zip(pools, groups, sess):
            pool.push_many({s: auxs[i][:, :, f0:f1] for s, (i, _) in zip(ss, group)}, finish=ss if f1 == F else ())
        ev[1].record()
        for pool in pools:
            pool.step(steps)
        ev[2].record()
        host = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        rows.append((ev[0].elapsed_time(ev[2]), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), host))
        f0 = f1
    kept = rows[skip:-1] if len(rows) > skip + 1 else rows
    med = [statistics.median(r[k] for r in kept) for k in range(4)]
    return dict(device_ms=round(med[0], 4), frontend_ms=round(med[1], 4), decode_ms=round(med[2], 4), host_ms=round(med[3], 4),
                ticks_measured=len(kept))


def measure(name, cfg, fs, seconds, chunk_ms, M, skip):
    seg = 1 if cfg.kind == "softmax" else cfg.seg
    nets = [_net(name, cfg, k) for k in range(M)]
    frames = max(1, int(round(chunk_ms * 1e-3 * fs / cfg.U)))
    F = max(4 * frames, int(round(seconds * fs / cfg.U)))
    steps = frames * cfg.U // seg
    auxs = [torch.from_numpy(synth_aux(cfg, 1, F, seed=10 + i)).cuda() for i in range(SESSIONS)]
    model = [i % M for i in range(SESSIONS)]

    pool = DecodePool(nets[0], SESSIONS, rng_seed=1)
    for n in nets[1:]:
        pool.add_model(n)
    mixed = _ticks([pool], [[(i, model[i]) for i in range(SESSIONS)]], auxs, F, frames, steps, skip)

    pools = [DecodePool(nets[m], SESSIONS // M, rng_seed=1) for m in range(M)]
    groups = [[(i, 0) for i in range(SESSIONS) if model[i] == m] for m in range(M)]
    separate = _ticks(pools, groups, auxs, F, frames, steps, skip)

    row = dict(config=name, chunk_ms=chunk_ms, chunk_frames=frames, chunk_steps=steps, sessions=SESSIONS, models=M,
               seconds=seconds, variant=pool.resolved_variant, packed_mb_per_model=round(nets[0].packed.numel() * 4 / 2 ** 20, 3),
               mixed=mixed, separate=separate, speedup=round(separate["device_ms"] / mixed["device_ms"], 3),
               host_speedup=round(separate["host_ms"] / mixed["host_ms"], 3),
               rtf_per_session=round(mixed["device_ms"] / (steps * seg / fs * 1e3), 4))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="audio per session")
    ap.add_argument("--models", default="1,2,4,16")
    ap.add_argument("--chunks", default="10,50", help="chunk lengths in ms")
    ap.add_argument("--only", default=None, help="one configuration name")
    ap.add_argument("--skip", type=int, default=3, help="leading ticks left out of the medians")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name, cfg, fs in CONFIGS:
        if a.only and a.only != name:
            continue
        for chunk_ms in [int(x) for x in a.chunks.split(",")]:
            base = None
            for M in [int(x) for x in a.models.split(",")]:
                if SESSIONS % M:
                    raise SystemExit(f"--models: {M} does not divide {SESSIONS} sessions")
                r = measure(name, cfg, fs, a.seconds, chunk_ms, M, a.skip)
                base = r["mixed"]["device_ms"] if M == 1 else base
                r["vs_m1"] = round(r["mixed"]["device_ms"] / base, 4) if base else None
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
