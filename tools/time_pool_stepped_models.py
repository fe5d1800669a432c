"""What a multi-model STEPPED decode pool buys on one MI355X (REF6, the run.sh geometry): 64 sessions over M models of one
geometry, one chunk (10 ms / 50 ms of audio) of features and of samples per session and tick, through push_many + step.

  mixed     ONE SteppedModelPool of 64 slots holding the M models (add_model), session i running model i % M: per tick one
            swn_frontend_pool[_models] call and one launch chain (swn_decode_pool_stepped_chunk[_models])
  separate  the baseline without the feature: M single-model SteppedDecodePools of 64 / M sessions each, ticked back to back

Per configuration, chunk length and M, medians (and the min .. max spread) over the ticks in which every session generates a
chunk (the first --skip ticks, which hold the prologues, and the last one are left out):

  device_ms    push_many + step of one tick between two device events;  frontend_ms / decode_ms: its two parts
  host_ms      wall clock the host spends issuing the tick (no synchronisation inside)
  us_per_step  decode_ms / chunk steps
  speedup      separate device_ms / mixed device_ms;  vs_m1 = mixed device_ms / the M = 1 mixed device_ms

    python tools/time_pool_stepped_models.py [--seconds 1] [--out profiles/pool_stepped_models_timing.json]

  --single_model_tick LABEL   instead: the tick of a single-model SteppedDecodePool at 64 sessions (the path this feature must
                              not slow down), one row appended to --out; run alternately on two builds of the library
                              (SWN_HIP_LIB selects one) to compare them inside one session of the machine
  --trace M                   instead: a few mixed ticks over M models and nothing else (for a kernel trace)
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
from shallow_wavenet_amd import streaming  # noqa: E402
from shallow_wavenet_amd.runtime import HipNet  # noqa: E402
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict  # noqa: E402

CONFIGS = [("ref6_laplace_s1", C.ref6_laplace(1, 4), 22050), ("ref6_softmax", C.ref6_softmax(), 22050)]
SESSIONS = 64
_NETS: dict = {}


def _net(name, cfg, k):
    if (name, k) not in _NETS:
        sd = synth_state_dict(cfg, seed=5 + k, flavor="trained" if cfg.kind == "laplace" else "xavier")
        _NETS[(name, k)] = HipNet.from_state_dict(cfg, sd, "cuda:0")
    return _NETS[(name, k)]


def _ticks(pools, groups, auxs, F, frames, steps, skip, several):
    """drive the pools (pools[p] serves the sessions groups[p] = [(session index, model)]) tick by tick -> the medians"""
    sess = [[pool.open(utt_id=i, model=m) if several else pool.open(utt_id=i) for i, m in group]
            for pool, group in zip(pools, groups)]
    rows = []
    f0 = 0
    while f0 < F:
        f1 = min(F, f0 + frames)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        # the separate pools run back to back: all their front end calls, then all their launch chains, as one tick
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
    return dict(device_ms=round(med[0], 4), device_ms_min=round(min(r[0] for r in kept), 4),
                device_ms_max=round(max(r[0] for r in kept), 4), frontend_ms=round(med[1], 4), decode_ms=round(med[2], 4),
                host_ms=round(med[3], 4), us_per_step=round(med[2] * 1e3 / steps, 2), ticks_measured=len(kept))


def _shape(cfg, fs, seconds, chunk_ms):
    seg = 1 if cfg.kind == "softmax" else cfg.seg
    frames = max(1, int(round(chunk_ms * 1e-3 * fs / cfg.U)))
    # the conditioning of a frame is final `lookahead` frames later: the first ticks run nothing, then the prologues
    F = max(4 * frames, int(round(seconds * fs / cfg.U)))
    return seg, frames, F, frames * cfg.U // seg


def measure(name, cfg, fs, seconds, chunk_ms, M, skip):
    seg, frames, F, steps = _shape(cfg, fs, seconds, chunk_ms)
    nets = [_net(name, cfg, k) for k in range(M)]
    auxs = [torch.from_numpy(synth_aux(cfg, 1, F, seed=10 + i)).cuda() for i in range(SESSIONS)]
    model = [i % M for i in range(SESSIONS)]
    skip = skip + -(-streaming.lookahead_frames(cfg) // frames)            # + the ticks before the first frame is final

    pool = streaming.SteppedModelPool(nets[0], SESSIONS, rng_seed=1)
    for n in nets[1:]:
        pool.add_model(n)
    mixed = _ticks([pool], [[(i, model[i]) for i in range(SESSIONS)]], auxs, F, frames, steps, skip, True)
    del pool

    pools = [streaming.SteppedDecodePool(nets[m], SESSIONS // M, rng_seed=1) for m in range(M)]
    groups = [[(i, 0) for i in range(SESSIONS) if model[i] == m] for m in range(M)]
    separate = _ticks(pools, groups, auxs, F, frames, steps, skip, False)

    return dict(config=name, chunk_ms=chunk_ms, chunk_frames=frames, chunk_steps=steps, sessions=SESSIONS, models=M,
                seconds=seconds, packed_mb_per_model=round(nets[0].packed.numel() * 4 / 2 ** 20, 3),
                mixed=mixed, separate=separate, speedup=round(separate["device_ms"] / mixed["device_ms"], 3),
                host_speedup=round(separate["host_ms"] / mixed["host_ms"], 3),
                rtf_per_session=round(mixed["device_ms"] / (steps * seg / fs * 1e3), 4))


def single_model_tick(label, name, cfg, fs, chunk_ms, ticks):
    """the tick of a single-model SteppedDecodePool at 64 sessions, prologues done: median and spread over `ticks` ticks"""
    seg, frames, _, steps = _shape(cfg, fs, 1.0, chunk_ms)
    net = _net(name, cfg, 0)
    pool = streaming.SteppedDecodePool(net, SESSIONS, rng_seed=1)
    for i in range(SESSIONS):
        pool.open().finish(torch.from_numpy(synth_aux(cfg, 1, frames * (ticks + 6) + 1, seed=10 + i)).cuda())
    pool.step(steps)                                           # every prologue and the first chunk
    for _ in range(3):
        pool.step(steps)                                       # warm-up
    torch.cuda.synchronize()
    evs = []
    for _ in range(ticks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pool.step(steps)
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return dict(label=label, lib=os.path.basename(os.path.dirname(os.environ.get("SWN_HIP_LIB", "")) or "tree"), config=name,
                chunk_ms=chunk_ms, chunk_steps=steps, sessions=SESSIONS, ticks=ticks, tick_ms_median=round(statistics.median(ms), 4),
                tick_ms_min=round(ms[0], 4), tick_ms_max=round(ms[-1], 4),
                us_per_step=round(statistics.median(ms) * 1e3 / steps, 2))


def trace(name, cfg, fs, chunk_ms, M, ticks):
    """a few mixed ticks over M models, prologues included, and nothing else"""
    seg, frames, _, steps = _shape(cfg, fs, 1.0, chunk_ms)
    pool = streaming.SteppedModelPool(_net(name, cfg, 0), SESSIONS, rng_seed=1)
    for k in range(1, M):
        pool.add_model(_net(name, cfg, k))
    for i in range(SESSIONS):
        pool.open(model=i % M).finish(torch.from_numpy(synth_aux(cfg, 1, frames * (ticks + 1) + 1, seed=10 + i)).cuda())
    for _ in range(ticks + 1):
        pool.step(steps)
    torch.cuda.synchronize()
    print(json.dumps(dict(config=name, models=M, ticks=ticks + 1, chunk_steps=steps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="audio per session")
    ap.add_argument("--models", default="1,2,4,16")
    ap.add_argument("--chunks", default="10,50", help="chunk lengths in ms")
    ap.add_argument("--only", default=None, help="one configuration name")
    ap.add_argument("--skip", type=int, default=3, help="leading ticks left out of the medians")
    ap.add_argument("--single_model_tick", default=None, metavar="LABEL")
    ap.add_argument("--trace", type=int, default=None, metavar="M")
    ap.add_argument("--ticks", type=int, default=20, help="ticks of --single_model_tick / --trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    configs = [c for c in CONFIGS if not a.only or a.only == c[0]]
    chunks = [int(x) for x in a.chunks.split(",")]
    if a.trace is not None:
        for name, cfg, fs in configs:
            trace(name, cfg, fs, chunks[0], a.trace, a.ticks)
        return
    if a.single_model_tick is not None:
        rows = [single_model_tick(a.single_model_tick, name, cfg, fs, ms, a.ticks) for name, cfg, fs in configs for ms in chunks]
        for r in rows:
            print(json.dumps(r), flush=True)
        if a.out:
            old = json.load(open(a.out))["rows"] if os.path.exists(a.out) else []
            with open(a.out, "w") as f:
                json.dump(dict(device=torch.cuda.get_device_name(0), rows=old + rows), f, indent=1)
                f.write("\n")
        return
    rows = []
    for name, cfg, fs in configs:
        for chunk_ms in chunks:
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
