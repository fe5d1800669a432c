"""A decode pool over several models with fp32 / bf16 / e4m3 head weights on one MI355X: 64 sessions over M models of one
geometry, one chunk (10 ms / 50 ms of audio) of features and of samples per session and tick, through push_many + step.

  mixed     per format ONE pool of 64 slots holding the M models (add_model; DecodeModelPool for bf16 / e4m3), session i running
            model i % M: per tick one swn_frontend_pool[_models] call and one swn_decode_pool_chunk[_models][_w16 | _w8] launch
  separate  the baseline without the feature: per format M single-model pools of 64 / M sessions each, ticked back to back

The pools of the formats tick in turn inside every tick of one run (fp32 mixed, bf16 mixed, e4m3 mixed, then the separate groups),
so they see the same device state.  Per net, chunk length, M and format, over the ticks in which every session runs (the first
--skip ticks, which hold the prologues, and the last one are left out): device time of a tick (push_many + step between two
device events) as median [min - max], and

  vs_fp32      mixed device median / the fp32 mixed median of the same run
  vs_m1        mixed device median / the M = 1 median of the same format
  separate_x   separate device median / mixed device median

    python tools/time_pool_models_weights.py [--seconds 1] [--models 1,2,4,16] [--formats fp32,bf16,e4m3] [--tree DIR]
                                             [--out profiles/pool_models_weights_timing.json]

--models 1 needs nothing but DecodePool, and --tree imports the package from another checkout: `--models 1 --tree <parent
checkout>` times the parent commit's fp32 and single-model image ticks with this tool (to show they did not move).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=1.0, help="audio per session")
ap.add_argument("--models", default="1,2,4,16")
ap.add_argument("--chunks", default="10,50", help="chunk lengths in ms")
ap.add_argument("--formats", default="fp32,bf16,e4m3")
ap.add_argument("--only", default=None, help="one net's name")
ap.add_argument("--skip", type=int, default=3, help="leading ticks left out")
ap.add_argument("--no-separate", action="store_true", help="leave the M single-model pools out")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ARGS = ap.parse_args() if __name__ == "__main__" else ap.parse_args([])
sys.path.insert(0, os.path.abspath(ARGS.tree))

import torch  # noqa: E402

from shallow_wavenet_amd import config as C  # noqa: E402
from shallow_wavenet_amd import streaming  # noqa: E402
from shallow_wavenet_amd.runtime import HipNet  # noqa: E402
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict  # noqa: E402

NETS = [("bl6_softmax", C.bl6_softmax(), 16000), ("bl6_laplace_s5l4", C.bl6_laplace(5, 4), 22050)]
SESSIONS = 64
_NETS: dict = {}


def _net(name, cfg, k):
    if (name, k) not in _NETS:
        sd = synth_state_dict(cfg, seed=5 + k, flavor="trained" if cfg.kind == "laplace" else "xavier")
        _NETS[(name, k)] = HipNet.from_state_dict(cfg, sd, "cuda:0")
    return _NETS[(name, k)]


def _summary(xs, nd=4):
    return dict(median=round(statistics.median(xs), nd), min=round(min(xs), nd), max=round(max(xs), nd), ticks=len(xs))


def _mixed_pool(nets, fmt):
    if len(nets) == 1:
        return streaming.DecodePool(nets[0], SESSIONS, rng_seed=1, weights=fmt)
    cls = streaming.DecodePool if fmt == "fp32" else streaming.DecodeModelPool
    pool = cls(nets[0], SESSIONS, rng_seed=1, weights=fmt)
    for n in nets[1:]:
        pool.add_model(n)
    return pool


def measure(name, cfg, fs, seconds, chunk_ms, M, formats, skip, separate):
    seg = 1 if cfg.kind == "softmax" else cfg.seg
    nets = [_net(name, cfg, k) for k in range(M)]
    frames = max(1, int(round(chunk_ms * 1e-3 * fs / cfg.U)))
    F = max(4 * frames, int(round(seconds * fs / cfg.U)))
    steps = frames * cfg.U // seg
    auxs = [torch.from_numpy(synth_aux(cfg, 1, F, seed=10 + i)).cuda() for i in range(SESSIONS)]
    model = [i % M for i in range(SESSIONS)]
    # a group = the pools that make one tick of a setting: (label, pools, per pool [(session index, model)])
    groups = []
    for fmt in formats:
        groups.append((f"{fmt}_mixed", [_mixed_pool(nets, fmt)], [[(i, model[i]) for i in range(SESSIONS)]]))
    if separate and M > 1:
        for fmt in formats:
            groups.append((f"{fmt}_separate", [streaming.DecodePool(nets[m], SESSIONS // M, rng_seed=1, weights=fmt) for m in range(M)],
                           [[(i, 0) for i in range(SESSIONS) if model[i] == m] for m in range(M)]))
    sess = {label: [[pool.open(utt_id=i, model=m) for i, m in group] for pool, group in zip(pools, parts)]
            for label, pools, parts in groups}
    rows = {label: [] for label, _, _ in groups}
    f0 = 0
    while f0 < F:
        f1 = min(F, f0 + frames)
        for label, pools, parts in groups:                 # the settings tick in turn
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for pool, group, ss in zip(pools, parts, sess[label]):
                pool.push_many({s: auxs[i][:, :, f0:f1] for s, (i, _) in zip(ss, group)}, finish=ss if f1 == F else ())
            for pool in pools:
                pool.step(steps)
            b.record()
            torch.cuda.synchronize()
            rows[label].append(a.elapsed_time(b))
        f0 = f1
    out = dict(net=name, chunk_ms=chunk_ms, chunk_frames=frames, chunk_steps=steps, sessions=SESSIONS, models=M, seconds=seconds)
    for label in rows:
        kept = rows[label][skip:-1] if len(rows[label]) > skip + 1 else rows[label]
        out[label] = _summary(kept)
    for fmt in formats:
        mixed = out[f"{fmt}_mixed"]["median"]
        if "fp32" in formats:
            out[f"{fmt}_vs_fp32"] = round(mixed / out["fp32_mixed"]["median"], 4)
        if f"{fmt}_separate" in out:
            out[f"{fmt}_separate_x"] = round(out[f"{fmt}_separate"]["median"] / mixed, 3)
    return out


def main():
    a = ARGS
    formats = a.formats.split(",")
    rows = []
    for name, cfg, fs in NETS:
        if a.only and a.only != name:
            continue
        for chunk_ms in [int(x) for x in a.chunks.split(",")]:
            base = {}
            for M in [int(x) for x in a.models.split(",")]:
                if SESSIONS % M:
                    raise SystemExit(f"--models: {M} does not divide {SESSIONS} sessions")
                r = measure(name, cfg, fs, a.seconds, chunk_ms, M, formats, a.skip, not a.no_separate)
                for fmt in formats:
                    if M == 1:
                        base[fmt] = r[f"{fmt}_mixed"]["median"]
                    if fmt in base:
                        r[f"{fmt}_vs_m1"] = round(r[f"{fmt}_mixed"]["median"] / base[fmt], 4)
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            json.dump(dict(device=torch.cuda.get_device_name(0), tree=os.path.relpath(os.path.abspath(a.tree), here), rows=rows),
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
