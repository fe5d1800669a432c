"""Device noise-shaping restoration (postfilter.NoiseShapingRestorer, run.sh stage 6) on one MI355X, against the host filter:

  (a) one_utt_us_per_sample     restore() of one 66 000-sample utterance (m = 49, pade 4, 22.05 kHz), device events, median
  (b) batch64_us_per_sample     restore() of 64 such utterances in one call, per sample of all of them (and per wave)
  (c) host_us_per_sample        dsp.noise_shaping of the same signal on one core, after a warm-up, median
  (d) pool_tick_ms              a BL6 Laplace DecodePool tick at E = 64 with 50 ms chunks (conditioning final up front), with and
                                without post_filter, median over the ticks in which every session runs; ratio = with / without

    python tools/time_postfilter.py [--out profiles/postfilter_timing.json]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from shallow_wavenet_amd import config as C, dsp  # noqa: E402
from shallow_wavenet_amd.postfilter import NoiseShapingRestorer  # noqa: E402
from shallow_wavenet_amd.runtime import HipNet  # noqa: E402
from shallow_wavenet_amd.streaming import DecodePool  # noqa: E402
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict  # noqa: E402

FS, ALPHA, N = 22050, 0.455, 66000
MEAN = np.concatenate([[0.9, 5.0, -3.0, -4.0, 0.1], 1.5 * np.exp(-0.15 * np.arange(50)) * np.cos(0.7 * np.arange(50))])


def _events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def pool_ticks(net, E, steps, post_filter, F):
    pool = DecodePool(net, E, rng_seed=1, post_filter=post_filter)
    sess = []
    for i in range(E):
        s = pool.open()
        s.finish(torch.from_numpy(synth_aux(net.cfg, 1, F, seed=10 + i)).cuda())
        sess.append(s)
    ticks = []
    while all(s.steps_done + steps <= s.steps_ready for s in sess):
        ticks += _events(lambda: pool.step(steps), 1)
    return ticks[1:] or ticks


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postfilter_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    x = (0.5 * np.sin(2 * np.pi * 220 * np.arange(N) / FS) + 0.45 * rng.uniform(-1, 1, N)).astype(np.float32)
    res = dict(samples=N, order=49, pade=4, fs=FS, gpu=torch.cuda.get_device_name(0))

    r = NoiseShapingRestorer(MEAN, FS, ALPHA, device="cuda")
    xd = torch.from_numpy(x).cuda()
    r.restore([xd])
    ms = statistics.median(_events(lambda: r.restore([xd]), args.reps))
    res["a_one_utt_ms"] = round(ms, 3)
    res["a_one_utt_us_per_sample"] = round(ms * 1e3 / N, 4)
    print(json.dumps({k: res[k] for k in ("a_one_utt_ms", "a_one_utt_us_per_sample")}), flush=True)

    xs = [torch.from_numpy(np.roll(x, 97 * i)).cuda() for i in range(64)]
    r.restore(xs)
    ms = statistics.median(_events(lambda: r.restore(xs), args.reps))
    res["b_batch64_ms"] = round(ms, 3)
    res["b_batch64_us_per_sample"] = round(ms * 1e3 / (64 * N), 5)
    res["b_batch64_us_per_sample_per_wave"] = round(ms * 1e3 / N, 4)
    print(json.dumps({k: res[k] for k in ("b_batch64_ms", "b_batch64_us_per_sample")}), flush=True)

    torch.set_num_threads(1)
    dsp.noise_shaping(x, MEAN, FS, ALPHA)
    host = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        dsp.noise_shaping(x, MEAN, FS, ALPHA)
        host.append(time.perf_counter() - t0)
    res["c_host_ms"] = round(statistics.median(host) * 1e3, 3)
    res["c_host_us_per_sample"] = round(statistics.median(host) * 1e6 / N, 4)
    res["c_host_note"] = "one core of the GPU host's CPU (scipy lfilter + the C MLSA filter)"
    print(json.dumps({k: res[k] for k in ("c_host_ms", "c_host_us_per_sample")}), flush=True)

    cfg = C.bl6_laplace()
    net = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=5, flavor="trained"), "cuda:0")
    E, frames = 64, 10                                      # 50 ms of 22.05 kHz audio = 10 frames of 110 samples
    steps, F = frames * cfg.U, 8 * frames + 2
    pf = NoiseShapingRestorer(MEAN, FS, ALPHA, capacity=E, device="cuda")
    plain = pool_ticks(net, E, steps, None, F)
    post = pool_ticks(net, E, steps, pf, F)
    res["d_pool_sessions"], res["d_pool_chunk_samples"] = E, steps
    res["d_pool_tick_ms"] = round(statistics.median(plain), 4)
    res["d_pool_tick_post_filter_ms"] = round(statistics.median(post), 4)
    res["d_ratio"] = round(statistics.median(post) / statistics.median(plain), 4)
    res["d_target_ratio"] = 1.10
    print(json.dumps({k: res[k] for k in ("d_pool_tick_ms", "d_pool_tick_post_filter_ms", "d_ratio")}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
