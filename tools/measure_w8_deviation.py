"""How far e4m3 and bf16 storage of the streamed head matrices move the heads: teacher-forced decode of the `trained`
synthetic flavour, weights="e4m3" and weights="bf16" each against fp32 on the same inputs (the fp32 model's own free-running
output is the forced input of all three), B = 2, `--steps` steps.

  softmax (BL6, Q = 256)      max / mean |delta logit|, per-step KL(p_fp32 || p_mode): mean and max
  Laplace (seg 5 lpc 4; seg 1 lpc 4 through variant 6)   max / mean |delta mu|, |delta sigmoid(scale)|, |delta a|

The synthetic weights say nothing about audio quality: these are arithmetic deviations, no threshold is attached and no claim
about how a trained voice sounds in either mode is made.

    python tools/measure_w8_deviation.py [--steps 4000] [--out profiles/decode_w8_deviation.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from shallow_wavenet_amd import config as C  # noqa: E402
from shallow_wavenet_amd.runtime import HipNet  # noqa: E402
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict  # noqa: E402

NETS = [("bl6_softmax", C.bl6_softmax(), 0), ("bl6_laplace_s5l4", C.bl6_laplace(5, 4), 0), ("bl6_laplace_s1l4", C.bl6_laplace(1, 4), 6)]
MODES = ("e4m3", "bf16")


def _mm(x):
    return dict(max=float(x.abs().max()), mean=float(x.abs().mean()))


def measure(name, cfg, variant, steps, B=2):
    seg = 1 if cfg.kind == "softmax" else cfg.seg
    net = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=5, flavor="trained"), "cuda:0")
    Tf = -(-steps * seg // cfg.U)
    aux = torch.from_numpy(synth_aux(cfg, B, Tf, seed=3)).cuda()
    kw = dict(want_heads=True, variant=variant, rng_seed=11)
    forced, _ = net.decode(aux, steps, **kw)
    _, h32 = net.decode(aux, steps, forced=forced, **kw)
    h32 = h32.double()
    row = dict(net=name, variant=variant, steps=steps, batch=B, flavor="trained")
    if cfg.kind == "softmax":
        row["logit_range"] = float(h32.max() - h32.min())
    for mode in MODES:
        _, h = net.decode(aux, steps, forced=forced, weights=mode, **kw)
        h = h.double()
        if cfg.kind == "softmax":
            lp32, lp = torch.log_softmax(h32, -1), torch.log_softmax(h, -1)
            kl = (lp32.exp() * (lp32 - lp)).sum(-1)
            row[mode] = dict(delta_logit=_mm(h - h32), kl_per_step=dict(mean=float(kl.mean()), max=float(kl.max())))
        else:
            row[mode] = dict(delta_mu=_mm(h[..., :seg] - h32[..., :seg]),
                             delta_sigmoid_scale=_mm(torch.sigmoid(h[..., seg:2 * seg]) - torch.sigmoid(h32[..., seg:2 * seg])))
            if cfg.lpc:
                row[mode]["delta_a"] = _mm(h[..., 2 * seg:] - h32[..., 2 * seg:])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [measure(n, cfg, v, a.steps) for n, cfg, v in NETS]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), note="arithmetic deviations on synthetic weights; no threshold, "
                           "no claim about audio quality", rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
