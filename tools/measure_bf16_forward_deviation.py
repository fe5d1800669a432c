"""dev tool: how far the forward of the bf16 stack (`swn_forward_bf16`, BL6 class) lies from the float64 oracle on every kernel it
dispatches to, in units of the error inherent in its arithmetic, over every case of tests/bf16_forward_ref.py::cases().

Per case: max |raw_gpu - raw_exact| / D_fwd and rms(raw_gpu - raw_exact) / D_rms on the distinct rows (D_fwd, D_rms: max and rms of
raw_rounded - raw_exact, the same graph on the CPU with the kernels' bf16 roundings), the distance from the MODEL
(max |raw_gpu - raw_rounded| / D_fwd), whether the copies of the batch are bit-identical to their originals, and the path the
library reports.  A kernel that rounds where the model rounds sits near 1.  Per path the worst of all its cases and runs:
the margins of tests/test_gpu_bf16_forward_paths.py (bf16_forward_ref.MARGIN_FWD) must be at least twice it.

  python tools/measure_bf16_forward_deviation.py [--out profiles/bf16_forward_deviation.json] [--only SUBSTRING ...] [--repeat 2]
"""
import argparse
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "bf16_forward_deviation.json"))
    ap.add_argument("--only", nargs="*", default=[])
    ap.add_argument("--repeat", type=int, default=2, help="GPU runs per case: the worst counts")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bf16_forward_ref as F
    torch.set_num_threads(max(1, min(8, len(os.sched_getaffinity(0)))))

    res = {"margins": dict(F.MARGIN_FWD), "cases": {}, "paths": {}}
    for case in F.cases():
        if args.only and not any(s in case.name for s in args.only):
            continue
        inp = F.inputs_of(case)
        y = F.yardstick(case, inp)
        worst = None
        for _ in range(args.repeat):
            path, raw, hs = F.gpu_run(case, inp)
            r = raw[: case.rows].double().cpu().numpy()
            d = F.deviations(case, y, r)
            row = {"path": path, "max": d["max"] / y.D_fwd, "rms": d["rms"] / y.D_rms,
                   "model": float(np.abs(r - y.raw_rounded).max()) / y.D_fwd, "finite": d["finite"],
                   "copies_identical": not F.copies_differ(case, raw, hs)}
            if worst is None or max(row["max"], row["rms"]) > max(worst["max"], worst["rms"]):
                worst = row
        worst.update(D_fwd=y.D_fwd, D_rms=y.D_rms, raw_max=float(np.abs(y.raw_exact).max()), old_bound=y.old_bound,
                     positions=case.B * case.Tp)
        res["cases"][case.name] = worst
        print(f"{case.name:32s} {worst['path']:8s} max {worst['max']:5.2f}  rms {worst['rms']:5.2f}  model {worst['model']:5.2f}  "
              f"D_fwd {y.D_fwd:.3e}  D_rms {y.D_rms:.3e}  copies identical {worst['copies_identical']}", flush=True)
        grp = res["paths"].setdefault(case.path, {"max": 0.0, "rms": 0.0, "model": 0.0})
        for q in grp:
            grp[q] = max(grp[q], worst[q])
    for name, grp in res["paths"].items():
        print(f"path {name:8s} worst max ratio {grp['max']:.2f}  rms ratio {grp['rms']:.2f}  model {grp['model']:.2f}")

    def short(v):                       # four significant digits: the file is read by people
        if isinstance(v, dict):
            return {k: short(x) for k, x in v.items()}
        return float(f"{v:.4g}") if isinstance(v, float) else v
    with open(args.out, "w") as f:
        json.dump(short(res), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
