"""dev tool: how far the mixed-precision backward (`train_precision("bf16")`) lies from the float64 oracle, in units of the
error inherent in its arithmetic, over every case of tests/mixed_ref.py::cases().

Per case and parameter tensor k: err_k = ||g_gpu - g_exact||, the yardstick D_k = ||g_rounded - g_exact|| (tests/mixed_ref.py:
the same graph on the CPU with the kernels' bf16 roundings) and the ratio err_k / (D_k + FLOOR * D_max); the worst ratio
err_row / mixed_ref.row_yardstick over the rows of the 2-D / 3-D weights; the forward's max |raw_gpu - raw_exact| / D_fwd; and ||g_gpu - g_rounded|| / D_k, how
far the kernels are from the MODEL (small where the model rounds where the kernels round).  A kernel that rounds where the
model rounds sits near 1.  The margins of tests/test_gpu_mixed_backward_edges.py are twice the worst ratio
(tensors and rows) of each path.

  python tools/measure_mixed_deviation.py [--out profiles/mixed_backward_deviation.json] [--only SUBSTRING ...] [--repeat 2]
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
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "mixed_backward_deviation.json"))
    ap.add_argument("--only", nargs="*", default=[])
    ap.add_argument("--verbose", action="store_true", help="print every tensor's figures (the file keeps the worst per case)")
    ap.add_argument("--repeat", type=int, default=2, help="GPU runs per case (the float atomics move from run to run): the worst counts")
    args = ap.parse_args()
    import numpy as np
    import torch
    import mixed_ref as M
    torch.set_num_threads(max(1, min(8, len(os.sched_getaffinity(0)))))

    res = {"floor": M.FLOOR, "cases": {}, "groups": {}}
    for case in M.cases():
        if args.only and not any(s in case.name for s in args.only):
            continue
        inp = M.inputs_of(case)
        y = M.yardstick(*inp, case.path)
        worst = None
        for _ in range(args.repeat):
            raw, g = M.gpu_run(case, inp)
            d = M.deviations(case, y, raw, g)
            row = {"fwd": d["fwd_err"] / d["D_fwd"], "nonzero": d["nonzero"], "tensors": {}}
            for k, t in d["tensors"].items():
                e = {"err": t["err"], "D": t["D"], "norm": t["norm"], "ratio": t["err"] / (t["D"] + M.FLOOR * d["D_max"]),
                     "model": t["model"] / (t["D"] + M.FLOOR * d["D_max"])}
                if "rows_err" in t:
                    rr = t["rows_err"] / t["rows_yard"]
                    e["rows"] = float(rr.max())
                    e["row"] = int(rr.argmax())
                row["tensors"][k] = e
            row["ratio"] = max(e["ratio"] for e in row["tensors"].values())
            row["rows"] = max(e.get("rows", 0.0) for e in row["tensors"].values())
            row["model"] = max(e["model"] for e in row["tensors"].values())
            if worst is None or max(row["ratio"], row["rows"]) > max(worst["ratio"], worst["rows"]):
                worst = row
        worst.update(group=case.margin_group, D_max=y.D_max, D_fwd=y.D_fwd, flips=y.flips, pre_min=y.pre_min)
        kt = max(worst["tensors"], key=lambda k: worst["tensors"][k]["ratio"])
        kr = max(worst["tensors"], key=lambda k: worst["tensors"][k].get("rows", 0.0))
        if args.verbose:
            for k, e in worst["tensors"].items():
                print(f"    {k}: " + "  ".join(f"{q} {v:.3g}" for q, v in e.items()))
        res["cases"][case.name] = dict({q: v for q, v in worst.items() if q != "tensors"}, worst_tensor=dict(worst["tensors"][kt], name=kt),
                                       worst_row=dict(worst["tensors"][kr], name=kr))
        print(f"{case.name:30s} {case.margin_group:12s} tensor {worst['ratio']:6.2f} ({kt})  row {worst['rows']:6.2f} ({kr} "
              f"[{worst['tensors'][kr].get('row')}])  fwd {worst['fwd']:5.2f}  model {worst['model']:6.3f}  nonzero {worst['nonzero']}", flush=True)
        grp = res["groups"].setdefault(case.margin_group, {"ratio": 0.0, "rows": 0.0, "fwd": 0.0, "model": 0.0})
        for q in grp:
            grp[q] = max(grp[q], worst[q])
    for name, grp in res["groups"].items():
        print(f"group {name:12s} worst tensor ratio {grp['ratio']:.2f}  row ratio {grp['rows']:.2f}  forward {grp['fwd']:.2f}  model {grp['model']:.3f}")
    def short(v):                       # four significant digits: the file is read by people
        if isinstance(v, dict):
            return {k: short(x) for k, x in v.items()}
        return float(f"{v:.4g}") if isinstance(v, float) else v
    with open(args.out, "w") as f:
        json.dump(short(res), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
