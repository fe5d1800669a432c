"""dev tool: how far the fp32 training backward (`train_precision("fp32")`, csrc/swn_train.hip) lies from the float64 oracle, in
units of the fp32 oracle's own distance to float64, over every case of tests/fp32_backward_ref.py::cases().

Per case and parameter tensor k: err_k = ||g_gpu - g_exact||, the yardstick D_k = ||g_32 - g_exact|| (the oracle evaluated in
float32 on the CPU) and the ratio err_k / (D_k + FLOOR * D_max / sqrt(n_k)); the worst ratio err_row / fp32_backward_ref.row_yardstick over
the rows of the 2-D / 3-D weights; the forward's max |raw_gpu - raw_exact| / D_fwd.  Every case runs `--repeat` times on the
device (the reduce kernels use float atomics, so the runs differ); the file keeps per case the worst run and the spread between the runs, and
per path the worst of each figure and the largest run-to-run spread.  The margins of tests/test_gpu_fp32_backward_edges.py are
twice the worst tensor ratio (and twice the worst forward ratio) of each path.

  python tools/measure_fp32_backward_deviation.py [--out profiles/fp32_backward_deviation.json] [--only SUBSTRING ...] [--repeat 2]
  python tools/measure_fp32_backward_deviation.py --seeds      (CPU only) the first decisive seed of every case, from its number
                                                               upwards: the SEEDS table of tests/fp32_backward_ref.py
"""
import argparse
import dataclasses
import json
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, "tests"))


def find_seeds(R, only):
    table = {}
    for number, case in enumerate(R.cases(), 1):
        if only and not any(s in case.name for s in only):
            continue
        for seed in range(number, number + 400):
            pre_min, flips = R.decisive(dataclasses.replace(case, seed=seed))
            if flips == 0 and pre_min >= R.PRE_MIN:
                break
        else:
            raise SystemExit(f"{case.name}: no decisive seed in 400")
        if seed != number:
            table[case.name] = seed
        print(f"{case.name:28s} number {number:3d} seed {seed:3d}  pre_min {pre_min:.2e}", flush=True)
    print("SEEDS: Dict[str, int] = " + json.dumps(table))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "fp32_backward_deviation.json"))
    ap.add_argument("--only", nargs="*", default=[])
    ap.add_argument("--verbose", action="store_true", help="print every tensor's figures (the file keeps the worst per case)")
    ap.add_argument("--repeat", type=int, default=2, help="GPU runs per case (the float atomics move from run to run)")
    ap.add_argument("--seeds", action="store_true", help="search the decisive seeds on the CPU and print the table")
    args = ap.parse_args()
    import torch
    import fp32_backward_ref as R
    torch.set_num_threads(max(1, min(8, len(os.sched_getaffinity(0)))))
    if args.seeds:
        return find_seeds(R, args.only)

    res = {"floor": R.FLOOR, "n_series": R.N_SERIES, "repeat": args.repeat, "cases": {}, "paths": {}}
    for case in R.cases():
        if args.only and not any(s in case.name for s in args.only):
            continue
        t0 = time.time()
        inp = R.inputs_of(case)
        y = R.yardstick(*inp)
        t_oracle = time.time() - t0
        runs = []
        for _ in range(args.repeat):
            raw, g, hs = R.gpu_run(case, inp)
            d = R.deviations(y, raw, g, hs)
            row = dict(R.ratios(d), nonzero=d["nonzero"], tensors={})
            for k, t in d["tensors"].items():
                e = {"err": t["err"], "D": t["D"], "norm": t["norm"], "ratio": t["err"] / (t["D"] + t["floor"])}
                if "rows_err" in t:
                    rr = t["rows_err"] / t["rows_yard"]
                    e["rows"], e["row"] = float(rr.max()), int(rr.argmax())
                row["tensors"][k] = e
            runs.append(row)
        worst = max(runs, key=lambda r: max(r["tensor"], r["rows"]))
        spread = {q: max(r[q] for r in runs) - min(r[q] for r in runs) for q in ("tensor", "rows", "fwd")}
        kt = max(worst["tensors"], key=lambda k: worst["tensors"][k]["ratio"])
        kr = max(worst["tensors"], key=lambda k: worst["tensors"][k].get("rows", 0.0))
        if args.verbose:
            for k, e in worst["tensors"].items():
                print(f"    {k}: " + "  ".join(f"{q} {v:.3g}" for q, v in e.items()))
        res["cases"][case.name] = dict(path=case.path, tensor=worst["tensor"], rows=worst["rows"], fwd=worst["fwd"], spread=spread,
                                       nonzero=worst["nonzero"], D_max=y.D_max, D_fwd=y.D_fwd, flips=y.flips, pre_min=y.pre_min,
                                       oracle_seconds=t_oracle, worst_tensor=dict(worst["tensors"][kt], name=kt),
                                       worst_row=dict(worst["tensors"][kr], name=kr))
        print(f"{case.name:28s} {case.path:6s} tensor {worst['tensor']:6.2f} ({kt})  row {worst['rows']:6.2f} ({kr} "
              f"[{worst['tensors'][kr].get('row')}])  fwd {worst['fwd']:5.2f}  spread {spread['tensor']:.3f}  flips {y.flips}  "
              f"nonzero {worst['nonzero'][:4]}  oracle {t_oracle:.1f} s", flush=True)
        grp = res["paths"].setdefault(case.path, {"tensor": 0.0, "rows": 0.0, "fwd": 0.0, "spread": 0.0})
        for q in ("tensor", "rows", "fwd"):
            grp[q] = max(grp[q], worst[q])
        grp["spread"] = max(grp["spread"], spread["tensor"])
    for name, grp in res["paths"].items():
        print(f"path {name:6s} worst tensor ratio {grp['tensor']:.2f}  row ratio {grp['rows']:.2f}  forward {grp['fwd']:.2f}  "
              f"largest run-to-run spread {grp['spread']:.3f}")

    def short(v):                       # four significant digits: the file is read by people
        if isinstance(v, dict):
            return {k: short(x) for k, x in v.items()}
        return float(f"{v:.4g}") if isinstance(v, float) else v
    with open(args.out, "w") as f:
        json.dump(short(res), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
