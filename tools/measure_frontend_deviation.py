"""dev tool: how far the one-shot front end (swn_frontend) lies from the float64 oracle at every row of the geometry table
tests/frontend_geometry.py, stage by stage, beside the fp32 oracle's own distance e32 and the bound
max(2e-6 * max(1, scale), 4 * e32) that tests/test_gpu_frontend_geometry.py holds it to.

Per row and stage the file keeps the shape (batch, frames) with the largest error / bound and its figures; `worst` is the
largest ratio over everything.

  python tools/measure_frontend_deviation.py [--out profiles/frontend_geometry_deviation.json] [--only SUBSTRING ...]
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
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "frontend_geometry_deviation.json"))
    ap.add_argument("--only", nargs="*", default=[])
    args = ap.parse_args()
    import torch
    import frontend_geometry as G
    from shallow_wavenet_amd.runtime import HipNet
    torch.set_num_threads(max(1, min(8, len(os.sched_getaffinity(0)))))
    assert torch.cuda.is_available(), "needs a HIP device"

    res = {"tol": G.TOL, "order": G.ORDER, "rows": {}, "worst": {"ratio": 0.0}}
    for row in G.ROWS:
        if args.only and not any(s in row.id for s in args.only):
            continue
        net = HipNet.from_state_dict(row.cfg, G.state_dict(row), "cuda:0")
        per = {}
        for batch, frames in [(1, f) for f in G.frame_counts(row.cfg)] + [(3, 65)]:
            got = G.device_stages(net, G.features(row.cfg, batch, frames))
            for what, err, bound, e32, scale in G.stage_errors(row, got, batch, frames):
                e = {"batch": batch, "frames": frames, "e32": e32, "scale": scale, "bound": bound, "error": err,
                     "ratio": err / bound}
                if what not in per or e["ratio"] > per[what]["ratio"]:
                    per[what] = e
                if e["ratio"] > res["worst"]["ratio"]:
                    res["worst"] = dict(e, row=row.id, stage=what)
        res["rows"][row.id] = dict(path=row.path, lds=row.lds, A0=row.cfg.A0, N=G.cond_width(row.cfg), stages=per)
        print(f"{row.id:10s} {row.path:10s} " + "  ".join(f"{w} {e['ratio']:.2f}" for w, e in per.items()), flush=True)
    print(f"worst: {res['worst']}")

    def short(v):                       # four significant digits: the file is read by people
        if isinstance(v, dict):
            return {k: short(x) for k, x in v.items()}
        return float(f"{v:.4g}") if isinstance(v, float) else v
    with open(args.out, "w") as f:
        json.dump(short(res), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
