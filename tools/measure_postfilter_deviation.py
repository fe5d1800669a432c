"""dev tool: how far the device noise-shaping post-filter (swn_postfilter_chunk) lies from the exact reference of
tests/postfilter_ref.py, as a share of the bound tests/test_gpu_postfilter_edges.py asserts, over every case of its grid.

Per case (three 1 537-sample signals from zero state, then 200 samples resumed from the reference's state):
  share        worst |y_gpu - y_ref| / (2^-24 |y_ref| (1 + 2^-20) + E64)
  share_near0  the same over the samples where E64 is more than a tenth of the bound (outputs near zero, where the fp64 term counts)
  state        worst |state_gpu - state_ref| / (E64 / max|x| * the section's scale) over the three state sections
  host_e64     the host C filter (dsp.MLSAFilter, then the FIR as a float64 convolution): worst |y_host - y_ref| / E64

  python tools/measure_postfilter_deviation.py [--out profiles/postfilter_deviation.json] [--only SUBSTRING ...]
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
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "postfilter_deviation.json"))
    ap.add_argument("--only", nargs="*", default=[])
    args = ap.parse_args()
    import numpy as np
    import torch
    import postfilter_ref as R
    from shallow_wavenet_amd import dsp, ops  # noqa: F401  (registers torch.ops.swn.*)

    if not torch.cuda.is_available():
        sys.exit("measure_postfilter_deviation: needs the GPU")
    dev = "cuda:0"
    res = {"gpu": torch.cuda.get_device_name(0), "samples": R.N_LONG, "resumed_samples": R.N_RESUME, "cases": {}}
    for name in R.CASE_NAMES:
        if args.only and not any(s in name for s in args.only):
            continue
        c = R.case(name)
        per = R.state_doubles(c.order, c.pade, c.n_taps)
        img = torch.from_numpy(np.concatenate([c.b, c.taps])).to(dev)
        x = torch.from_numpy(c.x).to(dev)
        state = torch.zeros(4 * per, dtype=torch.float64, device=dev)
        out = torch.ops.swn.postfilter_chunk(img, state, [x[s, :R.N_LONG] for s in range(3)], [0, 1, 2], [True] * 3, c.order,
                                             c.alpha, c.pade, c.n_taps, 4).cpu().numpy().astype(np.float64)
        got_state = state.view(4, per)[2].cpu().numpy().copy()
        yref, sref = c.long_run
        state.view(4, per)[3] = torch.from_numpy(sref[2]).to(dev)
        cont = torch.ops.swn.postfilter_chunk(img, state, [x[2, R.N_LONG:]], [3], [False], c.order, c.alpha, c.pade, c.n_taps,
                                              4)[0].cpu().numpy().astype(np.float64)
        share = near0 = host = 0.0
        mlsa = dsp.MLSAFilter(c.order, c.alpha, hopsize=110, pade=c.pade)
        for s in range(3):
            xs = c.x[s, :R.N_LONG].astype(np.float64)
            e = c.e64(float(np.abs(xs).max()))
            pairs = [(out[s], yref[s])] + ([(cont, c.resumed)] if s == 2 else [])
            for got, ref in pairs:
                bound = R.output_bound(ref, e)
                d = np.abs(got - ref) / bound
                share = max(share, float(d.max()))
                sel = e > 0.1 * bound
                if sel.any():
                    near0 = max(near0, float(d[sel].max()))
            y_host = np.convolve(c.taps, mlsa.synthesis(xs, c.b[None]))[:xs.size]
            host = max(host, float(np.abs(y_host - yref[s]).max()) / e)
        st = 0.0
        for got, ref in zip(R.state_sections(got_state, c.order, c.pade, c.n_taps),
                            R.state_sections(sref[2], c.order, c.pade, c.n_taps)):
            if ref.size:
                st = max(st, float(np.abs(got - ref).max()) / (c.e64(1.0) * float(np.abs(ref).max())))
        res["cases"][name] = dict(order=c.order, alpha=c.alpha, pade=c.pade, n_taps=c.n_taps, l1=c.l1, e64=c.e64(1.0), share=share,
                                  share_near0=near0, state=st, host_e64=host)
        print(f"{name:22s} share {share:.3f}  near zero {near0:.3f}  state {st:.2e}  host / E64 {host:.2e}", flush=True)

    def short(v):                       # four significant digits: the file is read by people
        if isinstance(v, dict):
            return {k: short(x) for k, x in v.items()}
        return float(f"{v:.4g}") if isinstance(v, float) else v
    with open(args.out, "w") as f:
        json.dump(short(res), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
