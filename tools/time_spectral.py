"""dev tool: what the spectral terms of the stage-7 loss cost, through torch.stft + autograd (the default path) and through
the HIP operator (spectral.MultiResolutionSTFTLoss), at the recipe's size (seg 5 -> 5 rows of ~8 100 samples, 17 FFT sizes):

  - the spectral part alone, forward (no_grad) and forward + backward, device events, the two paths alternating block by
    block, median over the blocks of the per-call mean;
  - the stage-7 chunk of tools/time_driver.py (bf16 and fp32, wall clock per chunk as the driver logs it) with
    --spectral_loss torch and hip (and, with --parent-tree, the parent commit's driver), one fresh process per run,
    alternating, median over the runs of the per-run mean;
  - the operator's arithmetic (counted from the shapes) over its time, as a fraction of the 155 TFLOP/s fp32 matrix rate.

  python tools/time_spectral.py [--out profiles/spectral_timing.json] [--blocks 5] [--calls 40] [--chunk-runs 3] [--chunk-iters 40]
                                [--parent-tree DIR]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)

FP32_MATRIX_FLOPS = 155e12


def op_flops(R, T, sizes):
    """multiply-adds x 2 of the dense transforms: forward = 2 signals x (re, im) x frames x n x bins, backward = 1 x the same"""
    per = sum((1 + T // (n // 4)) * n * (n // 2 + 1) * 2 for n in sizes)
    return 2 * 2 * R * per, 2 * R * per


def torch_spectral(samples, targets, sizes, windows):
    """the torch path of train_driver.batch_loss: one stft over the 2R stacked rows per size, both LSDloss formulas"""
    import torch
    from shallow_wavenet_amd.train_driver import _stft
    R = samples.shape[0]
    sig = torch.cat([samples, targets])
    l1, lsd = [], []
    for n, win in zip(sizes, windows):
        sp = _stft(sig, n, win)
        so, st = sp[:R], sp[R:]
        l1.append(torch.abs(so - st).mean(dim=(1, 2, 3)))
        px, py = torch.sum(so ** 2, -1), torch.sum(st ** 2, -1)
        lsd.append(torch.sqrt(torch.mean((10 * (torch.log10(px) - torch.log10(py))) ** 2, 1)).mean(1))
    return torch.stack(l1, 1), torch.stack(lsd, 1)


def time_op(blocks, calls, R=5, T=8114):
    import torch
    from shallow_wavenet_amd.spectral import MultiResolutionSTFTLoss
    from shallow_wavenet_amd.train_driver import fft_sizes
    assert torch.cuda.is_available(), "needs a HIP device"
    sizes = fft_sizes(17)
    g = torch.Generator().manual_seed(0)
    trg = torch.tanh(torch.randn(R, T, generator=g)).cuda()
    smp = (trg + 0.02 * torch.randn(R, T, generator=g).cuda()).clamp(-1, 1).requires_grad_(True)
    windows = [torch.hann_window(n).cuda() for n in sizes]
    hip = MultiResolutionSTFTLoss(sizes, "cuda")
    paths = {"torch": lambda: torch_spectral(smp, trg, sizes, windows), "hip": lambda: hip(smp, trg, T)}

    def run(path, backward, n):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(n):
            if backward:
                smp.grad = None
                l1, _ = paths[path]()
                l1.mean().backward()
            else:
                with torch.no_grad():
                    paths[path]()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / n

    out = {}
    for backward in (False, True):
        for p in paths:
            run(p, backward, 5)                                     # warm-up of every shape
        ms = {p: [] for p in paths}
        for _ in range(blocks):
            for p in paths:
                ms[p].append(run(p, backward, calls))
        out["forward_backward" if backward else "forward"] = {
            p: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for p, v in ms.items()}
    f_fwd, f_bwd = op_flops(R, T, sizes)
    out["hip_flop"] = {"forward": f_fwd, "backward": f_bwd}
    out["hip_fraction_of_fp32_matrix_rate"] = {
        "forward": f_fwd / (out["forward"]["hip"]["median_ms"] * 1e-3) / FP32_MATRIX_FLOPS,
        "forward_backward": (f_fwd + f_bwd) / (out["forward_backward"]["hip"]["median_ms"] * 1e-3) / FP32_MATRIX_FLOPS}
    out["shape"] = {"rows": R, "samples": T, "fft_sizes": sizes, "blocks": blocks, "calls_per_block": calls}
    return out


# tools/time_driver.py's run (same flags), printing every chunk time the driver logged instead of their median in whole ms
_CHUNK_CHILD = """
import sys, re, io, logging, tempfile
sys.path.insert(0, sys.argv[1])
from shallow_wavenet_amd import train_driver as T
buf = io.StringIO()
logging.getLogger().addHandler(logging.StreamHandler(buf)); logging.getLogger().setLevel(logging.INFO)
with tempfile.TemporaryDirectory() as d:
    T.main(["--expdir", d, "--synthetic", "6", "--max_iters", sys.argv[3], "--seg", "5", "--lpc", "4", "--do_prob", "0.5",
            "--wav_conv_flag", "true", "--precision", sys.argv[2], "--GPU_device", "0", "--verbose", "1"] + sys.argv[4:])
print("CHUNKS", " ".join(re.findall(r"\\((\\d+\\.\\d+) sec\\)", buf.getvalue())))
"""


def _chunk_ms(root, prec, iters, extra):
    """mean ms per chunk past the first five of one driver run in a fresh process (the log line carries whole ms, so the
    mean over the chunks, not their median, resolves below 1 ms)"""
    r = subprocess.run([sys.executable, "-c", _CHUNK_CHILD, root, prec, str(iters)] + extra, capture_output=True, text=True,
                       timeout=600, cwd=root)
    m = re.search(r"^CHUNKS (.+)$", r.stdout, re.M)
    if r.returncode != 0 or not m:
        raise RuntimeError(f"driver run {root} {prec} {extra} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    secs = [float(v) for v in m.group(1).split()]
    return 1e3 * statistics.mean(secs[5:] if len(secs) > 10 else secs)


def time_chunks(runs, iters, parent_tree=None):
    """the stage-7 chunk (tools/time_driver.py's flags) with --spectral_loss torch and hip, alternating run by run; with a
    built checkout of the parent commit in `parent_tree`, its chunk too (the check that `torch` still is the parent's path)"""
    out = {}
    for prec in ("bf16", "fp32"):
        ms = {"torch": [], "hip": []}
        if parent_tree:
            ms["parent_commit"] = []
        for _ in range(runs):
            for path in ms:
                if path == "parent_commit":
                    ms[path].append(_chunk_ms(os.path.abspath(parent_tree), prec, iters, []))
                else:
                    ms[path].append(_chunk_ms(_R, prec, iters, ["--spectral_loss", path]))
                print(f"chunk {prec} {path}: {ms[path][-1]:.2f} ms", flush=True)
        out[prec] = {p: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for p, v in ms.items()}
    out["runs"], out["chunks_per_run"] = runs, iters
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "spectral_timing.json"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--chunk-runs", type=int, default=3)
    ap.add_argument("--chunk-iters", type=int, default=40)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: time its chunk as well")
    a = ap.parse_args()
    res = {"spectral_part": time_op(a.blocks, a.calls)}
    print(json.dumps(res["spectral_part"]), flush=True)
    if a.chunk_runs > 0:
        res["stage7_chunk"] = time_chunks(a.chunk_runs, a.chunk_iters, a.parent_tree)
    import torch
    res["device"] = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
