"""dev tool: what mel-cepstra cost on the device, through the HIP operator (melspec.MelCepstrumExtractor, mcep_kernel of
csrc/swn_melspec.hip) and through the same definition composed from torch on the same device (torch.stft with the periodic
Hann window, centre, reflect; abs; clamp; log; one matmul with the same fp32 G), at fs 22 050, n_fft 1024, hop 110, order 49,
alpha 0.455:

  - 1 x 66 000 and 64 x 66 000 samples, one call each.

Device events around `calls` calls, the two paths alternating block by block in one run, median [min - max] over the blocks
of the per-call mean; the largest difference between the two paths' outputs is recorded with the times.  The operator's
arithmetic, counted from the shapes as it runs it (each frame folded once: (re, im) x frames x n / 2 x bins multiply-adds,
then frames x padded bins x 16-coefficient tiles), over its time, as a fraction of the 155 TFLOP/s fp32 matrix rate.  No
target is fixed: the result says which side is faster.

  python tools/time_mcep.py [--out profiles/mcep_timing.json] [--blocks 7] [--calls 20]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_mcep.py --profile-pass     (a run of its own)
"""
import argparse
import json
import os
import statistics
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)

FP32_MATRIX_FLOPS = 155e12
FS, N_FFT, HOP, ORDER, ALPHA, FLOOR = 22050, 1024, 110, 49, 0.455, 1e-5


def op_flops(rows, frames):
    bins_padded = (N_FFT // 2 + 1 + 3) & ~3
    tiles = (ORDER + 1 + 15) // 16
    return 2 * rows * frames * (2 * (N_FFT // 2) * (N_FFT // 2 + 1) + bins_padded * 16 * tiles)


def setup():
    import torch
    from shallow_wavenet_amd import melspec
    assert torch.cuda.is_available(), "needs a HIP device"
    ext = melspec.MelCepstrumExtractor(FS, N_FFT, HOP, ORDER, ALPHA, floor=FLOOR, device="cuda")
    G = torch.from_numpy(melspec.mcep_matrix(N_FFT, ORDER, ALPHA).astype("float32")).cuda()
    win = torch.hann_window(N_FFT, periodic=True).cuda()

    def torch_mcep(x):
        a = torch.stft(x, N_FFT, hop_length=HOP, window=win, center=True, pad_mode="reflect", return_complex=True).abs()
        return torch.matmul(G, a.clamp(min=FLOOR).log()).transpose(1, 2)

    g = torch.Generator().manual_seed(0)
    x64 = (0.3 * torch.tanh(torch.randn(64, 66000, generator=g))).cuda()
    return torch, ext, torch_mcep, x64


def measure(blocks, calls):
    torch, ext, torch_mcep, x64 = setup()
    x1 = x64[:1].contiguous()
    cases = {"1x66000": {"hip": lambda: ext(x1), "torch": lambda: torch_mcep(x1)},
             "64x66000": {"hip": lambda: ext(x64), "torch": lambda: torch_mcep(x64)}}

    def run(fn, n):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(n):
            fn()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / n

    out = {}
    for name, paths in cases.items():
        for fn in paths.values():
            run(fn, 5)                                              # warm-up of every shape
        ms = {p: [] for p in paths}
        for _ in range(blocks):
            for p, fn in paths.items():
                ms[p].append(run(fn, calls))
        out[name] = {p: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for p, v in ms.items()}
        out[name]["faster"] = min(paths, key=lambda p: out[name][p]["median_ms"])
        print(name, json.dumps(out[name]), flush=True)
    frames = 1 + 66000 // HOP
    for name, rows in (("1x66000", 1), ("64x66000", 64)):
        out[name]["hip_flop"] = op_flops(rows, frames)
        out[name]["hip_fraction_of_fp32_matrix_rate"] = out[name]["hip_flop"] / (out[name]["hip"]["median_ms"] * 1e-3) / FP32_MATRIX_FLOPS
    with torch.no_grad():
        a, b = ext(x64), torch_mcep(x64)
        out["64x66000"]["max_abs_difference_of_the_two_paths"] = float((a - b).abs().max())
        out["64x66000"]["shape"] = list(a.shape)
    out["geometry"] = {"fs": FS, "n_fft": N_FFT, "hop": HOP, "order": ORDER, "alpha": ALPHA, "blocks": blocks,
                       "calls_per_block": calls}
    out["device"] = torch.cuda.get_device_name(0)
    return out


def profile_pass(calls):
    """the calls of the two shapes, untimed, for a kernel trace"""
    torch, ext, torch_mcep, x64 = setup()
    x1 = x64[:1].contiguous()
    for fn in (lambda: ext(x1), lambda: torch_mcep(x1), lambda: ext(x64), lambda: torch_mcep(x64)):
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "mcep_timing.json"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    if a.profile_pass:
        profile_pass(a.calls)
        return
    if a.blocks < 7:
        ap.error("at least 7 repetitions")
    res = measure(a.blocks, a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
