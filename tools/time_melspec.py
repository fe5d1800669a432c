"""dev tool: what log-mel features cost on the device, through the HIP operator (melspec.LogMelExtractor / LogMelStream,
csrc/swn_melspec.hip) and through the same definition composed from torch on the same device (torch.stft with the periodic
Hann window, centre, reflect; abs; matmul with the same fp32 filter bank; clamp; log), at fs 22 050, n_fft 1024, hop 110,
80 mels:

  - 1 x 66 000 and 64 x 66 000 samples, one call each;
  - a LogMelStream.push of 50 ms (1 102 samples) in the steady state, against the torch composition over the same tail
    buffer (center=False over the samples the new frames read).

Device events around `calls` calls, the two paths alternating block by block in one run, median [min - max] over the blocks
of the per-call mean; the largest difference between the two paths' outputs is recorded with the times.  The operator's
arithmetic, counted from the shapes as it runs it (each frame folded once: (re, im) x frames x n / 2 x bins multiply-adds),
over its time, as a fraction of the 155 TFLOP/s fp32 matrix rate.

  python tools/time_melspec.py [--out profiles/melspec_timing.json] [--blocks 7] [--calls 20]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_melspec.py --profile-pass     (a run of its own)
"""
import argparse
import json
import os
import statistics
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)

FP32_MATRIX_FLOPS = 155e12
FS, N_FFT, HOP, N_MELS, FLOOR = 22050, 1024, 110, 80, 1e-5
PUSH = 1102                     # 50 ms


def op_flops(rows, frames):
    return 2 * 2 * rows * frames * (N_FFT // 2) * (N_FFT // 2 + 1)


def setup():
    import torch
    from shallow_wavenet_amd import melspec
    assert torch.cuda.is_available(), "needs a HIP device"
    ext = melspec.LogMelExtractor(FS, N_FFT, HOP, N_MELS, floor=FLOOR, device="cuda")
    W = torch.from_numpy(melspec.mel_filterbank(FS, N_FFT, N_MELS).astype("float32")).cuda()
    win = torch.hann_window(N_FFT, periodic=True).cuda()

    def torch_logmel(x, center=True):
        a = torch.stft(x, N_FFT, hop_length=HOP, window=win, center=center, pad_mode="reflect", return_complex=True).abs()
        return torch.matmul(W, a).clamp(min=FLOOR).log().transpose(1, 2)

    g = torch.Generator().manual_seed(0)
    x64 = (0.3 * torch.tanh(torch.randn(64, 66000, generator=g))).cuda()
    return torch, melspec, ext, torch_logmel, x64


def stream_pair(torch, melspec, ext, torch_logmel, x):
    """steady state of a stream: `hip()` pushes the next 50 ms into a LogMelStream; `tor()` appends them to a tail buffer and
    evaluates the torch composition on the frames they complete.  Both restart when the signal is used up."""
    state = {"hip": None, "hip_at": 0, "buf": None, "tor_at": 0, "frames": 0, "t0": 0}

    def restart_hip():
        state["hip"] = melspec.LogMelStream(ext)
        state["hip"].push(x[:4 * PUSH])
        state["hip_at"] = 4 * PUSH

    def hip():
        if state["hip"] is None or state["hip_at"] + PUSH > x.numel():
            restart_hip()
        out = state["hip"].push(x[state["hip_at"]:state["hip_at"] + PUSH])
        state["hip_at"] += PUSH
        return out

    def restart_tor():
        n = 4 * PUSH
        state["frames"] = 1 + (n - N_FFT // 2) // HOP
        state["t0"] = state["frames"] * HOP - N_FFT // 2
        state["buf"], state["tor_at"] = x[state["t0"]:n], n

    def tor():
        if state["buf"] is None or state["tor_at"] + PUSH > x.numel():
            restart_tor()
        buf = torch.cat([state["buf"], x[state["tor_at"]:state["tor_at"] + PUSH]])
        state["tor_at"] += PUSH
        k = (buf.numel() - N_FFT) // HOP + 1                      # frames the buffer completes
        out = torch_logmel(buf[None, :(k - 1) * HOP + N_FFT], center=False)[0]
        state["frames"] += k
        state["buf"] = buf[k * HOP:]
        return out

    return hip, tor


def measure(blocks, calls):
    torch, melspec, ext, torch_logmel, x64 = setup()
    x1 = x64[:1].contiguous()
    hip_push, tor_push = stream_pair(torch, melspec, ext, torch_logmel, x64[1].contiguous())
    cases = {"1x66000": {"hip": lambda: ext(x1), "torch": lambda: torch_logmel(x1)},
             "64x66000": {"hip": lambda: ext(x64), "torch": lambda: torch_logmel(x64)},
             "stream_push_50ms": {"hip": hip_push, "torch": tor_push}}

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
        print(name, json.dumps(out[name]), flush=True)
    frames = 1 + 66000 // HOP
    for name, rows in (("1x66000", 1), ("64x66000", 64)):
        out[name]["hip_flop"] = op_flops(rows, frames)
        out[name]["hip_fraction_of_fp32_matrix_rate"] = out[name]["hip_flop"] / (out[name]["hip"]["median_ms"] * 1e-3) / FP32_MATRIX_FLOPS
    with torch.no_grad():
        a, b = ext(x64), torch_logmel(x64)
        out["64x66000"]["max_abs_difference_of_the_two_paths"] = float((a - b).abs().max())
        out["64x66000"]["shape"] = list(a.shape)
    out["geometry"] = {"fs": FS, "n_fft": N_FFT, "hop": HOP, "n_mels": N_MELS, "push_samples": PUSH, "blocks": blocks,
                       "calls_per_block": calls}
    out["device"] = torch.cuda.get_device_name(0)
    return out


def profile_pass(calls):
    """the calls of the three shapes, untimed, for a kernel trace"""
    torch, melspec, ext, torch_logmel, x64 = setup()
    x1 = x64[:1].contiguous()
    hip_push, tor_push = stream_pair(torch, melspec, ext, torch_logmel, x64[1].contiguous())
    for fn in (lambda: ext(x1), lambda: torch_logmel(x1), lambda: ext(x64), lambda: torch_logmel(x64), hip_push, tor_push):
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "melspec_timing.json"))
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
