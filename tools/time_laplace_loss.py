"""dev tool: what the Laplace terms of the stage-7 loss cost between the stack and the spectral terms, as torch ops on the
head's outputs (the default path of train_driver.batch_loss) and through the HIP operator (laplace_loss.LaplaceChunkLoss), at
the recipe's size (seg 5, lpc 4, 8 114 kept positions):

  - the Laplace part alone on the same inputs, forward (no_grad) and forward + backward: `batch_loss` on a stub model that
    holds a fixed raw tensor (the torch path runs the head op, its flag round trip and the assembly; the hip path the
    operator) and a stub spectral loss (a linear functional of the sample rows, so that the backward carries both upstream
    gradients); wall clock per call with one synchronisation per block of calls, the two paths alternating block by block;
  - the stage-7 chunk as the driver runs it (slice, batch_loss with --spectral_loss hip, backward, Adam, the .item() calls
    of the log line), REF6 and BL6 geometry at seg 5 / lpc 4, bf16 and fp32, `laplace_loss` None and the operator alternating
    chunk by chunk in one process on the same model, wall clock per chunk;
  - with --parent-tree, the driver of the parent commit against this tree's `--laplace_loss torch` and `hip`, one fresh
    process per run, alternating (the check that `torch` still is the parent's path).

  python tools/time_laplace_loss.py [--out profiles/laplace_loss_timing.json] [--blocks 5] [--calls 40] [--chunks 120]
                                    [--driver-runs 2] [--driver-iters 40] [--parent-tree DIR]
"""
import argparse
import json
import logging
import os
import re
import statistics
import subprocess
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)

GEOMETRIES = {"ref6": [], "bl6": ["--hid_chn", "64", "--skip_chn", "128", "--dilation_depth", "6", "--dilation_repeat", "1",
                                  "--kernel_size", "2"]}


def _summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


class _StubModel:
    """a fixed raw tensor behind the two model calls of batch_loss: forward_raw, and the tail of CSWNV.forward(clip=True)"""

    def __init__(self, raw, seg, lpc):
        import types
        from shallow_wavenet_amd import ops
        from shallow_wavenet_amd.config import NetConfig
        self.raw, self.seg, self.lpc, self.receptive_field = raw, seg, lpc, 0
        cfg = NetConfig(kind="laplace", seg=seg, lpc=lpc)
        dlist = ops.desc_list(cfg)
        self.net = types.SimpleNamespace(cfg=cfg, dlist=dlist, laplace_head_backward=lambda raw, *g: ops.laplace_head_backward_impl(raw, *g, dlist))

    def forward_raw(self, aux, audio, do=False):
        return self.raw

    def __call__(self, aux, audio, do=False, clip=False):
        import torch
        from shallow_wavenet_amd import ops
        from shallow_wavenet_amd.nets._autograd import LaplaceHeadFunction
        if torch.is_grad_enabled() and self.raw.requires_grad:
            mu, b, log_b, a, b_clip, log_b_clip, flag = LaplaceHeadFunction.apply(self.net, self.raw, clip)
        else:
            mu, b, log_b, a, b_clip, log_b_clip, flag = ops.laplace_head(self.raw.detach(), self.net.dlist, clip)
        tail = (a,) if self.lpc > 0 else ()
        if int(flag.item()) != 0:
            return (mu, b, b_clip, log_b_clip) + tail
        return (mu, b, b, log_b) + tail


class _StubSpectral:
    def __init__(self, w):
        self.w = w

    def sizes_for(self, feat_len):
        return [128]

    def __call__(self, samples, targets, feat_len):
        import torch
        s = samples if torch.is_tensor(samples) else torch.stack(list(samples))
        l1 = (s * self.w).sum(1, keepdim=True)
        return l1, torch.ones_like(l1).detach()


def time_op(blocks, calls, seg=5, lpc=4, N=8114):
    import torch
    from shallow_wavenet_amd import train_driver as T
    from shallow_wavenet_amd.laplace_loss import LaplaceChunkLoss
    from shallow_wavenet_amd.nets.cswnv_shift1 import LaplaceLoss, LSDloss
    assert torch.cuda.is_available(), "needs a HIP device"
    g = torch.Generator().manual_seed(0)
    raw = torch.randn(1, 2 * seg + lpc, N, generator=g)
    raw[:, :seg] *= 0.3
    raw[:, seg:2 * seg] = raw[:, seg:2 * seg] * 2 - 3
    raw[:, 2 * seg:] *= 0.4
    raw = raw.cuda().requires_grad_(True)
    target = torch.tanh(torch.randn(N + seg - 1, generator=g)).cuda()
    x_prob = torch.tanh(torch.randn(1, N + seg + lpc - 1, generator=g)).cuda()
    model, spec = _StubModel(raw, seg, lpc), _StubSpectral((torch.randn(seg, N, generator=g) / N).cuda())
    crit, lsd = LaplaceLoss(), LSDloss()
    paths = {"torch": None, "hip": LaplaceChunkLoss(seg, lpc)}

    def call(path):
        return T.batch_loss(model, crit, lsd, None, None, target, x_prob, N, 0, [128], [None], do=False, eps_on_device=True,
                            spectral_loss=spec, laplace_loss=paths[path])[0]

    def run(path, backward, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            if backward:
                raw.grad = None
                call(path).backward()
            else:
                with torch.no_grad():
                    call(path)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    out = {}
    for backward in (False, True):
        for p in paths:
            run(p, backward, 5)
        ms = {p: [] for p in paths}
        for _ in range(blocks):
            for p in paths:
                ms[p].append(run(p, backward, calls))
        out["forward_backward" if backward else "forward"] = {p: _summary(v) for p, v in ms.items()}
    out["shape"] = {"seg": seg, "lpc": lpc, "positions": N, "blocks": blocks, "calls_per_block": calls}
    out["note"] = "wall clock per batch_loss call on a fixed raw tensor, log line included (INFO enabled), stub spectral term"
    return out


def time_chunks_alternating(geometry, precision, chunks, warm=10):
    """the driver's chunk (train_driver._run's loop body) on one model, laplace_loss None / operator alternating per chunk"""
    import numpy as np
    import torch
    from shallow_wavenet_amd import train_driver as T
    from shallow_wavenet_amd.laplace_loss import LaplaceChunkLoss
    from shallow_wavenet_amd.nets.cswnv_shift1 import CSWNV, LaplaceLoss, LSDloss, initialize
    from shallow_wavenet_amd.runtime import train_precision
    from shallow_wavenet_amd.spectral import MultiResolutionSTFTLoss
    args = T.build_parser().parse_args(["--expdir", "unused", "--synthetic", "6", "--seg", "5", "--lpc", "4", "--do_prob", "0.5",
                                        "--wav_conv_flag", "true"] + GEOMETRIES[geometry])
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    with train_precision(precision):
        model = CSWNV(n_aux=args.n_aux, skip_chn=args.skip_chn, hid_chn=args.hid_chn, dilation_depth=args.dilation_depth,
                      dilation_repeat=args.dilation_repeat, kernel_size=args.kernel_size, aux_kernel_size=args.aux_kernel_size,
                      aux_dilation_size=args.aux_dilation_size, do_prob=args.do_prob, seg=args.seg, lpc=args.lpc,
                      aux_conv2d_flag=args.aux_conv2d_flag, wav_conv_flag=args.wav_conv_flag,
                      upsampling_factor=args.upsampling_factor)
        model.dropout_source = "device"
        crit, lsd = LaplaceLoss().cuda(), LSDloss().cuda()
        dev = torch.device("cuda")
        wavs, feats, loader = T.synthetic_corpus(args.synthetic, args.n_aux, args.upsampling_factor, seed=args.seed)
        model.cuda().train()
        model.apply(initialize)
        T.set_scale_in(model, np.zeros(args.n_aux), np.ones(args.n_aux))
        opt = T.make_adam(T.optimizer_parameters(model), args.lr)
        gen = T.train_generator(wavs, feats, model.receptive_field, args.string_path, args.batch_size, model.seg, True,
                                args.upsampling_factor, dev, loader)
        fft = T.fft_sizes(args.n_fft_facts)
        spectral = MultiResolutionSTFTLoss(fft, dev)
        paths = {"torch": None, "hip": LaplaceChunkLoss(model.seg, model.lpc)}
        ms = {p: [] for p in paths}
        i = 0
        while i < 2 * (chunks + warm):
            x, h, c_idx, utt_idx, wavfile, h_bs, x_bs, h_ss, x_ss = next(gen)
            if c_idx < 0 or h_bs < 0:                           # epoch marker / the short tail chunk of an utterance
                continue
            path = ("torch", "hip")[i % 2]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bh, bx, trg, xp, flen = T.slice_chunk(model, x, h, h_bs, x_bs, h_ss, x_ss)
            loss, l_lap, l_lsd, l_err = T.batch_loss(model, crit, lsd, bh, bx, trg, xp, flen, h_ss, fft, [None] * len(fft),
                                                     do=True, eps_on_device=True, spectral_loss=spectral,
                                                     laplace_loss=paths[path])
            opt.zero_grad()
            loss.backward()
            opt.step()
            figures = (l_err.item(), l_lap.item(), l_lsd.item() if l_lsd is not None else None)
            torch.cuda.synchronize()
            if i >= 2 * warm:
                ms[path].append(1e3 * (time.perf_counter() - t0))
            assert all(f is None or np.isfinite(f) for f in figures), figures
            i += 1
    out = {p: dict(_summary(v), mean_ms=statistics.mean(v)) for p, v in ms.items()}
    out["chunks_per_path"] = chunks
    return out


# tools/time_driver.py's run (same flags), printing every chunk time the driver logged
_CHUNK_CHILD = """
import sys, re, io, logging, tempfile
sys.path.insert(0, sys.argv[1])
from shallow_wavenet_amd import train_driver as T
buf = io.StringIO()
logging.getLogger().addHandler(logging.StreamHandler(buf)); logging.getLogger().setLevel(logging.INFO)
with tempfile.TemporaryDirectory() as d:
    T.main(["--expdir", d, "--synthetic", "6", "--max_iters", sys.argv[3], "--seg", "5", "--lpc", "4", "--do_prob", "0.5",
            "--wav_conv_flag", "true", "--precision", sys.argv[2], "--GPU_device", "0", "--verbose", "1",
            "--spectral_loss", "hip"] + sys.argv[4:])
print("CHUNKS", " ".join(re.findall(r"\\((\\d+\\.\\d+) sec\\)", buf.getvalue())))
"""


def _driver_ms(root, prec, iters, extra):
    """mean ms per chunk past the first five of one driver run in a fresh process (the log line carries whole ms)"""
    r = subprocess.run([sys.executable, "-c", _CHUNK_CHILD, root, prec, str(iters)] + extra, capture_output=True, text=True,
                       timeout=600, cwd=root)
    m = re.search(r"^CHUNKS (.+)$", r.stdout, re.M)
    if r.returncode != 0 or not m:
        raise RuntimeError(f"driver run {root} {prec} {extra} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    secs = [float(v) for v in m.group(1).split()]
    return 1e3 * statistics.mean(secs[5:] if len(secs) > 10 else secs)


def time_driver_runs(runs, iters, parent_tree):
    out = {}
    for prec in ("bf16", "fp32"):
        ms = {"torch": [], "hip": []}
        if parent_tree:
            ms["parent_commit"] = []
        for _ in range(runs):
            for path in ms:
                if path == "parent_commit":
                    ms[path].append(_driver_ms(os.path.abspath(parent_tree), prec, iters, []))
                else:
                    ms[path].append(_driver_ms(_R, prec, iters, ["--laplace_loss", path]))
                print(f"driver {prec} {path}: {ms[path][-1]:.2f} ms", flush=True)
        out[prec] = {p: _summary(v) for p, v in ms.items()}
    out["runs"], out["chunks_per_run"] = runs, iters
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "laplace_loss_timing.json"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--chunks", type=int, default=120, help="timed chunks per path of an alternating run (0: skip)")
    ap.add_argument("--driver-runs", type=int, default=2, help="fresh driver processes per path and precision (0: skip)")
    ap.add_argument("--driver-iters", type=int, default=40)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: time its driver as well")
    a = ap.parse_args()
    logging.getLogger().addHandler(logging.NullHandler())
    logging.getLogger().setLevel(logging.INFO)                  # the log lines are formatted as under the driver's --verbose 1
    import torch
    res = {"device": torch.cuda.get_device_name(0), "laplace_part": time_op(a.blocks, a.calls)}
    print(json.dumps(res["laplace_part"]), flush=True)
    if a.chunks > 0:
        res["stage7_chunk_alternating"] = {}
        for geometry in GEOMETRIES:
            for prec in ("bf16", "fp32"):
                r = res["stage7_chunk_alternating"][f"{geometry}_{prec}"] = time_chunks_alternating(geometry, prec, a.chunks)
                print(f"chunk {geometry} {prec}: {json.dumps(r)}", flush=True)
    if a.driver_runs > 0:
        res["stage7_driver_ref6"] = time_driver_runs(a.driver_runs, a.driver_iters, a.parent_tree)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
