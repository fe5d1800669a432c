"""The grid of conv_aux geometries over which the front end (scale_in -> conv_aux -> hoisted in_x GEMM) is pinned to float64,
shared by tests/test_frontend_geometry_host.py (CPU: which path every row reaches, the oracle's own fp32 error),
tests/test_gpu_frontend_geometry.py (the kernels) and tools/measure_frontend_deviation.py.

csrc/swn_frontend.hip serves a conv_aux layer by one of four paths, reported by swn_frontend_conv_lds_bytes:
  staged       k = 3 and 4 * cin * (64 + 2 * dil + 48) <= 48 KB of dynamic LDS
  attribute    the same kernel above 48 KB, after raising its dynamic LDS limit (a high-water mark in the launch code)
  unstaged3    k = 3 above 150 KB: conv1d_same_kernel with ks == 3
  generic      any other k > 1: the run-time tap loop (k = 1 takes conv1d_same_kernel's ks == 1 instance)
Every row names the path of its largest layer.  k3l4_a8 puts the dilation-27 layer through the staged kernel (a window of 118
of the 128 columns a wave pair stages), k3l4_a9 the same layer through the unstaged one.  The stack behind a row is as small as the library accepts and varies so that
the edges of cond_gemm_kernel are met: N = L * seg * 2H off a multiple of 4 (scalar stores), N <= 64, a partial second n-tile,
A0 below 16, at 16 and at a multiple of 16, a softmax net and a Laplace net with the (seg, 1) Conv2d folded into in_x.

Weights come from synth_state_dict and features from synth_aux: nothing is stored."""
import ctypes
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from shallow_wavenet_amd.config import NetConfig
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

LDS_DEFAULT, LDS_MAX = 48 * 1024, 150 * 1024
TILE = 64                                       # frames per workgroup of every front end kernel
PROD_LDS = 76464                                # the attribute request of the 54-feature production nets (layer 1)

Row = namedtuple("Row", "id cfg path lds wseed flavor")


def _lap(n_aux, k, l, hid, dd, dr, seg=1, lpc=0, c2d=False, skip=4, K=2):
    return NetConfig(kind="laplace", n_aux=n_aux, hid_chn=hid, skip_chn=skip, aux_kernel_size=k, aux_dilation_size=l,
                     dilation_depth=dd, dilation_repeat=dr, kernel_size=K, upsampling_factor=4, seg=seg, lpc=lpc,
                     wav_conv_flag=False, aux_conv2d_flag=c2d)


def _smx(n_aux, k, l, hid, dd, dr, Q=8, audio_in=False, skip=4, K=2):
    return NetConfig(kind="softmax", n_aux=n_aux, hid_chn=hid, skip_chn=skip, aux_kernel_size=k, aux_dilation_size=l,
                     dilation_depth=dd, dilation_repeat=dr, kernel_size=K, upsampling_factor=4, n_quantize=Q,
                     wav_conv_flag=False, audio_in_flag=audio_in)


# id, cfg, path of the largest layer, largest dynamic LDS request of the row (0 = no layer staged)   N     A0
ROWS = (
    Row("k3l1_a1", _lap(1, 3, 1, 5, 3, 1), "staged", 456, 11, "xavier"),                     # 30      3  (A0p = 4)
    Row("k3l4_a9", _lap(9, 3, 4, 36, 3, 1, seg=2, lpc=2), "unstaged3", 42120, 12, "trained"), # 432   729
    Row("k3l4_a8", _lap(8, 3, 4, 6, 2, 1), "attribute", 143424, 22, "xavier"),                 # 24    648  staged at dilation 27
    Row("k3l3_a12", _smx(12, 3, 3, 8, 2, 1), "attribute", 56160, 13, "xavier"),                # 32    324
    Row("k3l3_a20", _lap(20, 3, 3, 4, 1, 1), "attribute", 93600, 14, "trained"),              # 8     540
    Row("k3l3_a32", _lap(32, 3, 3, 20, 2, 1), "attribute", 149760, 15, "xavier"),             # 80    864 = 54 * 16
    Row("k3l3_a33", _lap(33, 3, 3, 7, 1, 1), "unstaged3", 46728, 16, "trained"),              # 14    891
    Row("k5l3_a2", _lap(2, 5, 3, 8, 2, 1, seg=2, lpc=1, c2d=True), "generic", 0, 17, "trained"),   # 64  250
    Row("k5l4_a1", _lap(1, 5, 4, 17, 2, 1), "generic", 0, 18, "xavier"),                      # 68    625
    Row("k7l1_a2", _smx(2, 7, 1, 6, 1, 1, Q=6, audio_in=True), "generic", 0, 19, "xavier"),    # 12     14
    Row("k1l4_a5", _lap(5, 1, 4, 5, 3, 1, seg=3, lpc=2), "k1", 0, 20, "trained"),             # 90      5
    Row("k1l1_a16", _lap(16, 1, 1, 4, 1, 1), "k1", 0, 21, "xavier"),                          # 8      16
)
BY_ID = {r.id: r for r in ROWS}

# staged, attribute, attribute with the widest staged window (dilation 27: 118 of the 128 columns a wave pair stages, so 54
# lanes write a second column), unstaged3, generic, k = 1
CROP_ROWS = ("k3l1_a1", "k3l3_a20", "k3l4_a8", "k3l4_a9", "k5l3_a2", "k1l4_a5")
HIGH_WATER = ("k3l3_a12", "k3l3_a20", "k3l3_a32", "k3l3_a12")
POOL_ROWS = ("k3l4_a9", "k3l3_a12", "k5l3_a2", "k5l4_a1", "k7l1_a2", "k1l4_a5", "k3l1_a1",
             "k3l3_a32")                        # ... whose taps per output, 96 / 288 / 864, are whole passes of the pool kernel
MODELS_ROWS = ("k5l3_a2", "k3l4_a9")
STREAM_ROWS = ("k5l3_a2", "k1l4_a5")


# ------------------------------------------------------------------------------------------------------------ geometry
def seg_of(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


def cond_width(cfg):
    """N: floats per frame of cond"""
    return cfg.L * seg_of(cfg) * 2 * cfg.H


def layers(cfg):
    """(cin, cout, dilation, half-width) of every conv_aux layer"""
    k, n = cfg.aux_kernel_size, cfg.n_aux
    return [(n * k ** i, n * k ** (i + 1), k ** i, k ** i * (k - 1) // 2) for i in range(cfg.aux_dilation_size)]


def lookahead(cfg):
    return sum(h for _, _, _, h in layers(cfg))


def max_dilation(cfg):
    return max(d for _, _, d, _ in layers(cfg))


def lds_formula(cin, dil):
    """bytes conv1d_same_lds_kernel needs: the window of 64 + 2 * dil columns and 3 x 16 weights per input channel"""
    return 4 * cin * (TILE + 2 * dil + 48)


def expected_lds(cfg, i):
    """what swn_frontend_conv_lds_bytes must report for layer i"""
    cin, _, dil, _ = layers(cfg)[i]
    b = lds_formula(cin, dil)
    return b if cfg.aux_kernel_size == 3 and b <= LDS_MAX else 0


def query_lds(lib, cfg, i):
    from shallow_wavenet_amd import _lib
    d = _lib.desc_from_cfg(cfg)
    return int(lib.swn_frontend_conv_lds_bytes(ctypes.byref(d), i))


def frame_counts(cfg):
    """n_frames of the one-shot checks: around the largest dilation (a layer whose every tap is padding), the look-ahead, the
    64-frame tile and a halo that crosses from the last full tile into a partial one"""
    d, la = max_dilation(cfg), lookahead(cfg)
    return sorted({1, 2, d, d + 1, la + 1, 63, 64, 65, 64 + d, 65 + d, 130})


def pool_lengths(cfg):
    """utterance lengths of the pool check (an utterance has at least one frame; equal lengths get different features)"""
    d, la = max_dilation(cfg), lookahead(cfg)
    return [n for n in (1, 2, la, la + 1, 65, 64 + d, 130) if n > 0]


# ------------------------------------------------------------------------------------------------------- weights, oracle
_SD = {}


def state_dict(row):
    if row.id not in _SD:
        _SD[row.id] = synth_state_dict(row.cfg, seed=row.wseed, flavor=row.flavor)
    return _SD[row.id]


def params(row, dtype=torch.float32):
    return cpu_ref.as_params(state_dict(row), dtype)


def features(cfg, batch, n_frames, seed=1):
    """(B, n_aux, Tf) fp32; with batch > 1 every utterance is drawn on its own, so that utterance b is features(cfg, 1, Tf,
    seed + b)"""
    return torch.from_numpy(np.concatenate([synth_aux(cfg, 1, n_frames, seed=seed + b) for b in range(batch)], 0))


def stages(cfg, P, aux):
    """the activations of cpu_ref.frontend in the dtype of P: [scale_in output, every conv_aux layer's output], each
    (B, channels, Tf), and cond (B, Tf, N) by the einsum of test_gpu_offgrid_geometry.test_frontend_matches_float64"""
    dt = P["scale_in.weight"].dtype
    with torch.no_grad():
        c = F.conv1d(aux.to(dt), P["scale_in.weight"], P["scale_in.bias"])
        out = [c]
        for i, (_, _, dil, half) in enumerate(layers(cfg)):
            c = F.conv1d(c, P[f"conv_aux.conv.{i}.weight"], P[f"conv_aux.conv.{i}.bias"], dilation=dil, padding=half)
            out.append(c)
        seg = seg_of(cfg)
        conv2d = cfg.kind == "laplace" and cfg.aux_conv2d_flag and cfg.seg > 1
        rows = []
        for l in range(cfg.L):
            w = P[f"in_x.{l}.weight"][:, :, 0]
            if conv2d:      # in_x after the (seg,1) Conv2d: W_eff[o][c][s] = sum_p in_x.W[o][p] * conv2d.W[p][c][s]
                w = torch.einsum("op,pcs->ocs", w, P["aux_conv2d.weight"][:, :, :, 0])
            else:
                w = w[:, : cfg.A0 * seg].reshape(2 * cfg.H, cfg.A0, seg)
            rows.append(torch.einsum("ocs,bcf->bfso", w, c))                 # B,Tf,seg,2H
        cond = torch.stack(rows, 2).reshape(aux.shape[0], aux.shape[2], cond_width(cfg))
    return out, cond


def stage_names(cfg):
    return ["scale_in"] + [f"conv_aux.{i}" for i in range(cfg.aux_dilation_size)] + ["cond"]


_REF = {}


def reference(row, batch, n_frames, seed=1):
    """float64 stages + cond of features(row.cfg, batch, n_frames, seed), and per stage (e32, scale): the max-abs deviation of
    the same run with fp32 parameters from it, and the float64 stage's max-abs.  Made once per shape and left unchanged."""
    key = (row.id, batch, n_frames, seed)
    if key not in _REF:
        aux = features(row.cfg, batch, n_frames, seed)
        s64, c64 = stages(row.cfg, params(row, torch.float64), aux)
        s32, c32 = stages(row.cfg, params(row), aux)
        ref = s64 + [c64]
        figs = [(float((a.double() - b).abs().max()), float(b.abs().max())) for a, b in zip(s32 + [c32], ref)]
        _REF[key] = (aux, ref, figs)
    return _REF[key]


# --------------------------------------------------------------------------------------------------------------- device
TAIL, SENTINEL = 4096, 12345.5


def device_stages(net, aux):
    """swn_frontend through the C ABI on `work` and `cond` full of NaN, each with a tail of TAIL sentinel floats behind it:
    -> ([scale_in output, every conv_aux layer's output] as (B, channels, Tf), cond (B, Tf, N)), float32 on the host.
    Every float of both buffers must have been written and both tails must be untouched."""
    from shallow_wavenet_amd import _lib
    L, cfg, dev = _lib.lib(), net.cfg, net.packed.device
    desc = ctypes.byref(net.desc)
    B, na, Tf = aux.shape
    assert na == cfg.n_aux
    nw, nc = int(L.swn_frontend_work_floats(desc, B, Tf)), int(L.swn_cond_floats(desc, B, Tf))
    chans = [cfg.n_aux] + [cout for _, cout, _, _ in layers(cfg)]
    assert nw == B * Tf * sum(chans) and nc == B * Tf * cond_width(cfg)
    bufs = []
    for n in (nw, nc):
        t = torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device=dev)
        t[n:] = SENTINEL
        bufs.append(t)
    work, cond = bufs
    a = aux.to(dev, torch.float32).contiguous()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        rc = L.swn_frontend(desc, p(net.packed), p(a), B, Tf, p(work), p(cond),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    assert rc == 0, (rc, L.swn_last_error_detail().decode())
    work, cond = work.cpu(), cond.cpu()
    for what, t, n in (("work", work, nw), ("cond", cond, nc)):
        assert bool((t[n:] == SENTINEL).all()), f"{what}: the floats behind the buffer were written"
        assert not bool(torch.isnan(t[:n]).any()), f"{what}: floats of the buffer were never written"
    out, at = [], 0
    for c in chans:
        out.append(work[at:at + B * c * Tf].view(B, c, Tf))
        at += B * c * Tf
    return out, cond[:nc].view(B, Tf, cond_width(cfg))


def stage_errors(row, got, batch, n_frames, seed=1):
    """[(stage, error, bound, e32, scale)] of device_stages' result against reference()"""
    _, ref, figs = reference(row, batch, n_frames, seed)
    stages_, cond = got
    return [(what, float((g.double() - r).abs().max()), bound(e32, scale), e32, scale)
            for what, g, r, (e32, scale) in zip(stage_names(row.cfg), list(stages_) + [cond], ref, figs)]


TOL, ORDER, CAP = 2e-6, 4.0, 1e-4


def bound(e32, scale):
    """the kernel's bound for a stage: the rule of test_gpu_offgrid_geometry._bound over the front end tolerance there"""
    return max(TOL * max(1.0, scale), ORDER * e32)
