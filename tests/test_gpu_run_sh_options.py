"""The run.sh options away from the defaults - fs 16 / 24 / 44.1 / 48 kHz (upsampling factor U = 80 / 120 / 220 / 240), seg 2 / 10,
lpc 0 - on the kernels the launchers pick for exactly these options, where the golden fixtures cannot reach (synthetic weights,
the CPU oracle or the fp32 kernels as the reference):

  * BL6 decode across rates (wave-specialised 2, symmetric 6, generic 1, stepped 3) against the oracle, 1e-5;
  * REF6 seg 10: H * seg = 1920 > 1024 (and NO = 24 > 16), so the stepped chain runs its generic Laplace tail
    (step_tail_kernel<LAPLACE>) and, streamed or pooled, its <LAPLACE, true> / <LAPLACE, true, true> forms: bit-identical to the
    one-shot / solo decodes, and a pooled run replays in the oracle;
  * the bf16 GEMM stack at other U, seg 10 (ten conditioning taps per position) and both gate8 tile widths, the BL6 bf16 stack at
    U > 112 (more than 7 chunks per frame) and at seg 10, against the fp32 kernels at 3e-3 max / 3e-4 mean of the output scale;
  * (CPU) the routing table: which kernel the C ABI picks for every configuration above, so a dispatch change that reroutes one
    of them - and takes it out of reach of these tests - fails here.
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from shallow_wavenet_amd import _lib
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

DEV = "cuda:0"


def _u(cfg, U):
    return dataclasses.replace(cfg, upsampling_factor=U)


# ---- routing table (CPU) -------------------------------------------------------------------------------------------------------
# name -> (config, swn_decode_resolve_variant for variants (0, 2, 3, 6) at batch 1 and at batch 27,
#          swn_bf16_train_forward_supported, swn_backward_bf16_work_floats(batch 2, 9 frames) > 0)
# decode: 1 generic persistent kernel (decode_generic_kernel<SEGT>: seg 3 -> <5>, seg 10 -> <10>), 2 the BL6 fast kernels
# (bl6w / bl6), 3 the stepped chain, 6 the symmetric BL6 kernel, -4 SWN_E_UNSUPPORTED (no such kernel for the net)
NO_BL6 = (1, -4, 3, -4)          # BL6 class without a BL6 kernel (seg 10, seg 2 with lpc 0) and the tiny nets: the generic kernel
BL6 = (2, 2, 3, 6)
REF6 = (3, -4, 3, -4)            # auto = the stepped chain (its generic Laplace tail where H * seg > 1024 or NO > 16)
ROUTES = {
    "tiny_s10l4": (C.tiny("laplace", 10, 4), NO_BL6, 0, False),
    "tiny_s3l0": (C.tiny("laplace", 3, 0), NO_BL6, 0, False),
    "bl6_s10l4": (C.bl6_laplace(10, 4), NO_BL6, 1, False),
    "bl6_s2l0": (C.bl6_laplace(2, 0), NO_BL6, 1, False),
    "bl6_u256_s10l4": (_u(C.bl6_laplace(10, 4), 256), NO_BL6, 1, False),
    "ref6_s5l4": (C.ref6_laplace(5, 4), REF6, 1, False),
    "ref6_c2d_s2l4": (dataclasses.replace(C.ref6_laplace(2, 4), aux_conv2d_flag=True), REF6, 1, False),
}
for _U in (80, 120, 220, 240):
    for _lpc in (0, 4):
        # the fused BL6 backward needs seg 1 and U <= 112: 16 kHz keeps it, 24 kHz and up take the generic chain
        ROUTES[f"bl6_u{_U}_s1l{_lpc}"] = (_u(C.bl6_laplace(1, _lpc), _U), BL6, 1, _U <= 112)
for _U in (80, 110, 120, 240):
    for _seg in (1, 2, 10):
        for _lpc in (0, 4):
            ROUTES[f"ref6_u{_U}_s{_seg}l{_lpc}"] = (_u(C.ref6_laplace(_seg, _lpc), _U), REF6, 1, False)


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_routing_table(name):
    cfg, dec, bf16_fwd, fused_bwd = ROUTES[name]
    lib = _lib.lib()
    d = ctypes.byref(_lib.desc_from_cfg(cfg))
    for batch in (1, 27):
        got = tuple(lib.swn_decode_resolve_variant(d, batch, v) for v in (0, 2, 3, 6))
        assert got == dec, (name, batch, got)
    assert lib.swn_decode_resolve_variant(d, 1, 1) == 1
    assert lib.swn_bf16_train_forward_supported(d) == bf16_fwd, name
    assert (lib.swn_backward_bf16_work_floats(d, 2, 9) > 0) == fused_bwd, name


def test_generic_decode_template_widths():
    """the generic kernel's seg template (generic_segt: <1>, <2>, <5>, <10>) sizes its LDS: seg 3 / 4 run <5> with a runtime seg
    below the template width, seg 6-10 run <10>; every one of them resolves (fits the 160 KiB LDS) at the BL6 and REF6 sizes."""
    lib = _lib.lib()
    for seg in range(1, 11):
        for cfg in (C.bl6_laplace(seg, 4), C.ref6_laplace(seg, 4), C.tiny("laplace", seg, 0)):
            assert lib.swn_decode_resolve_variant(ctypes.byref(_lib.desc_from_cfg(cfg)), 2, 1) == 1, (cfg, seg)


# ---- BL6 decode across rates ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lpc", [0, 4])
@pytest.mark.parametrize("U", [80, 120, 220, 240])
def test_bl6_decode_across_rates_matches_the_oracle(gpu_ok, U, lpc):
    """three ragged utterances (4, 3, 2 frames: the shorter ones zero-padded like pad_list) over several frame boundaries, host
    noise; every kernel the library has for the net against cpu_ref.laplace_generate: samples and heads <= 1e-5."""
    from shallow_wavenet_amd.runtime import HipNet
    cfg = _u(C.bl6_laplace(1, lpc), U)
    sd = synth_state_dict(cfg, seed=U + lpc, flavor="trained")
    net, P = HipNet.from_state_dict(cfg, sd, DEV), cpu_ref.as_params(sd)
    frames = [4, 3, 2]
    aux = synth_aux(cfg, len(frames), max(frames), seed=U)
    for b, f in enumerate(frames):
        aux[b, :, f:] = 0.0
    n_samples = [f * U for f in frames]
    n_steps = max(n_samples)
    noise = cpu_ref.laplace_noise(cfg, n_steps, len(frames), generator=torch.Generator().manual_seed(U * 10 + lpc))
    ref, ref_heads = cpu_ref.laplace_generate(cfg, P, torch.from_numpy(aux), n_samples, noise, return_heads=True)
    ref_heads = np.transpose(ref_heads, (1, 0, 2))
    dev_noise = torch.from_numpy(noise).permute(1, 0, 2).contiguous()
    for variant in (2, 6, 1, 3):
        out, heads = net.decode(torch.from_numpy(aux), n_steps, dev_noise, want_heads=True, variant=variant)
        out, heads = out.cpu().numpy(), heads.cpu().numpy()
        assert heads.shape == ref_heads.shape
        assert np.abs(heads - ref_heads).max() <= 1e-5, (U, lpc, variant)
        for b, n in enumerate(n_samples):
            assert np.abs(out[b, :n] - ref[b]).max() <= 1e-5, (U, lpc, variant, b)
        assert float(np.abs(ref[0]).max()) > 1e-3                # a live signal


# ---- REF6 seg 10: streamed and pooled forms of the stepped chain's generic Laplace tail ------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [2, 27])
def test_ref6_seg10_stream_partitions_equal_one_shot(gpu_ok, B):
    from test_gpu_decode_stream import _check_partitions
    _check_partitions(C.ref6_laplace(10, 4), B, 0, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("n_sess", [5, 27])
def test_ref6_seg10_pool_sessions_equal_solo_decodes(gpu_ok, n_sess):
    """5 sessions: the per-entry kernels; 27: the tile kernels while 24 or more are active (test_gpu_decode_pool_stepped)."""
    from shallow_wavenet_amd.streaming import SteppedDecodePool
    from test_gpu_decode_pool_stepped import RNG_SEED, _check, _drive, _net, _Run, _seed_of
    cfg = C.ref6_laplace(10, 4)
    net = _net(cfg)
    rng = np.random.default_rng(100 + n_sess)
    runs = [_Run(cfg, int(rng.integers(2, 7)), _seed_of(cfg, rng), int(rng.integers(0, 100000)),
                 0 if n_sess > 8 and i < 26 else int(rng.integers(0, 4)), aux_seed=300 + i) for i in range(n_sess)]
    pool = SteppedDecodePool(net, 32, rng_seed=RNG_SEED, want_heads=True, want_noise=True)
    _drive(pool, runs, rng)
    for r in runs:
        assert r.s.steps_done == r.F * cfg.U // cfg.seg
        _check(net, r)


@pytest.mark.gpu
def test_ref6_seg10_pooled_run_replays_in_the_cpu_oracle(gpu_ok):
    from shallow_wavenet_amd.runtime import HipNet
    from shallow_wavenet_amd.streaming import SteppedDecodePool
    cfg = C.ref6_laplace(10, 4)
    sd = synth_state_dict(cfg, seed=5, flavor="trained")
    net, P = HipNet.from_state_dict(cfg, sd, DEV), cpu_ref.as_params(sd)
    F = 3                                                                   # 330 samples, 33 steps
    aux = torch.from_numpy(synth_aux(cfg, 1, F, seed=2))
    pool = SteppedDecodePool(net, 2, rng_seed=99, want_noise=True)
    other = pool.open(utt_id=3)
    other.finish(torch.from_numpy(synth_aux(cfg, 1, 2, seed=8)).to(DEV))
    s = pool.open()
    outs, used = [], []
    s.push(aux[:, :, :1].to(DEV))
    s.finish(aux[:, :, 1:].to(DEV))
    while not s.done:
        res = pool.step(7, max_prologue=300)
        if s in res:
            outs.append(res[s][0]), used.append(res[s][2])
    out = torch.cat(outs, 1).cpu().numpy()[0]
    noise = torch.cat(used, 1).permute(1, 0, 2).contiguous().cpu().numpy()
    ref = cpu_ref.laplace_generate(cfg, P, aux, [F * cfg.U], noise)[0]
    assert out.shape[0] == F * cfg.U
    assert float(np.abs(out - ref).max()) <= 1e-5
    assert float(np.abs(ref).max()) > 1e-3


# ---- bf16 forward against the fp32 kernels -------------------------------------------------------------------------------------
def _gate8_tile(batch, Tp, ncu):
    """the position-tile width launch_gate8 (csrc/swn_stack_bf16g.hip) takes: fewer rounds of tiles over the CUs wins, ties to 192"""
    rounds_cost = lambda bn: -(-(batch * -(-Tp // bn)) // ncu) * bn
    return 192 if rounds_cost(192) <= rounds_cost(128) else 128


def _bf16_against_fp32(cfg, B, Tf, seed):
    from shallow_wavenet_amd.runtime import HipNet
    net = HipNet.from_state_dict(cfg, synth_state_dict(cfg, seed=seed, flavor="trained"), DEV)
    aux = torch.from_numpy(synth_aux(cfg, B, Tf, seed=seed))
    audio = torch.rand(B, 1, Tf * cfg.U - cfg.seg, generator=torch.Generator().manual_seed(seed)) * 1.6 - 0.8
    r32, _ = net.forward(aux, audio)
    r16 = net.forward_bf16(aux, audio)
    assert r16.shape == r32.shape == (B, cfg.n_out, Tf * cfg.U - 2 * cfg.seg + 1)
    assert torch.isfinite(r16).all()
    d = (r32 - r16).abs()
    scale = max(1.0, float(r32.abs().max()))
    assert float(d.max()) <= 3e-3 * scale, (cfg, B, Tf, float(d.max()))
    assert float(d.mean()) <= 3e-4 * scale, (cfg, B, Tf, float(d.mean()))
    assert float(d.max()) > 0, "the bf16 stack did not engage"


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [128, 192])
@pytest.mark.parametrize("lpc", [0, 4])
@pytest.mark.parametrize("seg", [1, 2, 10])
@pytest.mark.parametrize("U", [80, 120, 240])
def test_ref6_bf16_gemm_stack_across_rates_and_segs(gpu_ok, U, seg, lpc, tile):
    """the GEMM stack of the run.sh geometry: frame stepping of the gated layer at other U (gate_frames), seg conditioning taps
    per position (gate_group: ten at seg 10), and both position-tile widths of the LDS-DMA gated layer - two utterances of
    ~1 000 positions take the 128-position tiles, eight of 4 097 .. 6 144 positions the 192-position ones."""
    cfg = _u(C.ref6_laplace(seg, lpc), U)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 if tile == 128 else 8
    Tp = lambda Tf: Tf * U - 2 * seg + 1
    if tile == 128:
        Tf = -(-1000 // U)
    else:
        Tf = next(f for f in range(1, 400) if Tp(f) > 4096 and _gate8_tile(B, Tp(f), ncu) == 192)
    assert _gate8_tile(B, Tp(Tf), ncu) == tile
    _bf16_against_fp32(cfg, B, Tf, seed=U + seg + lpc)


@pytest.mark.gpu
@pytest.mark.parametrize("lpc", [0, 4])
@pytest.mark.parametrize("U", [120, 240])
def test_bl6_bf16_stack_above_seven_chunks_per_frame(gpu_ok, U, lpc):
    """BL6 class, seg 1, U > 112: more than 7 sixteen-position chunks per frame leave the fused and frame-unit kernels for
    bf16_layer_kernel<0>; three utterances, a length that is no multiple of 16."""
    _bf16_against_fp32(_u(C.bl6_laplace(1, lpc), U), 3, 7, seed=U + lpc)


@pytest.mark.gpu
def test_bl6_bf16_stack_at_seg10(gpu_ok):
    """BL6 at seg 10 / lpc 4: NO = 24 > 16 takes it off the BL6 bf16 kernels onto the GEMM stack at H = 64, K = 2."""
    _bf16_against_fp32(C.bl6_laplace(10, 4), 2, 9, seed=7)
