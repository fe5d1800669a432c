"""GPU: decode, front end, forward and backward at network geometries OFF the tiny / bl6 / ref6 grid (fixtures g10_odd_*,
recorded from the reference): H, S, out_1 width and A0 that are not multiples of 4 (the Hp / Sp / O1p / A0p pad lanes), an
odd head width, seg 3 / 4 / 7 on the 5- and 10-segment templates of the generic kernel, aux kernels 1 / 3 / 5 with 1..3
layers, class counts off 64, and BL6-shaped nets that no BL6 kernel serves.

  * free-running decode of every variant the library resolves against the reference (samples, heads <= 1e-5; softmax
    indices exact, logits <= 2e-5), with the kernel that serves each net pinned (tests/test_offgrid_dispatch_host.py);
  * teacher-forced decode heads, front end, hidden states and raw head against the float64 oracle.  Bound per case =
    max(the project's tolerance, 4 x the fp32 oracle's own distance to float64 in that case), printed;
  * gradients through the drop-in modules against the reference's, with the rule of test_gpu_backward_parity;
  * the net with H % 4 != 0 is refused by forward and backward before anything is launched;
  * streams in chunks that are no multiple of a frame and 3-session pools are bit-identical to the one-shot decode."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_names, load_golden
from oracle import cpu_ref
from shallow_wavenet_amd import _lib
from shallow_wavenet_amd.nets import cswnv_shift1 as mc
from shallow_wavenet_amd.nets import dswnv as md
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream, SteppedDecodePool
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict
from test_offgrid_dispatch_host import SERVED, UNSUPPORTED, resolve

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G10 = golden_names("g10_odd_")
REFUSED = "g10_odd_laplace_h30_s50_seg3"                     # H % 4 != 0: decode only
TRAINABLE = [n for n in G10 if n != REFUSED]
WITH_GRADS = [n for n in G10 if "loss" in load_golden(n)[1]]
TOL_FREE, TOL_LOGIT = 1e-5, 2e-5
TOL_TF, TOL_TF_B = 2e-6, 1e-6                                # teacher-forced mu / a, sigmoid(scale)
TOL_HID, TOL_RAW = 5e-6, 1e-5

_cache = {}


def _case(name):
    """fixture, weights, fp32 / float64 oracle parameters and the net on the device - made once per fixture"""
    if name not in _cache:
        cfg, d = load_golden(name)
        sd = synth_state_dict(cfg, seed=int(d["wseed"]), flavor=str(d["flavor"]))
        _cache[name] = (cfg, d, sd, cpu_ref.as_params(sd), cpu_ref.as_params(sd, torch.float64),
                        HipNet.from_state_dict(cfg, sd, DEV))
    return _cache[name]


def _seg(cfg):
    return 1 if cfg.kind == "softmax" else cfg.seg


def _variants(cfg, batch):
    """(variant, kernel) for 1, 3 and 0 wherever the library resolves them; variant 1 must exist for every net"""
    out = [(v, resolve(cfg, v, batch)) for v in (1, 3, 0)]
    assert out[0][1] == 1
    return [(v, k) for v, k in out if k >= 0]


def _noise(cfg, d):
    """(B, n_steps, width) host noise of the fixture"""
    if cfg.kind == "laplace":
        nz = d["noise"]
    else:
        g = torch.Generator().manual_seed(int(d["noise_seed"]))
        nz = cpu_ref.softmax_noise(cfg, d["heads"].shape[0], d["aux"].shape[0], generator=g)
    return torch.from_numpy(nz).permute(1, 0, 2).contiguous()


def _bound(tol, e32, what, name):
    b = max(tol, 4.0 * e32)
    print(f"[offgrid] {name} {what}: fp32 oracle vs float64 {e32:.2e} -> bound {b:.2e}")
    return b


def _report(name, what, err, bound):
    print(f"[offgrid] {name} {what}: error {err:.2e} (bound {bound:.2e})")
    assert err <= bound, (name, what, err, bound)


# ------------------------------------------------------------------------------------------------ free-running decode
@pytest.mark.parametrize("name", G10)
def test_free_running_decode_matches_the_reference(gpu_ok, name):
    cfg, d, sd, P32, P64, net = _case(name)
    B, n_steps, seg = d["aux"].shape[0], d["heads"].shape[0], _seg(cfg)
    assert tuple(resolve(cfg, v, B) for v in (0, 1, 2, 3, 6)) == SERVED[name]
    if "nearbl6" in name:
        assert resolve(cfg, 2, B) == UNSUPPORTED and resolve(cfg, 6, B) == UNSUPPORTED
        assert resolve(cfg, 0, B) == 1
    noise = _noise(cfg, d)
    ref_heads = np.transpose(d["heads"], (1, 0, 2))
    variants = _variants(cfg, B)
    assert [k for _, k in variants] == [1, 3, 1]
    for variant, kernel in variants:
        out, heads = net.decode(torch.from_numpy(d["aux"]), n_steps, noise, want_heads=True, variant=variant)
        out, heads = out.cpu().numpy(), heads.cpu().numpy()
        _report(name, f"free heads v{variant}", float(np.abs(heads - ref_heads).max()),
                TOL_FREE if cfg.kind == "laplace" else TOL_LOGIT)
        for b, n in enumerate(d["n_samples"]):
            ref = d[f"samples_{b}"]
            assert ref.shape == (int(n),)
            if cfg.kind == "laplace":
                _report(name, f"free samples v{variant} utt {b}", float(np.abs(out[b, :n] - ref).max()), TOL_FREE)
            else:
                assert np.array_equal(out[b, :n], ref), (name, variant, b)


# ------------------------------------------------------------------------------------------------ teacher-forced decode
def _tf_heads(cfg, P, aux, forced, n_steps):
    """raw head rows (B, n_steps, n_out) of the decode fed `forced`, from the oracle's teacher-forced stack in the dtype
    of P: replicate-padded conditioning, rf + 1 zero (class Q//2) seed positions, step i read at column rf + i * seg -
    the construction of test_full_size_decode_is_self_consistent_with_the_oracle for any seg and for the softmax net."""
    dt = P["causal.conv.weight"].dtype
    seg, rf, B = _seg(cfg), cfg.receptive_field, aux.shape[0]
    n_pos = rf + 1 + (n_steps - 1) * seg
    with torch.no_grad():
        x = F.pad(cpu_ref.upsample(cfg, P, cpu_ref.frontend(cfg, P, aux.to(dt))), (rf, 0), "replicate")
        if cfg.kind == "laplace":
            x = cpu_ref._stack_seg(cfg, P, x)[:, :, :n_pos]
            audio = torch.cat((torch.zeros(B, 1, rf + seg, dtype=dt), forced[:, None, :(n_steps - 1) * seg].to(dt)), 2)
            h = F.softsign(cpu_ref.causal_conv(cpu_ref._lift(cfg, P, audio), P["causal.conv.weight"],
                                               P["causal.conv.bias"], 1)[:, :, seg - 1:])
        else:
            Q = cfg.n_quantize
            idx = torch.cat((torch.full((B, rf + 1), Q // 2, dtype=torch.int64), forced[:, :n_steps - 1].long()), 1)
            oh = cpu_ref.one_hot(idx, Q, dtype=dt).transpose(1, 2)
            x = x[:, :, :n_pos]
            if cfg.audio_in_flag:
                x = torch.cat((x, oh), 1)
            h = F.softsign(cpu_ref.causal_conv(cpu_ref._lift(cfg, P, oh), P["causal.conv.weight"], P["causal.conv.bias"], 1))
        assert x.shape[2] == n_pos and h.shape[2] == n_pos
        tot = None
        for l in range(cfg.L):
            sk, h = cpu_ref.gated_layer(cfg, P, l, x, h)
            tot = sk if tot is None else tot + sk
        raw = cpu_ref.head(cfg, P, tot)
    return raw[:, :, rf::seg].transpose(1, 2).double().numpy()


def _forced(cfg, d, P32):
    """the fixture's samples as the forced input, (B, n_steps * seg); an utterance shorter than the decode continues with
    the fp32 oracle's samples (the reference cuts it at its own length)"""
    B, n_steps, seg = d["aux"].shape[0], d["heads"].shape[0], _seg(cfg)
    aux = torch.from_numpy(d["aux"])
    if cfg.kind == "laplace":
        full = np.stack(cpu_ref.laplace_generate(cfg, P32, aux, [n_steps * seg] * B, d["noise"]))
    else:
        full = np.stack(cpu_ref.softmax_generate(cfg, P32, aux, [n_steps] * B, _noise(cfg, d).permute(1, 0, 2).numpy()))
    for b, n in enumerate(d["n_samples"]):
        full[b, :n] = d[f"samples_{b}"]
    return torch.from_numpy(full.astype(np.float32 if cfg.kind == "laplace" else np.int32))


@pytest.mark.parametrize("name", G10)
def test_teacher_forced_decode_heads_match_float64(gpu_ok, name):
    cfg, d, sd, P32, P64, net = _case(name)
    B, n_steps, seg = d["aux"].shape[0], d["heads"].shape[0], _seg(cfg)
    aux = torch.from_numpy(d["aux"])
    forced = _forced(cfg, d, P32)
    ref = _tf_heads(cfg, P64, aux, forced, n_steps)
    o32 = _tf_heads(cfg, P32, aux, forced, n_steps)
    # the construction itself: fed the reference's own samples it gives the reference's recorded heads
    assert np.abs(o32 - np.transpose(d["heads"], (1, 0, 2))).max() <= (TOL_FREE if cfg.kind == "laplace" else TOL_LOGIT)
    sig = lambda y: 1.0 / (1.0 + np.exp(-y.astype(np.float64)))
    if cfg.kind == "laplace":
        parts = [("mu", lambda y: y[..., :seg], TOL_TF), ("b", lambda y: sig(y[..., seg:2 * seg]), TOL_TF_B)]
        if cfg.lpc > 0:
            parts.append(("a", lambda y: y[..., 2 * seg:], TOL_TF))
    else:
        parts = [("logits", lambda y: y, TOL_LOGIT)]
    bounds = {w: _bound(tol, float(np.abs(f(o32) - f(ref)).max()), f"teacher-forced {w}", name) for w, f, tol in parts}
    noise = _noise(cfg, d)
    for variant, kernel in _variants(cfg, B):
        out, heads = net.decode(aux, n_steps, noise, forced=forced, want_heads=True, variant=variant)
        got = heads.cpu().double().numpy()
        for w, f, _ in parts:
            _report(name, f"teacher-forced {w} v{variant}", float(np.abs(f(got) - f(ref)).max()), bounds[w])


# ------------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("name", G10)
def test_frontend_matches_float64(gpu_ok, name):
    cfg, d, sd, P32, P64, net = _case(name)
    aux = torch.from_numpy(d["aux"])
    cond = net.frontend(aux).cpu().double()
    c = cpu_ref.frontend(cfg, P64, aux.double())                          # B, A0, Tf
    seg = _seg(cfg)
    conv2d = cfg.kind == "laplace" and cfg.aux_conv2d_flag and cfg.seg > 1
    ref = []
    for l in range(cfg.L):
        w = P64[f"in_x.{l}.weight"][:, :, 0]
        if conv2d:      # in_x after the (seg,1) Conv2d: W_eff[o][c][s] = sum_p in_x.W[o][p] * conv2d.W[p][c][s]
            w = torch.einsum("op,pcs->ocs", w, P64["aux_conv2d.weight"][:, :, :, 0])
        else:
            w = w[:, : cfg.A0 * seg].reshape(2 * cfg.H, cfg.A0, seg)
        ref.append(torch.einsum("ocs,bcf->bfso", w, c))                    # B,Tf,seg,2H
    ref = torch.stack(ref, 2).reshape(cond.shape)                          # B,Tf,L,seg,2H
    assert cond.shape[2] == cfg.L * seg * 2 * cfg.H
    scale = ref.abs().max().item()
    _report(name, "front end", (cond - ref).abs().max().item(), 2e-6 * max(1.0, scale))


# ------------------------------------------------------------------------------------------------ forward / backward
def _stack(cfg, P, d):
    aux = torch.from_numpy(d["aux"]).to(P["causal.conv.weight"].dtype)
    with torch.no_grad():
        if cfg.kind == "laplace":
            return cpu_ref.laplace_stack(cfg, P, aux, torch.from_numpy(d["fwd_audio"]).to(aux.dtype))
        return cpu_ref.softmax_stack(cfg, P, torch.from_numpy(d["fwd_audio_idx"]), aux)


@pytest.mark.parametrize("name", TRAINABLE)
def test_forward_hidden_states_and_raw_head_match_float64(gpu_ok, name):
    cfg, d, sd, P32, P64, net = _case(name)
    assert cfg.H % 4 == 0
    audio = torch.from_numpy(d["fwd_audio"] if cfg.kind == "laplace" else d["fwd_audio_idx"])
    raw, hs = net.forward(torch.from_numpy(d["aux"]), audio, want_hidden=True)
    raw, hs = raw.cpu().double().numpy(), hs.cpu().double().numpy()
    ref_raw, ref_hs = _stack(cfg, P64, d)
    o_raw, o_hs = _stack(cfg, P32, d)
    assert hs.shape[1] == cfg.L + 1 and raw.shape == tuple(ref_raw.shape)
    e_hid = max(float((a.double() - b).abs().max()) for a, b in zip(o_hs, ref_hs))
    b_hid = _bound(TOL_HID, e_hid, "hidden states", name)
    b_raw = _bound(TOL_RAW, float((o_raw.double() - ref_raw).abs().max()), "raw head", name)
    _report(name, "hidden states", max(float(np.abs(hs[:, l] - h.numpy()).max()) for l, h in enumerate(ref_hs)), b_hid)
    _report(name, "raw head", float(np.abs(raw - ref_raw.numpy()).max()), b_raw)


def _check_grads(name, model, d):
    """the rule of test_gpu_backward_parity._check"""
    worst = 0.0
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        g = p.grad.detach().cpu().numpy().astype(np.float64)
        dig = d[f"gdig_{k}"]
        scale = max(1e-3, dig[1])
        assert abs(g.sum() - dig[0]) <= 5e-4 * scale, (name, k, g.sum(), dig[0])
        assert abs(np.abs(g).sum() - dig[1]) <= 5e-4 * scale, (name, k)
        if f"grad_{k}" in d:
            ref = d[f"grad_{k}"]
            err, bound = np.abs(g - ref).max(), 2e-5 + 2e-4 * np.abs(ref).max()
            worst = max(worst, err / bound)
            assert err <= bound, (name, k, err, bound)
    print(f"[offgrid] {name} gradients: worst stored tensor at {worst:.2f} of its bound")


@pytest.mark.parametrize("name", WITH_GRADS)
def test_gradients_match_the_reference(gpu_ok, name):
    cfg, d, sd, *_ = _case(name)
    m = (mc.CSWNV if cfg.kind == "laplace" else md.DSWNV)(**cfg.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.cuda().train()
    aux, tgt = torch.from_numpy(d["aux"]).cuda(), torch.from_numpy(d["loss_target"]).cuda()
    if cfg.kind == "laplace":
        res = m(aux, torch.from_numpy(d["fwd_audio"]).cuda(), do=False, clip=False)
        loss = mc.LaplaceLoss()(res[0], res[1], tgt, log_b=res[2], log=False)
        if cfg.lpc > 0:
            loss = loss + 0.1 * res[3].pow(2).mean()
    else:
        idx = torch.from_numpy(d["fwd_audio_idx"]).cuda()
        logits = m(md.OneHot(idx, cfg.n_quantize).transpose(1, 2), aux)
        loss = torch.nn.CrossEntropyLoss()(logits.reshape(-1, cfg.n_quantize), tgt.reshape(-1))
    _report(name, "loss", abs(loss.item() - float(d["loss"])), 1e-5 * max(1.0, abs(float(d["loss"]))))
    loss.backward()
    _check_grads(name, m, d)


# ------------------------------------------------------------------------------------------------ refusal
def test_net_with_h_not_a_multiple_of_4_is_refused_before_any_launch(gpu_ok):
    cfg, d, sd, P32, P64, net = _case(REFUSED)
    assert cfg.H % 4 != 0
    aux, audio = torch.from_numpy(d["aux"]).to(DEV), torch.from_numpy(d["fwd_audio"]).to(DEV)
    with pytest.raises(RuntimeError, match="not supported"):
        net.forward(aux, audio)
    m = mc.CSWNV(**cfg.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.cuda().train()
    with pytest.raises(RuntimeError, match="not supported"):
        m(aux, audio, do=False, clip=False)

    # the C calls on buffers full of a sentinel: nothing is written, and the error text says that nothing was launched
    L, desc = _lib.lib(), ctypes.byref(net.desc)
    B, Tf = aux.shape[0], aux.shape[2]
    Tp = Tf * cfg.U - 2 * cfg.seg + 1
    cond = net.frontend(aux)
    fe_work = net._last_frontend_work
    SENT = 12345.5
    full = lambda n: torch.full((int(n),), SENT, dtype=torch.float32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    work, out, hs = full(L.swn_forward_work_floats(desc, B, Tf)), full(B * cfg.n_out * Tp), full(B * (cfg.L + 1) * cfg.H * Tp)
    assert work.numel() > 0
    # backward first, so that the text the forward call leaves replaces another call's and is its own
    bwork, gp = full(max(1, L.swn_backward_work_floats(desc, B, Tf))), full(net.packed.numel())
    grad = torch.ones(B * cfg.n_out * Tp, dtype=torch.float32, device=DEV)
    rc = L.swn_backward(desc, p(net.packed), p(aux), p(cond), p(fe_work), p(audio), p(work), None, p(grad), B, Tf,
                        p(bwork), p(gp), _lib.PRECISION_FP32, st)
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED
    detail = L.swn_last_error_detail().decode()
    assert detail.startswith("swn_backward") and "nothing was launched" in detail, detail
    assert bool((gp == SENT).all()) and bool((bwork == SENT).all())

    rc = L.swn_forward(desc, p(net.packed), p(cond), p(audio), B, Tf, p(work), p(out), p(hs), st)
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED
    detail = L.swn_last_error_detail().decode()
    assert detail.startswith("swn_forward:") and "nothing was launched" in detail, detail
    for t in (work, out, hs):
        assert bool((t == SENT).all())

    # the dropout-mode forward shares the check
    drop_x = torch.ones(B, cfg.A0, Tf * cfg.U - cfg.seg, device=DEV)
    with pytest.raises(RuntimeError, match="not supported"):
        net.forward_train(aux, audio, drop=(drop_x, [None] * cfg.L))
    assert "swn_forward_drop" in L.swn_last_error_detail().decode()


# ------------------------------------------------------------------------------------------------ streams and pools
STREAMED = ["g10_odd_laplace_h30_s50_seg3", "g10_odd_smx_q90_h28_audioin"]


@pytest.mark.parametrize("name", STREAMED)
def test_stream_in_chunks_off_the_frame_grid_equals_one_shot(gpu_ok, name):
    cfg, d, sd, P32, P64, net = _case(name)
    B, seg, F_ = 2, _seg(cfg), 6
    aux = torch.from_numpy(synth_aux(cfg, B, F_, seed=3)).to(DEV)
    N = F_ * cfg.U // seg
    for variant, kernel in _variants(cfg, B):
        ref_out, ref_heads, ref_used = net.decode(aux, N, want_heads=True, variant=variant, rng_seed=77, want_noise=True)
        s = DecodeStream(net, B, variant=variant, rng_seed=77, want_heads=True, want_noise=True)
        assert s.resolved_variant == kernel
        s.push(aux, generate=False)
        s.finish(generate=False)
        parts, left, k = [], N, 0
        while left > 0:                                       # 0, 1, 3, 5, 7 ... steps: never a whole frame
            n = min(left, [0, 1, 3, 5, 7, 2][k % 6])
            assert n == 0 or (n * seg) % cfg.U != 0
            parts.append(s.advance(n))
            left, k = left - n, k + 1
        assert s.steps_done == N and len(parts) > 4
        assert torch.equal(torch.cat([q[0] for q in parts], 1), ref_out), (name, variant)
        assert torch.equal(torch.cat([q[1] for q in parts], 1), ref_heads), (name, variant)
        assert torch.equal(torch.cat([q[2] for q in parts], 1), ref_used), (name, variant)


@pytest.mark.parametrize("name", STREAMED)
def test_three_session_pool_equals_solo_decodes(gpu_ok, name):
    cfg, d, sd, P32, P64, net = _case(name)
    m = (mc.CSWNV if cfg.kind == "laplace" else md.DSWNV)(**cfg.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.cuda().eval()
    m.noise_rng_seed = 4242
    pool = m.open_pool(3)
    # every one of these nets resolves variant 0 to the generic kernel, which serves pools itself
    assert isinstance(pool, DecodePool) and not isinstance(pool, SteppedDecodePool) and pool.resolved_variant == 1
    pool.want_heads = pool.want_noise = True
    seg = _seg(cfg)
    frames, ids = [5, 3, 4], [41, 7, 1000]
    auxs = [torch.from_numpy(synth_aux(cfg, 1, f, seed=100 + i)).to(DEV) for i, f in enumerate(frames)]
    sess = [pool.open(utt_id=u) for u in ids]
    got = {s: [] for s in sess}
    pushed = [0, 0, 0]
    for tick in range(200):
        for i, s in enumerate(sess):
            if not s.finished:                                 # one, two, one ... frames per tick, then finish
                piece = auxs[i][:, :, pushed[i]:pushed[i] + 1 + (tick + i) % 2]
                pushed[i] += piece.shape[2]
                (s.finish if pushed[i] >= frames[i] else s.push)(piece)
        for s, r in pool.step(4 + tick % 3).items():           # 4..6 steps per tick: never a whole frame
            got[s].append(r)
        if all(s.done for s in sess):
            break
    engine = m._engine()
    for i, s in enumerate(sess):
        n = frames[i] * cfg.U // seg
        assert s.steps_done == n
        ref = engine.decode(auxs[i], n, want_heads=True, variant=pool.variant, rng_seed=4242, want_noise=True, utt_ids=[ids[i]])
        for j in range(3):
            assert torch.equal(torch.cat([r[j] for r in got[s]], 1), ref[j]), (name, i, j)
