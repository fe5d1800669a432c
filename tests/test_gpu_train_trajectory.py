"""GPU: several full training steps through the drop-in modules against the same steps of the float64 CPU oracle.

The one-step tests (test_gpu_backward_parity.py, test_gpu_fused_backward.py, ...) cannot see whether step N+1 runs on the
weights step N wrote.  The kernels never read the Parameters: they read a packed copy that the module refreshes when a
parameter's (data_ptr, _version) changes (nets/_engine.py).  Here K steps (forward, loss, backward, optimizer step) run on
one fixed batch per geometry, without dropout, with scale_in frozen on both sides; the oracle is cpu_ref's forward on
float64 leaves with torch autograd and the same torch optimizer.  Geometries, one per class of derived state: tiny Laplace
with LP (generic chain), BL6 Laplace (fused bf16 backward, bf16 weight image), REF6 Laplace with LP (GEMM stack, kept
pre-activations), tiny and BL6 softmax.

Measured margins on an MI355X (worst error / tolerance over the five geometries):
  SGD, fp32 mode      0.07-0.47 (REF6 the largest); the loss moves 234x (BL6 softmax) to 10 000x its tolerance
  make_adam, fp32     losses <= 0.23, displacement norms <= 0.52 (both REF6: 2.6 % of the displacement norm)
  make_adam, bf16     losses <= 0.14, displacement norms <= 0.55 (BL6: 28 % of the norm, sign flips of small gradients)
  stale engine        (HipNet.repack a no-op) misses the SGD comparison by 364x (tiny softmax) to 11 600x.
Before make_adam bumped the version counters, every make_adam case failed its first coherence check ("the packed
parameters are stale" after step 1)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd import ops as _O
from shallow_wavenet_amd import train_driver as T
from shallow_wavenet_amd import train_softmax_driver as S
from shallow_wavenet_amd.nets import cswnv_shift1 as mc
from shallow_wavenet_amd.nets import dswnv as md
from shallow_wavenet_amd.runtime import HipNet, pack_parameters_device, train_precision
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

K = 4                    # optimizer steps per run
ADAM_LR = 1e-3
# name: (config, batch, frames, SGD learning rate: the loss falls 2-10 % in K steps, smoothly; 2.3x that lr makes the
#        Laplace runs oscillate)
GEOMS = {
    "tiny_lap_lp": (C.tiny("laplace", 1, 4), 2, 8, 1e-3),
    "bl6_lap": (C.bl6_laplace(1, 0), 2, 12, 1e-3),
    "ref6_lap_lp": (C.ref6_laplace(1, 4), 2, 8, 3e-4),
    "tiny_softmax": (C.tiny("softmax"), 2, 8, 0.5),
    "bl6_softmax": (C.bl6_softmax(), 2, 12, 2.0),
}
LOSS_TOL = 1e-5          # relative, as test_gpu_backward_parity.py
DISP_TOL = 2e-3          # SGD: per tensor, of that tensor's max |displacement| (+ 2e-5 of the largest over all tensors)
ADAM_TOL = {"fp32": 0.05, "bf16": 0.5}   # make_adam: per tensor, of that tensor's displacement norm


def _module(cfg):
    return (mc.CSWNV if cfg.kind == "laplace" else md.DSWNV)(**cfg.ctor_kwargs())


def _driver(cfg):
    return T if cfg.kind == "laplace" else S


@functools.lru_cache(maxsize=None)
def _trainable(geom):
    """state_dict names of what the driver's optimizer_parameters hands the optimizer (everything but scale_in)."""
    m = _module(GEOMS[geom][0])
    ids = {id(p) for p in _driver(GEOMS[geom][0]).optimizer_parameters(m)}
    return tuple(k for k, p in m.named_parameters() if id(p) in ids)


@functools.lru_cache(maxsize=None)
def _data(geom):
    """(state dict, aux, network input, target) on the CPU: one fixed batch per geometry."""
    cfg, B, Tf, _ = GEOMS[geom]
    sd = synth_state_dict(cfg, seed=3, flavor="trained", identity_scale_in=True)
    aux = torch.from_numpy(synth_aux(cfg, B, Tf))
    g = torch.Generator().manual_seed(11)
    T_ = Tf * cfg.U
    if cfg.kind == "laplace":
        Tp = T_ - 2 * cfg.seg + 1
        x = torch.rand(B, 1, T_ - cfg.seg, generator=g) * 0.6 - 0.3
        tgt = torch.rand(B, Tp, generator=g) * 0.6 - 0.3
    else:
        x = torch.randint(0, cfg.n_quantize, (B, T_ - 1), generator=g)
        tgt = torch.randint(0, cfg.n_quantize, (B, T_ - 1), generator=g)
    return sd, aux, x, tgt


def _loss(cfg, res, tgt):
    """the same loss on both sides: Laplace NLL (+ 0.1 mean a^2 with LP, so the LP rows get a gradient) | cross entropy."""
    if cfg.kind == "softmax":
        return F.cross_entropy(res.reshape(-1, cfg.n_quantize), tgt.reshape(-1))
    B = tgt.shape[0]
    loss = cpu_ref.laplace_nll(res[0].reshape(B, -1), res[1].reshape(B, -1), tgt, log_b=res[2].reshape(B, -1))
    return loss + 0.1 * res[3].pow(2).mean() if cfg.lpc > 0 else loss


def _make_opt(kind, params, lr):
    if kind == "sgd":
        return torch.optim.SGD(params, lr=lr)
    if kind == "make_adam":
        return T.make_adam(params, lr)
    return torch.optim.Adam(params, lr=lr)        # "adam": the default (foreach) form


@functools.lru_cache(maxsize=None)
def _oracle(geom, kind):
    """float64 CPU run: (losses at theta_0..theta_K, {name: theta_0}, {name: theta_K}) as float64 numpy."""
    cfg, _, _, sgd_lr = GEOMS[geom]
    sd, aux, x, tgt = _data(geom)
    train = set(_trainable(geom))
    P = {k: torch.from_numpy(v).double().requires_grad_(k in train) for k, v in sd.items()}
    opt = torch.optim.SGD([P[k] for k in _trainable(geom)], lr=sgd_lr) if kind == "sgd" else \
        torch.optim.Adam([P[k] for k in _trainable(geom)], lr=ADAM_LR)
    aux, tgt = aux.double(), (tgt.double() if cfg.kind == "laplace" else tgt)
    x = x.double() if cfg.kind == "laplace" else cpu_ref.one_hot(x, cfg.n_quantize).transpose(1, 2).double()

    def f():
        if cfg.kind == "laplace":
            return _loss(cfg, cpu_ref.laplace_forward(cfg, P, aux, x), tgt)
        return _loss(cfg, cpu_ref.softmax_forward(cfg, P, x, aux), tgt)
    losses = []
    for _ in range(K):
        loss = f()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(f()))
    return np.array(losses), {k: v.astype(np.float64) for k, v in sd.items()}, \
        {k: v.detach().numpy().copy() for k, v in P.items()}


def _assert_coherent(m, where):
    """the engine's packed buffer is what the live parameters pack to, bit for bit; so is the bf16 weight image where a
    bf16 forward has built one."""
    net = m._engine()
    fresh = pack_parameters_device(m._cfg, m._param_list())
    assert torch.equal(net.packed, fresh), f"{where}: the packed parameters are stale"
    if getattr(net, "_wbf16", None) is not None:
        assert net._wbf16_version == net.packed_version, f"{where}: the bf16 weight image lags the packed buffer"
        assert torch.equal(net._wbf16, _O.pack_bf16(fresh, net.dlist)), f"{where}: the bf16 weight image is stale"


def _gpu_run(geom, kind, precision="fp32", coherent=True):
    """K steps on the drop-in module; returns (losses at theta_0..theta_K, {name: theta_K}, module).  The forward that
    gives loss_K is a training-mode forward too (it builds the bf16 image of theta_K in bf16 mode); no backward follows."""
    cfg, _, _, sgd_lr = GEOMS[geom]
    sd, aux, x, tgt = _data(geom)
    m = _module(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.cuda().train()
    for p in m.scale_in.parameters():
        p.requires_grad = False
    opt = _make_opt(kind, _driver(cfg).optimizer_parameters(m), sgd_lr if kind == "sgd" else ADAM_LR)
    aux, x, tgt = aux.cuda(), x.cuda(), tgt.cuda()
    f = (lambda: _loss(cfg, m(aux, x), tgt)) if cfg.kind == "laplace" else (lambda: _loss(cfg, m(x, aux), tgt))
    losses = []
    with train_precision(precision):
        for i in range(K + 1):
            loss = f()
            losses.append(loss.item())
            if coherent:
                _assert_coherent(m, f"{geom} {kind} {precision} after step {i}")
            if i == K:
                break
            opt.zero_grad()
            loss.backward()
            opt.step()
    return np.array(losses), {k: v.detach().double().cpu().numpy() for k, v in m.state_dict().items()}, m


def _sgd_misses(geom, losses, theta):
    """worst error / tolerance of the SGD comparison (per-step losses, per-tensor displacements)."""
    ref_l, th0, thK = _oracle(geom, "sgd")
    worst = max(abs(a - b) / (LOSS_TOL * max(1.0, abs(b))) for a, b in zip(losses, ref_l))
    d_ref = {k: thK[k] - th0[k] for k in _trainable(geom)}
    big = max(np.abs(d).max() for d in d_ref.values())
    for k, d in d_ref.items():
        err = np.abs((theta[k] - th0[k]) - d).max()
        worst = max(worst, err / (DISP_TOL * np.abs(d).max() + 2e-5 * big))
    return worst


@pytest.mark.parametrize("geom", list(GEOMS))
def test_sgd_steps_match_the_oracle(gpu_ok, geom):
    """(a) + (c): SGD is linear in the gradient, so after K steps every parameter's displacement must match the oracle's
    element by element, and every step's loss must match; the packed buffer must follow every step."""
    ref_l, _, _ = _oracle(geom, "sgd")
    assert abs(ref_l[-1] - ref_l[0]) >= 100 * LOSS_TOL * max(1.0, abs(ref_l[0])), ref_l     # the loss really moves
    losses, theta, _ = _gpu_run(geom, "sgd")
    worst = _sgd_misses(geom, losses, theta)
    print(f"{geom}: sgd worst error/tol {worst:.3g}, loss move {abs(ref_l[-1] - ref_l[0]) / (LOSS_TOL * max(1.0, abs(ref_l[0]))):.0f}x tol")
    assert worst <= 1.0, (geom, worst, losses, ref_l)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_stale_engine_is_caught(gpu_ok, geom, monkeypatch):
    """(d) negative control: with HipNet.repack a no-op every step after the first runs on theta_0; the comparison of
    test_sgd_steps_match_the_oracle must miss by at least 10x, so a later change of lr or tolerance cannot disarm it."""
    monkeypatch.setattr(HipNet, "repack", lambda self, tensors: None)
    losses, theta, _ = _gpu_run(geom, "sgd", coherent=False)
    worst = _sgd_misses(geom, losses, theta)
    print(f"{geom}: stale engine misses by {worst:.3g}x")
    assert worst >= 10.0, (geom, worst)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_make_adam_steps_match_the_oracle(gpu_ok, geom, precision):
    """(b) + (c): the optimizer the drivers build (fused on a GPU) against float64 torch.optim.Adam.  Adam's first steps
    are about lr * sign(g), and gradients near zero may flip sign between fp32 and fp64, so each tensor's displacement
    is compared in norm; per-step losses as in test_gpu_backward_parity.py (fp32) and test_gpu_train_bf16.py (bf16)."""
    ref_l, th0, thK = _oracle(geom, "adam")
    losses, theta, _ = _gpu_run(geom, "make_adam", precision)
    worst_l, worst_d = 0.0, 0.0
    for a, b in zip(losses, ref_l):
        # fp32: the one-step tolerance plus 2e-3 of the distance travelled (the fp32 and fp64 trajectories part through
        # the sign flips); bf16: the loss-curve tolerance of test_gpu_train_bf16.py
        tol = LOSS_TOL * max(1.0, abs(b)) + 2e-3 * abs(ref_l[0] - b) if precision == "fp32" else \
            2e-2 * max(abs(b), 1e-3) + 2e-2 * abs(ref_l[0] - b)
        worst_l = max(worst_l, abs(a - b) / tol)
    for k in _trainable(geom):
        d_ref = thK[k] - th0[k]
        err = np.linalg.norm((theta[k] - th0[k]) - d_ref)
        worst_d = max(worst_d, err / (ADAM_TOL[precision] * np.linalg.norm(d_ref) + 1e-12))
    print(f"{geom} {precision}: make_adam worst loss error/tol {worst_l:.3g}, displacement error/tol {worst_d:.3g}")
    assert worst_l <= 1.0, (geom, precision, worst_l, losses, ref_l)
    assert worst_d <= 1.0, (geom, precision, worst_d)


@pytest.mark.parametrize("geom", ["tiny_lap_lp", "bl6_lap", "tiny_softmax"])
def test_every_way_parameters_change_reaches_the_engine(gpu_ok, geom):
    """(c) for the other writers: the default Adam, load_state_dict in the middle of training (--resume), replacing a
    Parameter (set_scale_in) and an in-place write under no_grad.  After each, the packed buffer (and, in bf16 mode, the
    bf16 weight image) must be what the live parameters pack to."""
    cfg = GEOMS[geom][0]
    sd, aux, x, tgt = _data(geom)
    m = _module(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.cuda().train()
    for p in m.scale_in.parameters():
        p.requires_grad = False
    drv = _driver(cfg)
    aux, x, tgt = aux.cuda(), x.cuda(), tgt.cuda()
    f = (lambda: _loss(cfg, m(aux, x), tgt)) if cfg.kind == "laplace" else (lambda: _loss(cfg, m(x, aux), tgt))
    precision = "bf16" if geom == "bl6_lap" else "fp32"
    with train_precision(precision):
        def changed(write, what):
            """apply `write`, check that it moved the parameters away from what the engine last packed (else the
            coherence check could not fail), then run a forward and check coherence"""
            held = m._engine().packed.clone()
            write()
            assert not torch.equal(held, pack_parameters_device(cfg, m._param_list())), f"{geom}: {what} changed nothing"
            f()
            _assert_coherent(m, f"{geom}: {what}")

        def step(opt):
            opt.zero_grad()
            f().backward()
            opt.step()

        f()
        opt = torch.optim.Adam(drv.optimizer_parameters(m), lr=ADAM_LR)
        for _ in range(2):
            changed(lambda: step(opt), "default Adam")
        snap = {k: v.detach().clone() for k, v in m.state_dict().items()}         # theta_2
        changed(lambda: step(drv.make_adam(drv.optimizer_parameters(m), ADAM_LR)), "make_adam")    # the engine holds theta_3
        changed(lambda: m.load_state_dict(snap), "load_state_dict")   # --resume: back to theta_2
        g = np.random.Generator(np.random.PCG64(4))
        changed(lambda: T.set_scale_in(m, g.normal(size=cfg.n_aux), g.uniform(0.5, 2.0, size=cfg.n_aux)), "set_scale_in")

        def in_place():
            with torch.no_grad():
                m.out_2.weight.mul_(0.5)
                m.conv_aux.conv[0].weight.add_(0.01)
        changed(in_place, "in-place write under no_grad")


@pytest.mark.parametrize("geom", list(GEOMS))
def test_decode_after_training_uses_the_trained_weights(gpu_ok, geom):
    """(e) after the K SGD steps, batch_fast_generate with host noise must reproduce the oracle's decode at the oracle's
    updated parameters: Laplace samples within 1e-5, softmax indices exactly.  Control: at theta_0 the oracle decodes
    something else (Laplace samples 2e-2 to 6e-2 away; softmax indices differ), so a decode on the old weights fails.
    Softmax runs 8 frames: at 2 frames the tiny net's indices do not yet tell theta_0 from theta_K."""
    cfg = GEOMS[geom][0]
    _, th0, thK = _oracle(geom, "sgd")
    _, _, m = _gpu_run(geom, "sgd", coherent=False)
    m.eval()
    frames = 2 if cfg.kind == "laplace" else 8
    n = frames * cfg.U
    aux = torch.from_numpy(synth_aux(cfg, 1, frames, seed=9))

    def oracle(theta):
        P = cpu_ref.as_params(theta)
        if cfg.kind == "laplace":
            noise = cpu_ref.laplace_noise(cfg, n // cfg.seg, 1, generator=torch.Generator().manual_seed(21))
            return cpu_ref.laplace_generate(cfg, P, aux, [n], noise)[0]
        noise = cpu_ref.softmax_noise(cfg, n, 1, generator=torch.Generator().manual_seed(21))
        return cpu_ref.softmax_generate(cfg, P, aux, [n], noise)[0]
    ref, ref0 = oracle(thK), oracle(th0)
    torch.manual_seed(21)
    if cfg.kind == "laplace":
        assert float(np.abs(ref0.astype(np.float64) - ref).max()) > 1e-3, geom          # control
        out = m.batch_fast_generate(torch.zeros(1, cfg.seg), aux.cuda(), [n])[0]
        err = float(np.abs(np.asarray(out, dtype=np.float64) - ref).max())
        assert err <= 1e-5, (geom, err)
    else:
        assert not np.array_equal(ref0, ref), geom                                        # control
        m.noise_source = "host"
        out = m.batch_fast_generate(torch.full((1, 1), cfg.n_quantize // 2), aux.cuda(), [n])[0]
        assert np.array_equal(np.asarray(out), ref), (geom, int(np.sum(np.asarray(out) != ref)))
