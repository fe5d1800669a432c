"""CPU: the float64 yardstick of the mixed-precision backward (tests/mixed_ref.py) before the HIP kernels are held against it
in test_gpu_mixed_backward_edges.py.

  - `exact` (the oracle in float64 under autograd) reproduces the reference's own loss and gradients of the g0_* / g1_*
    fixtures: the tolerances of test_oracle_golden.py for the float32 oracle (1e-5 + 1e-4 max|g| per element, 2e-4 of
    the summed magnitude for the digests), which are the float32 accuracy of the FIXTURES - float64 cannot be held tighter
    against them; the loss to 1e-6 (ten times tighter).
  - `rounded` with every rounding off is `exact`, bit for bit; in the hoisted form of the conditioning it agrees to 1e-12.
  - per case of cases(): D_k > 0 for every tensor the matrix cores touch; no ReLU unit at a probed position of an `edges` /
    `single` case changes side between the two graphs or lies within the case's gap of zero; and margin * D_k + floor_k stays
    below what the old tests allow that tensor (5e-2 ||g|| + 1e-3 of the largest norm, 1e-1 for the softmax nets), so the new
    file cannot be the weaker check anywhere.
  - the forward yardstick of tests/bf16_forward_ref.py (test_gpu_bf16_forward_paths.py): at the geometries it adds (seg 5 at the
    BL6 class, U = 15, 113, 240) `rounded` with every rounding off is `exact` bit for bit and the hoisted form agrees to 1e-12;
    per case D_rms and D_fwd are positive and m_f D_fwd lies below test_gpu_bf16_stack.py's 3e-3 x max(1, |raw| max).
"""
import numpy as np
import pytest
import torch

import bf16_forward_ref as F
import mixed_ref as M
from conftest import golden_names, load_golden
from oracle import cpu_ref
from shallow_wavenet_amd.synth import synth_state_dict

CASES = M.cases()
LAP = [n for n in golden_names() if n.startswith(("g0_", "g1_")) and "_lap_" in n and "loss" in load_golden(n)[1]]


@pytest.mark.parametrize("name", LAP)
def test_exact_reproduces_the_reference_gradients(name):
    """the loss is not linear in raw: d loss / d raw comes from autograd on the oracle's head, then `exact` takes it as the
    upstream gradient"""
    cfg, d = load_golden(name)
    sd = synth_state_dict(cfg, seed=int(d["wseed"]), flavor=str(d["flavor"]))
    P = cpu_ref.as_params(sd, dtype=torch.float64)
    aux, audio = torch.from_numpy(d["aux"]).double(), torch.from_numpy(d["fwd_audio"]).double()
    raw = cpu_ref.laplace_stack(cfg, P, aux, audio)[0].detach().requires_grad_(True)
    seg = cfg.seg
    out = raw.transpose(1, 2)
    mu, log_b = out[:, :, :seg], torch.nn.functional.logsigmoid(out[:, :, seg:2 * seg])
    if cfg.lpc == 0 and seg == 1:
        mu, log_b = mu.reshape(out.shape[0], -1), log_b.reshape(out.shape[0], -1)
    loss = cpu_ref.laplace_nll(mu, torch.exp(log_b), torch.from_numpy(d["loss_target"]).double(), log_b=log_b)
    if cfg.lpc > 0:
        loss = loss + 0.1 * out[:, :, 2 * seg:].pow(2).mean()
    assert abs(loss.item() - float(d["loss"])) <= 1e-6 * max(1.0, abs(float(d["loss"])))
    loss.backward()
    raw_e, g = M.exact(cfg, sd, d["aux"], d["fwd_audio"], raw.grad.numpy())
    assert np.array_equal(raw_e, raw.detach().numpy())
    seen = 0
    for k, gk in g.items():
        if f"gdig_{k}" in d:
            dig = d[f"gdig_{k}"]                      # (sum, sum of magnitudes) of the reference's gradient
            scale = max(1e-3, float(dig[1]))
            assert abs(gk.sum() - float(dig[0])) <= 2e-4 * scale, k
            assert abs(np.abs(gk).sum() - float(dig[1])) <= 2e-4 * scale, k
        if f"grad_{k}" in d:
            seen += 1
            assert np.abs(gk - d[f"grad_{k}"]).max() <= 1e-5 + 1e-4 * np.abs(d[f"grad_{k}"]).max(), k
    assert seen


SMX = [n for n in golden_names() if n.startswith(("g0_", "g1_")) and "softmax" in n and "loss" in load_golden(n)[1]]


def _against_fixture(d, g):
    seen = 0
    for k, gk in g.items():
        if f"gdig_{k}" in d:
            dig = d[f"gdig_{k}"]
            scale = max(1e-3, float(dig[1]))
            assert abs(gk.sum() - float(dig[0])) <= 2e-4 * scale, k
            assert abs(np.abs(gk).sum() - float(dig[1])) <= 2e-4 * scale, k
        if f"grad_{k}" in d:
            seen += 1
            assert np.abs(gk - d[f"grad_{k}"]).max() <= 1e-5 + 1e-4 * np.abs(d[f"grad_{k}"]).max(), k
    assert seen


@pytest.mark.parametrize("name", SMX)
def test_exact_reproduces_the_reference_gradients_softmax(name):
    """the softmax branch of `exact` (int64 class indices, one_hot in float64) on the fixtures that carry a loss: cross-entropy
    over the logits, as the reference's training script"""
    cfg, d = load_golden(name)
    sd = synth_state_dict(cfg, seed=int(d["wseed"]), flavor=str(d["flavor"]))
    P = cpu_ref.as_params(sd, dtype=torch.float64)
    idx = torch.from_numpy(d["fwd_audio_idx"]).long()
    raw = cpu_ref.softmax_stack(cfg, P, idx, torch.from_numpy(d["aux"]).double())[0].detach().requires_grad_(True)
    logits = raw.transpose(1, 2)
    loss = torch.nn.CrossEntropyLoss()(logits.reshape(-1, cfg.n_quantize), torch.from_numpy(d["loss_target"]).long().reshape(-1))
    assert abs(loss.item() - float(d["loss"])) <= 1e-6 * max(1.0, abs(float(d["loss"])))
    loss.backward()
    raw_e, g = M.exact(cfg, sd, d["aux"], d["fwd_audio_idx"], raw.grad.numpy())
    assert np.array_equal(raw_e, raw.detach().numpy())
    _against_fixture(d, g)


def _one_per_kind():
    seen, out = set(), []
    for c in CASES:
        key = (c.geom, c.drop, c.lpc, c.frames is not None)
        if key not in seen and c.B * c.Tf <= 12:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _one_per_kind(), ids=lambda c: c.name)
def test_rounding_switched_off_is_exact(case):
    inp = M.inputs_of(case)
    raw_e, g_e = M.exact(*inp)
    raw_0, g_0 = M.rounded(*inp, path=None)
    assert np.array_equal(raw_0, raw_e)
    for k in g_e:
        assert np.array_equal(g_0[k], g_e[k]), k
    raw_h, g_h = M.rounded(*inp, path="hoisted")
    assert np.abs(raw_h - raw_e).max() <= 1e-12 * max(1.0, np.abs(raw_e).max())
    for k in g_e:
        assert np.linalg.norm((g_h[k] - g_e[k]).ravel()) <= 1e-12 * np.linalg.norm(g_e[k].ravel()) + 1e-300, k


FWD_CASES = F.cases()


@pytest.mark.parametrize("case", [c for c in FWD_CASES if c.path == "layer0" and c.B <= 3], ids=lambda c: c.name)
def test_rounding_switched_off_is_exact_at_the_forward_geometries(case):
    """the geometries bf16_forward_ref.py adds to those of cases(): seg 5 at the BL6 class (five conditioning taps per
    position in the hoisted form), U = 15, U = 113 and U = 240 (frames shorter than a chunk, longer than seven)"""
    cfg, sd, aux, audio = F.inputs_of(case)
    grad_raw = np.random.Generator(np.random.PCG64(5)).standard_normal((case.rows, cfg.n_out, case.Tp)) / case.Tp
    raw_e, g_e = M.exact(cfg, sd, aux, audio, grad_raw)
    raw_0, g_0 = M.rounded(cfg, sd, aux, audio, grad_raw, path=None)
    assert raw_e.shape == (case.rows, cfg.n_out, case.Tp)
    assert np.array_equal(raw_0, raw_e)
    for k in g_e:
        assert np.array_equal(g_0[k], g_e[k]), k
    raw_h, g_h = M.rounded(cfg, sd, aux, audio, grad_raw, path="hoisted")
    assert np.abs(raw_h - raw_e).max() <= 1e-12 * max(1.0, np.abs(raw_e).max())
    for k in g_e:
        assert np.linalg.norm((g_h[k] - g_e[k]).ravel()) <= 1e-12 * np.linalg.norm(g_e[k].ravel()) + 1e-300, k


@pytest.mark.parametrize("case", FWD_CASES + [F.TRAIN_CASE], ids=lambda c: c.name)
def test_forward_yardstick_of_every_case(case):
    """D_fwd and D_rms exist, the padded utterance is among the rows, and the new bound lies below what
    test_gpu_bf16_stack.py allows (3e-3 x max(1, |raw| max)), so the new file cannot be the weaker check anywhere"""
    y = F.yardstick_of(case)
    assert y.raw_exact.shape == y.raw_rounded.shape == (case.rows, case.cfg().n_out, case.Tp)
    assert np.isfinite(y.raw_exact).all() and np.isfinite(y.raw_rounded).all()
    assert 0.0 < y.D_rms <= y.D_fwd
    assert F.MARGIN_FWD[case.path] * y.D_fwd < y.old_bound, (case.name, F.MARGIN_FWD[case.path] * y.D_fwd, y.old_bound)
    aux = F.inputs_of(case)[2]
    pad = min(F.PAD_ROW, case.rows - 1)
    assert case.Tf == 1 or (not aux[pad, :, 1:].any() and aux[pad, :, 0].any())
    assert all(aux[b, :, -1].any() for b in range(case.rows) if b != pad)


def test_forward_cases_cover_every_kernel_of_the_dispatch_table():
    assert {c.path for c in FWD_CASES} == set(F.MARGIN_FWD) == {"fused", "units4", "units5", "units7", "layer0"}
    assert len({c.name for c in FWD_CASES}) == len(FWD_CASES)
    assert max(c.B * c.Tp for c in FWD_CASES) <= 350_000


def test_margins_cover_every_group():
    groups = {c.margin_group for c in CASES}
    assert groups <= set(M.MARGIN) and groups <= set(M.MARGIN_FWD)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_yardstick_of_every_case(case):
    y = M.yardstick_of(case)
    # exact row sums of the upstream gradient: nothing rounds on the way to out_2.bias in the chain
    mma = [k for k in y.D if k.startswith(("dil_h.", "out_skip.", "out_1.", "out_2.weight", "in_x.", "conv_aux.", "scale_in."))]
    for k in mma:
        assert y.D[k] > 0.0, k
    assert y.D_fwd > 0.0
    if case.probe != "dense":
        assert y.flips == 0, (case.name, y.flips)
        assert y.pre_min >= case.pre_min, (case.name, y.pre_min)
    m = M.MARGIN[case.margin_group]
    for k in y.D:
        new = m * (y.D[k] + M.FLOOR * y.D_max)
        assert new <= M.old_bound(case, y, k), (case.name, k, new, M.old_bound(case, y, k))


@pytest.mark.parametrize("case", [c for c in CASES if c.probe == "single"], ids=lambda c: c.name)
def test_the_model_in_float32_meets_the_bounds_of_the_gpu_file(case):
    """the rounded model evaluated in float32 between its roundings - what the device does, in another order - is itself a
    'device' without a defect: tensors, rows and forward must lie within the bounds test_gpu_mixed_backward_edges.py applies
    (mixed_ref.violations).  It lands 0.3-0.4 D_k from the float64 evaluation in some cases, single rows at 2.5-2.7 D_row: the
    reason the rows' yardstick carries the number format's step (mixed_ref.row_yardstick)."""
    inp = M.inputs_of(case)
    y = M.yardstick_of(case)
    raw, g = M.rounded(*inp, path=case.path, dtype=torch.float32)
    assert not M.violations(case, M.deviations(case, y, raw.astype(np.float64), g))
