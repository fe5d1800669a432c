"""CPU: the float64 yardstick of the fp32 training backward (tests/fp32_backward_ref.py) and its case table, before the HIP
kernels are held against them in test_gpu_fp32_backward_edges.py.  For every case:

  - the seed is decisive: in the float64 AND the float32 evaluation of the oracle no pre-activation of either ReLU at a probed
    position lies within PRE_MIN = 1e-5 of zero, and none lies on different sides of zero (a condition, not a measurement);
  - the float64 evaluation is `mixed_ref.exact`, bit for bit, and the float32 one stands where an fp32 evaluation
    should: every D_k within 2e-5 ||g_k|| (2e-7 to 7e-7 typically; the scalar upsampler bias, a sum of cancelling terms, within
    1e-3), positive for every tensor a contraction produces;
  - every per-tensor bound m (D_k + FLOOR D_max / sqrt(n_k)) and every row bound, at the margins the GPU file uses, lies below
    what the rule of test_gpu_backward_parity.py allows (2e-5 + 2e-4 max |g_k|, as an L2 bound: fp32_backward_ref.old_bound); the
    ratio is printed;
  - the launch-arithmetic claims the case carries hold (fp32_backward_ref.launch_facts restates launch_time, launch_reduce,
    BwdCall::cond_layer, BwdCall::frontend, swn_train_path), and the table as a whole reaches both sides of every decision;
  - edge_positions lies inside [0, Tp) and contains what it promises.
"""
import numpy as np
import pytest

import fp32_backward_ref as R
import mixed_ref as M

CASES = R.cases()
FACTS = {c.name: R.launch_facts(c) for c in CASES}


def test_names_paths_and_margins():
    assert len({c.name for c in CASES}) == len(CASES)
    assert {c.path for c in CASES} == set(R.PATHS) == set(R.MARGIN) == set(R.MARGIN_FWD)
    assert all(c.net in R.NETS for c in CASES)
    assert M.edge_positions.__module__ == "mixed_ref" and R.edge_positions is not M.edge_positions


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_yardstick_of_every_case(case):
    inp = R.inputs_of(case)
    y = R.yardstick_of(case)
    assert y.flips == 0, (case.name, y.flips)
    assert y.pre_min >= R.PRE_MIN, (case.name, y.pre_min)
    pre_min, flips = R.decisive(case, inp)                       # the seed search's own figures (forwards only)
    assert flips == 0 and abs(pre_min - y.pre_min) <= 1e-6
    # the float64 evaluation is mixed_ref.exact
    raw_e, g_e = M.exact(*inp)
    assert np.array_equal(raw_e, y.raw)
    assert set(g_e) == set(y.g) == {k for k, _ in case.cfg().param_shapes()}
    for k in g_e:
        assert np.array_equal(g_e[k], y.g[k]), k
    # the float32 evaluation next to it
    assert 0.0 < y.D_fwd <= 1e-5 * max(1.0, float(np.abs(y.raw).max()))
    assert 0.0 < y.D_hs <= 1e-5
    for k, D in y.D.items():
        norm = float(np.linalg.norm(y.g[k].ravel()))
        # (the scalar upsampler bias is a sum of cancelling terms over every position: its error follows the terms, not the sum)
        assert D <= (1e-3 if k == "upsampling.conv.bias" else 2e-5) * norm + 1e-12, (k, D, norm)
        if k.endswith("weight") and not k.startswith(("upsampling", "aux_conv2d")):
            assert D > 0.0 and norm > 0.0, k
    # the new bound against the old rule's
    m, worst = R.MARGIN[case.path], 0.0
    for k in y.D:
        new, old = m * (y.D[k] + R.floor_of(y, k)), R.old_bound(y, k)
        worst = max(worst, new / old)
        assert new < old, (case.name, k, new, old)
    print(f"{case.name}: the new tensor bounds are at most {worst:.2e} of the old rule's")
    for k in y.D_rows:
        assert float((m * R.row_yardstick(y, k)).max()) < R.old_bound(y, k), k


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_launch_arithmetic_of_every_case(case):
    f = FACTS[case.name]
    for key, want in case.expect:
        assert f[key] == want, (case.name, key, f[key], want)
    assert f["route"] == "chain"
    base = {"time_gemm", "reduce_gemm", "gate_bwd", "input_bwd"}
    if case.path == "chain":
        assert f["kernels"] == base | {f"cond_bwd<{f['cond_nch']}>", "wup_fold"}
    else:
        assert f["kernels"] - {"mask_mul"} == base | {"xm_bwd"}
        assert f["dgx_all"] == (case.path == "drop1") and f["inx"] == ("inx_all" if case.path == "drop1" else "inx_layer")
        assert R.seg_of(case.cfg()) == 1 if case.path == "drop1" else R.seg_of(case.cfg()) > 1


def test_the_table_reaches_both_sides_of_every_launch_decision():
    fs = list(FACTS.values())
    have = lambda key: {f[key] for f in fs if key in f}
    assert {511, 512, 513, 1023, 1025} <= have("Tp")
    assert {1, 2, 3} <= have("segments")
    assert {7, 8, 9} <= have("time_pairs") and {1, 2} <= have("xcd_chunk")
    assert {7, 8, 9} <= have("segment_pairs") and {1, 2} <= have("segment_rounds")
    # ... with more than one tile / segment per utterance among them
    assert {(7, 7), (8, 4), (9, 3)} <= {(f["time_pairs"], f["time_tiles"]) for f in fs}
    assert {(8, 2), (9, 3)} <= {(f["segment_pairs"], f["segments"]) for f in fs}
    assert {1, 2, 3, 4} <= have("gate_tiles")
    assert {2, 5} == have("cond_nch") and {128, 129, 260} <= have("cond_columns") and {1, 2, 3, 5} <= have("cond_chunks")
    assert {1, 2} <= have("FR") and any(f.get("FR") == 2 and f["last_group"] == 1 for f in fs)
    assert {0, 4, 32} <= have("k_tail") and {1, 2, 6} <= have("row_tiles") and {2, 3, 5, 7} <= have("taps")
    assert {"inx_all", "inx_layer"} == have("inx")
    assert any("mask_mul" in f["kernels"] for f in fs)
    assert any(c.Tf == 1 for c in CASES) and any(c.frames for c in CASES)
    assert {c.path for c in CASES if c.own_hs} == {"chain", "drop1"}
    assert any(c.drop and c.unmasked for c in CASES)
    cfgs = [c.cfg() for c in CASES]
    assert {1, 3, 5} <= {c.aux_kernel_size for c in cfgs} and {1, 2, 3, 4} <= {c.aux_dilation_size for c in cfgs}
    assert any(c.aux_conv2d_flag for c in cfgs) and {90, 256, 300} <= {c.n_quantize for c in cfgs if c.kind == "softmax"}
    # a conv_aux dilation that reaches past the frame count
    assert any(c.cfg().aux_kernel_size ** (c.cfg().aux_dilation_size - 1) > c.Tf for c in CASES if c.net.startswith("fe_"))
    # every net of the table is one the backward serves
    assert all(c.H % 4 == 0 and c.K <= 8 and c.U <= 256 for c in cfgs)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_edge_positions(case):
    cfg = case.cfg()
    Tp, U, seg = case.Tp, cfg.U, R.seg_of(cfg)
    pos = R.edge_positions(cfg, case.Tf)
    assert pos == sorted(set(pos)) and pos[0] == 0 and pos[-1] == Tp - 1 and all(0 <= p < Tp for p in pos)
    want = {0, 1, Tp - 2, Tp - 1}
    d, rf = max(cfg.dilations), cfg.receptive_field
    want |= {d - 1, d, d + 1, rf - 1, rf}
    for tile in (16, 64, 256, 512):
        want |= {tile - 1, tile, (Tp - 1) // tile * tile - 1, (Tp - 1) // tile * tile}
    for k in (1, 2):
        want |= {k * U - seg - 1, k * U - seg, k * U - 2 * seg, k * U - 2 * seg + 1}
    assert {p for p in want if 0 <= p < Tp} <= set(pos)
    # the probe is what the case says
    grad = R.inputs_of(case)[4].numpy()
    probed = np.abs(grad).max(axis=1) > 0
    if case.probe == "edges":
        assert all(sorted(np.nonzero(row)[0]) == pos for row in probed)
    elif case.probe == "single":
        b, t = case.at
        assert probed.sum() == 1 and probed[b % case.B, t % Tp]
    else:
        assert probed.all()
