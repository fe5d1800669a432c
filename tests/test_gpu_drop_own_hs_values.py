"""The dropout-mode pair with a caller-owned hs in the mixed-precision mode, for VALUES.

test_gpu_train_work_bounds.py::test_drop_bf16_ref6_own_hs runs this pair for buffer bounds only, and the Python runtime never
passes its own hs in the dropout mode: only a C-ABI caller reaches it.  Forward and backward resolve one path record
(SwnTrainPath, csrc/swn_train_internal.hpp); with a caller-owned hs it takes no bf16 copies of the in_x operands, so the
backward reads xm in the format the forward wrote.

Net ref6_laplace(1, 4), B 1, Tf 3 (Tp = 329), the masks of the bounds test, the same inputs three ways:
  (a) fp32 precision, own hs      (b) bf16 precision, own hs      (c) bf16 precision, the library's hs
For every parameter tensor the relative L2 distance of (b) from (a) must be at most twice that of (c) from (a).  (c) is the path
the float64 oracle pins (ref6-keep-drop-edges), so it is the yardstick; (b) and (c) are different realisations of the same
roundings (tests/mixed_ref.py measures such pairs 0.3-0.4 of a deviation apart at tensor level), hence the factor 2.  A backward
that reads bf16 rows as fp32 misses by orders of magnitude.  No absolute tolerance."""
import pytest
import torch

import test_gpu_train_work_bounds as WB
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.nets._autograd import unfold_packed_grads
from shallow_wavenet_amd.runtime import _ptr
from shallow_wavenet_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

CFG, B, TF = C.ref6_laplace(1, 4), 1, 3


def _grads(mode, own_hs):
    """swn_forward_drop + swn_backward_drop as WB._drop calls them -> {state_dict key: gradient} on the host"""
    c = WB.Case(CFG, B, TF, cond=False)
    hptr = c.masks(range(CFG.L))
    fw = c.window(4 * c.L.swn_forward_drop_work_floats(c.d, B, TF), "forward work")
    bw = c.window(4 * c.L.swn_backward_drop_work_floats(c.d, B, TF), "backward work")
    hs_ptr = c.window(4 * B * (CFG.L + 1) * CFG.H * c.Tp, "hs").ptr if own_hs else None
    c.call("swn_forward_drop", c.d, _ptr(c.packed), c.fe.ptr, _ptr(c.audio), B, TF, _ptr(c.drop_x), hptr, fw.ptr, _ptr(c.out),
           hs_ptr, mode, c.st)
    c.call("swn_backward_drop", c.d, _ptr(c.packed), _ptr(c.aux), c.fe.ptr, _ptr(c.audio), fw.ptr, hs_ptr, _ptr(c.drop_x), hptr,
           _ptr(c.grad), B, TF, bw.ptr, _ptr(c.gp), mode, c.st)
    c.finish()
    params = {k: torch.from_numpy(v) for k, v in synth_state_dict(CFG, seed=5, flavor="trained").items()}
    return unfold_packed_grads(CFG, c.gp.cpu(), params)


def test_own_hs_bf16_is_as_close_to_fp32_as_the_library_hs_path(gpu_ok):
    a, b, c = _grads(WB.FP32, True), _grads(WB.BF16, True), _grads(WB.BF16, False)
    assert set(a) == set(b) == set(c)
    bad = []
    for k in a:
        na = float(a[k].double().norm())
        assert na > 0 and bool(torch.isfinite(b[k]).all()) and bool(torch.isfinite(c[k]).all()), k
        db, dc = float((b[k] - a[k]).double().norm()) / na, float((c[k] - a[k]).double().norm()) / na
        print(f"{k:28s} own-hs bf16 {db:.3e}   library-hs bf16 {dc:.3e}   ratio {db / dc if dc else float('inf'):.3f}")
        if not db <= 2.0 * dc:
            bad.append((k, db, dc))
    assert not bad, bad
