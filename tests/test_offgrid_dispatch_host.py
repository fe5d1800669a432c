"""CPU: which decode kernel the library picks for the off-grid nets of the g10 fixtures (swn_decode_resolve_variant is a
host function), and where the generic kernel's LDS plan - sized by the segment template it is launched with - stops
fitting.  tests/test_gpu_offgrid_geometry.py runs the kernels this table names."""
import ctypes

import pytest

from conftest import golden_names, load_golden
from shallow_wavenet_amd import _lib, config as C

UNSUPPORTED = -4                                # SWN_E_UNSUPPORTED
GENERIC, STEPPED = 1, 3

# net -> kernel of variants (0, 1, 2, 3, 6) at batch 2: every net decodes on the generic kernel (0 and 1) and on the stepped
# chain (3); none has a BL6 kernel (2, 6) - the two BL6-shaped ones included, whose (S, seg, lpc) is outside with_tr's list
SERVED = {
    "g10_odd_laplace_h30_s50_seg3": (GENERIC, GENERIC, UNSUPPORTED, STEPPED, UNSUPPORTED),
    "g10_odd_laplace_h20_s33_k5": (GENERIC, GENERIC, UNSUPPORTED, STEPPED, UNSUPPORTED),
    "g10_odd_laplace_h36_seg7": (GENERIC, GENERIC, UNSUPPORTED, STEPPED, UNSUPPORTED),
    "g10_odd_laplace_seg4_c2d": (GENERIC, GENERIC, UNSUPPORTED, STEPPED, UNSUPPORTED),
    "g10_odd_laplace_nearbl6_s144": (GENERIC, GENERIC, UNSUPPORTED, STEPPED, UNSUPPORTED),
    "g10_odd_laplace_nearbl6_seg2l0": (GENERIC, GENERIC, UNSUPPORTED, STEPPED, UNSUPPORTED),
    "g10_odd_smx_q90_h28_audioin": (GENERIC, GENERIC, UNSUPPORTED, STEPPED, UNSUPPORTED),
    "g10_odd_smx_q300_h44_wav": (GENERIC, GENERIC, UNSUPPORTED, STEPPED, UNSUPPORTED),
}


def resolve(cfg, variant, batch=2):
    return _lib.lib().swn_decode_resolve_variant(ctypes.byref(_lib.desc_from_cfg(cfg)), batch, variant)


def test_the_table_names_every_fixture():
    assert sorted(SERVED) == golden_names("g10_odd_")


@pytest.mark.parametrize("name", sorted(SERVED))
def test_kernel_that_serves_each_net(name):
    cfg, _ = load_golden(name)
    for batch in (1, 2, 3):
        assert tuple(resolve(cfg, v, batch) for v in (0, 1, 2, 3, 6)) == SERVED[name], (name, batch)


def test_near_bl6_nets_are_bl6_shaped():
    """the stack the BL6 kernels are written for (H 64, K 2, 1 x 6 layers, S % 16 == 0) - only S / (seg, lpc) differ from a
    net they serve, so the lane-tiled weight copies are packed and the dispatch must fall through to the generic kernel"""
    for name in ("g10_odd_laplace_nearbl6_s144", "g10_odd_laplace_nearbl6_seg2l0"):
        cfg, _ = load_golden(name)
        assert (cfg.H, cfg.K, cfg.dilation_depth, cfg.dilation_repeat, cfg.S % 16) == (64, 2, 6, 1, 0)
    ok = C.bl6_laplace(2, 4)
    assert resolve(ok, 0) == 2 and resolve(ok, 6) == 6


def _wide(seg, H):
    return C.NetConfig(kind="laplace", n_aux=2, hid_chn=H, skip_chn=4, kernel_size=2, dilation_depth=3, dilation_repeat=1,
                       upsampling_factor=4, seg=seg, lpc=0, aux_kernel_size=1, aux_dilation_size=1)


def test_generic_lds_plan_follows_the_segment_template():
    """the generic kernel is compiled for 1, 2, 5 and 10 segments and keeps SEGT gate rows of round4(2H) floats in LDS; seg 3
    and 4 run on the 5-segment template, 6..9 on the 10-segment one.  At H = 1800 the 5-segment plan is
    4 * (5 * 3600 + 3 * 1800 + ...) = 94 KB and fits the 160 KB the kernel may ask for, the 10-segment plan (167 KB) does
    not: a seg-3 net served by a wider template than it needs would be refused here."""
    for seg in (1, 2, 3, 4, 5):
        assert resolve(_wide(seg, 1800), 1) == GENERIC, seg
    for seg in (6, 7, 10):
        assert resolve(_wide(seg, 1800), 1) == UNSUPPORTED, seg
    for seg in (3, 7):
        assert resolve(_wide(seg, 1700), 1) == GENERIC, seg          # 157 KB with ten segments: both fit
