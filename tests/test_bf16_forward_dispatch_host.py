"""CPU: which kernels `swn_forward_bf16` runs for a call, read through `swn_forward_bf16_path` - the function the launcher itself
switches on (csrc/swn_stack_bf16.hip: bf16_forward_path), so what is asserted here is what is launched.  No device call.

The table is restated here from DESIGN.md, not derived from the C code.  BL6 class (H = 64, K = 2, S = 128, Laplace), in this
order, with frames = B x Tf and nch = ceil(U / 16):
    seg == 1, 33 <= U, nch <= 7, six layers, frames <= 3072      fused          bf16_stack_fused_kernel
    else seg == 1, 16 <= U, nch <= 7:  nch > 4, frames < 2048    units4_halves  bf16_layer_units_kernel<4>, SP = 2
                                       nch <= 4                  units4         bf16_layer_units_kernel<4>, SP = 1
                                       nch == 5                  units5         bf16_layer_units_kernel<5>
                                       nch 6 or 7                units7         bf16_layer_units_kernel<7>
    otherwise (seg > 1, U < 16, U > 112)                         layer0         bf16_layer_kernel<0>
The other geometries with H a multiple of 64 (run.sh sizes, and the BL6-shaped softmax net, whose head is not the Laplace one)
run the GEMM stack; everything else is refused with SWN_E_UNSUPPORTED, bad sizes with SWN_E_BADARG, as swn_forward_bf16 does.

units4_halves: nch > 4 means U >= 65, fewer than 2 048 frames is below the fused kernel's 3 072, so in the default build the
fused kernel takes every call the branch was written for; only SWN_OLD_UNITS diagnostic builds (no fused kernel) run it.  The
grid asserts that it is never reported (the SP = 2 paragraph).
"""
import ctypes
import dataclasses

import pytest

from shallow_wavenet_amd import _lib, config as C

SEGS = (1, 5)
US = (10, 15, 16, 17, 32, 33, 64, 65, 80, 81, 96, 97, 112, 113, 240)
SIZES = ((1536, 2), (1537, 2), (3072, 1), (3073, 1), (8, 150), (64, 150))
E_BADDESC, E_BADARG, E_UNSUPPORTED = -1, -2, -4


def path_of(cfg, B, Tf):
    """name of the path (or the negative SWN_E_* code) of one call"""
    d = _lib.desc_from_cfg(cfg)
    rc = _lib.lib().swn_forward_bf16_path(ctypes.byref(d), B, Tf)
    return _lib.BF16_PATHS[rc] if rc >= 0 else rc


def bl6(seg, U):
    return dataclasses.replace(C.bl6_laplace(seg, 4 if seg > 1 else 0), upsampling_factor=U)


def table(seg, U, B, Tf):
    """the dispatch table of the module docstring"""
    frames, nch = B * Tf, -(-U // 16)
    if seg == 1 and 33 <= U and nch <= 7 and frames <= 3072:
        return "fused"
    if seg == 1 and 16 <= U and nch <= 7:
        if nch > 4 and frames < 2048:
            return "units4_halves"
        return "units4" if nch <= 4 else "units5" if nch == 5 else "units7"
    return "layer0"


GRID = [(seg, U, B, Tf) for seg in SEGS for U in US for B, Tf in SIZES]


def test_enum_values_are_those_of_the_header():
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swn_hip.h")).read()
    got = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define\s+SWN_BF16_PATH_(\w+)\s+(\d+)", txt)}
    assert got == {n: i for i, n in enumerate(_lib.BF16_PATHS)}


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("U", US)
def test_path_follows_the_table(seg, U):
    for B, Tf in SIZES:
        assert path_of(bl6(seg, U), B, Tf) == table(seg, U, B, Tf), (seg, U, B, Tf)


@pytest.mark.parametrize("U", [33, 64, 65, 80, 81, 96, 97, 110, 112])
def test_3072_frames_is_fused_and_3073_is_not(U):
    want = "units4" if U <= 64 else "units5" if U <= 80 else "units7"
    for B, Tf in ((3072, 1), (1536, 2), (1024, 3), (24, 128)):
        assert path_of(bl6(1, U), B, Tf) == "fused", (U, B, Tf)
    for B, Tf in ((3073, 1), (1537, 2), (1025, 3), (64, 150)):
        assert path_of(bl6(1, U), B, Tf) == want, (U, B, Tf)


def test_every_path_but_the_halves_is_reached_and_the_halves_never():
    seen = {path_of(bl6(seg, U), B, Tf) for seg, U, B, Tf in GRID}
    for cfg in (C.ref6_laplace(1, 4), C.ref6_laplace(5, 4), C.ref6_softmax()):
        seen |= {path_of(cfg, B, Tf) for B, Tf in SIZES}
    assert seen == set(_lib.BF16_PATHS) - {"units4_halves"}
    # the table itself never names it on the grid either: the fused kernel's range covers the branch
    assert "units4_halves" not in {table(seg, U, B, Tf) for seg, U, B, Tf in GRID}
    # ... nor anywhere else in the range of the units kernels, whatever the split of the frames
    for U in range(16, 113):
        for B, Tf in ((1, 1), (1, 2), (3, 7), (8, 150), (2047, 1), (2048, 1), (1, 2047), (3072, 1), (3073, 1)):
            assert path_of(bl6(1, U), B, Tf) != "units4_halves", (U, B, Tf)


def test_the_legs_the_benchmark_times():
    """cfg4: 8 x 150 frames is the fused kernel, 64 x 150 (9 600 frames, U = 110) six launches of bf16_layer_units_kernel<7>"""
    assert path_of(C.bl6_laplace(1, 0), 8, 150) == "fused"
    assert path_of(C.bl6_laplace(1, 0), 64, 150) == "units7"
    assert path_of(C.bl6_laplace(1, 0), 21, 150) == "units7"          # 3 150 frames


@pytest.mark.parametrize("cfg", [C.ref6_laplace(1, 4), C.ref6_laplace(5, 4), C.ref6_laplace(10, 4), C.ref6_softmax(),
                                 dataclasses.replace(C.ref6_softmax(), audio_in_flag=True)],
                         ids=["ref6_s1l4", "ref6_s5l4", "ref6_s10l4", "ref6_softmax", "ref6_softmax_audio_in"])
def test_run_sh_geometries_report_the_gemm_stack(cfg):
    for B, Tf in SIZES + ((1, 1), (2, 3)):
        assert path_of(cfg, B, Tf) == "gemm_stack"


def test_other_geometries_follow_swn_forward_bf16():
    """what swn_forward_bf16 does with a geometry outside the BL6 Laplace class, found on the host before any launch (its
    first statement is this same function): the GEMM stack where H is a multiple of 64 (up to 256) and S, O1 multiples of
    32 - the BL6-shaped softmax net (S = 256) and a BL6 Laplace net with another skip width among them - else unsupported"""
    assert path_of(C.bl6_softmax(), 2, 3) == "gemm_stack"
    assert path_of(dataclasses.replace(C.bl6_laplace(1, 0), skip_chn=64), 2, 3) == "gemm_stack"
    assert path_of(dataclasses.replace(C.bl6_laplace(1, 0), skip_chn=48), 2, 3) == E_UNSUPPORTED
    for cfg in (C.tiny("laplace", 1, 0), C.tiny("laplace", 5, 4), C.tiny("softmax")):
        for B, Tf in SIZES + ((1, 2),):
            assert path_of(cfg, B, Tf) == E_UNSUPPORTED
    assert _lib.lib().swn_forward_bf16_work_bytes(ctypes.byref(_lib.desc_from_cfg(C.tiny())), 2, 3) == 0


def test_refusals_are_those_of_the_launcher():
    cfg = C.bl6_laplace(1, 0)
    for B, Tf in ((0, 3), (-1, 3), (65536, 1), (2, 0), (2, -4)):
        assert path_of(cfg, B, Tf) == E_BADARG, (B, Tf)
        assert path_of(C.ref6_laplace(1, 4), B, Tf) == E_BADARG, (B, Tf)
    assert path_of(cfg, 65535, 1) == "units7"
    # seg 5: Tp = Tf U - 2 seg + 1 must be at least 1
    assert path_of(bl6(5, 8), 1, 1) == E_BADARG
    assert path_of(bl6(5, 10), 1, 1) == "layer0"
    # 32-bit buffer offsets: one level of hidden states (B Tp 128 bytes) below 2 GiB
    assert path_of(cfg, 65535, 3) == E_UNSUPPORTED
    assert path_of(bl6(1, 240), 65535, 1) == "layer0"                  # 65 535 x 239 x 128 bytes: just below
    assert path_of(bl6(1, 240), 65535, 2) == E_UNSUPPORTED
    # a descriptor the library rejects outright, and the launcher with null pointers (nothing is launched)
    d = _lib.desc_from_cfg(cfg)
    d.kernel_size = 1
    L, null = _lib.lib(), ctypes.c_void_p(None)
    assert L.swn_forward_bf16_path(ctypes.byref(d), 2, 3) == E_BADDESC
    assert L.swn_forward_bf16(ctypes.byref(d), null, null, null, null, 2, 3, null, null, null) == E_BADDESC
    d = _lib.desc_from_cfg(cfg)
    assert L.swn_forward_bf16(ctypes.byref(d), null, null, null, null, 2, 3, null, null, null) == E_BADARG
    d = _lib.desc_from_cfg(C.tiny())
    assert L.swn_forward_bf16(ctypes.byref(d), null, null, null, null, 2, 3, null, null, null) == E_UNSUPPORTED
