"""CPU: the return codes of the one-shot swn_decode for every refusal that comes before a launch.  It chooses its kernel
through the same resolution as the streamed entry points, and keeps its own order of checks around it."""
import ctypes

import pytest

from shallow_wavenet_amd import _lib, config as C

OK, BADARG, UNSUPPORTED = 0, -2, -4


def _io():
    return _lib.DecodeIO(noise_dev=None, forced_dev=None, seed_dev=None, noise_out_dev=None, rng_seed=1, rng_utt0=0,
                         reserved=0, rng_utt_ids_dev=None)


def _decode(cfg, variant=0, batch=1, frames=4, n_steps=4, io=True, packed=1, cond=1, state=1, out=1):
    """fake non-null addresses are fine: every call here is refused before the library touches them"""
    d = _lib.desc_from_cfg(cfg)
    p = lambda v: ctypes.c_void_p(v) if v else None
    return _lib.lib().swn_decode(ctypes.byref(d), p(packed), p(cond), batch, frames, n_steps,
                                 ctypes.byref(_io()) if io else None, p(state), p(out), None, variant, None)


BL6, TINY, REF6 = C.bl6_laplace(), C.tiny("laplace", 2, 4), C.ref6_laplace()


def test_argument_checks_come_first_and_in_order():
    assert _decode(BL6, batch=0) == BADARG
    assert _decode(BL6, frames=0) == BADARG
    assert _decode(BL6, n_steps=-1) == BADARG
    assert _decode(BL6, io=False) == BADARG
    # nothing to generate: fine whatever the buffers and the variant are
    assert _decode(BL6, n_steps=0, packed=0, cond=0, out=0, state=0, variant=9) == OK
    assert _decode(BL6, packed=0) == BADARG
    assert _decode(BL6, cond=0) == BADARG
    assert _decode(BL6, out=0) == BADARG
    assert _decode(BL6, n_steps=4 * 110 + 1) == BADARG           # conditioning too short
    assert _decode(TINY, variant=6, n_steps=10 ** 6) == BADARG   # ... is checked before the variant is


@pytest.mark.parametrize("cfg", [TINY, REF6, C.tiny("softmax")])
@pytest.mark.parametrize("state", [0, 1])
def test_bl6_only_variants_on_another_net(cfg, state):
    """2 and 6 ask for the BL6 class alone: unsupported, with or without a state buffer"""
    assert _decode(cfg, variant=2, state=state) == UNSUPPORTED
    assert _decode(cfg, variant=6, state=state) == UNSUPPORTED


@pytest.mark.parametrize("cfg", [BL6, TINY, REF6])
@pytest.mark.parametrize("state", [0, 1])
@pytest.mark.parametrize("variant", [4, 5, 7, -1])
def test_retired_and_unknown_variants(cfg, state, variant):
    """4 and 5 (ABI 2) are retired; on a BL6-class net too, where 0 / 2 / 6 never look at the state"""
    assert _decode(cfg, variant=variant, state=state) == BADARG


@pytest.mark.parametrize("cfg,variant", [(TINY, 0), (TINY, 1), (TINY, 3), (REF6, 0), (REF6, 1), (REF6, 3), (BL6, 1), (BL6, 3)])
def test_generic_and_stepped_kernels_want_a_state_buffer(cfg, variant):
    assert _decode(cfg, variant=variant, state=0) == BADARG
