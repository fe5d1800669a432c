"""CPU: the stepped decode pool (swn_decode_pool_stepped_chunk / SteppedDecodePool): the C ABI's argument checks, the op
schema, tick planning with split prologues, slot bookkeeping and the routing of open_pool - everything that runs before a
device is touched."""
import ctypes
import re

import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops
from shallow_wavenet_amd.streaming import DecodePool, SteppedDecodePool, plan_stepped_tick

BADARG, UNSUPPORTED = -2, -4                   # SWN_E_BADARG, SWN_E_UNSUPPORTED (include/swn_hip.h)


def test_stepped_pool_symbols_are_exported_and_bound():
    lib = _lib.lib()
    for name in ("swn_decode_pool_stepped_chunk", "swn_decode_stepped_prologue_iterations"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.DecodeSteppedPoolEntry) == 32
    assert _lib.DECODE_STEPPED_POOL_TABLE_FLOATS * 4 >= 64 * 32
    assert "decode_pool_stepped_chunk" in ops.OP_NAMES
    schema = str(torch.ops.swn.decode_pool_stepped_chunk.default._schema)
    assert schema.startswith("swn::decode_pool_stepped_chunk(") and re.search(r"Tensor\(a\d*!\) session", schema)


def test_prologue_iterations_of_ref6():
    lib = _lib.lib()
    assert lib.swn_decode_stepped_prologue_iterations(ctypes.byref(_lib.desc_from_cfg(C.ref6_laplace(1, 4)))) == 690
    assert lib.swn_decode_stepped_prologue_iterations(ctypes.byref(_lib.desc_from_cfg(C.ref6_laplace(5, 4)))) == 686


def _io(noise=0, forced=0):
    return _lib.DecodeIO(noise_dev=noise or None, forced_dev=forced or None, seed_dev=None, noise_out_dev=None, rng_seed=1,
                         rng_utt0=0, reserved=0, rng_utt_ids_dev=None)


def _entry(slot=0, it0=0, n_it=4, flags=1, frames=4, cond=1, reserved=0):
    return _lib.DecodeSteppedPoolEntry(cond_dev=cond or None, n_frames=frames, slot=slot, it0=it0, n_it=n_it, flags=flags,
                                       reserved=reserved)


def _pool(d, entries, capacity=4, io=None, session=1, packed=1, out=1, n_entries=None, table=True):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    arr = (_lib.DecodeSteppedPoolEntry * max(1, len(entries)))(*entries)
    return lib.swn_decode_pool_stepped_chunk(ctypes.byref(d), p(packed), capacity, arr if table else None,
                                             len(entries) if n_entries is None else n_entries,
                                             ctypes.byref(io if io is not None else _io()), p(session), p(out), None, None)


def test_stepped_pool_rejects_bad_arguments_before_any_launch():
    """fake non-null addresses are fine: every one of these is refused before the library touches them"""
    d = _lib.desc_from_cfg(C.ref6_laplace())
    n_pro = 690
    U = C.ref6_laplace().U
    ok = [_entry(0, n_it=100), _entry(1, it0=n_pro + 8, n_it=2, flags=0, frames=8)]
    assert _pool(d, ok, session=0) == BADARG                       # null pointers
    assert _pool(d, ok, packed=0) == BADARG
    assert _pool(d, [_entry(0, it0=n_pro, n_it=2, flags=0)], out=0) == BADARG   # generation steps need out
    assert _pool(d, ok, table=False) == BADARG
    assert _pool(d, [_entry(cond=0)]) == BADARG
    assert _lib.lib().swn_decode_pool_stepped_chunk(ctypes.byref(d), ctypes.c_void_p(1), 4,
                                                    (_lib.DecodeSteppedPoolEntry * 1)(_entry()), 1, None,
                                                    ctypes.c_void_p(1), ctypes.c_void_p(1), None, None) == BADARG
    assert _pool(d, ok, n_entries=0) == BADARG                     # entry count outside [1, 64]
    assert _pool(d, [_entry(i, n_it=0, flags=0, it0=5) for i in range(65)], capacity=65, n_entries=65) == BADARG
    assert _pool(d, ok, capacity=0) == BADARG
    assert _pool(d, [_entry(4)]) == BADARG                         # slot outside [0, capacity)
    assert _pool(d, [_entry(-1)]) == BADARG
    assert _pool(d, [_entry(2), _entry(2, it0=4, flags=0)]) == BADARG               # one slot in two entries
    assert _pool(d, [_entry(0, it0=1, flags=1)]) == BADARG         # BEGIN must start at iteration 0
    assert _pool(d, [_entry(0, it0=0, n_it=3, flags=0)]) == BADARG  # iteration 0 without BEGIN
    assert _pool(d, [_entry(0, it0=-1, flags=0)]) == BADARG
    assert _pool(d, [_entry(0, it0=5, n_it=-1, flags=0)]) == BADARG
    # the last generation step past the final conditioning: (step + 1) * seg <= n_frames * U
    assert _pool(d, [_entry(0, it0=n_pro, n_it=4 * U + 1, flags=0, frames=4)]) == BADARG
    assert _pool(d, [_entry(0, n_it=n_pro + 4 * U + 1, frames=4)]) == BADARG
    assert _pool(d, [_entry(0, flags=2)]) == BADARG                # unknown flag
    assert _pool(d, [_entry(0, reserved=1)]) == BADARG
    assert _pool(d, ok, io=_io(noise=1)) == BADARG                 # pools draw their noise on the device
    assert _pool(d, ok, io=_io(forced=1)) == BADARG                # ... and take no teacher forcing


def test_stepped_pool_unsupported_and_idle_calls_launch_nothing():
    d = _lib.desc_from_cfg(C.ref6_laplace())
    # a capacity whose state passes the 2 GiB buffer-offset limit: the stepped chain does not run it
    per_slot = _lib.lib().swn_decode_session_floats(ctypes.byref(d), 1, 3)
    big = (1 << 31) // (4 * per_slot) + 1
    assert _lib.lib().swn_decode_resolve_variant(ctypes.byref(d), big, 3) < 0
    assert _pool(d, [_entry(0)], capacity=big) == UNSUPPORTED
    # entries of 0 iterations without BEGIN leave their slots as they are: nothing to launch, so fake addresses are fine
    assert _pool(d, [_entry(0, it0=5, n_it=0, flags=0), _entry(3, it0=700, n_it=0, flags=0)], out=0) == 0
    # the existing pool keeps refusing the stepped decode
    e = (_lib.DecodePoolEntry * 1)(_lib.DecodePoolEntry(cond_dev=1, n_frames=4, slot=0, step0=0, n_steps=4, flags=1,
                                                        reserved=0))
    assert _lib.lib().swn_decode_pool_chunk(ctypes.byref(d), ctypes.c_void_p(1), 4, e, 1, ctypes.byref(_io()),
                                            ctypes.c_void_p(1), ctypes.c_void_p(1), None, 3, None) == UNSUPPORTED


def test_plan_stepped_tick_runs_prologue_then_steps():
    n_pro = 10
    s = [("new", 5, 0), ("mid", 5, 4), ("gen", 20, n_pro + 3), ("wait", 0, 0), ("done", 6, n_pro + 6)]
    assert plan_stepped_tick(s, n_pro) == [[("new", 0, 15), ("mid", 4, 11), ("gen", 13, 17)]]
    assert plan_stepped_tick(s, n_pro, max_steps=2) == [[("new", 0, 12), ("mid", 4, 8), ("gen", 13, 2)]]
    # a split prologue: no generation until the prologue is complete
    assert plan_stepped_tick(s, n_pro, max_prologue=3) == [[("new", 0, 3), ("mid", 4, 3), ("gen", 13, 17)]]
    assert plan_stepped_tick(s, n_pro, max_steps=1, max_prologue=6) == [[("new", 0, 6), ("mid", 4, 7), ("gen", 13, 1)]]
    assert plan_stepped_tick([("wait", 0, 0), ("wait2", 0, 3)], n_pro) == []
    for bad in (0, -1):
        with pytest.raises(ValueError):
            plan_stepped_tick(s, n_pro, max_steps=bad)
        with pytest.raises(ValueError):
            plan_stepped_tick(s, n_pro, max_prologue=bad)


def test_plan_stepped_tick_splits_calls_at_64_entries():
    s = [(i, 5, 690 if i % 2 else 0) for i in range(130)]
    calls = plan_stepped_tick(s, 690, max_steps=2, max_prologue=100)
    assert [len(c) for c in calls] == [64, 64, 2]
    assert [e[0] for c in calls for e in c] == list(range(130))            # admission order kept
    assert all(e[1:] == ((690, 2) if e[0] % 2 else (0, 100)) for c in calls for e in c)


class _FakeNet:
    """what the pools read of a HipNet before any launch (the session buffer lives on the CPU here)"""

    def __init__(self, cfg):
        self.cfg, self.device = cfg, torch.device("cpu")
        self.dlist = ops.desc_list(cfg)


def test_stepped_pool_slots_are_claimed_and_reused_after_close():
    cfg = C.ref6_laplace()
    pool = SteppedDecodePool(_FakeNet(cfg), 3, rng_seed=5)
    d = _lib.desc_from_cfg(cfg)
    assert pool._session.numel() == (_lib.lib().swn_decode_session_floats(ctypes.byref(d), 3, 3)
                                     + _lib.DECODE_STEPPED_POOL_TABLE_FLOATS)
    assert pool.n_pro == 690 and pool.variant == 3
    a, b, c = pool.open(), pool.open(), pool.open(utt_id=42)
    assert (a.slot, b.slot, c.slot) == (0, 1, 2)
    assert (a.utt_id, b.utt_id, c.utt_id) == (0, 1, 42)
    with pytest.raises(RuntimeError, match="full"):
        pool.open()
    pool.close(b)
    e = pool.open()
    assert e.slot == 1 and e.utt_id == 3 and e._it_done == 0
    assert e.steps_done == 0 and e.steps_ready == 0
    with pytest.raises(RuntimeError, match="closed"):
        b.push(torch.zeros(1, cfg.n_aux, 2))
    with pytest.raises(RuntimeError):
        pool.close(b)
    assert pool.step() == {} and pool.step(max_prologue=5) == {}           # no features yet: no call
    assert [s.slot for s in pool.sessions] == [0, 2, 1]


def test_stepped_pool_argument_checks_and_the_plain_pool_unchanged():
    net = _FakeNet(C.ref6_laplace())
    for cap in (0, -1, 1.5, None):
        with pytest.raises(ValueError):
            SteppedDecodePool(net, cap)
    SteppedDecodePool(_FakeNet(C.tiny("laplace", 2, 4)), 2)             # every net variant 3 runs, tiny ones included
    SteppedDecodePool(_FakeNet(C.ref6_softmax()), 2)
    with pytest.raises(ValueError, match="stepped"):
        DecodePool(net, 2, variant=0)                                    # DecodePool still refuses stepped nets
