"""CPU: the decode-pool entry point of the C ABI (swn_decode_pool_chunk), the op schema, DecodePool's tick planning, slot
bookkeeping and argument checks - everything that runs before a device is touched."""
import ctypes
import re

import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops
from shallow_wavenet_amd.streaming import DecodePool, plan_tick

BADARG, UNSUPPORTED = -2, -4                   # SWN_E_BADARG, SWN_E_UNSUPPORTED (include/swn_hip.h)


def test_pool_symbol_is_exported_and_bound():
    lib = _lib.lib()
    assert hasattr(lib, "swn_decode_pool_chunk") and "swn_decode_pool_chunk" in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.DecodePoolEntry) == 32
    assert _lib.DECODE_POOL_MAX_ENTRIES == 64
    assert "decode_pool_chunk" in ops.OP_NAMES
    schema = str(torch.ops.swn.decode_pool_chunk.default._schema)
    assert schema.startswith("swn::decode_pool_chunk(") and re.search(r"Tensor\(a\d*!\) session", schema)


def _io(noise=0, forced=0):
    return _lib.DecodeIO(noise_dev=noise or None, forced_dev=forced or None, seed_dev=None, noise_out_dev=None, rng_seed=1,
                         rng_utt0=0, reserved=0, rng_utt_ids_dev=None)


def _entry(slot=0, step0=0, n_steps=4, flags=1, frames=4, cond=1, reserved=0):
    return _lib.DecodePoolEntry(cond_dev=cond or None, n_frames=frames, slot=slot, step0=step0, n_steps=n_steps, flags=flags,
                                reserved=reserved)


def _pool(d, entries, capacity=4, io=None, session=1, packed=1, out=1, variant=0, n_entries=None, table=True):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    arr = (_lib.DecodePoolEntry * max(1, len(entries)))(*entries)
    return lib.swn_decode_pool_chunk(ctypes.byref(d), p(packed), capacity, arr if table else None,
                                     len(entries) if n_entries is None else n_entries,
                                     ctypes.byref(io if io is not None else _io()), p(session), p(out), None, variant, None)


def test_pool_chunk_rejects_bad_arguments_before_any_launch():
    """fake non-null addresses are fine: every one of these is refused before the library touches them"""
    d = _lib.desc_from_cfg(C.bl6_laplace())
    ok = [_entry(0), _entry(1, step0=8, n_steps=2, flags=0, frames=8)]
    assert _pool(d, ok, session=0) == BADARG                       # null pointers
    assert _pool(d, ok, packed=0) == BADARG
    assert _pool(d, ok, out=0) == BADARG
    assert _pool(d, ok, table=False) == BADARG
    assert _pool(d, [_entry(cond=0)]) == BADARG
    assert _lib.lib().swn_decode_pool_chunk(ctypes.byref(d), ctypes.c_void_p(1), 4, (_lib.DecodePoolEntry * 1)(_entry()), 1,
                                            None, ctypes.c_void_p(1), ctypes.c_void_p(1), None, 0, None) == BADARG
    assert _pool(d, ok, n_entries=0) == BADARG                     # entry count outside [1, 64]
    assert _pool(d, [_entry(i % 4, n_steps=0, flags=0) for i in range(65)], capacity=65, n_entries=65) == BADARG
    assert _pool(d, ok, capacity=0) == BADARG
    assert _pool(d, [_entry(4)]) == BADARG                         # slot outside [0, capacity)
    assert _pool(d, [_entry(-1)]) == BADARG
    assert _pool(d, [_entry(2), _entry(2, step0=4, flags=0, frames=8)]) == BADARG    # one slot in two entries
    assert _pool(d, [_entry(0, step0=1, flags=1)]) == BADARG       # BEGIN must start at step 0
    assert _pool(d, [_entry(0, step0=-1, flags=0)]) == BADARG
    assert _pool(d, [_entry(0, n_steps=-1, flags=0)]) == BADARG
    assert _pool(d, [_entry(0, n_steps=4 * 110 + 1, frames=4)]) == BADARG   # past the final conditioning (U = 110)
    assert _pool(d, [_entry(0, flags=2)]) == BADARG                # unknown flag
    assert _pool(d, [_entry(0, reserved=1)]) == BADARG
    assert _pool(d, ok, io=_io(noise=1)) == BADARG                 # pools draw their noise on the device
    assert _pool(d, ok, io=_io(forced=1)) == BADARG                # ... and take no teacher forcing
    assert _pool(d, ok, variant=4) == BADARG                       # retired
    assert _pool(_lib.desc_from_cfg(C.tiny("laplace", 2, 4)), [_entry(0, frames=4)], variant=6) == BADARG


def test_pool_refuses_the_stepped_decode():
    d = _lib.desc_from_cfg(C.ref6_laplace())
    e = [_entry(0, n_steps=4, frames=4)]
    assert _lib.lib().swn_decode_resolve_variant(ctypes.byref(d), 4, 0) == 3
    assert _pool(d, e, variant=0) == UNSUPPORTED
    assert _pool(d, e, variant=3) == UNSUPPORTED
    # variant 1 resolves (to the generic kernel): with an argument error the call still stops before any launch
    assert _lib.lib().swn_decode_resolve_variant(ctypes.byref(d), 4, 1) == 1
    assert _pool(d, e + [_entry(0, frames=4)], variant=1) == BADARG


def test_pool_of_idle_entries_launches_nothing():
    """entries of 0 steps without BEGIN leave their slots as they are: nothing to launch, so fake addresses are fine"""
    d = _lib.desc_from_cfg(C.bl6_laplace())
    assert _pool(d, [_entry(0, step0=5, n_steps=0, flags=0), _entry(3, n_steps=0, flags=0)], out=0) == 0


def test_plan_tick_gives_each_session_its_ready_steps():
    s = [("a", 10, 0), ("b", 3, 3), ("c", 200, 63), ("d", 0, 0), ("e", 7, 2)]
    assert plan_tick(s) == [[("a", 0, 10), ("c", 63, 137), ("e", 2, 5)]]
    assert plan_tick(s, max_steps=4) == [[("a", 0, 4), ("c", 63, 4), ("e", 2, 4)]]
    assert plan_tick(s, max_steps=1) == [[("a", 0, 1), ("c", 63, 1), ("e", 2, 1)]]
    assert plan_tick([("x", 0, 0)]) == []
    with pytest.raises(ValueError):
        plan_tick(s, max_steps=0)


def test_plan_tick_splits_launches_at_64_entries():
    s = [(i, 5, 0) for i in range(130)]
    launches = plan_tick(s, max_steps=2)
    assert [len(l) for l in launches] == [64, 64, 2]
    assert [e[0] for l in launches for e in l] == list(range(130))          # admission order kept
    assert all(e[1:] == (0, 2) for l in launches for e in l)
    assert [len(l) for l in plan_tick(s[:64])] == [64]


class _FakeNet:
    """what DecodePool reads of a HipNet before any launch (the session buffer lives on the CPU here)"""

    def __init__(self, cfg):
        self.cfg, self.device = cfg, torch.device("cpu")
        self.dlist = ops.desc_list(cfg)


def test_pool_slots_are_claimed_and_reused_after_close():
    pool = DecodePool(_FakeNet(C.bl6_laplace()), 3, rng_seed=5)
    a, b, c = pool.open(), pool.open(), pool.open(utt_id=42)
    assert (a.slot, b.slot, c.slot) == (0, 1, 2)
    assert (a.utt_id, b.utt_id, c.utt_id) == (0, 1, 42)
    with pytest.raises(RuntimeError, match="full"):
        pool.open()
    pool.close(b)
    d = pool.open()
    assert d.slot == 1 and d.utt_id == 3                                  # the freed slot, the next admission index
    assert d.steps_done == 0 and d.steps_ready == 0
    with pytest.raises(RuntimeError, match="closed"):
        b.push(torch.zeros(1, C.bl6_laplace().n_aux, 2))
    with pytest.raises(RuntimeError, match="closed"):
        b.finish()
    with pytest.raises(RuntimeError):
        pool.close(b)
    assert pool.step() == {}                                             # no features yet: nothing to run, no launch
    assert [s.slot for s in pool.sessions] == [0, 2, 1]


def test_pool_argument_checks():
    net = _FakeNet(C.bl6_laplace())
    for cap in (0, -1, 1.5, None):
        with pytest.raises(ValueError):
            DecodePool(net, cap)
    with pytest.raises(ValueError, match="stepped"):
        DecodePool(_FakeNet(C.ref6_laplace()), 2, variant=0)
    with pytest.raises(ValueError):
        DecodePool(_FakeNet(C.ref6_laplace()), 2, variant=3)
    DecodePool(_FakeNet(C.ref6_laplace()), 2, variant=1)                # the generic kernel serves REF6
    with pytest.raises(ValueError):
        DecodePool(_FakeNet(C.tiny("laplace", 2, 4)), 2, variant=6)       # not a BL6-class net
