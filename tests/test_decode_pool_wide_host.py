"""CPU: the wide decode pool launch (swn_decode_pool_chunk_wide: up to 256 entries, the table in device memory) - its symbols
and constants, the argument rules of the C ABI (all checked before anything is launched, so fake non-null addresses do), the
op's schema and fake, plan_tick at the wide limit, and the launch_width keyword of the pools."""
import ctypes
import os
import re

import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops
from shallow_wavenet_amd.streaming import DecodeModelPool, DecodePool, SteppedDecodePool, SteppedModelPool, plan_tick

BADARG, UNSUPPORTED = -2, -4                   # SWN_E_BADARG, SWN_E_UNSUPPORTED (include/swn_hip.h)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swn_hip.h")


def _define(name):
    with open(HEADER) as f:
        m = re.search(rf"^#define {name}\s+(\d+)", f.read(), re.M)
    assert m, name
    return int(m.group(1))


def test_symbols_constants_and_the_op():
    lib = _lib.lib()
    for name in ("swn_decode_pool_chunk_wide", "swn_decode_pool_wide_table_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.DECODE_POOL_WIDE_MAX_ENTRIES == _define("SWN_DECODE_POOL_WIDE_MAX_ENTRIES") == 256
    assert _lib.DECODE_POOL_MAX_ENTRIES == _define("SWN_DECODE_POOL_MAX_ENTRIES") == 64     # the narrow calls keep theirs
    assert (_lib.WEIGHTS_FP32, _lib.WEIGHTS_BF16, _lib.WEIGHTS_E4M3) == tuple(
        _define(f"SWN_WEIGHTS_{w}") for w in ("FP32", "BF16", "E4M3"))
    assert lib.swn_abi_version() == 3                                    # symbols were added, none changed
    assert "decode_pool_chunk_wide" in ops.OP_NAMES
    schema = str(torch.ops.swn.decode_pool_chunk_wide.default._schema)
    assert schema.startswith("swn::decode_pool_chunk_wide(Tensor[] models, Tensor[] images, str weights, SymInt[] model_of, ")
    assert re.search(r"Tensor\(a\d*!\) session", schema)


def test_table_bytes():
    lib = _lib.lib()
    assert lib.swn_decode_pool_wide_table_bytes(0) == 0 and lib.swn_decode_pool_wide_table_bytes(257) == 0
    assert lib.swn_decode_pool_wide_table_bytes(-1) == 0
    one = lib.swn_decode_pool_wide_table_bytes(1)
    assert one >= ctypes.sizeof(_lib.DecodePoolEntry) + 2 * ctypes.sizeof(ctypes.c_void_p)   # entry, model, image
    assert [lib.swn_decode_pool_wide_table_bytes(n) for n in (64, 65, 256)] == [64 * one, 65 * one, 256 * one]


def _ptrs(vals):
    return (ctypes.c_void_p * max(1, len(vals)))(*[v or None for v in vals])


def _entry(slot=0, step0=0, n_steps=4, flags=1, frames=4, cond=1, reserved=0):
    return _lib.DecodePoolEntry(cond_dev=cond or None, n_frames=frames, slot=slot, step0=step0, n_steps=n_steps, flags=flags,
                                reserved=reserved)


def _wide(d, entries, models=(16,), of=None, n_models=None, capacity=256, session=16, out=16, variant=0, images=None, fmt=0,
          table=16, n_entries=None):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    E = len(entries)
    of = [e % len(models) for e in range(E)] if of is None else of
    io = _lib.DecodeIO(noise_dev=None, forced_dev=None, seed_dev=None, noise_out_dev=None, rng_seed=1, rng_utt0=0, reserved=0,
                       rng_utt_ids_dev=None)
    return lib.swn_decode_pool_chunk_wide(
        ctypes.byref(d), _ptrs(models), len(models) if n_models is None else n_models,
        (ctypes.c_int32 * max(1, E))(*of), capacity, (_lib.DecodePoolEntry * max(1, E))(*entries),
        E if n_entries is None else n_entries, ctypes.byref(io), p(session), p(out), None, variant,
        None if images is None else _ptrs(images), fmt, p(table), None)


def _entries(n):
    return [_entry(slot=e) for e in range(n)]


def test_wide_call_rejects_bad_arguments_before_any_launch():
    """fake non-null addresses are fine: every one of these is refused before the library touches them"""
    d = _lib.desc_from_cfg(C.bl6_laplace())
    assert _wide(d, [], n_entries=0) == BADARG                           # n_entries outside [1, 256]
    assert _wide(d, _entries(257), capacity=300) == BADARG
    assert _wide(d, _entries(256), table=0) == BADARG                    # a null table buffer
    assert _wide(d, _entries(65), table=0) == BADARG
    assert _wide(d, _entries(65), table=24) == BADARG                    # ... or one that is not 16-byte aligned
    assert _wide(d, _entries(65), table=4) == BADARG
    dup = _entries(256)
    dup[200] = _entry(slot=dup[3].slot)                                  # one slot at entries 3 and 200: across a 64 boundary
    assert _wide(d, dup) == BADARG
    dup = _entries(256)
    dup[255] = _entry(slot=0)
    assert _wide(d, dup) == BADARG
    # the rules of swn_decode_pool_chunk and of the model tables
    ok = _entries(70)
    assert _wide(d, ok, session=0) == BADARG
    assert _wide(d, ok, out=0) == BADARG
    assert _wide(d, ok, capacity=69) == BADARG                           # slot 69 outside [0, capacity)
    assert _wide(d, ok[:69] + [_entry(slot=69, step0=1)]) == BADARG      # BEGIN with step0 != 0
    assert _wide(d, ok[:69] + [_entry(slot=69, reserved=1)]) == BADARG
    assert _wide(d, ok, n_models=0) == BADARG
    assert _wide(d, ok, models=(16, 0)) == BADARG                        # a null model pointer
    assert _wide(d, ok, of=[0] * 69 + [1]) == BADARG                     # an index outside [0, n_models)
    assert _wide(d, ok, models=[16] * 257, of=[0] * 70) == BADARG        # n_models outside [1, 256]
    assert _wide(d, ok, fmt=3) == BADARG                                 # an unknown weight format
    assert _wide(d, ok, fmt=-1) == BADARG
    assert _wide(d, ok, variant=4) == BADARG
    # a stored format wants one image per model
    assert _wide(d, ok, fmt=_lib.WEIGHTS_BF16, variant=6) == BADARG
    assert _wide(d, ok, models=(16, 32), images=(16, 0), fmt=_lib.WEIGHTS_E4M3, variant=6) == BADARG


def test_wide_call_refuses_what_the_narrow_calls_refuse_in_their_words():
    lib = _lib.lib()
    ref6 = _lib.desc_from_cfg(C.ref6_laplace())
    assert _wide(ref6, _entries(2), variant=0) == UNSUPPORTED            # the stepped chain
    assert _wide(ref6, _entries(2), variant=3) == UNSUPPORTED
    d = _lib.desc_from_cfg(C.bl6_laplace())                              # single-sample Laplace: variant 0 is the BL6W kernel
    for fmt, word in ((_lib.WEIGHTS_BF16, "bf16"), (_lib.WEIGHTS_E4M3, "e4m3")):
        assert _wide(d, _entries(70), images=(16,), fmt=fmt, variant=0) == UNSUPPORTED
        detail = lib.swn_last_error_detail().decode()
        assert "swn_decode_pool_chunk_wide" in detail
        assert f"{word} weights run on the symmetric BL6 kernel; this net resolves to the wave-specialised kernel" in detail
        assert "pass variant = 6" in detail
        assert _wide(d, _entries(70), images=(16,), fmt=fmt, variant=1) == UNSUPPORTED
        assert f"{word} weights run on the symmetric BL6 kernel only" in lib.swn_last_error_detail().decode()


def test_wide_call_of_idle_entries_launches_nothing():
    """entries of 0 steps without BEGIN have nothing to launch: accepted, and no setup launch writes the (fake) table; more than
    16 models are fine - the rows carry the pointers"""
    d = _lib.desc_from_cfg(C.bl6_laplace())
    idle = [_entry(slot=e, step0=5, n_steps=0, flags=0, frames=8) for e in range(256)]
    assert _wide(d, idle, out=0) == 0
    assert _wide(d, idle, models=[16 * (m + 1) for m in range(40)], out=0) == 0
    soft = _lib.desc_from_cfg(C.bl6_softmax())
    assert _wide(soft, idle, models=(16, 32), images=(16, 32), fmt=_lib.WEIGHTS_BF16, out=0) == 0


def test_plan_tick_at_the_wide_limit():
    for n, launches in ((1, 1), (64, 1), (65, 1), (256, 1), (257, 2)):
        calls = plan_tick([(i, 5, 0) for i in range(n)], limit=256)
        assert len(calls) == launches, n
        assert [e[0] for c in calls for e in c] == list(range(n))
    assert [len(c) for c in plan_tick([(i, 5, 0) for i in range(257)], limit=256)] == [256, 1]
    assert [len(c) for c in plan_tick([(i, 5, 0) for i in range(257)])] == [64, 64, 64, 64, 1]   # the default stays 64


def test_fake_implementation_gives_the_shapes_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode
    cfg = C.bl6_softmax()
    d = ops.desc_list(cfg)
    E = 200
    with FakeTensorMode():
        packed, session = torch.empty(10), torch.empty(10)
        conds = [torch.empty(4, 8) for _ in range(E)]
        out, heads, used = torch.ops.swn.decode_pool_chunk_wide(
            [packed], [], "fp32", [0] * E, session, conds, list(range(E)), [0] * E, [e % 7 for e in range(E)], [True] * E,
            None, list(range(E)), d, 256, 0, 1, True, True)
    assert tuple(out.shape) == (E, 6) and tuple(heads.shape) == (E, 6, 256) and tuple(used.shape) == (E, 6, 256)


class _FakeNet:
    """what a pool reads of a HipNet before any launch (the session buffer lives on the CPU here)"""

    def __init__(self, cfg, device="cpu"):
        self.cfg, self.device = cfg, torch.device(device)
        self.dlist = ops.desc_list(cfg)


def test_launch_width_of_the_pools():
    cfg = C.bl6_laplace()
    assert DecodePool(_FakeNet(cfg), 4).launch_width == 64               # the default is today's path
    for w in (1, 64, 65, 256):
        assert DecodePool(_FakeNet(cfg), 256, launch_width=w).launch_width == w
    assert DecodeModelPool(_FakeNet(C.bl6_softmax()), 256, weights="bf16", launch_width=256).launch_width == 256
    for bad in (0, 257, -1, None, 64.0, True, "64"):
        with pytest.raises(ValueError, match="launch_width"):
            DecodePool(_FakeNet(cfg), 4, launch_width=bad)
    pool = DecodePool(_FakeNet(cfg), 256, launch_width=256)
    pool.open()
    assert pool.step() == {}                                             # no features yet: nothing to run, no launch


def test_stepped_pools_refuse_a_wide_launch():
    cfg = C.ref6_laplace()
    for cls in (SteppedDecodePool, SteppedModelPool):
        assert cls(_FakeNet(cfg), 2, launch_width=64).launch_width == 64
        assert cls(_FakeNet(cfg), 2, launch_width=8).launch_width == 64      # validated, not a knob of the stepped pools
        for w in (65, 256):
            with pytest.raises(ValueError, match="stepped decode pools take at most 64 sessions per call"):
                cls(_FakeNet(cfg), 2, launch_width=w)
        with pytest.raises(ValueError, match="launch_width"):
            cls(_FakeNet(cfg), 2, launch_width=0)
