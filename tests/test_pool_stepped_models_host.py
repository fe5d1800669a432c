"""CPU: the stepped decode pool over several models (swn_decode_pool_stepped_chunk_models / SteppedModelPool): the C ABI's
argument checks, the grouping of a tick's table by model (swn_decode_stepped_pool_plan, the function the launch code uses),
the op schema, the pool's model bookkeeping and the routing of open_pool - everything that runs before a device is touched."""
import ctypes
import re

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops
from shallow_wavenet_amd.streaming import DecodePool, SteppedDecodePool, SteppedModelPool

BADARG, UNSUPPORTED = -2, -4                   # SWN_E_BADARG, SWN_E_UNSUPPORTED (include/swn_hip.h)
N_PRO = 690                                    # prologue iterations of C.ref6_laplace()


def test_symbols_op_and_the_table_size():
    lib = _lib.lib()
    for name in ("swn_decode_pool_stepped_chunk_models", "swn_decode_stepped_pool_plan"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.swn_abi_version() == 3
    assert _lib.DECODE_STEPPED_POOL_TABLE_FLOATS == 512                  # the single-model call keeps its table
    assert _lib.DECODE_STEPPED_POOL_MODELS_TABLE_FLOATS * 4 >= 64 * 40   # 40-byte rows: the entry and its model's pointer
    assert _lib.DECODE_STEPPED_POOL_MAX_TILES == 23
    assert "decode_pool_stepped_chunk_models" in ops.OP_NAMES
    schema = str(torch.ops.swn.decode_pool_stepped_chunk_models.default._schema)
    assert schema.startswith("swn::decode_pool_stepped_chunk_models(Tensor[] models, SymInt[] model_of, ")
    assert re.search(r"Tensor\(a\d*!\) session", schema)
    # the argument list of decode_pool_stepped_chunk with `packed` replaced by (models, model_of)
    names = lambda s: re.findall(r"(\w+)(?:=[^,)]*)?[,)]", s[s.index("("):s.index("->")])
    single = names(str(torch.ops.swn.decode_pool_stepped_chunk.default._schema))
    assert names(schema) == ["models", "model_of"] + single[1:] and single[0] == "packed"
    d = _lib.desc_from_cfg(C.ref6_laplace())
    assert ops.stepped_pool_models_session_floats(d, 4) == ops.stepped_pool_session_floats(d, 4) + 128


def _ptrs(vals):
    return (ctypes.c_void_p * max(1, len(vals)))(*[v or None for v in vals])


def _idx(vals):
    return (ctypes.c_int32 * max(1, len(vals)))(*vals)


def _io(noise=0, forced=0):
    return _lib.DecodeIO(noise_dev=noise or None, forced_dev=forced or None, seed_dev=None, noise_out_dev=None, rng_seed=1,
                         rng_utt0=0, reserved=0, rng_utt_ids_dev=None)


def _entry(slot=0, it0=0, n_it=4, flags=1, frames=4, cond=1, reserved=0):
    return _lib.DecodeSteppedPoolEntry(cond_dev=cond or None, n_frames=frames, slot=slot, it0=it0, n_it=n_it, flags=flags,
                                       reserved=reserved)


def _call(d, entries, models=(1, 2), of=None, n_models=None, capacity=4, io=None, session=1, out=1, n_entries=None,
          table=True, null_models=False, null_of=False, null_io=False):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    of = [e % len(models) for e in range(len(entries))] if of is None else of
    arr = (_lib.DecodeSteppedPoolEntry * max(1, len(entries)))(*entries)
    return lib.swn_decode_pool_stepped_chunk_models(
        ctypes.byref(d), None if null_models else _ptrs(models), len(models) if n_models is None else n_models,
        None if null_of else _idx(of), capacity, arr if table else None, len(entries) if n_entries is None else n_entries,
        None if null_io else ctypes.byref(io if io is not None else _io()), p(session), p(out), None, None)


def _ok():
    return [_entry(0, n_it=100), _entry(1, it0=N_PRO + 8, n_it=2, flags=0, frames=8)]


def test_models_call_rejects_bad_model_arguments_before_any_launch():
    """fake non-null addresses are fine: every one of these is refused before the library touches them"""
    d = _lib.desc_from_cfg(C.ref6_laplace())
    ok = _ok()
    assert _call(d, ok, n_models=0) == BADARG                            # n_models outside [1, 16]
    assert _call(d, ok, n_models=-1) == BADARG
    assert _call(d, ok, models=list(range(1, 18)), of=[0, 16]) == BADARG
    assert _call(d, ok, null_models=True) == BADARG                      # a null array
    assert _call(d, ok, null_of=True) == BADARG
    assert _call(d, ok, models=(1, 0)) == BADARG                         # a null model pointer, named ...
    assert _call(d, ok, models=(1, 0, 3), of=[0, 2]) == BADARG           # ... or not
    assert _call(d, ok, of=[0, 2]) == BADARG                             # an index outside [0, n_models)
    assert _call(d, ok, of=[-1, 0]) == BADARG


def test_models_call_keeps_the_rules_of_the_single_model_call():
    d = _lib.desc_from_cfg(C.ref6_laplace())
    U = C.ref6_laplace().U
    ok = _ok()
    assert _call(d, ok, session=0) == BADARG                             # null pointers
    assert _call(d, [_entry(0, it0=N_PRO, n_it=2, flags=0)], out=0) == BADARG   # generation steps need out
    assert _call(d, ok, table=False) == BADARG
    assert _call(d, ok, null_io=True) == BADARG
    assert _call(d, [_entry(cond=0)]) == BADARG
    assert _call(d, ok, n_entries=0) == BADARG                           # entry count outside [1, 64]
    assert _call(d, [_entry(i, n_it=0, flags=0, it0=5) for i in range(65)], capacity=65, n_entries=65) == BADARG
    assert _call(d, ok, capacity=0) == BADARG
    assert _call(d, [_entry(4)]) == BADARG                               # slot outside [0, capacity)
    assert _call(d, [_entry(-1)]) == BADARG
    assert _call(d, [_entry(2), _entry(2, it0=4, flags=0)]) == BADARG    # one slot in two entries
    assert _call(d, [_entry(0, it0=1, flags=1)]) == BADARG               # BEGIN must start at iteration 0
    assert _call(d, [_entry(0, it0=0, n_it=3, flags=0)]) == BADARG       # iteration 0 without BEGIN
    assert _call(d, [_entry(0, it0=-1, flags=0)]) == BADARG
    assert _call(d, [_entry(0, it0=5, n_it=-1, flags=0)]) == BADARG
    # the last generation step past the final conditioning: (step + 1) * seg <= n_frames * U
    assert _call(d, [_entry(0, it0=N_PRO, n_it=4 * U + 1, flags=0, frames=4)]) == BADARG
    assert _call(d, [_entry(0, n_it=N_PRO + 4 * U + 1, frames=4)]) == BADARG
    assert _call(d, [_entry(0, flags=2)]) == BADARG                      # unknown flag
    assert _call(d, [_entry(0, reserved=1)]) == BADARG
    assert _call(d, ok, io=_io(noise=1)) == BADARG                       # pools draw their noise on the device
    assert _call(d, ok, io=_io(forced=1)) == BADARG                      # ... and take no teacher forcing
    bad = _lib.desc_from_cfg(C.ref6_laplace())
    bad.kernel_size = 1
    assert _call(bad, ok) == -1                                          # the descriptor is checked first


def test_models_call_unsupported_and_idle_calls_launch_nothing():
    d = _lib.desc_from_cfg(C.ref6_laplace())
    per_slot = _lib.lib().swn_decode_session_floats(ctypes.byref(d), 1, 3)
    big = (1 << 31) // (4 * per_slot) + 1                                # the state passes the 2 GiB buffer-offset limit
    assert _call(d, [_entry(0)], capacity=big) == UNSUPPORTED
    # entries of 0 iterations without BEGIN leave their slots as they are: nothing to launch, so fake addresses are fine;
    # a model that no entry names is allowed
    idle = [_entry(0, it0=5, n_it=0, flags=0), _entry(3, it0=700, n_it=0, flags=0)]
    assert _call(d, idle, models=(1, 2, 3), of=[2, 0], out=0) == 0
    assert _call(d, idle, models=list(range(1, 17)), of=[15, 0], out=0) == 0
    # the BL6 pool call keeps refusing nets of the stepped chain
    e = (_lib.DecodePoolEntry * 1)(_lib.DecodePoolEntry(cond_dev=1, n_frames=4, slot=0, step0=0, n_steps=4, flags=1,
                                                        reserved=0))
    assert _lib.lib().swn_decode_pool_chunk_models(ctypes.byref(d), _ptrs([1, 2]), 2, _idx([0]), 4, e, 1,
                                                   ctypes.byref(_io()), ctypes.c_void_p(1), ctypes.c_void_p(1), None, 0,
                                                   None) == UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------ the grouping
def _plan_raw(of, n_it, n_models, j, n_entries=None, null=None):
    E = len(of) if n_entries is None else n_entries
    order, tiles = _idx([0] * 64), _idx([0] * (3 * _lib.DECODE_STEPPED_POOL_MAX_TILES))
    args = [_idx(of), _idx(n_it), E, n_models, j, order, tiles]
    if null is not None:
        args[null] = None
    return _lib.lib().swn_decode_stepped_pool_plan(*args)


def test_plan_rejects_bad_arguments():
    assert _plan_raw([0, 1], [3, 4], 2, 0) == 2
    for null in (0, 1, 5, 6):
        assert _plan_raw([0, 1], [3, 4], 2, 0, null=null) == BADARG
    assert _plan_raw([0, 1], [3, 4], 2, 0, n_entries=0) == BADARG
    assert _plan_raw([0] * 65, [1] * 65, 1, 0) == BADARG
    assert _plan_raw([0, 1], [3, 4], 0, 0) == BADARG
    assert _plan_raw([0, 1], [3, 4], 17, 0) == BADARG
    assert _plan_raw([0, 2], [3, 4], 2, 0) == BADARG
    assert _plan_raw([-1, 0], [3, 4], 2, 0) == BADARG
    assert _plan_raw([0, 1], [3, -1], 2, 0) == BADARG
    assert _plan_raw([0, 1], [3, 4], 2, -1) == BADARG
    with pytest.raises(RuntimeError):
        ops.stepped_pool_plan([0, 2], [3, 4], 2)


def _check_plan(of, n_it, n_models, j):
    E = len(of)
    order, tiles = ops.stepped_pool_plan(of, n_it, n_models, j)
    assert sorted(order) == list(range(E))                               # a permutation
    # (model, n_it descending), stable
    assert order == sorted(range(E), key=lambda e: (of[e], -n_it[e]))
    covered = []
    for first, rows, model in tiles:
        assert 1 <= rows <= 8 and 0 <= first and first + rows <= E
        ents = order[first:first + rows]
        assert all(of[e] == model for e in ents)                         # one model per tile
        covered += ents
    active = [e for e in range(E) if n_it[e] > j]
    assert sorted(covered) == active                                     # exactly the active entries, each once
    assert [t[0] for t in tiles] == sorted(t[0] for t in tiles)          # in table order
    want = sum(-(-sum(1 for e in active if of[e] == m) // 8) for m in range(n_models))
    assert len(tiles) == want <= _lib.DECODE_STEPPED_POOL_MAX_TILES
    return order, tiles


def test_plan_properties_over_random_tables():
    rng = np.random.default_rng(7)
    for _ in range(400):
        E, M = int(rng.integers(1, 65)), int(rng.integers(1, 17))
        of = [int(m) for m in rng.integers(0, M, E)]
        n_it = [int(n) for n in rng.integers(0, 51, E)]
        order, _ = _check_plan(of, n_it, M, int(rng.integers(0, 51)))
        if M == 1:                                                       # the single-model call's order
            assert order == sorted(range(E), key=lambda e: -n_it[e])
    for E in (1, 8, 9, 24, 64):                                          # one model
        n_it = [int(n) for n in rng.integers(0, 51, E)]
        order, _ = _check_plan([0] * E, n_it, 1, 3)
        assert order == sorted(range(E), key=lambda e: -n_it[e])


def test_plan_fixed_cases():
    _, tiles = _check_plan([e % 16 for e in range(64)], [5] * 64, 16, 0)
    assert tiles == [(4 * m, 4, m) for m in range(16)]                   # 64 entries over 16 models: 16 tiles of 4
    _, tiles = _check_plan([0] * 9, [3] * 9, 1, 2)
    assert tiles == [(0, 8, 0), (8, 1, 0)]
    assert _check_plan([0, 1, 1, 2] * 5, list(range(20)), 3, 20)[1] == []   # j past every n_it
    assert _check_plan([0, 1, 1, 2] * 5, [50] * 20, 3, 50)[1] == []
    # the worst case of 64 entries over 16 models: one model of 49 and fifteen of 1
    _, tiles = _check_plan([0] * 49 + list(range(1, 16)), [2] * 64, 16, 1)
    assert len(tiles) == 7 + 15
    # entries that ran out leave their model's prefix: model 1 keeps 2 of 3 rows at j = 4
    order, tiles = _check_plan([1, 0, 1, 1], [4, 9, 7, 5], 2, 4)
    assert order == [1, 2, 3, 0] and tiles == [(0, 1, 0), (1, 2, 1)]


# ------------------------------------------------------------------------------------------------------------------- pool
class _FakeNet:
    """what a pool reads of a HipNet before any launch (the session buffer lives on the CPU here)"""

    def __init__(self, cfg, device="cpu"):
        self.cfg, self.device = cfg, torch.device(device)
        self.dlist = ops.desc_list(cfg)


def test_stepped_model_pool_takes_nets_of_its_geometry_only():
    cfg = C.ref6_laplace()
    pool = SteppedModelPool(_FakeNet(cfg), 4, rng_seed=5)
    assert isinstance(pool, SteppedDecodePool) and pool.resolved_variant == 3
    assert pool._session.numel() == ops.stepped_pool_models_session_floats(_lib.desc_from_cfg(cfg), 4)
    s0 = pool.open()
    assert s0.model == 0 and s0._it_done == 0                            # the pool's own net is model 0
    with pytest.raises(ValueError, match="NetConfig"):
        pool.add_model(_FakeNet(C.ref6_laplace(5, 4)))
    with pytest.raises(ValueError, match="NetConfig"):
        pool.add_model(_FakeNet(C.ref6_softmax()))
    with pytest.raises(ValueError, match="meta"):
        pool.add_model(_FakeNet(cfg, "meta"))                            # another device
    other = _FakeNet(C.ref6_laplace())
    assert pool.add_model(other) == 1 and pool.add_model(_FakeNet(cfg)) == 2
    s = pool.open(model=1)
    assert s.model == 1 and s._stream.net is other and s.slot == 1 and s._it_done == 0
    for bad in (3, -1, None, 1.0):
        with pytest.raises(ValueError, match="model"):
            pool.open(model=bad)
    assert len(pool.sessions) == 2                                       # a refused open claims no slot
    assert pool.step() == {} and pool.step(3, max_prologue=100) == {}    # no features yet: nothing to run, no launch
    pool.close(s)
    assert pool.open(model=2).slot == 1                                  # the slot passes to another model


def test_stepped_decode_pool_still_serves_one_model():
    cfg = C.ref6_laplace()
    pool = SteppedDecodePool(_FakeNet(cfg), 2)
    with pytest.raises(ValueError, match="weight rows once for eight sessions") as e:
        pool.add_model(_FakeNet(cfg))
    assert "SteppedModelPool" in str(e.value)
    assert pool._session.numel() == ops.stepped_pool_session_floats(_lib.desc_from_cfg(cfg), 2)


def test_open_pool_multi_model_routes_by_the_resolved_variant():
    from shallow_wavenet_amd.nets import cswnv_shift1 as mc

    def pool_of(cfg, **kw):
        m = mc.CSWNV(**cfg.ctor_kwargs())
        m._engine = lambda: _FakeNet(cfg)                                # the module's parameters are on the CPU here
        return m.open_pool(4, **kw)

    p = pool_of(C.ref6_laplace(), multi_model=True)
    assert type(p) is SteppedModelPool
    assert type(pool_of(C.ref6_laplace())) is SteppedDecodePool          # the default changes nothing
    assert type(pool_of(C.bl6_laplace(), multi_model=True)) is DecodePool
    assert type(pool_of(C.bl6_laplace())) is DecodePool
