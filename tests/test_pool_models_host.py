"""CPU: the multi-model pool entry points of the C ABI (swn_decode_pool_chunk_models, swn_frontend_pool_models and its work
query), the op schemas, the call splitter and DecodePool.add_model - everything that runs before a device is touched."""
import ctypes
import re

import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops
from shallow_wavenet_amd.streaming import DecodePool, SteppedDecodePool, plan_push, plan_tick, split_models

BADARG, UNSUPPORTED = -2, -4                   # SWN_E_BADARG, SWN_E_UNSUPPORTED (include/swn_hip.h)


def test_symbols_ops_and_the_cap():
    lib = _lib.lib()
    for name in ("swn_decode_pool_chunk_models", "swn_frontend_pool_models", "swn_frontend_pool_models_work_floats"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.POOL_MAX_MODELS == 16 and lib.swn_abi_version() == 3
    assert "decode_pool_chunk_models" in ops.OP_NAMES and "frontend_pool_models" in ops.OP_NAMES
    schema = str(torch.ops.swn.decode_pool_chunk_models.default._schema)
    assert schema.startswith("swn::decode_pool_chunk_models(Tensor[] models, SymInt[] model_of, ")
    assert re.search(r"Tensor\(a\d*!\) session", schema)
    schema = str(torch.ops.swn.frontend_pool_models.default._schema)
    assert schema.startswith("swn::frontend_pool_models(Tensor[] models, SymInt[] model_of, ")
    assert re.search(r"Tensor\(a\d*!\)\[\] auxs", schema) and re.search(r"Tensor\(a\d*!\)\[\] conds", schema)


def _ptrs(vals):
    return (ctypes.c_void_p * max(1, len(vals)))(*[v or None for v in vals])


def _idx(vals):
    return (ctypes.c_int32 * max(1, len(vals)))(*vals)


# ---------------------------------------------------------------------------------------------------------------- decode
def _entry(slot=0, step0=0, n_steps=4, flags=1, frames=4, cond=1, reserved=0):
    return _lib.DecodePoolEntry(cond_dev=cond or None, n_frames=frames, slot=slot, step0=step0, n_steps=n_steps, flags=flags,
                                reserved=reserved)


def _decode(d, entries, models=(1, 2), of=None, n_models=None, capacity=4, session=1, out=1, variant=0, null_models=False,
            null_of=False):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    of = [e % len(models) for e in range(len(entries))] if of is None else of
    io = _lib.DecodeIO(noise_dev=None, forced_dev=None, seed_dev=None, noise_out_dev=None, rng_seed=1, rng_utt0=0, reserved=0,
                       rng_utt_ids_dev=None)
    return lib.swn_decode_pool_chunk_models(
        ctypes.byref(d), None if null_models else _ptrs(models), len(models) if n_models is None else n_models,
        None if null_of else _idx(of), capacity, (_lib.DecodePoolEntry * len(entries))(*entries), len(entries), ctypes.byref(io),
        p(session), p(out), None, variant, None)


def test_decode_models_rejects_bad_model_arguments_before_any_launch():
    """fake non-null addresses are fine: every one of these is refused before the library touches them"""
    d = _lib.desc_from_cfg(C.bl6_laplace())
    ok = [_entry(0), _entry(1, step0=8, n_steps=2, flags=0, frames=8)]
    assert _decode(d, ok, n_models=0) == BADARG                          # n_models outside [1, 16]
    assert _decode(d, ok, n_models=-1) == BADARG
    assert _decode(d, ok, models=list(range(1, 18)), of=[0, 16]) == BADARG
    assert _decode(d, ok, null_models=True) == BADARG                    # a null array
    assert _decode(d, ok, null_of=True) == BADARG
    assert _decode(d, ok, models=(1, 0)) == BADARG                       # a null model pointer, named ...
    assert _decode(d, ok, models=(1, 0, 3), of=[0, 2]) == BADARG         # ... or not
    assert _decode(d, ok, of=[0, 2]) == BADARG                           # an index outside [0, n_models)
    assert _decode(d, ok, of=[-1, 0]) == BADARG
    # the rules of swn_decode_pool_chunk still hold
    assert _decode(d, ok, session=0) == BADARG
    assert _decode(d, ok, out=0) == BADARG
    assert _decode(d, [_entry(2), _entry(2, step0=4, flags=0, frames=8)]) == BADARG
    assert _decode(d, [_entry(4)]) == BADARG
    assert _decode(d, ok, variant=4) == BADARG
    ref6 = _lib.desc_from_cfg(C.ref6_laplace())
    assert _decode(ref6, [_entry(0)], variant=0) == UNSUPPORTED          # the stepped chain
    assert _decode(ref6, [_entry(0)], variant=3) == UNSUPPORTED


def test_decode_models_of_idle_entries_launches_nothing():
    """a model that no entry names is allowed; entries of 0 steps without BEGIN have nothing to launch"""
    d = _lib.desc_from_cfg(C.bl6_laplace())
    idle = [_entry(0, step0=5, n_steps=0, flags=0), _entry(3, n_steps=0, flags=0)]
    assert _decode(d, idle, models=(1, 2, 3), of=[2, 0], out=0) == 0
    assert _decode(d, idle, models=list(range(1, 17)), of=[15, 0], out=0) == 0


# -------------------------------------------------------------------------------------------------------------- front end
def _fe(aux=1, new=0, cond=16, stride=64, n_received=8, n_new=0, f0=0, f1=0, flags=0):
    return _lib.FrontendPoolEntry(aux_dev=aux or None, new_dev=new or None, cond_dev=cond or None, aux_stride=stride,
                                  n_received=n_received, n_new=n_new, f0=f0, f1=f1, flags=flags)


def _frontend(d, entries, models=(1, 2), of=None, n_models=None, work=1, null_models=False, null_of=False):
    """-> (work floats, return code of the call)"""
    lib = _lib.lib()
    of = [e % len(models) for e in range(len(entries))] if of is None else of
    n_models = len(models) if n_models is None else n_models
    table = (_lib.FrontendPoolEntry * len(entries))(*entries)
    ofp = None if null_of else _idx(of)
    floats = lib.swn_frontend_pool_models_work_floats(ctypes.byref(d), table, ofp, len(entries), n_models)
    rc = lib.swn_frontend_pool_models(ctypes.byref(d), None if null_models else _ptrs(models), n_models, ofp, table,
                                      len(entries), ctypes.c_void_p(work) if work else None, None)
    return floats, rc


def test_frontend_models_rejects_bad_model_arguments_before_any_launch():
    d = _lib.desc_from_cfg(C.bl6_laplace())
    # entries that only stand in the table (no new frames, nothing to finalise): an accepted call launches nothing
    ok = [_fe(cond=16), _fe(cond=32)]
    assert _frontend(d, ok, n_models=0) == (0, BADARG)
    assert _frontend(d, ok, models=list(range(1, 18)), of=[0, 16]) == (0, BADARG)
    assert _frontend(d, ok, null_of=True) == (0, BADARG)
    assert _frontend(d, ok, of=[0, 2]) == (0, BADARG)
    assert _frontend(d, ok, of=[-1, 0]) == (0, BADARG)
    assert _frontend(d, ok, null_models=True)[1] == BADARG               # (the query takes no model array)
    assert _frontend(d, ok, models=(1, 0))[1] == BADARG
    assert _frontend(d, ok, models=(1, 0, 3), of=[0, 2])[1] == BADARG
    # the rules of swn_frontend_pool still hold
    assert _frontend(d, [_fe(cond=16), _fe(cond=16)]) == (0, BADARG)     # one cond buffer in two entries
    assert _frontend(d, [_fe(f0=0, f1=8)]) == (0, BADARG)                # not FINAL: the lookahead is not final yet
    assert _frontend(d, [_fe(cond=8)]) == (0, BADARG)                    # rows are stored in 16-byte pieces
    assert _frontend(d, ok, work=0)[1] == BADARG
    floats, rc = _frontend(d, ok, models=(1, 2, 3), of=[2, 0])           # a model that no entry names is allowed
    assert floats > 0 and rc == 0


def test_frontend_models_work_floats_include_the_alignment_padding():
    """every model's columns start at a multiple of 64 in every stage: two models of 2 and 3 kept frames need 64 + 3 columns
    in the last stage where one model needs 5"""
    cfg = C.bl6_laplace()
    d = _lib.desc_from_cfg(cfg)
    lib = _lib.lib()
    fin = _lib.FRONTEND_FINAL
    en = [_fe(cond=16, n_received=2, f1=2, flags=fin), _fe(cond=32, n_received=3, f1=3, flags=fin)]
    table = (_lib.FrontendPoolEntry * 2)(*en)
    one = lib.swn_frontend_pool_work_floats(ctypes.byref(d), table, 2)
    per_col = cfg.n_aux * sum(cfg.aux_kernel_size ** i for i in range(cfg.aux_dilation_size + 1))
    assert one == 1024 + 5 * per_col                                     # FINAL: every stage holds the kept frames only
    same = lib.swn_frontend_pool_models_work_floats(ctypes.byref(d), table, _idx([0, 0]), 2, 1)
    two = lib.swn_frontend_pool_models_work_floats(ctypes.byref(d), table, _idx([0, 1]), 2, 2)
    swapped = lib.swn_frontend_pool_models_work_floats(ctypes.byref(d), table, _idx([1, 0]), 2, 2)
    assert same == 2048 + 5 * per_col
    assert two == 2048 + (64 + 3) * per_col
    assert swapped == 2048 + (64 + 2) * per_col                          # model order, not entry order


# --------------------------------------------------------------------------------------------------------------- splitter
def test_split_models_caps_the_models_of_a_call_and_keeps_the_order():
    model = {i: i % 17 for i in range(20)}                               # 20 entries over 17 models
    calls = plan_tick([(i, 5, 0) for i in range(20)])
    assert len(calls) == 1
    cut = split_models(calls, model.get)
    assert len(cut) >= 2
    assert all(len({model[e[0]] for e in c}) <= 16 for c in cut)
    assert [e for c in cut for e in c] == calls[0]                        # same entries, same order
    assert [len(c) for c in cut] == [16, 4]                              # greedy: cut where the 17th model would enter
    # a lower limit, entries of plan_push
    pushes = plan_push([(i, 0, 0, 3, False) for i in range(7)], lookahead=1)
    cut = split_models(pushes, lambda i: "ab"[i % 2] if i < 4 else "c", limit=2)
    assert [[e[0] for e in c] for c in cut] == [[0, 1, 2, 3], [4, 5, 6]]
    with pytest.raises(ValueError):
        split_models(calls, model.get, limit=0)


def test_split_models_returns_calls_within_the_cap_unchanged():
    calls = plan_tick([(i, 5, 0) for i in range(130)], max_steps=2)
    assert [len(c) for c in calls] == [64, 64, 2]
    one = split_models(calls, lambda k: 0)
    assert one == calls and all(a is b for a, b in zip(one, calls))
    sixteen = split_models(calls, lambda k: k % 16)
    assert sixteen == calls
    assert split_models([], lambda k: 0) == []


# ------------------------------------------------------------------------------------------------------------------- pool
class _FakeNet:
    """what DecodePool reads of a HipNet before any launch (the session buffer lives on the CPU here)"""

    def __init__(self, cfg, device="cpu"):
        self.cfg, self.device = cfg, torch.device(device)
        self.dlist = ops.desc_list(cfg)


def test_add_model_takes_nets_of_the_pools_geometry_only():
    cfg = C.bl6_laplace()
    pool = DecodePool(_FakeNet(cfg), 4, rng_seed=5)
    assert pool.open().model == 0                                        # the pool's own net is model 0
    with pytest.raises(ValueError, match="NetConfig"):
        pool.add_model(_FakeNet(C.bl6_laplace(1, 4)))
    with pytest.raises(ValueError, match="NetConfig"):
        pool.add_model(_FakeNet(C.bl6_softmax()))
    with pytest.raises(ValueError, match="meta"):
        pool.add_model(_FakeNet(cfg, "meta"))                            # another device
    other = _FakeNet(C.bl6_laplace())
    assert pool.add_model(other) == 1 and pool.add_model(_FakeNet(cfg)) == 2
    s = pool.open(model=1)
    assert s.model == 1 and s._stream.net is other and s.slot == 1
    for bad in (3, -1, None, 1.0):
        with pytest.raises(ValueError, match="model"):
            pool.open(model=bad)
    assert len(pool.sessions) == 2                                       # a refused open claims no slot
    assert pool.step() == {}                                             # no features yet: nothing to run, no launch


def test_stepped_pool_serves_one_model():
    cfg = C.ref6_laplace()
    pool = SteppedDecodePool(_FakeNet(cfg), 2)
    with pytest.raises(ValueError, match="weight rows once for eight sessions"):
        pool.add_model(_FakeNet(cfg))
    assert pool.open().model == 0
