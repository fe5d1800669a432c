"""CPU: the pool front end of the C ABI (swn_frontend_pool), its op schema, plan_push and the argument checks of
DecodePool.push_many - everything that runs before a device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops
from shallow_wavenet_amd.streaming import DecodePool, SteppedDecodePool, final_frames, lookahead_frames, plan_push

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -2                                    # SWN_E_BADARG (include/swn_hip.h)
LA = 4                                         # lookahead of the shipped geometry: dilations 1 + 3


def test_symbol_is_exported_and_bound():
    lib = _lib.lib()
    for name in ("swn_frontend_pool", "swn_frontend_pool_work_floats"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "swn_hip.h")).read()
    stated = int(re.search(r"sizeof\(swn_frontend_pool_entry\) == (\d+)", header).group(1))
    assert ctypes.sizeof(_lib.FrontendPoolEntry) == stated
    assert _lib.FRONTEND_POOL_MAX_ENTRIES == 64
    assert int(re.search(r"#define SWN_FRONTEND_POOL_MAX_ENTRIES (\d+)", header).group(1)) == 64
    assert int(re.search(r"#define SWN_FRONTEND_FINAL (\d+)", header).group(1)) == _lib.FRONTEND_FINAL
    assert "frontend_pool" in ops.OP_NAMES
    schema = str(torch.ops.swn.frontend_pool.default._schema)
    assert schema.startswith("swn::frontend_pool(")
    assert re.search(r"Tensor\(a\d*!\)\[\] auxs", schema) and re.search(r"Tensor\(a\d*!\)\[\] conds", schema)
    assert lookahead_frames(C.bl6_laplace()) == LA


def _entry(aux=0x1000, new=0x2000, cond=0x3000, stride=64, received=20, n_new=2, f0=10, f1=16, flags=0, r0=0, r1=0):
    return _lib.FrontendPoolEntry(aux_dev=aux or None, new_dev=new or None, cond_dev=cond or None, aux_stride=stride,
                                  n_received=received, n_new=n_new, f0=f0, f1=f1, flags=flags,
                                  reserved=(ctypes.c_int32 * 2)(r0, r1))


def _call(d, entries, packed=1, work=1, n_entries=None, table=True):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    arr = (_lib.FrontendPoolEntry * max(1, len(entries)))(*entries)
    n = len(entries) if n_entries is None else n_entries
    rc = lib.swn_frontend_pool(ctypes.byref(d), p(packed), arr if table else None, n, p(work), None)
    if rc == BADARG and table and packed and work:
        assert lib.swn_frontend_pool_work_floats(ctypes.byref(d), arr, n) == 0
    return rc


def test_frontend_pool_rejects_bad_arguments_before_any_launch():
    """fake non-null addresses are fine: every one of these is refused before the library touches them"""
    d = _lib.desc_from_cfg(C.bl6_laplace())
    ok = [_entry(), _entry(aux=0x5000, cond=0x6000, received=9, n_new=0, new=0, f0=3, f1=9, flags=1)]
    assert _lib.lib().swn_frontend_pool_work_floats(ctypes.byref(d), (_lib.FrontendPoolEntry * 2)(*ok), 2) > 0
    assert _call(d, ok, packed=0) == BADARG                        # null pointers
    assert _call(d, ok, work=0) == BADARG
    assert _call(d, ok, table=False) == BADARG
    assert _call(d, [_entry(aux=0)]) == BADARG
    assert _call(d, [_entry(cond=0)]) == BADARG
    assert _call(d, [_entry(new=0)]) == BADARG                     # new frames announced, none given
    assert _call(d, ok, n_entries=0) == BADARG                     # entry count outside [1, 64]
    assert _call(d, [_entry(cond=0x3000 + 64 * i, n_new=0, f0=5, f1=5) for i in range(65)]) == BADARG
    assert _call(d, [_entry(f0=-1)]) == BADARG
    assert _call(d, [_entry(f0=12, f1=11)]) == BADARG
    assert _call(d, [_entry(n_new=-1)]) == BADARG
    assert _call(d, [_entry(received=3, n_new=4, f0=0, f1=0)]) == BADARG           # more new frames than received
    assert _call(d, [_entry(received=20, f1=17)]) == BADARG                        # f1 > n_received - lookahead, not FINAL
    assert _call(d, [_entry(received=3, n_new=0, f0=0, f1=1)]) == BADARG
    assert _call(d, [_entry(received=20, f1=21, flags=1)]) == BADARG               # f1 > n_received with FINAL
    assert _call(d, [_entry(stride=19)]) == BADARG                                 # aux_stride < n_received
    assert _call(d, [_entry(), _entry(aux=0x5000)]) == BADARG                      # one cond buffer in two entries
    assert _call(d, [_entry(cond=0x3004)]) == BADARG                               # cond rows are stored in 16-byte pieces
    assert _call(d, [_entry(flags=2)]) == BADARG                                   # unknown flag
    assert _call(d, [_entry(r0=1)]) == BADARG
    assert _call(d, [_entry(r1=1)]) == BADARG


def test_frontend_pool_of_idle_entries_launches_nothing():
    """f1 == f0 and n_new == 0: nothing to do, so fake addresses are fine"""
    d = _lib.desc_from_cfg(C.bl6_laplace())
    assert _call(d, [_entry(n_new=0, new=0, f0=7, f1=7), _entry(cond=0x7000, received=2, n_new=0, f0=0, f1=0)]) == 0


def test_work_buffer_holds_the_table_and_every_stage():
    cfg = C.bl6_laplace()
    d = _lib.desc_from_cfg(cfg)
    # kept [10, 16) of 20: stage 0 frames [6, 20), layer 0 [7, 19), layer 1 [10, 16); FINAL [3, 9) of 9: [0, 9), [0, 9), [3, 9)
    arr = (_lib.FrontendPoolEntry * 2)(_entry(), _entry(aux=0x5000, cond=0x6000, received=9, n_new=0, new=0, f0=3, f1=9, flags=1))
    na = cfg.n_aux
    want = 1024 + na * (14 + 9) + 3 * na * (12 + 9) + 9 * na * (6 + 6)
    assert _lib.lib().swn_frontend_pool_work_floats(ctypes.byref(d), arr, 2) == want


def _simulate(schedule, la):
    """the separate push / finish calls of DecodeStream on the counters alone"""
    out = []
    for key, received, done, n_new, finishing in schedule:
        received += n_new
        new_done = final_frames(received, la, finishing) if (finishing or received > 0) else done
        out.append((key, received, done, max(done, new_done), finishing))
    return out


@pytest.mark.parametrize("seed", range(8))
def test_plan_push_equals_the_separate_calls(seed):
    rng = np.random.default_rng(seed)
    la = int(rng.integers(0, 6))
    n = int(rng.integers(1, 64))
    state = {k: [0, 0] for k in range(n)}                     # received, final
    ended = set()
    for _tick in range(12):
        sched = []
        for k in range(n):
            if k in ended or rng.random() < 0.2:
                continue
            n_new = int(rng.integers(0, 8)) if rng.random() < 0.8 else 0      # 0-frame pushes included
            fin = bool(rng.random() < 0.15) and state[k][0] + n_new > 0       # ending with and without a tail
            sched.append((k, state[k][0], state[k][1], n_new, fin))
        calls = plan_push(sched, la)
        got = {e[0]: e for c in calls for e in c}
        assert all(1 <= len(c) <= 64 for c in calls)
        assert [e[0] for c in calls for e in c] == [s[0] for s in sched if s[0] in got]       # order kept
        for key, after, f0, f1, fin in _simulate(sched, la):
            if key in got:
                assert got[key] == (key, after, f0, f1, fin)
                assert after > state[key][0] or f1 > f0
            else:
                assert after == state[key][0] and f1 == f0     # nothing appended, nothing finalised: no entry
            state[key] = [after, f1]
            if fin:
                ended.add(key)
                assert f1 == after
            else:
                assert f1 == max(0, after - la)               # at most the lookahead received: nothing final


def test_plan_push_splits_calls_at_64_entries():
    sched = [(i, 10, 6, 2, i % 3 == 0) for i in range(65)]
    calls = plan_push(sched, LA)
    assert [len(c) for c in calls] == [64, 1]
    assert [e[0] for c in calls for e in c] == list(range(65))
    assert calls[0][0] == (0, 12, 6, 12, True) and calls[0][1] == (1, 12, 6, 8, False)
    assert [len(c) for c in plan_push(sched * 2, LA, limit=50)] == [50, 50, 30]
    assert plan_push([("x", 3, 0, 0, False)], LA) == []


def test_plan_push_rejects_bad_input():
    for bad in ([("a", -1, 0, 1, False)], [("a", 4, 0, -1, False)], [("a", 8, 5, 1, False)], [("a", 8, -1, 1, False)],
                [("a", 0, 0, 0, True)]):
        with pytest.raises(ValueError):
            plan_push(bad, LA)
    with pytest.raises(ValueError):
        plan_push([("a", 8, 4, 1, False)], -1)
    with pytest.raises(ValueError):
        plan_push([("a", 8, 4, 1, False)], LA, limit=0)


class _FakeNet:
    """what a pool reads of a HipNet before any launch"""

    def __init__(self, cfg):
        self.cfg, self.device = cfg, torch.device("cpu")
        self.dlist = ops.desc_list(cfg)


@pytest.mark.parametrize("stepped", [False, True])
def test_push_many_checks_everything_before_the_device(stepped):
    cfg = C.ref6_laplace() if stepped else C.bl6_laplace()
    pool = SteppedDecodePool(_FakeNet(cfg), 3) if stepped else DecodePool(_FakeNet(cfg), 3)
    other = DecodePool(_FakeNet(C.bl6_laplace()), 1)
    a, b, c = pool.open(), pool.open(), pool.open()
    good = torch.zeros(1, cfg.n_aux, 2)

    def untouched():
        return all(s._stream.frames_received == 0 and s._stream.frames_final == 0 and not s.finished
                   and s._stream._aux is None and s._stream._cond is None for s in (a, b, c))

    with pytest.raises(ValueError):
        pool.push_many({a: good, b: torch.zeros(cfg.n_aux, 2)})               # rank
    with pytest.raises(ValueError):
        pool.push_many({a: good, b: torch.zeros(2, cfg.n_aux, 2)})            # batch
    with pytest.raises(ValueError):
        pool.push_many({a: good, b: torch.zeros(1, cfg.n_aux + 1, 2)})        # channels
    with pytest.raises(ValueError):
        pool.push_many({a: good, b: "features"})
    with pytest.raises(ValueError):
        pool.push_many([(a, good)])
    with pytest.raises(RuntimeError, match="never received"):
        pool.push_many({a: good}, finish=[b])                                  # ended without any features
    with pytest.raises(RuntimeError, match="never received"):
        pool.push_many({a: good, b: torch.zeros(1, cfg.n_aux, 0)}, finish=[b])
    with pytest.raises(RuntimeError, match="not open"):
        pool.push_many({a: good, other.open(): good})                          # a session of another pool
    with pytest.raises(ValueError):
        pool.push_many({a: good}, finish=[a, a])
    pool.close(c)
    with pytest.raises(RuntimeError, match="closed"):
        pool.push_many({a: good, c: good})
    b._stream.frames_received, b._stream.finished = 3, True                    # as finish() leaves it
    with pytest.raises(RuntimeError, match="finished"):
        pool.push_many({a: good, b: good})
    with pytest.raises(RuntimeError, match="finished"):
        pool.push_many({a: good}, finish=[b])
    b._stream.frames_received, b._stream.finished = 0, False
    assert untouched()
    pool.push_many({})                                                         # nothing to do: no launch
    pool.push_many({a: torch.zeros(1, cfg.n_aux, 0)})
    assert untouched()
