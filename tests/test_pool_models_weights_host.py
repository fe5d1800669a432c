"""CPU: the decode pool over several models with bf16 / E4M3 head weights - the C entry points swn_decode_pool_chunk_models_w16 /
_w8, the two ops, DecodeModelPool.add_model and the call planning of a mixed tick: everything that runs before a device is
touched."""
import ctypes
import re

import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops, streaming
from shallow_wavenet_amd.streaming import DecodeModelPool, DecodePool, _local_models

BADARG, UNSUPPORTED = -2, -4                   # SWN_E_BADARG, SWN_E_UNSUPPORTED (include/swn_hip.h)
FORMATS = [("bf16", "w16"), ("e4m3", "w8")]


# ---------------------------------------------------------------------------------------------------------------- ops
@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_ops_are_the_fp32_models_op_with_the_images_second(fmt, sfx):
    name = f"decode_pool_chunk_models_{sfx}"
    assert name in ops.OP_NAMES
    assert ops.DECODE_IMAGES[fmt].suffix == sfx
    lib = _lib.lib()
    assert hasattr(lib, "swn_" + name) and "swn_" + name in _lib.SIGNATURES and lib.swn_abi_version() == 3
    alias = lambda schema: re.sub(r"\(a\d+!\)", "(a!)", schema)         # (the alias set is numbered by argument position)
    fp32 = alias(str(torch.ops.swn.decode_pool_chunk_models.default._schema))
    got = alias(str(getattr(torch.ops.swn, name).default._schema))
    head = "swn::decode_pool_chunk_models(Tensor[] models, "
    assert fp32.startswith(head)
    assert got == f"swn::{name}(Tensor[] models, Tensor[] {sfx}, " + fp32[len(head):]
    mutated = re.findall(r"Tensor\(a!\)(?:\[\])? (\w+)", got)
    assert mutated == ["session"]


# ------------------------------------------------------------------------------------------------------------- C entry points
def _ptrs(vals):
    return (ctypes.c_void_p * max(1, len(vals)))(*[v or None for v in vals])


def _entry(slot=0, step0=0, n_steps=4, flags=1, frames=4, cond=1):
    return _lib.DecodePoolEntry(cond_dev=cond or None, n_frames=frames, slot=slot, step0=step0, n_steps=n_steps, flags=flags,
                                reserved=0)


def _io():
    return _lib.DecodeIO(noise_dev=None, forced_dev=None, seed_dev=None, noise_out_dev=None, rng_seed=1, rng_utt0=0, reserved=0,
                         rng_utt_ids_dev=None)


def _call(sfx, d, entries, models=(1, 2), images=(3, 4), of=None, n_models=None, capacity=4, session=1, out=1, variant=6,
          null_images=False):
    """fake non-null addresses: every call here is refused, or has nothing to launch, before the library touches them"""
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    of = [e % len(models) for e in range(len(entries))] if of is None else of
    io = _io()
    return getattr(lib, f"swn_decode_pool_chunk_models_{sfx}")(
        ctypes.byref(d), _ptrs(models), len(models) if n_models is None else n_models,
        (ctypes.c_int32 * max(1, len(of)))(*of), capacity, (_lib.DecodePoolEntry * len(entries))(*entries), len(entries),
        ctypes.byref(io), p(session), p(out), None, variant, None if null_images else _ptrs(images), None)


@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_entry_points_refuse_before_any_device_call(fmt, sfx):
    d = _lib.desc_from_cfg(C.bl6_laplace(5, 4))
    ok = [_entry(0), _entry(1, step0=8, n_steps=2, flags=0, frames=8)]
    assert _call(sfx, d, ok, n_models=0) == BADARG                                     # n_models outside [1, 16]
    m17 = list(range(1, 18))
    assert _call(sfx, d, ok, models=m17, images=m17, of=[0, 16]) == BADARG
    assert _call(sfx, d, ok, null_images=True) == BADARG                               # a null image array
    assert _call(sfx, d, ok, images=(3, 0)) == BADARG                                  # a null image, named ...
    assert _call(sfx, d, ok, models=(1, 2, 3), images=(3, 0, 5), of=[0, 2]) == BADARG  # ... or not
    assert _call(sfx, d, ok, of=[0, 2]) == BADARG                                      # a model index out of range
    assert _call(sfx, d, ok, of=[-1, 0]) == BADARG
    assert _call(sfx, d, ok, models=(1, 0)) == BADARG                                  # the rules of the fp32 models call ...
    assert _call(sfx, d, ok, session=0) == BADARG                                      # ... and of the pool call still hold
    assert _call(sfx, d, [_entry(4)]) == BADARG
    # entries of 0 steps without BEGIN: accepted, nothing to launch; the images of models past n_models are not read
    idle = [_entry(0, step0=5, n_steps=0, flags=0), _entry(3, n_steps=0, flags=0)]
    assert _call(sfx, d, idle, out=0) == 0
    assert _call(sfx, d, idle, models=(1, 2, 3), images=(3, 4, 0), n_models=2, out=0) == 0


@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_entry_points_refuse_what_the_single_model_call_refuses(fmt, sfx):
    """a net or variant outside the symmetric kernel: the return code of swn_decode_pool_chunk_<suffix> for it"""
    lib = _lib.lib()
    single = getattr(lib, f"swn_decode_pool_chunk_{sfx}")
    cases = [(C.bl6_laplace(1, 4), 0), (C.bl6_laplace(1, 4), 2), (C.bl6_laplace(5, 4), 1), (C.bl6_laplace(5, 4), 3),
             (C.ref6_laplace(), 0), (C.ref6_laplace(), 6), (C.tiny("laplace", 2, 4), 0)]
    for cfg, variant in cases:
        d = _lib.desc_from_cfg(cfg)
        en = (_lib.DecodePoolEntry * 1)(_entry(0))
        io = _io()
        want = single(ctypes.byref(d), ctypes.c_void_p(1), 2, en, 1, ctypes.byref(io), ctypes.c_void_p(1), ctypes.c_void_p(1),
                      None, variant, ctypes.c_void_p(3), None)
        detail = lib.swn_last_error_detail().decode()
        assert want == UNSUPPORTED, (cfg, variant)
        assert _call(sfx, d, [_entry(0)], capacity=2, variant=variant) == want, (cfg, variant)
        mine = lib.swn_last_error_detail().decode()
        assert mine.replace(f"swn_decode_pool_chunk_models_{sfx}", f"swn_decode_pool_chunk_{sfx}") == detail
    # the argument rules come first: a null image on a net the kernel does not serve is SWN_E_BADARG
    assert _call(sfx, _lib.desc_from_cfg(C.ref6_laplace()), [_entry(0)], images=(0, 4)) == BADARG


# ------------------------------------------------------------------------------------------------------------------- pool
class _FakeNet:
    """what the pools read of a HipNet before any launch, and - for the planning test - at a launch"""

    def __init__(self, cfg, device="cpu", tag=0):
        self.cfg, self.device = cfg, torch.device(device)
        self.dlist = ops.desc_list(cfg)
        self.packed = ("packed", tag)
        self.images = 0

    def decode_w16_image(self):
        self.images += 1
        return ("w16", self.packed[1])

    def decode_w8_image(self):
        self.images += 1
        return ("w8", self.packed[1])


@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_add_model_takes_nets_of_the_pools_geometry_and_device(fmt, sfx):
    cfg = C.bl6_laplace(5, 4)
    pool = DecodeModelPool(_FakeNet(cfg), 4, rng_seed=5, weights=fmt)
    assert isinstance(pool, DecodePool) and pool.weights == fmt
    assert pool.open().model == 0
    with pytest.raises(ValueError, match="NetConfig"):
        pool.add_model(_FakeNet(C.bl6_laplace(2, 4)))
    with pytest.raises(ValueError, match="NetConfig"):
        pool.add_model(_FakeNet(C.bl6_softmax()))
    with pytest.raises(ValueError, match="meta"):
        pool.add_model(_FakeNet(cfg, "meta"))
    other = _FakeNet(C.bl6_laplace(5, 4))
    assert pool.add_model(other) == 1 and pool.add_model(_FakeNet(cfg)) == 2            # indices count from 1
    s = pool.open(model=1)
    assert s.model == 1 and s._stream.net is other and s._stream.weights == fmt
    with pytest.raises(ValueError, match="model"):
        pool.open(model=3)
    assert pool.step() == {}
    # the rules of the weights keyword are DecodePool's: variant 6 for the single-sample Laplace nets, no other kernel
    with pytest.raises(ValueError, match="variant=6"):
        DecodeModelPool(_FakeNet(C.bl6_laplace(1, 4)), 4, weights=fmt)
    assert DecodeModelPool(_FakeNet(C.bl6_laplace(1, 4)), 4, variant=6, weights=fmt).add_model(_FakeNet(C.bl6_laplace(1, 4))) == 1
    with pytest.raises(ValueError):
        DecodeModelPool(_FakeNet(C.ref6_laplace()), 4, variant=1, weights=fmt)


@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_a_decode_pool_of_stored_weights_still_serves_one_model(fmt, sfx):
    cfg = C.bl6_softmax()
    with pytest.raises(ValueError, match="one model") as e:
        DecodePool(_FakeNet(cfg), 4, weights=fmt).add_model(_FakeNet(cfg))
    assert "DecodeModelPool" in str(e.value)
    assert DecodeModelPool(_FakeNet(cfg), 4, weights="fp32").add_model(_FakeNet(cfg)) == 1


@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_open_pool_routes_stored_weights_with_multi_model_to_the_model_pool(fmt, sfx):
    from shallow_wavenet_amd.nets import cswnv_shift1 as mc

    def pool_of(cfg, **kw):
        m = mc.CSWNV(**cfg.ctor_kwargs())
        m._engine = lambda: _FakeNet(cfg)                                # the module's parameters are on the CPU here
        return m.open_pool(4, **kw)

    cfg = C.bl6_laplace(5, 4)
    assert type(pool_of(cfg, multi_model=True, weights=fmt)) is DecodeModelPool
    assert type(pool_of(cfg, multi_model=True)) is DecodePool            # fp32: DecodePool takes add_model as it is
    assert type(pool_of(cfg, weights=fmt)) is DecodePool                 # one model
    assert type(pool_of(C.bl6_laplace(1, 4), variant=6, multi_model=True, weights=fmt)) is DecodeModelPool
    with pytest.raises(ValueError, match="variant=6"):
        pool_of(C.bl6_laplace(1, 4), multi_model=True, weights=fmt)
    with pytest.raises(ValueError, match="stepped"):                     # stepped nets: nothing changes
        pool_of(C.ref6_laplace(), multi_model=True, weights=fmt)


class _SpyOps:
    """stands in for torch.ops.swn in streaming: records every call and returns outputs of the op's shapes"""

    def __init__(self, seg):
        self.calls, self.seg = [], seg

    def __getattr__(self, name):
        def op(*args):
            self.calls.append((name, args))
            n_steps = args[-10]
            E, n_max = len(n_steps), max(n_steps)
            return torch.zeros(E, n_max * self.seg), torch.zeros(0), torch.zeros(0)
        return op


@pytest.mark.parametrize("fmt,sfx", FORMATS)
def test_a_tick_over_17_models_is_cut_into_calls_of_16(fmt, sfx, monkeypatch):
    cfg = C.bl6_laplace(5, 4)
    nets = [_FakeNet(cfg, tag=k) for k in range(17)]
    pool = DecodeModelPool(nets[0], 20, rng_seed=5, weights=fmt)
    for n in nets[1:]:
        pool.add_model(n)
    order = [16, 3, 3, 0] + list(range(1, 16)) + [16]                    # 20 sessions over 17 models, not sorted
    sess = [pool.open(model=m) for m in order]
    for i, s in enumerate(sess):                                         # one final frame each: U / seg ready steps
        s._stream._cond = torch.zeros(1, 1, 4)
        s._stream.frames_received = s._stream.frames_final = 1
    spy = _SpyOps(cfg.seg)
    monkeypatch.setattr(streaming, "_O", spy)
    res = pool.step(max_steps=2)
    assert set(res) == set(sess) and all(s.steps_done == 2 for s in sess)
    assert [name for name, _ in spy.calls] == [f"decode_pool_chunk_models_{sfx}"] * 2
    seen = 0
    for name, args in spy.calls:
        packed, images, of = args[0], args[1], args[2]
        slots = args[5]
        part = order[seen:seen + len(slots)]
        assert slots == [s.slot for s in sess[seen:seen + len(slots)]]
        distinct, local = _local_models(part)
        assert len(distinct) <= _lib.POOL_MAX_MODELS
        assert of == local
        assert packed == [("packed", m) for m in distinct]               # the call's own table, in order of first appearance
        assert images == [(sfx, m) for m in distinct]
        seen += len(slots)
    assert seen == len(order) and len(spy.calls[0][1][5]) == 18          # greedy: cut where the 17th model (15) would enter
    assert spy.calls[1][1][0] == [("packed", 15), ("packed", 16)] and spy.calls[1][1][2] == [0, 1]
    # a tick over one model issues the single-model image op with that model
    for s in sess[:19]:
        pool.close(s)
    del spy.calls[:]
    pool.step(max_steps=1)
    assert [name for name, _ in spy.calls] == [f"decode_pool_chunk_{sfx}"]
    assert spy.calls[0][1][:2] == (("packed", 16), (sfx, 16))
