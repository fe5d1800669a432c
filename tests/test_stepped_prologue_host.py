"""CPU: the parallel prologue of the stepped decode (swn_decode_stepped_prologue, prologue="parallel"): the C ABI's argument
checks and work-size query, the op schema, the `prologue` keyword of the streams and pools, and the tick bookkeeping with
the op mocked - everything that runs before a device is touched."""
import ctypes
import dataclasses
import re

import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops, streaming
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream, SteppedDecodePool, SteppedModelPool

BADARG, UNSUPPORTED = -2, -4                   # SWN_E_BADARG, SWN_E_UNSUPPORTED (include/swn_hip.h)


def test_prologue_symbols_are_exported_and_bound():
    lib = _lib.lib()
    for name in ("swn_decode_stepped_prologue", "swn_decode_stepped_prologue_work_floats"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.DecodeSteppedPrologueEntry) == 16
    assert lib.swn_abi_version() == 3
    assert "decode_stepped_prologue" in ops.OP_NAMES
    schema = str(torch.ops.swn.decode_stepped_prologue.default._schema)
    assert schema.startswith("swn::decode_stepped_prologue(") and re.search(r"Tensor\(a\d*!\) session", schema)
    assert "Tensor? seeds" in schema


def _io(noise=0, forced=0):
    return _lib.DecodeIO(noise_dev=noise or None, forced_dev=forced or None, seed_dev=None, noise_out_dev=None, rng_seed=1,
                         rng_utt0=0, reserved=0, rng_utt_ids_dev=None)


def _entry(slot=0, frames=4, cond=1):
    return _lib.DecodeSteppedPrologueEntry(cond_dev=cond or None, n_frames=frames, slot=slot)


def _call(d, entries, n_slots=4, io=None, session=1, packed=1, work=1, n_entries=None, table=True, models=None, model_of=None,
          n_models=0, no_io=False):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    arr = (_lib.DecodeSteppedPrologueEntry * max(1, len(entries)))(*entries)
    mp = None if models is None else (ctypes.c_void_p * len(models))(*models)
    of = None if model_of is None else (ctypes.c_int32 * len(model_of))(*model_of)
    return lib.swn_decode_stepped_prologue(ctypes.byref(d), p(packed), mp, n_models, of, n_slots, arr if table else None,
                                           len(entries) if n_entries is None else n_entries,
                                           None if no_io else ctypes.byref(io if io is not None else _io()), p(session),
                                           p(work), None)


def test_prologue_rejects_bad_arguments_before_any_launch():
    """fake non-null addresses are fine: every one of these is refused before the library touches them"""
    d = _lib.desc_from_cfg(C.ref6_laplace())
    ok = [_entry(0), _entry(3, frames=1)]
    assert _call(d, ok, session=0) == BADARG                        # null pointers
    assert _call(d, ok, packed=0) == BADARG
    assert _call(d, ok, work=0) == BADARG
    assert _call(d, ok, table=False) == BADARG
    assert _call(d, ok, no_io=True) == BADARG
    assert _call(d, [_entry(cond=0)]) == BADARG
    assert _call(d, ok, n_entries=0) == BADARG                      # entry count outside [1, 64]
    assert _call(d, [_entry(i) for i in range(65)], n_slots=65) == BADARG
    assert _call(d, ok, n_slots=0) == BADARG
    assert _call(d, [_entry(4)]) == BADARG                          # slot outside [0, n_slots)
    assert _call(d, [_entry(-1)]) == BADARG
    assert _call(d, [_entry(2), _entry(1), _entry(2)]) == BADARG    # one slot in two entries
    assert _call(d, [_entry(0, frames=0)]) == BADARG                # the prologue reads frame 0
    assert _call(d, ok, io=_io(noise=1)) == BADARG                  # as the pool calls: no host noise, no teacher forcing
    assert _call(d, ok, io=_io(forced=1)) == BADARG
    # the model rules of the *_models calls
    assert _call(d, ok, packed=0, models=[1, 1], model_of=[0, 1], n_models=0) == BADARG
    assert _call(d, ok, packed=0, models=[1] * 17, model_of=[0, 1], n_models=17) == BADARG
    assert _call(d, ok, packed=0, models=[1, 0], model_of=[0, 0], n_models=2) == BADARG      # a null model pointer
    assert _call(d, ok, packed=0, models=[1, 1], model_of=[0, 2], n_models=2) == BADARG      # index outside [0, n_models)
    assert _call(d, ok, packed=0, models=[1, 1], model_of=[-1, 0], n_models=2) == BADARG
    assert _call(d, ok, packed=0, models=[1, 1], model_of=None, n_models=2) == BADARG        # models without indices
    assert _call(d, ok, models=None, model_of=[0, 0], n_models=1) == BADARG                  # indices without models
    # a descriptor that is none
    bad = _lib.desc_from_cfg(C.ref6_laplace())
    bad.kernel_size = 1
    assert _call(bad, ok) < 0


def test_prologue_unsupported_geometry_launches_nothing():
    d = _lib.desc_from_cfg(C.ref6_laplace())
    # slots whose state passes the 2 GiB buffer-offset limit: the stepped chain does not run them
    per_slot = _lib.lib().swn_decode_session_floats(ctypes.byref(d), 1, 3)
    big = (1 << 31) // (4 * per_slot) + 1
    assert _call(d, [_entry(0)], n_slots=big) == UNSUPPORTED
    # a tap-major row of more than 8 x 256 floats: not a net of the stepped chain
    wide = _lib.desc_from_cfg(dataclasses.replace(C.ref6_laplace(), hid_chn=320))
    assert _lib.lib().swn_decode_resolve_variant(ctypes.byref(wide), 1, 3) < 0
    assert _call(wide, [_entry(0)]) == UNSUPPORTED


def test_prologue_work_floats_query():
    lib = _lib.lib()
    for cfg in (C.ref6_laplace(1, 4), C.ref6_laplace(5, 4), C.ref6_softmax(), C.tiny(), C.bl6_laplace()):
        d = _lib.desc_from_cfg(cfg)
        n_pro = lib.swn_decode_stepped_prologue_iterations(ctypes.byref(d))
        hp = (cfg.hid_chn + 3) & ~3
        sizes = [lib.swn_decode_stepped_prologue_work_floats(ctypes.byref(d), n) for n in range(1, 65)]
        assert sizes[0] == 2 * n_pro * hp                            # two ping-pong levels of n_pro x Hp floats per entry
        assert all(b > a for a, b in zip(sizes, sizes[1:]))          # monotone in the entry count
        assert sizes == [sizes[0] * n for n in range(1, 65)]
        assert ops.stepped_prologue_work_floats(d, 9) == sizes[8]
        for n in (0, -1, 65):
            assert lib.swn_decode_stepped_prologue_work_floats(ctypes.byref(d), n) == 0
    wide = _lib.desc_from_cfg(dataclasses.replace(C.ref6_laplace(), hid_chn=320))
    assert lib.swn_decode_stepped_prologue_work_floats(ctypes.byref(wide), 1) == 0
    bad = _lib.desc_from_cfg(C.ref6_laplace())
    bad.kernel_size = 1
    assert lib.swn_decode_stepped_prologue_work_floats(ctypes.byref(bad), 1) == 0


class _FakeNet:
    """what the streams and pools read of a HipNet before any launch (buffers live on the CPU here)"""

    def __init__(self, cfg):
        self.cfg, self.device = cfg, torch.device("cpu")
        self.dlist = ops.desc_list(cfg)
        self.packed = torch.zeros(4)


def test_parallel_prologue_needs_the_stepped_chain():
    bl6, ref6 = _FakeNet(C.bl6_laplace()), _FakeNet(C.ref6_laplace())
    with pytest.raises(ValueError, match="parallel"):
        DecodeStream(bl6, 1, prologue="parallel")                   # BL6 resolves to its register-resident kernel
    with pytest.raises(ValueError, match="parallel"):
        DecodeStream(ref6, 1, variant=1, prologue="parallel")       # the generic kernel, asked for by number
    assert DecodeStream(bl6, 1).prologue == "stepped"
    assert DecodeStream(ref6, 2, prologue="parallel").prologue == "parallel"       # variant 0 resolves to 3 on REF6
    assert DecodeStream(_FakeNet(C.tiny()), 2, variant=3, prologue="parallel").resolved_variant == 3
    assert SteppedDecodePool(ref6, 2).prologue == "stepped"
    assert SteppedDecodePool(ref6, 2, prologue="parallel").prologue == "parallel"
    assert SteppedModelPool(ref6, 2, prologue="parallel").prologue == "parallel"


@pytest.mark.parametrize("bad", ["", "Parallel", "fast", None, 1])
def test_bad_prologue_strings_raise(bad):
    ref6 = _FakeNet(C.ref6_laplace())
    with pytest.raises(ValueError, match="prologue"):
        DecodeStream(ref6, 1, prologue=bad)
    with pytest.raises(ValueError, match="prologue"):
        SteppedDecodePool(ref6, 2, prologue=bad)
    with pytest.raises(ValueError, match="prologue"):
        SteppedModelPool(ref6, 2, prologue=bad)


def test_plain_pool_takes_no_prologue_keyword():
    with pytest.raises(TypeError):
        DecodePool(_FakeNet(C.bl6_laplace()), 2, prologue="parallel")


class _Ops:
    """torch.ops.swn of streaming.py with the two calls of a stepped tick recorded instead of launched"""

    def __init__(self, cfg):
        self.fills, self.chunks, self.seg = [], [], cfg.seg

    def decode_stepped_prologue(self, models, model_of, session, conds, slots, seeds, desc, n_slots):
        self.fills.append(dict(models=models, model_of=list(model_of), slots=list(slots), conds=conds, seeds=seeds,
                               n_slots=n_slots))

    def _chunk(self, slots, it0s, n_its, begins, seeds):
        self.chunks.append(dict(slots=list(slots), it0s=list(it0s), n_its=list(n_its), begins=list(begins), seeds=seeds))
        n_max = max(n_its)
        return torch.zeros(len(slots), n_max * self.seg), torch.zeros(0), torch.zeros(0)

    def decode_pool_stepped_chunk(self, packed, session, conds, slots, it0s, n_its, begins, seeds, utt_ids, desc, capacity,
                                  rng_seed, want_heads, want_noise):
        return self._chunk(slots, it0s, n_its, begins, seeds)

    def decode_pool_stepped_chunk_models(self, models, of, session, conds, slots, it0s, n_its, begins, seeds, utt_ids, desc,
                                         capacity, rng_seed, want_heads, want_noise):
        r = self._chunk(slots, it0s, n_its, begins, seeds)
        self.chunks[-1]["models"] = (len(models), list(of))
        return r


def _ready(s, cfg, frames):
    """give a pool session `frames` final frames without a front end"""
    st = s._stream
    st._cond = torch.zeros(1, 8, 4)
    st.frames_received = st.frames_final = frames


def test_parallel_tick_fills_beginning_sessions_then_plans_generation_only(monkeypatch):
    cfg = C.tiny("laplace", 2, 4)
    fake = _Ops(cfg)
    monkeypatch.setattr(streaming, "_O", fake)
    pool = SteppedDecodePool(_FakeNet(cfg), 70, prologue="parallel")
    n_pro = pool.n_pro
    sess = [pool.open(seed=torch.full((1, cfg.seg), 0.25) if i == 3 else None) for i in range(70)]
    for s in sess[:67]:
        _ready(s, cfg, 1)                                            # 67 begin; 3 still wait for features
    res = pool.step(max_steps=4, max_prologue=10)
    # one fill call per at most 64 beginning sessions, in admission order, over the pool's slots
    assert [len(f["slots"]) for f in fake.fills] == [64, 3]
    assert [x for f in fake.fills for x in f["slots"]] == list(range(67))
    assert all(f["n_slots"] == 70 and len(f["models"]) == 1 for f in fake.fills)
    assert fake.fills[0]["seeds"] is not None and tuple(fake.fills[0]["seeds"].shape) == (64, cfg.seg)
    assert fake.fills[0]["seeds"][3].tolist() == [0.25] * cfg.seg and fake.fills[0]["seeds"][2].abs().sum() == 0
    assert fake.fills[1]["seeds"] is None
    # the plan holds generation entries only: it0 = n_pro, no BEGIN, and max_prologue had nothing left to spread
    assert [len(c["slots"]) for c in fake.chunks] == [64, 3]
    for c in fake.chunks:
        assert set(c["it0s"]) == {n_pro} and set(c["n_its"]) == {4} and not any(c["begins"]) and c["seeds"] is None
    assert all(s._it_done == n_pro + 4 and s.steps_done == 4 and s._stream._begun for s in sess[:67])
    assert all(s._it_done == 0 and not s._stream._begun for s in sess[67:])
    assert set(res) == set(sess[:67]) and all(r[0].shape == (1, 4 * cfg.seg) for r in res.values())
    # the next tick: nobody begins, so no fill call; a session that becomes ready later is filled then
    fake.fills.clear(), fake.chunks.clear()
    _ready(sess[68], cfg, 1)
    pool.step(max_steps=1)
    assert [f["slots"] for f in fake.fills] == [[68]]
    assert sorted(x for c in fake.chunks for x in c["slots"]) == list(range(67)) + [68]
    assert sess[68]._it_done == n_pro + 1


def test_stepped_setting_makes_no_fill_call(monkeypatch):
    cfg = C.tiny("laplace", 2, 4)
    fake = _Ops(cfg)
    monkeypatch.setattr(streaming, "_O", fake)
    pool = SteppedDecodePool(_FakeNet(cfg), 4)
    s = pool.open()
    _ready(s, cfg, 1)
    pool.step(max_steps=2)
    assert fake.fills == [] and fake.chunks[0]["begins"] == [True] and fake.chunks[0]["it0s"] == [0]
    assert fake.chunks[0]["n_its"] == [pool.n_pro + 2]


def test_parallel_tick_of_a_model_pool_cuts_fill_calls_at_16_models(monkeypatch):
    cfg = C.tiny("laplace", 1, 0)
    fake = _Ops(cfg)
    monkeypatch.setattr(streaming, "_O", fake)
    nets = [_FakeNet(cfg) for _ in range(18)]
    pool = SteppedModelPool(nets[0], 40, prologue="parallel")
    for n in nets[1:]:
        pool.add_model(n)
    sess = [pool.open(model=i % 18) for i in range(36)]
    for s in sess:
        _ready(s, cfg, 2)
    pool.step(max_steps=3)
    # entries 0 .. 15 name 16 models; entry 16 would bring the 17th: the existing split_models cuts there
    assert [len(f["slots"]) for f in fake.fills] == [16, 16, 4]
    assert all(len(f["models"]) <= _lib.POOL_MAX_MODELS for f in fake.fills)
    assert fake.fills[0]["model_of"] == list(range(16))
    assert [len(f["models"]) for f in fake.fills] == [16, 16, 4]
    assert all(f["models"][k] is nets[sess[f["slots"][e]].model].packed
               for f in fake.fills for e, k in enumerate(f["model_of"]))
    assert all(s._it_done == pool.n_pro + 3 for s in sess)
    assert all(not any(c["begins"]) and set(c["it0s"]) == {pool.n_pro} for c in fake.chunks)


def test_parallel_stream_fills_before_its_first_chunk_only(monkeypatch):
    cfg = C.tiny("laplace", 2, 4)
    calls = []

    class _S:
        def decode_stepped_prologue(self, models, model_of, session, conds, slots, seeds, desc, n_slots):
            calls.append(("fill", len(models), list(slots), [tuple(c.shape) for c in conds], seeds, n_slots))

        def decode_chunk(self, packed, cond, session, noise, forced, seed, desc, step0, n, begin, variant, *rest):
            calls.append(("chunk", step0, n, begin))
            return torch.zeros(cond.shape[0], n * cfg.seg), torch.zeros(0), torch.zeros(0)

    monkeypatch.setattr(streaming, "_O", _S())
    seed = torch.arange(6, dtype=torch.float32).reshape(3, 2)
    st = DecodeStream(_FakeNet(cfg), 3, variant=3, seed=seed, prologue="parallel")
    st._cond = torch.zeros(3, 8, 4)
    st.frames_received = st.frames_final = 2
    st.advance(5)
    st.advance(4)
    assert calls[0][:4] == ("fill", 1, [0, 1, 2], [(8, 4)] * 3) and calls[0][4] is seed and calls[0][5] == 3
    assert calls[1:] == [("chunk", 0, 5, False), ("chunk", 5, 4, False)]
    calls.clear()
    st = DecodeStream(_FakeNet(cfg), 3, variant=3)
    st._cond = torch.zeros(3, 8, 4)
    st.frames_received = st.frames_final = 2
    st.advance(5)
    assert calls == [("chunk", 0, 5, True)]
