"""CPU: the return code of every decode entry point of the C ABI (swn_decode, swn_decode_chunk, swn_decode_pool_chunk,
swn_decode_pool_chunk_models and the three *_w16 and *_w8 forms) for the argument combinations that are decided before a
launch - the common refusals, and the places where the fp32 family and the families over a stored image answer differently.
Fake non-null addresses: no row of these tables reaches a launch."""
import ctypes

import pytest

from shallow_wavenet_amd import _lib, config as C

OK, BADARG, UNSUPPORTED = 0, -2, -4            # SWN_OK, SWN_E_BADARG, SWN_E_UNSUPPORTED (include/swn_hip.h)
MAX_ENTRIES, MAX_MODELS = _lib.DECODE_POOL_MAX_ENTRIES, _lib.POOL_MAX_MODELS

SMX = C.bl6_softmax()                          # the symmetric BL6 kernel at variants 0, 2 and 6
S1 = C.bl6_laplace(1, 4)                       # the wave-specialised kernel at variants 0 and 2, the symmetric one at 6
S5 = C.bl6_laplace(5, 4)                       # the symmetric BL6 kernel
REF = C.ref6_laplace()                         # the stepped chain at variants 0 and 3
TINY = C.tiny("laplace", 2, 4)                 # the generic kernel at variants 0 and 1
NETS = {"smx": SMX, "s1": S1, "s5": S5, "ref": REF, "tiny": TINY}

VARIANT6 = "variant = 6"                       # detail text of a *_w16 / *_w8 call that resolves to the wave-specialised kernel ...
BL6_ONLY = "symmetric BL6 kernel only"         # ... and to any other kernel, or to none
WORD = {"w16": "bf16", "w8": "e4m3"}           # ... both of which name the format of the call's image


def _p(v):
    return ctypes.c_void_p(v) if v else None


def _io(noise=0, forced=0):
    return _lib.DecodeIO(noise_dev=noise or None, forced_dev=forced or None, seed_dev=None, noise_out_dev=None, rng_seed=1,
                         rng_utt0=0, reserved=0, rng_utt_ids_dev=None)


def _detail():
    return _lib.lib().swn_last_error_detail().decode()


def _run(call, rows, word=None):
    """rows of (keyword arguments, return code[, text the error detail holds - next to `word`, if given])"""
    for row in rows:
        kw, want, text = row if len(row) == 3 else (*row, None)
        got = call(**kw)
        assert got == want, (kw, got, want)
        if text is not None:
            assert text in _detail(), (kw, _detail())
            assert word is None or word + " weights" in _detail(), (kw, _detail())


def test_the_nets_resolve_to_the_kernels_these_tables_assume():
    lib = _lib.lib()
    res = lambda cfg, v, batch=1: lib.swn_decode_resolve_variant(ctypes.byref(_lib.desc_from_cfg(cfg)), batch, v)
    assert [res(SMX, v) for v in (0, 1, 2, 3, 6)] == [2, 1, 2, 3, 6]
    assert [res(S1, v) for v in (0, 1, 2, 3, 6)] == [2, 1, 2, 3, 6]
    assert [res(S5, v) for v in (0, 1, 2, 3, 6)] == [2, 1, 2, 3, 6]
    assert [res(REF, v) for v in (0, 2, 3, 6)] == [3, UNSUPPORTED, 3, UNSUPPORTED]
    assert [res(TINY, v) for v in (0, 1, 2, 3, 6)] == [1, 1, UNSUPPORTED, 3, UNSUPPORTED]
    for cfg in NETS.values():
        assert [res(cfg, v) for v in (-1, 4, 5, 7)] == [BADARG] * 4
        assert res(cfg, 0, batch=0) == BADARG


# ------------------------------------------------------------------------------------------------------------------ one-shot
def _oneshot(fmt):
    """fmt: None (swn_decode), "w16" (swn_decode_w16) or "w8" (swn_decode_w8)"""
    def call(net=SMX, variant=0, packed=1, cond=1, batch=1, frames=4, n_steps=4, io=1, state=1, out=1, image=1, desc=1):
        lib, d = _lib.lib(), _lib.desc_from_cfg(net)
        args = [ctypes.byref(d) if desc else None, _p(packed), _p(cond), batch, frames, n_steps,
                ctypes.byref(_io()) if io else None, _p(state), _p(out), None, variant]
        return getattr(lib, "swn_decode_" + fmt)(*args, _p(image), None) if fmt else lib.swn_decode(*args, None)
    return call


ONESHOT_COMMON = [
    (dict(desc=0), BADARG), (dict(io=0), BADARG), (dict(batch=0), BADARG), (dict(frames=0), BADARG),
    (dict(n_steps=-1), BADARG), (dict(packed=0), BADARG), (dict(cond=0), BADARG), (dict(out=0), BADARG),
    (dict(n_steps=4 * 80 + 1), BADARG),                    # past the conditioning: n_steps * seg > n_frames * U
    (dict(net=S5, n_steps=4 * 22 + 1), BADARG),
    (dict(io=0, n_steps=0), BADARG), (dict(batch=0, n_steps=0), BADARG), (dict(frames=0, n_steps=0), BADARG),
]


def test_swn_decode():
    _run(_oneshot(None), ONESHOT_COMMON + [
        # nothing to generate: SWN_OK before the buffers and the variant are looked at
        (dict(n_steps=0, packed=0, cond=0, out=0, state=0), OK),
        (dict(n_steps=0, variant=99), OK), (dict(net=REF, n_steps=0, variant=2, state=0), OK),
        (dict(net=TINY, n_steps=0, variant=6, packed=0), OK),
        # the state buffer comes before an unresolvable variant, except for the variants that ask for the BL6 class alone
        (dict(net=REF, state=0, variant=0), BADARG), (dict(net=REF, state=0, variant=3), BADARG),
        (dict(net=REF, state=0, variant=2), UNSUPPORTED), (dict(net=REF, state=0, variant=6), UNSUPPORTED),
        (dict(net=REF, variant=2), UNSUPPORTED), (dict(net=REF, variant=6), UNSUPPORTED),
        (dict(net=TINY, state=0, variant=0), BADARG), (dict(net=TINY, state=0, variant=1), BADARG),
        (dict(net=TINY, state=0, variant=2), UNSUPPORTED), (dict(net=TINY, variant=6), UNSUPPORTED),
        (dict(net=SMX, state=0, variant=1), BADARG), (dict(net=S5, state=0, variant=3), BADARG),
        (dict(state=0, variant=4), BADARG), (dict(variant=4), BADARG), (dict(variant=-1), BADARG), (dict(variant=7), BADARG),
        (dict(net=REF, variant=5), BADARG),
        # the other checks come before the variant
        (dict(net=REF, variant=2, out=0), BADARG), (dict(net=REF, variant=2, n_steps=4 * 110 + 1), BADARG),
    ])


ONESHOT_IMAGE = ONESHOT_COMMON + [
        (dict(image=0), BADARG), (dict(image=0, n_steps=0), BADARG),
        # nothing to generate: still an image and a variant that resolves to the symmetric kernel
        (dict(n_steps=0, packed=0, cond=0, out=0, state=0), OK), (dict(net=S1, n_steps=0, variant=6, packed=0), OK),
        (dict(net=S5, n_steps=0, variant=2, out=0), OK),
        (dict(net=S1, n_steps=0), UNSUPPORTED, VARIANT6), (dict(net=S1, n_steps=0, variant=2), UNSUPPORTED, VARIANT6),
        (dict(net=REF, n_steps=0), UNSUPPORTED, BL6_ONLY), (dict(net=TINY, n_steps=0, variant=6), UNSUPPORTED, BL6_ONLY),
        (dict(n_steps=0, variant=99), UNSUPPORTED, BL6_ONLY),
        # the state buffer is never looked at
        (dict(net=REF, state=0, variant=0), UNSUPPORTED, "stepped"), (dict(net=REF, state=0, variant=2), UNSUPPORTED),
        (dict(net=REF, variant=6), UNSUPPORTED), (dict(net=TINY, state=0), UNSUPPORTED, "generic"),
        (dict(net=S1), UNSUPPORTED, VARIANT6), (dict(net=S1, variant=2, state=0), UNSUPPORTED, VARIANT6),
        (dict(net=S5, variant=1), UNSUPPORTED, BL6_ONLY), (dict(net=SMX, variant=3), UNSUPPORTED, BL6_ONLY),
        (dict(variant=4), UNSUPPORTED, BL6_ONLY), (dict(variant=-1), UNSUPPORTED), (dict(variant=7), UNSUPPORTED),
        # the other checks come before the variant
        (dict(net=REF, out=0), BADARG), (dict(net=S1, n_steps=4 * 110 + 1), BADARG), (dict(net=S1, image=0), BADARG),
]


def test_swn_decode_w16():
    _run(_oneshot("w16"), ONESHOT_IMAGE, WORD["w16"])


def test_swn_decode_w8():
    _run(_oneshot("w8"), ONESHOT_IMAGE, WORD["w8"])


# --------------------------------------------------------------------------------------------------------------------- chunk
def _chunk(fmt):
    """fmt: None (swn_decode_chunk), "w16" (swn_decode_chunk_w16) or "w8" (swn_decode_chunk_w8)"""
    def call(net=SMX, variant=0, packed=1, cond=1, batch=1, frames=4, step0=0, n_steps=4, flags=1, io=1, session=1, out=1,
             image=1, desc=1):
        lib, d = _lib.lib(), _lib.desc_from_cfg(net)
        args = [ctypes.byref(d) if desc else None, _p(packed), _p(cond), batch, frames, step0, n_steps, flags,
                ctypes.byref(_io()) if io else None, _p(session), _p(out), None, variant]
        return getattr(lib, "swn_decode_chunk_" + fmt)(*args, _p(image), None) if fmt else lib.swn_decode_chunk(*args, None)
    return call


CHUNK_COMMON = [
    (dict(desc=0), BADARG), (dict(io=0), BADARG), (dict(session=0), BADARG), (dict(packed=0), BADARG), (dict(cond=0), BADARG),
    (dict(batch=0), BADARG), (dict(frames=0), BADARG), (dict(step0=-1, flags=0), BADARG), (dict(n_steps=-1), BADARG),
    (dict(flags=2), BADARG), (dict(flags=3), BADARG), (dict(flags=-1), BADARG),
    (dict(step0=1), BADARG),                               # BEGIN starts at step 0
    (dict(out=0), BADARG),
    (dict(n_steps=4 * 80 + 1), BADARG),                    # past the conditioning: (step0 + n_steps) * seg > n_frames * U
    (dict(step0=4 * 80 - 3, flags=0), BADARG), (dict(step0=4 * 80 + 1, n_steps=0, flags=0, out=0), BADARG),
    (dict(step0=2 ** 31 - 1, n_steps=2 ** 31 - 1, flags=0), BADARG),
    (dict(net=S5, step0=80, n_steps=9, flags=0), BADARG),
    # the buffers are wanted even when there is nothing to generate
    (dict(n_steps=0, flags=0, packed=0), BADARG), (dict(n_steps=0, flags=0, session=0), BADARG),
    # nothing to generate and no BEGIN: SWN_OK once the variant has resolved, the session stays as it is
    (dict(n_steps=0, flags=0, out=0), OK), (dict(step0=4 * 80, n_steps=0, flags=0, out=0), OK),
    (dict(net=S1, variant=6, n_steps=0, flags=0, out=0), OK),
]


def test_swn_decode_chunk():
    _run(_chunk(None), CHUNK_COMMON + [
        (dict(net=S1, n_steps=0, flags=0, out=0), OK), (dict(net=REF, n_steps=0, flags=0, out=0), OK),
        (dict(net=TINY, n_steps=0, flags=0, out=0, variant=3), OK),
        # an unresolvable (net, batch, variant) is a bad argument here, with or without work
        (dict(net=REF, variant=2), BADARG), (dict(net=REF, variant=6), BADARG), (dict(net=TINY, variant=2), BADARG),
        (dict(variant=4), BADARG), (dict(variant=-1), BADARG), (dict(variant=7), BADARG),
        (dict(net=REF, variant=2, n_steps=0, flags=0, out=0), BADARG), (dict(variant=5, n_steps=0, flags=0), BADARG),
    ])


CHUNK_IMAGE = CHUNK_COMMON + [
        (dict(image=0), BADARG), (dict(image=0, n_steps=0, flags=0), BADARG),
        # what does not resolve to the symmetric kernel is unsupported, with the detail text, with or without work
        (dict(net=S1), UNSUPPORTED, VARIANT6), (dict(net=S1, variant=2), UNSUPPORTED, VARIANT6),
        (dict(net=S5, variant=1), UNSUPPORTED, "generic"), (dict(net=SMX, variant=3), UNSUPPORTED, BL6_ONLY),
        (dict(net=REF), UNSUPPORTED, "stepped"), (dict(net=REF, variant=2), UNSUPPORTED, BL6_ONLY),
        (dict(net=REF, variant=6), UNSUPPORTED, BL6_ONLY), (dict(net=TINY), UNSUPPORTED, BL6_ONLY),
        (dict(variant=4), UNSUPPORTED, BL6_ONLY), (dict(variant=-1), UNSUPPORTED, BL6_ONLY), (dict(variant=7), UNSUPPORTED),
        (dict(net=S1, n_steps=0, flags=0, out=0), UNSUPPORTED, VARIANT6),
        (dict(net=REF, n_steps=0, flags=0, out=0), UNSUPPORTED, BL6_ONLY),
        # the other checks come before the variant
        (dict(net=S1, out=0), BADARG), (dict(net=REF, step0=1), BADARG), (dict(net=S1, image=0), BADARG),
]


def test_swn_decode_chunk_w16():
    _run(_chunk("w16"), CHUNK_IMAGE, WORD["w16"])


def test_swn_decode_chunk_w8():
    _run(_chunk("w8"), CHUNK_IMAGE, WORD["w8"])


# ---------------------------------------------------------------------------------------------------------------------- pool
def _entry(slot=0, step0=0, n_steps=4, flags=1, frames=4, cond=1, reserved=0):
    return _lib.DecodePoolEntry(cond_dev=cond or None, n_frames=frames, slot=slot, step0=step0, n_steps=n_steps, flags=flags,
                                reserved=reserved)


IDLE = [dict(slot=0, step0=5, n_steps=0, flags=0), dict(slot=1, n_steps=0, flags=0)]      # no work in any entry


def _pool(kind):
    """kind: "fp32" (swn_decode_pool_chunk), "w16" / "w8" (swn_decode_pool_chunk_w16 / _w8) or "models"
    (swn_decode_pool_chunk_models)"""
    def call(net=SMX, variant=0, packed=1, capacity=2, entries=(dict(),), n_entries=None, table=1, io=1, session=1, out=1,
             image=1, desc=1, models=(1, 2), n_models=None, of=None, null_models=False, null_of=False):
        lib, d = _lib.lib(), _lib.desc_from_cfg(net)
        E = len(entries) if n_entries is None else n_entries
        rows = [_entry(**e) for e in entries]
        rows += [_entry(slot=len(rows) + k) for k in range(E - len(rows))]     # a table as long as the call says it is
        tab = (_lib.DecodePoolEntry * max(1, len(rows)))(*rows) if table else None
        io = ctypes.byref(io if isinstance(io, _lib.DecodeIO) else _io()) if io else None
        tail = [capacity, tab, E, io, _p(session), _p(out), None, variant]
        if kind == "fp32":
            return lib.swn_decode_pool_chunk(ctypes.byref(d) if desc else None, _p(packed), *tail, None)
        if kind in WORD:
            return getattr(lib, "swn_decode_pool_chunk_" + kind)(ctypes.byref(d) if desc else None, _p(packed), *tail, _p(image),
                                                                 None)
        of = [e % len(models) for e in range(max(1, len(rows)))] if of is None else of
        ptrs = None if null_models else (ctypes.c_void_p * max(1, len(models)))(*[m or None for m in models])
        idx = None if null_of else (ctypes.c_int32 * max(1, len(of)))(*of)
        return lib.swn_decode_pool_chunk_models(ctypes.byref(d) if desc else None, ptrs,
                                                len(models) if n_models is None else n_models, idx, *tail, None)
    return call


POOL_COMMON = [
    (dict(desc=0), BADARG), (dict(table=0), BADARG), (dict(io=0), BADARG), (dict(session=0), BADARG), (dict(out=0), BADARG),
    (dict(capacity=0), BADARG), (dict(n_entries=0), BADARG), (dict(n_entries=-1, table=1, entries=()), BADARG),
    (dict(n_entries=MAX_ENTRIES + 1, capacity=MAX_ENTRIES + 1), BADARG),
    (dict(io=_io(noise=1)), BADARG), (dict(io=_io(forced=1)), BADARG),       # pools draw their noise, no teacher forcing
    (dict(entries=[dict(cond=0)]), BADARG), (dict(entries=[dict(frames=0)]), BADARG), (dict(entries=[dict(slot=-1)]), BADARG),
    (dict(entries=[dict(slot=2)]), BADARG), (dict(entries=[dict(slot=1)], capacity=1), BADARG),
    (dict(entries=[dict(step0=-1, flags=0)]), BADARG), (dict(entries=[dict(n_steps=-1)]), BADARG),
    (dict(entries=[dict(flags=2)]), BADARG), (dict(entries=[dict(flags=3)]), BADARG), (dict(entries=[dict(reserved=1)]), BADARG),
    (dict(entries=[dict(step0=1)]), BADARG),               # BEGIN starts at step 0
    (dict(entries=[dict(n_steps=4 * 80 + 1)]), BADARG),    # past the entry's conditioning
    (dict(entries=[dict(step0=4 * 80 - 3, flags=0)]), BADARG), (dict(entries=[dict(step0=4 * 80 + 1, n_steps=0, flags=0)]), BADARG),
    (dict(entries=[dict(slot=1), dict(slot=1)]), BADARG),  # two entries on one session
    (dict(entries=[dict(slot=0), dict(slot=1), dict(slot=0, flags=0, n_steps=0)], capacity=3), BADARG),
    (dict(entries=[dict(slot=0), dict(slot=1, reserved=7)]), BADARG),       # every entry is checked, not the first alone
    (dict(entries=IDLE + [dict(slot=2)], capacity=3, out=0), BADARG),        # one entry with work wants `out`
    # no entry has work: SWN_OK once the variant has resolved, without `out`
    (dict(entries=IDLE, out=0), OK), (dict(net=S1, variant=6, entries=IDLE, out=0), OK), (dict(net=S5, entries=IDLE, variant=2), OK),
    (dict(entries=IDLE, session=0), BADARG), (dict(entries=[dict(slot=0, n_steps=0, flags=0)] * 2), BADARG),
]
# variant 3 and nets that resolve to the stepped chain are unsupported, every other unresolvable variant a bad argument
POOL_FP32 = [
    (dict(entries=IDLE, out=0, variant=1), OK), (dict(net=S1, entries=IDLE, out=0), OK), (dict(net=TINY, entries=IDLE, out=0), OK),
    (dict(variant=3), UNSUPPORTED), (dict(net=TINY, variant=3), UNSUPPORTED), (dict(net=REF), UNSUPPORTED),
    (dict(net=REF, variant=3), UNSUPPORTED), (dict(net=REF, entries=IDLE, out=0), UNSUPPORTED),
    (dict(entries=IDLE, out=0, variant=3), UNSUPPORTED),
    (dict(net=REF, variant=2), BADARG), (dict(net=REF, variant=6), BADARG), (dict(net=TINY, variant=2), BADARG),
    (dict(variant=4), BADARG), (dict(variant=-1), BADARG), (dict(variant=7), BADARG),
    (dict(net=REF, variant=2, entries=IDLE, out=0), BADARG), (dict(variant=5, entries=IDLE, out=0), BADARG),
    # the other checks come before the variant
    (dict(net=REF, out=0), BADARG), (dict(variant=3, entries=[dict(slot=2)]), BADARG),
]


def test_swn_decode_pool_chunk():
    _run(_pool("fp32"), POOL_COMMON + POOL_FP32 + [(dict(packed=0), BADARG), (dict(packed=0, entries=IDLE), BADARG)])


def test_swn_decode_pool_chunk_models():
    _run(_pool("models"), POOL_COMMON + POOL_FP32 + [
        (dict(packed=0, entries=IDLE, out=0), OK),                           # `packed` is not an argument of this call
        (dict(n_models=0), BADARG), (dict(n_models=-1), BADARG),
        (dict(models=list(range(1, MAX_MODELS + 2)), of=[MAX_MODELS]), BADARG),
        (dict(null_models=True), BADARG), (dict(null_of=True), BADARG),
        (dict(models=(1, 0)), BADARG), (dict(models=(1, 0, 3), of=[2]), BADARG),      # a null model, named or not
        (dict(of=[2]), BADARG), (dict(of=[-1]), BADARG), (dict(entries=[dict(slot=0), dict(slot=1)], of=[0, 2]), BADARG),
        (dict(n_models=0, entries=IDLE, out=0), BADARG), (dict(of=[2, 0], entries=IDLE, out=0), BADARG),
        (dict(models=list(range(1, MAX_MODELS + 1)), of=[MAX_MODELS - 1, 0], entries=IDLE, out=0), OK),
        # the model checks come before the variant
        (dict(net=REF, of=[2]), BADARG), (dict(variant=3, n_models=0), BADARG),
    ])


POOL_IMAGE = POOL_COMMON + [
        (dict(packed=0), BADARG), (dict(image=0), BADARG), (dict(image=0, entries=IDLE), BADARG),
        # what does not resolve to the symmetric kernel is unsupported, with the detail text, with or without work
        (dict(net=S1), UNSUPPORTED, VARIANT6), (dict(net=S1, variant=2), UNSUPPORTED, VARIANT6),
        (dict(net=S5, variant=1), UNSUPPORTED, "generic"), (dict(variant=3), UNSUPPORTED, BL6_ONLY),
        (dict(net=REF), UNSUPPORTED, "stepped"), (dict(net=REF, variant=2), UNSUPPORTED, BL6_ONLY),
        (dict(net=REF, variant=6), UNSUPPORTED, BL6_ONLY), (dict(net=TINY), UNSUPPORTED, BL6_ONLY),
        (dict(variant=4), UNSUPPORTED, BL6_ONLY), (dict(variant=-1), UNSUPPORTED, BL6_ONLY), (dict(variant=7), UNSUPPORTED),
        (dict(net=S1, entries=IDLE, out=0), UNSUPPORTED, VARIANT6), (dict(net=REF, entries=IDLE, out=0), UNSUPPORTED, BL6_ONLY),
        # the other checks come before the variant
        (dict(net=REF, out=0), BADARG), (dict(net=S1, entries=[dict(slot=2)]), BADARG), (dict(net=S1, image=0), BADARG),
]


def test_swn_decode_pool_chunk_w16():
    _run(_pool("w16"), POOL_IMAGE, WORD["w16"])


def test_swn_decode_pool_chunk_w8():
    _run(_pool("w8"), POOL_IMAGE, WORD["w8"])


@pytest.mark.parametrize("name", sorted(NETS))
def test_the_size_queries_agree_with_the_resolved_kernel(name):
    """swn_decode_session_floats is 0 exactly where swn_decode_resolve_variant refuses; swn_decode_state_floats covers the
    generic and the stepped kernel at every batch"""
    lib, d = _lib.lib(), _lib.desc_from_cfg(NETS[name])
    for variant in (-1, 0, 1, 2, 3, 4, 6, 7):
        for batch in (0, 1, 3):
            k = lib.swn_decode_resolve_variant(ctypes.byref(d), batch, variant)
            n = lib.swn_decode_session_floats(ctypes.byref(d), batch, variant)
            assert (n > 0) == (k > 0), (variant, batch, k, n)
            if k > 0 and batch == 3:
                assert n == 3 * lib.swn_decode_session_floats(ctypes.byref(d), 1, variant) or k == 3
            if k in (1, 3):
                assert lib.swn_decode_state_floats(ctypes.byref(d), batch) > 0
    assert lib.swn_decode_state_floats(ctypes.byref(d), 0) == 0 and lib.swn_decode_session_floats(None, 1, 0) == 0
