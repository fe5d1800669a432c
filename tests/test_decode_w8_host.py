"""CPU: FP8 (OCP E4M3) storage of the streamed head matrices (weights="e4m3") - the host quantiser against a reference built
from the format's definition, the bounds the definition implies, the new entry points of the C ABI and every refusal that is
decided before a device is touched."""
import ctypes
import math
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops
from shallow_wavenet_amd import runtime as R
from shallow_wavenet_amd.runtime import (bf16_weight_names, check_decode_weights, e4m3_quantise, e4m3_weight_state_dict)
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream, SteppedDecodePool, SteppedModelPool
from shallow_wavenet_amd.synth import synth_state_dict

NEW_SYMBOLS = ("swn_decode_w8_bytes", "swn_pack_decode_w8", "swn_decode_w8", "swn_decode_chunk_w8", "swn_decode_pool_chunk_w8",
               "swn_e4m3_table")


# ------------------------------------------------------------------------------------------------------------- reference
def _format_value(code: int) -> float:
    """OCP E4M3FN from its definition, in float64: 1 sign, 4 exponent (bias 7), 3 fraction bits; exponent field 0 holds the
    subnormals fraction x 2^-9; 0x7f / 0xff are NaN; no infinities"""
    ex, fr = (code >> 3) & 15, code & 7
    if ex == 15 and fr == 7:
        return math.nan
    mag = fr * 2.0 ** -9 if ex == 0 else (1 + fr / 8.0) * 2.0 ** (ex - 7)
    return -mag if code & 0x80 else mag


GRID = np.array([_format_value(c) for c in range(0x7f)])     # the 127 non-negative finite values, rising with the code


def test_the_format_has_253_finite_values_up_to_448():
    finite = {_format_value(c) for c in range(256) if not math.isnan(_format_value(c))}
    assert len(finite) == 253 and max(finite) == 448.0 and min(v for v in finite if v > 0) == 2.0 ** -9
    assert np.all(np.diff(GRID) > 0)
    assert np.array_equal(R.e4m3_values()[np.arange(256) & 0x7f != 0x7f].astype(np.float64),
                          np.array([_format_value(c) for c in range(256) if c & 0x7f != 0x7f]))
    assert np.isnan(R.e4m3_values()[[0x7f, 0xff]]).all()


def _ref_exponent(amax: float) -> int:
    if amax == 0:
        return 0
    m, x = math.frexp(amax)
    return max(-100, min(100, 9 - x if m <= 0.875 else 8 - x))


def _ref_quantise(w):
    """search over the grid in float64: nearest value, a tie to the even code; the sign bit of the input is kept"""
    w = np.asarray(w, dtype=np.float32)
    rows = w.reshape(w.shape[0], -1).astype(np.float64)
    e = np.array([_ref_exponent(float(np.abs(r).max())) for r in rows], dtype=np.int32)
    a = np.abs(rows) * 2.0 ** e.astype(np.float64)[:, None]
    d = np.abs(a[:, :, None] - GRID[None, None, :])
    k = d.argmin(axis=2)                                     # the lower code of a tie
    nxt = np.minimum(k + 1, len(GRID) - 1)
    tie = (np.take_along_axis(d, nxt[:, :, None], 2)[:, :, 0] == np.take_along_axis(d, k[:, :, None], 2)[:, :, 0]) & (nxt != k)
    k = np.where(tie & (k % 2 == 1), nxt, k)
    return (k | (np.signbit(rows) << 7)).astype(np.uint8).reshape(w.shape), e


def _check(w):
    codes, e = e4m3_quantise(w)
    want_codes, want_e = _ref_quantise(w)
    assert codes.dtype == np.uint8 and e.dtype == np.int32 and codes.shape == np.shape(w) and e.shape == (np.shape(w)[0],)
    assert np.array_equal(e, want_e), (e, want_e)
    assert np.array_equal(codes, want_codes), np.argwhere(codes != want_codes)[:5]
    assert not np.any((codes & 0x7f) == 0x7f)                # a NaN code is never produced
    return codes, e


# -------------------------------------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("seed,scale", [(0, 1.0), (1, 0.05), (2, 3e-4), (3, 7e3), (4, 1e-30), (5, 1e30)])
def test_quantiser_equals_the_reference_on_random_rows(seed, scale):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((48, 64)) * scale * np.exp(rng.uniform(-6, 6, (48, 64)))).astype(np.float32)
    w[rng.random(w.shape) < 0.02] = 0.0
    w[3, 5] = -0.0
    _check(w)


def test_quantiser_on_the_constructed_cases():
    z = np.zeros(8, dtype=np.float32)

    def row(*v):
        r = z.copy()
        r[:len(v)] = v
        return r

    below, above = np.nextafter(np.float32(0.875), np.float32(0)), np.nextafter(np.float32(0.875), np.float32(1))
    w = np.stack([
        row(56.0, -56.0, 7.0),                               # 0: amax = 448 x 2^-3 exactly -> the largest code
        row(0.875 * 2.0 ** -5, 1e-3),                        # 1: m = 0.875 -> e = 9 - x
        row(below * 2.0 ** 4, 1.0),                          # 2: m just below 0.875 -> e = 9 - x, top binade
        row(above * 2.0 ** 4, 1.0),                          # 3: m just above -> e = 8 - x: the row scales to 224 ..
        row(32.0, 17 / 8, 19 / 8, -17 / 8, 21 / 8, 23 / 8),  # 4: e = 3: 17, 19, 21, 23 are ties in the binade [16, 32)
        row(256.0, 1.5 * 2.0 ** -9, 0.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, -3.5 * 2.0 ** -9, 7.5 * 2.0 ** -9),   # 5: e = 0: subnormal ties
        row(256.0, 0.49 * 2.0 ** -9, -0.49 * 2.0 ** -9, 2.0 ** -11, -2.0 ** -30, -0.0, 0.0),   # 6: below 2^-10: signed zeros
        z,                                                   # 7: all zero
        row(-0.0, 0.0, -0.0),                                # 8: all zero, the signs stay
        row(2.0 ** -105, -2.0 ** -107, 2.0 ** -120),         # 9: e = 113 clamped to 100
        row(2.0 ** -120, -2.0 ** -121),                      # 10: clamped, everything below 2^-10: signed zeros
        row(1.0),                                            # 11: a single 1: m = 0.5 -> 2^8 = 256
    ]).astype(np.float32)
    codes, e = _check(w)
    assert e.tolist() == [3, 14, 5, 4, 3, 0, 0, 0, 0, 100, 100, 8]
    assert codes[0, :3].tolist() == [0x7e, 0xfe, 0x66]                                  # 448, -448, 56
    assert codes[1, 0] == 0x7e and codes[2, 0] == 0x7e and codes[3, 0] == 0x76          # 448, 448 (rounded up), 224
    assert R.e4m3_values()[codes[4, :6]].tolist() == [256.0, 16.0, 20.0, -16.0, 20.0, 24.0]   # ties to the even fraction
    assert codes[5, 1:6].tolist() == [2, 0, 2, 0x84, 8]                                 # 1.5 -> 2, 0.5 -> 0, 2.5 -> 2, -3.5 -> -4, 7.5 -> 2^-6
    assert codes[6, 1:7].tolist() == [0, 0x80, 0, 0x80, 0x80, 0]
    assert codes[7].tolist() == [0] * 8 and codes[8, :3].tolist() == [0x80, 0, 0x80]
    assert R.e4m3_values()[codes[9, :3]].tolist() == [2.0 ** -5, -2.0 ** -7, 0.0]
    assert codes[10, :2].tolist() == [0, 0x80]
    assert codes[11, 0] == 0x78                                                          # 256 = 1.0 x 2^8
    for bad in (np.nan, np.inf, -np.inf):
        v = w.copy()
        v[4, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            e4m3_quantise(v)
        with pytest.raises(ValueError, match="not finite"):
            e4m3_quantise(torch.from_numpy(v))


def test_dequantised_weights_keep_the_bounds_of_the_definition():
    rng = np.random.default_rng(9)
    w = (rng.standard_normal((64, 256)) * np.exp(rng.uniform(-8, 2, (64, 256)))).astype(np.float32)
    w[5] = 0.0
    w[6] *= np.float32(2.0 ** -118)                          # clamped
    codes, e = e4m3_quantise(w)
    deq = R.e4m3_dequantise(codes, e)
    assert deq.dtype == np.float32
    up = 2.0 ** e.astype(np.float64)[:, None]
    finite = set(GRID.tolist())
    assert all(abs(v) in finite for v in (deq.astype(np.float64) * up).ravel())          # W^ 2^e is an E4M3 value
    aw, err = np.abs(w.astype(np.float64)), np.abs(deq.astype(np.float64) - w.astype(np.float64))
    normal = aw * up >= 2.0 ** -6
    assert np.all(err[normal] <= 2.0 ** -4 * aw[normal])                                 # half a step of 3 fraction bits
    assert np.all((err <= 2.0 ** -10 / up)[~normal])                                     # half a subnormal step
    top = np.abs(R.e4m3_values()[codes]).max(axis=1)
    for r in range(w.shape[0]):
        if r == 5:
            assert top[r] == 0 and e[r] == 0
        elif r == 6:
            assert e[r] == 100 and top[r] < 224
        else:
            assert 224 <= top[r] <= 448, (r, top[r])
    assert np.array_equal(np.signbit(deq), np.signbit(w))


@pytest.mark.parametrize("cfg", [C.bl6_softmax(), C.bl6_laplace(5, 4), C.bl6_laplace(1, 0)],
                         ids=["softmax", "lap_s5l4", "lap_s1l0"])
def test_state_dict_helper_changes_exactly_the_named_tensors(cfg):
    sd = synth_state_dict(cfg, seed=3, flavor="xavier")
    names = bf16_weight_names(cfg)
    got = e4m3_weight_state_dict(cfg, sd)
    assert list(got) == list(sd)
    for k, v in sd.items():
        if k in names:
            codes, e = _ref_quantise(v)
            want = np.array([_format_value(int(c)) for c in codes.ravel()]).reshape(v.shape[0], -1) * 2.0 ** -e.astype(np.float64)[:, None]
            assert got[k].dtype == np.float32 and got[k].shape == v.shape
            assert np.array_equal(got[k].astype(np.float64).reshape(v.shape[0], -1), want), k
            assert not np.array_equal(got[k], v), k          # synthetic weights are not E4M3 values: every matrix moved
        else:
            assert got[k] is v, k                            # untouched, not even copied (biases, Laplace out_2 among them)
    got_t = e4m3_weight_state_dict(cfg, {k: torch.from_numpy(v) for k, v in sd.items()})
    for k in names:
        assert isinstance(got_t[k], torch.Tensor) and got_t[k].dtype == torch.float32
        assert np.array_equal(got_t[k].numpy(), got[k])
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    assert all(e4m3_weight_state_dict(cfg, tsd)[k] is tsd[k] for k in tsd if k not in names)
    with pytest.raises(KeyError):
        e4m3_weight_state_dict(cfg, {k: v for k, v in sd.items() if k != "out_1.weight"})
    bad = dict(sd)
    bad["out_1.weight"] = sd["out_1.weight"].copy()
    bad["out_1.weight"][1, 2, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        e4m3_weight_state_dict(cfg, bad)


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_w8_symbols_are_exported_bound_and_registered():
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.swn_abi_version() == 3
    for op in ("pack_decode_w8", "decode_w8", "decode_chunk_w8", "decode_pool_chunk_w8", "e4m3_table"):
        assert op in ops.OP_NAMES, op
        assert hasattr(torch.ops.swn, op)
    for op in ("decode_chunk_w8", "decode_pool_chunk_w8"):
        schema = str(getattr(torch.ops.swn, op).default._schema)
        assert re.search(r"Tensor\(a\d*!\) session", schema), schema
    assert R.DECODE_WEIGHTS == ("fp32", "bf16", "e4m3")


def test_fake_implementations_give_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    cfg = C.bl6_softmax()
    dlist = ops.desc_list(cfg)
    need = _lib.lib().swn_decode_w8_bytes(ctypes.byref(_lib.desc_from_cfg(cfg)))
    with FakeTensorMode():
        packed = torch.empty(16, dtype=torch.float32)
        w8 = torch.ops.swn.pack_decode_w8(packed, dlist)
        assert w8.dtype == torch.uint8 and w8.shape == (need,)
        assert torch.ops.swn.e4m3_table(packed, 1.0).shape == (256,)
        cond = torch.empty(2, 3, 8, dtype=torch.float32)
        out, heads, used = torch.ops.swn.decode_w8(packed, w8, cond, None, None, None, dlist, 5, 0, 1, 0, True, False)
        assert out.shape == (2, 5) and out.dtype == torch.int32 and heads.shape == (2, 5, 256) and used.shape == (0,)
        sess = torch.empty(8, dtype=torch.float32)
        out, heads, _ = torch.ops.swn.decode_chunk_w8(packed, w8, cond, sess, None, None, None, dlist, 0, 4, True, 0, 1, 0,
                                                      False, False)
        assert out.shape == (2, 4) and heads.shape == (0,)
        out, _, _ = torch.ops.swn.decode_pool_chunk_w8(packed, w8, sess, [cond[0], cond[1]], [0, 1], [0, 0], [3, 7],
                                                       [True, True], None, [0, 1], dlist, 2, 0, 1, False, False)
        assert out.shape == (2, 7)


def test_image_size_query():
    lib = _lib.lib()
    size = lambda cfg: lib.swn_decode_w8_bytes(ctypes.byref(_lib.desc_from_cfg(cfg)))
    assert size(C.ref6_laplace()) == 0 and size(C.ref6_softmax()) == 0 and size(C.tiny("laplace", 2, 4)) == 0
    assert size(C.bl6_laplace(10, 4)) == 0                  # BL6-shaped, but no symmetric kernel at seg 10
    assert lib.swn_decode_w8_bytes(None) == 0
    # one byte per weight plus four per row
    assert size(C.bl6_softmax()) == (6 * 256 * 64 + 256 * 256 + 256 * 256) + 4 * (6 * 256 + 256 + 256)
    for seg, lpc in ((1, 0), (1, 4), (2, 4), (5, 0), (5, 4)):
        assert size(C.bl6_laplace(seg, lpc)) == (6 * 128 * 64 + 128 * 128) + 4 * (6 * 128 + 128)


def _io(noise=0, forced=0):
    return _lib.DecodeIO(noise_dev=noise or None, forced_dev=forced or None, seed_dev=None, noise_out_dev=None, rng_seed=1,
                         rng_utt0=0, reserved=0, rng_utt_ids_dev=None)


def _p(v):
    return ctypes.c_void_p(v) if v else None


def test_calls_check_their_arguments_before_any_launch():
    """fake non-null addresses: every one of these is refused before the library touches them (the checks of the _w16 calls)"""
    lib = _lib.lib()
    detail = lambda: lib.swn_last_error_detail().decode()
    smx, s1, s5, ref = (_lib.desc_from_cfg(c) for c in (C.bl6_softmax(), C.bl6_laplace(1, 4), C.bl6_laplace(5, 4), C.ref6_laplace()))

    def dec(d, variant=0, w8=1, packed=1, out=1, n_steps=4):
        return lib.swn_decode_w8(ctypes.byref(d), _p(packed), _p(1), 1, 4, n_steps, ctypes.byref(_io()), None, _p(out), None,
                                 variant, _p(w8), None)

    def chunk(d, variant=0, w8=1, session=1, step0=0, flags=1):
        return lib.swn_decode_chunk_w8(ctypes.byref(d), _p(1), _p(1), 1, 4, step0, 4, flags, ctypes.byref(_io()), _p(session),
                                       _p(1), None, variant, _p(w8), None)

    def pool(d, variant=0, w8=1, slot=0, io=None, capacity=2):
        en = (_lib.DecodePoolEntry * 1)(_lib.DecodePoolEntry(cond_dev=1, n_frames=4, slot=slot, step0=0, n_steps=4, flags=1,
                                                             reserved=0))
        return lib.swn_decode_pool_chunk_w8(ctypes.byref(d), _p(1), capacity, en, 1, ctypes.byref(io or _io()), _p(1), _p(1),
                                            None, variant, _p(w8), None)

    for call in (dec, chunk, pool):
        assert call(smx, w8=0) == -2                        # SWN_E_BADARG: no image
        assert call(s1, variant=0) == -4                    # SWN_E_UNSUPPORTED: the wave-specialised kernel takes variant 0
        assert "variant = 6" in detail() and "e4m3" in detail()
        assert call(s1, variant=2) == -4 and "variant = 6" in detail()
        assert call(s5, variant=1) == -4 and "generic" in detail()        # the generic kernel
        assert call(s5, variant=3) == -4
        assert call(ref, variant=0) == -4 and "stepped" in detail()
        assert call(ref, variant=6) == -4
    assert dec(smx, packed=0) == -2 and dec(smx, out=0) == -2
    assert dec(smx, n_steps=4 * 80 + 1) == -2               # past the conditioning
    assert dec(smx, n_steps=0, packed=0, out=0) == 0        # nothing to generate
    assert chunk(smx, session=0) == -2 and chunk(smx, step0=1) == -2 and chunk(smx, flags=2) == -2
    assert pool(smx, slot=2) == -2 and pool(smx, io=_io(noise=1)) == -2 and pool(smx, io=_io(forced=1)) == -2
    assert lib.swn_pack_decode_w8(ctypes.byref(smx), None, _p(1), None) == -2
    assert lib.swn_pack_decode_w8(ctypes.byref(smx), _p(1), None, None) == -2
    assert lib.swn_pack_decode_w8(ctypes.byref(ref), _p(1), _p(1), None) == -4
    assert lib.swn_e4m3_table(None, 1.0, None) == -2


# ---------------------------------------------------------------------------------------------------------------- Python
def _fake_net(cfg):
    return SimpleNamespace(cfg=cfg, dlist=ops.desc_list(cfg), device=torch.device("cpu"), packed=None)


def _outcome(f):
    try:
        return ("ok", f())
    except ValueError as ex:
        return ("ValueError", str(ex))


def test_weights_keyword_is_checked_on_the_host_as_for_bf16():
    assert check_decode_weights("e4m3", C.bl6_softmax(), 3, 0) == "e4m3"
    assert check_decode_weights("e4m3", C.bl6_laplace(5, 4), 1, 6) == "e4m3"
    assert check_decode_weights("e4m3", C.bl6_laplace(1, 4), 2, 6) == "e4m3"
    for bad in ("fp8", "e5m2", "E4M3", None, 8):
        with pytest.raises(ValueError, match="weights must be one of"):
            check_decode_weights(bad, C.bl6_softmax(), 1, 0)
        with pytest.raises(ValueError, match="weights must be one of"):
            DecodeStream(_fake_net(C.bl6_softmax()), 1, weights=bad)
    # every (net, batch, variant): the outcome of "e4m3" is that of "bf16", the messages with the mode's name
    cfgs = (C.bl6_softmax(), C.bl6_laplace(1, 0), C.bl6_laplace(1, 4), C.bl6_laplace(2, 4), C.bl6_laplace(5, 0), C.bl6_laplace(5, 4),
            C.bl6_laplace(10, 4), C.ref6_laplace(), C.ref6_softmax(), C.tiny("laplace", 2, 4))
    accepted = 0
    for cfg in cfgs:
        for batch in (1, 3):
            for v in (0, 1, 2, 3, 6):
                a = _outcome(lambda: check_decode_weights("bf16", cfg, batch, v))
                b = _outcome(lambda: check_decode_weights("e4m3", cfg, batch, v))
                assert a[0] == b[0], (cfg, batch, v)
                assert b[1] == a[1].replace("bf16", "e4m3"), (cfg, batch, v)
                for cls in (DecodeStream, DecodePool):
                    a = _outcome(lambda: cls(_fake_net(cfg), 2, variant=v, weights="bf16").weights)
                    b = _outcome(lambda: cls(_fake_net(cfg), 2, variant=v, weights="e4m3").weights)
                    assert a[0] == b[0] and b[1] == a[1].replace("bf16", "e4m3"), (cfg, cls, v)
                    accepted += a[0] == "ok"
    assert accepted > 0
    for cfg in (C.bl6_laplace(1, 0), C.bl6_laplace(1, 4)):
        for v in (0, 2):
            with pytest.raises(ValueError, match="variant=6"):
                DecodeStream(_fake_net(cfg), 2, variant=v, weights="e4m3")
        assert DecodeStream(_fake_net(cfg), 2, variant=6, weights="e4m3").weights == "e4m3"
    with pytest.raises(ValueError, match="symmetric BL6"):
        DecodePool(_fake_net(C.ref6_laplace()), 2, weights="e4m3")
    for cls in (SteppedDecodePool, SteppedModelPool):
        with pytest.raises(ValueError, match="stepped"):
            cls(_fake_net(C.ref6_laplace()), 2, weights="e4m3")
        with pytest.raises(ValueError, match="weights must be one of"):
            cls(_fake_net(C.ref6_laplace()), 2, weights="fp8")


def test_modules_and_driver_carry_the_mode():
    from shallow_wavenet_amd import decode_driver as DD
    from shallow_wavenet_amd.nets import _engine
    from shallow_wavenet_amd.nets import dswnv as md
    m = md.DSWNV(**C.tiny("softmax", wav_conv_flag=False).ctor_kwargs())
    m.decode_weights = "e4m3"
    assert _engine.resolve_decode_weights(m) == "e4m3"
    assert _engine.decode_weight_kwargs(m) == {"weights": "e4m3", "variant": 6}
    assert DD._weights_variant(m) == 6
    m.decode_weights = "fp8"
    with pytest.raises(ValueError, match="decode_weights"):
        _engine.resolve_decode_weights(m)
    p = DD.make_parser()
    base = ["--feats", "f", "--checkpoint", "c", "--config", "j", "--outdir", "o"]
    assert p.parse_args(base + ["--weights", "e4m3"]).weights == "e4m3"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--weights", "fp8"])
    assert "e4m3" in next(a.help for a in p._actions if a.dest == "weights")
