"""CPU: bf16 storage of the streamed head matrices (weights="bf16") - the host rounding helper, the new entry points of the
C ABI and every refusal that is decided before a device is touched."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops
from shallow_wavenet_amd.runtime import bf16_weight_names, bf16_weight_state_dict, check_decode_weights
from shallow_wavenet_amd.streaming import DecodePool, DecodeStream, SteppedDecodePool, SteppedModelPool
from shallow_wavenet_amd.synth import synth_state_dict

NEW_SYMBOLS = ("swn_decode_w16_bytes", "swn_pack_decode_w16", "swn_decode_w16", "swn_decode_chunk_w16",
               "swn_decode_pool_chunk_w16")


def _round(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize("cfg", [C.bl6_softmax(), C.bl6_laplace(5, 4), C.bl6_laplace(1, 0)],
                         ids=["softmax", "lap_s5l4", "lap_s1l0"])
def test_state_dict_helper_rounds_exactly_the_named_tensors(cfg):
    sd = synth_state_dict(cfg, seed=3, flavor="xavier")
    names = bf16_weight_names(cfg)
    want = [f"out_skip.{l}.weight" for l in range(cfg.L)] + ["out_1.weight"] + (["out_2.weight"] if cfg.kind == "softmax" else [])
    assert names == want
    got = bf16_weight_state_dict(cfg, sd)
    assert list(got) == list(sd)
    changed = 0
    for k, v in sd.items():
        if k in names:
            assert got[k].dtype == np.float32 and np.array_equal(got[k], _round(v)), k
            changed += int(not np.array_equal(got[k], v))
        else:
            assert got[k] is v, k                           # untouched, not even copied (Laplace out_2 among them)
    assert changed == len(names)                            # synthetic weights are not bf16 values: every one moved
    if cfg.kind == "laplace":
        assert "out_2.weight" not in names and got["out_2.weight"] is sd["out_2.weight"]
    # tensors in, tensors out, the same values
    got_t = bf16_weight_state_dict(cfg, {k: torch.from_numpy(v) for k, v in sd.items()})
    for k in names:
        assert isinstance(got_t[k], torch.Tensor) and got_t[k].dtype == torch.float32
        assert np.array_equal(got_t[k].numpy(), got[k])
    with pytest.raises(KeyError):
        bf16_weight_state_dict(cfg, {k: v for k, v in sd.items() if k != "out_1.weight"})


def test_state_dict_helper_rounds_ties_to_even():
    cfg = C.bl6_softmax()
    sd = {k: v.copy() for k, v in synth_state_dict(cfg, seed=3, flavor="xavier").items()}
    w = sd["out_1.weight"]
    # bf16 keeps 7 fraction bits: 1 + k / 256 with odd k lies exactly between two bf16 values
    w[0, :6, 0] = [1 + 1 / 256, 1 + 3 / 256, -(1 + 1 / 256), -(1 + 3 / 256), 1 + 1 / 256 + 2.0 ** -20, 1 + 3 / 256 - 2.0 ** -20]
    got = bf16_weight_state_dict(cfg, sd)["out_1.weight"][0, :6, 0]
    assert got.tolist() == [1.0, 1 + 2 / 128, -1.0, -(1 + 2 / 128), 1 + 1 / 128, 1 + 1 / 128]


def test_w16_symbols_are_exported_bound_and_registered():
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.swn_abi_version() == 3
    for op in ("pack_decode_w16", "decode_w16", "decode_chunk_w16", "decode_pool_chunk_w16"):
        assert op in ops.OP_NAMES, op
    for op in ("decode_chunk_w16", "decode_pool_chunk_w16"):
        schema = str(getattr(torch.ops.swn, op).default._schema)
        assert re.search(r"Tensor\(a\d*!\) session", schema), schema


def test_image_size_query():
    lib = _lib.lib()
    size = lambda cfg: lib.swn_decode_w16_bytes(ctypes.byref(_lib.desc_from_cfg(cfg)))
    assert size(C.ref6_laplace()) == 0 and size(C.ref6_softmax()) == 0 and size(C.tiny("laplace", 2, 4)) == 0
    assert size(C.bl6_laplace(10, 4)) == 0                  # BL6-shaped, but no symmetric kernel at seg 10
    assert lib.swn_decode_w16_bytes(None) == 0
    # out_skip 6 x S x 64, out_1 O1 x S, softmax out_2 Q x Q - two bytes each
    assert size(C.bl6_softmax()) == 2 * (6 * 256 * 64 + 256 * 256 + 256 * 256)
    for seg, lpc in ((1, 0), (1, 4), (2, 4), (5, 0), (5, 4)):
        assert size(C.bl6_laplace(seg, lpc)) == 2 * (6 * 128 * 64 + 128 * 128)


def _io(noise=0, forced=0):
    return _lib.DecodeIO(noise_dev=noise or None, forced_dev=forced or None, seed_dev=None, noise_out_dev=None, rng_seed=1,
                         rng_utt0=0, reserved=0, rng_utt_ids_dev=None)


def _p(v):
    return ctypes.c_void_p(v) if v else None


def test_calls_check_their_arguments_before_any_launch():
    """fake non-null addresses: every one of these is refused before the library touches them"""
    lib = _lib.lib()
    detail = lambda: lib.swn_last_error_detail().decode()
    smx, s1, s5, ref = (_lib.desc_from_cfg(c) for c in (C.bl6_softmax(), C.bl6_laplace(1, 4), C.bl6_laplace(5, 4), C.ref6_laplace()))

    def dec(d, variant=0, w16=1, packed=1, out=1, n_steps=4):
        return lib.swn_decode_w16(ctypes.byref(d), _p(packed), _p(1), 1, 4, n_steps, ctypes.byref(_io()), None, _p(out), None,
                                  variant, _p(w16), None)

    def chunk(d, variant=0, w16=1, session=1, step0=0, flags=1):
        return lib.swn_decode_chunk_w16(ctypes.byref(d), _p(1), _p(1), 1, 4, step0, 4, flags, ctypes.byref(_io()), _p(session),
                                        _p(1), None, variant, _p(w16), None)

    def pool(d, variant=0, w16=1, slot=0, io=None, capacity=2):
        en = (_lib.DecodePoolEntry * 1)(_lib.DecodePoolEntry(cond_dev=1, n_frames=4, slot=slot, step0=0, n_steps=4, flags=1,
                                                             reserved=0))
        return lib.swn_decode_pool_chunk_w16(ctypes.byref(d), _p(1), capacity, en, 1, ctypes.byref(io or _io()), _p(1), _p(1),
                                             None, variant, _p(w16), None)

    for call in (dec, chunk, pool):
        assert call(smx, w16=0) == -2                       # SWN_E_BADARG: no image
        assert call(s1, variant=0) == -4                    # SWN_E_UNSUPPORTED: the wave-specialised kernel takes variant 0
        assert "variant = 6" in detail()
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
    assert lib.swn_pack_decode_w16(ctypes.byref(smx), None, _p(1), None) == -2
    assert lib.swn_pack_decode_w16(ctypes.byref(smx), _p(1), None, None) == -2
    assert lib.swn_pack_decode_w16(ctypes.byref(ref), _p(1), _p(1), None) == -4


def _fake_net(cfg):
    return SimpleNamespace(cfg=cfg, dlist=ops.desc_list(cfg), device=torch.device("cpu"), packed=None)


def test_weights_keyword_is_checked_on_the_host():
    assert check_decode_weights("fp32", C.ref6_laplace(), 1, 0) == "fp32"
    assert check_decode_weights("bf16", C.bl6_softmax(), 3, 0) == "bf16"
    assert check_decode_weights("bf16", C.bl6_laplace(5, 4), 1, 6) == "bf16"
    assert check_decode_weights("bf16", C.bl6_laplace(1, 4), 2, 6) == "bf16"
    for bad in ("fp8", "bfloat16", None, 16):
        with pytest.raises(ValueError, match="weights must be one of"):
            check_decode_weights(bad, C.bl6_softmax(), 1, 0)
        with pytest.raises(ValueError, match="weights must be one of"):
            DecodeStream(_fake_net(C.bl6_softmax()), 1, weights=bad)
    # the single-sample Laplace nets: variant 0 is the wave-specialised kernel
    for cfg in (C.bl6_laplace(1, 0), C.bl6_laplace(1, 4)):
        for v in (0, 2):
            with pytest.raises(ValueError, match="variant=6"):
                DecodeStream(_fake_net(cfg), 2, variant=v, weights="bf16")
        assert DecodeStream(_fake_net(cfg), 2, variant=6, weights="bf16").weights == "bf16"
    assert DecodeStream(_fake_net(C.bl6_laplace(5, 4)), 2, weights="bf16").weights == "bf16"
    assert DecodeStream(_fake_net(C.bl6_softmax()), 2).weights == "fp32"
    # other kernels, other nets
    for cfg, v in ((C.bl6_softmax(), 1), (C.bl6_softmax(), 3), (C.ref6_laplace(), 0), (C.ref6_softmax(), 3),
                   (C.tiny("laplace", 2, 4), 0), (C.bl6_laplace(10, 4), 0)):
        with pytest.raises(ValueError, match="symmetric BL6"):
            DecodeStream(_fake_net(cfg), 1, variant=v, weights="bf16")
        with pytest.raises(ValueError, match="symmetric BL6"):
            DecodePool(_fake_net(cfg), 2, variant=v, weights="bf16")
    with pytest.raises(ValueError, match="variant=6"):
        DecodePool(_fake_net(C.bl6_laplace(1, 4)), 2, weights="bf16")
    # stepped pools have no bf16 form
    for cls in (SteppedDecodePool, SteppedModelPool):
        with pytest.raises(ValueError, match="stepped"):
            cls(_fake_net(C.ref6_laplace()), 2, weights="bf16")
        with pytest.raises(ValueError, match="weights must be one of"):
            cls(_fake_net(C.ref6_laplace()), 2, weights="fp8")


def test_modules_and_driver_carry_the_mode():
    from shallow_wavenet_amd import decode_driver as DD
    from shallow_wavenet_amd.nets import _engine
    from shallow_wavenet_amd.nets import dswnv as md
    m = md.DSWNV(**C.tiny("softmax", wav_conv_flag=False).ctor_kwargs())
    assert m.decode_weights == "fp32" and _engine.decode_weight_kwargs(m) == {}
    m.decode_weights = "bf16"
    assert _engine.decode_weight_kwargs(m) == {"weights": "bf16", "variant": 6}
    m.decode_weights = "fp16"
    with pytest.raises(ValueError, match="decode_weights"):
        _engine.resolve_decode_weights(m)
    p = DD.make_parser()
    base = ["--feats", "f", "--checkpoint", "c", "--config", "j", "--outdir", "o"]
    assert p.parse_args(base).weights == "fp32" and p.parse_args(base + ["--weights", "bf16"]).weights == "bf16"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--weights", "fp8"])
    assert "not a reference flag" in next(a.help for a in p._actions if a.dest == "weights")
