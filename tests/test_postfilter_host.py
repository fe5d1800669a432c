"""CPU: the device post-filter of run.sh stage 6 (swn_postfilter_chunk, postfilter.NoiseShapingRestorer) - its symbols are exported
and bound, the per-slot state size follows the documented layout, bad arguments are rejected before any device call, and the
restorer builds exactly the filter dsp.noise_shaping builds."""
import ctypes

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib, dsp, ops
from shallow_wavenet_amd.postfilter import NoiseShapingRestorer

MEAN = np.concatenate([[0.9, 5.0, -3.0, -4.0, 0.1], 1.5 * np.exp(-0.15 * np.arange(50)) * np.cos(0.7 * np.arange(50))])


def test_symbols_are_exported_and_bound():
    lib = _lib.lib()
    for name in ("swn_postfilter_state_doubles", "swn_postfilter_chunk"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.swn_abi_version() == 3
    assert "postfilter_chunk" in ops.OP_NAMES
    assert str(torch.ops.swn.postfilter_chunk.default._schema).startswith("swn::postfilter_chunk(")
    assert ctypes.sizeof(_lib.PostfilterEntry) == 32


@pytest.mark.parametrize("order,pade,n_taps", [(49, 4, 255), (49, 5, 255), (1, 4, 1), (62, 5, 256), (24, 4, 31)])
def test_state_size(order, pade, n_taps):
    want = 2 * (pade + 1) + pade * (order + 2) + pade + 1 + (n_taps - 1)
    assert _lib.lib().swn_postfilter_state_doubles(order, pade, n_taps) == want


@pytest.mark.parametrize("order,pade,n_taps", [(49, 3, 255), (49, 6, 255), (0, 4, 255), (49, 4, 0), (49, 4, 257)])
def test_state_size_of_bad_arguments_is_zero(order, pade, n_taps):
    assert _lib.lib().swn_postfilter_state_doubles(order, pade, n_taps) == 0


def _entries(**kw):
    e = dict(in_dev=1 << 20, out_dev=1 << 21, slot=0, n=16, kind=_lib.POSTFILTER_IN_F32, flags=_lib.POSTFILTER_RESET)
    e.update(kw)
    return e


def _call(order=49, alpha=0.455, pade=4, n_taps=255, b=1 << 12, taps=1 << 13, mulaw=None, state=1 << 14, capacity=2,
          entries=None, n_entries=None):
    """the C entry point with fake (never dereferenced) device addresses: every case here must fail before a device call"""
    entries = [_entries()] if entries is None else entries
    table = (_lib.PostfilterEntry * max(1, len(entries)))(*[_lib.PostfilterEntry(**e) for e in entries])
    n = len(entries) if n_entries is None else n_entries
    vp = ctypes.c_void_p
    return _lib.lib().swn_postfilter_chunk(order, alpha, pade, vp(b), n_taps, vp(taps), vp(mulaw), vp(state), capacity,
                                           table, n, vp(None))


@pytest.mark.parametrize("kw", [
    dict(pade=3), dict(pade=6), dict(alpha=1.0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(n_taps=0),
    dict(n_taps=257), dict(order=0), dict(b=None), dict(taps=None), dict(state=None), dict(capacity=0), dict(n_entries=-1),
    dict(entries=[_entries(slot=2)]), dict(entries=[_entries(slot=-1)]), dict(entries=[_entries(), _entries()]),
    dict(entries=[_entries(n=-1)]), dict(entries=[_entries(kind=2)]), dict(entries=[_entries(flags=2)]),
    dict(entries=[_entries(in_dev=None)]), dict(entries=[_entries(out_dev=None)]),
    dict(entries=[_entries(kind=_lib.POSTFILTER_IN_MULAW)]),
    dict(order=63, pade=7)])
def test_bad_arguments_are_rejected_before_any_device_call(kw):
    assert _call(**kw) == -2


def test_orders_past_one_wave_are_unsupported_and_empty_calls_succeed():
    assert _call(order=63) == -4
    assert _call(entries=[], n_entries=0) == 0


@pytest.mark.parametrize("inv", [True, False])
@pytest.mark.parametrize("fs,alpha,mag,start", [(22050, 0.455, 0.5, 5), (24000, 0.466, 0.3, 5), (16000, 0.41, 0.5, 6)])
def test_restorer_builds_the_filter_of_noise_shaping(monkeypatch, inv, fs, alpha, mag, start):
    """b and the taps are those dsp.noise_shaping hands to the MLSA filter and to lfilter (captured from its own calls)"""
    seen = {}
    real_synth = dsp.MLSAFilter.synthesis

    def synth(self, x, b):
        seen["b"] = np.array(b)
        return real_synth(self, x, b)

    import scipy.signal
    real_lfilter = scipy.signal.lfilter

    def lfilter(b, a, x):
        seen["taps"] = np.array(b)
        return real_lfilter(b, a, x)

    monkeypatch.setattr(dsp.MLSAFilter, "synthesis", synth)
    monkeypatch.setattr(scipy.signal, "lfilter", lfilter)
    dsp.noise_shaping(np.zeros(300), MEAN, fs, alpha, mag=mag, mcep_dim_start=start, inv=inv)
    r = NoiseShapingRestorer(MEAN, fs, alpha, mag=mag, mcep_dim_start=start, inv=inv, device="meta")   # no device memory
    assert np.all(seen["b"] == seen["b"][0])                                   # time-invariant frames
    assert np.array_equal(r.b, seen["b"][0])
    assert r.b[0] != 0.0                                                       # mc2b moves c(1..) into b(0)
    assert np.array_equal(r.taps, seen["taps"]) and r.n_taps == 255
    assert r.order == MEAN.size - start - 1


def test_restorer_rejects_what_the_device_cannot_run():
    with pytest.raises(ValueError):
        NoiseShapingRestorer(MEAN, 22050, 0.455, pade=3, device="meta")
    with pytest.raises(ValueError):
        NoiseShapingRestorer(MEAN, 22050, 1.0, device="meta")
    with pytest.raises(ValueError):
        NoiseShapingRestorer(np.zeros(80), 22050, 0.455, mcep_dim_start=5, device="meta")     # order 74 > 62


def test_slots_open_and_close_without_a_device():
    r = NoiseShapingRestorer(MEAN, 22050, 0.455, capacity=3, device="meta")
    assert r.state_doubles == _lib.lib().swn_postfilter_state_doubles(49, 4, 255)
    assert [r.open(), r.open()] == [0, 1]
    assert r.open(2) == 2
    with pytest.raises(RuntimeError):
        r.open()
    r.close(1)
    assert r.open() == 1 and 1 in r._reset
    with pytest.raises(RuntimeError):
        r.open(1)
    r.close(0)
    with pytest.raises(RuntimeError):
        r.close(0)
    with pytest.raises(RuntimeError):
        r.run({0: torch.zeros(4)})                                              # not open


def test_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        img = torch.empty(50 + 255, dtype=torch.float64)
        st = torch.empty(10, dtype=torch.float64)
        out = torch.ops.swn.postfilter_chunk(img, st, [torch.empty(7), torch.empty(3)], [0, 1], [True, False], 49, 0.455, 4,
                                             255, 2)
        assert tuple(out.shape) == (2, 7) and out.dtype == torch.float32
