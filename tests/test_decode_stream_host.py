"""CPU: the streamed-decode entry points of the C ABI, the frame / step planning of DecodeStream and its argument
checks - everything that runs before a device is touched."""
import ctypes
import re
from dataclasses import replace

import pytest
import torch

from shallow_wavenet_amd import _lib, config as C
from shallow_wavenet_amd import ops
from shallow_wavenet_amd.streaming import DecodeStream, final_frames, lookahead_frames, ready_steps

NEW_SYMBOLS = ("swn_decode_resolve_variant", "swn_decode_session_floats", "swn_decode_chunk")


def test_streaming_symbols_are_exported_and_bound():
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.swn_abi_version() == 3
    assert "decode_chunk" in ops.OP_NAMES
    schema = str(torch.ops.swn.decode_chunk.default._schema)
    assert schema.startswith("swn::decode_chunk(") and re.search(r"Tensor\(a\d*!\) session", schema)


def _io():
    return _lib.DecodeIO(noise_dev=None, forced_dev=None, seed_dev=None, noise_out_dev=None, rng_seed=1, rng_utt0=0,
                         reserved=0, rng_utt_ids_dev=None)


def _chunk(d, step0=0, n_steps=4, flags=1, io=True, session=1, packed=1, cond=1, out=1, variant=0, batch=1, frames=4):
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v) if v else None
    return lib.swn_decode_chunk(ctypes.byref(d), p(packed), p(cond), batch, frames, step0, n_steps, flags,
                                ctypes.byref(_io()) if io else None, p(session), p(out), None, variant, None)


def test_chunk_rejects_bad_arguments_before_any_launch():
    """fake non-null addresses are fine: every one of these is refused before the library touches them"""
    d = _lib.desc_from_cfg(C.bl6_laplace())
    assert _chunk(d, io=False) == -2
    assert _chunk(d, session=0) == -2
    assert _chunk(d, packed=0) == -2
    assert _chunk(d, cond=0) == -2
    assert _chunk(d, out=0) == -2
    assert _chunk(d, step0=1, flags=1) == -2            # BEGIN must start at step 0
    assert _chunk(d, step0=-1, flags=0) == -2
    assert _chunk(d, n_steps=-1, flags=0) == -2
    assert _chunk(d, variant=4) == -2                   # retired (cohort / cluster)
    assert _chunk(d, variant=5) == -2
    assert _chunk(d, variant=7) == -2
    assert _chunk(d, flags=2) == -2                      # unknown flag
    assert _chunk(d, step0=0, n_steps=4 * 110 + 1, frames=4) == -2   # past the final conditioning
    # the symmetric / wave-specialised BL6 variant does not resolve for a net outside the BL6 class
    assert _chunk(_lib.desc_from_cfg(C.tiny("laplace", 2, 4)), variant=6, frames=4) == -2
    lib = _lib.lib()
    assert lib.swn_decode_chunk(None, ctypes.c_void_p(1), ctypes.c_void_p(1), 1, 4, 0, 4, 1, ctypes.byref(_io()),
                                ctypes.c_void_p(1), ctypes.c_void_p(1), None, 0, None) == -2          # no descriptor
    # a chunk of no steps that does not begin a stream is a no-op and touches nothing
    assert _chunk(d, step0=3, n_steps=0, flags=0, out=0) == 0


@pytest.mark.parametrize("cfg,batch,variant,want", [
    (C.bl6_laplace(), 1, 0, 2), (C.bl6_laplace(1, 4), 3, 0, 2), (C.bl6_laplace(5, 4), 2, 0, 2), (C.bl6_softmax(), 2, 0, 2),
    (C.bl6_laplace(), 1, 6, 6), (C.bl6_laplace(), 1, 1, 1), (C.bl6_laplace(), 1, 3, 3),
    (C.ref6_laplace(), 2, 0, 3), (C.ref6_laplace(), 27, 0, 3), (C.ref6_softmax(), 1, 0, 3),
    (C.tiny("laplace", 2, 4), 2, 0, 1), (C.tiny("softmax"), 2, 0, 1)])
def test_variant_resolution_and_session_sizes(cfg, batch, variant, want):
    lib = _lib.lib()
    d = _lib.desc_from_cfg(cfg)
    assert lib.swn_decode_resolve_variant(ctypes.byref(d), batch, variant) == want
    n1 = lib.swn_decode_session_floats(ctypes.byref(d), 1, variant)
    nb = lib.swn_decode_session_floats(ctypes.byref(d), batch, variant)
    assert n1 > 0 and nb >= n1 * batch - 64 * batch
    # the session holds at least every history ring: sum over layers of (padding + seg) positions x H
    rings = sum(p + (1 if cfg.kind == "softmax" else cfg.seg) for p in cfg.paddings) * cfg.H
    assert n1 >= rings


def test_unresolvable_variants():
    lib = _lib.lib()
    d = _lib.desc_from_cfg(C.tiny("laplace", 2, 4))
    for v in (4, 5, -1, 9):
        assert lib.swn_decode_resolve_variant(ctypes.byref(d), 1, v) == -2
    assert lib.swn_decode_resolve_variant(ctypes.byref(d), 1, 2) == -4      # no BL6-class kernel for this net
    assert lib.swn_decode_resolve_variant(ctypes.byref(d), 0, 0) == -2
    assert lib.swn_decode_session_floats(ctypes.byref(d), 1, 4) == 0


@pytest.mark.parametrize("k,layers,want", [(3, 2, 4), (3, 3, 13), (5, 2, 12), (3, 1, 1), (1, 2, 0)])
def test_lookahead_frames_known_answers(k, layers, want):
    cfg = replace(C.bl6_laplace(), aux_kernel_size=k, aux_dilation_size=layers)
    assert lookahead_frames(cfg) == want
    assert lookahead_frames(C.ref6_laplace()) == 4                # the run.sh geometry


@pytest.mark.parametrize("seg,U", [(1, 110), (5, 110), (1, 80), (5, 80)])
def test_step_planning_one_frame_at_a_time(seg, U):
    """frames arriving one by one: every frame after the halo releases U / seg steps, finish() releases the rest, and the
    total is the one-shot frames * U // seg"""
    cfg = replace(C.bl6_laplace(seg, 4 if seg > 1 else 0), upsampling_factor=U)
    la = lookahead_frames(cfg)
    F = 23
    done, released = 0, []
    for r in range(1, F + 1):
        ff = final_frames(r, la, False)
        assert ff == max(0, r - la)
        target = ready_steps(cfg, ff)
        released.append(target - done)
        done = target
    tail = ready_steps(cfg, final_frames(F, la, True)) - done
    assert released[:la] == [0] * la
    assert all(n == U // seg for n in released[la:])
    assert tail == la * U // seg
    assert done + tail == F * U // seg
    # every step of a release reads only final frames: the last position of step i is (i + 1) * seg - 1
    for ff in range(1, F + 1):
        n = ready_steps(cfg, ff)
        assert ((n * seg) - 1) // U <= ff - 1


def test_softmax_steps_use_seg_one():
    cfg = C.bl6_softmax()
    assert ready_steps(cfg, 3) == 3 * 80


class _FakeNet:
    """what DecodeStream reads from a HipNet before it allocates anything"""
    def __init__(self, cfg):
        self.cfg, self.dlist, self.packed = cfg, ops.desc_list(cfg), None
        self.device = torch.device("cpu")


def test_stream_argument_errors_raise_before_touching_a_device():
    cfg = C.bl6_laplace()
    net = _FakeNet(cfg)
    with pytest.raises(ValueError):
        DecodeStream(net, 0)
    with pytest.raises(ValueError):
        DecodeStream(net, 2, variant=4)
    with pytest.raises(ValueError):
        DecodeStream(_FakeNet(C.tiny("laplace", 2, 4)), 2, variant=6)
    with pytest.raises(ValueError):
        DecodeStream(net, 2, seed=torch.zeros(3))
    with pytest.raises(ValueError):
        DecodeStream(net, 2, utt_ids=[1])
    s = DecodeStream(net, 2)
    assert s.lookahead_frames == 4 and s.steps_done == 0 and s.frames_received == 0 and not s.finished
    with pytest.raises(ValueError):
        s.push(torch.zeros(3, cfg.n_aux, 5))            # batch mismatch
    with pytest.raises(ValueError):
        s.push(torch.zeros(2, cfg.n_aux + 1, 5))        # feature width mismatch
    with pytest.raises(ValueError):
        s.push(torch.zeros(2, cfg.n_aux))               # not (B, n_aux, f)
    with pytest.raises(RuntimeError):
        s.advance(1)                                     # no final conditioning yet
    with pytest.raises(ValueError):
        s.advance(-1)
    assert s.frames_received == 0 and s._session is None and s._cond is None
    s.finished = True
    with pytest.raises(RuntimeError):
        s.push(torch.zeros(2, cfg.n_aux, 1))             # push after finish
