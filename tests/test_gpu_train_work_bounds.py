"""No training call writes outside the size its query returned.

Every work buffer a training call receives - the front end's activations, the forward work, the bf16 work, the kept gate
pre-activations, the backward scratch - is a WINDOW of exactly the queried size inside a larger tensor, 256-byte aligned,
with 4096 floats of a fixed bit pattern before and after it.  The calls go through the C ABI directly, as runtime.py makes
them: front end, forward, backward.  After a synchronise both guards of every window must be unchanged.  (torch's allocator
rounds sizes up, so an overrun of a few KB passes every other test.)  Nothing here looks at numerics: the parity tests do.

One case per branch of the carving code (csrc/swn_train_internal.hpp), each at the smallest shape that reaches it."""
import ctypes

import numpy as np
import pytest
import torch

from shallow_wavenet_amd import _lib
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.runtime import _ptr, _stream_ptr, pack_state_dict
from shallow_wavenet_amd.synth import synth_aux, synth_state_dict

pytestmark = pytest.mark.gpu

GUARD = 4096 * 4            # bytes on either side of a window
PATTERN = 0xA5              # every byte; as fp32 and as bf16 a tiny finite number, so a read of the guard does no harm
FP32, BF16 = _lib.PRECISION_FP32, _lib.PRECISION_BF16


class Window:
    """`nbytes` bytes, 256-byte aligned, between two guards inside one tensor"""

    def __init__(self, nbytes, device, name):
        self.name, self.nbytes = name, int(nbytes)
        self.buf = torch.full((self.nbytes + 2 * GUARD + 256,), PATTERN, dtype=torch.uint8, device=device)
        self.off = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
        assert (self.buf.data_ptr() + self.off) % 256 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.off)

    def check(self):
        before = self.buf[self.off - GUARD:self.off]
        after = self.buf[self.off + self.nbytes:self.off + self.nbytes + GUARD]
        for side, g in (("before", before), ("after", after)):
            bad = torch.nonzero(g != PATTERN).flatten()
            assert bad.numel() == 0, (f"{self.name} ({self.nbytes} bytes): {bad.numel()} guard bytes {side} the window changed, "
                                      f"first at guard byte {int(bad[0])}")


class Case:
    """one net and shape on the device: inputs, the front end run into a guarded fe_work, and the windows made so far"""

    def __init__(self, cfg, B, Tf, cond=True):
        self.cfg, self.B, self.Tf = cfg, B, Tf
        self.dev = torch.device("cuda:0")
        self.L = _lib.lib()
        self.desc = _lib.desc_from_cfg(cfg)
        self.d = ctypes.byref(self.desc)
        self.st = _stream_ptr(self.dev)
        self.windows = []
        soft = cfg.kind == "softmax"
        self.T = Tf * cfg.U
        self.Tp = self.T - 1 if soft else self.T - 2 * cfg.seg + 1
        self.coff = 1 if soft else cfg.seg
        self.packed = pack_state_dict(cfg, synth_state_dict(cfg, seed=5, flavor="trained")).to(self.dev)
        self.aux = torch.from_numpy(synth_aux(cfg, B, Tf)).to(self.dev, torch.float32).contiguous()
        rng = np.random.Generator(np.random.PCG64(7))
        if soft:
            self.audio = torch.from_numpy(rng.integers(0, cfg.n_quantize, (B, self.T - 1)).astype(np.int32)).to(self.dev)
        else:
            self.audio = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, 1, self.T - cfg.seg)).astype(np.float32)).to(self.dev)
        self.grad = torch.from_numpy(rng.standard_normal((B, cfg.n_out, self.Tp)).astype(np.float32)).to(self.dev)
        self.out = torch.empty((B, cfg.n_out, self.Tp), dtype=torch.float32, device=self.dev)
        self.gp = torch.empty_like(self.packed)
        self.fe = self.window(4 * self.L.swn_frontend_work_floats(self.d, B, Tf), "fe_work")
        self.cond = torch.empty(self.L.swn_cond_floats(self.d, B, Tf), dtype=torch.float32, device=self.dev) if cond else None
        self.call("swn_frontend", self.d, _ptr(self.packed), _ptr(self.aux), B, Tf, self.fe.ptr, _ptr(self.cond), self.st)

    def window(self, nbytes, name):
        assert nbytes > 0, f"{name}: the size query answered 0"
        w = Window(nbytes, self.dev, name)
        self.windows.append(w)
        return w

    def call(self, fn, *args):
        _lib.check(getattr(self.L, fn)(*args), fn)

    def masks(self, which):
        """drop_x and one (B, H, Tp) mask for every layer in `which` (inverted dropout at p = 0.5: values 0 and 2)"""
        cfg, g = self.cfg, torch.Generator().manual_seed(11)
        draw = lambda *shape: ((torch.rand(shape, generator=g) > 0.5).float() * 2.0).to(self.dev)
        self.drop_x = draw(self.B, cfg.A0, self.T - self.coff)
        self.drop_h = [draw(self.B, cfg.H, self.Tp) if l in which else None for l in range(cfg.L)]
        self.hptrs = (ctypes.c_void_p * cfg.L)(*[_ptr(m) for m in self.drop_h])
        return ctypes.cast(self.hptrs, ctypes.c_void_p)

    def finish(self):
        torch.cuda.synchronize(self.dev)
        for w in self.windows:
            w.check()


def _plain(cfg, B, Tf, mode):
    """swn_forward + swn_backward"""
    c = Case(cfg, B, Tf)
    fw = c.window(4 * c.L.swn_forward_work_floats(c.d, B, Tf), "forward work")
    bw = c.window(4 * c.L.swn_backward_work_floats(c.d, B, Tf), "backward work")
    c.call("swn_forward", c.d, _ptr(c.packed), _ptr(c.cond), _ptr(c.audio), B, Tf, fw.ptr, _ptr(c.out), None, c.st)
    c.call("swn_backward", c.d, _ptr(c.packed), _ptr(c.aux), _ptr(c.cond), c.fe.ptr, _ptr(c.audio), fw.ptr, None, _ptr(c.grad),
           B, Tf, bw.ptr, _ptr(c.gp), mode, c.st)
    c.finish()


def _bf16_forward(c, keep):
    """swn_pack_bf16 + swn_forward_bf16[_keep] into guarded windows -> (bf16 work, a_keep or None)"""
    B, Tf = c.B, c.Tf
    assert c.L.swn_bf16_train_forward_supported(c.d) == 1
    c.wbf = torch.empty(c.L.swn_bf16_weight_bytes(c.d), dtype=torch.uint8, device=c.dev)
    c.call("swn_pack_bf16", c.d, _ptr(c.packed), _ptr(c.wbf), c.st)
    wb = c.window(c.L.swn_forward_bf16_work_bytes(c.d, B, Tf), "bf16 work")
    if not keep:
        c.call("swn_forward_bf16", c.d, _ptr(c.packed), _ptr(c.wbf), _ptr(c.cond), _ptr(c.audio), B, Tf, wb.ptr, _ptr(c.out), c.st)
        return wb, None
    ak = c.window(4 * c.L.swn_forward_bf16_keep_floats(c.d, B, Tf), "a_keep")
    c.call("swn_forward_bf16_keep", c.d, _ptr(c.packed), _ptr(c.wbf), _ptr(c.cond), _ptr(c.audio), B, Tf, wb.ptr, _ptr(c.out),
           ak.ptr, c.st)
    return wb, ak


def _keep(cfg, B, Tf):
    """swn_forward_bf16_keep + swn_bf16_work_to_f32 + swn_backward_keep"""
    c = Case(cfg, B, Tf)
    wb, ak = _bf16_forward(c, True)
    fw = c.window(4 * c.L.swn_forward_work_floats(c.d, B, Tf), "forward work")
    bw = c.window(4 * c.L.swn_backward_work_floats(c.d, B, Tf), "backward work")
    c.call("swn_bf16_work_to_f32", c.d, _ptr(c.packed), wb.ptr, B, Tf, fw.ptr, BF16, c.st)
    c.call("swn_backward_keep", c.d, _ptr(c.packed), _ptr(c.aux), _ptr(c.cond), c.fe.ptr, _ptr(c.audio), fw.ptr, ak.ptr,
           _ptr(c.grad), B, Tf, bw.ptr, _ptr(c.gp), c.st)
    c.finish()


def _compact(cfg, B, Tf):
    """swn_forward_bf16 + swn_backward_bf16"""
    c = Case(cfg, B, Tf)
    wb, _ = _bf16_forward(c, False)
    bw = c.window(4 * c.L.swn_backward_bf16_work_floats(c.d, B, Tf), "backward work")
    c.call("swn_backward_bf16", c.d, _ptr(c.packed), _ptr(c.aux), _ptr(c.cond), c.fe.ptr, _ptr(c.audio), None, wb.ptr,
           _ptr(c.grad), B, Tf, bw.ptr, _ptr(c.gp), c.st)
    c.finish()


def _drop(cfg, B, Tf, mode, masked=None, own_hs=False, fused=False):
    """swn_forward_drop + swn_backward_drop; masked: the layers whose output gets a mask (default: every layer)"""
    c = Case(cfg, B, Tf, cond=False)
    hptr = c.masks(range(cfg.L) if masked is None else masked)
    assert c.L.swn_drop_fused_path(c.d, B, Tf, hptr) == (1 if fused else 0)
    fw = c.window(4 * c.L.swn_forward_drop_work_floats(c.d, B, Tf), "forward work")
    bw = c.window(4 * c.L.swn_backward_drop_work_floats(c.d, B, Tf), "backward work")
    hs = c.window(4 * B * (cfg.L + 1) * cfg.H * c.Tp, "hs") if own_hs else None
    hs_ptr = hs.ptr if own_hs else None
    c.call("swn_forward_drop", c.d, _ptr(c.packed), c.fe.ptr, _ptr(c.audio), B, Tf, _ptr(c.drop_x), hptr, fw.ptr, _ptr(c.out),
           hs_ptr, mode, c.st)
    c.call("swn_backward_drop", c.d, _ptr(c.packed), _ptr(c.aux), c.fe.ptr, _ptr(c.audio), fw.ptr, hs_ptr, _ptr(c.drop_x), hptr,
           _ptr(c.grad), B, Tf, bw.ptr, _ptr(c.gp), mode, c.st)
    c.finish()


def test_window_check_sees_a_changed_guard(gpu_ok):
    w = Window(1024, torch.device("cuda:0"), "probe")
    w.check()
    w.buf[w.off + w.nbytes] = 0
    with pytest.raises(AssertionError):
        w.check()


def test_fp32_chain(gpu_ok):                    # plain chain
    _plain(C.tiny("laplace", 2, 4), 2, 3, FP32)


def test_bf16_chain_short(gpu_ok):              # Tp = 59: da16 / wdt16 without h16
    _plain(C.tiny("laplace", 1, 0), 2, 3, BF16)


def test_bf16_chain_long(gpu_ok):               # Tp = 279: h16, skip_da32
    _plain(C.tiny("laplace", 1, 0), 3, 14, BF16)


def test_keep_bl6_softmax(gpu_ok):              # keep path
    _keep(C.bl6_softmax(), 1, 4)


def test_keep_ref6(gpu_ok):                     # keep path, H = 192 layer kernel
    _keep(C.ref6_laplace(1, 4), 1, 3)


def test_compact_bl6(gpu_ok):                   # compact layout around the fused stack's scratch
    _compact(C.bl6_laplace(1, 0), 2, 3)


def test_drop_fp32_seg1(gpu_ok):                # dgx_all
    _drop(C.tiny("laplace", 1, 0), 2, 3, FP32)


def test_drop_fp32_seg2(gpu_ok):                # per-layer in_x contractions
    _drop(C.tiny("laplace", 2, 4), 2, 3, FP32)


def test_drop_bf16_ref6_seg5(gpu_ok):           # kept pre-activations without bf16 in_x copies
    _drop(C.ref6_laplace(5, 4), 1, 2, BF16)


def test_drop_bf16_ref6_stack(gpu_ok):          # GEMM-stack forward, dgx16_all / wxt16
    _drop(C.ref6_laplace(1, 4), 1, 3, BF16)


def test_drop_bf16_ref6_own_hs(gpu_ok):         # caller-owned hs: bf16-operand layers, no bf16 in_x copies, recomputed pre-activations
                                                # (values: test_gpu_drop_own_hs_values.py)
    _drop(C.ref6_laplace(1, 4), 1, 3, BF16, own_hs=True)


def test_drop_bf16_bl6_fused(gpu_ok):           # fused path: the mask on the last layer only
    cfg = C.bl6_laplace(1, 0)
    _drop(cfg, 2, 3, BF16, masked=[cfg.L - 1], fused=True)
