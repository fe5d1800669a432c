"""PyTorch custom ops over the C ABI: `torch.ops.swn.*` (one `torch.library` namespace).

(Each op NAME is registered from a plain function NAME_impl; the training autograd Functions of nets/_autograd.py call
the _impl functions directly - they already sit inside an autograd node, and a Python custom op costs 30-50 us of
dispatch per call, which the BL6 training step notices.)

Every op is a thin, stateless wrapper of one entry point of `include/swn_hip.h`: it takes contiguous device tensors
plus the network descriptor as a list of 16 integers (the fields of `swn_net_desc`, i.e. the reference constructor
arguments), allocates its outputs with torch, and launches on torch's current HIP stream.  Failures of the library
surface as `RuntimeError` (the reference's own convention for bad shapes is whatever torch raises).  Fake (meta)
implementations are registered so the ops trace under `torch.compile` / `FakeTensorMode`; gradients are wired by
`nets/_autograd.py` (the backward entry points are ops of this namespace too).

    torch.ops.swn.pack_params(tensors, desc)                       -> packed
    torch.ops.swn.frontend(packed, aux, desc)                      -> (cond, work)
    torch.ops.swn.frontend_pool(packed, auxs, conds, staged?, n_news, n_receiveds, f0s, f1s, finals, desc)  -> ()
    torch.ops.swn.frontend_pool_models(models, model_of, auxs, conds, staged?, n_news, n_receiveds, f0s, f1s, finals, desc)  -> ()
    torch.ops.swn.decode(packed, cond, noise?, forced?, seed?, desc, n_steps, variant, rng_seed, rng_utt0,
                         want_heads, want_noise, utt_ids?)         -> (out, heads, noise_used)
    torch.ops.swn.decode_chunk(packed, cond, session, noise?, forced?, seed?, desc, step0, n_steps, begin, variant,
                               rng_seed, rng_utt0, want_heads, want_noise, utt_ids?)  -> (out, heads, noise_used)
    torch.ops.swn.decode_pool_chunk(packed, session, conds, slots, step0s, n_steps, begins, seeds?, utt_ids, desc, capacity,
                                    variant, rng_seed, want_heads, want_noise)  -> (out, heads, noise_used)
    torch.ops.swn.decode_pool_chunk_models(models, model_of, session, conds, slots, step0s, n_steps, begins, seeds?, utt_ids,
                                           desc, capacity, variant, rng_seed, want_heads, want_noise)  -> (out, heads, noise_used)
    per stored format of the streamed head matrices (DECODE_IMAGES: bf16 -> w16, e4m3 -> w8; one factory, _image_ops):
    torch.ops.swn.pack_decode_<sfx>(packed, desc)                  -> image (w16: bf16; w8: FP8 E4M3 codes + row scales)
    torch.ops.swn.decode_<sfx>(packed, image, cond, ...decode's arguments)            -> (out, heads, noise_used)
    torch.ops.swn.decode_chunk_<sfx>(packed, image, cond, session, ...decode_chunk's) -> (out, heads, noise_used)
    torch.ops.swn.decode_pool_chunk_<sfx>(packed, image, session, ...decode_pool_chunk's) -> (out, heads, noise_used)
    torch.ops.swn.decode_pool_chunk_models_<sfx>(models, images, model_of, session, ...decode_pool_chunk_models')
                                                                   -> (out, heads, noise_used)   (images[m]: the image of models[m])
    torch.ops.swn.e4m3_table(like, scale)                          -> (256,) fp32: the kernels' conversion of codes 0 .. 255
    torch.ops.swn.decode_pool_chunk_wide(models, images, weights, model_of, session, ...decode_pool_chunk_models')
                                                                   -> (out, heads, noise_used)   (up to 256 entries per launch)
    torch.ops.swn.decode_pool_stepped_chunk(packed, session, conds, slots, it0s, n_its, begins, seeds?, utt_ids, desc,
                                            capacity, rng_seed, want_heads, want_noise)  -> (out, heads, noise_used)
    torch.ops.swn.decode_pool_stepped_chunk_models(models, model_of, session, conds, slots, it0s, n_its, begins, seeds?, utt_ids,
                                                   desc, capacity, rng_seed, want_heads, want_noise)  -> (out, heads, noise_used)
    torch.ops.swn.decode_stepped_prologue(models, model_of, session, conds, slots, seeds?, desc, n_slots)  -> ()
    torch.ops.swn.postfilter_chunk(image, state, inputs, slots, resets, order, alpha, pade, n_taps, capacity)  -> restored
    torch.ops.swn.stack_forward(packed, cond, audio, desc, want_hidden) -> (raw, work, hidden)
    torch.ops.swn.stack_forward_bf16(packed, wbf16, cond, audio, desc)  -> (raw, work)
    torch.ops.swn.pack_bf16(packed, desc)                          -> wbf16
    torch.ops.swn.laplace_head(raw, desc, clip)                    -> (mu, b, logb, a, b_clip, logb_clip, below_floor)
    torch.ops.swn.stack_backward(packed, aux, cond, fe_work, audio, fwd_work, grad_raw, desc, precision) -> grad_packed
    torch.ops.swn.laplace_head_backward(raw, gmu?, gb?, glogb?, ga?, gb_clip?, glogb_clip?, desc) -> grad_raw
    torch.ops.swn.spectral_loss(samples, targets, tables, sizes, keep_state) -> (l1, lsd, state)
    torch.ops.swn.spectral_loss_backward(grad_l1, state, tables, sizes, length) -> grad_samples
    torch.ops.swn.logmel(wav, tables, bank, t0s, n_avails, lens, f0s, f1s, n_fft, hop, floor, linear) -> features
    torch.ops.swn.logmel_pool(win, staged, tables, bank, slots, t0s, n_helds, n_drops, n_news, lens, f0s, f1s, n_fft, hop,
                              floor, linear) -> features of all sessions, channel-major (updates win)
    torch.ops.swn.mcep(wav, tables, t0s, n_avails, lens, f0s, f1s, n_fft, hop, order, floor) -> mel-cepstra
    torch.ops.swn.lowcut_chunk(taps, state, inputs, slots, resets, capacity) -> low-cut chunks (updates state)
    torch.ops.swn.logmel_pool_lowcut(win, hist, staged, tables, bank, taps, slots, t0s, n_helds, n_drops, n_news, lens, f0s, f1s,
                                     n_fft, hop, floor, linear) -> logmel_pool on raw samples (updates win and hist)
    torch.ops.swn.resample_chunk(table, state, inputs, slots, in0s, out0s, n_outs, lens, up, down, n_taps, capacity, dense)
                                     -> resampled chunks (updates state)
    torch.ops.swn.resample_staged(table, state, staged, n_ins, slots, in0s, out0s, n_outs, lens, up, down, n_taps, capacity)
                                     -> resample_chunk on chunks staged back to back, dense outputs (updates state)
    torch.ops.swn.f0(wav, t0s, n_avails, lens, f0s, f1s, fs, hop, win, lag_lo, lag_hi, threshold) -> (F0 in Hz, aperiodicity) per frame
    torch.ops.swn.bap(wav, taps, t0s, n_avails, lens, f0s, f1s, fs, hop, win, lag_lo, lag_hi, threshold, band_win, floor)
                                                    -> (F0 in Hz, aperiodicity, B coded band aperiodicities in dB) per frame
    torch.ops.swn.envelope(wav, f0, tables, t0s, n_avails, lens, f0s, f1s, fs, n_fft, hop, order, floor, q1, default_f0, what)
                                                    -> mel-cepstra (what 0) or log amplitudes (what 1) of the F0-adaptive envelope
    torch.ops.swn.laplace_loss(raw, ctx?, target, eps, desc, skip) -> (nll, err, samples, targets, stats)
    torch.ops.swn.laplace_loss_backward(raw, ctx?, target, eps, g_nll, g_samples?, desc, skip) -> grad_raw
"""
from __future__ import annotations

import ctypes
import inspect
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch.library import custom_op

from . import _lib
from .config import NetConfig

DESC_FIELDS = [n for n, _ in _lib.NetDesc._fields_]


def desc_list(cfg: NetConfig) -> List[int]:
    d = _lib.desc_from_cfg(cfg)
    return [int(getattr(d, f)) for f in DESC_FIELDS]


_DESC_CACHE: dict = {}


def _desc(vals: Sequence[int]) -> "_lib.NetDesc":
    key = tuple(vals)
    d = _DESC_CACHE.get(key)
    if d is None:
        if len(vals) != len(DESC_FIELDS):
            raise RuntimeError(f"descriptor needs {len(DESC_FIELDS)} integers ({', '.join(DESC_FIELDS)})")
        d = _DESC_CACHE[key] = _lib.NetDesc(**{f: int(v) for f, v in zip(DESC_FIELDS, vals)})
    return d


class _on:
    """`with _on(dev):` = torch.cuda.device(dev) only when dev is not the current device (the context manager costs
    more host time than a launch)."""
    __slots__ = ("ctx",)

    def __init__(self, dev):
        self.ctx = None if dev.index is None or dev.index == torch.cuda.current_device() else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _geom(d) -> Tuple[int, int, int, int, int, int]:
    """(soft, seg, L, H, n_out, out1) from a descriptor."""
    soft = d.kind == 1
    seg = 1 if soft else d.seg
    L = d.dilation_depth * d.dilation_repeat
    n_out = d.n_quantize if soft else 2 * d.seg + d.lpc
    return soft, seg, L, d.hid_chn, n_out, (d.n_quantize if soft else d.skip_chn)


def _need_cuda(t: torch.Tensor, what: str) -> None:
    if t.device.type != "cuda":
        raise RuntimeError(f"swn ops need {what} on a HIP device (no CPU path)")


# ------------------------------------------------------------------------------------------ pack
def pack_params_impl(tensors: List[torch.Tensor], desc: List[int]) -> torch.Tensor:
    """state_dict tensors (reference order, on the device) -> packed buffer (swn_pack_params_device)."""
    L = _lib.lib()
    d = _desc(desc)
    dev = tensors[0].device
    _need_cuda(tensors[0], "the parameters")
    keep = [t.detach().to(torch.float32).contiguous() for t in tensors]
    total = L.swn_packed_floats(ctypes.byref(d))
    out = torch.empty(total, dtype=torch.float32, device=dev)
    ptrs = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
    with _on(dev):
        _lib.check(L.swn_pack_params_device(ctypes.byref(d), ptrs, len(keep), _ptr(out), total, _stream(dev)),
                   "pack_params_device")
    return out


pack_params = custom_op("swn::pack_params", mutates_args=())(pack_params_impl)


@pack_params.register_fake
def _(tensors, desc):
    d = _desc(desc)
    return tensors[0].new_empty(_lib.lib().swn_packed_floats(ctypes.byref(d)), dtype=torch.float32)


# ------------------------------------------------------------------------------------------ front end
def frontend_impl(packed: torch.Tensor, aux: torch.Tensor, desc: List[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """aux (B, n_aux, Tf) -> cond (B, Tf, L*seg*2H) and the work buffer the backward needs (swn_frontend)."""
    L = _lib.lib()
    d = _desc(desc)
    _need_cuda(packed, "the packed parameters")
    dev = packed.device
    aux = aux.to(dev, torch.float32).contiguous()
    B, na, Tf = aux.shape
    if na != d.n_aux:
        raise RuntimeError(f"aux has {na} channels, model expects {d.n_aux}")
    r = ctypes.byref(d)
    work = torch.empty(L.swn_frontend_work_floats(r, B, Tf), dtype=torch.float32, device=dev)
    cond = torch.empty(L.swn_cond_floats(r, B, Tf), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.swn_frontend(r, _ptr(packed), _ptr(aux), B, Tf, _ptr(work), _ptr(cond), _stream(dev)), "frontend")
    return cond.view(B, Tf, -1), work


frontend = custom_op("swn::frontend", mutates_args=())(frontend_impl)


@frontend.register_fake
def _(packed, aux, desc):
    L, d = _lib.lib(), _desc(desc)
    B, _, Tf = aux.shape
    r = ctypes.byref(d)
    n = L.swn_cond_floats(r, B, Tf)
    return packed.new_empty((B, Tf, n // (B * Tf))), packed.new_empty(L.swn_frontend_work_floats(r, B, Tf))


# ------------------------------------------------------------------------------------------ pool front end
def frontend_pool_impl(packed: torch.Tensor, auxs: List[torch.Tensor], conds: List[torch.Tensor],
                       staged: Optional[torch.Tensor], n_news: List[int], n_receiveds: List[int], f0s: List[int],
                       f1s: List[int], finals: List[bool], desc: List[int]) -> None:
    """one front end call for the sessions of a pool tick (swn_frontend_pool): entry e appends its n_news[e] new frames - the
    next n_aux * n_news[e] floats of `staged`, the flat concatenation of the entries' (n_aux, n_new) chunks - to its feature
    buffer auxs[e] (n_aux, stride) at frames [n_receiveds[e] - n_news[e], n_receiveds[e]) and writes the cond rows of the
    absolute frames [f0s[e], f1s[e]) into conds[e] (rows, N); finals[e]: the features end at n_receiveds[e].  Both lists are
    updated in place; the rows are bit-identical to `frontend` over the whole utterance."""
    L = _lib.lib()
    d = _desc(desc)
    _need_cuda(packed, "the packed parameters")
    dev = packed.device
    table = _frontend_pool_table(L, d, dev, auxs, conds, staged, n_news, n_receiveds, f0s, f1s, finals)
    r, E = ctypes.byref(d), len(auxs)
    floats = L.swn_frontend_pool_work_floats(r, table, E)
    if floats == 0:
        raise RuntimeError(_FP_REFUSED)
    work = torch.empty(floats, dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.swn_frontend_pool(r, _ptr(packed), table, E, _ptr(work), _stream(dev)), "frontend_pool")


_FP_REFUSED = ("swn_hip frontend_pool: bad argument: the entry table is refused (frame ranges, strides, flags or a "
               "cond buffer in two entries)")


def _frontend_pool_table(L, d, dev, auxs, conds, staged, n_news, n_receiveds, f0s, f1s, finals):
    """the checked entry table of a pool front end call (frontend_pool and frontend_pool_models)"""
    E = len(auxs)
    if not (len(conds) == len(n_news) == len(n_receiveds) == len(f0s) == len(f1s) == len(finals) == E):
        raise RuntimeError("frontend_pool: auxs, conds, n_news, n_receiveds, f0s, f1s and finals must have one entry each")
    if not 1 <= E <= _lib.FRONTEND_POOL_MAX_ENTRIES:
        raise RuntimeError(f"frontend_pool: {E} entries, a call takes 1 .. {_lib.FRONTEND_POOL_MAX_ENTRIES}")
    na = d.n_aux
    total_new = sum(int(n) for n in n_news)
    base = 0
    if total_new > 0:
        if staged is None or staged.device != dev or staged.dtype != torch.float32 or not staged.is_contiguous():
            raise RuntimeError("frontend_pool: staged must be a contiguous fp32 tensor on the device of the packed parameters")
        if staged.numel() != na * total_new:
            raise RuntimeError(f"frontend_pool: staged holds {staged.numel()} floats, the entries' new frames need {na * total_new}")
        base = staged.data_ptr()
    table = (_lib.FrontendPoolEntry * E)()
    r = ctypes.byref(d)
    N = L.swn_cond_floats(r, 1, 1)
    off = 0
    for e in range(E):
        a, c = auxs[e], conds[e]
        if a.device != dev or a.dtype != torch.float32 or not a.is_contiguous() or a.dim() < 2 or \
                a.numel() != na * a.shape[-1]:
            raise RuntimeError("frontend_pool: every feature buffer must be a contiguous (n_aux, stride) fp32 tensor on the device")
        if c.device != dev or c.dtype != torch.float32 or not c.is_contiguous() or c.dim() != 2 or c.shape[1] != N:
            raise RuntimeError("frontend_pool: every cond buffer must be a contiguous (rows, N) fp32 tensor on the device")
        n_new, f1 = int(n_news[e]), int(f1s[e])
        if f1 > c.shape[0]:
            raise RuntimeError(f"frontend_pool: entry {e} writes cond rows up to {f1}, its buffer has {c.shape[0]}")
        t = table[e]
        t.aux_dev, t.cond_dev = a.data_ptr(), c.data_ptr()
        t.new_dev = base + 4 * na * off if n_new > 0 else None
        t.aux_stride, t.n_received, t.n_new = int(a.shape[-1]), int(n_receiveds[e]), n_new
        t.f0, t.f1, t.flags = int(f0s[e]), f1, _lib.FRONTEND_FINAL if finals[e] else 0
        off += max(n_new, 0)
    return table


frontend_pool = custom_op("swn::frontend_pool", mutates_args=("auxs", "conds"))(frontend_pool_impl)


@frontend_pool.register_fake
def _(packed, auxs, conds, staged, n_news, n_receiveds, f0s, f1s, finals, desc):
    return None


def _model_tables(L, d, models: List[torch.Tensor], model_of: List[int], E: int, what: str,
                  max_models: int = _lib.POOL_MAX_MODELS):
    """the checked model arguments of a *_models call -> (device, HOST array of the models' device pointers, int32 array of
    the entries' model indices).  Every model buffer is fp32, contiguous, on one HIP device and swn_packed_floats long."""
    if not 1 <= len(models) <= max_models:
        raise RuntimeError(f"{what}: {len(models)} models, a call takes 1 .. {max_models}")
    _need_cuda(models[0], "the packed parameters")
    dev = models[0].device
    total = L.swn_packed_floats(ctypes.byref(d))
    for m, t in enumerate(models):
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != total:
            raise RuntimeError(f"{what}: model {m} must be a contiguous fp32 buffer of {total} floats (swn_packed_floats) on "
                               f"{dev}")
    if len(model_of) != E:
        raise RuntimeError(f"{what}: model_of has {len(model_of)} entries, the call has {E}")
    for e, m in enumerate(model_of):
        if not 0 <= int(m) < len(models):
            raise RuntimeError(f"{what}: entry {e} names model {int(m)}, the call has {len(models)}")
    ptrs = (ctypes.c_void_p * len(models))(*[t.data_ptr() for t in models])
    return dev, ptrs, (ctypes.c_int32 * E)(*[int(m) for m in model_of])


def frontend_pool_models_impl(models: List[torch.Tensor], model_of: List[int], auxs: List[torch.Tensor],
                              conds: List[torch.Tensor], staged: Optional[torch.Tensor], n_news: List[int],
                              n_receiveds: List[int], f0s: List[int], f1s: List[int], finals: List[bool],
                              desc: List[int]) -> None:
    """frontend_pool over sessions of several models of one geometry (swn_frontend_pool_models): entry e is finalised with the
    packed parameters models[model_of[e]] (at most 16 models per call); everything else as frontend_pool, and every row
    bit-identical to `frontend` with that entry's model."""
    L = _lib.lib()
    d = _desc(desc)
    dev, ptrs, of = _model_tables(L, d, models, model_of, len(auxs), "frontend_pool_models")
    table = _frontend_pool_table(L, d, dev, auxs, conds, staged, n_news, n_receiveds, f0s, f1s, finals)
    r, E = ctypes.byref(d), len(auxs)
    floats = L.swn_frontend_pool_models_work_floats(r, table, of, E, len(models))
    if floats == 0:
        raise RuntimeError(_FP_REFUSED)
    work = torch.empty(floats, dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.swn_frontend_pool_models(r, ptrs, len(models), of, table, E, _ptr(work), _stream(dev)),
                   "frontend_pool_models")


frontend_pool_models = custom_op("swn::frontend_pool_models", mutates_args=("auxs", "conds"))(frontend_pool_models_impl)


@frontend_pool_models.register_fake
def _(models, model_of, auxs, conds, staged, n_news, n_receiveds, f0s, f1s, finals, desc):
    return None


# ------------------------------------------------------------------------------------------ decode
class DecodeImage(NamedTuple):
    """a storage format, other than fp32, of the head matrices the symmetric BL6 decode kernel streams (out_skip, out_1, the
    softmax out_2).  pack_decode_<suffix> builds its image, and decode_<suffix>, decode_chunk_<suffix> and
    decode_pool_chunk_<suffix> take it behind the packed parameters (_image_ops); the C entry points carry the same suffix."""
    name: str       # the `weights` keyword of the decode calls
    suffix: str

    def bytes(self, d) -> int:
        """of the image of net `d` (swn_decode_<suffix>_bytes); 0: the symmetric kernel does not serve the net"""
        return getattr(_lib.lib(), f"swn_decode_{self.suffix}_bytes")(ctypes.byref(d))


# bf16: the weights rounded to nearest even and re-tiled - bit-identical to the fp32 decode of runtime.bf16_weight_state_dict.
# e4m3: per output row a power-of-two scale and the nearest-even OCP FP8 E4M3 codes (runtime.e4m3_quantise), re-tiled, then one
#       fp32 2^-e per row - bit-identical to the fp32 decode of runtime.e4m3_weight_state_dict.
# A further format is a row here, its C entry points, and its instantiation of the kernel.
DECODE_IMAGES = {f.name: f for f in (DecodeImage("bf16", "w16"), DecodeImage("e4m3", "w8"))}


def _check_image(fmt: DecodeImage, image: torch.Tensor, packed: torch.Tensor, d) -> torch.Tensor:
    """the image of pack_decode_<suffix> as the *_<suffix> calls want it: uint8, contiguous, on the device of `packed`, of the
    size the net's image has (a net the symmetric BL6 kernel does not serve has none)"""
    need = fmt.bytes(d)
    if need == 0:
        raise RuntimeError(f"{fmt.name} weights exist for the nets the symmetric BL6 decode kernel serves only")
    if image.device != packed.device or image.dtype != torch.uint8 or not image.is_contiguous() or image.numel() != need:
        raise RuntimeError(f"{fmt.suffix} must be the contiguous uint8 image of pack_decode_{fmt.suffix} ({need} bytes) on the "
                           "device of the packed parameters")
    return image


def _image_entry(stem: str, fmt: Optional[DecodeImage], image, packed, d):
    """the C entry point of the decode call `stem` over weights stored as `fmt` (None: fp32: swn_<stem>, else
    swn_<stem>_<suffix>) -> (the function, its name in error texts, its arguments between the variant and the stream: the
    checked image)"""
    if fmt is None:
        return getattr(_lib.lib(), "swn_" + stem), stem, ()
    name = f"{stem}_{fmt.suffix}"
    return getattr(_lib.lib(), "swn_" + name), name, (_ptr(_check_image(fmt, image, packed, d)),)


def decode_impl(packed: torch.Tensor, cond: torch.Tensor, noise: Optional[torch.Tensor], forced: Optional[torch.Tensor],
           seed: Optional[torch.Tensor], desc: List[int], n_steps: int, variant: int, rng_seed: int, rng_utt0: int,
           want_heads: bool, want_noise: bool, utt_ids: Optional[torch.Tensor] = None
           ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """prologue + n_steps generation steps for every utterance (swn_decode).  noise None = drawn in the kernels, utterance
    b as global utterance utt_ids[b] (int32 (B), values < 2^31) or rng_utt0 + b."""
    return _decode_call(None, None, packed, cond, noise, forced, seed, desc, n_steps, variant, rng_seed, rng_utt0, want_heads,
                        want_noise, utt_ids)


def _decode_io(d, dev, cond, noise, forced, seed, utt_ids, n_steps, rng_seed, rng_utt0, want_heads, want_noise):
    """the checked inputs of the sampling loop and the outputs of decode / decode_chunk and their image forms over the
    utterances of `cond` -> (io, out, heads, used); io keeps its tensors alive"""
    soft, seg, _, _, n_out, _ = _geom(d)
    B = cond.shape[0]
    width = d.n_quantize if soft else seg
    if noise is not None:
        noise = noise.to(dev, torch.float32).contiguous()
        if tuple(noise.shape) != (B, n_steps, width):
            raise RuntimeError(f"noise shape {tuple(noise.shape)} != {(B, n_steps, width)}")
    if forced is not None:
        forced = forced.to(dev, torch.int32 if soft else torch.float32).contiguous()
        if forced.numel() != B * n_steps * seg:
            raise RuntimeError("forced history has the wrong size")
    if seed is not None:
        seed = seed.to(dev, torch.int32 if soft else torch.float32).contiguous()
        if seed.numel() != B * seg:
            raise RuntimeError(f"seed waveform has {seed.numel()} elements, expected {B * seg}")
    if utt_ids is not None:
        utt_ids = utt_ids.to(dev, torch.int32).contiguous()
        if utt_ids.numel() != B:
            raise RuntimeError(f"utt_ids has {utt_ids.numel()} elements, expected {B}")
    out = torch.empty((B, n_steps * seg), dtype=torch.int32 if soft else torch.float32, device=dev)
    heads = torch.empty((B, n_steps, n_out) if want_heads else (0,), dtype=torch.float32, device=dev)
    used = torch.empty((B, n_steps, width) if want_noise else (0,), dtype=torch.float32, device=dev)
    io = _lib.DecodeIO(noise_dev=_ptr(noise), forced_dev=_ptr(forced), seed_dev=_ptr(seed),
                       noise_out_dev=_ptr(used if want_noise else None),
                       rng_seed=int(rng_seed) & 0xFFFFFFFFFFFFFFFF, rng_utt0=int(rng_utt0) & 0xFFFFFFFF, reserved=0,
                       rng_utt_ids_dev=_ptr(utt_ids))
    io._keep = (noise, forced, seed, utt_ids)
    return io, out, heads, used


def _decode_call(fmt, image, packed, cond, noise, forced, seed, desc, n_steps, variant, rng_seed, rng_utt0, want_heads,
                 want_noise, utt_ids=None):
    """decode (fmt None: swn_decode) and decode_<suffix> over the image of a stored format (swn_decode_<suffix>)"""
    L = _lib.lib()
    d = _desc(desc)
    _need_cuda(packed, "the packed parameters")
    dev = packed.device
    B, Tf = cond.shape[0], cond.shape[1]
    cond = cond.contiguous()
    io, out, heads, used = _decode_io(d, dev, cond, noise, forced, seed, utt_ids, n_steps, rng_seed, rng_utt0, want_heads,
                                      want_noise)
    r = ctypes.byref(d)
    call, name, trail = _image_entry("decode", fmt, image, packed, d)
    # (the symmetric BL6 kernel, the only one that takes an image, keeps its state on chip)
    state = torch.empty(L.swn_decode_state_floats(r, B), dtype=torch.float32, device=dev) if fmt is None else None
    with _on(dev):
        _lib.check(call(r, _ptr(packed), _ptr(cond), B, Tf, n_steps, ctypes.byref(io), _ptr(state), _ptr(out),
                        _ptr(heads if want_heads else None), variant, *trail, _stream(dev)), name)
    return out, heads, used


decode = custom_op("swn::decode", mutates_args=())(decode_impl)


def e4m3_table_impl(like: torch.Tensor, scale: float) -> torch.Tensor:
    """what the W8 kernels' conversion helper makes of the E4M3 codes 0 .. 255 at `scale` (swn_e4m3_table): (256,) fp32 on the
    device of `like`"""
    _need_cuda(like, "the tensor that names the device")
    out = torch.empty(256, dtype=torch.float32, device=like.device)
    with _on(like.device):
        _lib.check(_lib.lib().swn_e4m3_table(_ptr(out), float(scale), _stream(like.device)), "e4m3_table")
    return out


e4m3_table = custom_op("swn::e4m3_table", mutates_args=())(e4m3_table_impl)


@e4m3_table.register_fake
def _(like, scale):
    return like.new_empty(256, dtype=torch.float32)


def _decode_fake(packed, cond, desc, n_steps, want_heads, want_noise):
    d = _desc(desc)
    soft, seg, _, _, n_out, _ = _geom(d)
    B = cond.shape[0]
    width = d.n_quantize if soft else seg
    return (packed.new_empty((B, n_steps * seg), dtype=torch.int32 if soft else torch.float32),
            packed.new_empty((B, n_steps, n_out) if want_heads else (0,)),
            packed.new_empty((B, n_steps, width) if want_noise else (0,)))


@decode.register_fake
def _decode_op_fake(packed, cond, noise, forced, seed, desc, n_steps, variant, rng_seed, rng_utt0, want_heads, want_noise, utt_ids=None):
    return _decode_fake(packed, cond, desc, n_steps, want_heads, want_noise)


# ------------------------------------------------------------------------------------------ streamed decode
def decode_chunk_impl(packed: torch.Tensor, cond: torch.Tensor, session: torch.Tensor, noise: Optional[torch.Tensor],
                      forced: Optional[torch.Tensor], seed: Optional[torch.Tensor], desc: List[int], step0: int,
                      n_steps: int, begin: bool, variant: int, rng_seed: int, rng_utt0: int, want_heads: bool,
                      want_noise: bool, utt_ids: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """steps [step0, step0 + n_steps) of a streamed decode (swn_decode_chunk): `session` (swn_decode_session_floats() fp32,
    updated in place) carries the decode state from one chunk to the next; begin=True runs the prologue (step0 0).  cond
    holds the frames final so far (absolute indexing); noise / forced / out / heads / used noise are the chunk's rows."""
    return _decode_chunk_call(None, None, packed, cond, session, noise, forced, seed, desc, step0, n_steps, begin, variant,
                              rng_seed, rng_utt0, want_heads, want_noise, utt_ids)


def _decode_chunk_call(fmt, image, packed, cond, session, noise, forced, seed, desc, step0, n_steps, begin, variant, rng_seed,
                       rng_utt0, want_heads, want_noise, utt_ids=None):
    """decode_chunk (fmt None: swn_decode_chunk) and decode_chunk_<suffix> over the image of a stored format
    (swn_decode_chunk_<suffix>)"""
    L = _lib.lib()
    d = _desc(desc)
    _need_cuda(packed, "the packed parameters")
    dev = packed.device
    B, Tf = cond.shape[0], cond.shape[1]
    cond = cond.contiguous()
    if session.device != dev or session.dtype != torch.float32 or not session.is_contiguous():
        raise RuntimeError("session must be a contiguous fp32 tensor on the device of the packed parameters")
    if session.numel() < L.swn_decode_session_floats(ctypes.byref(d), B, variant):
        raise RuntimeError("session buffer too small for this (net, batch, variant)")
    io, out, heads, used = _decode_io(d, dev, cond, noise, forced, seed, utt_ids, n_steps, rng_seed, rng_utt0, want_heads,
                                      want_noise)
    args = (ctypes.byref(d), _ptr(packed), _ptr(cond), B, Tf, int(step0), int(n_steps), _lib.CHUNK_BEGIN if begin else 0,
            ctypes.byref(io), _ptr(session), _ptr(out if n_steps > 0 else None), _ptr(heads if want_heads else None),
            int(variant))
    call, name, trail = _image_entry("decode_chunk", fmt, image, packed, d)
    with _on(dev):
        _lib.check(call(*args, *trail, _stream(dev)), name)
    return out, heads, used


decode_chunk = custom_op("swn::decode_chunk", mutates_args=("session",))(decode_chunk_impl)


@decode_chunk.register_fake
def _decode_chunk_op_fake(packed, cond, session, noise, forced, seed, desc, step0, n_steps, begin, variant, rng_seed, rng_utt0, want_heads,
      want_noise, utt_ids=None):
    return _decode_fake(packed, cond, desc, n_steps, want_heads, want_noise)


# ------------------------------------------------------------------------------------------ decode pool
def decode_pool_chunk_impl(packed: torch.Tensor, session: torch.Tensor, conds: List[torch.Tensor], slots: List[int],
                           step0s: List[int], n_steps: List[int], begins: List[bool], seeds: Optional[torch.Tensor],
                           utt_ids: List[int], desc: List[int], capacity: int, variant: int, rng_seed: int,
                           want_heads: bool, want_noise: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """one launch of a decode pool (swn_decode_pool_chunk): entry e advances the session in slot slots[e] of `session`
    (swn_decode_session_floats(capacity) fp32, updated in place) by steps [step0s[e], step0s[e] + n_steps[e]) over its own
    conditioning conds[e] (n_frames, N); begins[e] runs the prologue from seeds[e] (laplace (E, seg) fp32 | softmax (E,)
    classes; None = zeros / Q/2).  Noise is drawn on the device, keyed by rng_seed and utt_ids[e].  out / heads / used noise
    are dense (E, n_max * seg) | (E, n_max, n_out) | (E, n_max, width), n_max = max(n_steps); rows past an entry's own steps
    are not written."""
    return _decode_pool_chunk_call(None, None, packed, session, conds, slots, step0s, n_steps, begins, seeds, utt_ids, desc,
                                   capacity, variant, rng_seed, want_heads, want_noise)


def _decode_pool_chunk_call(fmt, image, packed, session, conds, slots, step0s, n_steps, begins, seeds, utt_ids, desc, capacity,
                            variant, rng_seed, want_heads, want_noise):
    """decode_pool_chunk (fmt None: swn_decode_pool_chunk) and decode_pool_chunk_<suffix> over the image of a stored format
    (swn_decode_pool_chunk_<suffix>)"""
    d = _desc(desc)
    _need_cuda(packed, "the packed parameters")
    call, _, trail = _image_entry("decode_pool_chunk", fmt, image, packed, d)
    return _decode_pool_call(call, d, packed.device, (_ptr(packed),), trail, session, conds, slots, step0s, n_steps, begins,
                             seeds, utt_ids, capacity, variant, rng_seed, want_heads, want_noise)


def _decode_pool_call(call, d, dev, lead, trail, session, conds, slots, step0s, n_steps, begins, seeds, utt_ids, capacity,
                      variant, rng_seed, want_heads, want_noise, max_entries: int = _lib.DECODE_POOL_MAX_ENTRIES,
                      what: str = "decode_pool_chunk"):
    """one pool launch through the library's `call` (decode_pool_chunk and its image / *_models / wide forms): checks the
    entries and builds their table, the io block and the outputs.  `lead` are the call's arguments between the descriptor and
    the capacity (the packed parameters, or the model tables), `trail` those between the variant and the stream (the image; the
    wide call: images, format and table buffer), max_entries the call's limit, `what` the op's name in error texts"""
    L = _lib.lib()
    soft, seg, _, _, n_out, _ = _geom(d)
    E = len(conds)
    if not (len(slots) == len(step0s) == len(n_steps) == len(begins) == len(utt_ids) == E):
        raise RuntimeError(f"{what}: conds, slots, step0s, n_steps, begins and utt_ids must have one entry each")
    if not 1 <= E <= max_entries:
        raise RuntimeError(f"{what}: {E} entries, a launch takes 1 .. {max_entries}")
    width = d.n_quantize if soft else seg
    if session.device != dev or session.dtype != torch.float32 or not session.is_contiguous():
        raise RuntimeError("session must be a contiguous fp32 tensor on the device of the packed parameters")
    if session.numel() < L.swn_decode_session_floats(ctypes.byref(d), int(capacity), int(variant)):
        raise RuntimeError("session buffer too small for this (net, capacity, variant)")
    table = (_lib.DecodePoolEntry * E)()
    for e, c in enumerate(conds):
        if c.device != dev or c.dtype != torch.float32 or not c.is_contiguous() or c.dim() != 2:
            raise RuntimeError("every cond buffer must be a contiguous (n_frames, N) fp32 tensor on the device")
        table[e] = _lib.DecodePoolEntry(cond_dev=c.data_ptr(), n_frames=int(c.shape[0]), slot=int(slots[e]),
                                        step0=int(step0s[e]), n_steps=int(n_steps[e]),
                                        flags=_lib.CHUNK_BEGIN if begins[e] else 0, reserved=0)
    if seeds is not None:
        seeds = seeds.to(dev, torch.int32 if soft else torch.float32).contiguous()
        if seeds.numel() != E * seg:
            raise RuntimeError(f"seeds have {seeds.numel()} elements, expected {E * seg}")
    ids = torch.tensor([int(u) & 0xFFFFFFFF for u in utt_ids], dtype=torch.int64).to(torch.int32).to(dev)
    n_max = max(int(n) for n in n_steps)
    out = torch.empty((E, n_max * seg), dtype=torch.int32 if soft else torch.float32, device=dev)
    heads = torch.empty((E, n_max, n_out) if want_heads else (0,), dtype=torch.float32, device=dev)
    used = torch.empty((E, n_max, width) if want_noise else (0,), dtype=torch.float32, device=dev)
    io = _lib.DecodeIO(noise_dev=None, forced_dev=None, seed_dev=_ptr(seeds),
                       noise_out_dev=_ptr(used if want_noise else None),
                       rng_seed=int(rng_seed) & 0xFFFFFFFFFFFFFFFF, rng_utt0=0, reserved=0, rng_utt_ids_dev=_ptr(ids))
    with _on(dev):
        _lib.check(call(ctypes.byref(d), *lead, int(capacity), table, E, ctypes.byref(io), _ptr(session),
                        _ptr(out if n_max > 0 else None), _ptr(heads if want_heads else None), int(variant), *trail,
                        _stream(dev)), call.__name__[len("swn_"):])
    return out, heads, used


decode_pool_chunk = custom_op("swn::decode_pool_chunk", mutates_args=("session",))(decode_pool_chunk_impl)


@decode_pool_chunk.register_fake
def _decode_pool_chunk_op_fake(packed, session, conds, slots, step0s, n_steps, begins, seeds, utt_ids, desc, capacity, variant, rng_seed,
      want_heads, want_noise):
    return _decode_pool_fake(packed, conds, n_steps, desc, want_heads, want_noise)


def _decode_pool_fake(packed, conds, n_steps, desc, want_heads, want_noise):
    d = _desc(desc)
    soft, seg, _, _, n_out, _ = _geom(d)
    E, n_max = len(conds), max(int(n) for n in n_steps)
    width = d.n_quantize if soft else seg
    return (packed.new_empty((E, n_max * seg), dtype=torch.int32 if soft else torch.float32),
            packed.new_empty((E, n_max, n_out) if want_heads else (0,)),
            packed.new_empty((E, n_max, width) if want_noise else (0,)))


def decode_pool_chunk_models_impl(models: List[torch.Tensor], model_of: List[int], session: torch.Tensor,
                                  conds: List[torch.Tensor], slots: List[int], step0s: List[int], n_steps: List[int],
                                  begins: List[bool], seeds: Optional[torch.Tensor], utt_ids: List[int], desc: List[int],
                                  capacity: int, variant: int, rng_seed: int, want_heads: bool, want_noise: bool
                                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """decode_pool_chunk over sessions of several models of one geometry (swn_decode_pool_chunk_models): entry e runs with the
    packed parameters models[model_of[e]] (at most 16 models per call); everything else as decode_pool_chunk, and every
    entry's rows bit-identical to decode_pool_chunk with that entry's model."""
    return _decode_pool_chunk_models_call(None, None, models, model_of, session, conds, slots, step0s, n_steps, begins, seeds,
                                          utt_ids, desc, capacity, variant, rng_seed, want_heads, want_noise)


def _decode_pool_chunk_models_call(fmt, images, models, model_of, session, conds, slots, step0s, n_steps, begins, seeds, utt_ids,
                                   desc, capacity, variant, rng_seed, want_heads, want_noise):
    """decode_pool_chunk_models (fmt None: swn_decode_pool_chunk_models) and decode_pool_chunk_models_<suffix> over one image
    of a stored format per model (swn_decode_pool_chunk_models_<suffix>): images[m] is the image of models[m]"""
    d = _desc(desc)
    L = _lib.lib()
    name = "decode_pool_chunk_models" + ("" if fmt is None else f"_{fmt.suffix}")
    dev, ptrs, of = _model_tables(L, d, models, model_of, len(conds), name)
    trail = ()
    if fmt is not None:
        if len(images) != len(models):
            raise RuntimeError(f"{name}: {len(images)} images for {len(models)} models")
        trail = ((ctypes.c_void_p * len(models))(*[_check_image(fmt, im, t, d).data_ptr() for im, t in zip(images, models)]),)
    return _decode_pool_call(getattr(L, "swn_" + name), d, dev, (ptrs, len(models), of), trail, session, conds, slots, step0s,
                             n_steps, begins, seeds, utt_ids, capacity, variant, rng_seed, want_heads, want_noise)


decode_pool_chunk_models = custom_op("swn::decode_pool_chunk_models",
                                     mutates_args=("session",))(decode_pool_chunk_models_impl)


@decode_pool_chunk_models.register_fake
def _decode_pool_chunk_models_op_fake(models, model_of, session, conds, slots, step0s, n_steps, begins, seeds, utt_ids, desc,
                                      capacity, variant, rng_seed, want_heads, want_noise):
    return _decode_pool_fake(models[0], conds, n_steps, desc, want_heads, want_noise)


# ------------------------------------------------------------------------------------------ wide decode pool launch
_WIDE_FORMATS = {"fp32": _lib.WEIGHTS_FP32, "bf16": _lib.WEIGHTS_BF16, "e4m3": _lib.WEIGHTS_E4M3}


def decode_pool_chunk_wide_impl(models: List[torch.Tensor], images: List[torch.Tensor], weights: str, model_of: List[int],
                                session: torch.Tensor, conds: List[torch.Tensor], slots: List[int], step0s: List[int],
                                n_steps: List[int], begins: List[bool], seeds: Optional[torch.Tensor], utt_ids: List[int],
                                desc: List[int], capacity: int, variant: int, rng_seed: int, want_heads: bool,
                                want_noise: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """one WIDE launch of a decode pool (swn_decode_pool_chunk_wide): up to 256 entries, their table in a device buffer this op
    allocates per call (as it does out and heads, so the caching allocator's stream rules keep it alive for the launches).
    Entry e runs with models[model_of[e]] - one model or any number up to the entries' - and, for weights "bf16" | "e4m3",
    images[model_of[e]] (the images of pack_decode_w16 / _w8, one per model; weights "fp32": images is empty).  Everything
    else, and every entry's rows bit for bit, as decode_pool_chunk / decode_pool_chunk_models and their stored forms."""
    d = _desc(desc)
    L = _lib.lib()
    E = len(conds)
    if weights not in _WIDE_FORMATS:
        raise RuntimeError(f"decode_pool_chunk_wide: weights must be one of {sorted(_WIDE_FORMATS)}, not {weights!r}")
    dev, ptrs, of = _model_tables(L, d, models, model_of, E, "decode_pool_chunk_wide", _lib.DECODE_POOL_WIDE_MAX_ENTRIES)
    imgs = None
    if weights != "fp32":
        if len(images) != len(models):
            raise RuntimeError(f"decode_pool_chunk_wide: {len(images)} images for {len(models)} models")
        fmt = DECODE_IMAGES[weights]
        imgs = (ctypes.c_void_p * len(models))(*[_check_image(fmt, im, t, d).data_ptr() for im, t in zip(images, models)])
    elif len(images) != 0:
        raise RuntimeError("decode_pool_chunk_wide: fp32 weights take no images")
    table = torch.empty(max(1, L.swn_decode_pool_wide_table_bytes(E)), dtype=torch.uint8, device=dev)
    return _decode_pool_call(L.swn_decode_pool_chunk_wide, d, dev, (ptrs, len(models), of),
                             (imgs, _WIDE_FORMATS[weights], _ptr(table)), session, conds, slots, step0s, n_steps, begins, seeds,
                             utt_ids, capacity, variant, rng_seed, want_heads, want_noise, _lib.DECODE_POOL_WIDE_MAX_ENTRIES,
                             "decode_pool_chunk_wide")


decode_pool_chunk_wide = custom_op("swn::decode_pool_chunk_wide", mutates_args=("session",))(decode_pool_chunk_wide_impl)


@decode_pool_chunk_wide.register_fake
def _decode_pool_chunk_wide_op_fake(models, images, weights, model_of, session, conds, slots, step0s, n_steps, begins, seeds,
                                    utt_ids, desc, capacity, variant, rng_seed, want_heads, want_noise):
    return _decode_pool_fake(models[0], conds, n_steps, desc, want_heads, want_noise)


def decode_wide_lead(nets, weights: str):
    """the leading arguments of decode_pool_chunk_wide for the models `nets` with weights stored as `weights`: their packed
    parameters, their images of the format (none for fp32) - both read now, so a repacked net brings its new ones - and the
    format's name"""
    if weights == "fp32":
        return [n.packed for n in nets], [], weights
    suffix = DECODE_IMAGES[weights].suffix
    return [n.packed for n in nets], [getattr(n, f"decode_{suffix}_image")() for n in nets], weights


# ------------------------------------------------------------------------------------------ decode over a stored format
def _image_ops(fmt: DecodeImage) -> dict:
    """registers the five ops of a stored format -> {name: op, name_impl: function}: pack_decode_<suffix>(packed, desc) -> the
    image, uint8; and decode_<suffix>, decode_chunk_<suffix>, decode_pool_chunk_<suffix>, decode_pool_chunk_models_<suffix>:
    the fp32 ops with the image (the models form: one image per model, Tensor[]) as their second argument (named <suffix>), in
    everything else - annotations, defaults, the mutated session - the fp32 signature.
    The variant must resolve to the symmetric BL6 kernel (6 for the single-sample Laplace nets); the chunks of a stream
    concatenate to the one-shot decode of the format bit for bit, and a pool entry's rows are those of its session alone."""
    s = fmt.suffix

    def pack_impl(packed: torch.Tensor, desc: List[int]) -> torch.Tensor:
        d = _desc(desc)
        _need_cuda(packed, "the packed parameters")
        n = fmt.bytes(d)
        if n == 0:
            raise RuntimeError(f"{fmt.name} weights exist for the nets the symmetric BL6 decode kernel serves only")
        image = torch.empty(n, dtype=torch.uint8, device=packed.device)
        with _on(packed.device):
            _lib.check(getattr(_lib.lib(), f"swn_pack_decode_{s}")(ctypes.byref(d), _ptr(packed), _ptr(image),
                                                                   _stream(packed.device)), f"pack_decode_{s}")
        return image

    made = {f"pack_decode_{s}_impl": pack_impl, f"pack_decode_{s}": custom_op(f"swn::pack_decode_{s}", pack_impl, mutates_args=())}
    made[f"pack_decode_{s}"].register_fake(lambda packed, desc: packed.new_empty(fmt.bytes(_desc(desc)), dtype=torch.uint8))

    def image_form(fp32_impl, call, fake, mutates):
        def impl(packed, image, *args, **kw):
            return call(fmt, image, packed, *args, **kw)

        sig = inspect.signature(fp32_impl)                  # what the op's schema is inferred from
        par = list(sig.parameters.values())
        impl.__signature__ = sig.replace(parameters=par[:1] + [par[0].replace(name=s)] + par[1:])
        name = f"{fp32_impl.__name__[:-len('_impl')]}_{s}"
        impl.__name__ = impl.__qualname__ = name + "_impl"
        made[name + "_impl"] = impl
        made[name] = custom_op(f"swn::{name}", impl, mutates_args=mutates)
        made[name].register_fake(lambda packed, image, *args, **kw: fake(packed, *args, **kw))

    image_form(decode_impl, _decode_call, _decode_op_fake, ())
    image_form(decode_chunk_impl, _decode_chunk_call, _decode_chunk_op_fake, ("session",))
    image_form(decode_pool_chunk_impl, _decode_pool_chunk_call, _decode_pool_chunk_op_fake, ("session",))
    # ... and the pool over several models: `models` first, then one image per model (Tensor[] <suffix>)
    image_form(decode_pool_chunk_models_impl, _decode_pool_chunk_models_call, _decode_pool_chunk_models_op_fake, ("session",))
    return made


for _fmt in DECODE_IMAGES.values():
    globals().update(_image_ops(_fmt))


def decode_lead(net, op: str, weights: str):
    """the name of the op of torch.ops.swn that runs the decode call `op` ("decode" | "decode_chunk" | "decode_pool_chunk") of
    `net` (a runtime.HipNet) with weights stored as `weights` ("fp32" or a key of DECODE_IMAGES, checked by
    runtime.check_decode_weights), and the op's leading arguments: the packed parameters and, unless fp32, the format's image
    (net.decode_<suffix>_image())"""
    if weights == "fp32":
        return op, (net.packed,)
    suffix = DECODE_IMAGES[weights].suffix
    return f"{op}_{suffix}", (net.packed, getattr(net, f"decode_{suffix}_image")())


def decode_models_lead(nets, op: str, weights: str):
    """decode_lead for a call over several models (op: "decode_pool_chunk_models"): the op's name and its leading arguments, the
    nets' packed parameters and, unless fp32, their images of the format - both read now, so a repacked net brings its new ones"""
    if weights == "fp32":
        return op, ([n.packed for n in nets],)
    suffix = DECODE_IMAGES[weights].suffix
    return f"{op}_{suffix}", ([n.packed for n in nets], [getattr(n, f"decode_{suffix}_image")() for n in nets])


def stepped_pool_session_floats(d, capacity: int) -> int:
    """floats of a stepped pool's session buffer: the slots (swn_decode_session_floats(capacity, 3)) and the device copy of
    each call's entry table; 0 when the stepped chain does not run the net at this capacity"""
    n = int(_lib.lib().swn_decode_session_floats(ctypes.byref(d), int(capacity), 3))
    return n + _lib.DECODE_STEPPED_POOL_TABLE_FLOATS if n > 0 else 0


def _gen_steps(it0: int, n_it: int, n_pro: int) -> int:
    """generation steps among iterations [it0, it0 + n_it)"""
    return max(0, it0 + n_it - max(it0, n_pro))


def decode_pool_stepped_chunk_impl(packed: torch.Tensor, session: torch.Tensor, conds: List[torch.Tensor],
                                   slots: List[int], it0s: List[int], n_its: List[int], begins: List[bool],
                                   seeds: Optional[torch.Tensor], utt_ids: List[int], desc: List[int], capacity: int,
                                   rng_seed: int, want_heads: bool, want_noise: bool
                                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """one call of a stepped decode pool (swn_decode_pool_stepped_chunk): entry e runs iterations [it0s[e], it0s[e] + n_its[e])
    (prologue positions, then generation steps) of the session in slot slots[e] of `session` (stepped_pool_session_floats()
    fp32, updated in place) over its own conditioning conds[e] (n_frames, N); begins[e] zeroes and seeds that slot from
    seeds[e] (laplace (E, seg) fp32 | softmax (E,) classes; None = zeros / Q/2).  out / heads / used noise are dense
    (E, n_max * seg) | (E, n_max, n_out) | (E, n_max, width) over the entries' generation steps, n_max = their maximum."""
    L = _lib.lib()
    d = _desc(desc)
    _need_cuda(packed, "the packed parameters")
    dev = packed.device
    table, io, out, heads, used, n_max = _stepped_pool_args(L, d, dev, session, conds, slots, it0s, n_its, begins, seeds,
                                                            utt_ids, capacity, rng_seed, want_heads, want_noise,
                                                            stepped_pool_session_floats(d, int(capacity)))
    with _on(dev):
        _lib.check(L.swn_decode_pool_stepped_chunk(ctypes.byref(d), _ptr(packed), int(capacity), table, len(conds),
                                                   ctypes.byref(io), _ptr(session), _ptr(out if n_max > 0 else None),
                                                   _ptr(heads if want_heads else None), _stream(dev)),
                   "decode_pool_stepped_chunk")
    return out, heads, used


def _stepped_pool_args(L, d, dev, session, conds, slots, it0s, n_its, begins, seeds, utt_ids, capacity, rng_seed, want_heads,
                       want_noise, need):
    """the checked entry table, io block and outputs of a stepped pool call (decode_pool_stepped_chunk and
    decode_pool_stepped_chunk_models) -> (table, io, out, heads, used, n_max); io keeps the seeds and ids alive.  need: floats
    the call's session buffer holds (0 = the stepped chain does not run the net at this capacity)"""
    soft, seg, _, _, n_out, _ = _geom(d)
    E = len(conds)
    if not (len(slots) == len(it0s) == len(n_its) == len(begins) == len(utt_ids) == E):
        raise RuntimeError("decode_pool_stepped_chunk: conds, slots, it0s, n_its, begins and utt_ids must have one entry each")
    if not 1 <= E <= _lib.DECODE_POOL_MAX_ENTRIES:
        raise RuntimeError(f"decode_pool_stepped_chunk: {E} entries, a call takes 1 .. {_lib.DECODE_POOL_MAX_ENTRIES}")
    width = d.n_quantize if soft else seg
    if session.device != dev or session.dtype != torch.float32 or not session.is_contiguous():
        raise RuntimeError("session must be a contiguous fp32 tensor on the device of the packed parameters")
    if need == 0:
        raise RuntimeError("decode_pool_stepped_chunk: the stepped decode does not run this net at this capacity")
    if session.numel() < need:
        raise RuntimeError("session buffer too small for this (net, capacity)")
    table = (_lib.DecodeSteppedPoolEntry * E)()
    for e, c in enumerate(conds):
        if c.device != dev or c.dtype != torch.float32 or not c.is_contiguous() or c.dim() != 2:
            raise RuntimeError("every cond buffer must be a contiguous (n_frames, N) fp32 tensor on the device")
        table[e] = _lib.DecodeSteppedPoolEntry(cond_dev=c.data_ptr(), n_frames=int(c.shape[0]), slot=int(slots[e]),
                                               it0=int(it0s[e]), n_it=int(n_its[e]),
                                               flags=_lib.CHUNK_BEGIN if begins[e] else 0, reserved=0)
    if seeds is not None:
        seeds = seeds.to(dev, torch.int32 if soft else torch.float32).contiguous()
        if seeds.numel() != E * seg:
            raise RuntimeError(f"seeds have {seeds.numel()} elements, expected {E * seg}")
    ids = torch.tensor([int(u) & 0xFFFFFFFF for u in utt_ids], dtype=torch.int64).to(torch.int32).to(dev)
    n_pro = int(L.swn_decode_stepped_prologue_iterations(ctypes.byref(d)))
    n_max = max(_gen_steps(int(i), int(n), n_pro) for i, n in zip(it0s, n_its))
    out = torch.empty((E, n_max * seg), dtype=torch.int32 if soft else torch.float32, device=dev)
    heads = torch.empty((E, n_max, n_out) if want_heads else (0,), dtype=torch.float32, device=dev)
    used = torch.empty((E, n_max, width) if want_noise else (0,), dtype=torch.float32, device=dev)
    io = _lib.DecodeIO(noise_dev=None, forced_dev=None, seed_dev=_ptr(seeds),
                       noise_out_dev=_ptr(used if want_noise else None),
                       rng_seed=int(rng_seed) & 0xFFFFFFFFFFFFFFFF, rng_utt0=0, reserved=0, rng_utt_ids_dev=_ptr(ids))
    io._keep = (seeds, ids)
    return table, io, out, heads, used, n_max


decode_pool_stepped_chunk = custom_op("swn::decode_pool_stepped_chunk", mutates_args=("session",))(
    decode_pool_stepped_chunk_impl)


@decode_pool_stepped_chunk.register_fake
def _(packed, session, conds, slots, it0s, n_its, begins, seeds, utt_ids, desc, capacity, rng_seed, want_heads,
      want_noise):
    return _stepped_pool_fake(packed, conds, it0s, n_its, desc, want_heads, want_noise)


def _stepped_pool_fake(packed, conds, it0s, n_its, desc, want_heads, want_noise):
    d = _desc(desc)
    soft, seg, _, _, n_out, _ = _geom(d)
    n_pro = int(_lib.lib().swn_decode_stepped_prologue_iterations(ctypes.byref(d)))
    E, n_max = len(conds), max(_gen_steps(int(i), int(n), n_pro) for i, n in zip(it0s, n_its))
    width = d.n_quantize if soft else seg
    return (packed.new_empty((E, n_max * seg), dtype=torch.int32 if soft else torch.float32),
            packed.new_empty((E, n_max, n_out) if want_heads else (0,)),
            packed.new_empty((E, n_max, width) if want_noise else (0,)))


def stepped_pool_models_session_floats(d, capacity: int) -> int:
    """floats of the session buffer of a stepped pool over several models: the slots of stepped_pool_session_floats and the
    wider table rows of swn_decode_pool_stepped_chunk_models (the single-model call serves such a buffer too); 0 when the
    stepped chain does not run the net at this capacity"""
    n = int(_lib.lib().swn_decode_session_floats(ctypes.byref(d), int(capacity), 3))
    return n + _lib.DECODE_STEPPED_POOL_MODELS_TABLE_FLOATS if n > 0 else 0


def decode_pool_stepped_chunk_models_impl(models: List[torch.Tensor], model_of: List[int], session: torch.Tensor,
                                          conds: List[torch.Tensor], slots: List[int], it0s: List[int], n_its: List[int],
                                          begins: List[bool], seeds: Optional[torch.Tensor], utt_ids: List[int],
                                          desc: List[int], capacity: int, rng_seed: int, want_heads: bool, want_noise: bool
                                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """decode_pool_stepped_chunk over sessions of several models of one geometry (swn_decode_pool_stepped_chunk_models): entry
    e runs with the packed parameters models[model_of[e]] (at most 16 models per call) in the same launches as the others;
    `session` holds stepped_pool_models_session_floats() floats.  Everything else as decode_pool_stepped_chunk, and every
    entry's rows bit-identical to decode_pool_stepped_chunk with that entry's model."""
    L = _lib.lib()
    d = _desc(desc)
    dev, ptrs, of = _model_tables(L, d, models, model_of, len(conds), "decode_pool_stepped_chunk_models")
    table, io, out, heads, used, n_max = _stepped_pool_args(L, d, dev, session, conds, slots, it0s, n_its, begins, seeds,
                                                            utt_ids, capacity, rng_seed, want_heads, want_noise,
                                                            stepped_pool_models_session_floats(d, int(capacity)))
    with _on(dev):
        _lib.check(L.swn_decode_pool_stepped_chunk_models(ctypes.byref(d), ptrs, len(models), of, int(capacity), table,
                                                          len(conds), ctypes.byref(io), _ptr(session),
                                                          _ptr(out if n_max > 0 else None),
                                                          _ptr(heads if want_heads else None), _stream(dev)),
                   "decode_pool_stepped_chunk_models")
    return out, heads, used


decode_pool_stepped_chunk_models = custom_op("swn::decode_pool_stepped_chunk_models", mutates_args=("session",))(
    decode_pool_stepped_chunk_models_impl)


@decode_pool_stepped_chunk_models.register_fake
def _(models, model_of, session, conds, slots, it0s, n_its, begins, seeds, utt_ids, desc, capacity, rng_seed, want_heads,
      want_noise):
    return _stepped_pool_fake(models[0], conds, it0s, n_its, desc, want_heads, want_noise)


def stepped_prologue_work_floats(d, n_entries: int) -> int:
    """floats of scratch a parallel prologue call over n_entries sessions needs (swn_decode_stepped_prologue_work_floats); 0
    when the stepped chain does not run the net"""
    return int(_lib.lib().swn_decode_stepped_prologue_work_floats(ctypes.byref(d), int(n_entries)))


def decode_stepped_prologue_impl(models: List[torch.Tensor], model_of: List[int], session: torch.Tensor,
                                 conds: List[torch.Tensor], slots: List[int], seeds: Optional[torch.Tensor],
                                 desc: List[int], n_slots: int) -> None:
    """the prologue of new sessions of the stepped decode in parallel launches (swn_decode_stepped_prologue): entry e zeroes
    slot slots[e] of `session` (the session of a DecodeStream of batch n_slots on variant 3, or a stepped pool's of capacity
    n_slots; updated in place), seeds it from seeds[e] (laplace (E, seg) fp32 | softmax (E,) classes; None = zeros / Q/2) and
    fills its history rings over conds[e] (n_frames, N) - every float of the slot as a BEGIN entry of
    decode_pool_stepped_chunk with it0 = 0, n_it = n_pro leaves it.  models: one packed buffer for all entries (model_of is
    then ignored), or up to 16 with model_of[e] naming entry e's.  Other slots are not touched."""
    L = _lib.lib()
    d = _desc(desc)
    E = len(conds)
    if len(slots) != E:
        raise RuntimeError("decode_stepped_prologue: conds and slots must have one entry each")
    if not 1 <= E <= _lib.DECODE_POOL_MAX_ENTRIES:
        raise RuntimeError(f"decode_stepped_prologue: {E} entries, a call takes 1 .. {_lib.DECODE_POOL_MAX_ENTRIES}")
    if len(models) == 1:
        _need_cuda(models[0], "the packed parameters")
        dev, packed, ptrs, of, n_models = models[0].device, models[0], None, None, 0
    else:
        dev, ptrs, of = _model_tables(L, d, models, model_of, E, "decode_stepped_prologue")
        packed, n_models = None, len(models)
    soft, seg, _, _, _, _ = _geom(d)
    if session.device != dev or session.dtype != torch.float32 or not session.is_contiguous():
        raise RuntimeError("session must be a contiguous fp32 tensor on the device of the packed parameters")
    need = int(L.swn_decode_session_floats(ctypes.byref(d), int(n_slots), 3)) if int(n_slots) >= 1 else 0
    work_floats = stepped_prologue_work_floats(d, E)
    if need == 0 or work_floats == 0:
        raise RuntimeError("decode_stepped_prologue: the stepped decode does not run this net with this many slots")
    if session.numel() < need:
        raise RuntimeError("session buffer too small for this (net, n_slots)")
    table = (_lib.DecodeSteppedPrologueEntry * E)()
    for e, c in enumerate(conds):
        if c.device != dev or c.dtype != torch.float32 or not c.is_contiguous() or c.dim() != 2:
            raise RuntimeError("every cond buffer must be a contiguous (n_frames, N) fp32 tensor on the device")
        table[e] = _lib.DecodeSteppedPrologueEntry(cond_dev=c.data_ptr(), n_frames=int(c.shape[0]), slot=int(slots[e]))
    if seeds is not None:
        seeds = seeds.to(dev, torch.int32 if soft else torch.float32).contiguous()
        if seeds.numel() != E * seg:
            raise RuntimeError(f"seeds have {seeds.numel()} elements, expected {E * seg}")
    work = torch.empty(work_floats, dtype=torch.float32, device=dev)
    io = _lib.DecodeIO(noise_dev=None, forced_dev=None, seed_dev=_ptr(seeds), noise_out_dev=None, rng_seed=0, rng_utt0=0,
                       reserved=0, rng_utt_ids_dev=None)
    with _on(dev):
        _lib.check(L.swn_decode_stepped_prologue(ctypes.byref(d), _ptr(packed), ptrs, n_models, of, int(n_slots), table, E,
                                                 ctypes.byref(io), _ptr(session), _ptr(work), _stream(dev)),
                   "decode_stepped_prologue")


decode_stepped_prologue = custom_op("swn::decode_stepped_prologue", mutates_args=("session",))(decode_stepped_prologue_impl)


@decode_stepped_prologue.register_fake
def _(models, model_of, session, conds, slots, seeds, desc, n_slots):
    return None


def stepped_pool_plan(model_of: List[int], n_its: List[int], n_models: int, j: int = 0) -> Tuple[List[int], List[tuple]]:
    """the grouping swn_decode_pool_stepped_chunk_models launches by (swn_decode_stepped_pool_plan; pure host arithmetic) ->
    (table order, [(first table row, rows, model)] of the tiles of tick-local iteration j)"""
    E = len(model_of)
    if len(n_its) != E:
        raise RuntimeError("stepped_pool_plan: model_of and n_its must have one entry each")
    order = (ctypes.c_int32 * max(E, 1))()
    tiles = (ctypes.c_int32 * (3 * _lib.DECODE_STEPPED_POOL_MAX_TILES))()
    nt = _lib.lib().swn_decode_stepped_pool_plan((ctypes.c_int32 * max(E, 1))(*[int(m) for m in model_of]),
                                                 (ctypes.c_int32 * max(E, 1))(*[int(n) for n in n_its]), E, int(n_models),
                                                 int(j), order, tiles)
    _lib.check(min(nt, 0), "stepped_pool_plan")
    return list(order[:E]), [tuple(tiles[3 * t:3 * t + 3]) for t in range(nt)]


# ------------------------------------------------------------------------------------------ noise-shaping post-filter
def postfilter_chunk_impl(image: torch.Tensor, state: torch.Tensor, inputs: List[torch.Tensor], slots: List[int],
                          resets: List[bool], order: int, alpha: float, pade: int, n_taps: int,
                          capacity: int) -> torch.Tensor:
    """one call of the device post-filter (swn_postfilter_chunk): entry e filters inputs[e] (1-D: fp32 samples | int32 mu-law
    classes) as the next chunk of the session in slot slots[e] of `state` (capacity * swn_postfilter_state_doubles() fp64,
    updated in place); resets[e] starts that slot from zero state.  image: fp64 [b (order + 1) | FIR taps (n_taps) | mu-law
    table (SWN_POSTFILTER_MULAW_ENTRIES), only needed for class inputs].  -> (E, n_max) fp32, rows past an entry's own length
    not written."""
    L = _lib.lib()
    dev = image.device
    _need_cuda(image, "the filter image")
    E = len(inputs)
    if not (len(slots) == len(resets) == E):
        raise RuntimeError("postfilter_chunk: inputs, slots and resets must have one entry each")
    if image.dtype != torch.float64 or not image.is_contiguous() or image.dim() != 1:
        raise RuntimeError("postfilter_chunk: the filter image must be a contiguous 1-D fp64 tensor")
    base = int(order) + 1 + int(n_taps)
    has_mulaw = image.numel() == base + _lib.POSTFILTER_MULAW_ENTRIES
    if image.numel() != base and not has_mulaw:
        raise RuntimeError(f"postfilter_chunk: the filter image has {image.numel()} values, expected {base} "
                           f"(+ {_lib.POSTFILTER_MULAW_ENTRIES} with a mu-law table)")
    per = int(L.swn_postfilter_state_doubles(int(order), int(pade), int(n_taps)))
    if state.device != dev or state.dtype != torch.float64 or not state.is_contiguous() or state.numel() < per * int(capacity):
        raise RuntimeError("postfilter_chunk: state must be a contiguous fp64 tensor of capacity * "
                           "swn_postfilter_state_doubles() values on the device of the image")
    ins = []
    for x in inputs:
        if x.device != dev or x.dim() != 1 or x.dtype not in (torch.float32, torch.int32):
            raise RuntimeError("postfilter_chunk: every input must be a 1-D fp32 or int32 tensor on the device")
        ins.append(x.contiguous())
    n_max = max((x.numel() for x in ins), default=0)
    out = torch.empty((E, n_max), dtype=torch.float32, device=dev)
    table = (_lib.PostfilterEntry * max(E, 1))()
    for e, x in enumerate(ins):
        n = x.numel()
        table[e] = _lib.PostfilterEntry(in_dev=x.data_ptr() if n else None, out_dev=out[e].data_ptr() if n else None,
                                        slot=int(slots[e]), n=n,
                                        kind=_lib.POSTFILTER_IN_MULAW if x.dtype == torch.int32 else _lib.POSTFILTER_IN_F32,
                                        flags=_lib.POSTFILTER_RESET if resets[e] else 0)
    b = image[: int(order) + 1]
    taps = image[int(order) + 1: base]
    with _on(dev):
        _lib.check(L.swn_postfilter_chunk(int(order), float(alpha), int(pade), _ptr(b), int(n_taps), _ptr(taps),
                                          _ptr(image[base:] if has_mulaw else None), _ptr(state), int(capacity), table, E,
                                          _stream(dev)), "postfilter_chunk")
    return out


postfilter_chunk = custom_op("swn::postfilter_chunk", mutates_args=("state",))(postfilter_chunk_impl)


@postfilter_chunk.register_fake
def _(image, state, inputs, slots, resets, order, alpha, pade, n_taps, capacity):
    return image.new_empty((len(inputs), max((x.numel() for x in inputs), default=0)), dtype=torch.float32)


# ------------------------------------------------------------------------------------------ teacher-forced stack
def _tp(d, Tf: int) -> Tuple[int, int]:
    soft, seg, *_ = _geom(d)
    T = Tf * d.upsampling_factor
    return T, (T - 1 if soft else T - 2 * seg + 1)


def stack_forward_impl(packed: torch.Tensor, cond: torch.Tensor, audio: torch.Tensor, desc: List[int],
                  want_hidden: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """raw out_2 outputs (B, n_out, Tp) of the fp32 parity kernels, the work buffer swn_backward reads, and
    optionally the hidden states (B, L+1, H, Tp) (swn_forward)."""
    Lb = _lib.lib()
    d = _desc(desc)
    _need_cuda(packed, "the packed parameters")
    dev = packed.device
    soft, seg, L, H, n_out, _ = _geom(d)
    B, Tf = cond.shape[0], cond.shape[1]
    T, Tp = _tp(d, Tf)
    audio = audio.to(dev, torch.int32 if soft else torch.float32).contiguous()
    if audio.numel() != B * (T - seg):
        raise RuntimeError(f"audio has {audio.numel()} elements, expected {B * (T - seg)}")
    r = ctypes.byref(d)
    work = torch.empty(Lb.swn_forward_work_floats(r, B, Tf), dtype=torch.float32, device=dev)
    out = torch.empty((B, n_out, Tp), dtype=torch.float32, device=dev)
    hs = torch.empty((B, L + 1, H, Tp) if want_hidden else (0,), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(Lb.swn_forward(r, _ptr(packed), _ptr(cond.contiguous()), _ptr(audio), B, Tf, _ptr(work), _ptr(out),
                                  _ptr(hs if want_hidden else None), _stream(dev)), "forward")
    return out, work, hs


stack_forward = custom_op("swn::stack_forward", mutates_args=())(stack_forward_impl)


@stack_forward.register_fake
def _(packed, cond, audio, desc, want_hidden):
    Lb, d = _lib.lib(), _desc(desc)
    _, _, L, H, n_out, _ = _geom(d)
    B, Tf = cond.shape[0], cond.shape[1]
    _, Tp = _tp(d, Tf)
    return (packed.new_empty((B, n_out, Tp)), packed.new_empty(Lb.swn_forward_work_floats(ctypes.byref(d), B, Tf)),
            packed.new_empty((B, L + 1, H, Tp) if want_hidden else (0,)))


def pack_bf16_impl(packed: torch.Tensor, desc: List[int]) -> torch.Tensor:
    """bf16 weight images of the MFMA stacks (swn_pack_bf16); raises where the geometry has no bf16 stack."""
    Lb = _lib.lib()
    d = _desc(desc)
    _need_cuda(packed, "the packed parameters")
    r = ctypes.byref(d)
    nbytes = Lb.swn_bf16_weight_bytes(r)
    if nbytes == 0:
        raise RuntimeError("bf16 stack kernels are built for the BL6-class and the H%64==0 Laplace geometries only")
    w = torch.empty(nbytes, dtype=torch.uint8, device=packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(Lb.swn_pack_bf16(r, _ptr(packed), _ptr(w), _stream(packed.device)), "pack_bf16")
    return w


pack_bf16 = custom_op("swn::pack_bf16", mutates_args=())(pack_bf16_impl)


@pack_bf16.register_fake
def _(packed, desc):
    d = _desc(desc)
    return packed.new_empty(_lib.lib().swn_bf16_weight_bytes(ctypes.byref(d)), dtype=torch.uint8)


def stack_forward_bf16_impl(packed: torch.Tensor, wbf16: torch.Tensor, cond: torch.Tensor, audio: torch.Tensor,
                       desc: List[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 MFMA variant of stack_forward: raw (B, n_out, Tp) fp32 and the bf16 work buffer (swn_forward_bf16)."""
    Lb = _lib.lib()
    d = _desc(desc)
    _need_cuda(packed, "the packed parameters")
    dev = packed.device
    soft, seg, _, _, n_out, _ = _geom(d)
    B, Tf = cond.shape[0], cond.shape[1]
    T, Tp = _tp(d, Tf)
    audio = audio.to(dev, torch.int32 if soft else torch.float32).contiguous()
    if audio.numel() != B * (T - seg):
        raise RuntimeError("audio has the wrong size")
    r = ctypes.byref(d)
    work = torch.empty(Lb.swn_forward_bf16_work_bytes(r, B, Tf), dtype=torch.uint8, device=dev)
    out = torch.empty((B, n_out, Tp), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(Lb.swn_forward_bf16(r, _ptr(packed), _ptr(wbf16), _ptr(cond.contiguous()), _ptr(audio), B, Tf,
                                       _ptr(work), _ptr(out), _stream(dev)), "forward_bf16")
    return out, work


stack_forward_bf16 = custom_op("swn::stack_forward_bf16", mutates_args=())(stack_forward_bf16_impl)


@stack_forward_bf16.register_fake
def _(packed, wbf16, cond, audio, desc):
    Lb, d = _lib.lib(), _desc(desc)
    _, _, _, _, n_out, _ = _geom(d)
    B, Tf = cond.shape[0], cond.shape[1]
    _, Tp = _tp(d, Tf)
    return (packed.new_empty((B, n_out, Tp)),
            packed.new_empty(Lb.swn_forward_bf16_work_bytes(ctypes.byref(d), B, Tf), dtype=torch.uint8))


# ------------------------------------------------------------------------------------------ Laplace head
def laplace_head_impl(raw: torch.Tensor, desc: List[int], clip: bool
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """raw (B, n_out, Tp) -> mu, b, logb, a, b_clip, logb_clip (time-major; empty where not produced), below_floor."""
    Lb = _lib.lib()
    d = _desc(desc)
    _need_cuda(raw, "the stack outputs")
    dev = raw.device
    B, _, Tp = raw.shape
    seg, lpc = d.seg, d.lpc
    mk = lambda w, on=True: torch.empty((B, Tp, w) if on else (0,), dtype=torch.float32, device=dev)
    mu, b, logb = mk(seg), mk(seg), mk(seg)
    a = mk(lpc, lpc > 0)
    bc, lc = mk(seg, clip), mk(seg, clip)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(Lb.swn_laplace_head(ctypes.byref(d), _ptr(raw.contiguous()), B, Tp, _ptr(mu), _ptr(b), _ptr(logb),
                                       _ptr(a if lpc > 0 else None), _ptr(bc if clip else None),
                                       _ptr(lc if clip else None), _ptr(flag), _stream(dev)), "laplace_head")
    return mu, b, logb, a, bc, lc, flag


laplace_head = custom_op("swn::laplace_head", mutates_args=())(laplace_head_impl)


@laplace_head.register_fake
def _(raw, desc, clip):
    d = _desc(desc)
    B, _, Tp = raw.shape
    mk = lambda w, on=True: raw.new_empty((B, Tp, w) if on else (0,))
    return (mk(d.seg), mk(d.seg), mk(d.seg), mk(d.lpc, d.lpc > 0), mk(d.seg, clip), mk(d.seg, clip),
            raw.new_empty(1, dtype=torch.int32))


def laplace_head_backward_impl(raw: torch.Tensor, gmu: Optional[torch.Tensor], gb: Optional[torch.Tensor],
                          glogb: Optional[torch.Tensor], ga: Optional[torch.Tensor], gb_clip: Optional[torch.Tensor],
                          glogb_clip: Optional[torch.Tensor], desc: List[int]) -> torch.Tensor:
    Lb = _lib.lib()
    d = _desc(desc)
    dev = raw.device
    B, _, Tp = raw.shape
    c = lambda t: None if t is None else t.to(dev, torch.float32).contiguous()
    gmu, gb, glogb, ga, gb_clip, glogb_clip = c(gmu), c(gb), c(glogb), c(ga), c(gb_clip), c(glogb_clip)
    raw = raw.contiguous()
    graw = torch.empty_like(raw)
    with _on(dev):
        _lib.check(Lb.swn_laplace_head_backward(ctypes.byref(d), _ptr(raw), B, Tp, _ptr(gmu), _ptr(gb), _ptr(glogb),
                                                _ptr(ga), _ptr(gb_clip), _ptr(glogb_clip), _ptr(graw), _stream(dev)),
                   "laplace_head_backward")
    return graw


laplace_head_backward = custom_op("swn::laplace_head_backward", mutates_args=())(laplace_head_backward_impl)


@laplace_head_backward.register_fake
def _(raw, gmu, gb, glogb, ga, gb_clip, glogb_clip, desc):
    return torch.empty_like(raw)


# ------------------------------------------------------------------------------------------ backward of the stack
def stack_backward_impl(packed: torch.Tensor, aux: torch.Tensor, cond: torch.Tensor, fe_work: torch.Tensor,
                   audio: torch.Tensor, fwd_work: torch.Tensor, grad_raw: torch.Tensor, desc: List[int],
                   precision: int = 0) -> torch.Tensor:
    """gradient of the loss wrt the packed parameter buffer given d loss / d raw (swn_backward); precision =
    SWN_PRECISION_FP32 (0, parity) | SWN_PRECISION_BF16 (1, bf16 operands / fp32 accumulation)."""
    Lb = _lib.lib()
    d = _desc(desc)
    dev = packed.device
    B, Tf = cond.shape[0], cond.shape[1]
    r = ctypes.byref(d)
    grad_raw = grad_raw.to(dev, torch.float32).contiguous()
    work = torch.empty(Lb.swn_backward_work_floats(r, B, Tf), dtype=torch.float32, device=dev)
    gp = torch.empty_like(packed)
    with _on(dev):
        _lib.check(Lb.swn_backward(r, _ptr(packed), _ptr(aux), _ptr(cond), _ptr(fe_work), _ptr(audio), _ptr(fwd_work),
                                   _ptr(None), _ptr(grad_raw), B, Tf, _ptr(work), _ptr(gp), int(precision), _stream(dev)),
                   "backward")
    return gp


stack_backward = custom_op("swn::stack_backward", mutates_args=())(stack_backward_impl)


@stack_backward.register_fake
def _(packed, aux, cond, fe_work, audio, fwd_work, grad_raw, desc, precision=0):
    return torch.empty_like(packed)


def stack_backward_bf16_impl(packed: torch.Tensor, aux: torch.Tensor, cond: torch.Tensor, fe_work: torch.Tensor,
                        audio: torch.Tensor, work_bf16: torch.Tensor, grad_raw: torch.Tensor,
                        desc: List[int]) -> torch.Tensor:
    """stack_backward after a bf16 forward of the BL6 class with the sample-rate part fused (swn_backward_bf16): reads
    the bf16 work buffer of the forward directly; raises where swn_backward_bf16_work_floats() is 0 (callers check
    `backward_bf16_supported` first)."""
    Lb = _lib.lib()
    d = _desc(desc)
    dev = packed.device
    B, Tf = cond.shape[0], cond.shape[1]
    r = ctypes.byref(d)
    n = Lb.swn_backward_bf16_work_floats(r, B, Tf)
    if n == 0:
        raise RuntimeError("swn_backward_bf16 does not cover this geometry / size")
    grad_raw = grad_raw.to(dev, torch.float32).contiguous()
    work = torch.empty(n, dtype=torch.float32, device=dev)
    gp = torch.empty_like(packed)
    with _on(dev):
        _lib.check(Lb.swn_backward_bf16(r, _ptr(packed), _ptr(aux), _ptr(cond), _ptr(fe_work), _ptr(audio), _ptr(None),
                                        _ptr(work_bf16), _ptr(grad_raw), B, Tf, _ptr(work), _ptr(gp), _stream(dev)),
                   "backward_bf16")
    return gp


stack_backward_bf16 = custom_op("swn::stack_backward_bf16", mutates_args=())(stack_backward_bf16_impl)


@stack_backward_bf16.register_fake
def _(packed, aux, cond, fe_work, audio, work_bf16, grad_raw, desc):
    return torch.empty_like(packed)


def backward_bf16_supported(desc: List[int], batch: int, n_frames: int) -> bool:
    return _lib.lib().swn_backward_bf16_work_floats(ctypes.byref(_desc(desc)), batch, n_frames) > 0


# ------------------------------------------------------------------------------------------ multi-resolution STFT loss
def _spectral_sizes(sizes: Sequence[int]):
    return (ctypes.c_int * len(sizes))(*[int(n) for n in sizes])


def _spectral_check(rows: int, length: int, sizes: Sequence[int]) -> None:
    """the argument rules of swn_spectral_* as messages (the library itself answers SWN_E_BADARG)."""
    if not 1 <= len(sizes) <= _lib.SPECTRAL_MAX_SIZES:
        raise RuntimeError(f"spectral_loss takes 1 to {_lib.SPECTRAL_MAX_SIZES} FFT sizes, got {len(sizes)}")
    for n in sizes:
        if n % 32 != 0 or not 32 <= n <= _lib.SPECTRAL_MAX_FFT:
            raise RuntimeError(f"FFT size {n} is not a multiple of 32 in [32, {_lib.SPECTRAL_MAX_FFT}]")
        if length <= n // 2:
            raise RuntimeError(f"FFT size {n} needs signals longer than {n // 2} samples (reflect padding), got {length}")
    if rows < 1:
        raise RuntimeError("spectral_loss needs at least one row")


def spectral_loss_impl(samples: torch.Tensor, targets: torch.Tensor, tables: torch.Tensor, sizes: List[int],
                       keep_state: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """samples, targets (R, T) -> l1 (R, K), lsd (R, K) per FFT size (swn_spectral_forward) and, with keep_state, the byte
    state spectral_loss_backward reads (empty otherwise).  tables: cos and Hann tables of the K sizes (spectral.py)."""
    Lb = _lib.lib()
    _need_cuda(samples, "the signals")
    dev = samples.device
    if samples.dim() != 2 or samples.shape != targets.shape:
        raise RuntimeError(f"spectral_loss needs samples and targets of one shape (R, T), got {tuple(samples.shape)} and "
                           f"{tuple(targets.shape)}")
    R, T = samples.shape
    _spectral_check(R, T, sizes)
    if tables.numel() != 2 * sum(sizes):
        raise RuntimeError(f"tables hold {tables.numel()} floats, the sizes need {2 * sum(sizes)}")
    samples = samples.to(dev, torch.float32).contiguous()
    targets = targets.to(dev, torch.float32).contiguous()
    tables = tables.to(dev, torch.float32).contiguous()
    K, sz = len(sizes), _spectral_sizes(sizes)
    l1 = torch.empty((R, K), dtype=torch.float32, device=dev)
    lsd = torch.empty((R, K), dtype=torch.float32, device=dev)
    state = torch.empty(Lb.swn_spectral_state_bytes(R, T, sz, K) if keep_state else 0, dtype=torch.uint8, device=dev)
    work = torch.empty(Lb.swn_spectral_work_bytes(R, T, sz, K), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(Lb.swn_spectral_forward(_ptr(samples), _ptr(targets), R, T, sz, K, _ptr(tables), _ptr(l1), _ptr(lsd),
                                           _ptr(state if keep_state else None), _ptr(work), _stream(dev)), "spectral_forward")
    return l1, lsd, state


spectral_loss = custom_op("swn::spectral_loss", mutates_args=())(spectral_loss_impl)


@spectral_loss.register_fake
def _(samples, targets, tables, sizes, keep_state):
    R, T = samples.shape
    _spectral_check(R, T, sizes)
    K, sz = len(sizes), _spectral_sizes(sizes)
    nb = _lib.lib().swn_spectral_state_bytes(R, T, sz, K) if keep_state else 0
    return (samples.new_empty((R, K), dtype=torch.float32), samples.new_empty((R, K), dtype=torch.float32),
            samples.new_empty(nb, dtype=torch.uint8))


def spectral_loss_backward_impl(grad_l1: torch.Tensor, state: torch.Tensor, tables: torch.Tensor, sizes: List[int],
                                length: int) -> torch.Tensor:
    """d sum(grad_l1 * l1) / d samples, (R, T), from the state of a spectral_loss(keep_state=True) call
    (swn_spectral_backward)."""
    Lb = _lib.lib()
    _need_cuda(state, "the forward state")
    dev = state.device
    R, K = grad_l1.shape
    _spectral_check(R, length, sizes)
    sz = _spectral_sizes(sizes)
    if K != len(sizes) or state.numel() != Lb.swn_spectral_state_bytes(R, length, sz, K):
        raise RuntimeError("spectral_loss_backward: grad_l1 / state do not belong to these sizes and this length")
    g = grad_l1.to(dev, torch.float32).contiguous()
    grad = torch.empty((R, length), dtype=torch.float32, device=dev)
    work = torch.empty(Lb.swn_spectral_work_bytes(R, length, sz, K), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(Lb.swn_spectral_backward(_ptr(g), _ptr(state.contiguous()), R, length, sz, K, _ptr(tables.contiguous()),
                                            _ptr(grad), _ptr(work), _stream(dev)), "spectral_backward")
    return grad


spectral_loss_backward = custom_op("swn::spectral_loss_backward", mutates_args=())(spectral_loss_backward_impl)


@spectral_loss_backward.register_fake
def _(grad_l1, state, tables, sizes, length):
    return grad_l1.new_empty((grad_l1.shape[0], length), dtype=torch.float32)


class SpectralLossFunction(torch.autograd.Function):
    """l1, lsd = SpectralLossFunction.apply(samples, targets, tables, sizes): l1 differentiable in the samples, lsd a
    reported figure; like the stack Functions of nets/_autograd.py it calls the _impl functions directly."""

    @staticmethod
    def forward(ctx, samples, targets, tables, sizes):
        l1, lsd, state = spectral_loss_impl(samples, targets, tables, list(sizes), True)
        ctx.save_for_backward(state, tables)
        ctx.sizes, ctx.length = list(sizes), samples.shape[1]
        ctx.mark_non_differentiable(lsd)
        return l1, lsd

    @staticmethod
    def backward(ctx, g_l1, _g_lsd):
        state, tables = ctx.saved_tensors
        return spectral_loss_backward_impl(g_l1, state, tables, ctx.sizes, ctx.length), None, None, None

# ------------------------------------------------------------------------------------------ Laplace chunk loss
def _laplace_loss_check(raw, ctx, target, eps, d, skip: int) -> Tuple[int, int, int]:
    """the argument rules of swn_laplace_loss_* as messages (the library itself answers SWN_E_BADARG) -> (B, tp, N)."""
    if d.kind != 0:
        raise RuntimeError("laplace_loss needs a Laplace (CSWNV) descriptor")
    seg, lpc = d.seg, d.lpc
    if raw.dim() != 3 or raw.shape[1] != 2 * seg + lpc:
        raise RuntimeError(f"laplace_loss needs raw (B, {2 * seg + lpc}, Tp) for seg {seg} / lpc {lpc}, got {tuple(raw.shape)}")
    B, _, tp = raw.shape
    N = tp - skip
    if skip < 0 or N < 1:
        raise RuntimeError(f"laplace_loss: skip {skip} leaves no position of {tp}")
    if lpc > 0 and ctx is None:
        raise RuntimeError(f"laplace_loss needs the LP context with lpc {lpc}")
    if lpc > 0 and tuple(ctx.shape) != (B, tp + seg + lpc - 1):
        raise RuntimeError(f"laplace_loss needs an LP context ({B}, {tp + seg + lpc - 1}), got {tuple(ctx.shape)}")
    if tuple(target.shape) != (B, tp + seg - 1):
        raise RuntimeError(f"laplace_loss needs a target ({B}, {tp + seg - 1}), got {tuple(target.shape)}")
    if tuple(eps.shape) != (B, seg, N):
        raise RuntimeError(f"laplace_loss needs deviates ({B}, {seg}, {N}), got {tuple(eps.shape)}")
    return B, tp, N


def laplace_loss_impl(raw: torch.Tensor, ctx: Optional[torch.Tensor], target: torch.Tensor, eps: torch.Tensor,
                      desc: List[int], skip: int
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """raw (B, NO, Tp), LP context (B, Tp + seg + lpc - 1) or None, target (B, Tp + seg - 1), deviates (B, seg, N) ->
    nll (B, seg), err (B, seg), samples (B seg, N), targets (B seg, N), stats (7,)   (swn_laplace_loss_forward)."""
    Lb = _lib.lib()
    d = _desc(desc)
    _need_cuda(raw, "the stack outputs")
    dev = raw.device
    B, tp, N = _laplace_loss_check(raw, ctx, target, eps, d, skip)
    c = lambda t: None if t is None else t.to(dev, torch.float32).contiguous()
    raw, ctx, target, eps = c(raw), (c(ctx) if d.lpc > 0 else None), c(target), c(eps)
    mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    nll, err, samples, targets, stats = mk(B, d.seg), mk(B, d.seg), mk(B * d.seg, N), mk(B * d.seg, N), mk(7)
    r = ctypes.byref(d)
    work = torch.empty(Lb.swn_laplace_loss_work_bytes(r, B, tp, skip), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(Lb.swn_laplace_loss_forward(r, _ptr(raw), _ptr(ctx), _ptr(target), _ptr(eps), B, tp, skip, _ptr(nll),
                                               _ptr(err), _ptr(samples), _ptr(targets), _ptr(stats), _ptr(work),
                                               _stream(dev)), "laplace_loss_forward")
    return nll, err, samples, targets, stats


laplace_loss = custom_op("swn::laplace_loss", mutates_args=())(laplace_loss_impl)


@laplace_loss.register_fake
def _(raw, ctx, target, eps, desc, skip):
    d = _desc(desc)
    B, tp, N = _laplace_loss_check(raw, ctx, target, eps, d, skip)
    mk = lambda *shape: raw.new_empty(shape, dtype=torch.float32)
    return mk(B, d.seg), mk(B, d.seg), mk(B * d.seg, N), mk(B * d.seg, N), mk(7)


def laplace_loss_backward_impl(raw: torch.Tensor, ctx: Optional[torch.Tensor], target: torch.Tensor, eps: torch.Tensor,
                               g_nll: torch.Tensor, g_samples: Optional[torch.Tensor], desc: List[int],
                               skip: int) -> torch.Tensor:
    """d (sum g_nll * nll + sum g_samples * samples) / d raw, (B, NO, Tp), from the inputs of the forward
    (swn_laplace_loss_backward)."""
    Lb = _lib.lib()
    d = _desc(desc)
    _need_cuda(raw, "the stack outputs")
    dev = raw.device
    B, tp, N = _laplace_loss_check(raw, ctx, target, eps, d, skip)
    if tuple(g_nll.shape) != (B, d.seg) or (g_samples is not None and tuple(g_samples.shape) != (B * d.seg, N)):
        raise RuntimeError("laplace_loss_backward: the upstream gradients do not belong to these shapes")
    c = lambda t: None if t is None else t.to(dev, torch.float32).contiguous()
    raw, ctx, target, eps, g_nll, g_samples = c(raw), (c(ctx) if d.lpc > 0 else None), c(target), c(eps), c(g_nll), c(g_samples)
    graw = torch.empty_like(raw)
    with _on(dev):
        _lib.check(Lb.swn_laplace_loss_backward(ctypes.byref(d), _ptr(raw), _ptr(ctx), _ptr(target), _ptr(eps), B, tp, skip,
                                                _ptr(g_nll), _ptr(g_samples), _ptr(graw), _stream(dev)),
                   "laplace_loss_backward")
    return graw


laplace_loss_backward = custom_op("swn::laplace_loss_backward", mutates_args=())(laplace_loss_backward_impl)


@laplace_loss_backward.register_fake
def _(raw, ctx, target, eps, g_nll, g_samples, desc, skip):
    return torch.empty_like(raw)


class LaplaceLossFunction(torch.autograd.Function):
    """nll, err, samples, targets, stats = LaplaceLossFunction.apply(raw, ctx, target, eps, desc, skip): nll and samples
    differentiable in raw, the rest reported figures; calls the _impl functions directly like SpectralLossFunction."""

    @staticmethod
    def forward(ctx_, raw, ctx, target, eps, desc, skip):
        out = laplace_loss_impl(raw, ctx, target, eps, list(desc), int(skip))
        ctx_.save_for_backward(raw, target, eps, *(() if ctx is None else (ctx,)))
        ctx_.desc, ctx_.skip = list(desc), int(skip)
        ctx_.set_materialize_grads(False)           # an unused samples output reaches the kernel as NULL, not as zeros
        ctx_.mark_non_differentiable(out[1], out[3], out[4])
        return out

    @staticmethod
    def backward(ctx_, g_nll, _g_err, g_samples, _g_targets, _g_stats):
        raw, target, eps, *rest = ctx_.saved_tensors
        if g_nll is None:
            g_nll = raw.new_zeros((raw.shape[0], ctx_.desc[DESC_FIELDS.index("seg")]))
        graw = laplace_loss_backward_impl(raw, rest[0] if rest else None, target, eps, g_nll, g_samples, ctx_.desc, ctx_.skip)
        return graw, None, None, None, None, None


# ------------------------------------------------------------------------------------------ log-mel features
def _stft_check(op: str, n_fft: int, hop: int, floor: float, own: Tuple[bool, str]) -> None:
    """the n_fft / hop / floor rules swn_logmel and swn_mcep share, as messages, with the op's `own` rule (holds, message)
    between hop's and floor's"""
    if n_fft % 32 != 0 or not 32 <= n_fft <= _lib.SPECTRAL_MAX_FFT:
        raise RuntimeError(f"{op}: n_fft {n_fft} is not a multiple of 32 in [32, {_lib.SPECTRAL_MAX_FFT}]")
    if not 1 <= hop <= n_fft:
        raise RuntimeError(f"{op}: hop {hop} outside [1, n_fft = {n_fft}]")
    if not own[0]:
        raise RuntimeError(f"{op}: {own[1]}")
    if not floor > 0.0:
        raise RuntimeError(f"{op}: floor {floor} must be > 0")


def _tables_check(op: str, tables: torch.Tensor, need: int, dev, of: str) -> None:
    if tables.device != dev or tables.dtype != torch.float32 or not tables.is_contiguous() or tables.numel() != need:
        raise RuntimeError(f"{op}: tables must be {need} contiguous fp32 values on the device of the {of}")


def _fmax(f0s: List[int], f1s: List[int]) -> int:
    return max([f1 - f0 for f0, f1 in zip(f0s, f1s)] + [0])


def _frames_fake(wav, f0s, f1s, cols: int) -> torch.Tensor:
    """the output of a frame-range op for shape inference"""
    return wav.new_empty((wav.shape[0], _fmax(f0s, f1s), cols), dtype=torch.float32)


def _frame_entries(op: str, wav: torch.Tensor, t0s: List[int], n_avails: List[int], lens: List[int], f0s: List[int],
                   f1s: List[int], cols: int, f0: Optional[torch.Tensor] = None):
    """the contract of logmel, mcep, f0, bap and envelope: row r of the contiguous fp32 buffer wav (R, S) holds the samples
    [t0s[r], t0s[r] + n_avails[r]) of signal r, whose total length is lens[r] (-1: not known yet); the call computes its frames
    [f0s[r], f1s[r]).  Checks the buffer and the lists -> (the zeroed (R, max(f1 - f0), cols) output, the launch groups
    [(LogMelEntry table, n), ...] of at most LOGMEL_MAX_ENTRIES rows each, in row order).  With `f0` (envelope), a contiguous fp32
    (R, >= max(f1 - f0)) tensor on wav's device whose row r holds the F0 of the frames f0s[r], f0s[r] + 1, ..., the tables are
    EnvelopeEntry and carry its rows."""
    if wav.dim() != 2 or wav.dtype != torch.float32 or not wav.is_contiguous():
        raise RuntimeError(f"{op} needs a contiguous fp32 (R, S) buffer, got {tuple(wav.shape)} {wav.dtype}")
    R, S = wav.shape
    if not (len(t0s) == len(n_avails) == len(lens) == len(f0s) == len(f1s) == R):
        raise RuntimeError(f"{op}: t0s, n_avails, lens, f0s and f1s must have one entry per row")
    if any(not 0 <= na <= S for na in n_avails):
        raise RuntimeError(f"{op}: a row has more samples available than the buffer's {S} columns")
    fmax = _fmax(f0s, f1s)
    out = torch.zeros((R, fmax, cols), dtype=torch.float32, device=wav.device)
    esz, osz = wav.element_size() * S, out.element_size() * fmax * cols
    kind, more = _lib.LogMelEntry, lambda r: {}
    if f0 is not None:
        if (f0.dim() != 2 or f0.dtype != torch.float32 or not f0.is_contiguous() or f0.device != wav.device or f0.shape[0] != R
                or f0.shape[1] < fmax):
            raise RuntimeError(f"{op}: f0 must be a contiguous fp32 ({R}, >= {fmax}) tensor on the waveforms' device, got "
                               f"{tuple(f0.shape)} {f0.dtype} on {f0.device}")
        fsz = f0.element_size() * f0.shape[1]
        kind, more = _lib.EnvelopeEntry, lambda r: {"f0_dev": f0.data_ptr() + r * fsz, "reserved2": 0}
    groups = []
    for r0 in range(0, R, _lib.LOGMEL_MAX_ENTRIES):
        r1 = min(R, r0 + _lib.LOGMEL_MAX_ENTRIES)
        groups.append(((kind * (r1 - r0))(*[
            kind(wav_dev=wav.data_ptr() + r * esz, out_dev=out.data_ptr() + r * osz, t0=int(t0s[r]),
                 n_avail=int(n_avails[r]), len=int(lens[r]), f0=int(f0s[r]), f1=int(f1s[r]), reserved=0, **more(r))
            for r in range(r0, r1)]), r1 - r0))
    return out, groups


def _logmel_check(n_fft: int, hop: int, n_mels: int, floor: float) -> None:
    """the size rules of swn_logmel as messages (the library itself answers SWN_E_BADARG)."""
    _stft_check("logmel", n_fft, hop, floor, (1 <= n_mels <= _lib.LOGMEL_MAX_MELS,
                                              f"n_mels {n_mels} outside [1, {_lib.LOGMEL_MAX_MELS}]"))


def logmel_impl(wav: torch.Tensor, tables: torch.Tensor, bank: List[int], t0s: List[int], n_avails: List[int],
                lens: List[int], f0s: List[int], f1s: List[int], n_fft: int, hop: int, floor: float,
                linear: bool) -> torch.Tensor:
    """wav (R, S): row r holds the samples [t0s[r], t0s[r] + n_avails[r]) of signal r, whose total length is lens[r] (-1: not
    known yet) -> (R, max(f1 - f0), n_mels) log-mel (or, with linear, mel) amplitudes of the frames [f0s[r], f1s[r]) of each
    row, zero past a row's own range (swn_logmel; the definition is in melspec.py).  tables / bank: melspec.tables()."""
    Lb = _lib.lib()
    _need_cuda(wav, "the waveforms")
    dev = wav.device
    n_mels = len(bank)
    _logmel_check(n_fft, hop, n_mels, floor)
    out, groups = _frame_entries("logmel", wav, t0s, n_avails, lens, f0s, f1s, n_mels)
    _tables_check("logmel", tables, Lb.swn_logmel_table_floats(n_fft, n_mels), dev, "waveforms")
    bank_c = (ctypes.c_int32 * n_mels)(*[int(b) for b in bank])
    for table, n in groups:
        nb = Lb.swn_logmel_work_bytes(n_fft, hop, table, n)
        work = torch.empty(max(nb, 4) // 4, dtype=torch.float32, device=dev)
        with _on(dev):
            _lib.check(Lb.swn_logmel(n_fft, hop, n_mels, float(floor), int(bool(linear)), _ptr(tables), bank_c, table, n,
                                     _ptr(work), _stream(dev)), "logmel")
    return out


logmel = custom_op("swn::logmel", mutates_args=())(logmel_impl)


@logmel.register_fake
def _(wav, tables, bank, t0s, n_avails, lens, f0s, f1s, n_fft, hop, floor, linear):
    _logmel_check(n_fft, hop, len(bank), floor)
    return _frames_fake(wav, f0s, f1s, len(bank))


def _mcep_check(n_fft: int, hop: int, order: int, floor: float) -> None:
    """the size rules of swn_mcep as messages (the library itself answers SWN_E_BADARG)."""
    _stft_check("mcep", n_fft, hop, floor, (0 <= order <= min(_lib.MCEP_MAX_ORDER, n_fft // 2),
                                            f"order {order} outside [0, min({_lib.MCEP_MAX_ORDER}, n_fft / 2 = {n_fft // 2})]"))


def mcep_impl(wav: torch.Tensor, tables: torch.Tensor, t0s: List[int], n_avails: List[int], lens: List[int], f0s: List[int],
              f1s: List[int], n_fft: int, hop: int, order: int, floor: float) -> torch.Tensor:
    """wav (R, S), t0s, n_avails, lens, f0s, f1s: as logmel takes them -> (R, max(f1 - f0), order + 1) mel-cepstra of the frames
    [f0s[r], f1s[r]) of each row, zero past a row's own range (swn_mcep; the definition is in melspec.py).  tables:
    melspec.mcep_tables()."""
    Lb = _lib.lib()
    _need_cuda(wav, "the waveforms")
    dev = wav.device
    _mcep_check(n_fft, hop, order, floor)
    out, groups = _frame_entries("mcep", wav, t0s, n_avails, lens, f0s, f1s, order + 1)
    _tables_check("mcep", tables, Lb.swn_mcep_table_floats(n_fft, order), dev, "waveforms")
    for table, n in groups:
        nb = Lb.swn_mcep_work_bytes(n_fft, hop, table, n)
        work = torch.empty(max(nb, 4) // 4, dtype=torch.float32, device=dev)
        with _on(dev):
            _lib.check(Lb.swn_mcep(n_fft, hop, order, float(floor), _ptr(tables), table, n, _ptr(work), _stream(dev)), "mcep")
    return out


mcep = custom_op("swn::mcep", mutates_args=())(mcep_impl)


@mcep.register_fake
def _(wav, tables, t0s, n_avails, lens, f0s, f1s, n_fft, hop, order, floor):
    _mcep_check(n_fft, hop, order, floor)
    return _frames_fake(wav, f0s, f1s, order + 1)


def _f0_check(fs: float, hop: int, win: int, lag_lo: int, lag_hi: int, threshold: float) -> None:
    """the size rules of swn_f0 as messages (the library itself answers SWN_E_BADARG)."""
    if not (fs > 0.0 and fs < float("inf")):
        raise RuntimeError(f"f0: fs {fs} must be a finite number > 0")
    if not 1 <= hop <= _lib.F0_MAX_HOP:
        raise RuntimeError(f"f0: hop {hop} outside [1, {_lib.F0_MAX_HOP}]")
    if not _lib.F0_MIN_WIN <= win <= _lib.F0_MAX_WIN:
        raise RuntimeError(f"f0: win {win} outside [{_lib.F0_MIN_WIN}, {_lib.F0_MAX_WIN}]")
    if not 2 <= lag_lo <= lag_hi <= _lib.F0_MAX_LAG - 1:
        raise RuntimeError(f"f0: lags [{lag_lo}, {lag_hi}], need 2 <= lag_lo <= lag_hi <= {_lib.F0_MAX_LAG - 1}")
    if not 0.0 < threshold <= 1.0:
        raise RuntimeError(f"f0: threshold {threshold} outside (0, 1]")


def f0_impl(wav: torch.Tensor, t0s: List[int], n_avails: List[int], lens: List[int], f0s: List[int], f1s: List[int], fs: float,
            hop: int, win: int, lag_lo: int, lag_hi: int, threshold: float) -> torch.Tensor:
    """wav (R, S), t0s, n_avails, lens, f0s, f1s: as logmel takes them -> (R, max(f1 - f0), 2): [F0 in Hz or 0.0 when unvoiced,
    aperiodicity d'(tau*)] of the frames [f0s[r], f1s[r]) of each row, zero past a row's own range (swn_f0; the definition is
    in pitch.py)."""
    Lb = _lib.lib()
    _need_cuda(wav, "the waveforms")
    dev = wav.device
    _f0_check(fs, hop, win, lag_lo, lag_hi, threshold)
    out, groups = _frame_entries("f0", wav, t0s, n_avails, lens, f0s, f1s, 2)
    for table, n in groups:
        with _on(dev):
            _lib.check(Lb.swn_f0(float(fs), hop, win, lag_lo, lag_hi, float(threshold), table, n, _stream(dev)), "f0")
    return out


f0 = custom_op("swn::f0", mutates_args=())(f0_impl)


@f0.register_fake
def _(wav, t0s, n_avails, lens, f0s, f1s, fs, hop, win, lag_lo, lag_hi, threshold):
    _f0_check(fs, hop, win, lag_lo, lag_hi, threshold)
    return _frames_fake(wav, f0s, f1s, 2)


def _bap_check(taps: torch.Tensor, win: int, band_win: int, floor: float) -> Tuple[int, int]:
    """the size rules swn_bap adds to swn_f0's, as messages -> (n_bands, n_taps)"""
    if taps.dim() != 2 or taps.dtype != torch.float64:
        raise RuntimeError(f"bap: taps must be a (n_bands, n_taps) float64 tensor, got {tuple(taps.shape)} {taps.dtype}")
    B, T = int(taps.shape[0]), int(taps.shape[1])
    if not 1 <= B <= _lib.BAP_MAX_BANDS:
        raise RuntimeError(f"bap: {B} bands, need 1 .. {_lib.BAP_MAX_BANDS}")
    if not (1 <= T <= _lib.BAP_MAX_TAPS and T % 2 == 1):
        raise RuntimeError(f"bap: {T} taps, need an odd count in 1 .. {_lib.BAP_MAX_TAPS}")
    if not _lib.F0_MIN_WIN <= band_win <= win:
        raise RuntimeError(f"bap: band_win {band_win} outside [{_lib.F0_MIN_WIN}, win = {win}]")
    if not 0.0 < floor < 1.0:
        raise RuntimeError(f"bap: floor {floor} outside (0, 1)")
    return B, T


def bap_impl(wav: torch.Tensor, taps: torch.Tensor, t0s: List[int], n_avails: List[int], lens: List[int], f0s: List[int],
             f1s: List[int], fs: float, hop: int, win: int, lag_lo: int, lag_hi: int, threshold: float, band_win: int,
             floor: float) -> torch.Tensor:
    """wav (R, S), t0s, n_avails, lens, f0s, f1s: as f0 takes them; taps: contiguous (B, T) float64 band-pass filters on wav's
    device -> (R, max(f1 - f0), 2 + B): f0's two values and the B coded band aperiodicities in dB of the frames [f0s[r], f1s[r])
    of each row, zero past a row's own range (swn_bap; the definition is in pitch.py)."""
    Lb = _lib.lib()
    _need_cuda(wav, "the waveforms")
    dev = wav.device
    _f0_check(fs, hop, win, lag_lo, lag_hi, threshold)
    B, T = _bap_check(taps, win, band_win, floor)
    if taps.device != dev or not taps.is_contiguous():
        raise RuntimeError("bap: taps must be contiguous and on the waveforms' device")
    out, groups = _frame_entries("bap", wav, t0s, n_avails, lens, f0s, f1s, 2 + B)
    # one scratch for all groups, which run one after the other on the stream (never empty: the call refuses a null pointer)
    nb = max([int(Lb.swn_bap_work_bytes(hop, win, lag_hi, B, table, n)) for table, n in groups] + [8])
    work = torch.empty((nb // 8,), dtype=torch.float64, device=dev)
    for table, n in groups:
        with _on(dev):
            _lib.check(Lb.swn_bap(float(fs), hop, win, lag_lo, lag_hi, float(threshold), band_win, B, T, taps.data_ptr(), float(floor),
                                  table, n, work.data_ptr(), _stream(dev)), "bap")
    return out


bap = custom_op("swn::bap", mutates_args=())(bap_impl)


@bap.register_fake
def _(wav, taps, t0s, n_avails, lens, f0s, f1s, fs, hop, win, lag_lo, lag_hi, threshold, band_win, floor):
    _f0_check(fs, hop, win, lag_lo, lag_hi, threshold)
    B, _ = _bap_check(taps, win, band_win, floor)
    return _frames_fake(wav, f0s, f1s, 2 + B)


def _envelope_check(fs: float, n_fft: int, hop: int, order: int, floor: float, q1: float, default_f0: float, what: int) -> int:
    """the size rules of swn_envelope as messages (the library itself answers SWN_E_BADARG) -> the columns of a frame"""
    if not (fs > 0.0 and fs < float("inf")):
        raise RuntimeError(f"envelope: fs {fs} must be a finite number > 0")
    if n_fft % 32 != 0 or not 32 <= n_fft <= _lib.SPECTRAL_MAX_FFT:
        raise RuntimeError(f"envelope: n_fft {n_fft} is not a multiple of 32 in [32, {_lib.SPECTRAL_MAX_FFT}]")
    if not 1 <= hop <= _lib.F0_MAX_HOP:
        raise RuntimeError(f"envelope: hop {hop} outside [1, {_lib.F0_MAX_HOP}]")
    if not 0 <= order <= min(_lib.MCEP_MAX_ORDER, n_fft // 2):
        raise RuntimeError(f"envelope: order {order} outside [0, min({_lib.MCEP_MAX_ORDER}, n_fft / 2 = {n_fft // 2})]")
    if not 0.0 < floor < float("inf"):
        raise RuntimeError(f"envelope: floor {floor} must be a finite number > 0")
    if not abs(q1) < float("inf"):
        raise RuntimeError(f"envelope: q1 {q1} must be finite")
    if not 3.0 * fs / (n_fft - 3.0) < default_f0 <= fs / 4.0:
        raise RuntimeError(f"envelope: default_f0 {default_f0} outside (3 fs / (n_fft - 3) = {3.0 * fs / (n_fft - 3.0):g}, "
                           f"fs / 4 = {fs / 4.0:g}]: n_fft {n_fft} is too short for fs {fs}")
    if what not in (_lib.ENVELOPE_MCEP, _lib.ENVELOPE_LOGAMP):
        raise RuntimeError(f"envelope: what {what} is neither ENVELOPE_MCEP (0) nor ENVELOPE_LOGAMP (1)")
    return order + 1 if what == _lib.ENVELOPE_MCEP else n_fft // 2 + 1


def envelope_impl(wav: torch.Tensor, f0: torch.Tensor, tables: torch.Tensor, t0s: List[int], n_avails: List[int], lens: List[int],
                  f0s: List[int], f1s: List[int], fs: float, n_fft: int, hop: int, order: int, floor: float, q1: float,
                  default_f0: float, what: int) -> torch.Tensor:
    """wav (R, S), t0s, n_avails, lens, f0s, f1s: as f0 takes them; f0: contiguous fp32 (R, >= max(f1 - f0)), row r holding the
    F0 in Hz of the frames f0s[r], f0s[r] + 1, ...; tables: melspec.envelope_tables(), float64 -> (R, max(f1 - f0), order + 1)
    mel-cepstra of the F0-adaptive spectral envelope (what 0) or (R, max(f1 - f0), n_fft / 2 + 1) log amplitudes of it (what 1)
    of the frames [f0s[r], f1s[r]) of each row, zero past a row's own range (swn_envelope; the definition is in melspec.py)."""
    Lb = _lib.lib()
    _need_cuda(wav, "the waveforms")
    dev = wav.device
    cols = _envelope_check(fs, n_fft, hop, order, floor, q1, default_f0, what)
    out, groups = _frame_entries("envelope", wav, t0s, n_avails, lens, f0s, f1s, cols, f0)
    need = int(Lb.swn_envelope_table_doubles(n_fft, order))
    if tables.device != dev or tables.dtype != torch.float64 or not tables.is_contiguous() or tables.numel() != need:
        raise RuntimeError(f"envelope: tables must be {need} contiguous float64 values on the device of the waveforms")
    nb = max([int(Lb.swn_envelope_work_bytes(n_fft, hop, table, n)) for table, n in groups] + [8])
    work = torch.empty((nb // 8,), dtype=torch.float64, device=dev)
    for table, n in groups:
        with _on(dev):
            _lib.check(Lb.swn_envelope(float(fs), n_fft, hop, order, float(floor), float(q1), float(default_f0), what,
                                       tables.data_ptr(), table, n, work.data_ptr(), _stream(dev)), "envelope")
    return out


envelope = custom_op("swn::envelope", mutates_args=())(envelope_impl)


@envelope.register_fake
def _(wav, f0, tables, t0s, n_avails, lens, f0s, f1s, fs, n_fft, hop, order, floor, q1, default_f0, what):
    return _frames_fake(wav, f0s, f1s, _envelope_check(fs, n_fft, hop, order, floor, q1, default_f0, what))


def logmel_pool_impl(win: torch.Tensor, staged: Optional[torch.Tensor], tables: torch.Tensor, bank: List[int], slots: List[int],
                     t0s: List[int], n_helds: List[int], n_drops: List[int], n_news: List[int], lens: List[int], f0s: List[int],
                     f1s: List[int], n_fft: int, hop: int, floor: float, linear: bool) -> torch.Tensor:
    """one log-mel pool call (swn_logmel_pool; at most LOGMEL_POOL_MAX_ENTRIES entries).  win (slots, window_floats): entry e's
    window win[slots[e]] holds n_helds[e] samples from the absolute index t0s[e] on; the call drops n_drops[e] of them from
    the front, appends the next n_news[e] samples of `staged` (the entries' new samples back to back; None when there are
    none) and computes the frames [f0s[e], f1s[e]) -> a flat buffer with every entry's (n_mels, f1 - f0) block back to back
    in entry order.  `win` is updated in place."""
    return _logmel_pool_call(win, staged, tables, bank, slots, t0s, n_helds, n_drops, n_news, lens, f0s, f1s, n_fft, hop, floor,
                             linear, None, None)


def _logmel_pool_call(win, staged, tables, bank, slots, t0s, n_helds, n_drops, n_news, lens, f0s, f1s, n_fft, hop, floor, linear,
                      hist, taps) -> torch.Tensor:
    """logmel_pool (hist and taps None: swn_logmel_pool) and logmel_pool_lowcut (swn_logmel_pool_lowcut)"""
    Lb = _lib.lib()
    _need_cuda(win, "the windows")
    dev = win.device
    n_mels, E = len(bank), len(slots)
    _logmel_check(n_fft, hop, n_mels, floor)
    if win.dim() != 2 or win.dtype != torch.float32 or not win.is_contiguous():
        raise RuntimeError(f"logmel_pool needs a contiguous fp32 (slots, window) buffer, got {tuple(win.shape)} {win.dtype}")
    if not 1 <= E <= _lib.LOGMEL_POOL_MAX_ENTRIES:
        raise RuntimeError(f"logmel_pool: {E} entries, a call takes 1 .. {_lib.LOGMEL_POOL_MAX_ENTRIES}")
    if not (len(t0s) == len(n_helds) == len(n_drops) == len(n_news) == len(lens) == len(f0s) == len(f1s) == E):
        raise RuntimeError("logmel_pool: slots, t0s, n_helds, n_drops, n_news, lens, f0s and f1s must have one entry per session")
    if any(not 0 <= s < win.shape[0] for s in slots):
        raise RuntimeError(f"logmel_pool: a slot outside the buffer's {win.shape[0]} windows")
    total_new = sum(int(n) for n in n_news)
    if any(n < 0 for n in n_news) or (total_new > 0 and (staged is None or staged.device != dev or staged.dtype != torch.float32
                                                         or not staged.is_contiguous() or staged.numel() != total_new)):
        raise RuntimeError(f"logmel_pool: staged must be the {total_new} new samples as contiguous fp32 values on the windows' device")
    _tables_check("logmel_pool", tables, Lb.swn_logmel_table_floats(n_fft, n_mels), dev, "windows")
    table = (_lib.LogMelPoolEntry * E)()
    new_off = out_off = 0
    for e in range(E):
        k = max(int(f1s[e]) - int(f0s[e]), 0)
        table[e] = _lib.LogMelPoolEntry(slot=int(slots[e]), t0=int(t0s[e]), n_held=int(n_helds[e]), n_drop=int(n_drops[e]),
                                        new_off=new_off, n_new=int(n_news[e]), len=int(lens[e]), f0=int(f0s[e]), f1=int(f1s[e]),
                                        out_off=out_off, out_stride=k, reserved=0)
        new_off += int(n_news[e])
        out_off += k * n_mels
    out = torch.empty(out_off, dtype=torch.float32, device=dev)
    nb = Lb.swn_logmel_pool_work_bytes(n_fft, hop, n_mels, win.shape[1], table, E)
    work = torch.empty(max(nb, 4) // 4, dtype=torch.float32, device=dev)
    bank_c = (ctypes.c_int32 * n_mels)(*[int(b) for b in bank])
    with _on(dev):
        if taps is None:
            _lib.check(Lb.swn_logmel_pool(n_fft, hop, n_mels, float(floor), int(bool(linear)), _ptr(tables), bank_c, _ptr(win),
                                          win.shape[1], _ptr(staged), _ptr(out) if out_off else None, table, E, _ptr(work),
                                          _stream(dev)), "logmel_pool")
        else:
            _lib.check(Lb.swn_logmel_pool_lowcut(n_fft, hop, n_mels, float(floor), int(bool(linear)), _ptr(tables), bank_c,
                                                 _ptr(win), win.shape[1], _ptr(staged), _ptr(out) if out_off else None, table, E,
                                                 _ptr(work), taps.numel(), _ptr(taps), _ptr(hist), _stream(dev)),
                       "logmel_pool_lowcut")
    return out


logmel_pool = custom_op("swn::logmel_pool", mutates_args=("win",))(logmel_pool_impl)


@logmel_pool.register_fake
def _(win, staged, tables, bank, slots, t0s, n_helds, n_drops, n_news, lens, f0s, f1s, n_fft, hop, floor, linear):
    _logmel_check(n_fft, hop, len(bank), floor)
    return win.new_empty((len(bank) * sum(max(f1 - f0, 0) for f0, f1 in zip(f0s, f1s)),), dtype=torch.float32)


# ------------------------------------------------------------------------------------------ stage-1 low cut
def _lowcut_taps_check(taps: torch.Tensor, what: str) -> int:
    if taps.dim() != 1 or taps.dtype != torch.float64 or not taps.is_contiguous() or not 1 <= taps.numel() <= _lib.LOWCUT_MAX_TAPS:
        raise RuntimeError(f"{what}: taps must be 1 .. {_lib.LOWCUT_MAX_TAPS} contiguous fp64 values")
    return taps.numel()


def lowcut_chunk_impl(taps: torch.Tensor, state: torch.Tensor, inputs: List[torch.Tensor], slots: List[int],
                      resets: List[bool], capacity: int) -> torch.Tensor:
    """one call of the device low cut (swn_lowcut_chunk; the definition is in melspec.py): entry e filters inputs[e] (1-D fp32)
    as the next chunk of the session in slot slots[e] of `state` (at least capacity * (n_taps - 1) fp32, the slots' last raw
    samples, updated in place); resets[e] starts that slot from zero history.  taps: the n_taps fp64 taps.  Any number of
    entries.  -> (E, n_max) fp32, rows past an entry's own length not written."""
    L = _lib.lib()
    dev = taps.device
    _need_cuda(taps, "the taps")
    n_taps = _lowcut_taps_check(taps, "lowcut_chunk")
    E = len(inputs)
    if not (len(slots) == len(resets) == E):
        raise RuntimeError("lowcut_chunk: inputs, slots and resets must have one entry each")
    if (state.device != dev or state.dtype != torch.float32 or not state.is_contiguous()
            or state.numel() < max(1, (n_taps - 1) * int(capacity))):
        raise RuntimeError("lowcut_chunk: state must be a contiguous fp32 tensor of capacity * (n_taps - 1) values (at least one) "
                           "on the device of the taps")
    ins = []
    for x in inputs:
        if x.device != dev or x.dim() != 1 or x.dtype != torch.float32:
            raise RuntimeError("lowcut_chunk: every input must be a 1-D fp32 tensor on the device")
        ins.append(x.contiguous())
    n_max = max((x.numel() for x in ins), default=0)
    out = torch.empty((E, n_max), dtype=torch.float32, device=dev)
    table = (_lib.LowcutEntry * max(E, 1))()
    for e, x in enumerate(ins):
        n = x.numel()
        table[e] = _lib.LowcutEntry(in_dev=x.data_ptr() if n else None, out_dev=out[e].data_ptr() if n else None,
                                    slot=int(slots[e]), n=n, flags=_lib.LOWCUT_RESET if resets[e] else 0, reserved=0)
    with _on(dev):
        _lib.check(L.swn_lowcut_chunk(n_taps, _ptr(taps), _ptr(state), int(capacity), table, E, _stream(dev)), "lowcut_chunk")
    return out


lowcut_chunk = custom_op("swn::lowcut_chunk", mutates_args=("state",))(lowcut_chunk_impl)


@lowcut_chunk.register_fake
def _(taps, state, inputs, slots, resets, capacity):
    return taps.new_empty((len(inputs), max((x.numel() for x in inputs), default=0)), dtype=torch.float32)


def logmel_pool_lowcut_impl(win: torch.Tensor, hist: torch.Tensor, staged: Optional[torch.Tensor], tables: torch.Tensor,
                            bank: List[int], taps: torch.Tensor, slots: List[int], t0s: List[int], n_helds: List[int],
                            n_drops: List[int], n_news: List[int], lens: List[int], f0s: List[int], f1s: List[int], n_fft: int,
                            hop: int, floor: float, linear: bool) -> torch.Tensor:
    """logmel_pool whose `staged` samples are RAW: they reach the windows through the low cut of `taps` (n_taps fp64 values;
    swn_logmel_pool_lowcut, the bits of lowcut_chunk).  hist (slots, n_taps - 1) fp32 - at least one column - holds every
    window slot's last raw samples; an entry with t0 == 0 and n_held == 0 starts from zero history whatever its row holds.
    `win` and `hist` are updated in place."""
    _need_cuda(win, "the windows")
    n_taps = _lowcut_taps_check(taps, "logmel_pool_lowcut")
    if taps.device != win.device:
        raise RuntimeError("logmel_pool_lowcut: the taps must be on the device of the windows")
    if (hist.device != win.device or hist.dtype != torch.float32 or not hist.is_contiguous() or hist.dim() != 2
            or hist.shape[0] != win.shape[0] or hist.shape[1] != max(1, n_taps - 1)):
        raise RuntimeError(f"logmel_pool_lowcut: hist must be a contiguous fp32 ({win.shape[0]}, {max(1, n_taps - 1)}) buffer on "
                           "the device of the windows")
    return _logmel_pool_call(win, staged, tables, bank, slots, t0s, n_helds, n_drops, n_news, lens, f0s, f1s, n_fft, hop, floor,
                             linear, hist, taps)


logmel_pool_lowcut = custom_op("swn::logmel_pool_lowcut", mutates_args=("win", "hist"))(logmel_pool_lowcut_impl)


@logmel_pool_lowcut.register_fake
def _(win, hist, staged, tables, bank, taps, slots, t0s, n_helds, n_drops, n_news, lens, f0s, f1s, n_fft, hop, floor, linear):
    _logmel_check(n_fft, hop, len(bank), floor)
    return win.new_empty((len(bank) * sum(max(f1 - f0, 0) for f0, f1 in zip(f0s, f1s)),), dtype=torch.float32)


# ------------------------------------------------------------------------------------------ rational resampler
def _resample_call(table, state, in_ptrs, n_ins, slots, in0s, out0s, n_outs, lens, up, down, n_taps, capacity, dense, what):
    """the checks and the swn_resample_chunk call that resample_chunk and resample_staged share: entry e reads n_ins[e] floats
    at the device address in_ptrs[e]"""
    Lb = _lib.lib()
    dev = table.device
    _need_cuda(table, "the polyphase table")
    up, down, n_taps, capacity = int(up), int(down), int(n_taps), int(capacity)
    doubles = int(Lb.swn_resample_table_doubles(up, down, n_taps))
    if doubles == 0:
        raise RuntimeError(f"{what}: no table for up {up}, down {down}, n_taps {n_taps} (coprime, n_taps odd, up <= "
                           f"{_lib.RESAMPLE_MAX_UP}, Q <= {_lib.RESAMPLE_MAX_Q})")
    H = doubles // up - 1
    if table.dim() != 1 or table.dtype != torch.float64 or not table.is_contiguous() or table.numel() != doubles:
        raise RuntimeError(f"{what}: table must be {doubles} contiguous fp64 values")
    E = len(n_ins)
    if not (len(slots) == len(in0s) == len(out0s) == len(n_outs) == len(lens) == E):
        raise RuntimeError(f"{what}: the inputs, slots, in0s, out0s, n_outs and lens must have one entry each")
    if (state.device != dev or state.dtype != torch.float32 or not state.is_contiguous()
            or state.numel() < max(1, H * capacity)):
        raise RuntimeError(f"{what}: state must be a contiguous fp32 tensor of capacity * (Q - 1) values (at least one) on the "
                           "device of the table")
    counts = [int(n) for n in n_outs]
    if min(counts, default=0) < 0:
        raise RuntimeError(f"{what}: a negative output count")
    if dense:
        out, stride = torch.empty((sum(counts),), dtype=torch.float32, device=dev), 0
    else:
        out = torch.empty((E, max(counts, default=0)), dtype=torch.float32, device=dev)
        stride = 4 * out.shape[1]
    tab = (_lib.ResampleEntry * max(E, 1))()
    at = out.data_ptr()
    for e in range(E):
        k = counts[e]
        tab[e] = _lib.ResampleEntry(in_ptrs[e] if n_ins[e] else None, at if k else None, int(in0s[e]), int(out0s[e]), int(lens[e]),
                                    n_ins[e], k, int(slots[e]), 0)
        at += stride if stride else 4 * k
    with _on(dev):
        _lib.check(Lb.swn_resample_chunk(up, down, n_taps, _ptr(table), _ptr(state), capacity, tab, E, _stream(dev)), what)
    return out


def resample_chunk_impl(table: torch.Tensor, state: torch.Tensor, inputs: List[torch.Tensor], slots: List[int], in0s: List[int],
                        out0s: List[int], n_outs: List[int], lens: List[int], up: int, down: int, n_taps: int, capacity: int,
                        dense: bool) -> torch.Tensor:
    """one call of the device resampler (swn_resample_chunk; the definition is in melspec.py): entry e takes inputs[e] (1-D fp32,
    the session's inputs [in0s[e], in0s[e] + n)) as the next chunk of the session in slot slots[e] of `state` (at least
    capacity * (Q - 1) fp32, the slots' last raw inputs, updated in place) and computes its outputs
    [out0s[e], out0s[e] + n_outs[e]); lens[e] is the signal's length (the chunk then ends it), or -1 while it goes on.  An entry
    with in0 == 0 starts from zero history.  table: the up * Q fp64 values of the polyphase table, row by row.  Any number of
    entries.  -> dense: a flat buffer with every entry's outputs back to back in entry order; else (E, max n_out) fp32, rows
    past an entry's own count not written."""
    dev = table.device
    ins = []
    for x in inputs:
        if x.device != dev or x.dim() != 1 or x.dtype != torch.float32:
            raise RuntimeError("resample_chunk: every input must be a 1-D fp32 tensor on the device of the table")
        ins.append(x.contiguous())
    return _resample_call(table, state, [x.data_ptr() for x in ins], [x.numel() for x in ins], slots, in0s, out0s, n_outs, lens,
                          up, down, n_taps, capacity, dense, "resample_chunk")


resample_chunk = custom_op("swn::resample_chunk", mutates_args=("state",))(resample_chunk_impl)


@resample_chunk.register_fake
def _(table, state, inputs, slots, in0s, out0s, n_outs, lens, up, down, n_taps, capacity, dense):
    if dense:
        return table.new_empty((sum(n_outs),), dtype=torch.float32)
    return table.new_empty((len(inputs), max(n_outs, default=0)), dtype=torch.float32)


def resample_staged_impl(table: torch.Tensor, state: torch.Tensor, staged: Optional[torch.Tensor], n_ins: List[int],
                         slots: List[int], in0s: List[int], out0s: List[int], n_outs: List[int], lens: List[int], up: int,
                         down: int, n_taps: int, capacity: int) -> torch.Tensor:
    """resample_chunk for a whole tick of a pool, with no tensor per entry: `staged` holds the entries' chunks back to back in
    entry order (n_ins[e] fp32 samples each; None when there are none), as logmel_pool takes its new samples -> a flat buffer
    with every entry's n_outs[e] outputs back to back in entry order: what the pool call that follows takes as `staged`."""
    total = sum(int(n) for n in n_ins)
    if min((int(n) for n in n_ins), default=0) < 0:
        raise RuntimeError("resample_staged: a negative input count")
    if total and (staged is None or staged.device != table.device or staged.dim() != 1 or staged.dtype != torch.float32
                  or not staged.is_contiguous() or staged.numel() < total):
        raise RuntimeError(f"resample_staged: staged must be a contiguous 1-D fp32 tensor of at least {total} samples on the device "
                           "of the table")
    ptrs, at = [], staged.data_ptr() if total else 0
    for n in n_ins:
        ptrs.append(at)
        at += 4 * int(n)
    return _resample_call(table, state, ptrs, [int(n) for n in n_ins], slots, in0s, out0s, n_outs, lens, up, down, n_taps,
                          capacity, True, "resample_staged")


resample_staged = custom_op("swn::resample_staged", mutates_args=("state",))(resample_staged_impl)


@resample_staged.register_fake
def _(table, state, staged, n_ins, slots, in0s, out0s, n_outs, lens, up, down, n_taps, capacity):
    return table.new_empty((sum(n_outs),), dtype=torch.float32)


OP_NAMES = ("pack_params", "frontend", "frontend_pool", "decode", "decode_chunk", "decode_pool_chunk", "decode_pool_stepped_chunk",
            "pack_decode_w16", "decode_w16", "decode_chunk_w16", "decode_pool_chunk_w16",
            "pack_decode_w8", "decode_w8", "decode_chunk_w8", "decode_pool_chunk_w8", "e4m3_table",
            "frontend_pool_models", "decode_pool_chunk_models", "decode_pool_chunk_models_w16", "decode_pool_chunk_models_w8",
            "decode_pool_chunk_wide",
            "decode_pool_stepped_chunk_models", "decode_stepped_prologue",
            "postfilter_chunk",
            "stack_forward", "pack_bf16", "stack_forward_bf16", "laplace_head",
            "laplace_head_backward", "stack_backward", "stack_backward_bf16", "spectral_loss", "spectral_loss_backward",
            "laplace_loss", "laplace_loss_backward", "logmel", "logmel_pool", "mcep", "lowcut_chunk", "logmel_pool_lowcut",
            "resample_chunk", "resample_staged", "f0", "bap", "envelope")
