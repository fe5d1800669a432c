"""ctypes binding of the C ABI in include/swn_hip.h (libswn_hip.so, built in-tree by
csrc/Makefile with hipcc --offload-arch=gfx950).

There is deliberately no fallback: if the library cannot be loaded the product path raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

from .config import NetConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWN_HIP_LIB", os.path.join(_HERE, "libswn_hip.so"))   # override: diagnostic builds
CSRC = os.path.join(_HERE, "csrc")

_lock = threading.Lock()
_lib = None


class NetDesc(ctypes.Structure):
    """mirror of `swn_net_desc` (include/swn_hip.h)."""
    _fields_ = [(n, c_int32) for n in (
        "kind", "n_aux", "hid_chn", "skip_chn", "aux_kernel_size", "aux_dilation_size",
        "dilation_depth", "dilation_repeat", "kernel_size", "upsampling_factor", "seg", "lpc",
        "n_quantize", "wav_conv_flag", "audio_in_flag", "aux_conv2d_flag")]


class DecodeIO(ctypes.Structure):
    """mirror of `swn_decode_io` (include/swn_hip.h): inputs of the sampling loop."""
    _fields_ = [("noise_dev", c_void_p), ("forced_dev", c_void_p), ("seed_dev", c_void_p), ("noise_out_dev", c_void_p),
                ("rng_seed", ctypes.c_uint64), ("rng_utt0", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("rng_utt_ids_dev", c_void_p)]


class DecodePoolEntry(ctypes.Structure):
    """mirror of `swn_decode_pool_entry` (include/swn_hip.h): one session's share of a pool launch."""
    _fields_ = [("cond_dev", c_void_p), ("n_frames", c_int32), ("slot", c_int32), ("step0", c_int32),
                ("n_steps", c_int32), ("flags", c_int32), ("reserved", c_int32)]


class DecodeSteppedPoolEntry(ctypes.Structure):
    """mirror of `swn_decode_stepped_pool_entry` (include/swn_hip.h): one session's share of a stepped pool call."""
    _fields_ = [("cond_dev", c_void_p), ("n_frames", c_int32), ("slot", c_int32), ("it0", c_int32),
                ("n_it", c_int32), ("flags", c_int32), ("reserved", c_int32)]


class DecodeSteppedPrologueEntry(ctypes.Structure):
    """mirror of `swn_decode_stepped_prologue_entry` (include/swn_hip.h): one beginning session of a parallel prologue call."""
    _fields_ = [("cond_dev", c_void_p), ("n_frames", c_int32), ("slot", c_int32)]


class FrontendPoolEntry(ctypes.Structure):
    """mirror of `swn_frontend_pool_entry` (include/swn_hip.h): one session's share of a pool front end call."""
    _fields_ = [("aux_dev", c_void_p), ("new_dev", c_void_p), ("cond_dev", c_void_p), ("aux_stride", c_int32),
                ("n_received", c_int32), ("n_new", c_int32), ("f0", c_int32), ("f1", c_int32), ("flags", c_int32),
                ("reserved", c_int32 * 2)]


class PostfilterEntry(ctypes.Structure):
    """mirror of `swn_postfilter_entry` (include/swn_hip.h): one session's share of a post-filter call."""
    _fields_ = [("in_dev", c_void_p), ("out_dev", c_void_p), ("slot", c_int32), ("n", c_int32), ("kind", c_int32),
                ("flags", c_int32)]


class LogMelEntry(ctypes.Structure):
    """mirror of `swn_logmel_entry` (include/swn_hip.h): one row's share of a log-mel call."""
    _fields_ = [("wav_dev", c_void_p), ("out_dev", c_void_p), ("t0", c_int32), ("n_avail", c_int32), ("len", c_int32),
                ("f0", c_int32), ("f1", c_int32), ("reserved", c_int32)]


class EnvelopeEntry(ctypes.Structure):
    """mirror of `swn_envelope_entry` (include/swn_hip.h): one row's share of a spectral envelope call."""
    _fields_ = [("wav_dev", c_void_p), ("out_dev", c_void_p), ("f0_dev", c_void_p), ("t0", c_int32), ("n_avail", c_int32),
                ("len", c_int32), ("f0", c_int32), ("f1", c_int32), ("reserved", ctypes.c_int16), ("reserved2", ctypes.c_int16)]


class LogMelPoolEntry(ctypes.Structure):
    """mirror of `swn_logmel_pool_entry` (include/swn_hip.h): one session's share of a log-mel pool call."""
    _fields_ = [(n, c_int32) for n in ("slot", "t0", "n_held", "n_drop", "new_off", "n_new", "len", "f0", "f1", "out_off",
                                       "out_stride", "reserved")]


class LowcutEntry(ctypes.Structure):
    """mirror of `swn_lowcut_entry` (include/swn_hip.h): one session's share of a low-cut call."""
    _fields_ = [("in_dev", c_void_p), ("out_dev", c_void_p), ("slot", c_int32), ("n", c_int32), ("flags", c_int32),
                ("reserved", c_int32)]


class ResampleEntry(ctypes.Structure):
    """mirror of `swn_resample_entry` (include/swn_hip.h): one session's next chunk of a resampler call."""
    _fields_ = [("in_dev", c_void_p), ("out_dev", c_void_p), ("in0", c_int64), ("out0", c_int64), ("len", c_int64),
                ("n_in", c_int32), ("n_out", c_int32), ("slot", c_int32), ("reserved", c_int32)]


ABI_VERSION = 3
DECODE_POOL_MAX_ENTRIES = 64                   # SWN_DECODE_POOL_MAX_ENTRIES (include/swn_hip.h): entries per pool launch
DECODE_POOL_WIDE_MAX_ENTRIES = 256             # SWN_DECODE_POOL_WIDE_MAX_ENTRIES: entries per wide launch (swn_decode_pool_chunk_wide)
WEIGHTS_FP32, WEIGHTS_BF16, WEIGHTS_E4M3 = 0, 1, 2   # SWN_WEIGHTS_*: the weight_format of swn_decode_pool_chunk_wide
DECODE_STEPPED_POOL_TABLE_FLOATS = 512          # SWN_DECODE_STEPPED_POOL_TABLE_FLOATS (include/swn_hip.h)
DECODE_STEPPED_POOL_MODELS_TABLE_FLOATS = 640   # SWN_DECODE_STEPPED_POOL_MODELS_TABLE_FLOATS (include/swn_hip.h)
DECODE_STEPPED_POOL_MAX_TILES = 23             # SWN_DECODE_STEPPED_POOL_MAX_TILES (include/swn_hip.h)
FRONTEND_POOL_MAX_ENTRIES = 64                 # SWN_FRONTEND_POOL_MAX_ENTRIES (include/swn_hip.h): entries per front end call
POOL_MAX_MODELS = 16                           # SWN_POOL_MAX_MODELS (include/swn_hip.h): distinct models per *_models call
FRONTEND_FINAL = 1                             # SWN_FRONTEND_FINAL: the entry's features end at n_received
CHUNK_BEGIN = 1                                # SWN_CHUNK_BEGIN (include/swn_hip.h): first chunk of a streamed decode
PRECISION_FP32, PRECISION_BF16 = 0, 1          # SWN_PRECISION_* (include/swn_hip.h)
# SWN_BF16_PATH_* (include/swn_hip.h): what swn_forward_bf16_path returns, by value
BF16_PATHS = ("fused", "units4", "units4_halves", "units5", "units7", "layer0", "gemm_stack")
POSTFILTER_IN_F32, POSTFILTER_IN_MULAW = 0, 1   # SWN_POSTFILTER_IN_* (include/swn_hip.h)
POSTFILTER_RESET = 1                           # SWN_POSTFILTER_RESET
POSTFILTER_MAX_ORDER = 62                      # SWN_POSTFILTER_MAX_ORDER
POSTFILTER_MAX_TAPS = 256                      # SWN_POSTFILTER_MAX_TAPS
POSTFILTER_MULAW_ENTRIES = 256                 # SWN_POSTFILTER_MULAW_ENTRIES
LOWCUT_MAX_TAPS, LOWCUT_TILE = 256, 1024       # SWN_LOWCUT_MAX_TAPS, SWN_LOWCUT_TILE: output samples per block of the kernel
LOWCUT_MAX_ENTRIES, LOWCUT_RESET = 64, 1       # SWN_LOWCUT_MAX_ENTRIES (entries per launch group), SWN_LOWCUT_RESET
RESAMPLE_MAX_UP, RESAMPLE_MAX_Q, RESAMPLE_MAX_TAPS = 1024, 256, 65535    # SWN_RESAMPLE_MAX_UP, _MAX_Q, _MAX_TAPS
RESAMPLE_MAX_ENTRIES, RESAMPLE_TILE, RESAMPLE_MAX_SPAN = 64, 1024, 8192  # SWN_RESAMPLE_MAX_ENTRIES, _TILE (outputs per block), _MAX_SPAN
SPECTRAL_MAX_SIZES, SPECTRAL_MAX_FFT = 32, 2048   # SWN_SPECTRAL_MAX_SIZES, SWN_SPECTRAL_MAX_FFT
LOGMEL_MAX_MELS, LOGMEL_MAX_ENTRIES = 128, 64     # SWN_LOGMEL_MAX_MELS, SWN_LOGMEL_MAX_ENTRIES
LOGMEL_POOL_MAX_ENTRIES = 64                   # SWN_LOGMEL_POOL_MAX_ENTRIES (include/swn_hip.h): entries per log-mel pool call
MCEP_MAX_ORDER = 63                            # SWN_MCEP_MAX_ORDER (include/swn_hip.h)
F0_MAX_HOP, F0_MIN_WIN, F0_MAX_WIN, F0_MAX_LAG = 4096, 16, 2048, 1536    # SWN_F0_MAX_HOP, _MIN_WIN, _MAX_WIN, _MAX_LAG
BAP_MAX_BANDS, BAP_MAX_TAPS, BAP_TILE = 5, 255, 1280                     # SWN_BAP_MAX_BANDS, _MAX_TAPS, _TILE
ENVELOPE_MCEP, ENVELOPE_LOGAMP = 0, 1                                    # SWN_ENVELOPE_MCEP, SWN_ENVELOPE_LOGAMP


def desc_from_cfg(cfg: NetConfig) -> NetDesc:
    soft = cfg.kind == "softmax"
    return NetDesc(kind=1 if soft else 0, n_aux=cfg.n_aux, hid_chn=cfg.hid_chn, skip_chn=cfg.skip_chn,
                   aux_kernel_size=cfg.aux_kernel_size, aux_dilation_size=cfg.aux_dilation_size,
                   dilation_depth=cfg.dilation_depth, dilation_repeat=cfg.dilation_repeat,
                   kernel_size=cfg.kernel_size, upsampling_factor=cfg.upsampling_factor,
                   seg=1 if soft else cfg.seg, lpc=0 if soft else cfg.lpc,
                   n_quantize=cfg.n_quantize if soft else 0,
                   wav_conv_flag=int(cfg.wav_conv_flag), audio_in_flag=int(cfg.audio_in_flag and soft),
                   aux_conv2d_flag=int(cfg.aux_conv2d_flag and not soft))


# name -> (restype, argtypes); must list every symbol include/swn_hip.h declares
SIGNATURES = {
    "swn_abi_version": (c_int, []),
    "swn_strerror": (c_char_p, [c_int]),
    "swn_last_error_detail": (c_char_p, []),
    "swn_device_count": (c_int, []),
    "swn_receptive_field": (c_int, [POINTER(NetDesc)]),
    "swn_num_tensors": (c_int, [POINTER(NetDesc)]),
    "swn_packed_floats": (c_size_t, [POINTER(NetDesc)]),
    "swn_layout_offsets": (c_int, [POINTER(NetDesc), POINTER(c_size_t), c_int]),
    "swn_pack_params": (c_int, [POINTER(NetDesc), POINTER(c_void_p), c_int, c_void_p, c_size_t]),
    "swn_pack_params_device": (c_int, [POINTER(NetDesc), POINTER(c_void_p), c_int, c_void_p, c_size_t, c_void_p]),
    "swn_frontend_conv_lds_bytes": (c_size_t, [POINTER(NetDesc), c_int]),
    "swn_frontend_work_floats": (c_size_t, [POINTER(NetDesc), c_int, c_int]),
    "swn_cond_floats": (c_size_t, [POINTER(NetDesc), c_int, c_int]),
    "swn_frontend": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "swn_frontend_pool_work_floats": (c_size_t, [POINTER(NetDesc), POINTER(FrontendPoolEntry), c_int]),
    "swn_frontend_pool": (c_int, [POINTER(NetDesc), c_void_p, POINTER(FrontendPoolEntry), c_int, c_void_p, c_void_p]),
    "swn_frontend_pool_models_work_floats": (c_size_t, [POINTER(NetDesc), POINTER(FrontendPoolEntry), POINTER(c_int32), c_int,
                                                        c_int]),
    "swn_frontend_pool_models": (c_int, [POINTER(NetDesc), POINTER(c_void_p), c_int, POINTER(c_int32),
                                         POINTER(FrontendPoolEntry), c_int, c_void_p, c_void_p]),
    "swn_decode_state_floats": (c_size_t, [POINTER(NetDesc), c_int]),
    "swn_decode": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_int, c_int, c_int, POINTER(DecodeIO),
                           c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "swn_decode_bl6w_lds_bytes": (c_size_t, [POINTER(NetDesc), c_int]),
    "swn_decode_resolve_variant": (c_int, [POINTER(NetDesc), c_int, c_int]),
    "swn_decode_session_floats": (c_size_t, [POINTER(NetDesc), c_int, c_int]),
    "swn_decode_chunk": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(DecodeIO),
                                 c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "swn_decode_pool_chunk": (c_int, [POINTER(NetDesc), c_void_p, c_int, POINTER(DecodePoolEntry), c_int, POINTER(DecodeIO),
                                      c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "swn_decode_pool_chunk_models": (c_int, [POINTER(NetDesc), POINTER(c_void_p), c_int, POINTER(c_int32), c_int,
                                             POINTER(DecodePoolEntry), c_int, POINTER(DecodeIO), c_void_p, c_void_p, c_void_p,
                                             c_int, c_void_p]),
    "swn_decode_pool_wide_table_bytes": (c_size_t, [c_int]),
    "swn_decode_pool_chunk_wide": (c_int, [POINTER(NetDesc), POINTER(c_void_p), c_int, POINTER(c_int32), c_int,
                                           POINTER(DecodePoolEntry), c_int, POINTER(DecodeIO), c_void_p, c_void_p, c_void_p,
                                           c_int, POINTER(c_void_p), c_int, c_void_p, c_void_p]),
    "swn_e4m3_table": (c_int, [c_void_p, c_float, c_void_p]),
    "swn_decode_stepped_prologue_iterations": (c_int, [POINTER(NetDesc)]),
    "swn_decode_pool_stepped_chunk": (c_int, [POINTER(NetDesc), c_void_p, c_int, POINTER(DecodeSteppedPoolEntry), c_int,
                                              POINTER(DecodeIO), c_void_p, c_void_p, c_void_p, c_void_p]),
    "swn_decode_stepped_pool_plan": (c_int, [POINTER(c_int32), POINTER(c_int32), c_int, c_int, c_int, POINTER(c_int32),
                                             POINTER(c_int32)]),
    "swn_decode_pool_stepped_chunk_models": (c_int, [POINTER(NetDesc), POINTER(c_void_p), c_int, POINTER(c_int32), c_int,
                                                     POINTER(DecodeSteppedPoolEntry), c_int, POINTER(DecodeIO), c_void_p,
                                                     c_void_p, c_void_p, c_void_p]),
    "swn_decode_stepped_prologue_work_floats": (c_size_t, [POINTER(NetDesc), c_int]),
    "swn_decode_stepped_prologue": (c_int, [POINTER(NetDesc), c_void_p, POINTER(c_void_p), c_int, POINTER(c_int32), c_int,
                                            POINTER(DecodeSteppedPrologueEntry), c_int, POINTER(DecodeIO), c_void_p, c_void_p,
                                            c_void_p]),
    "swn_postfilter_state_doubles": (c_size_t, [c_int, c_int, c_int]),
    "swn_postfilter_chunk": (c_int, [c_int, ctypes.c_double, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                     POINTER(PostfilterEntry), c_int, c_void_p]),
    "swn_forward_work_floats": (c_size_t, [POINTER(NetDesc), c_int, c_int]),
    "swn_forward": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                            c_void_p, c_void_p, c_void_p]),
    "swn_bf16_weight_bytes": (c_size_t, [POINTER(NetDesc)]),
    "swn_pack_bf16": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p]),
    "swn_forward_bf16_work_bytes": (c_size_t, [POINTER(NetDesc), c_int, c_int]),
    "swn_forward_bf16": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_void_p, c_void_p, c_void_p]),
    "swn_forward_bf16_path": (c_int, [POINTER(NetDesc), c_int, c_int]),
    "swn_backward_work_floats": (c_size_t, [POINTER(NetDesc), c_int, c_int]),
    "swn_backward": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "swn_drop_fused_path": (c_int, [POINTER(NetDesc), c_int, c_int, c_void_p]),
    "swn_forward_drop_work_floats": (c_size_t, [POINTER(NetDesc), c_int, c_int]),
    "swn_forward_drop": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "swn_unfold_grads_device": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "swn_forward_bf16_keep_floats": (c_size_t, [POINTER(NetDesc), c_int, c_int]),
    "swn_forward_bf16_keep": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "swn_backward_keep": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "swn_backward_bf16_work_floats": (c_size_t, [POINTER(NetDesc), c_int, c_int]),
    "swn_backward_bf16": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "swn_backward_drop_work_floats": (c_size_t, [POINTER(NetDesc), c_int, c_int]),
    "swn_backward_drop": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "swn_bf16_train_forward_supported": (c_int, [POINTER(NetDesc)]),
    "swn_bf16_work_to_f32": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]),
    "swn_laplace_head_backward": (c_int, [POINTER(NetDesc), c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "swn_laplace_head": (c_int, [POINTER(NetDesc), c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "swn_spectral_work_bytes": (c_size_t, [c_int, c_int, POINTER(c_int), c_int]),
    "swn_spectral_state_bytes": (c_size_t, [c_int, c_int, POINTER(c_int), c_int]),
    "swn_spectral_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
    "swn_spectral_backward": (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "swn_laplace_loss_work_bytes": (c_size_t, [POINTER(NetDesc), c_int, c_int, c_int]),
    "swn_laplace_loss_forward": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "swn_laplace_loss_backward": (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_void_p, c_void_p, c_void_p, c_void_p]),
    "swn_logmel_table_floats": (c_size_t, [c_int, c_int]),
    "swn_logmel_work_bytes": (c_size_t, [c_int, c_int, POINTER(LogMelEntry), c_int]),
    "swn_logmel": (c_int, [c_int, c_int, c_int, c_float, c_int, c_void_p, POINTER(c_int32), POINTER(LogMelEntry), c_int,
                           c_void_p, c_void_p]),
    "swn_mcep_table_floats": (c_size_t, [c_int, c_int]),
    "swn_mcep_work_bytes": (c_size_t, [c_int, c_int, POINTER(LogMelEntry), c_int]),
    "swn_mcep": (c_int, [c_int, c_int, c_int, c_float, c_void_p, POINTER(LogMelEntry), c_int, c_void_p, c_void_p]),
    "swn_logmel_pool_window_floats": (c_size_t, [c_int, c_int]),
    "swn_logmel_pool_work_bytes": (c_size_t, [c_int, c_int, c_int, c_size_t, POINTER(LogMelPoolEntry), c_int]),
    "swn_logmel_pool": (c_int, [c_int, c_int, c_int, c_float, c_int, c_void_p, POINTER(c_int32), c_void_p, c_size_t, c_void_p,
                                c_void_p, POINTER(LogMelPoolEntry), c_int, c_void_p, c_void_p]),
    "swn_lowcut_state_floats": (c_size_t, [c_int]),
    "swn_lowcut_chunk": (c_int, [c_int, c_void_p, c_void_p, c_int, POINTER(LowcutEntry), c_int, c_void_p]),
    "swn_logmel_pool_lowcut": (c_int, [c_int, c_int, c_int, c_float, c_int, c_void_p, POINTER(c_int32), c_void_p, c_size_t,
                                       c_void_p, c_void_p, POINTER(LogMelPoolEntry), c_int, c_void_p, c_int, c_void_p, c_void_p,
                                       c_void_p]),
    "swn_resample_table_doubles": (c_size_t, [c_int, c_int, c_int]),
    "swn_resample_state_floats": (c_size_t, [c_int, c_int]),
    "swn_resample_chunk": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int, POINTER(ResampleEntry), c_int, c_void_p]),
    "swn_f0_span": (c_int, [c_int, c_int]),
    "swn_f0": (c_int, [ctypes.c_double, c_int, c_int, c_int, c_int, ctypes.c_double, POINTER(LogMelEntry), c_int, c_void_p]),
    "swn_bap_reach": (c_int, [c_int, c_int, c_int]),
    "swn_bap_work_bytes": (c_size_t, [c_int, c_int, c_int, c_int, POINTER(LogMelEntry), c_int]),
    "swn_bap": (c_int, [ctypes.c_double, c_int, c_int, c_int, c_int, ctypes.c_double, c_int, c_int, c_int, c_void_p, ctypes.c_float,
                POINTER(LogMelEntry), c_int, c_void_p, c_void_p]),
    "swn_envelope_table_doubles": (c_size_t, [c_int, c_int]),
    "swn_envelope_work_bytes": (c_size_t, [c_int, c_int, POINTER(EnvelopeEntry), c_int]),
    "swn_envelope": (c_int, [ctypes.c_double, c_int, c_int, c_int, ctypes.c_float, ctypes.c_double, ctypes.c_double, c_int, c_void_p,
                     POINTER(EnvelopeEntry), c_int, c_void_p, c_void_p]),
}


# the stored formats of the streamed head matrices (ops.DECODE_IMAGES): the size and the packing of the image, and the three
# decode calls with the image between the variant and the stream; the pool over several models takes a host array of images there
for _s in ("w16", "w8"):
    SIGNATURES[f"swn_decode_{_s}_bytes"] = (c_size_t, [POINTER(NetDesc)])
    SIGNATURES[f"swn_pack_decode_{_s}"] = (c_int, [POINTER(NetDesc), c_void_p, c_void_p, c_void_p])
    for _n, _image in (("swn_decode", c_void_p), ("swn_decode_chunk", c_void_p), ("swn_decode_pool_chunk", c_void_p),
                       ("swn_decode_pool_chunk_models", POINTER(c_void_p))):
        _res, _args = SIGNATURES[_n]
        SIGNATURES[f"{_n}_{_s}"] = (_res, _args[:-1] + [_image] + _args[-1:])


STAMP_PATH = os.path.join(_HERE, "libswn_hip.so.srchash")


def source_hash() -> str:
    """sha256 over everything the library is built from: csrc/* sources + Makefile + the public header."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".hpp")) or f == "Makefile")
    for path in [os.path.join(CSRC, f) for f in files] + [os.path.join(os.path.dirname(_HERE), "include", "swn_hip.h")]:
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def is_stale() -> bool:
    """True when the in-tree .so is missing or was not built from the sources now in the tree (the .so and its
    hash stamp are git-ignored but travel to the GPU box, so a stale binary would otherwise go unnoticed)."""
    if not (os.path.exists(LIB_PATH) and os.path.exists(STAMP_PATH)):
        return True
    with open(STAMP_PATH) as f:
        return f.read().strip() != source_hash()


def build(force: bool = False) -> str:
    """compile the HIP library in-tree (hipcc cross-compiles gfx950 without a GPU).  A library whose recorded source
    hash differs from the tree is rebuilt from scratch; `force` rebuilds regardless."""
    if force or is_stale():
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=True)
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libswn_hip.so failed:\n" + r.stdout + r.stderr)
    write_stamp()
    return LIB_PATH


def write_stamp() -> None:
    """record which sources the in-tree .so was built from (also called by csrc/Makefile after linking)."""
    with open(STAMP_PATH, "w") as f:
        f.write(source_hash() + "\n")


def lib() -> ctypes.CDLL:
    """load (building if absent) libswn_hip.so; raises RuntimeError when unavailable."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            build()
        elif is_stale():
            # a binary that was not built from the sources in the tree: rebuild where a compiler exists, else say so
            import shutil
            import warnings
            if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
                build()
            else:
                warnings.warn(f"{LIB_PATH} was not built from the sources in this tree (source hash differs) and no hipcc "
                              "is available to rebuild it", RuntimeWarning)
        # torch ships its own libamdhip64; it must be in the process BEFORE our library so that both
        # resolve to ONE HIP runtime (device pointers and streams come from torch).  Loading ours
        # first binds /opt/rocm's copy, which then reports "no ROCm-capable device".
        import torch  # noqa: F401
        try:
            l = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise RuntimeError(f"shallow_wavenet_amd: cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        if l.swn_abi_version() != ABI_VERSION:
            raise RuntimeError("shallow_wavenet_amd: ABI version mismatch")
        _lib = l
        return l


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().swn_strerror(rc).decode()
        detail = lib().swn_last_error_detail().decode()
        raise RuntimeError(f"swn_hip {what}: {msg} ({rc}) {detail}")
