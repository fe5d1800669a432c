"""Noise-shaping restoration on the device: run.sh stage 6 / 9 (`noise_shaping.py --inv false`, run.sh:713-740) as a resumable
post-filter of decode streams and pools (swn_postfilter_chunk, csrc/swn_postfilter.hip).

`NoiseShapingRestorer` computes what `dsp.noise_shaping(x, mean_mcep, fs, alpha, mag, mcep_dim_start, inv)` computes - the
time-invariant MLSA filter of the corpus-mean mel-cepstrum, then the 255-tap causal low cut, both from zero state - on the
device in fp64, with fp32 samples out.  Each of its `capacity` slots keeps one session's filter state between calls, so the
restored chunks of a session concatenate to exactly the restore of the whole signal, whatever the chunking.

    r = NoiseShapingRestorer(mean_mcep, fs, alpha, capacity=8)
    ys = r.restore([x0, x1])                 # one-shot: 1-D device tensors, each filtered from zero state
    s = r.open()                             # a free slot (or open(slot) for a given one); starts from zero state
    out = r.run({s: chunk})                  # {slot: restored chunk}; one device call for all slots
    r.close(s)

Inputs are fp32 samples, or integer mu-law classes (decoded on the device through decode_mu_law(arange(Q)) in fp64).
"""
from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib, dsp
from . import ops as _ops          # registers torch.ops.swn.*

_O = torch.ops.swn


class NoiseShapingRestorer:
    """the device post-filter of one (mean mel-cepstrum, fs, alpha, mag, mcep_dim_start, inv) setting, with `capacity` session
    slots.  pade: the Pade order of the MLSA filter (4 as dsp.MLSAFilter defaults to, or 5); cutoff: the low cut in Hz."""

    def __init__(self, mean_mcep, fs: int, alpha: float, mag: float = 0.5, mcep_dim_start: int = 5, inv: bool = False,
                 pade: int = 4, capacity: int = 1, device="cuda", cutoff: float = 70.0):
        if pade not in (4, 5):
            raise ValueError("Pade order must be 4 or 5")
        if not abs(float(alpha)) < 1.0:
            raise ValueError(f"|alpha| must be < 1, not {alpha!r}")
        if not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer, not {capacity!r}")
        self.b = dsp.mc2b(dsp.shaping_mcep(mean_mcep, mag, mcep_dim_start, inv), alpha)
        self.taps = np.asarray(dsp.low_cut_taps(fs, cutoff), dtype=np.float64)
        self.order = self.b.size - 1
        if self.order < 1:
            raise ValueError("the mel-cepstrum needs at least two coefficients from mcep_dim_start on")
        if self.order > _lib.POSTFILTER_MAX_ORDER:
            raise ValueError(f"order {self.order} exceeds the device post-filter's {_lib.POSTFILTER_MAX_ORDER}")
        self.fs, self.alpha, self.pade, self.capacity = int(fs), float(alpha), int(pade), capacity
        self.n_taps = self.taps.size
        self.device = torch.device(device)
        self.state_doubles = int(_lib.lib().swn_postfilter_state_doubles(self.order, self.pade, self.n_taps))
        base = np.concatenate([self.b, self.taps])
        self._image = torch.from_numpy(base).to(self.device)
        self._images = {}                                     # Q -> image with the mu-law table of Q classes
        self._state = torch.zeros(capacity * self.state_doubles, dtype=torch.float64, device=self.device)
        self._free = list(range(capacity))
        self._reset = set()                                   # opened slots that have not run yet

    # ------------------------------------------------------------------ image
    def _image_for(self, n_quantize: Optional[int]) -> torch.Tensor:
        if n_quantize is None:
            return self._image
        q = int(n_quantize)
        img = self._images.get(q)
        if img is None:
            if not 1 <= q <= _lib.POSTFILTER_MULAW_ENTRIES:
                raise ValueError(f"mu-law with {q} classes: the device table holds {_lib.POSTFILTER_MULAW_ENTRIES}")
            from .nets.dswnv import decode_mu_law
            table = np.zeros(_lib.POSTFILTER_MULAW_ENTRIES, dtype=np.float64)
            table[:q] = decode_mu_law(np.arange(q, dtype=np.float64), q)
            table[q:] = table[q - 1]
            img = self._images[q] = torch.cat([self._image, torch.from_numpy(table).to(self.device)])
        return img

    def _prep(self, x: torch.Tensor, n_quantize: Optional[int]) -> torch.Tensor:
        x = torch.as_tensor(x).reshape(-1)
        if x.is_floating_point():
            return x.to(self.device, torch.float32)
        if n_quantize is None:
            raise ValueError("integer (mu-law class) input needs n_quantize")
        return x.to(self.device, torch.int32)

    def _call(self, state: torch.Tensor, capacity: int, xs: Sequence[torch.Tensor], slots: Sequence[int],
              resets: Sequence[bool], n_quantize: Optional[int]) -> torch.Tensor:
        ins = [self._prep(x, n_quantize) for x in xs]
        if any(x.dtype == torch.int32 for x in ins) and n_quantize is None:
            raise ValueError("integer (mu-law class) input needs n_quantize")
        return _O.postfilter_chunk(self._image_for(n_quantize if any(x.dtype == torch.int32 for x in ins) else None),
                                   state, ins, [int(s) for s in slots], [bool(r) for r in resets], self.order,
                                   self.alpha, self.pade, self.n_taps, capacity)

    # ------------------------------------------------------------------ one shot
    def restore(self, xs: Sequence[torch.Tensor], n_quantize: Optional[int] = None) -> List[torch.Tensor]:
        """each 1-D signal restored from zero state (one device call; the open sessions' slots are not touched) -> fp32 tensors
        on the device, of the input lengths."""
        xs = list(xs)
        if not xs:
            return []
        state = torch.empty(len(xs) * self.state_doubles, dtype=torch.float64, device=self.device)
        out = self._call(state, len(xs), xs, range(len(xs)), [True] * len(xs), n_quantize)
        return [out[e, :int(torch.as_tensor(x).numel())] for e, x in enumerate(xs)]

    # ------------------------------------------------------------------ sessions
    def open(self, slot: Optional[int] = None) -> int:
        """claim a slot (the lowest free one when slot is None); its session starts from zero state."""
        if slot is None:
            if not self._free:
                raise RuntimeError(f"the restorer is full: all {self.capacity} slots are open")
            slot = self._free[0]
        slot = int(slot)
        if slot not in self._free:
            raise RuntimeError(f"slot {slot} is not free (capacity {self.capacity})")
        self._free.remove(slot)
        self._reset.add(slot)
        return slot

    def close(self, slot: int) -> None:
        """free the slot; a session opened in it later starts from zero state."""
        slot = int(slot)
        if slot in self._free or not 0 <= slot < self.capacity:
            raise RuntimeError(f"slot {slot} is not open")
        self._reset.discard(slot)
        self._free.append(slot)
        self._free.sort()

    def run(self, chunks: Mapping[int, torch.Tensor], n_quantize: Optional[int] = None) -> Dict[int, torch.Tensor]:
        """the next chunk of each open slot's session, all in one device call -> {slot: restored fp32 chunk (1-D, views of one
        dense output)}.  Integer chunks are mu-law classes of n_quantize levels."""
        slots = [int(s) for s in chunks]
        for s in slots:
            if s in self._free or not 0 <= s < self.capacity:
                raise RuntimeError(f"slot {s} is not open")
        if not slots:
            return {}
        xs = [chunks[s] for s in chunks]
        out = self.run_dense(slots, xs, n_quantize)
        return {s: out[e, :int(torch.as_tensor(x).numel())] for e, (s, x) in enumerate(zip(slots, xs))}

    def run_dense(self, slots: Sequence[int], xs: Sequence[torch.Tensor], n_quantize: Optional[int] = None) -> torch.Tensor:
        """run() for parallel lists -> the dense (E, n_max) fp32 output; row e past len(xs[e]) is not written."""
        resets = [int(s) in self._reset for s in slots]
        out = self._call(self._state, self.capacity, xs, slots, resets, n_quantize)
        self._reset.difference_update(int(s) for s in slots)
        return out
