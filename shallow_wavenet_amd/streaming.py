"""Streaming decode: features arrive a few frames at a time, samples come out as soon as their conditioning is final.

`DecodeStream` wraps the resumable decode of the C ABI (swn_decode_chunk): a session buffer on the device carries the
decode state from one chunk to the next, so the concatenated output of any sequence of chunks is bit-identical to one
`HipNet.decode` over the whole utterance (same kernel variant, noise key, seed waveform and utterance indices).

Conditioning.  conv_aux is two-sided (cswnv_shift1.py:95-127): frame f depends on frames f - la .. f + la, with the
halo la = lookahead_frames(cfg).  After R frames have arrived, frames [0, R - la) are final.  Each push runs the front end
(swn_frontend) on the window [max(0, done - la), R) and keeps only its interior frames [done, R - la): those see exactly
the inputs the one-shot front end sees, so their cond rows are bit-identical.  `finish` ends the features; the front end's
own zero padding on the right then is the one-shot padding, and every remaining frame becomes final.

Pools.  DecodePool.push_many hands a whole tick of sessions their features at once: plan_push turns their frame counts into
the entries of one swn_frontend_pool call, which appends every chunk and writes every new final row in a fixed number of
launches (csrc/swn_frontend_pool.hip), bit-identical to the per-session pushes.

Models.  A deployment holds one checkpoint per target speaker, all of one geometry (run.sh stage 8).  DecodePool.add_model
registers further nets of the pool's NetConfig and open(model=k) binds a session to one of them; a tick whose sessions name
more than one model issues the *_models ops (swn_decode_pool_chunk_models, swn_frontend_pool_models), which take at most 16
models per call - split_models cuts the planned calls accordingly.  A tick over one model issues the single-model ops.
Over bf16 / E4M3 head matrices (weights=...) the pool of several models is DecodeModelPool: its mixed ticks issue
decode_pool_chunk_models_w16 / _w8 with one image per model of the call; a DecodePool of stored weights keeps to one model.
The nets people fine-tune per speaker (REF6) decode on the stepped chain: their multi-voice pool is SteppedModelPool
(swn_decode_pool_stepped_chunk_models), whose launch chain serves the sessions of all models of a call at once - the table is
grouped by model, so a tile of eight sessions fetches ONE model's weight rows.  SteppedDecodePool stays the one-model pool.

Width.  A decode launch of the calls above takes 64 sessions (its table travels in the kernel arguments).  launch_width > 64
on DecodePool / DecodeModelPool makes a tick issue the wide launch instead (swn_decode_pool_chunk_wide: up to 256 sessions, the
table in device memory, every row naming its model and image - so no cut at 16 models), the same bits per session.  push_many,
the post-filter and the stepped pools keep 64.

Steps.  A generation step i reads cond frames up to ((i + 1) * seg - 1) // U, so with F final frames the steps
[0, F * U // seg) can run (the bound of swn_decode).  Step counts come from frame counts on the host: nothing here
waits for the device.

Prologue.  A session of the stepped chain fills its history rings before its first sample: rf - seg + 1 positions, each a
launch per layer.  prologue="parallel" (DecodeStream on variant 3, SteppedDecodePool, SteppedModelPool) fills them with
swn_decode_stepped_prologue instead - all positions of a level in one launch, every float of the session bit-identical - before
the first chunk / at the start of the tick in which the session has its first ready steps.  The default stays "stepped".
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import _lib
from . import ops as _ops          # registers torch.ops.swn.*
from .config import NetConfig

_O = torch.ops.swn

PROLOGUES = ("stepped", "parallel")


def _check_prologue(prologue, stepped: bool) -> str:
    """the `prologue` keyword of the streams and pools: "stepped" | "parallel", the latter on the stepped chain only"""
    if prologue not in PROLOGUES:
        raise ValueError(f"prologue must be one of {PROLOGUES}, not {prologue!r}")
    if prologue == "parallel" and not stepped:
        raise ValueError('prologue="parallel" fills the history rings of the stepped multi-launch decode (variant 3); this '
                         "net and variant resolve to another kernel, whose prologue runs inside its first launch")
    return prologue


def _check_weights(weights, cfg: NetConfig, batch: int, variant: int) -> str:
    """the `weights` keyword of the streams and pools: runtime.check_decode_weights ("fp32" | "bf16" | "e4m3", the latter two where
    (net, batch, variant) resolves to the symmetric BL6 kernel)"""
    from .runtime import check_decode_weights
    return check_decode_weights(weights, cfg, batch, variant)


def _check_launch_width(launch_width, stepped: bool) -> int:
    """the launch_width keyword of the pools: sessions per decode launch, 1 .. 256; above 64 the tick issues the wide launch
    (swn_decode_pool_chunk_wide), which the stepped chain does not have"""
    if not isinstance(launch_width, int) or isinstance(launch_width, bool) or \
            not 1 <= launch_width <= _lib.DECODE_POOL_WIDE_MAX_ENTRIES:
        raise ValueError(f"launch_width must be an integer in 1 .. {_lib.DECODE_POOL_WIDE_MAX_ENTRIES}, not {launch_width!r}")
    if stepped and launch_width > _lib.DECODE_POOL_MAX_ENTRIES:
        raise ValueError(f"launch_width={launch_width}: the stepped decode pools take at most {_lib.DECODE_POOL_MAX_ENTRIES} "
                         "sessions per call - every launch of the chain tiles its sessions by a plan made for 64 entries, and "
                         "the wide launch (one workgroup per session) has no stepped form")
    return launch_width


def lookahead_frames(cfg: NetConfig) -> int:
    """frames of right context conv_aux needs before a frame's conditioning is final: the half-width of the two-sided
    dilated stack, sum over layers of dilation * (k - 1) / 2 = (k ** layers - 1) / 2 for an odd kernel k."""
    k, layers = int(cfg.aux_kernel_size), int(cfg.aux_dilation_size)
    if k % 2 == 0:
        raise ValueError("conv_aux needs an odd kernel size")
    return (k ** layers - 1) // 2


def final_frames(received: int, lookahead: int, finished: bool) -> int:
    """frames whose conditioning is final after `received` frames (all of them once the features have ended)."""
    return received if finished else max(0, received - lookahead)


def ready_steps(cfg: NetConfig, frames_final: int) -> int:
    """generation steps whose conditioning lies inside the first `frames_final` frames."""
    seg = 1 if cfg.kind == "softmax" else int(cfg.seg)
    return frames_final * int(cfg.U) // seg


class DecodeStream:
    """one streamed decode of a batch of `batch` utterances that advance in lockstep.

    net        a HipNet (packed parameters on the device); anything with `cfg`, `packed`, `device` and `dlist`
    variant    decode kernel, as HipNet.decode (0 = auto); it is resolved once and kept for the whole stream
    seed       the seed waveform of batch_fast_generate: laplace (B, seg) fp32 | softmax (B,) classes; None = zeros / Q/2
    rng_seed, rng_utt0, utt_ids   the device generator's key and utterance indices, as HipNet.decode
    want_heads / want_noise       also return the raw out_2 rows / the noise the kernels used, per chunk

    post_filter   a postfilter.NoiseShapingRestorer: the stream claims `batch` of its slots (close() frees them) and
                  restores every chunk on the device (run.sh stage 6)
    prologue      "stepped" (default) | "parallel": on the stepped chain (variant 3), fill the history rings before the first
                  chunk with swn_decode_stepped_prologue - L + 2 launches instead of (rf - seg + 1) x (L + 1), same bits
    weights       "fp32" (default) | "bf16" | "e4m3": the streamed head matrices stored as bf16 / FP8, as HipNet.decode(weights=...) - the
                  chunks then concatenate to that one-shot decode; the symmetric BL6 kernel only (variant=6 for the
                  single-sample Laplace nets), ValueError otherwise

    push / finish / advance return what HipNet.decode returns for the new steps: (out, heads) or, with want_noise,
    (out, heads, noise) - out laplace (B, n * seg) fp32 | softmax (B, n) int32 on the device, heads None unless asked for.
    With a post_filter, one more element follows: the restored chunk, (B, n * seg) fp32 (softmax classes mu-law decoded on
    the device); its concatenation over the chunks is the restore of the whole output.
    With generate=False, push / finish only extend the final conditioning (then `advance` runs steps explicitly: host
    noise and teacher forcing are streamed that way) and return None.
    """

    def __init__(self, net, batch: int, *, variant: int = 0, seed: Optional[torch.Tensor] = None, rng_seed: int = 0,
                 rng_utt0: int = 0, utt_ids: Optional[Sequence[int]] = None, want_heads: bool = False,
                 want_noise: bool = False, post_filter=None, prologue: str = "stepped", weights: str = "fp32"):
        cfg = net.cfg
        if not isinstance(batch, int) or batch < 1:
            raise ValueError(f"batch must be a positive integer, not {batch!r}")
        self.weights = _check_weights(weights, cfg, batch, variant)
        self.net, self.cfg, self.batch = net, cfg, batch
        self.soft = cfg.kind == "softmax"
        self.seg = 1 if self.soft else int(cfg.seg)
        self.width = int(cfg.n_quantize) if self.soft else self.seg
        self.lookahead_frames = lookahead_frames(cfg)
        desc = _ops._desc(net.dlist)
        lib = _lib.lib()
        resolved = lib.swn_decode_resolve_variant(desc, batch, int(variant))
        if resolved < 0:
            raise ValueError(f"decode variant {variant} does not resolve for this net and batch "
                             f"({lib.swn_strerror(resolved).decode()})")
        self.variant = int(variant)
        self.resolved_variant = resolved
        self.prologue = _check_prologue(prologue, resolved == 3)
        self._session_floats = int(lib.swn_decode_session_floats(desc, batch, int(variant)))
        if seed is not None:
            seed = torch.as_tensor(seed)
            if seed.numel() != batch * self.seg:
                raise ValueError(f"seed has {seed.numel()} elements, expected {batch * self.seg}")
        if utt_ids is not None:
            utt_ids = [int(u) for u in utt_ids]
            if len(utt_ids) != batch:
                raise ValueError(f"utt_ids has {len(utt_ids)} entries, expected {batch}")
        self._seed = seed
        self._ids = None if utt_ids is None else torch.tensor(utt_ids, dtype=torch.int32)
        self.rng_seed = int(rng_seed) & 0x7FFFFFFFFFFFFFFF
        self.rng_utt0 = int(rng_utt0) & 0xFFFFFFFF
        self.want_heads, self.want_noise = bool(want_heads), bool(want_noise)
        self.steps_done = 0
        self.frames_received = 0
        self.frames_final = 0
        self.finished = False
        self._begun = False
        self._session = None          # device buffers: allocated on the first push
        self._aux = None              # (B, n_aux, capacity) features received so far
        self._cond = None             # (B, capacity, N) final conditioning rows (zeros beyond frames_final)
        self.post_filter = post_filter
        self._pf_slots = [post_filter.open() for _ in range(batch)] if post_filter is not None else []

    def close(self) -> None:
        """free the post-filter slots of the stream (nothing else to release)."""
        for s in self._pf_slots:
            self.post_filter.close(s)
        self._pf_slots = []

    # ------------------------------------------------------------------ properties
    @property
    def steps_ready(self) -> int:
        return ready_steps(self.cfg, self.frames_final)

    @property
    def cond(self) -> Optional[torch.Tensor]:
        """the final conditioning rows so far, (B, frames_final, N)."""
        return None if self._cond is None else self._cond[:, :self.frames_final]

    # ------------------------------------------------------------------ features
    def _check_aux(self, aux: torch.Tensor) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("the stream is finished: no features can be pushed after finish()")
        if not isinstance(aux, torch.Tensor) or aux.dim() != 3:
            raise ValueError("features must be a (B, n_aux, frames) tensor")
        if aux.shape[0] != self.batch:
            raise ValueError(f"features for {aux.shape[0]} utterances pushed to a stream of batch {self.batch}")
        if aux.shape[1] != self.cfg.n_aux:
            raise ValueError(f"features have {aux.shape[1]} channels, the model expects {self.cfg.n_aux}")
        return aux

    @staticmethod
    def _grow(buf: Optional[torch.Tensor], dim: int, need: int, shape, device) -> torch.Tensor:
        """buffer with at least `need` entries along `dim`, capacity doubled on growth (old contents kept)."""
        cap = 0 if buf is None else buf.shape[dim]
        if cap >= need:
            return buf
        new_cap = max(64, cap)
        while new_cap < need:
            new_cap *= 2
        shp = list(shape)
        shp[dim] = new_cap
        nb = torch.zeros(shp, dtype=torch.float32, device=device)
        if buf is not None:
            nb.narrow(dim, 0, cap).copy_(buf)
        return nb

    def _append(self, aux: torch.Tensor) -> None:
        B, na, f = aux.shape
        if f == 0:
            return
        dev = self.net.device
        self._aux = self._grow(self._aux, 2, self.frames_received + f, (B, na, 0), dev)
        self._aux[:, :, self.frames_received:self.frames_received + f].copy_(aux.to(dev, torch.float32))
        self.frames_received += f

    def _finalise(self, upto: int) -> None:
        """cond rows of frames [frames_final, upto) from the front end over the window they need."""
        if upto <= self.frames_final:
            return
        w0 = max(0, self.frames_final - self.lookahead_frames)
        window = self._aux[:, :, w0:self.frames_received].contiguous()
        cw, _work = _O.frontend(self.net.packed, window, self.net.dlist)
        self._cond = self._grow(self._cond, 1, upto, (self.batch, 0, cw.shape[2]), self.net.device)
        self._cond[:, self.frames_final:upto].copy_(cw[:, self.frames_final - w0:upto - w0])
        self.frames_final = upto

    def push(self, aux_chunk: torch.Tensor, generate: bool = True):
        """append (B, n_aux, f) fp32 features; finalise the conditioning they complete and generate every step it
        allows (possibly none)."""
        self._append(self._check_aux(aux_chunk))
        if self.frames_received > 0:
            self._finalise(final_frames(self.frames_received, self.lookahead_frames, False))
        return self._run_to(self.steps_ready) if generate else None

    def finish(self, aux_tail: Optional[torch.Tensor] = None, generate: bool = True):
        """the features end here (optionally with a last piece): every frame becomes final (zero padding on the right, as
        the one-shot front end pads) and the steps up to frames * U // seg are generated."""
        if aux_tail is not None:
            self._append(self._check_aux(aux_tail))
        elif self.finished:
            raise RuntimeError("the stream is already finished")
        self.finished = True
        if self.frames_received == 0:
            raise RuntimeError("finish() on a stream that received no features")
        self._finalise(self.frames_received)
        return self._run_to(self.steps_ready) if generate else None

    # ------------------------------------------------------------------ steps
    def _run_to(self, target: int):
        return self.advance(max(0, target - self.steps_done))

    def advance(self, n_steps: int, noise: Optional[torch.Tensor] = None, forced: Optional[torch.Tensor] = None):
        """run the next n_steps steps over conditioning that is already final.  noise: the host-drawn stream of these steps,
        laplace (B, n_steps, seg) | softmax (B, n_steps, Q); forced: their teacher-forced inputs, as HipNet.decode."""
        n = int(n_steps)
        if n < 0:
            raise ValueError("n_steps must be >= 0")
        if self.steps_done + n > self.steps_ready:
            raise RuntimeError(f"steps [{self.steps_done}, {self.steps_done + n}) need conditioning beyond the "
                               f"{self.frames_final} final frames (at most {self.steps_ready} steps)")
        if n == 0:
            dev = self.net.device
            out = torch.empty((self.batch, 0), dtype=torch.int32 if self.soft else torch.float32, device=dev)
            heads = torch.empty((self.batch, 0, self.cfg.n_out), dtype=torch.float32, device=dev) if self.want_heads else None
            res = (out, heads)
            if self.want_noise:
                res += (torch.empty((self.batch, 0, self.width), dtype=torch.float32, device=dev),)
            if self.post_filter is not None:
                res += (torch.empty((self.batch, 0), dtype=torch.float32, device=dev),)
            return res
        if self._session is None:
            self._session = torch.empty(self._session_floats, dtype=torch.float32, device=self.net.device)
        # n_frames of the call = the buffer's capacity (the per-utterance stride of the rows); the bound that matters is
        # the one on frames_final checked above - rows past it are zeros that no step of this chunk reads
        begin = not self._begun
        if begin and self.prologue == "parallel":
            _O.decode_stepped_prologue([self.net.packed], [], self._session, [self._cond[b] for b in range(self.batch)],
                                       list(range(self.batch)), self._seed, self.net.dlist, self.batch)
            begin = False                           # the first chunk resumes from the filled session
        args = (self._cond, self._session, noise, forced, self._seed, self.net.dlist, self.steps_done, n, begin, self.variant,
                self.rng_seed, self.rng_utt0, self.want_heads, self.want_noise, self._ids)
        op, lead = _ops.decode_lead(self.net, "decode_chunk", self.weights)
        out, heads, used = getattr(_O, op)(*lead, *args)
        self._begun = True
        self.steps_done += n
        heads = heads if self.want_heads else None
        res = (out, heads, used) if self.want_noise else (out, heads)
        if self.post_filter is not None:
            if not self._pf_slots:
                raise RuntimeError("the stream's post-filter slots were closed")
            res += (self.post_filter.run_dense(self._pf_slots, list(out), self._n_quantize()),)
        return res

    def _n_quantize(self) -> Optional[int]:
        return int(self.cfg.n_quantize) if self.soft else None


# ---------------------------------------------------------------------------------------------------------- decode pool
def plan_tick(sessions: Sequence[Tuple[object, int, int]], max_steps: Optional[int] = None,
              limit: int = _lib.DECODE_POOL_MAX_ENTRIES) -> List[List[Tuple[object, int, int]]]:
    """the launches of one pool tick.  sessions: (key, steps_ready, steps_done) of every open session, in admission order.
    Each session with ready steps runs min(ready - done, max_steps) of them; the entries (key, step0, n_steps) are split
    into launches of at most `limit`.  Pure host arithmetic: nothing here touches a device."""
    if max_steps is not None and int(max_steps) < 1:
        raise ValueError(f"max_steps must be a positive integer or None, not {max_steps!r}")
    entries = []
    for key, ready, done in sessions:
        n = int(ready) - int(done)
        if max_steps is not None:
            n = min(n, int(max_steps))
        if n > 0:
            entries.append((key, int(done), n))
    return [entries[i:i + limit] for i in range(0, len(entries), limit)]


def plan_push(sessions: Sequence[Tuple[object, int, int, int, bool]], lookahead: int,
              limit: int = _lib.FRONTEND_POOL_MAX_ENTRIES) -> List[List[tuple]]:
    """the front end calls of one batched push.  sessions: (key, frames_received, frames_final, n_new, finishing) of every
    session that is handed features or ended, in the caller's order.  Each one's entry (key, n_received_after, f0, f1, final)
    appends its n_new frames and finalises the frames [f0, f1) = [frames_final, final_frames(n_received_after)); sessions with
    neither (an empty chunk) have no entry.  The entries are split into calls of at most `limit`.  Pure host arithmetic:
    nothing here touches a device."""
    lookahead, limit = int(lookahead), int(limit)
    if lookahead < 0:
        raise ValueError(f"lookahead must be >= 0, not {lookahead}")
    if limit < 1:
        raise ValueError(f"limit must be a positive integer, not {limit}")
    entries = []
    for key, received, done, n_new, finishing in sessions:
        received, done, n_new, finishing = int(received), int(done), int(n_new), bool(finishing)
        if received < 0 or n_new < 0:
            raise ValueError(f"session {key!r}: frames_received and n_new must be >= 0")
        if not 0 <= done <= final_frames(received, lookahead, False):
            raise ValueError(f"session {key!r}: {done} final frames do not fit {received} received frames")
        after = received + n_new
        if finishing and after == 0:
            raise ValueError(f"session {key!r} ends without ever having received features")
        f1 = final_frames(after, lookahead, finishing)
        if n_new > 0 or f1 > done:
            entries.append((key, after, done, f1, finishing))
    return [entries[i:i + limit] for i in range(0, len(entries), limit)]


def split_models(calls: Sequence[Sequence[tuple]], model_of: Callable[[object], int],
                 limit: int = _lib.POOL_MAX_MODELS) -> List[List[tuple]]:
    """the calls of plan_tick / plan_push cut so that none names more than `limit` distinct models (SWN_POOL_MAX_MODELS): each
    call is split greedily, in entry order, where the next entry would bring one model too many.  model_of maps an entry's key
    (its first element) to its model.  Entries keep their order, and a call that is within the limit comes back as it was.
    Pure host arithmetic: nothing here touches a device."""
    limit = int(limit)
    if limit < 1:
        raise ValueError(f"limit must be a positive integer, not {limit}")
    out: List[List[tuple]] = []
    for entries in calls:
        parts, cur, seen = [], [], set()
        for en in entries:
            m = model_of(en[0])
            if m not in seen and len(seen) == limit:
                parts.append(cur)
                cur, seen = [], set()
            seen.add(m)
            cur.append(en)
        parts.append(cur)
        out.extend(parts if len(parts) > 1 else [entries])
    return out


def _local_models(models: Sequence[int]) -> Tuple[List[int], List[int]]:
    """the distinct models of a call in order of first appearance, and every entry's index into that list"""
    distinct: List[int] = []
    at: dict = {}
    for m in models:
        if m not in at:
            at[m] = len(distinct)
            distinct.append(m)
    return distinct, [at[m] for m in models]


class PoolSession:
    """one utterance of a DecodePool.  push / finish hand it features (they only finalise conditioning: the pool's ticks
    generate); steps_ready / steps_done / finished tell where it stands.  Made by DecodePool.open."""

    def __init__(self, pool: "DecodePool", slot: int, utt_id: int, seed: Optional[torch.Tensor], model: int = 0):
        self._pool = pool
        self.slot, self.utt_id, self.model = slot, utt_id, model
        # the conditioning of a batch-1 DecodeStream over the session's model: the pool reads its _cond, steps_ready and
        # steps_done
        self._stream = DecodeStream(pool._models[model], 1, variant=pool.variant, seed=seed, rng_seed=pool.rng_seed, utt_ids=[utt_id],
                                    weights=getattr(pool, "weights", "fp32"))
        self._seed = self._stream._seed
        self.closed = False
        self._pf_slot = pool.post_filter.open() if pool.post_filter is not None else None

    def _check(self) -> None:
        if self.closed:
            raise RuntimeError(f"pool session {self.utt_id} (slot {self.slot}) is closed")

    def push(self, aux_chunk: torch.Tensor) -> None:
        """append (1, n_aux, f) fp32 features."""
        self._check()
        self._stream.push(aux_chunk, generate=False)

    def finish(self, aux_tail: Optional[torch.Tensor] = None) -> None:
        """the features end here (optionally with a last piece)."""
        self._check()
        self._stream.finish(aux_tail, generate=False)

    @property
    def steps_ready(self) -> int:
        return self._stream.steps_ready

    @property
    def steps_done(self) -> int:
        return self._stream.steps_done

    @property
    def finished(self) -> bool:
        """no more features will come."""
        return self._stream.finished

    @property
    def done(self) -> bool:
        """finished and every step generated."""
        return self._stream.finished and self.steps_done == self.steps_ready


class DecodePool:
    """many independent streamed decodes advanced together: one kernel launch per tick (per 64 active sessions) instead of
    one per session (swn_decode_pool_chunk).  Sessions arrive, receive features at their own rate and end at their own
    length; each one's output is bit-identical to HipNet.decode of that utterance alone (batch 1, the same variant, rng_seed,
    utterance id and seed waveform), whatever else shares its launches.

    net        a HipNet;  capacity  session slots (sessions open at once)
    variant    decode kernel as HipNet.decode; the stepped multi-launch decode (variant 3, and what 0 picks for REF6-class
               nets) cannot serve a pool - variant 1 runs those nets on the generic kernel
    rng_seed   the device generator's key (pools draw their noise on the device)
    want_heads / want_noise   also return the raw out_2 rows / the noise used
    post_filter   a postfilter.NoiseShapingRestorer: every session holds one of its slots, and each tick ends with one
               post-filter call over the sessions that ran; each result then ends with the restored chunk (1, n * seg) fp32
    weights    "fp32" (default) | "bf16" | "e4m3": the streamed head matrices stored as bf16 (swn_decode_pool_chunk_w16) or FP8
               E4M3 (swn_decode_pool_chunk_w8), each session bit-identical to its solo DecodeStream of that mode.  Symmetric BL6
               kernel only (variant=6 for the single-sample Laplace nets); such a DecodePool serves one model (add_model raises:
               DecodeModelPool is the pool of several models over stored weights) and no stepped pool has the modes
    launch_width   sessions per decode launch, 1 .. 256 (default 64).  Up to 64 a tick issues swn_decode_pool_chunk and its
               forms, whose entry table travels in the kernel arguments.  Above 64 it issues the wide launch
               (swn_decode_pool_chunk_wide: the table in device memory, one workgroup per session, every session's bits
               unchanged) once per launch_width sessions, for any number of models.  The batched features, the post-filter
               and the log-mel pool keep their groups of 64

        k = pool.add_model(other_net)           # another net of the same NetConfig (the pool's own net is model 0)
        s = pool.open(seed=None, utt_id=None, model=0)   # a free slot; utt_id defaults to the admission counter
        s.push(aux_piece); s.finish(aux_tail)  # (1, n_aux, f) features
        pool.push_many({s: aux_piece, ...}, finish=[...])   # the same for every session of a tick in ONE front end call
        results = pool.step(max_steps=None)    # one tick -> {session: (out, heads[, noise])}, views of the launch outputs
        pool.close(s)                          # frees the slot, finished or not
    """

    _stored_models = False        # add_model on a pool of stored weights: DecodeModelPool's

    def __init__(self, net, capacity: int, *, variant: int = 0, rng_seed: int = 0, want_heads: bool = False,
                 want_noise: bool = False, post_filter=None, weights: str = "fp32", launch_width: int = 64):
        if not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer, not {capacity!r}")
        self.launch_width = _check_launch_width(launch_width, False)
        self.net, self.cfg, self.capacity = net, net.cfg, capacity
        self.weights = _check_weights(weights, net.cfg, capacity, variant)
        self.soft = self.cfg.kind == "softmax"
        self.seg = 1 if self.soft else int(self.cfg.seg)
        desc = _ops._desc(net.dlist)
        lib = _lib.lib()
        resolved = lib.swn_decode_resolve_variant(desc, capacity, int(variant))
        if resolved < 0:
            raise ValueError(f"decode variant {variant} does not resolve for this net ({lib.swn_strerror(resolved).decode()})")
        if resolved == 3:
            raise ValueError(f"decode variant {variant} resolves to the stepped multi-launch decode, which cannot serve a "
                             "pool; variant=1 runs this net on the generic kernel")
        self.variant, self.resolved_variant = int(variant), resolved
        self.rng_seed = int(rng_seed) & 0x7FFFFFFFFFFFFFFF
        self.want_heads, self.want_noise = bool(want_heads), bool(want_noise)
        self._session = torch.empty(int(lib.swn_decode_session_floats(desc, capacity, int(variant))), dtype=torch.float32,
                                    device=net.device)
        self.post_filter = post_filter
        self._models = [net]                        # model 0 is the pool's own net
        self._free = list(range(capacity))          # free slots, lowest first
        self._open: dict = {}                       # slot -> PoolSession, in admission order
        self.admitted = 0

    @property
    def sessions(self) -> List[PoolSession]:
        return list(self._open.values())

    def add_model(self, net) -> int:
        """register another net of the pool's geometry (a voice fine-tuned from the same recipe) -> its model index for
        open(model=...).  A session slot's layout depends on the geometry only, so sessions of all models share the pool's
        slots and launches.  The pool may hold any number of models; the nets' packed buffers are read at call time."""
        if self.weights != "fp32" and not self._stored_models:
            raise ValueError(f'add_model: a weights="{self.weights}" DecodePool serves one model - DecodeModelPool serves '
                             f"several models over {self.weights} weights")
        if net.cfg != self.cfg:
            raise ValueError("add_model: the net's NetConfig differs from the pool's - the models of a pool share one geometry")
        if torch.device(net.device) != torch.device(self.net.device):
            raise ValueError(f"add_model: the net lives on {net.device}, the pool on {self.net.device}")
        self._models.append(net)
        return len(self._models) - 1

    def open(self, seed: Optional[torch.Tensor] = None, utt_id: Optional[int] = None, model: int = 0) -> PoolSession:
        """claim a free slot for a new utterance of model `model` (its generator index is utt_id, else the admission
        count)."""
        if not self._free:
            raise RuntimeError(f"the pool is full: all {self.capacity} slots hold open sessions")
        if not isinstance(model, int) or not 0 <= model < len(self._models):
            raise ValueError(f"model must be an index in [0, {len(self._models)}), not {model!r}")
        uid = self.admitted if utt_id is None else int(utt_id)
        slot = self._free[0]
        s = PoolSession(self, slot, uid, seed, model)
        self._free.pop(0)
        self._open[slot] = s
        self.admitted += 1
        return s

    def close(self, s: PoolSession) -> None:
        """free the session's slot (finished or not); a new session may begin in it at the next tick."""
        if s.closed or self._open.get(s.slot) is not s:
            raise RuntimeError("this session is not open in this pool")
        s.closed = True
        del self._open[s.slot]
        if s._pf_slot is not None:
            self.post_filter.close(s._pf_slot)
        self._free.append(s.slot)
        self._free.sort()

    def step(self, max_steps: Optional[int] = None) -> dict:
        """one tick: every open session with ready steps advances by min(ready, max_steps) of them, in launches of at most
        launch_width sessions.  Returns {session: (out, heads) or (out, heads, noise)} for the sessions that ran - out laplace
        (1, n * seg) fp32 | softmax (1, n) int32, heads (1, n, n_out) or None, noise (1, n, width) - views of the dense
        launch outputs.  Nothing here waits for the device."""
        launches = plan_tick([(s, s.steps_ready, s.steps_done) for s in self._open.values()], max_steps, self.launch_width)
        wide = self.launch_width > _lib.DECODE_POOL_MAX_ENTRIES   # the rows of a wide launch name each entry's model themselves
        several = len(self._models) > 1             # a pool of one model pays nothing for the others
        if several and not wide:
            launches = split_models(launches, lambda s: s.model)
        results = {}
        for entries in launches:
            sess = [e[0] for e in entries]
            begins = [not s._stream._begun for s in sess]
            seeds = None
            if any(b and s._seed is not None for s, b in zip(sess, begins)):
                seeds = torch.stack([s._seed.reshape(-1).to(torch.int32 if self.soft else torch.float32).cpu()
                                     if s._seed is not None else self._default_seed() for s in sess])
            models, of = _local_models([s.model for s in sess]) if several else ([0], None)
            args = (self._session, [s._stream._cond[0] for s in sess], [s.slot for s in sess],
                    [e[1] for e in entries], [e[2] for e in entries], begins, seeds, [s.utt_id for s in sess],
                    self.net.dlist, self.capacity, self.variant, self.rng_seed, self.want_heads, self.want_noise)
            if wide:
                lead = _ops.decode_wide_lead([self._models[m] for m in models], self.weights)
                out, heads, used = _O.decode_pool_chunk_wide(*lead, of if several else [0] * len(sess), *args)
            elif len(models) == 1:
                op, lead = _ops.decode_lead(self._models[models[0]], "decode_pool_chunk", self.weights)
                out, heads, used = getattr(_O, op)(*lead, *args)
            else:                                   # (stored weights: a DecodeModelPool - one image per model of the call)
                op, lead = _ops.decode_models_lead([self._models[m] for m in models], "decode_pool_chunk_models", self.weights)
                out, heads, used = getattr(_O, op)(*lead, of, *args)
            for e, (s, step0, n) in enumerate(entries):
                s._stream.steps_done = step0 + n
                s._stream._begun = True
                o = out[e:e + 1, :n * self.seg]
                h = heads[e:e + 1, :n] if self.want_heads else None
                results[s] = (o, h, used[e:e + 1, :n]) if self.want_noise else (o, h)
        return self._post_filter(results)

    # ------------------------------------------------------------------ batched features
    def _check_push_many(self, chunks, finish) -> List[Tuple["PoolSession", Optional[torch.Tensor], bool]]:
        """(session, chunk or None, finishing) of a push_many call in its order, or the error the separate calls would raise;
        nothing is changed."""
        if not isinstance(chunks, dict):
            raise ValueError("chunks must map pool sessions to (1, n_aux, f) feature tensors")
        finish = list(finish)
        if len(set(map(id, finish))) != len(finish):
            raise ValueError("a session is named twice in finish")
        ending = set(map(id, finish))
        order = [(s, c, id(s) in ending) for s, c in chunks.items()] + [(s, None, True) for s in finish if s not in chunks]
        for s, c, fin in order:
            if not isinstance(s, PoolSession) or s.closed or self._open.get(s.slot) is not s:
                if isinstance(s, PoolSession) and s._pool is self and s.closed:
                    raise RuntimeError(f"pool session {s.utt_id} (slot {s.slot}) is closed")
                raise RuntimeError("this session is not open in this pool")
            st = s._stream
            if st.finished:
                raise RuntimeError(f"pool session {s.utt_id} is finished: no features can be pushed after finish()")
            if c is not None:
                if not isinstance(c, torch.Tensor) or c.dim() != 3:
                    raise ValueError("features must be a (1, n_aux, frames) tensor")
                if c.shape[0] != 1:
                    raise ValueError(f"features for {c.shape[0]} utterances pushed to a pool session (batch 1)")
                if c.shape[1] != self.cfg.n_aux:
                    raise ValueError(f"features have {c.shape[1]} channels, the model expects {self.cfg.n_aux}")
            if fin and st.frames_received + (0 if c is None else c.shape[2]) == 0:
                raise RuntimeError(f"pool session {s.utt_id} is named in finish but never received features")
        return order

    def _stage(self, pieces: List[torch.Tensor]) -> Optional[torch.Tensor]:
        """the chunks of one call, flattened and concatenated in entry order, on the device: one host-to-device copy for the
        host chunks, one cat for the device chunks."""
        if not pieces:
            return None
        dev = self.net.device
        flat = [c.reshape(-1) if c.dtype == torch.float32 else c.reshape(-1).to(torch.float32) for c in pieces]
        host = [i for i, c in enumerate(flat) if not c.is_cuda]
        if host:
            up = (flat[host[0]] if len(host) == 1 else torch.cat([flat[i] for i in host])).to(dev)
            if len(host) == len(flat):
                return up
            at = 0
            for i in host:
                n = flat[i].numel()
                flat[i] = up[at:at + n]
                at += n
        return flat[0].contiguous() if len(flat) == 1 else torch.cat(flat)

    def push_many(self, chunks: dict, finish: Sequence[PoolSession] = ()) -> None:
        """one front end call for a whole tick of features: s.push(chunk) for every session of `chunks` ({session: (1, n_aux, f)
        features on the host or the device, f >= 0}) and s.finish(chunk or None) for every session of `finish` (which may also
        have a last chunk in `chunks`), with the same counters and bit-identical cond rows afterwards.  The chunks are staged
        with one copy and finalised by one swn_frontend_pool call per 64 sessions (swn_frontend_pool_models where they name
        several models, per 16 of those), which appends them to the sessions' feature
        buffers and writes the cond rows where the decode reads them.  Everything is checked first, and the counters move only
        after every call is enqueued: a call that raises leaves every session's frames_received, frames_final, steps_ready,
        finished and cond rows [0, frames_final) as they were.  Its _aux and _cond buffers may already have been grown
        (new objects, old contents kept) and frames appended past frames_received, where the next push overwrites them."""
        order = self._check_push_many(chunks, finish)
        la = lookahead_frames(self.cfg)
        calls = plan_push([(i, s._stream.frames_received, s._stream.frames_final, 0 if c is None else c.shape[2], fin)
                           for i, (s, c, fin) in enumerate(order)], la)
        several = len(self._models) > 1
        if several:
            calls = split_models(calls, lambda i: order[i][0].model)
        dev = self.net.device
        for entries in calls:
            auxs, conds, pieces = [], [], []
            for i, after, f0, f1, _fin in entries:
                s, c, _ = order[i]
                st = s._stream
                if after > st.frames_received:
                    st._aux = st._grow(st._aux, 2, after, (1, self.cfg.n_aux, 0), dev)
                    pieces.append(c)
                if f1 > f0:
                    st._cond = st._grow(st._cond, 1, f1, (1, 0, self._cond_width()), dev)
                auxs.append(st._aux[0])
                # nothing final yet (the session only appends): the call still wants a row pointer of its own
                conds.append(st._cond[0] if st._cond is not None else self._spare_cond(len(conds)))
            models, of = _local_models([order[e[0]][0].model for e in entries]) if several else ([0], None)
            args = (auxs, conds, self._stage(pieces),
                    [e[1] - order[e[0]][0]._stream.frames_received for e in entries], [e[1] for e in entries],
                    [e[2] for e in entries], [e[3] for e in entries], [e[4] for e in entries], self.net.dlist)
            if len(models) == 1:
                _O.frontend_pool(self._models[models[0]].packed, *args)
            else:
                _O.frontend_pool_models([self._models[m].packed for m in models], of, *args)
        # every call has been enqueued: only now do the sessions move (a call that raised left the counters as they were)
        for entries in calls:
            for i, after, _f0, f1, _fin in entries:
                st = order[i][0]._stream
                st.frames_received, st.frames_final = after, f1
        for s, _c, fin in order:
            if fin:
                s._stream.finished = True

    def _spare_cond(self, e: int) -> torch.Tensor:
        if getattr(self, "_spare", None) is None:
            self._spare = torch.zeros((_lib.FRONTEND_POOL_MAX_ENTRIES, self._cond_width()), dtype=torch.float32,
                                      device=self.net.device)
        return self._spare[e:e + 1]

    def _cond_width(self) -> int:
        n = getattr(self, "_n_cond", None)
        if n is None:
            n = self._n_cond = int(_lib.lib().swn_cond_floats(_ops._desc(self.net.dlist), 1, 1))
        return n

    def _post_filter(self, results: dict) -> dict:
        """with a post_filter: one call restores the outputs of every session of the tick, each result gains its row."""
        if self.post_filter is None or not results:
            return results
        sess = list(results)
        restored = self.post_filter.run_dense([s._pf_slot for s in sess], [results[s][0][0] for s in sess],
                                              int(self.cfg.n_quantize) if self.soft else None)
        return {s: results[s] + (restored[e:e + 1, :results[s][0].shape[1]],) for e, s in enumerate(sess)}

    def _default_seed(self) -> torch.Tensor:
        if self.soft:
            return torch.full((1,), int(self.cfg.n_quantize) // 2, dtype=torch.int32)
        return torch.zeros(self.seg, dtype=torch.float32)


class DecodeModelPool(DecodePool):
    """a decode pool of any `weights` whose sessions may each run a different model of the pool's geometry - one checkpoint per
    target speaker - in the SAME launch, also over bf16 / E4M3 head matrices (swn_decode_pool_chunk_models_w16 / _w8): the
    workgroup of a session reads its model's packed parameters and its model's image, so each session's output is bit-identical
    to its solo DecodeStream(model, 1, weights=...) whatever shares its launch.  add_model / open(model=k) and everything else
    as DecodePool; with weights="fp32" it is DecodePool.  A tick whose sessions name several models issues
    decode_pool_chunk_models_<suffix> with the packed buffers and decode_<suffix>_image() of the launch's models, both read at
    call time (a repacked net brings its new image), in calls cut at 16 models (split_models); a tick over one model issues the
    single-model op with that model, so a pool that never mixes pays nothing.  push_many / PoolSession.push are DecodePool's:
    the front end has no stored format."""

    _stored_models = True


# -------------------------------------------------------------------------------------------------- stepped decode pool
def plan_stepped_tick(sessions: Sequence[Tuple[object, int, int]], n_pro: int, max_steps: Optional[int] = None,
                      max_prologue: Optional[int] = None,
                      limit: int = _lib.DECODE_POOL_MAX_ENTRIES) -> List[List[Tuple[object, int, int]]]:
    """the calls of one stepped-pool tick.  sessions: (key, steps_ready, iterations_done) of every open session, in
    admission order; n_pro: prologue iterations of the net (swn_decode_stepped_prologue_iterations).  A session with ready
    steps (its first frame is final: the prologue reads it) runs the rest of its prologue, at most max_prologue iterations
    of it, and - once the prologue is complete - min(ready - done, max_steps) generation steps.  Entries (key, it0, n_it) are
    split into calls of at most `limit`.  Pure host arithmetic: nothing here touches a device."""
    if max_steps is not None and int(max_steps) < 1:
        raise ValueError(f"max_steps must be a positive integer or None, not {max_steps!r}")
    if max_prologue is not None and int(max_prologue) < 1:
        raise ValueError(f"max_prologue must be a positive integer or None, not {max_prologue!r}")
    n_pro = int(n_pro)
    entries = []
    for key, ready, it_done in sessions:
        ready, it_done = int(ready), int(it_done)
        if ready <= 0:
            continue                                   # waiting for features
        p = max(0, n_pro - it_done)
        if max_prologue is not None:
            p = min(p, int(max_prologue))
        g = 0
        if it_done + p >= n_pro:
            g = ready - max(0, it_done - n_pro)
            if max_steps is not None:
                g = min(g, int(max_steps))
        if p + g > 0:
            entries.append((key, it_done, p + g))
    return [entries[i:i + limit] for i in range(0, len(entries), limit)]


class SteppedDecodePool(DecodePool):
    """the decode pool of the stepped multi-launch decode (variant 3: what REF6-class nets resolve to;
    swn_decode_pool_stepped_chunk).  Every launch of the chain serves all sessions of a call, each at its own iteration, so a
    tick costs about one session's chunk; each session's output is bit-identical to HipNet.decode of that utterance alone
    with variant=3 (same rng_seed, utterance id and seed waveform).  Same interface and results as DecodePool; in addition,
    step(max_prologue=n) spreads a new session's prologue (rf - seg + 1 iterations, each a launch per layer) over ticks of at
    most n iterations, so the sessions already generating do not wait for all of it in one tick.  A session that only
    advanced its prologue in a tick has no result for it.
    prologue="parallel": a tick first fills the history rings of the sessions that begin in it with one
    swn_decode_stepped_prologue call per 64 of them (L + 2 launches, whatever their number), so they generate in the same tick
    and max_prologue has nothing left to spread; same bits as the default "stepped"."""

    def __init__(self, net, capacity: int, *, rng_seed: int = 0, want_heads: bool = False, want_noise: bool = False,
                 post_filter=None, prologue: str = "stepped", weights: str = "fp32", launch_width: int = 64):
        if not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer, not {capacity!r}")
        _check_launch_width(launch_width, True)     # (validated only: the stepped pools keep their calls of 64)
        self.launch_width = _lib.DECODE_POOL_MAX_ENTRIES
        from .runtime import DECODE_WEIGHTS
        if weights not in DECODE_WEIGHTS:
            raise ValueError(f"weights must be one of {DECODE_WEIGHTS}, not {weights!r}")
        if weights != "fp32":
            raise ValueError(f'weights="{weights}" is not served by the stepped decode pools: the chain is launch-bound, weight bytes '
                             "are not its limit")
        self.weights = "fp32"
        self.net, self.cfg, self.capacity = net, net.cfg, capacity
        self.soft = self.cfg.kind == "softmax"
        self.seg = 1 if self.soft else int(self.cfg.seg)
        desc = _ops._desc(net.dlist)
        lib = _lib.lib()
        floats = self._session_floats(desc)
        if floats == 0:
            raise ValueError(f"the stepped decode does not run this net with {capacity} slots "
                             f"({lib.swn_strerror(lib.swn_decode_resolve_variant(desc, capacity, 3)).decode()})")
        self.variant = self.resolved_variant = 3
        self.prologue = _check_prologue(prologue, True)
        self.n_pro = int(lib.swn_decode_stepped_prologue_iterations(desc))
        self.rng_seed = int(rng_seed) & 0x7FFFFFFFFFFFFFFF
        self.want_heads, self.want_noise = bool(want_heads), bool(want_noise)
        self._session = torch.empty(floats, dtype=torch.float32, device=net.device)
        self.post_filter = post_filter
        self._models = [net]
        self._free = list(range(capacity))
        self._open: dict = {}
        self.admitted = 0

    def add_model(self, net) -> int:
        raise ValueError("a stepped decode pool serves one model: the chain's tile kernels fetch a channel pair's weight rows "
                         "once for eight sessions, so the sessions of a call cannot run different weights - SteppedModelPool "
                         "groups a call's sessions by model and serves several")

    def open(self, seed: Optional[torch.Tensor] = None, utt_id: Optional[int] = None) -> PoolSession:
        s = super().open(seed, utt_id)
        s._it_done = 0                               # iterations run: prologue positions, then generation steps
        return s

    def _session_floats(self, desc) -> int:
        return _ops.stepped_pool_session_floats(desc, self.capacity)

    def _calls(self, calls):
        """the calls of a tick as (entries, models of the call, each entry's index into them)"""
        return [(entries, [0], None) for entries in calls]

    def step(self, max_steps: Optional[int] = None, max_prologue: Optional[int] = None) -> dict:
        """one tick: every open session with ready steps runs the rest of its prologue (at most max_prologue iterations of
        it) and then up to min(ready, max_steps) steps, in calls of at most 64 sessions.  Returns {session: (out, heads) or
        (out, heads, noise)} for the sessions that generated, as DecodePool.step.  Nothing here waits for the device."""
        if self.prologue == "parallel":
            self._fill_prologues()
        calls = plan_stepped_tick([(s, s.steps_ready, s._it_done) for s in self._open.values()], self.n_pro, max_steps,
                                  max_prologue)
        results = {}
        for entries, models, of in self._calls(calls):
            sess = [e[0] for e in entries]
            begins = [s._it_done == 0 for s in sess]
            seeds = self._seeds_of(sess, begins)
            args = (self._session, [s._stream._cond[0] for s in sess], [s.slot for s in sess],
                    [e[1] for e in entries], [e[2] for e in entries], begins, seeds, [s.utt_id for s in sess],
                    self.net.dlist, self.capacity, self.rng_seed, self.want_heads, self.want_noise)
            if len(models) == 1:
                out, heads, used = _O.decode_pool_stepped_chunk(self._models[models[0]].packed, *args)
            else:
                out, heads, used = _O.decode_pool_stepped_chunk_models([self._models[m].packed for m in models], of, *args)
            for e, (s, it0, n_it) in enumerate(entries):
                s._it_done = it0 + n_it
                s._stream._begun = True
                n = max(0, it0 + n_it - max(it0, self.n_pro))
                s._stream.steps_done = max(0, s._it_done - self.n_pro)
                if n == 0:
                    continue
                o = out[e:e + 1, :n * self.seg]
                h = heads[e:e + 1, :n] if self.want_heads else None
                results[s] = (o, h, used[e:e + 1, :n]) if self.want_noise else (o, h)
        return self._post_filter(results)


    def _seeds_of(self, sess, begins) -> Optional[torch.Tensor]:
        """the seed rows of a call, one per entry, when a beginning session brought a seed waveform; else None"""
        if not any(b and s._seed is not None for s, b in zip(sess, begins)):
            return None
        return torch.stack([s._seed.reshape(-1).to(torch.int32 if self.soft else torch.float32).cpu()
                            if s._seed is not None else self._default_seed() for s in sess])

    def _fill_prologues(self) -> None:
        """prologue="parallel": the sessions that begin in this tick (nothing run yet, steps ready: their first frame is
        final) get their history rings filled by one swn_decode_stepped_prologue call per 64 of them, cut at 16 models, and
        stand at iteration n_pro afterwards - the tick then plans generation entries only."""
        new = [(s,) for s in self._open.values() if s._it_done == 0 and s.steps_ready > 0]
        limit = _lib.DECODE_POOL_MAX_ENTRIES
        calls = [new[i:i + limit] for i in range(0, len(new), limit)]
        if len(self._models) > 1:
            calls = split_models(calls, lambda s: s.model)
        for entries in calls:
            sess = [e[0] for e in entries]
            models, of = _local_models([s.model for s in sess])
            _O.decode_stepped_prologue([self._models[m].packed for m in models], of, self._session,
                                       [s._stream._cond[0] for s in sess], [s.slot for s in sess],
                                       self._seeds_of(sess, [True] * len(sess)), self.net.dlist, self.capacity)
            for s in sess:
                s._it_done = self.n_pro
                s._stream._begun = True


class SteppedModelPool(SteppedDecodePool):
    """a stepped decode pool whose sessions may each run a different model of the pool's geometry - one checkpoint per target
    speaker of the REF6 recipe - in the SAME launch chain (swn_decode_pool_stepped_chunk_models): a tick over sessions of M
    models makes the launches a one-model tick makes, not M chains.  add_model / open(model=k) as DecodePool; everything else
    as SteppedDecodePool, and each session's output is bit-identical to HipNet.decode(variant=3) of that utterance alone on its
    own model.  A tick whose sessions name one model issues the single-model op with that model's packed buffer, so a pool
    that never mixes models pays nothing; calls are cut at 16 models (split_models).  The session buffer is that of
    SteppedDecodePool with a wider table tail (ops.stepped_pool_models_session_floats)."""

    def add_model(self, net) -> int:
        return DecodePool.add_model(self, net)

    def open(self, seed: Optional[torch.Tensor] = None, utt_id: Optional[int] = None, model: int = 0) -> PoolSession:
        s = DecodePool.open(self, seed, utt_id, model)
        s._it_done = 0
        return s

    def _session_floats(self, desc) -> int:
        return _ops.stepped_pool_models_session_floats(desc, self.capacity)

    def _calls(self, calls):
        if len(self._models) == 1:
            return super()._calls(calls)
        return [(entries,) + _local_models([e[0].model for e in entries])
                for entries in split_models(calls, lambda s: s.model)]
