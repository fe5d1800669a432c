/*
 * swn_hip.h  --  C ABI of the MI355X (gfx950) shallow-WaveNet hot path.
 *
 * The reference (patrickltobing/shallow-wavenet) has no native code and no FFI: its hot
 * path is the PyTorch module code of src/nets/{cswnv_shift1,dswnv}.py.  This header is the
 * boundary a maintainer would bind from those modules (see INTEGRATION.md for the ctypes
 * stub); every entry point cites the reference lines it replaces.
 *
 * Conventions
 *   - plain C: pointers, sizes, a POD descriptor; no torch / C++ types.
 *   - `*_dev` pointers are device (HBM) addresses, `*_host` pointers host addresses.
 *   - all tensors fp32, contiguous, channels-first (B, C, T) exactly as the reference
 *     holds them; integer data (mu-law indices) are int32 on the device.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream). Launches are
 *     asynchronous; nothing in here synchronises, allocates or frees device memory.
 *   - every function returns 0 on success or a negative SWN_E_* code;
 *     swn_strerror() maps it to text.  No global mutable state (the arithmetic mode of the training
 *     entry points is an argument of each call, SWN_PRECISION_*); nothing reads the environment.
 */
#ifndef SWN_HIP_H
#define SWN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWN_ABI_VERSION 3   /* 3: `precision` argument instead of a process-wide switch; swn_decode_io.rng_utt_ids_dev;
                             *    decode variants 4 / 5 (cohort, cluster) retired */

/* arithmetic of the training contractions, an argument of every entry point it applies to
 *   FP32: fp32 operands on the matrix cores (v_mfma_f32_16x16x4_f32), bit-compatible with an fmaf chain - the parity
 *         mode every gradient fixture is checked in;
 *   BF16: mixed precision - the same fp32 tensors in HBM, operands rounded to bf16 on their way into LDS,
 *         v_mfma_f32_16x16x32_bf16 with fp32 accumulation (what torch.autocast(bfloat16) would do to the reference's
 *         conv forward / backward); gradients agree with FP32 to ~1e-2 relative per tensor.
 * A forward and the backward that reads its work buffer must be given the same value (the BF16 dropout forward keeps
 * gate pre-activations in the work buffer that the FP32 one does not). */
#define SWN_PRECISION_FP32 0
#define SWN_PRECISION_BF16 1

#define SWN_KIND_LAPLACE 0   /* CSWNV, cswnv_shift1.py:130 */
#define SWN_KIND_SOFTMAX 1   /* DSWNV, dswnv.py:190       */

#define SWN_OK            0
#define SWN_E_BADDESC    -1  /* descriptor outside what the kernels support            */
#define SWN_E_BADARG     -2  /* null pointer / size mismatch                           */
#define SWN_E_LAUNCH     -3  /* HIP reported a launch error (hipGetLastError)          */
#define SWN_E_UNSUPPORTED -4 /* valid reference configuration not built yet            */
#define SWN_E_NODEVICE   -5

/* Constructor arguments of CSWNV / DSWNV (cswnv_shift1.py:131-133, dswnv.py:191-193). */
typedef struct swn_net_desc {
    int32_t kind;              /* SWN_KIND_*                                  */
    int32_t n_aux;
    int32_t hid_chn;
    int32_t skip_chn;
    int32_t aux_kernel_size;
    int32_t aux_dilation_size;
    int32_t dilation_depth;
    int32_t dilation_repeat;
    int32_t kernel_size;
    int32_t upsampling_factor;
    int32_t seg;               /* laplace only, 1 for softmax                 */
    int32_t lpc;               /* laplace only                                */
    int32_t n_quantize;        /* softmax only                                */
    int32_t wav_conv_flag;
    int32_t audio_in_flag;     /* softmax only                                */
    int32_t aux_conv2d_flag;   /* laplace only; the (seg,1) Conv2d is folded into in_x at pack time */
} swn_net_desc;

/* ---- introspection --------------------------------------------------------------- */
int         swn_abi_version(void);
const char* swn_strerror(int code);
/* text of the last HIP runtime failure seen by an entry point on this thread ("" if none) */
const char* swn_last_error_detail(void);
/* number of HIP devices visible, or a negative SWN_E_* */
int         swn_device_count(void);
/* receptive field / number of state_dict tensors, as CSWNV.__init__ computes them
 * (cswnv_shift1.py:170-183).  Negative on a bad descriptor. */
int         swn_receptive_field(const swn_net_desc* d);
int         swn_num_tensors(const swn_net_desc* d);

/* ---- parameter packing (host side) ---------------------------------------------------
 * Re-lays the reference state_dict (tensors given in state_dict order, fp32 host pointers,
 * reference shapes: SURVEY.md 8b) into one flat fp32 buffer the kernels stream from:
 * tap-major dilated-conv rows, fused wav_conv+causal taps, the skip 1x1s concatenated, the
 * in_x 1x1s stacked for the frame-rate GEMM, summed biases.  The packed buffer is what is
 * uploaded once and broadcast over RCCL (decode_cswnv_laplace-shift1.py:223-224 loads the
 * checkpoint per process instead). */
size_t swn_packed_floats(const swn_net_desc* d);
/* float offsets of the packed sections in the order scale_w, scale_b, aux_w[0..3], aux_b[0..3], wx, wxa, wup,
 * bup, bx, cb, cv, cc, ct, wd, bd, wsk, bsk, w1, b1, w2, b2, total, bxr (csrc/swn_geom.hpp::SwnLayout); returns
 * the number written (29) or a negative SWN_E_*.  Used to unfold swn_backward's packed gradients. */
int    swn_layout_offsets(const swn_net_desc* d, size_t* out, int n);
int    swn_pack_params(const swn_net_desc* d, const float* const* tensors_host, int n_tensors,
                       float* packed_host, size_t packed_floats);
/* The same re-layout on the device, for parameters that already live in HBM (a training step ends with
 * optimizer.step(), train_cswnv_laplace-stftcmplx_shift1.py:872-874, after which every packed section is stale):
 *   tensors_dev  HOST array of n_tensors DEVICE pointers (state_dict order, fp32, contiguous, reference shapes)
 *   packed_dev   swn_packed_floats() floats, overwritten (padding zeroed); bit-identical to swn_pack_params      */
int    swn_pack_params_device(const swn_net_desc* d, const float* const* tensors_dev, int n_tensors,
                              float* packed_dev, size_t packed_floats, void* stream);
/* The way back for a training step: gradients in the packed layout (swn_backward*) -> the gradient of every parameter
 * tensor in the reference's shapes, i.e. the chain rule through the pack-time folds, in one launch
 * (csrc/swn_unfold_dev.hip; the torch-op version is nets/_autograd.py unfold_packed_grads).
 *   tensors_dev  HOST array of n_tensors DEVICE pointers: the live parameters (state_dict order)
 *   grads_dev    HOST array of n_tensors DEVICE pointers: contiguous fp32 outputs of the same shapes, overwritten;
 *                a NULL entry skips that tensor (requires_grad = False)
 * SWN_E_UNSUPPORTED with aux_conv2d_flag and seg > 1 (callers keep the torch path there). */
int    swn_unfold_grads_device(const swn_net_desc* d, const float* gpacked_dev, const float* const* tensors_dev,
                               float* const* grads_dev, int n_tensors, void* stream);

/* ---- frame-rate front end  (cswnv_shift1.py:193,297 / dswnv.py:252,302) ---------------
 * scale_in -> conv_aux (two-sided dilated k=3 stack) -> hoisted in_x:
 *   cond[b][f][l][s][o] = sum_c in_x[l].weight[o, c*seg+s] * conv_aux(scale_in(aux))[b,c,f]
 * The rank-1 upsampling (ConvTranspose2d (1,U), cswnv_shift1.py:37-65) is folded into the
 * consumers as  in_x(x)[o,t] = bx[l][o] + sum_s w_up[(t+s)%U] * cond[b][(t+s)/U][l][s][o].
 *   aux_dev   (B, n_aux, Tf)             in
 *   work_dev  swn_frontend_work_floats() scratch
 *   cond_dev  (B, Tf, L*seg*2H)          out; NULL = stop after conv_aux (the dropout mode, swn_forward_drop, applies
 *                                        in_x at sample rate and reads only the activations kept in work_dev)
 * swn_frontend_conv_lds_bytes: which kernel serves conv_aux layer `layer` (0-based) - the bytes of dynamic LDS swn_frontend
 * requests for it when the layer runs with its window and weight rows staged in LDS (k = 3, at most 150 KB:
 * 4 * (cin * (64 + 2 * dilation) + 16 * cin * 3) - the window of all input rows and sixteen weight rows; above 48 KB the launch first raises the kernel's limit), 0 when it runs unstaged (any
 * other k, a larger layer) or when the descriptor or the layer index is refused.  swn_frontend decides by the same function;
 * only a refusal of the raised limit at run time sends a staged layer to the unstaged kernel (same bits). */
size_t swn_frontend_conv_lds_bytes(const swn_net_desc* d, int layer);
size_t swn_frontend_work_floats(const swn_net_desc* d, int batch, int n_frames);
size_t swn_cond_floats(const swn_net_desc* d, int batch, int n_frames);
int    swn_frontend(const swn_net_desc* d, const float* packed_dev, const float* aux_dev,
                    int batch, int n_frames, float* work_dev, float* cond_dev, void* stream);

/* ---- pool front end: the conditioning of many independent sessions finalised by one call --------------------------------
 * The ragged form of swn_frontend for a decode pool's tick (csrc/swn_frontend_pool.hip).  Entry e of the table is one session
 * at its own position: its feature buffer aux_dev, channel-major (n_aux, aux_stride), holds frames [0, n_received) once the
 * call has appended the n_new frames new_dev (n_aux, n_new) - a slice of a staging buffer all entries may share - at frames
 * [n_received - n_new, n_received); the call then writes the cond rows of the absolute frames [f0, f1) to
 * cond_dev + frame * N (N = L*seg*2H, the row of swn_frontend), and no other row.  Every row is bit-identical to the row
 * swn_frontend writes for the whole utterance: the same fmaf chains, frames outside [0, n_received) read as zero at every
 * layer.  Without SWN_FRONTEND_FINAL more features may follow, so only frames whose right context has arrived can be written:
 * f1 <= max(0, n_received - lookahead), lookahead = sum over conv_aux layers of dilation * (k - 1) / 2.  With it the features
 * end at n_received (the one-shot front end's zero padding on the right) and f1 <= n_received.
 * The call makes 3 + aux_dilation_size launches whatever n_entries is (the first one only when nothing is kept), works on the
 * concatenated frame list of all entries, and neither copies nor synchronises on the host: the table travels in the first
 * launch's arguments, which leaves a device copy at the head of work_dev for the others.
 *   work_dev  swn_frontend_pool_work_floats(d, entries_host, n_entries) floats of scratch (0 = the table is refused)
 * An entry with f1 == f0 and n_new == 0 does nothing.  SWN_E_BADARG, checked before anything is launched: a null pointer
 * (new_dev may be NULL when n_new == 0), n_entries outside [1, SWN_FRONTEND_POOL_MAX_ENTRIES], f0 < 0, f1 < f0, n_new < 0,
 * n_new > n_received, aux_stride < n_received, the bounds on f1 above, a cond_dev that is not 16-byte aligned when N is a multiple
 * of 4 (rows are then stored in 16-byte pieces), the same cond_dev in two entries, an unknown flag or a
 * non-zero reserved field, more than 2^24 frames in one stage over all entries.
 * sizeof(swn_frontend_pool_entry) == 56. */
typedef struct swn_frontend_pool_entry {
    float*       aux_dev;      /* this session's feature buffer (n_aux, aux_stride); frames [n_received - n_new, n_received) are written */
    const float* new_dev;      /* (n_aux, n_new) new frames, or NULL with n_new == 0 */
    float*       cond_dev;     /* this session's cond rows, 16-byte aligned (N % 4 == 0), at least f1 rows of N floats; rows [f0, f1) are written */
    int32_t aux_stride;        /* frames per channel row of aux_dev, >= n_received */
    int32_t n_received;        /* frames received, the n_new new ones included */
    int32_t n_new;             /* >= 0 */
    int32_t f0, f1;            /* absolute frames whose cond rows the call writes, 0 <= f0 <= f1 */
    int32_t flags;             /* SWN_FRONTEND_FINAL: the features end at n_received */
    int32_t reserved[2];       /* 0 */
} swn_frontend_pool_entry;
#define SWN_FRONTEND_POOL_MAX_ENTRIES 64
#define SWN_FRONTEND_FINAL 1
size_t swn_frontend_pool_work_floats(const swn_net_desc* d, const swn_frontend_pool_entry* entries_host, int n_entries);
int    swn_frontend_pool(const swn_net_desc* d, const float* packed_dev, const swn_frontend_pool_entry* entries_host,
                         int n_entries, float* work_dev, void* stream);

/* ---- pools over several models of one geometry ----------------------------------------------------------------------------
 * A deployment of the recipe holds one checkpoint per target speaker (run.sh stage 8: the multi-speaker net fine-tuned per
 * voice), all of one swn_net_desc.  The *_models calls serve sessions of different such models in ONE call: models_host is a
 * HOST array of n_models DEVICE pointers, each to swn_packed_floats(d) floats, and model_of_entry_host[e] in [0, n_models)
 * names the model of entry e.  A model that no entry names is allowed.  Entry structs, io layouts, bounds and every SWN_E_*
 * rule are those of the single-model call; SWN_E_BADARG in addition: n_models outside [1, SWN_POOL_MAX_MODELS], a null array
 * or a null model pointer, an index outside [0, n_models) - checked before anything is launched (the work-floats query then
 * returns 0).  Every result is bit-identical to the single-model call made with that entry's model.  Like the entry tables,
 * the model tables travel in kernel arguments: the calls neither copy nor synchronise on the host.
 *   swn_frontend_pool_models   every tile of the ragged front end reads ONE model's weight rows: each stage's column list is
 *       ordered by model and each model's columns start at a multiple of 64 (the padding columns between two models are
 *       computed from valid addresses and never stored), so the call still makes 3 + aux_dilation_size launches whatever
 *       n_entries and n_models are.  work_dev holds swn_frontend_pool_models_work_floats() floats (it includes that padding).
 *   swn_decode_pool_chunk_models (declared behind swn_decode_pool_chunk below)   the workgroup of entry e runs with the weight
 *       pointer of its model; the stepped chain is SWN_E_UNSUPPORTED as in swn_decode_pool_chunk.
 *   swn_decode_pool_chunk_models_w16 / _w8 (declared behind swn_decode_pool_chunk_w16 / _w8 below)   the same launch over the
 *       bf16 / FP8 images of the models: images_host is a HOST array of n_models DEVICE pointers, images_host[m] the image
 *       swn_pack_decode_w16 / _w8 made of models_host[m]; the workgroup of entry e reads its model's packed buffer AND its
 *       model's image, the resident out_1 slices and the FP8 row scales included.  SWN_E_BADARG in addition: a null images_host
 *       or a null image of a model below n_models; then SWN_E_UNSUPPORTED as swn_decode_pool_chunk_w16 / _w8 refuse (the variant
 *       must resolve to the symmetric BL6 kernel).  Every entry's rows are bit-identical to swn_decode_pool_chunk_w16 / _w8
 *       made with that entry's model and image. */
#define SWN_POOL_MAX_MODELS 16
size_t swn_frontend_pool_models_work_floats(const swn_net_desc* d, const swn_frontend_pool_entry* entries_host,
                                            const int32_t* model_of_entry_host, int n_entries, int n_models);
int    swn_frontend_pool_models(const swn_net_desc* d, const float* const* models_host, int n_models,
                                const int32_t* model_of_entry_host, const swn_frontend_pool_entry* entries_host,
                                int n_entries, float* work_dev, void* stream);

/* ---- autoregressive decode  (CSWNV.batch_fast_generate cswnv_shift1.py:287-430,
 *                              DSWNV.batch_fast_generate dswnv.py:296-399) ---------------
 * One persistent workgroup per utterance runs prologue (rf+1 seed positions) and all
 * n_steps steps; all utterances run n_steps = max(n_samples)/seg steps like the reference.
 *   cond_dev    (B, Tf, L*seg*2H)  from swn_frontend
 *   io          inputs of the sampling loop, see swn_decode_io below
 *   state_dev   swn_decode_state_floats() scratch (history rings; zeroed by the call)
 *   out_dev     laplace: (B, n_steps*seg) fp32 ; softmax: (B, n_steps) int32
 *   heads_dev   optional (B, n_steps, n_out) raw out_2 outputs at each step (may be NULL)
 *   variant     0 = auto, 1 = generic persistent kernel, 2 = register/LDS-resident BL6-class kernels (the wave-specialised
 *                   form for the single-sample Laplace nets, the symmetric form for the others), 6 = the symmetric BL6-class
 *                   kernel whatever the net (A/B and parity runs),
 *               3 = stepped multi-launch decode for large geometries (REF6: what auto picks there)
 *                   (from 24 utterances on in tiles of 8 channel pairs x 8 utterances that fetch a pair's weight rows once per
 *                   tile and stage the utterances' activations in LDS).
 *               Variants 4 and 5 of ABI 2 (cohort / cluster experiments) are retired: SWN_E_BADARG.                       */
typedef struct swn_decode_io {
    /* sampling noise.  noise_dev != NULL: the host-drawn stream (parity mode; the host draws it with the torch CPU
     * generator in the reference's order): laplace (B, n_steps, seg) uniform(-0.4999, 0.5) draws
     * (cswnv_shift1.py:373,380,387), softmax (B, n_steps, Q) Exp(1) draws (the multinomial of dswnv.py:364-365).
     * noise_dev == NULL: the kernels draw the same quantities themselves with a counter-based generator
     * (Philox4x32-10 keyed by rng_seed, counter = (global utterance index of b, step, element): csrc/swn_noise.hpp), like the
     * reference drawing on the model's device; nothing is drawn, stored or uploaded by the host. */
    const float* noise_dev;
    /* optional teacher forcing (may be NULL): laplace (B, n_steps*seg) fp32 samples, softmax (B, n_steps) int32
     * indices fed back instead of the generated ones */
    const void*  forced_dev;
    /* optional seed waveform `audio` of batch_fast_generate (may be NULL = the decode drivers' seed: zeros /
     * mu-law class Q/2, decode_cswnv_laplace-shift1.py:93, decode_dswnv_softmax.py:94-99):
     * laplace (B, seg) fp32 samples, softmax (B) int32 classes (cswnv_shift1.py:300-334, dswnv.py:305-336) */
    const void*  seed_dev;
    /* optional (may be NULL): every noise value used is also written here, layout of noise_dev - lets a test replay
     * a device-drawn run in the CPU oracle ("given the same noise") */
    float*       noise_out_dev;
    uint64_t     rng_seed;      /* used when noise_dev == NULL */
    uint32_t     rng_utt0;      /* global index of utterance 0 (utterance b draws as rng_utt0 + b) ... */
    uint32_t     reserved;      /* 0 */
    /* ... or, when not NULL, (B) uint32 global utterance indices, one per utterance of the batch: a decode driver that
     * sorts utterances by length into batches (decode_cswnv_laplace-shift1.py:77-84) passes each utterance's position in
     * the unsorted list, so that the draws depend neither on batching nor on how the list is sharded over GPUs */
    const uint32_t* rng_utt_ids_dev;
} swn_decode_io;
size_t swn_decode_state_floats(const swn_net_desc* d, int batch);
int    swn_decode(const swn_net_desc* d, const float* packed_dev, const float* cond_dev,
                  int batch, int n_frames, int n_steps, const swn_decode_io* io,
                  float* state_dev, void* out_dev, float* heads_dev,
                  int variant, void* stream);
/* Bytes of dynamic LDS one workgroup of the wave-specialised kernel (variant 2) takes for this net: the classic
 * instantiation (host-drawn noise, zero seed), or with extended != 0 the one the noise generator, the noise dump, a seed
 * waveform, streamed chunks and pools run.  0 when the descriptor is refused or the kernel does not serve the geometry.
 * Every word the kernel addresses lies inside it (at most 160 KB). */
size_t swn_decode_bl6w_lds_bytes(const swn_net_desc* d, int extended);

/* ---- streamed decode: swn_decode in resumable chunks, bit-identical to the one-shot call --------------------------
 * A session holds everything a decode kernel carries from one step to the next (history rings, sample window, and
 * whatever the kernel computes one step ahead).  Chunk k runs steps [step0, step0 + n_steps): positions, conditioning
 * frames and generator counters (swn_decode_io.rng_*) are absolute, the io arrays and out / heads are chunk-local
 * (B, n_steps, ...).  Concatenating the chunks of any partition of [0, N) gives swn_decode(..., n_steps = N) bit for bit.
 *   cond_dev    frames [0, n_frames) as swn_frontend wrote them; the bound (step0 + n_steps) * seg <= n_frames * U applies
 *   flags       SWN_CHUNK_BEGIN on the first chunk (runs the prologue from io->seed_dev; step0 must be 0), else 0: the
 *               state comes from session_dev, which the previous chunk of the SAME (net, batch, variant) left there
 *   session_dev swn_decode_session_floats() floats, owned by the caller for the life of the stream
 * A chunk of 0 steps without BEGIN changes nothing.  SWN_E_BADARG: a null pointer, BEGIN with step0 != 0, a negative
 * step0 / n_steps, the bound above, or a variant that is retired or does not resolve for the net - all checked before
 * anything is launched. */
#define SWN_CHUNK_BEGIN 1
/* the kernel swn_decode(variant) runs for (net, batch): 1, 2 (either BL6 form), 3, 6, or a negative SWN_E_* */
int    swn_decode_resolve_variant(const swn_net_desc* d, int batch, int variant);
size_t swn_decode_session_floats(const swn_net_desc* d, int batch, int variant);
int    swn_decode_chunk(const swn_net_desc* d, const float* packed_dev, const float* cond_dev, int batch, int n_frames,
                        int step0, int n_steps, int flags, const swn_decode_io* io, float* session_dev,
                        void* out_dev, float* heads_dev, int variant, void* stream);

/* ---- decode pool: many independent streamed decodes advanced by one launch -----------------------------------------
 * session_dev holds swn_decode_session_floats(d, capacity, variant) floats: `capacity` session slots, slot s laid out as
 * utterance b = s of a streamed decode of batch `capacity`.  Entry e of the table is one workgroup: it runs steps
 * [step0, step0 + n_steps) of the session in its slot over its own conditioning, exactly as swn_decode_chunk of that
 * session alone (batch 1) would.  The io arrays are indexed by entry, with n_max = max_e n_steps:
 *   out_dev  laplace (E, n_max*seg) fp32 | softmax (E, n_max) int32;  heads_dev (E, n_max, n_out);  io->noise_out_dev
 *   (E, n_max, width);  io->seed_dev (E, seg) fp32 | (E) int32;  io->rng_utt_ids_dev (E) (else entry e draws as rng_utt0 + e).
 *   Rows past an entry's own n_steps are not written.
 * An entry of 0 steps without SWN_CHUNK_BEGIN leaves its slot as it was.  The table travels in the kernel arguments: the
 * call neither copies nor synchronises on the host.  SWN_E_BADARG, checked before anything is launched: a null pointer,
 * n_entries outside [1, SWN_DECODE_POOL_MAX_ENTRIES], a slot outside [0, capacity) or in two entries, BEGIN with
 * step0 != 0, a negative step0 / n_steps, the conditioning bound, a non-zero reserved field or unknown flag, a non-NULL
 * io->noise_dev or io->forced_dev (pools draw their noise on the device), a variant that does not resolve.
 * SWN_E_UNSUPPORTED: the variant resolves to the stepped multi-launch decode (variant 0 on REF6-class nets; variant 1
 * runs them on the generic kernel). */
typedef struct swn_decode_pool_entry {
    const float* cond_dev;   /* this session's cond rows (n_frames, N) as swn_frontend wrote them */
    int32_t n_frames;        /* rows in cond_dev; (step0 + n_steps) * seg <= n_frames * U */
    int32_t slot;            /* session slot in [0, capacity) */
    int32_t step0;           /* absolute index of the entry's first step (0 with SWN_CHUNK_BEGIN) */
    int32_t n_steps;         /* >= 0 */
    int32_t flags;           /* SWN_CHUNK_BEGIN: run the prologue from io->seed_dev[e] into the slot */
    int32_t reserved;        /* 0 */
} swn_decode_pool_entry;
#define SWN_DECODE_POOL_MAX_ENTRIES 64
int    swn_decode_pool_chunk(const swn_net_desc* d, const float* packed_dev, int capacity,
                             const swn_decode_pool_entry* entries_host, int n_entries,
                             const swn_decode_io* io, float* session_dev,
                             void* out_dev, float* heads_dev, int variant, void* stream);
/* the same launch with one model per entry (see "pools over several models" above): a session slot's layout depends on the
 * geometry only, so slots of different models share session_dev, and a slot may pass from one model to another at BEGIN */
int    swn_decode_pool_chunk_models(const swn_net_desc* d, const float* const* models_host, int n_models,
                                    const int32_t* model_of_entry_host, int capacity,
                                    const swn_decode_pool_entry* entries_host, int n_entries,
                                    const swn_decode_io* io, float* session_dev,
                                    void* out_dev, float* heads_dev, int variant, void* stream);

/* ---- decode with bf16 storage of the streamed head matrices ------------------------------------------------------------
 * The symmetric BL6-class kernel (what variant 6 runs, and variants 0 / 2 for every net of the class but the single-sample
 * Laplace ones) streams out_skip, out_1 and - softmax - out_2 from L2 at every step.  The *_w16 calls stream a bf16 image of
 * those matrices instead: half the bytes, nothing else changed.  Semantics: out_skip.{l}.weight, out_1.weight and, for softmax
 * nets, out_2.weight are rounded to bf16, round to nearest even (torch's tensor.to(torch.bfloat16)); a Laplace net's out_2 (a
 * few rows resident on chip), every bias, the dilated-conv weights, the conditioning, activations, accumulation, gates and
 * sampling stay fp32.  bf16 -> fp32 is exact and the kernel widens the stored values and runs the fp32 kernel's FMAs in the fp32
 * kernel's order, so every output (out, heads, noise dump, session) is BIT-IDENTICAL to the fp32 call of the same variant on a
 * model whose named matrices were rounded beforehand.  The session layout is that of the fp32 calls.
 *   w16_dev     swn_decode_w16_bytes() bytes, filled by swn_pack_decode_w16 from packed_dev (one small launch; refill it
 *               whenever packed_dev changes).  The query returns 0 for a net the symmetric BL6 kernel does not serve.
 * swn_decode_w16 / swn_decode_chunk_w16 / swn_decode_pool_chunk_w16 take the arguments of swn_decode / swn_decode_chunk /
 * swn_decode_pool_chunk plus w16_dev, with their argument rules (state_dev of swn_decode_w16 is not read and may be NULL).
 * Checked before anything is launched: SWN_E_BADARG for a NULL w16_dev; SWN_E_UNSUPPORTED (text in swn_last_error_detail)
 * when `variant` does not resolve to the symmetric BL6 kernel for the net - variant 0 / 2 on a single-sample Laplace net
 * resolve to the wave-specialised kernel, so those nets need variant = 6; the stepped chain (launch-bound: weight bytes are
 * not its limit), the generic kernel and the wave-specialised kernel have no bf16 form.  One precision below bf16 exists: the
 * *_w8 calls below.
 * swn_decode_pool_chunk_models_w16 is swn_decode_pool_chunk_models over one image per model (see "pools over several models"
 * above): its arguments plus images_host, n_models device pointers in a host array.  Checked in this order before anything is
 * launched: the rules of swn_decode_pool_chunk, those of the model tables, a NULL images_host or images_host[m] (m < n_models)
 * is SWN_E_BADARG, then the refusals of swn_decode_pool_chunk_w16. */
size_t swn_decode_w16_bytes(const swn_net_desc* d);
int    swn_pack_decode_w16(const swn_net_desc* d, const float* packed_dev, void* w16_dev, void* stream);
int    swn_decode_w16(const swn_net_desc* d, const float* packed_dev, const float* cond_dev,
                      int batch, int n_frames, int n_steps, const swn_decode_io* io,
                      float* state_dev, void* out_dev, float* heads_dev, int variant, const void* w16_dev, void* stream);
int    swn_decode_chunk_w16(const swn_net_desc* d, const float* packed_dev, const float* cond_dev, int batch, int n_frames,
                            int step0, int n_steps, int flags, const swn_decode_io* io, float* session_dev,
                            void* out_dev, float* heads_dev, int variant, const void* w16_dev, void* stream);
int    swn_decode_pool_chunk_w16(const swn_net_desc* d, const float* packed_dev, int capacity,
                                 const swn_decode_pool_entry* entries_host, int n_entries,
                                 const swn_decode_io* io, float* session_dev,
                                 void* out_dev, float* heads_dev, int variant, const void* w16_dev, void* stream);
int    swn_decode_pool_chunk_models_w16(const swn_net_desc* d, const float* const* models_host, int n_models,
                                        const int32_t* model_of_entry_host, int capacity,
                                        const swn_decode_pool_entry* entries_host, int n_entries,
                                        const swn_decode_io* io, float* session_dev,
                                        void* out_dev, float* heads_dev, int variant, const void* const* images_host,
                                        void* stream);

/* ---- decode with FP8 (E4M3) storage of the streamed head matrices -------------------------------------------------------
 * The *_w8 calls are the *_w16 calls over a quarter of the fp32 bytes: the same kernel, the same tensors, the same guarantee.
 * The definition (also in runtime.py and DESIGN 3.1):
 *   tensors   out_skip.{l}.weight, out_1.weight and, for softmax nets, out_2.weight; everything else, biases included, fp32.
 *   format    OCP E4M3FN: 1 sign, 4 exponent (bias 7), 3 fraction bits; subnormals in steps of 2^-9; largest finite value 448;
 *             no infinities; codes 0x7f / 0xff are NaN and are never produced.
 *   scale     one power of two per output row r of each matrix, chosen without a logarithm: amax = max_k |W[r][k]|; e_r = 0
 *             if amax is 0; else frexp gives amax = m 2^x with m in [0.5, 1), and e_r = 9 - x if m <= 0.875 (448 = 0.875 x 2^9),
 *             else 8 - x; e_r is clamped to [-100, 100].  Then amax 2^e_r <= 448 and the row uses the top binade whenever it
 *             can (behind the lower clamp, amax >= 0.875 x 2^109, larger products saturate to +-448).
 *   code      q[r][k] = the E4M3 value nearest to W[r][k] 2^e_r, ties to the even fraction; the sign of a zero is kept.
 *   refusal   a weight that is not finite: SWN_E_BADARG from swn_pack_decode_w8 (which therefore waits for its stream).
 *   weight    the dequantised W^[r][k] = q[r][k] 2^-e_r; both scalings are exact in fp32.
 *   kernel    widens each streamed code to exactly W^ in fp32 (v_cvt_scalef32_pk_f32_fp8 with the row's 2^-e_r, exact for
 *             powers of two) and runs the fp32 kernel's FMAs in the fp32 kernel's order: every output is BIT-IDENTICAL to
 *             the fp32 call of the same variant on a model whose named matrices were replaced by W^.
 *   w8_dev    swn_decode_w8_bytes() bytes = one per weight + four per row (the fp32 2^-e_r), filled by swn_pack_decode_w8
 *             from packed_dev; refill it whenever packed_dev changes.  0 for a net the symmetric BL6 kernel does not serve.
 * Arguments, checks and refusals are those of the *_w16 counterparts with w8_dev in place of w16_dev (and, for
 * swn_decode_pool_chunk_models_w8, the images of swn_pack_decode_w8 in images_host).
 * swn_e4m3_table writes what the kernels' conversion makes of codes 0 .. 255 at `scale` (a power of two) into out_dev[256]. */
size_t swn_decode_w8_bytes(const swn_net_desc* d);
int    swn_pack_decode_w8(const swn_net_desc* d, const float* packed_dev, void* w8_dev, void* stream);
int    swn_decode_w8(const swn_net_desc* d, const float* packed_dev, const float* cond_dev,
                     int batch, int n_frames, int n_steps, const swn_decode_io* io,
                     float* state_dev, void* out_dev, float* heads_dev, int variant, const void* w8_dev, void* stream);
int    swn_decode_chunk_w8(const swn_net_desc* d, const float* packed_dev, const float* cond_dev, int batch, int n_frames,
                           int step0, int n_steps, int flags, const swn_decode_io* io, float* session_dev,
                           void* out_dev, float* heads_dev, int variant, const void* w8_dev, void* stream);
int    swn_decode_pool_chunk_w8(const swn_net_desc* d, const float* packed_dev, int capacity,
                                const swn_decode_pool_entry* entries_host, int n_entries,
                                const swn_decode_io* io, float* session_dev,
                                void* out_dev, float* heads_dev, int variant, const void* w8_dev, void* stream);
int    swn_decode_pool_chunk_models_w8(const swn_net_desc* d, const float* const* models_host, int n_models,
                                       const int32_t* model_of_entry_host, int capacity,
                                       const swn_decode_pool_entry* entries_host, int n_entries,
                                       const swn_decode_io* io, float* session_dev,
                                       void* out_dev, float* heads_dev, int variant, const void* const* images_host,
                                       void* stream);
int    swn_e4m3_table(float* out_dev /*256*/, float scale, void* stream);

/* ---- wide decode pool launch: up to 256 sessions per launch, the entry table on the device ----------------------------------
 * swn_decode_pool_chunk and its forms carry their table in the 4 KB of kernel arguments, hence 64 entries.  The wide call takes
 * up to SWN_DECODE_POOL_WIDE_MAX_ENTRIES (one workgroup per CU of an MI355X): it writes the table into table_dev - small setup
 * launches of 64 rows each, from their own kernel arguments - and the decode launch reads row blockIdx.x from there (scalar
 * loads).  Every row also holds the entry's packed buffer and image, so ONE entry point serves one model (n_models = 1) and
 * several, fp32 and stored weights; it is the whole wide surface.  Every session's rows and slot are BIT-IDENTICAL to those of
 * the 64-entry calls (the same kernels' bodies run the same batch-1 chunk), whatever shares its launch.
 *   arguments     those of swn_decode_pool_chunk_models, with its layouts (io arrays indexed by entry 0 .. n_entries - 1), then
 *   images_host   weight_format SWN_WEIGHTS_FP32: not read, may be NULL; else n_models device pointers in a host array, the
 *                 images of swn_pack_decode_w16 (SWN_WEIGHTS_BF16) / swn_pack_decode_w8 (SWN_WEIGHTS_E4M3) of models_host[m]
 *   table_dev     swn_decode_pool_wide_table_bytes(n_entries) bytes of device memory (0 for n_entries outside the range), 16-byte
 *                 aligned, owned by the call until its launches have run: it is written and read on `stream`, so a buffer
 *                 that is reused must be reused on that stream (or after an event).  Its content is private to the library.
 * Like the 64-entry calls the call neither synchronises nor copies on the host.  Checked before anything is launched, in this
 * order: the rules of swn_decode_pool_chunk with n_entries in [1, SWN_DECODE_POOL_WIDE_MAX_ENTRIES] - a slot in two entries is
 * SWN_E_BADARG wherever they sit; the model rules of swn_decode_pool_chunk_models with n_models in [1,
 * SWN_DECODE_POOL_WIDE_MAX_ENTRIES] (no table of 16 bounds them: the rows carry the pointers); an unknown weight_format, a NULL
 * table_dev or, for a stored format, a NULL images_host / images_host[m] is SWN_E_BADARG; then SWN_E_UNSUPPORTED as the
 * 64-entry calls refuse: the stepped chain for fp32 (swn_decode_pool_stepped_chunk serves it, 64 entries per call), and for a
 * stored format the refusals of swn_decode_pool_chunk_w16 / _w8, in their words.
 * What a wide tick still does per 64: the pool front end, the log-mel pool, the low cut, the resampler and the post-filter. */
#define SWN_DECODE_POOL_WIDE_MAX_ENTRIES 256
#define SWN_WEIGHTS_FP32 0
#define SWN_WEIGHTS_BF16 1
#define SWN_WEIGHTS_E4M3 2
size_t swn_decode_pool_wide_table_bytes(int n_entries);
int    swn_decode_pool_chunk_wide(const swn_net_desc* d, const float* const* models_host, int n_models,
                                  const int32_t* model_of_entry_host, int capacity,
                                  const swn_decode_pool_entry* entries_host, int n_entries,
                                  const swn_decode_io* io, float* session_dev,
                                  void* out_dev, float* heads_dev, int variant, const void* const* images_host,
                                  int weight_format, void* table_dev, void* stream);

/* ---- stepped decode pool: the decode pool of the stepped multi-launch decode (variant 3: REF6-class nets) -----------
 * Every launch of the stepped chain (input layer, L gated layers, skip / out_1 [/ out_2] mat-vecs, tail) serves all
 * entries of the table, each at its own iteration, so a tick costs about what one utterance's chunk costs while up to 64
 * sessions share it.  Entries count ITERATIONS: iterations 0 .. n_pro - 1 are the prologue positions
 * (n_pro = swn_decode_stepped_prologue_iterations()), iteration n_pro + i is generation step i; a new session's prologue
 * can therefore be spread over several ticks.  Entry e runs iterations [it0, it0 + n_it) of the session in its slot over its
 * own conditioning, exactly as swn_decode_chunk of that session alone (batch 1, variant 3) would; its generation steps of
 * the call go to rows [0, n_gen_e) of its out / heads / noise row (n_max = max_e n_gen_e, layouts of swn_decode_pool_chunk).
 *   session_dev  swn_decode_session_floats(d, capacity, 3) + SWN_DECODE_STEPPED_POOL_TABLE_FLOATS floats: slot s is laid
 *                out as utterance s of the stepped state; the tail holds the device copy of each call's entry table
 *                (written by the call's first launch, read by the others: the table travels once per call).
 * A BEGIN entry's slot is zeroed and seeded by a kernel; no other slot is touched.  An entry of 0 iterations without BEGIN
 * leaves its slot as it was.  SWN_E_BADARG, checked before anything is launched: a null pointer, n_entries outside
 * [1, SWN_DECODE_POOL_MAX_ENTRIES], a slot outside [0, capacity) or in two entries, BEGIN with it0 != 0, it0 == 0 without
 * BEGIN and n_it > 0, a negative it0 / n_it, a last generation step beyond the conditioning bound
 * (step + 1) * seg <= n_frames * U, an unknown flag or non-zero reserved field, a non-NULL io->noise_dev or io->forced_dev.
 * SWN_E_UNSUPPORTED: the stepped chain does not run this net at this capacity (swn_decode_resolve_variant(d, capacity, 3)
 * fails). */
typedef struct swn_decode_stepped_pool_entry {
    const float* cond_dev;   /* this session's cond rows (n_frames, N) as swn_frontend wrote them */
    int32_t n_frames;
    int32_t slot;            /* [0, capacity) */
    int32_t it0;             /* absolute iteration of the entry's first: prologue positions 0 .. n_pro - 1, then generation
                                step i at n_pro + i */
    int32_t n_it;            /* >= 0 */
    int32_t flags;           /* SWN_CHUNK_BEGIN: zero this slot, seed it from io->seed_dev[e]; it0 must be 0 */
    int32_t reserved;        /* 0 */
} swn_decode_stepped_pool_entry;
#define SWN_DECODE_STEPPED_POOL_TABLE_FLOATS 512
int    swn_decode_stepped_prologue_iterations(const swn_net_desc* d);
int    swn_decode_pool_stepped_chunk(const swn_net_desc* d, const float* packed_dev, int capacity,
                                     const swn_decode_stepped_pool_entry* entries_host, int n_entries,
                                     const swn_decode_io* io, float* session_dev, void* out_dev, float* heads_dev,
                                     void* stream);

/* ---- stepped decode pool over several models of one geometry -----------------------------------------------------------
 * swn_decode_pool_stepped_chunk with one model per entry (see "pools over several models" above): the multi-voice pool for
 * the nets people fine-tune per speaker (REF6).  Entry struct, io layouts, bounds and every SWN_E_* rule are those of
 * swn_decode_pool_stepped_chunk; the model rules (n_models, null array or model pointer, index range - a model nobody names
 * is allowed) are those of the other *_models calls, all checked before anything is launched.  Every entry's rows are
 * bit-identical to swn_decode_pool_stepped_chunk made with that entry's model.  A slot may pass from one model to another at
 * BEGIN.
 *   session_dev  swn_decode_session_floats(d, capacity, 3) + SWN_DECODE_STEPPED_POOL_MODELS_TABLE_FLOATS floats.  The slot
 *                region is that of swn_decode_pool_stepped_chunk, so both calls may serve one buffer of this size in turn; the
 *                tail holds 40-byte table rows (the single-model row and the resolved weight pointer of the entry's model).
 * The call makes exactly the launches the single-model call makes for the same entries, whatever n_models is.  The table is
 * sorted by (model, n_it descending, stable): the per-entry kernels read their weights through their row's pointer, and while
 * 24 or more entries are active the tile kernels serve tiles of at most 8 rows of ONE model, listed in the kernel arguments
 * and rebuilt on the host when an entry runs out.
 * swn_decode_stepped_pool_plan is that grouping as a pure host function (no device is touched): order_out[n_entries] is the
 * table order, tiles_out[3 * t + {0, 1, 2}] = first table row, rows (1 .. 8) and model of tile t at tick-local iteration j (the
 * entries with n_it > j).  tiles_out holds room for SWN_DECODE_STEPPED_POOL_MAX_TILES tiles.  Returns the number of tiles, or
 * SWN_E_BADARG (a null pointer, n_entries outside [1, SWN_DECODE_POOL_MAX_ENTRIES], n_models outside [1, SWN_POOL_MAX_MODELS],
 * a model index outside [0, n_models), a negative n_it or j). */
#define SWN_DECODE_STEPPED_POOL_MODELS_TABLE_FLOATS 640
#define SWN_DECODE_STEPPED_POOL_MAX_TILES 23
int    swn_decode_stepped_pool_plan(const int32_t* model_of_entry_host, const int32_t* n_it_host, int n_entries, int n_models,
                                    int j, int32_t* order_out, int32_t* tiles_out);
int    swn_decode_pool_stepped_chunk_models(const swn_net_desc* d, const float* const* models_host, int n_models,
                                            const int32_t* model_of_entry_host, int capacity,
                                            const swn_decode_stepped_pool_entry* entries_host, int n_entries,
                                            const swn_decode_io* io, float* session_dev, void* out_dev, float* heads_dev,
                                            void* stream);

/* ---- stepped decode: a new session's prologue in parallel launches -------------------------------------------------------
 * Before its first sample a session of the stepped chain fills its history rings: n_pro prologue positions, each a launch per
 * layer (about 690 x 7 dependent launches on REF6).  None of that is autoregressive - the input sample of every prologue
 * position is the seed padding (0 / class Q/2), the conditioning is frame 0 at phase 0 and the state starts from zeros - so
 * swn_decode_stepped_prologue computes all positions of a level in ONE launch: setup, input level and one launch per layer.
 * It zeroes and seeds the slot of every entry exactly as a SWN_CHUNK_BEGIN entry does and leaves each slot's whole state block
 * bit-identical to what a BEGIN entry with it0 = 0, n_it = n_pro of swn_decode_pool_stepped_chunk leaves (the same sums in the
 * same order).  Generation then continues through the existing calls: a pool entry with it0 = n_pro and no BEGIN, or
 * swn_decode_chunk without BEGIN at step0 = 0.  A slot no entry names is not touched.
 *   packed_dev | models_host, n_models, model_of_entry_host   one model (models_host and model_of_entry_host NULL), or one model
 *                per entry as in the *_models calls (packed_dev is then not read)
 *   n_slots      slots of session_dev: slot s lies at s * swn_decode_session_floats(d, 1, 3) floats, in the session of a
 *                streamed decode of batch n_slots and in a stepped pool's session of capacity n_slots alike
 *   io           only seed_dev is read: (n_entries, seg) fp32 | (n_entries) int32, indexed by entry, or NULL
 *   work_dev     swn_decode_stepped_prologue_work_floats(d, n_entries) floats of scratch (two levels of n_pro x Hp floats per
 *                entry); the query returns 0 for a geometry the stepped chain does not run or an entry count outside the range
 * SWN_E_BADARG, checked before anything is launched: a null pointer, n_entries outside [1, SWN_DECODE_POOL_MAX_ENTRIES],
 * n_slots < 1, a slot outside [0, n_slots) or in two entries, n_frames < 1, a non-NULL io->noise_dev or io->forced_dev, and
 * the model rules of the *_models calls.  SWN_E_UNSUPPORTED: the stepped chain does not run this net with n_slots slots. */
typedef struct swn_decode_stepped_prologue_entry {
    const float* cond_dev;   /* this session's cond rows (n_frames, N) as swn_frontend wrote them: the prologue reads frame 0 */
    int32_t n_frames;        /* >= 1 */
    int32_t slot;            /* [0, n_slots) */
} swn_decode_stepped_prologue_entry;
size_t swn_decode_stepped_prologue_work_floats(const swn_net_desc* d, int n_entries);
int    swn_decode_stepped_prologue(const swn_net_desc* d, const float* packed_dev, const float* const* models_host, int n_models,
                                   const int32_t* model_of_entry_host, int n_slots,
                                   const swn_decode_stepped_prologue_entry* entries_host, int n_entries,
                                   const swn_decode_io* io, float* session_dev, float* work_dev, void* stream);

/* ---- noise-shaping restoration on the device (run.sh stage 6 / 9: noise_shaping.py --inv false, run.sh:713-740) -------------
 * y = lowcut(MLSA_b(x)): the time-invariant MLSA filter of the coefficients b[0 .. order] (gain exp(b[0]) applied to the input,
 * Pade order `pade`, all-pass constant alpha; csrc/swn_dsp.c is the host version) followed by the causal FIR taps[0 .. n_taps-1],
 * both in fp64 from zero state.  Resumable: each session slot of state_dev keeps both filters' state between calls, so the
 * concatenated outputs of any sequence of chunks are bit-identical to one call over the whole signal.
 *   b_dev, taps_dev   device fp64 arrays of order + 1 / n_taps values;  mulaw_dev  device fp64 table of
 *                     SWN_POSTFILTER_MULAW_ENTRIES values (class -> sample; classes are clamped to it), or NULL without
 *                     mu-law entries
 *   state_dev         capacity slots of swn_postfilter_state_doubles(order, pade, n_taps) doubles, laid out as
 *                     [stage 1: 2 (pade + 1)] [stage 2: pade (order + 2) + pade + 1] (the layout of swn_dsp.c) [last n_taps - 1
 *                     MLSA outputs]
 *   entries_host      one entry per session of the call, any number (launched in groups of SWN_POSTFILTER_MAX_ENTRIES, one
 *                     wave each); a slot may appear once per call.  SWN_POSTFILTER_RESET starts the slot from zero state.
 * SWN_E_BADARG, before any device call: pade other than 4 / 5, |alpha| >= 1, n_taps outside [1, SWN_POSTFILTER_MAX_TAPS],
 * order < 1, a null pointer, capacity < 1, n_entries < 0, a slot outside [0, capacity) or in two entries, n < 0, an unknown
 * kind or flag, a mu-law entry without mulaw_dev.  SWN_E_UNSUPPORTED: order > SWN_POSTFILTER_MAX_ORDER.
 * swn_postfilter_state_doubles returns 0 for a bad (order, pade, n_taps). */
#define SWN_POSTFILTER_IN_F32 0         /* in_dev: fp32 samples */
#define SWN_POSTFILTER_IN_MULAW 1       /* in_dev: int32 mu-law classes, looked up in mulaw_dev */
#define SWN_POSTFILTER_RESET 1          /* flags: the slot starts from zero state */
#define SWN_POSTFILTER_MAX_ORDER 62
#define SWN_POSTFILTER_MAX_TAPS 256
#define SWN_POSTFILTER_MAX_ENTRIES 64
#define SWN_POSTFILTER_MULAW_ENTRIES 256
typedef struct swn_postfilter_entry {
    const void* in_dev;      /* n input samples (kind) */
    float* out_dev;          /* n fp32 restored samples */
    int32_t slot;            /* [0, capacity) */
    int32_t n;               /* >= 0; 0 with SWN_POSTFILTER_RESET only clears the slot */
    int32_t kind;            /* SWN_POSTFILTER_IN_* */
    int32_t flags;           /* SWN_POSTFILTER_RESET or 0 */
} swn_postfilter_entry;
size_t swn_postfilter_state_doubles(int order, int pade, int n_taps);
int    swn_postfilter_chunk(int order, double alpha, int pade, const double* b_dev, int n_taps, const double* taps_dev,
                            const double* mulaw_dev, double* state_dev, int capacity,
                            const swn_postfilter_entry* entries_host, int n_entries, void* stream);

/* ---- teacher-forced stack  (CSWNV.forward cswnv_shift1.py:191-267,
 *                             DSWNV.forward dswnv.py:250-276) ----------------------------
 *   audio_dev   laplace: (B, 1, T - seg) fp32 samples ; softmax: (B, T - 1) int32 indices
 *               (the one-hot of dswnv.py:68-93 is never materialised)
 *   cond_dev    (B, Tf, L*seg*2H) from swn_frontend, T = Tf * U
 *   work_dev    swn_forward_work_floats() scratch (hidden states, skip accumulator)
 *   out_dev     (B, n_out, Tp) raw out_2 outputs, Tp = T - 2*seg + 1 (softmax: T - 1);
 *               the host splits mu / log b / a (cswnv_shift1.py:228-267)
 *   hs_dev      optional (B, L+1, H, Tp) hidden states h_0..h_L for backward / tests
 * SWN_E_UNSUPPORTED (text in swn_last_error_detail), found on the host before anything is launched, for a net whose
 * hid_chn is not a multiple of 4; swn_forward_drop and the backward calls refuse such a net the same way.          */
size_t swn_forward_work_floats(const swn_net_desc* d, int batch, int n_frames);
int    swn_forward(const swn_net_desc* d, const float* packed_dev, const float* cond_dev,
                   const void* audio_dev, int batch, int n_frames, float* work_dev,
                   float* out_dev, float* hs_dev, void* stream);

/* ---- bf16 MFMA teacher-forced stack -------------------------------------------------------------
 * Training-speed variant of swn_forward: bf16 weights (device copy made by swn_pack_bf16) and bf16
 * time-major hidden states, fp32 accumulation, fp32 gate math.  Two geometry classes:
 *   BL6 class (H=64, K=2, S=128, Laplace head): register-resident layer kernels (HBM-bound);
 *   H a multiple of 64 up to 256, any K, Laplace or softmax (the reference's run.sh sizes): tiled GEMM stack.
 * Other geometries return SWN_E_UNSUPPORTED (use swn_forward).
 *   wbf16_dev  swn_bf16_weight_bytes() bytes, filled once per parameter set by swn_pack_bf16
 *   audio_dev  as for swn_forward: float waveform (Laplace) or int32 class indices (softmax)
 *   work_dev   swn_forward_bf16_work_bytes() bytes: hidden states [L+1][B][Tp][H] bf16 (+ skip / out_1 activations)
 *   out_dev    (B, n_out, Tp) fp32 raw out_2 outputs, same meaning as swn_forward            */
size_t swn_bf16_weight_bytes(const swn_net_desc* d);
int    swn_pack_bf16(const swn_net_desc* d, const float* packed_dev, void* wbf16_dev, void* stream);
size_t swn_forward_bf16_work_bytes(const swn_net_desc* d, int batch, int n_frames);
int    swn_forward_bf16(const swn_net_desc* d, const float* packed_dev, const void* wbf16_dev,
                        const float* cond_dev, const void* audio_dev, int batch, int n_frames,
                        void* work_dev, float* out_dev, void* stream);

/* Which kernels swn_forward_bf16 runs for a call of this geometry and size (host only, nothing is launched): one of
 * SWN_BF16_PATH_*, or the negative SWN_E_* code with which swn_forward_bf16 refuses the call given non-null pointers.
 * swn_forward_bf16 switches on this same value.  BL6 class, in this order (U the upsampling factor, frames = batch *
 * n_frames):
 *   FUSED          seg 1, 33 <= U <= 112, six layers, frames <= 3072: bf16_stack_fused_kernel, all gated layers in one launch
 *   UNITS4_HALVES  seg 1, 65 <= U <= 112, frames < 2048: half-frame units; FUSED takes all of these except in diagnostic
 *                  builds (SWN_OLD_UNITS), which have no FUSED
 *   UNITS4 / UNITS5 / UNITS7   seg 1, 16 <= U <= 64 / 65 <= U <= 80 / 81 <= U <= 112: bf16_layer_units_kernel<4 / 5 / 7>
 *   LAYER0         seg > 1, U < 16 or U > 112: bf16_layer_kernel<0>
 * GEMM_STACK: the other geometry class (swn_stack_bf16g.hip). */
#define SWN_BF16_PATH_FUSED         0
#define SWN_BF16_PATH_UNITS4        1
#define SWN_BF16_PATH_UNITS4_HALVES 2
#define SWN_BF16_PATH_UNITS5        3
#define SWN_BF16_PATH_UNITS7        4
#define SWN_BF16_PATH_LAYER0        5
#define SWN_BF16_PATH_GEMM_STACK    6
int    swn_forward_bf16_path(const swn_net_desc* d, int batch, int n_frames);

/* mixed-precision training: expand what swn_forward_bf16 kept in work_dev (bf16, time-major) into the fp32 work layout
 * of swn_forward (hidden states | relu(skip) | relu(out_1); swn_forward_work_floats() floats), so that swn_backward can
 * follow a bf16 forward of the same (cond, audio).  GEMM-stack class: all three are expanded from memory.  BL6 class:
 * the head kernel keeps the two activations on chip, so the hidden states are expanded and the two 1x1 products are
 * redone from them in the arithmetic `precision` selects (packed_dev is read only there).  _supported: 1 where swn_forward_bf16 exists, else 0. */
int    swn_bf16_train_forward_supported(const swn_net_desc* d);
int    swn_bf16_work_to_f32(const swn_net_desc* d, const float* packed_dev, const void* work_bf16_dev, int batch,
                            int n_frames, float* fwd_work_dev, int precision, void* stream);

/* ---- Laplace output split  (cswnv_shift1.py:228-267) -----------------------------------
 * raw (B, n_out, Tp) from swn_forward  ->  time-major tensors the reference returns:
 *   mu (B,Tp,seg) ; logb = logsigmoid(.) (B,Tp,seg) ; b = exp(logb) ; a (B,Tp,lpc) (NULL if lpc==0)
 *   b_clip / logb_clip (optional, may be NULL): logb floored at -14.1621 (b >= 7.07e-7), :233-236
 *   below_floor: int32[1] set non-zero when any logb < floor (the reference's torch.min test);
 *   the caller zeroes it before the call.                                                    */
int    swn_laplace_head(const swn_net_desc* d, const float* out_dev, int batch, int tp,
                        float* mu_dev, float* b_dev, float* logb_dev, float* a_dev,
                        float* b_clip_dev, float* logb_clip_dev, int32_t* below_floor_dev,
                        void* stream);

/* ---- backward of the teacher-forced stack (fp32)  (loss.backward() through CSWNV/DSWNV.forward,
 *      train_cswnv_laplace-stftcmplx_shift1.py:724-874) ----------------------------------------------
 *   aux_dev, cond_dev, audio_dev   the forward inputs
 *   fe_work_dev    the work buffer swn_frontend filled (scaled features and conv_aux activations)
 *   fwd_work_dev   the work buffer swn_forward filled (hidden states, relu(skip), relu(out_1))
 *   hs_dev         the hidden states if swn_forward wrote them to a separate hs_dev, else NULL
 *   grad_out_dev   (B, n_out, Tp) gradient of the loss wrt the raw out_2 outputs
 *   work_dev       swn_backward_work_floats() scratch
 *   gpacked_dev    swn_packed_floats() floats, ZEROED AND FILLED by the call: gradients in the packed
 *                  parameter layout (csrc/swn_geom.hpp); the host unfolds them onto the parameters  */
size_t swn_backward_work_floats(const swn_net_desc* d, int batch, int n_frames);
int    swn_backward(const swn_net_desc* d, const float* packed_dev, const float* aux_dev, const float* cond_dev,
                    const float* fe_work_dev, const void* audio_dev, const float* fwd_work_dev,
                    const float* hs_dev, const float* grad_out_dev, int batch, int n_frames,
                    float* work_dev, float* gpacked_dev, int precision, void* stream);
/* The same backward after a bf16 forward of the BL6 class, in the mixed-precision arithmetic (SWN_PRECISION_BF16) only, with
 * everything at sample rate fused (csrc/swn_bwd_bl6.hip): one launch for the head (recompute of relu(skip) / relu(out_1),
 * d out_1, d skip, g out_2), one per gated layer (the layer above's data gradient, the skip path's share, recompute, gate
 * derivative, highway carry, conditioning) plus one that also does the input layer, and one for every other weight
 * gradient - all reading the bf16 time-major hidden states directly.
 *   work_bf16_dev  the work buffer swn_forward_bf16 filled
 *   fwd_work_dev   ignored (may be NULL): the fp32 expansion of swn_bf16_work_to_f32 is not needed on this path
 *   work_dev       swn_backward_bf16_work_floats() floats (0 = geometry / size not covered: seg == 1, 16 <= U <= 112,
 *                  Laplace, BL6 stack, S = 128; the call then returns SWN_E_UNSUPPORTED and the caller uses swn_backward) */
size_t swn_backward_bf16_work_floats(const swn_net_desc* d, int batch, int n_frames);
int    swn_backward_bf16(const swn_net_desc* d, const float* packed_dev, const float* aux_dev, const float* cond_dev,
                         const float* fe_work_dev, const void* audio_dev, const float* fwd_work_dev,
                         const void* work_bf16_dev, const float* grad_out_dev, int batch, int n_frames,
                         float* work_dev, float* gpacked_dev, void* stream);
/* Mixed-precision training at the GEMM-stack geometries (hid_chn % 64 == 0 outside the BL6 class): the bf16 forward that also
 * keeps every layer's gate pre-activations (fp32, swn_forward_bf16_keep_floats() floats; 0 = variant not applicable), and the
 * backward that reads them instead of recomputing each layer's dilated conv (1.7 of 13 ms per step at the run.sh geometry).
 * swn_backward_keep takes swn_backward's arguments with a_keep_dev in place of hs_dev; fwd_work_dev is the fp32 expansion
 * swn_bf16_work_to_f32 made of the same forward's work buffer. */
size_t swn_forward_bf16_keep_floats(const swn_net_desc* d, int batch, int n_frames);
int    swn_forward_bf16_keep(const swn_net_desc* d, const float* packed_dev, const void* wbf16_dev,
                             const float* cond_dev, const void* audio_dev, int batch, int n_frames,
                             void* work_dev, float* out_dev, float* a_keep_dev, void* stream);
int    swn_backward_keep(const swn_net_desc* d, const float* packed_dev, const float* aux_dev, const float* cond_dev,
                         const float* fe_work_dev, const void* audio_dev, const float* fwd_work_dev,
                         const float* a_keep_dev, const float* grad_out_dev, int batch, int n_frames,
                         float* work_dev, float* gpacked_dev, void* stream);
/* ---- training-mode forward / backward WITH DROPOUT  (model.train(), forward(..., do=True) with do_prob > 0:
 *      cswnv_shift1.py:194-195,211-217,269-273 ; dswnv.py:253-254,264-270,278-282) --------------------------
 * The reference draws its Bernoulli masks inside nn.Dropout; here they are explicit inputs, like the decode
 * noise, so that the host can draw them with the torch CPU generator in the reference's order:
 *   drop_x_dev   (B, A0, T - coff) multiplicative mask (0 or 1/(1-p)) on the upsampled conditioning
 *                (A0 = n_aux * aux_kernel^aux_layers, coff = seg | 1 for softmax)
 *   drop_h_host  HOST array of L device pointers: drop_h[l] = (B, H, Tp) mask on the hidden state that layer l
 *                hands to layer l+1 (its skip output is not masked), NULL where the reference does not drop
 * aux_drop acts at sample rate, so the frame-rate hoisting of in_x does not apply: in_x is evaluated as a
 * sample-rate GEMM on the masked conditioning (no cond_dev input; fe_work_dev = swn_frontend's work buffer).
 * fwd_work_dev of swn_backward_drop must be the buffer swn_forward_drop filled, and `precision` must be the same for
 * both calls: with SWN_PRECISION_BF16, for nets with hid_chn % 64 == 0, the forward runs its sample-rate in_x GEMM and, per
 * layer, the dilated conv as a bf16-operand GEMM followed by an element-wise gate kernel (instead of the fused exact-fp32
 * layer kernel) and keeps every layer's gate pre-activations in that buffer; the backward reads them instead of
 * recomputing them. */
/* BL6 class (swn_backward_bf16's geometries) with SWN_PRECISION_BF16 and no mask between layers (drop_h_host[l] == NULL for
 * l < L-1; with dilation_repeat == 1 the reference's only hidden-state mask lands on the last layer's output, which nothing
 * reads - cswnv_shift1.py:211-217): both calls take a fused path instead - masked conditioning and in_x products as bf16
 * time-major rows from one tiled GEMM, the bf16 layer kernels of swn_forward_bf16 reading those rows, and the fused per-layer
 * backward of swn_backward_bf16 handing back their gradients for the two in_x contractions.  swn_drop_fused_path() tells
 * which path a (batch, n_frames, drop_h_host) takes in that mode: 1 fused, 0 the generic chain. */
int    swn_drop_fused_path(const swn_net_desc* d, int batch, int n_frames, const float* const* drop_h_host);
size_t swn_forward_drop_work_floats(const swn_net_desc* d, int batch, int n_frames);
int    swn_forward_drop(const swn_net_desc* d, const float* packed_dev, const float* fe_work_dev, const void* audio_dev,
                        int batch, int n_frames, const float* drop_x_dev, const float* const* drop_h_host,
                        float* work_dev, float* out_dev, float* hs_dev, int precision, void* stream);
size_t swn_backward_drop_work_floats(const swn_net_desc* d, int batch, int n_frames);
int    swn_backward_drop(const swn_net_desc* d, const float* packed_dev, const float* aux_dev, const float* fe_work_dev,
                         const void* audio_dev, const float* fwd_work_dev, const float* hs_dev,
                         const float* drop_x_dev, const float* const* drop_h_host, const float* grad_out_dev,
                         int batch, int n_frames, float* work_dev, float* gpacked_dev, int precision, void* stream);
/* gradient of swn_laplace_head: grads wrt mu / b / logb / a (time-major, any may be NULL) -> grad wrt raw */
int    swn_laplace_head_backward(const swn_net_desc* d, const float* out_dev, int batch, int tp,
                                 const float* gmu_dev, const float* gb_dev, const float* glogb_dev,
                                 const float* ga_dev, const float* gb_clip_dev, const float* glogb_clip_dev,
                                 float* graw_dev, void* stream);

/* ---- multi-resolution STFT loss (train_driver.batch_loss's spectral terms; csrc/swn_spectral.hip) ------------------------
 * rows sample signals and rows target signals of len samples (fp32, contiguous), n_sizes FFT sizes (HOST array `sizes`):
 *   l1_dev [rows][n_sizes]   mean over (bins, frames, re/im) of |STFT_n(sample) - STFT_n(target)|
 *   lsd_dev[rows][n_sizes]   mean_frames sqrt(mean_bins (10 log10 |S|^2 - 10 log10 |T|^2)^2), inf / nan as the formula gives them
 * STFT_n = torch.stft(x, n, window=hann_window(n)) with its defaults (hop n/4, reflect-centred, one-sided, 1 + len / hop
 * frames).  tables_dev: per size, in the order of `sizes`, cos(2 pi m / n) for m < n followed by the periodic Hann window
 * (2 n floats each).  state_dev (swn_spectral_state_bytes) receives what swn_spectral_backward needs, one byte per
 * (row, frame, bin); NULL (evaluation) writes none.  Its layout: the sizes in call order, per size [row][frame][bin], each
 * byte the two signs of STFT_n(sample - target) at that entry - bits 0-1 the real part, bits 2-3 the imaginary part, as
 * 1 = positive, 2 = negative, 0 = exactly zero; bits 4-7 are 0.  The backward gives grad_dev[rows][len] = d sum(g * l1) / d samples for
 * g_dev[rows][n_sizes]; targets get no gradient.  work_dev: swn_spectral_work_bytes, scratch of either call.  Results are
 * bit-identical from call to call.  SWN_E_BADARG: a null pointer, n_sizes outside [1, SWN_SPECTRAL_MAX_SIZES], a size that
 * is not a multiple of 32 in [32, SWN_SPECTRAL_MAX_FFT], or len <= size / 2 (the size queries return 0 then). */
#define SWN_SPECTRAL_MAX_SIZES 32
#define SWN_SPECTRAL_MAX_FFT 2048
size_t swn_spectral_work_bytes(int rows, int len, const int* sizes, int n_sizes);
size_t swn_spectral_state_bytes(int rows, int len, const int* sizes, int n_sizes);
int    swn_spectral_forward(const float* samples_dev, const float* targets_dev, int rows, int len, const int* sizes,
                            int n_sizes, const float* tables_dev, float* l1_dev, float* lsd_dev,
                            unsigned char* state_dev, void* work_dev, void* stream);
int    swn_spectral_backward(const float* g_dev, const unsigned char* state_dev, int rows, int len, const int* sizes,
                             int n_sizes, const float* tables_dev, float* grad_dev, void* work_dev, void* stream);

/* ---- Laplace chunk loss (train_driver.batch_loss between the stack and the spectral terms; csrc/swn_laplace_loss.hip) ----
 * NO = 2 seg + lpc, N = tp - skip >= 1.  Inputs (fp32, contiguous): raw_dev (batch, NO, tp) the stack's output; ctx_dev
 * (batch, tp + seg + lpc - 1) the LP context, NULL allowed only with lpc == 0; target_dev (batch, tp + seg - 1); eps_dev
 * (batch, seg, N) uniform deviates in (-0.5, 0.5); skip = leading positions dropped (the receptive field past the first
 * chunk of an utterance).  Per b, segment j < seg and position t in [skip, tp):
 *   mu = raw[j][t] + sum_k raw[2 seg + lpc-1-k][t] * ctx[j + t + k]      lb = logsigmoid(raw[seg + j][t])
 *   b_noclip = exp(lb), lc = max(lb, -14.1621), b = exp(lc)              trg = target[t + j]
 *   nll_dev[b][j]              = mean_t (ln 2 + lc + |trg - mu| / b)
 *   samples_dev[b][j][t-skip]  = mu - b_noclip * sign(eps) * log1p(-2 |eps|)          targets_dev[b][j][t-skip] = trg
 *   err_dev[b][j]              = mean_t |sample - trg|
 * samples_dev / targets_dev are (batch * seg, N) rows as swn_spectral_forward takes them.  stats_dev[7]: min, mean, max and
 * unbiased variance of mu, then min, mean, max of 2 b^2, of segment 0 over every b and kept position (the LaplaceLoss log
 * line).  work_dev: swn_laplace_loss_work_bytes, scratch of the forward.  The backward recomputes the head from raw and
 * writes every element of graw_dev (batch, NO, tp) = d (sum g_nll * nll + sum g_samples * samples) / d raw, zeros at
 * positions < skip; g_nll_dev (batch, seg), g_samples_dev (batch * seg, N) or NULL; sign(0) = 0 in |trg - mu| and in
 * sign(eps); the floor passes gradient only where lb >= -14.1621.  Results are bit-identical from call to call.
 * SWN_E_BADARG: a null pointer (ctx_dev with lpc > 0 included), N < 1, a softmax descriptor (the size query returns 0). */
size_t swn_laplace_loss_work_bytes(const swn_net_desc* d, int batch, int tp, int skip);
int    swn_laplace_loss_forward(const swn_net_desc* d, const float* raw_dev, const float* ctx_dev, const float* target_dev,
                                const float* eps_dev, int batch, int tp, int skip, float* nll_dev, float* err_dev,
                                float* samples_dev, float* targets_dev, float* stats_dev, void* work_dev, void* stream);
int    swn_laplace_loss_backward(const swn_net_desc* d, const float* raw_dev, const float* ctx_dev, const float* target_dev,
                                 const float* eps_dev, int batch, int tp, int skip, const float* g_nll_dev,
                                 const float* g_samples_dev, float* graw_dev, void* stream);

/* ---- log-mel conditioning features from waveforms (melspec.py; csrc/swn_melspec.hip) --------------------------------------
 * The definition, for a signal of len samples, len > n_fft / 2 (n_fft a multiple of 32 in [32, SWN_SPECTRAL_MAX_FFT],
 * 1 <= hop <= n_fft, hop need not divide n_fft; 1 <= n_mels <= SWN_LOGMEL_MAX_MELS; floor > 0):
 *   frames     F = 1 + len / hop.  Frame f reads the padded positions p = f * hop - n_fft / 2 + j, j < n_fft; reflect padding
 *              without repeating the edge sample: p < 0 -> -p, p >= len -> 2 (len - 1) - p
 *              (torch.stft(center=True, pad_mode="reflect"))
 *   window     periodic Hann, w[j] = 0.5 - 0.5 cos(2 pi j / n_fft)
 *   amplitude  A[f][b] = | sum_j x[p] w[j] e^(-2 pi i j b / n_fft) |, b = 0 .. n_fft / 2: the amplitude, not the power
 *   bank       HTK mel, mel(h) = 2595 log10(1 + h / 700), no area normalisation.  Points P_k = mel^-1 of n_mels + 2 equally
 *              spaced values from mel(fmin) to mel(fmax), 0 <= fmin < fmax <= fs / 2;
 *              W[m][b] = max(0, min((h_b - P_m) / (P_m+1 - P_m), (P_m+2 - h_b) / (P_m+2 - P_m+1))), h_b = b fs / n_fft,
 *              evaluated in float64 on the host and stored as fp32; a filter's non-zero weights are one run of bins
 *   mel        M[f][m] = sum_b W[m][b] A[f][b] over the filter's run in ascending b (one fmaf chain: the order is fixed)
 *   output     ln(max(M, floor)) as fp32, or M itself when `linear` is 1, time-major: frame f at out + f * n_mels
 * tables_dev (swn_logmel_table_floats floats): cos(2 pi m / n_fft) for m < n_fft, the window (n_fft), then the runs of
 * weights of filter 0, 1, ... back to back, zero-filled to 2 (n_fft / 2 + 1) floats.  bank_host[n_mels] (HOST): the run of
 * filter m as first bin | bins << 16.  fs, fmin and fmax exist only in how the caller built these two.
 * Entry e (HOST table, at most SWN_LOGMEL_MAX_ENTRIES, carried in the launch arguments: no host copy, no synchronisation)
 * is one row: wav_dev addresses the row's ABSOLUTE sample t0 and n_avail samples are there; len is the row's total length
 * or -1 while it is not known yet; the call writes the frames [f0, f1), frame f at out_dev + (f - f0) * n_mels.  The kernel
 * reads no sample outside [t0, t0 + n_avail).  A frame's values do not depend on the entry, the range or the call it is
 * computed in: any partition of the frames, and any window that holds what a range reads, gives the same bits.
 * work_dev: swn_logmel_work_bytes of scratch (the amplitudes of the call's frames).
 * SWN_E_BADARG, found on the host before anything is launched, text in swn_last_error_detail: a null pointer, n_fft, hop,
 * n_mels or floor out of range, linear not 0 / 1, n_entries out of range, a non-zero reserved field, a run outside the bins
 * or more than 2 (n_fft / 2 + 1) weights, len <= n_fft / 2 or > 2^30, a window that leaves the signal, f0 < 0, f1 < f0,
 * f1 > F, a frame whose span leaves the window, a frame that needs the reflected end (or any sample past the window) while
 * len is -1.  Entries with f1 == f0 do nothing and may carry null pointers; a call without any frame launches nothing.
 * The size queries return 0 for arguments the call refuses.  sizeof(swn_logmel_entry) == 40. */
typedef struct swn_logmel_entry {
    const float* wav_dev;      /* sample t0 of this row */
    float*       out_dev;      /* frame f0 of this row's output, (f1 - f0) * n_mels floats */
    int32_t t0;                /* absolute index of the first available sample, >= 0 */
    int32_t n_avail;           /* samples available from t0 on */
    int32_t len;               /* total length of the row, or -1: not known yet */
    int32_t f0, f1;            /* frames to compute, 0 <= f0 <= f1 */
    int32_t reserved;          /* 0 */
} swn_logmel_entry;
#define SWN_LOGMEL_MAX_MELS 128
#define SWN_LOGMEL_MAX_ENTRIES 64
size_t swn_logmel_table_floats(int n_fft, int n_mels);
size_t swn_logmel_work_bytes(int n_fft, int hop, const swn_logmel_entry* entries_host, int n_entries);
int    swn_logmel(int n_fft, int hop, int n_mels, float floor, int linear, const float* tables_dev, const int32_t* bank_host,
                  const swn_logmel_entry* entries_host, int n_entries, float* work_dev, void* stream);

/* ---- mel-cepstrum from waveforms (melspec.MelCepstrumExtractor; csrc/swn_melspec.hip) -----------------------------------------
 * The definition.  Frames, reflect padding, periodic Hann window and amplitude A[f][b], b = 0 .. n_fft / 2, are exactly those
 * of swn_logmel (F = 1 + len / hop).  Then, with 0 <= order <= min(SWN_MCEP_MAX_ORDER, n_fft / 2) and floor > 0:
 *   1. L[f][b] = ln(max(A[f][b], floor)), evaluated in double and rounded once to fp32, as the log-mel output is
 *   2. the real cepstrum v = irfft(L) of length n_fft
 *   3. the one-sided cepstrum c[0] = v[0], c[k] = 2 v[k] for 0 < k < n_fft / 2, c[n_fft / 2] = v[n_fft / 2], so that
 *      |exp(sum_k c(k) z^-k)| = A (the convention of the MLSA filter of swn_postfilter_chunk)
 *   4. the frequency transform with all-pass constant alpha to order M = order (SPTK freqt): mc[f][0 .. M]
 *   5. steps 2 - 4 are linear: mc[f] = G L[f], G of shape (M + 1, n_fft / 2 + 1), evaluated in float64 on the host, stored
 *      as fp32, its columns zero-padded to a multiple of 4 (alpha exists only in how the caller built G)
 *   6. output fp32, time-major: frame f, coefficient m at out_dev + (f - f0) * (order + 1) + m.  Each coefficient is one
 *      chain over the bins in ascending order (the k order of the matrix instruction), so a frame's values do not depend on
 *      the tile, the entry, the batch, the frame range or the window: any partition gives the same bits, as for swn_logmel.
 * On the first n_fft / 2 + 1 cepstral coefficients this is pysptk.sp2mc(A^2, M, alpha); parity with pysptk is not pinned.  It
 * is the cepstrum of the short-time spectrum, not of WORLD's cheaptrick envelope.
 * tables_dev (swn_mcep_table_floats floats): cos(2 pi m / n_fft) for m < n_fft, the window (n_fft), then G row by row, every
 * row (n_fft / 2 + 1 rounded up to 4) floats.  Entries, their rules and work_dev (swn_mcep_work_bytes) are those of
 * swn_logmel, with out_dev holding (f1 - f0) * (order + 1) floats.
 * SWN_E_BADARG, found on the host before anything is launched, text in swn_last_error_detail: order < 0, order >
 * SWN_MCEP_MAX_ORDER, order > n_fft / 2, floor <= 0 or not finite, and everything swn_logmel refuses for n_fft, hop and the
 * entries.  The size queries return 0 for arguments the call refuses. */
#define SWN_MCEP_MAX_ORDER 63
size_t swn_mcep_table_floats(int n_fft, int order);
size_t swn_mcep_work_bytes(int n_fft, int hop, const swn_logmel_entry* entries_host, int n_entries);
int    swn_mcep(int n_fft, int hop, int order, float floor, const float* tables_dev, const swn_logmel_entry* entries_host,
                int n_entries, float* work_dev, void* stream);

/* ---- log-mel pool: the new frames of many sessions per call (melspec.LogMelPool; csrc/swn_melspec.hip) -----------------------
 * Every session owns one slot of win_dev: window_floats floats (swn_logmel_pool_window_floats(n_fft, max_chunk) = n_fft +
 * max_chunk: under the streaming rule of melspec.py a session holds at most n_fft samples between calls) that hold the tail
 * of its signal from the window's first float on.  new_dev is one staged buffer with the new samples of all entries, out_dev
 * one output buffer.  Entry e (HOST table, at most SWN_LOGMEL_POOL_MAX_ENTRIES, integers only, carried in the launch
 * arguments: no host copy, no synchronisation) says: before the call the window of `slot` holds the n_held samples from the
 * ABSOLUTE index t0 on.  The call
 *   1. drops n_drop samples from the window's front and appends the n_new samples at new_dev + new_off, so that the window
 *      holds the samples [t0 + n_drop, t0 + n_held + n_new) from its first float, and then
 *   2. computes the frames [f0, f1) from it, with the definition and the arithmetic of swn_logmel (a frame has the bits
 *      swn_logmel gives it), and writes frame f, filter m at out_dev[out_off + m * out_stride + (f - f0)]: channel-major,
 *      the (n_aux, frames) layout swn_frontend_pool stages.
 * len is the signal's total length, or -1 while it is not known.  Two launches at most (the window update, one block per
 * entry; the frame kernel), no copy; an entry without frames only updates its window, a call in which nothing moves and no
 * frame is due launches nothing.  The kernels read no window float outside the held range and write none outside
 * [0, n_held - n_drop + n_new).  The caller answers for win_dev holding a window for every slot it names and out_dev for
 * every range.
 * work_dev: swn_logmel_pool_work_bytes of scratch.
 * SWN_E_BADARG, found on the host before anything is launched, text in swn_last_error_detail: a null pointer (new_dev only
 * where an entry has new samples; out_dev, tables_dev and work_dev only where a frame is due), n_entries out of range, a slot
 * named twice or negative, a negative count or offset, n_drop > n_held, n_held or n_held - n_drop + n_new beyond
 * window_floats, window_floats outside [1, 2^24], a non-zero reserved field, output rows of two entries (or of one:
 * out_stride < f1 - f0) that overlap, and every rule of swn_logmel for n_fft, hop, n_mels, floor, linear, the bank, len and
 * the frame range, applied to the updated window: a frame whose samples (the reflected ones included) are not all in it,
 * f1 > 1 + len / hop, a frame that needs the reflected end while len is -1.
 * The size queries return 0 for arguments the call refuses.  sizeof(swn_logmel_pool_entry) == 48. */
typedef struct swn_logmel_pool_entry {
    int32_t slot;              /* which window of win_dev */
    int32_t t0;                /* absolute index of the window's first sample before the call */
    int32_t n_held;            /* samples in the window before the call */
    int32_t n_drop;            /* samples to discard from its front, <= n_held */
    int32_t new_off, n_new;    /* the entry's new samples: new_dev + new_off, n_new of them */
    int32_t len;               /* total length of the signal, or -1: not known yet */
    int32_t f0, f1;            /* frames to compute, 0 <= f0 <= f1 */
    int32_t out_off;           /* frame f0 of filter 0 in out_dev */
    int32_t out_stride;        /* floats between two filters' rows, >= f1 - f0 */
    int32_t reserved;          /* 0 */
} swn_logmel_pool_entry;
#define SWN_LOGMEL_POOL_MAX_ENTRIES 64
size_t swn_logmel_pool_window_floats(int n_fft, int max_chunk);
size_t swn_logmel_pool_work_bytes(int n_fft, int hop, int n_mels, size_t window_floats,
                                  const swn_logmel_pool_entry* entries_host, int n_entries);
int    swn_logmel_pool(int n_fft, int hop, int n_mels, float floor, int linear, const float* tables_dev,
                       const int32_t* bank_host, float* win_dev, size_t window_floats, const float* new_dev, float* out_dev,
                       const swn_logmel_pool_entry* entries_host, int n_entries, float* work_dev, void* stream);

/* ---- stage-1 low cut on the device (melspec.LowCut; csrc/swn_lowcut.hip, csrc/swn_lowcut.hpp) --------------------------------
 * The definition (melspec.py restates it).  Taps h[0 .. n_taps - 1] in fp64, 1 <= n_taps <= SWN_LOWCUT_MAX_TAPS; input samples
 * x in fp32 with x[t] = 0 for t < 0.  Output sample t:
 *     acc = 0.0;  for q = 0 .. n_taps - 1 ascending: acc = fma(h[q], (double)x[t - q], acc);  y[t] = (float)acc
 * - the last stage of swn_postfilter_chunk: one fp64 fma chain over the taps in ascending order, rounded once to fp32.  Every
 * output sample depends only on its absolute index and the signal, not on the chunking, the entry, the batch, the tile or the
 * call: any partition of a signal into chunks gives the bits of the one-shot call.  The state of a session is its last
 * n_taps - 1 RAW input samples in fp32 (exact: the inputs are fp32), which is what makes a call parallel over time.
 *
 * swn_lowcut_chunk: state_dev holds `capacity` slots of swn_lowcut_state_floats(n_taps) = n_taps - 1 floats, slot s from float
 * s * (n_taps - 1) on, oldest sample first.  Entry e (HOST table, any number, launched in groups of SWN_LOWCUT_MAX_ENTRIES and
 * carried in the launch arguments: no host copy, no synchronisation) filters the n samples at in_dev as the next chunk of the
 * session in `slot` and writes n floats at out_dev; SWN_LOWCUT_RESET starts the slot from zero history, an entry with n == 0 and
 * no RESET leaves its slot untouched.  Blocks cover (entry, tile of SWN_LOWCUT_TILE outputs).  Every tile of an entry reads the
 * slot's state, so the filter launch writes no state: a second small launch (one block per entry, stream-ordered after the
 * first) replaces it, reading it whole before writing where n < n_taps - 1 makes the new state a shift of the old one.
 * SWN_E_BADARG, found on the host before anything is launched, text in swn_last_error_detail: n_taps out of range, a null
 * pointer (in_dev / out_dev only where n > 0), capacity < 1, n_entries < 0, a slot outside [0, capacity) or named twice, n < 0,
 * an unknown flag or a non-zero reserved field, in_dev and out_dev ranges of one entry that overlap.
 * swn_lowcut_state_floats returns 0 for a refused n_taps (and for n_taps == 1, which has no state).
 * sizeof(swn_lowcut_entry) == 32. */
#define SWN_LOWCUT_MAX_TAPS 256
#define SWN_LOWCUT_MAX_ENTRIES 64
#define SWN_LOWCUT_TILE 1024            /* output samples per block */
#define SWN_LOWCUT_RESET 1              /* flags: the slot starts from zero history */
typedef struct swn_lowcut_entry {
    const float* in_dev;     /* n raw fp32 samples */
    float* out_dev;          /* n filtered fp32 samples; must not overlap in_dev's range */
    int32_t slot;            /* [0, capacity) */
    int32_t n;               /* >= 0; 0 with SWN_LOWCUT_RESET only clears the slot */
    int32_t flags;           /* SWN_LOWCUT_RESET or 0 */
    int32_t reserved;        /* 0 */
} swn_lowcut_entry;
size_t swn_lowcut_state_floats(int n_taps);
int    swn_lowcut_chunk(int n_taps, const double* taps_dev, float* state_dev, int capacity,
                        const swn_lowcut_entry* entries_host, int n_entries, void* stream);

/* swn_logmel_pool_lowcut: swn_logmel_pool whose new samples are RAW; the window receives the filtered samples.  hist_dev holds
 * one slot of n_taps - 1 floats per window slot (slot s from float s * (n_taps - 1) on, oldest first): after the call it holds
 * the last n_taps - 1 raw samples before t0 + n_held + n_new.  An entry with t0 == 0 and n_held == 0 has received nothing yet
 * and starts from zero history whatever the slot's floats hold; an entry with n_new == 0 leaves them untouched.  The filtering
 * happens inside the window-update launch (one block per entry, which reads the history it needs before it replaces it), so a
 * call still makes at most two launches.  A frame has the bits swn_logmel gives it on the filtered signal.  Every rule of
 * swn_logmel_pool applies; SWN_E_BADARG also for n_taps outside [1, SWN_LOWCUT_MAX_TAPS] and a null taps_dev or hist_dev. */
int    swn_logmel_pool_lowcut(int n_fft, int hop, int n_mels, float floor, int linear, const float* tables_dev,
                              const int32_t* bank_host, float* win_dev, size_t window_floats, const float* new_dev, float* out_dev,
                              const swn_logmel_pool_entry* entries_host, int n_entries, float* work_dev, int n_taps,
                              const double* taps_dev, float* hist_dev, void* stream);

/* ---- rational resampler on the device (melspec.Resampler; csrc/swn_resample.hip) -----------------------------------------------
 * The definition (melspec.py restates it, tests/resample_ref.py pins it).  fs_in and fs_out are integers, up = L = fs_out / g and
 * down = M = fs_in / g with g = gcd(fs_in, fs_out).  Prototype filter h[0 .. N - 1] in fp64, N = n_taps odd, D = (N - 1) / 2
 * (melspec.resample_taps: L * firwin(2 * 10 * max(L, M) + 1, 1 / max(L, M), ("kaiser", 5.0)), the filter of scipy's resample_poly).
 * Polyphase table P[r][q], r < L, q < Q = ceil(N / L): P[r][q] = h[r + q L], and 0.0 where r + q L >= N; fp64 on the device, row
 * by row (swn_resample_table_doubles = L Q doubles).  Output sample n (absolute index) of a signal of `len` fp32 input samples,
 * x[t] = 0 outside [0, len):
 *     p = n M + D (64-bit),  r = p mod L,  i0 = p div L
 *     acc = +0.0;  for q = 0 .. Q - 1 ascending: acc = fma(P[r][q], (double)x[i0 - q], acc);  y[n] = (float)acc
 * and there are ceil(len L / M) outputs: one fp64 fma chain in a fixed order, rounded once to fp32 - the arithmetic of
 * swn_lowcut_chunk.  A sample's bits depend only on its absolute index and the signal, not on the chunking, the entry, the batch,
 * the tile or the call.  Streaming rule (melspec.resample_ready is the one place it is written): while the signal goes on and T
 * inputs have arrived, the computable outputs are those with i0 <= T - 1 - none if T L - 1 - D < 0, else (T L - 1 - D) div M + 1 of
 * them; when the signal ends at T, all ceil(T L / M).  A session's state is its last Q - 1 RAW inputs in fp32 (exact), which is
 * what makes a call parallel over time.
 *
 * swn_resample_chunk: state_dev holds `capacity` slots of swn_resample_state_floats(up, n_taps) = Q - 1 floats, slot s from float
 * s (Q - 1) on, oldest sample first.  Entry e (HOST table, any number, launched in groups of SWN_RESAMPLE_MAX_ENTRIES and carried
 * in the launch arguments: no host copy, no synchronisation) is one session's next chunk: in_dev holds the n_in new inputs at
 * absolute indices [in0, in0 + n_in), out_dev receives the n_out outputs at absolute indices [out0, out0 + n_out); len is the
 * signal's length, or -1 while it is unknown.  An entry with in0 == 0 starts from zero history whatever the slot holds;
 * n_in == 0 && n_out == 0 leaves the slot untouched; n_in == 0 with len == in0 is the flush at the end.  Blocks cover (entry, tile
 * of SWN_RESAMPLE_TILE outputs); a block stages the input span its tile reads (from the chunk, or from the slot's state below the
 * chunk's first sample) in LDS and writes its outputs; the table is read through the caches.  That launch writes no state: a
 * second small launch, one block per entry and stream-ordered behind the first, replaces it, reading the old state whole before
 * writing any of it.
 * SWN_E_BADARG, found on the host before anything is launched, text in swn_last_error_detail:
 *   - up or down < 1, or not coprime; n_taps even or outside [1, SWN_RESAMPLE_MAX_TAPS]; up > SWN_RESAMPLE_MAX_UP;
 *     Q > SWN_RESAMPLE_MAX_Q; a tile's input span ceil(SWN_RESAMPLE_TILE down / up) + Q > SWN_RESAMPLE_MAX_SPAN
 *   - a null table_dev or state_dev, capacity < 1, n_entries < 0, a null entries_host with n_entries > 0; a null in_dev with
 *     n_in > 0 or a null out_dev with n_out > 0
 *   - a slot outside [0, capacity) or named twice; n_in, n_out, in0 or out0 < 0, len < -1, an index too large for the 64-bit
 *     arithmetic; a non-zero reserved field; in_dev and out_dev ranges of one entry that overlap
 *   - an output that is not computable: i0 > in0 + n_in - 1 for the last output while len is -1; or, with len given,
 *     len != in0 + n_in, or an output index >= ceil(len up / down)
 *   - an output that reads below the state: i0 of output out0 is < in0.
 * The size queries return 0 for refused arguments (swn_resample_state_floats also for Q == 1, which has no state).
 * sizeof(swn_resample_entry) == 56. */
#define SWN_RESAMPLE_MAX_UP 1024
#define SWN_RESAMPLE_MAX_Q 256
#define SWN_RESAMPLE_MAX_TAPS 65535
#define SWN_RESAMPLE_MAX_ENTRIES 64
#define SWN_RESAMPLE_TILE 1024          /* output samples per block */
#define SWN_RESAMPLE_MAX_SPAN 8192      /* floats of a block's LDS image of the input */
typedef struct swn_resample_entry {
    const float* in_dev;     /* n_in raw fp32 inputs, absolute indices [in0, in0 + n_in) */
    float* out_dev;          /* n_out fp32 outputs, absolute indices [out0, out0 + n_out); must not overlap in_dev's range */
    int64_t in0;             /* inputs the session received before this chunk; 0 starts from zero history */
    int64_t out0;            /* outputs the session was given before this chunk */
    int64_t len;             /* the signal's length (then == in0 + n_in), or -1 while it goes on */
    int32_t n_in;            /* >= 0 */
    int32_t n_out;           /* >= 0 */
    int32_t slot;            /* [0, capacity) */
    int32_t reserved;        /* 0 */
} swn_resample_entry;
size_t swn_resample_table_doubles(int up, int down, int n_taps);
size_t swn_resample_state_floats(int up, int n_taps);
int    swn_resample_chunk(int up, int down, int n_taps, const double* table_dev, float* state_dev, int capacity,
                          const swn_resample_entry* entries_host, int n_entries, void* stream);

/* ---- F0 and voicing from waveforms (pitch.F0Extractor; csrc/swn_f0.hip) ---------------------------------------------------------
 * The definition (pitch.py restates it, tests/f0_ref.py pins it).  fs > 0; 1 <= hop <= SWN_F0_MAX_HOP; SWN_F0_MIN_WIN <= win = W <=
 * SWN_F0_MAX_WIN, any integer; lags 2 <= lag_lo <= lag_hi <= SWN_F0_MAX_LAG - 1 (pitch.f0_lags: lag_lo = floor(fs / maxf0),
 * lag_hi = ceil(fs / minf0)); 0 < threshold <= 1.  With L1 = lag_hi + 1 a frame spans S = W + L1 samples (swn_f0_span).  Input
 * samples are fp32 and finite, len >= 1 of them, and x[t] = 0 outside [0, len): the padding is zeros, not reflection.
 *   frames      F = 1 + len / hop, the grid of swn_logmel.  Frame f reads x[s .. s + S) with s = f * hop - S / 2.
 *   difference  for tau = 1 .. L1, in fp64, one chain over j = 0 .. W - 1 ascending, from acc = +0.0:
 *                   diff = (double)x[s + j] - (double)x[s + j + tau];  acc = fma(diff, diff, acc);      d(tau) = acc
 *   normalised  c(0) = 0, c(tau) = c(tau - 1) + d(tau) strictly in this order; d'(tau) = (d(tau) * (double)tau) / c(tau) if
 *               c(tau) > 0, else 1.0; d'(0) = 1
 *   decision    scan tau = lag_lo .. lag_hi ascending; at the first tau with d'(tau) < threshold walk to the local minimum
 *               (while tau < lag_hi and d'(tau + 1) < d'(tau): tau += 1): the frame is voiced with lag tau*.  If no tau is below
 *               the threshold the frame is unvoiced and tau* is the first arg-min of d' over [lag_lo, lag_hi]
 *   refinement  voiced frames only: ym, y0, yp = d'(tau* - 1), d'(tau*), d'(tau* + 1); den = ym - 2 y0 + yp;
 *               shift = 0.5 * (ym - yp) / den if den > 0 and y0 <= ym and y0 <= yp, else 0; f0 = fs / ((double)tau* + shift)
 *   output      fp32, each value rounded once, frame f at out_dev + (f - f0) * 2: [0] = F0 in Hz, exactly 0.0 when unvoiced;
 *               [1] = d'(tau*), the aperiodicity (1.0 on silence)
 * A frame's two values depend on the signal and the frame index alone - not on the entry, the batch, the frame range, the window
 * or the call: any partition gives the same bits.  Streaming rule (pitch.f0_frames_ready is the one place it is written): while
 * the signal goes on, frame f is computable iff f * hop - S / 2 + S <= n_received; when it ends, all 1 + n_received / hop
 * frames are.  The latency is S - S / 2 samples (n_fft / 2 for swn_logmel).  This is not WORLD's Harvest and parity with it is
 * not claimed.
 * Entries are swn_logmel_entry with the meaning swn_logmel gives them (wav_dev at absolute sample t0, n_avail samples there, len
 * or -1, the frames [f0, f1), reserved 0); out_dev holds (f1 - f0) * 2 floats.  At most SWN_LOGMEL_MAX_ENTRIES entries, carried
 * in the launch arguments: one launch, one block per frame, no scratch buffer, no host copy, no synchronisation.  The kernel
 * reads nothing outside [t0, t0 + n_avail).
 * SWN_E_BADARG, found on the host before anything is launched, text in swn_last_error_detail: fs, hop, win, the lags or the
 * threshold out of range, a null pointer, n_entries out of range, a non-zero reserved field, len < 1 or > 2^30, a window that
 * leaves the signal, f0 < 0, f1 < f0, f1 > F, a frame whose in-signal samples are not all in the window, a frame that needs
 * samples past the window while len is -1, more than 2^24 frames in one call.  Entries with f1 == f0 do nothing and may carry
 * null pointers; a call without any frame launches nothing.  swn_f0_span returns S, or 0 for a win or lag_hi the call refuses. */
#define SWN_F0_MAX_HOP 4096
#define SWN_F0_MIN_WIN 16
#define SWN_F0_MAX_WIN 2048
#define SWN_F0_MAX_LAG 1536
int    swn_f0_span(int win, int lag_hi);
int    swn_f0(double fs, int hop, int win, int lag_lo, int lag_hi, double threshold, const swn_logmel_entry* entries_host,
              int n_entries, void* stream);

/* ---- Band aperiodicity from waveforms (pitch.BandAperiodicityExtractor; csrc/swn_f0.hip) -----------------------------------------
 * Per frame: swn_f0's two values and, for each of B band-pass filters, how far the band signal is from periodic at the frame's
 * decided lag, coded in dB - the counterpart of the reference's `codeap` columns, by a definition of this project's own.  This is
 * not WORLD's D4C / code_aperiodicity: parity with them is neither claimed nor pinned.
 * The definition (pitch.py restates it, tests/bap_ref.py pins it).  Everything about F0 is swn_f0's, unchanged: fs, hop, win = W,
 * lag_lo, lag_hi, threshold, L1 = lag_hi + 1, S = W + L1, zeros outside [0, len), F = 1 + len / hop, frame f at s = f hop - S / 2
 * with its decided lag tau* (defined on unvoiced frames too) and its voicing decision.  New: 1 <= n_bands = B <=
 * SWN_BAP_MAX_BANDS filters of n_taps = T fp64 taps h_b[0 .. T) each, T odd, 1 <= T <= SWN_BAP_MAX_TAPS, c = (T - 1) / 2, as a
 * device table of B * T doubles (the call knows nothing of Hz: the band edges exist only in how the caller built the table);
 * a sum window SWN_F0_MIN_WIN <= band_win = Wb <= W; a floor, 0 < floor < 1.
 *   band signal  for every integer t, x = 0 outside [0, len):  y_b[t] = sum_k h_b[k] * (double)x[t + c - k], one fp64 chain
 *                acc = fma(h_b[k], x, acc), k ascending from acc = +0.0.  Centred: no group delay is left in it.
 *   frame sums   s_b = f hop - (Wb + tau*) / 2 (C division of a non-negative number): the windows [s_b, s_b + Wb) and
 *                [s_b + tau*, s_b + tau* + Wb) lie inside [s, s + S).  Over j = 0 .. Wb - 1:
 *                    d = sum (y_b[s_b + j] - y_b[s_b + j + tau*])^2,  e0 = sum y_b[s_b + j]^2,  e1 = sum y_b[s_b + j + tau*]^2
 *   order        of each sum, depending on Wb alone: partial chain l = 0 .. 63 runs over j = l, l + 64, .. ascending by fma
 *                (diff = y0 - y1 rounded, then fma(diff, diff, acc); fma(y, y, acc)) from +0.0; the 64 partials are then added
 *                into +0.0 in ascending l
 *   ratio        e = e0 + e1; ap = d / e if e > 0, else 1.0: 0 for a band exactly periodic at tau*, about 1 for noise, at most 2
 *   coded        10 * log10(min(max(ap, (double)floor), 1.0)) dB (<= 0) on voiced frames; exactly 0.0 on unvoiced frames
 *   output       fp32, each value rounded once, frame f at out_dev + (f - f0) * (2 + B): [0], [1] have swn_f0's bits for the same
 *                frame, [2 + b] is the coded value of band b
 * A frame reads x[s - c .. s + S + c) (swn_bap_reach = S + 2 c samples).  Its values depend on the signal and the frame index
 * alone: any batch, frame range, window or chunking gives the same bits.  Streaming rule (pitch.bap_frames_ready is the one place
 * it is written): while the signal goes on, frame f is computable iff f hop - S / 2 + S + c <= n_received; when it ends, all F
 * frames are.  The latency is S - S / 2 + c samples.
 * Known limits: tau* is an integer lag, so a band around frequency nu cannot go below about 1 - cos(pi nu / fs) for a period
 * that falls between two lags, and vibrato inside the window raises the value further.
 * Entries are swn_logmel_entry with swn_f0's meaning; out_dev holds (f1 - f0) * (2 + B) floats.  Two launches per call: one
 * fills the fp64 scratch work_dev (swn_bap_work_bytes for the same entries; 8-byte aligned) with y_b over the samples each
 * entry's frame range spans, in tiles of SWN_BAP_TILE samples; one runs a block per frame.  No atomics, no host copy, no
 * synchronisation.  The kernels read nothing outside [t0, t0 + n_avail).
 * SWN_E_BADARG, found on the host before anything is launched, text in swn_last_error_detail: everything swn_f0 refuses;
 * n_bands, n_taps (even counts included), band_win or floor out of range; a null taps_dev or work_dev; a frame range whose
 * in-signal samples, INCLUDING the c samples on either side, are not all in the window; a frame range that needs samples past
 * the window while len is -1.  Entries with f1 == f0 do nothing; a call without any frame launches nothing.  swn_bap_reach
 * returns S + 2 c, swn_bap_work_bytes the scratch size in bytes; both return 0 for arguments the call refuses. */
#define SWN_BAP_MAX_BANDS 5
#define SWN_BAP_MAX_TAPS 255
#define SWN_BAP_TILE 1280
int    swn_bap_reach(int win, int lag_hi, int n_taps);
size_t swn_bap_work_bytes(int hop, int win, int lag_hi, int n_bands, const swn_logmel_entry* entries_host, int n_entries);
int    swn_bap(double fs, int hop, int win, int lag_lo, int lag_hi, double threshold, int band_win, int n_bands, int n_taps,
               const double* taps_dev, float floor, const swn_logmel_entry* entries_host, int n_entries, void* work_dev,
               void* stream);

/* ---- spectral envelope by F0-adaptive smoothing, and its mel-cepstrum (melspec.SpectralEnvelopeExtractor; csrc/swn_envelope.hip) ---
 * The envelope swn_mcep does not compute: a frame is analysed under a window of three pitch periods and its power spectrum
 * smoothed over 2 f0 / 3, so the harmonics are not in it.  It is CheapTrick's procedure (Morise 2015) in a fixed arithmetic; it
 * omits WORLD's added noise and its eps and has a floor instead.  Parity with pyworld / pysptk is neither claimed nor pinned.
 * The definition (melspec.py restates it, tests/envelope_ref.py pins it).  fs > 0; n_fft a multiple of 32 in [32,
 * SWN_SPECTRAL_MAX_FFT]; 1 <= hop <= SWN_F0_MAX_HOP; 0 <= order <= min(SWN_MCEP_MAX_ORDER, n_fft / 2); floor > 0, an amplitude,
 * fp32; q1 (CheapTrick's -0.15); default_f0.  With D = fs / n_fft and f0_floor = 3 fs / (n_fft - 3) the call needs f0_floor <
 * default_f0 <= fs / 4 (fs 8 000 needs n_fft >= 64, 22 050 needs 160).  Input: len >= 1 finite fp32 samples, x[t] = 0 outside
 * [0, len) (zero padding, as swn_f0); F = 1 + len / hop frames on the grid of the other extractors; one fp32 value f0[f] per frame,
 * any number (column 0 of swn_f0 is the intended source).  Everything below is IEEE double in the order written; every sum is one
 * chain in ascending index from +0.0 with fma; each output value is rounded once to fp32.
 *   1. f0e = (double)f0[f] if f0_floor < f0[f] <= fs / 4, else default_f0: unvoiced 0.0, NaN and values outside take the default
 *   2. hl = floor(1.5 fs / f0e + 0.5), so 2 hl + 1 <= n_fft - 1; w[k] = 0.5 cos(pi k f0e / (1.5 fs)) + 0.5 for k = -hl .. hl;
 *      w /= sqrt(sum w^2); xw[k] = x[f hop + k] w[k]; then xw[k] -= w[k] (sum xw / sum w) with the normalised w
 *   3. P[b] = |sum_k xw[k] e^(-2 pi i b (k + hl) / n_fft)|^2 = re^2 + im^2, b = 0 .. n_fft / 2; the twiddle of sample j = k + hl is
 *      T[(b j) mod n_fft] for re and T[(b j + n_fft / 4) mod n_fft] for im, T[m] = cos(2 pi m / n_fft) the host's fp64 table
 *   4. DC correction from the uncorrected P: for b = 0 .. floor(f0e / D): u = f0e / D - b, i = floor(u),
 *      P'[b] = (P[b] + P[i]) + (u - i)(P[i + 1] - P[i]); P' = P elsewhere
 *   5. box smoothing of width wd = 2 f0e / 3 over the spectrum as one rectangle of width D per bin, mirrored at 0 and Nyquist:
 *      S[b] = (1 / wd) sum_n ov(n) P'[mir(n)], n ascending from floor((b D - wd / 2) / D + 0.5) to floor((b D + wd / 2) / D + 0.5),
 *      ov(n) = min(b D + wd / 2, (n + 0.5) D) - max(b D - wd / 2, (n - 0.5) D), terms with ov <= 0 skipped,
 *      mir(n) = -n for n < 0, n_fft - n for n > n_fft / 2, else n
 *   6. L[b] = ln max(S[b], floor^2)
 *   7. v[k] = (1 / n_fft) sum_b e_b L[b] T[(k b) mod n_fft], k = 0 .. n_fft / 2, e = 1 at 0 and n_fft / 2 and 2 between (irfft);
 *      l_s[0] = 1, l_s[k] = sin(x) / x with x = pi f0e k / fs; l_c[k] = (1 - 2 q1) + 2 q1 cos(2 pi k f0e / fs);
 *      ct[k] = v[k] l_s[k] l_c[k]
 *   8. what = SWN_ENVELOPE_MCEP: the one-sided cepstrum of the log AMPLITUDE envelope, c[0] = ct[0] / 2, c[k] = ct[k], c[n_fft / 2]
 *      = ct[n_fft / 2] / 2, then mc[m] = sum_k G[m][k] c[k], G the fp64 matrix (order + 1, n_fft / 2 + 1) of SPTK's freqt on the
 *      unit vectors (alpha exists only in how the caller built G); frame f, coefficient m at out_dev + (f - f0) (order + 1) + m.
 *      what = SWN_ENVELOPE_LOGAMP: E[b] = 0.5 sum_k e_k ct[k] T[(k b) mod n_fft], ln of the amplitude envelope, n_fft / 2 + 1
 *      values per frame.
 * A frame's values depend on the signal, the frame index and that frame's f0 value alone - not on the batch, the entry, the
 * frame range, the window or the call: any partition gives the same bits.  Streaming rule (melspec.envelope_frames_ready is the
 * one place it is written): frame f is computable iff f hop + n_fft / 2 <= n_received, or when the signal has ended.
 * tables_dev (swn_envelope_table_doubles doubles): T, then G row by row.  Entries follow the rules of swn_logmel_entry (a HOST
 * table of at most SWN_LOGMEL_MAX_ENTRIES, carried in the launch arguments; no read outside [t0, t0 + n_avail); len may be -1
 * while unknown); f0_dev addresses the F0 of frame f0 of the range, f1 - f0 floats.  One launch, a block per frame, the frame's
 * vectors in LDS; work_dev (swn_envelope_work_bytes, 8-byte aligned) is reserved scratch.
 * SWN_E_BADARG, found on the host before anything is launched, text in swn_last_error_detail: every rule above, what not 0 / 1,
 * a null pointer, n_entries out of range, a non-zero reserved field, len < 1 or > 2^30, a window that leaves the signal, f0 < 0,
 * f1 < f0, f1 > F, a frame whose span [f hop - (n_fft / 2 - 1), f hop + n_fft / 2) leaves the window where it lies inside the
 * signal, or reaches past the window while len is -1, more than 2^24 frames in one call.  Entries with f1 == f0 do nothing and may
 * carry null pointers; a call without any frame launches nothing.  The size queries return 0 for arguments the call refuses.
 * sizeof(swn_envelope_entry) == 48. */
typedef struct swn_envelope_entry {
    const float* wav_dev;      /* sample t0 of this row */
    float*       out_dev;      /* frame f0 of this row's output, (f1 - f0) * columns floats */
    const float* f0_dev;       /* F0 in Hz of frame f0 of this row, f1 - f0 floats */
    int32_t t0;                /* absolute index of the first available sample, >= 0 */
    int32_t n_avail;           /* samples available from t0 on */
    int32_t len;               /* total length of the row, or -1: not known yet */
    int32_t f0, f1;            /* frames to compute, 0 <= f0 <= f1 */
    int16_t reserved;          /* 0 */
    int16_t reserved2;         /* 0 */
} swn_envelope_entry;
#define SWN_ENVELOPE_MCEP 0
#define SWN_ENVELOPE_LOGAMP 1
size_t swn_envelope_table_doubles(int n_fft, int order);
size_t swn_envelope_work_bytes(int n_fft, int hop, const swn_envelope_entry* entries_host, int n_entries);
int    swn_envelope(double fs, int n_fft, int hop, int order, float floor, double q1, double default_f0, int what,
                    const double* tables_dev, const swn_envelope_entry* entries_host, int n_entries, void* work_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWN_HIP_H */
