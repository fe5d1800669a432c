// Library-internal interface between the decode dispatcher (swn_decode.hip) and the kernel files it hands a call to: the
// record of one checked call, and per kernel file one run function that takes it.  The functions have C++ linkage, so a
// declaration that drifted from its definition does not link; every file that defines one of them includes this header.
#pragma once
#include <hip/hip_runtime.h>
#include "swn_geom.hpp"
#include "swn_noise.hpp"
#include "swn_pool.hpp"

// the noise source of a call: the caller's stream / dump / generator key and utterance ids (include/swn_hip.h) ...
static inline SwnNoise swn_noise_of(const swn_decode_io* io) {
    SwnNoise nz;
    nz.ptr = io->noise_dev; nz.dump = io->noise_out_dev;
    nz.key0 = (uint32_t)(io->rng_seed & 0xffffffffu); nz.key1 = (uint32_t)(io->rng_seed >> 32);
    nz.utt0 = io->rng_utt0; nz.ids = io->rng_utt_ids_dev;
    return nz;
}
// ... and of a pool, which draws its noise on the device
static inline SwnNoise swn_pool_noise_of(const swn_decode_io* io) {
    SwnNoise nz = swn_noise_of(io);
    nz.ptr = nullptr;
    return nz;
}

// storage of the streamed head matrices: of a call (SwnDecodeCall::wk), and the last template argument of the symmetric kernel
enum : int { WK_F32 = 0, WK_BF16 = 1, WK_E4M3 = 2 };

// One call of swn_decode, swn_decode_chunk, swn_decode_pool_chunk or one of their *_w16 / *_w8 / *_models forms, as the dispatcher's
// checks (swn_decode.hip) leave it: every field is valid for the kernel the call resolved to, and a run function only fills
// its kernel's argument struct from it and picks the instantiation.
struct SwnDecodeCall {
    SwnGeom g;                                 // made once, by the check
    const float* packed = nullptr;             // (not read when `models` is set)
    int wk = WK_F32;                           // how the streamed head matrices are stored (WK_*: SWN_WEIGHTS_* of the ABI) ...
    const void* image = nullptr;               // ... and their image in that format (swn_pack_decode_w16 / _w8); fp32, `models`: null
    const SwnPoolModels* models = nullptr;     // a pool over several models; null: one model
    const void* const* images = nullptr;       // ... and, over a stored format, their images: SWN_POOL_MAX_MODELS of them, as models->p
    const SwnPoolTable* pool = nullptr;        // the checked entry table of a pool launch; null: not a pool
    const SwnPoolWideRow* wide = nullptr;      // a wide pool launch: its device table, written by the call's setup launches
                                               // (then pool, models, image and images are null: the rows carry them)
    const float* cond = nullptr;               // (pool: every entry has its own)
    int batch = 0;                             // utterances; pool: entries
    int capacity = 0;                          // utterances `state` holds: batch; pool: the slots of the session buffer
    int n_frames = 0;                          // (pool: every entry has its own)
    int step0 = 0, n_steps = 0;                // pool: 0 and the most steps of an entry (n_max)
    bool stream = false;                       // a chunk of a streamed decode (pools are streams); false: the one-shot decode
    bool resume = false;                       // stream: the state comes from the session, no prologue
    SwnNoise nz;
    const void* forced = nullptr;
    const void* seed = nullptr;
    float* state = nullptr;                    // the one-shot decode's state buffer, or the session
    void* out = nullptr;
    float* heads = nullptr;
    hipStream_t hip_stream = nullptr;
};

// swn_decode_bl6.hip (the symmetric BL6-class kernel; the only one that takes an `image`) and swn_decode_bl6w.hip (the
// wave-specialised form for the single-sample Laplace nets of that class).  *_session_floats: per-utterance session of a
// streamed decode, 0 = the kernel does not take the geometry.
size_t swn_decode_bl6_session_floats(const SwnGeom& g);
size_t swn_decode_bl6w_session_floats(const SwnGeom& g);
int swn_decode_bl6_run(const SwnDecodeCall& c);
int swn_decode_bl6w_run(const SwnDecodeCall& c);

// swn_decode_stepped.hip (one launch per phase of a step, for the large geometries; no pools through this record: the stepped
// pool has entry points of its own).  *_state_floats: the state buffer, which is also the session of a streamed decode.
size_t swn_decode_stepped_state_floats(const SwnGeom& g, int batch);
bool swn_decode_stepped_supported(const SwnGeom& g, int batch);
int swn_decode_stepped_run(const SwnDecodeCall& c);
