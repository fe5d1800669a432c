// Library-internal interface between the decode dispatcher (swn_decode.hip) and the kernel files it hands a call to.  The
// functions are C-linkage, so a prototype that drifted from its definition would link and misbehave at run time: every file
// that defines one of them includes this header, which makes the compiler compare the two.
#pragma once
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

extern "C" {

// swn_decode_bl6.hip (the symmetric BL6-class kernel) and swn_decode_bl6w.hip (the wave-specialised form for the
// single-sample Laplace nets of that class).  *_try: the one-shot decode, SWN_E_UNSUPPORTED when the kernel does not take
// the geometry.  *_session_floats: per-utterance session of a streamed decode (swn_decode_chunk), 0 = the kernel does not
// apply.  *_chunk: one chunk.  *_pool: one pool launch over the entry table swn_decode_pool_chunk checked; with `models`
// (swn_decode_pool_chunk_models) every entry runs its own model's weights and `packed` is not read.
int swn_decode_bl6_try(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames, int n_steps,
                       const SwnNoise* nz, const void* forced, const void* seed, void* out, float* heads, void* stream);
int swn_decode_bl6w_try(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames, int n_steps,
                        const SwnNoise* nz, const void* forced, const void* seed, void* out, float* heads, void* stream);
size_t swn_decode_bl6_session_floats(const swn_net_desc* d);
size_t swn_decode_bl6w_session_floats(const swn_net_desc* d);
int swn_decode_bl6_chunk(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames, int step0,
                         int n_steps, int resume, const SwnNoise* nz, const void* forced, const void* seed, float* sess,
                         void* out, float* heads, void* stream);
int swn_decode_bl6w_chunk(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames, int step0,
                          int n_steps, int resume, const SwnNoise* nz, const void* forced, const void* seed, float* sess,
                          void* out, float* heads, void* stream);
int swn_decode_bl6_pool(const swn_net_desc* d, const float* packed, const SwnPoolTable* t, const SwnPoolModels* models,
                        int n_entries, int n_max, const SwnNoise* nz, const void* seed, float* sess, void* out, float* heads,
                        void* stream);
int swn_decode_bl6w_pool(const swn_net_desc* d, const float* packed, const SwnPoolTable* t, const SwnPoolModels* models,
                         int n_entries, int n_max, const SwnNoise* nz, const void* seed, float* sess, void* out, float* heads,
                         void* stream);
// the symmetric kernel over the bf16 image of its streamed head matrices (w16: swn_pack_decode_w16), extended mode only
int swn_decode_bl6_w16_try(const swn_net_desc* d, const float* packed, const void* w16, const float* cond, int batch,
                           int n_frames, int n_steps, const SwnNoise* nz, const void* forced, const void* seed, void* out,
                           float* heads, void* stream);
int swn_decode_bl6_w16_chunk(const swn_net_desc* d, const float* packed, const void* w16, const float* cond, int batch,
                             int n_frames, int step0, int n_steps, int resume, const SwnNoise* nz, const void* forced,
                             const void* seed, float* sess, void* out, float* heads, void* stream);
int swn_decode_bl6_w16_pool(const swn_net_desc* d, const float* packed, const void* w16, const SwnPoolTable* t, int n_entries,
                            int n_max, const SwnNoise* nz, const void* seed, float* sess, void* out, float* heads, void* stream);

// swn_decode_stepped.hip (one launch per phase of a step, for the large geometries)
size_t swn_decode_stepped_state_floats(const swn_net_desc* d, int batch);
int swn_decode_stepped_supported(const swn_net_desc* d, int batch);
int swn_decode_stepped(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames, int n_steps,
                       const SwnNoise* nz, const void* forced, const void* seed, float* state, void* out, float* heads,
                       void* stream);
int swn_decode_stepped_chunk(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames,
                             int step0, int n_steps, int resume, const SwnNoise* nz, const void* forced, const void* seed,
                             float* sess, void* out, float* heads, void* stream);

}  // extern "C"
