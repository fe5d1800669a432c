// Decode pool (swn_decode_pool_chunk, include/swn_hip.h): one launch advances many independent streamed decodes, one
// workgroup per entry of a table that travels in the kernel arguments.  Each workgroup turns the launch-wide arguments of a
// streamed chunk into those of its own entry - one session of batch 1 - and then runs the STREAM code path unchanged.
#pragma once
#include "swn_geom.hpp"
#include "swn_noise.hpp"

// the entry table of a pool launch (64 x 32 B of kernel arguments)
struct SwnPoolTable {
    swn_decode_pool_entry e[SWN_DECODE_POOL_MAX_ENTRIES];
};
static_assert(sizeof(swn_decode_pool_entry) == 32, "swn_decode_pool_entry is 32 bytes (include/swn_hip.h)");

// Rewrites `a` - the arguments of a streamed chunk over the E entries (io rows indexed by entry, n_steps = n_max) - into those
// of entry blockIdx.x as a batch-1 chunk: conditioning, frame count, step0, resume and step count come from the entry, and
// every io pointer moves to the entry's row, so that the body runs with utterance index b = 0.  The caller moves its session
// pointer to swn_pool_slot().  The entry index is uniform over the workgroup, so its fields are scalar loads and stay in SGPRs.
// The first form takes the entry itself (a wide launch reads it from its device table), the second the table of the arguments.
// false: the entry has nothing to do (0 steps, no BEGIN) - the workgroup returns before its first barrier.
//   seg    out elements (fp32 samples | int32 classes) and seed elements per step / entry
//   width  noise values per step;  n_out  head outputs per step
template <class A>
__device__ __forceinline__ bool swn_pool_entry_args(A& a, const swn_decode_pool_entry& en, int seg, int width, int n_out) {
    const int e = blockIdx.x;
    const bool begin = (en.flags & SWN_CHUNK_BEGIN) != 0;
    if (en.n_steps == 0 && !begin) return false;
    const size_t n_max = (size_t)a.n_steps;
    a.cond = en.cond_dev;
    a.Tf = en.n_frames;
    a.step0 = en.step0;
    a.resume = begin ? 0 : 1;
    a.n_steps = en.n_steps;
    a.out = reinterpret_cast<char*>(a.out) + (size_t)e * n_max * seg * 4;
    if (a.heads) a.heads += (size_t)e * n_max * n_out;
    if (a.seed) a.seed = reinterpret_cast<const char*>(a.seed) + (size_t)e * seg * 4;
    if (a.nz.dump) a.nz.dump += (size_t)e * n_max * width;
    if (a.nz.ids) a.nz.ids += e;
    else a.nz.utt0 += (uint32_t)e;
    return true;
}
template <class A>
__device__ __forceinline__ bool swn_pool_entry_args(A& a, const SwnPoolTable& t, int seg, int width, int n_out) {
    const int e = blockIdx.x;                  // (signed, as the io rows are indexed: the code of these kernels is pinned)
    return swn_pool_entry_args(a, t.e[e], seg, width, n_out);
}

__device__ __forceinline__ int swn_pool_slot(const SwnPoolTable& t) { return t.e[blockIdx.x].slot; }

// the model table of a multi-model pool launch (swn_decode_pool_chunk_models, 192 B of kernel arguments behind the entry
// table): the workgroup of entry e reads its weights through p[of[e]].  Like the entry index, the model index is uniform over
// the workgroup, so the pointer is a scalar load and the body addresses its weights exactly as a single-model launch does.
struct SwnPoolModels {
    const float* p[SWN_POOL_MAX_MODELS];
    unsigned char of[SWN_DECODE_POOL_MAX_ENTRIES];
};
__device__ __forceinline__ const float* swn_pool_model(const SwnPoolModels& m) { return m.p[m.of[blockIdx.x]]; }
// ... and the index itself, for launches that carry a second per-model table beside p (the images of a stored format)
__device__ __forceinline__ int swn_pool_model_index(const SwnPoolModels& m) { return m.of[blockIdx.x]; }

// the checks the *_models entry points add to their single-model twins; SWN_OK or SWN_E_BADARG
// (max_models: the model table of a 64-entry launch bounds them; the rows of a wide launch carry the pointers themselves)
inline int swn_pool_models_check(const float* const* models, int n_models, const int32_t* model_of_entry, int n_entries,
                                 int max_models = SWN_POOL_MAX_MODELS) {
    if (!models || !model_of_entry || n_models < 1 || n_models > max_models) return SWN_E_BADARG;
    for (int m = 0; m < n_models; ++m)
        if (!models[m]) return SWN_E_BADARG;
    for (int e = 0; e < n_entries; ++e)
        if (model_of_entry[e] < 0 || model_of_entry[e] >= n_models) return SWN_E_BADARG;
    return SWN_OK;
}

// ---- the wide pool launch (swn_decode_pool_chunk_wide): up to SWN_DECODE_POOL_WIDE_MAX_ENTRIES entries, more than 4 KB of kernel
// arguments hold, so the table lies in device memory and the kernel arguments carry its address.  Row e is entry e with what the
// model tables of a narrow launch resolve for it: the packed buffer of its model and, over a stored format, that model's image -
// so one instantiation serves ticks over one model and over several, and no model table bounds the models of a launch.  The
// workgroup of entry blockIdx.x copies its row once, at its start and before its first store: the address is uniform and the
// table is written by an earlier launch only, so the copy is scalar loads (s_load_dword / x2 / x4 of the fields the kernel
// uses) and the fields stay in SGPRs.
struct SwnPoolWideRow {
    swn_decode_pool_entry e;
    const float* model;
    const void* image;                         // fp32: null
};
static_assert(sizeof(SwnPoolWideRow) == 48, "swn_decode_pool_wide_table_bytes is 48 bytes per entry");
__device__ __forceinline__ SwnPoolWideRow swn_pool_wide_row(const SwnPoolWideRow* __restrict__ rows) { return rows[blockIdx.x]; }

// the rows one setup launch writes from its kernel arguments (3 KB of them)
constexpr int SWN_POOL_WIDE_SETUP_ROWS = 64;
