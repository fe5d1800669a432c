// Stage-1 low cut on the device (swn_lowcut_chunk of include/swn_hip.h; melspec.LowCut): the causal FIR high-pass of run.sh
// stage 1 (feature_extract.py low_cut_filter; host version dsp.low_cut_filter) as a resumable call of its own, with the
// arithmetic of the last stage of postfilter_kernel - one fp64 fma chain over the taps in ascending order, rounded once to
// fp32 (swn_lowcut.hpp).
//
// Two launches per group of at most SWN_LOWCUT_MAX_ENTRIES entries.  lowcut_kernel: blocks cover (entry, tile of LC_TILE
// outputs), so a long utterance is spread over the device; a block puts the taps and its tile's inputs behind the n_taps - 1
// samples before them (from the chunk, or from the slot's state for the first tile) into LDS and writes its outputs.  It
// writes no state: every tile of an entry may read the slot, in any order.  lowcut_state_kernel, stream-ordered behind it,
// one block per entry: thread i picks up float i of the new state - a chunk sample, or for a chunk shorter than the state a
// float of the old state further up - and after a barrier writes it.  The slots of a call are distinct, so the groups of a
// long table do not meet either.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "swn_lowcut.hpp"

namespace {

struct LcTable {
    swn_lowcut_entry e[SWN_LOWCUT_MAX_ENTRIES];
    int tile0[SWN_LOWCUT_MAX_ENTRIES];      // first block of each entry
    int n_entries;
};
static_assert(sizeof(swn_lowcut_entry) == 32, "swn_lowcut_entry is 32 bytes (include/swn_hip.h)");
static_assert(sizeof(LcTable) + 4 * sizeof(void*) <= 4096, "the by-value kernel arguments must stay inside 4 KB");

__global__ __launch_bounds__(LC_THREADS) void lowcut_kernel(const LcTable t, const double* __restrict__ taps,
                                                            const float* __restrict__ state, int n_taps) {
    __shared__ LcShared s;
    int ei = 0;
    for (int i = 1; i < t.n_entries; ++i)           // the last entry whose first tile is not past this block (empty ones share
        if (t.tile0[i] <= (int)blockIdx.x) ei = i;  // their tile0 with the next entry, which wins)
    const swn_lowcut_entry& en = t.e[ei];
    const int base = ((int)blockIdx.x - t.tile0[ei]) * LC_TILE;
    const int cnt = en.n - base < LC_TILE ? en.n - base : LC_TILE;
    const float* hist = (en.flags & SWN_LOWCUT_RESET) ? nullptr : state + (size_t)en.slot * (n_taps - 1);
    lc_load_taps(s, taps, n_taps);
    lc_load_tile(s, en.in_dev, en.n, hist, n_taps, base);
    __syncthreads();
    lc_fir_tile(s, n_taps, cnt, en.out_dev + base);
}

__global__ __launch_bounds__(LC_THREADS) void lowcut_state_kernel(const LcTable t, float* state, int n_taps) {
    const swn_lowcut_entry& en = t.e[blockIdx.x];
    const bool reset = (en.flags & SWN_LOWCUT_RESET) != 0;
    if (en.n == 0 && !reset) return;
    const int H = n_taps - 1, i = threadIdx.x;
    float* st = state + (size_t)en.slot * H;
    const float v = i < H ? lc_next_hist(en.in_dev, en.n, reset ? nullptr : st, n_taps, i) : 0.f;
    __syncthreads();                                // the old state is read whole before any of it is replaced
    if (i < H) st[i] = v;
}

int lc_fail(const char* what) {
    swn_set_error_detail("swn_lowcut_chunk", what);
    return SWN_E_BADARG;
}

}  // namespace

extern "C" size_t swn_lowcut_state_floats(int n_taps) { return lc_taps_ok(n_taps) ? (size_t)(n_taps - 1) : 0; }

extern "C" int swn_lowcut_chunk(int n_taps, const double* taps_dev, float* state_dev, int capacity,
                                const swn_lowcut_entry* entries_host, int n_entries, void* stream) {
    char msg[160];
    if (!lc_taps_ok(n_taps)) return lc_fail("n_taps outside [1, SWN_LOWCUT_MAX_TAPS]");
    if (!taps_dev || !state_dev) return lc_fail("null pointer (taps_dev, state_dev)");
    if (capacity < 1) return lc_fail("capacity < 1");
    if (n_entries < 0) return lc_fail("n_entries < 0");
    if (n_entries > 0 && !entries_host) return lc_fail("entries_host is NULL");
    std::vector<unsigned char> used((size_t)capacity, 0);
    for (int e = 0; e < n_entries; ++e) {
        const swn_lowcut_entry& en = entries_host[e];
        if (en.slot < 0 || en.slot >= capacity) {
            snprintf(msg, sizeof msg, "entry %d: slot %d outside [0, %d)", e, en.slot, capacity);
            return lc_fail(msg);
        }
        if (used[en.slot]) {
            snprintf(msg, sizeof msg, "entry %d: slot %d is named twice: a slot takes one entry per call", e, en.slot);
            return lc_fail(msg);
        }
        used[en.slot] = 1;
        if (en.n < 0) { snprintf(msg, sizeof msg, "entry %d: n = %d", e, en.n); return lc_fail(msg); }
        if ((en.flags & ~SWN_LOWCUT_RESET) != 0) { snprintf(msg, sizeof msg, "entry %d: unknown flag %d", e, en.flags); return lc_fail(msg); }
        if (en.reserved != 0) { snprintf(msg, sizeof msg, "entry %d: reserved field is not 0", e); return lc_fail(msg); }
        if (en.n > 0) {
            if (!en.in_dev || !en.out_dev) { snprintf(msg, sizeof msg, "entry %d: null pointer", e); return lc_fail(msg); }
            const uintptr_t a = reinterpret_cast<uintptr_t>(en.in_dev), b = reinterpret_cast<uintptr_t>(en.out_dev);
            const uintptr_t bytes = (uintptr_t)en.n * sizeof(float);
            if (a < b + bytes && b < a + bytes) {
                snprintf(msg, sizeof msg, "entry %d: the in_dev and out_dev ranges overlap (other tiles read what one writes)", e);
                return lc_fail(msg);
            }
        }
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    for (int e0 = 0; e0 < n_entries; e0 += SWN_LOWCUT_MAX_ENTRIES) {
        const int ne = n_entries - e0 < SWN_LOWCUT_MAX_ENTRIES ? n_entries - e0 : SWN_LOWCUT_MAX_ENTRIES;
        LcTable t;
        int tiles = 0;                              // at most 64 * 2^21
        bool touches = false;
        for (int e = 0; e < SWN_LOWCUT_MAX_ENTRIES; ++e) {
            t.e[e] = e < ne ? entries_host[e0 + e] : swn_lowcut_entry{nullptr, nullptr, 0, 0, 0, 0};
            t.tile0[e] = tiles;
            tiles += (int)(((long long)t.e[e].n + LC_TILE - 1) / LC_TILE);
            touches = touches || t.e[e].n > 0 || (t.e[e].flags & SWN_LOWCUT_RESET) != 0;
        }
        t.n_entries = ne;
        if (tiles > 0) {
            hipLaunchKernelGGL(lowcut_kernel, dim3((unsigned)tiles), dim3(LC_THREADS), 0, st, t, taps_dev, state_dev, n_taps);
            const int rc = swn_launch_status("swn_lowcut_chunk");
            if (rc != SWN_OK) return rc;
        }
        if (touches && n_taps > 1) {
            hipLaunchKernelGGL(lowcut_state_kernel, dim3((unsigned)ne), dim3(LC_THREADS), 0, st, t, state_dev, n_taps);
            const int rc = swn_launch_status("swn_lowcut_chunk (state)");
            if (rc != SWN_OK) return rc;
        }
    }
    return SWN_OK;
}
