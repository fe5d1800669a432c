// Rational resampler on the device (swn_resample_chunk of include/swn_hip.h, which states the definition; melspec.Resampler):
// output n of a session reads the polyphase row r = (n M + D) mod L against the inputs i0, i0 - 1, ... i0 - (Q - 1),
// i0 = (n M + D) div L - one fp64 fma chain over q ascending, rounded once to fp32, the arithmetic of swn_lowcut_chunk.
//
// Two launches per group of at most SWN_RESAMPLE_MAX_ENTRIES entries.  resample_kernel: blocks cover (entry, tile of RS_TILE
// outputs).  A block puts the input span its tile reads - absolute indices [i0(first) - (Q - 1), i0(last)], from the chunk, from
// the slot's state below the chunk's first sample, zero outside the signal - into LDS and writes its outputs; thread t runs the
// chains of outputs t, t + 256, ... side by side.  The table stays in global memory: a thread walks its row q ascending (one
// cache line serves 8 steps), neighbouring outputs read rows M apart (mod L), and the whole table (at most ~70 KB with the
// default design) is shared by every block through the caches.  The launch writes no state: every tile of an entry may read the
// slot, in any order.  resample_state_kernel, stream-ordered behind it, one block per entry: thread i picks up float i of the new
// state - a chunk sample, or for a chunk shorter than the state a float of the old state further up - and after a barrier writes
// it.  The slots of a call are distinct, so the groups of a long table do not meet either.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "swn_geom.hpp"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = SWN_RESAMPLE_TILE;
constexpr int RS_PER_THREAD = RS_TILE / RS_THREADS;
static_assert(RS_TILE % RS_THREADS == 0, "a thread runs RS_TILE / RS_THREADS chains");
static_assert(SWN_RESAMPLE_MAX_Q - 1 <= RS_THREADS, "one thread per float of a slot's state");

struct RsTable {
    swn_resample_entry e[SWN_RESAMPLE_MAX_ENTRIES];
    int tile0[SWN_RESAMPLE_MAX_ENTRIES];    // first block of each entry
    int n_entries;
};
static_assert(sizeof(swn_resample_entry) == 56, "swn_resample_entry is 56 bytes (include/swn_hip.h)");
static_assert(sizeof(RsTable) + 2 * sizeof(void*) + 4 * sizeof(int) <= 4096, "the by-value kernel arguments must stay inside 4 KB");

// input sample `a` (absolute index) as entry `en` sees it: zero outside the signal, the chunk from in0 on, the slot's state
// (its Q - 1 floats `st`, oldest first; never read by a session that starts at in0 == 0) below it
__device__ __forceinline__ float rs_input(const swn_resample_entry& en, const float* __restrict__ st, int H, long long a) {
    if (a < 0 || (en.len >= 0 && a >= en.len)) return 0.f;
    const long long j = a - en.in0;
    if (j >= 0) return j < en.n_in ? en.in_dev[j] : 0.f;
    return j + H >= 0 ? st[j + H] : 0.f;            // in0 > 0 here; the host refused a tile that reads below the state
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const RsTable t, const double* __restrict__ table,
                                                              const float* __restrict__ state, int up, int down, int n_taps,
                                                              int Q) {
    __shared__ float xs[SWN_RESAMPLE_MAX_SPAN];
    int ei = 0;
    for (int i = 1; i < t.n_entries; ++i)           // the last entry whose first tile is not past this block (entries without
        if (t.tile0[i] <= (int)blockIdx.x) ei = i;  // outputs share their tile0 with the next entry, which wins)
    const swn_resample_entry& en = t.e[ei];
    const int base = ((int)blockIdx.x - t.tile0[ei]) * RS_TILE;
    const int cnt = en.n_out - base < RS_TILE ? en.n_out - base : RS_TILE;
    const int H = Q - 1, tid = threadIdx.x;
    // the tile's first output: p0 = n M + D in 64-bit; output k of the tile has p = p0 + k M, and r0 + k M fits 32 bits
    const long long p0 = (en.out0 + base) * (long long)down + (n_taps - 1) / 2;
    const long long i00 = p0 / up;
    const int r0 = (int)(p0 - i00 * up);
    const long long lo = i00 - H;                   // absolute index of xs[0]
    const int span = (r0 + (cnt - 1) * down) / up + Q;      // <= ceil(RS_TILE down / up) + Q <= SWN_RESAMPLE_MAX_SPAN
    const float* st = state + (size_t)en.slot * H;
    for (int i = tid; i < span; i += RS_THREADS) xs[i] = rs_input(en, st, H, lo + i);
    __syncthreads();
    if (tid >= cnt) return;                         // outputs tid + 256 u lie further still
    double acc[RS_PER_THREAD];
    const double* row[RS_PER_THREAD];
    const float* x[RS_PER_THREAD];
#pragma unroll
    for (int u = 0; u < RS_PER_THREAD; ++u) {
        // a chain past cnt repeats the tile's last output: it reads inside the span and its result is dropped
        const int k = tid + u * RS_THREADS < cnt ? tid + u * RS_THREADS : cnt - 1;
        const int w = r0 + k * down;
        acc[u] = 0.0;
        row[u] = table + (size_t)(w % up) * Q;
        x[u] = xs + w / up + H;                     // x[i0]; the chain reads x[i0 - q]
    }
    for (int q = 0; q < Q; ++q) {
#pragma unroll
        for (int u = 0; u < RS_PER_THREAD; ++u) acc[u] = fma(row[u][q], (double)x[u][-q], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < RS_PER_THREAD; ++u)
        if (tid + u * RS_THREADS < cnt) en.out_dev[base + tid + u * RS_THREADS] = static_cast<float>(acc[u]);
}

__global__ __launch_bounds__(RS_THREADS) void resample_state_kernel(const RsTable t, float* state, int Q) {
    const swn_resample_entry& en = t.e[blockIdx.x];
    if (en.n_in == 0) return;                       // the last Q - 1 inputs are the ones they were
    const int H = Q - 1, i = threadIdx.x;
    float* st = state + (size_t)en.slot * H;
    float v = 0.f;
    if (i < H) {
        const int j = en.n_in - H + i;              // chunk sample that lands on float i
        if (j >= 0) v = en.in_dev[j];
        else if (en.in0 > 0) v = st[en.n_in + i];   // n_in + i < H: the old state, shifted
    }
    __syncthreads();                                // the old state is read whole before any of it is replaced
    if (i < H) st[i] = v;
}

int rs_gcd(int a, int b) {
    while (b) { const int c = a % b; a = b; b = c; }
    return a;
}

// nullptr when (up, n_taps) describe a table this library takes, else what is wrong
const char* rs_table_why(int up, int n_taps) {
    if (up < 1) return "up < 1";
    if (up > SWN_RESAMPLE_MAX_UP) return "up beyond SWN_RESAMPLE_MAX_UP";
    if (n_taps < 1 || n_taps > SWN_RESAMPLE_MAX_TAPS) return "n_taps outside [1, SWN_RESAMPLE_MAX_TAPS]";
    if (n_taps % 2 == 0) return "n_taps is even (the filter's delay (n_taps - 1) / 2 must be whole)";
    if ((n_taps + up - 1) / up > SWN_RESAMPLE_MAX_Q) return "Q = ceil(n_taps / up) beyond SWN_RESAMPLE_MAX_Q";
    return nullptr;
}

const char* rs_ratio_why(int up, int down, int n_taps) {
    if (down < 1) return "down < 1";
    if (const char* why = rs_table_why(up, n_taps)) return why;
    if (rs_gcd(up, down) != 1) return "up and down are not coprime";
    const long long span = ((long long)RS_TILE * down + up - 1) / up + (n_taps + up - 1) / up;
    if (span > SWN_RESAMPLE_MAX_SPAN) return "a tile's input span ceil(SWN_RESAMPLE_TILE down / up) + Q beyond SWN_RESAMPLE_MAX_SPAN";
    return nullptr;
}

int rs_fail(const char* what) {
    swn_set_error_detail("swn_resample_chunk", what);
    return SWN_E_BADARG;
}

}  // namespace

extern "C" size_t swn_resample_table_doubles(int up, int down, int n_taps) {
    return rs_ratio_why(up, down, n_taps) ? 0 : (size_t)up * (size_t)((n_taps + up - 1) / up);
}

extern "C" size_t swn_resample_state_floats(int up, int n_taps) {
    return rs_table_why(up, n_taps) ? 0 : (size_t)((n_taps + up - 1) / up - 1);
}

extern "C" int swn_resample_chunk(int up, int down, int n_taps, const double* table_dev, float* state_dev, int capacity,
                                  const swn_resample_entry* entries_host, int n_entries, void* stream) {
    char msg[200];
    if (const char* why = rs_ratio_why(up, down, n_taps)) return rs_fail(why);
    if (!table_dev || !state_dev) return rs_fail("null pointer (table_dev, state_dev)");
    if (capacity < 1) return rs_fail("capacity < 1");
    if (n_entries < 0) return rs_fail("n_entries < 0");
    if (n_entries > 0 && !entries_host) return rs_fail("entries_host is NULL");
    const int Q = (n_taps + up - 1) / up;
    const long long D = (n_taps - 1) / 2, L = up, M = down;
    const long long in_max = INT64_MAX / L - 1, out_max = (INT64_MAX - D) / M - 1;    // n L and n M + D stay inside 64 bits
    std::vector<unsigned char> used((size_t)capacity, 0);
    for (int e = 0; e < n_entries; ++e) {
        const swn_resample_entry& en = entries_host[e];
        if (en.slot < 0 || en.slot >= capacity) {
            snprintf(msg, sizeof msg, "entry %d: slot %d outside [0, %d)", e, en.slot, capacity);
            return rs_fail(msg);
        }
        if (used[en.slot]) {
            snprintf(msg, sizeof msg, "entry %d: slot %d is named twice: a slot takes one entry per call", e, en.slot);
            return rs_fail(msg);
        }
        used[en.slot] = 1;
        if (en.n_in < 0 || en.n_out < 0 || en.in0 < 0 || en.out0 < 0 || en.len < -1) {
            snprintf(msg, sizeof msg, "entry %d: negative count (n_in %d, n_out %d, in0 %lld, out0 %lld, len %lld)", e, en.n_in,
                     en.n_out, (long long)en.in0, (long long)en.out0, (long long)en.len);
            return rs_fail(msg);
        }
        if (en.in0 > in_max - en.n_in || en.out0 > out_max - en.n_out || en.len > in_max) {
            snprintf(msg, sizeof msg, "entry %d: an index too large for the 64-bit arithmetic of n up and n down + D", e);
            return rs_fail(msg);
        }
        if (en.reserved != 0) { snprintf(msg, sizeof msg, "entry %d: reserved field is not 0", e); return rs_fail(msg); }
        if ((en.n_in > 0 && !en.in_dev) || (en.n_out > 0 && !en.out_dev)) {
            snprintf(msg, sizeof msg, "entry %d: null pointer (in_dev with n_in > 0, out_dev with n_out > 0)", e);
            return rs_fail(msg);
        }
        if (en.n_in > 0 && en.n_out > 0) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(en.in_dev), b = reinterpret_cast<uintptr_t>(en.out_dev);
            if (a < b + (uintptr_t)en.n_out * sizeof(float) && b < a + (uintptr_t)en.n_in * sizeof(float)) {
                snprintf(msg, sizeof msg, "entry %d: the in_dev and out_dev ranges overlap (other tiles read what one writes)", e);
                return rs_fail(msg);
            }
        }
        const long long end = en.in0 + en.n_in;     // inputs received after this chunk
        if (en.len >= 0 && en.len != end) {
            snprintf(msg, sizeof msg, "entry %d: len %lld is given but in0 + n_in = %lld: the signal ends with the chunk that "
                     "states its length", e, (long long)en.len, end);
            return rs_fail(msg);
        }
        if (en.n_out > 0) {
            const long long last = en.out0 + en.n_out - 1;
            if (en.len < 0 && (last * M + D) / L > end - 1) {
                snprintf(msg, sizeof msg, "entry %d: output %lld is not computable: it reads input %lld, %lld have arrived and "
                         "len is unknown", e, last, (last * M + D) / L, end);
                return rs_fail(msg);
            }
            if (en.len >= 0 && last >= (en.len * L + M - 1) / M) {
                snprintf(msg, sizeof msg, "entry %d: output %lld is not computable: a signal of %lld inputs has %lld outputs", e,
                         last, (long long)en.len, (en.len * L + M - 1) / M);
                return rs_fail(msg);
            }
            if ((en.out0 * M + D) / L < en.in0) {
                snprintf(msg, sizeof msg, "entry %d: output %lld reads below the state: its newest input %lld lies before in0 %lld",
                         e, (long long)en.out0, (en.out0 * M + D) / L, (long long)en.in0);
                return rs_fail(msg);
            }
        }
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    for (int e0 = 0; e0 < n_entries; e0 += SWN_RESAMPLE_MAX_ENTRIES) {
        const int ne = n_entries - e0 < SWN_RESAMPLE_MAX_ENTRIES ? n_entries - e0 : SWN_RESAMPLE_MAX_ENTRIES;
        RsTable t;
        int tiles = 0;                              // at most 64 * 2^21
        bool receives = false;
        for (int e = 0; e < SWN_RESAMPLE_MAX_ENTRIES; ++e) {
            t.e[e] = e < ne ? entries_host[e0 + e] : swn_resample_entry{nullptr, nullptr, 0, 0, -1, 0, 0, 0, 0};
            t.tile0[e] = tiles;
            tiles += (int)(((long long)t.e[e].n_out + RS_TILE - 1) / RS_TILE);
            receives = receives || t.e[e].n_in > 0;
        }
        t.n_entries = ne;
        if (tiles > 0) {
            hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles), dim3(RS_THREADS), 0, st, t, table_dev, state_dev, up, down,
                               n_taps, Q);
            const int rc = swn_launch_status("swn_resample_chunk");
            if (rc != SWN_OK) return rc;
        }
        if (receives && Q > 1) {
            hipLaunchKernelGGL(resample_state_kernel, dim3((unsigned)ne), dim3(RS_THREADS), 0, st, t, state_dev, Q);
            const int rc = swn_launch_status("swn_resample_chunk (state)");
            if (rc != SWN_OK) return rc;
        }
    }
    return SWN_OK;
}
