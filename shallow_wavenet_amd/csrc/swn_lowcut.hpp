// The low cut's arithmetic, shared by swn_lowcut_chunk (swn_lowcut.hip) and the window update of swn_logmel_pool_lowcut
// (swn_melspec.hip): both must give a sample the same bits.  The definition is in include/swn_hip.h:
//     acc = 0.0;  for q = 0 .. n_taps - 1 ascending: acc = fma(h[q], (double)x[t - q], acc);  y[t] = (float)acc
// A block of LC_THREADS threads works on a tile of LC_TILE outputs.  Its LDS image xs holds the tile's inputs behind the
// n_taps - 1 samples before them, xs[i] = x[base - (n_taps - 1) + i], every one of its LC_HIST + LC_TILE floats filled (zeros
// past the chunk), so that the four chains a thread runs (outputs tid, tid + 256, ...) never read a float nobody wrote.
// Neighbouring lanes read neighbouring floats; the tap is one broadcast read per step.
#pragma once
#include <hip/hip_runtime.h>
#include "swn_geom.hpp"

constexpr int LC_THREADS = 256;
constexpr int LC_TILE = SWN_LOWCUT_TILE;
constexpr int LC_HIST = SWN_LOWCUT_MAX_TAPS - 1;
constexpr int LC_PER_THREAD = LC_TILE / LC_THREADS;
static_assert(LC_TILE % LC_THREADS == 0, "a thread runs LC_TILE / LC_THREADS chains");
static_assert(LC_HIST <= LC_THREADS, "one thread per float of a slot's history");

struct LcShared {
    double h[SWN_LOWCUT_MAX_TAPS];
    float xs[LC_HIST + LC_TILE];
};

__device__ __forceinline__ void lc_load_taps(LcShared& s, const double* __restrict__ taps, int n_taps) {
    for (int i = threadIdx.x; i < n_taps; i += LC_THREADS) s.h[i] = taps[i];
}

// xs of the tile that starts at chunk sample `base`: chunk samples from `in` (n of them), the samples before the chunk from
// `hist` (the slot's n_taps - 1 floats, oldest first; zero history when it is null), zeros from sample n on
__device__ __forceinline__ void lc_load_tile(LcShared& s, const float* __restrict__ in, int n, const float* hist, int n_taps,
                                             int base) {
    const int H = n_taps - 1;
    for (int i = threadIdx.x; i < H + LC_TILE; i += LC_THREADS) {
        const int j = base - H + i;                 // chunk sample; >= -H
        float v = 0.f;
        if (j >= 0) {
            if (j < n) v = in[j];
        } else if (hist) {
            v = hist[H + j];
        }
        s.xs[i] = v;
    }
}

// the tile's outputs [0, cnt) to dst, after a barrier behind lc_load_taps / lc_load_tile
__device__ __forceinline__ void lc_fir_tile(const LcShared& s, int n_taps, int cnt, float* __restrict__ dst) {
    const int H = n_taps - 1, tid = threadIdx.x;
    if (tid >= cnt) return;                         // outputs tid + 256 u lie further still
    double acc[LC_PER_THREAD];
#pragma unroll
    for (int u = 0; u < LC_PER_THREAD; ++u) acc[u] = 0.0;
    const float* x = s.xs + H + tid;
    for (int q = 0; q < n_taps; ++q) {
        const double h = s.h[q];
#pragma unroll
        for (int u = 0; u < LC_PER_THREAD; ++u) acc[u] = fma(h, (double)x[u * LC_THREADS - q], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < LC_PER_THREAD; ++u)
        if (tid + u * LC_THREADS < cnt) dst[tid + u * LC_THREADS] = static_cast<float>(acc[u]);
}

// float i of a slot's history after a chunk of n samples: the last n_taps - 1 raw samples, the old history shifted where the
// chunk is shorter than it (zero history when hist is null).  The caller puts a barrier between every thread's call of this
// and the first write of the slot.
__device__ __forceinline__ float lc_next_hist(const float* __restrict__ in, int n, const float* hist, int n_taps, int i) {
    const int H = n_taps - 1, j = n - H + i;        // chunk sample that lands on float i
    if (j >= 0) return in[j];
    return hist ? hist[n + i] : 0.f;                // n + i < H
}

inline bool lc_taps_ok(int n_taps) { return n_taps >= 1 && n_taps <= SWN_LOWCUT_MAX_TAPS; }
