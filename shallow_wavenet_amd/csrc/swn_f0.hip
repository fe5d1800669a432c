// F0 and voicing from waveforms (pitch.py, swn_f0 of include/swn_hip.h, which states the definition; tests/f0_ref.py pins it):
// per frame the squared-difference function d(tau) = sum_j (x[s + j] - x[s + j + tau])^2 over a window of W samples for every lag
// tau = 1 .. L1 = lag_hi + 1, its cumulative mean normalisation d'(tau) = d(tau) tau / (d(1) + .. + d(tau)), the first lag of
// [lag_lo, lag_hi] below the threshold walked down to its local minimum, and a parabolic refinement.  Everything is fp64 on fp32
// samples, every sum one chain in a fixed order, so a frame's two output values depend on the signal and the frame index alone.
//
// One block of 256 threads per frame, one launch per call.  The frame's S = W + L1 samples go to LDS as doubles (exact; zeros
// where the index leaves the signal or - never, for a call the host accepted - the entry's window), so the chains convert
// nothing.  Lanes take lags, five neighbouring ones each (lane l of a wave's group: 5 l + 1 .. 5 l + 5 above the group's base;
// wave w runs the groups of 320 lags w, w + 4, ...): five independent chains hide the latency of the fp64 fma, and of the five
// samples x[s + j + tau .. tau + 4] a step needs, four are the previous step's, kept in registers.  So a step costs a wave two LDS
// reads for five chains - xs[j], one address for the whole wave, a broadcast; and one new double per lane, 40 bytes apart across
// the lanes, which no two lanes of a 16-lane access group put on one bank (an even number of lags per lane would) - and the loop
// is bound by the fp64 pipe (ten operations per step), not by LDS.  d goes to LDS; lane 0 then adds c(tau) = c(tau - 1) + d(tau) in order (the only serial part: L1 dependent
// additions), all threads divide, and two block reductions find the first lag below the threshold and the first arg-min.
// Lane 0 walks, refines and writes the frame's two floats.  No scratch buffer, no atomics.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>

#include "swn_geom.hpp"

#pragma clang fp contract(off)      // the chains are explicit fma calls; nothing else may be fused or re-associated

namespace {

constexpr int F0_THREADS = 256;
constexpr int F0_WAVES = F0_THREADS / 64;
constexpr int F0_SIDE = 5;                              // neighbouring lags per lane
constexpr int F0_GROUP = 64 * F0_SIDE;                  // lags per wave and round
constexpr int F0_MAX_SPAN = SWN_F0_MAX_WIN + SWN_F0_MAX_LAG;
constexpr int F0_MAX_LEN = 1 << 30;
constexpr long long F0_MAX_FRAMES = 1LL << 24;          // frames (= blocks) per call

struct F0Entry {
    const float* wav;   // sample t0
    float* out;         // frame f0
    int t0, n_avail, len, f0, f1, blk0;
};
struct F0Args {
    F0Entry e[SWN_LOGMEL_MAX_ENTRIES];
    double fs, threshold;
    int n_entries, hop, win, lag_lo, lag_hi;
};
static_assert(sizeof(F0Args) <= 4096, "the by-value kernel arguments must stay inside 4 KB");

// F0_SIDE chains side by side, the lags tau .. tau + F0_SIDE - 1: step j reads the broadcast x[s + j] and ONE new sample per lane,
// x[s + j + tau + F0_SIDE - 1]; the others come down from the step before in registers (p = xs + tau)
__device__ __forceinline__ void f0_chains(const double* __restrict__ xs, const double* __restrict__ p, int W, double* acc) {
    double r[F0_SIDE];
#pragma unroll
    for (int u = 0; u < F0_SIDE - 1; ++u) r[u] = p[u];
#pragma unroll
    for (int u = 0; u < F0_SIDE; ++u) acc[u] = 0.0;
#pragma unroll 5
    for (int j = 0; j < W; ++j) {
        const double a = xs[j];
        r[F0_SIDE - 1] = p[j + F0_SIDE - 1];
#pragma unroll
        for (int u = 0; u < F0_SIDE; ++u) {
            const double diff = a - r[u];
            acc[u] = fma(diff, diff, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < F0_SIDE - 1; ++u) r[u] = r[u + 1];
    }
}

__global__ __launch_bounds__(F0_THREADS) void f0_kernel(const F0Args a) {
    // the frame, x[s + k], and zeros behind it for the lags past L1 of the last lane; c(tau) once the chains are done
    __shared__ double xs[F0_MAX_SPAN + F0_SIDE - 1];
    __shared__ double dn[SWN_F0_MAX_LAG + 1];           // d(tau), then d'(tau); [0] = d'(0) = 1
    double* cs = xs;
    __shared__ int red_first[F0_WAVES], red_arg[F0_WAVES];
    __shared__ double red_min[F0_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int ei = 0;
    for (int i = 1; i < a.n_entries; ++i)               // the last entry whose first block is not past this one (entries without
        if (a.e[i].blk0 <= (int)blockIdx.x) ei = i;     // frames share their blk0 with the next entry, which wins)
    const F0Entry& e = a.e[ei];
    const int f = e.f0 + ((int)blockIdx.x - e.blk0);
    const int W = a.win, L1 = a.lag_hi + 1, S = W + L1;
    const int s = f * a.hop - S / 2;

    // x[t] = 0 outside [0, len); nothing outside the window [t0, t0 + n_avail) is read
    const int hi = e.t0 + e.n_avail;
    for (int k = tid; k < S + F0_SIDE - 1; k += F0_THREADS) {
        const int t = s + k;
        const bool in = k < S && t >= e.t0 && t < hi && (e.len < 0 || t < e.len);
        xs[k] = in ? (double)e.wav[t - e.t0] : 0.0;
    }
    if (tid == 0) dn[0] = 1.0;
    __syncthreads();

    // lag group g holds the lags 320 g + 1 .. 320 g + 320, five neighbours per lane.  The chains of lags past L1 read the zeros
    // behind the frame and are dropped; a lane wholly past L1 runs the first lane's and stores nothing
    const int n_groups = (L1 + F0_GROUP - 1) / F0_GROUP;
    for (int g = w; g < n_groups; g += F0_WAVES) {
        const int t0 = F0_GROUP * g + F0_SIDE * lane + 1;
        double acc[F0_SIDE];
        f0_chains(xs, xs + (t0 <= L1 ? t0 : 1), W, acc);
#pragma unroll
        for (int u = 0; u < F0_SIDE; ++u)
            if (t0 + u <= L1) dn[t0 + u] = acc[u];
    }
    __syncthreads();

    if (tid == 0) {                                     // c(tau) = c(tau - 1) + d(tau), strictly in this order; the frame is dead
        double c = 0.0;
        for (int t = 1; t <= L1; ++t) {
            c = c + dn[t];
            cs[t] = c;
        }
    }
    __syncthreads();
    for (int t = 1 + tid; t <= L1; t += F0_THREADS) {
        const double c = cs[t];
        dn[t] = c > 0.0 ? (dn[t] * (double)t) / c : 1.0;
    }
    __syncthreads();

    // over [lag_lo, lag_hi]: the first lag below the threshold, and the first arg-min
    int first = INT_MAX, arg = INT_MAX;
    double mn = INFINITY;
    for (int t = a.lag_lo + tid; t <= a.lag_hi; t += F0_THREADS) {      // ascending per thread: `<` keeps the first
        const double y = dn[t];
        if (y < a.threshold && t < first) first = t;
        if (y < mn) { mn = y; arg = t; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int of = __shfl_down(first, off), oa = __shfl_down(arg, off);
        const double om = __shfl_down(mn, off);
        first = of < first ? of : first;
        if (om < mn || (om == mn && oa < arg)) { mn = om; arg = oa; }
    }
    if (lane == 0) { red_first[w] = first; red_arg[w] = arg; red_min[w] = mn; }
    __syncthreads();
    if (tid != 0) return;
    for (int i = 1; i < F0_WAVES; ++i) {
        first = red_first[i] < first ? red_first[i] : first;
        if (red_min[i] < mn || (red_min[i] == mn && red_arg[i] < arg)) { mn = red_min[i]; arg = red_arg[i]; }
    }
    float* o = e.out + (size_t)(f - e.f0) * 2;
    if (first == INT_MAX) {                             // unvoiced
        o[0] = 0.f;
        o[1] = static_cast<float>(mn);
        return;
    }
    int t = first;
    while (t < a.lag_hi && dn[t + 1] < dn[t]) ++t;
    const double ym = dn[t - 1], y0 = dn[t], yp = dn[t + 1];            // t - 1 >= 1 and t + 1 <= L1
    const double den = ym - 2.0 * y0 + yp;
    const double shift = (den > 0.0 && y0 <= ym && y0 <= yp) ? 0.5 * (ym - yp) / den : 0.0;
    o[0] = static_cast<float>(a.fs / ((double)t + shift));
    o[1] = static_cast<float>(y0);
}

int f0_fail(const char* what) {
    swn_set_error_detail("swn_f0", what);
    return SWN_E_BADARG;
}

bool f0_span_ok(int win, int lag_hi) {
    return win >= SWN_F0_MIN_WIN && win <= SWN_F0_MAX_WIN && lag_hi >= 2 && lag_hi <= SWN_F0_MAX_LAG - 1;
}

}  // namespace

extern "C" int swn_f0_span(int win, int lag_hi) {
    return f0_span_ok(win, lag_hi) ? win + lag_hi + 1 : 0;
}

extern "C" int swn_f0(double fs, int hop, int win, int lag_lo, int lag_hi, double threshold, const swn_logmel_entry* entries_host,
                      int n_entries, void* stream) {
    char msg[200];
    if (!(fs > 0.0) || !std::isfinite(fs)) return f0_fail("fs must be a finite number > 0");
    if (hop < 1 || hop > SWN_F0_MAX_HOP) return f0_fail("hop outside [1, SWN_F0_MAX_HOP]");
    if (win < SWN_F0_MIN_WIN || win > SWN_F0_MAX_WIN) return f0_fail("win outside [16, SWN_F0_MAX_WIN]");
    if (lag_lo < 2 || lag_hi < lag_lo || lag_hi > SWN_F0_MAX_LAG - 1)
        return f0_fail("lags: need 2 <= lag_lo <= lag_hi <= SWN_F0_MAX_LAG - 1");
    if (!(threshold > 0.0) || !(threshold <= 1.0)) return f0_fail("threshold outside (0, 1]");
    if (!entries_host) return f0_fail("entries_host is NULL");
    if (n_entries < 1 || n_entries > SWN_LOGMEL_MAX_ENTRIES) return f0_fail("n_entries outside [1, SWN_LOGMEL_MAX_ENTRIES]");
    const int S = win + lag_hi + 1;
    F0Args a;
    long long blocks = 0;
    for (int i = 0; i < SWN_LOGMEL_MAX_ENTRIES; ++i) {
        F0Entry& o = a.e[i];
        o.wav = nullptr; o.out = nullptr; o.t0 = o.n_avail = o.len = o.f0 = o.f1 = 0; o.blk0 = (int)blocks;
        if (i >= n_entries) continue;
        const swn_logmel_entry& e = entries_host[i];
        if (e.reserved != 0) { snprintf(msg, sizeof msg, "entry %d: reserved field is not 0", i); return f0_fail(msg); }
        if (e.f0 < 0 || e.f1 < e.f0) { snprintf(msg, sizeof msg, "entry %d: frame range [%d, %d)", i, e.f0, e.f1); return f0_fail(msg); }
        if (e.len != -1 && (e.len < 1 || e.len > F0_MAX_LEN)) {
            snprintf(msg, sizeof msg, "entry %d: length %d, need 1 <= len <= 2^30 (or -1 while unknown)", i, e.len);
            return f0_fail(msg);
        }
        if (e.t0 < 0 || e.n_avail < 0 || (long long)e.t0 + e.n_avail > F0_MAX_LEN ||
            (e.len != -1 && (long long)e.t0 + e.n_avail > e.len)) {
            snprintf(msg, sizeof msg, "entry %d: window [%d, %d + %d) is not inside the signal", i, e.t0, e.t0, e.n_avail);
            return f0_fail(msg);
        }
        if (e.f1 == e.f0) continue;
        if (!e.wav_dev || !e.out_dev) { snprintf(msg, sizeof msg, "entry %d: null pointer", i); return f0_fail(msg); }
        if (e.len != -1 && e.f1 > 1 + e.len / hop) {
            snprintf(msg, sizeof msg, "entry %d: f1 = %d, a signal of %d samples has %d frames", i, e.f1, e.len, 1 + e.len / hop);
            return f0_fail(msg);
        }
        // samples the range touches: frame f covers f hop - S / 2 + (0 .. S - 1); those outside [0, len) are zeros
        const long long end = (long long)e.t0 + e.n_avail;
        const long long lo = (long long)e.f0 * hop - S / 2, hi = (long long)(e.f1 - 1) * hop - S / 2 + S - 1;
        long long mn = lo < 0 ? 0 : lo, mx = hi;
        if (e.len == -1) {
            if (hi >= end) {
                snprintf(msg, sizeof msg, "entry %d: frames [%d, %d) need sample %lld, the window ends at %lld and the total "
                         "length is unknown", i, e.f0, e.f1, hi, end);
                return f0_fail(msg);
            }
        } else if (mx > e.len - 1) {
            mx = e.len - 1;
        }
        if (mn <= mx && (mn < e.t0 || mx >= end)) {
            snprintf(msg, sizeof msg, "entry %d: frames [%d, %d) read samples [%lld, %lld], the window holds [%d, %lld)", i, e.f0,
                     e.f1, mn, mx, e.t0, end);
            return f0_fail(msg);
        }
        o.wav = e.wav_dev; o.out = e.out_dev; o.t0 = e.t0; o.n_avail = e.n_avail; o.len = e.len; o.f0 = e.f0; o.f1 = e.f1;
        blocks += e.f1 - e.f0;
        if (blocks > F0_MAX_FRAMES) return f0_fail("more than 2^24 frames in one call");
    }
    if (blocks == 0) return SWN_OK;                     // no frame in any entry
    a.fs = fs; a.threshold = threshold;
    a.n_entries = n_entries; a.hop = hop; a.win = win; a.lag_lo = lag_lo; a.lag_hi = lag_hi;
    (void)hipGetLastError();
    hipLaunchKernelGGL(f0_kernel, dim3((unsigned)blocks), dim3(F0_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return swn_launch_status("swn_f0");
}
