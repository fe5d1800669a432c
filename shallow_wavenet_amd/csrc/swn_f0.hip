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
// Lane 0 walks, refines and writes the frame's two floats.  No scratch buffer, no atomics.  The procedure is one __device__
// function, f0_frame, which the band aperiodicity kernel further down (swn_bap) runs too before its own sums.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "swn_frame_entry.hpp"
#include "swn_geom.hpp"

#pragma clang fp contract(off)      // the chains are explicit fma calls; nothing else may be fused or re-associated

namespace {

constexpr int F0_THREADS = 256;
constexpr int F0_WAVES = F0_THREADS / 64;
constexpr int F0_SIDE = 5;                              // neighbouring lags per lane
constexpr int F0_GROUP = 64 * F0_SIDE;                  // lags per wave and round
constexpr int F0_MAX_SPAN = SWN_F0_MAX_WIN + SWN_F0_MAX_LAG;
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

// The frame procedure of swn_f0, the one statement of it, for the frame of this block (F0_THREADS threads) in a call whose
// arguments A carry the entries e[], n_entries and the geometry: writes the frame's two floats to e.out + (f - e.f0) * cols.
// Thread 0 alone returns true, with the entry ei, the frame f, the decided lag tau* (on unvoiced frames too) and the voicing
// decision; the other threads return false once the procedure's last barrier is behind them.
template <class A>
__device__ __forceinline__ bool f0_frame(const A& a, int cols, int& ei_out, int& f_out, int& tau, bool& voiced) {
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
    if (tid != 0) return false;
    for (int i = 1; i < F0_WAVES; ++i) {
        first = red_first[i] < first ? red_first[i] : first;
        if (red_min[i] < mn || (red_min[i] == mn && red_arg[i] < arg)) { mn = red_min[i]; arg = red_arg[i]; }
    }
    float* o = e.out + (size_t)(f - e.f0) * cols;
    if (first == INT_MAX) {                             // unvoiced
        o[0] = 0.f;
        o[1] = static_cast<float>(mn);
        ei_out = ei; f_out = f; tau = arg; voiced = false;
        return true;
    }
    int t = first;
    while (t < a.lag_hi && dn[t + 1] < dn[t]) ++t;
    const double ym = dn[t - 1], y0 = dn[t], yp = dn[t + 1];            // t - 1 >= 1 and t + 1 <= L1
    const double den = ym - 2.0 * y0 + yp;
    const double shift = (den > 0.0 && y0 <= ym && y0 <= yp) ? 0.5 * (ym - yp) / den : 0.0;
    o[0] = static_cast<float>(a.fs / ((double)t + shift));
    o[1] = static_cast<float>(y0);
    ei_out = ei; f_out = f; tau = t; voiced = true;
    return true;
}

__global__ __launch_bounds__(F0_THREADS) void f0_kernel(const F0Args a) {
    int ei, f, tau;
    bool voiced;
    f0_frame(a, 2, ei, f, tau, voiced);
}

// ---- band aperiodicity (swn_bap of include/swn_hip.h, which states the definition; tests/bap_ref.py pins it) ---------------------
// Two launches.  bap_band_kernel fills an fp64 scratch with the band signals y_b[t] = sum_k h_b[k] x[t + c - k] of every entry with
// frames over the samples its frame range spans, [f0 hop - S / 2, (f1 - 1) hop - S / 2 + S): entry e's band b is the n_e doubles
// at work + yoff[e] + b n_e.  A block takes SWN_BAP_TILE output samples of one band: the input tile with its T - 1 halo goes to
// LDS as doubles, the taps too, and a thread runs BAP_SIDE neighbouring outputs like f0_chains runs neighbouring lags - a step
// reads the broadcast tap and ONE new sample per lane, 40 bytes apart across the lanes - so five fp64 fma stand against two LDS
// reads.  bap_frame_kernel, one block per frame, runs f0_frame and then, on voiced frames, wave w the bands w, w + 4, ..: lane l
// runs the three chains of d, e0, e1 over j = l, l + 64, .. and the 64 partials are added in lane order, so the bits depend on the
// signal and the frame alone.
constexpr int BAP_THREADS = 256;
constexpr int BAP_SIDE = 5;                             // neighbouring output samples per thread
static_assert(BAP_THREADS * BAP_SIDE == SWN_BAP_TILE, "a block's threads cover one tile");
static_assert(SWN_BAP_MAX_TAPS % 2 == 1, "odd tap counts only");

struct BapArgs {
    F0Entry e[SWN_LOGMEL_MAX_ENTRIES];
    long long yoff[SWN_LOGMEL_MAX_ENTRIES];             // doubles from work to the entry's band 0
    const double* taps;                                 // (n_bands, n_taps)
    double* work;
    double fs, threshold, floor;
    int n_entries, hop, win, lag_lo, lag_hi, band_win, n_bands, n_taps;
};
static_assert(sizeof(BapArgs) <= 4096, "the by-value kernel arguments must stay inside 4 KB");

// grid (tiles of the longest entry, bands, entries)
__global__ __launch_bounds__(BAP_THREADS) void bap_band_kernel(const BapArgs a) {
    __shared__ double xin[SWN_BAP_TILE + SWN_BAP_MAX_TAPS - 1];     // x[ylo + j0 - c + i]
    __shared__ double hs[SWN_BAP_MAX_TAPS];
    const F0Entry& e = a.e[blockIdx.z];
    if (e.f1 == e.f0) return;
    const int tid = threadIdx.x, T = a.n_taps, c = (T - 1) / 2, S = a.win + a.lag_hi + 1;
    const long long ylo = (long long)e.f0 * a.hop - S / 2, n = (long long)(e.f1 - e.f0 - 1) * a.hop + S;
    const long long j0 = (long long)blockIdx.x * SWN_BAP_TILE;
    if (j0 >= n) return;
    // x[t] = 0 outside [0, len); nothing outside the window [t0, t0 + n_avail) is read
    const long long hi = (long long)e.t0 + e.n_avail;
    for (int i = tid; i < SWN_BAP_TILE + T - 1; i += BAP_THREADS) {
        const long long t = ylo + j0 - c + i;
        const bool in = t >= e.t0 && t < hi && (e.len < 0 || t < e.len);
        xin[i] = in ? (double)e.wav[t - e.t0] : 0.0;
    }
    const double* h = a.taps + (size_t)blockIdx.y * T;
    for (int k = tid; k < T; k += BAP_THREADS) hs[k] = h[k];
    __syncthreads();

    // output o of the tile: sum_k h[k] xin[o + T - 1 - k].  Step k holds r[u] = xin[o0 + u + T - 1 - k]: r[0] is read, the others
    // are the step before's r[u - 1]
    const int o0 = BAP_SIDE * tid;
    const double* p = xin + o0 + T - 1;
    double r[BAP_SIDE], acc[BAP_SIDE];
#pragma unroll
    for (int u = 1; u < BAP_SIDE; ++u) r[u] = p[u];
#pragma unroll
    for (int u = 0; u < BAP_SIDE; ++u) acc[u] = 0.0;
#pragma unroll 5
    for (int k = 0; k < T; ++k) {
        const double hk = hs[k];
        r[0] = p[-k];
#pragma unroll
        for (int u = 0; u < BAP_SIDE; ++u) acc[u] = fma(hk, r[u], acc[u]);
#pragma unroll
        for (int u = BAP_SIDE - 1; u > 0; --u) r[u] = r[u - 1];
    }
    double* y = a.work + a.yoff[blockIdx.z] + (long long)blockIdx.y * n + j0;
#pragma unroll
    for (int u = 0; u < BAP_SIDE; ++u)
        if (j0 + o0 + u < n) y[o0 + u] = acc[u];
}

__global__ __launch_bounds__(F0_THREADS) void bap_frame_kernel(const BapArgs a) {
    __shared__ int sh[3];                               // entry, frame, tau* (-1 on an unvoiced frame)
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cols = 2 + a.n_bands;
    int ei, f, tau;
    bool voiced;
    if (f0_frame(a, cols, ei, f, tau, voiced)) { sh[0] = ei; sh[1] = f; sh[2] = voiced ? tau : -1; }
    __syncthreads();
    ei = sh[0]; f = sh[1]; tau = sh[2];
    const F0Entry& e = a.e[ei];
    float* o = e.out + (size_t)(f - e.f0) * cols + 2;
    if (tau < 0) {                                      // unvoiced: exactly 0.0
        if (tid < a.n_bands) o[tid] = 0.f;
        return;
    }
    // s_b - ylo = (f - f0) hop + S / 2 - (Wb + tau*) / 2 >= 0, and s_b + tau* + Wb <= s + S: inside the entry's n doubles
    const int Wb = a.band_win, S = a.win + a.lag_hi + 1;
    const long long n = (long long)(e.f1 - e.f0 - 1) * a.hop + S;
    const long long at = (long long)(f - e.f0) * a.hop + S / 2 - (Wb + tau) / 2;
    for (int b = w; b < a.n_bands; b += F0_WAVES) {
        const double* y = a.work + a.yoff[ei] + (long long)b * n + at;
        double d = 0.0, e0 = 0.0, e1 = 0.0;
        for (int j = lane; j < Wb; j += 64) {
            const double y0 = y[j], y1 = y[j + tau];
            const double diff = y0 - y1;
            d = fma(diff, diff, d);
            e0 = fma(y0, y0, e0);
            e1 = fma(y1, y1, e1);
        }
        double sd = 0.0, s0 = 0.0, s1 = 0.0;            // the 64 partials in lane order, the same in every lane
        for (int l = 0; l < 64; ++l) {
            sd = sd + __shfl(d, l);
            s0 = s0 + __shfl(e0, l);
            s1 = s1 + __shfl(e1, l);
        }
        if (lane == 0) {
            const double en = s0 + s1;
            const double ap = en > 0.0 ? sd / en : 1.0;
            o[b] = static_cast<float>(10.0 * log10(fmin(fmax(ap, a.floor), 1.0)));
        }
    }
}

int f0_fail(const char* who, const char* what) {
    swn_set_error_detail(who, what);
    return SWN_E_BADARG;
}

bool f0_span_ok(int win, int lag_hi) {
    return win >= SWN_F0_MIN_WIN && win <= SWN_F0_MAX_WIN && lag_hi >= 2 && lag_hi <= SWN_F0_MAX_LAG - 1;
}

bool bap_shape_ok(int n_bands, int n_taps) {
    return n_bands >= 1 && n_bands <= SWN_BAP_MAX_BANDS && n_taps >= 1 && n_taps <= SWN_BAP_MAX_TAPS && n_taps % 2 == 1;
}

// doubles of scratch an entry's band takes: the samples its frame range spans
long long bap_region(const swn_logmel_entry& e, int hop, int S) {
    return (long long)(e.f1 - e.f0 - 1) * hop + S;
}

// The checks swn_f0 and swn_bap share, in swn_f0's words: the geometry, then every entry, whose frames read c samples more on
// either side (0 for swn_f0).  Fills all SWN_LOGMEL_MAX_ENTRIES device entries and counts the frames.
int f0_check(const char* who, double fs, int hop, int win, int lag_lo, int lag_hi, double threshold,
             const swn_logmel_entry* entries_host, int n_entries, int c, F0Entry* dev, long long* n_blocks) {
    auto fail = [who](const char* what) { return f0_fail(who, what); };
    char msg[200];
    if (!(fs > 0.0) || !std::isfinite(fs)) return fail("fs must be a finite number > 0");
    if (hop < 1 || hop > SWN_F0_MAX_HOP) return fail("hop outside [1, SWN_F0_MAX_HOP]");
    if (win < SWN_F0_MIN_WIN || win > SWN_F0_MAX_WIN) return fail("win outside [16, SWN_F0_MAX_WIN]");
    if (lag_lo < 2 || lag_hi < lag_lo || lag_hi > SWN_F0_MAX_LAG - 1)
        return fail("lags: need 2 <= lag_lo <= lag_hi <= SWN_F0_MAX_LAG - 1");
    if (!(threshold > 0.0) || !(threshold <= 1.0)) return fail("threshold outside (0, 1]");
    if (!entries_host) return fail("entries_host is NULL");
    if (n_entries < 1 || n_entries > SWN_LOGMEL_MAX_ENTRIES) return fail("n_entries outside [1, SWN_LOGMEL_MAX_ENTRIES]");
    const int S = win + lag_hi + 1;
    long long blocks = 0;
    for (int i = 0; i < SWN_LOGMEL_MAX_ENTRIES; ++i) {
        F0Entry& o = dev[i];
        o.wav = nullptr; o.out = nullptr; o.t0 = o.n_avail = o.len = o.f0 = o.f1 = 0; o.blk0 = (int)blocks;
        if (i >= n_entries) continue;
        const swn_logmel_entry& e = entries_host[i];
        const int rc = frame_entry_check(e, i, hop, 1, "1 <= len", true, fail);
        if (rc == FE_EMPTY) continue;
        if (rc != SWN_OK) return rc;
        // samples the range touches: frame f covers f hop - S / 2 + (-c .. S - 1 + c); those outside [0, len) are zeros
        const long long end = (long long)e.t0 + e.n_avail;
        const long long lo = (long long)e.f0 * hop - S / 2 - c, hi = (long long)(e.f1 - 1) * hop - S / 2 + S - 1 + c;
        long long mn = lo < 0 ? 0 : lo, mx = hi;
        if (e.len == -1) {
            if (hi >= end) {
                snprintf(msg, sizeof msg, "entry %d: frames [%d, %d) need sample %lld, the window ends at %lld and the total "
                         "length is unknown", i, e.f0, e.f1, hi, end);
                return fail(msg);
            }
        } else if (mx > e.len - 1) {
            mx = e.len - 1;
        }
        if (mn <= mx && (mn < e.t0 || mx >= end)) {
            snprintf(msg, sizeof msg, "entry %d: frames [%d, %d) read samples [%lld, %lld], the window holds [%d, %lld)", i, e.f0,
                     e.f1, mn, mx, e.t0, end);
            return fail(msg);
        }
        o.wav = e.wav_dev; o.out = e.out_dev; o.t0 = e.t0; o.n_avail = e.n_avail; o.len = e.len; o.f0 = e.f0; o.f1 = e.f1;
        blocks += e.f1 - e.f0;
        if (blocks > F0_MAX_FRAMES) return fail("more than 2^24 frames in one call");
    }
    *n_blocks = blocks;
    return SWN_OK;
}

}  // namespace

extern "C" int swn_f0_span(int win, int lag_hi) {
    return f0_span_ok(win, lag_hi) ? win + lag_hi + 1 : 0;
}

extern "C" int swn_f0(double fs, int hop, int win, int lag_lo, int lag_hi, double threshold, const swn_logmel_entry* entries_host,
                      int n_entries, void* stream) {
    F0Args a;
    long long blocks = 0;
    const int rc = f0_check("swn_f0", fs, hop, win, lag_lo, lag_hi, threshold, entries_host, n_entries, 0, a.e, &blocks);
    if (rc != SWN_OK) return rc;
    if (blocks == 0) return SWN_OK;                     // no frame in any entry
    a.fs = fs; a.threshold = threshold;
    a.n_entries = n_entries; a.hop = hop; a.win = win; a.lag_lo = lag_lo; a.lag_hi = lag_hi;
    (void)hipGetLastError();
    hipLaunchKernelGGL(f0_kernel, dim3((unsigned)blocks), dim3(F0_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return swn_launch_status("swn_f0");
}

extern "C" int swn_bap_reach(int win, int lag_hi, int n_taps) {
    return f0_span_ok(win, lag_hi) && bap_shape_ok(1, n_taps) ? win + lag_hi + 1 + (n_taps - 1) : 0;
}

extern "C" size_t swn_bap_work_bytes(int hop, int win, int lag_hi, int n_bands, const swn_logmel_entry* entries_host, int n_entries) {
    if (hop < 1 || hop > SWN_F0_MAX_HOP || !f0_span_ok(win, lag_hi) || !bap_shape_ok(n_bands, 1) || !entries_host || n_entries < 1 ||
        n_entries > SWN_LOGMEL_MAX_ENTRIES)
        return 0;
    size_t doubles = 0;
    for (int i = 0; i < n_entries; ++i) {
        const swn_logmel_entry& e = entries_host[i];
        if (e.f0 < 0 || e.f1 < e.f0) return 0;
        if (e.f1 > e.f0) doubles += (size_t)n_bands * (size_t)bap_region(e, hop, win + lag_hi + 1);
    }
    return doubles * sizeof(double);
}

extern "C" int swn_bap(double fs, int hop, int win, int lag_lo, int lag_hi, double threshold, int band_win, int n_bands, int n_taps,
                       const double* taps_dev, float floor, const swn_logmel_entry* entries_host, int n_entries, void* work_dev,
                       void* stream) {
    auto fail = [](const char* what) { return f0_fail("swn_bap", what); };
    if (n_bands < 1 || n_bands > SWN_BAP_MAX_BANDS) return fail("n_bands outside [1, SWN_BAP_MAX_BANDS]");
    if (!bap_shape_ok(1, n_taps)) return fail("n_taps must be odd and in [1, SWN_BAP_MAX_TAPS]");
    if (!(floor > 0.f) || !(floor < 1.f)) return fail("floor outside (0, 1)");
    if (!taps_dev) return fail("taps_dev is NULL");
    if (!work_dev || (uintptr_t)work_dev % sizeof(double) != 0) return fail("work_dev is NULL or not aligned for doubles");
    BapArgs a;
    long long blocks = 0;
    const int rc = f0_check("swn_bap", fs, hop, win, lag_lo, lag_hi, threshold, entries_host, n_entries, (n_taps - 1) / 2, a.e,
                            &blocks);
    if (rc != SWN_OK) return rc;
    if (band_win < SWN_F0_MIN_WIN || band_win > win) return fail("band_win outside [SWN_F0_MIN_WIN, win]");
    if (blocks == 0) return SWN_OK;                     // no frame in any entry
    const int S = win + lag_hi + 1;
    long long at = 0, longest = 0;
    for (int i = 0; i < SWN_LOGMEL_MAX_ENTRIES; ++i) {
        a.yoff[i] = at;
        if (i >= n_entries || entries_host[i].f1 == entries_host[i].f0) continue;
        const long long n = bap_region(entries_host[i], hop, S);
        at += n_bands * n;
        longest = n > longest ? n : longest;
    }
    a.taps = taps_dev; a.work = static_cast<double*>(work_dev);
    a.fs = fs; a.threshold = threshold; a.floor = (double)floor;
    a.n_entries = n_entries; a.hop = hop; a.win = win; a.lag_lo = lag_lo; a.lag_hi = lag_hi;
    a.band_win = band_win; a.n_bands = n_bands; a.n_taps = n_taps;
    const long long tiles = (longest + SWN_BAP_TILE - 1) / SWN_BAP_TILE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(bap_band_kernel, dim3((unsigned)tiles, (unsigned)n_bands, (unsigned)n_entries), dim3(BAP_THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    hipLaunchKernelGGL(bap_frame_kernel, dim3((unsigned)blocks), dim3(F0_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return swn_launch_status("swn_bap");
}

