// Spectral envelope by F0-adaptive smoothing and its mel-cepstrum (melspec.SpectralEnvelopeExtractor, swn_envelope of
// include/swn_hip.h, which states the definition; tests/envelope_ref.py pins it): CheapTrick's procedure in a fixed arithmetic.
// Per frame: a Hann window of three pitch periods, the power spectrum by a direct DFT over the window's 2 hl + 1 samples, the DC
// correction, a box smoothing of width 2 f0 / 3, the log, and a liftering in the cepstral domain; then either the frequency
// transform to a mel-cepstrum or the cosine sum back to the log amplitude.  Everything is fp64 on fp32 samples; every sum is one
// fma chain in ascending index from +0.0, so a frame's values depend on the signal, the frame index and the frame's F0 alone.
//
// One block per frame, one launch per call.  The frame's vectors live in LDS as doubles: T (first the window, then the cos table,
// each row of 32 padded by one double so that the strided reads of the transforms spread over the banks), xw (the windowed
// samples), and three vectors of bins + 1 that the steps hand on: A (P), B (P', later the cepstrum the output step reads), C (the
// weighted log).  The three sums of the window step are serial by definition (one thread each; sum xw and sum w run in two waves
// at once); in every other step a thread owns whole output values and runs two chains side by side.  The freqt matrix is read
// through L2.  No scratch buffer, no atomics.  Measured at 8 % of the fp64 vector rate: a chain step is one fma
// against one gathered LDS read and the integer work of walking (i + b) mod n_fft through the padded table, which is what a
// faster version would have to take out (a table of (cos, -sin) pairs read as one 16-byte value; a mask for powers of two).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "swn_frame_entry.hpp"
#include "swn_geom.hpp"

#pragma clang fp contract(off)      // the chains are explicit fma calls; nothing else may be fused or re-associated

namespace {

constexpr long long ENV_MAX_FRAMES = 1LL << 24;         // frames (= blocks) per call
constexpr double ENV_PI = 3.14159265358979323846;

struct EnvEntry {
    const float* wav;   // sample t0
    float* out;         // frame f0
    const float* f0v;   // F0 of frame f0
    int t0, n_avail, len, f0, f1, blk0;
};
struct EnvArgs {
    EnvEntry e[SWN_LOGMEL_MAX_ENTRIES];
    const double* tables;                               // cos(2 pi m / n_fft), then the freqt matrix (order + 1, bins)
    double fs, q1, default_f0, floor2, f0_lo, f0_hi, D;  // floor^2; the validity limits f0_floor and fs / 4; D = fs / n_fft
    int n_entries, n_fft, hop, order, what;
};
static_assert(sizeof(EnvArgs) <= 4096, "the by-value kernel arguments must stay inside 4 KB");

__host__ __device__ constexpr int env_tpad(int m) { return m + (m >> 5); }

// doubles of LDS a block needs: T, xw and three vectors of bins + 1
size_t env_lds_doubles(int n_fft) {
    return (size_t)env_tpad(n_fft) + n_fft + 3 * (size_t)(n_fft / 2 + 2);
}

// two cosine sums side by side: acc_i = sum_j src[j] T[(k_i j) mod n], j = 0 .. count - 1 ascending
__device__ __forceinline__ void env_cos_chains(const double* __restrict__ src, const double* __restrict__ T, int n, int count, int k0,
                                               int k1, double& r0, double& r1) {
    double a0 = 0.0, a1 = 0.0;
    int i0 = 0, i1 = 0;
    for (int j = 0; j < count; ++j) {
        const double s = src[j];
        a0 = fma(s, T[env_tpad(i0)], a0);
        a1 = fma(s, T[env_tpad(i1)], a1);
        i0 += k0; i0 = i0 >= n ? i0 - n : i0;
        i1 += k1; i1 = i1 >= n ? i1 - n : i1;
    }
    r0 = a0; r1 = a1;
}

__global__ __launch_bounds__(256) void envelope_kernel(const EnvArgs a) {
    extern __shared__ double env_lds[];
    __shared__ double red[3];                           // sqrt(sum w^2), sum xw, sum w
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = a.n_fft, half = n / 2, bins = half + 1, quarter = n / 4;
    double* T = env_lds;
    double* xw = T + env_tpad(n);
    double* A = xw + n;
    double* B = A + bins + 1;
    double* C = B + bins + 1;

    int ei = 0;
    for (int i = 1; i < a.n_entries; ++i)               // the last entry whose first block is not past this one (entries without
        if (a.e[i].blk0 <= (int)blockIdx.x) ei = i;     // frames share their blk0 with the next entry, which wins)
    const EnvEntry& e = a.e[ei];
    const int f = e.f0 + ((int)blockIdx.x - e.blk0);

    // 1. the effective F0: NaN fails both comparisons
    const double v0 = (double)e.f0v[f - e.f0];
    const double f0e = (v0 > a.f0_lo && v0 <= a.f0_hi) ? v0 : a.default_f0;
    int hl = (int)floor(1.5 * a.fs / f0e + 0.5);
    hl = hl < 1 ? 1 : (hl > half - 1 ? half - 1 : hl);  // never taken for a call the host accepted: 6 <= hl <= n_fft / 2 - 1
    const int N = 2 * hl + 1;

    // 2. the window, in T
    for (int i = tid; i < N; i += nt) T[i] = 0.5 * cos(ENV_PI * (double)(i - hl) * f0e / (1.5 * a.fs)) + 0.5;
    __syncthreads();
    if (tid == 0) {
        double q = 0.0;
        for (int i = 0; i < N; ++i) q = fma(T[i], T[i], q);
        red[0] = sqrt(q);
    }
    __syncthreads();
    {   // x[t] = 0 outside [0, len); nothing outside the window [t0, t0 + n_avail) is read
        const double sq = red[0];
        const int hi = e.t0 + e.n_avail;
        for (int i = tid; i < N; i += nt) {
            const int t = f * a.hop + (i - hl);
            const bool in = t >= e.t0 && t < hi && (e.len < 0 || t < e.len);
            const double w = T[i] / sq;
            T[i] = w;
            xw[i] = (in ? (double)e.wav[t - e.t0] : 0.0) * w;
        }
    }
    __syncthreads();
    if (tid == 0 || tid == 64) {                        // two waves, one chain each
        const double* src = tid == 0 ? xw : T;
        double s = 0.0;
        for (int i = 0; i < N; ++i) s = fma(src[i], 1.0, s);
        red[tid == 0 ? 1 : 2] = s;
    }
    __syncthreads();
    {
        const double r = red[1] / red[2];
        for (int i = tid; i < N; i += nt) xw[i] = xw[i] - T[i] * r;
    }
    __syncthreads();
    for (int m = tid; m < n; m += nt) T[env_tpad(m)] = a.tables[m];
    __syncthreads();

    // 3. the power spectrum: bin b's twiddle for sample j is T[(b j) mod n] - i T[(b j + n / 4) mod n]; two bins per thread
    for (int b0 = tid; b0 < bins; b0 += 2 * nt) {
        const int b1 = b0 + nt < bins ? b0 + nt : b0;
        double re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
        int i0 = 0, i1 = 0;
        for (int j = 0; j < N; ++j) {
            const double s = xw[j];
            const int q0 = i0 + quarter >= n ? i0 + quarter - n : i0 + quarter;
            const int q1 = i1 + quarter >= n ? i1 + quarter - n : i1 + quarter;
            re0 = fma(s, T[env_tpad(i0)], re0);
            im0 = fma(s, T[env_tpad(q0)], im0);
            re1 = fma(s, T[env_tpad(i1)], re1);
            im1 = fma(s, T[env_tpad(q1)], im1);
            i0 += b0; i0 = i0 >= n ? i0 - n : i0;
            i1 += b1; i1 = i1 >= n ? i1 - n : i1;
        }
        A[b0] = re0 * re0 + im0 * im0;
        if (b1 != b0) A[b1] = re1 * re1 + im1 * im1;
    }
    if (tid == 0) A[bins] = 0.0;
    __syncthreads();

    // 4. the DC correction, from the uncorrected P
    {
        const double fb = f0e / a.D;
        const int nb = (int)floor(fb);                  // <= n_fft / 4: f0e <= fs / 4
        for (int b = tid; b < bins; b += nt) {
            double p = A[b];
            if (b <= nb) {
                const double u = fb - (double)b;
                int i = (int)floor(u);
                i = i < 0 ? 0 : (i > half - 1 ? half - 1 : i);
                p = (p + A[i]) + (u - (double)i) * (A[i + 1] - A[i]);
            }
            B[b] = p;
        }
    }
    __syncthreads();

    // 5. - 6. the box of width wd over rectangles of width D, mirrored at 0 and Nyquist; the log; C = e_b L[b] for the cosine sum
    {
        const double wd = 2.0 * f0e / 3.0;
        for (int b = tid; b < bins; b += nt) {
            const double lo = (double)b * a.D - wd / 2.0, hi = (double)b * a.D + wd / 2.0;
            const int n_lo = (int)floor(lo / a.D + 0.5), n_hi = (int)floor(hi / a.D + 0.5);
            double acc = 0.0;
            for (int m = n_lo; m <= n_hi; ++m) {
                const double ov = fmin(hi, ((double)m + 0.5) * a.D) - fmax(lo, ((double)m - 0.5) * a.D);
                int at = m < 0 ? -m : (m > half ? n - m : m);
                at = at < 0 ? 0 : (at > half ? half : at);
                if (ov > 0.0) acc = fma(ov, B[at], acc);
            }
            const double L = log(fmax((1.0 / wd) * acc, a.floor2));
            C[b] = (b == 0 || b == half) ? L : 2.0 * L;
        }
    }
    __syncthreads();

    // 7. the cepstrum v = irfft(L) as a cosine sum, and the two lifters; B receives what the output step sums: the one-sided
    //    cepstrum c for the mel-cepstrum, e_k ct[k] for the log amplitude
    for (int k0 = tid; k0 < bins; k0 += 2 * nt) {
        const int k1 = k0 + nt < bins ? k0 + nt : k0;
        double s[2];
        env_cos_chains(C, T, n, bins, k0, k1, s[0], s[1]);
        for (int u = 0; u < 2; ++u) {
            const int k = u == 0 ? k0 : k1;
            if (u == 1 && k1 == k0) break;
            const double v = s[u] / (double)n;
            double ls = 1.0;
            if (k > 0) {
                const double x = ENV_PI * f0e * (double)k / a.fs;
                ls = sin(x) / x;
            }
            const double lc = (1.0 - 2.0 * a.q1) + 2.0 * a.q1 * cos(2.0 * ENV_PI * (double)k * f0e / a.fs);
            const double ct = v * ls * lc;
            const bool end = k == 0 || k == half;
            B[k] = a.what == SWN_ENVELOPE_MCEP ? (end ? ct * 0.5 : ct) : (end ? ct : 2.0 * ct);
        }
    }
    __syncthreads();

    // 8. the outputs, each value rounded once to fp32
    if (a.what == SWN_ENVELOPE_MCEP) {
        float* o = e.out + (size_t)(f - e.f0) * (a.order + 1);
        const double* G = a.tables + n;
        for (int m = tid; m <= a.order; m += nt) {
            const double* g = G + (size_t)m * bins;
            double acc = 0.0;
            for (int k = 0; k < bins; ++k) acc = fma(g[k], B[k], acc);
            o[m] = static_cast<float>(acc);
        }
    } else {
        float* o = e.out + (size_t)(f - e.f0) * bins;
        for (int b0 = tid; b0 < bins; b0 += 2 * nt) {
            const int b1 = b0 + nt < bins ? b0 + nt : b0;
            double s0, s1;
            env_cos_chains(B, T, n, bins, b0, b1, s0, s1);
            o[b0] = static_cast<float>(0.5 * s0);
            if (b1 != b0) o[b1] = static_cast<float>(0.5 * s1);
        }
    }
}

int env_fail(const char* what) {
    swn_set_error_detail("swn_envelope", what);
    return SWN_E_BADARG;
}

bool env_size_ok(int n_fft, int order) {
    return n_fft >= 32 && n_fft <= SWN_SPECTRAL_MAX_FFT && n_fft % 32 == 0 && order >= 0 && order <= SWN_MCEP_MAX_ORDER &&
           order <= n_fft / 2;
}

}  // namespace

extern "C" size_t swn_envelope_table_doubles(int n_fft, int order) {
    return env_size_ok(n_fft, order) ? (size_t)n_fft + (size_t)(order + 1) * (n_fft / 2 + 1) : 0;
}

// The kernel keeps a frame's vectors in LDS: the scratch is one double, so that a later layout can grow it behind the same call
extern "C" size_t swn_envelope_work_bytes(int n_fft, int hop, const swn_envelope_entry* entries_host, int n_entries) {
    if (!env_size_ok(n_fft, 0) || hop < 1 || hop > SWN_F0_MAX_HOP || !entries_host || n_entries < 1 ||
        n_entries > SWN_LOGMEL_MAX_ENTRIES)
        return 0;
    for (int i = 0; i < n_entries; ++i)
        if (entries_host[i].f0 < 0 || entries_host[i].f1 < entries_host[i].f0) return 0;
    return sizeof(double);
}

extern "C" int swn_envelope(double fs, int n_fft, int hop, int order, float floor, double q1, double default_f0, int what,
                            const double* tables_dev, const swn_envelope_entry* entries_host, int n_entries, void* work_dev,
                            void* stream) {
    auto fail = [](const char* w) { return env_fail(w); };
    char msg[200];
    if (!(fs > 0.0) || !std::isfinite(fs)) return fail("fs must be a finite number > 0");
    if (n_fft < 32 || n_fft > SWN_SPECTRAL_MAX_FFT || n_fft % 32 != 0)
        return fail("n_fft must be a multiple of 32 in [32, SWN_SPECTRAL_MAX_FFT]");
    if (hop < 1 || hop > SWN_F0_MAX_HOP) return fail("hop outside [1, SWN_F0_MAX_HOP]");
    if (order < 0 || order > SWN_MCEP_MAX_ORDER || order > n_fft / 2) return fail("order outside [0, min(SWN_MCEP_MAX_ORDER, n_fft / 2)]");
    if (!(floor > 0.f) || !std::isfinite(floor)) return fail("floor must be a finite number > 0");
    if (!std::isfinite(q1)) return fail("q1 must be finite");
    const double f0_lo = 3.0 * fs / ((double)n_fft - 3.0), f0_hi = fs / 4.0;
    if (!(default_f0 > f0_lo) || !(default_f0 <= f0_hi)) {
        snprintf(msg, sizeof msg, "default_f0 %g outside (3 fs / (n_fft - 3) = %g, fs / 4 = %g]: a longer transform", default_f0,
                 f0_lo, f0_hi);
        return fail(msg);
    }
    if (what != SWN_ENVELOPE_MCEP && what != SWN_ENVELOPE_LOGAMP) return fail("what must be SWN_ENVELOPE_MCEP or SWN_ENVELOPE_LOGAMP");
    if (!tables_dev || (uintptr_t)tables_dev % sizeof(double) != 0) return fail("tables_dev is NULL or not aligned for doubles");
    if (!entries_host) return fail("entries_host is NULL");
    if (!work_dev || (uintptr_t)work_dev % sizeof(double) != 0) return fail("work_dev is NULL or not aligned for doubles");
    if (n_entries < 1 || n_entries > SWN_LOGMEL_MAX_ENTRIES) return fail("n_entries outside [1, SWN_LOGMEL_MAX_ENTRIES]");

    EnvArgs a;
    const int half = n_fft / 2;
    long long blocks = 0;
    for (int i = 0; i < SWN_LOGMEL_MAX_ENTRIES; ++i) {
        EnvEntry& o = a.e[i];
        o.wav = nullptr; o.out = nullptr; o.f0v = nullptr; o.t0 = o.n_avail = o.len = o.f0 = o.f1 = 0; o.blk0 = (int)blocks;
        if (i >= n_entries) continue;
        const swn_envelope_entry& e = entries_host[i];
        // the rules that do not depend on the feature are swn_logmel_entry's
        const swn_logmel_entry le = {e.wav_dev, e.out_dev, e.t0, e.n_avail, e.len, e.f0, e.f1, (e.reserved | e.reserved2) != 0};
        const int rc = frame_entry_check(le, i, hop, 1, "1 <= len", true, fail);
        if (rc == FE_EMPTY) continue;
        if (rc != SWN_OK) return rc;
        if (!e.f0_dev) { snprintf(msg, sizeof msg, "entry %d: null pointer", i); return fail(msg); }
        // frame f spans [f hop - (n_fft / 2 - 1), f hop + n_fft / 2) whatever its F0; what lies outside [0, len) is zeros
        const long long end = (long long)e.t0 + e.n_avail;
        const long long lo = (long long)e.f0 * hop - (half - 1), hi = (long long)(e.f1 - 1) * hop + half - 1;
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
        o.wav = e.wav_dev; o.out = e.out_dev; o.f0v = e.f0_dev;
        o.t0 = e.t0; o.n_avail = e.n_avail; o.len = e.len; o.f0 = e.f0; o.f1 = e.f1;
        blocks += e.f1 - e.f0;
        if (blocks > ENV_MAX_FRAMES) return fail("more than 2^24 frames in one call");
    }
    if (blocks == 0) return SWN_OK;                     // no frame in any entry
    a.tables = tables_dev;
    a.fs = fs; a.q1 = q1; a.default_f0 = default_f0; a.floor2 = (double)floor * (double)floor;
    a.f0_lo = f0_lo; a.f0_hi = f0_hi; a.D = fs / (double)n_fft;
    a.n_entries = n_entries; a.n_fft = n_fft; a.hop = hop; a.order = order; a.what = what;
    const int threads = n_fft / 2 + 1 <= 64 ? 128 : 256;   // the window step needs two waves
    (void)hipGetLastError();
    hipLaunchKernelGGL(envelope_kernel, dim3((unsigned)blocks), dim3(threads), env_lds_doubles(n_fft) * sizeof(double),
                       static_cast<hipStream_t>(stream), a);
    return swn_launch_status("swn_envelope");
}
