// Noise-shaping restoration on the device (swn_postfilter_chunk, include/swn_hip.h): the time-invariant MLSA filter of
// run.sh stage 6 / 9 (noise_shaping.py --inv false; host version csrc/swn_dsp.c) followed by the causal low-cut FIR, resumable
// per session slot.
//
// One wave per entry.  Lane k holds chain element k of every stage-2 Pade section (the all-pass chain of swn_dsp.c basic_fir,
// d[0 .. m+1]), so the order is limited to m <= 62.  Within one sample the sections are independent (section i reads pt[i-1]
// of the previous sample); only the feedback pt[0] = x + sum(+-v) joins them.  The chain update of basic_fir,
//     n[k] = (s[k] + a s[k+1]) - a n[k-1],  k = 2 .. m,   n[1] = (1 - a^2) u + a s[1],
// is a first-order linear recurrence with the constant coefficient p = -a.  It is split into the part that does not depend
// on the section's input u - a weighted log-step scan S over lanes of c[k] = s[k] + a s[k+1] - and the part that does,
// n[k] = S[k] + p^(k-1) n[1].  The section output y = sum_{k=2..m} b[k] n[k] is then  sum_k c[k] B[k] + G n[1]  with
// B[k] = sum_{i=k..m} b[i] p^(i-k) and G = sum_{i=2..m} b[i] p^(i-1): one butterfly reduction that does not wait for u.
// Butterfly sums are bit-identical in every lane (fp addition commutes), so all lanes agree on every uniform value.
//
// Lane k keeps r[k] = n[k] of the last sample (= s[k+1], the host layout after its shift loop).  The state of a slot is the
// host layout of swn_dsp.c: stage 1 (2 (pd+1) doubles), stage 2 (pd (m+2) + pd + 1), then the last n_taps - 1 MLSA outputs for
// the FIR.  A call loads it, runs its samples in tiles of PF_TILE (the MLSA outputs of a tile go to LDS, the FIR over them runs
// parallel over output samples, each output summed over the taps in one fixed order) and writes it back.  Every output sample
// is thus computed by the same operations whatever the chunk boundaries: concatenated chunk outputs equal the one-shot output.
// Arithmetic is fp64 throughout (the recursion is latency-bound; fp64 keeps the host C code a tight parity anchor).
#include <hip/hip_runtime.h>
#include <math.h>

#include <vector>

#include "swn_geom.hpp"

namespace {

constexpr int PF_WAVE = 64;
constexpr int PF_TILE = 512;
constexpr int PF_MAX_HIST = SWN_POSTFILTER_MAX_TAPS - 1;

__constant__ double k_pf_pade4[5] = {1.0, 4.999273e-1, 1.067005e-1, 1.170221e-2, 5.656279e-4};
__constant__ double k_pf_pade5[6] = {1.0, 4.999391e-1, 1.107098e-1, 1.369984e-2, 9.564853e-4, 3.041721e-5};

struct PfTable {
    swn_postfilter_entry e[SWN_POSTFILTER_MAX_ENTRIES];
};
static_assert(sizeof(swn_postfilter_entry) == 32, "swn_postfilter_entry is 32 bytes (include/swn_hip.h)");

struct PfArgs {
    const double* b;       // order + 1 MLSA coefficients
    const double* taps;    // n_taps FIR taps
    const double* mulaw;   // SWN_POSTFILTER_MULAW_ENTRIES values, or null
    double* state;         // capacity slots of `stride` doubles
    size_t stride;
    double alpha;
    int m, n_taps;
};

template <int PD>
__global__ __launch_bounds__(PF_WAVE) void postfilter_kernel(const PfTable t, const PfArgs a) {
    __shared__ double lh[SWN_POSTFILTER_MAX_TAPS];          // FIR taps
    __shared__ double lw[PF_MAX_HIST + PF_TILE];             // MLSA outputs: the last n_taps - 1 | this tile
    __shared__ double lx[PF_TILE];                           // this tile's inputs, gain applied

    const swn_postfilter_entry& en = t.e[blockIdx.x];
    const bool reset = (en.flags & SWN_POSTFILTER_RESET) != 0;
    const int n = en.n;
    if (n == 0 && !reset) return;
    const int k = threadIdx.x;
    const int m = a.m, H = a.n_taps - 1;
    const double al = a.alpha, p = -al, one_a2 = 1.0 - al * al;
    const double* pp = PD == 4 ? k_pf_pade4 : k_pf_pade5;
    double* st1 = a.state + (size_t)en.slot * a.stride;
    double* st2 = st1 + 2 * (PD + 1);
    double* sth = st2 + PD * (m + 2) + PD + 1;

    // ---- coefficients: lane constants and uniform values (computed the same way by every call)
    double pw = 0.0;                                         // p^(k-1), lanes k >= 1
    if (k >= 1) {
        pw = 1.0;
        for (int j = 1; j < k; ++j) pw *= p;
    }
    double Bk = 0.0;                                         // B[k], lanes 2 .. m
    if (k >= 2 && k <= m) {
        Bk = a.b[m];
        for (int i = m - 1; i >= k; --i) Bk = a.b[i] + p * Bk;
    }
    double G = 0.0;
    for (int i = m; i >= 2; --i) G = a.b[i] + p * G;
    G *= p;
    double P[6];                                             // p^1, p^2, p^4 .. p^32 of the scan steps
    P[0] = p;
#pragma unroll
    for (int s = 1; s < 6; ++s) P[s] = P[s - 1] * P[s - 1];
    const bool chain = k >= 2 && k <= m;                     // lanes of c[k]
    const bool keep = k >= 1 && k <= m;                      // lanes of r[k]
    const double gain = exp(a.b[0]), b1 = a.b[1];
    double ppv[PD + 1];
#pragma unroll
    for (int i = 0; i <= PD; ++i) ppv[i] = pp[i];

    // ---- state
    double d1[PD + 1], pt1[PD + 1], pt2[PD + 1], r[PD], s1[PD], u0[PD];
#pragma unroll
    for (int i = 0; i <= PD; ++i) {
        d1[i] = reset ? 0.0 : st1[i];
        pt1[i] = reset ? 0.0 : st1[PD + 1 + i];
        pt2[i] = reset ? 0.0 : st2[PD * (m + 2) + i];
    }
#pragma unroll
    for (int j = 0; j < PD; ++j) {
        const double* sec = st2 + j * (m + 2);
        u0[j] = reset ? 0.0 : sec[0];
        s1[j] = reset ? 0.0 : sec[1];
        r[j] = (reset || !keep) ? 0.0 : sec[k + 1];
    }
    for (int i = k; i < a.n_taps; i += PF_WAVE) lh[i] = a.taps[i];
    for (int i = k; i < H; i += PF_WAVE) lw[i] = reset ? 0.0 : sth[i];

    for (int t0 = 0; t0 < n; t0 += PF_TILE) {
        const int cnt = min(PF_TILE, n - t0);
        for (int i = k; i < cnt; i += PF_WAVE) {
            double x;
            if (en.kind == SWN_POSTFILTER_IN_MULAW) {
                const int q = static_cast<const int32_t*>(en.in_dev)[t0 + i];
                x = a.mulaw[min(max(q, 0), SWN_POSTFILTER_MULAW_ENTRIES - 1)];
            } else {
                x = static_cast<const float*>(en.in_dev)[t0 + i];
            }
            lx[i] = x * gain;
        }
        __syncthreads();

        // ---- MLSA, one sample after the other; every lane runs it, lane 0 keeps the output
        for (int j = 0; j < cnt; ++j) {
            // stage 1: exp(b(1) Phi_1), uniform
            double x = lx[j], out = 0.0;
#pragma unroll
            for (int i = PD; i >= 1; --i) {
                d1[i] = one_a2 * pt1[i - 1] + al * d1[i];
                pt1[i] = d1[i] * b1;
                const double v = pt1[i] * ppv[i];
                x += (i & 1) ? v : -v;
                out += v;
            }
            pt1[0] = x;
            x += out;
            // stage 2: exp(sum_{m >= 2} b(m) Phi_m); section j is the host's section j + 1, its input pt2[j] (previous sample)
            double S[PD], R[PD];
#pragma unroll
            for (int s = 0; s < PD; ++s) {
                const double rup = __shfl_up(r[s], 1u, PF_WAVE);
                const double c = chain ? rup + al * r[s] : 0.0;
                S[s] = c;
                R[s] = c * Bk;
            }
#pragma unroll
            for (int st = 0; st < 6; ++st) {
                const int off = 1 << st;
#pragma unroll
                for (int s = 0; s < PD; ++s) {
                    const double w = __shfl_up(S[s], (unsigned)off, PF_WAVE);
                    if (k >= off) S[s] += P[st] * w;
                    R[s] += __shfl_xor(R[s], PF_WAVE >> (st + 1), PF_WAVE);
                }
            }
            double y[PD];
#pragma unroll
            for (int s = 0; s < PD; ++s) {
                const double u = pt2[s];
                const double n1 = one_a2 * u + al * s1[s];
                y[s] = R[s] + G * n1;
                r[s] = keep ? S[s] + pw * n1 : 0.0;
                s1[s] = n1;
                u0[s] = u;
            }
            out = 0.0;
#pragma unroll
            for (int i = PD; i >= 1; --i) {
                pt2[i] = y[i - 1];
                const double v = pt2[i] * ppv[i];
                x += (i & 1) ? v : -v;
                out += v;
            }
            pt2[0] = x;
            if (k == 0) lw[H + j] = out + x;
        }
        __syncthreads();

        // ---- low cut over the tile: y[t] = sum_q h[q] w[t - q], q = 0 .. n_taps - 1 in this order
        float* dst = en.out_dev + t0;
        for (int o = k; o < cnt; o += PF_WAVE) {
            double acc = 0.0;
            const double* w = lw + H + o;
            for (int q = 0; q < a.n_taps; ++q) acc = fma(lh[q], w[-q], acc);
            dst[o] = static_cast<float>(acc);
        }
        // keep the last H MLSA outputs for the next tile / call
        double tmp[(PF_MAX_HIST + PF_WAVE - 1) / PF_WAVE];
#pragma unroll
        for (int c = 0; c < (PF_MAX_HIST + PF_WAVE - 1) / PF_WAVE; ++c) {
            const int i = k + c * PF_WAVE;
            if (i < H) tmp[c] = lw[cnt + i];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < (PF_MAX_HIST + PF_WAVE - 1) / PF_WAVE; ++c) {
            const int i = k + c * PF_WAVE;
            if (i < H) lw[i] = tmp[c];
        }
        __syncthreads();
    }

    // ---- state back, in the host layout
    if (k == 0) {
#pragma unroll
        for (int i = 0; i <= PD; ++i) {
            st1[i] = d1[i];
            st1[PD + 1 + i] = pt1[i];
            st2[PD * (m + 2) + i] = pt2[i];
        }
#pragma unroll
        for (int j = 0; j < PD; ++j) {
            st2[j * (m + 2)] = u0[j];
            st2[j * (m + 2) + 1] = s1[j];
        }
    }
    if (keep) {
#pragma unroll
        for (int j = 0; j < PD; ++j) st2[j * (m + 2) + k + 1] = r[j];
    }
    for (int i = k; i < H; i += PF_WAVE) sth[i] = lw[i];
}

bool pf_args_ok(int order, double alpha, int pade, int n_taps) {
    return order >= 1 && (pade == 4 || pade == 5) && fabs(alpha) < 1.0 && n_taps >= 1 && n_taps <= SWN_POSTFILTER_MAX_TAPS;
}

}  // namespace

extern "C" size_t swn_postfilter_state_doubles(int order, int pade, int n_taps) {
    if (!pf_args_ok(order, 0.0, pade, n_taps)) return 0;
    return 2 * (size_t)(pade + 1) + (size_t)pade * (order + 2) + pade + 1 + (size_t)(n_taps - 1);
}

extern "C" int swn_postfilter_chunk(int order, double alpha, int pade, const double* b_dev, int n_taps, const double* taps_dev,
                                    const double* mulaw_dev, double* state_dev, int capacity,
                                    const swn_postfilter_entry* entries_host, int n_entries, void* stream) {
    if (!pf_args_ok(order, alpha, pade, n_taps) || !b_dev || !taps_dev || !state_dev || capacity < 1 || n_entries < 0 ||
        (n_entries > 0 && !entries_host))
        return SWN_E_BADARG;
    std::vector<unsigned char> used((size_t)capacity, 0);
    for (int e = 0; e < n_entries; ++e) {
        const swn_postfilter_entry& en = entries_host[e];
        if (en.slot < 0 || en.slot >= capacity || used[en.slot] || en.n < 0 || (en.flags & ~SWN_POSTFILTER_RESET) != 0 ||
            (en.kind != SWN_POSTFILTER_IN_F32 && en.kind != SWN_POSTFILTER_IN_MULAW) ||
            (en.n > 0 && (!en.in_dev || !en.out_dev)) || (en.kind == SWN_POSTFILTER_IN_MULAW && !mulaw_dev))
            return SWN_E_BADARG;
        used[en.slot] = 1;
    }
    if (order > SWN_POSTFILTER_MAX_ORDER) return SWN_E_UNSUPPORTED;
    if (n_entries == 0) return SWN_OK;
    const PfArgs a{b_dev, taps_dev, mulaw_dev, state_dev, swn_postfilter_state_doubles(order, pade, n_taps), alpha, order, n_taps};
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    for (int e0 = 0; e0 < n_entries; e0 += SWN_POSTFILTER_MAX_ENTRIES) {
        const int ne = n_entries - e0 < SWN_POSTFILTER_MAX_ENTRIES ? n_entries - e0 : SWN_POSTFILTER_MAX_ENTRIES;
        PfTable t;
        for (int e = 0; e < SWN_POSTFILTER_MAX_ENTRIES; ++e)
            t.e[e] = e < ne ? entries_host[e0 + e] : swn_postfilter_entry{nullptr, nullptr, 0, 0, 0, 0};
        if (pade == 4)
            hipLaunchKernelGGL(postfilter_kernel<4>, dim3(ne), dim3(PF_WAVE), 0, st, t, a);
        else
            hipLaunchKernelGGL(postfilter_kernel<5>, dim3(ne), dim3(PF_WAVE), 0, st, t, a);
        const int rc = swn_launch_status("swn_postfilter_chunk");
        if (rc != SWN_OK) return rc;
    }
    return SWN_OK;
}
