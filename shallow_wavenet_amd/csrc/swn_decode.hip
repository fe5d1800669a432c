// Autoregressive decode on gfx950: ONE persistent workgroup per utterance runs the prologue
// (seed positions 0..rf-seg) and every generation step inside a single launch; the ~22
// convolution launches and ~5.3k ATen calls per sample of the reference loop
// (cswnv_shift1.py:348-402, dswnv.py:338-374) become LDS/L2 traffic and s_barriers.
//
// This file holds the GENERIC kernel: any (H, S, K, dd, dr, seg, lpc, Q) at run time, history
// rings in a global scratch buffer (L2-resident), weights streamed from the packed buffer.
// The register/LDS-resident BL6-class kernel lives in swn_decode_bl6.hip.
//
// Per position q the math is (cswnv_shift1.py:281-285, :352-391):
//   h0[q]  = softsign(cb + sum_k [valid] (cv_k * S[q-(K-1-k)] + cc_k))         fused wav_conv+causal
//   a      = bd_l + Wd_l . [h_{l-1}[q-(K-1)d] .. h_{l-1}[q]]                    dilated causal conv
//   g      = in_x_l(x)[q] (.) a ;  z = sigmoid(g[:H]) ; h_l = (1-z) tanh(g[H:]) + z h_{l-1}[q]
//   head   = out_2(relu(out_1(relu(sum_l out_skip_l(h_l)))))   at the last position of a step
// The "true zero" left padding of the reference prologue is reproduced by zero-initialised
// rings: a slot that would hold a negative position has not been written yet.
#include <cstdio>
#include <hip/hip_runtime.h>
#include "swn_decode_internal.hpp"

namespace {

constexpr int NT = 256;

struct DecArgs {
    SwnGeom g;
    SwnLayout y;
    const float* packed;
    const float* cond;
    SwnNoise nz;
    const void* forced;
    const void* seed;
    float* state;
    void* out;
    float* heads;
    int B, Tf, n_steps;
    int ring_off[SWN_MAXL];
    int ring_len[SWN_MAXL];
    int state_stride;
    // streamed chunk (STREAM instantiations only): absolute index of the chunk's first step, 1 = the state comes from
    // the session (no prologue), the session's sample windows ([B][round4(WN)] floats behind the rings in `state`)
    int step0, resume;
    float* win;
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float softsignf_(float x) { return x / (1.f + fabsf(x)); }
__device__ __forceinline__ int pmod(int r, int m) { int t = r % m; return t < 0 ? t + m : t; }

// rows x (nseg segments of SL floats) mat-vec for NP right-hand sides.  16 lanes per row read
// 16-byte pieces of the row (256 B contiguous per row and pass), rows are reduced with
// row-local shuffles.  xf(j, s) returns the base of segment s of right-hand side j.
template <int NP, class XF>
__device__ __forceinline__ void matvec16(const float* __restrict__ W, int NR, int nseg, int SL, XF xf,
                                         float* out, int ldout, const float* __restrict__ bias,
                                         bool relu, int np) {
    const int p = threadIdx.x & 15, rs = threadIdx.x >> 4;
    const size_t rowlen = (size_t)nseg * SL;
    for (int r0 = 0; r0 < NR; r0 += NT / 16) {
        const int row = r0 + rs;
        float acc[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) acc[j] = 0.f;
        if (row < NR) {
            const float* wr = W + (size_t)row * rowlen;
            for (int s = 0; s < nseg; ++s) {
                const float* xs[NP];
#pragma unroll
                for (int j = 0; j < NP; ++j) xs[j] = (j < np) ? xf(j, s) : nullptr;
                for (int i0 = p * 4; i0 < SL; i0 += 64) {
                    const float4 w = *reinterpret_cast<const float4*>(wr + (size_t)s * SL + i0);
#pragma unroll
                    for (int j = 0; j < NP; ++j) {
                        if (j < np) {
                            const float4 x = *reinterpret_cast<const float4*>(xs[j] + i0);
                            acc[j] = fmaf(w.x, x.x, acc[j]);
                            acc[j] = fmaf(w.y, x.y, acc[j]);
                            acc[j] = fmaf(w.z, x.z, acc[j]);
                            acc[j] = fmaf(w.w, x.w, acc[j]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            float v = acc[j];
            v += __shfl_xor(v, 8, 16);
            v += __shfl_xor(v, 4, 16);
            v += __shfl_xor(v, 2, 16);
            v += __shfl_xor(v, 1, 16);
            if (p == 0 && row < NR && j < np) {
                v += bias[row];
                out[j * ldout + row] = relu ? fmaxf(v, 0.f) : v;
            }
        }
    }
}

// the arguments of a pool launch: a streamed chunk over the entries (batch = E, n_steps = n_max), then the entry table
struct DecPoolArgs {
    DecArgs c;
    SwnPoolTable t;
};
static_assert(sizeof(DecPoolArgs) <= 4096, "kernel arguments are limited to 4 KB");
// ... and of a multi-model pool launch (swn_decode_pool_chunk_models): the model table behind them
struct DecPoolModelsArgs : DecPoolArgs {
    SwnPoolModels m;
};
static_assert(sizeof(DecPoolModelsArgs) <= 4096, "kernel arguments are limited to 4 KB");
// ... and of a wide pool launch (swn_decode_pool_chunk_wide): the table lies in device memory
struct DecPoolWideArgs {
    DecArgs c;
    const SwnPoolWideRow* rows;
};
template <bool POOL, bool MODELS, bool WIDE = false> struct GenericArgs { using type = DecArgs; };
template <> struct GenericArgs<true, false, false> { using type = DecPoolArgs; };
template <> struct GenericArgs<true, true, false> { using type = DecPoolModelsArgs; };
template <> struct GenericArgs<true, false, true> { using type = DecPoolWideArgs; };
__device__ __forceinline__ const DecArgs& pool_or_launch(const DecArgs& launch, const DecArgs&) { return launch; }
__device__ __forceinline__ const DecArgs& pool_or_launch(const DecPoolArgs&, const DecArgs& entry) { return entry; }
__device__ __forceinline__ const DecArgs& pool_or_launch(const DecPoolWideArgs&, const DecArgs& entry) { return entry; }
__device__ __forceinline__ const DecArgs& launch_args(const DecArgs& launch) { return launch; }
__device__ __forceinline__ const DecArgs& launch_args(const DecPoolArgs& launch) { return launch.c; }
__device__ __forceinline__ const DecArgs& launch_args(const DecPoolWideArgs& launch) { return launch.c; }

// STREAM: a chunk of a streamed decode (swn_decode_chunk): steps [step0, step0 + n_steps) with absolute positions and
// generator counters, chunk-local out / heads / noise / forced rows; the rings stay in the session (a.state) and the sample
// window is loaded from / saved to the session.  STREAM = false is the one-shot decode.
// POOL (with STREAM): the workgroup runs one entry of a decode pool (swn_decode_pool_chunk) - `a` already holds that entry as
// a batch-1 chunk (swn_pool_entry_args), so b = 0; a BEGIN entry zeroes its own slot's rings here (the other slots of the
// session buffer belong to other streams).
// MODELS (with POOL): the entry's weights are those of its model (SwnPoolModels); an instantiation of its own, so that the
// single-model pool kernel stays the code it was.
// WIDE (with POOL, without MODELS): the entry, its model's packed buffer included, is row blockIdx.x of the launch's device table
// (swn_decode_pool_chunk_wide); again an instantiation of its own.
template <int SEGT, int KIND, bool STREAM = false, bool POOL = false, bool MODELS = false, bool WIDE = false>
__global__ __launch_bounds__(NT) void decode_generic_kernel(const typename GenericArgs<POOL, MODELS, WIDE>::type ka) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    DecArgs pa;                                             // POOL: this workgroup's entry as a batch-1 chunk
    if constexpr (WIDE) {
        static_assert(POOL && !MODELS, "a wide launch is a pool launch whose rows name the models");
        pa = ka.c;
        const SwnPoolWideRow row = swn_pool_wide_row(ka.rows);
        pa.packed = row.model;
        const SwnGeom& g = ka.c.g;
        if (!swn_pool_entry_args(pa, row.e, g.seg, KIND == SWN_KIND_SOFTMAX ? g.Q : g.seg, g.NO)) return;
        pa.state += (size_t)row.e.slot * pa.state_stride;
        pa.win += (size_t)row.e.slot * swn_round4((g.K - 1 > g.lpc ? g.K - 1 : g.lpc) + g.seg);
    } else if constexpr (POOL) {
        static_assert(POOL || !MODELS, "only pools take a model table");
        pa = ka.c;
        if constexpr (MODELS) pa.packed = swn_pool_model(ka.m);
        const SwnGeom& g = ka.c.g;
        if (!swn_pool_entry_args(pa, ka.t, g.seg, KIND == SWN_KIND_SOFTMAX ? g.Q : g.seg, g.NO)) return;
        const int slot = swn_pool_slot(ka.t);
        pa.state += (size_t)slot * pa.state_stride;
        pa.win += (size_t)slot * swn_round4((g.K - 1 > g.lpc ? g.K - 1 : g.lpc) + g.seg);
    }
    const DecArgs& a = pool_or_launch(ka, pa);
    // the geometry and the ring plan are read where the launch put them: indexed by layer, a private copy would be scratch
    const DecArgs& ar = launch_args(ka);
    const SwnGeom& g = ar.g;
    const int tid = threadIdx.x;
    const int b = POOL ? 0 : blockIdx.x;
    const int H = g.H, Hp = g.Hp, H2 = 2 * g.H, K = g.K, L = g.L, seg = g.seg, S = g.S;
    const int WN = (K - 1 > g.lpc ? K - 1 : g.lpc) + seg;
    const float* __restrict__ P = a.packed;

    // ---- LDS carve (all offsets multiples of 4 floats)
    float* a_out = smem;                                    // [SEGT][2H]
    float* hcat = a_out + SEGT * swn_round4(H2);            // [L][Hp]
    float* skipv = hcat + L * Hp;                           // [Sp]
    float* o1v = skipv + g.Sp;                              // [O1p]
    float* o2v = o1v + g.O1p;                               // [round4(NO)]
    float* shist = o2v + swn_round4(g.NO);                  // [round4(WN)]  (int bits for softmax)
    float* tw = shist + swn_round4(WN);                     // [SEGT*SEGT]
    int* tf = reinterpret_cast<int*>(tw + SEGT * SEGT);     // [SEGT*SEGT]
    const int lds_floats = (int)((tf + SEGT * SEGT) - reinterpret_cast<int*>(smem));
    for (int e = tid; e < lds_floats; e += NT) smem[e] = 0.f;
    int* ihist = reinterpret_cast<int*>(shist);
    if (POOL && !a.resume)
        for (int e = tid; e < a.state_stride; e += NT) a.state[e] = 0.f;
    __syncthreads();
    if (KIND == SWN_KIND_SOFTMAX) {
        // padding class Q/2 = encode_mu_law(0), dswnv.py:308; the newest slot is the caller's seed class
        const int sc = a.seed ? reinterpret_cast<const int*>(a.seed)[b] : g.Q / 2;
        for (int e = tid; e < WN; e += NT) ihist[e] = (e == WN - 1) ? sc : g.Q / 2;
    } else if (a.seed) {
        // seed waveform `audio` (B, seg): the newest seg samples of the window (cswnv_shift1.py:300-334)
        for (int e = tid; e < seg; e += NT) shist[WN - seg + e] = reinterpret_cast<const float*>(a.seed)[(size_t)b * seg + e];
    }
    __syncthreads();
    const int WNR = swn_round4(WN);
    if (STREAM && a.resume) {
        for (int e = tid; e < WN; e += NT) shist[e] = a.win[(size_t)b * WNR + e];
        __syncthreads();
    }

    float* st = a.state + (size_t)b * a.state_stride;
    const float* condb = a.cond + (size_t)b * a.Tf * g.N;
    const int ld_a = swn_round4(H2);
    const int rf = g.rf;
    const int n_pro = rf - seg + 1;                          // prologue positions 0..rf-seg
    const int total = n_pro + a.n_steps;
    const int s0 = STREAM ? a.step0 : 0;                    // absolute index of step i = 0

    for (int it = (STREAM && a.resume) ? n_pro : 0; it < total; ++it) {
        const bool gen = it >= n_pro;
        const int i = it - n_pro;                            // generation step index (chunk-local)
        const int ia = s0 + i;                               // ... and of the utterance
        const int np = gen ? seg : 1;
        const int q0 = gen ? rf + 1 - seg + ia * seg : it;   // first position handled now

        // ---- conditioning lookups for this step (frame index / upsampler tap per (j,s))
        if (tid < np * seg) {
            const int j = tid / seg, s = tid % seg;
            int tt = q0 + j + s - rf; tt = tt < 0 ? 0 : tt;
            int f = tt / g.U; const int jj = tt - f * g.U;
            f = f < a.Tf ? f : a.Tf - 1;
            tf[j * SEGT + s] = f;
            tw[j * SEGT + s] = P[a.y.wup + jj];
        }
        // ---- input layer: h0 = softsign(causal(lift(S)))  -> ring 0
        for (int e = tid; e < H * np; e += NT) {
            const int j = e / H, o = e - j * H;
            const int q = q0 + j;
            float acc = P[a.y.cb + o];
            for (int k = 0; k < K; ++k) {
                const int r = q - (K - 1 - k);               // sample position feeding tap k
                if (KIND == SWN_KIND_LAPLACE) {
                    if (r >= -(seg - 1)) {
                        // window holds S[qe-WN+1..qe], qe = last known position
                        const int qe = gen ? rf + ia * seg : rf;
                        const float sv = gen ? shist[r - qe + WN - 1] : 0.f;
                        acc += fmaf(P[a.y.cv + (size_t)k * H + o], sv, P[a.y.cc + (size_t)k * H + o]);
                    }
                } else {
                    if (r >= 0) {
                        const int qe = gen ? rf + ia : rf;
                        const int idx = gen ? ihist[r - qe + WN - 1] : g.Q / 2;
                        acc += P[a.y.ct + ((size_t)k * g.Q + idx) * H + o];
                    }
                }
            }
            st[ar.ring_off[0] + pmod(q, ar.ring_len[0]) * Hp + o] = softsignf_(acc);
        }
        __syncthreads();

        // ---- stack
        for (int l = 0; l < L; ++l) {
            const int dil = g.dil[l], R = ar.ring_len[l];
            const float* ring = st + ar.ring_off[l];
            auto xf = [&](int j, int k) -> const float* {
                return ring + (size_t)pmod(q0 + j - (K - 1 - k) * dil, R) * Hp;
            };
            matvec16<SEGT>(P + a.y.wd + (size_t)l * H2 * K * Hp, H2, K, Hp, xf, a_out, ld_a,
                           P + a.y.bd + (size_t)l * H2, false, np);
            __syncthreads();
            for (int e = tid; e < H * np; e += NT) {
                const int j = e / H, o = e - j * H;
                const int q = q0 + j;
                float gxz = P[a.y.bx + (size_t)l * H2 + o];
                float gxc = P[a.y.bx + (size_t)l * H2 + H + o];
                for (int s = 0; s < seg; ++s) {
                    const float* cr = condb + (size_t)tf[j * SEGT + s] * g.N + (size_t)(l * seg + s) * H2;
                    const float w = tw[j * SEGT + s];
                    gxz = fmaf(w, cr[o], gxz);
                    gxc = fmaf(w, cr[H + o], gxc);
                }
                if (KIND == SWN_KIND_SOFTMAX && g.audio_in) {
                    const int qe = gen ? rf + ia : rf;
                    const int idx = gen ? ihist[q - qe + WN - 1] : g.Q / 2;
                    const float* wa = P + a.y.wxa + ((size_t)l * g.Q + idx) * H2;
                    gxz += wa[o]; gxc += wa[H + o];
                }
                const float z = sigmoidf_(gxz * a_out[j * ld_a + o]);
                const float c = tanhf(gxc * a_out[j * ld_a + H + o]);
                const float hp = ring[(size_t)pmod(q, R) * Hp + o];
                const float hn = (1.f - z) * c + z * hp;
                if (l + 1 < L) st[ar.ring_off[l + 1] + pmod(q, ar.ring_len[l + 1]) * Hp + o] = hn;
                if (j == np - 1) hcat[l * Hp + o] = hn;
            }
            __syncthreads();
        }
        if (!gen) continue;

        // ---- head at the last position of the step
        {
            auto x1 = [&](int, int) -> const float* { return hcat; };
            matvec16<1>(P + a.y.wsk, S, 1, L * Hp, x1, skipv, 0, P + a.y.bsk, true, 1);
            __syncthreads();
            auto x2 = [&](int, int) -> const float* { return skipv; };
            matvec16<1>(P + a.y.w1, g.O1, 1, g.Sp, x2, o1v, 0, P + a.y.b1, true, 1);
            __syncthreads();
            auto x3 = [&](int, int) -> const float* { return o1v; };
            matvec16<1>(P + a.y.w2, g.NO, 1, g.O1p, x3, o2v, 0, P + a.y.b2, false, 1);
            __syncthreads();
        }
        if (a.heads)
            for (int e = tid; e < g.NO; e += NT) a.heads[((size_t)b * a.n_steps + i) * g.NO + e] = o2v[e];

        if (KIND == SWN_KIND_LAPLACE) {
            // Laplace head, cswnv_shift1.py:368-391: b = exp(logsigmoid(.)), LP coefficients flipped,
            // one uniform draw per sample, clamp before feedback.
            if (tid == 0) {
#pragma clang fp contract(off)
                const float* forced = reinterpret_cast<const float*>(a.forced);
                float* outp = reinterpret_cast<float*>(a.out) + (size_t)b * a.n_steps * seg + (size_t)i * seg;
                float lp[16];
                const int lpc = g.lpc;
                for (int k = 0; k < lpc; ++k) lp[k] = shist[WN - lpc + k];
                float fed[SEGT];
                for (int j = 0; j < seg; ++j) {
                    const float mu = o2v[j];
                    const float yv = o2v[seg + j];
                    const float bsc = expf(fminf(yv, 0.f) - log1pf(expf(-fabsf(yv))));
                    float lpv = 0.f;
                    for (int k = 0; k < lpc; ++k) lpv += o2v[2 * seg + lpc - 1 - k] * lp[k];
                    const float e = swn_noise_laplace_at(a.nz, b, i, ia, j, a.n_steps, seg);
                    const float sg = (e > 0.f) ? 1.f : ((e < 0.f) ? -1.f : 0.f);
                    const float t = (bsc * sg) * log1pf(-2.f * fabsf(e));
                    float sv = (lpc > 0) ? (lpv + mu) - t : mu - t;
                    sv = fminf(fmaxf(sv, -1.f), 1.f);
                    outp[j] = sv;
                    const float fd = forced ? forced[(size_t)b * a.n_steps * seg + (size_t)i * seg + j] : sv;
                    fed[j] = fd;
                    for (int k = 0; k + 1 < lpc; ++k) lp[k] = lp[k + 1];
                    if (lpc > 0) lp[lpc - 1] = fd;
                }
                for (int k = 0; k + seg < WN; ++k) shist[k] = shist[k + seg];
                for (int j = 0; j < seg; ++j) shist[WN - seg + j] = fed[j];
            }
        } else {
            // softmax head, dswnv.py:361-369: softmax -> Categorical renormalisation ->
            // multinomial(n=1) == argmax(p / q) with q ~ Exp(1) supplied by the host.
            if (tid < 64) {
                const int Q = g.Q;
                float m = -INFINITY;
                for (int e = tid; e < Q; e += 64) m = fmaxf(m, o2v[e]);
                for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
                float sum = 0.f;
                for (int e = tid; e < Q; e += 64) sum += expf(o2v[e] - m);
                for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
                float sum2 = 0.f;
                for (int e = tid; e < Q; e += 64) sum2 += expf(o2v[e] - m) / sum;
                for (int d = 32; d >= 1; d >>= 1) sum2 += __shfl_xor(sum2, d, 64);
                float best = -1.f; int bi = 0x7fffffff;
                for (int e = tid; e < Q; e += 64) {
                    const float r = ((expf(o2v[e] - m) / sum) / sum2) / swn_noise_exp1_at(a.nz, b, i, ia, e, a.n_steps, Q);
                    if (r > best) { best = r; bi = e; }
                }
                for (int d = 32; d >= 1; d >>= 1) {
                    const float ob = __shfl_xor(best, d, 64);
                    const int oi = __shfl_xor(bi, d, 64);
                    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
                }
                if (tid == 0) {
                    const int* forced = reinterpret_cast<const int*>(a.forced);
                    reinterpret_cast<int*>(a.out)[(size_t)b * a.n_steps + i] = bi;
                    const int fd = forced ? forced[(size_t)b * a.n_steps + i] : bi;
                    for (int k = 0; k + 1 < WN; ++k) ihist[k] = ihist[k + 1];
                    ihist[WN - 1] = fd;
                }
            }
        }
        __syncthreads();
    }
    if (STREAM)
        for (int e = tid; e < WN; e += NT) a.win[(size_t)b * WNR + e] = shist[e];
}


int ring_plan(const SwnGeom& g, int* off, int* len) {
    int o = 0;
    for (int l = 0; l < g.L; ++l) {
        off[l] = o; len[l] = g.pad[l] + g.seg;
        o += len[l] * g.Hp;
    }
    return (o + 63) & ~63;
}

int generic_segt(const SwnGeom& g) { return g.seg <= 1 ? 1 : (g.seg <= 2 ? 2 : (g.seg <= 5 ? 5 : 10)); }
int generic_wn(const SwnGeom& g) { return (g.K - 1 > g.lpc ? g.K - 1 : g.lpc) + g.seg; }
size_t generic_lds(const SwnGeom& g) {
    const int segt = generic_segt(g);
    const size_t lds_floats = (size_t)segt * swn_round4(2 * g.H) + (size_t)g.L * g.Hp + g.Sp + g.O1p +
                              swn_round4(g.NO) + swn_round4(generic_wn(g)) + 2 * (size_t)segt * segt;
    return lds_floats * sizeof(float);
}

// one workgroup per utterance / pool entry
template <int SEGT, bool STREAM, bool POOL, bool MODELS, bool WIDE = false>
int launch_generic(const typename GenericArgs<POOL, MODELS, WIDE>::type& a, const SwnDecodeCall& c, size_t lds, const char* where) {
    const auto kern = c.g.kind == SWN_KIND_LAPLACE ? &decode_generic_kernel<SEGT, SWN_KIND_LAPLACE, STREAM, POOL, MODELS, WIDE>
                                                   : &decode_generic_kernel<SEGT, SWN_KIND_SOFTMAX, STREAM, POOL, MODELS, WIDE>;
    hipLaunchKernelGGL(kern, dim3(c.batch), dim3(NT), lds, c.hip_stream, a);
    return swn_launch_status(where);
}

// the instantiation of a call: one-shot, streamed chunk, pool, pool over several models, wide pool
template <int SEGT>
int launch_generic_call(const DecPoolModelsArgs& p, const SwnDecodeCall& c, size_t lds) {
    if (c.wide) {
        const DecPoolWideArgs w = {p.c, c.wide};
        return launch_generic<SEGT, true, true, false, true>(w, c, lds, "swn_decode_pool_chunk_wide(generic)");
    }
    if (c.models) return launch_generic<SEGT, true, true, true>(p, c, lds, "swn_decode_pool_chunk_models(generic)");
    if (c.pool) return launch_generic<SEGT, true, true, false>(p, c, lds, "swn_decode_pool_chunk(generic)");
    if (c.stream) return launch_generic<SEGT, true, false, false>(p.c, c, lds, "swn_decode(generic)");
    return launch_generic<SEGT, false, false, false>(p.c, c, lds, "swn_decode(generic)");
}

// the generic kernel over a call: `state` holds the rings of c.capacity utterances (zeroed here unless a streamed chunk
// resumes; a pool's BEGIN entries zero their own slots in the kernel), a stream's sample windows lie behind them
int generic_run(const SwnDecodeCall& c) {
    const size_t lds = generic_lds(c.g);
    if (lds > 160 * 1024) return SWN_E_UNSUPPORTED;
    DecPoolModelsArgs p;
    DecArgs& a = p.c;
    a.g = c.g;
    swn_make_layout(&a.g, &a.y);
    a.packed = c.packed; a.cond = c.cond; a.nz = c.nz; a.forced = c.forced; a.seed = c.seed; a.state = c.state;
    a.out = c.out; a.heads = c.heads; a.B = c.batch; a.Tf = c.n_frames; a.n_steps = c.n_steps;
    a.state_stride = ring_plan(a.g, a.ring_off, a.ring_len);
    a.step0 = c.step0; a.resume = c.resume;
    a.win = c.stream ? c.state + (size_t)a.state_stride * c.capacity : nullptr;
    if (c.pool) p.t = *c.pool;
    if (c.models) p.m = *c.models;
    if (!c.pool && !c.wide && !c.resume &&
        hipMemsetAsync(a.state, 0, sizeof(float) * (size_t)a.state_stride * a.B, c.hip_stream) != hipSuccess)
        return SWN_E_LAUNCH;
    switch (generic_segt(c.g)) {
        case 1: return launch_generic_call<1>(p, c, lds);
        case 2: return launch_generic_call<2>(p, c, lds);
        case 5: return launch_generic_call<5>(p, c, lds);
        default: return launch_generic_call<10>(p, c, lds);
    }
}

enum { KSEL_GENERIC = 1, KSEL_BL6W = 2, KSEL_STEPPED = 3, KSEL_BL6 = 6 };

// the kernel that variant `variant` of swn_decode, swn_decode_chunk and swn_decode_pool_chunk runs for (net, batch): KSEL_*, or a
// negative SWN_E_*.  0 = the best one that applies, 2 / 6 = the BL6 class only (6: the symmetric kernel, whatever the net - A/B
// and parity runs), 3 = the stepped chain only, 1 = the generic kernel
int resolve_kernel(const SwnGeom& g, int batch, int variant) {
    if (batch < 1) return SWN_E_BADARG;
    if ((variant == 0 || variant == 2) && swn_decode_bl6w_session_floats(g) > 0) return KSEL_BL6W;
    if (variant == 0 || variant == 2 || variant == 6) {
        if (swn_decode_bl6_session_floats(g) > 0) return KSEL_BL6;
        if (variant != 0) return SWN_E_UNSUPPORTED;
    }
    if (variant < 0 || variant > 3) return SWN_E_BADARG;   // (4 and 5, the cohort and cluster experiments of ABI 2, are retired)
    // large geometries (REF6: MBs of weights per step) run one launch per phase over many CUs
    const bool big = (size_t)g.L * 2 * g.H * g.K * g.Hp >= (size_t)256 * 1024;
    if (variant == 3 || (variant == 0 && big)) {
        if (swn_decode_stepped_supported(g, batch)) return KSEL_STEPPED;
        if (variant == 3) return SWN_E_UNSUPPORTED;
    }
    if (generic_lds(g) > 160 * 1024) return SWN_E_UNSUPPORTED;
    return KSEL_GENERIC;
}

// the *_w16 / *_w8 calls run on the symmetric BL6 kernel alone: SWN_OK when `variant` resolves to it for (net, batch)
int image_kernel_check(int wk, const SwnGeom& g, int batch, int variant, const char* where) {
    static const char* const word[] = {"fp32", "bf16", "e4m3"};   // by WK_*
    const int k = resolve_kernel(g, batch, variant);
    if (k == KSEL_BL6) return SWN_OK;
    char detail[256];
    if (k == KSEL_BL6W)
        snprintf(detail, sizeof detail, "%s weights run on the symmetric BL6 kernel; this net resolves to the wave-specialised "
                                        "kernel with this variant: pass variant = 6", word[wk]);
    else
        snprintf(detail, sizeof detail, "%s weights run on the symmetric BL6 kernel only (variant 0, 2 or 6 on a net of its "
                                        "class); the stepped and generic kernels are not served", word[wk]);
    swn_set_error_detail(where, detail);
    return SWN_E_UNSUPPORTED;
}

// the kernel of a pool launch over one or several fp32 models: the stepped chain runs one launch per phase for all
// utterances at one step, so it is not served here (swn_decode_pool_stepped_chunk is)
int pool_kernel(const SwnGeom& g, int capacity, int variant) {
    const int k = resolve_kernel(g, capacity, variant);
    if (k == KSEL_STEPPED || variant == 3) return SWN_E_UNSUPPORTED;
    return k < 0 ? SWN_E_BADARG : k;
}

// hands a checked call to kernel `k` (KSEL_*)
int run_call(int k, const SwnDecodeCall& c) {
    (void)hipGetLastError();   // drop stale errors of earlier runtime calls; only this call's launches are reported
    if (k == KSEL_BL6W) return swn_decode_bl6w_run(c);
    if (k == KSEL_BL6) return swn_decode_bl6_run(c);
    if (k == KSEL_STEPPED) return swn_decode_stepped_run(c);
    return generic_run(c);
}

// ---- the argument rules of the entry points (include/swn_hip.h) up to the variant: each makes the geometry, refuses what no
// kernel takes and fills the record with what the caller passed.  The arguments keep the order of the C ABI.  What the fp32
// and the *_w16 / *_w8 calls ask on top of these (the image, the kernel a variant resolves to) is in the entry points.

// swn_decode, swn_decode_w16, swn_decode_w8 (empty buffers may be null when there is nothing to generate)
int oneshot_check(SwnDecodeCall& c, const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames,
                  int n_steps, const swn_decode_io* io, float* state, void* out, float* heads, void* stream_) {
    const int rc = swn_make_geom(d, &c.g);
    if (rc < 0) return rc;
    if (batch < 1 || n_frames < 1 || n_steps < 0 || !io) return SWN_E_BADARG;
    if (n_steps > 0 && (!packed || !cond || !out)) return SWN_E_BADARG;
    if ((long)n_steps * c.g.seg > (long)n_frames * c.g.U) return SWN_E_BADARG;   // conditioning too short
    c.packed = packed; c.cond = cond; c.batch = c.capacity = batch; c.n_frames = n_frames; c.n_steps = n_steps;
    c.nz = swn_noise_of(io); c.forced = io->forced_dev; c.seed = io->seed_dev;
    c.state = state; c.out = out; c.heads = heads; c.hip_stream = (hipStream_t)stream_;
    return SWN_OK;
}

// swn_decode_chunk, swn_decode_chunk_w16, swn_decode_chunk_w8
int chunk_check(SwnDecodeCall& c, const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames,
                int step0, int n_steps, int flags, const swn_decode_io* io, float* session, void* out, float* heads,
                void* stream_) {
    const int rc = swn_make_geom(d, &c.g);
    if (rc < 0) return rc;
    if (!io || !session || !packed || !cond) return SWN_E_BADARG;
    if (batch < 1 || n_frames < 1 || step0 < 0 || n_steps < 0 || (flags & ~SWN_CHUNK_BEGIN)) return SWN_E_BADARG;
    const bool begin = (flags & SWN_CHUNK_BEGIN) != 0;
    if (begin && step0 != 0) return SWN_E_BADARG;
    if (n_steps > 0 && !out) return SWN_E_BADARG;
    if (((long long)step0 + n_steps) * c.g.seg > (long long)n_frames * c.g.U) return SWN_E_BADARG;   // conditioning not final yet
    c.packed = packed; c.cond = cond; c.batch = c.capacity = batch; c.n_frames = n_frames; c.step0 = step0; c.n_steps = n_steps;
    c.stream = true; c.resume = !begin;
    c.nz = swn_noise_of(io); c.forced = io->forced_dev; c.seed = io->seed_dev;
    c.state = session; c.out = out; c.heads = heads; c.hip_stream = (hipStream_t)stream_;
    return SWN_OK;
}
// nothing to generate and no prologue to run: the session stays as it is
bool chunk_is_idle(const SwnDecodeCall& c) { return c.n_steps == 0 && c.resume; }

// swn_decode_pool_chunk, swn_decode_pool_chunk_models, swn_decode_pool_chunk_w16 / _w8: the record of a streamed chunk over the
// entries (n_steps = the most steps of an entry), the checked table in `t`; work = an entry has steps to run or begins
// (the wide call, swn_decode_pool_chunk_wide, keeps the caller's entries instead of a table: t null, max_entries its own limit)
int pool_check(SwnDecodeCall& c, SwnPoolTable* t, bool& work, const swn_net_desc* d, int capacity,
               const swn_decode_pool_entry* entries, int n_entries, const swn_decode_io* io, float* session, void* out,
               float* heads, void* stream_, int max_entries = SWN_DECODE_POOL_MAX_ENTRIES) {
    const int rc = swn_make_geom(d, &c.g);
    if (rc < 0) return rc;
    const SwnGeom& g = c.g;
    if (!entries || !io || !session) return SWN_E_BADARG;
    if (capacity < 1 || n_entries < 1 || n_entries > max_entries) return SWN_E_BADARG;
    if (io->noise_dev || io->forced_dev) return SWN_E_BADARG;    // pools draw their noise on the device, no teacher forcing
    if (t) *t = {};
    int n_max = 0;
    work = false;
    for (int e = 0; e < n_entries; ++e) {
        const swn_decode_pool_entry& en = entries[e];
        const bool begin = (en.flags & SWN_CHUNK_BEGIN) != 0;
        if (!en.cond_dev || en.n_frames < 1 || en.slot < 0 || en.slot >= capacity || en.step0 < 0 || en.n_steps < 0 ||
            (en.flags & ~SWN_CHUNK_BEGIN) || en.reserved != 0)
            return SWN_E_BADARG;
        if (begin && en.step0 != 0) return SWN_E_BADARG;
        if (((long long)en.step0 + en.n_steps) * g.seg > (long long)en.n_frames * g.U) return SWN_E_BADARG;
        for (int f = 0; f < e; ++f)
            if (entries[f].slot == en.slot) return SWN_E_BADARG;   // two workgroups on one session
        if (t) t->e[e] = en;
        n_max = en.n_steps > n_max ? en.n_steps : n_max;
        work = work || begin || en.n_steps > 0;
    }
    if (n_max > 0 && !out) return SWN_E_BADARG;
    c.pool = t; c.batch = n_entries; c.capacity = capacity; c.n_steps = n_max; c.stream = true;
    c.nz = swn_pool_noise_of(io); c.seed = io->seed_dev;
    c.state = session; c.out = out; c.heads = heads; c.hip_stream = (hipStream_t)stream_;
    return SWN_OK;
}

}  // namespace

extern "C" size_t swn_decode_state_floats(const swn_net_desc* d, int batch) {
    SwnGeom g; if (swn_make_geom(d, &g) < 0 || batch < 1) return 0;
    int off[SWN_MAXL], len[SWN_MAXL];
    size_t a = (size_t)ring_plan(g, off, len) * batch;
    const size_t b = swn_decode_stepped_state_floats(g, batch);
    return a > b ? a : b;                                  // large enough for every kernel variant
}

extern "C" int swn_decode(const swn_net_desc* d, const float* packed, const float* cond, int batch,
                          int n_frames, int n_steps, const swn_decode_io* io,
                          float* state, void* out, float* heads, int variant, void* stream_) {
    SwnDecodeCall c;
    const int rc = oneshot_check(c, d, packed, cond, batch, n_frames, n_steps, io, state, out, heads, stream_);
    if (rc < 0) return rc;
    if (n_steps == 0) return SWN_OK;                       // nothing to generate, whatever the variant
    const int k = resolve_kernel(c.g, batch, variant);
    // the BL6 kernels keep their state on chip; every other kernel, and every refusal but that of a variant that asks for the
    // BL6 class alone, wants the caller's state buffer first
    if (k != KSEL_BL6W && k != KSEL_BL6) {
        if (!state && variant != 2 && variant != 6) return SWN_E_BADARG;
        if (k < 0) return k;
    }
    return run_call(k, c);
}

// ---- streamed decode ---------------------------------------------------------------------------------------------
extern "C" int swn_decode_resolve_variant(const swn_net_desc* d, int batch, int variant) {
    SwnGeom g;
    const int rc = swn_make_geom(d, &g);
    if (rc < 0) return rc;
    const int k = resolve_kernel(g, batch, variant);
    if (k < 0) return k;
    if (k == KSEL_BL6W) return 2;
    if (k == KSEL_BL6) return variant == 6 ? 6 : 2;
    return k;
}

extern "C" size_t swn_decode_session_floats(const swn_net_desc* d, int batch, int variant) {
    SwnGeom g;
    if (swn_make_geom(d, &g) < 0) return 0;
    const int k = resolve_kernel(g, batch, variant);
    if (k < 0) return 0;
    if (k == KSEL_BL6W) return swn_decode_bl6w_session_floats(g) * (size_t)batch;
    if (k == KSEL_BL6) return swn_decode_bl6_session_floats(g) * (size_t)batch;
    if (k == KSEL_STEPPED) return swn_decode_stepped_state_floats(g, batch);
    int off[SWN_MAXL], len[SWN_MAXL];
    return ((size_t)ring_plan(g, off, len) + swn_round4(generic_wn(g))) * (size_t)batch;   // rings, then the sample windows
}

extern "C" int swn_decode_chunk(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames,
                                int step0, int n_steps, int flags, const swn_decode_io* io, float* session,
                                void* out, float* heads, int variant, void* stream_) {
    SwnDecodeCall c;
    const int rc = chunk_check(c, d, packed, cond, batch, n_frames, step0, n_steps, flags, io, session, out, heads, stream_);
    if (rc < 0) return rc;
    const int k = resolve_kernel(c.g, batch, variant);
    if (k < 0) return SWN_E_BADARG;
    if (chunk_is_idle(c)) return SWN_OK;
    return run_call(k, c);
}

// ---- decode pool ---------------------------------------------------------------------------------------------------
extern "C" int swn_decode_pool_chunk(const swn_net_desc* d, const float* packed, int capacity,
                                     const swn_decode_pool_entry* entries, int n_entries, const swn_decode_io* io,
                                     float* session, void* out, float* heads, int variant, void* stream_) {
    SwnDecodeCall c;
    SwnPoolTable t;
    bool work;
    const int rc = pool_check(c, &t, work, d, capacity, entries, n_entries, io, session, out, heads, stream_);
    if (rc < 0) return rc;
    if (!packed) return SWN_E_BADARG;
    const int k = pool_kernel(c.g, capacity, variant);
    if (k < 0) return k;
    if (!work) return SWN_OK;                              // every slot stays as it is
    c.packed = packed;
    return run_call(k, c);
}

// entry e runs models[model_of_entry[e]]
extern "C" int swn_decode_pool_chunk_models(const swn_net_desc* d, const float* const* models, int n_models,
                                            const int32_t* model_of_entry, int capacity,
                                            const swn_decode_pool_entry* entries, int n_entries, const swn_decode_io* io,
                                            float* session, void* out, float* heads, int variant, void* stream_) {
    SwnDecodeCall c;
    SwnPoolTable t;
    bool work;
    const int rc = pool_check(c, &t, work, d, capacity, entries, n_entries, io, session, out, heads, stream_);
    if (rc < 0) return rc;
    if (swn_pool_models_check(models, n_models, model_of_entry, n_entries) < 0) return SWN_E_BADARG;
    const int k = pool_kernel(c.g, capacity, variant);
    if (k < 0) return k;
    if (!work) return SWN_OK;                              // every slot stays as it is
    SwnPoolModels m = {};
    for (int i = 0; i < SWN_POOL_MAX_MODELS; ++i) m.p[i] = models[i < n_models ? i : 0];
    for (int e = 0; e < n_entries; ++e) m.of[e] = (unsigned char)model_of_entry[e];
    c.models = &m;
    return run_call(k, c);
}

// ---- bf16 / FP8 (E4M3) storage of the streamed head matrices: the same rules, the image of swn_pack_decode_w16 / _w8 in
// format `wk`, and the symmetric BL6 kernel alone; `where` names the entry point
namespace {

int oneshot_image(int wk, const void* image, const char* where, const swn_net_desc* d, const float* packed, const float* cond,
                  int batch, int n_frames, int n_steps, const swn_decode_io* io, float* state, void* out, float* heads,
                  int variant, void* stream_) {
    SwnDecodeCall c;
    int rc = oneshot_check(c, d, packed, cond, batch, n_frames, n_steps, io, state, out, heads, stream_);
    if (rc < 0) return rc;
    if (!image) return SWN_E_BADARG;
    rc = image_kernel_check(wk, c.g, batch, variant, where);
    if (rc < 0) return rc;
    if (n_steps == 0) return SWN_OK;
    c.wk = wk; c.image = image;
    return run_call(KSEL_BL6, c);
}

int chunk_image(int wk, const void* image, const char* where, const swn_net_desc* d, const float* packed, const float* cond,
                int batch, int n_frames, int step0, int n_steps, int flags, const swn_decode_io* io, float* session, void* out,
                float* heads, int variant, void* stream_) {
    SwnDecodeCall c;
    int rc = chunk_check(c, d, packed, cond, batch, n_frames, step0, n_steps, flags, io, session, out, heads, stream_);
    if (rc < 0) return rc;
    if (!image) return SWN_E_BADARG;
    rc = image_kernel_check(wk, c.g, batch, variant, where);
    if (rc < 0) return rc;
    if (chunk_is_idle(c)) return SWN_OK;
    c.wk = wk; c.image = image;
    return run_call(KSEL_BL6, c);
}

int pool_image(int wk, const void* image, const char* where, const swn_net_desc* d, const float* packed, int capacity,
               const swn_decode_pool_entry* entries, int n_entries, const swn_decode_io* io, float* session, void* out,
               float* heads, int variant, void* stream_) {
    SwnDecodeCall c;
    SwnPoolTable t;
    bool work;
    int rc = pool_check(c, &t, work, d, capacity, entries, n_entries, io, session, out, heads, stream_);
    if (rc < 0) return rc;
    if (!packed || !image) return SWN_E_BADARG;
    rc = image_kernel_check(wk, c.g, capacity, variant, where);
    if (rc < 0) return rc;
    if (!work) return SWN_OK;                              // every slot stays as it is
    c.packed = packed; c.wk = wk; c.image = image;
    return run_call(KSEL_BL6, c);
}

// ... over several models: entry e runs models[model_of_entry[e]] with images_host[model_of_entry[e]]
int pool_models_image(int wk, const void* const* images_host, const char* where, const swn_net_desc* d,
                      const float* const* models, int n_models, const int32_t* model_of_entry, int capacity,
                      const swn_decode_pool_entry* entries, int n_entries, const swn_decode_io* io, float* session, void* out,
                      float* heads, int variant, void* stream_) {
    SwnDecodeCall c;
    SwnPoolTable t;
    bool work;
    int rc = pool_check(c, &t, work, d, capacity, entries, n_entries, io, session, out, heads, stream_);
    if (rc < 0) return rc;
    if (swn_pool_models_check(models, n_models, model_of_entry, n_entries) < 0) return SWN_E_BADARG;
    if (!images_host) return SWN_E_BADARG;
    for (int m = 0; m < n_models; ++m)
        if (!images_host[m]) return SWN_E_BADARG;
    rc = image_kernel_check(wk, c.g, capacity, variant, where);
    if (rc < 0) return rc;
    if (!work) return SWN_OK;                              // every slot stays as it is
    SwnPoolModels m = {};
    const void* images[SWN_POOL_MAX_MODELS];
    for (int i = 0; i < SWN_POOL_MAX_MODELS; ++i) {
        m.p[i] = models[i < n_models ? i : 0];
        images[i] = images_host[i < n_models ? i : 0];
    }
    for (int e = 0; e < n_entries; ++e) m.of[e] = (unsigned char)model_of_entry[e];
    c.models = &m; c.images = images; c.wk = wk;
    return run_call(KSEL_BL6, c);
}

}  // namespace

extern "C" int swn_decode_pool_chunk_models_w16(const swn_net_desc* d, const float* const* models, int n_models,
                                                const int32_t* model_of_entry, int capacity,
                                                const swn_decode_pool_entry* entries, int n_entries, const swn_decode_io* io,
                                                float* session, void* out, float* heads, int variant,
                                                const void* const* images_host, void* stream_) {
    return pool_models_image(WK_BF16, images_host, "swn_decode_pool_chunk_models_w16", d, models, n_models, model_of_entry,
                             capacity, entries, n_entries, io, session, out, heads, variant, stream_);
}

extern "C" int swn_decode_pool_chunk_models_w8(const swn_net_desc* d, const float* const* models, int n_models,
                                               const int32_t* model_of_entry, int capacity,
                                               const swn_decode_pool_entry* entries, int n_entries, const swn_decode_io* io,
                                               float* session, void* out, float* heads, int variant,
                                               const void* const* images_host, void* stream_) {
    return pool_models_image(WK_E4M3, images_host, "swn_decode_pool_chunk_models_w8", d, models, n_models, model_of_entry,
                             capacity, entries, n_entries, io, session, out, heads, variant, stream_);
}

extern "C" int swn_decode_w16(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames,
                              int n_steps, const swn_decode_io* io, float* state, void* out, float* heads, int variant,
                              const void* w16, void* stream_) {
    return oneshot_image(WK_BF16, w16, "swn_decode_w16", d, packed, cond, batch, n_frames, n_steps, io, state, out, heads, variant,
                         stream_);
}

extern "C" int swn_decode_chunk_w16(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames,
                                    int step0, int n_steps, int flags, const swn_decode_io* io, float* session, void* out,
                                    float* heads, int variant, const void* w16, void* stream_) {
    return chunk_image(WK_BF16, w16, "swn_decode_chunk_w16", d, packed, cond, batch, n_frames, step0, n_steps, flags, io, session,
                       out, heads, variant, stream_);
}

extern "C" int swn_decode_pool_chunk_w16(const swn_net_desc* d, const float* packed, int capacity,
                                         const swn_decode_pool_entry* entries, int n_entries, const swn_decode_io* io,
                                         float* session, void* out, float* heads, int variant, const void* w16,
                                         void* stream_) {
    return pool_image(WK_BF16, w16, "swn_decode_pool_chunk_w16", d, packed, capacity, entries, n_entries, io, session, out, heads,
                      variant, stream_);
}

extern "C" int swn_decode_w8(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames,
                             int n_steps, const swn_decode_io* io, float* state, void* out, float* heads, int variant,
                             const void* w8, void* stream_) {
    return oneshot_image(WK_E4M3, w8, "swn_decode_w8", d, packed, cond, batch, n_frames, n_steps, io, state, out, heads, variant,
                         stream_);
}

extern "C" int swn_decode_chunk_w8(const swn_net_desc* d, const float* packed, const float* cond, int batch, int n_frames,
                                   int step0, int n_steps, int flags, const swn_decode_io* io, float* session, void* out,
                                   float* heads, int variant, const void* w8, void* stream_) {
    return chunk_image(WK_E4M3, w8, "swn_decode_chunk_w8", d, packed, cond, batch, n_frames, step0, n_steps, flags, io, session,
                       out, heads, variant, stream_);
}

extern "C" int swn_decode_pool_chunk_w8(const swn_net_desc* d, const float* packed, int capacity,
                                        const swn_decode_pool_entry* entries, int n_entries, const swn_decode_io* io,
                                        float* session, void* out, float* heads, int variant, const void* w8,
                                        void* stream_) {
    return pool_image(WK_E4M3, w8, "swn_decode_pool_chunk_w8", d, packed, capacity, entries, n_entries, io, session, out, heads,
                      variant, stream_);
}

// ---- wide pool launch: the entry table in device memory (swn_pool.hpp) -----------------------------------------------------
namespace {

static_assert(WK_F32 == SWN_WEIGHTS_FP32 && WK_BF16 == SWN_WEIGHTS_BF16 && WK_E4M3 == SWN_WEIGHTS_E4M3, "one code per format");

// the rows one setup launch brings in its kernel arguments
struct PoolWideSetupArgs {
    SwnPoolWideRow r[SWN_POOL_WIDE_SETUP_ROWS];
};
static_assert(sizeof(PoolWideSetupArgs) + 16 <= 4096, "kernel arguments are limited to 4 KB");

// block k writes row k of its launch, one dword per lane (vector stores), to the device table the decode launch reads
__global__ __launch_bounds__(64) void pool_wide_setup_kernel(const PoolWideSetupArgs a, SwnPoolWideRow* tab, int n_rows) {
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k < n_rows && tid < (int)(sizeof(SwnPoolWideRow) / 4))
        reinterpret_cast<int*>(tab + k)[tid] = reinterpret_cast<const int*>(&a.r[k])[tid];
}

}  // namespace

extern "C" size_t swn_decode_pool_wide_table_bytes(int n_entries) {
    if (n_entries < 1 || n_entries > SWN_DECODE_POOL_WIDE_MAX_ENTRIES) return 0;
    return (size_t)n_entries * sizeof(SwnPoolWideRow);
}

extern "C" int swn_decode_pool_chunk_wide(const swn_net_desc* d, const float* const* models, int n_models,
                                          const int32_t* model_of_entry, int capacity,
                                          const swn_decode_pool_entry* entries, int n_entries, const swn_decode_io* io,
                                          float* session, void* out, float* heads, int variant,
                                          const void* const* images_host, int weight_format, void* table_dev, void* stream_) {
    SwnDecodeCall c;
    bool work;
    int rc = pool_check(c, nullptr, work, d, capacity, entries, n_entries, io, session, out, heads, stream_,
                        SWN_DECODE_POOL_WIDE_MAX_ENTRIES);
    if (rc < 0) return rc;
    if (swn_pool_models_check(models, n_models, model_of_entry, n_entries, SWN_DECODE_POOL_WIDE_MAX_ENTRIES) < 0) return SWN_E_BADARG;
    if (weight_format != SWN_WEIGHTS_FP32 && weight_format != SWN_WEIGHTS_BF16 && weight_format != SWN_WEIGHTS_E4M3)
        return SWN_E_BADARG;
    if (!table_dev || (reinterpret_cast<uintptr_t>(table_dev) & 15)) return SWN_E_BADARG;
    int k = KSEL_BL6;
    if (weight_format == SWN_WEIGHTS_FP32) {
        k = pool_kernel(c.g, capacity, variant);
        if (k < 0) return k;
    } else {
        if (!images_host) return SWN_E_BADARG;
        for (int m = 0; m < n_models; ++m)
            if (!images_host[m]) return SWN_E_BADARG;
        rc = image_kernel_check(weight_format, c.g, capacity, variant, "swn_decode_pool_chunk_wide");
        if (rc < 0) return rc;
    }
    if (!work) return SWN_OK;                              // every slot stays as it is
    // the table: row e = entry e, its model's packed buffer and image; SWN_POOL_WIDE_SETUP_ROWS rows per setup launch
    SwnPoolWideRow* rows = static_cast<SwnPoolWideRow*>(table_dev);
    (void)hipGetLastError();
    for (int e0 = 0; e0 < n_entries; e0 += SWN_POOL_WIDE_SETUP_ROWS) {
        const int n = n_entries - e0 < SWN_POOL_WIDE_SETUP_ROWS ? n_entries - e0 : SWN_POOL_WIDE_SETUP_ROWS;
        PoolWideSetupArgs a = {};
        for (int e = 0; e < n; ++e) {
            const int m = model_of_entry[e0 + e];
            a.r[e].e = entries[e0 + e];
            a.r[e].model = models[m];
            a.r[e].image = weight_format == SWN_WEIGHTS_FP32 ? nullptr : images_host[m];
        }
        hipLaunchKernelGGL(pool_wide_setup_kernel, dim3(n), dim3(64), 0, c.hip_stream, a, rows + e0, n);
        rc = swn_launch_status("swn_decode_pool_chunk_wide(setup)");
        if (rc < 0) return rc;
    }
    c.wide = rows; c.wk = weight_format;
    return run_call(k, c);
}
