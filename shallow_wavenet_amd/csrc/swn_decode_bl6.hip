// BL6-class autoregressive decode on gfx950 (BASELINE-literal shape: 1x6 dilated stack, H=64,
// K=2, dilations 1..32, rf=64; Laplace S=128 with seg/lpc variants, softmax S=Q=256).
//
// One persistent 512-thread workgroup (8 waves, 2 per SIMD) per utterance.  What makes it
// different from the generic kernel (swn_decode.hip):
//   * the six dilated-conv weight matrices (6 x 128 x 128 fp32 = 384 KB) live in VGPRs for the
//     whole utterance: thread (o,p) owns gate row o and candidate row o+64 over 16 of the
//     128 inputs, 192 registers; rows are reduced over 8 adjacent lanes with DPP adds;
//   * the per-dilation history rings (cswnv_shift1.py:324-334 output_buffer) are LDS rings
//     with power-of-two lengths: 32-36 KB; a tap is one broadcast ds_read_b128 per 16 bytes;
//   * the gate  z=sigmoid, tanh, highway  epilogue is fused behind the reduction (no second
//     pass, one s_barrier per layer); with seg>1 lane p finishes position p;
//   * out_skip is accumulated layer by layer in the shadow of the next layer's phase, so only
//     one 128x64 slice sits on the critical path; out_1/out_skip stream from L2 in a
//     lane-tiled layout (1 KiB contiguous per wave instruction);
//   * conditioning: the current and next frame of the hoisted in_x product sit in LDS, the
//     rank-1 upsampler is one fma per gate input (cswnv_shift1.py:37-65,276).
// 9 s_barriers per generated step (10 for softmax).
#include "swn_decode_bl6_common.hpp"
#include "swn_decode_internal.hpp"
#include <type_traits>

namespace {

using namespace swn_bl6;

template <int S_, int SEG_, int LPC_, int KIND_, int Q_, bool EXT_ = false>
struct Tr {
    static constexpr int S = S_, SEG = SEG_, LPC = LPC_, KIND = KIND_, Q = Q_;
    static constexpr bool EXT = EXT_;     // extended mode: in-kernel noise generator / noise dump / seed waveform
    using Ext = Tr<S_, SEG_, LPC_, KIND_, Q_, true>;
    static constexpr int O1 = KIND_ == SWN_KIND_SOFTMAX ? Q_ : S_;
    static constexpr int NO = KIND_ == SWN_KIND_SOFTMAX ? Q_ : 2 * SEG_ + LPC_;
    static constexpr int WN = cmax(1, LPC_) + SEG_;
    static constexpr int ring_len(int l) { return pow2ceil((1 << l) + SEG_); }
    static constexpr int ring_off(int l) { int o = 0; for (int i = 0; i < l; ++i) o += ring_len(i) * H; return o; }
    static constexpr int PF = L * SEG_ * 2 * H;          // floats of one conditioning frame
    static constexpr int NREG = 5;                        // layers whose weights stay in VGPRs; the rest sit in LDS
    // LDS carve (float offsets)
    static constexpr int o_ring = 0;
    static constexpr int o_hcat = o_ring + ring_off(L);
    static constexpr int o_gp = o_hcat + L * H;
    static constexpr int o_bx = o_gp + 2 * PF;
    static constexpr int o_bd = o_bx + L * 2 * H;
    static constexpr int o_wup = o_bd + L * 2 * H;
    static constexpr int o_skip = o_wup + 256;
    static constexpr int o_o1 = o_skip + S_;
    static constexpr int o_o2 = o_o1 + O1;
    static constexpr int o_hist = o_o2 + r4(NO);
    // sampling noise staged off the critical path: Laplace [4 chunks][64 steps][SEG] transformed deviates (wave 1 fills
    // a chunk of 64 future steps at once, lane = step); softmax [2 steps][Q] Exp(1) draws (wave 2, one step ahead)
    static constexpr int NZC = 64, NZB = 4;
    static constexpr int o_tnz = o_hist + r4(WN);
    // (the classic Laplace instantiation keeps the round-1 carve: [2][8] deviates of the next step - LDS offsets past
    //  64 KB cost an address add each, so the layout is part of the measured kernel)
    static constexpr int o_cz = o_tnz + (KIND_ == SWN_KIND_LAPLACE ? (EXT_ ? r4(NZB * NZC * SEG_) : 16) : 2 * Q_);   // cb[64], cv[2][64], cc[2][64]
    static constexpr int o_w2 = o_cz + 5 * H;             // laplace: out_2 rows [NO][S] (+b2)
    static constexpr int o_bias = o_w2 + (KIND_ == SWN_KIND_LAPLACE ? NO * S_ + r4(NO) : 0);   // bsk[S], b1[O1], (softmax) b2[NO]
    static constexpr int o_wl = o_bias + S_ + O1 + (KIND_ == SWN_KIND_SOFTMAX ? NO : 0);          // [L-NREG][8][512][4]
    // most of the out_1 matrix (input slices 0..W1L-1 of 8, lane-tiled like the global copy; as many as the 160 KB
    // of LDS allow) stays in LDS for the single-sample Laplace net: the streamed rest's L2 latency then hides
    // under the resident slices' FMAs
    static constexpr int W1L = (KIND_ == SWN_KIND_LAPLACE && S_ == 128 && SEG_ <= 2) ? 4 : 0;
    static constexpr int o_w1l = o_wl + (L - NREG) * 8 * NT * 4;
    static constexpr int o_end = o_w1l + W1L * O1 * 16;
    static constexpr size_t lds_bytes = (size_t)o_end * sizeof(float);
    // per-utterance session of a streamed decode: the history rings as LDS holds them, then the sample window
    static constexpr int sess_floats = ring_off(L) + r4(WN);
};

template <int NP>
__device__ __forceinline__ float pick(const float (&a)[NP], int p) {
    float v = a[0];
#pragma unroll
    for (int j = 1; j < NP; ++j) v = (p == j) ? a[j] : v;
    return v;
}

// One DCRNN layer for NP consecutive positions q0..q0+NP-1 (cswnv_shift1.py:281-285).
template <class T, int LAYER, int NP>
__device__ __forceinline__ void layer_phase(float* lds, const float (&w)[2][16], int q0,
                                            const float (&wj)[T::SEG], const int (&pb)[T::SEG]) {
    constexpr int dil = 1 << LAYER;
    constexpr int R = T::ring_len(LAYER);
    const int tid = threadIdx.x, o = tid >> 3, p = tid & 7;
    const float* ring = lds + T::o_ring + T::ring_off(LAYER);
    float az[NP], ac[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) { az[j] = 0.f; ac[j] = 0.f; }
    // operands of the gate epilogue are fetched up front so their LDS latency hides under the FMAs
    // (lanes 0/1 of an octet: gate / candidate row; other lanes read valid but unused words)
    [[maybe_unused]] float e_bd = 0.f, e_gx = 0.f, e_hp = 0.f;
    if constexpr (NP == 1) {
        const int pr = p & 1;
        e_bd = lds[T::o_bd + LAYER * 2 * H + pr * H + o];
        e_gx = lds[T::o_bx + LAYER * 2 * H + pr * H + o];
#pragma unroll
        for (int s = 0; s < T::SEG; ++s)
            e_gx = fmaf(wj[s], lds[T::o_gp + pb[s] + (LAYER * T::SEG + s) * 2 * H + pr * H + o], e_gx);
        e_hp = ring[(q0 & (R - 1)) * H + o];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        // inputs 32m+4p..+3 of [tap0 = position q-dil | tap1 = position q]
        float4 w0, w1;
        if (LAYER < T::NREG) {
            w0 = make_float4(w[0][4 * m], w[0][4 * m + 1], w[0][4 * m + 2], w[0][4 * m + 3]);
            w1 = make_float4(w[1][4 * m], w[1][4 * m + 1], w[1][4 * m + 2], w[1][4 * m + 3]);
        } else {
            constexpr int wl = LAYER < T::NREG ? 0 : LAYER - T::NREG;
            w0 = *reinterpret_cast<const float4*>(lds + T::o_wl + ((wl * 8 + m) * NT + tid) * 4);
            w1 = *reinterpret_cast<const float4*>(lds + T::o_wl + ((wl * 8 + 4 + m) * NT + tid) * 4);
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int pos = q0 + j - (m < 2 ? dil : 0);
            const float4 x = *reinterpret_cast<const float4*>(ring + (pos & (R - 1)) * H + 32 * (m & 1) + 4 * p);
            az[j] = fmaf(w0.x, x.x, az[j]); ac[j] = fmaf(w1.x, x.x, ac[j]);
            az[j] = fmaf(w0.y, x.y, az[j]); ac[j] = fmaf(w1.y, x.y, ac[j]);
            az[j] = fmaf(w0.z, x.z, az[j]); ac[j] = fmaf(w1.z, x.z, ac[j]);
            az[j] = fmaf(w0.w, x.w, az[j]); ac[j] = fmaf(w1.w, x.w, ac[j]);
        }
        // keep the scheduler from hoisting every tap read of the phase at once (80 VGPRs at seg=5)
        if (NP > 2) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) { az[j] = sum8(az[j]); ac[j] = sum8(ac[j]); }
    __builtin_amdgcn_sched_barrier(0);              // keep the gate epilogue behind the reduction
#ifndef SWN_NO_SPLIT
    if constexpr (NP == 1) {
        // one position: lane 0 evaluates the gate (sigmoid), lane 1 the candidate (tanh), concurrently
        if (p < 2) {
            const int q = q0;
            const float sa = (p == 0 ? az[0] : ac[0]) + e_bd;
            const float v = e_gx * sa;
            float res;
            if (fabsf(v) > 9.02f && p == 1) {
                res = copysignf(1.f, v);                                       // tanh saturated in fp32
            } else {
                const float e = exp_c(p == 0 ? -v : -2.f * fabsf(v));
                const float r = rcp_c(1.f + e);
                res = p == 0 ? r : copysignf((1.f - e) * r, v);                // z | tanh
            }
            const float c = dpp_f<0xF5>(res);                                  // quad_perm [1,1,3,3]: lane 0 <- lane 1
            if (p == 0) {
                const float hn = (1.f - res) * c + res * e_hp;
                if (LAYER + 1 < L) {
                    constexpr int R2 = T::ring_len(LAYER + 1 < L ? LAYER + 1 : LAYER);
                    lds[T::o_ring + T::ring_off(LAYER + 1 < L ? LAYER + 1 : LAYER) + (q & (R2 - 1)) * H + o] = hn;
                }
                lds[T::o_hcat + LAYER * H + o] = hn;
            }
        }
    } else
#endif
    if (p < NP) {                                   // lane p finishes position q0+p
        const int q = q0 + p;
        const float sz = pick<NP>(az, p) + lds[T::o_bd + LAYER * 2 * H + o];
        const float sc = pick<NP>(ac, p) + lds[T::o_bd + LAYER * 2 * H + H + o];
        float gz = lds[T::o_bx + LAYER * 2 * H + o];
        float gc = lds[T::o_bx + LAYER * 2 * H + H + o];
#pragma unroll
        for (int s = 0; s < T::SEG; ++s) {
            const float* pr = lds + T::o_gp + pb[s] + (LAYER * T::SEG + s) * 2 * H;
            gz = fmaf(wj[s], pr[o], gz);
            gc = fmaf(wj[s], pr[H + o], gc);
        }
        const float z = sigm(gz * sz);
        const float c = tanh_c(gc * sc);
        const float hp = ring[(q & (R - 1)) * H + o];
        const float hn = (1.f - z) * c + z * hp;
        if (LAYER + 1 < L) {
            constexpr int R2 = T::ring_len(LAYER + 1 < L ? LAYER + 1 : LAYER);
            lds[T::o_ring + T::ring_off(LAYER + 1 < L ? LAYER + 1 : LAYER) + (q & (R2 - 1)) * H + o] = hn;
        }
        if (p == NP - 1) lds[T::o_hcat + LAYER * H + o] = hn;
    }
    __builtin_amdgcn_sched_barrier(0);
}

// The same three streams over the bf16 image (W16 instantiations; layout: Bl6W16Layout).  One 16-byte load holds slices
// 2g (low halves) and 2g + 1 (high halves) of a lane's inputs; they are widened and accumulated slice 2g first, input by
// input, into the accumulator the fp32 form uses - the same FMAs in the same order on the rounded weights.
template <class T, int LAYER>
__device__ __forceinline__ void skip_fma16(const float* lds, const uint4& w, int g, int hp, float& acc) {
    const float4 x0 = *reinterpret_cast<const float4*>(lds + T::o_hcat + LAYER * H + 32 * g + 4 * hp);
    const float4 x1 = *reinterpret_cast<const float4*>(lds + T::o_hcat + LAYER * H + 32 * g + 16 + 4 * hp);
    acc = fmaf(w16_lo(w.x), x0.x, acc); acc = fmaf(w16_lo(w.y), x0.y, acc);
    acc = fmaf(w16_lo(w.z), x0.z, acc); acc = fmaf(w16_lo(w.w), x0.w, acc);
    acc = fmaf(w16_hi(w.x), x1.x, acc); acc = fmaf(w16_hi(w.y), x1.y, acc);
    acc = fmaf(w16_hi(w.z), x1.z, acc); acc = fmaf(w16_hi(w.w), x1.w, acc);
}
template <class T, int LAYER>
__device__ __forceinline__ void skip_slice16(const float* lds, __amdgpu_buffer_rsrc_t wsk, float (&sacc)[T::S / 128]) {
    const int hr = threadIdx.x >> 2, hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < T::S / 128; ++ps)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint4 w = buf_ld4u(wsk, (unsigned)((hr + 128 * ps) * 4 + hp) * 16u, (unsigned)((LAYER * 2 + g) * T::S) * 64u);
            skip_fma16<T, LAYER>(lds, w, g, hp, sacc[ps]);
        }
}
template <class T, int LAYER>
__device__ __forceinline__ void skip_issue(__amdgpu_buffer_rsrc_t wsk, uint4 (&wsl)[2 * (T::S / 128)]) {
    const int hr = threadIdx.x >> 2, hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < T::S / 128; ++ps)
#pragma unroll
        for (int g = 0; g < 2; ++g)
            wsl[ps * 2 + g] = buf_ld4u(wsk, (unsigned)((hr + 128 * ps) * 4 + hp) * 16u, (unsigned)((LAYER * 2 + g) * T::S) * 64u);
}
template <class T, int LAYER>
__device__ __forceinline__ void skip_consume(const float* lds, const uint4 (&wsl)[2 * (T::S / 128)],
                                             float (&sacc)[T::S / 128]) {
    const int hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < T::S / 128; ++ps)
#pragma unroll
        for (int g = 0; g < 2; ++g) skip_fma16<T, LAYER>(lds, wsl[ps * 2 + g], g, hp, sacc[ps]);
}
// rows x NI mat-vec over image section [NI / 32][rows][4][4 words]: a0 takes the even slices, a1 the odd ones, as below
template <int ROWS, int NI>
__device__ __forceinline__ void tiled_matvec16(__amdgpu_buffer_rsrc_t wt, const float* bias, const float* x, float* y,
                                               bool relu) {
    const int hr = threadIdx.x >> 2, hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < ROWS / 128; ++ps) {
        const int row = hr + 128 * ps;
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int mm = 0; mm < NI / 16; mm += 2) {
            const uint4 w = buf_ld4u(wt, (unsigned)(row * 4 + hp) * 16u, (unsigned)((mm / 2) * ROWS) * 64u);
            const float4 x0 = *reinterpret_cast<const float4*>(x + 16 * mm + 4 * hp);
            const float4 x1 = *reinterpret_cast<const float4*>(x + 16 * (mm + 1) + 4 * hp);
            a0 = fmaf(w16_lo(w.x), x0.x, a0); a0 = fmaf(w16_lo(w.y), x0.y, a0);
            a0 = fmaf(w16_lo(w.z), x0.z, a0); a0 = fmaf(w16_lo(w.w), x0.w, a0);
            a1 = fmaf(w16_hi(w.x), x1.x, a1); a1 = fmaf(w16_hi(w.y), x1.y, a1);
            a1 = fmaf(w16_hi(w.z), x1.z, a1); a1 = fmaf(w16_hi(w.w), x1.w, a1);
        }
        float v = sum4(a0 + a1);
        if (hp == 0) {
            v += bias[row];
            y[row] = relu ? fmaxf(v, 0.f) : v;
        }
        if (ps + 1 < ROWS / 128) __builtin_amdgcn_sched_barrier(0);     // <= 8 loads (one pass of rows) in flight
    }
}

// ... and over the FP8 image (W8 instantiations; layout: Bl6W8Layout).  One 16-byte load holds the four slices 4g .. 4g + 3
// of a lane's inputs - for out_skip all 64 inputs of a layer's row quarter; w8_slices widens them to code * 2^-e_row, and
// they are accumulated slice by slice, input by input, into the accumulators the fp32 form uses.  The rows' 2^-e sit in LDS
// at w8_o_sc: [L][S] out_skip, [O1] out_1, [NO] out_2 - behind the kernel's carve, except for the nets that keep out_1 slices
// resident (W1L > 0, LDS full): there the resident slices stay codes (a quarter of the fp32 slices' room, one 16-byte LDS read
// for all four, widened at every step) and the scales follow them inside the W1L region.
template <class T> constexpr int w8_sc_floats() { return L * T::S + T::O1 + (T::KIND == SWN_KIND_SOFTMAX ? T::NO : 0); }
template <class T> constexpr int w8_o_sc() { return T::W1L > 0 ? T::o_w1l + (T::W1L / 4) * T::O1 * 16 : T::o_end; }
template <class T> constexpr size_t w8_lds_bytes() {
    static_assert(T::W1L % 4 == 0 && (T::W1L == 0 || w8_o_sc<T>() + w8_sc_floats<T>() <= T::o_end), "codes and scales fit the W1L region");
    return T::W1L > 0 ? T::lds_bytes : T::lds_bytes + (size_t)w8_sc_floats<T>() * sizeof(float);
}
template <class T, int LAYER>
__device__ __forceinline__ void skip_fma8(const float* lds, const uint4& w, int row, int hp, float& acc) {
    float4 s[4];
    w8_slices(w, lds[w8_o_sc<T>() + LAYER * T::S + row], s);
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
        const float4 x = *reinterpret_cast<const float4*>(lds + T::o_hcat + LAYER * H + 16 * mm + 4 * hp);
        acc = fmaf(s[mm].x, x.x, acc); acc = fmaf(s[mm].y, x.y, acc);
        acc = fmaf(s[mm].z, x.z, acc); acc = fmaf(s[mm].w, x.w, acc);
    }
}
template <class T, int LAYER>
__device__ __forceinline__ void skip_slice8(const float* lds, __amdgpu_buffer_rsrc_t wsk, float (&sacc)[T::S / 128]) {
    const int hr = threadIdx.x >> 2, hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < T::S / 128; ++ps) {
        const uint4 w = buf_ld4u(wsk, (unsigned)((hr + 128 * ps) * 4 + hp) * 16u, (unsigned)(LAYER * T::S) * 64u);
        skip_fma8<T, LAYER>(lds, w, hr + 128 * ps, hp, sacc[ps]);
    }
}
template <class T, int LAYER>
__device__ __forceinline__ void skip_issue(__amdgpu_buffer_rsrc_t wsk, uint4 (&wsl)[T::S / 128]) {
    const int hr = threadIdx.x >> 2, hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < T::S / 128; ++ps)
        wsl[ps] = buf_ld4u(wsk, (unsigned)((hr + 128 * ps) * 4 + hp) * 16u, (unsigned)(LAYER * T::S) * 64u);
}
template <class T, int LAYER>
__device__ __forceinline__ void skip_consume(const float* lds, const uint4 (&wsl)[T::S / 128], float (&sacc)[T::S / 128]) {
    const int hr = threadIdx.x >> 2, hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < T::S / 128; ++ps) skip_fma8<T, LAYER>(lds, wsl[ps], hr + 128 * ps, hp, sacc[ps]);
}
// rows x NI mat-vec over image section [NI / 64][rows][4][4 words]; sc: the rows' 2^-e in LDS.  a0 takes the even slices,
// a1 the odd ones, each in rising order, as below
template <int ROWS, int NI>
__device__ __forceinline__ void tiled_matvec8(__amdgpu_buffer_rsrc_t wt, const float* bias, const float* sc, const float* x,
                                              float* y, bool relu) {
    static_assert(NI % 64 == 0, "whole image slices");
    const int hr = threadIdx.x >> 2, hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < ROWS / 128; ++ps) {
        const int row = hr + 128 * ps;
        const float scale = sc[row];
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int g = 0; g < NI / 64; ++g) {
            const uint4 w = buf_ld4u(wt, (unsigned)(row * 4 + hp) * 16u, (unsigned)(g * ROWS) * 64u);
            float4 s[4];
            w8_slices(w, scale, s);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 xv = *reinterpret_cast<const float4*>(x + 16 * (4 * g + k) + 4 * hp);
                float& acc = (k & 1) ? a1 : a0;
                acc = fmaf(s[k].x, xv.x, acc); acc = fmaf(s[k].y, xv.y, acc);
                acc = fmaf(s[k].z, xv.z, acc); acc = fmaf(s[k].w, xv.w, acc);
            }
        }
        float v = sum4(a0 + a1);
        if (hp == 0) {
            v += bias[row];
            y[row] = relu ? fmaxf(v, 0.f) : v;
        }
        if (ps + 1 < ROWS / 128) __builtin_amdgcn_sched_barrier(0);     // <= 4 loads (one pass of rows) in flight
    }
}

// out_skip slice of one layer, 4 lanes per row, weights streamed from the lane-tiled copy.
template <class T, int LAYER, int WK = WK_F32>
__device__ __forceinline__ void skip_slice(const float* lds, __amdgpu_buffer_rsrc_t wsk2,
                                           float (&sacc)[T::S / 128]) {
    if constexpr (WK == WK_BF16) { skip_slice16<T, LAYER>(lds, wsk2, sacc); return; }
    if constexpr (WK == WK_E4M3) { skip_slice8<T, LAYER>(lds, wsk2, sacc); return; }
    constexpr int layer = LAYER;
    const int hr = threadIdx.x >> 2, hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < T::S / 128; ++ps) {
        const int row = hr + 128 * ps;
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) {
            const float4 w = buf_ld4(wsk2, (unsigned)(row * 4 + hp) * 16u, (unsigned)((layer * 4 + mm) * T::S) * 64u);
            const float4 x = *reinterpret_cast<const float4*>(lds + T::o_hcat + layer * H + 16 * mm + 4 * hp);
            sacc[ps] = fmaf(w.x, x.x, sacc[ps]); sacc[ps] = fmaf(w.y, x.y, sacc[ps]);
            sacc[ps] = fmaf(w.z, x.z, sacc[ps]); sacc[ps] = fmaf(w.w, x.w, sacc[ps]);
        }
    }
}

// Software-pipelined form: the weights of slice LAYER are issued into registers one phase ahead and
// stay in flight across the LDS-only barrier.
template <class T, int LAYER>
__device__ __forceinline__ void skip_issue(__amdgpu_buffer_rsrc_t wsk2, float4 (&wsl)[4 * (T::S / 128)]) {
    const int hr = threadIdx.x >> 2, hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < T::S / 128; ++ps)
#pragma unroll
        for (int mm = 0; mm < 4; ++mm)
            wsl[ps * 4 + mm] = buf_ld4(wsk2, (unsigned)((hr + 128 * ps) * 4 + hp) * 16u,
                                       (unsigned)((LAYER * 4 + mm) * T::S) * 64u);
}
template <class T, int LAYER>
__device__ __forceinline__ void skip_consume(const float* lds, const float4 (&wsl)[4 * (T::S / 128)],
                                             float (&sacc)[T::S / 128]) {
    const int hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < T::S / 128; ++ps)
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) {
            const float4 w = wsl[ps * 4 + mm];
            const float4 x = *reinterpret_cast<const float4*>(lds + T::o_hcat + LAYER * H + 16 * mm + 4 * hp);
            sacc[ps] = fmaf(w.x, x.x, sacc[ps]); sacc[ps] = fmaf(w.y, x.y, sacc[ps]);
            sacc[ps] = fmaf(w.z, x.z, sacc[ps]); sacc[ps] = fmaf(w.w, x.w, sacc[ps]);
        }
}

// rows x NI mat-vec, 4 lanes per row, lane-tiled weights [NI/16][rows][4][4] streamed from L2.
template <int ROWS, int NI, int WK = WK_F32>
__device__ __forceinline__ void tiled_matvec(__amdgpu_buffer_rsrc_t wt, const float* bias,
                                             const float* x, float* y, bool relu, [[maybe_unused]] const float* sc = nullptr) {
    if constexpr (WK == WK_BF16) { tiled_matvec16<ROWS, NI>(wt, bias, x, y, relu); return; }
    if constexpr (WK == WK_E4M3) { tiled_matvec8<ROWS, NI>(wt, bias, sc, x, y, relu); return; }
    const int hr = threadIdx.x >> 2, hp = threadIdx.x & 3;
#pragma unroll
    for (int ps = 0; ps < ROWS / 128; ++ps) {
        const int row = hr + 128 * ps;
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int mm = 0; mm < NI / 16; mm += 2) {
            const float4 w0 = buf_ld4(wt, (unsigned)(row * 4 + hp) * 16u, (unsigned)(mm * ROWS) * 64u);
            const float4 w1 = buf_ld4(wt, (unsigned)(row * 4 + hp) * 16u, (unsigned)((mm + 1) * ROWS) * 64u);
            const float4 x0 = *reinterpret_cast<const float4*>(x + 16 * mm + 4 * hp);
            const float4 x1 = *reinterpret_cast<const float4*>(x + 16 * (mm + 1) + 4 * hp);
            a0 = fmaf(w0.x, x0.x, a0); a0 = fmaf(w0.y, x0.y, a0); a0 = fmaf(w0.z, x0.z, a0); a0 = fmaf(w0.w, x0.w, a0);
            a1 = fmaf(w1.x, x1.x, a1); a1 = fmaf(w1.y, x1.y, a1); a1 = fmaf(w1.z, x1.z, a1); a1 = fmaf(w1.w, x1.w, a1);
            if ((mm & 7) == 6 && mm + 2 < NI / 16) __builtin_amdgcn_sched_barrier(0);   // <= 8 loads in flight
        }
        float v = sum4(a0 + a1);
        if (hp == 0) {
            v += bias[row];
            y[row] = relu ? fmaxf(v, 0.f) : v;
        }
    }
}

template <bool POOL, bool MODELS, int WK = WK_F32> struct B6ArgsOf;
template <> struct B6ArgsOf<false, false> { using type = Bl6Args; };
template <> struct B6ArgsOf<true, false> { using type = Bl6PoolArgs; };
template <> struct B6ArgsOf<true, true> { using type = Bl6PoolModelsArgs; };
template <int WK> struct B6ArgsOf<false, false, WK> { using type = Bl6ImageArgs; };       // every stored format but fp32
template <int WK> struct B6ArgsOf<true, false, WK> { using type = Bl6PoolImageArgs; };
template <int WK> struct B6ArgsOf<true, true, WK> { using type = Bl6PoolModelsImageArgs; };
__device__ __forceinline__ const Bl6Args& pool_or_launch(const Bl6Args& launch, const Bl6Args&) { return launch; }
__device__ __forceinline__ const Bl6Args& pool_or_launch(const Bl6PoolArgs&, const Bl6Args& entry) { return entry; }
__device__ __forceinline__ const Bl6Args& pool_or_launch(const Bl6PoolWideArgs&, const Bl6Args& entry) { return entry; }
// (a wide launch has one argument struct for every format: its rows carry the images)
template <bool POOL, bool MODELS, int WK, bool WIDE>
using B6KernelArgs = typename std::conditional<WIDE, Bl6PoolWideArgs, typename B6ArgsOf<POOL, MODELS, WK>::type>::type;

// EXT = false: the classic instantiation (host-drawn noise stream, zero seed) - the code the round-1 measurements
// belong to, kept instruction for instruction; EXT = true adds the in-kernel generator / noise dump / seed waveform.
// STREAM (with EXT only): one chunk of a streamed decode (swn_decode_chunk) - steps [step0, step0 + n_steps) at absolute
// positions and generator counters, chunk-local out / heads / noise / forced rows; when resuming, the rings and the sample
// window come from the session instead of the prologue, and they go back to it at the end.  The step itself is the same code.
// POOL (with STREAM): one entry of a decode pool (swn_decode_pool_chunk); `a` holds the workgroup's entry as a batch-1 chunk
// (swn_pool_entry_args), b = 0.  MODELS (with POOL): the entry's weights are those of its model (SwnPoolModels).
// WK = WK_BF16 (W16; with EXT): out_skip, out_1 and the softmax out_2 stream from the bf16 image `img` instead of the fp32
// lane-tiled copies, and the LDS-resident out_1 slices are widened from it; every other load and every FMA is the fp32 code.
// WK = WK_E4M3 (W8): the same over the FP8 image `img`, whose row scales are copied into LDS behind the carve.  `img` is the
// launch's image ka.img, or with MODELS the image of the entry's model, ka.img[model] - read through the model index once, so
// the one-time loads (resident out_1 slices, W8 codes and row scales) and the three streams all take the entry's own image.
// WIDE (with POOL, without MODELS): the entry, its model's packed buffer and its image are row blockIdx.x of the launch's device
// table (swn_decode_pool_chunk_wide), whatever the format.
template <class T, bool STREAM = false, bool POOL = false, bool MODELS = false, int WK = WK_F32, bool WIDE = false>
__global__ __launch_bounds__(NT) void decode_bl6_kernel(const B6KernelArgs<POOL, MODELS, WK, WIDE> ka) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr bool W16 = WK == WK_BF16, W8 = WK == WK_E4M3;
    static_assert(WK == WK_F32 || T::EXT, "stored formats: extended instantiations only");
    Bl6Args pa;                                            // POOL: this workgroup's entry as a batch-1 chunk
    [[maybe_unused]] const void* img_e = nullptr;          // stored formats with MODELS: the image of this entry's model
    // stored formats: the image every section below is read from (one model: the launch's, read where it is used)
    [[maybe_unused]] auto img = [&]() -> const void* {
        if constexpr (WK == WK_F32) return nullptr;
        else if constexpr (MODELS || WIDE) return img_e;
        else return ka.img;
    };
    if constexpr (WIDE) {
        static_assert(POOL && !MODELS && STREAM && T::EXT, "a wide launch is a pool launch whose rows name the models");
        pa = ka.c;
        const SwnPoolWideRow row = swn_pool_wide_row(ka.rows);
        pa.P = row.model;
        img_e = row.image;
        if (!swn_pool_entry_args(pa, row.e, T::SEG, T::KIND == SWN_KIND_SOFTMAX ? T::Q : T::SEG, T::NO)) return;
        pa.sess += (size_t)row.e.slot * T::sess_floats;
    } else if constexpr (POOL) {
        static_assert(STREAM && T::EXT, "pools run the streamed extended mode");
        pa = ka.c;
        if constexpr (MODELS && WK != WK_F32) {            // the entry's model names its packed buffer and its image
            const int mi = swn_pool_model_index(ka.m);
            pa.P = ka.m.p[mi];
            img_e = ka.img[mi];
        } else if constexpr (MODELS) pa.P = swn_pool_model(ka.m);
        if (!swn_pool_entry_args(pa, ka.t, T::SEG, T::KIND == SWN_KIND_SOFTMAX ? T::Q : T::SEG, T::NO)) return;
        pa.sess += (size_t)swn_pool_slot(ka.t) * T::sess_floats;
    }
    const Bl6Args& a = pool_or_launch(ka, pa);
    constexpr int SEG = T::SEG, S = T::S, KIND = T::KIND;
    constexpr bool EXT = T::EXT;
    const int tid = threadIdx.x, b = POOL ? 0 : blockIdx.x;
    const float* __restrict__ P = a.P;
    const int U = a.U;
    static_assert(!STREAM || EXT, "streamed chunks run the extended mode");
    const int s0 = STREAM ? a.step0 : 0;                  // absolute index of step i = 0
    const bool resume = STREAM && a.resume;
    // conditioning frame of the first step: the frame pair the one-shot decode holds in LDS when it reaches that step
    const int fb0 = STREAM ? cmax(0, 1 - SEG + s0 * SEG) / U : 0;

    // ---- one-time loads: LDS constants, register-resident dilated-conv weights
    for (int e = tid; e < T::o_end; e += NT) lds[e] = 0.f;
    __syncthreads();
    for (int e = tid; e < L * 2 * H; e += NT) { lds[T::o_bx + e] = P[a.y.bx + e]; lds[T::o_bd + e] = P[a.y.bd + e]; }
    for (int e = tid; e < U; e += NT) lds[T::o_wup + e] = P[a.y.wup + e];
    for (int e = tid; e < H; e += NT) lds[T::o_cz + e] = P[a.y.cb + e];
    // head biases live in LDS: a global load consumed inside a phase would drain (in-order vmcnt) every
    // weight load that is deliberately in flight
    for (int e = tid; e < S; e += NT) lds[T::o_bias + e] = P[a.y.bsk + e];
    for (int e = tid; e < T::O1; e += NT) lds[T::o_bias + S + e] = P[a.y.b1 + e];
    if (KIND == SWN_KIND_SOFTMAX)
        for (int e = tid; e < T::NO; e += NT) lds[T::o_bias + S + T::O1 + e] = P[a.y.b2 + e];
    if (KIND == SWN_KIND_LAPLACE) {
        for (int e = tid; e < 2 * H; e += NT) { lds[T::o_cz + H + e] = P[a.y.cv + e]; lds[T::o_cz + 3 * H + e] = P[a.y.cc + e]; }
        for (int e = tid; e < T::NO * S; e += NT) lds[T::o_w2 + e] = P[a.y.w2 + (size_t)(e / S) * r4(S) + (e % S)];
        for (int e = tid; e < T::NO; e += NT) lds[T::o_w2 + T::NO * S + e] = P[a.y.b2 + e];
        if constexpr (W16) {
            // the resident out_1 slices hold the rounded values, widened once: slice mm is half mm & 1 of image slice mm / 2
            const unsigned* w1i = reinterpret_cast<const unsigned*>(
                static_cast<const char*>(img()) + w16_layout(S, T::O1, T::NO, false).w1);
            for (int e = tid; e < T::W1L * T::O1 * 16; e += NT) {
                const int mm = e / (T::O1 * 16);
                const unsigned w = w1i[(mm >> 1) * T::O1 * 16 + e % (T::O1 * 16)];
                lds[T::o_w1l + e] = (mm & 1) ? w16_hi(w) : w16_lo(w);
            }
        } else if constexpr (W8) {
            // ... or stay codes: the first W1L / 4 image slices as they lie in the image (bit patterns, not numbers)
            const unsigned* w1i = reinterpret_cast<const unsigned*>(
                static_cast<const char*>(img()) + w8_layout(S, T::O1, T::NO, false).w1);
            unsigned* dst = reinterpret_cast<unsigned*>(lds + T::o_w1l);
            for (int e = tid; e < (T::W1L / 4) * T::O1 * 16; e += NT) dst[e] = w1i[e];
        } else
        for (int e = tid; e < T::W1L * T::O1 * 16; e += NT) lds[T::o_w1l + e] = P[a.y.w12 + e];
    }
    if constexpr (W8) {   // the rows' 2^-e: the three scale sections of the image are one run of floats
        const float* sc = reinterpret_cast<const float*>(
            static_cast<const char*>(img()) + w8_layout(S, T::O1, T::NO, KIND == SWN_KIND_SOFTMAX).ssk);
        for (int e = tid; e < w8_sc_floats<T>(); e += NT) lds[w8_o_sc<T>() + e] = sc[e];
    }
    // conditioning frames are copied 16 B per lane through a buffer resource (32-bit offsets)
    const __amdgpu_buffer_rsrc_t condr =
        make_rsrc(a.cond + (size_t)b * a.Tf * a.N, (unsigned)((size_t)a.Tf * a.N * sizeof(float)));
    auto load_frame = [&](int fr) {
        float* dst = lds + T::o_gp + (fr & 1) * T::PF;
#pragma unroll
        for (int it = 0; it < (T::PF / 4 + NT - 1) / NT; ++it) {
            const int e4 = it * NT + tid;
            if (e4 < T::PF / 4)
                *reinterpret_cast<float4*>(dst + 4 * e4) =
                    buf_ld4(condr, (unsigned)tid * 16u, (unsigned)(fr * a.N * 4 + it * NT * 16));
        }
    };
    for (int fr = fb0; fr < fb0 + 2 && fr < a.Tf; ++fr) load_frame(fr);
    float wreg[L][2][16];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const float4* src = reinterpret_cast<const float4*>(P + a.y.wd2 + ((size_t)l * NT + tid) * 32);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const float4 t = src[v];
            if (l < T::NREG) {
                wreg[l][v >> 2][4 * (v & 3) + 0] = t.x; wreg[l][v >> 2][4 * (v & 3) + 1] = t.y;
                wreg[l][v >> 2][4 * (v & 3) + 2] = t.z; wreg[l][v >> 2][4 * (v & 3) + 3] = t.w;
            } else {
                *reinterpret_cast<float4*>(lds + T::o_wl + (((l - T::NREG) * 8 + v) * NT + tid) * 4) = t;
                wreg[l][v >> 2][4 * (v & 3) + 0] = 0.f; wreg[l][v >> 2][4 * (v & 3) + 1] = 0.f;
                wreg[l][v >> 2][4 * (v & 3) + 2] = 0.f; wreg[l][v >> 2][4 * (v & 3) + 3] = 0.f;
            }
        }
    }
    __syncthreads();
    const float* sess_b = STREAM ? a.sess + (size_t)b * T::sess_floats : nullptr;
    if (resume) {
        for (int e = tid; e < T::ring_off(L); e += NT) lds[T::o_ring + e] = sess_b[e];
        __syncthreads();
    }

    int fb = fb0, tb = fb0 * U;               // base conditioning frame resident in buffer fb&1
    const int p = tid & 7;
    const int n_pro = RF - SEG + 1;

    // conditioning taps of the position this lane finishes: upsampler weight and frame buffer offset
    // `single`: one position per pass (prologue, or seg == 1): every lane takes the taps of q0 itself,
    // because the split gate epilogue runs on lanes 0 AND 1 of an octet for that one position.
    auto cond_taps = [&](int q0, float (&wj)[SEG], int (&pb)[SEG], bool single) {
        const int t0 = q0 - RF;
        const int tlo = t0 < 0 ? 0 : t0;
        if (tlo >= tb + U) {                  // step crossed into the next frame: refill the free buffer
            fb += 1; tb += U;
            if (fb + 1 < a.Tf) load_frame(fb + 1);
        }
#pragma unroll
        for (int s = 0; s < SEG; ++s) {
            int tt = t0 + (single ? 0 : p) + s; tt = tt < 0 ? 0 : tt;
            int rel = tt - tb;
            int fsel = fb;
            if (rel >= U) { rel -= U; fsel = fb + 1; }
            rel = rel < U ? rel : U - 1;
            wj[s] = lds[T::o_wup + rel];
            pb[s] = (fsel & 1) * T::PF;
        }
    };

    // input layer h0 = softsign(causal(lift(S)))  (wave 0; fused wav_conv+causal taps).
    // Prologue form: all seed samples are zero / the mu-law zero index, only tap validity matters.
    auto input_seed = [&](int q) {
        if (tid < H) {
            const int o = tid;
            constexpr int R0 = T::ring_len(0);
            float acc = c_b;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int r = q - (1 - k);
                if (KIND == SWN_KIND_LAPLACE) {
                    if (r >= -(SEG - 1)) acc += fmaf(k ? c_v1 : c_v0, 0.f, k ? c_c1 : c_c0);
                } else {
                    if (r >= 0) acc += P[a.y.ct + ((size_t)k * T::Q + T::Q / 2) * H + o];
                }
            }
            lds[T::o_ring + (q & (R0 - 1)) * H + o] = ssign(acc);
        }
    };
    // Generation form: the sample window lives in registers of wave 0 (uniform across its lanes):
    // win[] = S[qe-WN+1 .. qe], qe = last position whose input sample is known.
    constexpr int WNF = KIND == SWN_KIND_LAPLACE ? T::WN : 1, WNI = KIND == SWN_KIND_SOFTMAX ? T::WN : 1;
    float win[WNF];
    int iwin[WNI];
#pragma unroll
    for (int k = 0; k < WNF; ++k) win[k] = 0.f;
#pragma unroll
    for (int k = 0; k < WNI; ++k) iwin[k] = T::Q / 2;
    if (EXT && a.seed) {       // seed waveform `audio` of batch_fast_generate: the newest SEG samples / the newest class
        if constexpr (KIND == SWN_KIND_LAPLACE) {
#pragma unroll
            for (int j = 0; j < SEG; ++j) win[WNF - SEG + j] = reinterpret_cast<const float*>(a.seed)[(size_t)b * SEG + j];
        } else {
            iwin[WNI - 1] = reinterpret_cast<const int*>(a.seed)[b];
        }
    }
    if (resume) {              // the window as the previous chunk left it
#pragma unroll
        for (int k = 0; k < WNF; ++k) if (KIND == SWN_KIND_LAPLACE) win[k] = sess_b[T::ring_off(L) + k];
#pragma unroll
        for (int k = 0; k < WNI; ++k) if (KIND == SWN_KIND_SOFTMAX) iwin[k] = __builtin_bit_cast(int, sess_b[T::ring_off(L) + k]);
    }
    auto input_gen = [&](int q0n) {
        if (tid < H) {
            const int o = tid;
            constexpr int R0 = T::ring_len(0);
#pragma unroll
            for (int j = 0; j < SEG; ++j) {
                float acc = c_b;
                if constexpr (KIND == SWN_KIND_LAPLACE) {
                    acc += fmaf(c_v0, win[T::WN - SEG + j - 1], c_c0);
                    acc += fmaf(c_v1, win[T::WN - SEG + j], c_c1);
                } else {
                    acc += P[a.y.ct + ((size_t)0 * T::Q + iwin[T::WN - SEG + j - 1]) * H + o];
                    acc += P[a.y.ct + ((size_t)1 * T::Q + iwin[T::WN - SEG + j]) * H + o];
                }
                lds[T::o_ring + ((q0n + j) & (R0 - 1)) * H + o] = ssign(acc);
            }
        }
    };
    // Sampling noise, staged in LDS off the critical path (host stream or in-kernel generator: swn_noise.hpp).
    // Laplace: wave 1 transforms the draws of a whole chunk of 64 future steps at once (lane = step):
    //   tn = sign(e) * log1p(-2|e|)   (cswnv_shift1.py:374-376); chunk c lives in buffer c & 3 and is filled two chunks
    //   ahead of its first reader, so the filler needs no barrier of its own.
    auto noise_chunk = [&](int c) {
        if (EXT && KIND == SWN_KIND_LAPLACE && tid >= 64 && tid < 128) {
            const int k = tid - 64, step = c * T::NZC + k;
            if (step < a.n_steps) {
#pragma unroll
                for (int j = 0; j < SEG; ++j) {
                    const float e = swn_noise_laplace_at(a.nz, b, step, s0 + step, j, a.n_steps, SEG);
                    const float sg = (e > 0.f) ? 1.f : ((e < 0.f) ? -1.f : 0.f);
                    lds[T::o_tnz + ((c & (T::NZB - 1)) * T::NZC + k) * SEG + j] = sg * log1pf(-2.f * fabsf(e));
                }
            }
        }
    };
    // softmax: wave 2 fetches / draws the Q Exp(1) deviates of step `step` (lane t: classes 4t..4t+3) into buffer step & 1
    auto q_ahead = [&](int step) {
        if constexpr (KIND == SWN_KIND_SOFTMAX) {
            static_assert(T::Q == 256, "one float4 of classes per lane");
            if (tid >= 128 && tid < 192 && step < a.n_steps) {
                float4 q4;
                if constexpr (EXT) q4 = swn_noise_exp1x4_at(a.nz, b, step, s0 + step, tid - 128, a.n_steps, T::Q);
                else q4 = *reinterpret_cast<const float4*>(a.noise + ((size_t)b * a.n_steps + step) * T::Q + 4 * (tid - 128));
                *reinterpret_cast<float4*>(lds + T::o_tnz + (step & 1) * T::Q + 4 * (tid - 128)) = q4;
            }
        }
    };
    // classic mode: wave 1 transforms the deviate of the next step, its raw draw fetched one call earlier still
    float e_next = 0.f;
    auto noise_ahead = [&](int step) {
        if (!EXT && KIND == SWN_KIND_LAPLACE && tid >= 64 && tid < 64 + SEG) {
            const int j = tid - 64;
            if (step < a.n_steps) {
                const float e = e_next;
                const float sg = (e > 0.f) ? 1.f : ((e < 0.f) ? -1.f : 0.f);
                lds[T::o_tnz + (step & 1) * 8 + j] = sg * log1pf(-2.f * fabsf(e));
            }
            if (step + 1 < a.n_steps) e_next = a.noise[((size_t)b * a.n_steps + step + 1) * SEG + j];
        }
    };
    if (!EXT && KIND == SWN_KIND_LAPLACE && tid >= 64 && tid < 64 + SEG && a.n_steps > 0)
        e_next = a.noise[(size_t)b * a.n_steps * SEG + (tid - 64)];
    noise_chunk(0);
    noise_chunk(1);
    q_ahead(0);

    // ---- prologue: seed positions 0..rf-seg, one position per pass (cswnv_shift1.py:321-334)
#pragma unroll 1
    for (int q = resume ? n_pro : 0; q < n_pro; ++q) {
        float wj[SEG]; int pb[SEG];
        cond_taps(q, wj, pb, true);
        input_seed(q);
        lds_barrier();
        layer_phase<T, 0, 1>(lds, wreg[0], q, wj, pb); lds_barrier();
        layer_phase<T, 1, 1>(lds, wreg[1], q, wj, pb); lds_barrier();
        layer_phase<T, 2, 1>(lds, wreg[2], q, wj, pb); lds_barrier();
        layer_phase<T, 3, 1>(lds, wreg[3], q, wj, pb); lds_barrier();
        layer_phase<T, 4, 1>(lds, wreg[4], q, wj, pb); lds_barrier();
        layer_phase<T, 5, 1>(lds, wreg[5], q, wj, pb); lds_barrier();
    }

    // ---- generation (cswnv_shift1.py:348-402 / dswnv.py:338-374)
    // W16: the same three names over the sections of the bf16 image (half the bytes)
    // W8: over the code sections of the FP8 image (a quarter)
    constexpr unsigned WB = W8 ? 1 : W16 ? 2 : sizeof(float);
    [[maybe_unused]] const Bl6W16Layout y16 = w16_layout(S, T::O1, T::NO, KIND == SWN_KIND_SOFTMAX);
    [[maybe_unused]] const Bl6W8Layout y8 = w8_layout(S, T::O1, T::NO, KIND == SWN_KIND_SOFTMAX);
    auto wsrc = [&](size_t f32_off, [[maybe_unused]] size_t w16_off, [[maybe_unused]] size_t w8_off) -> const void* {
        if constexpr (W16) return static_cast<const char*>(img()) + w16_off;
        else if constexpr (W8) return static_cast<const char*>(img()) + w8_off;
        else return P + f32_off;
    };
    const __amdgpu_buffer_rsrc_t wsk2 = make_rsrc(wsrc(a.y.wsk2, y16.wsk, y8.wsk), (unsigned)(L * S * 64 * WB));
    const __amdgpu_buffer_rsrc_t w12 = make_rsrc(wsrc(a.y.w12, y16.w1, y8.w1), (unsigned)(T::O1 * S * WB));
    const __amdgpu_buffer_rsrc_t w22 = make_rsrc(wsrc(a.y.w22, y16.w2, y8.w2), (unsigned)(T::NO * T::O1 * WB));
#ifdef SWN_STAMP
    // diagnostic build only (tools/stamp_decode.py): per-phase cycle sums of wave 0 leave the kernel
    // through the `heads` debug buffer, which this build writes nothing else into.
    unsigned long long tacc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev = 0;
#define STAMP(k) { const unsigned long long tn = __builtin_amdgcn_s_memtime(); tacc[k] += tn - tprev; tprev = tn; }
#else
#define STAMP(k)
#endif
    input_gen(RF + 1 - SEG + s0 * SEG);
    noise_ahead(0);       // classic mode: visible to wave 0 after the barriers of step 0
    auto gen_step = [&](const int i) __attribute__((always_inline)) {
        const int q0 = RF + 1 - SEG + (s0 + i) * SEG;
        float wj[SEG]; int pb[SEG];
#ifdef SWN_STAMP
        tprev = __builtin_amdgcn_s_memtime();
#endif
        cond_taps(q0, wj, pb, SEG == 1);
        float sacc[S / 128];
#pragma unroll
        for (int ps = 0; ps < S / 128; ++ps) sacc[ps] = 0.f;
        [[maybe_unused]] float4 w1p[8];
        lds_barrier(); STAMP(0)
#ifdef SWN_NO_PREF
        if constexpr (false) {
#else
        if constexpr (S == 128 && SEG <= 2) {
#endif
            // out_skip weights are issued one phase ahead and stay in flight across the LDS-only barrier
            typename std::conditional<W8, uint4[1], typename std::conditional<W16, uint4[2], float4[4]>::type>::type wsl;
            layer_phase<T, 0, SEG>(lds, wreg[0], q0, wj, pb); skip_issue<T, 0>(wsk2, wsl); lds_barrier(); STAMP(1)
            layer_phase<T, 1, SEG>(lds, wreg[1], q0, wj, pb); skip_consume<T, 0>(lds, wsl, sacc); skip_issue<T, 1>(wsk2, wsl); lds_barrier(); STAMP(2)
            layer_phase<T, 2, SEG>(lds, wreg[2], q0, wj, pb); skip_consume<T, 1>(lds, wsl, sacc); skip_issue<T, 2>(wsk2, wsl); lds_barrier(); STAMP(3)
            layer_phase<T, 3, SEG>(lds, wreg[3], q0, wj, pb); skip_consume<T, 2>(lds, wsl, sacc); skip_issue<T, 3>(wsk2, wsl); lds_barrier(); STAMP(4)
            layer_phase<T, 4, SEG>(lds, wreg[4], q0, wj, pb); skip_consume<T, 3>(lds, wsl, sacc); skip_issue<T, 4>(wsk2, wsl); lds_barrier(); STAMP(5)
            layer_phase<T, 5, SEG>(lds, wreg[5], q0, wj, pb); skip_consume<T, 4>(lds, wsl, sacc); skip_issue<T, 5>(wsk2, wsl); lds_barrier(); STAMP(6)
            skip_consume<T, 5>(lds, wsl, sacc);
#ifdef SWN_W1PREF
            // out_1 weights: issued now, they fly during the reduction and the barrier
            if constexpr (WK == WK_F32) {
                const int hr = tid >> 2, hp = tid & 3;
#pragma unroll
                for (int mm = 0; mm < 8; ++mm)
                    w1p[mm] = buf_ld4(w12, (unsigned)(hr * 4 + hp) * 16u, (unsigned)(mm * T::O1) * 64u);
            }
#endif
        } else {
            layer_phase<T, 0, SEG>(lds, wreg[0], q0, wj, pb); lds_barrier(); STAMP(1)
            layer_phase<T, 1, SEG>(lds, wreg[1], q0, wj, pb); skip_slice<T, 0, WK>(lds, wsk2, sacc); lds_barrier(); STAMP(2)
            layer_phase<T, 2, SEG>(lds, wreg[2], q0, wj, pb); skip_slice<T, 1, WK>(lds, wsk2, sacc); lds_barrier(); STAMP(3)
            layer_phase<T, 3, SEG>(lds, wreg[3], q0, wj, pb); skip_slice<T, 2, WK>(lds, wsk2, sacc); lds_barrier(); STAMP(4)
            layer_phase<T, 4, SEG>(lds, wreg[4], q0, wj, pb); skip_slice<T, 3, WK>(lds, wsk2, sacc); lds_barrier(); STAMP(5)
            layer_phase<T, 5, SEG>(lds, wreg[5], q0, wj, pb); skip_slice<T, 4, WK>(lds, wsk2, sacc); lds_barrier(); STAMP(6)
            skip_slice<T, 5, WK>(lds, wsk2, sacc);
        }
        {
            const int hr = tid >> 2, hp = tid & 3;
#pragma unroll
            for (int ps = 0; ps < S / 128; ++ps) {
                const float v = sum4(sacc[ps]);
                if (hp == 0) lds[T::o_skip + hr + 128 * ps] = fmaxf(v + lds[T::o_bias + hr + 128 * ps], 0.f);
            }
        }
        lds_barrier(); STAMP(7)
        // softmax: wave 2 stages the draws of step i+1 (into the buffer wave 0 read in step i-1's tail, which is behind
        // this step's barriers) while the out_1 weights are in flight
        noise_ahead(i + 1);
        q_ahead(i + 1);
#ifndef SWN_W1PREF
        if constexpr (false) {
#else
        if constexpr (S == 128 && SEG <= 2 && WK == WK_F32) {
#endif
            const int hr = tid >> 2, hp = tid & 3;
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int mm = 0; mm < 8; mm += 2) {
                const float4 x0 = *reinterpret_cast<const float4*>(lds + T::o_skip + 16 * mm + 4 * hp);
                const float4 x1 = *reinterpret_cast<const float4*>(lds + T::o_skip + 16 * (mm + 1) + 4 * hp);
                a0 = fmaf(w1p[mm].x, x0.x, a0); a0 = fmaf(w1p[mm].y, x0.y, a0);
                a0 = fmaf(w1p[mm].z, x0.z, a0); a0 = fmaf(w1p[mm].w, x0.w, a0);
                a1 = fmaf(w1p[mm + 1].x, x1.x, a1); a1 = fmaf(w1p[mm + 1].y, x1.y, a1);
                a1 = fmaf(w1p[mm + 1].z, x1.z, a1); a1 = fmaf(w1p[mm + 1].w, x1.w, a1);
            }
            const float v = sum4(a0 + a1);
            if (hp == 0) lds[T::o_o1 + hr] = fmaxf(v + lds[T::o_bias + S + hr], 0.f);
        } else {
            if constexpr (T::W1L > 0) {
                // out_1, 128 x 128: the streamed slices are requested from L2 first, the resident ones come from LDS meanwhile
                constexpr int NG = S / 16 - T::W1L;
                const int hr = tid >> 2, hp = tid & 3;
                float4 wg[NG];
                [[maybe_unused]] float4 wl[4];                       // W8: the resident slices, widened from their codes
                if constexpr (W16) {
                    static_assert(T::W1L % 2 == 0 && NG % 2 == 0, "whole image slices on either side");
#pragma unroll
                    for (int g = 0; g < NG / 2; ++g) {
                        const uint4 w = buf_ld4u(w12, (unsigned)(hr * 4 + hp) * 16u, (unsigned)((T::W1L / 2 + g) * T::O1) * 64u);
                        wg[2 * g] = make_float4(w16_lo(w.x), w16_lo(w.y), w16_lo(w.z), w16_lo(w.w));
                        wg[2 * g + 1] = make_float4(w16_hi(w.x), w16_hi(w.y), w16_hi(w.z), w16_hi(w.w));
                    }
                } else if constexpr (W8) {
                    static_assert(T::W1L == 4 && NG == 4, "one image slice on either side");
                    const uint4 w = buf_ld4u(w12, (unsigned)(hr * 4 + hp) * 16u, (unsigned)((T::W1L / 4) * T::O1) * 64u);
                    const float scale = lds[w8_o_sc<T>() + L * S + hr];
                    w8_slices(*reinterpret_cast<const uint4*>(lds + T::o_w1l + (hr * 4 + hp) * 4), scale, wl);
                    w8_slices(w, scale, wg);
                } else
#pragma unroll
                for (int mm = 0; mm < NG; ++mm) wg[mm] = buf_ld4(w12, (unsigned)(hr * 4 + hp) * 16u, (unsigned)((T::W1L + mm) * T::O1) * 64u);
                float a0 = 0.f, a1 = 0.f;
#pragma unroll
                for (int mm = 0; mm < T::W1L; ++mm) {
                    float4 w0;
                    if constexpr (W8) w0 = wl[mm & 3];
                    else w0 = *reinterpret_cast<const float4*>(lds + T::o_w1l + ((mm * T::O1 + hr) * 4 + hp) * 4);
                    const float4 x0 = *reinterpret_cast<const float4*>(lds + T::o_skip + 16 * mm + 4 * hp);
                    float& acc = (mm & 1) ? a1 : a0;
                    acc = fmaf(w0.x, x0.x, acc); acc = fmaf(w0.y, x0.y, acc); acc = fmaf(w0.z, x0.z, acc); acc = fmaf(w0.w, x0.w, acc);
                }
#pragma unroll
                for (int mm = 0; mm < NG; ++mm) {
                    const float4 x0 = *reinterpret_cast<const float4*>(lds + T::o_skip + 16 * (T::W1L + mm) + 4 * hp);
                    float& acc = ((T::W1L + mm) & 1) ? a1 : a0;
                    acc = fmaf(wg[mm].x, x0.x, acc); acc = fmaf(wg[mm].y, x0.y, acc); acc = fmaf(wg[mm].z, x0.z, acc); acc = fmaf(wg[mm].w, x0.w, acc);
                }
                const float v = sum4(a0 + a1);
                if (hp == 0) lds[T::o_o1 + hr] = fmaxf(v + lds[T::o_bias + S + hr], 0.f);
            } else {
                tiled_matvec<T::O1, S, WK>(w12, lds + T::o_bias + S, lds + T::o_skip, lds + T::o_o1, true, lds + w8_o_sc<T>() + L * S);
            }
        }
        lds_barrier(); STAMP(8)

        if (KIND == SWN_KIND_LAPLACE) {
            if (tid < 64) {
                // out_2: NO <= 14 rows, 4 lanes per row, weights resident in LDS
                const int r = tid >> 2, pp = tid & 3;
                float acc = 0.f;
                if (r < T::NO) {
#pragma unroll
                    for (int mm = 0; mm < S / 16; ++mm) {
                        const float4 w = *reinterpret_cast<const float4*>(lds + T::o_w2 + r * S + 16 * mm + 4 * pp);
                        const float4 x = *reinterpret_cast<const float4*>(lds + T::o_o1 + 16 * mm + 4 * pp);
                        acc = fmaf(w.x, x.x, acc); acc = fmaf(w.y, x.y, acc);
                        acc = fmaf(w.z, x.z, acc); acc = fmaf(w.w, x.w, acc);
                    }
                }
                acc = sum4(acc);
                if (r < T::NO) acc += lds[T::o_w2 + T::NO * S + r];
                if (HEADS_ON && a.heads && pp == 0 && r < T::NO) a.heads[((size_t)b * a.n_steps + i) * T::NO + r] = acc;
                // park the NO head outputs in LDS; every lane re-reads them (same wave: LDS ops are in
                // order, the fences only pin the compiler)
                if (pp == 0 && r < T::NO) lds[T::o_o2 + r] = acc;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const float* o2 = lds + T::o_o2;
                {
#pragma clang fp contract(off)
                    // Laplace head, cswnv_shift1.py:368-391, evaluated uniformly by every lane of wave 0
                    // so the new samples are in registers for the next input layer (no LDS round trip).
                    float* outp = reinterpret_cast<float*>(a.out) + (size_t)b * a.n_steps * SEG + (size_t)i * SEG;
#pragma unroll
                    for (int j = 0; j < SEG; ++j) {
                        const float mu = o2[j];
                        const float bsc = sigm(o2[SEG + j]);                 // exp(logsigmoid(y))
                        float lpv = 0.f;
#pragma unroll
                        for (int k = 0; k < T::LPC; ++k) lpv += o2[2 * SEG + T::LPC - 1 - k] * win[T::WN - T::LPC + k];
                        
                        const float t = bsc * (EXT ? lds[T::o_tnz + (((i >> 6) & (T::NZB - 1)) * T::NZC + (i & (T::NZC - 1))) * SEG + j]
                                                   : lds[T::o_tnz + (i & 1) * 8 + j]);
                        float sv = (T::LPC > 0) ? (lpv + mu) - t : mu - t;
                        sv = fminf(fmaxf(sv, -1.f), 1.f);
                        if (tid == 0) outp[j] = sv;
                        const float fd = a.forced ? reinterpret_cast<const float*>(a.forced)[((size_t)b * a.n_steps + i) * SEG + j] : sv;
#pragma unroll
                        for (int k = 0; k + 1 < T::WN; ++k) win[k] = win[k + 1];
                        win[T::WN - 1] = fd;
                    }
                }
            }
        } else {
            constexpr int Q = T::Q;
            constexpr int QL = Q > 0 ? (Q + 63) / 64 : 1;     // classes per lane (this branch is also compiled for Laplace nets)
            tiled_matvec<T::NO, T::O1, WK>(w22, lds + T::o_bias + S + T::O1, lds + T::o_o1, lds + T::o_o2, false,
                                           lds + w8_o_sc<T>() + L * S + T::O1);
            lds_barrier();
            if (HEADS_ON && a.heads)
                for (int e = tid; e < T::NO; e += NT) a.heads[((size_t)b * a.n_steps + i) * T::NO + e] = lds[T::o_o2 + e];
            if (tid < 64) {
                // softmax head, dswnv.py:361-369: p = softmax(logits); p /= sum(p); index = argmax(p / q).
                // lane t owns classes 4t..4t+3 (one 16-byte LDS read each for logits and noise); exp(logit - max) is
                // evaluated once per class and kept in registers for the three passes.
                static_assert(KIND != SWN_KIND_SOFTMAX || QL == 4, "four classes per lane");
                const float4 l4 = *reinterpret_cast<const float4*>(lds + T::o_o2 + 4 * tid);
                const float4 q4 = *reinterpret_cast<const float4*>(lds + T::o_tnz + (i & 1) * Q + 4 * tid);
                const float lg[4] = {l4.x, l4.y, l4.z, l4.w}, qv[4] = {q4.x, q4.y, q4.z, q4.w};
                float ex[4];
                float m = fmaxf(fmaxf(lg[0], lg[1]), fmaxf(lg[2], lg[3]));
                for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
                float sum = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) { ex[k] = expf(lg[k] - m); sum += ex[k]; }
                for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
                float sum2 = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) { ex[k] = ex[k] / sum; sum2 += ex[k]; }
                for (int d = 32; d >= 1; d >>= 1) sum2 += __shfl_xor(sum2, d, 64);
                float best = -1.f; int bi = 0x7fffffff;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float r = (ex[k] / sum2) / qv[k];
                    if (r > best) { best = r; bi = 4 * tid + k; }
                }
                for (int d = 32; d >= 1; d >>= 1) {
                    const float ob = __shfl_xor(best, d, 64);
                    const int oi = __shfl_xor(bi, d, 64);
                    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
                }
                if (tid == 0) reinterpret_cast<int*>(a.out)[(size_t)b * a.n_steps + i] = bi;
                const int fd = a.forced ? reinterpret_cast<const int*>(a.forced)[(size_t)b * a.n_steps + i] : bi;
#pragma unroll
                for (int k = 0; k + 1 < T::WN; ++k) iwin[k] = iwin[k + 1];
                iwin[T::WN - 1] = fd;
            }
        }
        // next step's input layer, still inside wave 0 (no barrier between sampling and h0)
        if (i + 1 < a.n_steps) input_gen(q0 + SEG);
        STAMP(9)
    };
    if constexpr (EXT) {
        // chunks of 64 steps: wave 1 fills the noise of chunk c+2 at the top of chunk c (buffer (c+2)&3 held chunk c-2,
        // whose readers are two chunks behind)
#pragma unroll 1
        for (int i0 = 0; i0 < a.n_steps; i0 += T::NZC) {
            noise_chunk((i0 >> 6) + 2);
            const int iend = i0 + T::NZC < a.n_steps ? i0 + T::NZC : a.n_steps;
#pragma unroll 1
            for (int i = i0; i < iend; ++i) gen_step(i);
        }
    } else {
#pragma unroll 1
        for (int i = 0; i < a.n_steps; ++i) gen_step(i);
    }
    if constexpr (STREAM) {    // the state the next chunk resumes from: rings (all written behind barriers) and wave 0's window
        __syncthreads();
        float* so = a.sess + (size_t)b * T::sess_floats;
        for (int e = tid; e < T::ring_off(L); e += NT) so[e] = lds[T::o_ring + e];
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < WNF; ++k) if (KIND == SWN_KIND_LAPLACE) so[T::ring_off(L) + k] = win[k];
#pragma unroll
            for (int k = 0; k < WNI; ++k) if (KIND == SWN_KIND_SOFTMAX) so[T::ring_off(L) + k] = __builtin_bit_cast(float, iwin[k]);
        }
    }
#ifdef SWN_STAMP
    if (tid == 0 && b == 0 && a.heads)
        for (int k = 0; k < 10; ++k) a.heads[k] = (float)((double)tacc[k] / (double)a.n_steps);
#endif
}

// the instantiation a geometry runs: f(Tr<...>{}) for a BL6-class net, SWN_E_UNSUPPORTED otherwise
template <class F>
int with_tr(const SwnGeom& g, F&& f) {
    if (!g.bl6 || g.U > 256 || g.U < 2 * g.seg || g.audio_in) return SWN_E_UNSUPPORTED;
    if (g.kind == SWN_KIND_LAPLACE && g.S == 128) {
        if (g.seg == 1 && g.lpc == 0) return f(Tr<128, 1, 0, SWN_KIND_LAPLACE, 0>{});
        if (g.seg == 1 && g.lpc == 4) return f(Tr<128, 1, 4, SWN_KIND_LAPLACE, 0>{});
        if (g.seg == 2 && g.lpc == 4) return f(Tr<128, 2, 4, SWN_KIND_LAPLACE, 0>{});
        if (g.seg == 5 && g.lpc == 0) return f(Tr<128, 5, 0, SWN_KIND_LAPLACE, 0>{});
        if (g.seg == 5 && g.lpc == 4) return f(Tr<128, 5, 4, SWN_KIND_LAPLACE, 0>{});
    }
    if (g.kind == SWN_KIND_SOFTMAX && g.S == 256 && g.Q == 256) return f(Tr<256, 1, 0, SWN_KIND_SOFTMAX, 256>{});
    return SWN_E_UNSUPPORTED;
}

// the bf16 image of one section: fp32 lane-tiled slices [ns][rows][16] -> [ns / 2][rows][16] words, slice 2g rounded into
// the low half and slice 2g + 1 into the high half (round to nearest even; a NaN stays a quiet NaN, as torch rounds)
__device__ __forceinline__ unsigned bf16_rne(float f) {
    const unsigned u = __builtin_bit_cast(unsigned, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
struct W16PackArgs {
    const float* src[3];       // wsk2, w12, w22 of the packed buffer
    unsigned* dst[3];
    unsigned words[3];         // words of each image section (0: none)
    unsigned slice[3];         // words of one image slice = floats of one fp32 slice: rows * 16
};
__global__ __launch_bounds__(256) void pack_w16_kernel(const W16PackArgs a) {
    const unsigned sec = blockIdx.y;
    for (unsigned w = blockIdx.x * 256 + threadIdx.x; w < a.words[sec]; w += gridDim.x * 256) {
        const unsigned g = w / a.slice[sec], rem = w % a.slice[sec];
        const float lo = a.src[sec][(size_t)(2 * g) * a.slice[sec] + rem];
        const float hi = a.src[sec][(size_t)(2 * g + 1) * a.slice[sec] + rem];
        a.dst[sec][w] = bf16_rne(lo) | (bf16_rne(hi) << 16);
    }
}

// The FP8 image (Bl6W8Layout) from the same three lane-tiled copies: one thread per output row of a matrix finds the row's
// largest magnitude, derives e_r from its exponent and fraction (frexp without a logarithm: amax = m 2^x, m in [0.5, 1);
// e_r = 9 - x if m <= 0.875, else 8 - x, clamped to [-100, 100]; 0 for a zero row), writes 2^-e_r and the row's codes.
// A section holds `mats` matrices of `ns` slices of 16 inputs and `rows` rows (out_skip: L matrices of 4 slices).
__device__ __forceinline__ unsigned e4m3_rne(float v) {      // nearest E4M3FN code, ties to even; the sign of a zero is kept
    const unsigned sign = (__builtin_bit_cast(unsigned, v) >> 24) & 0x80u;
    const float a = fabsf(v);
    if (!(a <= 448.f)) return sign | 0x7eu;                 // only behind the lower clamp of e_r: saturate, never a NaN code
    if (a < 0.015625f) return sign | (unsigned)rintf(a * 512.f);          // subnormal steps of 2^-9; 8 = the code of 2^-6
    const unsigned u = __builtin_bit_cast(unsigned, a);
    return sign | (((u + 0x7ffffu + ((u >> 20) & 1u)) >> 20) - (120u << 3));
}
struct W8PackArgs {
    const float* src[3];       // wsk2, w12, w22 of the packed buffer
    unsigned* dst[3];          // code sections
    float* sc[3];              // scale sections
    int mats[3], ns[3], rows[3];   // mats = 0: no such section
    int* bad;                  // set when a weight is not finite
};
__global__ __launch_bounds__(256) void pack_w8_kernel(const W8PackArgs a) {
    const int sec = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    const int rows = a.rows[sec], ns = a.ns[sec];
    if (idx >= a.mats[sec] * rows) return;
    const int m = idx / rows, r = idx % rows;
    const float* src = a.src[sec] + ((size_t)m * ns * rows + r) * 16;
    unsigned amax = 0;                                      // bits of the largest magnitude (ordered as the values are)
    for (int sl = 0; sl < ns; ++sl)
        for (int k = 0; k < 16; ++k) {
            const unsigned u = __builtin_bit_cast(unsigned, src[(size_t)sl * rows * 16 + k]) & 0x7fffffffu;
            amax = u > amax ? u : amax;
        }
    if (amax >= 0x7f800000u) { *a.bad = 1; return; }
    int e = 0;
    if (amax != 0) {
        const int x = (int)(amax >> 23) - 126;              // (a subnormal's true x is smaller still: clamped either way)
        e = ((amax & 0x7fffffu) <= 0x600000u ? 9 : 8) - x;
        e = e < -100 ? -100 : e > 100 ? 100 : e;
    }
    const float up = __builtin_bit_cast(float, (unsigned)(127 + e) << 23);
    a.sc[sec][idx] = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
    unsigned* dst = a.dst[sec] + ((size_t)m * (ns / 4) * rows + r) * 16;
    for (int g = 0; g < ns / 4; ++g)
        for (int k = 0; k < 16; ++k) {
            unsigned w = 0;
            for (int s = 0; s < 4; ++s) w |= e4m3_rne(src[(size_t)(4 * g + s) * rows * 16 + k] * up) << (8 * s);
            dst[(size_t)g * rows * 16 + k] = w;
        }
}
// what w8_pair makes of every code: code c sits in byte c & 3 of a word whose other bytes hold other codes
__global__ __launch_bounds__(256) void e4m3_table_kernel(float* out, float scale) {
    const unsigned c = threadIdx.x, pos = c & 3u;
    const unsigned w = (((~c) & 0xffu) * 0x01010101u & ~(0xffu << (8 * pos))) | (c << (8 * pos));
    float f[4];
    w8_word(w, scale, f);
    out[c] = pos == 0 ? f[0] : pos == 1 ? f[1] : pos == 2 ? f[2] : f[3];
}

// the one-shot decode and the streamed chunk, one workgroup per utterance; `sess` holds sess_floats per utterance.  The
// classic instantiation takes what it was written for (host-drawn noise, no dump, zero seed, fp32 weights); everything else
// is the extended one's.
template <int WK>
int launch_utts(const SwnDecodeCall& c, const char* where) {
    typename B6ArgsOf<false, false, WK>::type a;
    fill_args(a, c);
    if constexpr (WK != WK_F32) a.img = c.image;
    return with_tr(c.g, [&](auto t) {
        using T = decltype(t);
        using X = typename T::Ext;
        static_assert(T::lds_bytes <= 160 * 1024 && X::lds_bytes <= 160 * 1024 && w8_lds_bytes<X>() <= 160 * 1024, "LDS budget");
        constexpr size_t xlds = WK == WK_E4M3 ? w8_lds_bytes<X>() : X::lds_bytes;   // W8: the row scales behind the carve
        if (c.stream) return launch_kernel(decode_bl6_kernel<X, true, false, false, WK>, xlds, a.B, a, c.hip_stream, where);
        if constexpr (WK == WK_F32)
            if (!wants_ext(a)) return launch_kernel(decode_bl6_kernel<T>, T::lds_bytes, a.B, a, c.hip_stream, where);
        return launch_kernel(decode_bl6_kernel<X, false, false, false, WK>, xlds, a.B, a, c.hip_stream, where);
    });
}

// one pool launch over the checked entry table: one workgroup per entry, sessions [capacity][sess_floats]
template <bool MODELS, int WK>
int launch_pool(const SwnDecodeCall& c, const char* where) {
    typename B6ArgsOf<true, MODELS, WK>::type p;
    fill_args(p.c, c);
    p.t = *c.pool;
    if constexpr (MODELS) p.m = *c.models;
    if constexpr (WK != WK_F32 && MODELS) {
        for (int m = 0; m < SWN_POOL_MAX_MODELS; ++m) p.img[m] = c.images[m];   // (filled to the end, as the model table is)
    } else if constexpr (WK != WK_F32) p.img = c.image;
    return with_tr(c.g, [&](auto tr) {
        using T = typename decltype(tr)::Ext;
        constexpr size_t lds = WK == WK_E4M3 ? w8_lds_bytes<T>() : T::lds_bytes;
        return launch_kernel(decode_bl6_kernel<T, true, true, MODELS, WK>, lds, c.batch, p, c.hip_stream, where);
    });
}

// ... and one wide pool launch over the call's device table (swn_decode_pool_chunk_wide)
template <int WK>
int launch_pool_wide(const SwnDecodeCall& c) {
    Bl6PoolWideArgs p;
    fill_args(p.c, c);
    p.rows = c.wide;
    return with_tr(c.g, [&](auto tr) {
        using T = typename decltype(tr)::Ext;
        constexpr size_t lds = WK == WK_E4M3 ? w8_lds_bytes<T>() : T::lds_bytes;
        return launch_kernel(decode_bl6_kernel<T, true, true, false, WK, true>, lds, c.batch, p, c.hip_stream,
                             "swn_decode_pool_chunk_wide(bl6)");
    });
}

// bytes of the image of format `wk` for net `d`; 0: the symmetric kernel does not serve the net
size_t image_bytes(const swn_net_desc* d, int wk) {
    SwnGeom g;
    if (swn_make_geom(d, &g) < 0) return 0;
    size_t n = 0;
    with_tr(g, [&](auto t) {
        using T = decltype(t);
        constexpr bool soft = T::KIND == SWN_KIND_SOFTMAX;
        n = wk == WK_BF16 ? w16_layout(T::S, T::O1, T::NO, soft).total : w8_layout(T::S, T::O1, T::NO, soft).total;
        return SWN_OK;
    });
    return n;
}

// what swn_pack_decode_w16 / _w8 check before they launch; on SWN_OK `g` and `y` are the net's geometry and packed layout
int pack_image_check(const swn_net_desc* d, const float* packed, void* image, int wk, const char* where, const char* refusal,
                     SwnGeom& g, SwnLayout& y) {
    const int rc = swn_make_geom(d, &g);
    if (rc < 0) return rc;
    if (!packed || !image) return SWN_E_BADARG;
    if (image_bytes(d, wk) == 0) {
        swn_set_error_detail(where, refusal);
        return SWN_E_UNSUPPORTED;
    }
    swn_make_layout(&g, &y);
    return SWN_OK;
}

}  // namespace

// ---- bf16 storage of the streamed head matrices (swn_decode_w16 / swn_decode_chunk_w16 / swn_decode_pool_chunk_w16)
extern "C" size_t swn_decode_w16_bytes(const swn_net_desc* d) { return image_bytes(d, WK_BF16); }

extern "C" int swn_pack_decode_w16(const swn_net_desc* d, const float* packed, void* w16, void* stream_) {
    SwnGeom g;
    SwnLayout y;
    const int rc = pack_image_check(d, packed, w16, WK_BF16, "swn_pack_decode_w16",
                                    "bf16 weights exist for the nets the symmetric BL6 kernel serves only", g, y);
    if (rc < 0) return rc;
    const bool soft = g.kind == SWN_KIND_SOFTMAX;
    const Bl6W16Layout y16 = w16_layout(g.S, g.O1, g.NO, soft);
    char* img = static_cast<char*>(w16);
    W16PackArgs a;
    a.src[0] = packed + y.wsk2; a.dst[0] = reinterpret_cast<unsigned*>(img + y16.wsk);
    a.src[1] = packed + y.w12;  a.dst[1] = reinterpret_cast<unsigned*>(img + y16.w1);
    a.src[2] = packed + y.w22;  a.dst[2] = reinterpret_cast<unsigned*>(img + y16.w2);
    a.words[0] = (unsigned)(L * g.S * 32); a.slice[0] = (unsigned)(g.S * 16);
    a.words[1] = (unsigned)(g.O1 * g.S / 2); a.slice[1] = (unsigned)(g.O1 * 16);
    a.words[2] = soft ? (unsigned)(g.NO * g.O1 / 2) : 0u; a.slice[2] = (unsigned)(g.NO * 16);
    (void)hipGetLastError();
    hipLaunchKernelGGL(pack_w16_kernel, dim3(32, 3), dim3(256), 0, (hipStream_t)stream_, a);
    return swn_launch_status("swn_pack_decode_w16");
}

// ---- FP8 (E4M3) storage of the streamed head matrices (swn_decode_w8 / swn_decode_chunk_w8 / swn_decode_pool_chunk_w8)
extern "C" size_t swn_decode_w8_bytes(const swn_net_desc* d) { return image_bytes(d, WK_E4M3); }

// (the one call of the family that waits for its stream: a weight that is not finite is reported as SWN_E_BADARG)
extern "C" int swn_pack_decode_w8(const swn_net_desc* d, const float* packed, void* w8, void* stream_) {
    SwnGeom g;
    SwnLayout y;
    int rc = pack_image_check(d, packed, w8, WK_E4M3, "swn_pack_decode_w8",
                              "e4m3 weights exist for the nets the symmetric BL6 kernel serves only", g, y);
    if (rc < 0) return rc;
    const bool soft = g.kind == SWN_KIND_SOFTMAX;
    const Bl6W8Layout y8 = w8_layout(g.S, g.O1, g.NO, soft);
    char* img = static_cast<char*>(w8);
    hipStream_t st = (hipStream_t)stream_;
    W8PackArgs a;
    a.src[0] = packed + y.wsk2; a.dst[0] = reinterpret_cast<unsigned*>(img + y8.wsk); a.sc[0] = reinterpret_cast<float*>(img + y8.ssk);
    a.src[1] = packed + y.w12;  a.dst[1] = reinterpret_cast<unsigned*>(img + y8.w1);  a.sc[1] = reinterpret_cast<float*>(img + y8.s1);
    a.src[2] = packed + y.w22;  a.dst[2] = reinterpret_cast<unsigned*>(img + y8.w2);  a.sc[2] = reinterpret_cast<float*>(img + y8.s2);
    a.mats[0] = L; a.ns[0] = 4; a.rows[0] = g.S;
    a.mats[1] = 1; a.ns[1] = g.S / 16; a.rows[1] = g.O1;
    a.mats[2] = soft ? 1 : 0; a.ns[2] = g.O1 / 16; a.rows[2] = g.NO;
    (void)hipGetLastError();
    if (hipMalloc(reinterpret_cast<void**>(&a.bad), sizeof(int)) != hipSuccess) return SWN_E_LAUNCH;
    int bad = 0;
    bool ok = hipMemsetAsync(a.bad, 0, sizeof(int), st) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(pack_w8_kernel, dim3((L * g.S + 255) / 256, 3), dim3(256), 0, st, a);
        rc = swn_launch_status("swn_pack_decode_w8");
        ok = hipMemcpyAsync(&bad, a.bad, sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    (void)hipFree(a.bad);
    if (!ok) return SWN_E_LAUNCH;
    if (rc < 0) return rc;
    if (bad) {
        swn_set_error_detail("swn_pack_decode_w8", "a weight of out_skip / out_1 / out_2 is not finite");
        return SWN_E_BADARG;
    }
    return SWN_OK;
}

extern "C" int swn_e4m3_table(float* out, float scale, void* stream_) {
    if (!out) return SWN_E_BADARG;
    (void)hipGetLastError();
    hipLaunchKernelGGL(e4m3_table_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream_, out, scale);
    return swn_launch_status("swn_e4m3_table");
}

// a checked call on the symmetric kernel (swn_decode.hip)
int swn_decode_bl6_run(const SwnDecodeCall& c) {
    if (c.wide) switch (c.wk) {
        case WK_E4M3: return launch_pool_wide<WK_E4M3>(c);
        case WK_BF16: return launch_pool_wide<WK_BF16>(c);
        default: return launch_pool_wide<WK_F32>(c);
    }
    if (c.pool) switch (c.wk) {
        case WK_E4M3: return c.models ? launch_pool<true, WK_E4M3>(c, "swn_decode_pool_chunk_models_w8(bl6)")
                                      : launch_pool<false, WK_E4M3>(c, "swn_decode_pool_chunk_w8(bl6)");
        case WK_BF16: return c.models ? launch_pool<true, WK_BF16>(c, "swn_decode_pool_chunk_models_w16(bl6)")
                                      : launch_pool<false, WK_BF16>(c, "swn_decode_pool_chunk_w16(bl6)");
        default: return c.models ? launch_pool<true, WK_F32>(c, "swn_decode_pool_chunk_models(bl6)")
                                 : launch_pool<false, WK_F32>(c, "swn_decode_pool_chunk(bl6)");
    }
    switch (c.wk) {
        case WK_E4M3: return launch_utts<WK_E4M3>(c, "swn_decode_w8(bl6)");
        case WK_BF16: return launch_utts<WK_BF16>(c, "swn_decode_w16(bl6)");
        default: return launch_utts<WK_F32>(c, "swn_decode(bl6)");
    }
}

// streamed decode (swn_decode_chunk): per-utterance session floats of the symmetric kernel, 0 = not a BL6-class net
size_t swn_decode_bl6_session_floats(const SwnGeom& g) {
    int n = 0;
    with_tr(g, [&](auto t) { n = decltype(t)::sess_floats; return SWN_OK; });
    return (size_t)n;
}
