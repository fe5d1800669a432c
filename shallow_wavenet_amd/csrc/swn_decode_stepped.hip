// Stepped autoregressive decode for LARGE geometries (reference-shipped REF6: H=192/256, K=7, 15-24 MB
// of weights touched per generated sample) on gfx950.
//
// One CU cannot hold or stream that much per step, and in-kernel cross-CU hand-offs cost 1-3 us each
// (MI355X_MICROARCH.md price list) - about what a dependent kernel boundary costs (1.45 us).  So every
// phase of a step is its OWN launch, spread over many CUs that each read a slice of the weight rows from
// L2 / Infinity Cache:
//     step_layer   x L : rows of one dilated conv + fused gate        one wave per channel pair
//     rowvec       skip (all out_skip 1x1s as one mat-vec), out_1    one wave per row
//     step_tail    out_2 + sampling + history update + the NEXT step's input layer   1 workgroup / utterance
// L+3 launches per generated step, no spinning, no inter-workgroup protocol: the stream order is the
// dependency chain (cswnv_shift1.py:348-402).  The iteration index is a launch argument (no dependent
// load at kernel entry); measured: the chain is bound by the L2 round trips inside each launch, not by
// host launch cost (hipGraph replay of the same chain ran at the same speed, so it is not used).
// State (history rings, hcat, skip, out_1, sample window) lives in the caller's scratch buffer; the math
// and the ring layout are those of the generic persistent kernel (swn_decode.hip).
// A new session's prologue (n_pro positions through the chain) can also be filled in L + 2 launches, bit for bit:
// swn_decode_stepped_prologue.hip; what both files share is in swn_decode_stepped_common.hpp.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "swn_decode_internal.hpp"
#include "swn_decode_stepped_common.hpp"

namespace {

// ---- stepped decode pool (swn_decode_pool_stepped_chunk): the launch chain serves the entries of a tick, each at its own
//      iteration.  Utterance index b of a launch is the entry's place in the tick's table (sorted by n_it, descending, so
//      that the entries still active at tick-local iteration j are a prefix); the launch argument is j, the entry works at
//      its absolute iteration it0 + j while j < n_it.  The table is written to the device once per tick (by
//      step_pool_setup_kernel, from its kernel arguments) and read by every later launch of the tick.
struct StPoolEnt {
    const float* cond;                         // the entry's cond rows (Tf, N)
    int Tf, slot, it0, n_it;
    int row;                                   // the entry's row of out / heads / noise / seed / utterance ids
    int g0;                                    // absolute iteration of its first generation step here: max(it0, n_pro)
};
static_assert(sizeof(StPoolEnt) == 32 && SWN_DECODE_POOL_MAX_ENTRIES * sizeof(StPoolEnt) <= SWN_DECODE_STEPPED_POOL_TABLE_FLOATS * 4,
              "the device copy of a pool table fits SWN_DECODE_STEPPED_POOL_TABLE_FLOATS (include/swn_hip.h)");
struct StPoolTable {
    StPoolEnt e[SWN_DECODE_POOL_MAX_ENTRIES];
};
static_assert(sizeof(StArgs) + sizeof(StPoolTable) + 16 <= 4096, "step_pool_setup_kernel's arguments fit 4 KB");
struct StPoolArgs : StArgs {
    const StPoolEnt* tab;                      // the device copy of the tick's table
};
// ---- stepped decode pool over several models of one geometry (swn_decode_pool_stepped_chunk_models).  A table row also
//      carries the resolved weight pointer of its entry's model: the per-entry kernels read their weights through their row's
//      pointer, a tile kernel through that of its tile's first row.  The table is sorted by (model, n_it descending), so the
//      entries of one model still active at tick-local iteration j are a prefix of that model's group; a tile is a run of at
//      most 8 active rows of one group.  The tile list (swn_decode_stepped_pool_plan) travels in the kernel arguments and is
//      rebuilt by the host when an entry runs out.  The per-entry kernels cover the rows up to the last active one (a row past
//      its n_it returns at once).
struct StPoolEntM : StPoolEnt {
    const float* P;                            // the packed parameters of the entry's model
};
static_assert(sizeof(StPoolEntM) == 40 && SWN_DECODE_POOL_MAX_ENTRIES * sizeof(StPoolEntM) <= SWN_DECODE_STEPPED_POOL_MODELS_TABLE_FLOATS * 4,
              "the device copy of a models table fits SWN_DECODE_STEPPED_POOL_MODELS_TABLE_FLOATS (include/swn_hip.h)");
struct StPoolTableM {
    StPoolEntM e[SWN_DECODE_POOL_MAX_ENTRIES];
};
static_assert(sizeof(StArgs) + sizeof(StPoolTableM) + 16 <= 4096, "step_pool_setup_kernel's arguments fit 4 KB");
struct StModelsArgs : StArgs {
    const StPoolEntM* tab;                     // the device copy of the tick's table
    int n_tiles, n_act;                        // host side: tiles / active entries of the iteration
    int tile[SWN_DECODE_STEPPED_POOL_MAX_TILES + 1];   // tile t: first table row | rows << 8
};
template <bool POOL, bool MODELS = false>
using StA = typename std::conditional<MODELS, StModelsArgs, typename std::conditional<POOL, StPoolArgs, StArgs>::type>::type;

// rows [b0, b0 + nb) of the table that tile blockIdx.y of a launch serves
template <bool MODELS, class A>
__device__ __forceinline__ int st_tile_b0(const A& a) {
    if constexpr (MODELS) return a.tile[blockIdx.y] & 255;
    else return blockIdx.y * 8;
}
template <bool MODELS, class A>
__device__ __forceinline__ int st_tile_nb(const A& a, const int b0) {
    if constexpr (MODELS) return a.tile[blockIdx.y] >> 8;
    else return a.B - b0 < 8 ? a.B - b0 : 8;
}

// iteration `it` of the per-utterance counter: it < n_pro is a prologue position, else generation step
struct Iter { bool gen; int i, np, q0; };
__device__ __forceinline__ Iter iter_of(const StArgs& a, int it) {
    Iter r; r.gen = it >= a.n_pro; r.i = it - a.n_pro; r.np = r.gen ? a.g.seg : 1;
    r.q0 = r.gen ? a.g.rf + 1 - a.g.seg + r.i * a.g.seg : it;
    return r;
}

// ---- input layer of iteration `it` -> ring 0 (device function: own launch in the prologue, fused into
//      the tail of the previous step during generation)
template <int KIND>
__device__ __forceinline__ void input_layer(const StArgs& a, const float* P, float* st, const int it, const int tid,
                                            const int nthreads, const float* win) {
    // win[0..WN): the sample window (LDS copy; float samples or int class indices).  All parameter loads are
    // unconditional and selected afterwards, so the K taps cost one memory round trip, not K.
    const SwnGeom& g = a.g;
    const Iter r = iter_of(a, it);
    const int H = g.H, K = g.K, seg = g.seg, WN = a.WN;
    for (int e = tid; e < H * r.np; e += nthreads) {
        const int j = e / H, o = e - j * H, q = r.q0 + j;
        float acc = P[a.y.cb + o];
        for (int k = 0; k < K; ++k) {
            const int rr = q - (K - 1 - k);
            if (KIND == SWN_KIND_LAPLACE) {
                const int qe = r.gen ? g.rf + r.i * seg : g.rf;
                int wi = rr - qe + WN - 1; wi = wi < 0 ? 0 : (wi >= WN ? WN - 1 : wi);
                const float sv = r.gen ? win[wi] : 0.f;
                const float t = fmaf(P[a.y.cv + (size_t)k * H + o], sv, P[a.y.cc + (size_t)k * H + o]);
                acc += (rr >= -(seg - 1)) ? t : 0.f;
            } else {
                const int qe = r.gen ? g.rf + r.i : g.rf;
                int wi = rr - qe + WN - 1; wi = wi < 0 ? 0 : (wi >= WN ? WN - 1 : wi);
                const int idx = r.gen ? __builtin_bit_cast(int, win[wi]) : g.Q / 2;
                const float t = P[a.y.ct + ((size_t)k * g.Q + idx) * H + o];
                acc += (rr >= 0) ? t : 0.f;
            }
        }
        st[a.ring_off[0] + pmod(q, a.ring_len[0]) * g.Hp + o] = acc / (1.f + fabsf(acc));
    }
}

// POOL: entry blockIdx.x, when it is in its prologue or at the first generation iteration of its range (later steps get their
// input layer from the tail of the step before).  MODELS (with POOL): the entry's weights are those of its row's model.
template <int KIND, bool POOL = false, bool MODELS = false>
__global__ __launch_bounds__(256) void step_in_kernel(const StA<POOL, MODELS> a, const int itj) {
    static_assert(!MODELS || POOL, "several models: a pool form");
    __shared__ float lwin[32];
    int it = itj;
    float* st;
    const float* P = a.P;
    if constexpr (POOL) {
        const auto& en = a.tab[blockIdx.x];
        it = en.it0 + itj;
        if (itj >= en.n_it || !(it < a.n_pro || it == en.g0)) return;
        st = a.state + (size_t)en.slot * a.stride;
        if constexpr (MODELS) P = en.P;
    } else {
        st = a.state + (size_t)blockIdx.x * a.stride;
    }
    if ((int)threadIdx.x < a.WN) lwin[threadIdx.x] = st[a.o_hist + threadIdx.x];
    __syncthreads();
    input_layer<KIND>(a, P, st, it, threadIdx.x, 256, lwin);
}

// ---- step_layer: ONE wave per channel pair (gate row + candidate row), weights kept in registers.
//      Kernel boundaries invalidate the per-XCD L2s, so every launch re-fetches its weight rows from the
//      Infinity Cache at ~30 GB/s per CU: H workgroups of 64 lanes keep each CU's share at ~10 KB.
// POOL (BT = 1): entry blockIdx.y at its own iteration, its state block in its slot, its own conditioning
// MODELS (with POOL): the weight rows are those of the entry's model
template <int NI, int KIND, int BT, bool POOL = false, bool MODELS = false>   // NI = ceil(K*Hp / 256): float4 pieces per lane and row; BT = utterances per tile
__global__ __launch_bounds__(64) void step_layer_kernel(const StA<POOL, MODELS> a, const int l, const int itj) {
    static_assert(!POOL || BT == 1, "pool form: one entry per workgroup");
    static_assert(!MODELS || POOL, "several models: a pool form");
    const SwnGeom& g = a.g;
    const int lane = threadIdx.x;
    const int o = blockIdx.x;
    const int H = g.H, Hp = g.Hp, K = g.K, H2 = 2 * g.H, seg = g.seg, KH = K * Hp;
    int it = itj;
    size_t pbase = 0;                                          // POOL: the entry's state block, in floats
    const float* pcond = nullptr;
    int pTf = 0;
    const float* pP = nullptr;                                 // MODELS: the packed parameters of the entry's model
    if constexpr (POOL) {
        const auto& en = a.tab[blockIdx.y];
        if (itj >= en.n_it) return;
        it = en.it0 + itj; pbase = (size_t)en.slot * a.stride; pcond = en.cond; pTf = en.Tf;
        if constexpr (MODELS) pP = en.P;
    }
    const bool live = o < H;
    const float* P = a.P;
    if constexpr (MODELS) P = pP;
    const __amdgpu_buffer_rsrc_t rP = st_rsrc(P), rS = st_rsrc(a.state);
    float4 wz[NI], wc[NI];
    {
        const size_t rz = a.y.wd + ((size_t)l * H2 + (live ? o : 0)) * KH, rc = rz + (size_t)H * KH;
#pragma unroll
        for (int pc = 0; pc < NI; ++pc) {
            const int idx = pc * 256 + lane * 4;
            const bool ok = live && idx < KH;
            wz[pc] = st_ld4(rP, ok ? (unsigned)((rz + idx) * 4) : ST_OOB);
            wc[pc] = st_ld4(rP, ok ? (unsigned)((rc + idx) * 4) : ST_OOB);
        }
    }
    const int dil = g.dil[l], R = a.ring_len[l];
    const Iter r = iter_of(a, it);
    const int b0 = blockIdx.y * BT;
    const int nb = a.B - b0 < BT ? a.B - b0 : BT;              // utterances of this tile, processed CONCURRENTLY:
    for (int j = 0; j < r.np; ++j) {                          // lane u finishes utterance b0+u
        const int q = r.q0 + j;
        float az[BT], ac[BT];
#pragma unroll
        for (int u = 0; u < BT; ++u) { az[u] = 0.f; ac[u] = 0.f; }
        float4 xv[NI][BT];                                     // all activation loads of the position in flight at once
#pragma unroll
        for (int pc = 0; pc < NI; ++pc) {
            const int idx = pc * 256 + lane * 4;
            const int ic = idx < KH ? idx : 0;
            const int tap = ic / Hp, i = ic - tap * Hp;
            const size_t xo = a.ring_off[l] + (size_t)pmod(q - (K - 1 - tap) * dil, R) * Hp + i;
#pragma unroll
            for (int u = 0; u < BT; ++u) {
                if constexpr (POOL) xv[pc][u] = st_ld4(rS, idx < KH ? st_off(pbase + xo) : ST_OOB);
                else xv[pc][u] = st_ld4(rS, (idx < KH && u < nb) ? (unsigned)(((size_t)(b0 + u) * a.stride + xo) * 4) : ST_OOB);
            }
        }
        // epilogue operands: issued behind the activation loads (this block is an exec-masked branch that waits for
        // its own loads; placed first it would hold the activation loads back by a round trip)
        float gz = 0.f, gc = 0.f, bdz = 0.f, bdc = 0.f, hp = 0.f;
        if (lane < nb && live) {
            const int b = b0 + lane;
            const float* st = POOL ? a.state + pbase : a.state + (size_t)b * a.stride;
            gz = P[a.y.bx + (size_t)l * H2 + o]; gc = P[a.y.bx + (size_t)l * H2 + H + o];
            bdz = P[a.y.bd + (size_t)l * H2 + o]; bdc = P[a.y.bd + (size_t)l * H2 + H + o];
            hp = st[a.ring_off[l] + (size_t)pmod(q, R) * Hp + o];
            const int Tf = POOL ? pTf : a.Tf;
            const float* condb = POOL ? pcond : a.cond + (size_t)b * a.Tf * g.N;
            for (int s = 0; s < seg; ++s) {
                int tt = q + s - g.rf; tt = tt < 0 ? 0 : tt;
                int f = tt / g.U; const int jj = tt - f * g.U;
                f = f < Tf ? f : Tf - 1;
                const float w = P[a.y.wup + jj];
                const float* cr = condb + (size_t)f * g.N + (size_t)(l * seg + s) * H2;
                gz = fmaf(w, cr[o], gz); gc = fmaf(w, cr[H + o], gc);
            }
            if (KIND == SWN_KIND_SOFTMAX && g.audio_in) {
                const int* ihist = reinterpret_cast<const int*>(st + a.o_hist);
                const int qe = r.gen ? g.rf + r.i : g.rf;
                const int idx = r.gen ? ihist[q - qe + a.WN - 1] : g.Q / 2;
                const float* wa = P + a.y.wxa + ((size_t)l * g.Q + idx) * H2;
                gz += wa[o]; gc += wa[H + o];
            }
        }
#pragma unroll
        for (int pc = 0; pc < NI; ++pc)
#pragma unroll
            for (int u = 0; u < BT; ++u) {
                const float4 x = xv[pc][u];
                az[u] = fmaf(wz[pc].x, x.x, az[u]); az[u] = fmaf(wz[pc].y, x.y, az[u]);
                az[u] = fmaf(wz[pc].z, x.z, az[u]); az[u] = fmaf(wz[pc].w, x.w, az[u]);
                ac[u] = fmaf(wc[pc].x, x.x, ac[u]); ac[u] = fmaf(wc[pc].y, x.y, ac[u]);
                ac[u] = fmaf(wc[pc].z, x.z, ac[u]); ac[u] = fmaf(wc[pc].w, x.w, ac[u]);
            }
        float myz = 0.f, myc = 0.f;
#pragma unroll
        for (int u = 0; u < BT; ++u) {
            if (u < nb) {
                const float sz = sum64(az[u]), sc = sum64(ac[u]);
                if (lane == u) { myz = sz; myc = sc; }
            }
        }
        if (lane < nb && live) {
            float* st = POOL ? a.state + pbase : a.state + (size_t)(b0 + lane) * a.stride;
            const float z = sigm(gz * (myz + bdz));
            const float c = tanhf(gc * (myc + bdc));
            const float hn = (1.f - z) * c + z * hp;
            if (l + 1 < g.L) st[a.ring_off[l + 1] + pmod(q, a.ring_len[l + 1]) * Hp + o] = hn;
            if (j == r.np - 1) st[a.o_hcat + l * Hp + o] = hn;
        }
    }
}

// ---- step_layer for MANY utterances: a 512-thread workgroup = 8 channel pairs x 8 utterances.  Per-utterance workgroups
//      re-read a pair's weight rows once per utterance and every pair's wave re-reads the utterance's K H activations:
//      98 MB through L2 per layer launch at 64 utterances, 9.5 us - the launch is bound by that traffic, not by latency.
//      Here wave w keeps the 2 K H weights of pair 8 bx + w in registers (fetched once per 8 utterances), wave u stages the
//      activations of utterance 8 by + u in LDS (fetched once per 8 pairs: 25 MB per launch), and after ONE barrier every
//      wave forms its pair's two sums for the eight utterances out of LDS - the same lane-by-lane sums as the kernels above
//      (bit-identical results).  Lane 8 u of a wave finishes utterance u.
// POOL: the eight entries of a tile may be at different iterations.  Wave w stages entry 8 by + w at its own position, lane
// octet u finishes entry 8 by + u at its own; the position loop (barriers inside) runs to the largest count of positions of
// the tile (1 in the prologue, seg in generation), and an entry past its own count, or past its n_it, stays idle.
// MODELS (with POOL): tile blockIdx.y is a run of rows of ONE model (a.tile), whose weight rows the waves fetch through the
// pointer of the tile's first row.
template <int NI, int KIND, bool POOL = false, bool MODELS = false>
__global__ __launch_bounds__(64 * ST_TU) void step_layer_tile_kernel(const StA<POOL, MODELS> a, const int l, const int itj) {
    static_assert(!MODELS || POOL, "several models: a pool form");
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [ST_TU][NI * 256]
    const SwnGeom& g = a.g;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int o = blockIdx.x * ST_TU + w;
    const int H = g.H, Hp = g.Hp, K = g.K, H2 = 2 * g.H, seg = g.seg, KH = K * Hp;
    if constexpr (POOL) {
        static_assert(ST_TU == 8, "st_tile_b0 / st_tile_nb: tiles of 8 rows");
        const int b0 = st_tile_b0<MODELS>(a);
        const int nb = st_tile_nb<MODELS>(a, b0);
        // the staging entry of this wave (uniform) and the finishing entry of this lane's octet
        const int kw = b0 + (w < nb ? w : 0), ku = b0 + ((lane >> 3) < nb ? (lane >> 3) : 0);
        const auto& ew = a.tab[kw];
        const auto& eu = a.tab[ku];
        const bool onw = w < nb && itj < ew.n_it, onu = (lane >> 3) < nb && itj < eu.n_it;
        const Iter rw = iter_of(a, ew.it0 + itj), ru = iter_of(a, eu.it0 + itj);
        // positions of the tile: the largest count over its active entries (every lane holds its octet's entry)
        int npm = onu ? ru.np : 0;
        npm = max(npm, __shfl_xor(npm, 8, 64)); npm = max(npm, __shfl_xor(npm, 16, 64)); npm = max(npm, __shfl_xor(npm, 32, 64));
        npm = __builtin_amdgcn_readfirstlane(npm);
        if (npm == 0) return;                                  // uniform over the workgroup: no entry of the tile is active
        const bool live = o < H;
        const float* P = a.P;
        if constexpr (MODELS) P = a.tab[b0].P;
        const __amdgpu_buffer_rsrc_t rP = st_rsrc(P), rS = st_rsrc(a.state);
        float4 wz[NI], wc[NI];
        {
            const size_t rz = a.y.wd + ((size_t)l * H2 + (live ? o : 0)) * KH, rc = rz + (size_t)H * KH;
#pragma unroll
            for (int pc = 0; pc < NI; ++pc) {
                const int idx = pc * 256 + lane * 4;
                const bool ok = live && idx < KH;
                wz[pc] = st_ld4(rP, ok ? (unsigned)((rz + idx) * 4) : ST_OOB);
                wc[pc] = st_ld4(rP, ok ? (unsigned)((rc + idx) * 4) : ST_OOB);
            }
        }
        const int dil = g.dil[l], R = a.ring_len[l];
        const size_t basew = (size_t)ew.slot * a.stride, baseu = (size_t)eu.slot * a.stride;
        for (int j = 0; j < npm; ++j) {
            const int qw = rw.q0 + j, qu = ru.q0 + j;
            {
                float4 xv[NI];
                const bool stage = onw && j < rw.np;
#pragma unroll
                for (int pc = 0; pc < NI; ++pc) {
                    const int idx = pc * 256 + lane * 4;
                    const int ic = idx < KH ? idx : 0;
                    const int tap = ic / Hp, i = ic - tap * Hp;
                    const size_t xo = a.ring_off[l] + (size_t)pmod(qw - (K - 1 - tap) * dil, R) * Hp + i;
                    xv[pc] = st_ld4(rS, (idx < KH && stage) ? st_off(basew + xo) : ST_OOB);
                }
                if (j > 0) __syncthreads();
#pragma unroll
                for (int pc = 0; pc < NI; ++pc) *reinterpret_cast<float4*>(xs + (w * NI + pc) * 256 + lane * 4) = xv[pc];
            }
            float gz = 0.f, gc = 0.f, bdz = 0.f, bdc = 0.f, hp = 0.f;
            const bool fin = (lane & 7) == 0 && onu && j < ru.np && live;
            if (fin) {
                const float* st = a.state + baseu;
                gz = P[a.y.bx + (size_t)l * H2 + o]; gc = P[a.y.bx + (size_t)l * H2 + H + o];
                bdz = P[a.y.bd + (size_t)l * H2 + o]; bdc = P[a.y.bd + (size_t)l * H2 + H + o];
                hp = st[a.ring_off[l] + (size_t)pmod(qu, R) * Hp + o];
                const float* condb = eu.cond;
                const int Tf = eu.Tf;
                for (int s = 0; s < seg; ++s) {
                    int tt = qu + s - g.rf; tt = tt < 0 ? 0 : tt;
                    int f = tt / g.U; const int jj = tt - f * g.U;
                    f = f < Tf ? f : Tf - 1;
                    const float wv = P[a.y.wup + jj];
                    const float* cr = condb + (size_t)f * g.N + (size_t)(l * seg + s) * H2;
                    gz = fmaf(wv, cr[o], gz); gc = fmaf(wv, cr[H + o], gc);
                }
                if (KIND == SWN_KIND_SOFTMAX && g.audio_in) {
                    const int* ihist = reinterpret_cast<const int*>(st + a.o_hist);
                    const int qe = ru.gen ? g.rf + ru.i : g.rf;
                    const int idx = ru.gen ? ihist[qu - qe + a.WN - 1] : g.Q / 2;
                    const float* wa = P + a.y.wxa + ((size_t)l * g.Q + idx) * H2;
                    gz += wa[o]; gc += wa[H + o];
                }
            }
            __syncthreads();
            float azv[ST_TU], acv[ST_TU];
#pragma unroll
            for (int u = 0; u < ST_TU; ++u) {
                float az = 0.f, ac = 0.f;
#pragma unroll
                for (int pc = 0; pc < NI; ++pc) {
                    const float4 x = *reinterpret_cast<const float4*>(xs + (u * NI + pc) * 256 + lane * 4);
                    az = fmaf(wz[pc].x, x.x, az); az = fmaf(wz[pc].y, x.y, az);
                    az = fmaf(wz[pc].z, x.z, az); az = fmaf(wz[pc].w, x.w, az);
                    ac = fmaf(wc[pc].x, x.x, ac); ac = fmaf(wc[pc].y, x.y, ac);
                    ac = fmaf(wc[pc].z, x.z, ac); ac = fmaf(wc[pc].w, x.w, ac);
                }
                azv[u] = az; acv[u] = ac;
            }
            const float myz = sum64x8(azv, lane), myc = sum64x8(acv, lane);
            if (fin) {
                float* st = a.state + baseu;
                const float z = sigm(gz * (myz + bdz));
                const float c = tanhf(gc * (myc + bdc));
                const float hn = (1.f - z) * c + z * hp;
                if (l + 1 < g.L) st[a.ring_off[l + 1] + pmod(qu, a.ring_len[l + 1]) * Hp + o] = hn;
                if (j == ru.np - 1) st[a.o_hcat + l * Hp + o] = hn;
            }
        }
        return;
    }
    const int it = itj;
    const bool live = o < H;
    const float* P = a.P;
    const __amdgpu_buffer_rsrc_t rP = st_rsrc(P), rS = st_rsrc(a.state);
    float4 wz[NI], wc[NI];
    {
        const size_t rz = a.y.wd + ((size_t)l * H2 + (live ? o : 0)) * KH, rc = rz + (size_t)H * KH;
#pragma unroll
        for (int pc = 0; pc < NI; ++pc) {
            const int idx = pc * 256 + lane * 4;
            const bool ok = live && idx < KH;
            wz[pc] = st_ld4(rP, ok ? (unsigned)((rz + idx) * 4) : ST_OOB);
            wc[pc] = st_ld4(rP, ok ? (unsigned)((rc + idx) * 4) : ST_OOB);
        }
    }
    const int dil = g.dil[l], R = a.ring_len[l];
    const Iter r = iter_of(a, it);
    const int b0 = blockIdx.y * ST_TU;
    const int nb = a.B - b0 < ST_TU ? a.B - b0 : ST_TU;
    for (int j = 0; j < r.np; ++j) {
        const int q = r.q0 + j;
        // wave w stages utterance b0 + w
        {
            float4 xv[NI];
#pragma unroll
            for (int pc = 0; pc < NI; ++pc) {
                const int idx = pc * 256 + lane * 4;
                const int ic = idx < KH ? idx : 0;
                const int tap = ic / Hp, i = ic - tap * Hp;
                const size_t xo = a.ring_off[l] + (size_t)pmod(q - (K - 1 - tap) * dil, R) * Hp + i;
                xv[pc] = st_ld4(rS, (idx < KH && w < nb) ? (unsigned)(((size_t)(b0 + w) * a.stride + xo) * 4) : ST_OOB);
            }
            if (j > 0) __syncthreads();                        // the previous position's sums are done with the buffer
#pragma unroll
            for (int pc = 0; pc < NI; ++pc) *reinterpret_cast<float4*>(xs + (w * NI + pc) * 256 + lane * 4) = xv[pc];
        }
        // epilogue operands: issued behind the activation loads (an exec-masked block that waits for its own loads)
        float gz = 0.f, gc = 0.f, bdz = 0.f, bdc = 0.f, hp = 0.f;
        const int ut = lane >> 3;                              // the utterance this lane's octet ends up with (sum64x8)
        const bool fin = (lane & 7) == 0 && ut < nb && live;
        if (fin) {
            const int b = b0 + ut;
            const float* st = a.state + (size_t)b * a.stride;
            gz = P[a.y.bx + (size_t)l * H2 + o]; gc = P[a.y.bx + (size_t)l * H2 + H + o];
            bdz = P[a.y.bd + (size_t)l * H2 + o]; bdc = P[a.y.bd + (size_t)l * H2 + H + o];
            hp = st[a.ring_off[l] + (size_t)pmod(q, R) * Hp + o];
            const float* condb = a.cond + (size_t)b * a.Tf * g.N;
            for (int s = 0; s < seg; ++s) {
                int tt = q + s - g.rf; tt = tt < 0 ? 0 : tt;
                int f = tt / g.U; const int jj = tt - f * g.U;
                f = f < a.Tf ? f : a.Tf - 1;
                const float wv = P[a.y.wup + jj];
                const float* cr = condb + (size_t)f * g.N + (size_t)(l * seg + s) * H2;
                gz = fmaf(wv, cr[o], gz); gc = fmaf(wv, cr[H + o], gc);
            }
            if (KIND == SWN_KIND_SOFTMAX && g.audio_in) {
                const int* ihist = reinterpret_cast<const int*>(st + a.o_hist);
                const int qe = r.gen ? g.rf + r.i : g.rf;
                const int idx = r.gen ? ihist[q - qe + a.WN - 1] : g.Q / 2;
                const float* wa = P + a.y.wxa + ((size_t)l * g.Q + idx) * H2;
                gz += wa[o]; gc += wa[H + o];
            }
        }
        __syncthreads();
        float azv[ST_TU], acv[ST_TU];
#pragma unroll
        for (int u = 0; u < ST_TU; ++u) {
            float az = 0.f, ac = 0.f;
#pragma unroll
            for (int pc = 0; pc < NI; ++pc) {
                const float4 x = *reinterpret_cast<const float4*>(xs + (u * NI + pc) * 256 + lane * 4);
                az = fmaf(wz[pc].x, x.x, az); az = fmaf(wz[pc].y, x.y, az);
                az = fmaf(wz[pc].z, x.z, az); az = fmaf(wz[pc].w, x.w, az);
                ac = fmaf(wc[pc].x, x.x, ac); ac = fmaf(wc[pc].y, x.y, ac);
                ac = fmaf(wc[pc].z, x.z, ac); ac = fmaf(wc[pc].w, x.w, ac);
            }
            azv[u] = az; acv[u] = ac;
        }
        const float myz = sum64x8(azv, lane), myc = sum64x8(acv, lane);
        if (fin) {
            float* st = a.state + (size_t)(b0 + ut) * a.stride;
            const float z = sigm(gz * (myz + bdz));
            const float c = tanhf(gc * (myc + bdc));
            const float hn = (1.f - z) * c + z * hp;
            if (l + 1 < g.L) st[a.ring_off[l + 1] + pmod(q, a.ring_len[l + 1]) * Hp + o] = hn;
            if (j == r.np - 1) st[a.o_hcat + l * Hp + o] = hn;
        }
    }
}

// ---- rowvec: y[b][row] = act(bias[row] + W[row][:] . x[b][:]), ONE wave per row -------------------------
// POOL (BT = 1): entry blockIdx.y, when it is generating at tick-local iteration `itj`; its state block is in its slot
// MODELS (with POOL): the rows are those of the entry's model
template <int BT, bool POOL = false, bool MODELS = false>
__global__ __launch_bounds__(64) void rowvec_kernel(const StA<POOL, MODELS> a, size_t w_off, int ldw, size_t b_off, int rows,
                                                    int ni, int x_off, int y_off, int relu, const int itj) {
    static_assert(!POOL || BT == 1, "pool form: one entry per workgroup");
    static_assert(!MODELS || POOL, "several models: a pool form");
    const int lane = threadIdx.x, row = blockIdx.x;
    size_t pbase = 0;                                          // POOL: the entry's state block, in floats
    const float* P = a.P;
    if constexpr (POOL) {
        const auto& en = a.tab[blockIdx.y];
        if (itj >= en.n_it || en.it0 + itj < en.g0) return;
        pbase = (size_t)en.slot * a.stride;
        if constexpr (MODELS) P = en.P;
    }
    const __amdgpu_buffer_rsrc_t rP = st_rsrc(P), rS = st_rsrc(a.state);
    const size_t wr = w_off + (size_t)row * ldw;
    const float bias = P[b_off + row];
    // (POOL: fetched here, beside the kernel arguments, as the pool form always did; left to the compiler, the load sinks
    //  behind the loop and costs a round trip of its own at the end of the launch)
    if constexpr (POOL) asm volatile("" :: "s"(bias));
    const int b0 = blockIdx.y * BT;
    const int nb = POOL ? 1 : (a.B - b0 < BT ? a.B - b0 : BT);   // utterances of this tile, processed concurrently
    float acc[BT];
#pragma unroll
    for (int u = 0; u < BT; ++u) acc[u] = 0.f;
    constexpr int RV = 5;                                      // 1280 inputs per pass: every row of these nets in one pass
    for (int i0 = 0; i0 < ni; i0 += 256 * RV) {
        float4 wv[RV], xv[RV][BT];
#pragma unroll
        for (int pc = 0; pc < RV; ++pc) {
            const int idx = i0 + pc * 256 + lane * 4;
            const bool ok = idx < ni;
            wv[pc] = st_ld4(rP, ok ? (unsigned)((wr + idx) * 4) : ST_OOB);
#pragma unroll
            for (int u = 0; u < BT; ++u) {
                if constexpr (POOL) xv[pc][u] = st_ld4(rS, ok ? st_off(pbase + x_off + idx) : ST_OOB);
                else xv[pc][u] = st_ld4(rS, (ok && u < nb) ? (unsigned)(((size_t)(b0 + u) * a.stride + x_off + idx) * 4) : ST_OOB);
            }
        }
#pragma unroll
        for (int pc = 0; pc < RV; ++pc)
#pragma unroll
            for (int u = 0; u < BT; ++u) {
                acc[u] = fmaf(wv[pc].x, xv[pc][u].x, acc[u]); acc[u] = fmaf(wv[pc].y, xv[pc][u].y, acc[u]);
                acc[u] = fmaf(wv[pc].z, xv[pc][u].z, acc[u]); acc[u] = fmaf(wv[pc].w, xv[pc][u].w, acc[u]);
            }
    }
    float mine = 0.f;
#pragma unroll
    for (int u = 0; u < BT; ++u) {
        if (u < nb) { const float sv = sum64(acc[u]); if (lane == u) mine = sv; }
    }
    if (lane < nb) {
        const float v = mine + bias;
        a.state[(POOL ? pbase : (size_t)(b0 + lane) * a.stride) + y_off + row] = relu ? fmaxf(v, 0.f) : v;
    }
}

// the same for the 1x1 layers: 8 rows x 8 utterances per workgroup, the utterances' input vectors staged in LDS
// POOL: wave w stages entry 8 by + w, lane octet u finishes entry 8 by + u, each only when that entry is generating at
// tick-local iteration `itj`
// MODELS (with POOL): tile blockIdx.y is a run of rows of ONE model (a.tile); the weight rows are that model's
template <int RV, bool POOL = false, bool MODELS = false>      // host: ni <= 256 RV
__global__ __launch_bounds__(64 * ST_TU) void rowvec_tile_kernel(const StA<POOL, MODELS> a, size_t w_off, int ldw, size_t b_off, int rows,
                                                                 int ni, int x_off, int y_off, int relu, const int itj) {
    static_assert(!MODELS || POOL, "several models: a pool form");
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [ST_TU][RV * 256]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = blockIdx.x * ST_TU + w;
    const bool live = row < rows;
    const float* P = a.P;
    if constexpr (MODELS) P = a.tab[st_tile_b0<MODELS>(a)].P;
    const __amdgpu_buffer_rsrc_t rP = st_rsrc(P), rS = st_rsrc(a.state);
    const size_t wr = w_off + (size_t)(live ? row : 0) * ldw;
    const float bias = live ? P[b_off + row] : 0.f;
    const int b0 = st_tile_b0<MODELS>(a);
    const int nb = st_tile_nb<MODELS>(a, b0);
    const int ut = lane >> 3;                                  // the utterance this lane's octet ends up with (sum64x8)
    bool onw = w < nb, onu = ut < nb;                          // this wave stages / this octet finishes an utterance
    size_t basew = (size_t)(b0 + w) * a.stride, baseu = (size_t)(b0 + ut) * a.stride;
    if constexpr (POOL) {
        const auto& ew = a.tab[b0 + (onw ? w : 0)];
        const auto& eu = a.tab[b0 + (onu ? ut : 0)];
        onw = onw && itj < ew.n_it && ew.it0 + itj >= ew.g0;
        onu = onu && itj < eu.n_it && eu.it0 + itj >= eu.g0;
        basew = (size_t)ew.slot * a.stride; baseu = (size_t)eu.slot * a.stride;
    }
    float4 wv[RV];
    {
        float4 xv[RV];
#pragma unroll
        for (int pc = 0; pc < RV; ++pc) {
            const int idx = pc * 256 + lane * 4;
            const bool ok = idx < ni;
            wv[pc] = st_ld4(rP, (ok && live) ? (unsigned)((wr + idx) * 4) : ST_OOB);
            if constexpr (POOL) xv[pc] = st_ld4(rS, (ok && onw) ? st_off(basew + x_off + idx) : ST_OOB);
            else xv[pc] = st_ld4(rS, (ok && onw) ? (unsigned)((basew + x_off + idx) * 4) : ST_OOB);
        }
#pragma unroll
        for (int pc = 0; pc < RV; ++pc) *reinterpret_cast<float4*>(xs + (w * RV + pc) * 256 + lane * 4) = xv[pc];
    }
    __syncthreads();
    float accv[ST_TU];
#pragma unroll
    for (int u = 0; u < ST_TU; ++u) {
        float acc = 0.f;
#pragma unroll
        for (int pc = 0; pc < RV; ++pc) {
            const float4 x = *reinterpret_cast<const float4*>(xs + (u * RV + pc) * 256 + lane * 4);
            acc = fmaf(wv[pc].x, x.x, acc); acc = fmaf(wv[pc].y, x.y, acc);
            acc = fmaf(wv[pc].z, x.z, acc); acc = fmaf(wv[pc].w, x.w, acc);
        }
        accv[u] = acc;
    }
    const float mine = sum64x8(accv, lane);
    if ((lane & 7) == 0 && onu && live) {
        const float v = mine + bias;
        a.state[baseu + y_off + row] = relu ? fmaxf(v, 0.f) : v;
    }
}

// ---- step_tail: out_2, sampling, history update, then the input layer of the next step ---------------
// STREAM: a chunk of a streamed decode (swn_decode_chunk): `it` stays the absolute iteration (positions, generator counters),
// out / heads / noise / forced rows are chunk-local (step ia - step0).  The other launches of the chain need no such form.
// POOL (with STREAM): entry blockIdx.x when it is generating at tick-local iteration `itj`; its io rows are those of its row
// (n_steps = the launch's n_max), its state block is in its slot, and the next input layer is formed while the entry's range
// goes on.
// MODELS (with POOL): out_2 and the next input layer read the weights of the entry's model
template <int KIND, bool STREAM = false, bool POOL = false, bool MODELS = false>
__global__ __launch_bounds__(256) void step_tail_kernel(const StA<POOL, MODELS> a, const int itj) {
    static_assert(!POOL || STREAM, "the pool form is a streamed chunk per entry");
    static_assert(!MODELS || POOL, "several models: a pool form");
    __shared__ float o2v[4096 + 16];
    __shared__ float lwin[32];                 // the updated sample window, for the fused next input layer
    const SwnGeom& g = a.g;
    int b = blockIdx.x, it = itj, step0 = a.step0, it_end = 0;
    size_t sb = (size_t)b;                     // state block
    const float* P = a.P;
    if constexpr (POOL) {
        const auto& en = a.tab[blockIdx.x];
        it = en.it0 + itj;
        if (itj >= en.n_it || it < en.g0) return;
        b = en.row; sb = (size_t)en.slot; step0 = en.g0 - a.n_pro; it_end = en.it0 + en.n_it;
        if constexpr (MODELS) P = en.P;
    }
    const int tid = threadIdx.x, lane = tid & 31, grp = tid >> 5;
    float* st = a.state + sb * a.stride;
    const int ia = it - a.n_pro, i = STREAM ? ia - step0 : ia, seg = g.seg, WN = a.WN;
    // out_2.  Wide heads (softmax: Q rows) arrive from a rowvec launch - one wave per row over the chip, like skip and
    // out_1 - in the state block; narrow heads (Laplace: <= 2 seg + lpc rows) are computed here:
    // 8 rows per pass, 32 lanes per row; branch-free loads (a row past NO / an input past O1p reads zeros)
    if (a.o2_by_rowvec) {
        for (int e = tid; e < g.NO; e += 256) o2v[e] = st[a.o_o2 + e];
    } else {
        const __amdgpu_buffer_rsrc_t rP = st_rsrc(P), rS = st_rsrc(a.state);
        const size_t xb = sb * a.stride + a.o_o1;
        for (int r0 = 0; r0 < g.NO; r0 += 8) {
            const int row = r0 + grp;
            const bool rok = row < g.NO;
            float acc = 0.f;
            for (int i0 = 0; i0 < g.O1p; i0 += 512) {
                float4 wv[4], xv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int idx = i0 + u * 128 + lane * 4;
                    const bool ok = rok && idx < g.O1p;
                    wv[u] = st_ld4(rP, ok ? (unsigned)((a.y.w2 + (size_t)row * g.O1p + idx) * 4) : ST_OOB);
                    if constexpr (POOL) xv[u] = st_ld4(rS, ok ? st_off(xb + idx) : ST_OOB);
                    else xv[u] = st_ld4(rS, ok ? (unsigned)((xb + idx) * 4) : ST_OOB);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc = fmaf(wv[u].x, xv[u].x, acc); acc = fmaf(wv[u].y, xv[u].y, acc);
                    acc = fmaf(wv[u].z, xv[u].z, acc); acc = fmaf(wv[u].w, xv[u].w, acc);
                }
            }
            acc = sum32(acc);
            if (lane == 0 && rok) o2v[row] = acc + P[a.y.b2 + row];
        }
    }
    __syncthreads();
    float* shist = st + a.o_hist;
    int* ihist = reinterpret_cast<int*>(shist);
    if (a.heads) for (int e = tid; e < g.NO; e += 256) a.heads[((size_t)b * a.n_steps + i) * g.NO + e] = o2v[e];
    if (KIND == SWN_KIND_LAPLACE) {
        if (tid == 0) {
#pragma clang fp contract(off)
            // Laplace head, cswnv_shift1.py:368-391
            const float* forced = reinterpret_cast<const float*>(a.forced);
            float* outp = reinterpret_cast<float*>(a.out) + (size_t)b * a.n_steps * seg + (size_t)i * seg;
            float lp[16], fed[16];
            const int lpc = g.lpc;
            for (int k = 0; k < lpc; ++k) lp[k] = shist[WN - lpc + k];
            for (int j = 0; j < seg; ++j) {
                const float mu = o2v[j], yv = o2v[seg + j];
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
            for (int k = 0; k + seg < WN; ++k) { const float v = shist[k + seg]; shist[k] = v; lwin[k] = v; }
            for (int j = 0; j < seg; ++j) { shist[WN - seg + j] = fed[j]; lwin[WN - seg + j] = fed[j]; }
        }
    } else if (tid < 64) {
        // softmax head, dswnv.py:361-369
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
        if ((Q & 3) == 0) {          // four classes per generator call / 16-byte noise load
            for (int g4 = tid; 4 * g4 < Q; g4 += 64) {
                const float4 q4 = swn_noise_exp1x4_at(a.nz, b, i, ia, g4, a.n_steps, Q);
                const float qv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = 4 * g4 + k;
                    const float r = ((expf(o2v[e] - m) / sum) / sum2) / qv[k];
                    if (r > best) { best = r; bi = e; }
                }
            }
        } else {
            for (int e = tid; e < Q; e += 64) {
                const float r = ((expf(o2v[e] - m) / sum) / sum2) / swn_noise_exp1_at(a.nz, b, i, ia, e, a.n_steps, Q);
                if (r > best) { best = r; bi = e; }
            }
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
            for (int k = 0; k + 1 < WN; ++k) { const int v = ihist[k + 1]; ihist[k] = v; lwin[k] = __builtin_bit_cast(float, v); }
            ihist[WN - 1] = fd; lwin[WN - 1] = __builtin_bit_cast(float, fd);
        }
    }
    // the sample window was just updated through global memory by thread 0: make it visible to the
    // block (same CU), then run the next step's input layer here - one launch less per step
    __syncthreads();
    if constexpr (POOL) {
        if (it + 1 < it_end) input_layer<KIND>(a, P, st, it + 1, tid, 256, lwin);
    } else {
        if (i + 1 < a.n_steps) input_layer<KIND>(a, P, st, it + 1, tid, 256, lwin);
    }
}

// ---- step_tail of the Laplace nets with every global operand requested up front.  The kernel above pays its dependent
//      round trips one after the other (out_2 operands, the out_2 bias, the LP window, the noise draw, the window shift, the
//      input layer's taps: 7.4-8.1 us per launch, the longest of the chain); nothing of that depends on out_2 except the
//      arithmetic, so here the sample window, the step's noise draws, the out_2 bias and the K + 1 parameter rows of the
//      next input layer are all in flight with the out_2 operands, and what follows the first barrier works on LDS and
//      registers.  Same formulas in the same order as step_tail_kernel<LAPLACE> + input_layer (bit-identical results).
// POOL (with STREAM): as step_tail_kernel
// MODELS (with POOL): as step_tail_kernel
template <int MAXE, bool STREAM = false, bool POOL = false, bool MODELS = false>   // elements (channel, position) of the next input layer per thread: ceil(H * seg / 256) <= MAXE
__global__ __launch_bounds__(256) void step_tail_laplace_kernel(const StA<POOL, MODELS> a, const int itj) {
    static_assert(!POOL || STREAM, "the pool form is a streamed chunk per entry");
    static_assert(!MODELS || POOL, "several models: a pool form");
    __shared__ float o2v[64];                  // NO <= 48
    __shared__ float lwin[32];                 // the updated sample window, for the fused next input layer
    __shared__ float lold[32];                 // the window as the step found it
    __shared__ float lnz[16];                  // the step's noise draws
    const SwnGeom& g = a.g;
    int b = blockIdx.x, it = itj, step0 = a.step0, it_end = 0;
    size_t sb = (size_t)b;                     // state block
    const float* P = a.P;
    if constexpr (POOL) {
        const auto& en = a.tab[blockIdx.x];
        it = en.it0 + itj;
        if (itj >= en.n_it || it < en.g0) return;
        b = en.row; sb = (size_t)en.slot; step0 = en.g0 - a.n_pro; it_end = en.it0 + en.n_it;
        if constexpr (MODELS) P = en.P;
    }
    const int tid = threadIdx.x, lane = tid & 31, grp = tid >> 5;
    float* st = a.state + sb * a.stride;
    const int ia = it - a.n_pro, i = STREAM ? ia - step0 : ia, seg = g.seg, WN = a.WN, H = g.H, K = g.K;
    float* shist = st + a.o_hist;
    // ---- requests: out_2 rows and bias, window, noise, input-layer parameters
    const __amdgpu_buffer_rsrc_t rP = st_rsrc(P), rS = st_rsrc(a.state);
    const size_t xb = sb * a.stride + a.o_o1;
    const int nin = g.O1p;                     // <= 512 (host)
    float4 wv[4], wv2[4], xv[4];
    const bool rok = grp < g.NO, rok2 = grp + 8 < g.NO;          // NO <= 16 (host): rows grp and grp + 8 of the 32-lane group
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int idx = u * 128 + lane * 4;
        wv[u] = st_ld4(rP, (rok && idx < nin) ? (unsigned)((a.y.w2 + (size_t)grp * g.O1p + idx) * 4) : ST_OOB);
        wv2[u] = st_ld4(rP, (rok2 && idx < nin) ? (unsigned)((a.y.w2 + (size_t)(grp + 8) * g.O1p + idx) * 4) : ST_OOB);
        if constexpr (POOL) xv[u] = st_ld4(rS, (rok && idx < nin) ? st_off(xb + idx) : ST_OOB);
        else xv[u] = st_ld4(rS, (rok && idx < nin) ? (unsigned)((xb + idx) * 4) : ST_OOB);
    }
    const float b2v = st_ld1(rP, (rok && lane == 0) ? (unsigned)((a.y.b2 + grp) * 4) : ST_OOB);
    const float b2v2 = st_ld1(rP, (rok2 && lane == 0) ? (unsigned)((a.y.b2 + grp + 8) * 4) : ST_OOB);
    float hv;
    if constexpr (POOL) hv = st_ld1(rS, tid < WN ? st_off(sb * a.stride + a.o_hist + tid) : ST_OOB);
    else hv = st_ld1(rS, tid < WN ? (unsigned)((((size_t)b * a.stride) + a.o_hist + tid) * 4) : ST_OOB);
    float ev = 0.f;
    if (tid >= 64 && tid < 64 + seg) ev = swn_noise_laplace_at(a.nz, b, i, ia, tid - 64, a.n_steps, seg);
    // next input layer (iteration it + 1, a generation step): element e = tid + 256 m -> position j = e / H, channel o
    const bool more = POOL ? it + 1 < it_end : i + 1 < a.n_steps;
    float pcb[MAXE], pcv[MAXE][8], pcc[MAXE][8];
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
        const int e = tid + 256 * m;
        const bool ok = more && e < H * seg;
        const int o = ok ? e % H : 0;
        pcb[m] = st_ld1(rP, ok ? (unsigned)((a.y.cb + o) * 4) : ST_OOB);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            pcv[m][k] = st_ld1(rP, (ok && k < K) ? (unsigned)((a.y.cv + (size_t)k * H + o) * 4) : ST_OOB);
            pcc[m][k] = st_ld1(rP, (ok && k < K) ? (unsigned)((a.y.cc + (size_t)k * H + o) * 4) : ST_OOB);
        }
    }
    // ---- out_2 (NO <= 16 rows, O1p <= 512 inputs: one pass over the inputs per row)
    {
        float acc = 0.f, acc2 = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc = fmaf(wv[u].x, xv[u].x, acc); acc = fmaf(wv[u].y, xv[u].y, acc);
            acc = fmaf(wv[u].z, xv[u].z, acc); acc = fmaf(wv[u].w, xv[u].w, acc);
            acc2 = fmaf(wv2[u].x, xv[u].x, acc2); acc2 = fmaf(wv2[u].y, xv[u].y, acc2);
            acc2 = fmaf(wv2[u].z, xv[u].z, acc2); acc2 = fmaf(wv2[u].w, xv[u].w, acc2);
        }
        acc = sum32(acc); acc2 = sum32(acc2);
        if (lane == 0 && rok) o2v[grp] = acc + b2v;
        if (lane == 0 && rok2) o2v[grp + 8] = acc2 + b2v2;
    }
    if (tid < WN) lold[tid] = hv;
    if (tid >= 64 && tid < 64 + seg) lnz[tid - 64] = ev;
    __syncthreads();
    if (a.heads) for (int e = tid; e < g.NO; e += 256) a.heads[((size_t)b * a.n_steps + i) * g.NO + e] = o2v[e];
    if (tid == 0) {
#pragma clang fp contract(off)
        // Laplace head, cswnv_shift1.py:368-391
        const float* forced = reinterpret_cast<const float*>(a.forced);
        float* outp = reinterpret_cast<float*>(a.out) + (size_t)b * a.n_steps * seg + (size_t)i * seg;
        float lp[16], fed[16];
        const int lpc = g.lpc;
        for (int k = 0; k < lpc; ++k) lp[k] = lold[WN - lpc + k];
        for (int j = 0; j < seg; ++j) {
            const float mu = o2v[j], yv = o2v[seg + j];
            const float bsc = expf(fminf(yv, 0.f) - log1pf(expf(-fabsf(yv))));
            float lpv = 0.f;
            for (int k = 0; k < lpc; ++k) lpv += o2v[2 * seg + lpc - 1 - k] * lp[k];
            const float e = lnz[j];
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
        for (int k = 0; k + seg < WN; ++k) { const float v = lold[k + seg]; shist[k] = v; lwin[k] = v; }
        for (int j = 0; j < seg; ++j) { shist[WN - seg + j] = fed[j]; lwin[WN - seg + j] = fed[j]; }
    }
    __syncthreads();
    if (!more) return;
    // ---- input layer of iteration it + 1 out of the prefetched rows (input_layer<LAPLACE>, generation form)
    const int i1 = ia + 1;
    const int q0 = g.rf + 1 - seg + i1 * seg, qe = g.rf + i1 * seg;
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
        const int e = tid + 256 * m;
        if (e < H * seg) {
            const int j = e / H, o = e - j * H, q = q0 + j;
            float acc = pcb[m];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < K) {
                    const int rr = q - (K - 1 - k);
                    int wi = rr - qe + WN - 1; wi = wi < 0 ? 0 : (wi >= WN ? WN - 1 : wi);
                    const float t = fmaf(pcv[m][k], lwin[wi], pcc[m][k]);
                    acc += (rr >= -(seg - 1)) ? t : 0.f;
                }
            }
            st[a.ring_off[0] + pmod(q, a.ring_len[0]) * g.Hp + o] = acc / (1.f + fabsf(acc));
        }
    }
}

// set the sample window after the state was zeroed: softmax = padding class Q/2 (dswnv.py:308) with the caller's seed
// class in the newest slot; Laplace = the caller's seed samples in the newest seg slots (cswnv_shift1.py:300-334)
__global__ void step_seed_kernel(const StArgs a) {
    const int b = blockIdx.x, k = threadIdx.x;
    float* hist = a.state + (size_t)b * a.stride + a.o_hist;
    if (k >= a.WN) return;
    if (a.g.kind == SWN_KIND_SOFTMAX) {
        const int sc = a.seed ? reinterpret_cast<const int*>(a.seed)[b] : a.g.Q / 2;
        reinterpret_cast<int*>(hist)[k] = (k == a.WN - 1) ? sc : a.g.Q / 2;
    } else if (a.seed && k >= a.WN - a.g.seg) {
        hist[k] = reinterpret_cast<const float*>(a.seed)[(size_t)b * a.g.seg + (k - (a.WN - a.g.seg))];
    }
}

// first launch of a pool tick: block (0, k) writes entry k of the table to the device copy the later launches read, and the
// blocks (x, k) of a BEGIN entry zero its slot and seed its sample window - what hipMemsetAsync + step_seed_kernel do for a
// whole streamed chunk, here for that slot alone (the other slots belong to other sessions).  Grid (zero blocks, entries).
// TAB / ENT: StPoolTable / StPoolEnt, or the wider rows of a call over several models (StPoolTableM / StPoolEntM).
template <class TAB, class ENT>
__global__ __launch_bounds__(256) void step_pool_setup_kernel(const StArgs a, const TAB t, ENT* tab,
                                                              unsigned long long begin_mask) {
    const int k = blockIdx.y, tid = threadIdx.x;
    const ENT& en = t.e[k];
    if (blockIdx.x == 0 && tid < (int)(sizeof(ENT) / 4)) reinterpret_cast<int*>(tab + k)[tid] = reinterpret_cast<const int*>(&en)[tid];
    if (!((begin_mask >> k) & 1ull)) return;
    float* blk = a.state + (size_t)en.slot * a.stride;
    const int n4 = a.stride / 4;                               // stride: a multiple of 64 floats
    const int WN = a.WN, seg = a.g.seg;
    const bool soft = a.g.kind == SWN_KIND_SOFTMAX;
    for (int v = blockIdx.x * 256 + tid; v < n4; v += gridDim.x * 256) {
        float q[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int kk = 4 * v + c - a.o_hist;               // step_seed_kernel's window slot
            float x = 0.f;
            if (kk >= 0 && kk < WN) {
                if (soft) {
                    const int sc = a.seed ? reinterpret_cast<const int*>(a.seed)[en.row] : a.g.Q / 2;
                    x = __builtin_bit_cast(float, (kk == WN - 1) ? sc : a.g.Q / 2);
                } else if (a.seed && kk >= WN - seg) {
                    x = reinterpret_cast<const float*>(a.seed)[(size_t)en.row * seg + (kk - (WN - seg))];
                }
            }
            q[c] = x;
        }
        reinterpret_cast<float4*>(blk)[v] = make_float4(q[0], q[1], q[2], q[3]);
    }
}

// dynamic LDS above 64 KB for the tile forms (NI = 8: 64 KB, RV = 9: 72 KB)
template <bool POOL, bool MODELS = false>
bool allow_tile_lds() {
    const int big = 72 * 1024;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(step_layer_tile_kernel<8, SWN_KIND_LAPLACE, POOL, MODELS>), hipFuncAttributeMaxDynamicSharedMemorySize, big) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(step_layer_tile_kernel<8, SWN_KIND_SOFTMAX, POOL, MODELS>), hipFuncAttributeMaxDynamicSharedMemorySize, big) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(rowvec_tile_kernel<9, POOL, MODELS>), hipFuncAttributeMaxDynamicSharedMemorySize, big) == hipSuccess;
}
constexpr int ST_SEQ = 24;                                     // utterances from which the tile forms run (launch_iteration)

// The launches of ONE iteration of the chain over the a.B utterances of `a` (POOL: the tick's active entries): the input layer
// when `in` (prologue positions and the first generation step of a launch sequence run their own; later steps get it from
// the tail of the step before), the L layers, and when `gen` the 1x1 mat-vecs and the tail.  `it` is the iteration every
// kernel takes: the absolute one, POOL: the tick-local one.  STREAM: the tails write chunk-local rows.
// MODELS: a.B covers the table rows up to the last active one (the per-entry kernels' grid), a.n_act of them are active (the
// figure the tile forms are chosen by, as in the single-model call) and the tile kernels run one workgroup row per tile of
// a.tile - the same launches as the single-model call makes.
template <bool POOL, bool STREAM, int KIND, bool MODELS = false>
void launch_iteration_of(const StA<POOL, MODELS>& a, int it, bool in, bool gen, hipStream_t st) {
    const SwnGeom& g = a.g;
    const int n = a.B;
    // up to 64 utterances: one utterance per workgroup (weights re-read per utterance from the Infinity Cache;
    // measured faster than sharing: B=8 63 vs 137 us/step, B=64 162 vs 182 us/step on REF6);
    // otherwise tiles of 8 utterances share one weight fetch and are processed concurrently (a pool has at most 64 entries)
    const bool solo = n <= 64;
    const unsigned by = solo ? (unsigned)n : (unsigned)((n + 7) / 8);
    // many utterances: tiles of 8 channel pairs (rows) x 8 utterances (step_layer_tile / rowvec_tile)
    bool seq = n >= ST_SEQ;                                    // measured crossover at REF6: 16 utterances 47 (solo) / 53 us per step, 24: 59 / 56
    unsigned sy = (unsigned)((n + ST_TU - 1) / ST_TU);
    if constexpr (MODELS) { seq = a.n_act >= ST_SEQ; sy = (unsigned)a.n_tiles; }
    if (in) hipLaunchKernelGGL((step_in_kernel<KIND, POOL, MODELS>), dim3(n), dim3(256), 0, st, a, it);
    auto layer = [&](auto ni_, int l) {
        constexpr int NI = decltype(ni_)::value;
        if (seq) hipLaunchKernelGGL((step_layer_tile_kernel<NI, KIND, POOL, MODELS>), dim3((g.H + ST_TU - 1) / ST_TU, sy), dim3(64 * ST_TU),
                                    (size_t)ST_TU * NI * 256 * sizeof(float), st, a, l, it);
        else if (solo) hipLaunchKernelGGL((step_layer_kernel<NI, KIND, 1, POOL, MODELS>), dim3(g.H, by), dim3(64), 0, st, a, l, it);
        else if constexpr (!POOL) hipLaunchKernelGGL((step_layer_kernel<NI, KIND, 8>), dim3(g.H, by), dim3(64), 0, st, a, l, it);
    };
    const int ni = (g.K * g.Hp + 255) / 256;
    for (int l = 0; l < g.L; ++l) {
        if (ni <= 1) layer(std::integral_constant<int, 1>{}, l);
        else if (ni <= 6) layer(std::integral_constant<int, 6>{}, l);
        else layer(std::integral_constant<int, 8>{}, l);
    }
    if (!gen) return;
    auto rowvec = [&](int rows, size_t w_off, int ldw, size_t b_off, int nin, int x_off, int y_off, int relu) {
        if (seq && nin <= 1280) hipLaunchKernelGGL((rowvec_tile_kernel<5, POOL, MODELS>), dim3((rows + ST_TU - 1) / ST_TU, sy), dim3(64 * ST_TU), (size_t)ST_TU * 5 * 1024, st, a, w_off, ldw, b_off, rows, nin, x_off, y_off, relu, it);
        else if (seq && nin <= 2304) hipLaunchKernelGGL((rowvec_tile_kernel<9, POOL, MODELS>), dim3((rows + ST_TU - 1) / ST_TU, sy), dim3(64 * ST_TU), (size_t)ST_TU * 9 * 1024, st, a, w_off, ldw, b_off, rows, nin, x_off, y_off, relu, it);
        else if (solo) hipLaunchKernelGGL((rowvec_kernel<1, POOL, MODELS>), dim3(rows, by), dim3(64), 0, st, a, w_off, ldw, b_off, rows, nin, x_off, y_off, relu, it);
        else if constexpr (!POOL) hipLaunchKernelGGL((rowvec_kernel<8>), dim3(rows, by), dim3(64), 0, st, a, w_off, ldw, b_off, rows, nin, x_off, y_off, relu, it);
    };
    rowvec(g.S, a.y.wsk, g.L * g.Hp, a.y.bsk, g.L * g.Hp, a.o_hcat, a.o_skip, 1);
    rowvec(g.O1, a.y.w1, g.Sp, a.y.b1, g.Sp, a.o_skip, a.o_o1, 1);
    if (a.o2_by_rowvec) rowvec(g.NO, a.y.w2, g.O1p, a.y.b2, g.O1p, a.o_o1, a.o_o2, 0);
    if constexpr (KIND == SWN_KIND_LAPLACE) {
        // Laplace heads of up to 16 rows over up to 512 inputs, K <= 8 taps, <= 1 024 input-layer elements: the prefetching tail
        if (g.NO <= 16 && g.O1p <= 512 && g.K <= 8 && g.H * g.seg <= 1024 && g.seg <= 16 && a.WN <= 32) {
            if (g.H * g.seg <= 256) hipLaunchKernelGGL((step_tail_laplace_kernel<1, STREAM, POOL, MODELS>), dim3(n), dim3(256), 0, st, a, it);
            else hipLaunchKernelGGL((step_tail_laplace_kernel<4, STREAM, POOL, MODELS>), dim3(n), dim3(256), 0, st, a, it);
            return;
        }
    }
    hipLaunchKernelGGL((step_tail_kernel<KIND, STREAM, POOL, MODELS>), dim3(n), dim3(256), 0, st, a, it);
}
template <bool POOL, bool STREAM, bool MODELS = false>
void launch_iteration(const StA<POOL, MODELS>& a, int it, bool in, bool gen, hipStream_t st) {
    if (a.g.kind == SWN_KIND_LAPLACE) launch_iteration_of<POOL, STREAM, SWN_KIND_LAPLACE, MODELS>(a, it, in, gen, st);
    else launch_iteration_of<POOL, STREAM, SWN_KIND_SOFTMAX, MODELS>(a, it, in, gen, st);
}

}  // namespace

// the launch chain of a checked call (swn_decode.hip): steps [step0, step0 + n_steps); stream = a chunk of a streamed decode:
// `state` is the session, which the prologue fills only when !resume, and the tails take their STREAM form (chunk-local rows)
int swn_decode_stepped_run(const SwnDecodeCall& c) {
    StArgs a;
    a.g = c.g;
    const int batch = c.batch, step0 = c.step0, n_steps = c.n_steps;
    if (!chain_takes(a.g, batch)) return SWN_E_UNSUPPORTED;
    fill_args(a, c.packed, c.cond, c.nz, c.forced, c.seed, c.state, c.out, c.heads, batch, c.n_frames, n_steps, step0);
    hipStream_t st = c.hip_stream;
    if (!c.resume) {
        if (hipMemsetAsync(c.state, 0, sizeof(float) * (size_t)a.stride * batch, st) != hipSuccess) return SWN_E_LAUNCH;
        if (a.g.kind == SWN_KIND_SOFTMAX || c.seed) hipLaunchKernelGGL(step_seed_kernel, dim3(batch), dim3(64), 0, st, a);
    }
    if (batch >= ST_SEQ) {
        static bool attr_set = false;
        if (!attr_set) {
            if (!allow_tile_lds<false>()) return SWN_E_LAUNCH;
            attr_set = true;
        }
    }
    // iterations: the prologue positions (not when resuming), then the chunk's generation steps at absolute indices
    const int it_gen0 = a.n_pro + step0, total = it_gen0 + n_steps;
    for (int it = c.resume ? it_gen0 : 0; it < total; ++it) {
        const bool in = it < a.n_pro || it == it_gen0, gen = it >= a.n_pro;
        if (c.stream) launch_iteration<false, true>(a, it, in, gen, st);
        else launch_iteration<false, false>(a, it, in, gen, st);
    }
    return swn_launch_status("swn_decode(stepped)");
}

// the state buffer of the chain, which is also the session of a streamed decode
size_t swn_decode_stepped_state_floats(const SwnGeom& g, int batch) {
    StArgs a;
    a.g = g;
    return batch < 1 ? 0 : (size_t)plan(a) * batch;
}

// whether the chain runs this (net, batch) (the conditions swn_decode_stepped_run returns SWN_E_UNSUPPORTED under)
bool swn_decode_stepped_supported(const SwnGeom& g, int batch) { return batch >= 1 && chain_takes(g, batch); }

// ---- stepped decode pool -------------------------------------------------------------------------------------------
extern "C" int swn_decode_stepped_prologue_iterations(const swn_net_desc* d) {
    SwnGeom g;
    const int rc = swn_make_geom(d, &g);
    if (rc < 0) return rc;
    return g.rf - g.seg + 1;
}

namespace {

// what the checks of a stepped pool call find out about its table
struct StPoolCall {
    int n_max, it_max;                         // most generation steps / iterations of an entry
    bool any_begin;
};

// the argument rules of swn_decode_pool_stepped_chunk (include/swn_hip.h), and with `models` those the call over several
// models adds; nothing is launched before they pass
int pool_check(const SwnGeom& g, const float* packed, const float* const* models, int n_models,
               const int32_t* model_of_entry, int capacity, const swn_decode_stepped_pool_entry* entries, int n_entries,
               const swn_decode_io* io, const float* session, const void* out, StPoolCall& c) {
    if ((!models && !packed) || !entries || !io || !session) return SWN_E_BADARG;
    if (capacity < 1 || n_entries < 1 || n_entries > SWN_DECODE_POOL_MAX_ENTRIES) return SWN_E_BADARG;
    if (models || model_of_entry) {
        const int rc = swn_pool_models_check(models, n_models, model_of_entry, n_entries);
        if (rc != SWN_OK) return rc;
    }
    if (io->noise_dev || io->forced_dev) return SWN_E_BADARG;    // pools draw their noise on the device, no teacher forcing
    const int n_pro = g.rf - g.seg + 1;
    int n_max = 0, it_max = 0;
    bool any_begin = false;
    for (int e = 0; e < n_entries; ++e) {
        const swn_decode_stepped_pool_entry& en = entries[e];
        const bool begin = (en.flags & SWN_CHUNK_BEGIN) != 0;
        if (!en.cond_dev || en.n_frames < 1 || en.slot < 0 || en.slot >= capacity || en.it0 < 0 || en.n_it < 0 ||
            (en.flags & ~SWN_CHUNK_BEGIN) || en.reserved != 0)
            return SWN_E_BADARG;
        if (begin && en.it0 != 0) return SWN_E_BADARG;
        if (!begin && en.it0 == 0 && en.n_it > 0) return SWN_E_BADARG;     // a session's iteration 0 runs from BEGIN only
        const long long end = (long long)en.it0 + en.n_it;
        if (end > (long long)INT32_MAX) return SWN_E_BADARG;
        const long long n_gen = end > n_pro ? end - (en.it0 > n_pro ? en.it0 : n_pro) : 0;
        if (end > n_pro && (end - n_pro) * g.seg > (long long)en.n_frames * g.U) return SWN_E_BADARG;   // conditioning
        for (int f = 0; f < e; ++f)
            if (entries[f].slot == en.slot) return SWN_E_BADARG;   // two entries on one session
        n_max = n_gen > n_max ? (int)n_gen : n_max;
        it_max = en.n_it > it_max ? en.n_it : it_max;
        any_begin = any_begin || begin;
    }
    if (n_max > 0 && !out) return SWN_E_BADARG;
    if (!swn_decode_stepped_supported(g, capacity)) return SWN_E_UNSUPPORTED;
    c.n_max = n_max; c.it_max = it_max; c.any_begin = any_begin;
    return SWN_OK;
}

// row k of a tick's table: entry `e` of the caller's
template <class ENT>
void pool_row(ENT& r, const swn_decode_stepped_pool_entry& en, int e, int n_pro) {
    r.cond = en.cond_dev; r.Tf = en.n_frames; r.slot = en.slot; r.it0 = en.it0;
    r.n_it = en.n_it; r.row = e; r.g0 = en.it0 > n_pro ? en.it0 : n_pro;
}

}  // namespace

extern "C" int swn_decode_pool_stepped_chunk(const swn_net_desc* d, const float* packed, int capacity,
                                             const swn_decode_stepped_pool_entry* entries, int n_entries,
                                             const swn_decode_io* io, float* session, void* out, float* heads,
                                             void* stream_) {
    StPoolArgs a;
    int rc = swn_make_geom(d, &a.g);
    if (rc < 0) return rc;
    const SwnGeom& g = a.g;
    StPoolCall c;
    rc = pool_check(g, packed, nullptr, 0, nullptr, capacity, entries, n_entries, io, session, out, c);
    if (rc != SWN_OK) return rc;
    const int n_pro = g.rf - g.seg + 1, n_max = c.n_max, it_max = c.it_max;
    const bool any_begin = c.any_begin;
    if (!any_begin && it_max == 0) return SWN_OK;           // every slot stays as it is

    fill_args(a, packed, nullptr, swn_pool_noise_of(io), nullptr, io->seed_dev, session, out, heads, n_entries, 0, n_max, 0);
    // the table, sorted by n_it (descending, stable): the entries active at tick-local iteration j are a prefix of it
    StPoolTable t = {};
    int order[SWN_DECODE_POOL_MAX_ENTRIES];
    for (int e = 0; e < n_entries; ++e) order[e] = e;
    for (int x = 1; x < n_entries; ++x)
        for (int y = x; y > 0 && entries[order[y]].n_it > entries[order[y - 1]].n_it; --y) {
            const int tmp = order[y]; order[y] = order[y - 1]; order[y - 1] = tmp;
        }
    unsigned long long begin_mask = 0;
    for (int k = 0; k < n_entries; ++k) {
        const swn_decode_stepped_pool_entry& en = entries[order[k]];
        pool_row(t.e[k], en, order[k], n_pro);
        if (en.flags & SWN_CHUNK_BEGIN) begin_mask |= 1ull << k;
    }
    StPoolEnt* tab = reinterpret_cast<StPoolEnt*>(session + (size_t)a.stride * capacity);
    a.tab = tab;
    hipStream_t st = (hipStream_t)stream_;
    (void)hipGetLastError();
    const StArgs& base = a;
    hipLaunchKernelGGL((step_pool_setup_kernel<StPoolTable, StPoolEnt>), dim3(any_begin ? 64 : 1, n_entries), dim3(256), 0, st, base, t, tab, begin_mask);

    // dynamic LDS above 64 KB for the tile forms (set on every call that uses them: the attribute is per device)
    bool any_seq = false;
    for (int j = 0; j < it_max && !any_seq; ++j) {
        int nact = 0;
        while (nact < n_entries && t.e[nact].n_it > j) ++nact;
        any_seq = nact >= ST_SEQ;
    }
    if (any_seq && !allow_tile_lds<true>()) return SWN_E_LAUNCH;
    int nact = n_entries;
    for (int j = 0; j < it_max; ++j) {
        while (nact > 0 && t.e[nact - 1].n_it <= j) --nact;
        bool need_in = false, need_gen = false;
        for (int k = 0; k < nact; ++k) {
            const int it = t.e[k].it0 + j;
            need_in = need_in || it < n_pro || it == t.e[k].g0;
            need_gen = need_gen || it >= t.e[k].g0;
        }
        a.B = nact;
        launch_iteration<true, true>(a, j, need_in, need_gen, st);
    }
    return swn_launch_status("swn_decode_pool_stepped_chunk");
}

// ---- stepped decode pool over several models -----------------------------------------------------------------------
extern "C" int swn_decode_stepped_pool_plan(const int32_t* model_of_entry, const int32_t* n_it, int n_entries, int n_models,
                                            int j, int32_t* order_out, int32_t* tiles_out) {
    if (!model_of_entry || !n_it || !order_out || !tiles_out || j < 0) return SWN_E_BADARG;
    if (n_entries < 1 || n_entries > SWN_DECODE_POOL_MAX_ENTRIES || n_models < 1 || n_models > SWN_POOL_MAX_MODELS)
        return SWN_E_BADARG;
    for (int e = 0; e < n_entries; ++e)
        if (model_of_entry[e] < 0 || model_of_entry[e] >= n_models || n_it[e] < 0) return SWN_E_BADARG;
    // (model, n_it descending), stable: insertion sort, as the single-model call sorts by n_it
    for (int e = 0; e < n_entries; ++e) order_out[e] = e;
    auto before = [&](int x, int y) {           // entry x must come in front of entry y, which now stands in front of it
        return model_of_entry[x] < model_of_entry[y] || (model_of_entry[x] == model_of_entry[y] && n_it[x] > n_it[y]);
    };
    for (int x = 1; x < n_entries; ++x)
        for (int y = x; y > 0 && before(order_out[y], order_out[y - 1]); --y) {
            const int tmp = order_out[y]; order_out[y] = order_out[y - 1]; order_out[y - 1] = tmp;
        }
    // the active entries of a model are a prefix of its group: cut it into runs of at most 8 rows
    int nt = 0;
    for (int k = 0; k < n_entries;) {
        const int m = model_of_entry[order_out[k]];
        int end = k, act = k;
        while (end < n_entries && model_of_entry[order_out[end]] == m) ++end;
        while (act < end && n_it[order_out[act]] > j) ++act;
        for (int r = k; r < act; r += ST_TU) {
            if (nt >= SWN_DECODE_STEPPED_POOL_MAX_TILES) return SWN_E_BADARG;   // (not reached: 64 entries over 16 models give 22)
            tiles_out[3 * nt] = r; tiles_out[3 * nt + 1] = act - r < ST_TU ? act - r : ST_TU; tiles_out[3 * nt + 2] = m;
            ++nt;
        }
        k = end;
    }
    return nt;
}

extern "C" int swn_decode_pool_stepped_chunk_models(const swn_net_desc* d, const float* const* models, int n_models,
                                                    const int32_t* model_of_entry, int capacity,
                                                    const swn_decode_stepped_pool_entry* entries, int n_entries,
                                                    const swn_decode_io* io, float* session, void* out, float* heads,
                                                    void* stream_) {
    StModelsArgs a;
    int rc = swn_make_geom(d, &a.g);
    if (rc < 0) return rc;
    const SwnGeom& g = a.g;
    if (!models || !model_of_entry) return SWN_E_BADARG;
    StPoolCall c;
    rc = pool_check(g, nullptr, models, n_models, model_of_entry, capacity, entries, n_entries, io, session, out, c);
    if (rc != SWN_OK) return rc;
    const int n_pro = g.rf - g.seg + 1, it_max = c.it_max;
    if (!c.any_begin && it_max == 0) return SWN_OK;         // every slot stays as it is

    // no kernel of this call reads a.P: every weight pointer comes from a table row
    fill_args(a, models[0], nullptr, swn_pool_noise_of(io), nullptr, io->seed_dev, session, out, heads, n_entries, 0, c.n_max, 0);
    // the table, sorted by (model, n_it descending), and the tiles of iteration 0
    int32_t n_it[SWN_DECODE_POOL_MAX_ENTRIES], order[SWN_DECODE_POOL_MAX_ENTRIES], tiles[3 * (SWN_DECODE_STEPPED_POOL_MAX_TILES + 1)];
    for (int e = 0; e < n_entries; ++e) n_it[e] = entries[e].n_it;
    int nt = swn_decode_stepped_pool_plan(model_of_entry, n_it, n_entries, n_models, 0, order, tiles);
    if (nt < 0) return nt;
    StPoolTableM t = {};
    unsigned long long begin_mask = 0;
    int n_act0 = 0;
    for (int k = 0; k < n_entries; ++k) {
        const swn_decode_stepped_pool_entry& en = entries[order[k]];
        pool_row(t.e[k], en, order[k], n_pro);
        t.e[k].P = models[model_of_entry[order[k]]];
        if (en.flags & SWN_CHUNK_BEGIN) begin_mask |= 1ull << k;
        n_act0 += en.n_it > 0 ? 1 : 0;
    }
    StPoolEntM* tab = reinterpret_cast<StPoolEntM*>(session + (size_t)a.stride * capacity);
    a.tab = tab;
    a.n_tiles = 0; a.n_act = 0;
    for (int& x : a.tile) x = 0;
    hipStream_t st = (hipStream_t)stream_;
    (void)hipGetLastError();
    const StArgs& base = a;
    hipLaunchKernelGGL((step_pool_setup_kernel<StPoolTableM, StPoolEntM>), dim3(c.any_begin ? 64 : 1, n_entries), dim3(256), 0, st, base, t, tab, begin_mask);

    // dynamic LDS above 64 KB for the tile forms (set on every call that uses them; iteration 0 has the most active entries)
    if (n_act0 >= ST_SEQ && !allow_tile_lds<true, true>()) return SWN_E_LAUNCH;
    for (int j = 0; j < it_max; ++j) {
        // the tiles change only when an entry runs out
        bool ran_out = false;
        for (int e = 0; e < n_entries; ++e) ran_out = ran_out || n_it[e] == j;
        if (j > 0 && ran_out) {
            nt = swn_decode_stepped_pool_plan(model_of_entry, n_it, n_entries, n_models, j, order, tiles);
            if (nt < 0) return nt;
        }
        if (j == 0 || ran_out) {
            a.n_tiles = nt; a.n_act = 0; a.B = 0;
            for (int x = 0; x < nt; ++x) {
                a.tile[x] = tiles[3 * x] | (tiles[3 * x + 1] << 8);
                a.n_act += tiles[3 * x + 1];
                a.B = tiles[3 * x] + tiles[3 * x + 1];      // the tiles are in table order: the last one ends the active rows
            }
        }
        bool need_in = false, need_gen = false;
        for (int x = 0; x < nt; ++x)
            for (int k = tiles[3 * x]; k < tiles[3 * x] + tiles[3 * x + 1]; ++k) {
                const int it = t.e[k].it0 + j;
                need_in = need_in || it < n_pro || it == t.e[k].g0;
                need_gen = need_gen || it >= t.e[k].g0;
            }
        launch_iteration<true, true, true>(a, j, need_in, need_gen, st);
    }
    return swn_launch_status("swn_decode_pool_stepped_chunk_models");
}
