// Pool form of the frame-rate front end (swn_frontend_pool, include/swn_hip.h): one call finalises the conditioning of up to
// 64 independent sessions, each at its own frame position, in a number of launches that does not depend on how many there are.
//
// A tick of a decode pool is 64 sessions x 2-10 new frames: one swn_frontend per session runs four launches for a handful of
// frames each and restages the same weight rows 64 times.  Here every stage works on the CONCATENATED frame list of all
// entries.  Stage 0 is the output of scale_in, stage i + 1 the output of conv_aux layer i; stage s of entry e holds the absolute
// frames  [f0 - h_s, f1 + h_s) ∩ [0, n_received)  where h_s is the half-width of the layers after it (fp_ranges).  Its
// activations lie channel-major in the work buffer, (channels, T_s) with T_s = the stage's frames over all entries, entry e at
// columns [pre[s][e], pre[s][e + 1]).  A tile is 64 consecutive columns of that list - whichever entries they belong to - so
// 64 entries of 2 frames fill two tiles of the last layer instead of 64, and a 600-frame entry beside them is ten more.
//
//   fp_setup_kernel   block 0 turns the entry table (kernel arguments) into the device table FpTab at the head of the work
//                     buffer; blocks 1 .. E append entry e's new frames to its feature buffer
//   fp_conv_kernel    scale_in (ks = 1, reads each entry's own feature buffer) and every conv_aux layer (reads the stage before)
//   fp_cond_kernel    the hoisted in_x GEMM over the kept rows of all entries: Wx is read once per 64 kept rows, each row is
//                     stored at its entry's cond_dev + frame * N
//
// Arithmetic: the fmaf chains of csrc/swn_frontend.hip - scale_in from the bias over ci ascending, conv_aux from the bias over
// (ci ascending, k ascending), cond from 0 over c ascending.  A tap outside [0, n_received) contributes fmaf(w, 0, acc) exactly
// as the one-shot kernels' zero padding does, so every row is bit-identical to swn_frontend over the whole utterance.
//
// Several models (swn_frontend_pool_models): a tile stages ONE set of weight rows, so it must not span two models.  The host
// orders the entries by model (stably), and in every stage the first column of each model's entries is rounded up to a
// multiple of 64: a tile then lies inside one model's columns, and takes that model's weights through the device table
// (FpTabM::model of the entry of its first column).  The columns skipped by the rounding belong to no entry: they are
// computed from valid addresses (their taps read as zero, their cond inputs are whatever the work buffer holds) and never
// stored.  The kernels are instantiations of the same bodies (MODELS), the single-model ones stay the code they were.
#include <hip/hip_runtime.h>
#include "swn_geom.hpp"
#include "swn_pool.hpp"

namespace {

constexpr int FP_MAXE = SWN_FRONTEND_POOL_MAX_ENTRIES;
constexpr int FP_STAGES = SWN_MAXAUX + 1;
constexpr int FP_JB = 96;                    // (ci, k) pairs staged per pass: 24 KB of taps + 6 KB of weight rows in LDS
constexpr long FP_MAX_COLS = 1L << 24;       // columns of one stage over all entries

// frames [lo[s], lo[s] + cnt[s]) of stage s that the kept frames [f0, f1) need; pad[i] = half-width of conv_aux layer i
__host__ __device__ inline void fp_ranges(int f0, int f1, int n_received, const int* pad, int auxl, int* lo, int* cnt) {
    int h = 0;
    for (int s = auxl; s >= 0; --s) {
        const int a = f0 > h ? f0 - h : 0;
        const int b = n_received - f1 > h ? f1 + h : n_received;
        lo[s] = a;
        cnt[s] = f1 > f0 ? b - a : 0;
        if (s > 0) h += pad[s - 1];
    }
}

// the device copy of a call's table, written by its first launch and read by the others
struct FpTab {
    const float* aux[FP_MAXE];               // feature buffers (n_aux, stride)
    float* cond[FP_MAXE];
    int stride[FP_MAXE];
    int lo[FP_STAGES][FP_MAXE];              // first absolute frame of the entry's columns in stage s
    int pre[FP_STAGES][FP_MAXE + 1];         // first column of the entry in stage s; pre[s][n] = T_s
};
constexpr size_t FP_TAB_FLOATS = 1024;
static_assert(sizeof(FpTab) <= FP_TAB_FLOATS * 4, "the device table fits the head of the work buffer");

// ... of a call over several models: the entries are in model order, pre[s][e] of a model's first entry is a multiple of 64, so
// pre[s][e + 1] - pre[s][e] no longer is entry e's column count
struct FpTabM : FpTab {
    int cnt[FP_STAGES][FP_MAXE];             // columns of the entry in stage s
    const float* model[FP_MAXE];             // the entry's packed parameters
};
constexpr size_t FP_TABM_FLOATS = 2048;
static_assert(sizeof(FpTabM) <= FP_TABM_FLOATS * 4, "the device table fits the head of the work buffer");

// columns of entry e in stage s
__device__ __forceinline__ int fp_cnt(const FpTab* t, int s, int e) { return t->pre[s][e + 1] - t->pre[s][e]; }
__device__ __forceinline__ int fp_cnt(const FpTabM* t, int s, int e) { return t->cnt[s][e]; }

struct FpSetupArgs {
    swn_frontend_pool_entry e[FP_MAXE];
    FpTab* tab;
    int n, n_aux, auxl;
    int pad[SWN_MAXAUX];
};
static_assert(sizeof(swn_frontend_pool_entry) == 56, "swn_frontend_pool_entry is 56 bytes (include/swn_hip.h)");
static_assert(sizeof(FpSetupArgs) <= 4096, "fp_setup_kernel's arguments fit 4 KB");

// the entries in model order, then the model table (m.of[e] = model of the e-th entry of THIS order)
struct FpSetupArgsM {
    swn_frontend_pool_entry e[FP_MAXE];
    FpTabM* tab;
    int n, n_aux, auxl;
    int pad[SWN_MAXAUX];
    SwnPoolModels m;
};
static_assert(sizeof(FpSetupArgsM) <= 4096, "fp_setup_models_kernel's arguments fit 4 KB");

// first column of a stage's next entry: where a new model begins, the next multiple of 64
__host__ __device__ inline int fp_model_start(int p, bool new_model) { return new_model ? (p + 63) & ~63 : p; }

template <bool MODELS, class A>
__device__ __forceinline__ void fp_setup_body(const A& a) {
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        if (blockIdx.y != 0) return;
        __shared__ int cnt[FP_STAGES][FP_MAXE];
        auto* t = a.tab;
        if (tid < a.n) {
            const swn_frontend_pool_entry& en = a.e[tid];
            int lo[FP_STAGES], c[FP_STAGES];
            fp_ranges(en.f0, en.f1, en.n_received, a.pad, a.auxl, lo, c);
            t->aux[tid] = en.aux_dev; t->cond[tid] = en.cond_dev; t->stride[tid] = en.aux_stride;
            for (int s = 0; s <= a.auxl; ++s) { t->lo[s][tid] = lo[s]; cnt[s][tid] = c[s]; }
            if constexpr (MODELS) {
                for (int s = 0; s <= a.auxl; ++s) t->cnt[s][tid] = c[s];
                t->model[tid] = a.m.p[a.m.of[tid]];
            }
        }
        __syncthreads();
        if (tid <= a.auxl) {                                 // one thread per stage: 64 additions
            int p = 0;
            for (int e = 0; e < a.n; ++e) {
                if constexpr (MODELS) p = fp_model_start(p, e > 0 && a.m.of[e] != a.m.of[e - 1]);
                t->pre[tid][e] = p; p += cnt[tid][e];
            }
            t->pre[tid][a.n] = p;
        }
        return;
    }
    // append: aux[c][n_received - n_new + j] = new[c][j]
    const swn_frontend_pool_entry& en = a.e[blockIdx.x - 1];
    const int n_new = en.n_new;
    if (n_new <= 0) return;
    const size_t tot = (size_t)a.n_aux * n_new;
    const size_t at = (size_t)(en.n_received - n_new);
    for (size_t i = (size_t)blockIdx.y * 256 + tid; i < tot; i += (size_t)gridDim.y * 256) {
        const size_t c = i / n_new, j = i - c * n_new;
        en.aux_dev[c * (size_t)en.aux_stride + at + j] = en.new_dev[i];
    }
}

__global__ __launch_bounds__(256) void fp_setup_kernel(const FpSetupArgs a) { fp_setup_body<false>(a); }
__global__ __launch_bounds__(256) void fp_setup_models_kernel(const FpSetupArgsM a) { fp_setup_body<true>(a); }

// column g of a stage -> its entry: the last e with pre[e] <= g (entries without columns are stepped over)
__device__ __forceinline__ int fp_entry_of(const int* pre, int n, int g) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// Stage s of the chain over a tile of 64 columns x 16 output channels (wave w: outputs 4w .. 4w + 3 of the sixteen, lane = column).
//   out[co][g] = bias[co] + sum_j W[co][j] * x_j(g),   j = ci * ks + k ascending,   x_j(g) = in[ci][frame(g) + (k - half) * dil]
// The J = cin * ks taps go through LDS in passes of FP_JB: each thread gathers its column's taps (neighbouring columns may belong
// to different entries, so a tap is addressed per column and never by the column beside it) with eight loads in flight, the
// sixteen weight rows of the pass are fetched coalesced, and the multiply-adds then run from LDS.  A tap outside the entry's
// input range is loaded from a valid address and replaced by zero: no branch sits between the loads.
// MODELS: the columns between a model's last entry and the next model's first belong to no entry: not valid, whatever g is.
template <int KS, bool MODELS, class Tab>
__device__ __forceinline__ void fp_conv_body(
    const Tab* __restrict__ tab, int s, int n, const float* __restrict__ in, float* __restrict__ out,
    const float* __restrict__ w, const float* __restrict__ bias, int cin, int cout, int ks_rt, int dil, int t_in, int t_out) {
    __shared__ float xs[FP_JB][64];
    __shared__ __attribute__((aligned(16))) float wl[4][FP_JB][4];
    __shared__ int pre_s[FP_MAXE + 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int cg = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ks = KS ? KS : ks_rt, half = (ks - 1) / 2, J = cin * ks;
    if (tid <= n) pre_s[tid] = tab->pre[s][tid];
    __syncthreads();
    const int g = blockIdx.x * 64 + lane;
    const int gc = g < t_out ? g : t_out - 1;
    const int e = fp_entry_of(pre_s, n, gc);
    const bool valid = g < t_out && (!MODELS || gc - pre_s[e] < fp_cnt(tab, s, e));
    const int f = tab->lo[s][e] + gc - pre_s[e];
    // the entry's input: its own feature buffer for scale_in (one tap, always inside), else its columns of the stage before
    const float* base; size_t pitch; int lo_in, hi_in;
    if (s == 0) {
        base = tab->aux[e]; pitch = (size_t)tab->stride[e]; lo_in = 0; hi_in = 0x7fffffff;
    } else {
        const int p0 = tab->pre[s - 1][e];
        lo_in = tab->lo[s - 1][e]; hi_in = lo_in + fp_cnt(tab, s - 1, e);
        base = in + ((ptrdiff_t)p0 - lo_in); pitch = (size_t)t_in;
    }
    const int co0 = blockIdx.y * 16 + 4 * cg;
    float acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = (co0 + r < cout) ? bias[co0 + r] : 0.f;

    for (int j0 = 0; j0 < J; j0 += FP_JB) {
        for (int u0 = 0; u0 < FP_JB; u0 += 32) {
            float v[8]; bool ok[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u0 + cg + 4 * u;
                const int ci = j / ks, k = j - ci * ks;
                const int ff = f + (k - half) * dil;
                ok[u] = valid && j < J && ff >= lo_in && ff < hi_in;
                const float* p = ok[u] ? base + ((size_t)ci * pitch + (size_t)ff) : w;
                v[u] = *p;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) xs[u0 + cg + 4 * u][lane] = ok[u] ? v[u] : 0.f;
        }
        {
            // this wave stages output `cg` of every wave's group of four
            float v[4][2]; bool ok[4][2];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int co = blockIdx.y * 16 + 4 * q + cg, jl = lane + 64 * h, j = j0 + jl;
                    ok[q][h] = co < cout && j < J && jl < FP_JB;
                    const float* p = ok[q][h] ? w + ((size_t)co * J + j) : w;
                    v[q][h] = *p;
                }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int jl = lane + 64 * h;
                    if (jl < FP_JB) wl[q][jl][cg] = ok[q][h] ? v[q][h] : 0.f;
                }
        }
        __syncthreads();
        const int jn = J - j0 < FP_JB ? J - j0 : FP_JB;
        const float4* wq = reinterpret_cast<const float4*>(&wl[cg][0][0]);
#pragma unroll 4
        for (int jl = 0; jl < jn; ++jl) {
            const float x = xs[jl][lane];
            const float4 w4 = wq[jl];
            acc[0] = fmaf(w4.x, x, acc[0]);
            acc[1] = fmaf(w4.y, x, acc[1]);
            acc[2] = fmaf(w4.z, x, acc[2]);
            acc[3] = fmaf(w4.w, x, acc[3]);
        }
        __syncthreads();
    }
    if (valid) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (co0 + r < cout) out[(size_t)(co0 + r) * t_out + g] = acc[r];
    }
}

template <int KS>
__global__ __launch_bounds__(256) void fp_conv_kernel(
    const FpTab* __restrict__ tab, int s, int n, const float* __restrict__ in, float* __restrict__ out,
    const float* __restrict__ w, const float* __restrict__ bias, int cin, int cout, int ks_rt, int dil, int t_in, int t_out) {
    fp_conv_body<KS, false>(tab, s, n, in, out, w, bias, cin, cout, ks_rt, dil, t_in, t_out);
}

// the packed parameters of a tile: those of the entry of its first column (a model's columns start at a multiple of 64)
__device__ __forceinline__ const float* fp_tile_model(const FpTabM* tab, int s, int n) {
    return tab->model[fp_entry_of(tab->pre[s], n, blockIdx.x * 64)];
}

// w_off, b_off: the layer's weights and bias in a packed buffer
template <int KS>
__global__ __launch_bounds__(256) void fp_conv_models_kernel(
    const FpTabM* __restrict__ tab, int s, int n, const float* __restrict__ in, float* __restrict__ out,
    size_t w_off, size_t b_off, int cin, int cout, int ks_rt, int dil, int t_in, int t_out) {
    const float* P = fp_tile_model(tab, s, n);
    fp_conv_body<KS, true>(tab, s, n, in, out, P + w_off, P + b_off, cin, cout, ks_rt, dil, t_in, t_out);
}

// cond row of column m of the last stage = sum_c Wx[n][c] * C[c][m]: the GEMM of cond_gemm_kernel (csrc/swn_frontend.hip: 64 x 64
// tile, BK = 16, 4 x 4 outputs per thread, fp32 fmaf chains in ascending c, the next k-tile fetched ahead) over the kept rows of
// ALL entries; row m is stored at its entry's cond_dev + frame * N.
template <bool MODELS, class Tab>
__device__ __forceinline__ void fp_cond_body(
    const Tab* __restrict__ tab, int s, int n, const float* __restrict__ C, const float* __restrict__ Wx,
    int M, int N, int A0, int A0p) {
    __shared__ float As[16][64 + 4];
    __shared__ float Bs[16][64 + 4];
    __shared__ int pre_s[FP_MAXE + 1];
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const int tid = threadIdx.x;
    const int tm = (tid & 15) * 4, tn = (tid >> 4) * 4;
    if (tid <= n) pre_s[tid] = tab->pre[s][tid];
    float acc[4][4] = {};
    float ra[4]; float4 rb;
    const int nn = tid >> 2, kq = (tid & 3) * 4;
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, kk = e >> 6, mm = e & 63;
            const int k = k0 + kk, m = m0 + mm;
            ra[i] = (k < A0 && m < M) ? C[(size_t)k * M + m] : 0.f;
        }
        const int nc = n0 + nn, k = k0 + kq;
        rb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nc < N && k < A0p) rb = *reinterpret_cast<const float4*>(Wx + (size_t)nc * A0p + k);
    };
    fetch(0);
    for (int k0 = 0; k0 < A0; k0 += 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int e = tid + 256 * i; As[e >> 6][e & 63] = ra[i]; }
        Bs[kq + 0][nn] = rb.x; Bs[kq + 1][nn] = rb.y; Bs[kq + 2][nn] = rb.z; Bs[kq + 3][nn] = rb.w;
        __syncthreads();
        if (k0 + 16 < A0) fetch(k0 + 16);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const float4 a = *reinterpret_cast<const float4*>(&As[kk][tm]);
            const float4 bb = *reinterpret_cast<const float4*>(&Bs[kk][tn]);
            const float av[4] = {a.x, a.y, a.z, a.w};
            const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + tm + i;
        if (m >= M) continue;
        const int e = fp_entry_of(pre_s, n, m);
        if (MODELS && m - pre_s[e] >= fp_cnt(tab, s, e)) continue;     // a column between two models
        const size_t frame = (size_t)(tab->lo[s][e] + m - pre_s[e]);
        float* row = tab->cond[e] + frame * (size_t)N;
        if (n0 + tn + 3 < N && (N & 3) == 0) {
            *reinterpret_cast<float4*>(row + n0 + tn) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n0 + tn + j < N) row[n0 + tn + j] = acc[i][j];
        }
    }
}

__global__ __launch_bounds__(256) void fp_cond_kernel(
    const FpTab* __restrict__ tab, int s, int n, const float* __restrict__ C, const float* __restrict__ Wx,
    int M, int N, int A0, int A0p) {
    fp_cond_body<false>(tab, s, n, C, Wx, M, N, A0, A0p);
}

__global__ __launch_bounds__(256) void fp_cond_models_kernel(
    const FpTabM* __restrict__ tab, int s, int n, const float* __restrict__ C, size_t wx_off, int M, int N, int A0, int A0p) {
    fp_cond_body<true>(tab, s, n, C, fp_tile_model(tab, s, n) + wx_off, M, N, A0, A0p);
}

// checks of swn_frontend_pool's table; on success tot[s] = columns of stage s over all entries, new_max = longest append
int fp_check(const SwnGeom& g, const swn_frontend_pool_entry* en, int n, long* tot, int* new_max) {
    if (!en || n < 1 || n > FP_MAXE) return SWN_E_BADARG;
    int la = 0;
    for (int i = 0; i < g.auxl; ++i) la += g.aux_pad[i];
    for (int s = 0; s <= g.auxl; ++s) tot[s] = 0;
    *new_max = 0;
    for (int e = 0; e < n; ++e) {
        const swn_frontend_pool_entry& x = en[e];
        if (!x.aux_dev || !x.cond_dev) return SWN_E_BADARG;
        if ((x.flags & ~SWN_FRONTEND_FINAL) != 0 || x.reserved[0] != 0 || x.reserved[1] != 0) return SWN_E_BADARG;
        if (x.f0 < 0 || x.f1 < x.f0 || x.n_new < 0 || x.n_received < 0) return SWN_E_BADARG;
        if (x.n_new > x.n_received || x.aux_stride < x.n_received) return SWN_E_BADARG;
        if (x.n_new > 0 && !x.new_dev) return SWN_E_BADARG;
        if ((g.N & 3) == 0 && ((uintptr_t)x.cond_dev & 15) != 0) return SWN_E_BADARG;   // rows are stored in 16-byte pieces
        const bool fin = (x.flags & SWN_FRONTEND_FINAL) != 0;
        // not FINAL: final_frames() of streaming.py, max(0, n_received - lookahead)
        if (fin ? x.f1 > x.n_received : (x.f1 > 0 && (long)x.f1 > (long)x.n_received - la)) return SWN_E_BADARG;
        for (int o = 0; o < e; ++o)
            if (en[o].cond_dev == x.cond_dev) return SWN_E_BADARG;
        int lo[FP_STAGES], cnt[FP_STAGES];
        fp_ranges(x.f0, x.f1, x.n_received, g.aux_pad, g.auxl, lo, cnt);
        for (int s = 0; s <= g.auxl; ++s) {
            tot[s] += cnt[s];
            if (tot[s] > FP_MAX_COLS) return SWN_E_BADARG;
        }
        if (x.n_new > *new_max) *new_max = x.n_new;
    }
    return SWN_OK;
}

// swn_frontend_pool_models: the checks of the table and of the model arguments; on success ord[i] = the entry at position i of
// the model order (stable), tot[s] = columns of stage s with every model's first column at a multiple of 64
int fp_check_models(const SwnGeom& g, const swn_frontend_pool_entry* en, const int32_t* model_of, int n, int n_models,
                    int* ord, long* tot, int* new_max) {
    long plain[FP_STAGES];
    const int rc = fp_check(g, en, n, plain, new_max);
    if (rc < 0) return rc;
    if (!model_of || n_models < 1 || n_models > SWN_POOL_MAX_MODELS) return SWN_E_BADARG;
    int at = 0;
    for (int m = 0; m < n_models; ++m)
        for (int e = 0; e < n; ++e) {
            if (model_of[e] < 0 || model_of[e] >= n_models) return SWN_E_BADARG;
            if (model_of[e] == m) ord[at++] = e;
        }
    for (int s = 0; s <= g.auxl; ++s) tot[s] = 0;
    for (int i = 0; i < n; ++i) {
        const swn_frontend_pool_entry& x = en[ord[i]];
        int lo[FP_STAGES], cnt[FP_STAGES];
        fp_ranges(x.f0, x.f1, x.n_received, g.aux_pad, g.auxl, lo, cnt);
        const bool new_model = i > 0 && model_of[ord[i]] != model_of[ord[i - 1]];
        for (int s = 0; s <= g.auxl; ++s) tot[s] = fp_model_start((int)tot[s], new_model) + cnt[s];
    }
    return SWN_OK;
}

}  // namespace

extern "C" size_t swn_frontend_pool_models_work_floats(const swn_net_desc* d, const swn_frontend_pool_entry* entries_host,
                                                       const int32_t* model_of_entry_host, int n_entries, int n_models) {
    SwnGeom g; long tot[FP_STAGES]; int new_max, ord[FP_MAXE];
    if (swn_make_geom(d, &g) < 0 ||
        fp_check_models(g, entries_host, model_of_entry_host, n_entries, n_models, ord, tot, &new_max) < 0)
        return 0;
    size_t fl = FP_TABM_FLOATS + (size_t)g.n_aux * tot[0];
    for (int i = 0; i < g.auxl; ++i) fl += (size_t)g.aux_cout[i] * tot[i + 1];
    return fl;
}

extern "C" int swn_frontend_pool_models(const swn_net_desc* d, const float* const* models, int n_models,
                                        const int32_t* model_of_entry, const swn_frontend_pool_entry* entries, int n_entries,
                                        float* work, void* stream_) {
    SwnGeom g; int rc = swn_make_geom(d, &g);
    if (rc < 0) return rc;
    if (!work) return SWN_E_BADARG;
    long tot[FP_STAGES]; int new_max, ord[FP_MAXE];
    if ((rc = fp_check_models(g, entries, model_of_entry, n_entries, n_models, ord, tot, &new_max)) < 0) return rc;
    if (swn_pool_models_check(models, n_models, model_of_entry, n_entries) < 0) return SWN_E_BADARG;
    if (tot[g.auxl] == 0 && new_max == 0) return SWN_OK;       // nothing to append, nothing to finalise
    SwnLayout y; swn_make_layout(&g, &y);
    hipStream_t st = (hipStream_t)stream_;
    (void)hipGetLastError();
    FpTabM* tab = reinterpret_cast<FpTabM*>(work);
    {
        FpSetupArgsM a;
        a.m = SwnPoolModels{};
        for (int i = 0; i < n_entries; ++i) { a.e[i] = entries[ord[i]]; a.m.of[i] = (unsigned char)model_of_entry[ord[i]]; }
        for (int i = n_entries; i < FP_MAXE; ++i) a.e[i] = swn_frontend_pool_entry{};
        for (int m = 0; m < SWN_POOL_MAX_MODELS; ++m) a.m.p[m] = models[m < n_models ? m : 0];
        a.tab = tab; a.n = n_entries; a.n_aux = g.n_aux; a.auxl = g.auxl;
        for (int i = 0; i < SWN_MAXAUX; ++i) a.pad[i] = i < g.auxl ? g.aux_pad[i] : 0;
        const size_t per = (size_t)g.n_aux * new_max;
        const int gy = per > 256 * 8 ? 8 : (per > 256 ? (int)((per + 255) / 256) : 1);
        hipLaunchKernelGGL(fp_setup_models_kernel, dim3(1 + n_entries, gy), dim3(256), 0, st, a);
    }
    if (tot[g.auxl] > 0) {
        float* cur = work + FP_TABM_FLOATS;
        const float* src = nullptr;
        for (int s = 0; s <= g.auxl; ++s) {
            const int cin = s == 0 ? g.n_aux : g.aux_cin[s - 1], cout = s == 0 ? g.n_aux : g.aux_cout[s - 1];
            const int ks = s == 0 ? 1 : g.auxk, dil = s == 0 ? 1 : g.aux_dil[s - 1];
            const size_t wo = s == 0 ? y.scale_w : y.aux_w[s - 1], bo = s == 0 ? y.scale_b : y.aux_b[s - 1];
            const int t_in = s == 0 ? 0 : (int)tot[s - 1], t_out = (int)tot[s];
            dim3 grid((t_out + 63) / 64, (cout + 15) / 16);
            if (ks == 1)
                hipLaunchKernelGGL(fp_conv_models_kernel<1>, grid, dim3(256), 0, st, tab, s, n_entries, src, cur, wo, bo, cin, cout, ks, dil, t_in, t_out);
            else if (ks == 3)
                hipLaunchKernelGGL(fp_conv_models_kernel<3>, grid, dim3(256), 0, st, tab, s, n_entries, src, cur, wo, bo, cin, cout, ks, dil, t_in, t_out);
            else
                hipLaunchKernelGGL(fp_conv_models_kernel<0>, grid, dim3(256), 0, st, tab, s, n_entries, src, cur, wo, bo, cin, cout, ks, dil, t_in, t_out);
            src = cur;
            cur += (size_t)cout * t_out;
        }
        const int M = (int)tot[g.auxl];
        dim3 grid((M + 63) / 64, (g.N + 63) / 64);
        hipLaunchKernelGGL(fp_cond_models_kernel, grid, dim3(256), 0, st, tab, g.auxl, n_entries, src, (size_t)y.wx, M, g.N, g.A0, g.A0p);
    }
    return swn_launch_status("swn_frontend_pool_models");
}

extern "C" size_t swn_frontend_pool_work_floats(const swn_net_desc* d, const swn_frontend_pool_entry* entries_host,
                                                int n_entries) {
    SwnGeom g; long tot[FP_STAGES]; int new_max;
    if (swn_make_geom(d, &g) < 0 || fp_check(g, entries_host, n_entries, tot, &new_max) < 0) return 0;
    size_t fl = FP_TAB_FLOATS + (size_t)g.n_aux * tot[0];
    for (int i = 0; i < g.auxl; ++i) fl += (size_t)g.aux_cout[i] * tot[i + 1];
    return fl;
}

extern "C" int swn_frontend_pool(const swn_net_desc* d, const float* packed, const swn_frontend_pool_entry* entries,
                                 int n_entries, float* work, void* stream_) {
    SwnGeom g; int rc = swn_make_geom(d, &g);
    if (rc < 0) return rc;
    if (!packed || !work) return SWN_E_BADARG;
    long tot[FP_STAGES]; int new_max;
    if ((rc = fp_check(g, entries, n_entries, tot, &new_max)) < 0) return rc;
    if (tot[g.auxl] == 0 && new_max == 0) return SWN_OK;       // nothing to append, nothing to finalise
    SwnLayout y; swn_make_layout(&g, &y);
    hipStream_t st = (hipStream_t)stream_;
    (void)hipGetLastError();
    FpTab* tab = reinterpret_cast<FpTab*>(work);
    {
        FpSetupArgs a;
        for (int e = 0; e < n_entries; ++e) a.e[e] = entries[e];
        for (int e = n_entries; e < FP_MAXE; ++e) a.e[e] = swn_frontend_pool_entry{};
        a.tab = tab; a.n = n_entries; a.n_aux = g.n_aux; a.auxl = g.auxl;
        for (int i = 0; i < SWN_MAXAUX; ++i) a.pad[i] = i < g.auxl ? g.aux_pad[i] : 0;
        const size_t per = (size_t)g.n_aux * new_max;
        const int gy = per > 256 * 8 ? 8 : (per > 256 ? (int)((per + 255) / 256) : 1);
        hipLaunchKernelGGL(fp_setup_kernel, dim3(1 + n_entries, gy), dim3(256), 0, st, a);
    }
    if (tot[g.auxl] > 0) {
        float* cur = work + FP_TAB_FLOATS;
        const float* src = nullptr;
        for (int s = 0; s <= g.auxl; ++s) {
            const int cin = s == 0 ? g.n_aux : g.aux_cin[s - 1], cout = s == 0 ? g.n_aux : g.aux_cout[s - 1];
            const int ks = s == 0 ? 1 : g.auxk, dil = s == 0 ? 1 : g.aux_dil[s - 1];
            const float* wv = packed + (s == 0 ? y.scale_w : y.aux_w[s - 1]);
            const float* bv = packed + (s == 0 ? y.scale_b : y.aux_b[s - 1]);
            const int t_in = s == 0 ? 0 : (int)tot[s - 1], t_out = (int)tot[s];
            dim3 grid((t_out + 63) / 64, (cout + 15) / 16);
            if (ks == 1)
                hipLaunchKernelGGL(fp_conv_kernel<1>, grid, dim3(256), 0, st, tab, s, n_entries, src, cur, wv, bv, cin, cout, ks, dil, t_in, t_out);
            else if (ks == 3)
                hipLaunchKernelGGL(fp_conv_kernel<3>, grid, dim3(256), 0, st, tab, s, n_entries, src, cur, wv, bv, cin, cout, ks, dil, t_in, t_out);
            else
                hipLaunchKernelGGL(fp_conv_kernel<0>, grid, dim3(256), 0, st, tab, s, n_entries, src, cur, wv, bv, cin, cout, ks, dil, t_in, t_out);
            src = cur;
            cur += (size_t)cout * t_out;
        }
        const int M = (int)tot[g.auxl];
        dim3 grid((M + 63) / 64, (g.N + 63) / 64);
        hipLaunchKernelGGL(fp_cond_kernel, grid, dim3(256), 0, st, tab, g.auxl, n_entries, src, packed + y.wx, M, g.N, g.A0, g.A0p);
    }
    return swn_launch_status("swn_frontend_pool");
}
