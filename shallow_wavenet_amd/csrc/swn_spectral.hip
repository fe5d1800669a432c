// Multi-resolution STFT loss of the CSWNV recipe (train_driver.batch_loss: complex-STFT L1 + the reported log-spectral
// distance over a list of FFT sizes), forward and backward, fp32 end to end.
//
// STFT_n(x) is torch.stft's default form: hop n/4, center = reflect padding of n/2, periodic Hann window, one-sided
// (n/2 + 1 bins), 1 + T / hop frames, no normalisation.  The sizes are multiples of 32, not powers of two, so the
// transform is the dense DFT of each windowed frame on the exact-fp32 matrix instruction (v_mfma_f32_16x16x4_f32):
//      Re[f][b] =  sum_j x[f*hop + j] * w[j] * cos(2 pi j b / n)          Im[f][b] = -sum_j x[..] * w[j] * sin(2 pi j b / n)
// Frames are read out of an LDS image of the reflect-padded signal span of the tile (never materialised in memory); the
// basis comes from a per-size table cos(2 pi m / n), m < n, indexed with (j * b) mod n; n is a multiple of 4, so
// sin(2 pi m / n) is the same table n/4 entries earlier.  The window is folded into the basis operand.
//
// Forward, per (size, row, tile of 8 frames, chunk of 128 bins): one 16-row MFMA tile holds 8 frames of d = sample - target
// (rows 0-7) and the same 8 frames of the target (rows 8-15): L1 is linear, so |STFT(sample) - STFT(target)| = |STFT(d)|,
// which avoids the cancellation of two nearly equal transforms; the LSD figure takes STFT(sample) = STFT(d) + STFT(target).
// Each wave owns 2 x 16 bins (4 independent accumulators: re / im of each).  The epilogue pairs a lane with the lane 32
// further (same frame, same bin, other signal), writes the two signs of STFT(d) as one byte per (frame, bin) when the
// backward will run, and reduces |.| and the squared dB difference in a fixed order into per-block partials; a second small
// kernel sums the partials per (row, size) in a fixed order.  No floating-point atomics anywhere: same input, same bits.
//
// Backward, per (size, row, tile of 16 frames, chunk of 256 frame samples): y[f][j] = w[j] * c * sum_b (sRe[f][b] *
// cos(2 pi j b / n) - sIm[f][b] * sin(2 pi j b / n)), c = g[row][size] / count, as a signs x basis product on the same
// instruction, written per frame; the fold kernel then gathers, per output sample, the <= 4 frames that cover each of
// its <= 3 positions in the reflect-padded signal, over all sizes, in a fixed order.
#include <hip/hip_runtime.h>
#include "swn_geom.hpp"
#include "swn_mma.hpp"
#include <climits>

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_FWD_FR = 8;      // frames per forward tile (x 2 signals = 16 MFMA rows)
constexpr int SP_FWD_BINS = 128;  // bins per forward block: 4 waves x 2 bin tiles x 16
constexpr int SP_BWD_FR = 16;     // frames per backward tile
constexpr int SP_BWD_J = 256;     // frame samples per backward block: 4 waves x 4 tiles x 16
constexpr int SP_BWD_RUN = 64;    // bins one backward accumulation chain runs over before it joins the total
constexpr int SP_HOPROWS = SP_FWD_FR + 3;   // hops a forward tile's signal span covers

struct SpecSize {
    int n, hop, frames, bins;
    int fwd_tiles, fwd_chunks, fwd_blk0;    // blocks [blk0, blk0 + rows * tiles * chunks) of the launch: the largest size first,
    int bwd_tiles, bwd_chunks, bwd_blk0;    // so that the long blocks start early and the short ones fill the tail
    int tab_off;        // floats into the tables: cos[n], window[n]
    int sign_off;       // bytes into the sign state: [row][frame][bin]
    int l1_off;         // floats into the l1 partials: [row][fwd_tile][fwd_chunk]
    int lsd_off;        // floats into the lsd partials: [row][fwd_tile * 8 + frame][fwd_chunk]
    int y_off;          // floats into the backward frame buffer: [row][frame][n]
    float inv_count;    // 1 / (bins * frames * 2)
};
struct SpecArgs {
    SpecSize s[SWN_SPECTRAL_MAX_SIZES];
    int nk, rows, len;
};
struct SpecPlan {
    SpecArgs a;
    int fwd_blocks, bwd_blocks;
    size_t sign_bytes, fwd_work_floats, bwd_work_floats, l1_floats;
    size_t fwd_lds, bwd_lds;
};

// LDS image of a forward tile: hop row q of the span at q * (hop + 4) (the pad keeps the 16 frame rows x 4 k lanes of an
// operand read on 64 different banks), the target's image 32 banks after a multiple of 64 for the same reason
__host__ __device__ inline int sp_fwd_pitch(int hop) { return hop + 4; }
__host__ __device__ inline int sp_fwd_xt(int hop) { return (SP_HOPROWS * sp_fwd_pitch(hop) + 63) / 64 * 64 + 32; }
__host__ __device__ inline int sp_fwd_lds_floats(int n) {
    return sp_fwd_xt(n / 4) + SP_HOPROWS * sp_fwd_pitch(n / 4) + 2 * n + 80;
}
__host__ __device__ inline int sp_bwd_pitch(int bins) { return (((bins + 3) / 4) | 1) * 4; }   // bytes, 4 * odd

int sp_plan(int rows, int len, const int* sizes, int n_sizes, SpecPlan* p) {
    if (!sizes || rows < 1 || len < 1 || n_sizes < 1 || n_sizes > SWN_SPECTRAL_MAX_SIZES) return SWN_E_BADARG;
    size_t sign = 0, l1 = 0, lsd = 0, y = 0, tab = 0, fb = 0, bb = 0;
    size_t fl = 0, bl = 0;
    p->a.nk = n_sizes; p->a.rows = rows; p->a.len = len;
    for (int k = 0; k < n_sizes; ++k) {
        const int n = sizes[k];
        if (n < 32 || n > SWN_SPECTRAL_MAX_FFT || n % 32 != 0 || len <= n / 2) return SWN_E_BADARG;
        SpecSize& z = p->a.s[k];
        z.n = n; z.hop = n / 4; z.frames = 1 + len / z.hop; z.bins = n / 2 + 1;
        z.fwd_tiles = (z.frames + SP_FWD_FR - 1) / SP_FWD_FR;
        z.fwd_chunks = (z.bins + SP_FWD_BINS - 1) / SP_FWD_BINS;
        z.bwd_tiles = (z.frames + SP_BWD_FR - 1) / SP_BWD_FR;
        z.bwd_chunks = (n + SP_BWD_J - 1) / SP_BWD_J;
        z.inv_count = (float)(1.0 / ((double)z.bins * z.frames * 2.0));
        if (sign > INT_MAX || l1 > INT_MAX || lsd > INT_MAX || y > INT_MAX) return SWN_E_UNSUPPORTED;
        z.tab_off = (int)tab; z.sign_off = (int)sign; z.l1_off = (int)l1; z.lsd_off = (int)lsd; z.y_off = (int)y;
        tab += 2 * (size_t)n;
        sign += (size_t)rows * z.frames * z.bins;
        l1 += (size_t)rows * z.fwd_tiles * z.fwd_chunks;
        lsd += (size_t)rows * z.fwd_tiles * SP_FWD_FR * z.fwd_chunks;
        y += (size_t)rows * z.frames * n;
        const size_t f = (size_t)sp_fwd_lds_floats(n) * sizeof(float);
        const size_t b = (size_t)n * sizeof(float) + (size_t)SP_BWD_FR * sp_bwd_pitch(z.bins);
        fl = f > fl ? f : fl; bl = b > bl ? b : bl;
    }
    bool placed[SWN_SPECTRAL_MAX_SIZES] = {};
    for (int i = 0; i < n_sizes; ++i) {                      // block ranges in descending order of size
        int k = -1;
        for (int c = 0; c < n_sizes; ++c)
            if (!placed[c] && (k < 0 || p->a.s[c].n > p->a.s[k].n)) k = c;
        placed[k] = true;
        SpecSize& z = p->a.s[k];
        if (fb > INT_MAX || bb > INT_MAX) return SWN_E_UNSUPPORTED;
        z.fwd_blk0 = (int)fb; z.bwd_blk0 = (int)bb;
        fb += (size_t)rows * z.fwd_tiles * z.fwd_chunks;
        bb += (size_t)rows * z.bwd_tiles * z.bwd_chunks;
    }
    if (sign > INT_MAX || l1 > INT_MAX || lsd > INT_MAX || y > INT_MAX || fb > INT_MAX || bb > INT_MAX ||
        (size_t)rows * len > INT_MAX)
        return SWN_E_UNSUPPORTED;
    p->fwd_blocks = (int)fb; p->bwd_blocks = (int)bb;
    p->sign_bytes = sign; p->l1_floats = l1; p->fwd_work_floats = l1 + lsd; p->bwd_work_floats = y;
    p->fwd_lds = fl; p->bwd_lds = bl;
    return SWN_OK;
}

__device__ __forceinline__ int sp_sign_code(float v) { return v > 0.f ? 1 : (v < 0.f ? 2 : 0); }
__device__ __forceinline__ float sp_sign_val(int c) { return c == 1 ? 1.f : (c == 2 ? -1.f : 0.f); }

// ---------------------------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(SP_THREADS) void spectral_fwd_kernel(const SpecArgs a, const float* __restrict__ samples,
                                                                  const float* __restrict__ targets,
                                                                  const float* __restrict__ tables,
                                                                  unsigned char* __restrict__ signs,
                                                                  float* __restrict__ l1part, float* __restrict__ lsdpart) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    int k = 0;
    for (int c = 1; c < a.nk; ++c)                          // the size whose block range holds this block
        if ((int)blockIdx.x >= a.s[c].fwd_blk0 && (a.s[k].fwd_blk0 > (int)blockIdx.x || a.s[c].fwd_blk0 > a.s[k].fwd_blk0)) k = c;
    const SpecSize z = a.s[k];
    const int local = (int)blockIdx.x - z.fwd_blk0;
    const int chunk = local % z.fwd_chunks, tile = (local / z.fwd_chunks) % z.fwd_tiles, r = local / (z.fwd_chunks * z.fwd_tiles);
    const int n = z.n, hop = z.hop, T = a.len, pitch = sp_fwd_pitch(hop);
    float* xd = sm;
    float* xt = sm + sp_fwd_xt(hop);
    float* tab = xt + SP_HOPROWS * pitch;
    float* win = tab + n;
    float* red = win + n;                                   // [4 waves][2 bin tiles][8 frames] + [4] l1
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, kq = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    for (int i = tid; i < 2 * n; i += SP_THREADS) tab[i] = tables[z.tab_off + i];           // cos, then the window
    const float* srow = samples + (size_t)r * T;
    const float* trow = targets + (size_t)r * T;
    const int p0 = tile * SP_FWD_FR * hop;                  // first position of the span in the padded signal
    const int span = SP_HOPROWS * hop;
    for (int e0 = tid; e0 < span; e0 += 4 * SP_THREADS) {   // 4 independent loads in flight per thread: no branch around them
        float sv[4], tv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = p0 + e0 + u * SP_THREADS;
            int i = p - n / 2;
            i = i < 0 ? -i : (i >= T ? 2 * (T - 1) - i : i);
            i = (p < T + n) ? i : 0;                        // past the padded signal: any valid address, value dropped below
            sv[u] = srow[i];
            tv[u] = trow[i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * SP_THREADS;
            if (e < span) {
                const bool in = p0 + e < T + n;
                const int q = e / hop, at = q * pitch + (e - q * hop);
                xd[at] = in ? sv[u] - tv[u] : 0.f;
                xt[at] = in ? tv[u] : 0.f;
            }
        }
    }
    __syncthreads();

    // both bin tiles of the wave always run (a tile past the last bin only in the last chunk; its lanes read valid table
    // entries and are dropped in the epilogue): no branch inside the loop, the accumulators stay where the MFMA wants them
    const int bt0 = chunk * SP_FWD_BINS + 32 * w;           // first bin of this wave
    swn_f32x4 acc[2][2] = {};                               // [bin tile][re, im]
    if (bt0 < z.bins) {
        const int b0 = bt0 + c, b1 = bt0 + 16 + c;
        const int st0 = (4 * b0) % n, st1 = (4 * b1) % n, quarter = n / 4;
        int i0 = (kq * b0) % n, i1 = (kq * b1) % n;
        const float* ap = (c < SP_FWD_FR ? xd + c * pitch : xt + (c - SP_FWD_FR) * pitch) + kq;
        const int steps = hop / 4;                          // even: hop is a multiple of 8
        for (int q = 0; q < 4; ++q) {
            const float* aq = ap + q * pitch;
            const float* wq = win + q * hop + kq;
            for (int it = 0; it < steps; it += 2) {         // two k steps per trip: 12 LDS reads ahead of 8 MFMAs
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float wv = wq[4 * (it + u)], x = aq[4 * (it + u)];
                    int s0 = i0 - quarter; s0 += s0 < 0 ? n : 0;
                    int s1 = i1 - quarter; s1 += s1 < 0 ? n : 0;
                    const float c0 = wv * tab[i0], n0 = -wv * tab[s0], c1 = wv * tab[i1], n1 = -wv * tab[s1];
                    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, c0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, n0, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, c1, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, n1, acc[1][1], 0, 0, 0);
                    i0 += st0; i0 -= i0 >= n ? n : 0;
                    i1 += st1; i1 -= i1 >= n ? n : 0;
                }
            }
        }
    }

    // accumulator element i of lane (c, kq): bin c of the tile, MFMA row 4 kq + i = frame 4 kq + i of d (kq < 2) or frame
    // 4 (kq - 2) + i of the target: lane ^ 32 holds the other signal of the same (frame, bin)
    float l1 = 0.f;
    const size_t srow0 = (size_t)z.sign_off + (size_t)r * z.frames * z.bins;
#pragma unroll
    for (int bt = 0; bt < 2; ++bt) {
        const int b = bt0 + 16 * bt + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float vr = acc[bt][0][i], vi = acc[bt][1][i];
            const float tr = __shfl_xor(vr, 32), ti = __shfl_xor(vi, 32);
            const int f = tile * SP_FWD_FR + 4 * kq + i;
            const bool ok = kq < 2 && f < z.frames && b < z.bins;
            float v = 0.f;
            if (ok) {
                l1 += fabsf(vr) + fabsf(vi);
                if (signs) signs[srow0 + (size_t)f * z.bins + b] = (unsigned char)(sp_sign_code(vr) | (sp_sign_code(vi) << 2));
                const float sr = vr + tr, si = vi + ti;
                const float db = 10.f * (log10f(sr * sr + si * si) - log10f(tr * tr + ti * ti));
                v = db * db;
            }
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
            if (c == 0 && kq < 2) red[(w * 2 + bt) * SP_FWD_FR + 4 * kq + i] = v;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) l1 += __shfl_xor(l1, m);
    if (lane == 0) red[64 + w] = l1;
    __syncthreads();
    if (tid < SP_FWD_FR) {
        float s = 0.f;
        for (int q = 0; q < 8; ++q) s += red[q * SP_FWD_FR + tid];
        lsdpart[(size_t)z.lsd_off + ((size_t)(r * z.fwd_tiles + tile) * SP_FWD_FR + tid) * z.fwd_chunks + chunk] = s;
    }
    if (tid == 0)
        l1part[(size_t)z.l1_off + (size_t)(r * z.fwd_tiles + tile) * z.fwd_chunks + chunk] = (red[64] + red[65]) + (red[66] + red[67]);
}

// fixed-order sum of SP_THREADS values, result in every thread
__device__ __forceinline__ float sp_block_sum(float v, float* red) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (size, row): l1[r][k] = sum of the |.| partials / count; lsd[r][k] = mean_frames sqrt(mean_bins dB^2)
__global__ __launch_bounds__(SP_THREADS) void spectral_finish_kernel(const SpecArgs a, const float* __restrict__ l1part,
                                                                     const float* __restrict__ lsdpart,
                                                                     float* __restrict__ l1, float* __restrict__ lsd) {
    __shared__ float red[4];
    const int k = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const SpecSize z = a.s[k];
    float s = 0.f;
    const int np = z.fwd_tiles * z.fwd_chunks;
    for (int i = tid; i < np; i += SP_THREADS) s += l1part[(size_t)z.l1_off + (size_t)r * np + i];
    s = sp_block_sum(s, red);
    float d = 0.f;
    for (int f = tid; f < z.frames; f += SP_THREADS) {
        const float* p = lsdpart + (size_t)z.lsd_off + ((size_t)r * z.fwd_tiles * SP_FWD_FR + f) * z.fwd_chunks;
        float m = 0.f;
        for (int ch = 0; ch < z.fwd_chunks; ++ch) m += p[ch];
        d += sqrtf(m / (float)z.bins);
    }
    d = sp_block_sum(d, red);
    if (tid == 0) {
        l1[(size_t)r * a.nk + k] = s * z.inv_count;
        lsd[(size_t)r * a.nk + k] = d / (float)z.frames;
    }
}

// --------------------------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(SP_THREADS) void spectral_bwd_kernel(const SpecArgs a, const float* __restrict__ g,
                                                                  const unsigned char* __restrict__ signs,
                                                                  const float* __restrict__ tables, float* __restrict__ ybuf) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    int k = 0;
    for (int c = 1; c < a.nk; ++c)                          // the size whose block range holds this block
        if ((int)blockIdx.x >= a.s[c].bwd_blk0 && (a.s[k].bwd_blk0 > (int)blockIdx.x || a.s[c].bwd_blk0 > a.s[k].bwd_blk0)) k = c;
    const SpecSize z = a.s[k];
    const int local = (int)blockIdx.x - z.bwd_blk0;
    const int chunk = local % z.bwd_chunks, tile = (local / z.bwd_chunks) % z.bwd_tiles, r = local / (z.bwd_chunks * z.bwd_tiles);
    const int n = z.n, bp = sp_bwd_pitch(z.bins);
    float* tab = sm;
    unsigned char* sg = reinterpret_cast<unsigned char*>(sm + n);     // [16 frames][bp]
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, kq = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    for (int i = tid; i < n; i += SP_THREADS) tab[i] = tables[z.tab_off + i];
    const unsigned char* srow = signs + (size_t)z.sign_off + (size_t)r * z.frames * z.bins;
    const int fr_left = z.frames - tile * SP_BWD_FR;        // frames of this tile that exist (>= 1)
    for (int e0 = tid; e0 < SP_BWD_FR * bp; e0 += 8 * SP_THREADS) {      // 8 independent loads in flight per thread
        unsigned char v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * SP_THREADS, f = e / bp, b = e - f * bp;
            const bool in = f < SP_BWD_FR && f < fr_left && b < z.bins;
            v[u] = srow[in ? (size_t)(tile * SP_BWD_FR + f) * z.bins + b : 0];
            v[u] = in ? v[u] : (unsigned char)0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * SP_THREADS;
            if (e < SP_BWD_FR * bp) sg[e] = v[u];
        }
    }
    __syncthreads();

    const int j0 = chunk * SP_BWD_J + 64 * w + c;           // frame sample of j tile 0; tile jt is 16 jt further
    if (j0 - c >= n) return;
    // blocked summation: the MFMA chain runs over SP_BWD_RUN bins (2 x 64 terms), then joins a second accumulator.  One
    // chain over all 2 (n / 2 + 1) terms of +-basis values random-walks to about sqrt(n) and rounds every step at that
    // magnitude: measured 1.2e-6 of the largest gradient value at n = 2 048 alone, 1.8e-7 with the runs
    swn_f32x4 acc[4] = {}, tot[4] = {};
    int idx[4], st[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + 16 * jt;
        idx[jt] = (kq * j) % n;
        st[jt] = (4 * j) % n;
    }
    const int quarter = n / 4;
    const unsigned char* sp = sg + c * bp + kq;
    for (int run0 = 0; run0 < z.bins; run0 += SP_BWD_RUN) {
        const int run1 = run0 + SP_BWD_RUN < z.bins ? run0 + SP_BWD_RUN : z.bins;
        for (int b0 = run0; b0 < run1; b0 += 4) {
            const int code = sp[b0];
            const float are = sp_sign_val(code & 3), aim = sp_sign_val(code >> 2);
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(are, tab[idx[jt]], acc[jt], 0, 0, 0);
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                int s = idx[jt] - quarter; s += s < 0 ? n : 0;
                acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aim, -tab[s], acc[jt], 0, 0, 0);
                idx[jt] += st[jt]; idx[jt] -= idx[jt] >= n ? n : 0;
            }
        }
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            tot[jt] += acc[jt];
            acc[jt] = swn_f32x4{};
        }
    }
    const float coef = g[(size_t)r * a.nk + k] * z.inv_count;
    const float* win = tables + z.tab_off + n;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + 16 * jt;
        if (j < n) {
            const float wc = win[j] * coef;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = tile * SP_BWD_FR + 4 * kq + i;
                if (f < z.frames) ybuf[(size_t)z.y_off + ((size_t)r * z.frames + f) * n + j] = tot[jt][i] * wc;
            }
        }
    }
}

// overlap-add of the frame gradients and the fold through the reflect padding: thread per output sample
__global__ __launch_bounds__(SP_THREADS) void spectral_fold_kernel(const SpecArgs a, const float* __restrict__ ybuf,
                                                                   float* __restrict__ grad) {
    const int t = blockIdx.x * SP_THREADS + threadIdx.x, r = blockIdx.y, T = a.len;
    if (t >= T) return;
    float acc = 0.f;
    for (int k = 0; k < a.nk; ++k) {
        const SpecSize z = a.s[k];
        const int n = z.n, hop = z.hop, half = n / 2;
        const float* y = ybuf + (size_t)z.y_off + (size_t)r * z.frames * n;
        const int i2 = 2 * (T - 1) - t;
        const int pos[3] = {t + half, (t >= 1 && t <= half) ? half - t : -1, (i2 >= T && i2 <= T - 1 + half) ? i2 + half : -1};
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const int p = pos[m];
            if (p < 0) continue;
            const int fh = p / hop;
            const int lo = fh - 3 > 0 ? fh - 3 : 0, hi = fh < z.frames - 1 ? fh : z.frames - 1;
            for (int f = lo; f <= hi; ++f) acc += y[(size_t)f * n + (p - f * hop)];
        }
    }
    grad[(size_t)r * T + t] = acc;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ C ABI
extern "C" size_t swn_spectral_work_bytes(int rows, int len, const int* sizes, int n_sizes) {
    SpecPlan p;
    if (sp_plan(rows, len, sizes, n_sizes, &p) != SWN_OK) return 0;
    return sizeof(float) * (p.fwd_work_floats > p.bwd_work_floats ? p.fwd_work_floats : p.bwd_work_floats);
}

extern "C" size_t swn_spectral_state_bytes(int rows, int len, const int* sizes, int n_sizes) {
    SpecPlan p;
    if (sp_plan(rows, len, sizes, n_sizes, &p) != SWN_OK) return 0;
    return p.sign_bytes;
}

extern "C" int swn_spectral_forward(const float* samples_dev, const float* targets_dev, int rows, int len, const int* sizes,
                                    int n_sizes, const float* tables_dev, float* l1_dev, float* lsd_dev,
                                    unsigned char* state_dev, void* work_dev, void* stream) {
    SpecPlan p;
    const int rc = sp_plan(rows, len, sizes, n_sizes, &p);
    if (rc != SWN_OK) return rc;
    if (!samples_dev || !targets_dev || !tables_dev || !l1_dev || !lsd_dev || !work_dev) return SWN_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    float* l1part = static_cast<float*>(work_dev);
    float* lsdpart = l1part + p.l1_floats;
    hipLaunchKernelGGL(spectral_fwd_kernel, dim3(p.fwd_blocks), dim3(SP_THREADS), p.fwd_lds, st, p.a, samples_dev, targets_dev,
                       tables_dev, state_dev, l1part, lsdpart);
    int lrc = swn_launch_status("swn_spectral_forward");
    if (lrc != SWN_OK) return lrc;
    hipLaunchKernelGGL(spectral_finish_kernel, dim3(n_sizes, rows), dim3(SP_THREADS), 0, st, p.a, l1part, lsdpart, l1_dev, lsd_dev);
    return swn_launch_status("swn_spectral_forward (finish)");
}

extern "C" int swn_spectral_backward(const float* g_dev, const unsigned char* state_dev, int rows, int len, const int* sizes,
                                     int n_sizes, const float* tables_dev, float* grad_dev, void* work_dev, void* stream) {
    SpecPlan p;
    const int rc = sp_plan(rows, len, sizes, n_sizes, &p);
    if (rc != SWN_OK) return rc;
    if (!g_dev || !state_dev || !tables_dev || !grad_dev || !work_dev) return SWN_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    float* ybuf = static_cast<float*>(work_dev);
    hipLaunchKernelGGL(spectral_bwd_kernel, dim3(p.bwd_blocks), dim3(SP_THREADS), p.bwd_lds, st, p.a, g_dev, state_dev,
                       tables_dev, ybuf);
    int lrc = swn_launch_status("swn_spectral_backward");
    if (lrc != SWN_OK) return lrc;
    hipLaunchKernelGGL(spectral_fold_kernel, dim3((len + SP_THREADS - 1) / SP_THREADS, rows), dim3(SP_THREADS), 0, st, p.a,
                       ybuf, grad_dev);
    return swn_launch_status("swn_spectral_backward (fold)");
}
