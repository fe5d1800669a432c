// Log-mel conditioning features from waveforms (melspec.py, swn_logmel of include/swn_hip.h), fp32 end to end.
//
// Definition (the contract; restated in include/swn_hip.h and melspec.py).  For a signal of len samples, len > n_fft / 2:
//   frames      F = 1 + len / hop; frame f reads the padded positions p = f * hop - n_fft / 2 + j, j < n_fft, with reflect
//               padding that does not repeat the edge sample: p < 0 -> -p, p >= len -> 2 (len - 1) - p
//               (torch.stft(center=True, pad_mode="reflect"))
//   window      periodic Hann, w[j] = 0.5 - 0.5 cos(2 pi j / n_fft)
//   amplitude   A[f][b] = | sum_j x[p] w[j] e^(-2 pi i j b / n_fft) |, b = 0 .. n_fft / 2 (the amplitude, not the power)
//   filter bank HTK mel (mel(h) = 2595 log10(1 + h / 700)), no area normalisation, n_mels + 2 points equally spaced in mel
//               from fmin to fmax; W[m][b] = max(0, min(rising, falling)) at h_b = b fs / n_fft: evaluated in float64 on the
//               host, stored as fp32, one run of consecutive bins per filter
//   mel         M[f][m] = sum_b W[m][b] A[f][b] over the filter's run in ascending b (an fmaf chain: the order is fixed)
//   output      ln(max(M, floor)), or M itself with `linear`, at out[frame][mel] (time-major)
//
// The transform is the dense DFT of each windowed frame on the exact-fp32 matrix instruction (v_mfma_f32_16x16x4_f32), as
// in swn_spectral.hip, with the basis cos(2 pi m / n), m < n, indexed by (j * b) mod n; sin is the same table n / 4 entries
// earlier (its sign does not matter to the amplitude).  What differs: the hop is arbitrary, so a block keeps the LDS image
// of its tile as 16 separate windowed frames (pitch n + 2: the 16 rows x 2 k lanes of an operand read fall on 32 different
// banks whatever the hop is) with the window folded into the image when it is filled, and each frame folded once
// (y[j] +- y[j + n / 2] for the even / odd bins), which halves the product; one MFMA tile holds 16 frames of ONE
// signal; the block owns all n / 2 + 1 bins of its frames (wave w takes the runs of 32 bins w, w + 4, ...), writes
// their amplitudes to its own slice of the work buffer, and then applies the sparse triangular bank (weights in LDS), the
// floor and the log.  No floating-point atomics, no reduction across lanes: row i of an MFMA result depends on row i of
// the frame operand alone, the chain over j is the same in every row, and the mel chain runs over one frame's amplitudes,
// so a frame's result does not depend on the tile, the row of the tile, the entry or the call it is computed in.
//
// Entries (swn_logmel_entry, host memory, checked before the launch and carried in the kernel arguments): a window
// [t0, t0 + n_avail) onto each row's samples, the row's total length or -1 while unknown, and a frame range [f0, f1).
// The kernel reads no sample outside the window; the rows of a tile past f1 are zero.
//
// Pool (swn_logmel_pool, melspec.LogMelPool): every session keeps the tail of its signal in a window of its own on the
// device.  A call is two launches.  logmel_pool_update_kernel, one block per entry, moves the retained floats
// [n_drop, n_held) to the window's front (ascending blocks of 256 floats, each read whole before it is written: a block's
// destination lies below every later block's source) and appends the entry's new samples from the staged buffer.  Then
// logmel_kernel<true> computes the frames from the updated windows with the arithmetic of swn_logmel and writes them
// channel-major, out[m * out_stride + (f - f0)]: the layout the pool front end stages.  swn_logmel_pool_lowcut runs
// logmel_pool_update_kernel<true>: the staged samples are raw and reach the window through the stage-1 low cut
// (swn_lowcut.hpp, the bits of swn_lowcut_chunk), whose state - the slot's last n_taps - 1 raw samples - lives in hist_dev and
// is replaced by the same block.
//
// Mel-cepstrum (swn_mcep, melspec.MelCepstrumExtractor; restated in include/swn_hip.h and melspec.py).  Frames, padding,
// window and amplitude A[f][b] are those above.  Then
//   log amplitude  L[f][b] = ln(max(A[f][b], floor)), floor > 0: in double, rounded once to fp32 (as the log-mel output)
//   cepstrum       v = irfft(L) of length n_fft; one-sided c[0] = v[0], c[k] = 2 v[k] for 0 < k < n_fft / 2,
//                  c[n_fft / 2] = v[n_fft / 2], so that |exp(sum_k c(k) z^-k)| = A: the convention of dsp.py and the MLSA filter
//   mel-cepstrum   the frequency transform with all-pass constant alpha to order M (SPTK freqt): mc[f][0 .. M]
//   as a product   these steps are linear: mc[f] = G L[f] with G (M + 1, n_fft / 2 + 1), evaluated in float64 on the host
//                  (melspec.mcep_matrix), stored as fp32, its columns zero-padded to a multiple of 4
//   output         fp32 at out[frame][coefficient] (time-major); each coefficient is one chain over the bins in ascending
//                  order - the k order of the matrix instruction - so a frame's values do not depend on the tile, the row of
//                  the tile, the entry, the batch, the frame range or the window, as for the log-mel frames
// On the first n_fft / 2 + 1 cepstral coefficients this is what pysptk.sp2mc(A^2, M, alpha) computes (parity with pysptk is
// not pinned: the library is absent).  It is the cepstrum of the short-time spectrum, not of WORLD's cheaptrick envelope.
// The table of swn_mcep: cos, window, then G padded.  mcep_kernel below says how the block works.
#include <hip/hip_runtime.h>
#include "swn_frame_entry.hpp"
#include "swn_geom.hpp"
#include "swn_lowcut.hpp"
#include "swn_mma.hpp"
#include <cstdio>
#include <algorithm>
#include <vector>

namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_FR = 16;          // frames per tile = MFMA rows
constexpr int LM_MAX_LEN = FE_MAX_LEN;   // 2^30: 2 (len - 1) - p stays inside int

struct LmEntry {
    const float* wav;   // sample t0
    float* out;         // frame f0
    int t0, len, f0, f1, tile0;
    int stride;         // channel-major output only: floats between two filters' rows
};
struct LmArgs {
    LmEntry e[SWN_LOGMEL_MAX_ENTRIES];
    int bank[SWN_LOGMEL_MAX_MELS];      // first bin | bins << 16 of each filter's run
    unsigned short woff[SWN_LOGMEL_MAX_MELS];   // first weight of each run in the table
    int n_entries, n, hop, n_mels, linear;
    float floor_;
};
static_assert(sizeof(LmArgs) + 2 * sizeof(void*) <= 4096, "the by-value kernel arguments must stay inside 4 KB");

struct McArgs {
    LmEntry e[SWN_LOGMEL_MAX_ENTRIES];
    int n_entries, n, hop, order;
    float floor_;
};
static_assert(sizeof(McArgs) + 2 * sizeof(void*) <= 4096, "the by-value kernel arguments must stay inside 4 KB");

struct LpMove {
    int slot, n_held, n_drop, new_off, n_new;
};
struct LpArgs {
    LpMove e[SWN_LOGMEL_POOL_MAX_ENTRIES];
    int window_floats;
};
static_assert(sizeof(LpArgs) + 2 * sizeof(void*) <= 4096, "the by-value kernel arguments must stay inside 4 KB");
constexpr int LP_MAX_WINDOW = 1 << 24;      // floats per slot
static_assert(LM_THREADS == LC_THREADS, "the window update runs the low cut's tiles with its own block");
// swn_logmel_pool_lowcut only: the taps, the slots' histories of raw samples, and which entries have received nothing yet
struct LpFir {
    const double* taps;
    float* hist;
    int n_taps;
    unsigned long long fresh;               // bit e: entry e starts from zero history
};
static_assert(SWN_LOGMEL_POOL_MAX_ENTRIES <= 64, "one bit of LpFir::fresh per entry");
static_assert(SWN_LOGMEL_POOL_MAX_ENTRIES <= SWN_LOGMEL_MAX_ENTRIES, "a pool call's entries are one frame launch");

__host__ __device__ inline int lm_pitch(int n) { return n + 2; }
__host__ __device__ inline int lm_amp_pitch(int n) { return (n / 2 + 1 + 3) & ~3; }
__host__ __device__ inline size_t lm_lds_floats(int n) {
    // 16 frames, cos table, weights (at most two filters cover a bin), weight offsets and runs
    return (size_t)LM_FR * lm_pitch(n) + n + 2 * (n / 2 + 1) + 2 * SWN_LOGMEL_MAX_MELS;
}

// mel-cepstrum: the pitch of L (the bins rounded up to 4, plus 2: see mcep_kernel) and the block's LDS: the frame image, which
// L later overlays (16 (n / 2 + 6) <= 16 (n + 2) floats), and the cos table
__host__ __device__ inline int mc_l_pitch(int n) { return lm_amp_pitch(n) + 2; }
__host__ __device__ inline size_t mc_lds_floats(int n) { return (size_t)LM_FR * lm_pitch(n) + n; }

thread_local const char* lm_who = "swn_logmel";      // the entry point the checks below report for
struct LmWho {
    const char* before;
    explicit LmWho(const char* who) : before(lm_who) { lm_who = who; }
    ~LmWho() { lm_who = before; }
};

int lm_fail(const char* what) {
    swn_set_error_detail(lm_who, what);
    return SWN_E_BADARG;
}

bool lm_sizes_ok(int n_fft, int n_mels) {
    return n_fft >= 32 && n_fft <= SWN_SPECTRAL_MAX_FFT && n_fft % 32 == 0 && n_mels >= 1 && n_mels <= SWN_LOGMEL_MAX_MELS;
}

// the entry rules; *tiles receives the number of frame tiles of the call
int lm_check_entries(int n, int hop, const swn_logmel_entry* en, int n_entries, long long* tiles, bool need_pointers = true) {
    char msg[160];
    if (!en) return lm_fail("entries_host is NULL");
    if (n_entries < 1 || n_entries > SWN_LOGMEL_MAX_ENTRIES) return lm_fail("n_entries outside [1, SWN_LOGMEL_MAX_ENTRIES]");
    if (hop < 1 || hop > n) return lm_fail("hop outside [1, n_fft]");
    long long nt = 0;
    for (int i = 0; i < n_entries; ++i) {
        const swn_logmel_entry& e = en[i];
        const int rc = frame_entry_check(e, i, hop, n / 2 + 1, "n_fft / 2 < len", need_pointers, lm_fail);
        if (rc == FE_EMPTY) continue;
        if (rc != SWN_OK) return rc;
        // samples the range touches: frame f covers lo .. hi = f hop - n / 2 + (0 .. n - 1); the left reflection of a frame
        // with lo < 0 reaches sample -lo, the right reflection of hi >= len comes back down to 2 (len - 1) - hi
        const long long lo0 = (long long)e.f0 * hop - n / 2, hi1 = (long long)(e.f1 - 1) * hop - n / 2 + n - 1;
        long long mn = lo0 < 0 ? 0 : lo0, mx = hi1;
        if (lo0 < 0 && -lo0 > mx) mx = -lo0;
        if (e.len == -1) {
            if (mx >= (long long)e.t0 + e.n_avail) {
                snprintf(msg, sizeof msg, "entry %d: frames [%d, %d) need sample %lld, the window ends at %lld and the total "
                         "length is unknown (the reflected end needs it)", i, e.f0, e.f1, mx, (long long)e.t0 + e.n_avail);
                return lm_fail(msg);
            }
        } else {
            if (hi1 >= e.len) {
                const long long back = 2LL * (e.len - 1) - hi1;
                mn = back < mn ? back : mn;
            }
            if (mx > e.len - 1) mx = e.len - 1;
        }
        if (mn < e.t0 || mx >= (long long)e.t0 + e.n_avail) {
            snprintf(msg, sizeof msg, "entry %d: frames [%d, %d) read samples [%lld, %lld], the window holds [%d, %lld)", i, e.f0,
                     e.f1, mn, mx, e.t0, (long long)e.t0 + e.n_avail);
            return lm_fail(msg);
        }
        nt += (e.f1 - e.f0 + LM_FR - 1) / LM_FR;
    }
    if (nt > (1 << 24)) return lm_fail("more than 2^24 frame tiles in one call");
    *tiles = nt;
    return SWN_OK;
}

// the entry this block's tile belongs to; *fbase receives the first frame of the tile
template <class Args>
__device__ inline LmEntry lm_block_entry(const Args& a, int* fbase) {
    int ei = 0;
    for (int i = 1; i < a.n_entries; ++i)       // the last entry whose first tile is not past this block (empty ones share
        if (a.e[i].tile0 <= (int)blockIdx.x) ei = i;    // their tile0 with the next entry, which wins)
    const LmEntry e = a.e[ei];
    *fbase = e.f0 + ((int)blockIdx.x - e.tile0) * LM_FR;
    return e;
}

// The phase logmel_kernel and mcep_kernel share: the cos table into `tab`, the windowed and folded frames of the tile into
// `img`, a barrier, the DFT, and the amplitudes A[fr][b] to amp[fr * lm_amp_pitch(n) + b] (global memory).  The caller puts
// __threadfence_block() and a barrier between this and its reads of amp; from that barrier on img is dead.
__device__ __forceinline__ void lm_tile_amplitudes(int n, int hop, const LmEntry& e, int fbase, const float* __restrict__ tables,
                                                   float* img, float* tab, float* amp) {
    const int pitch = lm_pitch(n), bins = n / 2 + 1, ap = lm_amp_pitch(n);
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, kq = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < n; i += LM_THREADS) tab[i] = tables[i];
    const float* win = tables + n;

    // frame image, folded once: with y[j] = x[p(j)] w[j], X[b] = sum over j < n / 2 of (y[j] + (-1)^b y[j + n / 2]) e^(-2 pi i j b / n),
    // so row fr holds s[j] = y[j] + y[j + n / 2] (even bins) and then d[j] = y[j] - y[j + n / 2] (odd bins), n / 2 each, and
    // the product runs over half the frame.  2 x 2 independent loads in flight per thread
    const int half = n / 2, total = LM_FR * half;
    for (int e0 = tid; e0 < total; e0 += 2 * LM_THREADS) {
        float y0[2], y1[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int el = e0 + u * LM_THREADS;
            const int fr = el / half, j = el - fr * half, f = fbase + fr;
            const bool in = el < total && f < e.f1;
            int i0 = f * hop - half + j, i1 = i0 + half;
            i0 = i0 < 0 ? -i0 : i0;                         // i1 >= 0; the left reflection stays below len (len > n / 2)
            i0 = (e.len >= 0 && i0 >= e.len) ? 2 * (e.len - 1) - i0 : i0;
            i1 = (e.len >= 0 && i1 >= e.len) ? 2 * (e.len - 1) - i1 : i1;
            y0[u] = in ? e.wav[i0 - e.t0] * win[j] : 0.f;
            y1[u] = in ? e.wav[i1 - e.t0] * win[j + half] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int el = e0 + u * LM_THREADS;
            if (el < total) {
                const int fr = el / half, j = el - fr * half;
                img[fr * pitch + j] = y0[u] + y1[u];
                img[fr * pitch + half + j] = y0[u] - y1[u];
            }
        }
    }
    __syncthreads();

    // wave w: the runs of 32 bins w, w + 4, ... as a 16-bin tile of the even bins (operand s) and one of the odd bins
    // (operand d); a bin past the last one reads valid table entries and is dropped
    const int n_runs = (bins + 31) / 32, quarter = n / 4, steps = n / 8;
    const float* srow = img + c * pitch + kq;
    const float* drow = srow + half;
    for (int pp = w; pp < n_runs; pp += 4) {
        const int b0 = 32 * pp + 2 * c, b1 = b0 + 1;
        const int st0 = (4 * b0) % n, st1 = (4 * b1) % n;
        int i0 = (kq * b0) % n, i1 = (kq * b1) % n;
        swn_f32x4 acc[2][2] = {};                           // [even, odd][re, im]
        for (int it = 0; it < steps; it += 2) {             // two k steps per trip: 12 LDS reads ahead of 8 MFMAs
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float xs = srow[4 * (it + u)], xd = drow[4 * (it + u)];
                int s0 = i0 - quarter; s0 += s0 < 0 ? n : 0;
                int s1 = i1 - quarter; s1 += s1 < 0 ? n : 0;
                const float c0 = tab[i0], n0 = tab[s0], c1 = tab[i1], n1 = tab[s1];     // cos, sin: the sign of Im is not needed
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xs, c0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xs, n0, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xd, c1, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xd, n1, acc[1][1], 0, 0, 0);
                i0 += st0; i0 -= i0 >= n ? n : 0;
                i1 += st1; i1 -= i1 >= n ? n : 0;
            }
        }
        // accumulator element i of lane (c, kq): frame 4 kq + i of the tile, bin 32 pp + 2 c (+ 1)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt) {
            const int b = b0 + bt;
            if (b < bins) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float re = acc[bt][0][i], im = acc[bt][1][i];
                    amp[(4 * kq + i) * ap + b] = sqrtf(re * re + im * im);
                }
            }
        }
    }
}

// CM: the output is channel-major (swn_logmel_pool), else time-major (swn_logmel); nothing else differs
template <bool CM>
__global__ __launch_bounds__(LM_THREADS) void logmel_kernel(const LmArgs a, const float* __restrict__ tables, float* amp_work) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int n = a.n, pitch = lm_pitch(n), bins = n / 2 + 1, ap = lm_amp_pitch(n);
    float* img = sm;                            // [16 frames][pitch]: windowed and folded, s then d
    float* tab = img + LM_FR * pitch;           // cos(2 pi m / n)
    float* wts = tab + n;                       // the filters' runs of weights, back to back
    int* woff = reinterpret_cast<int*>(wts + 2 * bins);     // [n_mels] first weight of each run
    int* sbank = woff + SWN_LOGMEL_MAX_MELS;                // [n_mels] first bin | bins << 16
    const int tid = threadIdx.x;
    int fbase;
    const LmEntry e = lm_block_entry(a, &fbase);

    for (int m = tid; m < a.n_mels; m += LM_THREADS) {
        sbank[m] = a.bank[m];
        woff[m] = a.woff[m];
    }
    const float* wsrc = tables + 2 * n;
    for (int i = tid; i < 2 * bins; i += LM_THREADS) wts[i] = wsrc[i];      // the table holds 2 bins floats, zero past the runs
    float* amp = amp_work + (size_t)blockIdx.x * LM_FR * ap;
    lm_tile_amplitudes(n, a.hop, e, fbase, tables, img, tab, amp);
    __threadfence_block();
    __syncthreads();

    const int fr_n = e.f1 - fbase < LM_FR ? e.f1 - fbase : LM_FR;     // frames of this tile that exist (>= 1)
    for (int o = tid; o < fr_n * a.n_mels; o += LM_THREADS) {
        // channel-major: frames fastest, so that neighbouring lanes store neighbouring floats of a filter's row
        const int fr = CM ? o % fr_n : o / a.n_mels, m = CM ? o / fr_n : o - fr * a.n_mels;
        const int start = sbank[m] & 0xffff, cnt = sbank[m] >> 16;
        const float* ar = amp + fr * ap + start;
        const float* wr = wts + woff[m];
        float s = 0.f;
        for (int k = 0; k < cnt; ++k) s = fmaf(wr[k], ar[k], s);
        // the log in double, rounded once: logf lands up to 2 ulp from ln (measured at the floor), and a frame costs n_mels of these
        const float v = a.linear ? s : (float)log((double)fmaxf(s, a.floor_));
        if (CM) e.out[(size_t)m * e.stride + (fbase - e.f0 + fr)] = v;
        else e.out[(size_t)(fbase - e.f0 + fr) * a.n_mels + m] = v;
    }
}

// Mel-cepstrum (swn_mcep; the definition is at the top of the file): the shared phase, then L = ln max(A, floor) of the tile's
// 16 frames written over the dead frame image (pitch mc_l_pitch: with it a multiple of 4 plus 2, the 16 rows x 2 k lanes that
// one half-wave's ds_read_b32 covers fall on 32 different banks; the columns from n / 2 + 1 on and the rows from f1 on are
// zero), then mc = L G^T on v_mfma_f32_16x16x4_f32: the frames are the rows, K runs over the padded bins in ascending order,
// wave w takes the 16-coefficient column tiles w, w + 4, ...; G comes from global memory (at most 64 x 1 028 floats, every
// block reads the same ones).  Lane (c, kq) feeds L[c][4 s + kq] and G[16 t + c][4 s + kq] to step s and receives
// frames 4 kq .. 4 kq + 3 of coefficient 16 t + c.  Coefficients past `order` are computed on zeros and not stored.
__global__ __launch_bounds__(LM_THREADS) void mcep_kernel(const McArgs a, const float* __restrict__ tables, float* amp_work) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int n = a.n, bins = n / 2 + 1, ap = lm_amp_pitch(n), lp = mc_l_pitch(n), nc = a.order + 1;
    float* img = sm;                            // [16 frames][lm_pitch(n)], then L [16 frames][lp]
    float* tab = img + LM_FR * lm_pitch(n);     // cos(2 pi m / n)
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, kq = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int fbase;
    const LmEntry e = lm_block_entry(a, &fbase);
    float* amp = amp_work + (size_t)blockIdx.x * LM_FR * ap;
    lm_tile_amplitudes(n, a.hop, e, fbase, tables, img, tab, amp);
    __threadfence_block();
    __syncthreads();                            // the amplitudes are there and no wave reads the image any more

    const int fr_n = e.f1 - fbase < LM_FR ? e.f1 - fbase : LM_FR;     // frames of this tile that exist (>= 1)
    for (int o = tid; o < LM_FR * lp; o += LM_THREADS) {
        const int fr = o / lp, b = o - fr * lp;
        // the log in double, rounded once, as the log-mel output takes it
        img[o] = (fr < fr_n && b < bins) ? (float)log((double)fmaxf(amp[fr * ap + b], a.floor_)) : 0.f;
    }
    __syncthreads();

    const float* G = tables + 2 * n;            // [order + 1][ap], zero from column n / 2 + 1 on
    const float* lrow = img + c * lp + kq;
    const int steps = ap / 4, n_tiles = (nc + 15) / 16;
    for (int t = w; t < n_tiles; t += 4) {
        const int col = 16 * t + c;
        const bool live = col < nc;
        const float* grow = G + (size_t)(live ? col : 0) * ap + kq;
        swn_f32x4 acc = {};
        int s = 0;
        for (; s + 4 <= steps; s += 4) {        // four k steps per trip: the global loads ahead of the MFMAs
            float g[4], l[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                g[u] = live ? grow[4 * (s + u)] : 0.f;
                l[u] = lrow[4 * (s + u)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(l[u], g[u], acc, 0, 0, 0);
        }
        for (; s < steps; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(lrow[4 * s], live ? grow[4 * s] : 0.f, acc, 0, 0, 0);
        if (live) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int fr = 4 * kq + i;
                if (fr < fr_n) e.out[(size_t)(fbase - e.f0 + fr) * nc + col] = acc[i];
            }
        }
    }
}

// swn_logmel_pool_lowcut: the entry's n_new RAW samples through the low cut (swn_lowcut.hpp: the bits of swn_lowcut_chunk) to
// dst, tile after tile, and the slot's history of raw samples replaced.  Only the first tile reads the history (LC_TILE
// exceeds it); every thread has picked up its float of the new history before the barrier behind that tile's load, and
// writes it after it.
__device__ __forceinline__ void lp_filter_new(const LpFir& f, int slot, bool fresh, const float* __restrict__ src, int n_new,
                                              float* __restrict__ dst) {
    __shared__ LcShared s;
    const int H = f.n_taps - 1, tid = threadIdx.x;
    float* slot_hist = f.hist + (size_t)slot * H;
    const float* hist = fresh ? nullptr : slot_hist;
    lc_load_taps(s, f.taps, f.n_taps);
    const float next = tid < H ? lc_next_hist(src, n_new, hist, f.n_taps, tid) : 0.f;
    for (int base = 0; base < n_new; base += LC_TILE) {             // uniform trip count: every thread meets the barriers
        lc_load_tile(s, src, n_new, hist, f.n_taps, base);
        __syncthreads();
        if (base == 0 && tid < H) slot_hist[tid] = next;
        lc_fir_tile(s, f.n_taps, n_new - base < LC_TILE ? n_new - base : LC_TILE, dst + base);
        __syncthreads();                        // the next tile's load overwrites what this tile's chains read
    }
}

// one block per entry: window[0 .. n_held - n_drop) <- window[n_drop .. n_held), then the n_new staged samples after them -
// as they are (LC false: swn_logmel_pool) or through the low cut (LC true: swn_logmel_pool_lowcut)
template <bool LC>
__global__ __launch_bounds__(LM_THREADS) void logmel_pool_update_kernel(const LpArgs a, float* __restrict__ win,
                                                                         const float* __restrict__ staged, const LpFir f) {
    const LpMove e = a.e[blockIdx.x];
    float* w = win + (size_t)e.slot * a.window_floats;
    const int keep = e.n_held - e.n_drop, tid = threadIdx.x;
    if (e.n_drop > 0) {
        for (int base = 0; base < keep; base += LM_THREADS) {      // uniform trip count: every thread meets the barrier
            const int i = base + tid;
            const float v = i < keep ? w[i + e.n_drop] : 0.f;
            __syncthreads();                    // the block [base, base + 256) is read whole before any of it is written
            if (i < keep) w[i] = v;
        }
        __syncthreads();                        // the new samples may land on floats the last blocks still read
    }
    if constexpr (LC) {
        if (e.n_new > 0) lp_filter_new(f, e.slot, (f.fresh >> blockIdx.x) & 1ull, staged + e.new_off, e.n_new, w + keep);
    } else {
        for (int i = tid; i < e.n_new; i += LM_THREADS) w[keep + i] = staged[e.new_off + i];
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ C ABI
extern "C" size_t swn_logmel_table_floats(int n_fft, int n_mels) {
    if (!lm_sizes_ok(n_fft, n_mels)) return 0;
    return 2 * (size_t)n_fft + 2 * (size_t)(n_fft / 2 + 1);
}

extern "C" size_t swn_logmel_work_bytes(int n_fft, int hop, const swn_logmel_entry* entries_host, int n_entries) {
    long long tiles = 0;
    if (!lm_sizes_ok(n_fft, 1) || lm_check_entries(n_fft, hop, entries_host, n_entries, &tiles) != SWN_OK) return 0;
    return (size_t)tiles * LM_FR * lm_amp_pitch(n_fft) * sizeof(float);
}

namespace {

int lm_check_sizes(int n_fft, int n_mels, float floor, int linear) {
    if (n_fft < 32 || n_fft > SWN_SPECTRAL_MAX_FFT || n_fft % 32 != 0)
        return lm_fail("n_fft is not a multiple of 32 in [32, SWN_SPECTRAL_MAX_FFT]");
    if (n_mels < 1 || n_mels > SWN_LOGMEL_MAX_MELS) return lm_fail("n_mels outside [1, SWN_LOGMEL_MAX_MELS]");
    if (!(floor > 0.f) || !(floor < 3.0e38f)) return lm_fail("floor must be a finite number > 0");
    if (linear != 0 && linear != 1) return lm_fail("linear must be 0 or 1");
    return SWN_OK;
}

// the filters' runs into the launch arguments
int lm_fill_bank(LmArgs& a, int n_fft, int n_mels, const int32_t* bank_host) {
    if (!bank_host) return lm_fail("bank_host is NULL");
    const int bins = n_fft / 2 + 1;
    int nnz = 0;
    for (int m = 0; m < n_mels; ++m) {
        const int start = bank_host[m] & 0xffff, cnt = (int)((unsigned)bank_host[m] >> 16);
        if (bank_host[m] < 0 || cnt < 1 || start + cnt > bins) {
            char msg[96];
            snprintf(msg, sizeof msg, "filter %d: run of %d bins from bin %d, the transform has %d", m, cnt, start, bins);
            return lm_fail(msg);
        }
        a.woff[m] = (unsigned short)(nnz < 0xffff ? nnz : 0xffff);      // nnz <= 2 bins is checked below
        nnz += cnt;
        a.bank[m] = bank_host[m];
    }
    if (nnz > 2 * bins) return lm_fail("the filter runs hold more than 2 (n_fft / 2 + 1) weights");
    for (int m = n_mels; m < SWN_LOGMEL_MAX_MELS; ++m) a.bank[m] = a.woff[m] = 0;
    return SWN_OK;
}

// the entries into the launch arguments (stride: channel-major calls)
void lm_fill_entries(LmEntry* out, const swn_logmel_entry* en, const int* strides, int n_entries) {
    int t = 0;
    for (int i = 0; i < SWN_LOGMEL_MAX_ENTRIES; ++i) {
        LmEntry& o = out[i];
        if (i < n_entries) {
            const swn_logmel_entry& e = en[i];
            o.wav = e.wav_dev; o.out = e.out_dev; o.t0 = e.t0; o.len = e.len; o.f0 = e.f0; o.f1 = e.f1; o.tile0 = t;
            o.stride = strides ? strides[i] : 0;
            t += (e.f1 - e.f0 + LM_FR - 1) / LM_FR;
        } else {
            o.wav = nullptr; o.out = nullptr; o.t0 = o.len = o.f0 = o.f1 = o.stride = 0; o.tile0 = t;
        }
    }
}

// ... then the frame kernel
template <bool CM>
int lm_launch(LmArgs& a, int n_fft, int hop, int n_mels, float floor, int linear, const swn_logmel_entry* en, const int* strides,
              int n_entries, long long tiles, const float* tables_dev, float* work_dev, hipStream_t st, const char* who) {
    lm_fill_entries(a.e, en, strides, n_entries);
    a.n_entries = n_entries; a.n = n_fft; a.hop = hop; a.n_mels = n_mels; a.linear = linear; a.floor_ = floor;
    const size_t lds = lm_lds_floats(n_fft) * sizeof(float);
    // dynamic LDS from 64 KB on: set on every call (the attribute is per device)
    if (lds >= 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(logmel_kernel<CM>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return swn_launch_status(CM ? "swn_logmel_pool (LDS size)" : "swn_logmel (LDS size)");
    hipLaunchKernelGGL(logmel_kernel<CM>, dim3((unsigned)tiles), dim3(LM_THREADS), lds, st, a, tables_dev, work_dev);
    return swn_launch_status(who);
}

}  // namespace

extern "C" int swn_logmel(int n_fft, int hop, int n_mels, float floor, int linear, const float* tables_dev,
                          const int32_t* bank_host, const swn_logmel_entry* entries_host, int n_entries, float* work_dev,
                          void* stream) {
    int rc = lm_check_sizes(n_fft, n_mels, floor, linear);
    if (rc != SWN_OK) return rc;
    long long tiles = 0;
    rc = lm_check_entries(n_fft, hop, entries_host, n_entries, &tiles);
    if (rc != SWN_OK) return rc;
    LmArgs a;
    rc = lm_fill_bank(a, n_fft, n_mels, bank_host);
    if (rc != SWN_OK) return rc;
    if (tiles == 0) return SWN_OK;                          // no frame in any entry
    if (!tables_dev || !work_dev) return lm_fail("null pointer");
    (void)hipGetLastError();
    return lm_launch<false>(a, n_fft, hop, n_mels, floor, linear, entries_host, nullptr, n_entries, tiles, tables_dev, work_dev,
                            static_cast<hipStream_t>(stream), "swn_logmel");
}

// ---------------------------------------------------------------------------------------------------------- mel-cepstrum
namespace {

bool mc_sizes_ok(int n_fft, int order) {
    return lm_sizes_ok(n_fft, 1) && order >= 0 && order <= SWN_MCEP_MAX_ORDER && order <= n_fft / 2;
}

}  // namespace

extern "C" size_t swn_mcep_table_floats(int n_fft, int order) {
    if (!mc_sizes_ok(n_fft, order)) return 0;
    return 2 * (size_t)n_fft + (size_t)(order + 1) * lm_amp_pitch(n_fft);
}

extern "C" size_t swn_mcep_work_bytes(int n_fft, int hop, const swn_logmel_entry* entries_host, int n_entries) {
    LmWho who("swn_mcep_work_bytes");
    long long tiles = 0;
    if (!lm_sizes_ok(n_fft, 1) || lm_check_entries(n_fft, hop, entries_host, n_entries, &tiles) != SWN_OK) return 0;
    return (size_t)tiles * LM_FR * lm_amp_pitch(n_fft) * sizeof(float);
}

extern "C" int swn_mcep(int n_fft, int hop, int order, float floor, const float* tables_dev, const swn_logmel_entry* entries_host,
                        int n_entries, float* work_dev, void* stream) {
    LmWho who("swn_mcep");
    if (!lm_sizes_ok(n_fft, 1)) return lm_fail("n_fft is not a multiple of 32 in [32, SWN_SPECTRAL_MAX_FFT]");
    if (order < 0 || order > SWN_MCEP_MAX_ORDER) return lm_fail("order outside [0, SWN_MCEP_MAX_ORDER]");
    if (order > n_fft / 2) return lm_fail("order exceeds n_fft / 2: the one-sided cepstrum has n_fft / 2 + 1 coefficients");
    if (!(floor > 0.f) || !(floor < 3.0e38f)) return lm_fail("floor must be a finite number > 0");
    long long tiles = 0;
    const int rc = lm_check_entries(n_fft, hop, entries_host, n_entries, &tiles);
    if (rc != SWN_OK) return rc;
    if (tiles == 0) return SWN_OK;                          // no frame in any entry
    if (!tables_dev || !work_dev) return lm_fail("null pointer");
    McArgs a;
    lm_fill_entries(a.e, entries_host, nullptr, n_entries);
    a.n_entries = n_entries; a.n = n_fft; a.hop = hop; a.order = order; a.floor_ = floor;
    const size_t lds = mc_lds_floats(n_fft) * sizeof(float);
    (void)hipGetLastError();
    // dynamic LDS from 64 KB on: set on every call (the attribute is per device)
    if (lds >= 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(mcep_kernel),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return swn_launch_status("swn_mcep (LDS size)");
    hipLaunchKernelGGL(mcep_kernel, dim3((unsigned)tiles), dim3(LM_THREADS), lds, static_cast<hipStream_t>(stream), a, tables_dev,
                       work_dev);
    return swn_launch_status("swn_mcep");
}

// ------------------------------------------------------------------------------------------------------------------ pool
namespace {

// every rule of a pool call that needs no device pointer; rows[i] receives entry i as the frame kernel takes it (the window
// after the update, pointers left null) and *tiles the frame tiles of the call
int lp_check(int n_fft, int hop, int n_mels, size_t window_floats, const swn_logmel_pool_entry* en, int n_entries,
             swn_logmel_entry* rows, long long* tiles) {
    char msg[200];
    if (!en) return lm_fail("entries_host is NULL");
    if (n_entries < 1 || n_entries > SWN_LOGMEL_POOL_MAX_ENTRIES)
        return lm_fail("n_entries outside [1, SWN_LOGMEL_POOL_MAX_ENTRIES]");
    if (window_floats < 1 || window_floats > (size_t)LP_MAX_WINDOW) return lm_fail("window_floats outside [1, 2^24]");
    for (int i = 0; i < n_entries; ++i) {
        const swn_logmel_pool_entry& e = en[i];
        if (e.reserved != 0) { snprintf(msg, sizeof msg, "entry %d: reserved field is not 0", i); return lm_fail(msg); }
        if (e.slot < 0) { snprintf(msg, sizeof msg, "entry %d: slot %d", i, e.slot); return lm_fail(msg); }
        for (int j = 0; j < i; ++j)
            if (en[j].slot == e.slot) {
                snprintf(msg, sizeof msg, "entries %d and %d name slot %d: a slot takes one entry per call", j, i, e.slot);
                return lm_fail(msg);
            }
        if (e.t0 < 0 || e.n_held < 0 || e.n_drop < 0 || e.new_off < 0 || e.n_new < 0 || e.out_off < 0 || e.out_stride < 0) {
            snprintf(msg, sizeof msg, "entry %d: a negative count or offset (t0 %d, n_held %d, n_drop %d, new_off %d, n_new %d, "
                     "out_off %d, out_stride %d)", i, e.t0, e.n_held, e.n_drop, e.new_off, e.n_new, e.out_off, e.out_stride);
            return lm_fail(msg);
        }
        if (e.n_drop > e.n_held) {
            snprintf(msg, sizeof msg, "entry %d: n_drop %d exceeds the %d samples held", i, e.n_drop, e.n_held);
            return lm_fail(msg);
        }
        const long long after = (long long)e.n_held - e.n_drop + e.n_new;
        if ((size_t)e.n_held > window_floats || (size_t)after > window_floats) {
            snprintf(msg, sizeof msg, "entry %d: %d held - %d dropped + %d new samples do not fit the window of %zu floats", i,
                     e.n_held, e.n_drop, e.n_new, window_floats);
            return lm_fail(msg);
        }
        if ((long long)e.new_off + e.n_new > (1LL << 30)) {
            snprintf(msg, sizeof msg, "entry %d: new_off + n_new beyond 2^30", i);
            return lm_fail(msg);
        }
        if ((long long)e.t0 + e.n_drop > LM_MAX_LEN) { snprintf(msg, sizeof msg, "entry %d: t0 + n_drop beyond 2^30", i); return lm_fail(msg); }
        swn_logmel_entry& r = rows[i];
        r.wav_dev = nullptr; r.out_dev = nullptr; r.len = e.len; r.f0 = e.f0; r.f1 = e.f1; r.reserved = 0;
        r.t0 = e.t0 + e.n_drop;
        r.n_avail = (int32_t)after;
    }
    const int rc = lm_check_entries(n_fft, hop, rows, n_entries, tiles, false);
    if (rc != SWN_OK) return rc;
    // the filters' rows of all entries, sorted by their first float: neighbours must not overlap
    struct Row { long long begin, end; int entry; };
    std::vector<Row> span;
    span.reserve((size_t)n_entries * n_mels);
    for (int i = 0; i < n_entries; ++i) {
        const int nf = en[i].f1 - en[i].f0;
        if (nf == 0) continue;
        if ((long long)en[i].out_off + (long long)(n_mels - 1) * en[i].out_stride + nf > (1LL << 31) - 1) {
            snprintf(msg, sizeof msg, "entry %d: the output range ends beyond 2^31 floats", i);
            return lm_fail(msg);
        }
        for (int m = 0; m < n_mels; ++m) {
            const long long begin = (long long)en[i].out_off + (long long)m * en[i].out_stride;
            span.push_back(Row{begin, begin + nf, i});
        }
    }
    std::sort(span.begin(), span.end(), [](const Row& x, const Row& y) { return x.begin < y.begin; });
    for (size_t k = 1; k < span.size(); ++k)
        if (span[k].begin < span[k - 1].end) {
            snprintf(msg, sizeof msg, "the output ranges of entries %d and %d overlap at float %lld (out_off, out_stride and "
                     "the frame counts)", span[k - 1].entry, span[k].entry, span[k].begin);
            return lm_fail(msg);
        }
    return SWN_OK;
}

}  // namespace

extern "C" size_t swn_logmel_pool_window_floats(int n_fft, int max_chunk) {
    if (!lm_sizes_ok(n_fft, 1) || max_chunk < 1 || (long long)n_fft + max_chunk > LP_MAX_WINDOW) return 0;
    return (size_t)n_fft + (size_t)max_chunk;       // one window: what a session holds between calls plus one chunk
}

extern "C" size_t swn_logmel_pool_work_bytes(int n_fft, int hop, int n_mels, size_t window_floats,
                                             const swn_logmel_pool_entry* entries_host, int n_entries) {
    LmWho who("swn_logmel_pool_work_bytes");
    swn_logmel_entry rows[SWN_LOGMEL_POOL_MAX_ENTRIES];
    long long tiles = 0;
    if (!lm_sizes_ok(n_fft, n_mels) || lp_check(n_fft, hop, n_mels, window_floats, entries_host, n_entries, rows, &tiles) != SWN_OK)
        return 0;
    return (size_t)tiles * LM_FR * lm_amp_pitch(n_fft) * sizeof(float);
}

namespace {

// swn_logmel_pool (fir null) and swn_logmel_pool_lowcut
int lp_run(int n_fft, int hop, int n_mels, float floor, int linear, const float* tables_dev, const int32_t* bank_host,
           float* win_dev, size_t window_floats, const float* new_dev, float* out_dev, const swn_logmel_pool_entry* entries_host,
           int n_entries, float* work_dev, const LpFir* fir, void* stream) {
    int rc = lm_check_sizes(n_fft, n_mels, floor, linear);
    if (rc != SWN_OK) return rc;
    if (fir) {
        if (!lc_taps_ok(fir->n_taps)) return lm_fail("n_taps outside [1, SWN_LOWCUT_MAX_TAPS]");
        if (!fir->taps || !fir->hist) return lm_fail("null pointer (taps_dev, hist_dev)");
    }
    swn_logmel_entry rows[SWN_LOGMEL_POOL_MAX_ENTRIES];
    long long tiles = 0;
    rc = lp_check(n_fft, hop, n_mels, window_floats, entries_host, n_entries, rows, &tiles);
    if (rc != SWN_OK) return rc;
    LmArgs a;
    rc = lm_fill_bank(a, n_fft, n_mels, bank_host);
    if (rc != SWN_OK) return rc;
    LpArgs u;
    LpFir f = fir ? *fir : LpFir{nullptr, nullptr, 0, 0ull};
    int strides[SWN_LOGMEL_POOL_MAX_ENTRIES];
    bool moves = false, news = false;
    for (int i = 0; i < SWN_LOGMEL_POOL_MAX_ENTRIES; ++i) {
        const bool in = i < n_entries;
        const swn_logmel_pool_entry* e = in ? entries_host + i : nullptr;
        u.e[i] = in ? LpMove{e->slot, e->n_held, e->n_drop, e->new_off, e->n_new} : LpMove{0, 0, 0, 0, 0};
        strides[i] = in ? e->out_stride : 0;
        if (in) {
            moves = moves || e->n_new > 0 || (e->n_drop > 0 && e->n_held > e->n_drop);
            news = news || e->n_new > 0;
            if (e->t0 == 0 && e->n_held == 0) f.fresh |= 1ull << i;     // nothing received yet: zero history
        }
    }
    u.window_floats = (int)window_floats;
    if (!win_dev || (news && !new_dev) || (tiles > 0 && (!tables_dev || !work_dev || !out_dev))) return lm_fail("null pointer");
    for (int i = 0; i < n_entries; ++i) {
        rows[i].wav_dev = win_dev + (size_t)entries_host[i].slot * window_floats;
        rows[i].out_dev = out_dev ? out_dev + entries_host[i].out_off : nullptr;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (moves) {
        if (fir)
            hipLaunchKernelGGL(logmel_pool_update_kernel<true>, dim3((unsigned)n_entries), dim3(LM_THREADS), 0, st, u, win_dev,
                               new_dev, f);
        else
            hipLaunchKernelGGL(logmel_pool_update_kernel<false>, dim3((unsigned)n_entries), dim3(LM_THREADS), 0, st, u, win_dev,
                               new_dev, f);
        rc = swn_launch_status(fir ? "swn_logmel_pool_lowcut (window update)" : "swn_logmel_pool (window update)");
        if (rc != SWN_OK) return rc;
    }
    if (tiles == 0) return SWN_OK;                          // no frame in any entry
    return lm_launch<true>(a, n_fft, hop, n_mels, floor, linear, rows, strides, n_entries, tiles, tables_dev, work_dev, st,
                           fir ? "swn_logmel_pool_lowcut" : "swn_logmel_pool");
}

}  // namespace

extern "C" int swn_logmel_pool(int n_fft, int hop, int n_mels, float floor, int linear, const float* tables_dev,
                               const int32_t* bank_host, float* win_dev, size_t window_floats, const float* new_dev,
                               float* out_dev, const swn_logmel_pool_entry* entries_host, int n_entries, float* work_dev,
                               void* stream) {
    LmWho who("swn_logmel_pool");
    return lp_run(n_fft, hop, n_mels, floor, linear, tables_dev, bank_host, win_dev, window_floats, new_dev, out_dev, entries_host,
                  n_entries, work_dev, nullptr, stream);
}

extern "C" int swn_logmel_pool_lowcut(int n_fft, int hop, int n_mels, float floor, int linear, const float* tables_dev,
                                      const int32_t* bank_host, float* win_dev, size_t window_floats, const float* new_dev,
                                      float* out_dev, const swn_logmel_pool_entry* entries_host, int n_entries, float* work_dev,
                                      int n_taps, const double* taps_dev, float* hist_dev, void* stream) {
    LmWho who("swn_logmel_pool_lowcut");
    const LpFir fir{taps_dev, hist_dev, n_taps, 0ull};
    return lp_run(n_fft, hop, n_mels, floor, linear, tables_dev, bank_host, win_dev, window_floats, new_dev, out_dev, entries_host,
                  n_entries, work_dev, &fir, stream);
}
