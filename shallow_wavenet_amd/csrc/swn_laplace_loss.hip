// Laplace chunk loss of the CSWNV recipe (train_driver.batch_loss between the stack and the spectral terms): from the raw
// output of the stack (B, NO = 2 seg + lpc, tp) to the per-segment NLL, the reparameterised sample rows, the target rows,
// the sample error and the seven figures of the LaplaceLoss log line - and back to d loss / d raw.
//
// Per (b, segment j < seg, position t in [skip, tp)), fp32:
//      mu       = raw[j][t] + sum_k raw[2 seg + lpc-1-k][t] * ctx[j + t + k]          (the flip of `a` folded into the index)
//      lb       = logsigmoid(raw[seg + j][t]), b_noclip = exp(lb), lc = max(lb, FLOOR), b = exp(lc)     (laplace_head_kernel)
//      nll term = ln 2 + lc + |target[t + j] - mu| / b
//      sample   = mu - b_noclip * sign(eps) * log1p(-2 |eps|)
// One thread per (b, t), 256 per block.  The 2 seg + 7 running values of a block (per segment the NLL and error sums, for
// segment 0 the sum / sum of squares / min / max of mu and the sum / min / max of 2 b^2) are reduced in float64: inside the
// wave with shuffles, across the four waves through LDS in wave order, and written as one partial row per block; the finish
// kernel adds the rows in block order.  No floating-point atomics: same input, same bits.
//
// The backward recomputes the head values from raw (no state buffer) and is purely element-wise: `a` is a per-position
// output, so d a_k[t] = sum_j d mu_j[t] * ctx[j + t + lpc-1-k] needs no reduction over time.
#include <hip/hip_runtime.h>
#include "swn_geom.hpp"

namespace {

constexpr int LL_THREADS = 256;
constexpr int LL_WAVES = LL_THREADS / 64;
constexpr int LL_MAXLPC = 16;                 // swn_make_geom's bound
constexpr int LL_MAXSEG = 10;
constexpr int LL_MAXV = 2 * LL_MAXSEG + 7;
constexpr float LL_FLOOR = -14.162084148244246758816564788835f;
constexpr float LL_LN2 = 0.69314718055994530941723212145818f;

// partial row of a block, NV = 2 seg + 7 doubles: [0, seg) NLL sums, [seg, 2 seg) error sums, then for segment 0
// sum mu, sum mu^2, sum 2b^2 (added) and -min mu, max mu, -min 2b^2, max 2b^2 (joined with max)
__host__ __device__ inline int ll_nv(int seg) { return 2 * seg + 7; }
__host__ __device__ inline int ll_blocks(int tp) { return (tp + LL_THREADS - 1) / LL_THREADS; }

__device__ inline double wave_add(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ inline double wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ inline float ll_logsigmoid(float y) { return fminf(y, 0.f) - log1pf(expf(-fabsf(y))); }
__device__ inline float ll_sign(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// mu of segment j at position t: a[k] = raw[2 seg + lpc-1-k][t]
__device__ inline float ll_mu(float m0, const float (&a)[LL_MAXLPC], const float* __restrict__ cx, int lpc) {
    float mu = m0;
#pragma unroll
    for (int k = 0; k < LL_MAXLPC; ++k)
        if (k < lpc) mu = fmaf(a[k], cx[k], mu);
    return mu;
}

__global__ __launch_bounds__(LL_THREADS) void laplace_loss_fwd_kernel(
    const float* __restrict__ raw, const float* __restrict__ ctx, const float* __restrict__ target,
    const float* __restrict__ eps, int tp, int skip, int seg, int lpc, float* __restrict__ samples,
    float* __restrict__ targets, double* __restrict__ part) {
    __shared__ double red[LL_WAVES][LL_MAXV];
    const int t = blockIdx.x * LL_THREADS + threadIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int NO = 2 * seg + lpc, N = tp - skip;
    const bool on = t >= skip && t < tp;
    const float* r = raw + (size_t)b * NO * tp + t;
    float a[LL_MAXLPC];
#pragma unroll
    for (int k = 0; k < LL_MAXLPC; ++k) a[k] = (on && k < lpc) ? r[(size_t)(2 * seg + lpc - 1 - k) * tp] : 0.f;
    const float* tg = target + (size_t)b * (tp + seg - 1) + t;
    const float* cx = lpc > 0 ? ctx + (size_t)b * (tp + seg + lpc - 1) + t : tg;      // never read when lpc == 0
    for (int j = 0; j < seg; ++j) {
        double v_nll = 0.0, v_err = 0.0;
        float mu = 0.f, var = 0.f;
        if (on) {
            mu = ll_mu(r[(size_t)j * tp], a, cx + j, lpc);
            const float lb = ll_logsigmoid(r[(size_t)(seg + j) * tp]);
            const float bn = expf(lb), lc = fmaxf(lb, LL_FLOOR), bc = expf(lc);
            const float trg = tg[j];
            const size_t o = ((size_t)b * seg + j) * N + (t - skip);
            const float e = eps[o];
            const float smp = mu - bn * ll_sign(e) * log1pf(-2.f * fabsf(e));
            samples[o] = smp;
            targets[o] = trg;
            v_nll = (double)(LL_LN2 + lc + fabsf(trg - mu) / bc);
            v_err = (double)fabsf(smp - trg);
            var = 2.f * (bc * bc);
        }
        v_nll = wave_add(v_nll);
        v_err = wave_add(v_err);
        if (lane == 0) { red[wv][j] = v_nll; red[wv][seg + j] = v_err; }
        if (j == 0) {                                              // the log line's figures: segment 0 only
            const double inf = __builtin_huge_val();
            const double dm = (double)mu, dv = (double)var;
            const double s1 = wave_add(on ? dm : 0.0), s2 = wave_add(on ? dm * dm : 0.0), s3 = wave_add(on ? dv : 0.0);
            const double n1 = wave_max(on ? -dm : -inf), x1 = wave_max(on ? dm : -inf);
            const double n2 = wave_max(on ? -dv : -inf), x2 = wave_max(on ? dv : -inf);
            if (lane == 0) {
                double* q = &red[wv][2 * seg];
                q[0] = s1; q[1] = s2; q[2] = s3; q[3] = n1; q[4] = x1; q[5] = n2; q[6] = x2;
            }
        }
    }
    __syncthreads();
    const int NV = ll_nv(seg), i = threadIdx.x;
    if (i < NV) {
        double v = red[0][i];
        if (i < 2 * seg + 3) for (int w = 1; w < LL_WAVES; ++w) v += red[w][i];
        else for (int w = 1; w < LL_WAVES; ++w) v = fmax(v, red[w][i]);
        part[((size_t)b * gridDim.x + blockIdx.x) * NV + i] = v;
    }
}

// one block: a thread per output adds the block partials in block order
__global__ __launch_bounds__(LL_THREADS) void laplace_loss_finish_kernel(const double* __restrict__ part, int B, int nblk,
                                                                         int seg, int N, float* __restrict__ nll,
                                                                         float* __restrict__ err, float* __restrict__ stats) {
    __shared__ double fin[7];
    const int NV = ll_nv(seg);
    for (int i = threadIdx.x; i < 2 * B * seg; i += LL_THREADS) {          // i = (b * 2 + which) * seg + j
        const int j = i % seg, which = (i / seg) & 1, b = i / (2 * seg);
        double s = 0.0;
        for (int k = 0; k < nblk; ++k) s += part[((size_t)b * nblk + k) * NV + which * seg + j];
        (which ? err : nll)[b * seg + j] = (float)(s / (double)N);
    }
    if (threadIdx.x < 7) {
        const int q = threadIdx.x, c = 2 * seg + q;
        double v = q < 3 ? 0.0 : -__builtin_huge_val();
        for (int k = 0; k < B * nblk; ++k) {
            const double p = part[(size_t)k * NV + c];
            v = q < 3 ? v + p : fmax(v, p);
        }
        fin[q] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = (double)B * (double)N, mean = fin[0] / n;
        stats[0] = (float)-fin[3];
        stats[1] = (float)mean;
        stats[2] = (float)fin[4];
        stats[3] = (float)((fin[1] - fin[0] * mean) / (n - 1.0));          // unbiased, nan for one value like torch.var
        stats[4] = (float)-fin[5];
        stats[5] = (float)(fin[2] / n);
        stats[6] = (float)fin[6];
    }
}

// d loss / d raw for upstream g_nll (B, seg) and g_samples (B seg, N) or NULL; zeros at the positions below skip
__global__ __launch_bounds__(LL_THREADS) void laplace_loss_bwd_kernel(
    const float* __restrict__ raw, const float* __restrict__ ctx, const float* __restrict__ target,
    const float* __restrict__ eps, int tp, int skip, int seg, int lpc, const float* __restrict__ g_nll,
    const float* __restrict__ g_samples, float* __restrict__ graw) {
    const int t = blockIdx.x * LL_THREADS + threadIdx.x, b = blockIdx.y;
    if (t >= tp) return;
    const int NO = 2 * seg + lpc, N = tp - skip;
    float* g = graw + (size_t)b * NO * tp + t;
    if (t < skip) {
        for (int c = 0; c < NO; ++c) g[(size_t)c * tp] = 0.f;
        return;
    }
    const float* r = raw + (size_t)b * NO * tp + t;
    float a[LL_MAXLPC], da[LL_MAXLPC];
#pragma unroll
    for (int k = 0; k < LL_MAXLPC; ++k) {
        a[k] = k < lpc ? r[(size_t)(2 * seg + lpc - 1 - k) * tp] : 0.f;
        da[k] = 0.f;
    }
    const float* tg = target + (size_t)b * (tp + seg - 1) + t;
    const float* cx = lpc > 0 ? ctx + (size_t)b * (tp + seg + lpc - 1) + t : tg;      // never read when lpc == 0
    for (int j = 0; j < seg; ++j) {
        const float mu = ll_mu(r[(size_t)j * tp], a, cx + j, lpc);
        const float y = r[(size_t)(seg + j) * tp];
        const float lb = ll_logsigmoid(y);
        const float bn = expf(lb), bc = expf(fmaxf(lb, LL_FLOOR));
        const float d = tg[j] - mu;
        const size_t o = ((size_t)b * seg + j) * N + (t - skip);
        const float w = g_nll[b * seg + j] / (float)N;
        const float gs = g_samples ? g_samples[o] : 0.f;
        const float e = eps[o];
        const float dmu = -ll_sign(d) * w / bc + gs;
        float dlb = -gs * ll_sign(e) * log1pf(-2.f * fabsf(e)) * bn;              // through b_noclip = exp(lb)
        if (lb >= LL_FLOOR) dlb += w * (1.f - fabsf(d) / bc);                     // through lc: torch's clamp
        g[(size_t)j * tp] = dmu;
        g[(size_t)(seg + j) * tp] = dlb / (1.f + expf(y));                        // d logsigmoid / dy = 1 - sigmoid(y)
#pragma unroll
        for (int k = 0; k < LL_MAXLPC; ++k)
            if (k < lpc) da[k] = fmaf(dmu, cx[j + k], da[k]);
    }
#pragma unroll
    for (int k = 0; k < LL_MAXLPC; ++k)
        if (k < lpc) g[(size_t)(2 * seg + lpc - 1 - k) * tp] = da[k];
}

int ll_check(const swn_net_desc* d, int batch, int tp, int skip) {
    if (!d || d->kind != SWN_KIND_LAPLACE) return SWN_E_BADARG;
    if (d->seg < 1 || d->seg > LL_MAXSEG || d->lpc < 0 || d->lpc > LL_MAXLPC) return SWN_E_BADDESC;
    if (batch < 1 || batch > 65535 || tp < 1 || skip < 0 || tp - skip < 1) return SWN_E_BADARG;
    return SWN_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ C ABI
extern "C" size_t swn_laplace_loss_work_bytes(const swn_net_desc* d, int batch, int tp, int skip) {
    if (ll_check(d, batch, tp, skip) != SWN_OK) return 0;
    return sizeof(double) * (size_t)batch * ll_blocks(tp) * ll_nv(d->seg);
}

extern "C" int swn_laplace_loss_forward(const swn_net_desc* d, const float* raw_dev, const float* ctx_dev,
                                        const float* target_dev, const float* eps_dev, int batch, int tp, int skip,
                                        float* nll_dev, float* err_dev, float* samples_dev, float* targets_dev,
                                        float* stats_dev, void* work_dev, void* stream) {
    const int rc = ll_check(d, batch, tp, skip);
    if (rc != SWN_OK) return rc;
    if (!raw_dev || !target_dev || !eps_dev || !nll_dev || !err_dev || !samples_dev || !targets_dev || !stats_dev ||
        !work_dev || (d->lpc > 0 && !ctx_dev))
        return SWN_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    double* part = static_cast<double*>(work_dev);
    const int nblk = ll_blocks(tp);
    hipLaunchKernelGGL(laplace_loss_fwd_kernel, dim3(nblk, batch), dim3(LL_THREADS), 0, st, raw_dev, ctx_dev, target_dev,
                       eps_dev, tp, skip, d->seg, d->lpc, samples_dev, targets_dev, part);
    const int lrc = swn_launch_status("swn_laplace_loss_forward");
    if (lrc != SWN_OK) return lrc;
    hipLaunchKernelGGL(laplace_loss_finish_kernel, dim3(1), dim3(LL_THREADS), 0, st, part, batch, nblk, d->seg, tp - skip,
                       nll_dev, err_dev, stats_dev);
    return swn_launch_status("swn_laplace_loss_forward (finish)");
}

extern "C" int swn_laplace_loss_backward(const swn_net_desc* d, const float* raw_dev, const float* ctx_dev,
                                         const float* target_dev, const float* eps_dev, int batch, int tp, int skip,
                                         const float* g_nll_dev, const float* g_samples_dev, float* graw_dev, void* stream) {
    const int rc = ll_check(d, batch, tp, skip);
    if (rc != SWN_OK) return rc;
    if (!raw_dev || !target_dev || !eps_dev || !g_nll_dev || !graw_dev || (d->lpc > 0 && !ctx_dev)) return SWN_E_BADARG;
    (void)hipGetLastError();
    hipLaunchKernelGGL(laplace_loss_bwd_kernel, dim3(ll_blocks(tp), batch), dim3(LL_THREADS), 0,
                       static_cast<hipStream_t>(stream), raw_dev, ctx_dev, target_dev, eps_dev, tp, skip, d->seg, d->lpc,
                       g_nll_dev, g_samples_dev, graw_dev);
    return swn_launch_status("swn_laplace_loss_backward");
}
