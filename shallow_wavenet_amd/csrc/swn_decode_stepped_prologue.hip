// A new session's prologue of the stepped decode in parallel launches (swn_decode_stepped_prologue, include/swn_hip.h).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "swn_decode_internal.hpp"
#include "swn_decode_stepped_common.hpp"

// ---- parallel prologue (swn_decode_stepped_prologue) -----------------------------------------------------------------
// Nothing in the prologue is autoregressive: the input sample of every prologue position is the constant 0 (softmax: class
// Q/2), its conditioning is frame 0 at upsampler phase 0 (tt = q + s - rf clamps to 0), the rings start from zeros, and level
// l + 1 at position q reads level l at q - k dil_l only.  So the n_pro positions of a level are independent, and the prologue
// is L + 2 launches (setup, input level, L layers) instead of n_pro x (L + 1).  The launches below form, for every position,
// the sums the stepped chain forms - lane `lane` owns elements pc 256 + 4 lane .. + 3 of the tap-major row, sequential fmafs
// over pc, then the sum64 pairings (sum64x8) - and the epilogue of step_layer_kernel with the same expressions, so every
// float they leave in the state block is the one the stepped prologue leaves.  The levels live in the caller's scratch
// (two ping-pong buffers [entry][q][Hp]); what the stepped run would still hold afterwards also goes to the state block: the
// last ring_len positions of each ring and hcat of position n_pro - 1.
namespace {

struct StProEnt {
    const float* cond; const float* P;         // the entry's cond rows and the packed parameters of its model
    int Tf, slot;
};
struct StProArgs : StArgs {                    // B = entries; seed rows are indexed by entry
    float* work;                               // [2][B][n_pro][Hp]
    int n_grp, gpw;                            // groups of ST_TU positions of an entry; groups per workgroup
    StProEnt e[SWN_DECODE_POOL_MAX_ENTRIES];
};
static_assert(sizeof(StProArgs) <= 4096, "the prologue kernels' arguments fit 4 KB");

// zero every named slot and seed its sample window: step_pool_setup_kernel without the table.  Grid (zero blocks, entries).
__global__ __launch_bounds__(256) void pro_setup_kernel(const StProArgs a) {
    const int k = blockIdx.y, tid = threadIdx.x;
    float* blk = a.state + (size_t)a.e[k].slot * a.stride;
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
                    const int sc = a.seed ? reinterpret_cast<const int*>(a.seed)[k] : a.g.Q / 2;
                    x = __builtin_bit_cast(float, (kk == WN - 1) ? sc : a.g.Q / 2);
                } else if (a.seed && kk >= WN - seg) {
                    x = reinterpret_cast<const float*>(a.seed)[(size_t)k * seg + (kk - (WN - seg))];
                }
            }
            q[c] = x;
        }
        reinterpret_cast<float4*>(blk)[v] = make_float4(q[0], q[1], q[2], q[3]);
    }
}

// input level: input_layer's prologue branch (same expression, same tap order, same masks) for all positions of entry
// blockIdx.y -> level 0 of the scratch (pad channels: zeros, as the zeroed ring holds) and the last ring_len[0] positions of
// ring 0
template <int KIND>
__global__ __launch_bounds__(256) void pro_in_kernel(const StProArgs a) {
    const SwnGeom& g = a.g;
    const int kE = blockIdx.y;
    const StProEnt& en = a.e[kE];
    const float* P = en.P;
    const int H = g.H, Hp = g.Hp, K = g.K, seg = g.seg, n_pro = a.n_pro, R = a.ring_len[0];
    float* st = a.state + (size_t)en.slot * a.stride;
    float* lv = a.work + (size_t)kE * n_pro * Hp;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n_pro * Hp; e += gridDim.x * 256) {
        const int q = e / Hp, o = e - q * Hp;
        float v = 0.f;
        if (o < H) {
            float acc = P[a.y.cb + o];
            for (int k = 0; k < K; ++k) {
                const int rr = q - (K - 1 - k);
                if (KIND == SWN_KIND_LAPLACE) {
                    const float sv = 0.f;
                    const float t = fmaf(P[a.y.cv + (size_t)k * H + o], sv, P[a.y.cc + (size_t)k * H + o]);
                    acc += (rr >= -(seg - 1)) ? t : 0.f;
                } else {
                    const int idx = g.Q / 2;
                    const float t = P[a.y.ct + ((size_t)k * g.Q + idx) * H + o];
                    acc += (rr >= 0) ? t : 0.f;
                }
            }
            v = acc / (1.f + fabsf(acc));
            if (q >= n_pro - R) st[a.ring_off[0] + pmod(q, R) * Hp + o] = v;
        }
        lv[e] = v;
    }
}

// layer l for the positions of a.gpw groups of ST_TU consecutive positions of entry blockIdx.z: step_layer_tile_kernel with
// "eight utterances of a tile" replaced by "eight consecutive positions of one session".  Wave w keeps the 2 K Hp weights of
// pair 8 bx + w in registers over all its groups and stages position q0 + w's K-tap window of level l (positions below 0:
// zeros, what the zeroed ring holds in the stepped run); the next group's window is requested before the sums of this one.
// Lane 8 u of a wave finishes position q0 + u.  Waves of the pad channels [H, Hp) write the zeros of their column.
template <int NI, int KIND>
__global__ __launch_bounds__(64 * ST_TU) void pro_layer_kernel(const StProArgs a, const int l) {
    extern __shared__ __attribute__((aligned(16))) float pxs[]; // [ST_TU][NI * 256]
    const SwnGeom& g = a.g;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int o = blockIdx.x * ST_TU + w;
    const int H = g.H, Hp = g.Hp, K = g.K, H2 = 2 * g.H, seg = g.seg, KH = K * Hp, n_pro = a.n_pro;
    const StProEnt& en = a.e[blockIdx.z];
    const float* P = en.P;
    const bool live = o < H;
    const __amdgpu_buffer_rsrc_t rP = st_rsrc(P), rW = st_rsrc(a.work);
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
    const int dil = g.dil[l];
    const size_t lvl = (size_t)a.B * n_pro * Hp, ent = (size_t)blockIdx.z * n_pro * Hp;
    const size_t src = (size_t)(l & 1) * lvl + ent, dst = (size_t)((l + 1) & 1) * lvl + ent;   // float offsets into a.work
    float* st = a.state + (size_t)en.slot * a.stride;
    const int Rn = l + 1 < g.L ? a.ring_len[l + 1] : 0;
    const int ut = lane >> 3;                                  // the position this lane's octet ends up with (sum64x8)
    const int g0 = blockIdx.y * a.gpw, g1 = g0 + a.gpw < a.n_grp ? g0 + a.gpw : a.n_grp;
    float4 xv[NI];
    auto request = [&](const int gi) {                         // wave w: the window of position gi ST_TU + w
        const int qw = gi * ST_TU + w;
#pragma unroll
        for (int pc = 0; pc < NI; ++pc) {
            const int idx = pc * 256 + lane * 4;
            const int ic = idx < KH ? idx : 0;
            const int tap = ic / Hp, i = ic - tap * Hp;
            const int p = qw - (K - 1 - tap) * dil;
            const bool ok = idx < KH && qw < n_pro && p >= 0;
            xv[pc] = st_ld4(rW, ok ? st_off(src + (size_t)(ok ? p : 0) * Hp + i) : ST_OOB);
        }
    };
    if (g0 < g1) request(g0);
    for (int gi = g0; gi < g1; ++gi) {
        const int q = gi * ST_TU + ut;
        if (gi > g0) __syncthreads();                          // the previous group's sums are done with the buffer
#pragma unroll
        for (int pc = 0; pc < NI; ++pc) *reinterpret_cast<float4*>(pxs + (w * NI + pc) * 256 + lane * 4) = xv[pc];
        if (gi + 1 < g1) request(gi + 1);
        float gz = 0.f, gc = 0.f, bdz = 0.f, bdc = 0.f, hp = 0.f;
        const bool fin = (lane & 7) == 0 && q < n_pro && live;
        if (fin) {
            gz = P[a.y.bx + (size_t)l * H2 + o]; gc = P[a.y.bx + (size_t)l * H2 + H + o];
            bdz = P[a.y.bd + (size_t)l * H2 + o]; bdc = P[a.y.bd + (size_t)l * H2 + H + o];
            hp = a.work[src + (size_t)q * Hp + o];
            const float* condb = en.cond;
            const int Tf = en.Tf;
            for (int s = 0; s < seg; ++s) {
                int tt = q + s - g.rf; tt = tt < 0 ? 0 : tt;
                int f = tt / g.U; const int jj = tt - f * g.U;
                f = f < Tf ? f : Tf - 1;
                const float wv = P[a.y.wup + jj];
                const float* cr = condb + (size_t)f * g.N + (size_t)(l * seg + s) * H2;
                gz = fmaf(wv, cr[o], gz); gc = fmaf(wv, cr[H + o], gc);
            }
            if (KIND == SWN_KIND_SOFTMAX && g.audio_in) {
                const int idx = g.Q / 2;
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
                const float4 x = *reinterpret_cast<const float4*>(pxs + (u * NI + pc) * 256 + lane * 4);
                az = fmaf(wz[pc].x, x.x, az); az = fmaf(wz[pc].y, x.y, az);
                az = fmaf(wz[pc].z, x.z, az); az = fmaf(wz[pc].w, x.w, az);
                ac = fmaf(wc[pc].x, x.x, ac); ac = fmaf(wc[pc].y, x.y, ac);
                ac = fmaf(wc[pc].z, x.z, ac); ac = fmaf(wc[pc].w, x.w, ac);
            }
            azv[u] = az; acv[u] = ac;
        }
        const float myz = sum64x8(azv, lane), myc = sum64x8(acv, lane);
        if (fin) {
            const float z = sigm(gz * (myz + bdz));
            const float c = tanhf(gc * (myc + bdc));
            const float hn = (1.f - z) * c + z * hp;
            if (l + 1 < g.L) {
                a.work[dst + (size_t)q * Hp + o] = hn;
                if (q >= n_pro - Rn) st[a.ring_off[l + 1] + pmod(q, Rn) * Hp + o] = hn;
            }
            if (q == n_pro - 1) st[a.o_hcat + l * Hp + o] = hn;
        } else if ((lane & 7) == 0 && q < n_pro && o < Hp && l + 1 < g.L) {
            a.work[dst + (size_t)q * Hp + o] = 0.f;
        }
    }
}

// floats of the two level buffers of `n` entries; 0 when they pass the range of a 32-bit buffer offset
size_t pro_work_floats(const SwnGeom& g, int n) {
    const size_t f = 2 * (size_t)n * (size_t)(g.rf - g.seg + 1) * g.Hp;
    return f < ST_OOB_FLOATS ? f : 0;
}

template <int KIND>
int pro_launch(const StProArgs& a, hipStream_t st) {
    const SwnGeom& g = a.g;
    const int n = a.B;
    hipLaunchKernelGGL(pro_setup_kernel, dim3(16, n), dim3(256), 0, st, a);
    const int nin = (a.n_pro * g.Hp + 255) / 256;
    hipLaunchKernelGGL((pro_in_kernel<KIND>), dim3(nin < 64 ? nin : 64, n), dim3(256), 0, st, a);
    const dim3 grid((g.H + ST_TU - 1) / ST_TU, (a.n_grp + a.gpw - 1) / a.gpw, n);
    auto layer = [&](auto ni_, int l) -> bool {
        constexpr int NI = decltype(ni_)::value;
        const size_t lds = (size_t)ST_TU * NI * 256 * sizeof(float);
        // dynamic LDS from 64 KB on: set on every call (the attribute is per device)
        if (lds >= 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(pro_layer_kernel<NI, KIND>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return false;
        hipLaunchKernelGGL((pro_layer_kernel<NI, KIND>), grid, dim3(64 * ST_TU), lds, st, a, l);
        return true;
    };
    const int ni = (g.K * g.Hp + 255) / 256;
    for (int l = 0; l < g.L; ++l) {
        bool ok;
        if (ni <= 1) ok = layer(std::integral_constant<int, 1>{}, l);
        else if (ni <= 6) ok = layer(std::integral_constant<int, 6>{}, l);
        else ok = layer(std::integral_constant<int, 8>{}, l);
        if (!ok) return SWN_E_LAUNCH;
    }
    return swn_launch_status("swn_decode_stepped_prologue");
}

}  // namespace

extern "C" size_t swn_decode_stepped_prologue_work_floats(const swn_net_desc* d, int n_entries) {
    SwnGeom g;
    if (swn_make_geom(d, &g) < 0 || n_entries < 1 || n_entries > SWN_DECODE_POOL_MAX_ENTRIES) return 0;
    if (!chain_takes(g, 1)) return 0;
    return pro_work_floats(g, n_entries);
}

extern "C" int swn_decode_stepped_prologue(const swn_net_desc* d, const float* packed, const float* const* models, int n_models,
                                           const int32_t* model_of_entry, int n_slots,
                                           const swn_decode_stepped_prologue_entry* entries, int n_entries,
                                           const swn_decode_io* io, float* session, float* work, void* stream_) {
    StProArgs a;
    int rc = swn_make_geom(d, &a.g);
    if (rc < 0) return rc;
    const SwnGeom& g = a.g;
    // the argument rules (include/swn_hip.h): those of the stepped pool call; nothing is launched before they pass
    if ((!models && !packed) || !entries || !io || !session || !work) return SWN_E_BADARG;
    if (n_slots < 1 || n_entries < 1 || n_entries > SWN_DECODE_POOL_MAX_ENTRIES) return SWN_E_BADARG;
    if (models || model_of_entry) {
        rc = swn_pool_models_check(models, n_models, model_of_entry, n_entries);
        if (rc != SWN_OK) return rc;
    }
    if (io->noise_dev || io->forced_dev) return SWN_E_BADARG;
    for (int e = 0; e < n_entries; ++e) {
        const swn_decode_stepped_prologue_entry& en = entries[e];
        if (!en.cond_dev || en.n_frames < 1 || en.slot < 0 || en.slot >= n_slots) return SWN_E_BADARG;
        for (int f = 0; f < e; ++f)
            if (entries[f].slot == en.slot) return SWN_E_BADARG;   // two entries on one session
    }
    if (!swn_decode_stepped_supported(g, n_slots) || pro_work_floats(g, n_entries) == 0) return SWN_E_UNSUPPORTED;

    fill_args(a, models ? models[0] : packed, nullptr, swn_pool_noise_of(io), nullptr, io->seed_dev, session, nullptr, nullptr,
              n_entries, 0, 0, 0);
    a.work = work;
    for (int e = 0; e < n_entries; ++e) {
        a.e[e].cond = entries[e].cond_dev; a.e[e].Tf = entries[e].n_frames; a.e[e].slot = entries[e].slot;
        a.e[e].P = models ? models[model_of_entry[e]] : packed;
    }
    // enough workgroups to fill the chip about twice (8 waves each), each keeping its weights over as many groups as that allows
    a.n_grp = (a.n_pro + ST_TU - 1) / ST_TU;
    const long long per_grp = (long long)((g.H + ST_TU - 1) / ST_TU) * n_entries;
    long long gpw = per_grp * a.n_grp / 512;
    a.gpw = gpw < 1 ? 1 : (gpw > a.n_grp ? a.n_grp : (int)gpw);
    (void)hipGetLastError();
    hipStream_t st = (hipStream_t)stream_;
    return g.kind == SWN_KIND_LAPLACE ? pro_launch<SWN_KIND_LAPLACE>(a, st) : pro_launch<SWN_KIND_SOFTMAX>(a, st);
}
