// What the two BL6-class decode kernels share (swn_decode_bl6.hip: the symmetric kernel, swn_decode_bl6w.hip: the
// wave-specialised one): the launch arguments, the constants of the class, the device helpers both step loops are written
// with, and the host side that fills the arguments and launches.  The kernels' own LDS carves (Tr, Tw) and phases stay in
// their files.  Both kernels sit at the register limit: a change here changes the generated code of both.
#pragma once
#include <hip/hip_runtime.h>
#include "swn_decode_internal.hpp"

namespace swn_bl6 {

constexpr int NT = 512;
constexpr int H = 64;
constexpr int L = 6;
constexpr int RF = 64;
#ifdef SWN_STAMP
constexpr bool HEADS_ON = false;
#else
constexpr bool HEADS_ON = true;
#endif

struct Bl6Args {
    const float* P;
    SwnLayout y;
    const float* cond;
    const float* noise;            // classic mode: the host-drawn stream
    const void* forced;
    void* out;
    float* heads;
    int B, Tf, n_steps, U, N;
    // extended mode only (in-kernel generator, noise dump, caller's seed waveform)
    SwnNoise nz;
    const void* seed;
    // streamed chunk only (STREAM instantiations): absolute index of the chunk's first step, 1 = resume from the
    // session instead of running the prologue, the session ([B][T::sess_floats])
    int step0, resume;
    float* sess;
};

// the arguments of a pool launch: a streamed chunk over the entries (batch = E, n_steps = n_max), then the entry table
struct Bl6PoolArgs {
    Bl6Args c;
    SwnPoolTable t;
};
static_assert(sizeof(Bl6PoolArgs) <= 4096, "kernel arguments are limited to 4 KB");
// ... and of a multi-model pool launch (swn_decode_pool_chunk_models): the model table behind them.  The kernels that take it
// are instantiations of their own (MODELS), so the single-model pool kernels stay the code they were.
struct Bl6PoolModelsArgs : Bl6PoolArgs {
    SwnPoolModels m;
};
static_assert(sizeof(Bl6PoolModelsArgs) <= 4096, "kernel arguments are limited to 4 KB");
// bf16 / FP8 storage of the streamed head matrices (swn_decode_w16, swn_decode_w8 and their chunk / pool forms, symmetric
// kernel only): the image pointer rides behind the arguments of the fp32 launch in structs of its own, taken by instantiations
// of their own (WK_BF16, WK_E4M3), so the fp32 kernels keep their arguments and their code.
struct Bl6ImageArgs : Bl6Args {
    const void* img;
};
struct Bl6PoolImageArgs : Bl6PoolArgs {
    const void* img;
};
static_assert(sizeof(Bl6PoolImageArgs) <= 4096, "kernel arguments are limited to 4 KB");
// ... and of a multi-model pool launch over a stored format (swn_decode_pool_chunk_models_w16 / _w8): one image per model behind
// the model table, indexed like its packed buffers (m.of[entry]); 128 bytes more
struct Bl6PoolModelsImageArgs : Bl6PoolModelsArgs {
    const void* img[SWN_POOL_MAX_MODELS];
};
static_assert(sizeof(Bl6PoolModelsImageArgs) <= 4096, "kernel arguments are limited to 4 KB");
// ... and of a wide pool launch (swn_decode_pool_chunk_wide): the table lies in device memory, and its rows carry each entry's
// packed buffer and image - one struct for every weight format, taken by instantiations of their own (WIDE)
struct Bl6PoolWideArgs {
    Bl6Args c;
    const SwnPoolWideRow* rows;
};
// The bf16 image (swn_pack_decode_w16): the three lane-tiled copies wsk2 / w12 / w22 of the packed buffer rounded to bf16 (nearest
// even), slices 2g and 2g + 1 of 16 inputs folded into one: section [NS / 2][rows][4 lanes][4 words], word j of a lane =
// bf16(slice 2g, input 4 lane + j) in bits 0-15 | bf16(slice 2g + 1, input 4 lane + j) in bits 16-31.  A lane's 16-byte load
// then carries what two of its fp32 loads carry, and it widens (<< 16, & 0xffff0000: exact) and accumulates them in the
// order of the fp32 kernel.  Byte offsets of the sections; w2 is empty for Laplace nets (their out_2 rows sit in LDS as fp32).
struct Bl6W16Layout {
    size_t wsk, w1, w2, total;
};
inline __host__ __device__ Bl6W16Layout w16_layout(int S, int O1, int NO, bool softmax) {
    Bl6W16Layout y;
    y.wsk = 0;
    y.w1 = y.wsk + (size_t)L * S * 64 * 2;
    y.w2 = y.w1 + (size_t)O1 * S * 2;
    y.total = y.w2 + (softmax ? (size_t)NO * O1 * 2 : 0);
    return y;
}

// FP8 (OCP E4M3FN) storage of the same matrices (swn_decode_w8 and its chunk / pool forms).  Contract (include/swn_hip.h):
// per output row r of each matrix one power of two 2^e_r that brings the row's largest magnitude into the top binade of E4M3
// (<= 448), code = nearest E4M3 value of W 2^e_r, ties to even; the kernel widens a code to exactly code * 2^-e_r in fp32
// (w8_pair) and runs the fp32 kernel's FMAs in the fp32 kernel's order.
// The image (swn_pack_decode_w8): the W16 image with four slices of 16 inputs folded into a word instead of two - section
// [NS / 4][rows][4 lanes][4 words], byte s of word j of a lane = code(slice 4g + s, input 4 lane + j), so a lane's 16-byte load
// carries what four of its fp32 loads carry and v_cvt_scalef32_pk_f32_fp8 widens bytes (0, 1) or (2, 3) of a word at once.
// Behind the three code sections: one fp32 2^-e_r per row, [L][S] for out_skip, [O1] for out_1, (softmax) [NO] for out_2; the
// kernel keeps them in LDS behind its carve (T::o_end).  Byte offsets; w2 / s2 are empty for Laplace nets.
struct Bl6W8Layout {
    size_t wsk, w1, w2, ssk, s1, s2, total;
};
inline __host__ __device__ Bl6W8Layout w8_layout(int S, int O1, int NO, bool softmax) {
    Bl6W8Layout y;
    y.wsk = 0;
    y.w1 = y.wsk + (size_t)L * S * 64;
    y.w2 = y.w1 + (size_t)O1 * S;
    y.ssk = y.w2 + (softmax ? (size_t)NO * O1 : 0);
    y.s1 = y.ssk + (size_t)L * S * 4;
    y.s2 = y.s1 + (size_t)O1 * 4;
    y.total = y.s2 + (softmax ? (size_t)NO * 4 : 0);
    return y;
}

constexpr int cmax(int a, int b) { return a > b ? a : b; }
constexpr int pow2ceil(int x) { int r = 1; while (r < x) r <<= 1; return r; }
constexpr int r4(int x) { return (x + 3) & ~3; }

// Streamed weights go through a buffer resource: one 32-bit per-thread offset plus scalar /
// immediate offsets per load, instead of a 64-bit VGPR address per load (which spilled).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 buf_ld4(__amdgpu_buffer_rsrc_t r, unsigned voff_bytes, unsigned soff_bytes) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, voff_bytes, soff_bytes, 0));
}
// 16 bytes of the bf16 image: four words of two bf16 each; lo / hi widen one half of a word to the fp32 it was rounded from
__device__ __forceinline__ uint4 buf_ld4u(__amdgpu_buffer_rsrc_t r, unsigned voff_bytes, unsigned soff_bytes) {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, voff_bytes, soff_bytes, 0));
}
__device__ __forceinline__ float w16_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float w16_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
// two E4M3 codes of a word of the FP8 image - bytes (0, 1), or (2, 3) with HI - as code * scale in fp32; scale is the row's
// power of two 2^-e_r, for which the scaled conversion is exact (tests: swn_e4m3_table against the format's definition).
// Every widening of the W8 instantiations, the resident out_1 slices and swn_e4m3_table included, goes through this helper.
template <bool HI>
__device__ __forceinline__ float2 w8_pair(unsigned w, float scale) {
    const auto v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, scale, HI);
    return make_float2(v[0], v[1]);
}
// the four slices of word w: f[s] = byte s
__device__ __forceinline__ void w8_word(unsigned w, float scale, float (&f)[4]) {
    const float2 lo = w8_pair<false>(w, scale), hi = w8_pair<true>(w, scale);
    f[0] = lo.x; f[1] = lo.y; f[2] = hi.x; f[3] = hi.y;
}
// a 16-byte load of the image as four fp32 slices of four inputs: s[k] = slice 4g + k
__device__ __forceinline__ void w8_slices(const uint4& w, float scale, float4 (&s)[4]) {
    float x[4], y[4], z[4], q[4];
    w8_word(w.x, scale, x); w8_word(w.y, scale, y); w8_word(w.z, scale, z); w8_word(w.w, scale, q);
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = make_float4(x[k], y[k], z[k], q[k]);
}

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float sum4(float v) {      // all 4 lanes of a quad get the quad sum
    v += dpp_f<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_f<0x4E>(v);      // quad_perm [2,3,0,1]
    return v;
}
__device__ __forceinline__ float sum8(float v) {      // all 8 lanes of an aligned octet get the sum
    v = sum4(v);
    v += dpp_f<0x141>(v);     // row_half_mirror
    return v;
}
// exp(x) = 2^(x*log2e) on the transcendental unit; the product's rounding error is fed back as a
// first-order correction, so the result stays within ~1.5 ulp (libm-grade) at 6 instructions
// (the 1e-5 bar is held through 66 000 recurrent steps).
__device__ __forceinline__ float exp_c(float x) {
    const float t = x * 1.44269504f;
    const float lo = fmaf(x, 1.44269504f, -t) + x * 1.92596299e-8f;
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, lo * 0.693147181f, e);
}
__device__ __forceinline__ float rcp_c(float x) {        // v_rcp_f32 + one Newton step (<= 1 ulp)
    const float r = __builtin_amdgcn_rcpf(x);
    return fmaf(r, fmaf(-x, r, 1.f), r);
}
__device__ __forceinline__ float sigm(float x) { return rcp_c(1.f + exp_c(-x)); }
__device__ __forceinline__ float tanh_c(float x) {        // (1 - e^-2|x|) / (1 + e^-2|x|), abs error ~1e-7
    if (fabsf(x) > 9.02f) return copysignf(1.f, x);    // saturated in fp32 (also keeps this a branchy block)
    const float t = exp_c(-2.f * fabsf(x));
    return copysignf((1.f - t) * rcp_c(1.f + t), x);
}
__device__ __forceinline__ float ssign(float x) { return x * rcp_c(1.f + fabsf(x)); }

// Workgroup barrier that orders LDS traffic only: the cross-wave hand-offs of these kernels all go
// through LDS; a plain __syncthreads() also drains (vmcnt(0)) global loads that may stay in flight.
__device__ __forceinline__ void lds_barrier() {
#ifdef SWN_SYNC
    __syncthreads(); return;
#endif
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The same barrier for a wave that has requested LDS reads it will use only behind it: rows no wave writes in the phase that
// ends here, so nothing of them depends on the barrier.  lds_barrier() cannot carry them across - its release fence waits for
// lgkmcnt(0) and no load moves over its acquire fence.  Here the wave waits until N operations are left on its LDS counter:
// LDS serves one wave's operations in order, so with the N reads issued BEHIND the wave's last hand-off write of the phase
// (lds_fence_compiler() between them, the issue order pinned with sched_barrier(0)) that write is retired and the reads stay in
// flight through the s_barrier.  lgkmcnt also counts scalar loads, which return out of order: none may be outstanding at the call
// (check the ISA of every instantiation; the compiler itself waits for lgkmcnt(0) before it uses one).  N <= 15: the counter has
// four bits.
__device__ __forceinline__ void lds_fence_compiler() { asm volatile("" ::: "memory"); }
template <int N>
__device__ __forceinline__ void lds_barrier_keep() {
    static_assert(N >= 0 && N <= 15, "lgkmcnt is a four-bit counter");
#ifdef SWN_SYNC
    __syncthreads(); return;
#endif
    __builtin_amdgcn_sched_barrier(0);          // (arithmetic is free to cross the asm and the s_barrier: the multiply-adds the
    asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(N) : "memory");   //  early reads feed moved in front of them, behind lgkmcnt(0))
    __builtin_amdgcn_s_barrier();
    lds_fence_compiler();
    __builtin_amdgcn_sched_barrier(0);
}

// the five input-layer constants of channel `o` in a kernel's carve (cb[64], cv[2][64], cc[2][64] at T::o_cz of `lds`)
#define c_b  lds[T::o_cz + o]
#define c_v0 lds[T::o_cz + H + o]
#define c_v1 lds[T::o_cz + 2 * H + o]
#define c_c0 lds[T::o_cz + 3 * H + o]
#define c_c1 lds[T::o_cz + 4 * H + o]

// ---- host side
// the launch-wide arguments of a checked call (one-shot: step0 = resume = 0, no session; pool: those of a chunk over the entries)
inline void fill_args(Bl6Args& a, const SwnDecodeCall& c) {
    swn_make_layout(&c.g, &a.y);
    a.P = c.packed; a.cond = c.cond; a.noise = c.nz.ptr; a.nz = c.nz; a.forced = c.forced; a.seed = c.seed; a.out = c.out;
    a.heads = c.heads; a.B = c.batch; a.Tf = c.n_frames; a.n_steps = c.n_steps; a.U = c.g.U; a.N = c.g.N;
    a.step0 = c.step0; a.resume = c.resume; a.sess = c.stream ? c.state : nullptr;
}

// the extended instantiation runs whenever the classic one's inputs (host-drawn noise, no dump, zero seed) are not given
inline bool wants_ext(const Bl6Args& a) { return !a.nz.ptr || a.nz.dump || a.seed; }

// one workgroup per utterance / pool entry; dynamic LDS above 64 KB has to be asked for
template <class A>
int launch_kernel(void (*kern)(A), size_t lds_bytes, int n_groups, const A& a, hipStream_t st, const char* where) {
    if (lds_bytes > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
        return SWN_E_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(n_groups), dim3(NT), lds_bytes, st, a);
    return swn_launch_status(where);
}

}  // namespace swn_bl6
