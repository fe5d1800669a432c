// What the kernel files of the stepped multi-launch decode share (swn_decode_stepped.hip: the launch chain;
// swn_decode_stepped_prologue.hip: a new session's prologue in parallel launches): the launch arguments and the layout of an
// utterance's state block, the branch-free buffer loads, and the canonical 64-lane sums - both files must form every sum in
// the same order, so there is one copy of each.  Everything here has internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include "swn_decode_internal.hpp"

namespace {

constexpr size_t ST_OOB_FLOATS = 0x20000000u;   // 2 GiB of floats: first offset a buffer load cannot take

struct StArgs {
    SwnGeom g;
    SwnLayout y;
    const float* P; const float* cond; SwnNoise nz; const void* forced; const void* seed;
    float* state; void* out; float* heads;
    int B, Tf, n_steps, n_pro, WN;
    int ring_off[SWN_MAXL], ring_len[SWN_MAXL];
    int o_hcat, o_skip, o_o1, o_o2, o_hist, o_cnt, stride;      // per-utterance float offsets
    int o2_by_rowvec;                                           // out_2 was computed by a rowvec launch into o_o2 (wide heads)
    int step0;                                                  // streamed chunk (STREAM tails): absolute index of its step 0
};

// 64-bit float offset -> buffer byte offset, ST_OOB when it does not fit the 31-bit range (never wraps)
__device__ __forceinline__ unsigned st_off(size_t floats) {
    return floats < (size_t)(ST_OOB_FLOATS) ? (unsigned)(floats * 4) : 0x80000000u;
}

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ int pmod(int r, int m) { int t = r % m; return t < 0 ? t + m : t; }

// Every launch of this chain is a handful of memory round trips, so the loads of a phase must all be in flight
// together.  A conditional load (`ok ? *p : 0`) compiles to an exec-masked branch followed by s_waitcnt vmcnt(0):
// the first version of these kernels paid 12-14 SERIAL round trips per launch (4.5-8 us).  Loads therefore go
// through buffer resources with 32-bit byte offsets, and "not mine / past the end" is the out-of-range offset
// (reads zero, no branch).  The packed parameters and the whole decode state must each stay below 2 GiB.
constexpr unsigned ST_OOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t st_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ float4 st_ld4(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
__device__ __forceinline__ float st_ld1(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
__device__ __forceinline__ float sum64(float v) {
    v += __shfl_xor(v, 32, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);  v += __shfl_xor(v, 1, 64);
    return v;
}
__device__ __forceinline__ float sum32(float v) {
    v += __shfl_xor(v, 16, 32); v += __shfl_xor(v, 8, 32); v += __shfl_xor(v, 4, 32);
    v += __shfl_xor(v, 2, 32);  v += __shfl_xor(v, 1, 32);
    return v;
}

// 64-lane sums of EIGHT values at once: a butterfly in which a lane keeps half of its values at each of the first three
// exchanges (xor 32, 16, 8) and sums the survivor over xor 4, 2, 1 - 10 exchanges instead of 8 x 6, and every value goes
// through exactly the pairings of sum64 in the same order (bit-identical).  Returns utterance (lane >> 3)'s total.
__device__ __forceinline__ float sum64x8(const float (&v)[8], int lane) {
    float a4[4], a2[2], a1;
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float keep = h5 ? v[k + 4] : v[k], give = h5 ? v[k] : v[k + 4];
        a4[k] = keep + __shfl_xor(give, 32, 64);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float keep = h4 ? a4[k + 2] : a4[k], give = h4 ? a4[k] : a4[k + 2];
        a2[k] = keep + __shfl_xor(give, 16, 64);
    }
    {
        const float keep = h3 ? a2[1] : a2[0], give = h3 ? a2[0] : a2[1];
        a1 = keep + __shfl_xor(give, 8, 64);
    }
    a1 += __shfl_xor(a1, 4, 64); a1 += __shfl_xor(a1, 2, 64); a1 += __shfl_xor(a1, 1, 64);
    return a1;
}

constexpr int ST_TU = 8;                                       // utterances (= waves) of a tile

int plan(StArgs& a) {
    const SwnGeom& g = a.g;
    int o = 0;
    for (int l = 0; l < g.L; ++l) { a.ring_off[l] = o; a.ring_len[l] = g.pad[l] + g.seg; o += a.ring_len[l] * g.Hp; }
    a.WN = (g.K - 1 > g.lpc ? g.K - 1 : g.lpc) + g.seg;
    a.o_hcat = o; o += g.L * g.Hp;
    a.o_skip = o; o += g.Sp;
    a.o_o1 = o; o += g.O1p;
    a.o_o2 = o; o += swn_round4(g.NO);
    a.o_hist = o; o += swn_round4(a.WN);
    a.o_cnt = o; o += 4;
    a.stride = (o + 63) & ~63;
    return a.stride;
}

// the geometries the chain runs, for `batch` utterances (pool: slots)
bool chain_takes(const SwnGeom& g, int batch) {
    if ((g.K * g.Hp + 255) / 256 > 8 || g.seg > 16 || g.lpc > 16 || g.NO > 4096) return false;
    StArgs t; t.g = g;
    return (size_t)plan(t) * batch * sizeof(float) < (1ull << 31) && t.WN <= 32;   // 32-bit buffer offsets; LDS window
}

// the launch arguments of `n` utterances (pool: entries) over a.g, all but a pool's table
void fill_args(StArgs& a, const float* packed, const float* cond, const SwnNoise& nz, const void* forced, const void* seed,
               float* state, void* out, float* heads, int n, int n_frames, int n_steps, int step0) {
    swn_make_layout(&a.g, &a.y);
    plan(a);
    a.P = packed; a.cond = cond; a.nz = nz; a.forced = forced; a.seed = seed; a.state = state; a.out = out; a.heads = heads;
    a.B = n; a.Tf = n_frames; a.n_steps = n_steps; a.n_pro = a.g.rf - a.g.seg + 1; a.step0 = step0;
    // one 256-thread workgroup evaluates 8 rows per pass: beyond 64 rows (8 passes, ~7 us) a launch of its own is cheaper
    a.o2_by_rowvec = a.g.NO > 64 ? 1 : 0;
}

}  // namespace
