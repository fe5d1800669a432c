// BL6-class autoregressive decode on gfx950, WAVE-SPECIALISED form (single-sample Laplace nets: 1x6 dilated stack, H = 64, K = 2,
// S = O1 = 128, seg = 1, lpc 0 / 4).
//
// swn_decode_bl6.hip gives all eight waves of the workgroup the same program: between two barriers the two waves of a SIMD run the
// same dependent chain (LDS read -> 16-deep FMA chains -> DPP reduction -> transcendentals -> LDS write) and stall in the same
// places, so a SIMD takes the time of two waves that do not overlap (9 900 cycles per step against 2 400 of VALU
// issue per wave).  A conv of kernel size 2 offers the asymmetry that lets them overlap: a layer's pre-activation is
//     W[:, tap 1] h_{l-1}(t)  +  W[:, tap 0] h_{l-1}(t - dil)  +  b
// and the second product does not depend on the step in progress - for every layer it is known one step ahead (dil >= 1).  So:
//   * group A (waves 0-3, one per SIMD) owns the chain: per layer the CURRENT-tap half (128 rows x 64 inputs: thread (o, p) two
//     rows x 16 inputs, reduced over 4 lanes - the two quad sums transposed, so that lane 0 of the quad ends with the gate's
//     and lane 1 with the candidate's in two DPP steps), the gate epilogue (one straight line for both lanes: sigmoid | tanh
//     from the same exp_c / rcp_c, no branch for a saturated tanh - the arithmetic itself returns +-1 there), the hand-off
//     through LDS;
//   * group B (waves 4-7, the other wave of every SIMD) works one step AHEAD and off the chain: the OLDER-tap halves (+ bias) of
//     layers 0-4 for step t + 1, left in LDS (formed where group B has room: two in the first phase, three beside group A's
//     out_1 - in the classic lpc 0 kernel three and two; the last layer's is formed by group A, from group B's half in LDS,
//     in the one phase where the chain waits for
//     group B - with lpc 0 half of its operands are requested a phase early, in front of barrier 5), and the whole out_skip
//     accumulation of step t (slice l in the phase after layer l: its four input quads read at the head of the phase, the
//     next slice's weights requested quarter by quarter behind the multiply-adds that free their registers; in the classic lpc 0
//     kernel slice 0 does not stream: it stays in 32 registers of group B from the launch's start, the last load of slices 1 - 4
//     is requested at the head of the next phase, and the input quads of slices 0 - 4 come from the ring rows group A writes);
//   * group A keeps its halves of all six matrices in registers (192 per thread), group B five of them (160) and the sixth in LDS
//     (it also holds a slice of out_skip weights in flight); the out_1 matrix is LDS-resident whole (the 64 KB the sixth layer of
//     the symmetric kernel took), only out_skip streams from L2;
//   * out_1 is group A's alone (two rows per thread), and out_2 beside it as one partial sum per wave; the sum of the four partials
//     + sampling + the next input layer run in every wave of group A, each forming its own copy of h0 and going straight on into
//     layer 0 (wave 0 alone stores the sample and the heads).  Between the sample and layer 0's first LDS read stands the input
//     layer's arithmetic and its one LDS write only: the next step's conditioning taps, parity offset and layer-0 row are formed
//     while the tail waits for the partials (one step ahead), the wave's own h0 is read back without a wait (LDS serves a wave's
//     operations in order), and in the classic lpc 0 kernel the sample and heads stores wait one step: the loop is rotated, they leave behind layer 0's
//     first LDS reads of the next step, with the refill test and the noise staging (the last step's behind the loop).
// Same arithmetic per element as the symmetric kernel up to the order of the partial sums (1e-7 relative); same noise, seed,
// forced-input and heads interface (swn_decode_bl6.hip: classic = host-drawn noise, zero seed; extended = in-kernel generator,
// noise dump, caller's seed waveform).  8 barriers per step.  cswnv_shift1.py:281-430.
#include <type_traits>
#include "swn_decode_bl6_common.hpp"
#include "swn_decode_internal.hpp"

// diagnostic builds only (the forms profiles/decode_bl6w_resident_bench.json compares): -DSWN_RES_SLICE=-1 streams every out_skip
// slice as the parent did, =5 keeps the last slice resident instead of the first; -DSWN_ROTATE=0 leaves group A's loop unrotated
#ifndef SWN_RES_SLICE
#define SWN_RES_SLICE 0
#endif
#ifndef SWN_ROTATE
#define SWN_ROTATE 1
#endif
// -DSWN_OLDER2_MERGED=0: layer 2's older-tap product stays beside out_1 (the parent's placement); -DSWN_EARLY_ROWS=n: of the two
// products left beside out_1, n have their operand rows read in front of barrier 6 (built: 1; 2 and 0 measured).
// -DSWN_HANDOFF=bits: group B takes over from group A 1 the stores, 2 the conditioning refill, 4 the noise staging.  Built: 0 -
// group A does all three itself, behind layer 0's reads; no subset was faster on the final build.
// Timing only, samples wrong by construction, never tested or shipped: -DSWN_DIAG_NOSIDE (nobody stores, refills or stages the
// noise inside the loop), -DSWN_DIAG_NOSIDE_B (with a hand-off: group B's share is left out), -DSWN_DIAG_NOSTREAM (group B
// requests no out_skip slice in L1 - L5 and consumes what its registers hold)
#ifndef SWN_HANDOFF
#define SWN_HANDOFF 0
#endif
#ifndef SWN_OLDER2_MERGED
#define SWN_OLDER2_MERGED 1
#endif
#ifndef SWN_EARLY_ROWS
#define SWN_EARLY_ROWS 1
#endif
// The classic lpc 0 kernel, both groups' layer phases started ahead of the barrier:
// -DSWN_LEAD=n: of the eight loads of out_skip slice l, the last n (0, 1, 2 = a quarter, 4 = a half) are not requested at the end
// of phase L(l) but at the head of L(l + 1), behind its four LDS reads and in front of its first multiply-add (skip_roll_b);
// -DSWN_RINGX=0: group A writes every layer's output to o_hcat too and group B reads its slice's inputs there (the parent's form);
// 1: layers 0 - 4 leave o_hcat alone, group B reads the ring row group A has just written.
// Built: one load and the ring rows - 412.3 k samples/s of the headline beside the parent's 407.3; a quarter 406.8, a half 376.1,
// one load without the ring rows and the ring rows without a lead both below the parent.
// Timing only, never tested or shipped: -DSWN_DIAG_PLAINEXP (layer_a's epilogue on the bare v_exp_f32 / v_rcp_f32)
#ifndef SWN_LEAD
#define SWN_LEAD 1
#endif
#ifndef SWN_RINGX
#define SWN_RINGX 1
#endif
// The classic lpc 0 kernel, instructions taken off group A's chain that produce nothing the result needs (each
// switch 0 = the parent's form; no multiply-add, operand or summation order differs, the samples are the parent's bits with
// every subset).  Built: SWN_SWAP_ROWS and SWN_FLAT_EPILOGUE - 421.1 k samples/s of the headline beside the parent's 413.2.
// Measured and left out: SWN_CARRY_HP (393.5 k alone beside 413.1, and 2 % off every build that has it) and SWN_PLAIN_TAIL
// (416.1 - 416.5 k on top of the built form's 419.6 - 420.6).
// -DSWN_CARRY_HP: layer l + 1's highway operand is the `hn` the same thread wrote to ring l + 1 one phase earlier - it stays in a
// register instead of coming back through LDS (layers 1 - 5, prologue too; layer 0's h0 lives in another lane mapping);
// -DSWN_SWAP_ROWS: lanes of odd p load their gate and candidate rows swapped, so the partial sums are "own" / "other" in every
// lane and quad_sum_by_parity takes them without the two selects;
// -DSWN_FLAT_EPILOGUE: the gate epilogue runs on all four lanes of the quad (lanes 2 / 3 hold the sums of lanes 0 / 1) with no
// exec mask; the hand-off store of lanes p != 0 goes to a per-thread dump word behind the carve (o_dump, 1 KB);
// -DSWN_PLAIN_TAIL: the one-shot launch without forced inputs runs a copy of the kernel that has no forced load, wait or select
// in the tail and forms the next input layer behind the last step too (its row exists and nobody reads it).
#ifndef SWN_CARRY_HP
#define SWN_CARRY_HP 0
#endif
#ifndef SWN_SWAP_ROWS
#define SWN_SWAP_ROWS 1
#endif
#ifndef SWN_FLAT_EPILOGUE
#define SWN_FLAT_EPILOGUE 1
#endif
#ifndef SWN_PLAIN_TAIL
#define SWN_PLAIN_TAIL 0
#endif
// (the stamp build hands skip_roll_b the counter of its wait for the loads requested at the head of the phase)
#ifdef SWN_STAMP
#define SWN_TDEF_PARAM , unsigned long long& tdef
#define SWN_TDEF_ARG(k) , td[k]
#else
#define SWN_TDEF_PARAM
#define SWN_TDEF_ARG(k)
#endif

namespace {

using namespace swn_bl6;

constexpr int NG = 256;            // threads per group
constexpr int S = 128;
constexpr int O1 = 128;

template <int LPC_, bool EXT_>
struct Tw {
    static constexpr int LPC = LPC_;
    static constexpr bool EXT = EXT_;
    using Ext = Tw<LPC_, true>;
    static constexpr bool NEWFORM = !EXT_ && LPC_ == 0;   // the classic lpc 0 kernel: resident slice, hand-off ring (decode_body)
    static constexpr int LEAD = NEWFORM ? SWN_LEAD : 0;   // loads of a slice requested at the head of the next phase (skip_roll_b)
    static constexpr bool RINGX = NEWFORM && SWN_RINGX;   // group B's inputs of slices 0 - 4 come from the rings, not from o_hcat
    static constexpr int NO = 2 + LPC_;
    static constexpr int WN = cmax(1, LPC_) + 1;
    static constexpr int ring_len(int l) { return pow2ceil((1 << l) + 1); }
    static constexpr int ring_off(int l) { int o = 0; for (int i = 0; i < l; ++i) o += ring_len(i) * H; return o; }
    static constexpr int PF = L * 2 * H;                  // floats of one conditioning frame
    static constexpr int NZC = 64, NZB = 4;
    // LDS carve (float offsets); everything the step loop addresses with immediates sits below 64 KB, the out_1 matrix last
    static constexpr int o_ring = 0;
    static constexpr int o_hcat = o_ring + ring_off(L);
    static constexpr int o_gp = o_hcat + L * H;
    static constexpr int o_bx = o_gp + 2 * PF;
    static constexpr int o_bd = o_bx + L * 2 * H;
    static constexpr int o_old = o_bd + L * 2 * H;         // [2][L][2H]: older-tap products + bias of the step in progress / the next
    static constexpr int o_wup = o_old + 2 * L * 2 * H;
    static constexpr int o_skip = o_wup + 256;
    static constexpr int o_p2 = o_skip + S;                // out_2 as [NO][4] partial sums, one per wave of group A (b2 in wave 0's)
    static constexpr int o_tnz = o_p2 + 4 * NO;
    static constexpr int o_cz = o_tnz + r4(NZB * NZC);     // (the noise ring, both modes)  cb[64], cv[2][64], cc[2][64]
    static constexpr int o_w2 = o_cz + 5 * H;              // out_2 rows [NO][S] (+b2)
    static constexpr int o_bias = o_w2 + NO * S + r4(NO);  // bsk[S], b1[O1]
    static constexpr int o_w1 = o_bias + S + O1;           // out_1, lane-tiled [8][O1][4][4] like the global copy w12
    static constexpr int o_wl = o_w1 + 8 * O1 * 16;        // group B's half of the LAST layer, [8][256 threads][4]: with it in registers
                                                           // too (192 + the out_skip weights in flight) the kernel spilled 22-35 registers
    static constexpr int o_h0w = o_wl + 8 * NG * 4;        // h0 of the next position as waves 1-3 of group A form it, [3][H] (wave 0's copy
                                                           // is the layer-0 ring slot); past 64 KB: addressed from a per-wave base
    // (classic lpc 0 with the hand-off) the NO head sums and the sample of the last NHO steps, [NHO][HO] with the sample at NO:
    // written by group A's wave 0 one step late, stored to memory by group B 64 steps at a time (decode_body)
    static constexpr int o_ho = o_h0w + 3 * H;
    static constexpr int HO = 4, NHO = 128;
    // group A's chain trims (the switches above), the classic lpc 0 kernel alone
    static constexpr bool CARRY_HP = NEWFORM && SWN_CARRY_HP;
    static constexpr bool SWAP_ROWS = NEWFORM && SWN_SWAP_ROWS;
    static constexpr bool FLAT_EPI = NEWFORM && SWN_FLAT_EPILOGUE;
    static constexpr bool PLAIN_TAIL = NEWFORM && SWN_PLAIN_TAIL;
    // (FLAT_EPI) one dump word per thread of group A: where lanes p != 0 of a quad leave the hand-off value nobody reads
    static constexpr int o_dump = o_ho + (NEWFORM && (SWN_HANDOFF & 1) && SWN_ROTATE ? NHO * HO : 0);
    static constexpr int o_end = o_dump + (FLAT_EPI ? NG : 0);
    static constexpr size_t lds_bytes = (size_t)o_end * sizeof(float);
    static_assert(o_dump == o_wl + 8 * NG * 4 + 3 * H + (o_dump - o_ho) && (o_dump - o_ho == 0 || o_dump - o_ho == NHO * HO),
                  "the carve ends with group B's last-layer half, the three h0 copies and the hand-off ring");
    static_assert(o_end - o_dump == (FLAT_EPI ? NG : 0) && (!FLAT_EPI || o_dump + (NG - 1) == o_end - 1),
                  "one dump word per thread of group A, the last one the carve's last float");
    static_assert(o_dump % 4 == 0 && (size_t)o_end * sizeof(float) <= 160 * 1024, "16-byte carve, 160 KB of LDS");
    // per-utterance session of a streamed decode: the history rings, the older-tap products group B formed one step ahead
    // (both parities, as LDS holds them), then the sample window
    static constexpr int sess_old = ring_off(L);
    static constexpr int sess_win = sess_old + 2 * L * 2 * H;
    static constexpr int sess_floats = sess_win + r4(WN);
};
// the dump words are the classic lpc 0 kernel's alone: 39 308 floats of the parent's carve and 256 behind them
static_assert((SWN_HANDOFF & 1) || Tw<0, false>::o_dump == 39308, "classic lpc 0 carve");
static_assert((SWN_HANDOFF & 1) || !SWN_FLAT_EPILOGUE || Tw<0, false>::o_end == 39564, "classic lpc 0 carve with the dump words");
static_assert(Tw<0, true>::o_end == Tw<0, true>::o_dump && Tw<4, false>::o_end == Tw<4, false>::o_dump &&
              Tw<4, true>::o_end == Tw<4, true>::o_dump, "the other kernels keep the parent's carve");

// the sum over the wave's 16 quads, per position in the quad: lane hp of the first quad gets the sum of lanes hp + 4 n
// (the swaps in inline assembly, with the two wait states a VALU write needs before them: the compiler returns the builtins'
//  second result as a copy of the first)
__device__ __forceinline__ float sum_quads(float v) {
    v += dpp_f<0x124>(v);     // row_ror:4
    v += dpp_f<0x128>(v);     // row_ror:8: the row's four quads
    float w = v;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(v), "+v"(w));   // rows 0 + 1, 2 + 3
    v += w;
    w = v;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(v), "+v"(w));   // the two halves
    return v + w;
}
// two quad sums in the steps of one: every lane gives the partial `own` of the sum its parity keeps and the partial `other` of
// the sum its neighbour keeps; lanes 0 / 2 get the sum of the even lanes' `own` and the odd lanes' `other`, lanes 1 / 3 the other one
__device__ __forceinline__ float quad_sum_by_parity(float own, float other) {
    float s = own + dpp_f<0xB1>(other);     // quad_perm [1,0,3,2]: p0 + p1 | p2 + p3
    s += dpp_f<0x4E>(s);                    // quad_perm [2,3,0,1]
    return s;
}
// ---- group A: layer LAYER at position q - current tap, gate epilogue, hand-off.  Thread (o, p): rows o (gate) and o + 64
//      (candidate) over inputs 16 p .. 16 p + 15 of h_{l-1}(q), read from the row `xr`; lanes 0 / 1 of the quad finish the gate / the
//      candidate.  `po`: the offset of position q's parity in o_old, (q & 1) * L * 2 * H (the step loop forms it one step ahead).
//      `behind`: work that is not the chain's, issued behind the layer's first LDS reads - the epilogue operands and NQ of the four
//      input quads - and in front of their first use, so that it runs while the reads are on their way (the rotated step loop: the
//      previous step's stores, the refill test, the noise staging); the other quads are read behind it, under the first
//      quads' multiply-adds.  NoWork: the reads stay where the multiply-adds want them.
//      (NQ, one session, k samples/s of the headline beside the parent's 397.6: 0 quads early 398.7, one 403.1, two 403.9, three
//       401.8, all four 396.4 - every early quad holds four registers through the stores, and from three on a kernel spills)
struct NoWork { __device__ __forceinline__ void operator()() const {} };
//      Returns `hn` (lane p = 0 of the quad; with T::FLAT_EPI lanes p != 0 return a finite value nobody needs) and takes the
//      previous layer's as `hp_in`: with T::CARRY_HP it is the highway operand of layers 1 - 5 - the value this thread wrote to
//      the row `xr` one phase earlier.
template <class T, int LAYER, int NQ = 2, class BEHIND = NoWork>
__device__ __forceinline__ float layer_a(float* lds, const float (&w)[2][16], const int q, const float wj, const int pb, const int po,
                                         const int ta, const float* xr, const float hp_in, BEHIND&& behind = NoWork{}) {
    constexpr bool ROT = !std::is_same<typename std::decay<BEHIND>::type, NoWork>::value;
    const int o = ta >> 2, p = ta & 3, pr = p & 1;
    // epilogue operands first: their LDS latency hides under the FMAs
    const float e_old = lds[T::o_old + po + LAYER * 2 * H + pr * H + o];
    const float g_gp = lds[T::o_gp + pb + LAYER * 2 * H + pr * H + o], g_bx = lds[T::o_bx + LAYER * 2 * H + pr * H + o];
    const float e_hp = (T::CARRY_HP && LAYER >= 1) ? hp_in : xr[o];
    static_assert(NQ >= 0 && NQ <= 4, "early quads");
    float4 xq[4];
    if constexpr (ROT) {
#pragma unroll
        for (int m = 0; m < NQ; ++m) xq[m] = *reinterpret_cast<const float4*>(xr + 16 * p + 4 * m);
        __builtin_amdgcn_sched_barrier(0);
        behind();
        __builtin_amdgcn_sched_barrier(0);
    }
    const float e_gx = fmaf(wj, g_gp, g_bx);
    float az = 0.f, ac = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        float4 x;
        if (ROT && m < NQ) x = xq[m];
        else x = *reinterpret_cast<const float4*>(xr + 16 * p + 4 * m);
        az = fmaf(w[0][4 * m], x.x, az); ac = fmaf(w[1][4 * m], x.x, ac);
        az = fmaf(w[0][4 * m + 1], x.y, az); ac = fmaf(w[1][4 * m + 1], x.y, ac);
        az = fmaf(w[0][4 * m + 2], x.z, az); ac = fmaf(w[1][4 * m + 2], x.z, ac);
        az = fmaf(w[0][4 * m + 3], x.w, az); ac = fmaf(w[1][4 * m + 3], x.w, ac);
    }
    // the two quad sums transposed: a lane of even parity keeps its gate partial and hands over its candidate partial, a lane of
    // odd parity the reverse, so two DPP steps leave the gate sum in lanes 0 / 2 and the candidate sum in lanes 1 / 3 - each
    // associated (p0 + p1) + (p2 + p3) as sum4 forms it (bit-identical), without the select between two full sums
    // (T::SWAP_ROWS: lanes of odd parity hold the candidate row in w[0] and the gate row in w[1] - az is every lane's own partial)
    const float sq = T::SWAP_ROWS ? quad_sum_by_parity(az, ac) : quad_sum_by_parity(pr ? ac : az, pr ? az : ac);
    __builtin_amdgcn_sched_barrier(0);              // keep the gate epilogue behind the reduction
    float hn = 0.f;
    if constexpr (T::FLAT_EPI) {
        // all four lanes: lanes 2 / 3 hold the sums and the operands of lanes 0 / 1 (every index above goes by pr), so the same
        // line runs in them with no exec mask; lane 2 forms lane 0's hn again, lanes 1 / 3 something finite from the candidate.
        // Only the store is the lane's own: p = 0 writes the ring slot (the last layer o_hcat), the others their dump word
        const float sa = sq + e_old;
        const float v = e_gx * sa;
        const float e = exp_c(pr == 0 ? -v : -2.f * fminf(fabsf(v), 64.f));
        const float r = rcp_c(1.f + e);
        const float res = pr == 0 ? r : copysignf((1.f - e) * r, v);        // z | tanh
        const float c = dpp_f<0xF5>(res);                                  // quad_perm [1,1,3,3]: lanes 0 / 2 <- lanes 1 / 3
        hn = (1.f - res) * c + res * e_hp;
        constexpr int R2 = T::ring_len(LAYER + 1 < L ? LAYER + 1 : LAYER);
        const int dst = LAYER + 1 < L ? T::o_ring + T::ring_off(LAYER + 1 < L ? LAYER + 1 : LAYER) + (q & (R2 - 1)) * H + o
                                      : T::o_hcat + LAYER * H + o;
        static_assert(T::RINGX || !T::FLAT_EPI, "one hand-off store per layer");
        float* const own = lds + T::o_dump + ta;
        *(p == 0 ? lds + dst : own) = hn;
    } else
    if (p < 2) {
        const float sa = sq + e_old;
        const float v = e_gx * sa;
        // One straight-line epilogue, no branch around the transcendentals for a saturated tanh lane (tanh_c's |v| > 9.02 test:
        // the gate lanes never took it, so it saved no instruction and put a compare, an exec-mask save and a branch on the chain).
        // The result does not need it: for |v| > 9.02, e <= 1.5e-8 < 2^-25, so 1 + e, rcp_c(1), and 1 - e are all exactly 1 and
        // the line below returns copysign(1, v) - the parent's bits for every finite v.  The clamp at 64 changes no finite result
        // (e is already 0 in fp32 from |v| = 52) and keeps exp_c's correction term from becoming 0 * inf where v * log2(e)
        // overflows: |v| >= 1.18e38 and +-inf give +-1 as before.  A NaN pre-activation now gives +-1 in the candidate (v_min
        // drops it) where the parent passed it on; the gate lane of the same channel still passes its own.
        // (plain v_exp_f32 / v_rcp_f32 without the corrections - nine instructions fewer on the chain - measured the same step
        //  time: the phase waits for both groups, not for this arithmetic)
#ifdef SWN_DIAG_PLAINEXP
        const float e = __builtin_amdgcn_exp2f((p == 0 ? -v : -2.f * fminf(fabsf(v), 64.f)) * 1.44269504f);
        const float r = __builtin_amdgcn_rcpf(1.f + e);
#else
        const float e = exp_c(p == 0 ? -v : -2.f * fminf(fabsf(v), 64.f));
        const float r = rcp_c(1.f + e);
#endif
        const float res = p == 0 ? r : copysignf((1.f - e) * r, v);        // z | tanh
        const float c = dpp_f<0xF5>(res);                                  // quad_perm [1,1,3,3]: lane 0 <- lane 1
        if (p == 0) {
            hn = (1.f - res) * c + res * e_hp;
            if (LAYER + 1 < L) {
                constexpr int R2 = T::ring_len(LAYER + 1 < L ? LAYER + 1 : LAYER);
                lds[T::o_ring + T::ring_off(LAYER + 1 < L ? LAYER + 1 : LAYER) + (q & (R2 - 1)) * H + o] = hn;
            }
            // (RINGX: group B reads layers 0 - 4 from the ring slot just written; the last layer has no ring)
            if (!T::RINGX || LAYER + 1 >= L) lds[T::o_hcat + LAYER * H + o] = hn;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    return hn;
}

// ---- group B: older-tap product of layer LAYER for position qn = q + 1 (its operand h_{l-1}(qn - dil) is at least one step old),
//      bias added, left for group A in the buffer of qn's parity.  (MB: operands of at most MB of the four input quads in flight
//      at once - group A forms the last layer's product beside its 192 weight registers)
template <class T, int LAYER, int MB = 4>
__device__ __forceinline__ void older_sum(const float* lds, const float (&w)[2][16], const int qn, const int tb, float& az, float& ac) {
    constexpr int dil = 1 << LAYER;
    constexpr int R = T::ring_len(LAYER);
    const int p = tb & 3;
    const float* ring = lds + T::o_ring + T::ring_off(LAYER);
    az = 0.f; ac = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float4 x = *reinterpret_cast<const float4*>(ring + ((qn - dil) & (R - 1)) * H + 16 * p + 4 * m);
        float4 w0, w1;
        if (LAYER < L - 1) {
            w0 = make_float4(w[0][4 * m], w[0][4 * m + 1], w[0][4 * m + 2], w[0][4 * m + 3]);
            w1 = make_float4(w[1][4 * m], w[1][4 * m + 1], w[1][4 * m + 2], w[1][4 * m + 3]);
        } else {                                              // the last layer's half comes from LDS
            w0 = *reinterpret_cast<const float4*>(lds + T::o_wl + (m * NG + tb) * 4);
            w1 = *reinterpret_cast<const float4*>(lds + T::o_wl + ((4 + m) * NG + tb) * 4);
        }
        az = fmaf(w0.x, x.x, az); ac = fmaf(w1.x, x.x, ac);
        az = fmaf(w0.y, x.y, az); ac = fmaf(w1.y, x.y, ac);
        az = fmaf(w0.z, x.z, az); ac = fmaf(w1.z, x.z, ac);
        az = fmaf(w0.w, x.w, az); ac = fmaf(w1.w, x.w, ac);
        if (MB < 4 && m % MB == MB - 1) __builtin_amdgcn_sched_barrier(0);
    }
    az = sum4(az); ac = sum4(ac);
}
template <class T, int LAYER>
__device__ __forceinline__ void older_store(float* lds, const int qn, const int tb, const float az, const float ac) {
    const int o = tb >> 2, p = tb & 3, pr = p & 1;            // (called under p < 2)
    lds[T::o_old + (qn & 1) * (L * 2 * H) + LAYER * 2 * H + pr * H + o] = (p == 0 ? az : ac) + lds[T::o_bd + LAYER * 2 * H + pr * H + o];
}
template <class T, int LAYER, int MB = 4>
__device__ __forceinline__ void older_b(float* lds, const float (&w)[2][16], const int qn, const int tb) {
    float az, ac;
    older_sum<T, LAYER, MB>(lds, w, qn, tb, az, ac);
    if ((tb & 3) < 2) older_store<T, LAYER>(lds, qn, tb, az, ac);
}
// The last layer's product as group A forms it in skip-fin (older_b<T, L - 1, 2>), with the operands of input quads 0 and 1 - the
// ring row and group B's half of the matrix in o_wl, six 16-byte reads - requested a phase early (older_last_rows behind layer 5's
// hand-off write and in front of lds_barrier_keep<6>, older_last_x behind the barrier): h_4(qn - 32) is 31 steps old and o_wl is
// written once, so neither depends on that barrier.  Quads 2 and 3 are read as before; the order of the multiply-adds is older_sum's.
template <class T>
__device__ __forceinline__ void older_last_rows(const float* lds, const int qn, const int tb, float4 (&x)[2], float4 (&w)[2][2]) {
    constexpr int LAYER = L - 1, dil = 1 << LAYER, R = T::ring_len(LAYER);
    const float* row = lds + T::o_ring + T::ring_off(LAYER) + ((qn - dil) & (R - 1)) * H + 16 * (tb & 3);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        x[m] = *reinterpret_cast<const float4*>(row + 4 * m);
        w[m][0] = *reinterpret_cast<const float4*>(lds + T::o_wl + (m * NG + tb) * 4);
        w[m][1] = *reinterpret_cast<const float4*>(lds + T::o_wl + ((4 + m) * NG + tb) * 4);
    }
}
template <class T>
__device__ __forceinline__ void older_last_x(float* lds, const float4 (&xe)[2], const float4 (&we)[2][2], const int qn, const int tb) {
    constexpr int LAYER = L - 1, dil = 1 << LAYER, R = T::ring_len(LAYER);
    const float* row = lds + T::o_ring + T::ring_off(LAYER) + ((qn - dil) & (R - 1)) * H + 16 * (tb & 3);
    float az = 0.f, ac = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        float4 x, w0, w1;
        if (m < 2) { x = xe[m]; w0 = we[m][0]; w1 = we[m][1]; }
        else {
            x = *reinterpret_cast<const float4*>(row + 4 * m);
            w0 = *reinterpret_cast<const float4*>(lds + T::o_wl + (m * NG + tb) * 4);
            w1 = *reinterpret_cast<const float4*>(lds + T::o_wl + ((4 + m) * NG + tb) * 4);
        }
        az = fmaf(w0.x, x.x, az); ac = fmaf(w1.x, x.x, ac);
        az = fmaf(w0.y, x.y, az); ac = fmaf(w1.y, x.y, ac);
        az = fmaf(w0.z, x.z, az); ac = fmaf(w1.z, x.z, ac);
        az = fmaf(w0.w, x.w, az); ac = fmaf(w1.w, x.w, ac);
        if (m == 1) __builtin_amdgcn_sched_barrier(0);
    }
    az = sum4(az); ac = sum4(ac);
    if ((tb & 3) < 2) older_store<T, LAYER>(lds, qn, tb, az, ac);
}
// several layers at once: one basic block of independent chains (the stores' lane branch between them kept the scheduler from
// overlapping the products: 570 cycles each, one after the other)
template <int... LS> struct Layers {};
template <class T, int NW, int... LS>
__device__ __forceinline__ void older_bn(Layers<LS...>, float* lds, const float (&w)[NW][2][16], const int qn, const int tb) {
    static_assert(((LS < NW) && ...), "register-resident halves only");
    float az[sizeof...(LS)], ac[sizeof...(LS)];
    int k = 0;
    ((older_sum<T, LS>(lds, w[LS], qn, tb, az[k], ac[k]), ++k), ...);
    if ((tb & 3) < 2) {
        k = 0;
        ((older_store<T, LS>(lds, qn, tb, az[k], ac[k]), ++k), ...);
    }
}

// The same products with their operand rows requested a phase early (older_rows in front of lds_barrier_keep, older_bn_x behind
// it): the rows are at least one barrier old when they are requested, and behind the barrier the products are multiply-add chains
// with nothing to wait for.  The order of the multiply-adds inside each chain is older_sum's.
template <class T, int LAYER>
__device__ __forceinline__ void older_rows(const float* lds, const int qn, const int tb, float4 (&x)[4]) {
    constexpr int dil = 1 << LAYER;
    constexpr int R = T::ring_len(LAYER);
    const float* row = lds + T::o_ring + T::ring_off(LAYER) + ((qn - dil) & (R - 1)) * H + 16 * (tb & 3);
#pragma unroll
    for (int m = 0; m < 4; ++m) x[m] = *reinterpret_cast<const float4*>(row + 4 * m);
}
__device__ __forceinline__ void older_sum_x(const float (&w)[2][16], const float4 (&x)[4], float& az, float& ac) {
    az = 0.f; ac = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        az = fmaf(w[0][4 * m], x[m].x, az); ac = fmaf(w[1][4 * m], x[m].x, ac);
        az = fmaf(w[0][4 * m + 1], x[m].y, az); ac = fmaf(w[1][4 * m + 1], x[m].y, ac);
        az = fmaf(w[0][4 * m + 2], x[m].z, az); ac = fmaf(w[1][4 * m + 2], x[m].z, ac);
        az = fmaf(w[0][4 * m + 3], x[m].w, az); ac = fmaf(w[1][4 * m + 3], x[m].w, ac);
    }
    az = sum4(az); ac = sum4(ac);
}
template <class T, int... LS>
__device__ __forceinline__ void older_rows_n(Layers<LS...>, const float* lds, const int qn, const int tb, float4 (&x)[sizeof...(LS)][4]) {
    int k = 0;
    ((older_rows<T, LS>(lds, qn, tb, x[k]), ++k), ...);
}
template <class T, int NW, int... LS>
__device__ __forceinline__ void older_bn_x(Layers<LS...>, float* lds, const float (&w)[NW][2][16], const float4 (&x)[sizeof...(LS)][4],
                                           const int qn, const int tb) {
    static_assert(((LS < NW) && ...), "register-resident halves only");
    float az[sizeof...(LS)], ac[sizeof...(LS)];
    int k = 0;
    ((older_sum_x(w[LS], x[k], az[k], ac[k]), ++k), ...);
    if ((tb & 3) < 2) {
        k = 0;
        ((older_store<T, LS>(lds, qn, tb, az[k], ac[k]), ++k), ...);
    }
}

// ---- group B: out_skip, slice by slice.  Thread (r, hp): rows r and r + 64 over inputs 16 mm + 4 hp .. + 3 of the slice (the
//      lane-tiled global copy wsk2 of the symmetric kernel: 1 KiB contiguous per wave instruction); weights issued a phase ahead
//      (slice 0 whole, at the start of the step; the others by skip_roll_b).
// (`step0` is an opaque zero the caller renews every step: the addresses are loop-invariant, and hoisted out of the step loop the
//  six slices - 192 registers - would be kept resident beside the 160 weight registers)
template <int LAYER>
__device__ __forceinline__ void skip_issue_b(__amdgpu_buffer_rsrc_t wsk2, float4 (&wsl)[8], const int tb, const unsigned step0) {
    const int r = tb >> 2, hp = tb & 3;
#pragma unroll
    for (int ps = 0; ps < 2; ++ps)
#pragma unroll
        for (int mm = 0; mm < 4; ++mm)
            wsl[ps * 4 + mm] = buf_ld4(wsk2, (unsigned)((r + 64 * ps) * 4 + hp) * 16u, (unsigned)((LAYER * 4 + mm) * S) * 64u + step0);
}
// the rolling request of a layer phase: slice LAYER - 1 is consumed quarter by quarter (inputs 16 mm .., mm = 0 .. 3, both rows),
// and behind each quarter the same quarter of slice LAYER is requested into the two float4 it has just freed (a second buffer
// does not fit beside the 160 weight registers).  The four waves' 32 KB of requests then no longer queue at the end of the
// phase, in front of the barrier: the first quarter leaves behind the phase's first eight multiply-adds.  All four input quads are
// read at the head of the phase - the row o_hcat[LAYER - 1] is complete at the barrier -, so the phase pays one LDS round trip
// and no piece waits for a read issued behind the previous piece's requests.  The order of the multiply-adds inside each sacc
// chain is that of a whole-slice pass.
// (Measured per launch of 66 000 steps with the inputs read piece by piece, each pair of reads behind the previous piece's
//  requests: whole slice behind its consumption 208.0 ms, halves 188.5 ms, quarters 200.6 ms, eighths 226.1 ms - every extra
//  piece paid another exposed round trip.  In this build, one session: halves 175.5 ms and quarters 176.9 ms with the reads
//  piece by piece, quarters 166.2 ms and eighths - one row of one quad - 166.2 ms with the four reads at the head; in another
//  session, both without layer_a's transposed reduction: halves 172.5 ms, quarters 167.4 ms with the reads at the head.  DESIGN 3.1.)
// (`wcur`: the registers slice LAYER - 1 is consumed from, `wnext`: those slice LAYER is requested into - the same eight of the
//  rolling buffer, or, for a slice kept resident across the steps, the resident registers on one side of it: consumed and left
//  as they are, with the buffer free for the requests.  REQ false: the next slice is resident, nothing is requested)
// The request LEADS across the barrier (the classic lpc 0 kernel, T::LEAD loads): a slice's eight loads are numbered in request
// order, k = 2 mm + ps.  Phase L(LAYER) leaves the last DEFER of slice LAYER unrequested - their registers, freed by the
// phase's last multiply-adds, stay empty through the barrier - and requests at its own head, behind the four LDS reads and in
// front of the first multiply-add, the last HEAD of slice LAYER - 1, which phase L(LAYER - 1) left out: they are consumed last,
// three quarters of a phase later.  So the vector-memory path has work while the inputs' round trip keeps the multiply-adds
// waiting, and the end of the phase, in front of the barrier, issues nothing.  HEAD_OWN (L1 beside a resident slice 0: the rolling
// buffer is empty): the head requests the FIRST HEAD loads of slice LAYER itself.  Every request is issued and consumed inside
// one step, in the order of k, so vmcnt counts down as before and no prologue, chunk or pool primes anything.
// q: the position of the step; with T::RINGX the inputs h_{LAYER-1}(q) are read from ring LAYER's slot q & (R - 1), which group
// A wrote in front of the barrier and rewrites R steps later, not from o_hcat.
template <class T, int LAYER, bool REQ = true, int HEAD = 0, int DEFER = 0, bool HEAD_OWN = false>
__device__ __forceinline__ void skip_roll_b(const float* lds, __amdgpu_buffer_rsrc_t wsk2, float4 (&wcur)[8], float4 (&wnext)[8],
                                            float (&sacc)[2], const int tb, const unsigned step0, const int q SWN_TDEF_PARAM) {
    static_assert(LAYER >= 1 && LAYER < L, "slice LAYER - 1 in flight, slice LAYER to request");
    static_assert(HEAD >= 0 && HEAD <= 4 && DEFER >= 0 && DEFER <= 4, "at most half a slice leads");
    const int r = tb >> 2, hp = tb & 3;
    auto request = [&](float4 (&dst)[8], const int slice, const int k) __attribute__((always_inline)) {
        const int mm = k >> 1, ps = k & 1;
        dst[ps * 4 + mm] = buf_ld4(wsk2, (unsigned)((r + 64 * ps) * 4 + hp) * 16u, (unsigned)((slice * 4 + mm) * S) * 64u + step0);
    };
    constexpr int R = T::ring_len(LAYER);
    const float* xrow = T::RINGX ? lds + T::o_ring + T::ring_off(LAYER) + (q & (R - 1)) * H : lds + T::o_hcat + (LAYER - 1) * H;
    float4 xs[4];
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) xs[mm] = *reinterpret_cast<const float4*>(xrow + 16 * mm + 4 * hp);
    if constexpr (REQ && HEAD > 0) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < HEAD; ++k) {
            if (HEAD_OWN) request(wnext, LAYER, k);
            else request(wcur, LAYER - 1, 8 - HEAD + k);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
#ifdef SWN_STAMP
        if (!HEAD_OWN && HEAD > 0 && mm == (8 - HEAD) >> 1) {     // the wait for the first load requested at the head
            const unsigned long long t0 = __builtin_amdgcn_s_memtime();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("" :: "v"(wcur[((8 - HEAD) & 1) * 4 + mm].x));
            tdef += __builtin_amdgcn_s_memtime() - t0;
        }
#endif
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const float4 x = xs[mm], w = wcur[ps * 4 + mm];
            sacc[ps] = fmaf(w.x, x.x, sacc[ps]); sacc[ps] = fmaf(w.y, x.y, sacc[ps]);
            sacc[ps] = fmaf(w.z, x.z, sacc[ps]); sacc[ps] = fmaf(w.w, x.w, sacc[ps]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int k = 2 * mm + ps;
            if (REQ && k >= (HEAD_OWN ? HEAD : 0) && k < 8 - DEFER) request(wnext, LAYER, k);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // pin the partial sums to this phase: only the end of the step uses them, and the optimiser otherwise sinks all six slices'
    // multiply-adds down to that use - with their 48 operand registers per slice live until then (238 registers spilled)
    asm volatile("" : "+v"(sacc[0]), "+v"(sacc[1]));
}
// the last slice (the skip-fin phase, the only work left there): four independent 4-deep chains per row instead of one 16-deep
// one, then the quad sums of both rows in three DPP steps - lane 0 finishes row r, lane 2 row r + 64 - and the ReLU (the bias
// entered sacc with the first slice)
template <class T>
__device__ __forceinline__ void skip_last_b(float* lds, const float4 (&wsl)[8], const float (&sacc)[2], const int tb) {
    const int r = tb >> 2, hp = tb & 3;
    float part[2][4];
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
        const float4 x = *reinterpret_cast<const float4*>(lds + T::o_hcat + (L - 1) * H + 16 * mm + 4 * hp);
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const float4 w = wsl[ps * 4 + mm];
            part[ps][mm] = fmaf(w.w, x.w, fmaf(w.z, x.z, fmaf(w.y, x.y, w.x * x.x)));
        }
    }
    float s[2];
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) s[ps] = sacc[ps] + ((part[ps][0] + part[ps][1]) + (part[ps][2] + part[ps][3]));
    const float t0 = s[0] + dpp_f<0xB1>(s[0]), t1 = s[1] + dpp_f<0xB1>(s[1]);   // lanes 0, 1: hp 0 + 1; lanes 2, 3: hp 2 + 3
    const float v = (hp < 2 ? t0 : t1) + dpp_f<0x4E>(hp < 2 ? t1 : t0);        // lane 0 <- lane 2's half of row r, and back
    if ((hp & 1) == 0) lds[T::o_skip + r + 32 * hp] = fmaxf(v, 0.f);
}

// group B's five older-tap products of position q + 1 (layer 5's is group A's, in skip-fin): those it forms in the merged phase and
// those beside group A's out_1 (layer 0's operand is h0(q): not before the step's first barrier)
// (MOVE2, the classic lpc 0 kernel: layer 2's too sits in the merged phase, where group B has 600 cycles of slack - its operand
//  h_1(q - 3) is three steps old -, and skip-fin, where group B arrives last, requests the rows of two products, not three)
template <bool MOVE2> using OlderMergedT = typename std::conditional<MOVE2, Layers<2, 3, 4>, Layers<3, 4>>::type;
template <bool MOVE2> using OlderOut1T = typename std::conditional<MOVE2, Layers<0, 1>, Layers<0, 1, 2>>::type;
// the products beside out_1 whose rows are read in front of barrier 6 (E of them) and those read behind it
template <int E> struct Out1Split;
template <> struct Out1Split<2> { using Early = Layers<0, 1>; using Late = Layers<>; };
template <> struct Out1Split<1> { using Early = Layers<0>; using Late = Layers<1>; };
template <> struct Out1Split<0> { using Early = Layers<>; using Late = Layers<0, 1>; };

// The program of one group (GA: group A).  The two groups run the SAME sequence of barriers; they are separate instantiations -
// not one body with a run-time branch per phase - so that each has its own register allocation: as one body the allocation was the
// union (192 weight registers of A + the out_skip weights B keeps in flight: 22-65 registers spilled inside the step loop).
// STREAM (with EXT only): one chunk of a streamed decode (swn_decode_chunk) - steps [step0, step0 + n_steps) at absolute
// positions and generator counters, chunk-local out / heads / noise / forced rows.  When resuming, the rings, the sample
// window and the older-tap products of the first position (group B formed them during the previous chunk's last step)
// are loaded from the session - carried over bit for bit, not recomputed - and the prologue is skipped; the next input
// layer is then formed by the same input_gen as in the one-shot loop.  At the end all of it goes back to the session.
// POOL (with STREAM): one entry of a decode pool (swn_decode_pool_chunk); `a` already holds it as a batch-1 chunk, b = 0.  The
// noise staging and the frame boundaries follow the entry's own step0 and n_steps, so entries of one launch sit at any phase.
// PLAIN (T::PLAIN_TAIL, the one-shot launch): the caller gave no forced inputs - the tail has no forced load, wait or select,
// and the next input layer is formed behind the last step as well.
template <class T, bool GA, bool STREAM, bool POOL = false, bool PLAIN = false>
__device__ __forceinline__ void decode_body(const Bl6Args& a, float* lds) {
    static_assert(!PLAIN || (T::PLAIN_TAIL && !STREAM), "the one-shot classic lpc 0 kernel");
    constexpr bool EXT = T::EXT;
    static_assert(!STREAM || EXT, "streamed chunks run the extended mode");
    constexpr bool grpA = GA;
    const int tid = threadIdx.x, b = POOL ? 0 : blockIdx.x;
    __builtin_assume(GA ? tid < NG : tid >= NG);              // group B compiles none of group A's side jobs (head, noise, input layer)
    // (a raised s_setprio for group A - the chain first at the SIMD's issue arbitration - measured no gain: 283.6 / 278.8 / 282.9 k
    //  samples/s at priority 0 / 1 / 3)
    const int tg = tid & (NG - 1);                            // index inside the group
    const float* __restrict__ P = a.P;
    const int U = a.U;
    const int s0 = STREAM ? a.step0 : 0;                      // absolute index of step i = 0
    const bool resume = STREAM && a.resume;
    const int fb0 = STREAM ? s0 / U : 0;                      // conditioning frame of the first step (t = q - RF = step)

    // ---- one-time loads
    for (int e = tid; e < T::o_end; e += NT) lds[e] = 0.f;
    __syncthreads();
    for (int e = tid; e < L * 2 * H; e += NT) {
        lds[T::o_bx + e] = P[a.y.bx + e];
        const float bd = P[a.y.bd + e];
        lds[T::o_bd + e] = bd;
        lds[T::o_old + e] = bd;                               // position 0: the older tap reads the zero padding
    }
    for (int e = tid; e < U; e += NT) lds[T::o_wup + e] = P[a.y.wup + e];
    for (int e = tid; e < H; e += NT) lds[T::o_cz + e] = P[a.y.cb + e];
    for (int e = tid; e < S; e += NT) lds[T::o_bias + e] = P[a.y.bsk + e];
    for (int e = tid; e < O1; e += NT) lds[T::o_bias + S + e] = P[a.y.b1 + e];
    for (int e = tid; e < 2 * H; e += NT) { lds[T::o_cz + H + e] = P[a.y.cv + e]; lds[T::o_cz + 3 * H + e] = P[a.y.cc + e]; }
    for (int e = tid; e < T::NO * S; e += NT) lds[T::o_w2 + e] = P[a.y.w2 + (size_t)(e / S) * r4(S) + (e % S)];
    for (int e = tid; e < T::NO; e += NT) lds[T::o_w2 + T::NO * S + e] = P[a.y.b2 + e];
    for (int e = tid; e < 8 * O1 * 16; e += NT) lds[T::o_w1 + e] = P[a.y.w12 + e];
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
    // register-resident halves of the six matrices: group A tap 1 (current), group B tap 0 (older); rows (o, o + 64), inputs 16 p ..
    constexpr int NWR = grpA ? L : L - 1;                     // (group B's half of the last layer is in LDS)
    float wreg[NWR][2][16];
    {
        const int o = tg >> 2, p = tg & 3, k = grpA ? 1 : 0;
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                // (T::SWAP_ROWS: group A's lanes of odd p hold the candidate row as row 0 and the gate row as row 1, layer_a)
                const int rs = (grpA && T::SWAP_ROWS) ? r ^ (p & 1) : r;
                const float4* src = reinterpret_cast<const float4*>(P + a.y.wd + (((size_t)l * 2 * H + o + rs * H) * 2 + k) * H + 16 * p);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float4 t = src[v];
                    if (l == L - 1 && !grpA) {                // group B leaves its half of the last layer in LDS (group A reads it)
                        *reinterpret_cast<float4*>(lds + T::o_wl + ((r * 4 + v) * NG + tg) * 4) = t;
                    } else {
                        float (&wr)[16] = wreg[l < NWR ? l : 0][r];
                        wr[4 * v] = t.x; wr[4 * v + 1] = t.y; wr[4 * v + 2] = t.z; wr[4 * v + 3] = t.w;
                    }
                }
            }
    }
    __syncthreads();
    const float* sess_b = STREAM ? a.sess + (size_t)b * T::sess_floats : nullptr;
    // (the session copies index from an opaque copy of tid: sharing their addresses with the one-time loads above kept those
    //  registers live - spilled - across the step loop)
    int tcp = tid;
    asm volatile("" : "+v"(tcp));
    if (resume) {
        for (int e = tcp; e < T::ring_off(L); e += NT) lds[T::o_ring + e] = sess_b[e];
        for (int e = tcp; e < 2 * L * 2 * H; e += NT) lds[T::o_old + e] = sess_b[T::sess_old + e];
        __syncthreads();
    }

    int fb = fb0, tb0 = fb0 * U;              // base conditioning frame resident in buffer fb & 1
    const int n_pro = RF;                     // seed positions 0 .. rf - 1 (seg = 1)
    auto cond_taps = [&](int q, float& wj, int& pb) {
        const int t0 = q - RF;
        const int tlo = t0 < 0 ? 0 : t0;
        if (tlo >= tb0 + U) {                 // step crossed into the next frame: refill the free buffer
            fb += 1; tb0 += U;
            if (fb + 1 < a.Tf) load_frame(fb + 1);
        }
        int rel = tlo - tb0;
        int fsel = fb;
        if (rel >= U) { rel -= U; fsel = fb + 1; }
        rel = rel < U ? rel : U - 1;
        wj = lds[T::o_wup + rel];
        pb = (fsel & 1) * T::PF;
    };

    // input layer h0 = softsign(causal(lift(S)))  (wave 0).  Prologue: the seed samples are zero, only tap validity matters
    auto input_seed = [&](int q) {
        if (tid < H) {
            const int o = tid;
            float acc = c_b;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int r = q - (1 - k);
                if (r >= 0) acc += fmaf(k ? c_v1 : c_v0, 0.f, k ? c_c1 : c_c0);
            }
            lds[T::o_ring + (q & 1) * H + o] = ssign(acc);
        }
    };
    float win[T::WN];
#pragma unroll
    for (int k = 0; k < T::WN; ++k) win[k] = 0.f;
    if (EXT && a.seed) win[T::WN - 1] = reinterpret_cast<const float*>(a.seed)[b];
    if (resume) {
#pragma unroll
        for (int k = 0; k < T::WN; ++k) win[k] = sess_b[T::sess_win + k];
    }
    // Every wave of group A forms h0 of the next position itself (lane = channel, the same instructions on the same inputs: the four
    // copies agree bit for bit) and goes straight into layer 0 with it - no barrier between the sample and the first layer.  Wave 0's
    // copy is the layer-0 ring slot (group B's older tap and the session read it), waves 1-3 keep theirs at o_h0w.
    // (the five input-layer constants of the wave's channel stay in registers: the tail is a dependent chain)
    const int wv = __builtin_amdgcn_readfirstlane(tg >> 6);   // wave inside the group
    float kcb = 0.f, kv0 = 0.f, kv1 = 0.f, kc0 = 0.f, kc1 = 0.f;
    if (grpA) { const int o = tg & (H - 1); kcb = c_b; kv0 = c_v0; kv1 = c_v1; kc0 = c_c0; kc1 = c_c1; }
    auto h0_row = [&](int qn) -> int {                        // (float offset in LDS)
        return wv == 0 ? T::o_ring + (qn & 1) * H : T::o_h0w + (wv - 1) * H;
    };
    // `row`: h0_row of the position the window now ends in front of
    auto input_gen = [&](int row) {
        if constexpr (grpA) {
            float acc = kcb;
            acc += fmaf(kv0, win[T::WN - 2], kc0);
            acc += fmaf(kv1, win[T::WN - 1], kc1);
            lds[row + (tg & (H - 1))] = ssign(acc);
            // the row is read by the other lanes of this wave only, and LDS serves a wave's instructions in issue order: a read
            // issued behind the write returns the written data, no wait between them.  The clobber keeps the
            // compiler from moving the reads above the write
            lds_fence_compiler();
        }
    };
    // Group A's side work handed to group B (HOFF, diagnostic: not built, see SWN_HANDOFF): the stores of the sample and the heads,
    // the conditioning refill and the noise staging in group B's merged phase (below, at gen_step)
#ifdef SWN_DIAG_NOSIDE
    constexpr bool NOSIDE = T::NEWFORM;
#else
    constexpr bool NOSIDE = false;
#endif
#ifdef SWN_DIAG_NOSTREAM
    constexpr bool NOSTREAM = T::NEWFORM;
#else
    constexpr bool NOSTREAM = false;
#endif
    constexpr bool HOFF = T::NEWFORM && (SWN_HANDOFF & 7) && SWN_ROTATE;
    constexpr bool HO_ST = HOFF && (SWN_HANDOFF & 1), HO_RF = HOFF && (SWN_HANDOFF & 2), HO_NZ = HOFF && (SWN_HANDOFF & 4);
    constexpr bool MOVE2 = T::NEWFORM && SWN_OLDER2_MERGED;
    using OlderMerged = OlderMergedT<MOVE2>;
    using OlderOut1 = OlderOut1T<MOVE2>;
    constexpr int NOUT1 = MOVE2 ? 2 : 3;                      // products beside out_1 ...
    constexpr int NEARLY = MOVE2 ? SWN_EARLY_ROWS : NOUT1;    // ... and how many of them have their rows read in front of barrier 6
    static_assert(NEARLY >= 0 && NEARLY <= NOUT1, "early rows");
    // sampling noise staged off the chain (swn_decode_bl6.hip): wave 1 transforms tn = sign(e) log1p(-2|e|) of 64 steps at once
    // (lane = step) into a ring of NZB chunks, two chunks ahead of the tail that reads it.  Classic mode: the host-drawn deviate
    // of chunk c + 1 is requested behind the transform of chunk c and stays in a register until then, so the pass - which
    // stands at the head of a step, once per 64 steps - never waits for memory
    // (HO_NZ: the second wave of group B stages it, in its merged phase)
    constexpr bool NZG = HO_NZ ? !grpA : grpA;
    const int tn = HO_NZ ? tg : tid;
    float e_next = 0.f;
    auto noise_load = [&](int c) {
        const int step = c * T::NZC + tn - 64;
        if (step < a.n_steps) e_next = a.noise[(size_t)b * a.n_steps + step];
    };
    auto noise_chunk = [&](int c) {
        if (NZG && tn >= 64 && tn < 128) {
            const int k = tn - 64, step = c * T::NZC + k;
            if (step < a.n_steps) {
                const float e = EXT ? swn_noise_laplace_at(a.nz, b, step, s0 + step, 0, a.n_steps, 1) : e_next;
                const float sg = (e > 0.f) ? 1.f : ((e < 0.f) ? -1.f : 0.f);
                lds[T::o_tnz + (c & (T::NZB - 1)) * T::NZC + k] = sg * log1pf(-2.f * fabsf(e));
            }
            if (!EXT) noise_load(c + 1);
        }
    };
    if (!EXT && NZG && tn >= 64 && tn < 128) noise_load(0);
    noise_chunk(0);
    noise_chunk(1);

    const __amdgpu_buffer_rsrc_t wsk2 = make_rsrc(P + a.y.wsk2, (unsigned)(L * S * 64 * sizeof(float)));
    // One out_skip slice RESIDENT in group B, in the 32 registers it has left beside the 160 of its weights, the rolling slice
    // and the rows in flight: loaded once here (of a pool entry's own model: P is the entry's), consumed every step where
    // the rolling buffer would have held it, never rewritten.  Slice 0: the merged phase requests nothing and L1 consumes the
    // resident registers while it requests slice 1 into the empty buffer.  Slice 5: L5 requests nothing and skip-fin waits for no
    // load.  Either way the stream is 160 KB per step instead of 192.  (RES < 0: the parent's form, every slice streamed)
    // Slice 0 is built: in one session the headline ran 399.9 k samples/s with it, 394.2 with slice 5, 395.5 as the parent, and
    // slice 5 spills 2 - 8 registers in the chunk and pool kernels, slice 0 in none of the ten.
    // The classic lpc 0 kernel alone takes this form and the rotated loop below (NEWFORM): it is the one whose launch they shorten
    // (2.530 -> 2.492 us per step).  The extended kernels fit them without a spill and are SLOWER with them - a streamed chunk of
    // 220 steps 2.581 -> 2.603 us per step with the slice, 2.619 with the rotation, 2.643 with both, the one-shot extended decode
    // and the pool tick no faster - so they keep the parent's form; the classic lpc 4 kernel keeps it too.
    constexpr bool NEWFORM = T::NEWFORM;
    constexpr int RES = (grpA || !NEWFORM) ? -1 : SWN_RES_SLICE;
    static_assert(RES == -1 || RES == 0 || RES == L - 1, "the first or the last slice");
    // the rolling request leads beside a resident slice 0 only: L1 then finds the rolling buffer empty (skip_roll_b, HEAD_OWN)
    constexpr int LEADB = RES == 0 ? T::LEAD : 0;
    static_assert(LEADB == 0 || LEADB == 1 || LEADB == 2 || LEADB == 4, "one load, a quarter or a half of a slice");
    float4 wres[8];
    if constexpr (RES == 0) skip_issue_b<0>(wsk2, wres, tg, 0u);
    if constexpr (RES == L - 1) skip_issue_b<L - 1>(wsk2, wres, tg, 0u);

#ifdef SWN_STAMP
    // diagnostic build only (tools/stamp_decode_w.py): per phase, the cycles each group's first wave WORKS between two barriers
    // (barrier waits excluded) leave through the `heads` debug buffer: [0..8) group A (phase 0 = the previous step's tail + layer
    // 0), [8] the tail's share of phase 0, [9] A's whole step, [10..18) group B, [20..26) of group B's phases L1 .. L5 and
    // skip-fin the cycles from the barrier's release until the first out_skip weight register of the slice in flight has landed,
    // [30..39) group A's wave 1 as [0..9) (the wave that stages the sampling noise: the first wave's stamps do not see that work)
    // [44..49) of group B's phases L1 .. L5 the cycles it waits, in front of their first use, for the loads it requested at the
    // head of the phase (skip_roll_b; two s_memtime round trips included; L1 requests its own slice there and waits for nothing)
    unsigned long long tw[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tv[6] = {0, 0, 0, 0, 0, 0}, td[5] = {0, 0, 0, 0, 0}, tstep = 0, tlast = 0, tbeg = 0;
#define SWN_BAR(k) { tw[k] += __builtin_amdgcn_s_memtime() - tlast; lds_barrier(); tlast = __builtin_amdgcn_s_memtime(); }
    // (the empty asm uses the register, so the compiler places the vmcnt wait of the slice's oldest request in front of it)
#define SWN_WAIT_STAMP(k) { asm volatile("" :: "v"(wsl[0].x)); tv[k] += __builtin_amdgcn_s_memtime() - tlast; }
    // a barrier that leaves N early reads in flight (lds_barrier_keep): the phase's work ends at SWN_PRE, behind the hand-off
    // write and in front of the early reads - the stamp's s_memtime counts on lgkmcnt too and returns out of order, so it is
    // waited for (lgkmcnt(0)) before the first of them is issued.  Issuing them is then in neither phase's figure, and the s_memtime
    // behind the barrier makes the first use of an early read wait for all of them
#define SWN_PRE(k) { tw[k] += __builtin_amdgcn_s_memtime() - tlast; asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
#define SWN_BAR_KEEP(k, N) { lds_barrier_keep<N>(); tlast = __builtin_amdgcn_s_memtime(); }
#else
#define SWN_BAR(k) lds_barrier();
#define SWN_WAIT_STAMP(k)
#define SWN_PRE(k)
#define SWN_BAR_KEEP(k, N) lds_barrier_keep<N>();
#endif
    // one layer phase: group A runs the chain, group B prepares position q + 1 (and, during generation, accumulates out_skip)
    // (GEN: a generation step - group B's older-tap products for position q + 1 then sit in the merged and the out_1 phase, and
    //  layer 5's is group A's; in the prologue group B forms layer LAYER's in this phase.  X0: the row of h0(q) layer 0 reads)
#define SWN_PHASE_WORK(LAYER, GEN, X0)                                                                                \
    if constexpr (grpA) hcar = layer_a<T, LAYER>(lds, wreg[LAYER], q, wj, pb, po, tg,                                  \
                                                 LAYER == 0 ? (X0) : lds + T::o_ring + T::ring_off(LAYER) +            \
                                                                         (q & (T::ring_len(LAYER) - 1)) * H, hcar);    \
    else {                                                                                                             \
        if (GEN) {   /* slice 0 is requested whole at the start of the step; every later slice rolls in by quarters, behind    */ \
                     /* the multiply-adds that free its registers (both slices live at once are 64 registers beside the 160   */ \
                     /* of the weights)                                                                                       */ \
                     /* (a resident slice 0 is consumed in L1 from its own registers, a resident slice 5 is not requested in L5) */ \
            if (LAYER == 0) { if (RES != 0) skip_issue_b<0>(wsk2, wsl, tg, step0); }                                   \
                     /* (LEADB loads of every slice but the last lead across the barrier, skip_roll_b)                        */ \
            else if (LAYER == 1 && RES == 0)                                                                           \
                skip_roll_b<T, 1, !NOSTREAM, LEADB, LEADB, true>(lds, wsk2, wres, wsl, sacc, tg, step0, q SWN_TDEF_ARG(0)); \
            else { SWN_WAIT_STAMP(LAYER > 0 ? LAYER - 1 : 0)                                                           \
                   skip_roll_b<T, (LAYER > 0 ? LAYER : 1), !(LAYER == L - 1 && RES == L - 1) && !NOSTREAM,             \
                               (LAYER >= 2 ? LEADB : 0), (LAYER < L - 1 ? LEADB : 0)>(lds, wsk2, wsl, wsl, sacc, tg, step0, q \
                                                                                      SWN_TDEF_ARG(LAYER > 0 ? LAYER - 1 : 0)); } \
            __builtin_amdgcn_sched_barrier(0);                                                                         \
        }                                                                                                              \
        if (!(GEN)) older_b<T, LAYER>(lds, wreg[LAYER < NWR ? LAYER : 0], q + 1, tg);                                  \
        else if (LAYER == 0) older_bn<T>(OlderMerged{}, lds, wreg, q + 1, tg);                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
    }
#define SWN_PHASE(LAYER, GEN, X0) SWN_PHASE_WORK(LAYER, GEN, X0) if (GEN) { SWN_BAR(LAYER) } else lds_barrier();

    // ---- prologue: seed positions 0 .. rf - 1 (cswnv_shift1.py:321-334)
#pragma unroll 1
    for (int q = resume ? n_pro : 0; q < n_pro; ++q) {
        float wj; int pb;
        float4 wsl[8]; float sacc[2]; const unsigned step0 = 0;
        float hcar = 0.f;                     // group A: the layer's hn, the next layer's highway operand (layer_a)
        cond_taps(q, wj, pb);
        const int po = (q & 1) * (L * 2 * H);
        input_seed(q);
        lds_barrier();
        const float* x0 = lds + T::o_ring + (q & 1) * H;
        SWN_PHASE(0, false, x0) SWN_PHASE(1, false, x0) SWN_PHASE(2, false, x0) SWN_PHASE(3, false, x0)
        SWN_PHASE(4, false, x0) SWN_PHASE(5, false, x0)
        (void)wsl; (void)sacc; (void)step0; (void)hcar;
    }

    // ---- generation (cswnv_shift1.py:348-402).  Eight barriers per step: the first phase of step q is the tail of step q - 1
    //      (out_2, head, sample, h0(q) in every wave of group A) followed by layer 0 of step q.
    //      The chain runs from the sample through the input layer into layer 0's first LDS read, so nothing else stands there: the
    //      conditioning taps of step q (wj, pb), the parity offset of o_old and layer 0's row are formed one step AHEAD, in the
    //      tail of step q - 1 behind the reads it issues after barrier 7 (taps_ahead; in front of the loop for the first step - a
    //      resumed chunk and a pool entry prime them from their own step0 like the one-shot decode from 0), and the sample and
    //      heads stores come behind the input layer's write, or one step later behind layer 0's first reads (the rotated loop, below).  Generation steps advance by one, so the
    //      position in the frame is counted (rel_c; cond_taps' clamps never bind behind the prologue).  All of it is group A's:
    //      group B reads none of these values.
    //      The conditioning refill of a frame crossing stays in the first step of the new frame fb (rotated: behind layer 0's first
    //      reads, in front of the stores - its wait must not be for them), as one
    //      load - wait - write of group A's threads 0 .. PF / 4 - 1 behind the `fill_c` flag the look-ahead left: the buffer it
    //      fills was last read in layer 5 of the previous step, in front of its barrier 5, and the next reader comes U steps later
    //      (handed to group B and split into a request and a later write it was slower than the parent).
    int rel_c = s0 - fb0 * U;                 // position of the step in progress in its frame fb
    bool fill_c = false;                      // the step in progress is the first of its frame and frame fb + 1 exists (never the
                                              //  first step of a launch: the one-time loads above brought frames fb0 and fb0 + 1)
    float wj_c = 0.f;
    int pb_c = 0, po_c = 0, x0_c = 0;
    auto taps_ahead = [&](int qn) {           // what step qn reads, from the counters already advanced to it
        wj_c = lds[T::o_wup + rel_c];
        pb_c = (fb & 1) * T::PF;
        po_c = (qn & 1) * (L * 2 * H);
        x0_c = h0_row(qn);
        // formed here, not at their uses behind the sample
        asm volatile("" : "+s"(pb_c), "+s"(po_c), "+s"(x0_c));
    };
    auto frame_advance = [&]() {
        rel_c += 1;
        const bool cross = rel_c >= U;
        if (cross) { rel_c = 0; fb += 1; }
        fill_c = cross && fb + 1 < a.Tf;    // one scalar flag: the head of the step tests it and nothing else
    };
    if constexpr (grpA) taps_ahead(RF + s0);
    input_gen(x0_c);
#ifdef SWN_STAMP
    tlast = tbeg = __builtin_amdgcn_s_memtime();
#endif
    // Group A's loop ROTATED by the stores: the sample and the heads of step i wait in two registers (sv_p, acc_p) and are stored
    // in step i + 1, behind layer 0's LDS reads and in front of their first use - their lane branches and addresses, the refill
    // test and the noise staging with them -, so that between the input layer's write and those reads stands the loop's branch
    // alone.  The last step's stores follow the loop.  (ROT false: the parent's loop, stores behind the input layer's write)
    constexpr bool ROT = SWN_ROTATE && NEWFORM;
    constexpr int ROTQ = 2;                   // input quads of layer 0 read in front of the stores (layer_a)
    float sv_p = 0.f, acc_p = 0.f;
    // (rotated: through buffer resources over the utterance's rows - the step enters as a scalar offset, so the stores bring no
    //  64-bit address arithmetic into layer 0 and hold no address register beside its operands; without a heads buffer the
    //  resource is empty and the hardware drops the store)
    const __amdgpu_buffer_rsrc_t outr =
        make_rsrc(reinterpret_cast<float*>(a.out) + (size_t)b * a.n_steps, (unsigned)((size_t)a.n_steps * sizeof(float)));
    const __amdgpu_buffer_rsrc_t headr =
        make_rsrc(HEADS_ON && a.heads ? a.heads + (size_t)b * a.n_steps * T::NO : nullptr,
                  HEADS_ON && a.heads ? (unsigned)((size_t)a.n_steps * T::NO * sizeof(float)) : 0u);
    auto store_step = [&](const int ip) __attribute__((always_inline)) {
        if constexpr (grpA && ROT) {
            if (tid == 0) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, sv_p), outr, 0u, (unsigned)ip * 4u, 0);
            if (wv == 0 && (tg & 63) < T::NO)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc_p), headr, (unsigned)(tg & 63) * 4u,
                                                      (unsigned)(ip * T::NO) * 4u, 0);
        } else if constexpr (grpA) {
            if (tid == 0) reinterpret_cast<float*>(a.out)[(size_t)b * a.n_steps + (size_t)ip] = sv_p;
            if (HEADS_ON && a.heads && wv == 0 && (tg & 63) < T::NO) a.heads[((size_t)b * a.n_steps + ip) * T::NO + (tg & 63)] = acc_p;
        }
    };
    // HOFF - the hand-off (not built: SWN_HANDOFF = 0; measured and dropped): the sample and the NO head sums of
    // step i wait in sv_p / acc_p as in the rotated loop, and behind
    // layer 0's first reads of step i + 1 wave 0 of group A writes them to slot i & 127 of the ring o_ho - two LDS writes behind
    // one scalar branch, nothing else - and goes on.  Group B's first wave stores them 64 steps at a time (lane = step, one
    // dword of `out` and one dwordx2 of `heads` per lane): chunk c, steps 64 c .. 64 c + 63, in the merged phase of step
    // 64 c + 65 - its last slot was written in front of barrier 0 of step 64 c + 64, eight barriers earlier, and its half of the
    // ring is next written in step 64 c + 129.  What is left - at most 65 steps - is stored behind the loop, the last step's
    // slot write and a barrier.  (A store per step from group B cost 3.6 % of the launch: every wave of group B counts its
    // weight stream down with vmcnt, a store counts there too, and its acknowledgement takes longer than the two phases to the
    // next wait - group A's waves wait for no load.  Once per 64 steps that wait is nothing.)
    // Group B's threads also refill the conditioning (its own rel_c / fb / fill_c, advanced at the end of its step: the buffer
    // was last read in front of barrier 5 of the previous step, its next reader is U steps away) and its second wave stages
    // the noise (slot (i / 64 + 2) & 3, read from step 64 (i / 64 + 2) on), all in the merged phase.
    static_assert(!HOFF || (T::PF / 4 <= NG && T::NO == 2 && T::HO == 4), "one refill request per thread, a slot is {head, head, sample, -}");
    auto ho_write = [&](const int ip) __attribute__((always_inline)) {
        if constexpr (grpA) {
            // (every lane from NO - 1 on holds row NO - 1's sum and writes it to the same word: no lane branch)
            if (wv == 0) {
                float* const slot = lds + T::o_ho + (ip & (T::NHO - 1)) * T::HO;
                slot[(tg & 63) < T::NO ? (tg & 63) : T::NO - 1] = acc_p;
                slot[T::NO] = sv_p;
            }
        }
    };
    auto load_frame_b = [&](int fr) {
        if (tg < T::PF / 4)
            *reinterpret_cast<float4*>(lds + T::o_gp + (fr & 1) * T::PF + 4 * tg) =
                buf_ld4(condr, (unsigned)tg * 16u, (unsigned)(fr * a.N * 4));
    };
    auto store_chunk_b = [&](const int c) __attribute__((always_inline)) {
        const int step = c * 64 + tg;
        if (tg < 64 && step < a.n_steps) {
            const float4 v = *reinterpret_cast<const float4*>(lds + T::o_ho + (step & (T::NHO - 1)) * T::HO);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v.z), outr, (unsigned)tg * 4u, (unsigned)c * 256u, 0);
            using u2 = unsigned __attribute__((ext_vector_type(2)));
            u2 h; h.x = __builtin_bit_cast(unsigned, v.x); h.y = __builtin_bit_cast(unsigned, v.y);
            __builtin_amdgcn_raw_buffer_store_b64(h, headr, (unsigned)tg * 8u, (unsigned)c * 512u, 0);
        }
    };
    auto gen_step = [&](const int i) __attribute__((always_inline)) {
        const int q = RF + s0 + i;
        const float wj = wj_c;
        const int pb = pb_c, po = po_c;
        if constexpr (grpA && !ROT) {
            if (fill_c) load_frame(fb + 1);                       // first step of frame fb: refill the buffer the old frame left
        }
        // the rotated loop: what stood between the input layer's write and layer 0's first read - the stores of the previous
        // step, the staging of the sampling noise every 64th step, the refill test - goes behind layer 0's reads (layer_a)
        auto behind0 = [&]() __attribute__((always_inline)) {
            if constexpr (NOSIDE) return;
            if constexpr (!HO_NZ) { if ((i & (T::NZC - 1)) == 0) noise_chunk((i >> 6) + 2); }
            if constexpr (!HO_RF) { if (fill_c) load_frame(fb + 1); }
            if constexpr (HO_ST) { if (i > 0) ho_write(i - 1); }
            else { if (i > 0) store_step(i - 1); }
        };
        float4 wsl[8];
        float sacc[2] = {0.f, 0.f};
        float hcar = 0.f;                                     // group A: the layer's hn, the next layer's highway operand (layer_a)
        if constexpr (!grpA) {                                // the out_skip bias enters in lane 0 of each row's quad
            const float bs0 = lds[T::o_bias + (tg >> 2)], bs1 = lds[T::o_bias + (tg >> 2) + 64];
            if ((tg & 3) == 0) { sacc[0] = bs0; sacc[1] = bs1; }
        }
        unsigned step0 = 0;
        asm volatile("" : "+s"(step0));                       // opaque zero, see skip_issue_b
        const float* x0 = lds + x0_c;
        // group B's older-tap products of position q + 1 sit in the first phase (OlderMerged: no slice to consume yet, group A's
        // tail + layer 0 the longest phase) and in the out_1 phase (OlderOut1: group A runs out_1 alone; layer 0 needs h0(q), which
        // is not ready before the first barrier); all six beside the out_skip slices made group B take 1 050 cycles per layer phase
        // against group A's 710
#ifdef SWN_DIAG_NOSIDE_B
        constexpr bool SIDE_B = false;
#else
        constexpr bool SIDE_B = HOFF && !grpA && !NOSIDE;
#endif
        if constexpr (SIDE_B) {
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (HO_NZ) { if ((i & (T::NZC - 1)) == 0) noise_chunk((i >> 6) + 2); }
            if constexpr (HO_RF) { if (fill_c) load_frame_b(fb + 1); }   // (in front of the stores: its wait must not be for them)
            if constexpr (HO_ST) { if ((i & 63) == 1 && i > 1) store_chunk_b((i >> 6) - 1); }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (NOSTREAM && !grpA) {                        // (opaque contents: the multiply-adds stay)
#pragma unroll
            for (int k = 0; k < 8; ++k) asm volatile("" : "=v"(wsl[k].x), "=v"(wsl[k].y), "=v"(wsl[k].z), "=v"(wsl[k].w));
        }
        if constexpr (grpA && ROT) {
            hcar = layer_a<T, 0, ROTQ>(lds, wreg[0], q, wj, pb, po, tg, x0, hcar, behind0);
            SWN_BAR(0)
        } else {
            SWN_PHASE(0, true, x0)
        }
        SWN_PHASE(1, true, x0) SWN_PHASE(2, true, x0) SWN_PHASE(3, true, x0)
        SWN_PHASE(4, true, x0)
        // layer 5, and behind group A's hand-off write of it the first half of the operands of the product group A forms in
        // skip-fin (older_last_rows): they ride through barrier 5 in the registers layer 5 has freed.  lpc 0 only: with lpc 4 the
        // 24 registers spill (2 - 4 VGPRs, 12 bytes of scratch in all five lpc 4 kernels), and those keep the parent's form
        constexpr bool EARLY5 = T::LPC == 0;
        float4 xl[2], wl[2][2];
        SWN_PHASE_WORK(5, true, x0)
        if constexpr (grpA && EARLY5) {
            SWN_PRE(5)
            lds_fence_compiler();
            __builtin_amdgcn_sched_barrier(0);
            older_last_rows<T>(lds, q + 1, tg + (int)step0, xl, wl);   // (opaque zero: no address of it stays resident)
            __builtin_amdgcn_sched_barrier(0);
            SWN_BAR_KEEP(5, 6)
        } else {
            SWN_BAR(5)
        }
        // out_skip: the last slice and the reduction (group B).  Group A, otherwise idle here, forms layer 5's older-tap product of
        // position q + 1 from group B's half in LDS, with group B's thread-to-row mapping and summation order (bit-identical): its
        // operand h_4(q - 31) is 31 steps old, o_old[(q + 1) & 1][5] was last read in layer 5 of step q - 1 and is next read
        // in layer 5 of step q + 1, two barriers ahead of the end of the step (the session copy of a chunk's last step)
        // Both groups then request, behind their hand-off write of this phase and in front of barrier 6 (lds_barrier_keep), rows the out_1
        // phase reads that do not depend on that barrier.  Group B: the operand rows of OlderOut1, in wsl's registers and sixteen more -
        // all older than barrier 5, none rewritten before barrier 7 (hazard table).  Group A (lpc 0; with lpc 4 it has no
        // registers for it: 4 - 16 spilled): the out_1 weights of input blocks 0 and 1, both rows, in the working registers the product
        // has freed - o_w1 is written once, in front of the step loop.
        constexpr bool ROLL1 = T::LPC == 0;
        // (MOVE2: two products are left here; of those, Out1Split's Early have their rows requested in front of barrier 6 and the
        //  Late ones behind it, where group B's out_1 phase has over 300 cycles to expose them in)
        using Split = Out1Split<MOVE2 ? NEARLY : 2>;
        float4 xo[cmax(NEARLY, 1)][4];
        float4 w1e[2][2];
        if constexpr (!grpA) {
            if constexpr (RES == L - 1) skip_last_b<T>(lds, wres, sacc, tg);
            else { SWN_WAIT_STAMP(5) skip_last_b<T>(lds, wsl, sacc, tg); }
            SWN_PRE(6)
            lds_fence_compiler();
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!MOVE2) {
                older_rows_n<T>(OlderOut1{}, lds, q + 1, tg, xo);
                __builtin_amdgcn_sched_barrier(0);
                SWN_BAR_KEEP(6, 12)
            } else if constexpr (NEARLY > 0) {
                older_rows_n<T>(typename Split::Early{}, lds, q + 1, tg, xo);
                __builtin_amdgcn_sched_barrier(0);
                SWN_BAR_KEEP(6, 4 * NEARLY)
            } else {
                SWN_BAR_KEEP(6, 0)
            }
        } else {
            if constexpr (EARLY5) older_last_x<T>(lds, xl, wl, q + 1, tg + (int)step0);
            else older_b<T, L - 1, 2>(lds, wreg[L - 1], q + 1, tg + (int)step0);   // (opaque zero: no address of it stays resident)
            if constexpr (ROLL1) {
                SWN_PRE(6)
                lds_fence_compiler();
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                    for (int r = 0; r < 2; ++r)
                        w1e[mm][r] = *reinterpret_cast<const float4*>(lds + T::o_w1 + ((mm * O1 + (tg >> 2) + 64 * r) * 4 + (tg & 3)) * 4);
                __builtin_amdgcn_sched_barrier(0);
                SWN_BAR_KEEP(6, 4)
            } else {
                SWN_BAR(6)
            }
        }
        if constexpr (grpA) {
            // out_1, 128 x 128, LDS-resident, by group A alone: thread (hr, hp) rows hr and hr + 64 over inputs 16 mm + 4 hp .. + 3 - one
            // read of the inputs serves both rows.  Group B meanwhile forms three of the older-tap products of position q + 1 (with
            // all eight waves on out_1 the phase took 1 020 cycles, and the six products had to sit beside the out_skip slices)
            const int hr = tg >> 2, hp = tg & 3;
            float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
            auto X = [&](int mm) { return *reinterpret_cast<const float4*>(lds + T::o_skip + 16 * mm + 4 * hp); };
            auto W = [&](int mm, int r) { return *reinterpret_cast<const float4*>(lds + T::o_w1 + ((mm * O1 + hr + 64 * r) * 4 + hp) * 4); };
            auto fma8 = [&](int mm, const float4& x0, const float4& w0, const float4& w1) {
                float& acc = (mm & 1) ? a1 : a0;
                float& bcc = (mm & 1) ? b1 : b0;
                acc = fmaf(w0.x, x0.x, acc); acc = fmaf(w0.y, x0.y, acc); acc = fmaf(w0.z, x0.z, acc); acc = fmaf(w0.w, x0.w, acc);
                bcc = fmaf(w1.x, x0.x, bcc); bcc = fmaf(w1.y, x0.y, bcc); bcc = fmaf(w1.z, x0.z, bcc); bcc = fmaf(w1.w, x0.w, bcc);
            };
            float e_b1[2] = {0.f, 0.f}, e_w2[2] = {0.f, 0.f}, e_b2 = 0.f;     // (rolled loop only)
            const int e_kc = hp < T::NO ? hp : T::NO - 1;
            if constexpr (ROLL1) {
                // rolled: the weights one input block ahead, the inputs two, each into the registers a block's multiply-adds have just
                // freed (28 working registers hold two blocks of weights and three of inputs).  Left to the scheduler, the 24 reads
                // were waited for about eight times, each issued a few instructions before; with the weights of three blocks early and
                // the rest left to it, it read the inputs one block at a time behind lgkmcnt(0) (slower than the parent)
                // The epilogue's five constants - the two out_1 biases, this lane's out_2 column at both rows, b2; all written
                // once in front of the step loop - ride in the roll: blocks 5 and 6 request them into registers their
                // multiply-adds have freed (the inputs' last request leaves with block 4, the weights' with block 5), so the
                // reduction and the out_2 product find them landed instead of asking for them behind the last multiply-add
                static_assert(T::NO <= 4, "one round of out_2 rows");
                float4 xr[3] = {X(0), X(1), X(2)};
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mm = 0; mm < 8; ++mm) {
                    fma8(mm, xr[mm % 3], w1e[mm % 2][0], w1e[mm % 2][1]);
                    __builtin_amdgcn_sched_barrier(0);
                    if (mm + 2 < 8) { w1e[mm % 2][0] = W(mm + 2, 0); w1e[mm % 2][1] = W(mm + 2, 1); }
                    if (mm + 3 < 8) xr[mm % 3] = X(mm + 3);
                    if (mm == 5) {
                        e_b1[0] = lds[T::o_bias + S + hr]; e_b1[1] = lds[T::o_bias + S + hr + 64];
                        e_w2[0] = lds[T::o_w2 + e_kc * S + hr]; e_w2[1] = lds[T::o_w2 + e_kc * S + hr + 64];
                    }
                    if (mm == 6) e_b2 = lds[T::o_w2 + T::NO * S + e_kc];
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int mm = 0; mm < 8; ++mm) {
                    fma8(mm, X(mm), W(mm, 0), W(mm, 1));
                    if ((mm & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // at most four slices of operands live beside the 192 weight registers
                }
            }
            const float v = sum4(a0 + a1), u = sum4(b0 + b1);
            // out_2 of this wave's 32 out_1 rows, off the chain: lane hp of every quad takes out_2 rows hp and hp + 4, the wave sums
            // them (sum_quads) and its first quad leaves them in o_p2 for the tail; wave 0's lane 0 .. 3 carry b2
            if constexpr (ROLL1) {
                const float o1a = fmaxf(v + e_b1[0], 0.f), o1b = fmaxf(u + e_b1[1], 0.f);
                const float pz = sum_quads(fmaf(e_w2[1], o1b, fmaf(e_w2[0], o1a, tg < 4 ? e_b2 : 0.f)));
                if ((tg & 63) < 4 && hp < T::NO) lds[T::o_p2 + 4 * hp + wv] = pz;
            } else {
                const float o1a = fmaxf(v + lds[T::o_bias + S + hr], 0.f), o1b = fmaxf(u + lds[T::o_bias + S + hr + 64], 0.f);
#pragma unroll
                for (int j = 0; j < (T::NO + 3) / 4; ++j) {
                    const int k = hp + 4 * j, kc = k < T::NO ? k : T::NO - 1;
                    const float* w2 = lds + T::o_w2 + kc * S;
                    const float b2 = lds[T::o_w2 + T::NO * S + kc];
                    const float pz = sum_quads(fmaf(w2[hr + 64], o1b, fmaf(w2[hr], o1a, tg < 4 ? b2 : 0.f)));
                    if ((tg & 63) < 4 && k < T::NO) lds[T::o_p2 + 4 * k + wv] = pz;
                }
            }
        } else if constexpr (!MOVE2) {
            older_bn_x<T>(OlderOut1{}, lds, wreg, xo, q + 1, tg);
        } else {
            if constexpr (NEARLY > 0) older_bn_x<T>(typename Split::Early{}, lds, wreg, xo, q + 1, tg);
            if constexpr (NEARLY < NOUT1) older_bn<T>(typename Split::Late{}, lds, wreg, q + 1, tg);
        }
        SWN_BAR(7)
        if constexpr (grpA) {
            // out_2 (NO <= 6 rows): the four waves' partial sums from the out_1 phase, added in one fixed order - all four waves form
            // the same sample; then the Laplace head, evaluated uniformly by every lane of every wave of group A so that the new sample
            // is in registers for the next input layer (cswnv_shift1.py:368-391).  Only wave 0 stores the heads and the sample.
            const int ln = tg & 63;
            // the deviate (classic mode) and the forced sample are requested first: the deviate's LDS latency then hides under
            // the partials' read, and the forced load is older than this step's stores - waiting for it must not wait for them
            // (vmcnt counts stores too)
            float tz = 0.f;                                // (an early read in the extended mode spilled four registers)
            if constexpr (!EXT) tz = lds[T::o_tnz + (i & (T::NZB * T::NZC - 1))];
            float fv = 0.f;
            const bool forced_on = !PLAIN && a.forced;
            if (forced_on) fv = reinterpret_cast<const float*>(a.forced)[(size_t)b * a.n_steps + i];
            const float4 pz = *reinterpret_cast<const float4*>(lds + T::o_p2 + 4 * (ln < T::NO ? ln : T::NO - 1));
            // step q + 1's taps, row and offsets while the partials are on their way: wj's read joins the batch waited for here,
            // and nothing of this is left to do between the sample and layer 0
            __builtin_amdgcn_sched_barrier(0);
            frame_advance();
            taps_ahead(q + 1);
            __builtin_amdgcn_sched_barrier(0);
            const float acc = (pz.x + pz.y) + (pz.z + pz.w);   // lane k < NO: out_2 row k
            // the NO head outputs sit in lanes 0 .. NO - 1: broadcast them through scalar registers (an LDS write, a wave barrier and
            // a broadcast read stood here: ~150 cycles of the chain the whole workgroup waits for)
            float o2[T::NO];
#pragma unroll
            for (int k = 0; k < T::NO; ++k) o2[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, acc), k));
            float sv;
            {
#pragma clang fp contract(off)
                const float mu = o2[0];
                const float bsc = sigm(o2[1]);                 // exp(logsigmoid(y))
                float lpv = 0.f;
#pragma unroll
                for (int k = 0; k < T::LPC; ++k) lpv += o2[2 + T::LPC - 1 - k] * win[T::WN - T::LPC + k];
                const float t = bsc * (EXT ? lds[T::o_tnz + ((i >> 6) & (T::NZB - 1)) * T::NZC + (i & (T::NZC - 1))] : tz);
                sv = (T::LPC > 0) ? (lpv + mu) - t : mu - t;
                sv = fminf(fmaxf(sv, -1.f), 1.f);
                // the window is updated and the next input layer formed BEFORE the sample and the heads are stored: the stores, their
                // lane branches and addresses are not on the chain, and a use of the forced load behind a conditional store would
                // wait for the stores themselves (it compiles to vmcnt(0)); the forced load stays older than every store of its step
                float fd = forced_on ? fv : sv;
                asm volatile("" : "+v"(fd));
#pragma unroll
                for (int k = 0; k + 1 < T::WN; ++k) win[k] = win[k + 1];
                win[T::WN - 1] = fd;
            }
            // (PLAIN: behind the last step too - the row exists, nobody reads it, and the test leaves the chain)
            if (PLAIN || i + 1 < a.n_steps) input_gen(x0_c);
            __builtin_amdgcn_sched_barrier(0);                 // the stores stay behind the input layer's write
            if constexpr (ROT) { sv_p = sv; acc_p = acc; }
            else {
                if (tid == 0) reinterpret_cast<float*>(a.out)[(size_t)b * a.n_steps + (size_t)i] = sv;
                if (HEADS_ON && a.heads && wv == 0 && ln < T::NO) a.heads[((size_t)b * a.n_steps + i) * T::NO + ln] = acc;
            }
        }
        if constexpr (HO_RF && !grpA) frame_advance();          // group B's own counters, for its refill test of step i + 1
#ifdef SWN_STAMP
        if constexpr (grpA) tw[8] += __builtin_amdgcn_s_memtime() - tlast;
#endif
    };
    if constexpr (ROT) {
        // one flat loop (the noise staging of every 64th step sits in layer 0 with the stores), and the last step's stores behind
        // it - in front of the session copy's barrier
#pragma unroll 1
        for (int i = 0; i < a.n_steps; ++i) gen_step(i);
        if constexpr (HO_ST) {
            // the chunks the loop has not stored (it stored chunk c in step 64 c + 65)
            if constexpr (grpA) { if (a.n_steps > 0) ho_write(a.n_steps - 1); }
            lds_barrier();
            if constexpr (!grpA) {
                for (int c = a.n_steps >= 66 ? ((a.n_steps - 66) >> 6) + 1 : 0; c * 64 < a.n_steps; ++c) store_chunk_b(c);
            }
        } else if (a.n_steps > 0) store_step(a.n_steps - 1);
    } else {
#pragma unroll 1
        for (int i0 = 0; i0 < a.n_steps; i0 += T::NZC) {
            noise_chunk((i0 >> 6) + 2);
            const int iend = i0 + T::NZC < a.n_steps ? i0 + T::NZC : a.n_steps;
#pragma unroll 1
            for (int i = i0; i < iend; ++i) gen_step(i);
        }
    }
#ifdef SWN_STAMP
    { const unsigned long long tn = __builtin_amdgcn_s_memtime(); tw[0] += tn - tlast; tstep = tn - tbeg; }
#endif
    if constexpr (STREAM) {    // the state the next chunk resumes from (all LDS writes of the last step are behind barriers)
        __syncthreads();
        float* so = a.sess + (size_t)b * T::sess_floats;
        tcp = tid;
        asm volatile("" : "+v"(tcp));
        for (int e = tcp; e < T::ring_off(L); e += NT) so[e] = lds[T::o_ring + e];
        for (int e = tcp; e < 2 * L * 2 * H; e += NT) so[T::sess_old + e] = lds[T::o_old + e];
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < T::WN; ++k) so[T::sess_win + k] = win[k];
        }
    }
#undef SWN_PHASE
#undef SWN_PHASE_WORK
#undef SWN_BAR
#undef SWN_WAIT_STAMP
#undef SWN_PRE
#undef SWN_BAR_KEEP
#ifdef SWN_STAMP
    if ((tid == 0 || tid == 64 || tid == NG) && b == 0 && a.heads) {
        float* h = a.heads + (tid == 0 ? 0 : tid == 64 ? 30 : 10);
        for (int k = 0; k < 9; ++k) h[k] = (float)((double)tw[k] / (double)a.n_steps);
        if (tid == 0) h[9] = (float)((double)tstep / (double)a.n_steps);
        else if (tid == NG) {
            for (int k = 0; k < 6; ++k) h[10 + k] = (float)((double)tv[k] / (double)a.n_steps);
            for (int k = 0; k < 5; ++k) h[34 + k] = (float)((double)td[k] / (double)a.n_steps);
        }
    }
#endif
}

template <class T, bool STREAM = false, bool PLAIN = false>
__global__ __launch_bounds__(NT) void decode_bl6w_kernel(const Bl6Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (threadIdx.x < NG) decode_body<T, true, STREAM, false, PLAIN>(a, lds);       // wave-uniform
    else decode_body<T, false, STREAM, false, PLAIN>(a, lds);
}

// MODELS: the entry's weights are those of its model (SwnPoolModels)
template <class T, bool MODELS = false>
__global__ __launch_bounds__(NT) void decode_bl6w_pool_kernel(
    const typename std::conditional<MODELS, Bl6PoolModelsArgs, Bl6PoolArgs>::type p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    static_assert(T::EXT, "pools run the extended mode");
    Bl6Args a = p.c;
    if constexpr (MODELS) a.P = swn_pool_model(p.m);
    if (!swn_pool_entry_args(a, p.t, 1, 1, T::NO)) return;
    a.sess += (size_t)swn_pool_slot(p.t) * T::sess_floats;
    if (threadIdx.x < NG) decode_body<T, true, true, true>(a, lds);   // wave-uniform
    else decode_body<T, false, true, true>(a, lds);
}

// ... of a wide launch (swn_decode_pool_chunk_wide): the entry and its model's packed buffer are row blockIdx.x of the device table
template <class T>
__global__ __launch_bounds__(NT) void decode_bl6w_pool_wide_kernel(const Bl6PoolWideArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    static_assert(T::EXT, "pools run the extended mode");
    Bl6Args a = p.c;
    const SwnPoolWideRow row = swn_pool_wide_row(p.rows);
    a.P = row.model;
    if (!swn_pool_entry_args(a, row.e, 1, 1, T::NO)) return;
    a.sess += (size_t)row.e.slot * T::sess_floats;
    if (threadIdx.x < NG) decode_body<T, true, true, true>(a, lds);   // wave-uniform
    else decode_body<T, false, true, true>(a, lds);
}

bool bl6w_applies(const SwnGeom& g) {
    return g.bl6 && g.U <= 256 && g.U >= 2 && !g.audio_in && g.kind == SWN_KIND_LAPLACE && g.S == 128 && g.O1 == 128 &&
           g.seg == 1 && (g.lpc == 0 || g.lpc == 4);
}

// the instantiation a geometry runs: f(Tw<lpc, false>{}) for a single-sample Laplace net of the BL6 class, SWN_E_UNSUPPORTED
// otherwise (the symmetric kernel, swn_decode_bl6.hip, takes the others)
template <class F>
int with_tw(const SwnGeom& g, F&& f) {
    if (!bl6w_applies(g)) return SWN_E_UNSUPPORTED;
    if (g.lpc == 0) return f(Tw<0, false>{});
    return f(Tw<4, false>{});
}

}  // namespace

// a checked call on the wave-specialised kernel (swn_decode.hip): a pool launch over the checked entry table (one workgroup
// per entry, sessions [capacity][sess_floats]), a streamed chunk (`sess` holds sess_floats per utterance) or the one-shot decode
int swn_decode_bl6w_run(const SwnDecodeCall& c) {
    const hipStream_t st = c.hip_stream;
    if (c.wide) {
        Bl6PoolWideArgs p;
        fill_args(p.c, c);
        p.rows = c.wide;
        return with_tw(c.g, [&](auto tw) {
            using T = typename decltype(tw)::Ext;
            return launch_kernel(decode_bl6w_pool_wide_kernel<T>, T::lds_bytes, c.batch, p, st, "swn_decode_pool_chunk_wide(bl6w)");
        });
    }
    if (c.pool) {
        Bl6PoolModelsArgs p;
        fill_args(p.c, c);
        p.t = *c.pool;
        if (c.models) p.m = *c.models;
        return with_tw(c.g, [&](auto tw) {
            using T = typename decltype(tw)::Ext;
            if (c.models)
                return launch_kernel(decode_bl6w_pool_kernel<T, true>, T::lds_bytes, c.batch, p, st, "swn_decode_pool_chunk_models(bl6w)");
            const Bl6PoolArgs& p1 = p;
            return launch_kernel(decode_bl6w_pool_kernel<T>, T::lds_bytes, c.batch, p1, st, "swn_decode_pool_chunk(bl6w)");
        });
    }
    Bl6Args a;
    fill_args(a, c);
    return with_tw(c.g, [&](auto t) {
        using T = decltype(t);
        using X = typename T::Ext;
        static_assert(T::lds_bytes <= 160 * 1024 && X::lds_bytes <= 160 * 1024, "LDS budget");
        if (c.stream) return launch_kernel(decode_bl6w_kernel<X, true>, X::lds_bytes, a.B, a, st, "swn_decode(bl6w)");
        if (wants_ext(a)) return launch_kernel(decode_bl6w_kernel<X>, X::lds_bytes, a.B, a, st, "swn_decode(bl6w)");
        // (T::PLAIN_TAIL: without forced inputs the copy whose tail has none of their instructions)
        if constexpr (T::PLAIN_TAIL) {
            if (!a.forced) return launch_kernel(decode_bl6w_kernel<T, false, true>, T::lds_bytes, a.B, a, st, "swn_decode(bl6w)");
        }
        return launch_kernel(decode_bl6w_kernel<T>, T::lds_bytes, a.B, a, st, "swn_decode(bl6w)");
    });
}

// streamed decode (swn_decode_chunk): per-utterance session floats of the wave-specialised kernel, 0 = it does not apply
// bytes of dynamic LDS a launch of the wave-specialised kernel takes (classic or extended instantiation), 0 = it does not apply
size_t swn_decode_bl6w_lds(const SwnGeom& g, bool extended) {
    size_t n = 0;
    with_tw(g, [&](auto t) {
        using T = decltype(t);
        n = extended ? T::Ext::lds_bytes : T::lds_bytes;
        return SWN_OK;
    });
    return n;
}
extern "C" size_t swn_decode_bl6w_lds_bytes(const swn_net_desc* d, int extended) {
    SwnGeom g;
    if (swn_make_geom(d, &g) < 0) return 0;
    return swn_decode_bl6w_lds(g, extended != 0);
}

size_t swn_decode_bl6w_session_floats(const SwnGeom& g) {
    int n = 0;
    with_tw(g, [&](auto t) { n = decltype(t)::sess_floats; return SWN_OK; });
    return (size_t)n;
}
