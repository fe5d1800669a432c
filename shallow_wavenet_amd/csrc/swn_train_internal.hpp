// Library-internal interface of the training translation units (swn_stack.hip, swn_stack_bf16.hip, swn_stack_bf16g.hip,
// swn_train.hip, swn_bwd_bl6.hip): the functions they call across files, each declared once, and the LAYOUT of every work
// buffer the training calls exchange with the host.  A size query returns its layout's `total`, a call forms its pointers
// as base + member of the same layout: where a section sits is decided here and nowhere else.  Host code only; every
// layout function is plain arithmetic (no device calls).  The functions have C++ linkage, so a declaration that drifted
// from its definition does not link.
#pragma once
#include <hip/hip_runtime.h>
#include "swn_geom.hpp"

// ---- cross-file functions ------------------------------------------------------------------------------------------------
// swn_stack.hip: may the dropout-mode forward of the mixed-precision mode run on the bf16 time-major GEMM stack?  (the
// geometry class of swn_stack_bf16g.hip, its 32-bit operand offsets, a sequence long enough for the bf16-copy contractions)
bool swn_drop_g16(const swn_net_desc* d, int batch, long Tp);

// swn_train.hip, through its contraction kernels in the arithmetic `bf16` (mixed precision) or exact fp32.  relu(skip),
// relu(out_1) from the hidden states in `work` (SwnFwdLayout); the gated layers of the dropout-mode forward in the
// mixed-precision mode (layer l's pre-activations kept at a_scr + l * a_stride); the sample-rate in_x of every layer over
// the masked conditioning
int swn_train_head_acts(const SwnGeom& g, const float* packed, float* work, int batch, long Tp, bool bf16, hipStream_t st);
int swn_train_layers_forward_drop(const SwnGeom& g, const SwnLayout& y, const float* packed, const void* audio, const float* gx,
                                  const float* const* drop_h, float* hs, float* a_scr, size_t a_stride, float* hmask, int B,
                                  int n_frames, int Tp, hipStream_t st);
int swn_train_inx_forward(const SwnGeom& g, const SwnLayout& y, const float* packed, const float* xm, float* gx,
                          int B, int Tx, int Tp, bool bf16, hipStream_t st, unsigned short* wx16, bool g4);

// swn_stack_bf16g.hip: the tiled bf16 GEMM stack of the large geometries (H a multiple of 64 beyond the BL6 class)
int swn_bf16g_geom(const swn_net_desc* d, SwnGeom* g);
size_t swn_bf16g_weight_bytes(const SwnGeom& g);
int swn_bf16g_pack(const SwnGeom& g, const float* packed, void* wbf, hipStream_t st);
int swn_bf16g_expand(const SwnGeom& g, const void* work, int batch, long Tp, float* fwd_work, bool hs_only, hipStream_t st);
int swn_bf16g_forward(const SwnGeom& g, const float* packed, const void* wbf, const float* cond, const void* audio,
                      int batch, int n_frames, void* work, float* out, hipStream_t st, float* a_keep = nullptr,
                      const float* gx = nullptr, const float* const* drop_h = nullptr, unsigned short* hm16 = nullptr);
int swn_bf16g_plain(const unsigned short* A, int M, const unsigned short* src, size_t blk_stride, size_t src_bytes, int KB, int nblk,
                    int Tp, int B, const float* bias, unsigned short* out_bf, int out_ld, float* out_f, int NO, hipStream_t st);

// swn_stack_bf16.hip: BL6 class, mixed-precision mode, dropout as run.sh trains it (dilation_repeat == 1: the only
// hidden-state mask lands on the last layer's output, which feeds nothing, so aux_drop is the one mask that acts -
// cswnv_shift1.py:194-195,211-217): the fused path.  Its forward work buffer (read back by swn_bl6_bwd_stack), byte
// offsets, every section 256-byte aligned:
struct SwnBl6DropLayout {
    size_t hs16;       // [L+1][B][Tp][64] bf16 hidden states, time-major
    size_t wbf;        // fragment-ordered bf16 weights of the layer / head kernels (swn_pack_bf16's image)
    size_t wx16;       // [L*128][A0x] bf16: in_x matrices, zero columns A0..A0x
    size_t xm16;       // [B][Tx][A0x] bf16: masked, upsampled conditioning, time-major
    size_t gx16;       // [B][Tp][L*128] bf16: sample-rate in_x products, bias included
    size_t total;
};
bool swn_bl6_drop_supported(const SwnGeom& g, int B, long Tp, int n_frames, const float* const* drop_h);
SwnBl6DropLayout swn_bl6_drop_layout(const SwnGeom& g, int B, long Tp);
int swn_bl6_drop_forward(const SwnGeom& g, const float* packed, const float* C, const float* audio, const float* drop_x,
                         int batch, int n_frames, void* work, float* out, hipStream_t st);

// swn_bwd_bl6.hip: fused per-layer backward of the BL6 class in the mixed-precision mode.  The inside of its scratch is that
// file's own; drop: + the sections of the dropout mode
bool swn_bl6_bwd_supported(const SwnGeom& g, int B, long Tp, int n_frames);
size_t swn_bl6_bwd_scratch_bytes(const SwnGeom& g, int B, long Tp, bool drop);
int swn_bl6_bwd_stack(const SwnGeom& g, const SwnLayout& y, const float* packed, const float* cond, const float* audio,
                      const void* hs_bf16, const float* grad_out, float* dcond, float* gpacked, void* scratch, int B, int n_frames,
                      long Tp, hipStream_t st, const unsigned short* gx16, const unsigned short* xm16, unsigned short* dxm16);

// ---- lengths of one call ---------------------------------------------------------------------------------------------------
// T samples; Tp teacher-forced positions; Tx positions of the sample-rate conditioning, which starts coff samples in.
// (softmax nets have seg == 1, swn_make_geom: Tp = T - 1 and coff = 1 are the same expressions.)  Tp < 1: the size queries
// answer 0, the calls SWN_E_BADARG.
struct SwnTrainLen { long T, Tp, Tx; int coff; };
static inline SwnTrainLen swn_train_len(const SwnGeom& g, int n_frames) {
    SwnTrainLen n;
    n.T = (long)n_frames * g.U;
    n.coff = g.seg;
    n.Tp = n.T - 2 * g.seg + 1;
    n.Tx = n.T - n.coff;
    return n;
}

// ---- work-buffer layouts ---------------------------------------------------------------------------------------------------
// Sections are rounded with swn_al (64 floats) in float buffers and swn_al256 in byte buffers: 256 bytes either way.
static inline size_t swn_al256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline size_t swn_al_bytes(size_t bytes) { return swn_al((bytes + 3) / 4); }     // a byte-sized section of a float buffer

constexpr int SWN_WUP_COPIES = 16;      // partial upsampler-tap gradients of cond_bwd_kernel (wup_fold_kernel, swn_train.hip)
static inline long swn_da16_pitch(long Tp) { return (Tp + 2 + 31) & ~31L; }      // bf16 rows of the backward's da / d gx / h copies

// swn_frontend's activation buffer (fe_work; swn_frontend.hip writes it in this order, unrounded): float offsets
struct SwnFeLayout {
    size_t act[SWN_MAXAUX + 1];      // [0] scale_in's output (B, n_aux, Tf), [i + 1] conv_aux layer i's (B, aux_cout[i], Tf)
    size_t C;                        // = act[auxl]: the conditioning C (B, A0, Tf) that in_x reads
    size_t total;
};
static inline SwnFeLayout swn_fe_layout(const SwnGeom& g, int B, int n_frames) {
    SwnFeLayout o{};
    const size_t bt = (size_t)B * n_frames;
    size_t p = bt * g.n_aux;
    for (int i = 0; i < g.auxl; ++i) { o.act[i + 1] = p; p += bt * g.aux_cout[i]; }
    o.C = o.act[g.auxl];
    o.total = p;
    return o;
}

// slot of one layer's gate pre-activations (B, 2H, Tp) fp32 wherever a forward keeps them for its backward
static inline size_t swn_keep_stride(const SwnGeom& g, int B, long Tp) { return swn_al((size_t)B * Tp * 2 * g.H); }

// work buffer of the bf16 GEMM stack (swn_forward_bf16[_keep] at its geometries; byte offsets, time-major bf16) and the
// keep buffer of swn_forward_bf16_keep (floats: one slot of keep_stride per layer)
struct SwnBf16gLayout {
    size_t hs;         // [L+1][B][Tp][H]
    size_t skip;       // [B][Tp][S] relu(skip)
    size_t o1;         // [B][Tp][O1] relu(out_1)
    size_t total;
    size_t keep_stride, keep_total;      // gate pre-activations (B, 2H, Tp) fp32, G4 layout (swn_geom.hpp)
};
static inline SwnBf16gLayout swn_bf16g_layout(const SwnGeom& g, int B, long Tp) {
    SwnBf16gLayout o;
    const size_t npos = (size_t)B * Tp, el = sizeof(unsigned short);
    o.hs = 0;
    o.skip = o.hs + (size_t)(g.L + 1) * g.H * npos * el;
    o.o1 = o.skip + (size_t)g.S * npos * el;
    o.total = o.o1 + (size_t)g.O1 * npos * el;
    o.keep_stride = swn_keep_stride(g, B, Tp);
    o.keep_total = (size_t)g.L * o.keep_stride;
    return o;
}

// fp32 forward work (swn_forward, swn_bf16_work_to_f32; these three sections are documented in include/swn_hip.h) and, behind
// it, the tail of the dropout mode (swn_forward_drop's chain; the fused BL6 path has SwnBl6DropLayout instead).  Float offsets.
struct SwnFwdLayout {
    size_t hs;         // (B, L+1, H, Tp) hidden states (not written when the caller passes its own hs)
    size_t s1;         // (B, S, Tp) relu(skip)
    size_t r1;         // (B, O1, Tp) relu(out_1)
    size_t total;      // swn_forward_work_floats
    // ---- swn_fwd_drop_layout only
    size_t xm;         // (B, A0x, Tx) masked, upsampled conditioning; swn_drop_inx16: bf16 rows of swn_pitch16(Tx)
    size_t gx;         // (B, L, 2H, Tp) sample-rate in_x products
    size_t a_keep, a_stride;      // mixed-precision forward: gate pre-activations, layer l at a_keep + l * a_stride
    size_t hmask;      // (B, H, Tp) masked input of one layer
    size_t wx16;       // [L*2H][A0x] bf16 in_x matrix (swn_drop_inx16)
    size_t work16;     // g16: SwnBf16gLayout
    size_t hm16;       // g16: [B][Tp][H] bf16 masked level
    size_t wbf;        // g16: the stack's bf16 weights
    size_t drop_total; // the chain's share of swn_forward_drop_work_floats
};
static inline SwnFwdLayout swn_fwd_layout(const SwnGeom& g, int B, long Tp) {
    SwnFwdLayout o{};
    const size_t npos = (size_t)B * Tp;
    o.hs = 0;
    o.s1 = o.hs + swn_al(npos * (g.L + 1) * g.H);
    o.r1 = o.s1 + swn_al(npos * g.S);
    o.total = o.r1 + swn_al(npos * g.O1);
    return o;
}
// g16: swn_drop_g16 holds - the tail then ends with the GEMM stack's sections, g16_weight_bytes = swn_bf16g_weight_bytes
static inline SwnFwdLayout swn_fwd_drop_layout(const SwnGeom& g, int B, const SwnTrainLen& n, bool g16, size_t g16_weight_bytes) {
    SwnFwdLayout o = swn_fwd_layout(g, B, n.Tp);
    const size_t npos = (size_t)B * n.Tp;
    o.xm = o.total;
    o.gx = o.xm + swn_al((size_t)B * swn_a0x(&g) * n.Tx);
    o.a_keep = o.gx + swn_al(npos * g.L * 2 * g.H);
    o.a_stride = swn_keep_stride(g, B, n.Tp);
    o.hmask = o.a_keep + (size_t)g.L * o.a_stride;
    o.wx16 = o.hmask + swn_al(npos * g.H);
    o.work16 = o.wx16 + swn_al((size_t)g.L * 2 * g.H * swn_a0x(&g) / 2 + 1);
    o.hm16 = o.wbf = o.drop_total = o.work16;
    if (g16) {
        o.hm16 = o.work16 + swn_al_bytes(swn_bf16g_layout(g, B, n.Tp).total);
        o.wbf = o.hm16 + swn_al(npos * g.H / 2 + 1);
        o.drop_total = o.wbf + swn_al_bytes(g16_weight_bytes);
    }
    return o;
}

// backward scratch.  Float offsets; the bf16 sections hold rows of swn_da16_pitch(Tp) elements.  Two forms:
// swn_bwd_layout      the chain (swn_backward, swn_backward_keep, swn_backward_drop off the fused path); drop: the dropout
//                     mode's sections exist.  Which of the mixed-precision sections a call uses: SwnTrainPath below
// swn_bwd_bl6_layout  the compact form of the fused BL6 path (swn_backward_bf16; swn_backward_drop after swn_bl6_drop_forward):
//                     dcond | dfe | dxm | bl6, none of the other sections exists; bl6_bytes = swn_bl6_bwd_scratch_bytes(.., drop)
struct SwnBwdLayout {
    size_t do1, dskip, dhs;      // (B, O1, Tp) | (B, S, Tp) | (B, L+1, H, Tp)
    size_t a_da;                 // (B, 2H, Tp) a layer's pre-activations, then their gradient
    size_t dgx;                  // (B, 2H, Tp) a layer's d gx
    size_t dcond;                // (B, Tf, N) (compact form: not used with dropout)
    size_t dfe;                  // SwnFeLayout: gradients of the front end's activations
    size_t dxm;                  // drop: (B, A0, Tx) gradient wrt the masked conditioning; compact form: [B][Tx][A0x] bf16
    size_t hmask;                // drop: (B, H, Tp) masked input of a layer
    size_t wup_part;             // without dropout: SWN_WUP_COPIES x 256 partial g w_up (reserved in both forms)
    size_t da16;                 // two bf16 copies of a layer's da
    size_t wdt16;                // [l][tap][i][o2] transposed bf16 layer matrices
    size_t h16;                  // two bf16 copies of a layer's (masked) input
    size_t dgx_all, dgx16_all;   // drop, seg == 1: every layer's d gx (B, L, 2H, Tp); as bf16 rows in the same section
    size_t wxt16;                // drop, seg == 1: transposed bf16 in_x matrix
    size_t bl6;                  // compact form: swn_bl6_bwd_stack's scratch
    size_t total;
};
static inline SwnBwdLayout swn_bwd_layout(const SwnGeom& g, int B, int n_frames, const SwnTrainLen& n, bool drop) {
    SwnBwdLayout o{};
    const size_t npos = (size_t)B * n.Tp, H2 = 2 * (size_t)g.H, prow = (size_t)B * swn_da16_pitch(n.Tp);
    o.do1 = 0;
    o.dskip = o.do1 + swn_al(npos * g.O1);
    o.dhs = o.dskip + swn_al(npos * g.S);
    o.a_da = o.dhs + swn_al(npos * (g.L + 1) * g.H);
    o.dgx = o.a_da + swn_al(npos * H2);
    o.dcond = o.dgx + swn_al(npos * H2);
    o.dfe = o.dcond + swn_al((size_t)B * n_frames * g.N);
    o.dxm = o.dfe + swn_al(swn_fe_layout(g, B, n_frames).total);
    o.hmask = drop ? o.dxm + swn_al((size_t)B * g.A0 * n.Tx) : o.dxm;
    o.wup_part = drop ? o.hmask + swn_al(npos * g.H) : o.hmask;
    o.da16 = o.wup_part + (size_t)SWN_WUP_COPIES * 256;
    o.wdt16 = o.da16 + swn_al(prow * H2);                       // (two copies of B * 2H * pitch bf16)
    o.h16 = o.wdt16 + swn_al((size_t)g.L * g.K * g.H * H2 / 2);
    o.dgx_all = o.dgx16_all = o.h16 + swn_al(prow * g.H);
    o.wxt16 = o.total = o.dgx_all;
    if (drop && g.seg == 1) {
        o.wxt16 = o.dgx_all + swn_al(npos * g.L * H2);
        o.total = o.wxt16 + swn_al((size_t)swn_a0x(&g) * g.L * H2 / 2 + 1);
    }
    return o;
}
static inline SwnBwdLayout swn_bwd_bl6_layout(const SwnGeom& g, int B, int n_frames, const SwnTrainLen& n, bool drop, size_t bl6_bytes) {
    SwnBwdLayout o{};
    o.dcond = 0;
    o.dfe = o.dcond + swn_al((size_t)B * n_frames * g.N);
    o.dxm = o.dfe + swn_al(swn_fe_layout(g, B, n_frames).total);
    o.bl6 = drop ? o.dxm + swn_al((size_t)B * n.Tx * swn_a0x(&g) / 2) : o.dxm;
    o.total = o.bl6 + swn_al_bytes(bl6_bytes);
    return o;
}

// ---- the path of one call --------------------------------------------------------------------------------------------------
// Which kernels a training call runs and which sections of its buffers they use, resolved ONCE from what the call is given.
// A forward and the backward that follows it resolve the same record (same net, sizes, precision, masks, owner of hs); the
// size queries resolve it too.  The predicates swn_drop_g16, swn_drop_inx16, swn_drop_bf16_forward, swn_bl6_drop_supported
// and swn_bl6_bwd_supported are asked here and nowhere else.  Plain host arithmetic, no device call.
enum SwnTrainEntry {      // the entry point that asks
    SWN_TRAIN_PLAIN,      // swn_forward, swn_backward
    SWN_TRAIN_KEEP,       // swn_backward_keep, after swn_forward_bf16_keep: mixed precision by construction
    SWN_TRAIN_BL6,        // swn_backward_bf16, after swn_forward_bf16 at the BL6 class: mixed precision by construction
    SWN_TRAIN_DROP        // swn_forward_drop, swn_backward_drop
};
enum SwnTrainRoute {
    SWN_ROUTE_CHAIN,      // the generic chain of contraction kernels (SwnFwdLayout, swn_bwd_layout)
    SWN_ROUTE_BL6,        // backward: swn_bl6_bwd_stack over swn_forward_bf16's hidden states (swn_bwd_bl6_layout)
    SWN_ROUTE_BL6_DROP    // swn_bl6_drop_forward (SwnBl6DropLayout), swn_bl6_bwd_stack with sample-rate in_x operands
};
enum SwnPreact {          // where the backward takes a layer's gate pre-activations from
    SWN_PREACT_RECOMPUTE, // one more conv GEMM per layer
    SWN_PREACT_FWD_WORK,  // SwnFwdLayout::a_keep: the dropout forward of the same mode kept them
    SWN_PREACT_CALLER     // swn_backward_keep's a_keep
};
struct SwnTrainPath {
    bool bf16, drop;      // mixed-precision arithmetic; dropout mode
    int route;
    bool bl6_bwd;         // swn_bl6_bwd_stack serves this net and size (entries BL6 and DROP)
    // dropout mode
    bool g16;             // SwnFwdLayout ends with the GEMM stack's sections (whatever the precision: the sizes cover both)
    bool fwd16;           // chain forward: bf16-operand layers, every layer's pre-activations kept
    bool inx16;           // the three in_x contractions read bf16 copies: xm bf16 rows, wx16 / wxt16, d gx of all layers bf16 rows
    bool stack16;         // ... and the forward runs on the GEMM stack
    int preact;
    bool g4;              // gx / the kept pre-activations are in the G4 layout (swn_geom.hpp)
    // backward chain
    bool da16;            // gate_bwd leaves da as bf16 rows
    bool h16;             // ... and the layer's (masked) input: Q operand of the layer weight gradients
    bool wdt16;           // transposed bf16 layer matrices: both operands of the layer data gradients are bf16
    bool skip_da32;       // nobody reads the fp32 da then
    bool dgx_all;         // every layer's d gx is kept, the in_x contractions run once behind the layers
    bool dgx16_cond;      // without dropout: cond_bwd_kernel reads a layer's d gx as bf16 rows
};
// own_hs: the caller passes its own hidden-state buffer.  drop_h: the dropout mode's host array of mask pointers (else null)
static inline SwnTrainPath swn_train_path(const swn_net_desc* d, const SwnGeom& g, int B, int n_frames, const SwnTrainLen& n,
                                          int entry, int precision, const float* const* drop_h, bool own_hs) {
    SwnTrainPath p{};
    const long Tp = n.Tp;
    p.drop = entry == SWN_TRAIN_DROP;
    p.bf16 = precision == SWN_PRECISION_BF16 || entry == SWN_TRAIN_KEEP || entry == SWN_TRAIN_BL6;
    p.bl6_bwd = (entry == SWN_TRAIN_BL6 || p.drop) && swn_bl6_bwd_supported(g, B, Tp, n_frames);
    // dropout as run.sh trains the BL6 class (no mask between layers): the fused path, unless the caller wants fp32 hidden states
    if (entry == SWN_TRAIN_BL6) p.route = SWN_ROUTE_BL6;
    else if (p.drop && p.bf16 && !own_hs && swn_bl6_drop_supported(g, B, Tp, n_frames, drop_h)) p.route = SWN_ROUTE_BL6_DROP;
    else p.route = SWN_ROUTE_CHAIN;
    const bool chain = p.route == SWN_ROUTE_CHAIN;
    p.g16 = p.drop && swn_drop_g16(d, B, Tp);
    p.fwd16 = chain && p.drop && p.bf16 && swn_drop_bf16_forward(&g);
    // a caller that owns hs gets the exact layout of the fp32 chain in every section it may read: no bf16 copies, and the
    // backward recomputes the pre-activations
    p.inx16 = p.fwd16 && !own_hs && swn_drop_inx16(&g, Tp);
    p.stack16 = p.g16 && p.inx16;
    p.preact = entry == SWN_TRAIN_KEEP ? SWN_PREACT_CALLER : p.fwd16 && !own_hs ? SWN_PREACT_FWD_WORK : SWN_PREACT_RECOMPUTE;
    p.g4 = entry == SWN_TRAIN_KEEP || p.stack16;
    // the kernels reach the second (odd) copy of da / h through a 32-bit byte offset from an utterance's rows: it must stay
    // below 2 GiB, else that operand stays fp32
    const size_t pitch = (size_t)swn_da16_pitch(Tp), H = g.H, H2 = 2 * H;
    p.da16 = chain && p.bf16;
    p.h16 = p.da16 && Tp >= 256 && ((size_t)B * H * pitch + H * pitch) * 2 < (1ull << 31);
    p.wdt16 = p.da16 && g.Hp == g.H && H2 % 32 == 0 && ((size_t)B * H2 * pitch + H2 * pitch) * 2 < (1ull << 31);
    p.skip_da32 = p.wdt16 && Tp >= 256;      // launch_reduce / launch_time take their bf16-copy kernels under exactly these conditions
    p.dgx_all = chain && p.drop && g.seg == 1;
    // (GEMM-stack class; the small nets keep fp32 here: the rounding moved a 2e-2 gradient check of the 32-channel fixtures)
    p.dgx16_cond = entry == SWN_TRAIN_KEEP && p.da16 && (long)pitch <= 2L * Tp;
    return p;
}
static inline SwnFwdLayout swn_fwd_layout_of(const SwnGeom& g, int B, const SwnTrainLen& n, const SwnTrainPath& p) {
    return p.drop ? swn_fwd_drop_layout(g, B, n, p.g16, p.g16 ? swn_bf16g_weight_bytes(g) : 0) : swn_fwd_layout(g, B, n.Tp);
}
