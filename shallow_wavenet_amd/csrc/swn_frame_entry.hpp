// Host only.  The rules of a swn_logmel_entry that do not depend on the feature: row i of a call holds the samples [t0, t0 +
// n_avail) of a signal of len samples (-1: not known yet) and asks for its frames [f0, f1) of F = 1 + len / hop.  swn_logmel,
// swn_mcep and the rows of swn_logmel_pool (swn_melspec.hip), swn_f0 and swn_bap (swn_f0.hip) and swn_envelope (swn_envelope.hip, whose
// entry carries one pointer more) check every entry with this
// before their own rule: which samples the range reads, and whether the window holds them.
#pragma once
#include <cstdio>

#include "../../include/swn_hip.h"

constexpr int FE_MAX_LEN = 1 << 30;
constexpr int FE_EMPTY = 1;             // not an error code: those are negative

// FE_EMPTY: the entry passes and has no frames (nothing more to check: it may carry null pointers); SWN_OK: it passes, and the
// caller's reach rule is next.  A known length must lie in [min_len, 2^30]; `len_rule` is how the message words the lower
// bound.  `fail(what)` records the message for the entry point it reports for and returns the error code.
template <class Fail>
int frame_entry_check(const swn_logmel_entry& e, int i, int hop, int min_len, const char* len_rule, bool need_pointers, Fail fail) {
    char msg[160];
    if (e.reserved != 0) { snprintf(msg, sizeof msg, "entry %d: reserved field is not 0", i); return fail(msg); }
    if (e.f0 < 0 || e.f1 < e.f0) { snprintf(msg, sizeof msg, "entry %d: frame range [%d, %d)", i, e.f0, e.f1); return fail(msg); }
    if (e.len != -1 && (e.len < min_len || e.len > FE_MAX_LEN)) {
        snprintf(msg, sizeof msg, "entry %d: length %d, need %s <= 2^30 (or -1 while unknown)", i, e.len, len_rule);
        return fail(msg);
    }
    if (e.t0 < 0 || e.n_avail < 0 || (long long)e.t0 + e.n_avail > FE_MAX_LEN ||
        (e.len != -1 && (long long)e.t0 + e.n_avail > e.len)) {
        snprintf(msg, sizeof msg, "entry %d: window [%d, %d + %d) is not inside the signal", i, e.t0, e.t0, e.n_avail);
        return fail(msg);
    }
    if (e.f1 == e.f0) return FE_EMPTY;
    if (need_pointers && (!e.wav_dev || !e.out_dev)) { snprintf(msg, sizeof msg, "entry %d: null pointer", i); return fail(msg); }
    if (e.len != -1 && e.f1 > 1 + e.len / hop) {
        snprintf(msg, sizeof msg, "entry %d: f1 = %d, a signal of %d samples has %d frames", i, e.f1, e.len, 1 + e.len / hop);
        return fail(msg);
    }
    return SWN_OK;
}
