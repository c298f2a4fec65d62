// Live kernel timing and the on-chip poison hook (csrc/prof.hip; include/linr_hip.h: linr_prof_*, linr_debug_poison), and the ONE
// table of kernel classes both are keyed by.  Not part of the C-ABI.
#pragma once
#include "common.h"

// The numbers are those of the class list in include/linr_hip.h (bench/ and tests/ address classes by number): a new class is a
// new LAST name here, LINR_PROF_KINDS + 1 and a line in that list.
enum ProfKind {
    // fp32 executor (csrc/net.hip, csrc/bwd_tail.hip)
    PK_FUSED88 = 0, PK_CONV88 = 1, PK_FUSED_DUAL = 2, PK_FUSED_C00 = 3, PK_HEAD_FWD = 4, PK_CONVPW_FWD = 5, PK_DUAL_FWD = 6,
    PK_OCC7 = 7, PK_HEAD_BWD = 8, PK_WGRAD = 9, PK_LIN_WGRAD = 10, PK_SCE = 11, PK_MISC = 12, PK_BWD_DATA = 13,
    // poison only (linr_poison_hook; never timed)
    PK_BF16_INFER = 14,      // the bf16 inference executors (csrc/net_bf16.hip, csrc/wide_bf16.hip)
    PK_DECODE = 15,          // the decoder scales (csrc/decode.hip) and the kernel map of frame segments (csrc/kmap.hip)
    PK_WIDE = 16,            // the entries of csrc/wide.hip
    // bf16 training executor (csrc/train_bf16.hip)
    TK_BWD88 = 17, TK_BWD_DUAL = 18, TK_BWD_C00 = 19, TK_FWD = 20, TK_HEAD_BWD = 21, TK_FIRST_WGRAD = 22, TK_MISC = 23
};
static_assert(TK_MISC + 1 == LINR_PROF_KINDS, "include/linr_hip.h: LINR_PROF_KINDS counts the classes above");

// poisons LDS and vector registers of every CU on `s` when bit `kind` of linr_debug_poison's mask is set
__attribute__((visibility("hidden"))) void linr_poison_hook(hipStream_t s, int kind);

struct ProfRec { hipEvent_t ev0, ev1; int passes; };
// Around one launch (an automatic variable in front of it): poisons first when the class's poison bit is set, then brackets what
// follows on `s` with an event pair until the end of the scope - only while timing is enabled, the class is in linr_prof_mask and a
// free event pair is left.  `passes`: row passes (groups) of the launch.  Nothing is recorded and no lock is taken when disabled.
struct ProfScope {
    hipStream_t s; int kind; bool live;
    ProfRec r;
    ProfScope(hipStream_t s, int kind, int passes);
    ~ProfScope();
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;
};
