// gs_host::L1FusedPolicy behind a C interface: tests/test_l1_fused_policy.py plays the renderer -- it asks whether a frame takes the
// one-pass level 1, reports retired frames and region overflows, and asks what the candidate buffer may grow to.
// Built by that test with g++; nothing here touches a GPU.
#include <cstdint>

#include "gs_depth_policy.h"

using gs_host::L1FusedPolicy;

extern "C" {

void* lf_new(int mode) {
    L1FusedPolicy* p = new L1FusedPolicy;
    p->mode = mode;
    return p;
}
void lf_free(void* h) { delete static_cast<L1FusedPolicy*>(h); }
uint32_t lf_hold(void* h) { return static_cast<L1FusedPolicy*>(h)->hold; }
uint32_t lf_region_cap(uint32_t cand_capacity, uint32_t bins) { return L1FusedPolicy::region_cap(cand_capacity, bins); }
// flags: bit 0 any_order, bit 1 planes regime, bit 2 the scene has its spatial copy
int lf_decide(void* h, int flags, uint32_t width, uint32_t height, int bin_shift, uint32_t cand_capacity, uint32_t bins) {
    return static_cast<int>(static_cast<L1FusedPolicy*>(h)->decide((flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, width, height, bin_shift,
                                                                   cand_capacity, bins));
}
uint32_t lf_grow_to(void* h, int flags, uint32_t width, uint32_t height, int bin_shift, uint32_t cand_capacity, uint32_t bins,
                    uint32_t default_cand_capacity) {
    L1FusedPolicy& p = *static_cast<L1FusedPolicy*>(h);
    const L1FusedPolicy::Verdict v = p.decide((flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, width, height, bin_shift, cand_capacity, bins);
    return p.grow_to(v, width, height, bin_shift, cand_capacity, bins, default_cand_capacity);
}
void lf_retired(void* h, uint32_t width, uint32_t height, int bin_shift, uint32_t max_bin, uint32_t e1, uint32_t v) {
    static_cast<L1FusedPolicy*>(h)->frame_retired(width, height, bin_shift, max_bin, e1, v);
}
void lf_region_overflowed(void* h) { static_cast<L1FusedPolicy*>(h)->region_overflowed(); }
// the verdicts' values by name order: engage, switched off, not any-order, dense regime, no spatial copy, held, cap too small, wide splats
int lf_verdict(int which) {
    const L1FusedPolicy::Verdict v[8] = {L1FusedPolicy::kEngage,        L1FusedPolicy::kSwitchedOff, L1FusedPolicy::kNotAnyOrder,
                                         L1FusedPolicy::kDenseRegime,   L1FusedPolicy::kNoSpatialCopy, L1FusedPolicy::kHeld,
                                         L1FusedPolicy::kCapTooSmall,   L1FusedPolicy::kWideSplats};
    return static_cast<int>(v[which]);
}
uint32_t lf_const(int which) {  // 0 hold, 1 grow ceiling, 2 wide ratio
    const uint32_t v[3] = {L1FusedPolicy::kHold, L1FusedPolicy::kGrowCeiling, L1FusedPolicy::kWideRatio};
    return v[which];
}

}  // extern "C"
