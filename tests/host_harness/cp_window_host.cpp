// TEST HARNESS ONLY: compiles the window bookkeeping of epsm_mitsuba3_amd/csrc/epsm_cp_core.h for the CPU -- the slot word a
// window of the backward kernel keeps per sorted path (cp::slot_word and its accessors) and the schedule that cuts a launch
// into windows (cp::window_schedule / window_at / windows_per_workgroup) -- the SAME functions the gfx950 kernel and its
// launcher call.  Batched entry points: a test hands over arrays, numpy does the comparing.
#include <stdint.h>

#include "../../epsm_mitsuba3_amd/csrc/epsm_cp_core.h"

using namespace epsm;

enum { kFieldNv = 0, kFieldIdstar = 1, kFieldA = 2, kFieldB = 7, kFieldDiffuse1 = 12, kFieldActive1 = 13, kFieldInRange = 14, kFieldSlot = 15, kFields = 16 };

// The plan word of flag word fw[i] as the kernel's planning phase forms it (K logged vertices; in-range and active1 set by the
// caller: in_range[i] != 0, bit 2 of the flag word) -> plan[i]; its slot word at window slot `slot` -> word[i]; and what the
// accessors read: fields_plan[i][*] from the plan word (slot: the one handed in, 0 out of range), fields_word[i][*] from the
// slot word alone.
extern "C" void epsm_host_slot_words(int variant, int K, const uint32_t *fw, const uint8_t *in_range, int64_t n, uint32_t slot,
                                     uint32_t *plan, uint32_t *word, int32_t *fields_plan, int32_t *fields_word) {
    for (int64_t i = 0; i < n; ++i) {
        uint32_t w = fw[i];
        if (K < 5) w &= (1u << (5 * K)) - 1u;
        uint32_t p = variant == 0 ? cp::manifold_plan(w) : cp::caustic_plan(w);
        p = in_range[i] ? (p | cp::kPlanInRange | ((w & 4u) ? cp::kPlanActive1 : 0u)) : 0u;
        const uint32_t s = cp::slot_word(p, slot);
        plan[i] = p; word[i] = s;
        int32_t *a = fields_plan + i * kFields, *b = fields_word + i * kFields;
        a[kFieldNv] = cp::plan_nv(p); b[kFieldNv] = cp::plan_nv(s);
        a[kFieldIdstar] = cp::plan_idstar(p); b[kFieldIdstar] = cp::plan_idstar(s);
        for (int k = 1; k <= 5; ++k) {
            a[kFieldA + k - 1] = cp::plan_a(p, k); b[kFieldA + k - 1] = cp::plan_a(s, k);
            a[kFieldB + k - 1] = cp::plan_b(p, k); b[kFieldB + k - 1] = cp::plan_b(s, k);
        }
        a[kFieldDiffuse1] = cp::plan_diffuse1(p); b[kFieldDiffuse1] = cp::slot_diffuse1(s);
        a[kFieldActive1] = (p & cp::kPlanActive1) != 0; b[kFieldActive1] = cp::slot_active1(s);
        a[kFieldInRange] = (p & cp::kPlanInRange) != 0; b[kFieldInRange] = cp::slot_in_range(s);
        a[kFieldSlot] = (p & cp::kPlanInRange) ? (int32_t) slot : 0; b[kFieldSlot] = cp::slot_of(s);
    }
}

// number of windows of n paths with S workgroup slots (0: no taper) and bulk windows of W: what the launcher sizes the grid with
extern "C" int64_t epsm_host_window_count(int64_t n, int64_t S, int W) { return cp::window_schedule(n, S, W).windows; }
// windows win0 .. win0 + count - 1 -> first[], size[]
extern "C" void epsm_host_windows(int64_t n, int64_t S, int W, int64_t win0, int64_t count, int64_t *first, int32_t *size) {
    const cp::WindowSchedule s = cp::window_schedule(n, S, W);
    for (int64_t i = 0; i < count; ++i) {
        int sz;
        cp::window_at(s, win0 + i, first[i], sz);
        size[i] = sz;
    }
}
extern "C" int64_t epsm_host_windows_per_workgroup(int64_t windows, int64_t workgroups) { return cp::windows_per_workgroup(windows, workgroups); }
