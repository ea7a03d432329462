// queue_plan.h -- which of a process's hardware queues each group stream of a context sits on, and a choice of streams
// that spreads the groups over all of them.  Host-only C++: no HIP type appears here, so tools/queue_plan_check.cpp can
// drive all of it with a fake runtime.
//
// Why: a process has a few in-order hardware queues (four by default) and the runtime deals every stream to one of them
// by a rule of its own, which also counts the streams the process held before.  Six group streams created in a row came
// out as two on each of THREE queues, the fourth carrying next to nothing (profiles/r10_queue_occupancy_after.json); a
// group's chain kernels hold its queue for half of a launch with a handful of waves, and the other group of that queue
// cannot start its grid-filling kernels meanwhile.  HIP has no call that names a stream's queue,
// so nothing here guesses from creation order: streams are CLASSIFIED by a probe ("does b wait behind a?"), candidates
// are created until the classes allow an even split, the groups take one stream each, and the rest are destroyed.
#pragma once
#include <algorithm>
#include <vector>

namespace nblic {

constexpr int kPlanMaxClasses = 32;

// What became of the plan (QueuePlan::state); everything but kPlanOn leaves the context with one stream per group as the
// runtime deals them.
enum QueuePlanState {
    kPlanOn = 0,
    kPlanFewGroups = 1,                                              // fewer than three groups: it did not run
    kPlanSwitchedOff = 2,                                            // NBLIC_AMD_QUEUE_PLAN=0
    kPlanOneClass = 3,                                               // every candidate waits behind every other: nothing to spread over
    kPlanInconclusive = 4,                                           // a probe could not tell (the busy kernel's duration could not be measured), or more classes than kPlanMaxClasses
    kPlanError = 5,                                                  // a call of the runtime failed
};
inline const char *queue_plan_state_name(int s) {
    static const char *const names[] = {"on", "fewer than three groups", "switched off (NBLIC_AMD_QUEUE_PLAN=0)", "one class found", "a probe was inconclusive", "a runtime call failed"};
    return s >= 0 && s < 6 ? names[s] : "?";
}

// What a probe says.
enum ProbeAnswer { kProbeFree = 0, kProbeBlocks = 1, kProbeInconclusive = -1, kProbeError = -2 };

struct QueuePlan {
    int state = kPlanFewGroups;
    int n_groups = 0;
    int classes = 0;                                                 // classes found: the hardware queues the process can use, as far as the candidates reached them
    int candidates = 0;                                              // candidate streams created
    int groups_per_class[kPlanMaxClasses] = {0};                     // of the chosen streams (state on), or all in class 0 (one class)
    int unplanned_per_class[kPlanMaxClasses] = {0};                  // the first n_groups candidates: what the runtime's own dealing gives
    double plan_ms = 0;                                              // filled by the caller
    std::vector<int> chosen;                                         // state on: the candidate each group takes, by group
    std::vector<int> chosen_class;                                   // and its class
    static int spread_of(const int *v, int n) { return n > 0 ? *std::max_element(v, v + n) - *std::min_element(v, v + n) : 0; }
    int spread() const { return spread_of(groups_per_class, classes); }                // largest minus smallest number of groups over the classes found
    int unplanned_spread() const { return spread_of(unplanned_per_class, classes); }
    int most() const { return classes > 0 ? *std::max_element(groups_per_class, groups_per_class + classes) : 0; }
    int unplanned_most() const { return classes > 0 ? *std::max_element(unplanned_per_class, unplanned_per_class + classes) : 0; }
};

namespace plan_detail {
// n groups over classes that hold members[k] candidates: every group goes to the class with the fewest groups so far
// that still has a candidate to give (the earliest found among equals).  No split over these classes has a smaller
// largest share or a larger smallest one.  false: fewer candidates than groups.
inline bool split(int n, const std::vector<int> &members, std::vector<int> &share) {
    share.assign(members.size(), 0);
    for (int g = 0; g < n; g++) {
        int best = -1;
        for (size_t k = 0; k < members.size(); k++)
            if (share[k] < members[k] && (best < 0 || share[k] < share[size_t(best)])) best = int(k);
        if (best < 0) return false;
        share[size_t(best)]++;
    }
    return true;
}
}  // namespace plan_detail

// The plan for n_groups groups.
//   new_candidate() -> id >= 0   a new stream (the ids are the caller's), or -1: the runtime refused
//   blocks(a, b)                 ProbeAnswer: does candidate b wait behind candidate a?
//   drop(id)                     destroys a candidate
// Candidates are classified one at a time against ONE representative per class found so far (its first member), so a
// candidate costs at most `classes` probes.  At least n_groups candidates are created -- the first n_groups are what
// not planning would have used -- and the search ends
//   * when as many classes as groups are found: every group can be alone, nothing is left to gain;
//   * from 2 n_groups candidates on, as soon as the classes allow a split whose shares differ by at most one (not sooner:
//     a queue that held streams before the context came is dealt nothing until the others have caught up, and shows
//     only then);
//   * at 4 n_groups candidates, with the best split there is.
// On return every candidate that no group takes has been dropped; unless state is kPlanOn, all of them.
template <class NewCandidate, class Blocks, class Drop>
inline QueuePlan plan_queues(int n_groups, NewCandidate new_candidate, Blocks blocks, Drop drop) {
    QueuePlan p;
    p.n_groups = n_groups;
    if (n_groups < 3) { p.state = kPlanFewGroups; return p; }
    std::vector<std::vector<int>> cls;                               // the classes' members, in the order they were created
    std::vector<int> all, members, share;
    auto give_up = [&](int state) {
        for (int id : all) drop(id);
        p.state = state; p.classes = int(cls.size()); p.chosen.clear(); p.chosen_class.clear();
        std::fill(p.groups_per_class, p.groups_per_class + kPlanMaxClasses, 0);
        std::fill(p.unplanned_per_class, p.unplanned_per_class + kPlanMaxClasses, 0);
        if (state != kPlanOneClass) p.classes = 0;                   // a classification that did not finish says nothing
        else p.groups_per_class[0] = p.unplanned_per_class[0] = n_groups;
        return p;
    };
    const int cap = 4 * n_groups;
    while (p.candidates < cap) {
        const int id = new_candidate();
        if (id < 0) return give_up(kPlanError);
        all.push_back(id); p.candidates++;
        int k = 0;
        for (; k < int(cls.size()); k++) {
            const int a = blocks(cls[size_t(k)][0], id);
            if (a == kProbeError) return give_up(kPlanError);
            if (a == kProbeInconclusive) return give_up(kPlanInconclusive);
            if (a == kProbeBlocks) break;
        }
        if (k == int(cls.size())) {
            if (k == kPlanMaxClasses) return give_up(kPlanInconclusive);
            cls.emplace_back();
        }
        cls[size_t(k)].push_back(id);
        if (p.candidates <= n_groups) p.unplanned_per_class[k]++;
        if (p.candidates < n_groups) continue;
        if (int(cls.size()) >= n_groups) break;
        if (p.candidates >= 2 * n_groups) {
            members.clear();
            for (auto &c : cls) members.push_back(int(c.size()));
            if (plan_detail::split(n_groups, members, share) && QueuePlan::spread_of(share.data(), int(share.size())) <= 1) break;
        }
    }
    if (cls.size() <= 1) return give_up(kPlanOneClass);
    members.clear();
    for (auto &c : cls) members.push_back(int(c.size()));
    plan_detail::split(n_groups, members, share);                    // cannot fail: there are at least n_groups candidates
    p.classes = int(cls.size());
    std::vector<char> kept(size_t(*std::max_element(all.begin(), all.end())) + 1, 0);
    for (size_t k = 0; k < cls.size(); k++) {
        p.groups_per_class[k] = share[k];
        for (int j = 0; j < share[k]; j++) { p.chosen.push_back(cls[k][size_t(j)]); p.chosen_class.push_back(int(k)); kept[size_t(cls[k][size_t(j)])] = 1; }
    }
    for (int id : all) if (!kept[size_t(id)]) drop(id);
    p.state = kPlanOn;
    return p;
}

}  // namespace nblic
