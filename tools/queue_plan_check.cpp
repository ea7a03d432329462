// queue_plan_check.cpp -- csrc/queue_plan.h alone, with its own main, for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o queue_plan_check tools/queue_plan_check.cpp
// The classification and the choice of streams (plan_queues) are driven with a FAKE runtime: a number of queues, a rule
// that deals every new stream to one of them, and a probe that answers from the queues themselves.  Swept: 3, 4, 6 and 12
// groups over streams dealt round-robin to 1, 2, 3, 4 and 16 queues; least-loaded dealing with 0-3 streams held on one
// queue beforehand (six groups on four queues must come out 2 / 2 / 1 / 1); a runtime with one queue; an error or an
// inconclusive answer injected at every call in turn; dealings under which the candidate cap is reached before balance.
// In every case: no probe names a destroyed stream, every stream no group takes is destroyed exactly once, the groups'
// streams are distinct and alive, and the classes reported are the fake's queues.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <numeric>
#include <set>
#include <vector>

#include "../nblic-image-compression_amd/csrc/queue_plan.h"

using namespace nblic;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "queue_plan_check: %s failed (line %d)\n", #x, __LINE__); exit(1); } } while (0)

namespace {

struct Fake {
    int queues = 4;
    std::vector<int> load;                                           // streams on each queue, the ones held beforehand included
    std::function<int(Fake &, int)> deal;                            // (this, index of the new stream) -> queue
    std::vector<int> queue_of; std::vector<char> alive;
    long calls = 0, fail_at = -1; int fail_with = kProbeError;       // calls of the runtime so far (creations and probes); which of them fails, and how
    long created = 0, destroyed = 0, probes = 0, probes_of_candidate = 0, most_probes_of_candidate = 0;
    explicit Fake(int q) : queues(q), load(size_t(q), 0) {}
    int new_candidate() {
        if (++calls == fail_at) return -1;
        const int q = deal(*this, int(queue_of.size()));
        CHECK(q >= 0 && q < queues);
        queue_of.push_back(q); alive.push_back(1); load[size_t(q)]++; created++;
        probes_of_candidate = 0;
        return int(queue_of.size()) - 1;
    }
    int blocks(int a, int b) {
        CHECK(a >= 0 && b >= 0 && a < int(alive.size()) && b < int(alive.size()) && a != b);
        CHECK(alive[size_t(a)] && alive[size_t(b)]);                 // a probe never launches on a destroyed stream
        if (++calls == fail_at) return fail_with;
        probes++;
        most_probes_of_candidate = std::max(most_probes_of_candidate, ++probes_of_candidate);
        return queue_of[size_t(a)] == queue_of[size_t(b)] ? kProbeBlocks : kProbeFree;
    }
    void drop(int id) {
        CHECK(id >= 0 && id < int(alive.size()) && alive[size_t(id)]);     // exactly once
        alive[size_t(id)] = 0; load[size_t(queue_of[size_t(id)])]--; destroyed++;
    }
    long live() const { return created - destroyed; }
};

int round_robin(Fake &f, int index) { return index % f.queues; }
int least_loaded(Fake &f, int) { return int(std::min_element(f.load.begin(), f.load.end()) - f.load.begin()); }     // the first among equals

QueuePlan run(Fake &f, int n) {
    return plan_queues(n, [&] { return f.new_candidate(); }, [&](int a, int b) { return f.blocks(a, b); }, [&](int id) { f.drop(id); });
}

// What holds for every plan that is on.
void check_on(const Fake &f, const QueuePlan &p, int n) {
    CHECK(p.state == kPlanOn && p.n_groups == n);
    CHECK(p.classes >= 2 && p.classes <= kPlanMaxClasses && p.classes <= f.queues);
    CHECK(p.candidates == f.created && p.candidates >= n && p.candidates <= 4 * n);
    CHECK(f.most_probes_of_candidate <= p.classes);                  // one representative per class
    CHECK(int(p.chosen.size()) == n && int(p.chosen_class.size()) == n && f.live() == n);
    CHECK(std::accumulate(p.groups_per_class, p.groups_per_class + p.classes, 0) == n);
    CHECK(std::accumulate(p.unplanned_per_class, p.unplanned_per_class + p.classes, 0) == n);
    std::set<int> ids(p.chosen.begin(), p.chosen.end());
    CHECK(int(ids.size()) == n);                                     // no two groups share a stream
    std::vector<int> per(size_t(p.classes), 0), queue_of_class(size_t(p.classes), -1);
    for (int g = 0; g < n; g++) {
        const int id = p.chosen[size_t(g)], k = p.chosen_class[size_t(g)];
        CHECK(id >= 0 && id < int(f.alive.size()) && f.alive[size_t(id)]);      // no group launches on a destroyed candidate
        CHECK(k >= 0 && k < p.classes);
        per[size_t(k)]++;
        if (queue_of_class[size_t(k)] < 0) queue_of_class[size_t(k)] = f.queue_of[size_t(id)];
        CHECK(queue_of_class[size_t(k)] == f.queue_of[size_t(id)]);  // a class is one queue
    }
    for (int k = 0; k < p.classes; k++) {
        CHECK(per[size_t(k)] == p.groups_per_class[k]);
        for (int j = 0; j < k; j++) CHECK(queue_of_class[size_t(k)] < 0 || queue_of_class[size_t(k)] != queue_of_class[size_t(j)]);   // and two classes are two
    }
    CHECK(p.spread() <= p.unplanned_spread() && p.most() <= p.unplanned_most());     // never worse than not planning
}

void check_off(const Fake &f, const QueuePlan &p, int state) {
    CHECK(p.state == state);
    CHECK(p.chosen.empty() && p.chosen_class.empty());
    CHECK(f.live() == 0 && f.created == p.candidates);               // every candidate destroyed
}

const int kGroups[] = {3, 4, 6, 12};

void round_robin_cases() {
    for (int q : {1, 2, 3, 4, 16})
        for (int n : kGroups) {
            Fake f(q);
            f.deal = round_robin;
            const QueuePlan p = run(f, n);
            if (q == 1) {
                check_off(f, p, kPlanOneClass);
                CHECK(p.classes == 1 && p.groups_per_class[0] == n);
                continue;
            }
            check_on(f, p, n);
            CHECK(p.classes == std::min(q, p.candidates));
            CHECK(p.spread() <= 1);
        }
}

void least_loaded_cases() {
    for (int held = 0; held <= 3; held++)
        for (int n : kGroups) {
            Fake f(4);
            f.deal = least_loaded;
            f.load[0] = held;
            const QueuePlan p = run(f, n);
            check_on(f, p, n);
            CHECK(p.spread() <= 1);
            CHECK(f.load[0] >= held);                                // what was held beforehand is nobody's to destroy
            if (n == 6) {                                            // the picture of profiles/r10_queue_occupancy_after.json: 2 / 2 / 2 / 0 unplanned once a queue is held
                CHECK(p.classes == 4);
                std::vector<int> s(p.groups_per_class, p.groups_per_class + 4);
                std::sort(s.begin(), s.end());
                CHECK(s[0] == 1 && s[1] == 1 && s[2] == 2 && s[3] == 2);
                if (held >= 2) CHECK(p.unplanned_spread() == 2);
            }
            if (n == 12) CHECK(p.classes == 4 && p.spread() == 0);
        }
}

void fewer_than_three() {
    for (int n : {0, 1, 2}) {
        Fake f(4);
        f.deal = round_robin;
        const QueuePlan p = run(f, n);
        CHECK(p.state == kPlanFewGroups && f.calls == 0 && p.candidates == 0 && p.classes == 0);
    }
}

void errors_at_every_call() {
    for (int n : kGroups)
        for (int held : {0, 3}) {
            Fake ok(4);
            ok.deal = least_loaded; ok.load[0] = held;
            run(ok, n);
            const long calls = ok.calls;
            CHECK(calls > n);
            for (long k = 1; k <= calls; k++)
                for (int with : {int(kProbeError), int(kProbeInconclusive)}) {
                    Fake f(4);
                    f.deal = least_loaded; f.load[0] = held;
                    f.fail_at = k; f.fail_with = with;
                    const QueuePlan p = run(f, n);
                    CHECK(p.state == kPlanError || p.state == kPlanInconclusive);      // (a creation that fails is an error whatever fail_with says)
                    check_off(f, p, p.state);
                    CHECK(p.classes == 0 && f.calls == k);           // nothing more is asked of the runtime after the failure
                }
        }
}

void cap_before_balance() {
    for (int n : kGroups) {
        {   // one stream on queue 0, every later one on queue 1: no split is even, the best one is 1 / n-1
            Fake f(2);
            f.deal = [](Fake &, int index) { return index == 0 ? 0 : 1; };
            const QueuePlan p = run(f, n);
            check_on(f, p, n);
            CHECK(p.candidates == (n - 2 <= 1 ? 2 * n : 4 * n));      // (three groups: 1 / 2 IS even, found at 2 n)
            CHECK(p.classes == 2 && p.groups_per_class[0] == 1 && p.groups_per_class[1] == n - 1);
            CHECK(p.spread() == n - 2 && p.spread() == p.unplanned_spread());
        }
        {   // the first n on queue 0, then one each on queues 1 and 2, the rest on queue 0 again: better than unplanned, not even
            Fake f(3);
            f.deal = [n](Fake &, int index) { return index == n ? 1 : index == n + 1 ? 2 : 0; };
            const QueuePlan p = run(f, n);
            check_on(f, p, n);
            CHECK(p.candidates == (n == 3 ? n + 2 : n == 4 ? 2 * n : 4 * n));            // (three groups: a class each; four: 2 / 1 / 1 is even)
            CHECK(p.classes == 3 && p.groups_per_class[0] == n - 2 && p.groups_per_class[1] == 1 && p.groups_per_class[2] == 1);
            CHECK(p.unplanned_spread() == n && p.spread() == n - 3);
        }
    }
    {   // more queues than classes the plan can name: it says so and keeps nothing
        Fake f(kPlanMaxClasses + 8);
        f.deal = round_robin;
        const QueuePlan p = run(f, kPlanMaxClasses + 4);
        check_off(f, p, kPlanInconclusive);
    }
}

}  // namespace

int main() {
    fewer_than_three();
    round_robin_cases();
    least_loaded_cases();
    errors_at_every_call();
    cap_before_balance();
    for (int s = 0; s < 6; s++) CHECK(queue_plan_state_name(s)[0] != '?');
    printf("queue_plan_check ok\n");
    return 0;
}
