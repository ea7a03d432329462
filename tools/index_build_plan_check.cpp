// Stand-alone check of index_entries.h's index_build_plan (host only): the launch schedule of a batch index build against a
// plain replay -- a job advances min(rows, next entry row - row) per launch -- on the cases tests/test_index_build_batch_host.py
// runs through the library.  Build with the sanitizers and run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o index_build_plan_check tools/index_build_plan_check.cpp && ./index_build_plan_check
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>

#include "../nblic-image-compression_amd/csrc/index_entries.h"

using namespace nblic;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static int check(const std::vector<BuildPlanImage> &im) {
    BuildPlan P;
    CHECK(index_build_plan(im.data(), int(im.size()), P));
    int launches[kBuildClasses] = {0};
    std::map<std::pair<int, int>, int> where;
    for (int k = 0; k < int(im.size()); k++) {
        const BuildPlanImage &I = im[size_t(k)];
        const int count = (I.h - 1) / I.every;
        int row = 0, launch = 0;
        while (row < I.h) {
            const int next = (row / I.every + 1) * I.every, stop = next <= count * I.every ? next : I.h;
            row += I.rows < stop - row ? I.rows : stop - row;
            if (row < I.h && row % I.every == 0) where[{k, row}] = launch;
            launch++;
        }
        const int cls = indexed_class(I.kind, I.effort);
        if (launch > launches[cls]) launches[cls] = launch;
    }
    for (int c = 0; c < kBuildClasses; c++) CHECK(P.launches[c] == launches[c]);
    CHECK(P.entries.size() == where.size());
    for (size_t j = 0; j < P.entries.size(); j++) {
        const BuildEntry &E = P.entries[j];
        CHECK(E.image >= 0 && E.image < int(im.size()));
        CHECK(E.cls == indexed_class(im[size_t(E.image)].kind, im[size_t(E.image)].effort));
        const auto it = where.find({E.image, E.row});
        CHECK(it != where.end() && it->second == E.launch);
        CHECK(E.launch >= 0 && E.launch < P.launches[E.cls]);
        if (j > 0) {
            const BuildEntry &D = P.entries[j - 1];
            CHECK(D.cls < E.cls || (D.cls == E.cls && D.launch <= E.launch));
            if (D.cls == E.cls && D.launch == E.launch) CHECK(D.image < E.image || (D.image == E.image && D.row < E.row));
        }
    }
    return 0;
}

int main() {
    const int classes[4][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 0}};
    // R = 1; R and rows that do not divide each other; R = h - 1; one row per launch
    if (check({{0, 1, 23, 149, 1, 23}}) || check({{0, 1, 23, 149, 1, 5}}) || check({{1, 0, 2, 1, 1, 2}})) return 1;
    const int pairs[7][2] = {{7, 3}, {3, 7}, {6, 4}, {4, 6}, {5, 5}, {10, 3}, {3, 10}};
    for (auto &p : pairs)
        for (int h : {p[0] + 1, 40, 67})
            if (check({{0, 2, h, 150, p[0], p[1] < h ? p[1] : h}})) return 1;
    for (int h : {2, 3, 40, 65535})
        if (check({{0, 1, h, 3, h - 1, h}}) || check({{0, 1, h, 3, h - 1, h < 100 ? 1 : 4096}})) return 1;
    if (check({{0, 1, 23, 149, 3, 1}, {0, 1, 67, 150, 7, 1}, {1, 0, 40, 131, 39, 1}, {0, 3, 12, 9, 4, 1}})) return 1;
    // mixed classes
    std::mt19937 rng(15);
    int plans = 0;
    for (int t = 0; t < 300; t++) {
        std::vector<BuildPlanImage> im;
        const int n = 1 + int(rng() % 13);
        for (int k = 0; k < n; k++) {
            const int *c = classes[rng() % 4];
            const int h = 2 + int(rng() % 78), rows = 1 + int(rng() % unsigned(h));
            im.push_back(BuildPlanImage{c[0], c[1], h, 1 + int(rng() % 299), 1 + int(rng() % unsigned(h - 1)), rows});
        }
        if (check(im)) return 1;
        plans++;
    }
    // fields out of range: refused, and the plan left empty
    const BuildPlanImage good{0, 1, 23, 149, 3, 23};
    const BuildPlanImage bad[] = {{0, 1, 23, 149, 0, 23}, {0, 1, 23, 149, 23, 23}, {0, 1, 23, 149, -1, 23}, {0, 0, 23, 149, 3, 23}, {0, 4, 23, 149, 3, 23},
                                  {1, 1, 23, 149, 3, 23}, {2, 1, 23, 149, 3, 23}, {0, 1, 0, 149, 3, 23}, {0, 1, 23, 0, 3, 23}, {0, 1, 65536, 149, 3, 23},
                                  {0, 1, 23, 65536, 3, 23}, {0, 1, 1, 149, 1, 1}, {0, 1, 23, 149, 3, 0}, {0, 1, 23, 149, 3, -4}};
    for (const BuildPlanImage &b : bad) {
        BuildPlan P;
        const BuildPlanImage two[2] = {good, b}, owt[2] = {b, good};
        CHECK(!index_build_plan(&b, 1, P) && P.entries.empty());
        CHECK(!index_build_plan(two, 2, P) && P.entries.empty());
        CHECK(!index_build_plan(owt, 2, P) && P.entries.empty());
    }
    BuildPlan P;
    CHECK(!index_build_plan(&good, 0, P) && !index_build_plan(nullptr, 1, P));
    printf("index_build_plan_check ok: %d random plans\n", plans);
    return 0;
}
