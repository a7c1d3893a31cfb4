// Stand-alone host test of image_search_amd/csrc/compact_host.h: the old-to-new map, the source rule, the chunk plan and the
// host columns of mi_knn_compact against brute-force restatements, and every plan REPLAYED on an array of row numbers with
// adversarial write orders — the check that the straight / staged decision is safe.  Built with the address and
// undefined-behaviour sanitizers by tests/test_compact_host.py; needs neither the library nor a GPU.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../image_search_amd/csrc/compact_host.h"

using namespace mi;

static int failures = 0;
#define CHECK(c, ...)                                                   \
    do {                                                                \
        if (!(c)) {                                                     \
            ++failures;                                                 \
            std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c);  \
            std::printf(__VA_ARGS__);                                   \
            std::printf("\n");                                          \
        }                                                               \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

struct Pattern {
    std::string name;
    std::vector<uint32_t> dead;
};

static std::vector<Pattern> patterns(uint64_t rows, uint64_t S) {
    std::vector<Pattern> v;
    auto run = [&](uint64_t a, uint64_t n) {
        std::vector<uint32_t> d;
        for (uint64_t r = a; r < a + n && r < rows; ++r) d.push_back((uint32_t)r);
        return d;
    };
    v.push_back({"none", {}});
    if (rows) v.push_back({"row 0 only", {0}});
    if (rows) v.push_back({"last row only", {(uint32_t)(rows - 1)}});
    {
        std::vector<uint32_t> d;
        for (uint64_t r = 0; r < rows; r += 2) d.push_back((uint32_t)r);
        v.push_back({"every other row", d});
        d.clear();
        for (uint64_t r = 1; r < rows; r += 2) d.push_back((uint32_t)r);
        v.push_back({"every other row, odd", d});
    }
    v.push_back({"a run longer than S", run(rows / 5, S + 3)});
    v.push_back({"a run exactly S", run(rows / 5, S)});
    v.push_back({"a run exactly S from row 0", run(0, S)});
    v.push_back({"everything", run(0, rows)});
    v.push_back({"the tail only", run(rows - rows / 7, rows)});
    for (int pct : {1, 10, 50, 90}) {
        std::vector<uint32_t> d;
        for (uint64_t r = 0; r < rows; ++r)
            if (rnd() % 100 < (uint64_t)pct) d.push_back((uint32_t)r);
        v.push_back({"random " + std::to_string(pct) + " %", d});
    }
    return v;
}

// chunk [j0, j1) straight into place, its writes in the given order: a[j] = a[src(j)]
static void replay_straight(std::vector<uint32_t>& a, const std::vector<uint32_t>& dead, const CompactChunk& c, int order) {
    const uint64_t n = c.j1 - c.j0;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t j;
        if (order == 0) j = c.j0 + i;                        // ascending
        else if (order == 1) j = c.j1 - 1 - i;               // descending: the order that shows a source overwritten too early
        else j = c.j0 + (i % 2 ? n - 1 - i / 2 : i / 2);     // from both ends inwards
        a[j] = a[compact_src(dead, j)];
    }
}

static void check_case(uint64_t rows, uint64_t S, const Pattern& p) {
    const std::vector<uint32_t>& dead = p.dead;
    const char* nm = p.name.c_str();
    // brute force: the survivors in order, and the map
    std::vector<uint32_t> live;
    std::vector<uint64_t> want_map(rows);
    {
        std::vector<char> gone(rows, 0);
        for (uint32_t d : dead) gone[d] = 1;
        for (uint64_t r = 0; r < rows; ++r) {
            want_map[r] = gone[r] ? COMPACT_NO_ID : 1000 + live.size();
            if (!gone[r]) live.push_back((uint32_t)r);
        }
    }
    std::vector<uint64_t> map(rows + 1, 0x5555);
    compact_map(dead, rows, 1000, map.data());
    for (uint64_t r = 0; r < rows; ++r) CHECK(map[r] == want_map[r], "%s rows %llu: map[%llu]", nm, (unsigned long long)rows, (unsigned long long)r);
    CHECK(map[rows] == 0x5555, "%s: the map wrote past its end", nm);
    for (uint64_t j = 0; j < live.size(); ++j)
        CHECK(compact_src(dead, j) == live[j], "%s rows %llu: src(%llu) = %llu, want %u", nm, (unsigned long long)rows, (unsigned long long)j,
              (unsigned long long)compact_src(dead, j), live[j]);

    const CompactPlan plan = compact_plan(dead, rows, S);
    CHECK(plan.live == live.size(), "%s: live", nm);
    CHECK(plan.first == (dead.empty() ? rows : dead[0]), "%s: first", nm);
    CHECK(plan.first <= plan.live, "%s: first beyond live", nm);
    CHECK(plan.n_straight + plan.n_staged == plan.chunks.size(), "%s: counts", nm);
    // the chunks tile [first, live) in ascending order, none longer than S, and the decision is the rule restated
    uint64_t at = plan.first, staged = 0;
    for (const CompactChunk& c : plan.chunks) {
        CHECK(c.j0 == at && c.j1 > c.j0 && c.j1 - c.j0 <= S && c.j1 <= plan.live, "%s: chunk [%llu, %llu)", nm, (unsigned long long)c.j0, (unsigned long long)c.j1);
        CHECK(c.staged == (live[c.j0] < c.j1), "%s: decision of chunk at %llu", nm, (unsigned long long)c.j0);
        if (c.staged) { ++staged; CHECK(c.j1 - c.j0 <= plan.stage_rows, "%s: staging buffer too small", nm); }
        at = c.j1;
    }
    if (plan.first >= plan.live) CHECK(plan.chunks.empty(), "%s: nothing to move, yet chunks", nm);
    else CHECK(at == plan.live, "%s: chunks stop at %llu of %llu", nm, (unsigned long long)at, (unsigned long long)plan.live);
    CHECK(staged == plan.n_staged, "%s: staged count", nm);

    // replay: rows hold their own number; chunks in order; a straight chunk's writes in three orders, a staged chunk through a buffer
    for (int order = 0; order < 3; ++order) {
        std::vector<uint32_t> a(rows);
        for (uint64_t r = 0; r < rows; ++r) a[r] = (uint32_t)r;
        std::vector<uint32_t> stage(plan.stage_rows, 0xFFFFFFFFu);
        for (const CompactChunk& c : plan.chunks) {
            if (!c.staged) replay_straight(a, dead, c, order);
            else {
                for (uint64_t j = c.j0; j < c.j1; ++j) stage[j - c.j0] = a[compact_src(dead, j)];
                for (uint64_t i = 0; i < c.j1 - c.j0; ++i) {
                    const uint64_t j = order == 1 ? c.j1 - 1 - i : c.j0 + i;
                    a[j] = stage[j - c.j0];
                }
            }
        }
        bool same = true;
        for (uint64_t j = 0; j < live.size(); ++j) same = same && a[j] == live[j];
        CHECK(same, "%s rows %llu S %llu order %d: the replay does not leave the survivors in order", nm, (unsigned long long)rows,
              (unsigned long long)S, order);
    }

    // a host column, full length and shorter than the table
    for (uint64_t len : {rows, rows / 2, (uint64_t)0}) {
        std::vector<uint64_t> col(len);
        for (uint64_t r = 0; r < len; ++r) col[r] = r * 3 + 1;
        size_t left = 0;
        for (uint32_t d : dead) left += d < len;
        CHECK(compact_column(col, dead) == left, "%s: entries that left", nm);
        CHECK(col.size() == len - left, "%s: column length", nm);
        bool same = true;
        for (size_t j = 0; j < col.size(); ++j) same = same && col[j] == (uint64_t)live[j] * 3 + 1;
        CHECK(same, "%s: column of %llu", nm, (unsigned long long)len);
    }
}

int main() {
    for (uint64_t rows : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)63, (uint64_t)64, (uint64_t)65, (uint64_t)1157}) {
        for (uint64_t S : {(uint64_t)1, (uint64_t)64, rows, rows + 17}) {
            if (S == 0) continue;
            for (const Pattern& p : patterns(rows, S)) check_case(rows, S, p);
        }
    }
    // the default chunk: a fixed staging buffer, and never more than one launch indexes
    CHECK(compact_chunk_rows(0, 768) == (64ull << 20) / 3072, "default chunk at dim 768");
    CHECK(compact_chunk_rows(0, 768) * 3072 <= COMPACT_STAGE_BYTES, "staging buffer");
    CHECK(compact_chunk_rows(64, 768) == 64, "option");
    for (uint32_t dim : {64u, 128u, 256u, 768u, 1024u, 4096u})
        CHECK(compact_chunk_rows(0x7FFFFFFF, dim) * (dim / 4) <= COMPACT_MAX_PIECES && compact_chunk_rows(0, dim) >= 1, "piece index at dim %u", dim);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
