// grouped_host.h — the host-only pieces of mi_knn_search_grouped (grouped.hip): the argument rules, the rule for group ids,
// the choice between the two forms of the reduce pass and its grid ("group_lds_max", "group_blocks"), the layout of the one
// record the device writes with how it (or "no candidate") reaches the caller's arrays, and what the sharded call does on the
// host: the merge of the shards' representatives by group id and the sums over the shards' per-group counts.  No HIP in here:
// tests/cpp/test_grouped_host.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mi355clip.h"
#include "page_host.h"

namespace mi {

// The block-private form of the reduce pass keeps 12 bytes per group (a 64-bit best key, a 32-bit count) in LDS.  4096 groups
// are 48 KiB: two workgroups fit the 160 KiB of a CU with room to spare, and the launch needs no raised LDS limit.
constexpr uint32_t GROUP_LDS_MAX = 4096;
constexpr size_t GROUP_SLOT_BYTES = 12;

// MI_OK, or the error the contract names with *why set: pointers, the bound (MI_ERR_INVALID), then k (0: MI_ERR_INVALID, above
// 4096: MI_ERR_UNSUPPORTED).  What needs the table — the dim, "every id of among is a row", cap_facets >= n_groups — is
// judged under the handle's lock.
inline int grouped_check_args(const void* t, const float* q, uint32_t k, float max_dist, const void* among, uint64_t n_among,
                              const void* idx, const void* dist, const char** why) {
    return page_check_args(t, q, k, 0.0f, MI_KNN_NO_ID, max_dist, among, n_among, idx, dist, why);
}

// a group id a row may hold: below MI_KNN_GROUPS_MAX, or "none"
inline bool grouped_id_ok(uint32_t g) { return g < MI_KNN_GROUPS_MAX || g == MI_KNN_NO_GROUP; }
// the first of n group ids that is out of range, or n
inline uint64_t grouped_first_bad(const uint32_t* groups, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (!grouped_id_ok(groups[i])) return i;
    return n;
}

// block-private LDS tables when the groups fit the option (0 forces the global form)
inline bool grouped_use_lds(uint64_t n_groups, uint32_t lds_max) { return n_groups >= 1 && n_groups <= std::min(lds_max, GROUP_LDS_MAX); }

// workgroups of the reduce and mark passes over n keys (a workgroup takes 256 at a time): option 0 = four per CU, v >= 1 =
// exactly min(v, needed)
inline uint32_t grouped_grid(uint64_t n, int n_cu, int option) {
    const uint64_t needed = std::max<uint64_t>(1, (n + 255) / 256);
    const uint64_t want = option >= 1 ? (uint64_t)option : (uint64_t)std::max(n_cu, 1) * 4;
    return (uint32_t)std::min(want, needed);
}

// The record: idx [k] u64 | totals [4] u64 = {representatives, window, beyond, nan} | members [k] u64 | dist [k] f32 |
// group [k] u32
struct GroupedRecord {
    size_t idx, totals, members, dist, group, bytes;
};
inline GroupedRecord grouped_record(uint32_t k) {
    GroupedRecord r;
    r.idx = 0;
    r.totals = (size_t)k * sizeof(uint64_t);
    r.members = r.totals + 4 * sizeof(uint64_t);
    r.dist = r.members + (size_t)k * sizeof(uint64_t);
    r.group = r.dist + (size_t)k * sizeof(float);
    r.bytes = r.group + (size_t)k * sizeof(uint32_t);
    return r;
}
inline void grouped_unpack(const unsigned char* rec, uint32_t k, uint64_t* idx, float* dist, uint32_t* group /* nullable */,
                           uint64_t* members /* nullable */, uint64_t* totals /* nullable */) {
    const GroupedRecord r = grouped_record(k);
    std::memcpy(idx, rec + r.idx, (size_t)k * sizeof(uint64_t));
    std::memcpy(dist, rec + r.dist, (size_t)k * sizeof(float));
    if (group) std::memcpy(group, rec + r.group, (size_t)k * sizeof(uint32_t));
    if (members) std::memcpy(members, rec + r.members, (size_t)k * sizeof(uint64_t));
    if (totals) std::memcpy(totals, rec + r.totals, 4 * sizeof(uint64_t));
}

// no candidate at all: all padding, every total 0
inline void grouped_pad(uint32_t k, uint64_t* idx, float* dist, uint32_t* group, uint64_t* members, uint64_t* totals) {
    for (uint32_t j = 0; j < k; ++j) {
        idx[j] = MI_KNN_NO_ID;
        dist[j] = std::numeric_limits<float>::infinity();
        if (group) group[j] = MI_KNN_NO_GROUP;
        if (members) members[j] = 0;
    }
    if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
}

// The group of an image in the index: its directory — the path up to and including its last '/' ("" for a bare name), so
// "a/b/c.jpg" and "a/b/d.jpg" share a group, "a/bb/c.jpg" does not, and the files directly in the media directory form one.
inline std::string grouped_dir_of(const std::string& path) {
    const size_t slash = path.find_last_of('/');
    return slash == std::string::npos ? std::string() : path.substr(0, slash + 1);
}
// directory <-> group id, ids in first-seen order
struct GroupDict {
    std::vector<std::string> names;
    std::unordered_map<std::string, uint32_t> ids;
    uint32_t of_path(const std::string& path) {
        const std::string dir = grouped_dir_of(path);
        auto it = ids.find(dir);
        if (it != ids.end()) return it->second;
        const uint32_t g = (uint32_t)names.size();
        ids.emplace(dir, g);
        names.push_back(dir);
        return g;
    }
};

// The sharded merge.  in: n_lists lists of k entries (global id, distance, group), each what mi_knn_search_grouped leaves.  A
// group's entries (one per list at most) collapse to the one with the smallest (distance word, id); entries without a group
// never merge.  out: the k smallest by (distance word, id), then padding.  Exact: in the list that holds a group's global
// best, every group ranked ahead of it there is ranked ahead of it globally, so a global top-k group is in that list's top k.
inline void grouped_merge(const uint64_t* all_idx, const float* all_dist, const uint32_t* all_group, uint32_t n_lists, uint32_t k,
                          uint64_t* idx, float* dist, uint32_t* group) {
    struct Hit {
        uint32_t key;
        uint64_t id;
        uint32_t group;
        bool operator<(const Hit& o) const { return key != o.key ? key < o.key : id < o.id; }
    };
    std::vector<Hit> hits;
    std::unordered_map<uint32_t, size_t> at;   // group -> its entry in hits
    for (size_t e = 0; e < (size_t)n_lists * k; ++e) {
        if (all_idx[e] == MI_KNN_NO_ID) continue;
        const Hit h{page_dist_key(all_dist[e]), all_idx[e], all_group[e]};
        if (h.group == MI_KNN_NO_GROUP) { hits.push_back(h); continue; }
        auto it = at.find(h.group);
        if (it == at.end()) { at.emplace(h.group, hits.size()); hits.push_back(h); }
        else if (h < hits[it->second]) hits[it->second] = h;
    }
    std::sort(hits.begin(), hits.end());
    for (uint32_t j = 0; j < k; ++j) {
        const bool hit = j < hits.size();
        idx[j] = hit ? hits[j].id : MI_KNN_NO_ID;
        // a key maps back to one float: the bits the shard reported
        uint32_t b = 0x7F800000u;
        if (hit) b = (hits[j].key & 0x80000000u) ? (hits[j].key & 0x7FFFFFFFu) : ~hits[j].key;
        std::memcpy(&dist[j], &b, sizeof b);
        group[j] = hit ? hits[j].group : MI_KNN_NO_GROUP;
    }
}

// The sums over the shards' per-group counts (cnt[s][g] = in-window candidates of group g in shard s, a shard's array may be
// shorter than n_groups) and their representative counts (reps[s] = its matched groups + its matched singletons):
// facets (nullable) [n_groups] = the summed counts, returns the table's representatives — a group matched in several shards
// counts once.
inline uint64_t grouped_sum_counts(const std::vector<std::vector<uint32_t>>& cnt, const uint64_t* reps, uint64_t n_groups,
                                   uint64_t* facets) {
    std::vector<uint64_t> sum((size_t)n_groups, 0);
    uint64_t total = 0;
    for (size_t s = 0; s < cnt.size(); ++s) {
        uint64_t matched = 0;
        for (size_t g = 0; g < cnt[s].size(); ++g) {
            if (!cnt[s][g]) continue;
            ++matched;
            if (g < sum.size()) sum[g] += cnt[s][g];
        }
        total += reps[s] - matched;   // this shard's matched singletons
    }
    for (uint64_t g = 0; g < n_groups; ++g) {
        if (sum[(size_t)g]) ++total;
        if (facets) facets[g] = sum[(size_t)g];
    }
    return total;
}

}  // namespace mi
