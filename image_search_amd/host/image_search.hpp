// image_search.hpp — C++ host-side mirror of the reference's interface for the hot path, on top of
// the C ABI (include/mi355clip.h).  The reference is Rust (no toolchain in this image), so the
// compiled-language host layer is C++: same names, argument meaning and error behaviour as
//   clip::clip_vit_large_patch14::Model::{from_file, forward}   clip/src/lib.rs:2-7, server/src/clip.rs:46-48,:118
//   average_slices                                              server/src/search.rs:127-150
//   image_prepare_resnet (arithmetic)                           server/src/clip.rs:158-172
//   the `embedding <|K|> $reference` statement                  server/src/search.rs:70-86
// Where the reference panics (assert!/unwrap) this throws std::runtime_error with the same message.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mi355clip.h"

namespace image_search {

inline void check(int rc) {
    if (rc != MI_OK) throw std::runtime_error(std::string("mi355clip: ") + mi_last_error());
}

// fn average_slices(vectors: &Vec<&Vec<f32>>) -> Vec<f32>
inline std::vector<float> average_slices(const std::vector<const std::vector<float>*>& vectors) {
    if (vectors.empty()) throw std::runtime_error("Input must not be empty");
    const size_t len = vectors[0]->size();
    std::vector<const float*> ptrs;
    for (auto v : vectors) {
        if (v->size() != len) throw std::runtime_error("All vectors must have the same length");
        ptrs.push_back(v->data());
    }
    std::vector<float> out(len);
    check(mi_average_slices(ptrs.data(), ptrs.size(), len, out.data()));
    return out;
}

// the extension allow-list of the ingest walk (server/src/clip.rs:60-66, test_matches :181-233)
inline bool is_image_path(const std::string& path) {
    const size_t slash = path.find_last_of("/\\");
    const std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
    const size_t dot = name.rfind('.');
    if (dot == std::string::npos || dot == 0) return false;
    std::string ext = name.substr(dot + 1);
    for (auto& c : ext) c = (char)std::tolower((unsigned char)c);
    for (const char* e : {"jpg", "jpeg", "png", "gif", "bmp", "webp", "tiff"})
        if (ext == e) return true;
    return false;
}

// fn image_prepare_resnet(img) -> Vec<f32>, minus the resize: RGB8 HWC (224x224) -> CHW f32
inline std::vector<float> image_prepare_resnet(const std::vector<uint8_t>& rgb8, uint32_t h = 224, uint32_t w = 224) {
    if (rgb8.size() != (size_t)h * w * 3) throw std::runtime_error("rgb8 buffer is not h*w*3 bytes");
    std::vector<float> out((size_t)h * w * 3);
    check(mi_preprocess_rgb8(rgb8.data(), 1, h, w, out.data()));
    return out;
}

// image_prepare_resnet whole (clip.rs:153-175): one decoded RGB8 image of any size -> CHW f32 [3][224][224]
inline std::vector<float> image_prepare_resnet(const uint8_t* rgb8, uint32_t width, uint32_t height, int device = 0) {
    std::vector<float> out((size_t)3 * 224 * 224);
    check(mi_image_prepare_resnet(device, rgb8, width, height, out.data()));
    return out;
}

namespace clip_vit_large_patch14 {
class Model {
    mi_clip* h_ = nullptr;
    uint32_t info_[8] = {0};
    explicit Model(mi_clip* h) : h_(h) { check(mi_clip_info(h_, info_)); }

   public:
    static Model from_file(const std::string& path, int device, int precision = MI_PRECISION_BF16) {
        mi_clip* h = nullptr;
        check(mi_clip_load(path.c_str(), device, precision, &h));
        return Model(h);
    }
    Model(Model&& o) noexcept { *this = std::move(o); }
    Model& operator=(Model&& o) noexcept { std::swap(h_, o.h_); std::swap(info_, o.info_); return *this; }
    Model(const Model&) = delete;
    ~Model() { mi_clip_free(h_); }
    uint32_t image() const { return info_[0]; }
    uint32_t proj() const { return info_[7]; }
    mi_clip* handle() const { return h_; }
    // [n,3,H,W] f32 NCHW -> [n,proj] f32, flat (what `output.to_data()` + cast gives, clip.rs:120-124)
    std::vector<float> forward(const std::vector<float>& nchw, size_t n) const {
        if (nchw.size() != n * 3 * (size_t)image() * image()) throw std::runtime_error("input is not [n,3,H,W]");
        std::vector<float> out(n * proj());
        check(mi_clip_embed(h_, nchw.data(), n, out.data()));
        return out;
    }
    // one chunk of the scan loop (clip.rs:92-124): decoded RGB8 images of any sizes -> [n,proj] f32;
    // CatmullRom resize_exact + normalisation + tower on the device
    struct Rgb8 { const uint8_t* data; uint32_t width, height; };
    std::vector<float> forward_images(const std::vector<Rgb8>& images) const {
        std::vector<const uint8_t*> p;
        std::vector<uint32_t> w, h;
        for (const auto& im : images) { p.push_back(im.data); w.push_back(im.width); h.push_back(im.height); }
        std::vector<float> out(images.size() * proj());
        check(mi_clip_embed_images(h_, p.data(), w.data(), h.data(), images.size(), out.data()));
        return out;
    }
};
}  // namespace clip_vit_large_patch14

// table `image` + index `mt_pts` (server/src/clip.rs:135-143) as one HBM-resident shard
// one page of results (mi_knn_search_page and its kin): the hits without the padding, counts = {before, window, beyond, nan} of
// the candidates, and the cursor for the following page — has_next is false when this page came back short
struct Page {
    std::vector<uint64_t> idx;
    std::vector<float> dist;
    uint64_t counts[4] = {0, 0, 0, 0};
    bool has_next = false;
    float next_dist = 0.0f;
    uint64_t next_id = MI_KNN_NO_ID;
};
inline void finish_page(Page& p, uint32_t k) {
    p.has_next = k > 0 && p.idx[k - 1] != MI_KNN_NO_ID;
    if (p.has_next) { p.next_dist = p.dist[k - 1]; p.next_id = p.idx[k - 1]; }   // the float as it came: -0 and +0 are different cursors
    size_t n = 0;
    while (n < p.idx.size() && p.idx[n] != MI_KNN_NO_ID) ++n;
    p.idx.resize(n); p.dist.resize(n);
}

// the best hit per group (mi_knn_search_grouped and its kin): the hits without the padding — group[j] = MI_KNN_NO_GROUP for a row
// that stands for itself, members[j] = the group's candidates within the bound — totals = {representatives, window, beyond,
// nan}, and facets (when asked for) = every group's count
struct Grouped {
    std::vector<uint64_t> idx, members, facets;
    std::vector<float> dist;
    std::vector<uint32_t> group;
    uint64_t totals[4] = {0, 0, 0, 0};
};
inline void finish_grouped(Grouped& g) {
    size_t n = 0;
    while (n < g.idx.size() && g.idx[n] != MI_KNN_NO_ID) ++n;
    g.idx.resize(n); g.dist.resize(n); g.group.resize(n); g.members.resize(n);
}

// a predicate search (mi_knn_search_where and its kin): the hits without the padding, and how many rows qualified
struct WhereHits {
    std::vector<uint64_t> idx;
    std::vector<float> dist;
    uint64_t matched = 0;
};
inline void finish_where(WhereHits& r) {
    size_t n = 0;
    while (n < r.idx.size() && r.idx[n] != MI_KNN_NO_ID) ++n;
    r.idx.resize(n); r.dist.resize(n);
}
// every tag, every stamp, any group: narrow the fields that matter (flags = MI_KNN_WHERE_GROUP makes `group` count)
inline mi_knn_where where_all() { return mi_knn_where{0, 0, 0, INT64_MIN, INT64_MAX, 0, 0}; }

// one page of a timeline (mi_knn_search_ordered and its kin): the hits without the padding in the order of their stamps, counts =
// {within, before, beyond, nan} of the candidates, and the cursor for the following page — has_next is false when this page came
// back short
struct OrderedPage {
    std::vector<uint64_t> idx;
    std::vector<float> dist;
    std::vector<int64_t> stamps;
    uint64_t counts[4] = {0, 0, 0, 0};
    bool has_next = false;
    int64_t next_stamp = 0;
    uint64_t next_id = 0;
};
inline void finish_ordered(OrderedPage& p, uint32_t k) {
    p.has_next = k > 0 && p.idx[k - 1] != MI_KNN_NO_ID;
    if (p.has_next) { p.next_stamp = p.stamps[k - 1]; p.next_id = p.idx[k - 1]; }
    size_t n = 0;
    while (n < p.idx.size() && p.idx[n] != MI_KNN_NO_ID) ++n;
    p.idx.resize(n); p.dist.resize(n); p.stamps.resize(n);
}
inline uint32_t ordered_flags(bool descending, const OrderedPage* after) {
    return (descending ? MI_KNN_ORDER_DESC : 0u) | (after && after->has_next ? MI_KNN_ORDER_AFTER : 0u);
}

class EmbeddingTable {
    mi_knn* h_ = nullptr;
    uint32_t dim_;

   public:
    explicit EmbeddingTable(uint32_t dim = 768, int device = 0, uint64_t base = 0) : dim_(dim) {
        check(mi_knn_create(dim, device, &h_));
        check(mi_knn_set_base(h_, base));
    }
    EmbeddingTable(const EmbeddingTable&) = delete;
    ~EmbeddingTable() { mi_knn_free(h_); }
    void insert(const std::vector<float>& rows) { check(mi_knn_append(h_, rows.data(), rows.size() / dim_)); }
    uint64_t size() const { uint64_t n = 0; check(mi_knn_size(h_, &n)); return n; }
    // DELETE FROM image WHERE id IN $ids: returns the rows that were live; ids stay, searches leave the rows out
    uint64_t remove_ids(const std::vector<uint64_t>& ids) { uint64_t n = 0; check(mi_knn_delete(h_, ids.data(), ids.size(), &n)); return n; }
    std::vector<uint64_t> deleted() const {
        uint64_t n = 0;
        check(mi_knn_deleted(h_, nullptr, 0, &n));
        std::vector<uint64_t> v(n);
        if (n) check(mi_knn_deleted(h_, v.data(), n, &n));
        return v;
    }
    // the deleted rows leave the table physically (mi_knn_compact); returns the old-to-new id map, [rows before the call],
    // MI_KNN_NO_ID for a deleted row: every id held outside the table (labels, cursors) must go through it
    std::vector<uint64_t> compact(uint64_t* removed = nullptr) {
        std::vector<uint64_t> new_ids(size());
        check(mi_knn_compact(h_, new_ids.data(), new_ids.size(), removed));
        return new_ids;
    }
    // {rows removed, rows moved, chunks gathered in place, chunks staged} of the last compact
    std::vector<uint64_t> compact_stats() const { std::vector<uint64_t> v(4); check(mi_knn_compact_stats(h_, v.data())); return v; }
    // what the database's storage did for the reference: one file per shard
    void save(const std::string& path) const { check(mi_knn_save(h_, path.c_str())); }
    void load(const std::string& path) { check(mi_knn_load(h_, path.c_str())); }
    // `WHERE embedding <|k|> $reference`: ids and cosine distances, ascending
    std::pair<std::vector<uint64_t>, std::vector<float>> knn(const std::vector<float>& reference, uint32_t k = 1000) const {
        std::vector<uint64_t> idx(k);
        std::vector<float> dist(k);
        check(mi_knn_search(h_, reference.data(), 1, k, idx.data(), dist.data()));
        return {idx, dist};
    }
    mi_knn* handle() const { return h_; }
    // near-duplicates (mi_knn_near_pairs): every pair of live rows a < b with cosine distance <= max_dist, ascending by
    // (a, b), with the distance knn(row a) reports for row b; first_new: only pairs with b >= first_new
    struct NearPairs { std::vector<uint64_t> a, b; std::vector<float> dist; };
    NearPairs near_pairs(float max_dist, uint64_t first_new = 0, uint64_t cap = 1ull << 20) const {
        NearPairs r;
        r.a.resize(cap); r.b.resize(cap); r.dist.resize(cap);
        uint64_t n = 0;
        check(mi_knn_near_pairs(h_, max_dist, first_new, r.a.data(), r.b.data(), r.dist.data(), cap, &n));
        r.a.resize(n); r.b.resize(n); r.dist.resize(n);
        return r;
    }
    // {candidate pairs, pairs accepted, strips run, tiles visited} of the last near_pairs
    std::vector<uint64_t> near_pairs_stats() const { std::vector<uint64_t> v(4); check(mi_knn_near_pairs_stats(h_, v.data())); return v; }
    // bursts (mi_knn_near_pairs_window): the pairs of near_pairs whose stamps (set_attrs) lie within `window` of each other,
    // |stamp_a - stamp_b| <= window taken exactly; 0: equal stamps, UINT64_MAX: every pair.  Same ids, order and distance bits
    NearPairs near_pairs_window(float max_dist, uint64_t window, uint64_t first_new = 0, uint64_t cap = 1ull << 20) const {
        NearPairs r;
        r.a.resize(cap); r.b.resize(cap); r.dist.resize(cap);
        uint64_t n = 0;
        check(mi_knn_near_pairs_window(h_, max_dist, window, first_new, r.a.data(), r.b.data(), r.dist.data(), cap, &n));
        r.a.resize(n); r.b.resize(n); r.dist.resize(n);
        return r;
    }
    // {candidates pass 1, pairs within, tiles computed pass 1, tiles skipped by the stamp ranges pass 1, candidates pass 2, tiles
    // computed pass 2, tiles skipped pass 2, stage-1 launches} of the last near_pairs_window / neighbor_counts_window / dbscan_window
    std::vector<uint64_t> window_stats() const { std::vector<uint64_t> v(8); check(mi_knn_window_stats(h_, v.data())); return v; }
    // the join with another table (mi_knn_near_pairs_between): every pair of a live row of this table (a, the query) and a live
    // row of `other` (b) with cosine distance <= max_dist, ascending by (a, b); neither table changes
    NearPairs near_pairs_with(const EmbeddingTable& other, float max_dist, uint64_t cap = 1ull << 20) const {
        NearPairs r;
        r.a.resize(cap); r.b.resize(cap); r.dist.resize(cap);
        uint64_t n = 0;
        check(mi_knn_near_pairs_between(h_, other.h_, max_dist, r.a.data(), r.b.data(), r.dist.data(), cap, &n));
        r.a.resize(n); r.b.resize(n); r.dist.resize(n);
        return r;
    }
    // {candidate pairs, pairs accepted, stage-1 launches, tiles computed} of the last near_pairs_with
    std::vector<uint64_t> near_pairs_with_stats() const { std::vector<uint64_t> v(4); check(mi_knn_near_pairs_between_stats(h_, v.data())); return v; }
    // how crowded it is around every row (mi_knn_density): the pairs of near_pairs(max_dist) that contain the row, by local row;
    // 0 for a deleted row and for an outlier.  No pair list is built
    std::vector<uint32_t> neighbor_counts(float max_dist) const {
        std::vector<uint32_t> counts(size());
        uint32_t none = 0;
        check(mi_knn_density(h_, max_dist, counts.empty() ? &none : counts.data()));
        return counts;
    }
    // density clusters without a k (mi_knn_dbscan), arrays by local row: labels 0 .. C - 1 in the order of the clusters' smallest
    // core ids (-1: noise or deleted, as scikit-learn numbers them), cluster = the id of the cluster's smallest core row, via =
    // a core's own id / the core a border row joined through, via_dist = +0 / that pair's distance bits / +inf, counts = the
    // neighbours within, summary = {clusters, core rows, border rows, noise rows}.  The labels fit set_groups
    struct Dbscan {
        std::vector<int64_t> labels;
        std::vector<uint64_t> cluster, via;
        std::vector<float> via_dist;
        std::vector<uint32_t> counts;
        uint64_t summary[4] = {0, 0, 0, 0};
    };
    Dbscan dbscan(float max_dist, uint32_t min_pts = 5) const {
        Dbscan r;
        const uint64_t n = size();
        r.cluster.resize(n + 1); r.via.resize(n + 1); r.via_dist.resize(n + 1); r.counts.resize(n + 1);   // (+ 1: never a null pointer)
        check(mi_knn_dbscan(h_, max_dist, min_pts, r.cluster.data(), r.via.data(), r.via_dist.data(), r.counts.data(), r.summary));
        dbscan_trim_and_label(r, n);
        return r;
    }
    // neighbor_counts and dbscan over the pairs of near_pairs_window (mi_knn_density_window, mi_knn_dbscan_window): the
    // neighbourhood is "within max_dist and within `window` in time" — a theme shot in two far-apart periods is two clusters
    std::vector<uint32_t> neighbor_counts_window(float max_dist, uint64_t window) const {
        std::vector<uint32_t> counts(size());
        uint32_t none = 0;
        check(mi_knn_density_window(h_, max_dist, window, counts.empty() ? &none : counts.data()));
        return counts;
    }
    Dbscan dbscan_window(float max_dist, uint64_t window, uint32_t min_pts = 5) const {
        Dbscan r;
        const uint64_t n = size();
        r.cluster.resize(n + 1); r.via.resize(n + 1); r.via_dist.resize(n + 1); r.counts.resize(n + 1);   // (+ 1: never a null pointer)
        check(mi_knn_dbscan_window(h_, max_dist, window, min_pts, r.cluster.data(), r.via.data(), r.via_dist.data(), r.counts.data(),
                                   r.summary));
        dbscan_trim_and_label(r, n);
        return r;
    }
    // the arrays cut back to n rows and the dense labels from the cluster ids (shared with ShardedTable::dbscan)
    static void dbscan_trim_and_label(Dbscan& r, uint64_t n) {
        r.cluster.resize(n); r.via.resize(n); r.via_dist.resize(n); r.counts.resize(n);
        std::vector<uint64_t> names;
        for (uint64_t c : r.cluster) if (c != MI_KNN_NO_ID) names.push_back(c);
        std::sort(names.begin(), names.end());
        names.erase(std::unique(names.begin(), names.end()), names.end());
        r.labels.assign(n, -1);
        for (uint64_t i = 0; i < n; ++i)
            if (r.cluster[i] != MI_KNN_NO_ID) r.labels[i] = (int64_t)(std::lower_bound(names.begin(), names.end(), r.cluster[i]) - names.begin());
    }
    // neighbor_counts at several distances from one tile pass (mi_knn_density_levels): [levels][rows], slice l =
    // neighbor_counts(max_dists[l]).  max_dists: strictly ascending, at most MI_KNN_LEVELS_MAX of them
    std::vector<uint32_t> neighbor_counts_levels(const std::vector<float>& max_dists) const {
        std::vector<uint32_t> counts(max_dists.size() * size() + 1);   // (+ 1: never a null pointer)
        check(mi_knn_density_levels(h_, max_dists.data(), (uint32_t)max_dists.size(), counts.data()));
        counts.resize(max_dists.size() * size());
        return counts;
    }
    // dbscan at several distances from the two tile passes one call runs (mi_knn_dbscan_levels): levels[l] is what
    // dbscan(max_dists[l], min_pts) returns, to the bit.  tree (mi_dbscan_levels_tree): one edge per cluster of every level below
    // the top, ascending by (level, child cluster id); parent = the cluster id one level up that holds the child's core rows — a
    // border row may sit in a cluster that is not its lower cluster's parent
    struct TreeEdge { uint32_t level; uint64_t child, parent; };
    struct DbscanLevels {
        std::vector<Dbscan> levels;
        std::vector<TreeEdge> tree;
    };
    DbscanLevels dbscan_levels(const std::vector<float>& max_dists, uint32_t min_pts = 5) const {
        const uint64_t n = size(), L = max_dists.size();
        std::vector<uint64_t> cluster(L * n + 1), via(L * n + 1), summary(L * 4 + 1);
        std::vector<float> via_dist(L * n + 1);
        std::vector<uint32_t> counts(L * n + 1);
        check(mi_knn_dbscan_levels(h_, max_dists.data(), (uint32_t)L, min_pts, cluster.data(), via.data(), via_dist.data(), counts.data(),
                                   summary.data()));
        DbscanLevels r;
        r.levels.resize(L);
        for (uint64_t l = 0; l < L; ++l) {
            Dbscan& d = r.levels[l];
            d.cluster.assign(cluster.begin() + l * n, cluster.begin() + (l + 1) * n);
            d.via.assign(via.begin() + l * n, via.begin() + (l + 1) * n);
            d.via_dist.assign(via_dist.begin() + l * n, via_dist.begin() + (l + 1) * n);
            d.counts.assign(counts.begin() + l * n, counts.begin() + (l + 1) * n);
            for (int i = 0; i < 4; ++i) d.summary[i] = summary[4 * l + i];
            dbscan_trim_and_label(d, n);
        }
        uint64_t n_edges = 0;
        check(mi_dbscan_levels_tree(cluster.data(), counts.data(), n, (uint32_t)L, min_pts, nullptr, nullptr, nullptr, 0, &n_edges));
        std::vector<uint32_t> level(n_edges + 1);
        std::vector<uint64_t> child(n_edges + 1), parent(n_edges + 1);
        check(mi_dbscan_levels_tree(cluster.data(), counts.data(), n, (uint32_t)L, min_pts, level.data(), child.data(), parent.data(), n_edges,
                                    &n_edges));
        for (uint64_t i = 0; i < n_edges; ++i) r.tree.push_back(TreeEdge{level[i], child[i], parent[i]});
        return r;
    }
    // {candidates pass 1, pairs within, tiles pass 1, candidates pass 2, tiles visited pass 2, tiles skipped pass 2, unions that
    // merged, stage-1 launches} of the last neighbor_counts / dbscan / neighbor_counts_levels / dbscan_levels (after a *_levels
    // call: pairs within = the top level's, unions = summed over the levels)
    std::vector<uint64_t> dbscan_stats() const { std::vector<uint64_t> v(8); check(mi_knn_dbscan_stats(h_, v.data())); return v; }
    // label every row by the nearest of C vectors (mi_knn_assign): for a live row what a table of the vectors answers to
    // knn(row, 1), id and distance bits; MI_KNN_NO_LABEL / +inf for a deleted row.  vectors: [C * dim]
    struct Assignment { std::vector<uint32_t> labels; std::vector<float> dist; };
    Assignment assign(const std::vector<float>& vectors, uint32_t C) const {
        uint64_t n = 0;
        check(mi_knn_size(h_, &n));
        Assignment r;
        r.labels.resize(n); r.dist.resize(n);
        check(mi_knn_assign(h_, vectors.data(), C, r.labels.data(), r.dist.data()));
        return r;
    }
    // {candidates, live rows labelled, stage-1 launches, tiles visited} of the last assign
    std::vector<uint64_t> assign_stats() const { std::vector<uint64_t> v(4); check(mi_knn_assign_stats(h_, v.data())); return v; }
    // up to m labels per row, only those within max_dist (mi_knn_assign_multi): labels / dist are [rows * m], a row's hits
    // nearest first, MI_KNN_NO_LABEL / +inf behind the last one and for a deleted row.  vectors: [C * dim]
    Assignment assign_multi(const std::vector<float>& vectors, uint32_t C, uint32_t m, float max_dist = INFINITY) const {
        uint64_t n = 0;
        check(mi_knn_size(h_, &n));
        Assignment r;
        r.labels.resize(n * m); r.dist.resize(n * m);
        check(mi_knn_assign_multi(h_, vectors.data(), C, m, max_dist, r.labels.data(), r.dist.data()));
        return r;
    }
    // {candidates, (row, label) hits written, stage-1 launches, tiles visited} of the last assign_multi
    std::vector<uint64_t> assign_multi_stats() const { std::vector<uint64_t> v(4); check(mi_knn_assign_multi_stats(h_, v.data())); return v; }
    // the k <= 16 nearest live rows for each of nq queries (mi_knn_search_many): idx / dist are [nq * k], per query what
    // knn(query, k) answers without the NaN distances, MI_KNN_NO_ID / +inf behind the last hit.  queries: [nq * dim]
    struct Neighbors { std::vector<uint64_t> idx; std::vector<float> dist; };
    Neighbors knn_many(const std::vector<float>& queries, uint32_t nq, uint32_t k) const {
        Neighbors r;
        r.idx.resize((size_t)nq * k); r.dist.resize((size_t)nq * k);
        check(mi_knn_search_many(h_, queries.data(), nq, k, r.idx.data(), r.dist.data()));
        return r;
    }
    // a slice of the kNN graph (mi_knn_neighbors): for the rows with ids first .. first + n - 1 the k <= 15 nearest OTHER
    // live rows, [n * k]; a deleted row gets MI_KNN_NO_ID / +inf
    Neighbors neighbors(uint32_t k, uint64_t first, uint64_t n) const {
        Neighbors r;
        r.idx.resize(n * k); r.dist.resize(n * k);
        check(mi_knn_neighbors(h_, first, n, k, r.idx.data(), r.dist.data()));
        return r;
    }
    // {candidates, (query, row) hits written, stage-1 launches, tiles visited} of the last knn_many / neighbors
    std::vector<uint64_t> search_many_stats() const { std::vector<uint64_t> v(4); check(mi_knn_search_many_stats(h_, v.data())); return v; }
    // spherical k-means (mi_knn_kmeans): centroids [C * dim] in = initial, out = final; labels / dist = assign(centroids)
    struct KMeans { Assignment assignment; uint32_t iters = 0; uint64_t changed = 0; double objective = 0.0; };
    KMeans kmeans(std::vector<float>& centroids, uint32_t C, uint32_t max_iters = 20) const {
        uint64_t n = 0;
        check(mi_knn_size(h_, &n));
        KMeans r;
        r.assignment.labels.resize(n); r.assignment.dist.resize(n);
        check(mi_knn_kmeans(h_, centroids.data(), C, max_iters, r.assignment.labels.data(), r.assignment.dist.data(), &r.iters,
                            &r.changed, &r.objective));
        return r;
    }
    // k-means++ seeding (mi_knn_kmeans_seed): C rows drawn in proportion to their cosine distance from the nearest row drawn
    // so far, among the live rows or the ids in `among`; centroids [C * dim] are what kmeans() takes as its start
    struct Seeds { std::vector<uint64_t> rows; std::vector<float> centroids; double potential = 0.0; };
    Seeds kmeans_seed(uint32_t C, uint64_t seed = 0, const std::vector<uint64_t>* among = nullptr) const {
        Seeds r;
        r.rows.resize(C); r.centroids.resize((size_t)C * dim_);
        static const uint64_t none = 0;   // an empty `among` is an empty set of candidates, not "every row"
        const uint64_t* ids = among ? (among->empty() ? &none : among->data()) : nullptr;
        check(mi_knn_kmeans_seed(h_, C, seed, ids, among ? among->size() : 0, r.rows.data(), r.centroids.data(), &r.potential));
        return r;
    }
    // {candidates, passes run, fallback picks, 0} of the last kmeans_seed
    std::vector<uint64_t> kmeans_seed_stats() const { std::vector<uint64_t> v(4); check(mi_knn_kmeans_seed_stats(h_, v.data())); return v; }
    // what every group looks like (mi_knn_summarize).  labels: one per local row (kmeans / assign labels, dbscan's dense labels,
    // anything; a value >= C belongs to nothing), nullptr: the table's group column.  centroids [C * dim] = the mean of x / |x|
    // over a group's members, bit-identical to kmeans' update; cover / odd = the ids of the member nearest to the centroid (the
    // group's exact medoid for unit vectors) and of the farthest, MI_KNN_NO_ID / +inf where there is none; spread = the measured
    // members' distances summed as integers of 2^-30; dist [rows] = a member's distance to its centroid with assign's bits;
    // totals = {members, live rows with a label >= C, unusable live rows with a label < C, non-empty groups}
    struct Summary {
        std::vector<float> centroids, cover_dist, odd_dist, dist;
        std::vector<uint64_t> count, cover, odd, measured, spread;
        uint64_t totals[4] = {0, 0, 0, 0};
        double mean_dist(uint32_t c) const { return measured[c] ? std::ldexp((double)spread[c] / (double)measured[c], -30) : NAN; }
    };
    Summary summarize(const std::vector<uint32_t>* labels, uint32_t C) const {
        uint64_t n = 0;
        check(mi_knn_size(h_, &n));
        if (labels && labels->size() != n) throw std::invalid_argument("summarize: one label per row");
        Summary r;
        r.centroids.resize((size_t)C * dim_); r.cover_dist.resize(C); r.odd_dist.resize(C); r.dist.resize(n + 1);   // (+ 1: never a null pointer)
        r.count.resize(C); r.cover.resize(C); r.odd.resize(C); r.measured.resize(C); r.spread.resize(C);
        check(mi_knn_summarize(h_, labels && n ? labels->data() : nullptr, C, r.centroids.data(), r.count.data(), r.cover.data(),
                               r.cover_dist.data(), r.odd.data(), r.odd_dist.data(), r.measured.data(), r.spread.data(), r.dist.data(),
                               r.totals));
        r.dist.resize(n);
        return r;
    }
    // {segments summed, workgroups of the distance pass, rows read by it, 0} of the last summarize
    std::vector<uint64_t> summarize_stats() const { std::vector<uint64_t> v(4); check(mi_knn_summarize_stats(h_, v.data())); return v; }
    // m pictures that span every group (mi_knn_representatives): farthest-first picks of every group at once.  labels / C as
    // summarize; start: nullptr = the member with the lowest id, else one member id per group (summarize's cover, say).
    // picks / gap [C * m] in pick order (MI_KNN_NO_ID / +inf behind n_picked[c]; gap = a pick's distance to the nearest
    // earlier one, non-increasing from pick 1 on); reach [C]; rep / rep_dist [rows] = the pick that stands for a row and the
    // distance to it; totals = {members, groups with a pick, picks, rounds that made a pick}
    struct Representatives {
        std::vector<uint64_t> picks;
        std::vector<float> gap, reach, rep_dist;
        std::vector<uint32_t> n_picked, rep;
        uint64_t totals[4] = {0, 0, 0, 0};
    };
    Representatives representatives(const std::vector<uint32_t>* labels, uint32_t C, uint32_t m = 9, float min_gap = -INFINITY,
                                    const std::vector<uint64_t>* start = nullptr) const {
        uint64_t n = 0;
        check(mi_knn_size(h_, &n));
        if (labels && labels->size() != n) throw std::invalid_argument("representatives: one label per row");
        if (start && start->size() != C) throw std::invalid_argument("representatives: one start id per group");
        Representatives r;
        r.picks.resize((size_t)C * m + 1); r.gap.resize((size_t)C * m + 1); r.reach.resize(C + 1); r.n_picked.resize(C + 1);   // (+ 1: never a null pointer)
        r.rep.resize(n + 1); r.rep_dist.resize(n + 1);
        check(mi_knn_representatives(h_, labels && n ? labels->data() : nullptr, C, m, min_gap, start ? start->data() : nullptr,
                                     r.picks.data(), r.gap.data(), r.n_picked.data(), r.reach.data(), r.rep.data(), r.rep_dist.data(),
                                     r.totals));
        r.picks.resize((size_t)C * m); r.gap.resize((size_t)C * m); r.reach.resize(C); r.n_picked.resize(C);
        r.rep.resize(n); r.rep_dist.resize(n);
        return r;
    }
    // {round launches, segments of the member walk, member rows read by the last round launched, 0} of the last representatives
    std::vector<uint64_t> representatives_stats() const { std::vector<uint64_t> v(4); check(mi_knn_representatives_stats(h_, v.data())); return v; }
    // the k best DISTINCT results (mi_knn_search_diverse): the first `pool` results of knn(query) walked in order, an entry
    // within cosine distance min_gap of an earlier kept one hidden behind it.  idx / dist / hidden [k] (padding MI_KNN_NO_ID /
    // +inf / 0 behind n_kept), rep [pool]: per pool rank its slot, MI_KNN_NO_LABEL when left over.  pool = 0: min(4096, max(4 k, 64))
    struct Diverse { std::vector<uint64_t> idx; std::vector<float> dist; std::vector<uint32_t> hidden, rep; uint32_t n_kept = 0; };
    Diverse knn_diverse(const std::vector<float>& query, uint32_t k, float min_gap, uint32_t pool = 0,
                        const std::vector<uint64_t>* among = nullptr) const {
        if (pool == 0) pool = std::min<uint32_t>(4096u, std::max<uint32_t>(4u * k, 64u));
        Diverse r;
        r.idx.resize(k); r.dist.resize(k); r.hidden.resize(k); r.rep.resize(pool);
        static const uint64_t none = 0;   // an empty `among` is an empty pool, not "the whole table"
        const uint64_t* ids = among ? (among->empty() ? &none : among->data()) : nullptr;
        check(mi_knn_search_diverse(h_, query.data(), k, pool, min_gap, ids, among ? among->size() : 0, r.idx.data(), r.dist.data(),
                                    r.hidden.data(), r.rep.data(), &r.n_kept));
        return r;
    }
    // {pool entries P, candidate pairs, conflicting pairs, pool entries hidden} of the last knn_diverse
    std::vector<uint64_t> knn_diverse_stats() const { std::vector<uint64_t> v(4); check(mi_knn_search_diverse_stats(h_, v.data())); return v; }
    // all-of / any-of / none-of terms in one exact pass (mi_knn_search_compound): terms [n_pos * dim]; mode MI_COMPOUND_ALL scores a
    // row by its largest distance to them, MI_COMPOUND_ANY by its smallest; without [n_neg * dim] + without_within [n_neg]: a row
    // within that cosine distance of a negative term is excluded.  idx / dist [k] by (score, id), padding MI_KNN_NO_ID / +inf;
    // term_dist [k * (n_pos + n_neg)] when asked for: the result rows' distance to every term, positives first
    struct Compound { std::vector<uint64_t> idx; std::vector<float> dist, term_dist; };
    Compound knn_compound(const std::vector<float>& terms, int mode, uint32_t k, const std::vector<float>& without = {},
                          const std::vector<float>& without_within = {}, const std::vector<uint64_t>* among = nullptr,
                          bool want_term_dist = false) const {
        const uint32_t n_pos = (uint32_t)(terms.size() / dim_), n_neg = (uint32_t)without_within.size();
        if (terms.size() != (size_t)n_pos * dim_ || without.size() != (size_t)n_neg * dim_) throw std::runtime_error("terms are not whole vectors");
        Compound r;
        r.idx.resize(k); r.dist.resize(k);
        if (want_term_dist) r.term_dist.resize((size_t)k * (n_pos + n_neg));
        static const uint64_t none = 0;   // an empty `among` is an empty set of candidates, not "every row"
        const uint64_t* ids = among ? (among->empty() ? &none : among->data()) : nullptr;
        check(mi_knn_search_compound(h_, terms.data(), n_pos, mode, n_neg ? without.data() : nullptr, n_neg ? without_within.data() : nullptr,
                                     n_neg, k, ids, among ? among->size() : 0, r.idx.data(), r.dist.data(),
                                     want_term_dist ? r.term_dist.data() : nullptr));
        return r;
    }
    // {rows or list entries scanned, rows excluded by a negative term, rows with a NaN score, results written} of the last knn_compound
    std::vector<uint64_t> knn_compound_stats() const { std::vector<uint64_t> v(4); check(mi_knn_search_compound_stats(h_, v.data())); return v; }
    // the k nearest rows after a cursor and within a distance (mi_knn_search_page).  Page 1: after = nullptr; page n + 1: the
    // previous Page (its next_dist / next_id go back exactly as they came).  max_dist: inclusive; among as for knn_compound
    Page knn_page(const std::vector<float>& reference, uint32_t k, const Page* after = nullptr, float max_dist = INFINITY,
                  const std::vector<uint64_t>* among = nullptr) const {
        Page r;
        r.idx.resize(k); r.dist.resize(k);
        static const uint64_t none = 0;   // an empty `among` is an empty set of candidates, not "every row"
        const uint64_t* ids = among ? (among->empty() ? &none : among->data()) : nullptr;
        const bool cur = after && after->has_next;
        check(mi_knn_search_page(h_, reference.data(), k, cur ? after->next_dist : 0.0f, cur ? after->next_id : MI_KNN_NO_ID, max_dist, ids,
                                 among ? among->size() : 0, r.idx.data(), r.dist.data(), r.counts));
        finish_page(r, k);
        return r;
    }
    // the group column (mi_knn_set_groups): groups[i] for row ids[i], or for the first groups.size() rows; not saved
    void set_groups(const std::vector<uint32_t>& groups, const std::vector<uint64_t>* ids = nullptr) {
        check(mi_knn_set_groups(h_, ids ? ids->data() : nullptr, groups.size(), groups.data()));
    }
    uint64_t n_groups() const { uint64_t info[2]; check(mi_knn_groups_info(h_, info)); return info[0]; }
    // of every group the row nearest to `reference` within max_dist, the k nearest of those (mi_knn_search_grouped)
    Grouped knn_grouped(const std::vector<float>& reference, uint32_t k, float max_dist = INFINITY,
                        const std::vector<uint64_t>* among = nullptr, bool facets = false) const {
        Grouped r;
        r.idx.resize(k); r.dist.resize(k); r.group.resize(k); r.members.resize(k);
        if (facets) r.facets.assign(n_groups(), 0);
        static const uint64_t none = 0;   // an empty `among` is an empty set of candidates, not "every row"
        const uint64_t* ids = among ? (among->empty() ? &none : among->data()) : nullptr;
        check(mi_knn_search_grouped(h_, reference.data(), k, max_dist, ids, among ? among->size() : 0, r.idx.data(), r.dist.data(),
                                    r.group.data(), r.members.data(), facets ? r.facets.data() : nullptr, r.facets.size(), r.totals));
        finish_grouped(r);
        return r;
    }
    // the attribute columns (mi_knn_set_attrs): 64 flags and one ordered value per row; nullptr keeps a column; not saved
    void set_attrs(const std::vector<uint64_t>& ids, const std::vector<uint64_t>* tags, const std::vector<int64_t>* stamps) {
        check(mi_knn_set_attrs(h_, ids.data(), ids.size(), tags ? tags->data() : nullptr, stamps ? stamps->data() : nullptr));
    }
    std::pair<std::vector<uint64_t>, std::vector<int64_t>> get_attrs(const std::vector<uint64_t>& ids) const {
        std::vector<uint64_t> tags(ids.size());
        std::vector<int64_t> stamps(ids.size());
        check(mi_knn_get_attrs(h_, ids.data(), ids.size(), tags.data(), stamps.data()));
        return {tags, stamps};
    }
    uint64_t count_where(const mi_knn_where& w) const { uint64_t n = 0; check(mi_knn_count_where(h_, &w, &n)); return n; }
    // the ids of the live rows the predicate keeps, ascending (mi_knn_rows_where)
    std::vector<uint64_t> rows_where(const mi_knn_where& w) const {
        uint64_t n = 0;
        check(mi_knn_rows_where(h_, &w, nullptr, 0, &n));
        std::vector<uint64_t> ids(n);
        check(mi_knn_rows_where(h_, &w, ids.data(), ids.size(), &n));
        ids.resize(std::min<uint64_t>(n, ids.size()));
        return ids;
    }
    // the k nearest among the rows the predicate keeps, evaluated on the device (mi_knn_search_where)
    WhereHits knn_where(const std::vector<float>& reference, uint32_t k, const mi_knn_where& w) const {
        WhereHits r;
        r.idx.resize(k); r.dist.resize(k);
        check(mi_knn_search_where(h_, reference.data(), 1, k, &w, r.idx.data(), r.dist.data(), &r.matched));
        finish_where(r);
        return r;
    }
    // the rows within max_dist in the order of their stamps, a page of k after the previous page (mi_knn_search_ordered).  w = nullptr:
    // every live row.  Page 1: after = nullptr; page n + 1: the page before
    OrderedPage knn_ordered(const std::vector<float>& reference, uint32_t k, float max_dist = INFINITY, bool descending = false,
                            const OrderedPage* after = nullptr, const mi_knn_where* w = nullptr) const {
        OrderedPage p;
        p.idx.resize(k); p.dist.resize(k); p.stamps.resize(k);
        const bool cur = after && after->has_next;
        check(mi_knn_search_ordered(h_, reference.data(), k, max_dist, w, ordered_flags(descending, after), cur ? after->next_stamp : 0,
              cur ? after->next_id : 0, p.idx.data(), p.dist.data(), p.stamps.data(), p.counts));
        finish_ordered(p, k);
        return p;
    }
    // the timeline facet (mi_knn_stamp_histogram): hist[b] = the rows within max_dist with exactly b of the ascending edges <= stamp
    std::vector<uint64_t> stamp_histogram(const std::vector<float>& reference, const std::vector<int64_t>& edges, float max_dist = INFINITY,
                                          const mi_knn_where* w = nullptr) const {
        std::vector<uint64_t> hist(edges.size() + 1);
        check(mi_knn_stamp_histogram(h_, reference.data(), max_dist, w, edges.data(), (uint32_t)edges.size(), hist.data()));
        return hist;
    }
    // "prefilter" = 2 (bytes) or 1 (bf16): the two-stage exact search, same results from a quarter / a half of the bytes
    void set_option(const std::string& key, int value) { check(mi_knn_set_option(h_, key.c_str(), value)); }
};

// pairs -> groups (mi_pairs_to_groups: connected components), ordered by their smallest id, ids ascending inside
inline std::vector<std::vector<uint64_t>> groups_from(const std::vector<uint64_t>& ids, const std::vector<uint64_t>& start) {
    std::vector<std::vector<uint64_t>> out;
    for (size_t g = 0; g + 1 < start.size(); ++g) out.emplace_back(ids.begin() + (ptrdiff_t)start[g], ids.begin() + (ptrdiff_t)start[g + 1]);
    return out;
}
inline std::vector<std::vector<uint64_t>> pairs_to_groups(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {
    if (a.size() != b.size()) throw std::runtime_error("pairs_to_groups: a and b differ in length");
    uint64_t n_ids = 0, n_groups = 0;
    check(mi_pairs_to_groups(a.data(), b.data(), a.size(), nullptr, 0, nullptr, 0, &n_ids, &n_groups));
    std::vector<uint64_t> ids(n_ids), start(n_groups + 1);
    check(mi_pairs_to_groups(a.data(), b.data(), a.size(), ids.data(), ids.size(), start.data(), start.size(), &n_ids, &n_groups));
    return groups_from(ids, start);
}

// the whole table `image` {id, image_path, embedding} (server/src/search.rs:13-18) and the four statements the
// server issues against it
class ImageIndex {
    mi_index* h_ = nullptr;
    static std::vector<const char*> ptrs(const std::vector<std::string>& v) {
        std::vector<const char*> p;
        for (const auto& s : v) p.push_back(s.c_str());
        return p;
    }

   public:
    explicit ImageIndex(uint32_t dim = 768, int device = 0, const std::string& media_dir = "") {
        check(mi_index_create(dim, device, media_dir.c_str(), &h_));
    }
    ImageIndex(const ImageIndex&) = delete;
    ~ImageIndex() { mi_index_free(h_); }
    mi_index* handle() const { return h_; }
    uint64_t size() const { uint64_t n = 0; check(mi_index_size(h_, &n)); return n; }
    // DELETE FROM image WHERE image_path IN $paths: returns the rows removed
    uint64_t remove(const std::vector<std::string>& paths) {
        const auto p = ptrs(paths);
        uint64_t n = 0;
        check(mi_index_remove(h_, p.data(), p.size(), &n));
        return n;
    }
    // SELECT image_path FROM image WHERE image_path IN $paths  (server/src/clip.rs:74-83)
    std::vector<bool> existing(const std::vector<std::string>& paths) const {
        std::vector<uint8_t> e(paths.size());
        const auto p = ptrs(paths);
        check(mi_index_existing(h_, p.data(), p.size(), e.data()));
        return std::vector<bool>(e.begin(), e.end());
    }
    // db.insert("image").content(rows)  (server/src/clip.rs:125-137): returns the id of the first row
    uint64_t insert(const std::vector<std::string>& paths, const std::vector<float>& embeddings) {
        uint64_t first = 0;
        const auto p = ptrs(paths);
        check(mi_index_insert(h_, p.data(), embeddings.data(), p.size(), &first));
        return first;
    }
    std::string path(uint64_t id, bool web = false) const {
        size_t need = 0;
        check(mi_index_path(h_, id, web ? 1 : 0, nullptr, 0, &need));
        std::string s(need - 1, '\0');  // `needed` counts the terminating NUL
        check(mi_index_path(h_, id, web ? 1 : 0, &s[0], need, &need));
        return s;
    }
    // web_search_text behind the text embedding (server/src/search.rs:43-110): refine with the referenced images'
    // stored embeddings, then `embedding <|k|> $reference`; (id, distance) ascending, missing results dropped
    std::vector<std::pair<uint64_t, float>> search(const std::vector<float>& text_embedding, const std::vector<std::string>& referenced_images,
                                                   uint32_t k = 1000) const {
        std::vector<uint64_t> idx(k);
        std::vector<float> dist(k);
        uint32_t n = 0;
        const auto p = ptrs(referenced_images);
        check(mi_index_search(h_, text_embedding.data(), p.data(), p.size(), k, idx.data(), dist.data(), &n));
        std::vector<std::pair<uint64_t, float>> out;
        for (uint32_t i = 0; i < n; ++i) out.emplace_back(idx[i], dist[i]);
        return out;
    }
    // search() with near-duplicates collapsed (mi_index_search_diverse): the k best distinct images as (id, distance,
    // look-alikes hidden behind it); folders as the client names them, none = everything; pool = 0: min(4096, max(4 k, 64))
    struct DiverseHit { uint64_t id; float dist; uint32_t hidden; };
    std::vector<DiverseHit> search_diverse(const std::vector<float>& text_embedding, const std::vector<std::string>& referenced_images,
                                           uint32_t k, float min_gap, uint32_t pool = 0,
                                           const std::vector<std::string>& folders = {}) const {
        if (pool == 0) pool = std::min<uint32_t>(4096u, std::max<uint32_t>(4u * k, 64u));
        std::vector<uint64_t> idx(k);
        std::vector<float> dist(k);
        std::vector<uint32_t> hidden(k);
        uint32_t n = 0;
        const auto p = ptrs(referenced_images);
        const auto f = ptrs(folders);
        check(mi_index_search_diverse(h_, text_embedding.data(), p.data(), p.size(), f.data(), f.size(), k, pool, min_gap, idx.data(),
                                      dist.data(), hidden.data(), &n));
        std::vector<DiverseHit> out;
        for (uint32_t i = 0; i < n; ++i) out.push_back(DiverseHit{idx[i], dist[i], hidden[i]});
        return out;
    }
    // and / or / not over embeddings (mi_index_search_compound): EmbeddingTable::knn_compound over the images under `folders`
    // (none = everything) as (id, score); removed paths never appear.  No refinement in here: refine a term first if wanted.
    // terms holds n_pos vectors, without one vector per entry of without_within
    std::vector<std::pair<uint64_t, float>> search_compound(const std::vector<float>& terms, uint32_t n_pos, int mode, uint32_t k,
                                                            const std::vector<float>& without = {}, const std::vector<float>& without_within = {},
                                                            const std::vector<std::string>& folders = {}, std::vector<float>* term_dist = nullptr) const {
        const uint32_t n_neg = (uint32_t)without_within.size();
        if (n_pos == 0 || terms.size() % n_pos != 0 || without.size() != (size_t)n_neg * (terms.size() / n_pos))
            throw std::runtime_error("terms are not whole vectors");
        std::vector<uint64_t> idx(k);
        std::vector<float> dist(k);
        if (term_dist) term_dist->assign((size_t)k * (n_pos + n_neg), 0.0f);
        uint32_t n = 0;
        const auto f = ptrs(folders);
        check(mi_index_search_compound(h_, terms.data(), n_pos, mode, n_neg ? without.data() : nullptr, n_neg ? without_within.data() : nullptr,
                                       n_neg, f.data(), f.size(), k, idx.data(), dist.data(), term_dist ? term_dist->data() : nullptr, &n));
        std::vector<std::pair<uint64_t, float>> out;
        for (uint32_t i = 0; i < n; ++i) out.emplace_back(idx[i], dist[i]);
        return out;
    }
    // one page of search() (mi_index_search_page): the refined query, the images under `folders` (none = everything), then the k
    // nearest after the cursor and within max_dist; removed paths never appear
    Page search_page(const std::vector<float>& text_embedding, const std::vector<std::string>& referenced_images, uint32_t k,
                     const Page* after = nullptr, float max_dist = INFINITY, const std::vector<std::string>& folders = {}) const {
        Page r;
        r.idx.resize(k); r.dist.resize(k);
        const auto p = ptrs(referenced_images);
        const auto f = ptrs(folders);
        const bool cur = after && after->has_next;
        uint32_t n = 0;
        check(mi_index_search_page(h_, text_embedding.data(), p.data(), p.size(), f.data(), f.size(), k, cur ? after->next_dist : 0.0f,
                                   cur ? after->next_id : MI_KNN_NO_ID, max_dist, r.idx.data(), r.dist.data(), &n, r.counts));
        finish_page(r, k);
        return r;
    }
    // the best picture of every directory (mi_index_search_grouped): search_page's query and folders, one hit per group
    Grouped search_grouped(const std::vector<float>& text_embedding, const std::vector<std::string>& referenced_images, uint32_t k,
                           float max_dist = INFINITY, const std::vector<std::string>& folders = {}, bool facets = false) const {
        Grouped r;
        r.idx.resize(k); r.dist.resize(k); r.group.resize(k); r.members.resize(k);
        uint32_t n_groups = 0, n = 0;
        check(mi_index_group_count(h_, &n_groups));
        if (facets) r.facets.assign(n_groups, 0);
        const auto p = ptrs(referenced_images);
        const auto f = ptrs(folders);
        check(mi_index_search_grouped(h_, text_embedding.data(), p.data(), p.size(), f.data(), f.size(), k, max_dist, r.idx.data(),
                                      r.dist.data(), r.group.data(), r.members.data(), &n, facets ? r.facets.data() : nullptr,
                                      r.facets.size(), r.totals));
        finish_grouped(r);
        return r;
    }
    // the group id of a directory as the client names it, "media/a/b" (mi_index_group_of): search_where's "in this folder"
    uint32_t group_of(const std::string& folder) const { uint32_t g = 0; check(mi_index_group_of(h_, folder.c_str(), &g)); return g; }
    // attributes by stored path (mi_index_set_attrs): every row of paths[i] takes tags[i] / stamps[i]; nullptr keeps a column
    void set_attrs(const std::vector<std::string>& paths, const std::vector<uint64_t>* tags, const std::vector<int64_t>* stamps) {
        const auto p = ptrs(paths);
        check(mi_index_set_attrs(h_, p.data(), p.size(), tags ? tags->data() : nullptr, stamps ? stamps->data() : nullptr));
    }
    // web_search_text among the images a predicate keeps (mi_index_search_where); w.group = group_of(folder) under
    // MI_KNN_WHERE_GROUP is "in this folder" without an id list
    WhereHits search_where(const std::vector<float>& text_embedding, const std::vector<std::string>& referenced_images, uint32_t k,
                           const mi_knn_where& w) const {
        WhereHits r;
        r.idx.resize(k); r.dist.resize(k);
        uint32_t n = 0;
        const auto p = ptrs(referenced_images);
        check(mi_index_search_where(h_, text_embedding.data(), p.data(), p.size(), k, &w, r.idx.data(), r.dist.data(), &n, &r.matched));
        finish_where(r);
        return r;
    }
    // web_search_text as a timeline (mi_index_search_ordered): the refined query, the images within max_dist newest first (or
    // oldest first), a page of k after the previous page; w as search_where takes it, nullptr = every image
    OrderedPage search_ordered(const std::vector<float>& text_embedding, const std::vector<std::string>& referenced_images, uint32_t k,
                               float max_dist = INFINITY, bool descending = true, const OrderedPage* after = nullptr,
                               const mi_knn_where* w = nullptr) const {
        OrderedPage r;
        r.idx.resize(k); r.dist.resize(k); r.stamps.resize(k);
        uint32_t n = 0;
        const auto p = ptrs(referenced_images);
        const bool cur = after && after->has_next;
        check(mi_index_search_ordered(h_, text_embedding.data(), p.data(), p.size(), k, max_dist, w, ordered_flags(descending, after),
                                      cur ? after->next_stamp : 0, cur ? after->next_id : 0, r.idx.data(), r.dist.data(), r.stamps.data(), &n,
                                      r.counts));
        finish_ordered(r, k);
        return r;
    }
    // the "matches per month" strip above it (mi_index_stamp_histogram)
    std::vector<uint64_t> timeline_histogram(const std::vector<float>& text_embedding, const std::vector<std::string>& referenced_images,
                                             const std::vector<int64_t>& edges, float max_dist = INFINITY, const mi_knn_where* w = nullptr) const {
        std::vector<uint64_t> hist(edges.size() + 1);
        const auto p = ptrs(referenced_images);
        check(mi_index_stamp_histogram(h_, text_embedding.data(), p.data(), p.size(), max_dist, w, edges.data(), (uint32_t)edges.size(),
                                       hist.data()));
        return hist;
    }
    // the directory behind a group id of search_grouped (mi_index_group_name)
    std::string group_name(uint32_t group, bool web = true) const {
        size_t need = 0;
        check(mi_index_group_name(h_, group, web ? 1 : 0, nullptr, 0, &need));
        std::string s(need, '\0');
        check(mi_index_group_name(h_, group, web ? 1 : 0, &s[0], need, nullptr));
        s.resize(need ? need - 1 : 0);
        return s;
    }
    // groups of near-duplicate images as paths (mi_index_duplicates), what a /duplicates handler returns; removed paths
    // never appear; first_new: only what the rows from that id on duplicate
    std::vector<std::vector<std::string>> duplicates(float max_dist, uint64_t first_new = 0, bool web = false,
                                                      uint64_t max_pairs = 1ull << 20) const {
        uint64_t n_ids = 0, n_groups = 0;
        check(mi_index_duplicates(h_, max_dist, first_new, max_pairs, nullptr, 0, nullptr, 0, &n_ids, &n_groups));
        std::vector<uint64_t> ids(n_ids), start(n_groups + 1);
        check(mi_index_duplicates(h_, max_dist, first_new, max_pairs, ids.data(), ids.size(), start.data(), start.size(), &n_ids, &n_groups));
        std::vector<std::vector<std::string>> out;
        for (const auto& g : groups_from(ids, start)) {
            out.emplace_back();
            for (uint64_t id : g) out.back().push_back(path(id, web));
        }
        return out;
    }
    // bursts (mi_index_bursts): duplicates' groups over the pairs that look alike and were taken within `window` of each other
    std::vector<std::vector<std::string>> bursts(float max_dist, uint64_t window, bool web = false, uint64_t max_pairs = 1ull << 20) const {
        uint64_t n_ids = 0, n_groups = 0;
        check(mi_index_bursts(h_, max_dist, window, 0, max_pairs, nullptr, 0, nullptr, 0, &n_ids, &n_groups));
        std::vector<uint64_t> ids(n_ids), start(n_groups + 1);
        check(mi_index_bursts(h_, max_dist, window, 0, max_pairs, ids.data(), ids.size(), start.data(), start.size(), &n_ids, &n_groups));
        std::vector<std::vector<std::string>> out;
        for (const auto& g : groups_from(ids, start)) {
            out.emplace_back();
            for (uint64_t id : g) out.back().push_back(path(id, web));
        }
        return out;
    }
    // "skip what I already have" (mi_index_matches): (path here, path in `other`, distance) of every pair of images within
    // max_dist, ordered by this index's row, then the other's; removed paths never appear
    struct Match { std::string mine, theirs; float dist; };
    std::vector<Match> matches(const ImageIndex& other, float max_dist, bool web = false, uint64_t max_pairs = 1ull << 20) const {
        std::vector<uint64_t> a(max_pairs), b(max_pairs);
        std::vector<float> d(max_pairs);
        uint64_t n = 0;
        check(mi_index_matches(h_, other.h_, max_dist, a.data(), b.data(), d.data(), max_pairs, &n));
        std::vector<Match> out;
        for (uint64_t i = 0; i < n; ++i) out.push_back(Match{path(a[i], web), other.path(b[i], web), d[i]});
        return out;
    }
    // the themes that are really there as lists of paths (mi_index_themes), what a /themes handler returns: the largest
    // cluster first, equal sizes by their first row; removed paths never appear.  *n_noise (may be null): the live rows in no theme
    std::vector<std::vector<std::string>> themes(float max_dist, uint32_t min_pts = 5, bool web = false, uint64_t* n_noise = nullptr) const {
        uint64_t n_ids = 0, n_groups = 0, noise = 0;
        std::vector<uint64_t> ids(size() + 1), start(size() + 1);   // every row in a theme of its own still fits: one call, not two
        check(mi_index_themes(h_, max_dist, min_pts, ids.data(), ids.size(), start.data(), start.size(), &n_ids, &n_groups, &noise));
        ids.resize(n_ids); start.resize(n_groups + 1);
        if (n_noise) *n_noise = noise;
        auto groups = groups_from(ids, start);
        std::stable_sort(groups.begin(), groups.end(), [](const auto& x, const auto& y) { return x.size() > y.size(); });
        std::vector<std::vector<std::string>> out;
        for (const auto& g : groups) {
            out.emplace_back();
            for (uint64_t id : g) out.back().push_back(path(id, web));
        }
        return out;
    }
    // events (mi_index_events): themes() with the neighbourhood "within max_dist and within `window` in time"; same output shape
    std::vector<std::vector<std::string>> events(float max_dist, uint64_t window, uint32_t min_pts = 5, bool web = false,
                                                 uint64_t* n_noise = nullptr) const {
        uint64_t n_ids = 0, n_groups = 0, noise = 0;
        std::vector<uint64_t> ids(size() + 1), start(size() + 1);
        check(mi_index_events(h_, max_dist, window, min_pts, ids.data(), ids.size(), start.data(), start.size(), &n_ids, &n_groups, &noise));
        ids.resize(n_ids); start.resize(n_groups + 1);
        if (n_noise) *n_noise = noise;
        auto groups = groups_from(ids, start);
        std::stable_sort(groups.begin(), groups.end(), [](const auto& x, const auto& y) { return x.size() > y.size(); });
        std::vector<std::vector<std::string>> out;
        for (const auto& g : groups) {
            out.emplace_back();
            for (uint64_t id : g) out.back().push_back(path(id, web));
        }
        return out;
    }
    // the folders at a glance (mi_index_folder_overview): per directory that holds an image its name, how many images, the
    // cover (the image nearest to the folder's centroid: its medoid) and the odd one out (the farthest; empty when no distance
    // is a number) as paths with their distances, and the mean distance; the largest folder first
    struct FolderOverview { std::string folder, cover, odd_one_out; uint64_t images = 0; float cover_dist = INFINITY, odd_dist = INFINITY; double mean_dist = NAN; };
    std::vector<FolderOverview> folder_overview(bool web = false) const {
        uint32_t C = 0;
        check(mi_index_group_count(h_, &C));
        std::vector<uint64_t> count(C + 1), cover(C + 1), odd(C + 1), measured(C + 1), spread(C + 1);
        std::vector<float> cover_dist(C + 1), odd_dist(C + 1);
        uint32_t n = 0;
        check(mi_index_folder_overview(h_, C, count.data(), cover.data(), cover_dist.data(), odd.data(), odd_dist.data(), measured.data(),
                                       spread.data(), &n));
        std::vector<uint32_t> order;
        for (uint32_t g = 0; g < std::min(C, n); ++g) if (count[g]) order.push_back(g);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return count[x] > count[y]; });
        std::vector<FolderOverview> out;
        for (uint32_t g : order) {
            FolderOverview o;
            o.folder = group_name(g, web);
            o.images = count[g];
            o.cover = path(cover[g], web);
            o.cover_dist = cover_dist[g];
            if (odd[g] != MI_KNN_NO_ID) o.odd_one_out = path(odd[g], web);
            o.odd_dist = odd_dist[g];
            if (measured[g]) o.mean_dist = std::ldexp((double)spread[g] / (double)measured[g], -30);
            out.push_back(o);
        }
        return out;
    }
    void save(const std::string& dir) const { check(mi_index_save(h_, dir.c_str())); }
    void load(const std::string& dir) { check(mi_index_load(h_, dir.c_str())); }
};

// the table row-sharded over several GPUs of ONE process: same results as one EmbeddingTable
class ShardedTable {
    mi_knn_sharded* h_ = nullptr;
    uint32_t dim_;

   public:
    ShardedTable(uint32_t dim, const std::vector<int>& devices, uint32_t block_rows = 0) : dim_(dim) {
        check(mi_knn_sharded_create(dim, devices.data(), (int)devices.size(), block_rows, &h_));
    }
    ShardedTable(const ShardedTable&) = delete;
    ~ShardedTable() { mi_knn_sharded_free(h_); }
    uint64_t insert(const std::vector<float>& rows) {
        uint64_t first = 0;
        check(mi_knn_sharded_append(h_, rows.data(), rows.size() / dim_, &first));
        return first;
    }
    uint64_t size() const { uint64_t n = 0; check(mi_knn_sharded_info(h_, &n, nullptr, nullptr, nullptr)); return n; }
    // DELETE FROM image WHERE id IN $ids on global ids
    uint64_t remove_ids(const std::vector<uint64_t>& ids) { uint64_t n = 0; check(mi_knn_sharded_delete(h_, ids.data(), ids.size(), &n)); return n; }
    std::vector<uint64_t> deleted() const {
        uint64_t n = 0;
        check(mi_knn_sharded_deleted(h_, nullptr, 0, &n));
        std::vector<uint64_t> v(n);
        if (n) check(mi_knn_sharded_deleted(h_, v.data(), n, &n));
        return v;
    }
    void set_option(const std::string& key, int value) { check(mi_knn_sharded_set_option(h_, key.c_str(), value)); }
    // {searches, ncclAllGather calls, transport copies, device merges} issued so far
    std::vector<uint64_t> stats() const { std::vector<uint64_t> v(4); check(mi_knn_sharded_stats(h_, v.data())); return v; }
    // EmbeddingTable::near_pairs over all shards (mi_knn_sharded_near_pairs): the one table's ids and distance bits, pairs that
    // cross shards included; first_new: only pairs whose larger id is >= first_new
    EmbeddingTable::NearPairs near_pairs(float max_dist, uint64_t first_new = 0, uint64_t cap = 1ull << 20) const {
        EmbeddingTable::NearPairs r;
        r.a.resize(cap); r.b.resize(cap); r.dist.resize(cap);
        uint64_t n = 0;
        check(mi_knn_sharded_near_pairs(h_, max_dist, first_new, r.a.data(), r.b.data(), r.dist.data(), cap, &n));
        r.a.resize(n); r.b.resize(n); r.dist.resize(n);
        return r;
    }
    // {candidate pairs, pairs accepted, stage-1 launches, tiles} of the last near_pairs, summed over shards and shard pairs
    std::vector<uint64_t> near_pairs_stats() const { std::vector<uint64_t> v(4); check(mi_knn_sharded_near_pairs_stats(h_, v.data())); return v; }
    // EmbeddingTable::neighbor_counts over all shards (mi_knn_sharded_density): by global row id, pairs that cross shards counted
    std::vector<uint32_t> neighbor_counts(float max_dist) const {
        std::vector<uint32_t> counts(size() + 1);   // (+ 1: never a null pointer)
        check(mi_knn_sharded_density(h_, max_dist, counts.data()));
        counts.pop_back();
        return counts;
    }
    // EmbeddingTable::dbscan over all shards (mi_knn_sharded_dbscan): arrays by global row id, bit for bit what one table
    // holding the same rows returns
    EmbeddingTable::Dbscan dbscan(float max_dist, uint32_t min_pts = 5) const {
        EmbeddingTable::Dbscan r;
        const uint64_t n = size();
        r.cluster.resize(n + 1); r.via.resize(n + 1); r.via_dist.resize(n + 1); r.counts.resize(n + 1);
        check(mi_knn_sharded_dbscan(h_, max_dist, min_pts, r.cluster.data(), r.via.data(), r.via_dist.data(), r.counts.data(), r.summary));
        EmbeddingTable::dbscan_trim_and_label(r, n);
        return r;
    }
    // mi_knn_dbscan_stats' eight fields of the last neighbor_counts / dbscan, summed over shards and shard pairs
    std::vector<uint64_t> dbscan_stats() const { std::vector<uint64_t> v(8); check(mi_knn_sharded_dbscan_stats(h_, v.data())); return v; }
    // EmbeddingTable::kmeans over all shards (mi_knn_sharded_kmeans): labels / dist by global row id; bit for bit what one
    // table holding the same rows returns with its option "kmeans_fixed_sum" = 1
    EmbeddingTable::KMeans kmeans(std::vector<float>& centroids, uint32_t C, uint32_t max_iters = 20) const {
        const uint64_t n = size();
        EmbeddingTable::KMeans r;
        r.assignment.labels.resize(n); r.assignment.dist.resize(n);
        check(mi_knn_sharded_kmeans(h_, centroids.data(), C, max_iters, r.assignment.labels.data(), r.assignment.dist.data(), &r.iters,
                                    &r.changed, &r.objective));
        return r;
    }
    // {updates run, bytes copied between shards, segments summed in the last update, merge launches} of the last kmeans
    std::vector<uint64_t> kmeans_stats() const { std::vector<uint64_t> v(4); check(mi_knn_sharded_kmeans_stats(h_, v.data())); return v; }
    // EmbeddingTable::kmeans_seed over all shards (mi_knn_sharded_kmeans_seed): rows are global ids; bit for bit what one table
    // holding the same rows returns.  centroids [C * dim] are what kmeans() takes as its start
    EmbeddingTable::Seeds kmeans_seed(uint32_t C, uint64_t seed = 0, const std::vector<uint64_t>* among = nullptr) const {
        EmbeddingTable::Seeds r;
        r.rows.resize(C); r.centroids.resize((size_t)C * dim_);
        static const uint64_t none = 0;   // an empty `among` is an empty set of candidates, not "every row"
        const uint64_t* ids = among ? (among->empty() ? &none : among->data()) : nullptr;
        check(mi_knn_sharded_kmeans_seed(h_, C, seed, ids, among ? among->size() : 0, r.rows.data(), r.centroids.data(), &r.potential));
        return r;
    }
    // {candidates, passes run, fallback picks, bytes copied between shards} of the last kmeans_seed
    std::vector<uint64_t> kmeans_seed_stats() const { std::vector<uint64_t> v(4); check(mi_knn_sharded_kmeans_seed_stats(h_, v.data())); return v; }
    // EmbeddingTable::summarize over all shards (mi_knn_sharded_summarize): labels / dist by global row id, cover / odd global
    // ids (a tie goes to the lowest global id); bit for bit what one table holding the same rows returns with its option
    // "kmeans_fixed_sum" = 1.  labels == nullptr: every shard's part of the group column
    EmbeddingTable::Summary summarize(const std::vector<uint32_t>* labels, uint32_t C) const {
        const uint64_t n = size();
        if (labels && labels->size() != n) throw std::invalid_argument("summarize: one label per row");
        EmbeddingTable::Summary r;
        r.centroids.resize((size_t)C * dim_); r.cover_dist.resize(C); r.odd_dist.resize(C); r.dist.resize(n + 1);   // (+ 1: never a null pointer)
        r.count.resize(C); r.cover.resize(C); r.odd.resize(C); r.measured.resize(C); r.spread.resize(C);
        check(mi_knn_sharded_summarize(h_, labels && n ? labels->data() : nullptr, C, r.centroids.data(), r.count.data(), r.cover.data(),
                                       r.cover_dist.data(), r.odd.data(), r.odd_dist.data(), r.measured.data(), r.spread.data(),
                                       r.dist.data(), r.totals));
        r.dist.resize(n);
        return r;
    }
    // {segments summed, bytes copied between shards, merge launches, members} of the last summarize
    std::vector<uint64_t> summarize_stats() const { std::vector<uint64_t> v(4); check(mi_knn_sharded_summarize_stats(h_, v.data())); return v; }
    // EmbeddingTable::assign_multi over all shards (mi_knn_sharded_assign_multi): labels / dist [rows * m] by global row id
    std::pair<std::vector<uint32_t>, std::vector<float>> assign_multi(const std::vector<float>& vectors, uint32_t C, uint32_t m,
                                                                      float max_dist = INFINITY) const {
        const uint64_t n = size();
        std::vector<uint32_t> labels(n * m);
        std::vector<float> dist(n * m);
        check(mi_knn_sharded_assign_multi(h_, vectors.data(), C, m, max_dist, labels.data(), dist.data()));
        return {std::move(labels), std::move(dist)};
    }
    // EmbeddingTable::knn_many over all shards (mi_knn_sharded_search_many): idx / dist [nq * k], global ids
    std::pair<std::vector<uint64_t>, std::vector<float>> knn_many(const std::vector<float>& queries, uint32_t nq, uint32_t k) const {
        std::vector<uint64_t> idx((size_t)nq * k);
        std::vector<float> dist((size_t)nq * k);
        check(mi_knn_sharded_search_many(h_, queries.data(), nq, k, idx.data(), dist.data()));
        return {std::move(idx), std::move(dist)};
    }
    void set_groups(const std::vector<uint32_t>& groups, const std::vector<uint64_t>* ids = nullptr) {
        check(mi_knn_sharded_set_groups(h_, ids ? ids->data() : nullptr, groups.size(), groups.data()));
    }
    uint64_t n_groups() const { uint64_t info[2]; check(mi_knn_sharded_groups_info(h_, info)); return info[0]; }
    // EmbeddingTable::knn_grouped over all shards (mi_knn_sharded_search_grouped): global ids, a group counted once
    Grouped knn_grouped(const std::vector<float>& reference, uint32_t k, float max_dist = INFINITY,
                        const std::vector<uint64_t>* among = nullptr, bool facets = false) const {
        Grouped r;
        r.idx.resize(k); r.dist.resize(k); r.group.resize(k); r.members.resize(k);
        if (facets) r.facets.assign(n_groups(), 0);
        static const uint64_t none = 0;
        const uint64_t* ids = among ? (among->empty() ? &none : among->data()) : nullptr;
        check(mi_knn_sharded_search_grouped(h_, reference.data(), k, max_dist, ids, among ? among->size() : 0, r.idx.data(), r.dist.data(),
                                            r.group.data(), r.members.data(), facets ? r.facets.data() : nullptr, r.facets.size(), r.totals));
        finish_grouped(r);
        return r;
    }
    // the attribute columns and predicates on global ids (mi_knn_sharded_set_attrs and its kin)
    void set_attrs(const std::vector<uint64_t>& ids, const std::vector<uint64_t>* tags, const std::vector<int64_t>* stamps) {
        check(mi_knn_sharded_set_attrs(h_, ids.data(), ids.size(), tags ? tags->data() : nullptr, stamps ? stamps->data() : nullptr));
    }
    std::pair<std::vector<uint64_t>, std::vector<int64_t>> get_attrs(const std::vector<uint64_t>& ids) const {
        std::vector<uint64_t> tags(ids.size());
        std::vector<int64_t> stamps(ids.size());
        check(mi_knn_sharded_get_attrs(h_, ids.data(), ids.size(), tags.data(), stamps.data()));
        return {tags, stamps};
    }
    uint64_t count_where(const mi_knn_where& w) const { uint64_t n = 0; check(mi_knn_sharded_count_where(h_, &w, &n)); return n; }
    WhereHits knn_where(const std::vector<float>& reference, uint32_t k, const mi_knn_where& w) const {
        WhereHits r;
        r.idx.resize(k); r.dist.resize(k);
        check(mi_knn_sharded_search_where(h_, reference.data(), 1, k, &w, r.idx.data(), r.dist.data(), &r.matched));
        finish_where(r);
        return r;
    }
    // the rows within max_dist in the order of their stamps, a page of k after the previous page (EmbeddingTable::knn_ordered over all shards: mi_knn_sharded_search_ordered).  w = nullptr:
    // every live row.  Page 1: after = nullptr; page n + 1: the page before
    OrderedPage knn_ordered(const std::vector<float>& reference, uint32_t k, float max_dist = INFINITY, bool descending = false,
                            const OrderedPage* after = nullptr, const mi_knn_where* w = nullptr) const {
        OrderedPage p;
        p.idx.resize(k); p.dist.resize(k); p.stamps.resize(k);
        const bool cur = after && after->has_next;
        check(mi_knn_sharded_search_ordered(h_, reference.data(), k, max_dist, w, ordered_flags(descending, after), cur ? after->next_stamp : 0,
              cur ? after->next_id : 0, p.idx.data(), p.dist.data(), p.stamps.data(), p.counts));
        finish_ordered(p, k);
        return p;
    }
    // the timeline facet (mi_knn_sharded_stamp_histogram): hist[b] = the rows within max_dist with exactly b of the ascending edges <= stamp
    std::vector<uint64_t> stamp_histogram(const std::vector<float>& reference, const std::vector<int64_t>& edges, float max_dist = INFINITY,
                                          const mi_knn_where* w = nullptr) const {
        std::vector<uint64_t> hist(edges.size() + 1);
        check(mi_knn_sharded_stamp_histogram(h_, reference.data(), max_dist, w, edges.data(), (uint32_t)edges.size(), hist.data()));
        return hist;
    }
    // EmbeddingTable::knn_page over all shards (mi_knn_sharded_search_page): global ids, summed counts
    Page knn_page(const std::vector<float>& reference, uint32_t k, const Page* after = nullptr, float max_dist = INFINITY,
                  const std::vector<uint64_t>* among = nullptr) const {
        Page r;
        r.idx.resize(k); r.dist.resize(k);
        static const uint64_t none = 0;
        const uint64_t* ids = among ? (among->empty() ? &none : among->data()) : nullptr;
        const bool cur = after && after->has_next;
        check(mi_knn_sharded_search_page(h_, reference.data(), k, cur ? after->next_dist : 0.0f, cur ? after->next_id : MI_KNN_NO_ID, max_dist,
                                         ids, among ? among->size() : 0, r.idx.data(), r.dist.data(), r.counts));
        finish_page(r, k);
        return r;
    }
    std::pair<std::vector<uint64_t>, std::vector<float>> knn(const std::vector<float>& reference, uint32_t k = 1000) const {
        std::vector<uint64_t> idx(k);
        std::vector<float> dist(k);
        check(mi_knn_sharded_search(h_, reference.data(), 1, k, idx.data(), dist.data()));
        return {idx, dist};
    }
    // the same search without the wait: idx / dist (caller-owned, k entries each) are filled when sync() returns
    void knn_async(const float* reference, uint32_t k, uint64_t* idx, float* dist) { check(mi_knn_sharded_search_async(h_, reference, 1, k, idx, dist)); }
    void sync() { check(mi_knn_sharded_sync(h_)); }
    // rows that are already in device memory on `src_device` (a replica's embeddings): routed to their shards device to device
    uint64_t insert_device(const float* d_rows, uint64_t n, int src_device, void* stream = nullptr) {
        uint64_t first = 0;
        check(mi_knn_sharded_append_device(h_, d_rows, n, src_device, stream, &first));
        return first;
    }
    // every row of `src` into this EMPTY table (another shard count / device set / block size), device to device
    void rebalance_from(ShardedTable& src) { check(mi_knn_sharded_rebalance(h_, src.h_)); }
    void save(const std::string& prefix) const { check(mi_knn_sharded_save(h_, prefix.c_str())); }
    void load(const std::string& prefix) { check(mi_knn_sharded_load(h_, prefix.c_str())); }
    mi_knn_sharded* handle() const { return h_; }
};

// the body of the scan loop and the query on HIP streams (BASELINE config 4)
class Pipeline {
    mi_pipeline* h_ = nullptr;

   public:
    Pipeline(clip_vit_large_patch14::Model& model, EmbeddingTable& table) { check(mi_pipeline_create(model.handle(), table.handle(), &h_)); }
    // ONE process over several GPUs: models[s] is the tower replica on the device of shard s
    Pipeline(const std::vector<clip_vit_large_patch14::Model*>& models, ShardedTable& table) {
        std::vector<mi_clip*> hs;
        for (auto* m : models) hs.push_back(m->handle());
        check(mi_pipeline_create_sharded(hs.data(), (int)hs.size(), table.handle(), &h_));
    }
    Pipeline(const Pipeline&) = delete;
    ~Pipeline() { mi_pipeline_free(h_); }
    // [n,3,H,W] f32 (pinned memory from mi_host_alloc makes the upload asynchronous): returns the id of the first new row
    uint64_t ingest(const float* nchw, size_t n) {
        uint64_t first = 0;
        check(mi_pipeline_ingest(h_, nchw, n, &first));
        return first;
    }
    // results land in idx / dist when sync() (or drain) returns
    void query(const float* q, uint32_t k, uint64_t* idx, float* dist) { check(mi_pipeline_query(h_, q, k, idx, dist)); }
    void sync() { check(mi_pipeline_sync(h_)); }
    // deliver finished queries until at most `leave_pending` remain (the ingest stream is not waited for)
    void drain(uint32_t leave_pending = 0) { check(mi_pipeline_drain(h_, leave_pending)); }
};


}  // namespace image_search
