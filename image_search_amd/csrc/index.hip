// index.hip — table `image` {id, image_path, embedding} (server/src/search.rs:13-18) behind the C ABI: one embedding
// shard (mi_knn) plus the image_path column, so that the statements the reference server issues need no host-language
// glue above the library:
//   SELECT image_path FROM image WHERE image_path IN $paths            server/src/clip.rs:74-83     mi_index_existing
//   db.insert("image").content(rows)                                   server/src/clip.rs:125-137   mi_index_insert
//   SELECT id, image_path, embedding FROM image WHERE image_path IN $p server/src/search.rs:43-58   mi_index_rows_of
//   refine + SELECT id, image_path, knn() ... <|K|> $reference         server/src/search.rs:20-110  mi_index_search
//   ... AND string::starts_with(image_path, $folder) (a pre-filter)                                 mi_index_search_within
//   DELETE FROM image WHERE image_path IN $paths                                                    mi_index_remove
// Row id = insertion ordinal; like the reference's table there is no uniqueness constraint on image_path (the scan
// loop filters first), a path may own several rows and lookups return all of them in id order.
// Persistence: `<dir>/embedding.miknn` (mi_knn_save) and `<dir>/image_path.bin`, each written to a temporary name,
// fsync'ed and renamed; the path file goes last and carries the row count, so a crash between the two leaves the OLD
// path file beside a NEWER embedding file — load then keeps the rows both files agree on (the reference's database
// commits per chunk; here a crash costs at most the chunks since the last save).
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "grouped_host.h"
#include "handles.h"
#include "ordered_host.h"
#include "representatives_host.h"
#include "summary_host.h"
#include "where_host.h"

using namespace mi;

struct mi_index {
    mi_knn* table = nullptr;
    uint32_t dim = 0;
    std::string media_dir;  // the server's media directory: "media/..." in requests maps onto it (search.rs:35-40)
    std::vector<std::string> paths;                            // row id -> image_path
    std::unordered_map<std::string, std::vector<uint64_t>> rows_of;  // image_path -> row ids, ascending (live rows only)
    std::set<std::string> live;                                // the keys of rows_of, ordered: a folder is one range of it
    std::vector<uint8_t> removed;                              // row id -> deleted by mi_index_remove (the table's tombstones)
    // mi_index_search_grouped: directory <-> group id, row id -> group id, and what the table's column holds of it: the first
    // groups_uploaded rows, as long as the table's groups_epoch is the one our last upload left (anybody else's
    // mi_knn_set_groups moves it on, and the next grouped search uploads everything again)
    GroupDict dirs;
    std::vector<uint32_t> row_dir;
    uint64_t groups_uploaded = 0, groups_epoch = 0;
    std::mutex mu;
};

namespace {

void add_path(mi_index* ix, const std::string& p, bool removed = false) {
    if (!removed) {
        ix->rows_of[p].push_back(ix->paths.size());
        ix->live.insert(p);
    }
    ix->paths.push_back(p);
    ix->removed.push_back(removed ? 1 : 0);
    ix->row_dir.push_back(ix->dirs.of_path(p));
}

uint64_t table_groups_epoch(mi_knn* t) {
    std::lock_guard<std::mutex> l(t->mu);
    return t->groups_epoch;
}

// the table's group column holds every row's directory id; ix->mu held
void sync_groups(mi_index* ix) {
    if (ix->dirs.names.size() > MI_KNN_GROUPS_MAX) fail(MI_ERR_UNSUPPORTED, "%zu directories: a table holds at most 2^24 groups", ix->dirs.names.size());
    if (table_groups_epoch(ix->table) != ix->groups_epoch) ix->groups_uploaded = 0;   // somebody else wrote the column (or nobody has)
    const uint64_t rows = ix->row_dir.size();
    if (ix->groups_uploaded == rows && (rows || ix->groups_epoch)) return;
    if (rows > ix->groups_uploaded) {
        std::vector<uint64_t> ids((size_t)(rows - ix->groups_uploaded));
        for (size_t i = 0; i < ids.size(); ++i) ids[i] = ix->groups_uploaded + i;
        call_ok(mi_knn_set_groups(ix->table, ids.data(), ids.size(), ix->row_dir.data() + ix->groups_uploaded));
    }
    ix->groups_uploaded = rows;
    ix->groups_epoch = table_groups_epoch(ix->table);
}

// "media/x.jpg" as the client names it -> the path the row was stored under (search.rs:35-40: only such names are looked up)
bool to_disk(const mi_index* ix, const char* web, std::string* out) {
    if (std::strncmp(web, "media/", 6) != 0) return false;
    *out = ix->media_dir + (web + 6);
    return true;
}

// the query of web_search_text: the text vector, refined with the marked images found in the table (search.rs:35-67)
std::vector<float> refined_query(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref) {
    std::vector<uint64_t> marked;
    {
        std::lock_guard<std::mutex> l(ix->mu);
        for (size_t i = 0; i < n_ref; ++i) {
            std::string disk;
            if (!referenced_images[i] || !to_disk(ix, referenced_images[i], &disk)) continue;  // search.rs:35-40
            auto it = ix->rows_of.find(disk);
            if (it != ix->rows_of.end()) marked.insert(marked.end(), it->second.begin(), it->second.end());
        }
    }
    std::sort(marked.begin(), marked.end());
    marked.erase(std::unique(marked.begin(), marked.end()), marked.end());
    std::vector<float> query(text_embedding, text_embedding + ix->dim);
    if (!marked.empty()) {  // search.rs:59-67
        std::vector<float> sel(marked.size() * ix->dim);
        std::vector<const float*> ptr(marked.size());
        for (size_t i = 0; i < marked.size(); ++i) {
            call_ok(mi_knn_get_rows(ix->table, marked[i], 1, &sel[i * ix->dim]));
            ptr[i] = &sel[i * ix->dim];
        }
        call_ok(mi_refine(text_embedding, ptr.data(), ptr.size(), ix->dim, query.data()));
    }
    return query;
}

// results in front of the MI_KNN_NO_ID padding
uint32_t hits(const uint64_t* idx, uint32_t k) {
    uint32_t n = 0;
    while (n < k && idx[n] != MI_KNN_NO_ID) ++n;
    return n;
}

// the ids of the live rows under `folders` (client names, whole path components): each folder is one range of the ordered
// live paths, found by lower_bound
std::vector<uint64_t> folder_rows(mi_index* ix, const char* const* folders, size_t n_folders) {
    std::vector<uint64_t> ids;
    std::lock_guard<std::mutex> l(ix->mu);
    for (size_t i = 0; i < n_folders; ++i) {
        if (!folders[i]) fail(MI_ERR_INVALID, "folder %zu is null", i);
        std::string prefix;
        if (!to_disk(ix, folders[i], &prefix)) continue;  // not under "media/": matches nothing
        // "media/" is the media directory itself; any deeper folder matches whole components: "<dir>/"
        if (prefix.size() > ix->media_dir.size() && prefix.back() != '/') prefix += '/';
        for (auto it = ix->live.lower_bound(prefix); it != ix->live.end() && it->compare(0, prefix.size(), prefix) == 0; ++it) {
            const std::vector<uint64_t>& r = ix->rows_of.at(*it);
            ids.insert(ids.end(), r.begin(), r.end());
        }
    }
    return ids;
}

void write_all(int fd, const void* p, size_t n, const char* what) {
    const char* c = static_cast<const char*>(p);
    while (n) {
        const ssize_t w = ::write(fd, c, n);
        if (w <= 0) fail(MI_ERR_IO, "write to %s failed (disk full?)", what);
        c += w; n -= (size_t)w;
    }
}

}  // namespace

extern "C" {

int mi_index_create(uint32_t dim, int device, const char* media_dir, mi_index** out) {
    mi_index* ix = nullptr;
    const int rc = guarded([&] {
        if (!out) fail(MI_ERR_INVALID, "out is null");
        *out = nullptr;
        ix = new mi_index();
        ix->dim = dim;
        ix->media_dir = media_dir ? media_dir : "";
        call_ok(mi_knn_create(dim, device, &ix->table));
        *out = ix;
    });
    if (rc != MI_OK && ix) { delete ix; }
    return rc;
}

void mi_index_free(mi_index* ix) {
    if (!ix) return;
    mi_knn_free(ix->table);
    delete ix;
}

mi_knn* mi_index_table(mi_index* ix) { return ix ? ix->table : nullptr; }

int mi_index_media_dir(mi_index* ix, char* buf, size_t cap, size_t* needed) {
    return guarded([&] {
        if (!ix) fail(MI_ERR_INVALID, "null index handle");
        std::lock_guard<std::mutex> l(ix->mu);
        if (needed) *needed = ix->media_dir.size() + 1;
        if (buf && cap) {
            const size_t n = std::min(cap - 1, ix->media_dir.size());
            std::memcpy(buf, ix->media_dir.data(), n);
            buf[n] = '\0';
        }
    });
}

int mi_index_size(mi_index* ix, uint64_t* rows) {
    return guarded([&] {
        if (!ix || !rows) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(ix->mu);
        *rows = ix->paths.size();
    });
}

int mi_index_existing(mi_index* ix, const char* const* paths, size_t n, uint8_t* exists) {
    return guarded([&] {
        if (!ix || (n && (!paths || !exists))) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(ix->mu);
        for (size_t i = 0; i < n; ++i) {
            if (!paths[i]) fail(MI_ERR_INVALID, "path %zu is null", i);
            exists[i] = ix->rows_of.count(paths[i]) ? 1 : 0;
        }
    });
}

int mi_index_insert(mi_index* ix, const char* const* paths, const float* embeddings, size_t n, uint64_t* first_id) {
    return guarded([&] {
        if (!ix) fail(MI_ERR_INVALID, "null index handle");
        std::lock_guard<std::mutex> l(ix->mu);
        if (first_id) *first_id = ix->paths.size();
        if (n == 0) return;
        if (!paths || !embeddings) fail(MI_ERR_INVALID, "null argument");
        for (size_t i = 0; i < n; ++i)
            if (!paths[i]) fail(MI_ERR_INVALID, "path %zu is null", i);
        call_ok(mi_knn_append(ix->table, embeddings, n));  // the rows first: a failure leaves the path column untouched
        for (size_t i = 0; i < n; ++i) add_path(ix, paths[i]);
    });
}

// paths whose embeddings came from the fused pipeline (mi_pipeline_ingest wrote the rows into mi_index_table already)
int mi_index_adopt(mi_index* ix, const char* const* paths, size_t n) {
    return guarded([&] {
        if (!ix || (n && !paths)) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(ix->mu);
        uint64_t rows = 0;
        call_ok(mi_knn_size(ix->table, &rows));
        if (ix->paths.size() + n != rows)
            fail(MI_ERR_INVALID, "%zu paths for %llu rows without one (the table holds %llu rows, the path column %zu)", n,
                 (unsigned long long)(rows - ix->paths.size()), (unsigned long long)rows, ix->paths.size());
        for (size_t i = 0; i < n; ++i) {
            if (!paths[i]) fail(MI_ERR_INVALID, "path %zu is null", i);
            add_path(ix, paths[i]);
        }
    });
}

int mi_index_rows_of(mi_index* ix, const char* const* paths, size_t n, uint64_t* ids, size_t cap, size_t* count) {
    return guarded([&] {
        if (!ix || !count || (n && !paths)) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(ix->mu);
        std::vector<uint64_t> found;
        for (size_t i = 0; i < n; ++i) {
            if (!paths[i]) fail(MI_ERR_INVALID, "path %zu is null", i);
            auto it = ix->rows_of.find(paths[i]);
            if (it != ix->rows_of.end()) found.insert(found.end(), it->second.begin(), it->second.end());
        }
        // table (id) order whatever the request order, each row once: average_slices adds in input order (search.rs:139-143)
        std::sort(found.begin(), found.end());
        found.erase(std::unique(found.begin(), found.end()), found.end());
        *count = found.size();
        if (ids) std::memcpy(ids, found.data(), std::min(cap, found.size()) * sizeof(uint64_t));
    });
}

int mi_index_path(mi_index* ix, uint64_t id, int web, char* buf, size_t cap, size_t* needed) {
    return guarded([&] {
        if (!ix) fail(MI_ERR_INVALID, "null index handle");
        std::lock_guard<std::mutex> l(ix->mu);
        if (id >= ix->paths.size()) fail(MI_ERR_INVALID, "id %llu out of range (%zu rows)", (unsigned long long)id, ix->paths.size());
        if (ix->removed[id]) fail(MI_ERR_INVALID, "row %llu was removed (mi_index_remove)", (unsigned long long)id);
        std::string p = ix->paths[id];
        // search.rs:104-109: what goes back to the client is relative to "media/"
        if (web && !ix->media_dir.empty() && p.compare(0, ix->media_dir.size(), ix->media_dir) == 0) p = "media/" + p.substr(ix->media_dir.size());
        if (needed) *needed = p.size() + 1;
        if (buf && cap) {
            const size_t n = std::min(cap - 1, p.size());
            std::memcpy(buf, p.data(), n);
            buf[n] = '\0';
        }
    });
}

// web_search_text after the text tower (search.rs:20-110): query = text, refined with the marked images that are in
// the table (mean of their embeddings in id order, then mean of that and the text vector); K nearest by cosine distance.
int mi_index_search(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref, uint32_t k,
                    uint64_t* idx, float* dist, uint32_t* n_found) {
    return guarded([&] {
        if (!ix || !text_embedding || !idx || !dist || (n_ref && !referenced_images)) fail(MI_ERR_INVALID, "null argument");
        const std::vector<float> query = refined_query(ix, text_embedding, referenced_images, n_ref);
        call_ok(mi_knn_search(ix->table, query.data(), 1, k, idx, dist));
        if (n_found) *n_found = hits(idx, k);
    });
}

// ... among the rows under `folders` (folder_rows); the search is mi_knn_search_filtered over those rows
int mi_index_search_within(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref,
                           const char* const* folders, size_t n_folders, uint32_t k, uint64_t* idx, float* dist,
                           uint32_t* n_found) {
    return guarded([&] {
        if (!ix || !text_embedding || !idx || !dist || (n_ref && !referenced_images) || (n_folders && !folders))
            fail(MI_ERR_INVALID, "null argument");
        const std::vector<uint64_t> ids = folder_rows(ix, folders, n_folders);
        const std::vector<float> query = refined_query(ix, text_embedding, referenced_images, n_ref);
        call_ok(mi_knn_search_filtered(ix->table, query.data(), 1, k, ids.data(), ids.size(), idx, dist));
        if (n_found) *n_found = hits(idx, k);
    });
}

// web_search_text with near-duplicates collapsed: the refined query of mi_index_search, the row set of mi_index_search_within
// when folders are given (n_folders = 0: the whole table), then mi_knn_search_diverse
int mi_index_search_diverse(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref,
                            const char* const* folders, size_t n_folders, uint32_t k, uint32_t pool, float min_gap, uint64_t* idx,
                            float* dist, uint32_t* hidden, uint32_t* n_found) {
    return guarded([&] {
        if (!ix || !text_embedding || !idx || !dist || (n_ref && !referenced_images) || (n_folders && !folders))
            fail(MI_ERR_INVALID, "null argument");
        std::vector<uint64_t> ids;
        if (n_folders) ids = folder_rows(ix, folders, n_folders);
        const std::vector<float> query = refined_query(ix, text_embedding, referenced_images, n_ref);
        const uint64_t none = 0;   // folders that match nothing are an empty row set, not "the whole table"
        const uint64_t* among = n_folders ? (ids.empty() ? &none : ids.data()) : nullptr;
        call_ok(mi_knn_search_diverse(ix->table, query.data(), k, pool, min_gap, among, ids.size(), idx, dist, hidden, nullptr,
                                      n_found));
    });
}

// mi_knn_search_compound with the row set of mi_index_search_within when folders are given (n_folders = 0: the whole table).
// No refinement in here: a term that should be refined goes through mi_refine first.
int mi_index_search_compound(mi_index* ix, const float* pos, uint32_t n_pos, int mode, const float* neg, const float* neg_within,
                             uint32_t n_neg, const char* const* folders, size_t n_folders, uint32_t k, uint64_t* idx, float* dist,
                             float* term_dist, uint32_t* n_found) {
    return guarded([&] {
        if (!ix || !pos || !idx || !dist || (n_folders && !folders)) fail(MI_ERR_INVALID, "null argument");
        std::vector<uint64_t> ids;
        if (n_folders) ids = folder_rows(ix, folders, n_folders);
        const uint64_t none = 0;   // folders that match nothing are an empty row set, not "the whole table"
        const uint64_t* among = n_folders ? (ids.empty() ? &none : ids.data()) : nullptr;
        call_ok(mi_knn_search_compound(ix->table, pos, n_pos, mode, neg, neg_within, n_neg, k, among, ids.size(), idx, dist, term_dist));
        if (n_found) *n_found = hits(idx, k);
    });
}

// a page of web_search_text: the refined query of mi_index_search, the row set of mi_index_search_within when folders are given
// (n_folders = 0: the whole table), then mi_knn_search_page
int mi_index_search_page(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref,
                         const char* const* folders, size_t n_folders, uint32_t k, float after_dist, uint64_t after_id, float max_dist,
                         uint64_t* idx, float* dist, uint32_t* n_results, uint64_t counts[4]) {
    return guarded([&] {
        if (!ix || !text_embedding || !idx || !dist || (n_ref && !referenced_images) || (n_folders && !folders))
            fail(MI_ERR_INVALID, "null argument");
        std::vector<uint64_t> ids;
        if (n_folders) ids = folder_rows(ix, folders, n_folders);
        const std::vector<float> query = refined_query(ix, text_embedding, referenced_images, n_ref);
        const uint64_t none = 0;   // folders that match nothing are an empty row set, not "the whole table"
        const uint64_t* among = n_folders ? (ids.empty() ? &none : ids.data()) : nullptr;
        call_ok(mi_knn_search_page(ix->table, query.data(), k, after_dist, after_id, max_dist, among, ids.size(), idx, dist, counts));
        if (n_results) *n_results = hits(idx, k);
    });
}

// the best hit per directory: the refined query of mi_index_search, the row set of mi_index_search_within when folders are
// given (n_folders = 0: the whole table), the table's column brought up to date, then mi_knn_search_grouped
int mi_index_search_grouped(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref,
                            const char* const* folders, size_t n_folders, uint32_t k, float max_dist, uint64_t* idx, float* dist,
                            uint32_t* group, uint64_t* members, uint32_t* n_found, uint64_t* facets, uint64_t cap_facets,
                            uint64_t totals[4]) {
    return guarded([&] {
        if (!ix || !text_embedding || !idx || !dist || (n_ref && !referenced_images) || (n_folders && !folders))
            fail(MI_ERR_INVALID, "null argument");
        std::vector<uint64_t> ids;
        if (n_folders) ids = folder_rows(ix, folders, n_folders);
        const std::vector<float> query = refined_query(ix, text_embedding, referenced_images, n_ref);
        size_t n_dirs = 0;
        {
            std::lock_guard<std::mutex> l(ix->mu);
            n_dirs = ix->dirs.names.size();
            if (facets && cap_facets < n_dirs) fail(MI_ERR_INVALID, "facets holds %llu entries, the index has %zu groups", (unsigned long long)cap_facets, n_dirs);
            sync_groups(ix);
        }
        // the table may know more groups than the index has directories (labels a caller once set on it): its facets go through
        // a buffer of the table's size, the directories' part reaches the caller
        uint64_t info[2] = {0, 0};
        call_ok(mi_knn_groups_info(ix->table, info), MI_ERR_INVALID);
        std::vector<uint64_t> all(facets ? (size_t)std::max<uint64_t>(info[0], 1) : 0);
        const uint64_t none = 0;   // folders that match nothing are an empty row set, not "the whole table"
        const uint64_t* among = n_folders ? (ids.empty() ? &none : ids.data()) : nullptr;
        call_ok(mi_knn_search_grouped(ix->table, query.data(), k, max_dist, among, ids.size(), idx, dist, group, members,
                                      facets ? all.data() : nullptr, all.size(), totals));
        if (facets) std::copy(all.begin(), all.begin() + std::min(n_dirs, all.size()), facets);
        if (n_found) *n_found = hits(idx, k);
    });
}

int mi_index_group_name(mi_index* ix, uint32_t group, int web, char* buf, size_t cap, size_t* needed) {
    return guarded([&] {
        if (!ix) fail(MI_ERR_INVALID, "null index handle");
        std::lock_guard<std::mutex> l(ix->mu);
        if (group >= ix->dirs.names.size()) fail(MI_ERR_INVALID, "group %u is not a directory of this index (%zu groups)", group, ix->dirs.names.size());
        std::string p = ix->dirs.names[group];
        if (web && !ix->media_dir.empty() && p.compare(0, ix->media_dir.size(), ix->media_dir) == 0) p = "media/" + p.substr(ix->media_dir.size());
        if (needed) *needed = p.size() + 1;
        if (buf && cap) {
            const size_t n = std::min(cap - 1, p.size());
            std::memcpy(buf, p.data(), n);
            buf[n] = '\0';
        }
    });
}

int mi_index_group_count(mi_index* ix, uint32_t* n_groups) {
    return guarded([&] {
        if (!ix || !n_groups) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(ix->mu);
        *n_groups = (uint32_t)ix->dirs.names.size();
    });
}

int mi_index_group_of(mi_index* ix, const char* folder, uint32_t* group) {
    return guarded([&] {
        if (!ix || !folder || !group) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(ix->mu);
        std::string dir;
        if (!to_disk(ix, folder, &dir)) fail(MI_ERR_INVALID, "'%s' is not under media/", folder);
        // the dictionary's keys end with their '/' (grouped_dir_of); "media/" itself is the media directory as it is stored
        if (dir.size() > ix->media_dir.size() && dir.back() != '/') dir += '/';
        auto it = ix->dirs.ids.find(grouped_dir_of(dir + "x"));
        if (it == ix->dirs.ids.end()) fail(MI_ERR_INVALID, "no image was stored under '%s'", folder);
        *group = it->second;
    });
}

// the folders at a glance: the table's column brought up to date, then mi_knn_summarize over it (labels = NULL) with one group
// per directory; results land in buffers of the call, the first min(cap, directories) entries reach the caller
int mi_index_folder_overview(mi_index* ix, uint32_t cap, uint64_t* count, uint64_t* cover, float* cover_dist, uint64_t* odd,
                             float* odd_dist, uint64_t* measured, uint64_t* spread, uint32_t* n_groups) {
    return guarded([&] {
        if (!ix || !n_groups) fail(MI_ERR_INVALID, "null argument");
        size_t n_dirs = 0;
        {
            std::lock_guard<std::mutex> l(ix->mu);
            n_dirs = ix->dirs.names.size();
            if (n_dirs > SUMMARY_MAX_C) fail(MI_ERR_UNSUPPORTED, "%zu directories: a summary holds at most %u groups", n_dirs, SUMMARY_MAX_C);
            if (n_dirs) sync_groups(ix);
        }
        if (n_dirs == 0) { *n_groups = 0; return; }
        const uint32_t C = (uint32_t)n_dirs;
        std::vector<uint64_t> u64((size_t)C * 5);
        std::vector<float> f32((size_t)C * 2);
        uint64_t *h_count = u64.data(), *h_cover = h_count + C, *h_odd = h_cover + C, *h_measured = h_odd + C, *h_spread = h_measured + C;
        call_ok(mi_knn_summarize(ix->table, nullptr, C, nullptr, h_count, h_cover, f32.data(), h_odd, f32.data() + C, h_measured,
                                 h_spread, nullptr, nullptr));
        const size_t n = std::min<size_t>(cap, C);
        if (count) std::copy(h_count, h_count + n, count);
        if (cover) std::copy(h_cover, h_cover + n, cover);
        if (cover_dist) std::copy(f32.data(), f32.data() + n, cover_dist);
        if (odd) std::copy(h_odd, h_odd + n, odd);
        if (odd_dist) std::copy(f32.data() + C, f32.data() + C + n, odd_dist);
        if (measured) std::copy(h_measured, h_measured + n, measured);
        if (spread) std::copy(h_spread, h_spread + n, spread);
        *n_groups = C;
    });
}

// the folders' highlights: the covers of mi_knn_summarize over the column, then mi_knn_representatives started at them; the
// first min(cap, directories) folders reach the caller
int mi_index_folder_highlights(mi_index* ix, uint32_t cap, uint32_t m, float min_gap, uint64_t* picks, float* gap, uint32_t* n_picked,
                               uint32_t* n_groups) {
    return guarded([&] {
        if (!ix || !n_groups) fail(MI_ERR_INVALID, "null argument");
        size_t n_dirs = 0;
        {
            std::lock_guard<std::mutex> l(ix->mu);
            n_dirs = ix->dirs.names.size();
            const char* why = "";
            const int bad = rep_check_args(ix, (uint32_t)std::min<size_t>(std::max<size_t>(n_dirs, 1), 0xFFFFFFFFu), m, min_gap, &why);
            if (bad != MI_OK) fail(bad, "%s (%zu directories, m %u)", why, n_dirs, m);
            if (n_dirs) sync_groups(ix);
        }
        if (n_dirs == 0) { *n_groups = 0; return; }
        const uint32_t C = (uint32_t)n_dirs;
        std::vector<uint64_t> cover(C), h_picks((size_t)C * m);
        std::vector<float> h_gap((size_t)C * m);
        std::vector<uint32_t> h_n(C);
        call_ok(mi_knn_summarize(ix->table, nullptr, C, nullptr, nullptr, cover.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr));
        call_ok(mi_knn_representatives(ix->table, nullptr, C, m, min_gap, cover.data(), h_picks.data(), h_gap.data(), h_n.data(), nullptr,
                                       nullptr, nullptr, nullptr));
        const size_t n = std::min<size_t>(cap, C);
        if (picks) std::copy(h_picks.begin(), h_picks.begin() + n * m, picks);
        if (gap) std::copy(h_gap.begin(), h_gap.begin() + n * m, gap);
        if (n_picked) std::copy(h_n.begin(), h_n.begin() + n, n_picked);
        *n_groups = C;
    });
}

// mi_knn_set_attrs by path: every path looked up before anything is written
int mi_index_set_attrs(mi_index* ix, const char* const* paths, size_t n, const uint64_t* tags, const int64_t* stamps) {
    return guarded([&] {
        if (!ix || (n && !paths)) fail(MI_ERR_INVALID, "null argument");
        if (n == 0 || (!tags && !stamps)) return;
        std::vector<uint64_t> ids, tg;
        std::vector<int64_t> st;
        {
            std::lock_guard<std::mutex> l(ix->mu);
            for (size_t i = 0; i < n; ++i) {
                if (!paths[i]) fail(MI_ERR_INVALID, "path %zu is null", i);
                auto it = ix->rows_of.find(paths[i]);
                if (it == ix->rows_of.end()) fail(MI_ERR_INVALID, "'%s' is not a path of this index", paths[i]);
                for (const uint64_t r : it->second) {
                    ids.push_back(r);
                    if (tags) tg.push_back(tags[i]);
                    if (stamps) st.push_back(stamps[i]);
                }
            }
        }
        if (ids.empty()) return;
        call_ok(mi_knn_set_attrs(ix->table, ids.data(), ids.size(), tags ? tg.data() : nullptr, stamps ? st.data() : nullptr));
    });
}

// web_search_text among the rows a predicate keeps: the refined query of mi_index_search, the directory groups brought up to
// date when the predicate names one, then mi_knn_search_where — no id list anywhere
int mi_index_search_where(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref, uint32_t k,
                          const mi_knn_where* where, uint64_t* idx, float* dist, uint32_t* n_found, uint64_t* matched) {
    return guarded([&] {
        if (!ix || !text_embedding || !idx || !dist || (n_ref && !referenced_images)) fail(MI_ERR_INVALID, "null argument");
        const char* why = "";
        const int bad = where_check_pred(where, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        const std::vector<float> query = refined_query(ix, text_embedding, referenced_images, n_ref);
        if (where->flags & MI_KNN_WHERE_GROUP) {
            std::lock_guard<std::mutex> l(ix->mu);
            sync_groups(ix);
        }
        call_ok(mi_knn_search_where(ix->table, query.data(), 1, k, where, idx, dist, matched));
        if (n_found) *n_found = hits(idx, k);
    });
}

// web_search_text as a timeline: the refined query of mi_index_search, the directory groups brought up to date when the
// predicate names one, then mi_knn_search_ordered — the rows of removed paths are deleted rows of the table and never appear
int mi_index_search_ordered(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref, uint32_t k,
                            float max_dist, const mi_knn_where* where, uint32_t flags, int64_t after_stamp, uint64_t after_id,
                            uint64_t* idx, float* dist, int64_t* stamps, uint32_t* n_found, uint64_t counts[4]) {
    return guarded([&] {
        if (!ix || !text_embedding || !idx || !dist || (n_ref && !referenced_images)) fail(MI_ERR_INVALID, "null argument");
        const char* why = "";
        const int bad = ordered_check_args(ix, text_embedding, k, max_dist, where, flags, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (k %u)", why, k);
        const std::vector<float> query = refined_query(ix, text_embedding, referenced_images, n_ref);
        if (where && (where->flags & MI_KNN_WHERE_GROUP)) {
            std::lock_guard<std::mutex> l(ix->mu);
            sync_groups(ix);
        }
        call_ok(mi_knn_search_ordered(ix->table, query.data(), k, max_dist, where, flags, after_stamp, after_id, idx, dist, stamps, counts));
        if (n_found) *n_found = hits(idx, k);
    });
}

// the timeline facet of the same query: mi_knn_stamp_histogram behind the refined query and the group column
int mi_index_stamp_histogram(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref,
                             float max_dist, const mi_knn_where* where, const int64_t* edges, uint32_t n_edges, uint64_t* hist) {
    return guarded([&] {
        if (!ix || !text_embedding || (n_ref && !referenced_images)) fail(MI_ERR_INVALID, "null argument");
        const char* why = "";
        const int bad = ordered_check_hist_args(ix, text_embedding, max_dist, where, edges, n_edges, hist, &why);
        if (bad != MI_OK) fail(bad, "%s (n_edges %u)", why, n_edges);
        const std::vector<float> query = refined_query(ix, text_embedding, referenced_images, n_ref);
        if (where && (where->flags & MI_KNN_WHERE_GROUP)) {
            std::lock_guard<std::mutex> l(ix->mu);
            sync_groups(ix);
        }
        call_ok(mi_knn_stamp_histogram(ix->table, query.data(), max_dist, where, edges, n_edges, hist));
    });
}

int mi_index_save(mi_index* ix, const char* dir) {
    return guarded([&] {
        if (!ix || !dir) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(ix->mu);
        if (::mkdir(dir, 0777) != 0 && errno != EEXIST) fail(MI_ERR_IO, "cannot create directory %s", dir);
        const std::string d(dir);
        call_ok(mi_knn_save(ix->table, (d + "/embedding.miknn").c_str()));  // tmp + fsync + rename inside
        // image_path.bin: "MIPATHv1", u64 rows, u32 media_dir length + bytes, then per row u32 length + bytes
        const std::string tmp = d + "/image_path.bin.tmp", fin = d + "/image_path.bin";
        const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd < 0) fail(MI_ERR_IO, "cannot create %s", tmp.c_str());
        try {
            std::string blob("MIPATHv1");
            const uint64_t rows = ix->paths.size();
            blob.append(reinterpret_cast<const char*>(&rows), 8);
            auto put = [&](const std::string& s) {
                const uint32_t n = (uint32_t)s.size();
                blob.append(reinterpret_cast<const char*>(&n), 4);
                blob.append(s);
                if (blob.size() > (8u << 20)) { write_all(fd, blob.data(), blob.size(), tmp.c_str()); blob.clear(); }
            };
            put(ix->media_dir);
            for (const std::string& p : ix->paths) put(p);
            write_all(fd, blob.data(), blob.size(), tmp.c_str());
            if (::fsync(fd) != 0) fail(MI_ERR_IO, "fsync of %s failed", tmp.c_str());
        } catch (...) {
            ::close(fd);
            throw;
        }
        if (::close(fd) != 0) fail(MI_ERR_IO, "close of %s failed", tmp.c_str());
        if (std::rename(tmp.c_str(), fin.c_str()) != 0) fail(MI_ERR_IO, "cannot rename %s", tmp.c_str());
        const int dfd = ::open(dir, O_RDONLY);  // the renames themselves become durable with the directory
        if (dfd >= 0) { (void)::fsync(dfd); ::close(dfd); }
    });
}

int mi_index_load(mi_index* ix, const char* dir) {
    return guarded([&] {
        if (!ix || !dir) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(ix->mu);
        uint64_t have = 0;
        (void)mi_knn_size(ix->table, &have);
        // (rows the pipeline has written into the table but mi_index_adopt has not named yet count too)
        if (!ix->paths.empty() || have != 0) fail(MI_ERR_INVALID, "mi_index_load needs an empty index (%zu paths, %llu embeddings)",
                                                  ix->paths.size(), (unsigned long long)have);
        const std::string d(dir), pf = d + "/image_path.bin";
        FILE* f = std::fopen(pf.c_str(), "rb");
        if (!f) fail(MI_ERR_IO, "cannot open %s", pf.c_str());
        struct stat sb {};
        const uint64_t file_bytes = ::fstat(fileno(f), &sb) == 0 ? (uint64_t)sb.st_size : 0;
        std::vector<std::string> paths;
        std::string media;
        try {
            char magic[8];
            uint64_t rows = 0;
            if (std::fread(magic, 1, 8, f) != 8 || std::memcmp(magic, "MIPATHv1", 8) != 0 || std::fread(&rows, 8, 1, f) != 1)
                fail(MI_ERR_IO, "%s is not a MIPATHv1 file", pf.c_str());
            auto get = [&](std::string* s) {
                uint32_t n = 0;
                if (std::fread(&n, 4, 1, f) != 1 || n > (1u << 20)) fail(MI_ERR_IO, "%s is truncated or corrupt", pf.c_str());
                s->resize(n);
                if (n && std::fread(&(*s)[0], 1, n, f) != n) fail(MI_ERR_IO, "%s is truncated", pf.c_str());
            };
            get(&media);
            // every row costs at least its 4-byte length: a count the file cannot hold is corruption, not an allocation request
            if (rows > file_bytes / 4) fail(MI_ERR_IO, "%s claims %llu rows in %llu bytes", pf.c_str(), (unsigned long long)rows,
                                            (unsigned long long)file_bytes);
            paths.resize(rows);
            for (auto& p : paths) get(&p);
        } catch (...) {
            std::fclose(f);
            throw;
        }
        std::fclose(f);
        call_ok(mi_knn_load(ix->table, (d + "/embedding.miknn").c_str()));
        uint64_t rows = 0;
        (void)mi_knn_size(ix->table, &rows);
        // the embedding file is written first: it may be NEWER than the path file (a crash between the two renames);
        // rows without a path cannot be served and are not kept.  The other way round cannot happen.
        if (rows < paths.size()) fail(MI_ERR_IO, "%s: %llu embeddings for %zu paths", dir, (unsigned long long)rows, paths.size());
        if (rows > paths.size()) knn_truncate(ix->table, paths.size());  // under the table's own lock; rows beyond are rewritten by later inserts
        ix->media_dir = media;
        // the removed rows are the table's deleted ones (saved in embedding.miknn): no lookup finds them
        uint64_t n_dead = 0;
        std::vector<uint64_t> dead;
        call_ok(mi_knn_deleted(ix->table, nullptr, 0, &n_dead), MI_ERR_INVALID);
        dead.resize(n_dead);
        if (n_dead) call_ok(mi_knn_deleted(ix->table, dead.data(), n_dead, &n_dead), MI_ERR_INVALID);
        std::vector<uint8_t> gone(paths.size(), 0);
        for (uint64_t id : dead)
            if (id < gone.size()) gone[id] = 1;
        for (size_t i = 0; i < paths.size(); ++i) add_path(ix, paths[i], gone[i] != 0);
    });
}

// every image_path that still has a row, once each, NUL-terminated one after the other (the prune of a scan compares them
// with what the walk found); *needed = bytes of the whole list, at most `cap` are written (whole paths only)
int mi_index_live_paths(mi_index* ix, char* buf, size_t cap, size_t* needed) {
    return guarded([&] {
        if (!ix || !needed) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(ix->mu);
        size_t total = 0, at = 0;
        for (const auto& kv : ix->rows_of) {
            const size_t n = kv.first.size() + 1;
            if (buf && at + n <= cap) { std::memcpy(buf + at, kv.first.c_str(), n); at += n; }
            total += n;
        }
        *needed = total;
    });
}

// DELETE FROM image WHERE image_path IN $paths: the rows go from the table (mi_knn_delete, ids stay) and from the lookups
int mi_index_remove(mi_index* ix, const char* const* paths, size_t n, uint64_t* removed_rows) {
    return guarded([&] {
        if (!ix || (n && !paths)) fail(MI_ERR_INVALID, "null argument");
        if (removed_rows) *removed_rows = 0;
        std::lock_guard<std::mutex> l(ix->mu);
        std::vector<uint64_t> ids;
        for (size_t i = 0; i < n; ++i) {
            if (!paths[i]) fail(MI_ERR_INVALID, "path %zu is null", i);
            auto it = ix->rows_of.find(paths[i]);
            if (it != ix->rows_of.end()) ids.insert(ids.end(), it->second.begin(), it->second.end());
        }
        if (ids.empty()) return;
        uint64_t newly = 0;
        call_ok(mi_knn_delete(ix->table, ids.data(), ids.size(), &newly));  // the rows first: a failure changes nothing
        for (uint64_t id : ids) ix->removed[id] = 1;
        for (size_t i = 0; i < n; ++i) {
            ix->rows_of.erase(paths[i]);
            ix->live.erase(paths[i]);
        }
        if (removed_rows) *removed_rows = newly;
    });
}

// mi_knn_compact on the table, then the path column by the same map: the rows the table dropped leave `paths` and `row_dir`,
// the lookups are rebuilt over the new ids (the directory dictionary keeps its group ids: the table's group column travelled
// with the rows, and the next grouped search uploads it again because the table's groups_epoch has moved on)
int mi_index_compact(mi_index* ix, uint64_t* new_ids, uint64_t cap, uint64_t* removed) {
    return guarded([&] {
        if (!ix) fail(MI_ERR_INVALID, "null index handle");
        std::lock_guard<std::mutex> l(ix->mu);
        uint64_t rows = 0;
        (void)mi_knn_size(ix->table, &rows);
        if (new_ids && cap < rows) fail(MI_ERR_INVALID, "new_ids holds %llu entries, the table %llu rows", (unsigned long long)cap, (unsigned long long)rows);
        std::vector<uint64_t> map((size_t)rows);
        uint64_t gone = 0;
        call_ok(mi_knn_compact(ix->table, map.data(), map.size(), &gone));   // the rows first: a failure changes nothing
        if (gone) {
            std::vector<std::string> old;
            old.swap(ix->paths);
            std::vector<uint32_t> old_dir;
            old_dir.swap(ix->row_dir);
            ix->removed.clear();
            ix->rows_of.clear();
            ix->live.clear();
            for (size_t o = 0; o < old.size(); ++o) {
                if (o < map.size() && map[o] == MI_KNN_NO_ID) continue;
                ix->rows_of[old[o]].push_back(ix->paths.size());
                ix->live.insert(old[o]);
                ix->paths.push_back(std::move(old[o]));
                ix->removed.push_back(0);
                ix->row_dir.push_back(old_dir[o]);
            }
            ix->groups_uploaded = 0;
        }
        if (new_ids) std::copy(map.begin(), map.end(), new_ids);
        if (removed) *removed = gone;
    });
}

}  // extern "C"
