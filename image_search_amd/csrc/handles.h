// handles.h — the opaque handles of include/mi355clip.h as the library's translation units see them,
// plus the few host-side routines that cross files (the fused pipeline and the sharded table are built
// from the same forward / scan launchers as the single-handle entry points).
#pragma once
#include <mutex>
#include <vector>

#include "columns.h"
#include "common.h"
#include "device_mem.h"
#include "ids.h"

namespace mi {
typedef unsigned short bf16_t;

struct Layer {
    float *ln1w, *ln1b, *ln2w, *ln2b;
    void *wqkv, *wo, *w1, *w2;  // T [N][K]
    float *bqkv, *bo, *b1, *b2;
    // the LayerNorm in front of q/k/v and of fc1 folded into the linear (bf16 image tower, option "ln_fold"):
    // W' = bf16(W diag(gamma)), c[n] = sum_k W'[n][k], b' = W beta + b
    void *wqkv_f = nullptr, *w1_f = nullptr;
    float *cqkv = nullptr, *bqkv_f = nullptr, *c1 = nullptr, *b1_f = nullptr;
};


}  // namespace mi

struct mi_clip {
    int device = 0, precision = 0;
    int image = 0, patch = 0, grid = 0, S = 0, D = 0, L = 0, H = 0, FF = 0, E = 0, Kp = 0;
    float eps = 1e-5f;
    mi::Scratch allocs;   // the weights, as uploaded at load
    float *cls = nullptr, *pos = nullptr, *pre_w = nullptr, *pre_b = nullptr, *post_w = nullptr, *post_b = nullptr,
          *proj = nullptr;
    void* wpatch = nullptr;  // T [D][Kp]
    std::vector<mi::Layer> layers;
    // workspace for `cap` images (text tower: `text_cap` sequences); the pointers below and in `act` are views into it
    size_t cap = 0;
    mi::Scratch ws;
    float *d_in = nullptr, *d_in2 = nullptr, *d_out = nullptr, *d_out2 = nullptr;
    // activations: set 0 serves a whole chunk; set 1 exists so that two half-chunks can run as two
    // independent streams (see forward()).
    struct Act {
        float *patch = nullptr, *x = nullptr;
        void *col = nullptr, *y = nullptr, *qkv = nullptr, *h = nullptr;
        mi::bf16_t *delta = nullptr, *delta2 = nullptr;  // bf16 path: out_proj / fc2 outputs, added to x by LayerNorm
        // last layer, CLS rows only (n rows, padded to 256): context, residual, LN output, MLP hidden, deltas
        void *c_ctx = nullptr, *c_y = nullptr, *c_h = nullptr;
        float* c_x = nullptr;
        mi::bf16_t *c_d1 = nullptr, *c_d2 = nullptr;
        // ln_fold: per-row partial sums written by the out_proj / fc2 epilogues [M][D / 32][2] and what the q/k/v / fc1
        // epilogues read, {rstd, -mean * rstd} [M][2]
        float *part = nullptr, *stats = nullptr;
        float* c_stats = nullptr;   // ... of the CLS rows (last layer: the query columns are computed for those rows only)
    } act[4];
    mi::Stream aux[3];
    mi::Event ev_fork, ev_join[3];
    // a forward's front (patch gather + patch GEMM) may run on a stream of its own, under the PREVIOUS forward's layers
    // (forward(..., front)): ev_embed[p] = the last embed_ln of activation set p has read `patch` (the next front may
    // overwrite col / patch), ev_front[p] = the front of set p has written `patch` (embed_ln may read it)
    mi::Event ev_embed[4], ev_front[4];
    bool ev_embed_set[4] = {false, false, false, false};
    bool x24 = true;          // bf16 image tower: the residual stream as 24-bit floats in two planes (3 bytes per element instead of 4; option "x24", MI_CLIP_X24)
    bool ln_fold = true;      // bf16 image tower without LayerNorm kernels in the layer loop where the geometry allows (option "ln_fold", MI_CLIP_LN_FOLD; forward() in vit.hip)
    bool fold_ready = false;  // the folded weights were built at load (geometry allows it)
    bool ln_center = true;    // fold_ready handles: the common mode of everything written to the residual stream removed at load / in embed_ln (vit.hip: center_writer; MI_CLIP_LN_CENTER)
    // ln_fold's watch on its own precondition (mi_clip_ln_fold_stats): live rows of the residual stream whose mean lies more
    // than 4 standard deviations off zero (mean^2 > 16 var) — there bf16(x), taken BEFORE the mean is subtracted, starts to
    // lose the bits the LayerNorm tower keeps.  Counted on the device by embed_ln_kernel / ln_stats_kernel (an atomic only when a
    // row trips), rows looked at counted on the host.
    unsigned long long* d_fold_offset_rows = nullptr;
    uint64_t fold_rows_checked = 0;
    int parts = 2;  // MI_CLIP_PARTS: sub-chunks run as independent streams
    int n_cu = 256;
    uint8_t* d_rgb = nullptr;
    // text tower (mi_clip_load_text): token table, device copies of the ids and of the EOS rows
    bool text = false;
    int vocab = 0;
    float* tok = nullptr;
    int *d_ids = nullptr, *d_rows = nullptr;
    size_t text_cap = 0;
    mi::PinnedBuf h_ids_pin, h_out_pin;   // pinned staging of one query's ids / its embedding: the graph copies from / to them
    // one text query as a captured hipGraph (forward_text_one is ~90 short kernels; launched one by one the host's launch
    // calls cost more than the kernels).  state: 0 = not yet run, 1 = ran once eagerly (function attributes are set), 2 = captured
    struct TextGraph {
        int state = 0;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        TextGraph() = default;
        TextGraph(const TextGraph&) = delete;
        TextGraph& operator=(const TextGraph&) = delete;
        ~TextGraph() { drop(); }
        void drop() {   // the caller has waited for the handle's work: a replay in flight reads the exec
            if (exec) (void)hipGraphExecDestroy(exec);
            if (graph) (void)hipGraphDestroy(graph);
            exec = nullptr; graph = nullptr;
            state = 0;
        }
    } text_graph;
    // mi_clip_embed_images: two upload buffers for decoded images (they grow together), the resize intermediate, a copy stream
    mi::DevArray<uint8_t> d_img_src[2];
    mi::DevArray<float> d_img_tmp;    // [image][widest source][3]
    mi::Stream copy_stream;
    mi::Event ev_up[2], ev_used[2];
    mi::Stream stream;
    size_t max_batch = 256;
    // options (mi_clip_set_option; the MI_CLIP_* / MI_GEMM_* environment variables only seed them at load)
    bool split_ln = false;    // MI_PRECISION_BF16_SPLIT: LayerNorm outputs as hi + lo bf16 pairs, q/k/v and fc1 run over K = 2D
    int attn_ver = 2;         // bf16 attention for 64 < S <= 288: 2 = 32-query tiles (attn32_kernels.h), 1 = 16-query tiles
    bool q_prescaled = false; // log2(e)/8 folded into W_q / b_q at load (attn_ver 2 in the tower)
    bool attn_shift = false;  // force the shifted (exact maximum) pass of attn32 — test hook
    int qkv_pad = 128;        // elements added to the image tower's qkv row pitch where attn32 runs (vit.hip: qkv_pitch)
    int qkv_layout = 0;       // 0 = token rows [M][3D + pad]; 1 = head-major planes [3][H][Mp][64] (vit.hip: qkv_head_major)
    bool front_overlap = false; // mi_pipeline_ingest / mi_clip_embed: a forward's patch gather + patch GEMM on the copy stream, under the previous forward (option "front_overlap")
    bool store_nt = true;     // persistent GEMM: q|k|v / h / delta stores with the nt cache policy (outputs a later kernel reads; -0.25..-0.45 ms per forward); option "store_nt"
    bool attn_nt = false;     // attn32: K / V LDS-DMA and query loads with the nt cache policy (read once by one CU); option "attn_nt": -8 % alone, +0.15 ms in the tower (its K / V are warm from the GEMM that wrote them): off
    int attn_order = 1;       // attn32: first pair of workgroup b (0 = b; 1 = transposed, an XCD's workgroups spread over all heads)
    bool full_last = false;   // compute the dead rows of the last layer too (A/B against the reference graph)
    bool split_tail = true;   // cut a short last round of GEMM tiles into quadrant tasks
    int gemm_order = 4;       // persistent GEMM tile order: 0 = row-major; np > 0 = column groups of np weight tiles, an XCD's
                              // concurrent tiles a (32 / np) x np patch (N / 256 > np and divisible by it, else row-major)
    bool text_fast = true;    // one text query (n == 1, CLIP-L text geometry, bf16): the skinny-GEMM path (vit.hip forward_text_one)
    bool attn_f32_mfma = true; // fp32 attention for S <= 272 on the matrix pipe (attn_f32_mfma_kernel); 0 = one thread per query (A/B; option "attn_f32_mfma")
    bool text_fuse = true;    // ... with out_proj inside the attention launch (text_attn_out_kernel; option "text_fuse")
    int ln_nt = 0;            // A/B hook (MI_CLIP_LN_NT / option "ln_nt"): bit 0 = LN1 writes the residual stream back non-temporally, bit 1 = LN1's last-use loads non-temporal; measured within noise, off
    bool im2col_rows = true;  // bf16 tower: the LDS-staged patch gather (im2col_rows_kernel); 0 = the 4P-byte-run form (A/B)
    mi::WorkOrder order;          // serialises this handle's enqueued work across caller streams
    std::mutex mu;
};


struct mi_knn {
    int device = 0;
    uint32_t dim = 0;
    uint64_t base = 0, rows = 0, cap = 0;
    // a shard of a block-cyclic table (mi_knn_sharded): ids = base + ((local / block) * n + rank) * block + local % block
    uint32_t cyc_block = 0, cyc_n = 0, cyc_rank = 0;
    mi::DevArray<float> table;   // [cap][dim] (`cap` counts rows, table.cap elements)
    mi::Stream stream;
    int n_cu = 0;
    // search workspace
    mi::DevArray<float> d_q;        // [16][dim]
    mi::DevArray<uint64_t> d_cand;  // per-wave lists
    mi::DevArray<uint64_t> d_tmp;   // merge level output
    mi::DevArray<uint64_t> d_keys;  // final keys (k rounded up to 1024 multiples)
    mi::DevArray<uint64_t> d_idx;
    mi::DevArray<float> d_dist;
    bool select_path = true;       // 64 < k <= 4096 by radix select over all keys (MI_KNN_SELECT=0: the per-wave LDS lists)
    mi::DevArray<uint32_t> d_keys32;  // one distance key per row (selection path, 64 < k <= 4096)
    mi::DevArray<uint32_t> d_sel;     // 6 x 2048 histogram bins + the collect counter
    // two-stage exact search (mi_knn_set_option "prefilter"): a bf16 copy of the rows + their squared norms, kept up to
    // `mirror_rows` and caught up by the next search; candidate rows / keys of stage 2
    int prefilter = 0;              // 0 off, 1 bf16 mirror, 2 byte mirror
    int coarse_ring = 8;            // rows in flight + 1 per lane group in the byte stage-1 scan (MI_KNN_RING: A/B)
    bool last_prefiltered = false;  // the most recent single-query search went through the two stages
    // bf16 rows (prefilter 1) or byte rows (prefilter 2: dim bytes per row).  Sized in 16-bit units for both: the byte
    // mirror of cap rows takes (cap * dim + 1) / 2 of them
    mi::DevArray<uint16_t> d_mirror;
    mi::DevArray<float> d_scale8;   // prefilter 2: per-row scale, per-row bound factor, rho of the query in flight
    mi::DevArray<float> d_cfac8;
    mi::DevArray<float> d_rho8;
    mi::DevArray<float> d_g8;       // prefilter 2: per-dimension scale [dim] (+ [dim] accumulators), fixed once the first rows are mirrored
    bool g8_ready = false;
    mi::DevArray<float> d_xx;
    bool batch_stage1_mfma = true;  // the shared stage 1 of a group of queries on the matrix pipe (option "batch_stage1")
    mi::DevArray<int8_t> d_digits;  // [KNN_GROUP_MAX = 16][3][dim]: the queries of a group as three signed 7-bit digits
    mi::DevArray<float> d_qs;       // [KNN_GROUP_MAX][4]: {digit scale S, |q|, rho, -}
    int pref_sample = 1;            // k <= 64 over the byte mirror: the collect threshold from a sample of the stage-1 keys — 1: for groups of queries, 2: for single queries too, 0: never (option "prefilter_sample")
    mi::DevArray<uint32_t> d_skeys; // [queries of a group][sample rows]: the keys of every 8th tile, compact
    uint64_t mirror_rows = 0;
    uint64_t g8_rows = 0;              // rows the table held when the channel scales were taken (refreshed at 4x)
    // Feedback of the two-stage search, read back asynchronously (a query or two late, never a host block): after two
    // consecutive fallbacks stage 1 is skipped for the next PREF_SKIP single-query searches and then probed again — a corpus the mirror cannot thin out pays the single
    // pass, not stage 1 on top of it ("prefilter_adaptive" = 0 turns this off).
    static constexpr int PREF_RING = 8, PREF_SKIP = 64;
    bool pref_adaptive = true;
    mi::PinnedBuf h_pref_ring;         // uint32_t [PREF_RING][2]: {candidates, fell back}
    mi::Event pref_ev[PREF_RING];
    bool pref_ev_pending[PREF_RING] = {};
    uint32_t pref_consec = 0, pref_skip_left = 0;
    // behind a skip window exactly two probes go out; until both have reported, later queries keep to the single pass
    // (a caller that enqueues faster than the device answers must not queue dozens of probes behind the first two)
    bool pref_probing = false;
    uint32_t pref_probes_left = 0, pref_reports_due = 0;
    uint64_t pref_seq = 0, pref_skipped = 0;
    mi::DevArray<uint32_t> d_pref_rows;   // [2 * PREF_CAP]: candidate rows, then their exact distance keys
    mi::DevArray<uint64_t> d_pref_keys;   // [4096]: the k best keys of stage 2
    mi::DevArray<uint32_t> d_pref_flag;   // {candidate count, fallback, go}
    // Order across caller streams.  `writes`: the last append (a search must see every row counted in
    // `rows`).  `reads`: the last search (searches share the workspace above, and a reallocation of the
    // table must wait for them).  An append only ever writes rows beyond `rows`, so it does not wait
    // for searches in flight: ingest and query streams overlap.
    mi::WorkOrder writes, reads;
    // Deleted rows (mi_knn_delete): they keep their ids and storage, every search leaves them out.  `dead` = the deleted
    // local rows, ascending; d_tomb = the same as a bitmap (one bit per row, sized by `cap`, carried over by grow()),
    // d_dead = the same rows on the device in deletion order (what a two-stage search walks after stage 1).  With `dead`
    // empty every search runs the code that ran before deletions existed.
    std::vector<uint32_t> dead;
    mi::DevArray<uint64_t> d_tomb;
    mi::DevArray<uint32_t> d_dead;
    // Filtered search (mi_knn_search_filtered): the filter's live local rows, ascending — n_flist of them in pinned host
    // memory, what the upload reads (kept until the next filtered search: every filtered entry point waits for its results),
    // and the device copy.
    mi::PinnedBuf h_flist{hipHostMallocPortable};   // uint32_t rows
    size_t n_flist = 0;
    mi::DevArray<uint32_t> d_flist;
    // Threshold self-join (mi_knn_near_pairs, join.hip): candidate pairs one strip of stage 1 may hand to stage 2 (option
    // "join_cap"; its buffers live for the call only), and {candidates, pairs, strips, tiles} of the last call.
    uint32_t join_cap = 1u << 22;
    uint64_t join_stats[4] = {0, 0, 0, 0};
    // The join with another table (mi_knn_near_pairs_between, join_between.hip), this table as the row side: {candidates, pairs,
    // stage-1 launches, tiles} of the last call; the column side goes through a staged copy even on this table's own device
    // (option "join_stage": what a column side on another device always takes); the column side is walked in chunks of that
    // many rows, staged or not (option "join_stage_rows": 0 = what the staging budget holds)
    uint64_t between_stats[4] = {0, 0, 0, 0};
    int join_stage = 0, join_stage_rows = 0;
    // mi_knn_density / mi_knn_dbscan (density.hip): {candidates pass 1, pairs within, tiles pass 1, candidates pass 2, tiles
    // visited pass 2, tiles skipped pass 2, unions that merged, stage-1 launches} of the last call
    uint64_t dbscan_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // mi_knn_near_pairs_window / mi_knn_density_window / mi_knn_dbscan_window (window.hip; window_call.h: WS_*): {candidates pass
    // 1, pairs within, tiles computed pass 1, tiles skipped by the stamp ranges pass 1, candidates pass 2, tiles computed pass 2,
    // tiles skipped pass 2, stage-1 launches} of the last windowed call; the unwindowed calls' words above are not touched by it
    uint64_t window_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // mi_knn_assign (assign.hip): {candidates, live rows labelled, stage-1 launches, tiles} of the last assign
    uint64_t assign_stats[4] = {0, 0, 0, 0};
    // mi_knn_assign_multi (assign_multi.hip): {candidates, (row, label) hits written, stage-1 launches, tiles} of the last call
    uint64_t assign_multi_stats[4] = {0, 0, 0, 0};
    // mi_knn_search_many / mi_knn_neighbors (search_many.hip): {candidates, (query, row) hits written, stage-1 launches, tiles} of
    // the last call; column segments of a stage-1 launch (option "many_segments": 0 = from the tile counts) and the stride of
    // the threshold pass over the column tiles (option "many_sample": 0 = chosen by the table's size)
    uint64_t search_many_stats[4] = {0, 0, 0, 0};
    int many_segments = 0, many_sample = 0;
    // mi_knn_propose_groups (search_many.hip): {candidates, stage-1 launches, tiles, strips} of the last call
    uint64_t propose_stats[4] = {0, 0, 0, 0};
    // mi_knn_kmeans_seed (kmeans_seed.hip): {candidates, passes run, fallback picks, 0} of the last call
    uint64_t kmeans_seed_stats[4] = {0, 0, 0, 0};
    // the update of mi_knn_kmeans and the centroids of mi_knn_summarize on exact integer sums of 2^-30 instead of the float
    // chains (option "kmeans_fixed_sum": 0 = the float sums; kmeans_update.h)
    int kmeans_fixed_sum = 0;
    // mi_knn_summarize (summary.hip): {segments summed, workgroups of the distance pass, rows read by it, 0} of the last call
    uint64_t summarize_stats[4] = {0, 0, 0, 0};
    // mi_knn_representatives (representatives.hip): {round launches, segments of the member walk, member rows read by the last
    // round launched, 0} of the last call
    uint64_t representatives_stats[4] = {0, 0, 0, 0};
    // mi_knn_search_diverse (diverse.hip): {pool entries P, candidate pairs, conflicting pairs, pool entries hidden} of the last call
    uint64_t diverse_stats[4] = {0, 0, 0, 0};
    // mi_knn_search_compound (compound.hip): {rows or list entries scanned, rows excluded by a negative term, rows with a NaN
    // score, results written} of the last call; workgroups of its scan (option "compound_blocks": 0 = the batched search's grid)
    uint64_t compound_stats[4] = {0, 0, 0, 0};
    int compound_blocks = 0;
    // mi_knn_search_page (page.hip): workgroups of its scan (option "page_blocks": 0 = the single pass's grid)
    int page_blocks = 0;
    // The group column (grouped.hip): one group id per row of capacity, MI_KNN_NO_GROUP = none.  d_groups exists from the first
    // mi_knn_set_groups on (sized by `cap`, carried over by grow(), the rows it gains hold no group); d_groups.host = the same on the
    // host for the rows it has been told about (what get_groups, groups_info and a rebalance read).  n_groups = 1 + the largest
    // group id ever set, n_grouped = rows that hold one; groups_epoch counts the set calls (the index tells from it whether the
    // column still holds what it uploaded).
    mi::RowColumn<uint32_t> d_groups{0xFF};
    uint32_t n_groups = 0;
    uint64_t n_grouped = 0, groups_epoch = 0;
    // mi_knn_search_grouped: the slot arrays best [n_groups] u64 | cnt [n_groups] u32 (d_gslots in 32-bit words) — after a
    // search they hold that search's values (gslots_valid; gslots_groups = its n_groups) for knn_grouped_members; d_gwin = the
    // groups asked there and their counts; workgroups of the reduce and mark passes (option "group_blocks": 0 = four per CU)
    // and the largest n_groups that takes the block-private LDS form of the reduce (option "group_lds_max")
    mi::DevArray<uint32_t> d_gslots;
    mi::DevArray<uint32_t> d_gwin;
    bool gslots_valid = false;
    uint32_t gslots_groups = 0;
    int group_blocks = 0, group_lds_max = 4096;
    // The attribute columns (where.hip): 64 flags (`tags`) and one ordered value (`stamp`) per row of capacity, both 0 by
    // default.  They exist from the first mi_knn_set_attrs on (sized by `cap`, carried over by grow(), the rows they gain hold
    // the defaults); their .host = the same on the host for the rows they have been told about (what get_attrs and a
    // rebalance read).  A table that never set attributes allocates nothing and matches as if every row held the defaults.
    mi::RowColumn<uint64_t> d_tags{0};
    mi::RowColumn<int64_t> d_stamps{0};
    // mi_knn_search_where and its kin: [0, 2) the total (one 64-bit word), [2, 2 + chunks) the chunk counts, then offsets, of
    // the predicate passes; the pinned word the total is copied to; rows per workgroup (option "where_chunk": 0 = 4096)
    mi::DevArray<uint32_t> d_wcounts;
    mi::PinnedBuf h_wtotal;
    int where_chunk = 0;
    // mi_knn_compact (compact.hip): destination rows of one chunk of the in-place move (option "compact_chunk_rows": 0 = what a
    // 64 MiB staging buffer holds), and {rows removed, rows moved, chunks gathered in place, chunks staged} of the last call
    int compact_chunk_rows = 0;
    uint64_t compact_stats[4] = {0, 0, 0, 0};
    std::mutex mu;
};


// The table row-sharded over several GPUs inside one process (sharded.hip).  Global row r lives in block r / block, block b
// on shard b % n at local block b / n; every shard is an ordinary mi_knn whose kernels emit global ids (IdMap).
typedef struct ncclComm* ncclComm_t;
namespace mi {
// one search in flight on a sharded table: per-shard query / result buffers, the gathered lists and the merged result
// on the first shard's device, pinned copies for the host, and where the caller wants them
struct ShardedSlot {
    // a shard's answer is one packed record [nq*k x u64 id | nq*k x f32 distance] (padded to 16 bytes)
    std::vector<DevArray<unsigned char>> d_q, d_rec;   // [shard], sized in bytes
    std::vector<DevArray<unsigned char>> g_rec;        // [shard] (RCCL receive side: n records) or [0] only (copy transport)
    DevArray<unsigned char> m_rec;                     // merged record, on shard 0's device
    PinnedBuf h_q{hipHostMallocPortable}, h_rec{hipHostMallocPortable};   // read and written by streams of several devices
    std::vector<Event> ev;                    // [shard]: list of shard s is in place
    Event done;
    uint32_t nq = 0, k = 0;
    uint64_t* user_idx = nullptr;
    float* user_dist = nullptr;
    bool busy = false;
};
}  // namespace mi

struct mi_knn_sharded {
    static constexpr int N_SLOTS = 8;
    uint32_t dim = 0, block = 0;
    uint64_t rows = 0;
    std::vector<int> devices;
    std::vector<mi_knn*> shard;
    mi::ShardedSlot slots[N_SLOTS];
    int next_slot = 0;
    std::vector<ncclComm_t> comms;
    bool use_rccl = false;
    struct { uint64_t searches = 0, collectives = 0, copies = 0, merges = 0; } stats;   // mi_knn_sharded_stats
    uint64_t generation = 0;                  // of the files last saved or loaded (mi_knn_sharded_save)
    std::vector<mi::Event> ev_src;            // [device ordinal]: the peer copies of the last append_device from that device
    uint64_t join_stats[4] = {0, 0, 0, 0};    // mi_knn_sharded_near_pairs_stats: summed over every shard and shard pair of the last call
    uint64_t dbscan_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // mi_knn_sharded_dbscan_stats: mi_knn::dbscan_stats summed the same way, plus the forest merge
    // mi_knn_sharded_kmeans_stats: {updates run, bytes copied between shards, segments summed in the last update (all shards),
    // merge launches} of the last call
    uint64_t kmeans_stats[4] = {0, 0, 0, 0};
    // mi_knn_sharded_summarize_stats: {segments summed (all shards), bytes copied between shards, merge launches (sums and
    // slots), members} of the last call
    uint64_t summarize_stats[4] = {0, 0, 0, 0};
    // mi_knn_sharded_kmeans_seed_stats: {candidates, passes run, fallback picks, bytes copied between shards} of the last call
    uint64_t kmeans_seed_stats[4] = {0, 0, 0, 0};
    std::mutex mu;
    uint32_t n() const { return (uint32_t)shard.size(); }
};

namespace mi {
// vit.hip
hipStream_t clip_own_stream(mi_clip* m);
void clip_ensure_workspace(mi_clip* m, size_t n);   // frees and reallocates: waits for the handle's pending work
void clip_ensure_copy_stream(mi_clip* m);
void clip_forward(mi_clip* m, const float* d_img, size_t n, float* d_out, hipStream_t s, hipStream_t front = nullptr);
// knn.hip
IdMap knn_id_map(const mi_knn* t);                  // the table's id space (ids.h): what its kernels emit and its calls accept
// ids (nullable: the first n rows) -> local rows, every one checked; MI_ERR_INVALID names the first that is no row.  t->mu held
std::vector<uint32_t> knn_local_rows(const mi_knn* t, const uint64_t* ids, uint64_t n);
hipStream_t knn_own_stream(mi_knn* t);
void knn_grow(mi_knn* t, uint64_t want_rows);       // may reallocate: waits for the handle's pending work
void knn_search_one(mi_knn* t, const float* d_q, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s);
void knn_search_many(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s);  // nq queries in groups that share their passes; results [nq][k]
void knn_truncate(mi_knn* t, uint64_t rows);        // forget the rows behind `rows` (a failed multi-shard append / load rolls back)
// the filtered search of nq queries (contiguous at d_q) over the ids (every one a row of t: checked by the caller), on s
void knn_search_filtered_many(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, const uint64_t* ids, uint64_t n_ids,
                              uint64_t* d_idx, float* d_dist, hipStream_t s);   // t->mu held, device selected
// for the calls that run a scan of their own through the search's selection (compound.hip); t->mu held, device selected
void knn_filter_rows(mi_knn* t, const uint64_t* ids, uint64_t n_ids);            // ids -> t->h_flist / n_flist: live local rows, ascending, once each; MI_ERR_INVALID for an id that is not a row
void knn_filter_upload(mi_knn* t, hipStream_t s);                                // ... -> t->d_flist
// nq queries (contiguous at d_q) over the list in t->d_flist / n_flist (knn_filter_upload's or knn_filter_where's), on s
void knn_filtered_many(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s);
void knn_reduce_lists64(mi_knn* t, uint32_t lists, uint32_t k, uint64_t* keys_out, hipStream_t s);   // the per-wave register lists in t->d_cand (lists x k keys, k <= 64) -> the k smallest, ascending
// the k <= 4096 smallest (key, position) of the n 32-bit keys in t->d_keys32, ascending; list (nullable): positions -> list[position]
void knn_select_keys32(mi_knn* t, uint64_t n, uint32_t k, uint64_t* keys_out, const uint32_t* list, hipStream_t s);
// list l of query u: ids at d_idx_in + l * idx_stride + u * k, distances at d_dist_in + l * dist_stride + u * k (elements)
void knn_merge_lists_device(const uint64_t* d_idx_in, const float* d_dist_in, uint32_t lists, uint32_t nq, uint32_t k,
                            size_t idx_stride, size_t dist_stride, uint64_t* d_idx, float* d_dist, hipStream_t s);   // caller has the device selected
// compound.hip: mi_knn_search_compound behind its argument check (compound_host.h); takes t->mu
void knn_search_compound(mi_knn* t, const float* pos, uint32_t n_pos, int mode, const float* neg, const float* neg_within, uint32_t n_neg,
                         uint32_t k, const uint64_t* among, uint64_t n_among, uint64_t* idx, float* dist, float* term_dist);
// page.hip: mi_knn_search_page behind its argument check (page_host.h); takes t->mu.  cursor_is_id: the lower end of the window is
// built from (after_dist, after_id), which must name a row of t; otherwise first_key (inclusive) is taken as given
void knn_search_page(mi_knn* t, const float* q, uint32_t k, bool cursor_is_id, float after_dist, uint64_t after_id, uint64_t first_key,
                     float max_dist, const uint64_t* among, uint64_t n_among, uint64_t* idx, float* dist, uint64_t* counts);
// page.hip: knn_page_scan_kernel<NCH, 1> without a cursor — one distance key per row or list entry (0xFFFFFFFF outside [0, hi]) and
// counts += {0, window, beyond, nan}; t->mu held, device selected, the query in t->d_q
void knn_page_scan_keys32(mi_knn* t, hipStream_t s, uint64_t n, const uint32_t* list, const uint64_t* tomb, uint64_t hi, uint32_t k,
                          uint32_t* keys32, unsigned long long* counts);
void knn_groups_fit(mi_knn* t);   // knn.hip: the group column covers `cap` rows (created on first use; new rows hold no group); t->mu held, device selected
// grouped.hip: mi_knn_search_grouped behind its argument check (grouped_host.h); takes t->mu.  cnt_out (nullable): the per-group
// counts of this search, [t->n_groups]
void knn_search_grouped(mi_knn* t, const float* q, uint32_t k, float max_dist, const uint64_t* among, uint64_t n_among, uint64_t* idx,
                        float* dist, uint32_t* group, uint64_t* members, uint64_t* facets, uint64_t cap_facets, uint64_t* totals,
                        std::vector<uint32_t>* cnt_out);
// out[j] = t's count, from its last grouped search, of group[j] (0: no group, unknown group, or that search had no candidate); takes t->mu
void knn_grouped_members(mi_knn* t, const uint32_t* group, uint32_t k, uint32_t* out);
void knn_attrs_fit(mi_knn* t);    // knn.hip: the attribute columns cover `cap` rows (created on first use; new rows hold 0 / 0); t->mu held, device selected
// where.hip: the predicate -> t->d_flist / t->n_flist, exactly what knn_filter_rows + knn_filter_upload leave for the ids of
// the qualifying rows (live local rows, ascending); t->h_flist is not touched.  Runs the predicate passes on s and waits for
// their total (8 bytes).  w checked by the caller (where_host.h); t->mu held, device selected
void knn_filter_where(mi_knn* t, const mi_knn_where* w, hipStream_t s);
// ordered.hip: mi_knn_search_ordered behind its argument check (ordered_host.h); takes t->mu.  cur (nullable): the cursor as the
// sharded call hands it to a shard (ordered_cursor_shard); otherwise it is built from (flags, after_stamp, after_id), which must
// name a row of t.  counts: {within, before, beyond, nan}
struct OrderedCursor;
void knn_search_ordered(mi_knn* t, const float* q, uint32_t k, float max_dist, const mi_knn_where* w, uint32_t flags, int64_t after_stamp,
                        uint64_t after_id, const OrderedCursor* cur, uint64_t* idx, float* dist, int64_t* stamps, uint64_t* counts);
// ordered.hip: mi_knn_stamp_histogram behind its argument check; takes t->mu
void knn_stamp_histogram(mi_knn* t, const float* q, float max_dist, const mi_knn_where* w, const int64_t* edges, uint32_t n_edges,
                         uint64_t* hist);
// join.hip: the self-join of mi_knn_near_pairs with first_new as a LOCAL row (0 = everything, >= rows = nothing): pairs as local
// rows a < b with the join's distance, ascending by (a, b); *over = more than user_cap qualify (out is then partial).  Takes
// t->mu and leaves the call's figures in t->join_stats
struct JoinPair { uint32_t a, b; float d; };
void knn_near_pairs_local(mi_knn* t, float max_dist, uint64_t first_new_local, uint64_t user_cap, std::vector<JoinPair>* out, bool* over);
// sharded.hip
void sharded_place(const mi_knn_sharded* t, uint64_t r, uint32_t* s, uint64_t* local);
uint64_t sharded_rows_of(const mi_knn_sharded* t, uint64_t total, uint32_t s);  // rows shard s holds when the table holds `total`
void sharded_search_enqueue(mi_knn_sharded* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist,
                            const std::vector<std::vector<uint64_t>>* filter = nullptr,
                            const mi_knn_where* where = nullptr);  // t->mu held
void sharded_deliver_all(mi_knn_sharded* t);                                    // t->mu held
// sharded_calls.hip: the predicate's count and the columns the shards keep for their own rows (mi_knn_sharded_rebalance carries
// them over with these), behind the argument checks of their public calls; t->mu held.  ids == nullptr: the first n rows
uint64_t sharded_count_where(mi_knn_sharded* t, const mi_knn_where* w);
uint64_t sharded_delete(mi_knn_sharded* t, const uint64_t* ids, uint64_t n);     // every id checked first; returns the newly deleted
std::vector<uint64_t> sharded_deleted(mi_knn_sharded* t);                        // the deleted global ids, ascending
void sharded_set_groups(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, const uint32_t* groups);
void sharded_get_groups(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, uint32_t* groups);
void sharded_groups_info(mi_knn_sharded* t, uint64_t info[2]);
void sharded_set_attrs(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, const uint64_t* tags, const int64_t* stamps);
void sharded_get_attrs(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, uint64_t* tags, int64_t* stamps);
}  // namespace mi
