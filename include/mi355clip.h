/*
 * mi355clip.h — C ABI of libmi355clip.so: the MI355X (gfx950) replacement for the
 * one compute hot path of olFi95/image_search:
 *   Seam A  CLIP ViT-L/14 image tower   [n,3,224,224] f32 -> [n,768] f32
 *   Seam B  cosine K-nearest over the stored [N,768] f32 embedding table
 *   + the 24-line query refinement (average_slices).
 * The reference has no FFI of its own; each entry point below cites the reference
 * call site (file:line under /root/reference) whose semantics it pins.  The Rust
 * binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; opaque handles; caller owns every buffer.
 *   - every function returns MI_OK (0) or a negative MI_ERR_*; nothing throws,
 *     aborts or panics across the ABI (the reference panics/aborts on errors,
 *     server/Cargo.toml:9 — a drop-in must not).  mi_last_error() gives the
 *     thread-local message of the last failure on the calling thread.
 *   - a handle serialises internally (one mutex per handle, the reference's
 *     model: server/src/main.rs:33-34); distinct handles are independent.
 *   - "host" pointers are ordinary memory; "_device" entry points take HIP
 *     device pointers on the handle's device and a hipStream_t passed as void*
 *     (NULL = the handle's own stream) and do not synchronise the stream.
 *     NB: NULL is NOT "the device's NULL stream": a device buffer that another stream is still writing — the legacy default
 *     stream of a framework included, which is what PyTorch's current stream is unless one is set — must be complete
 *     before it is handed over with NULL, or be handed over with the stream that produces it (a dev tool of this
 *     repository got this wrong for three rounds: tools/knn_prefilter_soak.py).
 *     The work a handle enqueues runs in CALL ORDER whichever streams the calls
 *     name: every entry point first makes its stream wait (an event, no host
 *     block) for what the handle enqueued before.  So embed_device(stream A) ->
 *     append_device(stream A) -> search(stream B) scans the appended rows.  One
 *     exception, on purpose: an append does not wait for searches in flight (it
 *     only writes rows they do not scan), so the ingest stream never stalls on a query.
 *   - there is NO CPU fallback: without a usable gfx950 device, creation fails
 *     with MI_ERR_NO_DEVICE.
 */
#ifndef MI355CLIP_H
#define MI355CLIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK 0
#define MI_ERR_INVALID (-1)     /* bad argument (null pointer, zero dim, ...) */
#define MI_ERR_IO (-2)          /* weights file missing / unreadable / malformed */
#define MI_ERR_HIP (-3)         /* a HIP runtime call failed */
#define MI_ERR_NO_DEVICE (-4)   /* no gfx950 device with that ordinal */
#define MI_ERR_UNSUPPORTED (-5) /* shape outside what the kernels are built for */
#define MI_ERR_OOM (-6)

#define MI_PRECISION_F32 0  /* fp32 in / fp32 accumulate: the parity path (<= 1e-4 rel) */
#define MI_PRECISION_BF16 1 /* bf16 MFMA operands, fp32 accumulate + fp32 residual stream */
#define MI_PRECISION_BF16_SPLIT 2 /* as BF16, but every LayerNorm output feeds its GEMM as a hi + lo bf16 pair (K = 2D
                                   * against [W | W]): for towers whose LayerNorm outputs carry outlier channels */
#define MI_PRECISION_BF16X3 3 /* image tower only: every encoder GEMM as three bf16 MFMA passes over hi + lo halves of both
                               * operands (x_hi w_hi + x_lo w_hi + x_hi w_lo), fp32 attention and residual: within 1e-4 */

#define MI_KNN_NO_ID UINT64_MAX /* id written for missing results (fewer than k rows) */

typedef struct mi_clip mi_clip;         /* a loaded vision (or text) tower on one GPU */
typedef struct mi_knn mi_knn;           /* one row-shard of the embedding table on one GPU */
typedef struct mi_pipeline mi_pipeline; /* scan-loop body + query fused on HIP streams (one GPU) */
typedef struct mi_knn_sharded mi_knn_sharded; /* the table row-sharded over several GPUs, one process */
typedef struct mi_index mi_index;       /* table `image` {id, image_path, embedding}: a shard + the path column */

const char* mi_last_error(void);
/* ABI version of this header (bumped on any signature change). */
int mi_abi_version(void);
/* number of visible HIP devices (0 when there is none; never fails hard). */
int mi_device_count(void);

/* ---------------------------------------------------------------- Seam A: ViT */

/* Replaces clip::clip_vit_large_patch14::Model::from_file(path, &device)
 * (server/src/clip.rs:46-48; weights produced by clip/build.rs:75-83).
 * `weights_path` is a Hugging Face safetensors file holding the
 * CLIPVisionModelWithProjection tensors (vision_model.* + visual_projection.weight,
 * F32/F16/BF16); dimensions are read from the tensor shapes, so the CLIP ViT
 * geometries the kernels are built for load (ViT-L/14: 24 x 1024, 16 heads, 257 tokens):
 * head_dim 64, hidden size 128, 256, 384, 512, 768, 1024, 1280, 1536 or 1664, intermediate
 * size a multiple of 128, G*G + 1 positions (at most 288 in the bf16 precisions).  Any other
 * geometry is refused here with MI_ERR_UNSUPPORTED, a malformed file with MI_ERR_IO — never
 * at the first forward.
 * The handle is meant to stay resident across scans (the reference reloads
 * 1.16 GB on every scan). */
int mi_clip_load(const char* weights_path, int device, int precision, mi_clip** out);
void mi_clip_free(mi_clip* m);
/* `weights_path` may also be the file the reference's `-w` points at (server/src/server_arguments.rs:8-9): the Burn
 * named-MessagePack record `vision_model.mpk` that burn-import writes at build time (clip/build.rs:75-83).  Its field
 * names are those of the GENERATED module, which is not in the reference tree, so its tensors are mapped to the
 * Hugging Face names by shape, module and graph order (Linear weights transposed from Burn's [in, out]).  Both the fused
 * LayerNorm inventory and the DECOMPOSED one of the opset-16 graph the reference builds (clip/scripts/upgrade_opset.py:9-28:
 * gamma / beta as bare constants, scalar and integer constants beside them) are recognised, with the linears as Linear modules
 * or as bare MatMul + Add constants; leaves that cannot be a tower tensor are set aside and listed; an inventory that fits
 * neither form is refused (MI_ERR_UNSUPPORTED) with the inventory in the message.
 * Untested against a real burn-import file (none exists offline); tools/make_synthetic_mpk.py writes the test files.
 *
 * mi_weights_list: the tensors either kind of file holds, as this library names them, one "name dtype [shape]" line
 * each, into buf (NUL-terminated, truncated to cap); *needed (may be NULL) = bytes for the whole listing.  Needs no GPU. */
int mi_weights_list(const char* weights_path, char* buf, size_t cap, size_t* needed);

/* Run-time options of a loaded handle (the MI_CLIP_* environment variables only seed them at load;
 * nothing on the hot path reads the environment):
 *   "max_batch"  images per internal pass (default 256)
 *   "parts"      1..4 sub-chunks of a pass run as independent streams (default 2; bf16 tower)
 *   "full_last"  1 = also compute the rows of the last layer that never reach the output (default 0:
 *                the pooled output is the CLS row, the result is bit-identical either way)
 *   "front_overlap" 1 = where the library uploads the images itself (mi_pipeline_ingest, mi_clip_embed) a forward's front — the
 *                patch gather and the patch GEMM, the only readers of the uploaded batch — is enqueued on the copy stream right
 *                behind its upload and runs under the PREVIOUS forward's layers (events order it against the embed kernels on
 *                either side).  Same bits.  mi_pipeline_stats' forward time then starts at the embed kernel
 *   "attn_shift" 1 = always take the shifted (exact row maximum) pass of the bf16 attention (default 0: taken
 *                only for queries whose softmax numerators leave the exponent range; same result)
 *   "attn_order" which (image, head) pairs a workgroup of the persistent bf16 attention walks: 1 (default) = the 32 workgroups
 *                that share an XCD start on all 16 heads of two images; 0 = workgroup b starts at pair b (an XCD then sits on
 *                two heads for the whole launch: a quarter of its L2 channels).  Same bits
 *   "qkv_pad"    elements added to the row pitch of the bf16 image tower's q|k|v activations where the persistent attention
 *                runs (default 128 = 256 bytes; a multiple of 64 in 0..1024; 0 = dense 3 D rows, the layout of rounds 1-4:
 *                a head's pieces then fall on few memory channels and attention takes 15-20 % longer).  Same bits
 *   "qkv_layout" how the bf16 image tower keeps q|k|v between the q/k/v GEMM and the persistent attention: 0 = token rows
 *                [M][3 D + qkv_pad]; 1 = head-major planes [3][H][Mp][64] (the GEMM's epilogue stores one contiguous KiB per
 *                wave-instruction, attention fetches a head's K / V / q of one image as one contiguous block).  Same bits
 *   "store_nt"   1 (default) = the persistent GEMM writes q|k|v, h and the deltas — outputs a LATER kernel reads — with the nt cache
 *                policy, so that they do not take the XCDs' L2 lines from the operands the same launch streams: - 0.25 ... - 0.45 ms
 *                per 256-image forward; 0 = default policy (A/B hook).  Same bits
 *   "attn_nt"    1 = the persistent attention fetches K, V and q — each read exactly once, by one CU — with the nt cache policy
 *                (A/B hook, default 0: the kernel alone is 8 % faster with it, the tower 0.4 % slower — its K / V are still warm
 *                from the GEMM that wrote them).  Same bits
 *   "split_tail" 0 = do not cut a short last round of GEMM tiles into quadrant tasks (A/B hook)
 *   "gemm_order" tile order of the persistent GEMM: np > 0 (default 4) = an XCD's concurrent tiles are a (32 / np) x np patch
 *                inside one column group of np weight tiles (which stay in its L2); 0 = row-major.  Same bits; -2.3 % per forward
 *   "im2col_rows" 0 = the patch gather in 4P-byte runs instead of the LDS-staged rows form (A/B hook; same bits)
 *   "ln_nt"      bit 0 = LN1 writes the residual stream back with non-temporal stores, bit 1 = LN1's last-use loads are
 *                non-temporal (A/B hook, default 0; same bits, no measurable effect)
 *   "x24"        1 (default) = the bf16 tower keeps its residual stream as 24-bit floats in two planes (16 significant
 *                bits, 3 bytes per element: -14 % LayerNorm traffic, -1 % per forward, error against fp32 unchanged);
 *                0 = fp32 rows.  Neither changes the fp32 parity path or the text tower
 *   "ln_fold"    1 (default) = the bf16 image tower runs layers 0 .. L-2 WITHOUT LayerNorm kernels: gamma is folded into the
 *                q/k/v and fc1 weights at load, out_proj / fc2 add their output to the residual planes in their own epilogue
 *                and emit per-row sums, q/k/v / fc1 finish the LayerNorm in theirs (rstd * (acc - mean * c) + b').  Needs
 *                hidden and intermediate sizes that are multiples of 256 and at least two layers (MI_ERR_UNSUPPORTED when
 *                set to 1 on another geometry; such handles silently keep the LayerNorm kernels).  0 = LayerNorm kernels
 *                (rounds 1-4).  -5.7 % per forward; error against fp32 unchanged; a different rounding sequence, so NOT the
 *                same bits as 0.  "x24" and "ln_nt" only act on the LayerNorm form.  Both weight forms stay resident
 *                so that the option switches per forward: + 0.35 GB per bf16 ViT-L/14 handle (W_qkv, W_fc1 plain and folded)
 *   "attn_f32_mfma" 0 = the fp32 path's attention as one thread per query (rounds 1-4) instead of the exact-f32 MFMA kernel
 *                (another summation order, both far inside 1e-4; A/B hook)
 *   "text_fast"  0 = a single text query takes the batched kernels instead of the skinny-GEMM path (text handles)
 *   "text_fuse"  0 = on that path, attention and out_proj as two launches with a bf16 delta between them (rounds 2-4);
 *                1 (default) = one launch per layer, the heads' out_proj contributions summed in fp32 by the LayerNorm */
int mi_clip_set_option(mi_clip* m, const char* key, int value);

/* geometry of a loaded model: out[0..7] = image, patch, tokens, hidden, layers,
 * heads, ff, proj */
int mi_clip_info(const mi_clip* m, uint32_t out[8]);

/* The LayerNorm-free layer loop ("ln_fold", the bf16 image tower's default) watches its own precondition.  It feeds the
 * q/k/v and fc1 GEMMs bf16(x) of the UN-normalised residual row, so a row whose mean lies r standard deviations off zero
 * carries about r times the rounding error of the LayerNorm tower (which rounds after subtracting the mean).  Measured on
 * seeded ViT-L/14 with a common offset planted on the stream (tools/bf16_acceptance.py; max error / rms against
 * the fp32 tower, stated bound 3e-2): r = 0, 1: 1.5e-2, where the LayerNorm tower is; r = 4: 2.3e-2; r = 16: 8.8e-2 (out of
 * bound, top-1 agreement 96 % instead of 99 %); r = 64: 0.30.  A single massive channel (100 sigma) is harmless: it moves the
 * deviation, not the mean.
 * Two defences.  (1) At load the library removes the common mode of everything that writes to the residual stream (out_proj
 * and fc2 weights and biases, the pre-LayerNorm's output): every reader of the stream is a LayerNorm, so the function is
 * unchanged and the rows have mean ~ 0 whatever the checkpoint's biases are (MI_CLIP_LN_CENTER=0 at load keeps the weights as
 * read; with it the r = 64 study reads 1.5e-2 again).  (2) Every forward counts, on the device, the live token rows (all
 * layers) with mean^2 > 16 var (r > 4):
 *   out[0] = such rows since load / the last reset,  out[1] = rows looked at.
 * out[0] != 0: set option "ln_fold" to 0 (LayerNorm kernels, +6 % per forward, insensitive to r).
 * Waits for the handle's enqueued forwards.  Handles without the loop (fp32, BF16_SPLIT, text, other geometries) report 0, 0.
 * The reference loads whatever checkpoint -w names (server/src/clip.rs:46-48): this is the check that goes with it. */
int mi_clip_ln_fold_stats(mi_clip* m, uint64_t out[2], int reset);

/* Replaces `model.forward(Tensor::from_data(TensorData::new(buf,[n,3,224,224])))`
 * + `output.to_data()` (server/src/clip.rs:112-124).  Host pointers.
 * nchw: [n,3,H,W] contiguous f32 (H = W = 224 for ViT-L/14), as
 * image_prepare_resnet lays it out (server/src/clip.rs:153-175);
 * out: [n,proj] contiguous f32 (proj = 768), NOT L2-normalised.
 * n = 0 is a successful no-op (the reference calls forward on an empty chunk,
 * server/src/clip.rs:112-118).  Any n: tiled internally. */
int mi_clip_embed(mi_clip* m, const float* nchw, size_t n, float* out);

/* Same computation on device-resident buffers (rows (a3) of SURVEY.md §8:
 * removes the two host copies and the blocking readback of
 * server/src/clip.rs:107-124).  Asynchronous on `stream`. */
int mi_clip_embed_device(mi_clip* m, const float* d_nchw, size_t n, float* d_out, void* stream);

/* image_prepare_resnet's arithmetic (server/src/clip.rs:158-172) fused in front
 * of the tower: rgb8 = [n,H,W,3] interleaved u8 already at model resolution
 * (what `resize_exact(..).to_rgb8().as_raw()` returns), host pointers. */
int mi_clip_embed_rgb8(mi_clip* m, const uint8_t* rgb8, size_t n, float* out);

/* host-only restatement of the same arithmetic for callers that keep the
 * reference's two-step flow: rgb8 [n,H,W,3] -> chw f32 [n,3,H,W]. */
int mi_preprocess_rgb8(const uint8_t* rgb8, size_t n, uint32_t height, uint32_t width, float* chw);

/* The resize in front of that arithmetic: `img.resize_exact(224, 224, FilterType::CatmullRom)`
 * (server/src/clip.rs:154), i.e. image-0.25.8's separable resampler (Cargo.lock:5008-5009;
 * imageops/sample.rs: vertical pass into f32, horizontal pass, clamp, round half away from zero),
 * run on GPU `device`.  rgb8 = [height][width][3] interleaved u8 (a decoded photo; RGBA / grey
 * inputs give the same RGB bytes when expanded first, the crate filters channels independently),
 * out = [new_height][new_width][3].  Equal sizes copy, as the crate does.  Extents up to 32768 and
 * reductions up to 255x; zero extents and sizes beyond those limits return MI_ERR_UNSUPPORTED. */
int mi_resize_catmullrom_rgb8(int device, const uint8_t* rgb8, uint32_t width, uint32_t height, uint32_t new_width,
                              uint32_t new_height, uint8_t* out);

/* image_prepare_resnet whole (server/src/clip.rs:153-175): one decoded RGB8 image of any size ->
 * chw f32 [3][224][224], resize and normalisation fused on the device. */
int mi_image_prepare_resnet(int device, const uint8_t* rgb8, uint32_t width, uint32_t height, float* chw);

/* One chunk of the scan loop (server/src/clip.rs:92-124) in one call: n decoded RGB8 images of
 * any sizes (rgb8[i] = [heights[i]][widths[i]][3], host pointers) -> resize + normalise on the
 * device straight into the tower's input -> out [n,768] f32.  Uploads overlap the resize of the
 * previous image. */
int mi_clip_embed_images(mi_clip* m, const uint8_t* const* rgb8, const uint32_t* widths, const uint32_t* heights,
                         size_t n, float* out);

/* The text tower of the same model (HF `CLIPTextModelWithProjection` tensors in the safetensors
 * file): what `clip(state, text)` gets from embed_anything (server/src/clip.rs:19-23, :35-40) and
 * feeds to the refine step / kNN as the query.  Tokenisation stays with the caller:
 * input_ids = [n][positions] int32 (BOS .. EOS, padded; positions = mi_clip_info()[2], 77 for CLIP),
 * the pooled row is the one holding the largest id (the EOS token), as in OpenAI CLIP / candle.
 * out = [n, 768] f32, not normalised.  MI_PRECISION_F32 (parity, 3.3 ms per query) or MI_PRECISION_BF16 (bf16 MFMA
 * GEMMs and causal bf16 attention: the request path, server/src/clip.rs:19-23 sits in front of every search).
 * The handle is freed with mi_clip_free; the image entry points reject it and vice versa. */
int mi_clip_load_text(const char* weights_path, int device, int precision, mi_clip** out);
int mi_clip_embed_text(mi_clip* m, const int32_t* input_ids, size_t n, float* out);

/* ---------------------------------------------------------------- Seam B: kNN */

/* One shard of table `image{embedding}` (server/src/search.rs:13-18; index DDL
 * server/src/clip.rs:140-143: DIMENSION 768, DIST COSINE, TYPE F32) resident in
 * HBM as row-major f32.  dim must be a multiple of 64.  Row ids are
 * base + insertion ordinal (uint64); base defaults to 0 and is the shard's
 * first global row when the table is row-sharded over several GPUs. */
int mi_knn_create(uint32_t dim, int device, mi_knn** out);
void mi_knn_free(mi_knn* t);
int mi_knn_set_base(mi_knn* t, uint64_t base);
/* Options of a shard.  "prefilter" = 1 or 2: two-stage EXACT search for k <= 4096 on shards of >= 2^18 rows — a mirror of the
 * rows (1: bf16, + 50 % device memory, dim % 128 == 0; 2: bytes with a per-row scale, + 25 %, dim % 256 == 0; built by the
 * next search, kept up to date by every later one) is scanned first, the rows that a rigorous error bound (1: data-
 * independent; 2: per row and query) cannot exclude are re-evaluated from the fp32 rows with the single-pass arithmetic:
 * same ids, same distance bits, a half (1) or a quarter (2) of the bytes per query.  Corpora that put more than 2^22
 * rows inside the bound fall back to the single pass on the device.  0 (default) frees the mirror.
 * "batch_stage1" = 1 (default) / 0: how a GROUP of queries (mi_knn_search with nq >= 2, mi_knn_search_batched_device) runs its
 * shared stage 1 over the byte mirror: 1 on the matrix pipe (any group size up to 16; HBM-bound), 0 on the vector ALU
 * (groups of 8 / 4 / 2; the round-3 form, kept for A/B).  Same answers either way.
 * "prefilter_sample" = 1 (default) / 2 / 0: with the byte mirror and k <= 64 a GROUP of queries takes its collect threshold from the
 * k-th smallest upper bound of a SAMPLE of the stage-1 keys (every 8th tile): a valid, looser threshold — a few times more rows
 * for stage 2, an eighth of the select's reads (16 queries per call: - 11 %).  2: single queries too (measured equal at k = 10,
 * 2 % slower at k = 64).  0: always the threshold over all keys.  Same answers either way.
 * "prefilter_adaptive" = 1 (default) / 0: the two-stage search watches itself — candidate counts and fallbacks are read
 * back asynchronously; after two consecutive fallbacks (more than 2^22 candidates) the next 64 single-query searches run
 * the single pass alone (what such a corpus would pay anyway, without stage 1 on top), then stage 1 is probed again with
 * two queries.  Results never change.  The channel scales of the byte mirror are taken again (and the
 * mirror rebuilt, 10 ms per 10 M rows) when the table has grown 4x since they were taken. */
int mi_knn_set_option(mi_knn* t, const char* key, int value);
/* Of the most recent single-query search of this shard (waits for it): how many rows stage 2 re-evaluated, and whether the
 * single pass had to answer instead (then `candidates` is the count that did not fit).  Both 0 when the search did not
 * go through the prefilter (option off, k > 4096, fewer than 2^18 rows, stage 1 switched off for the moment by the adaptive
 * rule).  Behind a batched call: of the FIRST query of its last group. */
int mi_knn_prefilter_stats(mi_knn* t, uint32_t* candidates, uint32_t* fell_back);
/* The adaptive state (waits for the searches in flight): out = {searches for which stage 1 is still switched off,
 * consecutive fallbacks seen, searches that skipped stage 1 so far, rows the table held when the byte mirror's channel
 * scales were taken}. */
int mi_knn_prefilter_state(mi_knn* t, uint32_t out[4]);
int mi_knn_reserve(mi_knn* t, uint64_t rows); /* capacity hint; keeps contents */
int mi_knn_size(const mi_knn* t, uint64_t* rows);

/* Replaces db.insert("image").content(rows) (server/src/clip.rs:125-137): append n
 * rows of dim f32 (host pointers). */
int mi_knn_append(mi_knn* t, const float* rows, uint64_t n);
/* append rows already on the device (e.g. straight from mi_clip_embed_device) */
int mi_knn_append_device(mi_knn* t, const float* d_rows, uint64_t n, void* stream);
/* append n synthetic rows generated on the device: global rows
 * [first_row, first_row+n) of the seeded corpus of image_search_amd/synth.py */
int mi_knn_append_synthetic(mi_knn* t, uint64_t seed, uint64_t first_row, uint64_t n);
/* copy rows [first, first+n) back to the host (tests, refine's row fetch:
 * server/src/search.rs:43-58) */
int mi_knn_get_rows(mi_knn* t, uint64_t first, uint64_t n, float* out);

/* Persistence of a shard (what the database's storage does for `image.embedding`,
 * server/src/clip.rs:125-137): mi_knn_save writes {32-byte header, rows*dim f32} to `path` (through
 * `path`.tmp + fsync + rename: a crash or a full disk leaves the previous file); mi_knn_load appends a
 * file's rows to the table (an empty table takes the file's id base; a non-empty one accepts only the
 * file that continues its ids).  Streamed in 64 MiB pieces: no host copy of the table on either side. */
int mi_knn_save(mi_knn* t, const char* path);
int mi_knn_load(mi_knn* t, const char* path);

/* Replaces `DELETE FROM image WHERE id IN $ids` (the row removal the reference's database offers; the scan of
 * server/src/clip.rs:42-151 only ever adds).  ids are the table's own (base + ordinal; on a shard borrowed through
 * mi_knn_sharded_shard: the ids its searches report).  A deleted row keeps its id and its storage (mi_knn_size counts it,
 * mi_knn_get_rows returns it) and no later search returns it; searches enqueued before the call may.  Deleting a deleted
 * row does nothing; an id that is not a row of the table fails the whole call (MI_ERR_INVALID) and nothing changes.
 * *newly (may be NULL) = rows that were live before the call.  mi_knn_save writes "MIKNNv02" files (the rows, then the
 * deleted rows) for a table with deletions, the MIKNNv01 file otherwise; mi_knn_load reads both. */
int mi_knn_delete(mi_knn* t, const uint64_t* ids, uint64_t n, uint64_t* newly);
/* *count = deleted rows; the first min(cap, count) of their ids, ascending, into ids (may be NULL) */
int mi_knn_deleted(mi_knn* t, uint64_t* ids, uint64_t cap, uint64_t* count);
/* Remove the deleted rows physically ("vacuum": a long-lived library gets the space of its deletions back).  Survivors keep
 * their relative order; the survivor at old local row o moves to local row o - (number of deleted rows below o) and its id
 * becomes base + that.  new_ids (may be NULL): [rows before the call], new_ids[o] = the new id, MI_KNN_NO_ID for a deleted
 * row; cap = its length (cap < rows before: MI_ERR_INVALID, nothing changes).  *removed (may be NULL) = rows reclaimed.
 * With L = rows - deleted, afterwards: mi_knn_size = L, mi_knn_deleted is empty, mi_knn_get_rows(0, L) returns the survivors'
 * fp32 rows in their old order bit for bit, and each survivor's group, tags and stamp have travelled with it (mi_knn_groups_info's
 * group count stays the high-water mark it was).  The freed rows [L, old rows) hold the defaults (no group, tags 0, stamp 0)
 * and the next append reuses them.  Every call of the library returns on the compacted table what it returns on a fresh
 * table of the same dim, base and options that was given the survivors by mi_knn_append and their columns by
 * mi_knn_set_groups / mi_knn_set_attrs — in particular every search runs the code of a table without deletions again, and
 * mi_knn_save writes the MIKNNv01 file of L rows.  What does NOT survive: every id the caller holds (label arrays, the
 * cursors of mi_knn_search_page / mi_knn_search_ordered): map them through new_ids.  The "prefilter" mirrors of the moved
 * rows are rebuilt by the next search.
 * The rows move in place on the device, in ascending chunks of option "compact_chunk_rows" destination rows (0 = default:
 * what 64 MiB hold, 21 845 rows at dim 768), each either gathered straight into place or through a staging buffer of one
 * chunk; rows below the first deleted row are not touched.  Extra device memory while the call runs: that buffer, 4 bytes
 * per deleted row and 12 per moved row; never a second table.  The allocation itself does not shrink.  The call waits for
 * everything enqueued on the table (as a reallocation does), checks every argument and allocates every buffer before the
 * first row moves, and has finished when it returns.  A table without deletions: *removed = 0, new_ids = the ids as they
 * are, nothing is launched.  Every row deleted: the table becomes empty.  A shard borrowed from a sharded table:
 * MI_ERR_UNSUPPORTED (its ids are not its own to renumber: mi_knn_sharded_compact_into).  A null handle: MI_ERR_INVALID. */
int mi_knn_compact(mi_knn* t, uint64_t* new_ids, uint64_t cap, uint64_t* removed);
/* {rows removed, rows moved, chunks gathered in place, chunks staged} of the last mi_knn_compact on this handle */
int mi_knn_compact_stats(mi_knn* t, uint64_t out[4]);

/* Replaces `SELECT id, image_path, vector::distance::knn() FROM image WHERE
 * embedding <|K|> $reference` (server/src/search.rs:70-86; K = 1000 there).
 * For each of nq queries (q: [nq,dim] host f32): the k rows of this shard with the
 * smallest cosine distance 1 - q.x/(|q||x|), sorted by (distance asc, id asc);
 * NaN distances (zero-norm row or query) sort last.  idx: [nq,k] uint64,
 * dist: [nq,k] f32.  Fewer than k rows: the tail is MI_KNN_NO_ID / +inf.
 * Each query is one pass over the table (the reference serves one query per
 * request, server/src/search.rs:20-102). */
int mi_knn_search(mi_knn* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist);
/* Same, queries and results on the device, asynchronous on `stream`.
 * d_idx [nq,k] uint64 and d_dist [nq,k] f32 are what each rank feeds to the
 * all-gather when the table is sharded. */
int mi_knn_search_device(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx,
                         float* d_dist, void* stream);
/* Throughput variant: ONE pass over the table serves all nq queries (nq <= 16).  With "prefilter" = 2 and dim 768 the whole
 * group of up to 16 queries shares one pass over the byte mirror on the matrix pipe (the queries cut into three signed 7-bit
 * digits, exact int8 MFMA dot products; option "batch_stage1" = 0: the vector-ALU form, groups of 8 / 4 / 2) and ONE launch
 * of every later kernel of the two-stage search; otherwise passes of 8 / 4 / 2 queries over the fp32 rows (k <= 64).
 * Results identical to nq calls of mi_knn_search_device with nq = 1: same ids, same distance bits.
 * Device memory: a group keeps per-query copies of the two-stage workspaces, allocated by the first group of that size
 * and kept — per query 4 bytes per table row (stage-1 keys: 640 MB for 16 queries over 10 M rows, 6.4 GB over 100 M),
 * 32 MB of candidate rows + keys, and the select / sort buffers; a failed allocation fails that search with MI_ERR_OOM. */
int mi_knn_search_batched_device(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx,
                                 float* d_dist, void* stream);
/* Filtered search: the k nearest among the rows the ids name (`WHERE embedding <|K|> $reference AND id IN $ids` as a
 * pre-filter — exactly k hits whenever k rows qualify).  The result is bit-identical to mi_knn_search over a table that
 * holds only the filter's live rows under their own ids: ids, order (distance ascending, then id, NaN last) and distance
 * bits, MI_KNN_NO_ID / +inf behind the last hit.  ids: any order, duplicates allowed, n_ids may be 0 (then every result is
 * MI_KNN_NO_ID); every id must be a row of the table (MI_ERR_INVALID otherwise, and nothing runs); ids of deleted rows
 * are allowed and left out.  k <= 4096 (MI_ERR_UNSUPPORTED above).  Runs on the handle's stream behind every write and
 * search enqueued before it; reads only the filter's fp32 rows (n x dim x 4 bytes; the "prefilter" mirrors are not used). */
int mi_knn_search_filtered(mi_knn* t, const float* q, uint32_t nq, uint32_t k, const uint64_t* ids, uint64_t n_ids,
                           uint64_t* idx, float* dist);
/* Near-duplicates ("which of my images are there twice?"): a threshold self-join on the matrix pipe.  Stage 1 multiplies a
 * bf16 mirror of the rows with itself in tiles (the table's own mirror when "prefilter" = 1 keeps one, else one built for
 * the call and freed before it returns: + 50 % of the rows' bytes meanwhile, MI_ERR_OOM when that does not fit; dim % 128
 * == 0, MI_ERR_UNSUPPORTED otherwise); every pair a rigorous data-independent bound cannot exclude is re-evaluated from the
 * fp32 rows.  Memory is bounded (option "join_cap": candidate pairs per strip of stage 1, default 2^22, >= 2^14; a strip
 * that finds more is redone in smaller pieces, nothing is dropped).  Runs on the handle's stream behind every write and
 * search enqueued before it, and waits for its results.
 * every pair of live rows (a < b) with cosine distance <= max_dist, ascending by (a, b); dist = what mi_knn_search(q = row a)
 * reports for row b, bit for bit.  first_new: only pairs with b >= first_new (0 = all pairs): "what did the rows I have just
 * appended duplicate?" without redoing the old-against-old part.  a, b, dist: [cap] (may be NULL when cap = 0);
 * *count = number of pairs.  More than cap pairs qualify: MI_ERR_UNSUPPORTED ("lower max_dist or raise cap"), *count =
 * cap + 1, the arrays' contents unspecified; the call stops early.  max_dist NaN or < 0: MI_ERR_INVALID.
 * first_new is not an id of the table and is not one past its last id (the end: no pairs): MI_ERR_INVALID. */
int mi_knn_near_pairs(mi_knn* t, float max_dist, uint64_t first_new, uint64_t* a, uint64_t* b, float* dist,
                      uint64_t cap, uint64_t* count);
/* of the last mi_knn_near_pairs on this handle: out = {candidate pairs stage 1 passed to stage 2, pairs accepted,
 * strips run (re-runs after an overflow included), tiles visited} */
int mi_knn_near_pairs_stats(mi_knn* t, uint64_t out[4]);
/* Bursts ("which shots were taken within a few seconds of each other and look alike?"): mi_knn_near_pairs restricted to the
 * pairs whose capture times lie within a window.  The stamp test: rows a and b pass when |stamp_a - stamp_b| <= window, stamp
 * being the column mi_knn_set_attrs sets.  The difference is taken exactly — max - min in uint64 arithmetic, right for every
 * pair of int64 values: INT64_MIN against INT64_MAX is 2^64 - 1 — so window == UINT64_MAX restricts nothing and window == 0
 * means equal stamps only.  A table that never set attributes behaves as if every stamp were 0: every pair passes.
 * W_win = the pairs of mi_knn_near_pairs(t, max_dist, first_new) whose two rows pass the stamp test; ids, order (ascending by
 * (a, b)) and distance bits are those of W.  The cap protocol, the errors, dim, mirror, "join_cap" and the stream ordering
 * are mi_knn_near_pairs'.  The test runs inside stage 1, so pairs that look alike but lie apart in time never reach the
 * candidate buffer, and tiles whose two blocks' stamp ranges lie further apart than the window are not computed at all: on a
 * table appended in capture order only a band along the diagonal is. */
int mi_knn_near_pairs_window(mi_knn* t, float max_dist, uint64_t window, uint64_t first_new, uint64_t* a, uint64_t* b,
                             float* dist, uint64_t cap, uint64_t* count);
/* The join of TWO tables ("which pictures on this card, or in that other library, do I already have?" — the reference has one
 * table in one server, server/src/main.rs, and could only answer this by inserting the other rows first): every pair of a
 * live row of `t` and a live row of `other` with cosine distance <= max_dist.  a[i]: an id of t; b[i]: an id of other (the two
 * id spaces are unrelated and may overlap); dist[i] = what mi_knn_search on `other` with q = row a[i] of t reports for row
 * b[i], bit for bit: the row of t is the query.  Ascending by (a, b).  Neither table is changed.  Stage 1 is the self-join's
 * bf16 tile with a row operand (t, where the work runs) and a column operand (other); the same bound decides what stage 2
 * re-evaluates from the fp32 rows (dim as mi_knn_near_pairs requires, MI_ERR_UNSUPPORTED otherwise).  `other` on t's device
 * is read where it lies; on another device (or with option "join_stage" = 1 on t) its rows pass through a staged copy on t's
 * device.  Either way `other` is walked in column chunks of at most 256 MiB of fp32 rows (option "join_stage_rows": rows
 * per chunk; same answers whatever the value): what the staged copy holds at a time.  Memory beyond that is mi_knn_near_pairs' (t's "join_cap").  Takes both handles' locks; runs on t's stream behind
 * every write and search enqueued on either table before it, and waits for its results.
 * a, b, dist: [cap] (may be NULL when cap = 0); *count = number of pairs.  More than cap pairs qualify: MI_ERR_UNSUPPORTED,
 * *count = cap + 1, the call stops early (the cap protocol of mi_knn_near_pairs).  t == other, a null handle, dims that
 * differ, max_dist NaN or < 0: MI_ERR_INVALID.  An empty table on either side: 0 pairs. */
int mi_knn_near_pairs_between(mi_knn* t, mi_knn* other, float max_dist, uint64_t* a, uint64_t* b, float* dist, uint64_t cap,
                              uint64_t* count);
/* of the last mi_knn_near_pairs_between with t as its first table: out = {candidate pairs stage 1 passed to stage 2, pairs
 * accepted, stage-1 launches (re-runs after an overflow included), tiles computed} */
int mi_knn_near_pairs_between_stats(mi_knn* t, uint64_t out[4]);
/* Density ("how crowded is it around every image?") and DBSCAN ("which themes are really there, however many, and which
 * pictures belong to none?") on the join's tiles; the pairs never leave the device, so a dense theme costs no pair list.
 * Let W be the pairs (a < b, d) that mi_knn_near_pairs(t, max_dist, first_new = 0) reports: live rows only, d the bits
 * mi_knn_search reports with q = row a for row b, a NaN never within.  Arrays are indexed by local row (rows = mi_knn_size,
 * deleted rows counted), as mi_knn_assign's are; ids go through the table's base / block-cyclic map.
 *   deg[r]     the number of pairs of W that contain r (the row itself is not counted); 0 for a deleted row.
 *   core       r is live and deg[r] + 1 >= min_pts (scikit-learn's min_samples: the point itself counts).
 *   clusters   the connected components of the graph on the core rows whose edges are the pairs of W with both ends core; a
 *              cluster is named by the id of its smallest core row.
 *   border     a live non-core row with a core neighbour in W: it belongs to the cluster of the core neighbour c that minimises
 *              (the search's 32-bit key of the pair's d — so -0 comes before +0 —, row of c); d is the pair's distance as W holds
 *              it whichever end the border row is.  This fixes what classic DBSCAN leaves to the visiting order.
 *   noise      every other live row.  A deleted row is nothing at all.
 * mi_knn_density: counts [rows] = deg.
 * mi_knn_dbscan: cluster [rows] = the id of the row's cluster, MI_KNN_NO_ID for noise and deleted rows; via [rows] (may be
 * NULL) = a core row: its own id, a border row: the core it joined through, else MI_KNN_NO_ID; via_dist [rows] (may be NULL) =
 * core: +0.0f, border: that pair's distance bits, else +inf; counts [rows] (may be NULL) = deg; summary = {clusters, core rows,
 * border rows, noise rows}.  The result does not depend on arrival order, grid or strip size.
 * max_dist NaN or < 0, min_pts == 0, a null handle or a null required pointer: MI_ERR_INVALID.  dim, mirror, "join_cap" and
 * stream ordering: as mi_knn_near_pairs (two tile passes for mi_knn_dbscan, one for mi_knn_density; 16 bytes of device memory
 * per row beside the join's buffers, plus the result arrays, freed before the call returns).  An error writes nothing.  An
 * empty table is valid (no clusters); with min_pts == 1 every live row is a core, a lone one a cluster of one.  Should the
 * bounded retry loops of the device's disjoint-set forest ever run out (they never should), the call fails with MI_ERR_HIP. */
int mi_knn_density(mi_knn* t, float max_dist, uint32_t* counts);
int mi_knn_dbscan(mi_knn* t, float max_dist, uint32_t min_pts, uint64_t* cluster, uint64_t* via, float* via_dist,
                  uint32_t* counts, uint64_t summary[4]);
/* of the last mi_knn_density / mi_knn_dbscan / mi_knn_density_levels / mi_knn_dbscan_levels on this handle: out = {candidate
 * pairs pass 1, pairs within, tiles pass 1, candidate pairs pass 2, tiles visited pass 2, tiles skipped pass 2 (both blocks must
 * hold a row with a neighbour and one a core: exact), unions that merged two trees, stage-1 launches of both passes (re-runs
 * after an overflow included)}.  The tile counts are those of the launches whose candidates were consumed: visited + skipped =
 * the triangle's tiles.  After a *_levels call: pairs within = those of the top level, unions merged = summed over the levels. */
int mi_knn_dbscan_stats(mi_knn* t, uint64_t out[8]);
/* Events ("beach 2019" and "beach 2023" as two clusters): density and DBSCAN whose neighbourhood is "within max_dist AND
 * within a time window" — ST-DBSCAN (Birant & Kut, 2007).  Exactly the contract of mi_knn_density / mi_knn_dbscan above with
 * W_win (mi_knn_near_pairs_window at first_new = 0) in place of W: deg, core, clusters named by their smallest core row, border
 * by the minimum of (distance key, core row) over the core neighbours in W_win, noise, a deleted row nothing at all.  The
 * arguments, errors (an error writes nothing), dim, mirror, "join_cap" and stream ordering are the unwindowed calls'. */
int mi_knn_density_window(mi_knn* t, float max_dist, uint64_t window, uint32_t* counts);
int mi_knn_dbscan_window(mi_knn* t, float max_dist, uint64_t window, uint32_t min_pts, uint64_t* cluster, uint64_t* via,
                         float* via_dist, uint32_t* counts, uint64_t summary[4]);
/* of the last mi_knn_near_pairs_window / mi_knn_density_window / mi_knn_dbscan_window (mi_index_bursts / mi_index_events
 * included) on this handle: out = {candidate pairs pass 1, pairs within, tiles computed pass 1, tiles skipped by the blocks' stamp
 * ranges pass 1, candidate pairs pass 2, tiles computed pass 2, tiles skipped pass 2 (by the stamp ranges or by the activity
 * bytes of mi_knn_dbscan_stats), stage-1 launches (re-runs after an overflow included)}.  The pass-2 words are 0 after
 * mi_knn_near_pairs_window and mi_knn_density_window.  Per pass, computed + skipped = the tiles of the triangle the pass covers
 * (the launches whose candidates were consumed are counted).  The windowed calls keep these words to themselves: they leave
 * mi_knn_near_pairs_stats and mi_knn_dbscan_stats as they were, and the unwindowed calls leave these. */
int mi_knn_window_stats(mi_knn* t, uint64_t out[8]);
/* Themes at several distances in one pass ("tighter / looser themes" on a slider, a theme that contains bursts): what
 * n_levels calls of mi_knn_density / mi_knn_dbscan with max_dists[0] < max_dists[1] < ... return on the same table, from the
 * two tile passes ONE such call runs.  Slice l of every output array ([n_levels][rows], level-major, by local row) is exactly
 * what mi_knn_density(t, max_dists[l], ...) / mi_knn_dbscan(t, max_dists[l], min_pts, ...) writes: ids, distance bits, counts
 * and summary ([n_levels][4]), under the definitions above (W, deg, core, clusters named by their smallest core row, border by
 * the minimum of (dist key, core row), noise, a deleted row nothing at all).  n_levels == 1 is mi_knn_dbscan's result.  For one
 * min_pts the core sets and the core-core edges only grow with the distance, so the clusters of level l nest inside those of
 * level l + 1 through their core rows (mi_dbscan_levels_tree).
 * max_dists: strictly ascending, every entry a number >= 0; 1 <= n_levels <= MI_KNN_LEVELS_MAX.  A null handle, max_dists or
 * required pointer (counts of mi_knn_density_levels; cluster and summary of mi_knn_dbscan_levels), n_levels 0 or above the
 * maximum, a NaN, a negative entry, two neighbouring entries that do not ascend strictly (equal ones included), min_pts == 0:
 * MI_ERR_INVALID.  dim, mirror, "join_cap", stream ordering and the step cap's MI_ERR_HIP: as mi_knn_dbscan; there is no new
 * option.  Device memory: n_levels * 16 + 1 bytes per row beside the join's buffers, plus the result arrays, all freed before
 * the call returns.  An error writes nothing.  An empty table is valid. */
#define MI_KNN_LEVELS_MAX 8
int mi_knn_density_levels(mi_knn* t, const float* max_dists, uint32_t n_levels, uint32_t* counts);
int mi_knn_dbscan_levels(mi_knn* t, const float* max_dists, uint32_t n_levels, uint32_t min_pts, uint64_t* cluster, uint64_t* via,
                         float* via_dist, uint32_t* counts, uint64_t* summary);
/* The tree between the levels of a mi_knn_dbscan_levels result (host only, no device): the edges (l, cluster id at level l,
 * cluster id at level l + 1) for l < n_levels - 1, ascending by (l, child), into level / child / parent [cap].  cluster and
 * counts: the call's arrays, [n_levels][rows].  Row r is a core at level l iff cluster[l][r] != MI_KNN_NO_ID and
 * counts[l][r] + 1 >= min_pts; the parent of a level-l cluster is the level-(l + 1) cluster of its core rows.  All cores of one
 * cluster must agree, and a core of level l must lie in a cluster at level l + 1: otherwise the input is no result of the call
 * above and the answer is MI_ERR_INVALID.  *n_edges is the full count even when cap is smaller (the first cap edges are
 * written), as for the index calls.  The tree is over clusters through their CORE rows: a border row of a level-l cluster may
 * sit in a level-(l + 1) cluster that is not the parent of its level-l cluster (a row that becomes a core only at the upper
 * level may be nearer to it than its lower-level core).  Null cluster, counts or n_edges, an output array null with cap > 0,
 * n_levels 0 or above the maximum, min_pts == 0: MI_ERR_INVALID; rows == 0 is valid (no edges).  An error writes nothing. */
int mi_dbscan_levels_tree(const uint64_t* cluster, const uint32_t* counts, uint64_t rows, uint32_t n_levels, uint32_t min_pts,
                          uint32_t* level, uint64_t* child, uint64_t* parent, uint64_t cap, uint64_t* n_edges);
/* Label every row by its nearest of C vectors ("tag my library" with C text embeddings; the inner step of k-means): the
 * search turned round.  For every row r of the table (rows = mi_knn_size, deleted rows counted):
 *   r live     labels[r], dist[r] = the first entry of mi_knn_search(T_v, q = row r, k = 1) where T_v holds exactly the C
 *              vectors under ids 0 .. C - 1: the same id and the same distance bits under the search's order (distance
 *              ascending, then id, NaN last).  A tie goes to the lower label; a row whose every distance is NaN (zero norm,
 *              a non-finite element) gets label 0 and NaN.
 *   r deleted  MI_KNN_NO_LABEL, +inf.
 * vectors: [C, dim] host f32, 1 <= C <= 65536 (MI_ERR_UNSUPPORTED above, MI_ERR_INVALID for 0 or a null pointer); labels:
 * [rows]; dist: [rows] or NULL.  dim as mi_knn_near_pairs requires (MI_ERR_UNSUPPORTED otherwise); an empty table succeeds
 * and writes nothing.  Stage 1 multiplies the rows' bf16 mirror (the table's own when "prefilter" = 1 keeps one, else one
 * built for the call and freed) with the vectors' on the matrix pipe and keeps, per row, every vector the join's bound
 * cannot separate from the best one; stage 2 re-evaluates those from the fp32 rows.  Memory is bounded by "join_cap" as for
 * the join (a strip of rows that finds more candidates is redone in smaller pieces, nothing is dropped).  Runs on the
 * handle's stream behind every write and search enqueued before it, and waits for its results. */
#define MI_KNN_NO_LABEL UINT32_MAX
int mi_knn_assign(mi_knn* t, const float* vectors, uint32_t C, uint32_t* labels, float* dist);
/* of the last mi_knn_assign (or the last assign inside mi_knn_kmeans) on this handle: out = {candidates stage 1 handed to
 * stage 2, live rows labelled, stage-1 launches (re-runs after an overflow included), tiles visited} */
int mi_knn_assign_stats(mi_knn* t, uint64_t out[4]);
/* Up to m labels per row, and only those within a distance ("beach", "sunset" and "dog" at once; no tag for a photo that
 * matches nothing; with a large m, the range search "every (row, vector) pair within max_dist").  For every row r of the
 * table (rows = mi_knn_size):
 *   r live     entries j = 0 .. m-1 of  mi_knn_search(T_v, q = row r, k = m)  over a table T_v that holds exactly the C
 *              vectors under ids 0 .. C-1, AFTER removing every entry whose distance is NaN or > max_dist: same ids, same
 *              distance bits, the search's order (distance ascending, then label).  Behind the last hit: MI_KNN_NO_LABEL / +inf.
 *   r deleted  m x (MI_KNN_NO_LABEL, +inf).
 * A row whose every distance is NaN gets only padding (unlike mi_knn_assign's "label 0, NaN": a NaN is never a tag).
 * labels: [rows][m] uint32, dist: [rows][m] f32 or NULL.  1 <= m <= 16, 1 <= C <= 65536 (MI_ERR_UNSUPPORTED above, MI_ERR_INVALID
 * for 0 / NULL); m > C is allowed (padding).  max_dist: +INFINITY = no threshold; NaN or < 0: MI_ERR_INVALID.  dim, mirror,
 * "join_cap", stream ordering and the empty table: as mi_knn_assign.  Stage 1 keeps, per row, every vector the join's bound
 * cannot separate from the m-th best one or from max_dist; stage 2 re-evaluates those from the fp32 rows and keeps the m
 * smallest per row in an order that does not depend on their arrival.  The rows are walked in strips whose results are
 * copied out one by one: the device workspace does not grow with rows x m. */
int mi_knn_assign_multi(mi_knn* t, const float* vectors, uint32_t C, uint32_t m, float max_dist, uint32_t* labels, float* dist);
/* of the last mi_knn_assign_multi on this handle: out = {candidates stage 1 handed to stage 2, (row, label) hits written,
 * stage-1 launches (re-runs after an overflow included), tiles visited} */
int mi_knn_assign_multi_stats(mi_knn* t, uint64_t out[4]);
/* Many queries at once ("the best k images for each of my C tags").  For each of nq queries (q: [nq][dim] host f32) the
 * entries of mi_knn_search(t, query, k) AFTER removing every entry whose distance is NaN: same ids, same distance bits, same
 * order (distance ascending, then id); MI_KNN_NO_ID / +inf behind the last hit.  idx: [nq][k] uint64, dist: [nq][k] f32.
 * 1 <= k <= 16 (MI_ERR_UNSUPPORTED above), nq >= 1 of any size (walked in strips: the device workspace does not grow with
 * nq); 0 / NULL: MI_ERR_INVALID.  dim, mirror, "join_cap" and stream ordering: as mi_knn_assign_multi.  Deleted rows are
 * never returned.  Empty table: all padding, MI_OK.  Stage 1 is a bf16 MFMA tile product of the queries with the table's
 * mirror, the table's columns spread over the machine (option "many_segments": 0 = chosen, v >= 1 = exactly min(v, column
 * tiles) segments; "many_sample": the threshold pass visits every v-th column tile, 0 = chosen); stage 2 re-evaluates what
 * the join's bound cannot exclude from the fp32 rows.  Same answers whatever the options. */
int mi_knn_search_many(mi_knn* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist);
/* out = {candidates stage 1 handed to stage 2, (query, row) hits written, stage-1 launches (threshold and emit passes and
 * re-runs after an overflow all counted), tiles visited} of the last search_many / neighbors on this handle */
int mi_knn_search_many_stats(mi_knn* t, uint64_t out[4]);
/* The kNN graph ("more like this" for every image), a slice at a time: for the n rows with ids first .. first + n - 1 (must
 * be rows of the table, else MI_ERR_INVALID and nothing runs; n may be 0) the k nearest OTHER live rows:
 * mi_knn_search_many(q = the row, k + 1) with the entry whose id is the row's own removed, or, where that entry is absent
 * (a row whose every distance is NaN; k + 1 or more exact copies of the row at lower ids), the last entry removed.
 * Distances are what mi_knn_search(q = row a) reports for row b, bit for bit (the contract of mi_knn_near_pairs).  A deleted
 * row gets k x (MI_KNN_NO_ID, +inf).  1 <= k <= 15.  idx: [n][k], dist: [n][k].  The queries are read where they lie: no
 * copy of the rows, their mirror rows are the table's.  Not offered on a shard borrowed from a sharded table (its ids are
 * not contiguous: MI_ERR_UNSUPPORTED). */
int mi_knn_neighbors(mi_knn* t, uint64_t first, uint64_t n, uint32_t k, uint64_t* idx, float* dist);
/* The many-query search narrowed ("the best k pictures for each of my tags among my favourites, 2019-2021"; a picture flagged
 * hidden under no tag): mi_knn_search_many among the rows that qualify under w (mi_knn_where, declared with mi_knn_search_where
 * below).  For each query the entries of mi_knn_search_where(t, query, 1, k, w) AFTER removing every entry whose distance is
 * NaN: same ids, same distance bits, same order; MI_KNN_NO_ID / +inf behind the last hit.  *matched (may be NULL) = the
 * qualifying rows (mi_knn_count_where).  w == NULL: exactly mi_knn_search_many (same launches, no mask built), *matched = the
 * live rows.  k, nq, dim, mirror, "join_cap", "many_segments", "many_sample", stream ordering and the empty table: as
 * mi_knn_search_many; the predicate's errors: as mi_knn_search_where; an argument error writes nothing.  A predicate nothing can
 * meet gives all padding without a tile launch.
 * One kernel evaluates the predicate for every row into a call-private bitmap (bit set = the row stays out: deleted or not
 * qualifying), and stage 1 takes that bitmap in place of the deletion bitmap: a masked column has weight 0, it is never
 * emitted and never enters a threshold slot, so the thresholds are those of a table that holds the qualifying rows only.
 * Stage 1 still multiplies every column tile: a narrow predicate saves stage 2's work, not stage 1's.  Known cost: the
 * thresholds come from m residue slots (row index mod m); where the qualifying rows fall into few residues a slot stays
 * empty and every qualifying row is emitted for every query (correct, slower).  When qualifying rows x a strip's queries fit
 * the candidate buffer the threshold pass is skipped and everything is emitted at once.
 * mi_knn_search_many_stats reports these calls too. */
struct mi_knn_where;
int mi_knn_search_many_where(mi_knn* t, const float* q, uint32_t nq, uint32_t k, const struct mi_knn_where* w, uint64_t* idx,
                             float* dist, uint64_t* matched /* may be NULL */);
/* mi_knn_neighbors with the candidates narrowed: the queries are the rows first .. first + n - 1 whether or not they qualify
 * themselves (a deleted row gets padding), the candidates the rows that qualify under w (NULL: every live row, exactly
 * mi_knn_neighbors).  Per row: mi_knn_search_many_where(q = the row, k + 1, w) with the entry whose id is the row's own removed,
 * or the last entry removed where that entry is absent (now also: the row does not qualify).  1 <= k <= 15; range errors and
 * the refusal on a borrowed shard as mi_knn_neighbors. */
int mi_knn_neighbors_where(mi_knn* t, uint64_t first, uint64_t n, uint32_t k, const struct mi_knn_where* w, uint64_t* idx,
                           float* dist);
/* "I sorted 300 pictures into albums by hand, where do the other 40 000 go?" — a k-nearest-neighbour vote that carries the
 * group column (mi_knn_set_groups) forward.  All arrays are [rows] by local row (rows = mi_knn_size, deleted rows counted).
 *   asker  a live row whose group is ask_group (MI_KNN_NO_GROUP: the rows without a group; a table whose group column was
 *          never set: every live row).
 *   voter  a live row whose group is neither MI_KNN_NO_GROUP nor ask_group and that, with voters != NULL, qualifies under it
 *          (hidden pictures do not vote).  No row is both.
 *   L(r)   for an asker r: the voters ordered by (the distance key mi_knn_search(q = row r) reports for them, id) ascending,
 *          without the entries whose distance is NaN and without those beyond the window dist_to_u32(d) <=
 *          dist_to_u32(max_dist) (mi_knn_search_page's inclusive window: +INFINITY = no bound, NaN or < 0: MI_ERR_INVALID);
 *          the first k of what remains.  Distances carry the search's bits.
 *   tally  n_g = the entries of L(r) whose group is g; the winner is the g with the largest n_g, among equal counts the one
 *          whose first entry stands earliest in L(r) (the nearest).
 * group[r] = the winner (MI_KNN_NO_GROUP: L(r) is empty or r is no asker), votes[r] = n_winner, heard[r] = |L(r)|, dist[r] = the
 * distance of the winner's first entry (+inf: none).  votes, heard, dist and totals may be NULL.  totals = {askers, askers
 * with a proposal, voters, askers with votes == heard > 0}.
 * 1 <= k <= 16 (0: MI_ERR_INVALID, above: MI_ERR_UNSUPPORTED); dim as mi_knn_near_pairs; ask_group >= MI_KNN_GROUPS_MAX and not
 * MI_KNN_NO_GROUP: MI_ERR_INVALID; a shard borrowed from a sharded table: MI_ERR_UNSUPPORTED (it sees only its own voters).
 * An empty table, no asker or no voter: padding, the counts in totals, MI_OK, no tile launch.  An argument error writes
 * nothing.  The group column is never written: applying the proposals is the caller's mi_knn_set_groups.  It is the
 * many-query search with the table's rows as queries, a column mask (not a voter) and a query mask (not an asker), and a
 * tally behind stage 2.  Runs on the handle's stream behind every write enqueued before it and waits for its results. */
int mi_knn_propose_groups(mi_knn* t, uint32_t k, float max_dist, uint32_t ask_group, const struct mi_knn_where* voters /* may be NULL */,
                          uint32_t* group, uint32_t* votes, uint32_t* heard, float* dist, uint64_t totals[4]);
/* out = {candidates stage 1 handed to stage 2, tile launches, tiles visited, strips} of the last mi_knn_propose_groups */
int mi_knn_propose_groups_stats(mi_knn* t, uint64_t out[4]);
/* Spherical k-means (Lloyd's iterations) over the live rows, mi_knn_assign as its inner step:
 *   it = 0
 *   loop: labels = assign(centroids); changed = rows whose label differs from the previous assign (first: the live rows)
 *         stop when (it > 0 and changed == 0) or it == max_iters
 *         every c: S = sum of x / |x| over the live rows labelled c whose dist is not NaN, n_c their number;
 *                  n_c > 0: centroid[c] = S / n_c, else unchanged;  it += 1
 * centroids: [C, dim] host, in = initial, out = final.  labels / dist ([rows], either may be NULL): exactly what
 * mi_knn_assign(t, returned centroids) reports.  *iters_run = updates done, *changed_last = as counted by the last assign,
 * *objective = sum of dist over the live rows with a non-NaN distance, in double, in row order (any of the three may be
 * NULL).  Deterministic: the sums run in an order fixed by the row ids (rows bucketed by label, fixed segments, segments in
 * order), so the same table, centroids and max_iters give the same bits.  max_iters = 0: one assign, centroids untouched.
 * Rows, labels and sums stay on the device between iterations.  Arguments and errors as mi_knn_assign.
 * Option "kmeans_fixed_sum" (mi_knn_set_option; 0 = default, 1 = on, anything else MI_ERR_INVALID) replaces the float sums of
 * this update, and of mi_knn_summarize's centroids, by exact integer sums.  For a member row r and component j:
 *   v = x[r][j] * inv[r]                     the fp32 product the float sum adds, inv[r] = 1 / |x[r]|
 *   q = (|v| < 2) ? rint(v * 2^30) : 0       to nearest, ties to even; the scaling is exact; |q| < 2^31 (a NaN or inf v,
 *                                            which no member row produces, fails the comparison)
 *   S[c][j] = sum of q as int64              fewer than 2^32 members: |S| < 2^63
 *   centroid[c][j] = (float)((double)S[c][j] * 2^-30 / (double)n_c), an empty cluster keeps its centroid
 * Membership, the stop rule and everything else are unchanged.  The result no longer depends on any summation order, which
 * is what mi_knn_sharded_kmeans rests on; a component's error is half a unit of 2^-30 per member before the division and
 * does not grow with n_c.  At 0 nothing changes: the launches and bits of the float path. */
int mi_knn_kmeans(mi_knn* t, float* centroids, uint32_t C, uint32_t max_iters, uint32_t* labels, float* dist,
                  uint32_t* iters_run, uint64_t* changed_last, double* objective);
/* k-means++ seeding on the device ("what mi_knn_kmeans should start from"): C rows, each drawn with probability proportional
 * to its cosine distance from the nearest row drawn so far.  For unit vectors the squared chord distance is 2 (1 - cos), so
 * the k-means++ weight of spherical k-means is the cosine distance itself, not its square.  Exact and deterministic: every
 * quantity the choice depends on is an integer or a distance with the search's bits.
 *   candidates  among == NULL: every live row, ascending by id.  Otherwise the n_among ids given, sorted and made unique,
 *               deleted rows left out (any order and duplicates allowed, as for mi_knn_search_filtered); an id that is not a
 *               row of the table: MI_ERR_INVALID, nothing runs.  S = their number, position p = 0 .. S-1 in that order.
 *   usable      a candidate for which mi_knn_search(q = the row) reports a non-NaN distance for the row itself (finite,
 *               non-zero norm).
 *   z_0, z_1 .. the outputs of splitmix64 started at `seed`: state += 0x9E3779B97F4A7C15; z = state;
 *               z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; output z ^ z >> 31.
 *   pick j      over weights w_p (uint32), total = sum of w_p, exact in uint64.  total > 0: T = floor(z_j * total / 2^64) (a
 *               64 x 64 -> high 64 multiply), the pick is the smallest p whose inclusive prefix sum exceeds T.  total == 0:
 *               the smallest p not picked before (a "fallback pick").  z_j is consumed either way.
 *   weights     for pick 0: w_p = 1 if p is usable, else 0.  After pick j with centre row c: d_p = the distance bits
 *               mi_knn_search(q = row c) reports for row p; D_p = d_p if d_p is not NaN and (D_p is unset or d_p < D_p), else
 *               unchanged; w_p = 0 if p was picked, is unusable or D_p is unset, else
 *               w_p = (uint32) floor(min(max(D_p, 0), 2) * 2^30) (an exact power-of-two scaling in fp32, then truncation).
 * rows: [C] = the id of pick j, in pick order.  centroids: [C, dim] or NULL = those rows' fp32 values, bit for bit (what
 * mi_knn_kmeans takes as its initial centroids).  potential (or NULL) = sum of w_p * 2^-30 in double after one more weight
 * update with the last pick: the k-means++ potential of the seeds.
 * C == 0, a null `rows` or C > S: MI_ERR_INVALID.  C > 65536: MI_ERR_UNSUPPORTED.  A shard borrowed from a sharded table:
 * MI_ERR_UNSUPPORTED, as for mi_knn_neighbors.  dim as mi_knn_near_pairs requires; the call reads the fp32 rows only: the
 * "prefilter" mirrors are not used and the result does not depend on that option.  One fp32 pass over the candidate rows
 * per seed, all launches enqueued without a host round trip.  Runs on the handle's stream behind every write and search
 * enqueued before it, and waits for its results. */
int mi_knn_kmeans_seed(mi_knn* t, uint32_t C, uint64_t seed, const uint64_t* among, uint64_t n_among, uint64_t* rows,
                       float* centroids, double* potential);
/* of the last mi_knn_kmeans_seed on this handle: out = {candidates S, passes over the candidates (the usable pass and one per
 * seed: C + 1), fallback picks, 0} */
int mi_knn_kmeans_seed_stats(mi_knn* t, uint64_t out[4]);
/* What a group looks like once it exists ("your 40 themes", "your folders"): per group its centroid, its cover picture, the
 * picture that does not belong and how tight it is — for ANY grouping: mi_knn_kmeans / mi_knn_assign labels, mi_knn_dbscan themes
 * (dense labels), mi_pairs_to_groups components, the index's directories or a caller's own column.  labels: [rows] by local row
 * (rows = mi_knn_size, deleted rows counted), as mi_knn_assign's arrays are, or NULL: the table's group column
 * (mi_knn_set_groups), read where it lies.  Ids go through the table's base / block-cyclic map, as mi_knn_dbscan's do.
 *   member of c   a live row with label c < C that is usable: mi_knn_search(q = the row) reports a non-NaN distance for the row
 *                 itself (mi_knn_kmeans_seed's "usable").  A label >= C (MI_KNN_NO_LABEL, MI_KNN_NO_GROUP) belongs to nothing.
 *   count[c]      the number of members.
 *   centroid[c]   S / count[c], S = the sum of x / |x| over the members in exactly the order of mi_knn_kmeans' update (members
 *                 ascending by row, fixed segments, segments in order): bit-identical to that update.  All zeros if empty.
 *   dist[r]       a member: the distance mi_knn_search over a table holding the C centroids under ids 0 .. C-1 reports with
 *                 q = row r for entry label[r], to the bit (mi_knn_assign's arithmetic); NaN for an unusable live row with a
 *                 label < C; +inf for every other row.
 *   cover[c]      the member with the smallest (32-bit distance key, id) — NaN sorts last, -0 before +0, among equal keys the
 *                 lowest id; cover_dist[c] its distance.  Empty group: MI_KNN_NO_ID, +inf.  For unit vectors
 *                 sum_j (1 - x_i . x_j) = n - x_i . S, so the member nearest to the centroid is the group's exact medoid (the
 *                 smallest total cosine distance to the other members) in real arithmetic.
 *   odd[c]        the member with the largest key among those whose distance is not NaN, the lowest id among equal keys;
 *                 odd_dist[c] its distance.  None: MI_KNN_NO_ID, +inf.
 *   measured[c]   the members whose distance is not NaN.
 *   spread[c]     the sum over those of w(d) = floor(min(max(d, 0), 2) * 2^30), exact in uint64 (mi_knn_kmeans_seed's weight):
 *                 the mean distance is spread / measured * 2^-30.
 *   totals        {members, live rows with a label >= C, unusable live rows with a label < C, non-empty groups}.
 * centroids: [C][dim]; count, cover, cover_dist, odd, odd_dist, measured, spread: [C] each; dist: [rows]; every output pointer
 * may be NULL.  1 <= C <= 65536 (MI_ERR_UNSUPPORTED above, MI_ERR_INVALID for 0 or a null handle).  labels == NULL on a table
 * whose group column was never set is valid: every row belongs to nothing.  dim as mi_knn_near_pairs requires.  An empty table
 * succeeds with zero counts and the padding above.  An argument error writes nothing.  The call reads the fp32 rows only: the
 * result does not depend on "prefilter".  Every per-group value except the centroid is an integer min, max or sum and the
 * centroid's order is fixed by the row ids: the same table and labels give the same bits on every call.  Two reads of the
 * member rows; device memory beside the outputs: 8 bytes per row, the k-means update's buffers and 32 bytes per group, freed
 * before the call returns.  Runs on the handle's stream behind every write and search enqueued before it, and waits for its
 * results. */
int mi_knn_summarize(mi_knn* t, const uint32_t* labels /* [rows] or NULL */, uint32_t C, float* centroids, uint64_t* count,
                     uint64_t* cover, float* cover_dist, uint64_t* odd, float* odd_dist, uint64_t* measured, uint64_t* spread,
                     float* dist, uint64_t totals[4]);
/* of the last mi_knn_summarize on this handle: out = {segments summed, workgroups of the distance pass, rows read by it, 0} */
int mi_knn_summarize_stats(mi_knn* t, uint64_t out[4]);
/* m pictures that span every group ("show me nine pictures that tell what is in this folder, theme or result list"):
 * farthest-first traversal, the greedy k-center picks, of every group at once — start at one member, then repeatedly take the
 * member farthest from everything taken so far.  The nearest members of the centroid all come from a group's largest part;
 * these picks reach its small parts too, and the gaps say how many thumbnails the group needs.
 * labels, C, "member of c" (a live usable row with label c < C; a label >= C belongs to nothing) and the id map are exactly
 * mi_knn_summarize's.
 *   d(p, r)       the distance mi_knn_search(q = row p) reports for row r, to the bit: the pick is the query, the member the
 *                 streamed row.  key(d) is the search's 32-bit order: NaN after every number, -0 before +0.
 *   K_r           per member r, the smallest key(d(p_i, r)) over the picks p_i of its group so far; rep[r] is the lowest i that
 *                 attains it.
 *   pick 0        of a non-empty group: start[c] when start is given — an id that is not a member of group c: MI_ERR_INVALID
 *                 and no round runs; the entry of an empty group is not looked at — else the member with the lowest id.
 *                 gap[c][0] = +inf.
 *   pick j >= 1   among the not-yet-picked members whose K_r is a number's key (not NaN's): the largest K_r, the lowest id
 *                 among equal keys.  It is made only if K_r > key(min_gap); min_gap = -INFINITY means no bound.  gap[c][j] =
 *                 the distance of that key.  No such member: the group is finished, n_picked[c] = j, the remaining picks are
 *                 MI_KNN_NO_ID and the remaining gaps +inf.
 *   consequence   gap[c][1] >= gap[c][2] >= ... in key order, to the bit: K only falls, so the largest K can only fall.
 *   reach[c]      the distance of the largest number key K_r over ALL members of c after the last pick: every measured member
 *                 lies within reach[c] of a pick.  +inf for an empty group and for one without a number key.
 *   rep[r]        the index i of the pick that stands for row r, rep_dist[r] the distance of K_r.  A member whose every d was
 *                 NaN: MI_KNN_NO_LABEL and NaN.  Every other row that is no member: MI_KNN_NO_LABEL and +inf.
 *   totals        {members, groups with at least one pick, picks made, rounds that made a pick (the largest n_picked)}.
 * picks, gap: [C][m]; n_picked, reach: [C]; rep, rep_dist: [rows] by local row; every output pointer may be NULL.
 * 1 <= C <= 65536, 1 <= m <= 4096 and C * m <= 2^22: MI_ERR_UNSUPPORTED above, MI_ERR_INVALID for a zero C or m, a NaN min_gap
 * or a null handle.  dim as mi_knn_near_pairs requires.  A shard borrowed from a sharded table: MI_ERR_UNSUPPORTED (a group's
 * members lie on other shards).  An empty table succeeds with the padding above.  An argument error writes nothing.
 * The call reads the fp32 rows only: the result does not depend on "prefilter".  Every decision is an integer compare on keys
 * or a 64-bit integer max, so the same table, labels and start give the same bits on every call.  One read of a group's member
 * rows per pick it takes (a finished group reads nothing); device memory beside the outputs: 24 bytes per row, the bucket
 * buffers of the k-means update, 8 bytes per (group, pick) and 28 per group, freed before the call returns.  Runs on the
 * handle's stream behind every write and search enqueued before it, and waits for its results; between the rounds the host
 * reads one word every 8 rounds to stop once a round made no pick. */
int mi_knn_representatives(mi_knn* t, const uint32_t* labels /* [rows] or NULL: the group column */, uint32_t C, uint32_t m,
                           float min_gap, const uint64_t* start /* [C] ids or NULL */, uint64_t* picks /* [C][m] */,
                           float* gap /* [C][m] */, uint32_t* n_picked /* [C] */, float* reach /* [C] */, uint32_t* rep /* [rows] */,
                           float* rep_dist /* [rows] */, uint64_t totals[4]);
/* of the last mi_knn_representatives on this handle: out = {round launches, segments of the member walk, member rows read by
 * the last round launched, 0} */
int mi_knn_representatives_stats(mi_knn* t, uint64_t out[4]);
/* The k best DISTINCT results of a search ("the grid without the same shot ten times"): the search's own list with
 * near-duplicates collapsed behind the best of them, greedily, and how many look-alikes stand behind each kept result.
 *   pool        L = the result of mi_knn_search(t, q, 1, pool) when among == NULL, else of mi_knn_search_filtered(t, q, 1,
 *               pool, among, n_among), with the entries that are MI_KNN_NO_ID or carry a NaN distance removed.  P = |L|; ranks
 *               r = 0 .. P-1 in the search's order (distance ascending, then id).
 *   g(x, y)     for two distinct ids, lo = min(x, y), hi = max(x, y): the distance mi_knn_search(q = row lo) reports for row
 *               hi, bit for bit (the contract of mi_knn_near_pairs).
 *   conflict    x and y conflict iff g(x, y) <= min_gap.  A NaN never conflicts.
 *   walk        ranks 0 .. P-1 in order.  For L[r] let F be the KEPT entry of smallest rank that conflicts with it.  F
 *               exists: L[r] is hidden behind F, hidden[slot(F)] += 1, rep[r] = slot(F).  Otherwise, fewer than k entries
 *               kept so far: L[r] is kept in the next slot, rep[r] = its slot.  Otherwise L[r] is left over, rep[r] =
 *               MI_KNN_NO_LABEL.  Greedy, not connected components: with A ~ B, B ~ C, A not ~ C in rank order, A is kept,
 *               B is hidden behind A and C is kept.
 * idx [k], dist [k]: the kept entries in slot order with the ids and distance bits the search reported; MI_KNN_NO_ID / +inf
 * behind the last kept entry.  hidden [k] (may be NULL): 0 in the padding.  rep [pool] (may be NULL): MI_KNN_NO_LABEL at
 * positions >= P.  *n_kept (may be NULL).
 * 1 <= k <= pool <= 4096: zero or a null t / q / idx / dist is MI_ERR_INVALID, pool > 4096 or k > pool MI_ERR_UNSUPPORTED; a
 * pool larger than the table is fine.  min_gap NaN or < 0: MI_ERR_INVALID; min_gap = +INFINITY keeps exactly one entry.
 * among as for mi_knn_search_filtered (any order, duplicates and deleted rows allowed, n_among may be 0: an empty pool); an id
 * that is not a row of the table: MI_ERR_INVALID and nothing runs.  No output is written on MI_ERR_INVALID.  dim as
 * mi_knn_near_pairs requires.  A shard borrowed from a sharded table: MI_ERR_UNSUPPORTED, as for mi_knn_neighbors.  An empty
 * table, or P = 0: all padding, *n_kept = 0, MI_OK.
 * The search's list stays on the device.  Its P rows are gathered into a contiguous copy (at most 12 MB at dim 768) whose
 * bf16 mirror is built for the call (the table's own mirror is not used); the join's stage 1 finds every pair of the pool
 * its bound cannot exclude, each is re-evaluated from the fp32 rows and the conflicts are set in a P x P bit matrix (at most
 * 2 MB, atomic ORs: order-free); one workgroup then performs the walk.  Candidates are bounded by "join_cap" as for the
 * join (an overflowing strip is redone in smaller pieces, nothing is dropped).  The result does not depend on the
 * "prefilter" option, on "join_cap" or on the order candidates arrive in.  Runs on the handle's stream behind every write
 * and search enqueued before it, and waits for its results. */
int mi_knn_search_diverse(mi_knn* t, const float* q, uint32_t k, uint32_t pool, float min_gap, const uint64_t* among,
                          uint64_t n_among, uint64_t* idx, float* dist, uint32_t* hidden, uint32_t* rep, uint32_t* n_kept);
/* of the last mi_knn_search_diverse on this handle: out = {P, candidate pairs stage 1 handed to stage 2, conflicting pairs
 * found, pool entries hidden} */
int mi_knn_search_diverse_stats(mi_knn* t, uint64_t out[4]);
/* All-of / any-of / none-of terms in ONE exact pass over the fp32 rows ("beach AND dog", "sunset OR sunrise", "beach
 * WITHOUT people"): every candidate row gets the distance to EVERY term before anything is selected; the per-term distances
 * are combined into one score per row and the k rows with the smallest (score, id) come back.
 *   per-term distance  d_j(r) is the distance mi_knn_search(q = term j) reports for row r, bit for bit: the same summation
 *               order and the same expression 1 - dot / (sqrt(qq) * sqrt(xx)).
 *   order       distances are compared under the search's key order: numeric order, -0 before +0, every NaN last and equal
 *               to every other NaN.
 *               MI_COMPOUND_ALL: score(r) = the largest d_j(r) over the positive terms under that order; one NaN term makes
 *               the score NaN.  MI_COMPOUND_ANY: the smallest; a NaN term is ignored unless every term is NaN.  The score
 *               carries the bits of the term that decides it (a NaN is 0x7FC00000).
 *   negatives   row r is excluded iff for some negative term j  d_j(r) <= neg_within[j]  (an ordinary float comparison: a NaN
 *               distance never excludes).  neg_within[j] NaN or < 0: MI_ERR_INVALID; +INFINITY excludes every row with a
 *               non-NaN distance to that term.
 *   candidates  among == NULL: every live row.  Otherwise the ids given, as for mi_knn_search_filtered: any order, duplicates
 *               allowed, deleted rows left out, n_among may be 0; an id that is not a row: MI_ERR_INVALID and nothing runs.
 *   result      the k candidates with the smallest (score, id), in that order; excluded rows and rows with a NaN score are
 *               left out; MI_KNN_NO_ID / +inf behind the last hit, so exactly k hits come back whenever k rows qualify.
 *               idx [k], dist [k] = the score.  term_dist (may be NULL) [k][n_pos + n_neg] = d_j of the result's row,
 *               positives first in the order given, then negatives; +inf in the padding.  It lets a UI say which term held a
 *               picture back.
 * pos: [n_pos][dim], neg: [n_neg][dim], neg_within: [n_neg].  1 <= n_pos, n_pos + n_neg <= 8, 1 <= k <= 4096 (larger:
 * MI_ERR_UNSUPPORTED).  MI_ERR_INVALID for zero, a null t / pos / idx / dist, an unknown mode, or n_neg > 0 with a null neg /
 * neg_within; no output is written on MI_ERR_INVALID.  dim in {128, 256, 512, 768, 1024} (the set mi_knn_kmeans_seed accepts),
 * MI_ERR_UNSUPPORTED otherwise.  An empty table or an empty candidate set: all padding, MI_OK.
 * n_pos = 1, n_neg = 0 equals mi_knn_search with its NaN entries removed; repeating a positive term changes nothing.
 * The call reads the fp32 rows only: the result does not depend on the "prefilter" option, nor on "compound_blocks"
 * (mi_knn_set_option: workgroups of the scan, 0 = the batched search's grid, v >= 1 = exactly min(v, tiles / 4)).  It works on
 * a shard borrowed from a sharded table and reports that shard's ids.  Runs on the handle's stream behind every write and
 * search enqueued before it, and waits for its results. */
#define MI_COMPOUND_ALL 0 /* near EVERY positive term: score = the largest of their distances  */
#define MI_COMPOUND_ANY 1 /* near AT LEAST ONE:        score = the smallest                    */
int mi_knn_search_compound(mi_knn* t, const float* pos, uint32_t n_pos, int mode, const float* neg, const float* neg_within,
                           uint32_t n_neg, uint32_t k, const uint64_t* among, uint64_t n_among, uint64_t* idx, float* dist,
                           float* term_dist /* may be NULL */);
/* of the last mi_knn_search_compound on this handle: out = {rows or list entries scanned, rows excluded by a negative term,
 * rows (not excluded) with a NaN score, results written} */
int mi_knn_search_compound_stats(mi_knn* t, uint64_t out[4]);
/* The k nearest rows AFTER a cursor and WITHIN a distance, with the counts a results page needs ("101-200 of 3 412"), exact,
 * in one pass over the fp32 rows.  Page n costs what page 1 costs, a row never appears on two pages, and no surviving row is
 * skipped when rows are appended or deleted between two pages.
 *   candidates  among == NULL: every live row.  Otherwise the live rows the ids name, as for mi_knn_search_filtered: any order,
 *               duplicates allowed, deleted rows left out, n_among == 0 with a non-null pointer is the empty set; an id that is
 *               not a row: MI_ERR_INVALID.
 *   distance    d(r) is what mi_knn_search(q) reports for row r, bit for bit.  key(r) = (dist_to_u32(d(r)) << 32) | local row,
 *               the search's own 64-bit key: distance ascending (-0 before +0), id ascending among equal distances, NaN last.
 *   cursor      after_id == MI_KNN_NO_ID: from the start, after_dist is ignored.  Otherwise after_id must be an id of the table
 *               (a DELETED row is allowed: the picture under the cursor may have been removed since) and after_dist must not be
 *               NaN.  The cursor key is built from the bits of after_dist exactly as given: -0 and +0 are different keys, so the
 *               caller passes back what it received — the (dist, idx) of the previous page's last hit.
 *   window      a candidate is in the window when key > cursor key and dist_to_u32(d) <= dist_to_u32(max_dist): the bound is
 *               inclusive and uses the key order.  max_dist = +INFINITY: no bound; NaN: MI_ERR_INVALID.
 *   result      the k smallest keys of the window, ascending by (distance, id): idx [k], dist [k]; MI_KNN_NO_ID / +inf behind
 *               the last hit.  A candidate whose distance is NaN is never returned, as in mi_knn_search_many.
 *   counts      (may be NULL) of the candidates, each in the first class that applies, so the four add up to the number of
 *               candidates: [0] before = key <= cursor key (0 without a cursor), [1] window, [2] beyond = not NaN and past both
 *               the cursor and the bound, [3] nan.
 * Any violation above returns MI_ERR_INVALID, and nothing runs or is written.  1 <= k <= 4096 (0: MI_ERR_INVALID, larger:
 * MI_ERR_UNSUPPORTED); dim in {128, 256, 512, 768, 1024} as for mi_knn_search_compound, MI_ERR_UNSUPPORTED otherwise.  An
 * empty table or an empty candidate set: all padding, every count 0, MI_OK.
 * Identities: (a) without a cursor and with max_dist = +INFINITY the result is mi_knn_search(q, k) without its NaN entries;
 * (b) calling again with the last hit of the previous page as the cursor, until a page has fewer than k hits, concatenates to
 * exactly the list of (a) with k = all rows, for any page size; with rows appended or deleted between two pages this holds for
 * the rows that exist when each page is asked for.
 * The call reads the fp32 rows only: the result does not depend on the "prefilter" option (there is no two-stage form), nor
 * on "page_blocks" (mi_knn_set_option: workgroups of the scan, 0 = the single pass's grid, v >= 1 = exactly min(v, tiles / 4)).
 * It works on a shard borrowed from a sharded table with that shard's ids.  Runs on the handle's stream behind every write
 * and search enqueued before it, and waits for its result. */
int mi_knn_search_page(mi_knn* t, const float* q, uint32_t k,
                       float after_dist, uint64_t after_id, /* the cursor: the last entry of the previous page */
                       float max_dist,                      /* +INFINITY: no bound */
                       const uint64_t* among, uint64_t n_among,
                       uint64_t* idx, float* dist, uint64_t counts[4] /* may be NULL */);
/* ---- groups: one 32-bit group id per row, resident on the device beside the deletion bitmap --------------------------------
 * A group is whatever the caller says it is: a folder, a component of mi_pairs_to_groups, a label of mi_knn_kmeans or
 * mi_knn_assign.  MI_KNN_NO_GROUP marks a row that belongs to no group; such a row is a group of its own, a singleton.
 * Appended rows start as MI_KNN_NO_GROUP, and a table whose column was never set behaves as all singletons.  The column grows
 * with the table.  It is NOT written to MIKNN files: mi_knn_load (and mi_index_load, mi_knn_sharded_load) leave the loaded
 * rows without a group, and the file format is unchanged.
 *   set   ids == NULL: the first n rows in table order; otherwise groups[i] goes to row ids[i] (a later entry for the same id
 *         wins).  Group ids are < MI_KNN_GROUPS_MAX (2^24), or MI_KNN_NO_GROUP.  An id that is not a row, or a group id out of
 *         range: MI_ERR_INVALID, nothing written.  Deleted rows may be named.
 *   get   the same addressing; rows never set report MI_KNN_NO_GROUP.
 *   info  {n_groups = 1 + the largest group id ever set on this handle (0: none), rows that hold a group}. */
#define MI_KNN_NO_GROUP 0xFFFFFFFFu
#define MI_KNN_GROUPS_MAX (1u << 24)
int mi_knn_set_groups(mi_knn* t, const uint64_t* ids, uint64_t n, const uint32_t* groups);
int mi_knn_get_groups(mi_knn* t, const uint64_t* ids, uint64_t n, uint32_t* groups);
int mi_knn_groups_info(mi_knn* t, uint64_t info[2]);
/* The best hit per group, with facet counts ("field collapsing plus facets"), exact over the whole table, in one pass over the
 * fp32 rows plus three short passes over 12 bytes per row.  In the terms of mi_knn_search_page:
 *   candidates, distance, key, window   exactly that call's with no cursor: a candidate is in the window when
 *               dist_to_u32(d) <= dist_to_u32(max_dist) (inclusive, on the key order; +INFINITY: no bound; NaN:
 *               MI_ERR_INVALID).  A NaN distance is never in the window.
 *   representative  of a group: its in-window row with the smallest key — among equal distances the lowest id.  Every
 *               in-window MI_KNN_NO_GROUP row is its own representative.
 *   result      the k representatives with the smallest keys, ascending: idx [k], dist [k] as the search reports them;
 *               group [k] (may be NULL) the group id or MI_KNN_NO_GROUP; members [k] (may be NULL) the in-window candidates
 *               of that group, 1 for a singleton.  Padding behind the last hit: MI_KNN_NO_ID, +inf, MI_KNN_NO_GROUP, 0.
 *   facets      (may be NULL) facets[g] = in-window candidates of group g, for g < n_groups (mi_knn_groups_info); it needs
 *               cap_facets >= n_groups, else MI_ERR_INVALID; entries past n_groups are left alone.  Asking for facets costs
 *               one more copy of 4 n_groups bytes from the device.
 *   totals      (may be NULL) {representatives in the window = matched groups + matched singletons, rows in the window, rows
 *               beyond it and not NaN, NaN rows}; the last three are mi_knn_search_page's counts[1..3].
 * 1 <= k <= 4096 (0: MI_ERR_INVALID, larger: MI_ERR_UNSUPPORTED); dim as for mi_knn_search_page.  Argument errors return
 * their code, and nothing runs or is written.  An empty table or an empty candidate set: all padding, zero counts, MI_OK.
 * Identities: (a) with every row MI_KNN_NO_GROUP the result is mi_knn_search_page(q, k, no cursor, max_dist), members = 1;
 * (b) with all rows in one group there is one hit, the search's top-1, members = the window count; (c) sum(facets) + matched
 * singletons = totals[1]; (d) for each hit, mi_knn_search_filtered over that group's rows with k = 1 gives the same id and
 * the same distance bits.
 * The call reads the fp32 rows only: the result does not depend on "prefilter", nor on "page_blocks", nor on the options
 * "group_blocks" (mi_knn_set_option: workgroups of the reduce and mark passes, 0 = four per CU, v >= 1 = exactly
 * min(v, keys / 256)) and "group_lds_max" (the largest n_groups whose reduce pass builds block-private tables in LDS; default
 * and maximum 4096, 0 = always the global form).  Every per-group value is an integer min or sum: the result does not depend
 * on the order in which rows arrive.  It works on a shard borrowed from a sharded table with that shard's ids and column.
 * Runs on the handle's stream behind every write and search enqueued before it, and waits for its result. */
int mi_knn_search_grouped(mi_knn* t, const float* q, uint32_t k, float max_dist, const uint64_t* among, uint64_t n_among,
                          uint64_t* idx, float* dist, uint32_t* group /* may be NULL */, uint64_t* members /* may be NULL */,
                          uint64_t* facets /* may be NULL */, uint64_t cap_facets, uint64_t totals[4] /* may be NULL */);
/* ---- attributes and predicates: "like this, among my favourites, taken 2019-2021, not hidden, in this folder" ---------------
 * Two more per-row columns, resident on the device beside the deletion bitmap and the group column:
 *   tags   one uint64_t per row: 64 flags whose meaning is the application's.  Default 0.
 *   stamp  one int64_t per row: a capture time, a rating, any ordered value.  Default 0.
 * They are created by the first mi_knn_set_attrs (a table that never sets attributes allocates nothing and behaves as if every
 * row held the defaults), grow with the table (appended rows hold the defaults) and are NOT written to MIKNN files: the file
 * format and mi_abi_version are unchanged; mi_knn_get_attrs lets the application persist them.
 *   set   tags[i] / stamps[i] go to row ids[i]; a NULL column keeps what the rows hold; a later entry for the same id wins.  An
 *         id that is not a row: MI_ERR_INVALID, nothing written.  Deleted rows may be set and read.
 *   get   the same addressing; either output may be NULL. */
int mi_knn_set_attrs(mi_knn* t, const uint64_t* ids, uint64_t n, const uint64_t* tags /* NULL: keep */,
                     const int64_t* stamps /* NULL: keep */);
int mi_knn_get_attrs(mi_knn* t, const uint64_t* ids, uint64_t n, uint64_t* tags /* may be NULL */, int64_t* stamps /* may be NULL */);
/* The predicate.  A row qualifies iff it is live (not deleted) and
 *   (tags & all_of) == all_of,   any_of == 0 || (tags & any_of) != 0,   (tags & none_of) == 0,
 *   stamp_lo <= stamp <= stamp_hi   (signed, inclusive: lo > hi matches nothing; INT64_MIN .. INT64_MAX: every stamp), and,
 *   with MI_KNN_WHERE_GROUP in flags, its group (mi_knn_set_groups) == group: MI_KNN_NO_GROUP selects the rows without a
 *   group, and a table without a group column matches nothing under the flag.
 * Any other bit in flags: MI_ERR_INVALID. */
#define MI_KNN_WHERE_GROUP 1u
typedef struct mi_knn_where {
    uint64_t all_of, any_of, none_of; /* on tags; any_of == 0: clause absent */
    int64_t stamp_lo, stamp_hi;       /* inclusive, signed; lo > hi matches nothing */
    uint32_t group;                   /* used only with MI_KNN_WHERE_GROUP */
    uint32_t flags;                   /* MI_KNN_WHERE_GROUP; other bits: MI_ERR_INVALID */
} mi_knn_where;
/* The predicate is evaluated on the device, over the columns, without the host touching a row: an ordered two-pass compaction
 * (count per chunk of rows, offsets, emit) leaves the qualifying rows as the ascending list the gathered search reads.  No
 * workgroup waits for another; integers only, the same list for any grid.  The host reads back one 8-byte total per call.
 * Option "where_chunk" (mi_knn_set_option): rows per workgroup of the two passes, 0 = 4096, otherwise a multiple of 64 up to
 * 65536; it changes no answer.
 *   count  *count = the qualifying rows.
 *   rows   their ids, ascending, the first `cap` of them into ids (may be NULL with cap == 0); *count = the number qualifying,
 *          also when that exceeds cap. */
int mi_knn_count_where(mi_knn* t, const mi_knn_where* w, uint64_t* count);
int mi_knn_rows_where(mi_knn* t, const mi_knn_where* w, uint64_t* ids, uint64_t cap, uint64_t* count);
/* The k nearest among the qualifying rows.  Contract: the result is bit-identical to mi_knn_search_filtered(t, q, nq, k, ids =
 * every qualifying row) — same ids, same order, same distance bits, same MI_KNN_NO_ID / +inf padding; k <= 4096, else
 * MI_ERR_UNSUPPORTED; nothing qualifying gives k no-id entries.  *matched (may be NULL) = the qualifying rows.  Behind the
 * predicate passes run the filtered search's own kernels over the list.  Runs on the handle's stream behind every write and
 * search enqueued before it, and waits for its result. */
int mi_knn_search_where(mi_knn* t, const float* q, uint32_t nq, uint32_t k, const mi_knn_where* w, uint64_t* idx, float* dist,
                        uint64_t* matched /* may be NULL */);
/* ---- ordered search: the hits within a distance in the order of their stamps -----------------------------------------------------
 * "Everything that looks like this, newest first, 100 at a time": the rows within max_dist of q, ordered by stamp instead of by
 * distance, one page per call, and the timeline facet ("matches per month") over the same rows.
 *   candidates  the live rows w keeps — exactly the rows mi_knn_rows_where returns; w == NULL: every live row.
 *   within      a candidate is within iff its distance is not NaN and <= max_dist on the search's key order (inclusive, -0
 *               before +0): the "window" class of mi_knn_search_page without a cursor.  A row's distance has the bits
 *               mi_knn_search reports for it.
 *   order       okey(s) = (uint64_t)s ^ 0x8000000000000000, bitwise complemented under MI_KNN_ORDER_DESC; the result order is
 *               (okey(stamp), id) ascending: equal stamps break by ascending id in both directions.  A table that never set
 *               attributes holds stamp 0 everywhere and is ordered by id.
 *   cursor      with MI_KNN_ORDER_AFTER only rows with (okey(stamp), id) > (okey(after_stamp), after_id) are returned.  after_id
 *               must name a row of the table (deleted or not), else MI_ERR_INVALID; after_stamp is taken as given, not looked up:
 *               pass back (stamps[k-1], idx[k-1]) of the previous page.  Page n costs what page 1 costs, no row appears twice and
 *               no surviving row is skipped when rows are appended or deleted between pages.  A row whose STAMP is changed
 *               between two pages may move across the cursor: it can then appear twice or not at all.
 *   result      the first min(k, remaining) slots: idx, dist (the distance bits), stamps (may be NULL) in the result order;
 *               MI_KNN_NO_ID / +inf / 0 behind them.
 *   counts      (may be NULL) {within, before, beyond, nan}: candidates within the bound (the cursor does not change it); those of
 *               them at or before the cursor (0 without the flag); candidates with a non-NaN distance above the bound; candidates
 *               with a NaN distance.  "101-200 of `within`".
 * 1 <= k <= 4096 (0: MI_ERR_INVALID, larger: MI_ERR_UNSUPPORTED); dim as for mi_knn_search_page; max_dist NaN, unknown flag bits
 * and a bad w (as mi_knn_search_where judges it): MI_ERR_INVALID.  An error writes nothing to any output.  An empty table, or a
 * predicate that keeps nothing, gives padding and zero counts.
 * How: the predicate's list (mi_knn_search_where's passes), mi_knn_search_page's scan leaving one distance key per candidate,
 * then integers only: a radix select over the 96-bit key (okey(stamp), position) — one short histogram pass per digit, six for
 * the stamp and three for the position, of which those behind a decided pick return at once — a collect, a one-block sort, one
 * packed record back.  The same answer for any grid (option "page_blocks" sizes these passes too).  Runs on the handle's stream
 * behind every write and search enqueued before it, and waits for its result. */
#define MI_KNN_ORDER_DESC  1u   /* largest stamp first; default: smallest first */
#define MI_KNN_ORDER_AFTER 2u   /* (after_stamp, after_id) is a cursor */
int mi_knn_search_ordered(mi_knn* t, const float* q, uint32_t k, float max_dist,
                          const mi_knn_where* w /* may be NULL: every live row */,
                          uint32_t flags, int64_t after_stamp, uint64_t after_id,
                          uint64_t* idx, float* dist, int64_t* stamps /* may be NULL */,
                          uint64_t counts[4] /* may be NULL */);
/* The timeline facet: hist[b] = the rows within (as above) with exactly b edges <= stamp — hist[0] is "before edges[0]",
 * hist[n_edges] "at or after the last edge"; sum(hist) == within.  edges: strictly ascending, 1 <= n_edges <= 4096, else
 * MI_ERR_INVALID (edges, not a bucket width: calendar months are not equal-width).  hist: [n_edges + 1], written only on
 * success. */
int mi_knn_stamp_histogram(mi_knn* t, const float* q, float max_dist, const mi_knn_where* w /* may be NULL */,
                           const int64_t* edges, uint32_t n_edges, uint64_t* hist /* [n_edges + 1] */);
/* host-only: pairs -> groups (connected components, union-find).  ids: every id that occurs in a pair, grouped; groups
 * ordered by their smallest id, ids ascending inside a group; group_start[g] .. group_start[g + 1] index ids
 * (group_start holds n_groups + 1 entries).  Two-call protocol: counts are always written, arrays up to their caps. */
int mi_pairs_to_groups(const uint64_t* a, const uint64_t* b, uint64_t n_pairs, uint64_t* ids, uint64_t cap_ids,
                       uint64_t* group_start, uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups);

/* ---------------------------------------------- Seam B over several GPUs, ONE process */

/* The reference server is one process holding one database handle (server/src/main.rs:30-35), one search at
 * a time (server/src/search.rs:26).  mi_knn_sharded keeps that shape for a table larger than one GPU:
 * `n_dev` shards on `devices[]` (BASELINE config 5: 8 x 10 M rows) behind one handle.
 *   rows    block-cyclic: global row r (= its id, the insertion ordinal) is in block r / block_rows, blocks are
 *           dealt round-robin to the shards (block_rows = 0 -> 4096; a multiple of 64).  Appends keep ids global.
 *   search  the query goes to every device, the shards scan concurrently on their own streams, the per-shard
 *           top-k lists (12 k bytes per shard and query) are all-gathered — RCCL ncclAllGather over xGMI between
 *           distinct devices; device-to-device / peer copies into the first shard's buffer when a device is listed twice
 *           or librccl is absent — and merged once, on the device.  Result = what ONE mi_knn holding every row returns,
 *           bit for bit.
 * A device may be listed more than once (several shards on one GPU: how a one-GPU box tests n > 1). */
int mi_knn_sharded_create(uint32_t dim, const int* devices, int n_dev, uint32_t block_rows, mi_knn_sharded** out);
void mi_knn_sharded_free(mi_knn_sharded* t);
/* any of the outputs may be NULL; transport: 0 = single shard, 1 = device-to-device / peer copies, 2 = RCCL all-gather
 * (a one-shard table made under MI_KNN_SHARDED_TRANSPORT=rccl reports 2: its one-rank communicator runs the collective) */
int mi_knn_sharded_info(const mi_knn_sharded* t, uint64_t* rows, uint32_t* n_shards, uint32_t* block_rows, int* transport);
/* What the exchange step of server/src/search.rs:70-86's replacement has really executed on this handle so far:
 * out = {searches enqueued, ncclAllGather calls issued (ONE per shard and search: ids and distances travel as one packed
 * record), transport copies issued instead, device merges}. */
int mi_knn_sharded_stats(const mi_knn_sharded* t, uint64_t out[4]);
int mi_knn_sharded_set_option(mi_knn_sharded* t, const char* key, int value); /* mi_knn_set_option on every shard */
int mi_knn_sharded_reserve(mi_knn_sharded* t, uint64_t rows);
int mi_knn_sharded_append(mi_knn_sharded* t, const float* rows, uint64_t n, uint64_t* first_id /* may be NULL */);
/* Rows that are already in device memory, on ANY device of the process (src_device; e.g. straight from
 * mi_clip_embed_device of a replica there): every run goes to its shard by a device-to-device copy (same GPU) or
 * hipMemcpyPeerAsync over xGMI (another GPU), enqueued on `stream` — a stream of src_device, NULL = its null stream — with
 * no trip through the host and no host block; searches enqueued afterwards see the rows.  A failure leaves the table as it was. */
int mi_knn_sharded_append_device(mi_knn_sharded* t, const float* d_rows, uint64_t n, int src_device, void* stream,
                                 uint64_t* first_id /* may be NULL */);
int mi_knn_sharded_append_synthetic(mi_knn_sharded* t, uint64_t seed, uint64_t first_row, uint64_t n);
/* shard s of the table, borrowed (its device, its size, mi_knn_get_rows on local rows, ...); NULL when out of range */
mi_knn* mi_knn_sharded_shard(mi_knn_sharded* t, uint32_t s);
int mi_knn_sharded_get_rows(mi_knn_sharded* t, uint64_t first, uint64_t n, float* out);
int mi_knn_sharded_search(mi_knn_sharded* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist);
/* The same search without the wait: everything (query upload, the shards' scans, exchange, merge, readback) is enqueued
 * and the call returns; idx / dist (caller-owned, must stay valid) are filled when mi_knn_sharded_sync returns, or when 8
 * later searches have been enqueued.  q is copied before the call returns. */
int mi_knn_sharded_search_async(mi_knn_sharded* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist);
int mi_knn_sharded_sync(mi_knn_sharded* t);
/* `<prefix>.g<gen>.<s>of<n>.miknn` per shard + the manifest `<prefix>.shards` (n, block, rows, dim, gen), written last:
 * every save is a new GENERATION of files, the previous one is deleted only after the manifest names the new one, so a
 * crash or an I/O error at any point of a save leaves a complete, loadable table on disk.  load needs an empty table
 * (and leaves it empty on failure) and re-deals the blocks when the shard count or block size differ from the saved ones. */
int mi_knn_sharded_save(mi_knn_sharded* t, const char* prefix);
int mi_knn_sharded_load(mi_knn_sharded* t, const char* prefix);
/* mi_knn_delete / mi_knn_deleted on global ids (`DELETE FROM image WHERE id IN $ids` over the whole table); save, load
 * (any shard count and block size) and rebalance carry the deletions */
int mi_knn_sharded_delete(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, uint64_t* newly);
int mi_knn_sharded_deleted(mi_knn_sharded* t, uint64_t* ids, uint64_t cap, uint64_t* count);
/* mi_knn_search_filtered on global ids: every shard searches the ids it holds, the merge does the rest; the result equals
 * the filtered search of one table that holds every row.  Waits for its results. */
int mi_knn_sharded_search_filtered(mi_knn_sharded* t, const float* q, uint32_t nq, uint32_t k, const uint64_t* ids,
                                   uint64_t n_ids, uint64_t* idx, float* dist);
/* mi_knn_search_compound on global ids, without term_dist: every shard answers for the rows (or the ids of `among`) it holds
 * on its own stream, the lists are merged with mi_knn_merge's ordering; the result equals the one-table result bit for bit.
 * Waits for its results. */
int mi_knn_sharded_search_compound(mi_knn_sharded* t, const float* pos, uint32_t n_pos, int mode, const float* neg,
                                   const float* neg_within, uint32_t n_neg, uint32_t k, const uint64_t* among, uint64_t n_among,
                                   uint64_t* idx, float* dist);
/* mi_knn_search_page on global ids: after_id must be a global row id of the table (deleted or not).  Every shard answers on
 * its own stream and host thread for the rows (or the ids of `among`) it holds; a shard's local rows ascend with their global
 * ids, so its window starts at (after_dist, the number of its rows with a global id <= after_id).  The lists are merged with
 * mi_knn_merge's ordering and the counts are summed; the result equals the one-table result bit for bit.  Waits for its result. */
int mi_knn_sharded_search_page(mi_knn_sharded* t, const float* q, uint32_t k, float after_dist, uint64_t after_id, float max_dist,
                               const uint64_t* among, uint64_t n_among, uint64_t* idx, float* dist, uint64_t counts[4]);
/* The group column of a sharded table, on global ids: every id is checked first (one bad id or group id: MI_ERR_INVALID,
 * nothing written), then each shard takes the entries of the rows it holds, as mi_knn_sharded_delete routes its ids.
 * ids == NULL: the first n global rows.  info = {1 + the largest group id ever set on any shard, rows that hold a group}.
 * mi_knn_sharded_rebalance re-applies the column to the destination by global id, as it re-applies deletions; the column is
 * not saved (mi_knn_sharded_load leaves it unset). */
int mi_knn_sharded_set_groups(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, const uint32_t* groups);
int mi_knn_sharded_get_groups(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, uint32_t* groups);
int mi_knn_sharded_groups_info(mi_knn_sharded* t, uint64_t info[2]);
/* mi_knn_search_grouped on global ids.  Every shard returns its k best representatives on its own stream and host thread; the
 * host merges them by group id (the smaller (distance word, global id) wins, singletons never merge), sorts and keeps k.  This
 * is exact: in the shard that holds a group's global best, every group ranked ahead of it there also ranks ahead of it
 * globally, so a globally top-k group is in that shard's top k.  members of the winners are gathered from every shard's
 * per-group counts on the device (k words per shard) and summed.  facets and totals[0] need every shard's whole count array
 * on the host — 4 n_groups bytes per shard — and are computed only when one of the two is asked for; totals[0] counts a group
 * matched in several shards once.  The result equals the one-table result bit for bit.  Waits for its result. */
int mi_knn_sharded_search_grouped(mi_knn_sharded* t, const float* q, uint32_t k, float max_dist, const uint64_t* among,
                                  uint64_t n_among, uint64_t* idx, float* dist, uint32_t* group, uint64_t* members,
                                  uint64_t* facets, uint64_t cap_facets, uint64_t totals[4]);
/* The attribute columns and predicates of a sharded table, on global ids.  set / get: every id is checked first (one bad id:
 * MI_ERR_INVALID, nothing written), then each shard takes the entries of the rows it holds, as mi_knn_sharded_set_groups
 * routes its ids.  count_where sums the shards.  search_where: every shard turns the predicate into its own list and runs its
 * gathered search; the packed exchange and the device merge are mi_knn_sharded_search's.  The result equals the one-table
 * result bit for bit; *matched (may be NULL) = the qualifying rows of all shards.  mi_knn_sharded_rebalance re-applies the
 * columns to the destination by global id; they are not saved. */
int mi_knn_sharded_set_attrs(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, const uint64_t* tags, const int64_t* stamps);
int mi_knn_sharded_get_attrs(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, uint64_t* tags, int64_t* stamps);
int mi_knn_sharded_count_where(mi_knn_sharded* t, const mi_knn_where* w, uint64_t* count);
int mi_knn_sharded_search_where(mi_knn_sharded* t, const float* q, uint32_t nq, uint32_t k, const mi_knn_where* w, uint64_t* idx,
                                float* dist, uint64_t* matched /* may be NULL */);
/* mi_knn_search_ordered / mi_knn_stamp_histogram on global ids: every shard runs the call on its own rows, on its own stream and
 * host thread; a shard that does not hold after_id starts at its first row whose global id is larger.  The host merges the
 * shards' lists by (okey(stamp), id) and sums the counts and the histograms: the result equals the one-table result bit for
 * bit.  after_id must be a global row id of the table (deleted or not). */
int mi_knn_sharded_search_ordered(mi_knn_sharded* t, const float* q, uint32_t k, float max_dist, const mi_knn_where* w, uint32_t flags,
                                  int64_t after_stamp, uint64_t after_id, uint64_t* idx, float* dist, int64_t* stamps,
                                  uint64_t counts[4]);
int mi_knn_sharded_stamp_histogram(mi_knn_sharded* t, const float* q, float max_dist, const mi_knn_where* w, const int64_t* edges,
                                   uint32_t n_edges, uint64_t* hist);
/* mi_knn_assign over the whole table: every shard labels its own rows on its own stream (concurrently: no exchange is
 * needed), the results land at the rows' global ids.  labels / dist: [rows of the table]; equals the one-table result
 * bit for bit.  (k-means over a sharded table, whose update needs a cross-shard reduction: mi_knn_sharded_kmeans.) */
int mi_knn_sharded_assign(mi_knn_sharded* t, const float* vectors, uint32_t C, uint32_t* labels, float* dist);
/* mi_knn_assign_multi over the whole table, as mi_knn_sharded_assign: per shard, results ([rows of the table][m]) at the
 * rows' global ids; equals the one-table result bit for bit */
int mi_knn_sharded_assign_multi(mi_knn_sharded* t, const float* vectors, uint32_t C, uint32_t m, float max_dist,
                                uint32_t* labels, float* dist);
/* mi_knn_search_many over the whole table: every shard answers on its own stream and host thread (as
 * mi_knn_sharded_assign_multi), the per-shard lists are merged with mi_knn_merge's ordering; equals the one-table result
 * bit for bit */
int mi_knn_sharded_search_many(mi_knn_sharded* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist);
/* mi_knn_search_many_where over the whole table: every shard masks and answers locally, the lists meet as
 * mi_knn_sharded_search_many's do, *matched (may be NULL) = the sum over the shards; equals the one-table result bit for bit */
int mi_knn_sharded_search_many_where(mi_knn_sharded* t, const float* q, uint32_t nq, uint32_t k, const mi_knn_where* w,
                                     uint64_t* idx, float* dist, uint64_t* matched /* may be NULL */);
/* mi_knn_near_pairs over the whole table (the reference's one table in one server, server/src/main.rs, at the size that needs
 * several GPUs): every pair of live rows a < b (global ids) with cosine distance <= max_dist whose larger id is >= first_new,
 * ascending by (a, b) — ids and distance bits are those of mi_knn_near_pairs on ONE table that holds the same rows in id
 * order.  A pair whose rows live in different shards is found by joining the two shards (mi_knn_near_pairs_between's
 * primitive, the row with the smaller id as the query); the S self-joins run side by side, then the S (S - 1) / 2 shard
 * pairs in round-robin rounds in which no shard occurs twice, the row side alternating between the shards; a column side on
 * another device is staged on the row side's device.  first_new: 0 (all pairs) or any id up to one past the last row
 * (beyond: MI_ERR_INVALID); it need not belong to a particular shard.  cap, *count, the errors and the early stop (checked
 * between launches across the whole call): as mi_knn_near_pairs. */
int mi_knn_sharded_near_pairs(mi_knn_sharded* t, float max_dist, uint64_t first_new, uint64_t* a, uint64_t* b, float* dist,
                              uint64_t cap, uint64_t* count);
/* of the last mi_knn_sharded_near_pairs: {candidates, pairs, stage-1 launches, tiles} summed over every shard and shard pair */
int mi_knn_sharded_near_pairs_stats(mi_knn_sharded* t, uint64_t out[4]);
/* mi_knn_density / mi_knn_dbscan over the whole table: every definition there (deg, core, clusters, border, noise, via,
 * via_dist, summary) applied to the pairs W that mi_knn_sharded_near_pairs(t, max_dist, first_new = 0) reports, with "row" read
 * as global row — a cluster is named by the id of its smallest core row in the whole table, a border row joins the core that
 * minimises (distance key, global row of the core) whichever shard that core lies in.  Arrays are [rows of the table], indexed
 * by global row as mi_knn_sharded_assign's labels are.  The result equals, bit for bit, mi_knn_dbscan's for ONE table that
 * holds the same rows, for any shard count, block size, chunking ("join_stage", "join_stage_rows") and arrival order: devices
 * exchange degrees (summed), border keys (64-bit minima) and disjoint-set forests (united) through copies only, never through
 * pointers or atomics across devices.  The pairs never leave the devices.  Memory per shard beside the join's buffers: 12 bytes
 * per local row and 4 bytes per row of the WHOLE table (the shard's forest over global rows), plus one more such array on the
 * first shard's device and the result arrays, freed before the call returns.
 * The argument rules and errors are mi_knn_density's / mi_knn_dbscan's; a table without shards: MI_ERR_INVALID; 2^32 or more
 * rows in the table: MI_ERR_UNSUPPORTED; dim as mi_knn_sharded_near_pairs requires.  An error writes nothing.  An empty
 * table and empty shards are valid. */
int mi_knn_sharded_density(mi_knn_sharded* t, float max_dist, uint32_t* counts);
int mi_knn_sharded_dbscan(mi_knn_sharded* t, float max_dist, uint32_t min_pts, uint64_t* cluster, uint64_t* via, float* via_dist,
                          uint32_t* counts, uint64_t summary[4]);
/* of the last mi_knn_sharded_density / mi_knn_sharded_dbscan: the eight fields of mi_knn_dbscan_stats summed over every shard
 * and shard pair.  "unions that merged" also counts the final merge of the shards' forests, so it is >= core rows - clusters
 * (two shards may each merge the same two components). */
int mi_knn_sharded_dbscan_stats(mi_knn_sharded* t, uint64_t out[8]);
/* mi_knn_kmeans over the whole table, always on the exact integer sums of option "kmeans_fixed_sum" (defined at mi_knn_kmeans;
 * the shards' option is not consulted).  Per iteration every shard assigns its own rows and sums them per cluster on its own
 * device; the sums S_s [C][dim] int64 and sizes n_s [C] uint32 of shards 1 .. S-1 are copied to the first shard's device (in
 * chunks of at most 16 MB) and added into the first shard's, the centroids are formed there and copied back to every shard.
 * Integer adds give the same sum in any order, so centroids, labels, dist, *iters_run, *changed_last and *objective (summed
 * in double in GLOBAL row order) equal, bit for bit, mi_knn_kmeans' on ONE table that holds the same rows with
 * "kmeans_fixed_sum" = 1 — for any shard count, block size and devices.  labels / dist: [rows of the table] by global row, as
 * mi_knn_sharded_assign's; either may be NULL.  Bytes that cross between shards per update:
 * (S - 1) * C * (8 * dim + 4) inward and (S - 1) * C * dim * 4 outward, nothing else; a shard without rows takes part with
 * zeros.  Streams are ordered by events; the host waits only where mi_knn_kmeans does (an assign's counts).
 * Arguments and errors as mi_knn_kmeans (they are checked first, and an error writes nothing); a table without shards:
 * MI_ERR_INVALID; 2^32 or more rows in the table: MI_ERR_UNSUPPORTED.  An empty table: MI_OK, zeros in *iters_run,
 * *changed_last and *objective, centroids untouched. */
int mi_knn_sharded_kmeans(mi_knn_sharded* t, float* centroids, uint32_t C, uint32_t max_iters, uint32_t* labels, float* dist,
                          uint32_t* iters_run, uint64_t* changed_last, double* objective);
/* of the last mi_knn_sharded_kmeans: {updates run, bytes copied between shards, segments summed in the last update (all
 * shards), merge launches} */
int mi_knn_sharded_kmeans_stats(mi_knn_sharded* t, uint64_t out[4]);
/* mi_knn_kmeans_seed over the whole table ("what mi_knn_sharded_kmeans should start from"): every output equals, bit for
 * bit, what mi_knn_kmeans_seed returns on ONE table holding the same rows under the same ids, with the same deleted rows, C,
 * seed and among — for any shard count, block size and devices.
 *   candidates  among == NULL: every live row, ascending by global id.  Otherwise the n_among global ids given, sorted and
 *               made unique, deleted rows left out; an id that is not a row of the table: MI_ERR_INVALID, nothing runs.
 *               S = their number, position p = 0 .. S-1 in that order (the GLOBAL position).
 *   usable, z_j, pick j, weights
 *               as defined at mi_knn_kmeans_seed: the splitmix64 stream started at `seed`, T = floor(z_j * total / 2^64),
 *               the smallest global position whose inclusive prefix sum of w exceeds T; total == 0: the lowest GLOBAL
 *               position not picked before (a fallback pick); z_j is consumed either way;
 *               w_p = (uint32) floor(min(max(D_p, 0), 2) * 2^30).
 * rows: [C] = the global id of pick j, in pick order.  centroids: [C, dim] or NULL = those rows' fp32 values (what
 * mi_knn_sharded_kmeans takes as its initial centroids).  potential (or NULL) = sum of w_p * 2^-30 in double after one more
 * weight update with the last pick.
 * How it runs: rows are dealt block-cyclically, so the global candidate order is a fixed interleaving of the shards' local
 * blocks.  Every shard keeps D, w and the flags of its own candidates and sums w per chunk (at most 256 consecutive positions
 * of one local block).  Per seed: every shard but the first copies its chunk sums and the lowest global id it has not picked
 * to the first shard's device; a pick there scans all chunk sums in global order and writes a 16-byte word {owning shard, its
 * chunk, remainder of T, mode}; the word goes to every shard; the owner finds the position inside its chunk and writes
 * {id, owner flag, the row} into a slot of 16 + 4 dim bytes; the slots go to the first shard, which appends the flagged one
 * and sends its 4 dim bytes back as the centre of every shard's next pass.  Sums of uint32 in uint64 are the same in any
 * order and the distances carry the search's bits, so the picks are the single table's.  Bytes copied between shards
 * (copies within the first shard not counted), with K = the chunks of shards 1 .. S-1:
 *     (C + 1) * 8 * (K + S - 1)  +  C * (S - 1) * (32 + 8 * dim).
 * Streams are ordered by events, nothing is polled, no atomics; everything is enqueued and the host waits once.  A shard
 * without rows or without candidates takes part with zero chunks.
 * Checked before the handle is followed: a null handle, a null `rows`, C == 0, among == NULL with n_among != 0:
 * MI_ERR_INVALID; C > 65536: MI_ERR_UNSUPPORTED.  Then: a table without shards: MI_ERR_INVALID; dim outside {128, 256, 512,
 * 768, 1024} or 2^32 or more rows: MI_ERR_UNSUPPORTED; an id that is not a row, C > S: MI_ERR_INVALID.  An error writes
 * nothing, apart from *potential = 0.  Delivers the searches pending on the table first, and waits for its results. */
int mi_knn_sharded_kmeans_seed(mi_knn_sharded* t, uint32_t C, uint64_t seed, const uint64_t* among, uint64_t n_among, uint64_t* rows,
                               float* centroids, double* potential);
/* of the last mi_knn_sharded_kmeans_seed: {candidates S, passes (C + 1), fallback picks, bytes copied between shards} */
int mi_knn_sharded_kmeans_seed_stats(mi_knn_sharded* t, uint64_t out[4]);
/* mi_knn_summarize over the whole table ("describe the themes mi_knn_sharded_kmeans / mi_knn_sharded_dbscan just found"):
 * every output is mi_knn_summarize's, evaluated over the table the shards form together, and equals, bit for bit, what ONE
 * mi_knn holding the same rows returns with "kmeans_fixed_sum" = 1 (the shards' option is not consulted) — for any shard
 * count, block size and devices.  labels: [rows of the table] by global row, as mi_knn_sharded_kmeans' labels are, or NULL:
 * every shard reads its own part of the group column (mi_knn_sharded_set_groups) on its device; a column that was never set
 * means every row belongs to nothing.  dist: [rows of the table] by global row; cover / odd are global ids.
 *   members, dist   as mi_knn_summarize defines them.
 *   centroid[c]     (float)((double)S * 2^-30 / count[c]), S the int64 sum of the members' components in units of 2^-30
 *                   (defined at mi_knn_kmeans) over ALL shards; all zeros if empty.
 *   cover / odd     the smallest / largest (32-bit distance key, id) over the members of the whole table, by the rules of
 *                   mi_knn_summarize; a tie goes to the lowest GLOBAL id, whichever shard holds it.
 *   measured, spread, count, totals   integer sums over the shards.
 * Every shard marks and sums its own rows; the sums S_s [C][dim] int64 and sizes n_s [C] of shards 1 .. S-1 are added into the
 * first shard's as mi_knn_sharded_kmeans adds them, the centroids go back to every shard, every shard measures its members
 * against them, turns the rows in its per-group words into global ids and the first shard folds the words together (min,
 * max, sum, sum).  Bytes that cross between shards: (S - 1) * C * (8 * dim + 4 + 32) inward and (S - 1) * 4 * C * dim
 * outward, nothing else; a shard without rows takes part with zeros.  Streams are ordered by events; the host waits once
 * per shard, for the results.
 * Every output pointer may be NULL.  1 <= C <= 65536 (MI_ERR_UNSUPPORTED above, MI_ERR_INVALID for 0 or a null handle), judged
 * before the handle is followed; a table without shards: MI_ERR_INVALID; 2^32 or more rows in the table: MI_ERR_UNSUPPORTED;
 * dim as mi_knn_near_pairs requires.  An error writes nothing.  An empty table succeeds with mi_knn_summarize's padding. */
int mi_knn_sharded_summarize(mi_knn_sharded* t, const uint32_t* labels /* [rows] by global row, or NULL */, uint32_t C,
                             float* centroids, uint64_t* count, uint64_t* cover, float* cover_dist, uint64_t* odd, float* odd_dist,
                             uint64_t* measured, uint64_t* spread, float* dist /* [rows] by global row */, uint64_t totals[4]);
/* of the last mi_knn_sharded_summarize: {segments summed (all shards), bytes copied between shards, merge launches (sums and
 * per-group words together), members} */
int mi_knn_sharded_summarize_stats(mi_knn_sharded* t, uint64_t out[4]);
/* Change the layout of a LIVE table: every row of `src` into the empty `dst` (another shard count, device set or block
 * size), block by block, device to device — a plain copy where source and destination shard share a GPU,
 * hipMemcpyPeerAsync over xGMI where they do not; nothing passes through the host.  src is unchanged. */
int mi_knn_sharded_rebalance(mi_knn_sharded* dst, mi_knn_sharded* src);
/* The compaction of a sharded table: every LIVE row of src into the empty dst (same dim; any shard count, device set or
 * block size), in global order — mi_knn_sharded_rebalance that leaves the deleted rows behind.  Groups, tags and stamps
 * travel by compacted global id; dst equals a fresh sharded table given the survivors in order.  src is unchanged.  new_ids
 * (may be NULL): [src's rows] by src's global row, the row's id in dst, MI_KNN_NO_ID for a deleted row; cap = its length
 * (cap < rows: MI_ERR_INVALID, nothing changes); *removed (may be NULL) = rows left behind.  A failure leaves dst empty.  (A
 * sharded table is not compacted in place: survivors change shard under the block-cyclic deal, so that would be this
 * redistribution anyway.) */
int mi_knn_sharded_compact_into(mi_knn_sharded* dst, mi_knn_sharded* src, uint64_t* new_ids, uint64_t cap, uint64_t* removed);
/* the placement arithmetic by itself (host-only): global row <-> (shard, local row) */
int mi_knn_sharded_place(uint32_t block_rows, uint32_t n_shards, uint64_t row, uint32_t* shard, uint64_t* local);
int mi_knn_sharded_id(uint32_t block_rows, uint32_t n_shards, uint32_t shard, uint64_t local, uint64_t* row);

/* Deterministic merge of `lists` candidate lists of k (id, dist) entries each —
 * what every rank holds after the all-gather of per-shard results — into the
 * global top-k under the same ordering.  Host-only. */
int mi_knn_merge(const uint64_t* idx_in, const float* dist_in, uint32_t lists, uint32_t k,
                 uint64_t* idx, float* dist);
/* The same merge on the device, asynchronous on `stream`: in = [lists][nq][k] (the rank-major buffer an all-gather of
 * per-shard [nq][k] results leaves on every rank), out = [nq][k].  Each input list must be in result order with its
 * MI_KNN_NO_ID padding at the tail (what every search entry point returns).  Bit-identical to mi_knn_merge. */
int mi_knn_merge_device(int device, const uint64_t* d_idx_in, const float* d_dist_in, uint32_t lists, uint32_t nq, uint32_t k,
                        uint64_t* d_idx, float* d_dist, void* stream);

/* ------------------------------------------- fused flow (BASELINE config 4, one GPU) */

/* The body of the scan loop (server/src/clip.rs:107-137: upload -> forward -> readback -> insert)
 * and the query (server/src/search.rs:70-86) as one pipeline on three HIP streams:
 *   copy stream    upload of chunk i+1 under the forward of chunk i
 *   ingest stream  forward; its last kernel writes the embeddings straight into the table's next
 *                  rows (no readback, no re-upload)
 *   search stream  the scan of a query and the readback of its k results; the host does not
 *                  block on it (results arrive at sync/drain).  Measured: on the device the
 *                  4.5 ms scan does NOT hide under the forward -- with the runtime's default 4
 *                  hardware queues it runs between two forwards, with 8 queues it overlaps and
 *                  slows the forward by as much; the stream buys host-side
 *                  asynchrony, not device time
 * `model` is an image tower, `table` a shard on the same device with dim == the model's output
 * width.  Both are borrowed and must outlive the pipeline; they stay usable through their own
 * entry points (the handles order all work, see Conventions). */
int mi_pipeline_create(mi_clip* model, mi_knn* table, mi_pipeline** out);
/* The same pipeline for ONE process over several GPUs (BASELINE config 5 as the reference's single server would run it:
 * one AppState, scan task and search handler side by side, server/src/main.rs:30-35): models[s] is the tower replica on the
 * device of the table's shard s (n_models == shard count; one handle may serve several shards of its GPU).
 *   ingest  a chunk is cut at the table's block boundaries; every run is uploaded to, and embedded by, the replica on the
 *           GPU that owns its block, whose last kernel writes the rows straight into that shard ("each
 *           replica appends its embeddings to its local shard"); runs of consecutive blocks occupy different GPUs at once,
 *           so a table created with block_rows = the chunk size per GPU keeps every replica busy.
 *   query   mi_knn_sharded_search_async: the shards scan side by side, lists all-gathered and merged on the device.
 * mi_pipeline_ingest / query / sync / drain / stats / free serve both forms (drain delivers everything pending here;
 * mi_pipeline_query_device is for the one-GPU form, whose caller does the exchange). */
int mi_pipeline_create_sharded(mi_clip* const* models, int n_models, mi_knn_sharded* table, mi_pipeline** out);
void mi_pipeline_free(mi_pipeline* p);
/* Enqueue one chunk: nchw = [n,3,H,W] f32, host memory.  The n embeddings become rows
 * [size, size+n) of the table; *first_id (may be NULL) = id of the first one.  Returns when the
 * chunk is queued (at most two chunks are in flight).  With pinned memory (mi_host_alloc) the upload
 * is asynchronous and the buffer may be refilled once the NEXT mi_pipeline_ingest (or
 * mi_pipeline_sync) has returned; ordinary memory is staged before the call returns.
 * n = 0 is a successful no-op, as in mi_clip_embed. */
int mi_pipeline_ingest(mi_pipeline* p, const float* nchw, size_t n, uint64_t* first_id);
/* Enqueue one query (q: [dim] f32 host, copied before the call returns) over every row ingested by
 * the calls made before this one.  idx [k] / dist [k] (host, caller-owned) are filled when
 * mi_pipeline_sync returns (or when 16 later queries have been enqueued).  Same results and
 * ordering as mi_knn_search. */
int mi_pipeline_query(mi_pipeline* p, const float* q, uint32_t k, uint64_t* idx, float* dist);
/* As mi_pipeline_query, the k results left on the device (d_idx [k] uint64, d_dist [k] f32, caller-owned, same device):
 * the per-shard list of a row-sharded table, ready for the all-gather without a trip through the host.  The scan runs
 * on the pipeline's search stream; `consumer_stream` (a hipStream_t; NULL = the device's default stream, e.g. what
 * torch.cuda.current_stream() is unless the caller changed it) is made to wait for it — an event, no host block — so work
 * enqueued on that stream afterwards (the collective) sees the results. */
int mi_pipeline_query_device(mi_pipeline* p, const float* q, uint32_t k, uint64_t* d_idx, float* d_dist, void* consumer_stream);
/* Wait for everything enqueued and deliver the pending query results. */
int mi_pipeline_sync(mi_pipeline* p);
/* Deliver finished queries, oldest first, until at most `leave_pending` are still pending (blocks
 * for those it delivers; the ingest stream is not waited for).  With leave_pending = 1 a caller gets
 * the results of query i-1 while query i scans: the per-shard lists a multi-GPU caller all-gathers. */
int mi_pipeline_drain(mi_pipeline* p, uint32_t leave_pending);
/* Device time spent in the pipeline's forwards and scans as measured by events on their own streams,
 * folded in at sync: out = {forwards, total ms of forwards, scans, total ms of scans}; reset != 0 clears. */
int mi_pipeline_stats(mi_pipeline* p, double out[4], int reset);

/* Page-locked host memory for upload buffers (hipHostMalloc). */
int mi_host_alloc(size_t bytes, void** out);
void mi_host_free(void* p);

/* ------------------------------------------- table `image` with its image_path column */

/* The statements the reference server issues against `image` {id, image_path, embedding} (server/src/search.rs:13-18),
 * so that the Rust side needs nothing between its handlers and this library:
 *   mi_index_existing   SELECT image_path FROM image WHERE image_path IN $paths              server/src/clip.rs:74-83
 *   mi_index_insert     db.insert("image").content(rows)                                     server/src/clip.rs:125-137
 *   mi_index_rows_of    SELECT id .. FROM image WHERE image_path IN $paths (then mi_knn_get_rows on mi_index_table)
 *                                                                                            server/src/search.rs:43-58
 *   mi_index_search     the refine step + `embedding <|K|> $reference`                       server/src/search.rs:20-110
 * Row id = insertion ordinal.  No uniqueness constraint on image_path (the reference's table has none; its scan loop
 * filters with the first statement): a path may own several rows.  media_dir: requests name files "media/<rel>", rows
 * store media_dir + <rel> (server/src/search.rs:35-40, :104-109); "" disables the mapping. */
int mi_index_create(uint32_t dim, int device, const char* media_dir, mi_index** out);
void mi_index_free(mi_index* ix);
mi_knn* mi_index_table(mi_index* ix); /* the embedding shard, borrowed (mi_pipeline_create, mi_knn_get_rows, ...) */
int mi_index_size(mi_index* ix, uint64_t* rows);
int mi_index_media_dir(mi_index* ix, char* buf, size_t cap, size_t* needed); /* as given at creation, or as loaded */
int mi_index_existing(mi_index* ix, const char* const* paths, size_t n, uint8_t* exists /* [n]: 1 = has a row */);
int mi_index_insert(mi_index* ix, const char* const* paths, const float* embeddings, size_t n, uint64_t* first_id);
/* paths for the n rows mi_pipeline_ingest has just written into mi_index_table (embeddings never left the device) */
int mi_index_adopt(mi_index* ix, const char* const* paths, size_t n);
/* ids of every row of the given paths, ascending and unique (table order: average_slices adds in input order);
 * *count = how many there are, at most `cap` are written */
int mi_index_rows_of(mi_index* ix, const char* const* paths, size_t n, uint64_t* ids, size_t cap, size_t* count);
/* image_path of row `id`; web != 0: as sent to the client, relative to "media/" (server/src/search.rs:104-109) */
int mi_index_path(mi_index* ix, uint64_t id, int web, char* buf, size_t cap, size_t* needed);
/* web_search_text behind the text tower: referenced_images are the client's "media/.." names; those found in the table
 * refine the query; idx/dist [k] as mi_knn_search; *n_found (may be NULL) = results before the MI_KNN_NO_ID padding */
int mi_index_search(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref, uint32_t k,
                    uint64_t* idx, float* dist, uint32_t* n_found);
/* mi_index_search among the rows under the given folders (`... AND string::starts_with(image_path, $folder)`, as a
 * pre-filter: exactly k hits whenever k rows qualify).  Folders are client names: "media/2024/trip" matches whole path
 * components (media/2024/trip/a.jpg and media/2024/trip/x/b.jpg, not media/2024/tripb/c.jpg); "media/" is the whole media
 * directory; names outside "media/" match nothing.  Refinement by referenced_images as in mi_index_search, marked images
 * outside the folders included.  Removed paths match nothing.  k <= 4096. */
int mi_index_search_within(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref,
                           const char* const* folders, size_t n_folders, uint32_t k, uint64_t* idx, float* dist,
                           uint32_t* n_found);
/* mi_index_search with near-duplicates collapsed (mi_knn_search_diverse): the query is refined as in mi_index_search;
 * n_folders = 0: the pool comes from the whole table, otherwise from the rows mi_index_search_within would search (folders
 * that match nothing: an empty pool).  idx / dist / hidden [k] as mi_knn_search_diverse (hidden may be NULL); *n_found (may
 * be NULL) = kept results before the padding. */
int mi_index_search_diverse(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref,
                            const char* const* folders, size_t n_folders, uint32_t k, uint32_t pool, float min_gap,
                            uint64_t* idx, float* dist, uint32_t* hidden, uint32_t* n_found);
/* mi_knn_search_compound over the index: terms as for that call; folders as in mi_index_search_within (n_folders = 0: the whole
 * table; folders that match nothing: an empty candidate set); removed paths never appear.  There is no refinement inside the
 * call: a caller who wants a term refined with marked images passes it through mi_refine first.  idx / dist [k], term_dist
 * [k][n_pos + n_neg] (may be NULL), *n_found (may be NULL) = results before the padding. */
int mi_index_search_compound(mi_index* ix, const float* pos, uint32_t n_pos, int mode, const float* neg, const float* neg_within,
                             uint32_t n_neg, const char* const* folders, size_t n_folders, uint32_t k, uint64_t* idx, float* dist,
                             float* term_dist, uint32_t* n_found);
/* mi_knn_search_page over the index: the text embedding refined with referenced_images exactly as mi_index_search does,
 * folders as in mi_index_search_within (n_folders = 0: the whole table; folders that match nothing: an empty candidate set),
 * then the page after (after_dist, after_id) within max_dist; removed paths never appear.  idx / dist [k], *n_results (may be
 * NULL) = results before the padding, counts (may be NULL) as for mi_knn_search_page. */
int mi_index_search_page(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref,
                         const char* const* folders, size_t n_folders, uint32_t k, float after_dist, uint64_t after_id,
                         float max_dist, uint64_t* idx, float* dist, uint32_t* n_results, uint64_t counts[4]);
/* mi_knn_search_grouped over the index, grouped by the image's DIRECTORY (the path without its last component; files directly
 * in the media directory form one group).  Group ids are assigned in first-seen order and kept in a dictionary of the index;
 * the table's column is brought up to date lazily, before a grouped search: only the rows inserted or adopted since the last
 * one are uploaded, everything after mi_index_load.  The text embedding is refined and `folders` restrict the candidates as in
 * mi_index_search_page; removed paths never appear.  idx / dist [k], group / members [k] (may be NULL), *n_found (may be NULL)
 * = results before the padding, facets / cap_facets / totals as for mi_knn_search_grouped (n_groups = mi_index_group_count).
 * The index owns the column of its table: a caller who sets groups on mi_index_table directly (labels of mi_knn_kmeans, say)
 * may search them with mi_knn_search_grouped, and makes the index upload its own column again, whole, on the next
 * mi_index_search_grouped. */
int mi_index_search_grouped(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref,
                            const char* const* folders, size_t n_folders, uint32_t k, float max_dist, uint64_t* idx, float* dist,
                            uint32_t* group, uint64_t* members, uint32_t* n_found, uint64_t* facets, uint64_t cap_facets,
                            uint64_t totals[4]);
/* the directory behind a group id of mi_index_search_grouped, with its trailing '/': as stored (web == 0) or as the client
 * names it ("media/...", web != 0); mi_index_path's buffer protocol.  An unknown group: MI_ERR_INVALID. */
int mi_index_group_name(mi_index* ix, uint32_t group, int web, char* buf, size_t cap, size_t* needed);
int mi_index_group_count(mi_index* ix, uint32_t* n_groups); /* directories seen so far */
/* the group id of a directory as the client names it ("media/a/b" or "media/a/b/"; "media/" = the files directly in the media
 * directory): what MI_KNN_WHERE_GROUP takes for "in this folder" (the folder itself, not the folders below it).  A directory
 * no image was ever stored under: MI_ERR_INVALID. */
int mi_index_group_of(mi_index* ix, const char* folder, uint32_t* group);
/* mi_knn_set_attrs by path: tags[i] / stamps[i] (either may be NULL: keep) go to every row stored under paths[i] (paths as
 * mi_index_rows_of takes them).  An unknown path: MI_ERR_INVALID, nothing written. */
int mi_index_set_attrs(mi_index* ix, const char* const* paths, size_t n, const uint64_t* tags, const int64_t* stamps);
/* web_search_text among the rows a predicate keeps (mi_knn_search_where): the refined query of mi_index_search, no id list at
 * all.  With MI_KNN_WHERE_GROUP the group is a directory id (mi_index_group_of): the table's group column is brought up to
 * date first, as mi_index_search_grouped does.  Removed paths never appear (they are deleted rows of the table).  idx / dist
 * [k], *n_found (may be NULL) = results before the padding, *matched (may be NULL) = the qualifying rows. */
int mi_index_search_where(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref, uint32_t k,
                          const mi_knn_where* where, uint64_t* idx, float* dist, uint32_t* n_found, uint64_t* matched);
/* web_search_text as a timeline (mi_knn_search_ordered / mi_knn_stamp_histogram): the refined query of mi_index_search, a
 * predicate as mi_index_search_where takes it (where may be NULL; with MI_KNN_WHERE_GROUP the group is a directory id and the
 * group column is brought up to date first), the cursor and the flags of mi_knn_search_ordered.  Removed paths never appear.
 * idx / dist [k], stamps [k] (may be NULL), *n_found (may be NULL) = results before the padding, counts (may be NULL) as for
 * mi_knn_search_ordered. */
int mi_index_search_ordered(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref, uint32_t k,
                            float max_dist, const mi_knn_where* where, uint32_t flags, int64_t after_stamp, uint64_t after_id,
                            uint64_t* idx, float* dist, int64_t* stamps, uint32_t* n_found, uint64_t counts[4]);
int mi_index_stamp_histogram(mi_index* ix, const float* text_embedding, const char* const* referenced_images, size_t n_ref,
                             float max_dist, const mi_knn_where* where, const int64_t* edges, uint32_t n_edges, uint64_t* hist);
/* `<dir>/embedding.miknn` + `<dir>/image_path.bin`, each through a temporary file, fsync and rename, the path file
 * last: after a crash the directory holds a consistent index (at worst the one before the save). */
int mi_index_save(mi_index* ix, const char* dir);
int mi_index_load(mi_index* ix, const char* dir); /* into an empty index */
/* Replaces `DELETE FROM image WHERE image_path IN $paths`: every row of each path (a path may own several) is deleted
 * (mi_knn_delete on mi_index_table).  Afterwards mi_index_existing reports 0 for the path (a later scan re-embeds a file
 * that comes back under it, as a new row), mi_index_rows_of and mi_index_search leave its rows out, and mi_index_path of
 * such a row fails with MI_ERR_INVALID.  Paths without rows are ignored.  *removed_rows (may be NULL) = rows deleted.
 * The removal is saved with the embedding file (MIKNNv02); the path file is unchanged. */
int mi_index_remove(mi_index* ix, const char* const* paths, size_t n, uint64_t* removed_rows);
/* mi_knn_compact on mi_index_table, and the path column with it: the removed rows leave, the others close up and take new
 * ids (new_ids, cap, *removed: as mi_knn_compact).  Every lookup and search names the same paths as before the call (the
 * server's responses carry paths, never row ids: clients notice nothing); mi_index_save then writes the MIKNNv01 file
 * (32 + L x dim x 4 bytes) and a path file of L entries. */
int mi_index_compact(mi_index* ix, uint64_t* new_ids, uint64_t cap, uint64_t* removed);
/* every image_path that has a row that was not removed, once each, as consecutive NUL-terminated strings; *needed = bytes
 * of the whole list, whole paths up to `cap` bytes are written (buf may be NULL) — what a scan's prune compares with the
 * files it found (search.py prune_missing_images) */
int mi_index_live_paths(mi_index* ix, char* buf, size_t cap, size_t* needed);
/* duplicate groups of table `image`: mi_knn_near_pairs on mi_index_table + mi_pairs_to_groups; removed paths never appear.
 * max_pairs bounds the join (MI_ERR_UNSUPPORTED beyond it). */
int mi_index_duplicates(mi_index* ix, float max_dist, uint64_t first_new, uint64_t max_pairs, uint64_t* ids,
                        uint64_t cap_ids, uint64_t* group_start, uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups);
/* bursts of table `image`: mi_index_duplicates over mi_knn_near_pairs_window — the connected components of W_win, i.e. groups
 * chained by pairs that look alike AND were taken within `window` of each other (the stamps mi_index_set_attrs set). */
int mi_index_bursts(mi_index* ix, float max_dist, uint64_t window, uint64_t first_new, uint64_t max_pairs, uint64_t* ids,
                    uint64_t cap_ids, uint64_t* group_start, uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups);
/* "skip what I already have" at import: mi_knn_near_pairs_between on the two indexes' tables (the reference, one table in one
 * server — server/src/main.rs — can only compare paths).  a[i]: a row id of ix, b[i]: a row id of other (mi_index_path names
 * them), ascending by (a, b); removed paths are deleted rows and never reported. */
int mi_index_matches(mi_index* ix, mi_index* other, float max_dist, uint64_t* a, uint64_t* b, float* dist, uint64_t cap,
                     uint64_t* count);
/* themes of table `image`: mi_knn_dbscan on mi_index_table in mi_index_duplicates' output shape — the clusters ordered by
 * their smallest id, ids ascending inside; noise is not listed, *n_noise counts it; removed paths are in neither. */
int mi_index_themes(mi_index* ix, float max_dist, uint32_t min_pts, uint64_t* ids, uint64_t cap_ids, uint64_t* group_start,
                    uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups, uint64_t* n_noise);
/* events of table `image`: mi_index_themes over mi_knn_dbscan_window — a theme photographed in two far-apart periods comes out
 * as two clusters. */
int mi_index_events(mi_index* ix, float max_dist, uint64_t window, uint32_t min_pts, uint64_t* ids, uint64_t cap_ids,
                    uint64_t* group_start, uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups, uint64_t* n_noise);
/* The folders at a glance (mi_knn_summarize over the directory groups of mi_index_search_grouped): for directory g <
 * min(cap, *n_groups) its number of images count[g], its cover and odd one out (row ids: mi_index_path names them) with their
 * distances to the folder's centroid, measured[g] and spread[g] as mi_knn_summarize defines them.  Removed paths are deleted
 * rows: they count nowhere.  Every array may be NULL; *n_groups = the directories seen so far (mi_index_group_name names them).
 * More than 65536 directories: MI_ERR_UNSUPPORTED.  An index without a row succeeds with *n_groups = 0. */
int mi_index_folder_overview(mi_index* ix, uint32_t cap, uint64_t* count, uint64_t* cover, float* cover_dist, uint64_t* odd,
                             float* odd_dist, uint64_t* measured, uint64_t* spread, uint32_t* n_groups);
/* The folders' highlights (mi_knn_representatives over the same directory groups, started at each folder's cover): for
 * directory g < min(cap, *n_groups) the row ids picks[g][0 .. m-1] (MI_KNN_NO_ID behind the last pick), their gaps gap[g][.]
 * and n_picked[g], as mi_knn_representatives defines them with labels = NULL, min_gap as given and start = the covers of
 * mi_index_folder_overview.  picks, gap: [cap][m]; every array may be NULL; *n_groups = the directories seen so far.  m and
 * the number of directories under mi_knn_representatives' limits, else MI_ERR_UNSUPPORTED; m = 0 or a NaN min_gap:
 * MI_ERR_INVALID.  An index without a row succeeds with *n_groups = 0. */
int mi_index_folder_highlights(mi_index* ix, uint32_t cap, uint32_t m, float min_gap, uint64_t* picks, float* gap, uint32_t* n_picked,
                               uint32_t* n_groups);

/* ------------------------------------------------------------ query refinement */

/* fn average_slices(vectors: &Vec<&Vec<f32>>) -> Vec<f32> (server/src/search.rs:127-150):
 * zero-init, add in input order, divide by (m as f32).  m = 0 -> MI_ERR_INVALID
 * (the reference asserts "Input must not be empty"). */
int mi_average_slices(const float* const* vectors, size_t m, size_t len, float* out);
/* the refine step of web_search_text (server/src/search.rs:28, :60-67):
 * m = 0 -> out = text; else out = average_slices([average_slices(selected), text]). */
int mi_refine(const float* text, const float* const* selected, size_t m, size_t len, float* out);

#ifdef __cplusplus
}
#endif
#endif /* MI355CLIP_H */
