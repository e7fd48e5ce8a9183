/*
 * gsrast.h -- C ABI of the MI355X (gfx950) differentiable Gaussian rasterizer.
 *
 * This is the drop-in boundary for the ONE hot path of yjb6/SaRO-GS: the three static entry
 * points of the reference's native rasterizer,
 *     CudaRasterizer::Rasterizer::forward      (cuda_rasterizer/rasterizer.h:34-58,  impl rasterizer_impl.cu:198-339)
 *     CudaRasterizer::Rasterizer::backward     (cuda_rasterizer/rasterizer.h:60-89,  impl rasterizer_impl.cu:343-436)
 *     CudaRasterizer::Rasterizer::markVisible  (cuda_rasterizer/rasterizer.h:27-32,  impl rasterizer_impl.cu:141-153)
 * (paths relative to /root/reference/submodules/gaussian_rasterization_ch3/), which the reference
 * binds to Python through pybind11 in ext.cpp:15-19 / rasterize_points.cu:35-215.
 *
 * Same argument sets, same meaning, plus an explicit HIP stream.  Differences, all deliberate:
 *   - the three std::function<char*(size_t)> allocators become plain C callbacks + context;
 *   - all pointers are DEVICE pointers (HBM); a NULL pointer means "absent optional input"
 *     exactly as in the reference (shs / colors_precomp / scales / rotations / cov3D_precomp);
 *   - functions return a status (or num_rendered) instead of throwing; gsrast_last_error() has text;
 *   - the contents of the three state buffers are opaque and differ from the reference's chunks
 *     (typed SoA arrays); gsrast_debug_export() copies them out in the
 *     reference's array layout for parity tests;
 *   - `prefiltered` != 0 is the caller's promise that no Gaussian lies behind the near plane: the reference prints and TRAPS the kernel
 *     when one does (auxiliary.h:156-160), gsrast_forward returns GSRAST_E_ARG (after waiting for the device: the promise costs a
 *     synchronisation; SaRO-GS always passes False);
 *   - arithmetic, all within north_star's 1e-5 bar and checked against the fp64 oracle: exp() is a fixed sequence of exactly rounded fp32
 *     operations shared with the oracle (options.exp_mode 0; the reference calls exp(), forward.cu:349), so "bit-exact forward" means
 *     HIP == oracle; the blend backward rebuilds T with v_rcp_f32(1 - alpha) (1 ulp) where the reference divides (backward.cu:503), takes the
 *     geometric sums about the 8 x 8 pixel block's origin and shifts them to the Gaussian's mean afterwards (csrc/gsrast_blend.h: separable
 *     moments), and evaluates backward.cu:505-507's accum_rec for the NEXT contributor (same operands); gradients are accumulated with
 *     float atomics into one 64-byte record per Gaussian (the reference: nine atomics per pixel pair), so their last bits depend on the order.
 * No torch / STL types cross this boundary.
 */
#ifndef GSRAST_H_INCLUDED
#define GSRAST_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSRAST_ABI_VERSION 6   /* 6: the render calls beside gsrast_forward / gsrast_backward are gsrast_render_forward / gsrast_render_backward over one versioned call record each
                                    (fourteen positional render symbols removed).  5: gsrast_grad_rows_clear / gsrast_grad_rows_add take P (indices received from peers are bounds-checked).  4: gsrast_raw_grads.d_sh_factor (the struct grew), gsrast_sh_grad_combine_rows.  3: gsrast_options.no_list_cut (the struct grew).  2: gsrast_backward OVERWRITES every output array (version 1 accumulated into caller-zeroed arrays like the
                                    reference); options.forward_only; the raw family (gsrast_raw_inputs / gsrast_raw_grads) */
#define GSRAST_TILE_X 16 /* reference config.h:16 */
#define GSRAST_TILE_Y 16 /* reference config.h:17 */

/* Allocation callback: must return a device pointer to at least `bytes` bytes, 256-byte aligned,
 * that stays valid until the matching backward call has completed (the reference keeps the
 * buffers alive through ctx.save_for_backward).  A callback may be invoked more than once per
 * forward call (the binning buffer is first requested from an estimate, then again if the estimate
 * was too small); the LAST pointer returned is the buffer in use, earlier ones may be released.
 * Replaces rasterize_points.cu:27-33. */
typedef void* (*gsrast_alloc_fn)(void* ctx, size_t bytes);

/* Forward pass.  Returns num_rendered (number of (Gaussian, tile) instances, >= 0) or a negative
 * GSRAST_E_* code.  out_color [3][H][W] planar, out_depth [1][H][W] (median depth, default 15.0),
 * radii [P] are fully written.  Blocks the host once on `stream` to learn num_rendered
 * (the reference does the same with a cudaMemcpy, rasterizer_impl.cu:282).
 * Replaces Rasterizer::forward, rasterizer.h:34-58. */
int gsrast_forward(gsrast_alloc_fn geometry_alloc, void* geometry_ctx,
                   gsrast_alloc_fn binning_alloc, void* binning_ctx,
                   gsrast_alloc_fn image_alloc, void* image_ctx,
                   int P, int D, int M,
                   const float* background,
                   int width, int height,
                   const float* means3D,
                   const float* shs,
                   const float* colors_precomp,
                   const float* opacities,
                   const float* scales,
                   float scale_modifier,
                   const float* rotations,
                   const float* cov3D_precomp,
                   const float* viewmatrix,
                   const float* projmatrix,
                   const float* cam_pos,
                   float tan_fovx, float tan_fovy,
                   int prefiltered,
                   float* out_color,
                   float* out_depth,
                   int* radii,
                   void* stream);

/* Backward pass.  Replaces Rasterizer::backward, rasterizer.h:60-89.
 * EVERY output array is fully overwritten (zeros for culled Gaussians), none has to be initialised -- the reference
 * accumulates into nine zero-filled arrays (300 B / Gaussian of memset, rasterize_points.cu:150-158); here the blend
 * backward accumulates into one 64-byte record per Gaussian inside geom_buffer (zero-filled by the forward, and again by
 * this call unless options->grads_zeroed says it is the first backward on that state) and the
 * per-Gaussian backward writes dL_dmean2D [P][3] (.z = 0), dL_dopacity [P], dL_dcolor [P][3], dL_dconic [P][4] (.z = 0,
 * as the reference never writes it) from it, next to dL_dmean3D [P][3], dL_dcov3D [P][6], dL_dsh [P][M][3],
 * dL_dscale [P][3], dL_drot [P][4].  May be NULL: dL_dconic (an intermediate), dL_dcolor unless colors_precomp is given,
 * dL_dcov3D when scales / rotations are given (the reference computes and returns all three regardless).
 * geom_buffer is written (the gradient records), binning_buffer / image_buffer are only read.
 * Returns 0 or GSRAST_E_*. */
int gsrast_backward(int P, int D, int M, int R,
                    const float* background,
                    int width, int height,
                    const float* means3D,
                    const float* shs,
                    const float* colors_precomp,
                    const float* scales,
                    float scale_modifier,
                    const float* rotations,
                    const float* cov3D_precomp,
                    const float* viewmatrix,
                    const float* projmatrix,
                    const float* campos,
                    float tan_fovx, float tan_fovy,
                    const int* radii,
                    char* geom_buffer,
                    char* binning_buffer,
                    char* image_buffer,
                    const float* dL_dpix,
                    float* dL_dmean2D,
                    float* dL_dconic,
                    float* dL_dopacity,
                    float* dL_dcolor,
                    float* dL_dmean3D,
                    float* dL_dcov3D,
                    float* dL_dsh,
                    float* dL_dscale,
                    float* dL_drot,
                    void* stream);

/* present[i] = view-space z of means3D[i] > 0.2.  Replaces Rasterizer::markVisible,
 * rasterizer.h:27-32 (kernel checkFrustum, rasterizer_impl.cu:54-66). */
int gsrast_mark_visible(int P, const float* means3D, const float* viewmatrix,
                        const float* projmatrix, unsigned char* present, void* stream);

/* Sizes the library will request through the callbacks (replaces required<T>(),
 * rasterizer_impl.h:67-73). */
size_t gsrast_geometry_bytes(int P);
size_t gsrast_binning_bytes(int num_rendered, int width, int height);
size_t gsrast_image_bytes(int width, int height);

/* A ready-made allocation callback over memory the caller ALREADY holds (round 6): pass gsrast_alloc_prealloc as the gsrast_alloc_fn and a
 * gsrast_prealloc* as its ctx.  Returns ptr when bytes <= capacity, NULL otherwise (the forward then fails with GSRAST_E_ALLOC); `requested`
 * records what was asked for.  The geometry and image buffers' sizes are known before the call (gsrast_geometry_bytes / gsrast_image_bytes), so a
 * host language whose callbacks are expensive (Python: ~5 us each, in front of the forward's first launch) need only keep its own callback for
 * the binning buffer, whose size the library decides. */
typedef struct gsrast_prealloc { void* ptr; size_t capacity; size_t requested; } gsrast_prealloc;
void* gsrast_alloc_prealloc(void* ctx /* gsrast_prealloc* */, size_t bytes);

/* Multi-GPU gradient exchange (no counterpart in the reference, which is single-GPU and sums the per-view gradients of a
 * batch in place, scene/saro_gaussian.py:226-247, :266-276).  Row k of a view's dL/dsh is w_k(view direction) * g, where
 * g[3] is that view's clamp-masked colour gradient of the Gaussian: instead of all-reducing 16 x 3 products per Gaussian,
 * ranks all-gather the 3 numbers and every rank recombines.  With gsrast_set_option("sh_grad_factors", 1),
 * gsrast_backward writes g into dL_dsh, which is then a [P][3] array.  gsrast_sh_grad_combine evaluates
 *     dL_dsh[i][k][c] = scale * sum_{r < N} w_k(normalize(means3D[i] - campos_r)) * g_r[i][c]
 * chunks = N records of chunk_stride floats: [3P floats g_r | 3 floats campos_r | padding].  All device pointers. */
int gsrast_sh_grad_combine(int P, int D, int M, int N, const float* means3D, const float* chunks, size_t chunk_stride,
                           float scale, float* dL_dsh /*[P][M][3]*/, void* stream);
/* Round 5: which Gaussians can have a non-zero gradient row in this view?  flags[i] = 1 if some pixel consumed Gaussian i in the forward
 * that filled geom_buffer (its blend keeps one bit per Gaussian for the backward, csrc/gsrast_common.h: GeomLayout::untouched), 0 if none
 * did -- every gradient row of such a Gaussian is exactly zero; all 1 if that forward kept no bits.  The sparse exchange takes its
 * "rows some rank touched" from here instead of scanning the five gradient arrays (56 B per Gaussian). */
int gsrast_touched_rows(int P, const char* geom_buffer, unsigned char* flags /*[P]*/, void* stream);
/* The same recombination for an exchange that moves only the rows some rank touched, and for the raw leaves (round 4):
 *   chunks = N records of chunk_stride floats: [3 * rows floats g_r | 3 floats campos_r | padding], rows <= P;
 *   row_of [P] or NULL: Gaussian i's factor is row row_of[i] of every record, -1 = no rank sent it (its dL/dsh is zero);
 *   NULL: rows == P, row i (then this is gsrast_sh_grad_combine);
 *   the result goes to dL_dsh [P][M][3] (rows [dc | rest]) and / or, split, to d_features_dc [P][1][3] + d_features_rest [P][M-1][3]
 *   (the gradients of SaRO-GS's two SH leaves, scene/saro_gaussian.py:836-845); every row of every array given is written. */
int gsrast_sh_grad_combine_rows(int P, int D, int M, int N, const float* means3D, const float* chunks, size_t chunk_stride, int rows,
                                const int* row_of, float scale, float* dL_dsh, float* d_features_dc, float* d_features_rest, void* stream);

/* Round 5: the recombination for the rows of the union ONLY.  idx [rows] (int64, ascending, distinct): record row j is Gaussian idx[j]'s
 * factor.  Rows of the output arrays outside the union are NOT written: the caller keeps them zero between steps (it clears the previous
 * step's union, a fraction of the array, instead of having all P rows rewritten: 3 M Gaussians, 150 k in the union, 29 MB instead of 576).
 * M * 3 must be a multiple of 4 and at most 48; dL_dsh 16-byte aligned. */
int gsrast_sh_grad_combine_union(int P, int D, int M, int N, const float* means3D, const float* chunks, size_t chunk_stride, int rows,
                                 const long long* idx, float scale, float* dL_dsh, float* d_features_dc, float* d_features_rest, void* stream);

/* Round 5: the compaction either side of the sparse exchange.  Rows idx[0..n) (int64, device) of n_arrays (<= 8) row-major float arrays
 * (arrays[k]: device pointer, widths[k] floats per row; `arrays` and `widths` themselves are HOST arrays) side by side into
 * packed [n][sum of widths], and back into those rows (other rows are not touched). */
int gsrast_rows_pack(long long n, const long long* idx, int n_arrays, const float* const* arrays, const int* widths, float* packed, void* stream);
int gsrast_rows_unpack(long long n, const long long* idx, int n_arrays, float* const* arrays, const int* widths, const float* packed, void* stream);

/* Round 5: the ALL-GATHER gradient exchange (csrc/gsrast_exchange.h; view_parallel.exchange_gradients(sparse="gather")).  Every rank
 * sends only the gradient rows its own view touched, 64-byte rows { Gaussian index | 11 dense floats: mean 3, opacity 1, scale 3,
 * rotation 4 | dL/dsh factor 3 | 0 }, in ONE all-gather of chunks { header row: count, campos x y z | cap rows }, and adds the chunks
 * into its arrays in rank order.  `dense`: a HOST array of four device pointers, [P][3], [P][1], [P][3], [P][4].
 *   pack : rows[0] word 0 (the count, zeroed by the caller) counts the touched rows, rows[1 + k] receive them (arrival order), at most cap.
 *   clear: zeroes, for every row the chunks name, the dense arrays' rows (dense != NULL) and / or the SH arrays' rows (any SH pointer given).
 *   add  : dense[idx] += scale * row, dL/dsh[idx] += scale * w(dir(means3D[idx] - campos)) (x) factor -- no atomics: indices within a chunk
 *          are distinct, chunks are added by consecutive launches.
 *   clear / add take P (round 6): the indices inside a chunk come from a peer; a row whose index is >= P is skipped, never written. */
int gsrast_grad_rows_pack(int P, const unsigned char* touched /*[P]*/, float* const* dense, const float* factor /*[P][3]*/, uint32_t* rows, uint32_t cap, void* stream);
int gsrast_grad_rows_clear(int P, const uint32_t* chunks, int n_chunks, size_t chunk_words, uint32_t cap, float* const* dense /* or NULL */, int M,
                           float* dL_dsh, float* d_features_dc, float* d_features_rest, void* stream);
int gsrast_grad_rows_add(int P, const uint32_t* chunk, uint32_t cap, float* const* dense, int D, int M, const float* means3D, float scale,
                         float* dL_dsh, float* d_features_dc, float* d_features_rest, void* stream);

/* Parity-test helper: copies internal state out in the reference's array layout
 * (GeometryState / BinningState / ImageState members, rasterizer_impl.h:30-65).  Any output
 * pointer may be NULL.  All pointers are device pointers.  keys_sorted is rebuilt as
 * (tile << 32) | depth_bits from the sorted instance list. */
/* NOTE for consumers of the state buffers: with options.tile_clip = 1 (the default) the binning lists a Gaussian only in the tiles
 * its alpha >= 1/255 ellipse reaches, so the instance list holds sum(ranges.y - ranges.x) <= num_rendered entries -- num_rendered (the
 * return value of gsrast_forward) keeps the REFERENCE's meaning (tiles of the 3-sigma squares, rasterizer_impl.cu:277-282) and is then
 * NOT the length of point_list / keys_sorted; size those arrays for num_rendered and read only the ranges.  With tile_clip = 0 the
 * lists are the reference's literal ones and the two numbers coincide.  n_contrib indexes the list in force. */
int gsrast_debug_export(int P, int R, int width, int height,
                        const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
                        float* depths, float* means2D /*[P][2]*/, float* cov3D /*[P][6]*/,
                        float* conic_opacity /*[P][4]*/, float* rgb /*[P][3]*/,
                        unsigned char* clamped /*[P][3]*/, uint32_t* tiles_touched,
                        uint64_t* keys_sorted /*[R]*/, uint32_t* point_list /*[R]*/,
                        uint32_t* ranges /*[T][2]*/, float* final_T /*[H*W]*/,
                        uint32_t* n_contrib /*[H*W]*/, void* stream);

/* ---- Reentrancy: per-call options and contexts ---------------------------------------------------------------------
 * The reference's Rasterizer::{forward, backward} are stateless statics (rasterizer.h:24-83): any number of host threads
 * may call them on different streams / devices.  The same holds here:
 *   - everything that changes what a call computes or how it is scheduled is a field of gsrast_options, passed per call to
 *     gsrast_render_forward / gsrast_render_backward (NULL = a snapshot of the process defaults, taken once at entry);
 *   - the only state that outlives a forward call -- the capacity hints of the speculative launch and the counts of the last
 *     call -- lives in a gsrast_context the caller owns (NULL = a context private to the calling host thread);
 *   - gsrast_last_error() is per host thread.
 * gsrast_forward / gsrast_backward are exactly gsrast_render_forward(NULL, NULL, ...) / gsrast_render_backward(NULL, ...) on a dense record with flags = 0.
 * gsrast_set_option only edits the process DEFAULTS (plus the process-wide diagnostics "profile", "debug_sync"): callers that
 * want different behaviour on different threads pass a gsrast_options instead. */
typedef struct gsrast_options {
    int exp_mode;             /* 0 fixed-sequence exp (default), 1 libm-grade expf, 2 v_exp_f32 */
    int binning;              /* 0 run-compressed (default), 1 instance-level two-pass radix sort */
    int tile_clip;            /* 1 (default) list a Gaussian only in tiles its alpha >= 1/255 ellipse reaches; 0 literal lists */
    int cull;                 /* 1 (default) wave-level strip culling in the blend kernels */
    int lpt;                  /* 1 (default) heaviest-tile-first launch order of the blend kernels */
    int speculative;          /* 1 (default) enqueue binning + blend before num_rendered is read back */
    int fwd_pixels_per_lane;  /* 0 auto (default), 1 / 2 / 4 */
    int bwd_pixels_per_lane;  /* 0 auto (default), 1 / 2 / 4 */
    int sh_grad_factors;      /* backward: dL_dsh receives the [P][3] factor, see gsrast_sh_grad_combine */
    int side_stream;          /* 1 (default) forward: the colour kernel (SH -> RGB) runs on a stream of the context, forked off
                                 `stream` at entry and joined in front of the blend, beside the depth sort and the binning, and the
                                 zero-fill of the gradient records follows on it under the blend (joined before the call returns);
                                 backward: the SH view-direction derivatives are evaluated on the calling thread's context stream
                                 beside the blend backward, joined in front of the per-Gaussian backward.
                                 0 = everything on `stream` */
    int grads_zeroed;         /* backward: 1 = no backward has run on this forward's geometry buffer yet (the forward leaves the
                                 gradient records zero), so the 64 B / Gaussian zero-fill is skipped; 0 (default) = fill */
    int backward_phase;       /* backward: 0 (default) everything; 1 = the blend backward only (fills the gradient records and, with
                                 sh_grad_factors, writes the factors: all a multi-GPU caller needs to START its exchange); 2 = the
                                 per-Gaussian backward only (the rest of the outputs).  1 then 2 on the same arguments == 0 */
    int depth_sort;           /* forward: 0 (default) bucket depth sort -- two launches: Gaussians into ~P/256 depth buckets, one LDS sort per
                                 bucket (run-compressed binning, P >= 32768); a scene whose depths pile up in one bucket is detected on
                                 the device and re-sorted by the radix passes, which the context then uses for its next 16 calls
                                 ("bucket_skip"; doubling with every further overflow, up to 4096); 1 = always the LSD radix sort (3-4 passes of three launches).  Same order either way */
    int forward_only;         /* forward: 1 = no backward will follow on this call's state (evaluation / torch.no_grad()): the colour kernel
                                 does not store d(colour)/d(view direction) (36 B / Gaussian) for the backward.  A backward on such a
                                 state must be given forward_only = 1 as well; it then evaluates those derivatives itself
                                 (sh_dir_derivs_kernel, re-reading the SH blocks).  0 (default) = the forward prepares them */
    int no_order_hint;        /* forward: 1 = do not use / update the context's launch-order hints.  By default a context remembers, per device and
                                 camera pose (hash of the view and projection matrices and the image size; 256 poses, least recently used
                                 replaced; device memory, 6 B per tile and pose with the cut depths of no_list_cut below), how deep every tile's list was consumed the last time
                                 that pose was rendered, and starts the forward blend's heaviest tiles first by it -- the list length, the
                                 only estimate a first-seen pose has, is a poor one in occluded scenes.  Results never depend on it */
    int dense_backward;       /* backward: 1 = the per-Gaussian backward reads every Gaussian's inputs (round 2's form).  0 (default): a
                                 Gaussian whose gradient record is all zero (frustum-culled, or occluded: its gradient IS zero) gets its
                                 zero rows written without its inputs being read */
    int no_list_cut;          /* forward: 1 = always bin every Gaussian.  0 (default): LIST CUT -- with the launch-order hints a context also
                                 remembers, per pose and tile, a cut depth (that of the list entry 1.5 x as deep as the deepest one any pixel
                                 of the tile consumed the last time; none for a tile whose pixels did not all saturate).  The next forward of
                                 that pose gives column runs only to the Gaussians in front of the cut depth of some tile they cover -- in an
                                 occluded scene a few per cent of them -- and VERIFIES the speculation on the device: a tile's list counts
                                 as ending at its cut depth, and if some pixel of a cut tile is not saturated there, the whole binning and
                                 blend run again over all Gaussians (enqueued behind the blend in any case, every kernel predicated on the
                                 verdict).  Results never depend on it; needs tile_clip = 1 and the bucket depth sort.  It is
                                 applied where it pays: when the context's last forward had at least 1.5 M column runs, and not for the next 64
                                 forwards after one in which it removed fewer than that (gsrast_set_option("list_cut_always", 1) lifts both) */
} gsrast_options;
void gsrast_options_init(gsrast_options* options);   /* fills in the built-in defaults listed above */
/* A context may be used by one host thread at a time (it owns one side stream and one set of fork / join events per device, and -- per
 * device it has rendered on -- 6 bytes per tile and pose of device memory (12.5 MB at 1080p, 50 MB at 4K): the pose table of options.no_order_hint / no_list_cut); contexts are
 * independent of each other.  Destroy it only after the calls that used it have returned (gsrast_context_destroy frees the device
 * memory, which waits for the device). */
typedef struct gsrast_context gsrast_context;
gsrast_context* gsrast_context_create(void);
void gsrast_context_destroy(gsrast_context* ctx);
/* "last_late" (Gaussians the list cut left without column runs in the context's last forward call), "last_early_runs" (column runs of the others),
 * "cut_pause" (forwards the list cut still sits out: it saved too little, or its lists kept turning out too short), "cut_fallbacks" (forwards on the
 * current device whose cut lists turned out too short and were redone from the full lists; this query waits for the device),
 * "last_instances" (num_rendered), "last_runs" (column runs) of the context's last forward call, "redo_count"
 * (speculative launches / depth sorts that had to be repeated), "bucket_skip" (forwards that will still go straight to the radix
 * depth sort after a bucket overflow); ctx NULL = the calling thread's context. */
int gsrast_context_query(const gsrast_context* ctx, const char* name);
/* Round 5: also "completion_passes" (completion passes of the list cut the device has reported to this context), "cut_margin_x4" (the remembered
 * cut's margin in quarters: 6 = 1.5 x), "tau_req" / "tau_force" (the predicted cut's requirement / forwards that still use predicted cut depths for
 * every pose), "gate_inline_calls".
 *
 * The host-side decisions of a context (csrc/gsrast_policy.h: when the list cut is applied, paused and widened; how the speculative launch is
 * sized; when the bucket depth sort backs off) can be driven WITHOUT a device -- a context that never renders touches no GPU.  One event per call, the return value is the
 * decision (or GSRAST_E_ARG for an unknown event):
 *   "begin"  (a = Gaussians P, b = column runs of the previous forward, c = 1: option list_cut_always) -> 1: the cut pays for this forward; 0: it sits out
 *   "counts" (a = all column runs Q, b = early column runs, c = bit 0: predicted cut depths available, bit 1: some Gaussian was late; P = the last "begin"'s) -> forwards of pause now pending
 *   "pass"   (a = column runs of the completion pass's candidates, b = column runs of the forward, c = 1: predicted cut depths available) -> the pass's points (0 ... 8)
 *   "clean"  (a cut forward behind which no pass was reported) -> the score
 *   "size"   (a = early-run hint, b = capacity in column runs, c = 1: an early set is expected) -> column runs the launches over the cut lists are sized for
 *   "grow"   (a = count) -> the capacity requested for it;   "follow" (a = hint, b = this forward's count, c = shift) -> the next hint
 *   "get"    (a = 0 pause, 1 score, 2 margin x 4, 3 tau_req, 4 tau_force, 5 length of the last fallback pause; the bucket depth sort's back-off:
 *            6 "bucket_skip", 7 length of its last pause, 8 bucket-sorted forwards without an overflow since, at most 1024)
 *   "depth_sort" (a forward's outcome for the bucket depth sort's back-off -- a = 0: it went to the radix sort although the bucket sort was asked for;
 *            1: bucket-sorted without overflow; 2: a bucket overflowed, b = 1: the depth histogram's table was a learned one that held every key) -> "bucket_skip"
 *   "zrange" (a = first | last << 16 occupied bin of the depth histogram a forward filled with the context's current table) -> the next table's
 *            shift, | 256 if the current table was a learned one that held every key;   "zget" (a = 0 klo / 256, 1 shift, 2 khi / 256)
 *   "reset"  (fresh policies, the back-off's included: tests);   "tau_min" (a = the predicted cut's requirement and its floor: experiments)
 * ctx NULL = the calling thread's context. */
int gsrast_policy_event(gsrast_context* ctx, const char* what, int a, int b, int c);
/* The forward's host-side plan (csrc/gsrast_policy.h: ForwardPlan) WITHOUT a device: what a forward with these options, flags and shape would decide
 * on a context whose remembered words are words[6] = { bucket_skip, R_hint, last_Q, depth_short, (1: SH coefficients) | (2: colors_precomp) | degree << 4,
 * 1: the pose table was acquired }, under the process-wide switches in force (gsrast_set_option) and ctx's cut policy.  Returns GSRAST_E_ARG (the
 * forward's own refusal in gsrast_last_error) or the decisions as bits: 0 run-compressed binning, 1 work buckets, 2 bucket depth sort, 3 its two-launch
 * scatter, 4 culled blend kernel, 5 heaviest tiles first, 6 launch-order hints wanted, 7 list cut's base condition, 8 predicted-cut mode, 9 records
 * zeroed in the blend, 10 only touched records zeroed, 11 untouched bits kept, 12 tile clip, 13 SH direction derivatives, 14 speculative launch
 * eligible, 15 adaptive radix sort, 16 three passes assumed, 17 the cut pays, 18 the list cut is applied.  ctx NULL = the calling thread's context. */
int gsrast_debug_forward_plan(gsrast_context* ctx, const gsrast_options* options, unsigned flags, int P, int W, int H, const int* words);
/* The backward's host-side plan (csrc/gsrast_policy.h: BackwardPlan) WITHOUT a device: what a backward with these options and flags would decide for
 * words[7] = { P, D, R, width, height, (1: a GSRAST_FAMILY_RAW record) | (2: SH coefficients) | (4: colors_precomp) | (8: cov3D_precomp) | (16: dL_dacc_depth or
 * dL_dalpha given), 1: the context's side stream can be had }, under the process-wide switches in force (gsrast_set_option).  Returns GSRAST_E_ARG (the
 * backward's own refusal in gsrast_last_error) or the decisions as bits: 0 aux gradients, 1 anti-aliased state, 2 blend phase, 3 per-Gaussian phase, 4 gradient
 * records zero-filled, 5 sh_dir_derivs runs, 6 ... on the side stream, 7 late fill wanted, 8 late fill (late_rows_zero on the side stream), 9 its kernel skipped
 * ("ablate" 3), 10 side stream joined BEHIND preprocess_bwd, 11 the blend backward runs, 12 culled, 13 transposed, 14 its aux instantiation, 15 launch order from
 * the work buckets, 16 from tile_order, 17 sh_factor runs, 18 preprocess_bwd leaves dL_dsh to it, 19 sparse preprocess_bwd, 20 grouped; bits 21-23 pixels per
 * lane (1 / 2 / 4), 24-25 the "ablate" blend kernel (0 / 1 / 2), 26-27 "mutate", 28 pose sums (GSRAST_RENDER_POSEGRAD).  words[5] also takes 32: a
 * record whose struct_size covers the pose fields (all four flag bits known), 64: its dL_dcamera given, 128: its pose_scratch given, 256: its dL_dmean2D_abs
 * given -- without 32 the plan stands for a GSRAST_BACKWARD_CALL_MIN record, which knows only GSRAST_RENDER_AUX | GSRAST_RENDER_ANTIALIAS.  grids (may be NULL) receives { sh_dir_derivs' grid, preprocess_bwd's grid } (0: not launched). */
int gsrast_debug_backward_plan(const gsrast_options* options, unsigned flags, const int* words, int* grids);

/* ---- Differentiable alpha and accumulated depth (no counterpart in the reference, whose only depth output is the median depth
 * above, whose gradient it drops) ----
 * With GSRAST_RENDER_AUX (the flags and the call records below) the forward also writes, for every pixel, over the same contributors and the
 * same early stop as the colour:
 *     out_acc_depth [1][H][W] = sum_i alpha_i T_i z_i     z_i = Gaussian i's view-space depth; the background adds nothing; NOT normalised
 *                                                        (expected depth = acc_depth / alpha, left to the caller)
 *     out_alpha     [1][H][W] = 1 - T_final
 * Both must be non-NULL.  Everything else it computes and leaves in the state buffers is what the forward without the bit computes.
 * The backward with the bit takes the upstream gradients dL_dacc_depth / dL_dalpha [1][H][W]; either may be NULL (= zero),
 * with both NULL it is the backward without the bit (the options->cull rule below is checked first).  The gradients reach the same outputs as the colour's (means3D through the view-space
 * depth as well, means2D, opacities, scales / rotations or cov3D; the raw leaves on the raw pair) with the colour's conventions (the 0.99
 * clamp passes gradients through).  The backward rebuilds the depth recurrence from final_T and n_contrib back to front, as the colour's:
 * it needs nothing of the forward's aux outputs, so an aux backward on the state of a forward without the bit is valid.  With
 * options->backward_phase, pass the same two pointers to both phases.
 * The same holds for the raw family below.
 * Only the default culled blend kernels have the aux outputs: options->cull == 0 (and, forward, fwd_pixels_per_lane != 0) return
 * GSRAST_E_ARG.  The aux backward always runs the one-pixel-per-lane transposed blend backward, whatever bwd_pixels_per_lane says (the
 * automatic choice would take two pixels per lane from 8 192 tiles, 4K images, on).  Argument errors return before any device work. */

/* Process defaults of the options above (and process-wide diagnostics): "exp_mode" 0 = fixed-sequence exp (bit-reproducible vs the CPU oracle), 1 = libm-grade
 * expf, 2 = hardware v_exp_f32;  "profile" = bit mask of kernel ids (gsrast_profile_kernel_name) whose launches are bracketed
 * with HIP events on the launch stream, -1 = all, 0 = off;
 * "debug_sync" 0/1 = synchronise + check errors after every launch;
 * "binning" 0 = run-compressed binning (default), 1 = instance-level two-pass radix sort;
 * "tile_clip" 1 (default) = with "binning" 0, a Gaussian is listed only in the tiles its alpha >= 1/255 ellipse can
 * reach instead of every tile of its 3-sigma square (outputs bit-identical, the internal lists get shorter;
 * num_rendered keeps the reference's meaning), 0 = the reference's literal lists;
 * "cull" / "lpt" 0/1 = wave-level strip culling / heaviest-tile-first launch order in the blend kernels;
 * "pixels_per_lane" (+ "fwd_" / "bwd_" prefixed) 0 = auto, 1 / 2 / 4.  Returns 0 or GSRAST_E_ARG.
 * "speculative" 1 (default) = binning + forward blend are enqueued before the host has read num_rendered back, against
 * a capacity remembered from earlier calls (repeated with exact sizes if it did not fit), 0 = wait first;
 * "sh_grad_factors" see gsrast_sh_grad_combine;
 * "bwd_transposed" (process-wide A/B switch) 1 (default) = the one-pixel-per-lane backward blend sums across lanes once per
 * group of eight staged instances (blend_bwd_cull_t_kernel), 0 = nine wave reductions per surviving (wave, instance) pair.
 * "chain_gate" (process-wide A/B switch) 1 (default) = the list cut's completion pass (no_list_cut above) is enqueued on the context's
 * second stream and the caller's stream is released by the cut forward's blend itself (hipStreamWaitValue32 on a word of the
 * context's own), 0 = its predicated launches on the caller's stream (also chosen by itself when the process runs under a counter-collecting
 * profiler -- ROCPROF_COUNTERS / ROCPROF_COUNTER_GROUPS in the environment: such a profiler serialises kernels, a stream that waits for another deadlocks);
 * "list_cut_always" 1 = the cut also where it does not pay;
 * Round 5 (process-wide A/B switches, default 1): "tau_cut" = cut depths PREDICTED from the call's own opacity mass for a pose without remembered
 * ones;  "touch_bits" = the forward blend keeps one "no pixel consumed it" bit per Gaussian for the backward;  "sparse_grec" = such a forward
 * zeroes only the consumed Gaussians' gradient records instead of all P (the backward takes every other record for zero);
 * "late_fill_min_p" (default 750000): scenes of at least that many Gaussians write the untouched Gaussians' zero rows beside the blend backward.
 * gsrast_get_option answers for every name gsrast_set_option accepts (the value stored: a flag reads 0 / 1, a clamped word its clamped value).
 * Read-only through gsrast_get_option: "last_instances" (num_rendered) and "last_runs" (column runs) of the
 * last forward call of the CALLING THREAD's context, "redo_count" (= gsrast_context_query(NULL, name)). */
int gsrast_set_option(const char* name, int value);
int gsrast_get_option(const char* name);

/* Per-kernel device timing gathered while "profile" is 1 (HIP events on the launch stream).
 * gsrast_profile_collect() synchronises outstanding events and folds them into the totals. */
int gsrast_profile_kernel_count(void);
const char* gsrast_profile_kernel_name(int kernel_id);
int gsrast_profile_collect(void);
int gsrast_profile_read(int kernel_id, double* total_ms, long long* launches);
void gsrast_profile_reset(void);

/* ---- "next" row of the scope table: the photometric loss right after the rasterizer ----
 * loss = (1 - lambda_dssim) * mean|img - gt| + lambda_dssim * (1 - mean(SSIM_map(img, gt)))
 * Replaces the pair l1_loss / ssim of the reference's utils/loss_utils.py:18-19, :38-68 as combined in
 * helper_train.py:50-53 (5 depthwise 11x11 convolutions forward, autograd through them backward) by one fused
 * forward and one fused backward kernel.  img, gt: [C][H][W] planar fp32 in HBM.
 * forward : out3 (device, 3 floats) = {loss, l1, ssim}; scratch keeps three derivative maps for the backward.
 * backward: dL_dimg [C][H][W] = dL_dloss * d loss / d img  (dL_dloss: device scalar, NULL means 1). */
size_t gsrast_loss_scratch_bytes(int C, int H, int W);
int gsrast_loss_forward(int C, int H, int W, const float* img, const float* gt, float lambda_dssim,
                        float* out3, char* scratch, void* stream);
int gsrast_loss_backward(int C, int H, int W, const float* img, const float* gt, float lambda_dssim,
                         const float* dL_dloss, const char* scratch, float* dL_dimg, void* stream);

/* ---- "next" row, rank 3: the activation / deformation epilogue that produces the rasterizer's inputs ----
 * Replaces the tail of get_deformation, scene/saro_gaussian.py:807-847 with the activations of :39-47:
 *   motion = xyz + motion_res;  rot = normalize(rotation + rot_res[:, :4]);  scale = exp(scaling + rot_res[:, 4:]);
 *   opacity = sigmoid(opacity_logit) * trbf;  shs = cat(features_dc [P][1][3], features_rest [P][M-1][3]) + shs_res [P][M][3]
 * motion_res, rot_res ([P][7]), trbf and shs_res may each be NULL (static stage: plain activations).
 * backward: upstream d_rot [P][4], d_scale [P][3], d_opacity [P] (NULL = zero) -> d_rotation [P][4], d_scaling [P][3],
 * d_rot_res [P][7] (NULL ok), d_opacity_logit [P], d_trbf [P] (NULL ok).  The other gradients need no kernel:
 * d_xyz = d_motion_res = d_motion; d_features_dc / d_features_rest are slices of d_shs, d_shs_res = d_shs.
 * rotation, rot, d_rot and d_rotation are accessed as float4: GSRAST_E_ARG unless they are 16-byte aligned. */
int gsrast_activate_forward(int P, int M, const float* xyz, const float* motion_res, const float* rotation,
                            const float* rot_res, const float* scaling, const float* opacity_logit, const float* trbf,
                            const float* features_dc, const float* features_rest, const float* shs_res,
                            float* motion, float* rot, float* scale, float* opacity, float* shs, void* stream);
int gsrast_activate_backward(int P, const float* rotation, const float* rot_res, const float* scale, const float* opacity_logit,
                             const float* trbf, const float* d_rot, const float* d_scale, const float* d_opacity,
                             float* d_rotation, float* d_scaling, float* d_rot_res, float* d_opacity_logit, float* d_trbf,
                             void* stream);

/* ---- rank 3 as SURVEY.md 8f wrote it: the epilogue FUSED INTO the per-Gaussian kernels (K1 / K7) ----
 * A GSRAST_FAMILY_RAW call record (below) is a render call taking the model's RAW leaves
 * (scene/saro_gaussian.py:306-319: _xyz, _rotation, _scaling, _opacity, _features_dc, _features_rest) and the optional deformation
 * residuals of get_deformation (:807-847) instead of activated attributes: the activations above run in registers inside
 * preprocess_fwd / preprocess_color, the chain rule inside preprocess_bwd, and the [P][M][3] coefficient tensor
 * (cat(dc, rest) + residual: 192 B / Gaussian written by the model and re-read by the rasterizer, and back) is never materialised.
 * The rasterizer's outputs and state are bit-identical to gsrast_activate_forward followed by the dense forward.
 * The reference-shaped entry points are untouched; this family is additional.  M in {4, 16}; rotation, features_dc, features_rest,
 * shs_res and the matching gradient arrays 16-byte aligned.  NULL = absent optional residual. */
typedef struct gsrast_raw_inputs {
    const float* xyz;             /* [P][3]  _xyz */
    const float* motion_res;      /* [P][3]  or NULL: means3D = xyz + motion_res */
    const float* rotation;        /* [P][4]  _rotation (not normalised) */
    const float* rot_res;         /* [P][7]  or NULL: [:, :4] added to rotation, [:, 4:] to scaling, before the activations */
    const float* scaling;         /* [P][3]  _scaling (log scale) */
    const float* opacity_logit;   /* [P]     _opacity */
    const float* trbf;            /* [P]     or NULL: opacity = sigmoid(logit) * trbf */
    const float* features_dc;     /* [P][1][3] */
    const float* features_rest;   /* [P][M-1][3] */
    const float* shs_res;         /* [P][M][3] or NULL */
} gsrast_raw_inputs;
typedef struct gsrast_raw_grads {   /* every array is fully overwritten */
    float* dL_dmean2D;            /* [P][3]  screen-space gradient (densification statistic), .z = 0 */
    float* d_xyz;                 /* [P][3]  = the gradient of motion_res too */
    float* d_rotation;            /* [P][4] */
    float* d_scaling;             /* [P][3] */
    float* d_rot_res;             /* [P][7]  or NULL ({d_rotation, d_scaling} side by side) */
    float* d_opacity_logit;       /* [P] */
    float* d_trbf;                /* [P]     or NULL */
    float* d_features_dc;         /* [P][1][3]    } may both be NULL when d_shs_res is given (its rows are [dc | rest]); given together with it, */
    float* d_features_rest;       /* [P][M-1][3]  } the rows are written twice -- cheaper than slicing them out afterwards */
    float* d_shs_res;             /* [P][M][3] or NULL; requires shs_res */
    float* d_sh_factor;           /* [P][3] or NULL (round 4, multi-GPU): the FACTOR of the SH leaves' gradient (gsrast_sh_grad_combine) instead of
                                     its 48 products per Gaussian -- d_features_dc / d_features_rest may then be NULL and are not written (the caller
                                     completes them with gsrast_sh_grad_combine_rows after the exchange); not together with shs_res / d_shs_res, whose
                                     gradient every rank needs whole for its own view */
} gsrast_raw_grads;

/* ---- Render flags: the `flags` word of a call record (below) selects every combination of the optional render features ----
 *   flags = 0                        the plain render (the aux pointers are ignored)
 *   GSRAST_RENDER_AUX                the aux outputs / gradients above (outputs non-NULL, gradients either NULL)
 *   GSRAST_RENDER_ANTIALIAS          the 2-D Mip filter of Mip-Splatting (Yu et al., CVPR 2024), upstream 3DGS's `antialiasing`: every
 *                                    Gaussian's 2-D covariance keeps the 0.3 px^2 dilation, and its opacity is scaled by
 *                                        comp = sqrt(max(0.000025, rho)),   rho = det(cov2D) / det(cov2D + 0.3 I)     (cov2D before the dilation)
 *                                    so that the dilation does not inflate the energy of small or distant Gaussians.  o * comp replaces the opacity
 *                                    in every downstream use (blend, median depth, acc_depth / alpha, the skip threshold, the list cut); conic,
 *                                    radius, means2D, depths and tiles are unchanged.  The backward adds the opacity's dependence on the covariance
 *                                    (zero where rho sits on the floor) and scales dL/dopacity by comp.
 * The backward must get the same GSRAST_RENDER_ANTIALIAS bit as the forward that filled the state (the state does not record it).  With
 * options->backward_phase, pass the same flags to both phases.
 * GSRAST_E_ARG before any device work: unknown bits; GSRAST_RENDER_AUX with options->cull == 0; forward, GSRAST_RENDER_AUX with a NULL aux output.
 * One set of checks, one error text per condition, whichever entry point the call came through. */
#define GSRAST_RENDER_AUX        0x1u
#define GSRAST_RENDER_ANTIALIAS  0x2u

/* ---- Absolute screen-space gradient: the densification statistic of AbsGS (Ye et al., 2024), gsplat's `absgrad` ----
 * dL_dmean2D[i] is the SIGNED sum over pixels of each pixel's gradient with respect to Gaussian i's projected centre: a large Gaussian
 * that half of its pixels pull one way and half the other gets a gradient near zero and is never split.  With GSRAST_RENDER_ABSGRAD the
 * backward also writes
 *     dL_dmean2D_abs[i][k] = sum over pixels p of | d(sum_c dL_dpix[c][p] colour[c][p]  (+ the aux terms of GSRAST_RENDER_AUX)) / d mean2D[i][k] |,  k = 0, 1
 * in the units of dL_dmean2D (the reference's normalised device coordinates: a pixel offset times 0.5 W, 0.5 H), so that
 * dL_dmean2D_abs[i][k] >= |dL_dmean2D[i][k]|, with equality when every pixel pulls the same way.  [P][2] floats, fully overwritten like every
 * other output: zero for every Gaussian whose dL_dmean2D row is zero because no pixel consumed it.  Densification thresholds for it are the
 * caller's choice and are higher than for the signed gradient (AbsGS: about 2x).
 * The sink is the field dL_dmean2D_abs of gsrast_backward_call; without the bit (and with a NULL sink) the call is the one without the
 * field.  The bit belongs to backward records whose struct_size covers that field: a shorter record, and every forward, refuses it as an
 * unknown bit (mask it off the flags word given to the forward).  With
 * options->backward_phase, pass the bit and the sink to both phases.  No other output changes with it.
 * GSRAST_E_ARG before any device work, one text each: the bit with a NULL sink; a sink without the bit; the bit on a record too short for
 * the sink (unknown bit); the bit where the transposed blend backward would not run (options->cull == 0, the ablation kernels) -- the rule of
 * GSRAST_RENDER_AUX.  Like GSRAST_RENDER_AUX it selects the transposed blend backward whatever the pixels per lane say. */
#define GSRAST_RENDER_ABSGRAD    0x4u

/* ---- Camera-pose gradients: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos (gsplat's gradients on `viewmats`; the pose-optimising 3DGS forks) ----
 * viewmatrix [4][4], projmatrix [4][4] and campos [3] are three INDEPENDENT inputs, as they are passed: a caller that composes them
 * (projmatrix = viewmatrix @ projection, campos = inverse(viewmatrix)[3][:3]) chains through its own composition.  Storage is row-vector,
 * transposed: t = [mean, 1] @ viewmatrix, hom = [mean, 1] @ projmatrix.  With GSRAST_RENDER_POSEGRAD the backward also writes
 *     dL_dcamera[35] = dL_dviewmatrix[16] | dL_dprojmatrix[16] | dL_dcampos[3]      (row-major like the inputs, fully overwritten)
 * -- the gradient of the function every other output of this backward differentiates, with its conventions (the 0.99 alpha clamp straight-through,
 * no gradient through the median depth, a frustum-clamped t.x / t.y a constant inside the Jacobian, det^2 / (det^2 + 1e-7) in the conic chain):
 *   viewmatrix: through the view-space mean (the accumulated depth of GSRAST_RENDER_AUX included) and through the rotation inside T = J W;
 *   projmatrix: through means2D, ndc = hom.xy / (hom.w + 1e-7): columns 0, 1 and 3;
 *   campos:     through the SH view direction: minus the sum of the direction part of dL_dmean3D.
 * Column 3 of dL_dviewmatrix and column 2 of dL_dprojmatrix are exactly zero (the forward never reads them), dL_dcampos is exactly zero with
 * colors_precomp or SH degree 0.  tan_fovx / tan_fovy (the focal lengths inside the Jacobian) are not differentiated.
 * Every workgroup of the per-Gaussian backward reduces its Gaussians' terms and writes one row of partial sums to pose_scratch
 * (gsrast_pose_scratch_bytes(P) bytes, 16-byte aligned, the caller's; no state buffer grows); a one-workgroup kernel adds the rows in a fixed order
 * in fp64.  No atomics: the same gradient records give the same bits.  No other output changes with the bit.
 * dL_dcamera and pose_scratch are the last two fields of gsrast_backward_call; without the bit (and with both NULL) the call is the one
 * without them.  The bit belongs to backward records whose struct_size covers them: a shorter record, and every forward, refuses it as an
 * unknown bit.  With options->backward_phase, pass the bit and both pointers to both phases: dL_dcamera is written by phase 2 (or by phase 0).
 * GSRAST_E_ARG before any device work, one text each: the bit on a record too short for the fields ("flags: unknown bits"); the bit with a NULL dL_dcamera;
 * the bit with a NULL pose_scratch; dL_dcamera or pose_scratch without the bit. */
#define GSRAST_RENDER_POSEGRAD   0x8u
size_t gsrast_pose_scratch_bytes(int P);

/* ---- The render calls: one versioned call record per direction ----
 * Every render feature is a FIELD of these records and a bit of `flags`, not a symbol.  gsrast_render_forward / gsrast_render_backward take
 * the per-call options and context (Reentrancy, above) and one record; gsrast_forward / gsrast_backward at the top are the same calls on a
 * dense record with flags = 0, NULL options and NULL context.  The fields have the meaning of the equally named arguments of that pair.
 *   family  GSRAST_FAMILY_DENSE: the dense arrays (and the dense gradient outputs); `raw` / `raw_grads` must be NULL.
 *           GSRAST_FAMILY_RAW:   `raw` (and `raw_grads`); the dense arrays and dense gradient outputs must be NULL, prefiltered 0.
 * How the records grow.  The caller sets struct_size = sizeof(the record) of the header it was compiled against.  A record is accepted when
 * GSRAST_*_CALL_MIN <= struct_size <= sizeof of the library's own; the library copies struct_size bytes into a zeroed record of its own, so
 * fields the caller's header did not have are NULL.  A flag bit whose fields lie beyond struct_size is an UNKNOWN bit, refused like any
 * other ("flags: unknown bits").  A later feature appends its fields behind the earlier ones; nothing in front ever moves.
 * GSRAST_E_ARG before any device work: a NULL `call`, a struct_size outside that range, an unknown family, a pointer of the other family. */
#define GSRAST_FAMILY_DENSE 0
#define GSRAST_FAMILY_RAW   1
typedef struct gsrast_forward_call {
    size_t struct_size;      /* sizeof(gsrast_forward_call) of the header the caller was compiled against */
    unsigned flags;          /* GSRAST_RENDER_* */
    int family;              /* GSRAST_FAMILY_* */
    gsrast_alloc_fn geometry_alloc; void* geometry_ctx;
    gsrast_alloc_fn binning_alloc; void* binning_ctx;
    gsrast_alloc_fn image_alloc; void* image_ctx;
    int P, D, M;
    const float* background;
    int width, height;
    const float* means3D;
    const float* shs;
    const float* colors_precomp;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    const gsrast_raw_inputs* raw;
    float scale_modifier;
    const float* viewmatrix;
    const float* projmatrix;
    const float* cam_pos;
    float tan_fovx, tan_fovy;
    int prefiltered;
    float* out_color;
    float* out_depth;
    int* radii;
    void* stream;
    float* out_acc_depth;    /* GSRAST_RENDER_AUX */
    float* out_alpha;
} gsrast_forward_call;
typedef struct gsrast_backward_call {
    size_t struct_size;      /* sizeof(gsrast_backward_call) of the header the caller was compiled against */
    unsigned flags;          /* GSRAST_RENDER_* */
    int family;              /* GSRAST_FAMILY_* */
    int P, D, M, R;
    const float* background;
    int width, height;
    const float* means3D;
    const float* shs;
    const float* colors_precomp;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    const gsrast_raw_inputs* raw;
    float scale_modifier;
    const float* viewmatrix;
    const float* projmatrix;
    const float* campos;
    float tan_fovx, tan_fovy;
    const int* radii;
    char* geom_buffer;
    char* binning_buffer;
    char* image_buffer;
    const float* dL_dpix;
    float* dL_dmean2D;
    float* dL_dconic;
    float* dL_dopacity;
    float* dL_dcolor;
    float* dL_dmean3D;
    float* dL_dcov3D;
    float* dL_dsh;
    float* dL_dscale;
    float* dL_drot;
    const gsrast_raw_grads* raw_grads;
    void* stream;
    const float* dL_dacc_depth;   /* GSRAST_RENDER_AUX */
    const float* dL_dalpha;       /* GSRAST_BACKWARD_CALL_MIN ends here */
    float* dL_dmean2D_abs;        /* GSRAST_RENDER_ABSGRAD; GSRAST_BACKWARD_CALL_ABS ends here */
    float* dL_dcamera;            /* GSRAST_RENDER_POSEGRAD: [35] */
    char* pose_scratch;
} gsrast_backward_call;
#define GSRAST_FORWARD_CALL_MIN  sizeof(gsrast_forward_call)
#define GSRAST_BACKWARD_CALL_MIN offsetof(gsrast_backward_call, dL_dmean2D_abs)
#define GSRAST_BACKWARD_CALL_ABS offsetof(gsrast_backward_call, dL_dcamera)
int gsrast_render_forward(gsrast_context* ctx, const gsrast_options* options, const gsrast_forward_call* call);
int gsrast_render_backward(const gsrast_options* options, const gsrast_backward_call* call);

/* Per-Gaussian blend-weight statistics of one finished forward (no counterpart in the reference): what importance-pruning schemes build
 * their masks from -- LightGaussian's hit count and sum of alpha T, RadSplat's max alpha T, Mini-Splatting's dominant-pixel counts.
 *
 * Definition.  For one finished forward, take pixel p inside the image and Gaussian i.  i CONTRIBUTES to p when the forward blended it
 * there: its position in the tile's list in force is below n_contrib[p] and it passed the forward's per-pair tests --
 *     power <= 0 && power >= threshold;  alpha = min(0.99, opacity * exp(power)) >= 1/255;  T * (1 - alpha) >= 1e-4
 * (the terminating entry does not contribute).  Its weight is w_ip = alpha_ip * T_ip, T_ip the transmittance in front of it.
 * m_p = pixel_weights[p] clamped to [0, 1]; without pixel_weights m_p = 1.  A pixel with m_p = 0 counts in no column.  One row per Gaussian:
 *     col 0  weight_sum   sum over p of m_p * w_ip
 *     col 1  weight_max   max over pixels with m_p > 0 of w_ip (unweighted)
 *     col 2  pixel_count  number of pixels with m_p > 0 that i contributes to
 *     col 3  top_count    number of those pixels where w_ip is the largest of the pixel's contributors (first in list order on a tie)
 * Gaussians that nobody consumed -- culled, off screen, late under the list cut, or listed behind every pixel's stop -- get a zero row.
 * It follows that  sum_i col0 = sum_p m_p (1 - T_final[p]),  sum_i col3 = number of pixels with m_p > 0 and at least one contributor,
 * col1 <= 0.99,  col2 >= col3,  col0 <= col1 * col2.
 *
 * The state already carries the opacity the forward blended with (the GSRAST_RENDER_ANTIALIAS compensation included), so the call has no
 * flags; pass the options (exp_mode) of the forward that filled the state (NULL: the process defaults).  The three state buffers are valid
 * for this call after the forward that filled them has been enqueued on `stream` and before a backward on them.  The call replays the
 * blend from that state (csrc/gsrast_contrib.h); every accumulation across waves and tiles is an integer atomic, so the same state gives
 * the same bits on every run.  weight_sum is accumulated in units of 2^-36 (each 64-pixel partial is truncated to that unit); the two counts
 * are stored as float32: exact up to 2^24, rounded above.
 * stats [P][4] float32 is fully overwritten (16-byte aligned).  scratch: gsrast_contrib_scratch_bytes(P) bytes of the caller's (20 bytes
 * per Gaussian, rounded up like every scratch size here; 16-byte aligned); the call zeroes it itself and leaves it zeroed.
 * GSRAST_E_ARG before any device work: P < 0 or R < 0, a zero-size image, and with P > 0 a NULL state buffer (binning_buffer only when R > 0),
 * a NULL stats, a NULL scratch.  P == 0 returns 0 without a launch.  Kernels "contrib_blend" and "contrib_finish" of the profile table. */
size_t gsrast_contrib_scratch_bytes(int P);
int gsrast_contrib_stats(const gsrast_options* options, int P, int R, int width, int height,
                         const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
                         const float* pixel_weights /* [H][W] or NULL */, float* stats /* [P][4] */,
                         char* scratch, void* stream);

/* Per-Gaussian feature vectors blended with the weights of one finished forward, and the gradients of that blend (no counterpart in the
 * reference; gsplat renders `colors` of any width): semantic / language features, decoder features, motion, normals, uncertainty.
 *
 * Definition.  Pair (pixel p, Gaussian i) CONTRIBUTES exactly as defined for gsrast_contrib_stats above; its weight is w_ip = alpha_ip T_ip,
 * with the opacity the state carries (the GSRAST_RENDER_ANTIALIAS compensation included).
 *     feature_map[c][p] = sum over contributing i of w_ip * features[i][c]          (no background term: composite with 1 - alpha of
 *                                                                                    GSRAST_RENDER_AUX if one is wanted)
 * features is [P][C] row-major float32, feature_map [C][H][W] planar; 1 <= C <= GSRAST_FEATURES_MAX_C.  Every pixel of the map is written,
 * 0 where nothing contributes.  The calls have no flags; of the options only exp_mode is read (pass the forward's; NULL: the process
 * defaults).  Both replay the blend from the state (csrc/gsrast_features.h), in passes of up to 32 channels.
 *
 * gsrast_features_forward is valid once the render forward that filled the three state buffers has been enqueued on `stream`.
 *
 * gsrast_features_backward takes dL_dfeature_map [C][H][W] and
 *   - OVERWRITES dL_dfeatures [P][C]:  dL/dfeatures[i][c] = sum_p w_ip dL_dfeature_map[c][p]  (rows of Gaussians nobody consumed: exactly 0);
 *   - ADDS the map's part of the screen-space mean, conic and opacity gradient sums to floats 0-5 of the Gaussians' gradient records
 *     inside geom_buffer, in the units the blend backward writes them (dL/dalpha_ip = T_ip sum_c dL_dfeature_map[c][p] (features[i][c] - A_c),
 *     A_c the blend behind i; the 0.99 clamp passes gradients through).  Nothing else of the record is touched.
 * It is therefore valid only BETWEEN a gsrast_render_backward with options.backward_phase = 1 and one with backward_phase = 2 on the same
 * state and stream: the window in which the records exist and have not been consumed.  The second call's mean, covariance, opacity, scale,
 * rotation (and GSRAST_RENDER_POSEGRAD camera) gradients then include the feature map's loss; dL_dmean2D_abs (GSRAST_RENDER_ABSGRAD) does not.
 *
 * GSRAST_E_ARG before any device work: C outside 1..GSRAST_FEATURES_MAX_C, P < 0 or R < 0, a zero-size image, and with P > 0 a NULL state
 * buffer (binning_buffer only when R > 0); a NULL features, feature_map, dL_dfeature_map or dL_dfeatures; a bad exp_mode.  P == 0: the
 * forward writes a zero map, the backward nothing; neither launches a kernel.  Kernels "features_fwd" and "features_bwd" of the profile table. */
#define GSRAST_FEATURES_MAX_C 64
int gsrast_features_forward(const gsrast_options* options, int P, int R, int C, int width, int height,
                            const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
                            const float* features /* [P][C] */, float* feature_map /* [C][H][W] */, void* stream);
int gsrast_features_backward(const gsrast_options* options, int P, int R, int C, int width, int height,
                             char* geom_buffer /* gradient records: floats 0-5 are ADDED to */, const char* binning_buffer, const char* image_buffer,
                             const float* features /* [P][C] */, const float* dL_dfeature_map /* [C][H][W] */,
                             float* dL_dfeatures /* [P][C], overwritten */, void* stream);

/* The depth-distortion map of one finished forward, and its gradients (no counterpart in the reference): the distortion loss of Mip-NeRF 360
 * that gsplat renders as render_distort (`distloss`) and 2DGS carries in its rasterizer -- the regulariser against floaters and
 * semi-transparent shells.
 *
 * Definition.  Pair (pixel p, Gaussian i) CONTRIBUTES exactly as defined for gsrast_contrib_stats above; its weight is w_i = alpha_i T_i, with
 * the opacity the state carries (the GSRAST_RENDER_ANTIALIAS compensation included); z_i is the view-space depth the state carries (the
 * value acc_depth of GSRAST_RENDER_AUX sums): raw view-space z, gsplat's convention, no near / far or NDC mapping.
 *     distort[p] = sum_i sum_j w_i w_j |z_i - z_j|                   (over the contributors of p; no background term)
 *                = 2 sum_i w_i (z_i A_{i-1} - D_{i-1}),   A_{i-1} = sum_{j<i} w_j,   D_{i-1} = sum_{j<i} w_j z_j
 * The second line is what the kernel evaluates, in list order; it equals the first because every tile list is in non-decreasing z (ties
 * contribute 0 either way).  The quantity does not change under z -> z - z0, and it is evaluated on depths RELATIVE to a tile-uniform z0,
 * the depth of the tile's first listed Gaussian, so that z_i A - D does not cancel against the scene's distance from the camera; the fp32
 * accuracy the tests hold the map to is measured on that association.  Every pixel of the map [H][W] is written, 0 with fewer than two
 * contributors.  The calls have no flags; of the options only exp_mode is read (pass the forward's; NULL: the process defaults).  Both
 * replay the blend from the state (csrc/gsrast_distort.h).
 *
 * gsrast_distortion_forward is valid once the render forward that filled the three state buffers has been enqueued on `stream`.  It also
 * writes moments [2][H][W] = (A_N, D_N), each pixel's totals over all its contributors, D_N relative to the same z0: the backward goes back
 * to front and cannot recover them.  z0 itself is not stored: both calls read it from the head of the tile's list.  The caller keeps
 * moments (2 * H * W floats) for the backward.
 *
 * gsrast_distortion_backward takes moments and g = dL_ddistort [H][W].  With the sums over the contributors k > i behind a pair,
 * SA = sum w_k, SD = sum w_k z_k, SG = sum G_k w_k:
 *     dL/dz_i = 2 g w_i (A_{i-1} - SA)              G_i = dL/dw_i = 2 g (z_i A_{i-1} - D_{i-1} + SD - z_i SA)
 *     dL/dalpha_i = T_i G_i - SG / (1 - alpha_i)    A_{i-1} = A_N - SA - w_i      D_{i-1} = D_N - SD - w_i z_i
 *   - ADDS the screen-space mean, conic and opacity gradient sums that follow from dL/dalpha to floats 0-5 of the Gaussians' gradient
 *     records inside geom_buffer, in the units the blend backward writes them (the 0.99 clamp passes gradients through);
 *   - ADDS sum_p dL/dz_i to float 9 of the record, the dL/d(view-space z) that the per-Gaussian backward consumes only under
 *     GSRAST_RENDER_AUX with a non-NULL aux gradient: a caller without aux gradients passes that flag and a zero dL_dacc_depth on both
 *     phases.  Nothing else of the record is touched.
 * It is therefore valid only BETWEEN a gsrast_render_backward with options.backward_phase = 1 and one with backward_phase = 2 on the same
 * state and stream, like gsrast_features_backward; the two may both run there, in either order: they only add.  dL_dmean2D_abs
 * (GSRAST_RENDER_ABSGRAD) does not include the map's loss.
 *
 * GSRAST_E_ARG before any device work: P < 0 or R < 0, a zero-size image, with P > 0 a NULL state buffer (binning_buffer only when R > 0),
 * a NULL distort_map or moments (forward; backward with P > 0: moments or dL_ddistort), a bad exp_mode.  P == 0: the forward writes a zero
 * map (and zero moments), the backward nothing; neither launches a kernel.  Kernels "distort_fwd" and "distort_bwd" of the profile table. */
int gsrast_distortion_forward(const gsrast_options* options, int P, int R, int width, int height,
                              const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
                              float* distort_map /* [H][W] */, float* moments /* [2][H][W], saved for the backward */, void* stream);
int gsrast_distortion_backward(const gsrast_options* options, int P, int R, int width, int height,
                               char* geom_buffer /* gradient records: floats 0-5 and 9 are ADDED to */, const char* binning_buffer, const char* image_buffer,
                               const float* moments /* [2][H][W] */, const float* dL_ddistort /* [H][W] */, void* stream);

/* Which Gaussians a pixel sees, and with what weight: each pixel's first or heaviest K contributors of one finished forward (no counterpart
 * in the reference; the per-pixel id output many forks of it add, gsplat's rasterize_to_indices_in_range): picking the Gaussian under a
 * cursor, finding the floater that spoils a pixel, lifting 2-D masks or labels by vote, visibility lists for editing.
 *
 * Definition.  Pair (pixel p, Gaussian i) CONTRIBUTES exactly as defined for gsrast_contrib_stats above; its weight is w = alpha * T, with
 * the opacity the state carries (the GSRAST_RENDER_ANTIALIAS compensation included).  For pixel p let c_1 ... c_n be its contributors in
 * blend order (the order of the tile's list: front to back).
 *     count[p] = n
 *     order = 0 ("weight")  slots 0 ... min(K, n) - 1 hold the contributors with the largest w, descending; on equal w the one earlier in
 *                           blend order comes first.  This is the top_count rule of gsrast_contrib_stats: slot 0 is that call's "top"
 *                           Gaussian of the pixel.
 *     order = 1 ("depth")   slots 0 ... min(K, n) - 1 hold c_1 ... c_min(K, n).
 * Unused slots hold id = -1 and weight = +0.0.  Ids are the caller's row numbers 0 ... P - 1.  Nothing is differentiable.
 * ids [K][H][W] int32, weights [K][H][W] float32 and count [H][W] int32 (may be NULL: not wanted) are planar and fully overwritten;
 * 1 <= K <= 16.  The call has no flags; of the options only exp_mode is read (pass the forward's; NULL: the process defaults).  It replays
 * the blend from the state (csrc/gsrast_topk.h), so every w is the forward's own, bit for bit; there are no atomics and every output
 * element has one writer: the same state gives the same bits on every run.  The three state buffers are valid for this call after the
 * forward that filled them has been enqueued on `stream` and before a backward on them.
 * GSRAST_E_ARG before any device work, each with a text of its own: P < 0 or R < 0, a zero-size image, K outside 1..16, order outside
 * {0, 1}, a bad exp_mode, with P > 0 and R > 0 a NULL state buffer, a NULL ids, a NULL weights.  P == 0 or R == 0 (nothing was blended)
 * reads no state: one small launch fills the outputs with -1 / +0.0 / 0.  The launches are not in the profile table. */
int gsrast_pixel_contributors(const gsrast_options* options, int P, int R, int width, int height,
                              const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
                              int K, int order, int32_t* ids, float* weights, int32_t* count /* may be NULL */, void* stream);

/* ---- "next" row, rank 4 (third item): Adam step of the per-Gaussian parameter groups with a PER-ROW learning rate ----
 * Replaces torch.optim.Adam(l, lr=0.0, eps=1e-15, fused=True) for the groups of scene/saro_gaussian.py:306-323 whose
 * 'lr' update_learning_rate (:345-398) sets to lr * inv_intergral, a [P,1] tensor.  One launch for up to 8 groups:
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= (lr_i / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * with lr_i = lr * (lr_rows ? lr_rows[row] : 1).  All tensors fp32, contiguous [rows][width], device pointers. */
typedef struct gsrast_adam_group {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    const float* lr_rows;   /* [rows] or NULL */
    float lr;
    int rows, width;
} gsrast_adam_group;
int gsrast_adam_step(int n_groups, const gsrast_adam_group* groups /* host array */, double beta1, double beta2, double eps,
                     int step /* 1-based */, void* stream);   /* betas in fp64: (1 - 0.999f) would be off by 1.3e-5 relative */
/* The same step for the rows a view saw -- what upstream 3DGS ships as SparseGaussianAdam(params, visibility, N), gsplat as SelectiveAdam and
 * PyTorch as torch.optim.SparseAdam.  visible: [rows] on the device, visible_elem_bytes 1 (bool / uint8: non-zero = visible) or 4 (int32:
 * > 0 = visible, so that a render's radii can be passed as it is).  A visible row gets exactly gsrast_adam_step's update (an all-true mask
 * reproduces it bit for bit); an invisible row keeps param, exp_avg and exp_avg_sq bit for bit, and neither its grad nor its lr_rows entry is
 * read (NaN / Inf there reach nothing).  `step` is the caller's one global count: it advances with every step, masked or not, so a row first
 * seen late is bias-corrected with the global t, not as if it were its first step (torch.optim.SparseAdam's and gsplat's choice).
 * One launch (profile name "adam_step_visible"): a wave takes 64 consecutive rows of a group and leaves at once when none is visible.
 * Refused before any device call (gsrast_last_error): what gsrast_adam_step refuses, visible_elem_bytes other than 1 or 4, rows < 0, a group
 * whose rows differ from `rows` or whose width exceeds 2^24, NULL visible with rows > 0.  rows == 0 or no groups: nothing is launched. */
int gsrast_adam_step_visible(int n_groups, const gsrast_adam_group* groups /* host array */, const void* visible, int visible_elem_bytes /* 1 or 4 */,
                             long long rows, double beta1, double beta2, double eps, int step /* 1-based */, void* stream);

/* ---- densification: clone / split / prune of every per-Gaussian array with its Adam moments, on the device ----
 * Replaces scene/saro_gaussian.py:705-736 densify_pruneclone with :685-701 densify_and_clone, :646-682 densify_and_splitv2,
 * :577-593 prune_points and the optimizer surgery of :555-617 (_prune_optimizer, cat_tensors_to_optimizer).  For Gaussian i < P:
 *   g_i    = accum_i / denom_i (NaN -> 0) [* grad_scale_i]             (accum == NULL: g_i = 0)
 *   smax_i = max_k exp(scaling[i][k])
 *   pruned = prune_src[i] != 0 (if given)  or  sigmoid(opacity_logit[i]) < min_opacity (if min_opacity > 0)
 *   clone  = g_i >= grad_threshold and smax_i <= size_threshold;   split = g_i >= grad_threshold and smax_i > size_threshold
 * grad_threshold must be > 0; +inf selects nothing ("prune only"; accum / denom / scaling may then be NULL).  Output rows:
 *   [ originals !split && !pruned | clones of clone && !pruned | split copy 0 of split && !pruned | copy 1 | ... | copy N-1 ]
 * each part in index order -- what the reference's clone, split, remove-the-sources, prune sequence leaves when the copies inherit their
 * source's prune flag.  counts[5] = { n_kept, n_clone, n_split, n_split_all, P' = n_kept + n_clone + N * n_split } (device memory);
 * n_split_all counts every split-selected source, pruned or not: copy k of source i reads noise[k * n_split_all + rank_all(i)], so a
 * caller who draws randn(N * n_split_all, 3) consumes its generator as torch.normal at :662 does.
 * gsrast_densify_plan classifies and scans (no atomics); the caller reads `counts` back -- the one synchronisation --, allocates
 * the P' rows and hands the counts to gsrast_densify_apply with the same P, N and scratch (>= gsrast_densify_scratch_bytes(P)).
 * The apply moves up to 16 groups in ONE launch.  A group: src [P][width] -> dst [P'][width], width in [1, 64]; with moments
 * (src_m -> dst_m, src_v -> dst_v; each optional) kept originals gather their rows bit for bit, clones and split copies get zeros.
 * Roles: COPY -- every row is a bit copy of its source; XYZ (width 3) -- a split copy is xyz + R(q / |q|) (noise * exp(scaling)), R as
 * utils/general_utils.py:127-148 build_rotation over `rotation` [P][4] raw (r, x, y, z); SCALING -- a split copy is
 * log(exp(scaling) / (0.8 N)).  `scaling` [P][3] raw.  A group without moments carries per-Gaussian extras through a prune.
 * Deterministic: the same bits on every run and every rank.  P = 0 and P' = 0 are valid. */
#define GSRAST_DENSIFY_COPY 0
#define GSRAST_DENSIFY_XYZ 1
#define GSRAST_DENSIFY_SCALING 2
typedef struct gsrast_densify_group {
    const float *src, *src_m, *src_v;   /* [P][width]; src_m / src_v NULL: no moments */
    float *dst, *dst_m, *dst_v;         /* [P'][width] */
    int width, role;
} gsrast_densify_group;
size_t gsrast_densify_scratch_bytes(int P);
int gsrast_densify_plan(int P, int N /* 1..4 */, const float* accum, const float* denom, const float* grad_scale /* NULL */,
                        const float* scaling /* [P][3] raw */, const float* opacity_logit /* [P] or NULL */, const unsigned char* prune_src /* NULL */,
                        float grad_threshold, float size_threshold /* percent_dense * extent */, float min_opacity /* <= 0: off */,
                        char* scratch, unsigned* counts /* device [5] */, void* stream);
int gsrast_densify_apply(int P, int N, const char* scratch, const unsigned* counts_host /* [5], as read back */, int n_groups /* <= 16 */,
                         const gsrast_densify_group* groups /* host array */, const float* rotation /* [P][4] raw */, const float* scaling,
                         const float* noise /* [N * n_split_all][3]; NULL allowed when n_split == 0 */, void* stream);
/* The transpose of a prune-only apply: dst [P][width] <- src [n_kept][width] on the rows the plan kept, +0.0f on every other row.
 * Same P, scratch and read-back counts as the gsrast_densify_plan that made them.  With gsrast_densify_apply over COPY groups it is the
 * differentiable row selection of fused_densify.RowSelection: each call is the other's vector-Jacobian product.  One launch for up to
 * 16 groups, one writer per element, no atomics, nothing read from a row the plan dropped; P = 0 launches nothing, n_kept = 0 zero-fills
 * every dst.  Refused before any device call (gsrast_last_error): P < 0; for P > 0 a NULL scratch, counts_host or groups; n_groups outside
 * [0, 16]; a width outside [1, 64]; a role other than GSRAST_DENSIFY_COPY; any moment pointer; a NULL src while n_kept > 0; a NULL dst;
 * counts that are not a prune-only plan's (n_clone, n_split or n_split_all != 0, counts[4] != counts[0]); n_kept > P.  It has no
 * profile name of its own. */
int gsrast_densify_scatter(int P, const char* scratch, const unsigned* counts_host /* [5] */, int n_groups /* <= 16 */,
                           const gsrast_densify_group* groups /* host array */, void* stream);
/* The per-iteration statistics of train.py:282-292 + add_densification_stats_grad (scene/saro_gaussian.py:745-750), one launch:
 * where visibility_count[i] > 0:  accum[i] += grad_is_mean ? grad[i] : grad[i] / visibility_count[i];  denom[i] += 1;
 * max_radii[i] = max(max_radii[i], radii[i]) (both NULL: skipped).  Other rows are untouched.  All arrays fp32 [P]. */
int gsrast_densify_stats_update(int P, const float* grad, const float* visibility_count, const float* radii,
                                float* accum, float* denom, float* max_radii, int grad_is_mean, void* stream);

/* ---- MCMC densification: relocate dead Gaussians, grow to a cap, position noise -- gsplat's MCMCStrategy on the device ----
 * Replaces gsplat/strategy/ops.py relocate, sample_add and inject_noise_to_position, and gsplat/relocation.py compute_relocation
 * (N_MAX = 51), with the optimizer surgery that goes with the first two.  Row layout: every array is [P][width] fp32, row i = Gaussian i.
 *
 * gsrast_mcmc_plan -- the multinomial's weights (relocate: opacities[alive]; sample_add: opacities.flatten()).  o_i =
 * sigmoid(opacity_logit[i]); row i is dead when o_i <= min_opacity or dead_src[i] != 0 (dead_src [P] bytes or NULL); weights_out[i] =
 * q_i = 0 for a dead row, max(1, floor(o_i * 2^24)) for an alive one (uint32 [P]).  counts[4] (device) = { n_dead, n_alive, W_lo, W_hi },
 * W = sum q_i in 64 bits.  The growth step plans with min_opacity = 0 and no dead_src: every row with o_i > 0 has weight.  The prefixes
 * of q and of the dead flag (two-level scans, no atomics) stay in scratch (>= gsrast_mcmc_scratch_bytes(P, n)) for the calls below.
 *
 * gsrast_mcmc_sample -- torch.multinomial(weights, n, replacement=True) as integer arithmetic: draws[n] int64 in [0, 2^62) (the
 * caller's torch.randint), draw j targets t_j = floor(draws[j] * W / 2^62) and selects the smallest i whose inclusive prefix of q
 * exceeds t_j; a zero-weight row is never selected.  src_out[n] int32 (-1 when W = 0); the draws per source (bincount) stay in scratch
 * and are copied to count_out [P] uint32 when it is not NULL.  Exact: the same q and draws give the same src on every run and rank.
 *
 * gsrast_mcmc_relocate -- relocate's index assignments, in place (groups: dst / dst_m / dst_v are the arrays; src / src_m / src_v NULL
 * or equal to them).  For every source s with count[s] > 0, from the PRE-call values:  r = min(count + 1, 51);  o' = 1 - (1 - o)^(1/r);
 * denom = sum_{i=1..r} sum_{k=0..i-1} C(i-1, k) (-1)^k / sqrt(k+1) o'^(k+1);  s' = (o / denom) exp(scaling);  o' clamped to
 * [min_opacity, 1 - FLT_EPSILON];  stored: logit(o'), log(s').  denom is accumulated in fp64 (gsplat: fp32) -- the one deliberate
 * difference.  The j-th dead row in index order (j < n <= n_dead) becomes a bit copy of row src[j] in every group, except that the
 * OPACITY (width 1) and SCALING (width 3) groups take the source's new values; row src[j] takes them too; exp_avg / exp_avg_sq of every
 * group become 0 at the sampled sources; a dead row keeps its own moments (as the 3DGS-MCMC code and gsplat leave them).  Every row has
 * one writer.  counts_host: the plan's counts as read back.
 *
 * gsrast_mcmc_grow -- sample_add: dst [P + n][width].  Rows [0, P) are bit copies of src with their moments, except that sampled sources
 * carry the new opacity and scaling (computed as above); row P + j is a copy of the updated row src[j] with zero moments.  Nothing in
 * the source arrays is written.  counts_host may be NULL (then W is not checked).
 *
 * gsrast_mcmc_noise -- inject_noise_to_position, one launch, in place:  xyz[i] += Sigma_i (noise[i] * gate_i * scale [* row_scale[i]]),
 * Sigma_i = R(q / |q|) diag(exp(scaling))^2 R(q / |q|)^T over rotation [P][4] raw (r, x, y, z; 16-byte aligned), gate_i = 1 / (1 +
 * exp(-k ((1 - o_i) - x0))) (gsplat: k = 100, x0 = 0.995).  noise [P][3]: the caller's randn; row_scale [P] or NULL; scale: the caller's
 * xyz_lr * noise_lr.
 *
 * Groups: gsrast_densify_group, at most 16, width in [1, 64], moments optional; roles GSRAST_MCMC_*, exactly one OPACITY and one SCALING
 * group when n > 0.  Refused before any device call (gsrast_last_error): P < 0 or n < 0, P + n > 2^31 - 1, min_opacity outside [0, 1),
 * more than 16 groups, a width outside [1, 64], an OPACITY group of width != 1 or a SCALING group of width != 3, NULL required pointers,
 * counts that are not a plan's for this P, n > n_dead (relocate), n > 0 with W = 0.  Profile names: "mcmc_plan" (weights + scan),
 * "mcmc_sample", "mcmc_apply" (values + apply), "mcmc_noise".  Deterministic: no floating-point atomics; P = 0 and n = 0 are valid. */
#define GSRAST_MCMC_COPY 0
#define GSRAST_MCMC_OPACITY 1
#define GSRAST_MCMC_SCALING 2
size_t gsrast_mcmc_scratch_bytes(int P, int n /* today's layout depends on P only */);
int gsrast_mcmc_plan(int P, const float* opacity_logit, const unsigned char* dead_src /* NULL */, float min_opacity, unsigned* weights_out /* [P] */,
                     char* scratch, unsigned* counts /* device [4] */, void* stream);
int gsrast_mcmc_sample(int P, int n, const long long* draws /* [n] in [0, 2^62) */, char* scratch, int* src_out /* [n] */,
                       unsigned* count_out /* [P] or NULL */, void* stream);
int gsrast_mcmc_relocate(int P, int n, const int* src /* [n] */, char* scratch, const unsigned* counts_host /* [4], as read back */, float min_opacity,
                         int n_groups /* <= 16 */, const gsrast_densify_group* groups /* host array */, void* stream);
int gsrast_mcmc_grow(int P, int n, const int* src /* [n] */, char* scratch, const unsigned* counts_host /* [4] or NULL */, float min_opacity,
                     int n_groups /* <= 16 */, const gsrast_densify_group* groups /* host array */, void* stream);
int gsrast_mcmc_noise(int P, float* xyz, const float* rotation, const float* scaling, const float* opacity_logit, const float* noise /* [P][3] */,
                      const float* row_scale /* [P] or NULL */, float scale, float k, float x0, void* stream);

/* ---- fused 3-layer MLP: the deformation heads between the residual-field lookup and the rasterizer ----
 * y = [sigmoid] (W3 relu(W2 relu(W1 [x | x_tail] + b1) + b2) + b3) over N rows, fp32 on the f32-input matrix instruction; replaces the
 * nn.Sequential(Linear, ReLU, Linear, ReLU, Linear[, Sigmoid]) heads motion_mlp / rot_mlp / shs_mlp / opacity_mlp of scene/saro_gaussian.py.
 * x [N][d_x], x_tail [N][d_tail] (read behind x's columns, no gradient; NULL when d_tail = 0), weights in nn.Linear's [out][in] layout,
 * y [N][d_out]; all contiguous fp32 device pointers.  The hidden activations never reach global memory: the backward recomputes them.
 * Shapes: 1 <= d_x, d_tail >= 0, d_x + d_tail <= 64; h1, h2 in {32, 64, 96, 128}; 1 <= d_out <= 64; n >= 0.  Anything else is refused
 * (GSRAST_E_ARG, gsrast_last_error) before any device call, as are NULL required pointers; there is no other path.
 *
 * gsrast_mlp3_forward  writes y.  No scratch.
 * gsrast_mlp3_backward reads x, x_tail, dy [N][d_out] and, for the sigmoid head, y; writes the gradients whose pointer is not NULL:
 *   dx [N][d_x], dw1 [h1][d_in], db1, dw2 [h2][h1], db2, dw3 [d_out][h2], db3 (each OVERWRITTEN; with n = 0 they are 0).  Each workgroup
 *   keeps its share of the weight gradients in registers over all of its row tiles, stores it to scratch (>= gsrast_mlp3_scratch_bytes,
 *   a function of the workgroup count and the widths, never of n) and a second launch sums the shares in workgroup order: no
 *   floating-point atomics, bit-identical results for the same workgroup count.  scratch may be NULL when no weight gradient is wanted.
 * workgroups: 0 = the library's default for the device (forward two per CU, backward one per CU: what their LDS images admit); a call never
 * launches more workgroups than it has 64-row tiles.
 * The backward is one kernel issued as a chain of ceil(n / (512 x workgroups)) launches on `stream` (no accumulator sums more than 512
 * rows in fp32): 8 at n = 1 M on 256 workgroups; a forced small workgroup count with a large n means that many launches.
 * A NaN pre-activation stays NaN through the ReLUs, as torch.relu.
 * Profile names: "mlp_fwd", "mlp_bwd" (ids behind the 32 bits of option "profile": timed when the option is -1). */
typedef struct {
    int n, d_x, d_tail, h1, h2, d_out;
    int sigmoid;                /* 1: the head ends in a Sigmoid */
    const float *x, *x_tail;
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float* y;                   /* forward: out; backward: in (sigmoid head only) */
    const float* dy;            /* backward only, as everything below */
    float *dx, *dw1, *db1, *dw2, *db2, *dw3, *db3;      /* NULL: not wanted, not computed */
} gsrast_mlp3;
size_t gsrast_mlp3_scratch_bytes(const gsrast_mlp3* d /* dims only */, int workgroups);      /* 0: the dims are refused (gsrast_last_error) */
int gsrast_mlp3_forward(const gsrast_mlp3* d, int workgroups, void* stream);
int gsrast_mlp3_backward(const gsrast_mlp3* d, int workgroups, char* scratch, void* stream);

/* The same head with the arithmetic chosen per call.  GSRAST_MLP_FP32 IS the three calls above (same code, same bits, same scratch size).
 * GSRAST_MLP_BF16 runs the products on the bf16 matrix instruction with fp32 accumulation (csrc/gsrast_mlp_bf16.h states the rounding model:
 * x, the weights, both hidden activations and the three back-propagated gradients are rounded to bfloat16, round-to-nearest-even, where a
 * product reads them; biases, bias add, ReLU, Sigmoid, y and every gradient written are fp32; bias gradients sum the unrounded values; the
 * weight gradients are the fp32 master weights', straight-through).  Tensors stay fp32 on both sides, the weights are converted inside each
 * launch and no bf16 copy outlives the call.  Same shapes, refusals, scratch size, launch chain (at most 512 rows per accumulator, tiles of
 * 128 rows), run-to-run bits for one workgroup count and profile names as fp32.  fp32 denormals: unspecified.
 * Any other precision is GSRAST_E_ARG ("precision ...") before any device call. */
#define GSRAST_MLP_FP32 0
#define GSRAST_MLP_BF16 1
size_t gsrast_mlp3_scratch_bytes_p(const gsrast_mlp3* d /* dims only */, int precision, int workgroups);
int gsrast_mlp3_forward_p(const gsrast_mlp3* d, int precision, int workgroups, void* stream);
int gsrast_mlp3_backward_p(const gsrast_mlp3* d, int precision, int workgroups, char* scratch, void* stream);

/* ---- temporal lifespan: the gate between the opacity head and the other heads, and Eq. 22's integral ----
 * What makes the model 4-D (scene/saro_gaussian.py: get_deformation :782-795, get_deformation_eval :871-881, get_intergral :761-777 and the
 * top of update_learning_rate :345-356).  All arrays fp32 [P] device pointers unless noted:  head = the opacity head's output after its
 * Sigmoid;  center = the raw _temporal_pos, read as c = center, or c = sigmoid(center) with sigmoid_center = 1 (args.sigmoid_tcenter);
 * min_scale = min_interval / duration in (0, 1].
 *   L = (1 - min_scale) (1 - head) + min_scale;   d = t - c;   state = exp(-4 (d / L)^2)
 *
 * gsrast_temporal_gate_forward writes lifespan = L, state and, where their pointer is not NULL:
 *   time_emb [P][2 multires + 1] = [d, sin d, cos d, sin 2d, cos 2d, ..., sin 2^(multires-1) d, cos 2^(multires-1) d]  (the reference's
 *   Embedder: include_input, log-sampled exact powers of two, sin before cos; multires in [0, 8]; 16-byte aligned: stored as float4);
 *   dead [P] u8 = !(state > dead_threshold)  (a NaN row is dead).  One launch.
 * gsrast_temporal_gate_backward recomputes L, d and state from head and center (the forward saves nothing) and writes, where their pointer
 *   is not NULL (each OVERWRITTEN):  with u = d / L,  g_L = d_lifespan + d_state (8 u^2 state / L)  and  g_d = d_state (-8 u state / L):
 *   d_head = -(1 - min_scale) g_L,  d_center = -g_d [x c (1 - c) under sigmoid_center].  d_lifespan / d_state NULL: zeros.  The time
 *   embedding carries no gradient (the reference detaches it).  A state that underflowed to 0 gives gradient 0.  One launch, no atomics.
 * gsrast_temporal_integral writes
 *   integral = I = L (sqrt(pi) / 2) (Q(2 sqrt2 (end - c) / L) - Q(2 sqrt2 (start - c) / L)),  Q(x) = 1 / (1 + exp(-(a1 x^3 + a2 x))),
 *   a1 = 0.070565902, a2 = 1.5976 (the reference's 1 - 1 / (1 + e^z) written as a sigmoid: no cancellation for very negative z);
 *   dead [P] u8 = !(I > min_integral);  stats (device int[2], zeroed by the call) = { the float bits of the largest I over the valid rows,
 *   the number of valid rows } (integer atomics: exact and order-free);  inv [P] (NULL: not wanted) = I_max / I on a valid row, 0 on a
 *   dead one -- the reference's (1/I) / min(1/I) with one rounding less.  No valid row: inv all zeros.  Two launches.
 * P = 0 returns 0 without a launch (and without touching stats).  Refused (GSRAST_E_ARG, gsrast_last_error) before any device call:
 * negative P, a NULL required pointer, multires outside [0, 8], sigmoid_center other than 0 / 1, min_scale outside (0, 1], a non-finite t /
 * start / end, end < start, a negative or non-finite min_integral, a time_emb that is not 16-byte aligned.  No floating-point atomics;
 * the launches have no entry in the profile table. */
int gsrast_temporal_gate_forward(int P, int multires, int sigmoid_center, float t, float min_scale, float dead_threshold, const float* head,
                                 const float* center, float* lifespan, float* state, float* time_emb /* NULL ok */, unsigned char* dead /* NULL ok */,
                                 void* stream);
int gsrast_temporal_gate_backward(int P, int sigmoid_center, float t, float min_scale, const float* head, const float* center,
                                  const float* d_lifespan /* NULL = 0 */, const float* d_state /* NULL = 0 */, float* d_head /* NULL ok */,
                                  float* d_center /* NULL ok */, void* stream);
int gsrast_temporal_integral(int P, int sigmoid_center, float start, float end, float min_scale, float min_integral, const float* head,
                             const float* center, float* integral, unsigned char* dead, float* inv /* NULL ok */, int* stats /* device [2] */,
                             void* stream);

/* ---- bilateral-grid colour correction between the render and the loss (gsplat's lib_bilagrid `slice`; 3DGS "exposure" = 1 x 1 x 1) ----
 * grid [12][L][GH][GW] (one camera's grid, PyTorch's [C, D, H, W] order), image / out / dL_dout / dL_dimage [3][H][W]; all contiguous
 * fp32 device pointers.  image is the crop at (x0, y0) of a full_W x full_H frame (a whole frame: x0 = y0 = 0, full = W x H).
 * Per pixel (px, py):   x = (x0 + px + 0.5) / full_W,   y = (y0 + py + 0.5) / full_H,   gray = 0.299 r + 0.587 g + 0.114 b,
 *   u = x (GW - 1),  v = y (GH - 1),  t = clamp(gray, 0, 1) (L - 1);   A[12] = the trilinear interpolation of the 12 channels at (u, v, t)
 *   -- torch.nn.functional.grid_sample(grid[None], 2 (x, y, gray) - 1, "bilinear", "border", align_corners=True); an axis of one vertex
 *   has the single index 0 --;   out_c = A[4c] r + A[4c+1] g + A[4c+2] b + A[4c+3]   (A read as a row-major 3 x 4 matrix).
 * gsrast_bilagrid_forward writes out.  One launch, no scratch.
 * gsrast_bilagrid_backward recomputes the weights and A from grid and image (the forward saves nothing) and writes, where their pointer is
 *   not NULL (each OVERWRITTEN; both NULL is refused):
 *   dL_dimage: through the matrix product and through gray (the t coordinate) as torch's autograd gives it: slope 0 where gray is
 *              outside (0, 1) or L = 1; x and y carry no gradient;
 *   dL_dgrid:  through the trilinear weights, by a gather: one workgroup per vertex column (gx, gy) and slab of its pixel rectangle, one
 *              writer per element, NO floating-point atomics; with more than one slab a second launch sums the slabs' partials (scratch,
 *              >= gsrast_bilagrid_scratch_bytes; may be NULL when dL_dgrid is) in slab order: bit-identical from run to run for a given
 *              slab count.  A vertex no pixel reaches gets exactly 0.
 *   splits: 0 = the library's choice (a function of the descriptor alone); > 0 forces that many slabs per vertex column.
 * A NaN / Inf pixel stays in its own output pixel and in the at most 8 x 12 grid-gradient entries it touches.
 * gsrast_bilagrid_tv: grids [N][12][L][GH][GW];  tv = sum over the axes GW, GH, L of the mean, over every element pair along that axis
 *   (all n, channels and positions), of the squared forward difference; an axis of one vertex contributes 0.  loss_out (device float;
 *   NULL: not wanted): one launch, fixed-order fp64 partial sums.  dL_dgrids (NULL: not wanted; OVERWRITTEN) = *upstream x d tv / d grids
 *   (upstream: device pointer to one float, NULL = 1): one launch, one writer per element.
 * Refused (GSRAST_E_ARG, gsrast_last_error) before any device call: a NULL descriptor or required pointer, GW / GH outside [1, 64], L
 * outside [1, 16], W or H < 1, a frame side outside [1, 32768], a window outside the frame, splits outside [0, 1024], N outside
 * [1, 2048], both outputs NULL.  fp32 only.  The launches have no entry in the profile table. */
typedef struct {
    int GW, GH, L;              /* the grid */
    int W, H;                   /* the image (crop) */
    int x0, y0, full_W, full_H; /* where the crop lies in its frame */
    int splits;                 /* backward: slabs per vertex column; 0 = the library's choice */
} gsrast_bilagrid;
size_t gsrast_bilagrid_scratch_bytes(const gsrast_bilagrid* d);      /* 0: the descriptor is refused (gsrast_last_error) */
int gsrast_bilagrid_forward(const gsrast_bilagrid* d, const float* grid, const float* image, float* out, void* stream);
int gsrast_bilagrid_backward(const gsrast_bilagrid* d, const float* grid, const float* image, const float* dL_dout,
                             float* dL_dimage /* NULL ok */, float* dL_dgrid /* NULL ok */, char* scratch, void* stream);
int gsrast_bilagrid_tv(int N, int GW, int GH, int L, const float* grids, float* loss_out /* NULL ok */, const float* upstream /* NULL = 1 */,
                       float* dL_dgrids /* NULL ok */, void* stream);

/* ---- the renderer's projection as a call of its own (gsplat's fully_fused_projection; csrc/gsrast_project.h) ----
 * What the render keeps inside its geometry state, per Gaussian, as differentiable outputs: 2-D supervision on projected centres (point
 * tracks, optical flow rendered through gsrast_features_forward), screen-size rules for pruning / LOD, statistics on projected quantities.
 * All arrays contiguous fp32 device pointers unless noted; viewmatrix / projmatrix are 16 floats each in the render calls' transposed
 * storage; width, height, tanfovx, tanfovy, scale_modifier as gsrast_forward takes them.  Exactly one of (scales [P][3] + rotations [P][4])
 * and cov3D_precomp [P][6].
 *
 * gsrast_project_forward writes every row of
 *   means2D [P][2]  the pixel centre ((ndc + 1) S - 1) / 2          depths [P]  view-space z
 *   conics  [P][3]  (c, -b, a) / det of the dilated 2-D covariance  radii  [P]  int32: ceil(3 sqrt(lambda_max)), 0 = culled
 *   compensation [P]  (GSRAST_PROJECT_ANTIALIAS only) sqrt(max(0.000025, det(cov2D) / det(cov2D + 0.3 I))): the factor
 *                     GSRAST_RENDER_ANTIALIAS multiplies the opacity with
 * with the expressions of the render's per-Gaussian kernel on the same operands: on a visible row the bits are those of the render's state
 * (gsrast_debug_export: means2D, depths, conic_opacity[0..2]; opacity * compensation = conic_opacity[3]) and radii equals the render's on
 * every row.  A row is visible iff view z > 0.2, det != 0 and its 16 x 16 tile rectangle has non-zero area; a culled row (a NaN mean is
 * one) reads +0.0 in every float output.  One launch, no scratch.
 * gsrast_project_backward recomputes the forward from the inputs (the forward saves nothing) and writes, where their pointer is not NULL
 *   (each row OVERWRITTEN; a culled row gets +0.0): dL_dmeans3D [P][3], dL_dscales [P][3], dL_drotations [P][4], dL_dcov3D [P][6], from
 *   dL_dmeans2D (in pixels), dL_ddepths, dL_dconics, dL_dcompensation (each NULL = zero).  Conventions are the render backward's, so the
 *   gradients of a render and of a projection of the same leaves add consistently: a frustum-clamped t.x / t.z, t.y / t.z (outside 1.3 x
 *   the field of view) is a constant of the Jacobian; d conic / d cov2D carries det^2 / (det^2 + 1e-7); dL_dscales is the gradient of
 *   scale_modifier * scale; the compensation has no gradient where it sits on its floor.  dL_dscales / dL_drotations with cov3D_precomp
 *   are zeros; dL_dcov3D with scales / rotations is the intermediate.  The camera is not differentiated.  One launch, no atomics.
 * P = 0 returns 0 without a launch.  Refused (GSRAST_E_ARG, gsrast_last_error) before any device call: a NULL descriptor, P < 0, a
 * non-positive width / height / tangent, a NULL means3D / viewmatrix / projmatrix, neither or both of (scales + rotations) / cov3D_precomp,
 * exactly one of scales / rotations, rotations or dL_drotations not 16-byte aligned, unknown flag bits; forward: a NULL means2D / depths /
 * conics / radii, a NULL compensation with the flag or one without it; backward: dL_dcompensation without the flag, all four gradient
 * outputs NULL.  The launches have no entry in the profile table. */
#define GSRAST_PROJECT_ANTIALIAS 1u
struct gsrast_project {
    int P, width, height;
    float tanfovx, tanfovy, scale_modifier;
    const float *viewmatrix, *projmatrix;
    const float *means3D, *scales, *rotations, *cov3D_precomp;
    unsigned flags;
    float *means2D, *depths, *conics;           /* forward: out (the backward reads none of the five) */
    int* radii;
    float* compensation;
    const float *dL_dmeans2D, *dL_ddepths, *dL_dconics, *dL_dcompensation;      /* backward only, as everything below; NULL = zero */
    float *dL_dmeans3D, *dL_dscales, *dL_drotations, *dL_dcov3D;                 /* NULL: not wanted, not written */
};
typedef struct gsrast_project gsrast_project;
int gsrast_project_forward(const gsrast_project* d, void* stream);
int gsrast_project_backward(const gsrast_project* d, void* stream);

/* ---- normal consistency: Gaussian normals, depth-map normals, the fused loss (2DGS, gsplat's 2DGS trainer, GOF, RaDe-GS, PGSR;
 *      csrc/gsrast_normal.h) ----
 * All arrays contiguous fp32 device pointers; images are planar [3][H][W] / [H][W]; viewmatrix is 16 floats in the render calls'
 * transposed storage; tanfovx / tanfovy as the render takes them, passed as doubles.  The inputs are fp32, the expressions are evaluated
 * in fp64 and every output is rounded once.  One writer per element, NO floating-point atomics: every value and gradient is
 * bit-identical from run to run.  Every backward recomputes the forward from its inputs (nothing is saved).
 *
 * gsrast_gaussian_normals_forward: normals [P][3], the unit normal of each Gaussian in VIEW space, facing the camera (what a render blends
 *   as gsrast_features_forward's features):  k = argmin(scales[i]) (a tie: the lowest index);  q^ = q / |q|, q = rotations[i] = (w, x, y, z);
 *   n_world = column k of the rotation matrix of q^ (the direction whose variance in the render's Sigma = R S^2 R^T is s_k^2);
 *   n = n_world V[:3,:3],  p = [mean, 1] V;  n is negated where n . p > 0 (an exact 0 is left).  |q| = 0 or a non-finite q: n = 0.
 * gsrast_gaussian_normals_backward: dL_drotations [P][4] (OVERWRITTEN) from dL_dnormals [P][3], through q^; 0 on a row whose normal is 0.
 *   scales, means3D and the camera get no gradient: the argmin and the sign are piecewise constant, the camera is not differentiated.
 *   One launch each, one lane per Gaussian.  P = 0 returns 0 without a launch.
 *
 * gsrast_depth_normal_forward: normals [3][H][W] of the surface depth [H][W] (view-space z: the render's depth, or acc_depth / alpha):
 *   u_x = ((2x + 1) / W - 1) tanfovx,  v_y = ((2y + 1) / H - 1) tanfovy   (the inverse of the render's means2D = ((ndc + 1) S - 1) / 2)
 *   P(x, y) = d(x, y) (u_x, v_y, 1);   a = P(x, y+1) - P(x, y-1),  b = P(x+1, y) - P(x-1, y);   c = a x b,  n = c / |c|
 *   -- gsplat's / 2DGS's central-difference depth_to_normal; a fronto-parallel plane gives (0, 0, -1): towards the camera.
 *   n = 0, with a zero gradient: on the one-pixel border (gsplat's zero padding); where any of the four neighbours' depths is not > 0 (an
 *   uncovered pixel, a NaN); where c . c < 1e-24.  The last two are DEVIATIONS from gsplat, which divides by max(|c|, 1e-12) and has no
 *   coverage rule.
 * gsrast_depth_normal_backward: dL_ddepth [H][W] (OVERWRITTEN) from dL_dnormals [3][H][W], by a gather: dL/dd(q) sums over the four pixels
 *   whose stencil contains q, their cross products recomputed from the depths within the radius-2 diamond around q.
 *
 * gsrast_normal_loss_forward: *loss (device float) = (1 / (H W)) sum_p (1 - w_p <N_p, n_p>), n as above and never written to memory,
 *   N = normal_map [3][H][W] used as given (not normalised: 2DGS's rend_normal), w = weight [H][W] (NULL = 1; e.g. the render's alpha).
 *   One launch writes one fp64 partial per workgroup into scratch (>= gsrast_normal_loss_scratch_bytes(W, H); 0 = the size is refused),
 *   one small launch sums them in a fixed order in fp64.
 * gsrast_normal_loss_backward: *upstream (device float) = dL/dloss;  dL_dnormal_map [3][H][W] = -(upstream / (H W)) w n pointwise, and
 *   dL_ddepth [H][W] by the gather above with dL/dn_p = -(upstream / (H W)) w_p N_p formed on the fly; each NULL = not wanted, else
 *   OVERWRITTEN; the weight gets no gradient.  One launch, no scratch.
 *
 * Refused (GSRAST_E_ARG, gsrast_last_error) before any device call, one text each: P < 0; W or H < 1; W or H > 32768; a tanfov that is
 * not finite or <= 0; a NULL required pointer; a backward whose gradient outputs are all NULL; a NULL scratch.  The launches have no
 * entry in the profile table. */
int gsrast_gaussian_normals_forward(int P, const float* means3D, const float* scales, const float* rotations, const float* viewmatrix,
                                    float* normals, void* stream);
int gsrast_gaussian_normals_backward(int P, const float* means3D, const float* scales, const float* rotations, const float* viewmatrix,
                                     const float* dL_dnormals, float* dL_drotations, void* stream);
int gsrast_depth_normal_forward(int W, int H, double tanfovx, double tanfovy, const float* depth, float* normals, void* stream);
int gsrast_depth_normal_backward(int W, int H, double tanfovx, double tanfovy, const float* depth, const float* dL_dnormals,
                                 float* dL_ddepth, void* stream);
size_t gsrast_normal_loss_scratch_bytes(int W, int H);      /* 0: the size is refused (gsrast_last_error) */
int gsrast_normal_loss_forward(int W, int H, double tanfovx, double tanfovy, const float* normal_map, const float* depth,
                               const float* weight /* NULL = 1 */, float* loss, char* scratch, void* stream);
int gsrast_normal_loss_backward(int W, int H, double tanfovx, double tanfovy, const float* normal_map, const float* depth,
                                const float* weight /* NULL = 1 */, const float* upstream, float* dL_dnormal_map /* NULL ok */,
                                float* dL_ddepth /* NULL ok */, void* stream);

/* ---- Mip-Splatting's 3-D smoothing filter (Yu et al., CVPR 2024): the camera sweep and the fused activation (csrc/gsrast_filter3d.h) ----
 * The companion of GSRAST_RENDER_ANTIALIAS (the 2-D screen-space filter): every Gaussian's size is bounded below by the highest sampling
 * rate at which any training camera sees it.  All arrays contiguous fp32 device pointers.
 *
 * table [C][16], one row per camera: floats 0-8 R = viewmatrix[:3,:3] row-major (viewmatrix in the render calls' transposed storage, so
 *   p_cam = p R + T: Mip-Splatting's camera.R / camera.T), 9-11 T = viewmatrix[3,:3], 12 focal_x, 13 focal_y, 14 W, 15 H.
 *
 * gsrast_filter3d_compute: per row (x, y, z) of means3D [P][3] and camera, in fp32, every operation rounded, no FMA:
 *     xc = ((x R00 + y R10) + z R20) + T0,  yc, zc with columns 1, 2;   zz = fmaxf(zc, 0.001f)
 *     px = (xc / zz) focal_x + W 0.5f,  py = (yc / zz) focal_y + H 0.5f
 *     seen = zc > near && zz < +inf && -(margin W) <= px <= W + margin W && -(margin H) <= py <= H + margin H
 *   dist = min of zz over the cameras that see the row;  valid [P] (bytes 0 / 1; NULL = not wanted) = some camera sees it;
 *   dmax = max of dist over the valid rows;  filter_3D [P] = (valid ? dist : dmax) k,  k = (float)(sqrt(variance) / focal_max) formed in
 *   fp64;  near, margin, variance are rounded to fp32 once.  A NaN or Inf row is never valid.  No valid row: every filter_3D is +0.0.
 *   Upstream's compute_3D_filter with near = 0.2, margin = 0.15, variance = 0.2, focal_max = the largest focal_x, except: one multiplication
 *   by k where it divides and multiplies; the bounds W + margin W where it writes W 1.15; zeros where its max() of nothing raises.
 *   Two launches (the sweep; the elementwise finish, once the maximum exists) and a clear of the two scratch words, all on `stream`.
 *   The maximum is an integer max on the bits of positive floats, one writer per element, no floating-point atomics: bit-identical from
 *   run to run and on every rank.  scratch: >= gsrast_filter3d_scratch_bytes(P, C) bytes (0 = the sizes are refused).
 *
 * gsrast_filter3d_apply_forward, on ACTIVATED scales [P][3] and opacities [P]:
 *     s_f,k = sqrt(s_k s_k + f f);  r_k = s_k / s_f,k (1 where s_f,k == 0);  o_f = o ((r_0 r_1) r_2)
 *   -- upstream's get_scaling_with_3D_filter and get_opacity_with_3D_filter (o sqrt(prod s^2 / prod (s^2 + f^2))) without the products
 *   of squares, which underflow in fp32 for thin Gaussians.
 * gsrast_filter3d_apply_backward recomputes s_f, r from the three inputs (nothing is saved);  q_k = f / s_f,k (0 where s_f,k == 0),
 *   G = g_o o:   d s_k = g_s,k r_k + (G prod_{j != k} r_j) ((q_k q_k) / s_f,k),   d o = g_o ((r_0 r_1) r_2).
 *   A NULL upstream gradient counts as zero; a NULL output is not wanted, else OVERWRITTEN; filter_3D gets no gradient.
 *   One launch each, one lane per row, no LDS, scratch or atomics.
 *
 * Refused (GSRAST_E_ARG, gsrast_last_error) before any device call, one text each: P < 0; C < 1; near, variance or focal_max not finite
 * or <= 0; margin not finite or < 0; a NULL required pointer; a NULL scratch; a backward whose gradient outputs are both NULL.
 * P = 0 returns 0 without a launch.  The launches have no entry in the profile table. */
size_t gsrast_filter3d_scratch_bytes(int P, int C);      /* 0: the sizes are refused (gsrast_last_error) */
int gsrast_filter3d_compute(int P, int C, const float* means3D, const float* table, double near, double margin, double variance,
                            double focal_max, float* filter_3D, unsigned char* valid /* may be NULL */, void* scratch, void* stream);
int gsrast_filter3d_apply_forward(int P, const float* scales, const float* opacities, const float* filter_3D, float* scales_f,
                                  float* opacities_f, void* stream);
int gsrast_filter3d_apply_backward(int P, const float* scales, const float* opacities, const float* filter_3D,
                                   const float* d_scales_f /* may be NULL */, const float* d_opacities_f /* may be NULL */,
                                   float* d_scales /* may be NULL */, float* d_opacities /* may be NULL */, void* stream);

/* ---- "next" row, rank 4 (second item): simple_knn._C.distCUDA2 ----
 * mean_dist2[i] = mean of the squared distances from point i to its 3 nearest neighbours (other indices; duplicates count).
 * Replaces the un-vendored dependency imported at scene/saro_gaussian.py:21 and used at :187 (scale initialisation).
 * points [P][3] fp32, mean_dist2 [P], scratch >= gsrast_knn_scratch_bytes(P) bytes; all device pointers.
 * With fewer than 4 points the missing neighbours count as FLT_MAX, as in the original. */
size_t gsrast_knn_scratch_bytes(int P);
int gsrast_knn3_mean_dist2(int P, const float* points, float* mean_dist2, char* scratch, void* stream);

/* ---- exact k-nearest-neighbour query with indices: mmcv.ops.knn ----
 * Replaces the un-vendored dependency imported at helper_model.py:27 and called as knn(2, xyz, xyz, False) at :150, :207, :354.
 * For every query point: the k reference points with the smallest (d2, index) in lexicographic order, ascending.
 *   ref [n_ref][3] fp32;  query [n_query][3] fp32, or NULL: the reference set queries itself (n_query must then equal n_ref)
 *   k 1..32;  idx [k][n_query] int32 (mmcv's (B, k, npoint) of one batch, no transpose);  dist2 [k][n_query] fp32, or NULL: not wanted
 *   scratch >= gsrast_knn_query_scratch_bytes(n_ref, n_query) bytes (negative sizes count as 0; never 0 itself; non-decreasing in each
 *   argument; pure host code).  All pointers are device pointers.
 * Semantics:
 *   exact       d2 = (dx dx + dy dy) + dz dz in fp32, each difference (query - reference) ONE fp32 subtraction, no FMA: the kernel's own
 *               value, and the search is exact in it.  Equal d2 puts the lower reference index first.
 *   self        a point is its own neighbour: in a self-query slot 0 has d2 = 0 and is the point itself, or a duplicate of it with a
 *               lower index (mmcv behaves so; the reference's xyznnpoints[0, 1] relies on it).
 *   missing     slots j >= n_ref hold idx -1 and dist2 +inf (n_ref = 0: every slot).
 *   determinism every output element has one writer, no atomics: bit-identical from run to run; dist2 does not depend on the order of
 *               the reference rows, and permuting the query rows permutes the output columns.
 *   non-finite  coordinates are unsupported (what such a query or neighbour returns is unspecified), but cause no out-of-range access:
 *               the Morton quantisation clamps through fminf / fmaxf and every index is bounded by the sizes.
 * Refused (GSRAST_E_ARG) before any device call: a negative size, k outside 1..32, a NULL idx, ref or scratch (n_ref > 0), a NULL query
 * with n_query != n_ref.  n_query = 0 returns 0 and touches nothing. */
size_t gsrast_knn_query_scratch_bytes(int n_ref, int n_query);
int gsrast_knn_query(int n_ref, const float* ref, int n_query, const float* query, int k, int32_t* idx, float* dist2, char* scratch,
                     void* stream);

/* ---- "next" row, rank 4 (first item): mip-mapped feature-plane lookup of the residual field ----
 * Replaces nvdiffrast.torch.texture(grid, coords, mip_level_bias=levels, boundary_mode="clamp", max_mip_level=7|0) at
 * scene/hexplane.py:49-56 together with the plane loop of interpolate_ms_features (scene/hexplane.py:95-139): every plane
 * of every scale in one forward launch.  Published algorithm of that op (linear-mipmap-linear, level from the bias only)
 * as restated in oracle/texture_oracle.py.
 *   plane      channel-last level 0 [H][W][C] fp32 (hexplane.py:35 layout); u = pts[n][cu], v = pts[n][cv] in [0,1]
 *              texture coordinates; bias = min(levels[n][cu], levels[n][cv]) (hexplane.py:46)
 *   features   [N][F]; plane p adds its C channels at features[n][out_offset .. out_offset + C); planes sharing an
 *              out_offset (the six planes of a scale) must be adjacent in the array and are summed in array order; two
 *              blocks are equal or disjoint (GSRAST_E_ARG otherwise).  Columns of a row that no block covers are left
 *              UNWRITTEN by the forward (the caller zeroes them if it reads them) and are not read by the backward
 *   C          power of two in [4, 64]; D = floats per pts / levels row (4 in the reference); F = floats per feature row,
 *              a multiple of 4, up to 24 blocks wide (the reference's 4 scales of 32 channels: F = 128)
 *   scratch    >= gsrast_hexplane_scratch_bytes() bytes (mip stacks: built by every forward call, as the op does; gradient
 *              stacks and the sorted (plane, point) pairs of the backward).  That call is not given F: it checks what does
 *              not depend on the row width and returns 0, with its reason in gsrast_last_error(), when a descriptor is
 *              refused; whether a block fits its row is checked by forward / backward
 * backward: grad_tex of every plane is overwritten with dL/dtex; d_pts / d_levels [N][D] optional (the reference detaches
 * both, scene/saro_gaussian.py:780); mips_built != 0 says scratch still holds the forward's stacks of these textures.
 * All pointers inside gsrast_plane and the tensor arguments are device pointers; `planes` itself is a host array. */
typedef struct {
    const float* tex;
    float* grad_tex;        /* backward only */
    int W, H;
    int cu, cv;
    int max_mip_level;      /* the op's max_mip_level: 0 = no mip stack */
    int out_offset;
} gsrast_plane;
size_t gsrast_hexplane_scratch_bytes(int n_planes, const gsrast_plane* planes, int C, int N);
int gsrast_hexplane_forward(int N, int D, int C, int F, int n_planes, const gsrast_plane* planes, const float* pts,
                            const float* levels, float* features, char* scratch, void* stream);
int gsrast_hexplane_backward(int N, int D, int C, int F, int n_planes, const gsrast_plane* planes, const float* pts,
                             const float* levels, const float* d_features, float* d_pts, float* d_levels, int mips_built,
                             char* scratch, void* stream);

const char* gsrast_last_error(void);
int gsrast_abi_version(void);

enum {
    GSRAST_OK = 0,
    GSRAST_E_ARG = -1,     /* bad argument combination / NULL required pointer */
    GSRAST_E_ALLOC = -2,   /* allocation callback returned NULL */
    GSRAST_E_DEVICE = -3,  /* HIP runtime error, see gsrast_last_error() */
    GSRAST_E_OVERFLOW = -4 /* more than 2^31-1 instances */
};

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_H_INCLUDED */
