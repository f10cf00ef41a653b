/*
 * recfilter_amd.h -- C ABI of the MI355X-native tiled recursive-filter runtime.
 *
 * This is the drop-in boundary for the hot path of mit-gfx/recfilter: everything
 * the reference hands to Halide at
 *      RecFilter::realize()   lib/recfilter.cpp:984-989  (Func::realize)
 *      RecFilter::profile()   lib/recfilter.cpp:991-1016
 *      RecFilter::compile_jit lib/recfilter.cpp:918-930  (Func::compile_jit)
 * after it has built the scan list with RecFilter::add_filter
 * (lib/recfilter.cpp:260-392) and tiled it with RecFilter::split
 * (lib/split.cpp:1850-2080).  A plan replaces the Func graph that split() builds and
 * the schedule that RecFilterSchedule (lib/schedule.cpp) attaches to it: the tiling
 * algebra becomes host-side tables, the four stages (intra-tile scans, tail extraction,
 * cross-tile carry recurrence, final correction) are hand-written gfx950 kernels.
 *
 * Conventions
 *   - plain C types only; every function returns an rf_status code, 0 = ok, and never throws;
 *     rf_last_error_string() describes the last failure on the calling thread.
 *   - images are dense, planar, x fastest (Halide's layout, lib/recfilter.cpp:969-981);
 *     a Halide Tuple is n_planes separate buffers that share the filter.
 *   - all image pointers are DEVICE pointers (hipMalloc or torch); `stream` is a
 *     hipStream_t passed as void* (NULL = the default stream).  rf_plan_execute is
 *     asynchronous on that stream.
 *   - the library has no CPU fallback: without a usable HIP device every entry point that
 *     needs one fails with RF_ERR_HIP.
 */
#ifndef RECFILTER_AMD_H
#define RECFILTER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_MAX_DIMS    3    /* the reference's auto-schedules stop at 3 (lib/recfilter.cpp:6,734) */
#define RF_MAX_ORDER   32   /* feedback taps per scan: RecFilter::add_filter takes any order (lib/recfilter.cpp:260-343);
                             * the reference's own sweep stops at 29 (apps/audio/audio_filter_high_order.cpp:14,38) */
#define RF_MAX_SCANS   32
#define RF_MAX_PLANES  16
/* desc.device value that builds the plan's host tables without touching a device; such a plan
 * answers rf_plan_table / rf_plan_tiles / rf_plan_path but refuses to execute (RF_ERR_HIP). */
#define RF_DEVICE_HOST_ONLY (-2)

typedef enum {
    RF_OK = 0,
    RF_ERR_INVALID_ARG = 1,   /* the misuse cases the reference asserts on (lib/recfilter.cpp:274,296) */
    RF_ERR_UNSUPPORTED = 2,
    RF_ERR_HIP = 3,           /* HIP runtime error or no device */
    RF_ERR_NOMEM = 4,
    RF_ERR_STATE = 5          /* stepping API called out of order */
} rf_status;

/* pixel type P = type of the defining expression (lib/recfilter.cpp:197); coefficients are
 * cast to P (lib/recfilter.cpp:324,335).
 *
 * RF_F16 (IEEE binary16) and RF_BF16 (bfloat16) deliberately depart from that rule: they are STORAGE types.  Input and output
 * planes hold 16-bit floats; every sample is widened exactly to f32 as it is loaded; coefficients, tails, carries, tables,
 * pointwise stages and every intermediate are those of an RF_F32 plan of the same description; the result is rounded ONCE,
 * to nearest even, at the final store (overflow to +-inf, NaN propagates):  out = round16(F_f32(widen(in))).
 * 2-D images (width a multiple of 4) and long 1-D signals run natively on RF_PATH_TILED_FUSED.  So do unsharded volumes
 * filtered along z whose depth the strided z kernels tile (a multiple of 32) and whose width is a multiple of 4, without an
 * epilogue: the x/y stage's result waits, unrounded, in a plan-owned f32 volume per plane (always allocated, counted in
 * rf_plan_workspace_bytes), and the final z pass rounds as it stores; the launch list is that of the RF_F32 plan built with
 * RF_PLAN_STAGED_PASS1.  RF_PATH_TILED_FUSED asks for that form at any size; RF_PATH_AUTO takes it from 2^23 samples per plane
 * on (measured: 0.69 of the staged step there, 0.52 at 1024^3; at 2^21 samples the staged form, three launches of the line
 * kernels between its conversions, is 1.27x ahead).  Every other plan is staged
 * through plan-owned f32 planes (steps "convert_in" / "convert_out", counted in rf_plan_workspace_bytes; rf_plan_path
 * reports the inner f32 plan's path).  RF_IN_U8 input and shards other than the row shards of a 2-D image on the fused
 * path: RF_ERR_UNSUPPORTED. */
typedef enum { RF_F32 = 0, RF_F64 = 1, RF_I32 = 2, RF_I16 = 3, RF_F16 = 4, RF_BF16 = 5 } rf_dtype;

/* default border is zero; RecFilter::set_clamped_image_border (lib/recfilter.cpp:252-258) */
typedef enum { RF_BORDER_ZERO = 0, RF_BORDER_CLAMP = 1 } rf_border;

/* how a plan executes */
typedef enum {
    RF_PATH_AUTO = 0,      /* fastest path the shape admits                                        */
    RF_PATH_UNTILED = 1,   /* one serial recurrence per line (a filter that was never split())      */
    RF_PATH_TILED_GENERIC = 2, /* tiled, any tile width dividing the extent (split(x,tx,..))        */
    RF_PATH_TILED_FUSED = 3,   /* tiled, LDS-staged fused x/y tiles with fixed MI355X tile shapes; a filter with more
                                * than four scans in a dimension runs as successive stages of such plans inside the
                                * one plan (stage 0 reads the input, later stages filter the output planes in place) */
    RF_PATH_TILED_OVERLAPPED = 4, /* tiled, ALL dimensions in one pass 1 / one pass 2 with the cross-dimension
                                  * residuals of lib/split.cpp:1215-1633 between every pair of dimensions (x->y, x->z,
                                  * y->z): the reference's fully overlapped N-D tiling.  Needs an explicit tile width
                                  * for every filtered dimension, tile volume <= 4096 samples; RF_PATH_AUTO picks it
                                  * for such filters when the fused path does not apply */
    RF_PATH_TILED_MATRIX = 5     /* tiled, one scan at a time, every stage a dense f32 GEMM on the matrix cores
                                  * (kernels_matrix.hip): tail extraction H[k x T] . tile, the carry recurrence as a chain
                                  * of k x k products, the final pass as 32 x 32 impulse-response blocks.  Scans of ANY
                                  * order up to RF_MAX_ORDER in their direct form (the reference's apps sweep orders up to
                                  * 29); f32 pixels, any extents whose width is a multiple of 4 samples.  RF_PATH_AUTO picks it for
                                  * filters with a scan of order above 3 that the fused path (sections) does not take */
} rf_path;

/* one RecFilter::add_filter(+-dim, {feedfwd, fb1..fbk}) call, lib/recfilter.cpp:264-343 */
typedef struct {
    int32_t dim;                    /* 0 = x (fastest), 1 = y, 2 = z                      */
    int32_t causal;                 /* 1 = +dim, 0 = -dim                                 */
    int32_t order;                  /* number of feedback coefficients, 1..RF_MAX_ORDER   */
    float   feedfwd;
    float   feedback[RF_MAX_ORDER]; /* y[i] = feedfwd*x[i] + sum_j feedback[j]*y[i-j-1]   */
} rf_scan_desc;

/* Pointwise stages fused around the filter.  The reference writes them as Halide expressions: the
 * defining expression of the filter (R(x,y) = cast<float>(in(x,y))/255, demo/demo_gaussian_filter.cpp:51-57)
 * and a consumer computed at the filter's tiles with RecFilter::compute_at (lib/recfilter.cpp:473-573),
 * e.g. USM = (1+w)*in - w*Blur in apps/usm/unsharp_mask_optimized.cpp:57-61.  Here they are two affine maps:
 *     x'  = pre_scale * in + pre_bias                               before the first scan
 *     out = post_filtered * F(x') + post_input * x' + post_bias      after the last scan (F = the filter)
 * flags = 0 (a zeroed struct) means both are the identity.  Float pixel types only.  On the fused path both
 * are applied inside pass 1 / pass 2 (no extra pass over the image); the other paths run them as separate
 * elementwise kernels.  RF_POINTWISE_POST with post_input != 0 needs out != in. */
#define RF_POINTWISE_PRE   1
#define RF_POINTWISE_POST  2
/* element type of the INPUT planes: the pixel type (default), or unsigned bytes converted on load -- the
 * `cast<float>(input(x,y,c)) / 255.0f` of demo/demo_gaussian_filter.cpp:51-53 with the uint8 image read directly
 * (1 byte per sample instead of 4 in both passes).  RF_IN_U8 needs dtype RF_F32; outputs stay f32.
 *
 * RF_IO_U8: input AND output planes hold unsigned bytes -- a STORAGE type under the contract of RF_F16 / RF_BF16 above.  dtype
 * must be RF_F32; the filter is the RF_F32 plan of the same description with RF_IN_U8 (bytes widened on load; prologue, tails,
 * carries, tables and epilogue are that plan's); no intermediate ever passes through a byte plane; the result is converted
 * ONCE, at the final store:  out = sat8(v),  sat8(v) = (uint8) min(max(rint(v), 0), 255),  v the f32 value behind the epilogue
 * (post_filtered * F(x') + post_input * x' + post_bias, or F(x') without one).  rint rounds to nearest, ties to even; values
 * below 0 store 0, values above 255 store 255, NaN stores 0 -- the reference's consumer cast<uint8_t>(...) computed at the filter.
 * 2-D images whose width is a multiple of 4, with orders <= 3 and at most four scans per dimension, run natively on
 * RF_PATH_TILED_FUSED: the launch list is the RF_IN_U8 plan's, name for name, and its final pass stores the bytes (3 bytes of
 * image traffic per sample instead of 6 and a conversion pass).  Volumes (ndim == 3) with scans along z and along x and / or y run
 * natively too where the depth is a multiple of 32 (the strided z kernels tile it), the width a multiple of 4, orders are <= 3
 * with at most four scans per dimension, post_input == 0 and none of RF_PLAN_STAGE_HALF / RF_PLAN_INPLACE_Z / RF_PLAN_WALK_PASS1
 * is set -- under RF_PATH_TILED_FUSED at any size, under RF_PATH_AUTO from 2^21 samples per plane on: the launch list is that of
 * the RF_IN_U8 plan with RF_PLAN_STAGED_PASS1 without its "pointwise_post" step, the x/y result waits in one plan-owned f32
 * volume per plane (counted in rf_plan_workspace_bytes, listed as scratch) and the final z pass stores
 * sat8(post_filtered * v + post_bias).  Every other plan the RF_IN_U8 plan can run is staged: that
 * plan writes plan-owned f32 planes (counted in rf_plan_workspace_bytes, listed as scratch by rf_plan_debug_buffer), one step
 * "convert_out" follows; rf_plan_path reports the inner plan's path.  in == out is allowed (an epilogue with post_input != 0
 * needs out != in, as everywhere).  Planes on both sides must be 4-byte aligned.  Any other dtype, sharded plans and
 * RF_PLAN_FORCE_EXCHANGE: RF_ERR_UNSUPPORTED. */
typedef enum { RF_IN_PIXEL = 0, RF_IN_U8 = 1, RF_IO_U8 = 2 } rf_input_dtype;
typedef struct {
    int32_t flags;                    /* RF_POINTWISE_PRE | RF_POINTWISE_POST */
    float   pre_scale, pre_bias;
    float   post_filtered, post_input, post_bias;
    int32_t in_dtype;                 /* rf_input_dtype */
} rf_pointwise_desc;

/* Plan options (rf_filter_desc.flags).  The library reads NO environment variable: what a caller (or a test) wants
 * to choose about a plan is chosen here.  (A/B timing switches of the kernel developers exist only in builds made
 * with -DRF_AB_KNOBS, tools/; the shipped library has none.)
 *   RF_PLAN_FORCE_EXCHANGE  build the sharded structure -- per-scan launches around the exchange points, exit carries,
 *                           the gather walk, the correction of the slab -- even for shard_world == 1, and insist on the
 *                           stepping calls.  The all-gather of one rank is the identity, so the result is the plain
 *                           filter; it lets a box with ONE GPU drive begin / exchange_local / all-gather (RCCL) /
 *                           exchange_apply / finish exactly as every rank of an N-GPU run does.
 *   RF_PLAN_TILED_ONLY      RF_PATH_AUTO never resolves to the line-parallel untiled kernels it prefers for images up
 *                           to 1024^2 (launch-bound regime): small images take the tiled kernels too.
 *   RF_PLAN_NO_CASCADE      a filter the fused kernels cannot take in one piece (more than four scans per dimension)
 *                           is not split into successive fused stages inside the plan; it runs as given on another path.
 *   RF_PLAN_NO_SECTIONS     scans of order 4..8 are not rewritten into sections of order <= 3.
 *   RF_PLAN_NO_OVERLAP      the consecutive same-direction scans of a 1-D signal (zero border, f32) are not merged into one
 *                           scan of their product transfer function (overlap_feedback_coeff, lib/iir_coeff.cpp:236-263) for
 *                           the matrix path -- what RF_PATH_AUTO does where a host-side probe finds the merged direct form
 *                           within 2e-5 of the cascade and fewer stages result (five biquads: two fused stages -> one scan).
 *   RF_PLAN_NO_PLANE_BATCH  the planes of a 2-D Tuple run as separate launches instead of one batched launch per step.
 *   RF_PLAN_STREAM_PASS1 /  pass 1 of the fused path as the LDS-DMA streaming kernel wherever its shape rules allow,
 *   RF_PLAN_STAGED_PASS1    whatever the image size / never (default: single planes of at least 2048 tiles).
 *                           STAGED also keeps the vector-ALU contraction (fused_tails_kernel) for every order.
 *   RF_PLAN_MFMA_PASS1      pass 1 with its x-tail contraction on the matrix cores (kernels_tails_mfma.hip) wherever its
 *                           shape rules allow -- f32 images of whole tiles, at most two scans per dimension -- whatever
 *                           the order (default: orders 2 and 3).  The streaming kernel keeps what it takes.
 *   RF_PLAN_WALK_PASS1      3-D: pass 1 reads the volume ONCE and forms the x, y and z tails together (the z operators commuted
 *                           in front of the x/y filter, kernels_tails_walk.hip; 20 instead of 24 bytes per sample) wherever
 *                           its shape rules allow -- f32 volumes whose depth is whole z tiles and whose width is a multiple of
 *                           four (partial tiles along x and y load as zeros; z slabs: with the early exchange), a prologue
 *                           x' = s x + b applied as the samples arrive (not 8-bit input), orders <= 3 along x / y and <= 2 along z,
 *                           one or two scans in each of the three dimensions -- whatever the size (default: volumes of at
 *                           least 256 patches of 256 x 32 samples x one z tile, one per compute unit);
 *                           RF_PLAN_STAGED_PASS1 keeps the two first passes of the x/y and z stages.
 *   RF_PLAN_LATE_EXCHANGE   a z-sharded volume exchanges the carries of the x/y-FILTERED data, after its x/y stage
 *                           (nothing runs beside the all-gather); default: the carries of the raw input first, the x/y
 *                           stage beside the all-gather (rf_plan_interior below).
 *   RF_PLAN_SERIAL_UNTILED  RF_PATH_UNTILED as one serial recurrence per line for every filter (the literal operator of
 *                           lib/recfilter.cpp:302-343; an independent on-device reference) instead of the line-parallel
 *                           kernels it uses where they apply.
 *   RF_PLAN_TILE_ROWS(n) /  n = 32, 64 or 128: tile height of the fused x/y stage / tile width of the strided z stage,
 *   RF_PLAN_TILE_PLANES(n)  where the shape admits it (default: chosen from the image size; rf_plan_tiles reports it).
 *                           rf_filter_desc.tile[] stays what RecFilter::split passes: binding on the generic and
 *                           overlapped paths, a hint on the fused path (the tile size never changes the result).
 *   RF_PLAN_INPLACE_Z       3-D on the fused path: the z stage filters the x/y stage's result where it lies, in the output
 *                           planes.  Default for volumes of at least 2^28 samples: the x/y stage writes a plan-owned
 *                           INTERMEDIATE VOLUME and the z stage reads it (rf_plan_workspace_bytes grows by one volume) --
 *                           a final z pass that reads and writes the same addresses runs 4 % slower (its read and write
 *                           fronts chase each other through the same DRAM banks: tools/microbench/zpass_shape.hip) -- as
 *                           long as that volume is at most a third of the device memory free when the plan is built.
 *                           Same kernels, same results either way.  (A native RF_F16 / RF_BF16 volume and a native
 *                           RF_IO_U8 byte volume NEED that volume, in f32: with this flag such a plan is staged through
 *                           f32 planes instead.)
 *   RF_PLAN_FULL_CARRY_SCAN the fused x/y stage runs its carry scans (carry_x / carry_y) for every filter.  Default: an f32
 *                           2-D image (or batched Tuple planes), unsharded, whose scans along a dimension are one scan or
 *                           a causal-then-anticausal pair, completes that dimension's carries from the neighbouring
 *                           tiles' tails alone where the filter decays within a tile -- the part that form drops is
 *                           at most 2^-32 of the largest carry (rf_plan_table("neighbour_carries")).
 *   RF_PLAN_SEPARATE_ROW_SCANS a neighbour-form step keeps its three kernels as they are for every filter: the launch between
 *                           the passes scans the y tails' combined rows, adds the cross-dimension residual and completes
 *                           the x tails.  Default: an f32 image of whole 256 x 128 tiles under an order-2 causal + anticausal
 *                           pair in x and in y, both in neighbour form and without pointwise stages, takes the row-scan
 *                           form (rf_plan_table("row_scans") = 1): pass 1 scans the rows it holds, that launch only contracts
 *                           the x tails into 64 bytes per tile, and the final pass forms the carries it loads.  Same step
 *                           names, same workspace, the same result to the bit.
 *   RF_PLAN_STAGE_HALF      RF_F16 / RF_BF16 pixels: the plan is staged through f32 planes even where the fused kernels
 *                           would run it natively -- 2-D images, 1-D signals and volumes alike (same result to the last
 *                           rounding; for comparisons).  RF_IO_U8 planes (rf_input_dtype): the plan is staged through f32
 *                           planes and "convert_out" even where the fused final pass (2-D images) or the final z pass
 *                           (volumes) would store the bytes itself.  Ignored for every other plan. */
#define RF_PLAN_FORCE_EXCHANGE  0x01u
#define RF_PLAN_TILED_ONLY      0x02u
#define RF_PLAN_NO_CASCADE      0x04u
#define RF_PLAN_NO_SECTIONS     0x08u
#define RF_PLAN_NO_PLANE_BATCH  0x10u
#define RF_PLAN_STREAM_PASS1    0x20u
#define RF_PLAN_STAGED_PASS1    0x40u
#define RF_PLAN_LATE_EXCHANGE   0x80u
#define RF_PLAN_SERIAL_UNTILED  0x01000000u
#define RF_PLAN_MFMA_PASS1      0x02000000u
#define RF_PLAN_WALK_PASS1      0x04000000u
#define RF_PLAN_NO_OVERLAP      0x08000000u
#define RF_PLAN_INPLACE_Z       0x10000000u
#define RF_PLAN_FULL_CARRY_SCAN 0x20000000u
#define RF_PLAN_STAGE_HALF      0x40000000u
#define RF_PLAN_SEPARATE_ROW_SCANS 0x80000000u
#define RF_PLAN_ALL_FLAGS       0xff0000ffu
#define RF_PLAN_TILE_ROWS(n)    (((uint32_t)(n) & 0xffu) << 8)
#define RF_PLAN_TILE_PLANES(n)  (((uint32_t)(n) & 0xffu) << 16)

/* Revision of the binary interface: the layout of the structs below as this header declares them.  rf_plan_create refuses a
 * descriptor whose `abi` is not RF_ABI -- a caller compiled against another revision of the header (revision 3: RF_MAX_ORDER
 * went from 8 to 32 in round 5, which changed sizeof(rf_scan_desc) and the row layout of rf_plan_table("scans")) gets
 * RF_ERR_INVALID_ARG instead of a mis-strided scans array.  The field sits in what used to be the padding behind `ndim`. */
#define RF_ABI 3u

typedef struct {
    int32_t  ndim;                    /* 1..RF_MAX_DIMS                                          */
    uint32_t abi;                     /* RF_ABI                                                  */
    int64_t  extent[RF_MAX_DIMS];     /* extent[0] = width (x)                                   */
    int32_t  dtype;                   /* rf_dtype                                                */
    int32_t  n_planes;                /* Tuple size, >= 1                                        */
    int32_t  border;                  /* rf_border                                               */
    int32_t  n_scans;
    const rf_scan_desc *scans;        /* in add_filter call order                                */
    int32_t  tile[RF_MAX_DIMS];       /* RecFilter::split widths; 0 = let the plan choose        */
    int32_t  path;                    /* rf_path                                                 */
    int32_t  device;                  /* HIP device ordinal, -1 = current, RF_DEVICE_HOST_ONLY   */
    /* outermost-dimension shard (multi-GPU); world = 1 for a single GPU.  extent[] is the LOCAL
     * slab; the slab of rank r follows the slab of rank r-1 along dimension ndim-1. */
    int32_t  shard_rank;
    int32_t  shard_world;
    rf_pointwise_desc pointwise;      /* zeroed = none                                           */
    /* slabs of different extents: shard_world extents along dimension ndim-1, one per rank, in rank order
     * (shard_extents[shard_rank] == extent[ndim-1]); NULL = every slab has this rank's extent.  All ranks pass
     * the same array: the tile width along the sharded dimension is chosen from their common divisor so that
     * every rank tiles alike. */
    const int64_t *shard_extents;
    uint32_t flags;                   /* RF_PLAN_* options below; 0 = the defaults                 */
} rf_filter_desc;

typedef struct rf_plan rf_plan;

/* ---- plan lifetime (replaces split()+schedule+compile_jit) ------------------------------- */
int rf_plan_create(const rf_filter_desc *desc, rf_plan **plan_out);
int rf_plan_destroy(rf_plan *plan);

/* bytes of device workspace the plan allocated for tails/carries (owned by the plan) */
size_t rf_plan_workspace_bytes(const rf_plan *plan);
/* execution instances the plan holds right now: 1 + the replicas concurrent executes made it build (see rf_plan_execute) */
int rf_plan_num_instances(rf_plan *plan);
/* which rf_path the plan resolved to, and the tile widths it uses (0 for an untiled dim) */
int rf_plan_path(const rf_plan *plan);
int rf_plan_tiles(const rf_plan *plan, int32_t tile_out[RF_MAX_DIMS]);
/* number of kernels one execute launches, and their names (for profilers) */
int rf_plan_num_kernels(const rf_plan *plan);

/* ---- execution (replaces Func::realize) --------------------------------------------------- */
/* Concurrent executions.  A plan is a description plus tables (immutable after rf_plan_create); an EXECUTION needs a
 * tail/carry workspace and a context (plane pointers, stream, stepping phase).  The plan holds one of each; an execute
 * that arrives on another stream while the previous one may still be in flight runs on a replica of the plan -- the same
 * description built again, with its own workspace (~8 % of one image) -- created on first need and kept for later
 * executes; an execute finds the instance that last ran on its stream (stream order separates the two), else one whose
 * last execution has finished (hipEventQuery), else builds a replica.  So rf_plan_execute may be called on distinct
 * streams, and from distinct host threads, without the executions waiting for one another (the call that builds a replica
 * takes the host time of a plan creation once; it does not wait for the device).  rf_plan_workspace_bytes reports one instance.  The stepping calls below belong to the
 * host thread that called rf_plan_begin, until its rf_plan_finish (or rf_plan_abort).
 *
 * in_planes/out_planes: n_planes device pointers each.  in == out (same pointers) is allowed.  A plan whose kernels
 * move 16 bytes per lane -- the fused path (rf_plan_path() == RF_PATH_TILED_FUSED) and the line-parallel untiled
 * kernels RF_PATH_AUTO / RF_PATH_UNTILED use for orders <= 3 with extents that are multiples of 16 -- needs 16-byte
 * aligned planes (4-byte for RF_IN_U8 input planes and for both sides of RF_IO_U8) and returns RF_ERR_INVALID_ARG otherwise (hipMalloc and torch
 * allocations are 256-byte aligned; only offset views are affected).  The generic and overlapped tiled paths take any
 * element-aligned pointer. */
int rf_plan_execute(rf_plan *plan, const void *const *in_planes, void *const *out_planes,
                    void *stream);

/* Same, but brackets every kernel with HIP events on `stream` and returns per-kernel
 * milliseconds in ms_out[0..n) (n = rf_plan_num_kernels) and their names in names_out
 * (pointers stay valid for the life of the plan).  Synchronises the stream. */
int rf_plan_execute_timed(rf_plan *plan, const void *const *in_planes, void *const *out_planes,
                          void *stream, float *ms_out, const char **names_out, int capacity);

/* ---- sharded execution: the same work as rf_plan_execute split at the exchange points ----- */
/* For a plan with shard_world > 1 the scans along the outermost dimension need the carry of
 * the neighbouring slab.  Protocol, per execute (all calls asynchronous on the begin() stream):
 *     rf_plan_begin(...)                         pass 1 + every slab-local carry stage
 *     for e in 0 .. rf_plan_num_exchanges()-1:   ONE for all scans of the sharded dimension (orders <= 3, at most
 *                                                4 scans, scans * world * order <= 128), else one per scan
 *                                                (RF_PATH_TILED_MATRIX: always one per scan along the sharded dimension)
 *         rf_plan_exchange_local(e, send)        slab-local recurrence; writes this slab's exit
 *                                                carries (rf_plan_exchange_bytes(e) bytes) to `send`
 *         -- caller all-gathers `send` over the ranks into `gathered` (world * bytes, rank-major;
 *            RCCL all-gather on the same stream) --
 *         rf_plan_exchange_apply(e, gathered)    forms the incoming carry; what it adds to the slab's tails is
 *                                                applied here, or by the final pass as it loads a carry (fused 2-D)
 *     rf_plan_finish(...)                        final correction pass
 * Work that does not depend on the exchange: between ISSUING the last all-gather and WAITING for it, call
 *     rf_plan_interior(plan)
 * A z-sharded volume (fused x/y stage + strided z stage, merged exchange, no pointwise stages) exchanges the z carries
 * of the RAW input -- the z operators commute with the x/y filter -- so its whole x/y stage is such work and runs beside
 * the collective; afterwards exchange_apply filters the few carry planes along x/y.  A caller whose all-gather is
 * asynchronous with respect to the begin() stream (RCCL on its own stream; torch.distributed with async_op=True) gets a
 * step of max(kernels, exchange) instead of their sum.  rf_plan_has_interior() tells whether a plan has such work; the
 * call is optional -- exchange_apply / finish run whatever is still pending -- and a no-op for plans without any.
 * `send` and `gathered` are caller-owned device buffers.  With shard_world == 1 the apply step
 * is a no-op and may be skipped.  Slabs may have different extents along the sharded dimension
 * (rf_filter_desc.shard_extents: a slab's exit carry is propagated across the slabs between it and the
 * receiver with one transfer table per slab); the exchanged bytes per rank do not depend on them. */
int rf_plan_num_exchanges(const rf_plan *plan);
size_t rf_plan_exchange_bytes(const rf_plan *plan, int exchange);
int rf_plan_begin(rf_plan *plan, const void *const *in_planes, void *const *out_planes, void *stream);
int rf_plan_exchange_local(rf_plan *plan, int exchange, void *send);
int rf_plan_exchange_apply(rf_plan *plan, int exchange, const void *gathered);
int rf_plan_has_interior(const rf_plan *plan);
int rf_plan_interior(rf_plan *plan);
int rf_plan_finish(rf_plan *plan);
/* Abandons the execute this host thread began with rf_plan_begin and did not finish (the caller's collective failed, an
 * exception unwound between the calls): the execution instance goes back to the plan's pool; kernels already enqueued still
 * run, the output planes are undefined.  A no-op without such an execute.  rf_plan_begin does the same to an unfinished
 * execute of the calling thread before it starts a new one, and rf_plan_destroy may be called in any state. */
int rf_plan_abort(rf_plan *plan);

/* ---- plan tables (host side of the tiling algebra; also what the CPU tests inspect) ------- */
/* Copies a named table into out (as doubles) and returns its element count through n_out;
 * pass out = NULL to query the size.  Names are documented in DESIGN.md ("plan tables").
 * "scans" lists the scans the plan EXECUTES, one row of 5 + 2 * RF_MAX_ORDER doubles each: where the plan rewrote the filter --
 * merged runs of a 1-D signal (one scan per run, RF_PLAN_NO_OVERLAP forbids it), sections of order <= 3 in place of a scan of
 * order 4..8 (RF_PLAN_NO_SECTIONS), the first stage of an in-plan cascade -- these are not the scans the caller gave.
 * "neighbour_carries" (fused x/y plans): {bound x, taken x, bound y, taken y} -- the largest part of a consumed carry the
 * neighbour form would drop, relative to the largest carry (-1: the dimension cannot take that form), and 1 / 0 for whether
 * the plan runs it (RF_PLAN_FULL_CARRY_SCAN). */
int rf_plan_table(const rf_plan *plan, const char *name, double *out, size_t capacity, size_t *n_out);

/* Debugging aids.  rf_plan_debug_buffer: device pointer and size of the i-th device buffer an execute of the plan's first
 * instance uses -- the plan's own (tables, tails, carries, staging planes; in allocation order), then those of the plans it
 * drives as stages (cascade stages, the f32 plan inside a staged 16-bit plan, the zero-border plan of a clamped signal) and
 * of its helper plans, depth first; RF_ERR_INVALID_ARG past the last one.  A host-only plan lists what it would have
 * allocated, with null pointers.
 * rf_plan_debug_buffer_kind: how the buffer was made.  RF_BUFFER_SCRATCH buffers hold samples, tails or carries in the plan's
 * arithmetic type and are written by every execute before it reads them; they hold no index, count or flag.
 * rf_plan_debug_fill: sets every byte of a zeroed or scratch buffer to `byte` (0..255), asynchronously on `stream`;
 * RF_ERR_INVALID_ARG for a table.  Filling a ZEROED buffer with anything but 0 breaks the plan; filling SCRATCH with any
 * byte must not change any result (tests/test_gpu_footprint.py). */
enum rf_buffer_kind { RF_BUFFER_TABLE = 0, RF_BUFFER_ZEROED = 1, RF_BUFFER_SCRATCH = 2 };
int rf_plan_debug_buffer(const rf_plan *plan, int index, void **ptr_out, size_t *bytes_out);
int rf_plan_debug_buffer_kind(const rf_plan *plan, int index, int *kind_out);
int rf_plan_debug_fill(rf_plan *plan, int index, int byte, void *stream);

/* ---- backward: the gradient of a loss through a plan ---------------------------------------------------------------------- */
/* Given grad_out = dL/d(out) of an execute, grad_in = dL/d(in) and, where asked for, the gradient with respect to every
 * coefficient of every scan.  Per line, in scan order r = 0 .. n-1 (an anticausal scan: the reversed line), a scan with input u,
 * output y, feed-forward c0 and feedback a_0 .. a_{k-1} is
 *     y[r] = c0 u[r] + sum_{j < r} a_j y[r-j-1]                                   zero border
 *          + t_r (r == 0 ? u[0] : y[0])  for r < k,   t_r = sum_{j >= r} a_j       clamped border
 * With g = dL/dy and mu the unit-gain zero-border scan of g in the OPPOSITE direction (same feedback, feed-forward 1):
 *     dL/du = c0 mu;    clamped: dL/du[0] += t_0 mu[0] + gamma sum_{1 <= r < k} t_r mu[r],   gamma = c0 + t_0
 *     dL/da_j = sum_{r > j} mu[r] y[r-j-1];    clamped: + beta + mu[0] u[0] + y[0] sum_{1 <= r <= j} mu[r]
 *     dL/dc0  = sum_r mu[r] u[r];              clamped: + beta,    beta = u[0] sum_{1 <= r < k} t_r mu[r]
 * summed over all lines and all planes (the planes share the coefficients); the scans' adjoints run in reverse order.  The
 * affine stages compose: out = pf F(ps in + pb) + pi (ps in + pb) + po gives grad_in = pf F^T(ps g) + pi ps g.
 *
 * grad_coeffs: NULL, or a DEVICE buffer of n_scans * (1 + RF_MAX_ORDER) doubles; row s holds dL/dfeedfwd and then
 * dL/dfeedback[j] of the caller's scan s, entries past the order are 0.  It lives on the device so that a backward call never
 * synchronises and can be captured into a graph like an execute (the FIRST call of each kind builds child plans and, with
 * grad_coeffs, allocates: make it outside a capture).  in_planes is needed exactly when grad_coeffs is given and must be NULL
 * otherwise.  grad_in[p] == grad_out[p] is allowed.
 *
 * Three routes, built by the first call that needs them (plan creation costs what it did) and freed with the plan:
 *   1. zero border, no grad_coeffs: ONE adjoint plan -- the caller's description with the scans reversed and every direction
 *      flipped, the same path, tiles and flags, prologue (ps, 0) and epilogue (pf, pi, 0).  The launch list is that plan's.
 *   2. clamped border, no grad_coeffs: per scan in reverse order a single-scan zero-border plan (feed-forward c0) and one
 *      "adjoint_border" launch that touches the first k samples of every line; in place on grad_in behind the first scan.
 *   3. with grad_coeffs: the forward rerun scan by scan (single-scan plans with the caller's border) into plan-owned planes, every
 *      scan's output kept; then per scan in reverse order a unit-gain single-scan plan (mu), "coeff_grad" (one streaming pass
 *      over mu, u and y, 16-byte loads, f64 sums, one slab of 1 + k doubles per workgroup; it also stores c0 mu, the next
 *      gradient: 16 bytes per sample in all; under a clamped border its lanes then add the clamp terms, one line per lane),
 *      "coeff_grad_sum" (one workgroup: the slabs in index order) and, clamped, "adjoint_border".  No atomics anywhere: two calls agree bit for bit, whatever else runs.  grad_in of route 3
 *      equals that of routes 1 / 2 up to rounding and is NOT bit-identical: it is formed scan by scan as fl(c0 * mu) behind a
 *      unit-gain scan, where routes 1 / 2 run the fused plan / scans with feed-forward c0.
 * rf_plan_backward_timed lists the launches in execution order -- the child plans' own step names, "coeff_grad",
 * "coeff_grad_sum", "adjoint_border" -- and synchronises the stream; rf_plan_backward_num_kernels(plan, with_coeffs) is the
 * length of that list (0 for a plan the backward refuses).  rf_plan_backward_workspace_bytes(plan, with_coeffs): 0 without
 * coefficients; with them (n_scans + 1) image sets of n_planes f32 planes and the slabs (1024 * (1 + RF_MAX_ORDER) doubles),
 * allocated by the first call that needs them.  The child plans' own tails and carries come on top and are not counted;
 * rf_plan_workspace_bytes, rf_plan_debug_buffer*, rf_plan_num_kernels and the plan tables do not change.
 * Backward calls of one plan are ordered by the caller (one stream, or the caller's synchronisation), as for
 * rf_var_plan_backward; forward executes keep their instance pool and may run beside them.
 *
 * Refused, before any HIP call and in this order:
 *   null plan / grad_out_planes / grad_in_planes or a null plane; in_planes NULL with grad_coeffs or given without it
 *                                                                                        RF_ERR_INVALID_ARG
 *   planes that are not aligned as rf_plan_execute asks for the plan's path (16 bytes on the fused path and the line-parallel
 *   kernels, except images whose width is not a multiple of 4); grad_coeffs not 8-byte aligned   RF_ERR_INVALID_ARG
 *   a written plane (grad_in, grad_coeffs) that overlaps any other plane of the call, except grad_in[p] being exactly
 *   grad_out[p] (which an epilogue with post_input != 0 does not allow either)              RF_ERR_INVALID_ARG
 *   dtype != RF_F32                                                                          RF_ERR_UNSUPPORTED
 *   in_dtype != RF_IN_PIXEL                                                                  RF_ERR_UNSUPPORTED
 *   shard_world > 1 or RF_PLAN_FORCE_EXCHANGE                                                RF_ERR_UNSUPPORTED
 *   grad_coeffs on a plan with pointwise stages                                              RF_ERR_UNSUPPORTED
 *   clamped border with an extent <= the order of a scan along that dimension, or with feedfwd == 0 (route 2 divides by it);
 *   clamped border with pointwise stages; grad_coeffs on a plan without scans                RF_ERR_UNSUPPORTED
 *   a host-only plan                                                                         RF_ERR_HIP
 * Out of scope: f64, integer, 16-bit and byte pixels; sharded plans; coefficient gradients through pointwise stages; pointwise
 * stages on a clamped plan; a derivative with respect to the sigma of rf_gaussian_weights; second derivatives; fusing the
 * clamped route's scans.  Routes 2 and 3 are not tuned for time. */
int    rf_plan_backward(rf_plan *plan, const void *const *in_planes, const void *const *grad_out_planes,
                        void *const *grad_in_planes, double *grad_coeffs, void *stream);
int    rf_plan_backward_timed(rf_plan *plan, const void *const *in_planes, const void *const *grad_out_planes,
                              void *const *grad_in_planes, double *grad_coeffs, void *stream, float *ms_out,
                              const char **names_out, int capacity);
int    rf_plan_backward_num_kernels(rf_plan *plan, int with_coeffs);
size_t rf_plan_backward_workspace_bytes(rf_plan *plan, int with_coeffs);

/* ---- coefficient design (lib/iir_coeff.cpp:162-177, 222-234, 236-263, 205-220) ------------ */
int rf_gaussian_weights(float sigma, int order, float *coeff_out /* order+1 */);
int rf_integral_image_coeff(int n, float *coeff_out /* n+1 */);
int rf_overlap_feedback_coeff(const float *a, int na, const float *b, int nb, float *c_out /* na+nb */);
int rf_gaussian_box_filter(int k, float sigma, int *width_out);

/* ---- finite differences of summed-area tables (iterated box filters) --------------------- */
/* The consumer of the reference's box-filter apps (apps/box/box_filter.h:36-39, 128-139; apps/DoG/diff_gauss.cpp:
 * 132-150): along every dimension d, order[d] times,
 *     out(i) = (s(min(i + radius, N-1)) - s(max(i - radius - 1, 0))) / (2*radius + 1)
 * with s a summed-area table of matching order (rf_integral_image_coeff).  The nested clamps are evaluated exactly
 * as written there.  order[d] in 0..2.  One elementwise kernel over dense x-fastest device planes; float pixel types.
 * in == out is NOT allowed (the operator gathers). */
int rf_box_difference(const void *in, void *out, int ndim, const int64_t *extent, int dtype, int radius,
                      const int32_t *order, void *stream);

/* ---- clamped tap combinations (the other pointwise-with-offsets Funcs of the reference's apps) -------- */
/* HARNESS UTILITY, OUTSIDE THE HOT PATH: SURVEY.md 2c marks apps/DoG out of scope; this entry point exists so that
 * tools/profile_app.py can run the reference's diff_gauss app end to end on device buffers.  Nothing of the tiled
 * recursive-filter path (plans, kernels, sharding) uses it; a drop-in integration does not need to bind it. */
/* out(p) = sum_t weight_t * in_planes[plane_t]( clamp(p + offset_t) ),  clamp per dimension to [0, extent-1].
 * Covers every difference operator the apps put behind a summed-area table that rf_box_difference does not:
 * apps/DoG/diff_gauss.cpp:176-197 (diff_op_x / diff_op_y: taps +B, -1 (twice), -2B-2, one division; diff_op_xy with two
 * radii on one table; the final difference of two planes).  At most RF_MAX_TAPS taps over at most RF_MAX_PLANES input
 * planes; dense x-fastest device planes of one floating-point type; `out` must not alias an input.  One gather kernel. */
#define RF_MAX_TAPS 16
typedef struct {
    int32_t plane;                    /* index into in_planes                                      */
    int32_t offset[RF_MAX_DIMS];      /* per dimension, x first                                    */
    float   weight;
} rf_tap;
int rf_tap_filter(const void *const *in_planes, int n_in, void *out, int ndim, const int64_t *extent, int dtype,
                  const rf_tap *taps, int n_taps, void *stream);

/* ---- measured copy ceiling ("also report against a measured stream-copy ceiling") ---------- */
/* MEASUREMENT UTILITY: the final pass of the fused path with its arithmetic taken out -- every 256 x 128 tile of a dense f32
 * image of `rows` x `width` samples (width a multiple of 256, rows a multiple of 128) read with 16-byte non-temporal loads and
 * written with 16-byte non-temporal stores by one workgroup of 256 threads, eight loads per thread in flight.  What a
 * read-once / write-once pass over an image reaches on the device it runs on: bench.py times it beside the filter
 * (roofline.copy_ceiling_gbps).  src != dst.  Nothing of the filter path calls it. */
int rf_stream_copy(const float *src, float *dst, int64_t width, int64_t rows, void *stream);

/* ---- spatially varying first-order scans (edge-aware smoothing) ------------------------------------------------------ */
/* A recurrence whose feedback changes from sample to sample: what the domain-transform recursive filter (Gastal & Oliveira
 * 2011) runs along x and along y with a per-pixel feedback a^d.  Nothing of rf_filter_desc can express it (a plan there turns
 * CONSTANT coefficients into tables); this family stands beside it, with the same three-stage tiling (tile-local tails, the
 * carry recurrence across tiles, a correction pass) whose carry operators are read from a weight plane.
 *
 * Planes are dense f32, x fastest, 2-D.  A weight plane has the image's extents; element i along the scanned dimension holds
 * the coupling between sample i-1 and sample i; element 0 is NEVER USED (it is masked by a select: a NaN stored there reaches
 * no output).  Values are expected in [0, 1]; anything else is the caller's business and NaN propagates.  With w~[0] = 0,
 * w~[N] = 0 and w~[i] = w[i] otherwise, along a line x[0..N):
 *     causal      (+d):  y[i] = (1 - w~[i])   * x[i] + w~[i]   * y[i-1]     i = 0 .. N-1   (y[0]   = x[0])
 *     anticausal  (-d):  y[i] = (1 - w~[i+1]) * x[i] + w~[i+1] * y[i+1]     i = N-1 .. 0   (y[N-1] = x[N-1])
 * A plan is a list of at most RF_VAR_MAX_SCANS scans (dim, causal, weights), applied in the order given; `weights` indexes the
 * weight planes handed to execute.  All n_planes image planes share the weight planes (the channels of an RGB image see the
 * same edges).  A +d scan directly followed by the -d scan of the same dimension and weight plane runs as ONE stage where
 * the two are a run of their own (the scans before and behind them, if any, are along the other dimension); every other scan
 * is a stage of its own (-d +d: two stages; +d -d +d along one dimension: three).  Every
 * stage is three launches ("var_tails_x|y", "var_carry", "var_pass2_x|y": rf_var_plan_num_kernels = 3 per stage).  The first
 * stage reads `in`, later stages filter `out` in place.  in == out is allowed; a weight plane must not overlap an output plane;
 * image and weight planes must be 16-byte aligned (RF_ERR_INVALID_ARG otherwise).
 * The plan owns ONE workspace (tails and carries, about 7/64 of the image planes): executes of one plan are ordered by the
 * caller -- one stream, or the caller's own synchronisation; concurrent executes of one plan are not supported.
 * Refused: ndim != 2, dtype != RF_F32, a width that is not a multiple of 4 (RF_ERR_UNSUPPORTED); abi != RF_ABI, n_scans outside
 * 1..RF_VAR_MAX_SCANS, dim outside 0..1, weights outside 0..n_weights-1, n_planes outside 1..RF_MAX_PLANES, n_weights outside
 * 1..RF_VAR_MAX_SCANS, extents below 1, nonzero flags (RF_ERR_INVALID_ARG).  A host-only plan (device = RF_DEVICE_HOST_ONLY)
 * answers the queries and refuses to execute with RF_ERR_HIP. */
#define RF_VAR_MAX_SCANS 8
typedef struct {
    int32_t dim;                      /* 0 = x (fastest), 1 = y                                  */
    int32_t causal;                   /* 1 = +dim, 0 = -dim                                      */
    int32_t weights;                  /* index into the weight planes                            */
} rf_var_scan_desc;
typedef struct {
    int32_t  ndim;                    /* 2                                                       */
    uint32_t abi;                     /* RF_ABI                                                  */
    int64_t  extent[RF_MAX_DIMS];     /* extent[0] = width (x)                                   */
    int32_t  dtype;                   /* RF_F32                                                  */
    int32_t  n_planes;                /* 1..RF_MAX_PLANES                                        */
    int32_t  n_weights;               /* 1..RF_VAR_MAX_SCANS                                     */
    int32_t  n_scans;
    const rf_var_scan_desc *scans;    /* in application order                                    */
    int32_t  device;                  /* HIP device ordinal, -1 = current, RF_DEVICE_HOST_ONLY   */
    uint32_t flags;                   /* 0                                                       */
} rf_var_desc;
typedef struct rf_var_plan rf_var_plan;
int    rf_var_plan_create(const rf_var_desc *desc, rf_var_plan **plan_out);
int    rf_var_plan_destroy(rf_var_plan *plan);
size_t rf_var_plan_workspace_bytes(const rf_var_plan *plan);
int    rf_var_plan_num_kernels(const rf_var_plan *plan);
/* in_planes / out_planes: n_planes device pointers each; weight_planes: n_weights device pointers.  Asynchronous on `stream`. */
int    rf_var_plan_execute(rf_var_plan *plan, const void *const *in_planes, const void *const *weight_planes,
                           void *const *out_planes, void *stream);
/* as rf_plan_execute_timed: per-kernel milliseconds and names (valid for the life of the plan); synchronises the stream */
int    rf_var_plan_execute_timed(rf_var_plan *plan, const void *const *in_planes, const void *const *weight_planes,
                                 void *const *out_planes, void *stream, float *ms_out, const char **names_out, int capacity);
/* The power form.  As rf_var_plan_execute, but plane k of `exponent_planes` holds exponents d >= 0 (+inf allowed) and the weight
 * a scan uses is
 *     w[i] = exp2f(d[i] * l_k),   l_k = (float)log2((double)bases[k]),   0 < bases[k] < 1,
 * formed in f32 as the kernels load the plane (one multiply, one hardware exp2 of 1 ulp whose denormal results flush to 0); no
 * weight plane is ever stored.  d = 0 gives w = 1 exactly, d = +inf gives w = 0 exactly.  Element 0 along the scanned dimension
 * is still never used (a select: NaN there reaches nothing).  Same plan object, workspace, stages, launch names and
 * rf_var_plan_num_kernels as rf_var_plan_execute: a plan may be run either way, call by call.  What the domain-transform filter
 * needs per iteration k is then two exponent planes (rf_var_distances) shared by all iterations and bases = {a_k, a_k}.
 * Checked in this order: null arrays; a base that is not finite or not inside (0, 1) (RF_ERR_INVALID_ARG, the message names the
 * plane); a host-only plan (RF_ERR_HIP); then the per-plane checks of rf_var_plan_execute. */
int    rf_var_plan_execute_power(rf_var_plan *plan, const void *const *in_planes, const void *const *exponent_planes,
                                 const float *bases /* n_weights */, void *const *out_planes, void *stream);
int    rf_var_plan_execute_power_timed(rf_var_plan *plan, const void *const *in_planes, const void *const *exponent_planes,
                                       const float *bases, void *const *out_planes, void *stream, float *ms_out,
                                       const char **names_out, int capacity);
/* The adjoint of a plan run by rf_var_plan_execute (the plane form): given grad_out = dL/d(out), grad_in = dL/d(in) and, where
 * asked for, dL/d(weight plane).  With g the gradient that enters a scan's adjoint, along a line:
 *     causal scan       lam[i] = g[i] + w~[i+1] lam[i+1]   (anticausal, unit input gain)     dL/dx[i] = (1 - w~[i])   lam[i]
 *                       dL/dw[i] = lam[i] (y[i-1] - x[i])      i = 1 .. N-1;  element 0: 0
 *     anticausal scan   mu[i]  = g[i] + w~[i]   mu[i-1]    (causal, unit input gain)         dL/dx[i] = (1 - w~[i+1]) mu[i]
 *                       dL/dw[i] = mu[i-1] (y[i] - x[i-1])     i = 1 .. N-1;  element 0: 0
 * The scans' adjoints run in reverse order, always scan by scan (no fused pair).  The gradient of a weight plane is the sum over
 * the scans that read it and over the image planes (planes in index order, in f32, in a register: no atomics -- two runs of one
 * call agree bit for bit).
 * grad_weight_planes = NULL or all entries NULL: 3 launches per scan ("var_adj_tails_x|y", "var_carry", "var_adj_pass2_x|y"); the
 * first stage reads grad_out, later stages run in place on grad_in; grad_out[pl] == grad_in[pl] is allowed; in_planes may be NULL;
 * no workspace beyond the plan's.
 * Otherwise in_planes is needed: the forward is rerun scan by scan ("var_tails_*", "var_carry", "var_pass2_*", 3 per scan) with
 * every scan's output kept, then per scan in reverse order the adjoint stage, which also stores lam, and one "var_grad_x|y"
 * launch: 7 launches per scan.  A weight plane whose entry is NULL gets no gradient and its var_grad launches are skipped (the
 * timed form reports 0 ms for them).  The (n_scans + 1) * n_planes extra planes are allocated by the first call that needs them
 * and freed with the plan: rf_var_plan_backward_workspace_bytes(plan, 1); rf_var_plan_workspace_bytes does not count them.
 * rf_var_plan_backward_num_kernels(plan, with_weight_gradients): 3 n_scans, or 7 n_scans.
 * The plan's one workspace is used: order backward calls with the plan's executes.  Checked in this order, before any HIP call:
 * null plan / weight_planes / grad_out_planes / grad_in_planes; a weight gradient asked for with in_planes NULL
 * (RF_ERR_INVALID_ARG); a host-only plan (RF_ERR_HIP); null or not 16-byte aligned planes; a grad_in plane or a gradient plane
 * that overlaps a weight plane, an input plane, another grad_in or gradient plane, or a grad_out plane -- except grad_in[pl]
 * being exactly grad_out[pl] (RF_ERR_INVALID_ARG; the message names the planes). */
int    rf_var_plan_backward(rf_var_plan *plan, const void *const *in_planes, const void *const *weight_planes,
                            const void *const *grad_out_planes, void *const *grad_in_planes,
                            void *const *grad_weight_planes /* NULL, or n_weights entries each NULL or a plane */, void *stream);
int    rf_var_plan_backward_timed(rf_var_plan *plan, const void *const *in_planes, const void *const *weight_planes,
                                  const void *const *grad_out_planes, void *const *grad_in_planes, void *const *grad_weight_planes,
                                  void *stream, float *ms_out, const char **names_out, int capacity);
/* The adjoint of a plan run by rf_var_plan_execute_power (the power form).  As rf_var_plan_backward, with exponent_planes and bases
 * in the place of weight_planes and grad_exponent_planes in the place of grad_weight_planes.  A scan uses
 *     w[i] = exp2f(d[i] * l_k),   l_k = (float)log2((double)bases[k])
 * formed in the kernels exactly as rf_var_plan_execute_power forms it; the image gradient is the plane form's adjoint on those
 * weights, and the gradient of an exponent plane is
 *     dL/dd[i] = (w[i] * c_k) * dL/dw[i],   c_k = (float)log((double)bases[k]),
 * dL/dw the quantity rf_var_plan_backward forms and w recomputed from d by the same hardware exp2.  d is never a factor: d = +inf
 * gives w = 0 and a gradient of exactly 0, d = 0 gives c_k * dL/dw.  Element 0 along the scanned dimension is 0 by a select (a NaN
 * exponent there reaches nothing).  Launch lists, names, workspace, rf_var_plan_backward_num_kernels and
 * rf_var_plan_backward_workspace_bytes are those of rf_var_plan_backward; one plan runs either form, call by call; the first
 * var_grad launch that touches a gradient plane stores, later ones add: no atomics, bit-reproducible.  Checked in the order of
 * rf_var_plan_backward, with the base check of rf_var_plan_execute_power (each base finite and inside (0, 1), RF_ERR_INVALID_ARG,
 * the message names the plane) directly before the host-only check. */
int    rf_var_plan_backward_power(rf_var_plan *plan, const void *const *in_planes, const void *const *exponent_planes,
                                  const float *bases /* n_weights */, const void *const *grad_out_planes, void *const *grad_in_planes,
                                  void *const *grad_exponent_planes /* NULL, or n_weights entries each NULL or a plane */, void *stream);
int    rf_var_plan_backward_power_timed(rf_var_plan *plan, const void *const *in_planes, const void *const *exponent_planes,
                                        const float *bases, const void *const *grad_out_planes, void *const *grad_in_planes,
                                        void *const *grad_exponent_planes, void *stream, float *ms_out, const char **names_out,
                                        int capacity);
int    rf_var_plan_backward_num_kernels(const rf_var_plan *plan, int with_weight_gradients);
size_t rf_var_plan_backward_workspace_bytes(const rf_var_plan *plan, int with_weight_gradients);
/* rf_var_plan_backward_power with the gradient of the BASES: the weight-gradient route of rf_var_plan_backward_power, whose var_grad
 * launches also reduce, and one more launch.  grad_bases is a DEVICE buffer of n_weights doubles, 8-byte aligned; entry k receives
 *     dL/dbases[k] = (1 / bases[k]) * sum over the scans that read plane k, over the image planes and over i, of t[i],
 *     t[i] = (w[i] == 0 ? 0 : d[i] * w[i] * dL/dw[i]),
 * dL/dw the register sum over the image planes that rf_var_plan_backward_power multiplies by w ln(base).  d is never a factor
 * where w is 0 (d = +inf contributes exactly 0, the rule dL/dd follows) and element 0 along the scanned dimension contributes 0 by
 * the same select as there.  The roundings of log2(bases[k]) to f32 are treated as the identity.  An entry whose plane no scan
 * reads is 0.  The sum is a streaming f64 reduction without atomics: a lane adds its t in the order it visits its rows, a workgroup
 * folds its lanes by a fixed tree and stores one f64 slab entry at an index that depends on (its block, the scan) alone, and the
 * last launch, one workgroup, sums the slabs in index order and multiplies by 1 / bases[k], formed on the host in double.  Nothing
 * synchronises; two runs of one call agree bit for bit.
 * Entries of grad_exponent_planes, or the whole array, may be NULL: the reduction still runs and that plane's store is left out
 * (no var_grad launch is skipped here).  grad_in and every exponent gradient asked for are bit for bit rf_var_plan_backward_power's.
 * Image, signal and volume plans alike.
 * Launches, in order: the 7 n_scans of rf_var_plan_backward_power with exponent gradients, then "var_param_sum":
 * rf_var_plan_backward_bases_num_kernels(plan) = 7 n_scans + 1.  The slabs are the plan's, one double per workgroup of every
 * var_grad launch, allocated by the first call that needs them and freed with the plan;
 * rf_var_plan_backward_bases_workspace_bytes(plan) is exact: rf_var_plan_backward_workspace_bytes(plan, 1) plus 8 bytes per slab
 * entry (a var_grad launch of w x h samples on b images or slices has ceil(w / 1024) * min(h, 65535) * b workgroups).
 * Checked in the order of rf_var_plan_backward_power: null plan / exponent_planes / bases / grad_out_planes / grad_in_planes; null
 * in_planes; directly behind these null grad_bases, then a grad_bases that is not 8-byte aligned (RF_ERR_INVALID_ARG); then the
 * base check, the host-only plan (RF_ERR_HIP) and the per-plane checks.  grad_bases must not overlap any plane of the call (not
 * checked). */
int    rf_var_plan_backward_power_bases(rf_var_plan *plan, const void *const *in_planes, const void *const *exponent_planes,
                                        const float *bases /* n_weights */, const void *const *grad_out_planes, void *const *grad_in_planes,
                                        void *const *grad_exponent_planes /* NULL, or n_weights entries each NULL or a plane */,
                                        double *grad_bases /* device, n_weights doubles */, void *stream);
int    rf_var_plan_backward_power_bases_timed(rf_var_plan *plan, const void *const *in_planes, const void *const *exponent_planes,
                                              const float *bases, const void *const *grad_out_planes, void *const *grad_in_planes,
                                              void *const *grad_exponent_planes, double *grad_bases, void *stream, float *ms_out,
                                              const char **names_out, int capacity);
int    rf_var_plan_backward_bases_num_kernels(const rf_var_plan *plan);
size_t rf_var_plan_backward_bases_workspace_bytes(const rf_var_plan *plan);
/* The varying scans on long 1-D SIGNALS.  rf_var_plan_create refuses ndim = 1, and a (1, N) image fills one lane of a wave; this
 * entry point builds an ordinary rf_var_plan whose "plane" is a dense f32 signal of `length` samples: execute, execute_power,
 * backward, backward_power, their timed forms, the four queries and destroy work on it as above.  The operator is the one above
 * with N = length: w~[0] = w~[N] = 0 by selects, element 0 of a weight signal is never used (a NaN there reaches nothing), every
 * scan has dim 0, and a +x scan directly followed by -x on one weight signal, where the two are the whole list, is one stage.
 * in == out is allowed; a weight signal must not overlap an output; signals are 16-byte aligned.
 * Tiling: a lane owns 64 consecutive samples, a wave a group of 64 such tiles (4096 samples).  A stage is three launches,
 * "var_tails_1d" (tile tails, then a scan of them across the wave: every lane stores the affine map from the carries that enter
 * its group to those that enter its tile, one lane the group's aggregate), "var_carry_1d" (the carry recurrences over groups, one
 * workgroup per plane sweeping 1024 groups at a time) and "var_pass2_1d" (reruns the recurrences from the carries; weights of
 * exactly 0 and 1 stay exact).  No kernel waits on another workgroup; results are reproducible bit for bit.
 * rf_var_plan_num_kernels = 3 per stage; rf_var_plan_backward_num_kernels = 3 n_scans ("var_adj_tails_1d", "var_carry_1d",
 * "var_adj_pass2_1d") or 7 n_scans (with the forward's three and "var_grad_x").  rf_var_plan_workspace_bytes is exact:
 * 4 * n_planes * (5 * (tiles + groups) + 2 * groups) bytes, tiles = ceil(length / 64), groups = ceil(tiles / 64) -- below 1/8 of
 * the signal planes from one full group (4096 samples) on.
 * Refused before any HIP call, the message naming the field: length not a multiple of 4 or above 2^30, dtype != RF_F32
 * (RF_ERR_UNSUPPORTED); abi != RF_ABI, nonzero flags, n_planes / n_weights / n_scans outside their ranges, null scans, a scan
 * with dim != 0 or weights outside 0..n_weights-1, length below 1 (RF_ERR_INVALID_ARG).  A host-only plan answers the queries and
 * refuses to run with RF_ERR_HIP.
 * Out of scope: lengths that are not multiples of 4 (pad with zero samples and zero weights: a weight of 0 decouples exactly);
 * batches of long signals with weights of their own (many short lines are the x scans of a 2-D plan); byte and 16-bit signals;
 * rf_smooth_plan and rf_var_distances on signals (their extent limit of 2^21 stays); orders above 1 (order 2: rf_var2_plan_*
 * below); sharding. */
typedef struct {
    uint32_t abi;                     /* RF_ABI                                                  */
    int64_t  length;                  /* samples per signal: a multiple of 4, 4 .. 2^30          */
    int32_t  dtype;                   /* RF_F32                                                  */
    int32_t  n_planes;                /* signals that share the weight signals, 1..RF_MAX_PLANES */
    int32_t  n_weights;               /* 1..RF_VAR_MAX_SCANS                                     */
    int32_t  n_scans;                 /* 1..RF_VAR_MAX_SCANS                                     */
    const rf_var_scan_desc *scans;    /* dim must be 0                                           */
    int32_t  device;                  /* HIP device ordinal, -1 = current, RF_DEVICE_HOST_ONLY   */
    uint32_t flags;                   /* 0                                                       */
} rf_var_signal_desc;
int    rf_var_plan_create_signal(const rf_var_signal_desc *desc, rf_var_plan **plan_out);
/* The varying scans on VOLUMES.  rf_var_plan_create refuses ndim = 3; this entry point builds an ordinary rf_var_plan whose
 * "plane" is a dense f32 volume [z][y][x] of width x height x depth samples, 16-byte aligned: execute, execute_power, backward,
 * backward_power, their timed forms, the four queries and destroy work on it as above.  A weight plane is a volume of the same
 * size; dim is 0 (x), 1 (y) or 2 (z).  The operator is the one above along the chosen axis: w~[0] = w~[N] = 0 by selects, and
 * element 0 along the scanned axis -- column 0, row 0 or slice 0 -- is never used (a NaN there reaches nothing).  Stages form as
 * above: a run {+d, -d} on one weight volume, alone along d, is one pair stage; every other run goes scan by scan.
 * The arithmetic of a line does not depend on its container.  An x or y stage takes the `depth` slices as a batch on gridDim.z
 * beside the planes (slice strides of width * height samples; tails and carries slice after slice in the single-image layout):
 * every slice is, bit for bit, what the 2-D plan of width x height gives on it.  A z stage runs the y kernels on the
 * (width * height) x depth view, one voxel column per lane, rows width * height samples apart: bit for bit the y scans of a 2-D
 * plan on that image.  Three launches per stage whatever the depth: "var_tails_x|y|z", "var_carry", "var_pass2_x|y|z"; the
 * backward adds "var_adj_tails_z", "var_adj_pass2_z" and "var_grad_z" to the names above.
 * rf_var_plan_workspace_bytes is exact: 4 * n_planes * (5 + 2) * slots bytes, slots = max over the dimensions d the plan scans of
 * ceil(n_d / 64) * (width * height * depth / n_d).  rf_var_plan_backward_workspace_bytes(plan, 1) is (n_scans + 1) * n_planes
 * volumes.
 * Refused before any HIP call, the message naming the limit: a width that is not a multiple of 4; an extent above 2^21;
 * width * height above 2^30 (a z scan indexes its lines in 32 bits); depth * n_planes above 65535 (the slices ride on gridDim.z);
 * dtype != RF_F32 (RF_ERR_UNSUPPORTED); abi != RF_ABI, nonzero flags, n_planes / n_weights / n_scans outside their ranges, null
 * scans, a scan with dim outside 0..2 or weights outside 0..n_weights-1, an extent below 1 (RF_ERR_INVALID_ARG).  A host-only
 * plan answers the queries and refuses to run with RF_ERR_HIP.
 * Out of scope: batches of volumes; byte and 16-bit volumes here (rf_smooth_plan_create_volume takes bytes); widths that are not
 * multiples of 4; orders above 1; sharding. */
typedef struct {
    uint32_t abi;                     /* RF_ABI                                                  */
    int64_t  width, height, depth;    /* x fastest; each 1 .. 2^21, width a multiple of 4        */
    int32_t  dtype;                   /* RF_F32                                                  */
    int32_t  n_planes;                /* volumes that share the weight volumes, 1..RF_MAX_PLANES */
    int32_t  n_weights;               /* 1..RF_VAR_MAX_SCANS                                     */
    int32_t  n_scans;                 /* 1..RF_VAR_MAX_SCANS                                     */
    const rf_var_scan_desc *scans;    /* dim 0, 1 or 2                                           */
    int32_t  device;                  /* HIP device ordinal, -1 = current, RF_DEVICE_HOST_ONLY   */
    uint32_t flags;                   /* 0                                                       */
} rf_var_volume_desc;
int    rf_var_plan_create_volume(const rf_var_volume_desc *desc, rf_var_plan **plan_out);
/* The three exponent volumes of the domain-transform filter from n_guide guide volumes [z][y][x], f32 or uint8, in one launch
 * ("var_distances_volume") that reads the guide once (a lane walks z with the slice before in registers):
 *     d_x, d_y      slice by slice what rf_var_distances gives on that slice, bit for bit
 *     d_z[z][r][c] = spacing_z + scale * sum_ch |g_ch[z][r][c] - g_ch[z-1][r][c]|   (z >= 1;  slice 0 holds spacing_z)
 * spacing_z, finite and > 0, is the sample distance along z in units of the x/y pitch (slice thickness; how far apart two frames
 * count); 1 = isotropic.  Refusals as rf_var_distances, with the volume domain of rf_var_plan_create_volume (n_planes = 1) in the
 * place of the 2-D extent check, a spacing_z that is not finite and positive (RF_ERR_INVALID_ARG, behind the scale check), and dz
 * in every alignment and overlap check.  Its adjoint for f32 guides is rf_var_distances_volume_backward. */
int    rf_var_distances_volume(const void *const *guide_volumes, int32_t n_guide, int32_t guide_u8, int64_t width, int64_t height,
                               int64_t depth, float scale, float spacing_z, void *dx, void *dy, void *dz, int32_t device,
                               void *stream);
/* The adjoint of rf_var_distances_volume for f32 guide volumes: from grad_dx, grad_dy, grad_dz = dL/d(d_x), dL/d(d_y), dL/d(d_z), per
 * channel, in f32 with the six terms in this order,
 *     gg[ch][z][r][c] = scale * ( ((((L - R) + U) - Dn) + B) - A )
 *     L  = sx(z,r,c) * gdx[z][r][c]        R  = sx(z,r,c+1) * gdx[z][r][c+1]
 *     U  = sy(z,r,c) * gdy[z][r][c]        Dn = sy(z,r+1,c) * gdy[z][r+1][c]
 *     B  = sz(z,r,c) * gdz[z][r][c]        A  = sz(z+1,r,c) * gdz[z+1][r][c]
 *     sx(z,r,c) = sgn(g[z][r][c] - g[z][r][c-1]) for 1 <= c < W, else 0;   sy, sz likewise along rows and slices;   sgn(0) = 0
 * (a constant guide gets a gradient of exactly 0; spacing_z is an additive constant of d_z and does not enter).  The signs are
 * applied by selects and the terms outside the volume are selected away: gdx[..][..][0], gdy[..][0][..] and gdz[0] are never part
 * of a result (a NaN there reaches nothing).  With grad_dz = 0 a slice receives the values rf_var_distances_backward gives on it.
 * accumulate = 0: stored to grad_guide_volumes; 1: added to what they hold.  One launch ("var_distances_volume_grad"), a gather: no
 * atomics, two runs agree bit for bit.  There is no entry point for byte guides.
 * Decided before any HIP call: the refusals of rf_var_distances_volume for f32 guides (n_guide, extents below 1, null pointers --
 * the three gradient inputs, grad_guide_volumes and its entries included --, the scale, the volume domain with n_planes = 1); then
 * accumulate other than 0 or 1, volumes not 16-byte aligned, a gradient volume that overlaps grad_dx, grad_dy, grad_dz, a guide
 * volume or another gradient volume (RF_ERR_INVALID_ARG; the message names the volumes). */
int    rf_var_distances_volume_backward(const void *const *guide_volumes, int32_t n_guide, int64_t width, int64_t height, int64_t depth,
                                        float scale, const void *grad_dx, const void *grad_dy, const void *grad_dz,
                                        void *const *grad_guide_volumes, int32_t accumulate, int32_t device, void *stream);
/* The distance planes of the domain-transform filter from a guide image of n_guide dense planes of width x height:
 *     d_x[r][c] = 1 + scale * sum_ch |g_ch[r][c] - g_ch[r][c-1]|   (c >= 1;  d_x[r][0] = 1)
 *     d_y[r][c] = 1 + scale * sum_ch |g_ch[r][c] - g_ch[r-1][c]|   (r >= 1;  d_y[0][c] = 1)
 * channels summed in order in f32; guide planes f32 (guide_u8 = 0) or uint8 (guide_u8 = 1: the differences are exact).  One
 * launch ("var_distances"), one read of the guide; asynchronous on `stream`; device -1 = the current one.  Decided before any
 * HIP call: n_guide outside 1..RF_MAX_PLANES, extents below 1, null pointers, a scale that is negative or not finite
 * (RF_ERR_INVALID_ARG); a width that is not a multiple of 4, extents above the varying plans' limit of 2^21 (RF_ERR_UNSUPPORTED);
 * dx / dy / f32 guide planes not 16-byte aligned, uint8 guide planes not 4-byte aligned, dx or dy overlapping each other or a
 * guide plane (RF_ERR_INVALID_ARG). */
int    rf_var_distances(const void *const *guide_planes, int32_t n_guide, int32_t guide_u8, int64_t width, int64_t height,
                        float scale, void *dx, void *dy, int32_t device, void *stream);
/* The adjoint of rf_var_distances for f32 guide planes: from grad_dx = dL/d(d_x) and grad_dy = dL/d(d_y), per channel, in f32 with
 * the terms in this order,
 *     gg[ch][r][c] = scale * (  sx(r,c) * gdx[r][c] - sx(r,c+1) * gdx[r][c+1] + sy(r,c) * gdy[r][c] - sy(r+1,c) * gdy[r+1][c] )
 *     sx(r,c) = sgn(g[r][c] - g[r][c-1]) for 1 <= c < W, else 0;   sy likewise along rows;   sgn(0) = 0
 * (a constant guide gets a gradient of exactly 0).  accumulate = 0: stored to grad_guide_planes; 1: added to what they hold.  One
 * launch ("var_distances_grad"), a gather: no atomics, two runs agree bit for bit.  There is no entry point for byte guides.
 * Decided before any HIP call: the refusals of rf_var_distances (null pointers include grad_guide_planes and its entries); then
 * accumulate other than 0 or 1, planes not 16-byte aligned, a gradient plane that overlaps grad_dx, grad_dy, a guide plane or
 * another gradient plane (RF_ERR_INVALID_ARG). */
int    rf_var_distances_backward(const void *const *guide_planes, int32_t n_guide, int64_t width, int64_t height, float scale,
                                 const void *grad_dx, const void *grad_dy, void *const *grad_guide_planes, int32_t accumulate,
                                 int32_t device, void *stream);

/* ---- edge-aware smoothing as one plan ------------------------------------------------------------------------------------- */
/* The domain-transform recursive filter (Gastal & Oliveira 2011) of an image of n_planes dense planes, f32 or uint8, that share
 * their edges.  The edges come from the image itself (n_guide = 0) or from n_guide separate guide planes, f32 or uint8.  A byte
 * guide means that guide divided by 255.  The plan owns the two distance planes and sequences every launch:
 *     "var_distances"  once, as rf_var_distances with scale = (float)(sigma_s / sigma_r), over 255 where the guiding planes are bytes;
 *     then for k = 0 .. K-1 the stages +x -x and +y -y of the power form on d_x, d_y with the bases {a_k, a_k}:
 *     "var_tails_x", "var_carry", "var_pass2_x", "var_tails_y", "var_carry", "var_pass2_y"
 *     sigma_k = sigma_s * sqrt(3) * 2^(K-1-k) / sqrt(4^K - 1)  (in double),   a_k = (float)exp(-sqrt(2) / sigma_k).
 * The number of launches is 1 + 6 K.  No conversion launch exists.
 * f32 images: the first stage reads image_planes, everything else runs in place on out_planes; the result is, bit for bit, that
 * of rf_var_distances followed by K calls of rf_var_plan_execute_power.
 * uint8 images (image_u8 = 1, input AND output; the storage contract of RF_IO_U8): the filter is the f32 filter on the widened
 * bytes.  The plan owns n_planes f32 working planes; the first stage reads the caller's bytes and writes them, the stages between
 * run in place on them, and the final pass of the last stage stores out = sat8(f32 result) to out_planes: to nearest, ties to
 * even, clamped to [0, 255], NaN -> 0.  Nothing between two iterations is rounded to bytes.
 * Workspace: two f32 distance planes + (uint8 images) n_planes f32 planes + the tails and carries of the varying scans.
 * Create refuses, before any HIP call: abi != RF_ABI, nonzero flags, n_planes outside 1..RF_MAX_PLANES, n_guide outside
 * 0..RF_MAX_PLANES, image_u8 or guide_u8 other than 0 or 1, guide_u8 = 1 with n_guide = 0, iterations outside
 * 1..RF_SMOOTH_MAX_ITERATIONS, extents below 1, a sigma that is not finite and positive (RF_ERR_INVALID_ARG); a width that is
 * not a multiple of 4, an extent above 2^21, an a_k that rounds to 1 or to 0 in f32 (RF_ERR_UNSUPPORTED; the message names k).
 * Execute refuses: null arrays or pointers, guide_planes that does not match n_guide (NULL iff n_guide == 0), f32 planes that
 * are not 16-byte aligned, uint8 planes that are not 4-byte aligned, an input plane that is neither the output plane of the same
 * index nor disjoint from every output plane (RF_ERR_INVALID_ARG); a host-only plan (RF_ERR_HIP).  in == out is allowed in both
 * image types; guide planes may overlap output planes (the distances are formed first, on the same stream).
 * Executes of one plan are ordered by the caller, as for a plan of varying scans: one stream, or the caller's synchronisation.
 * Every function returns a status and never throws. */
#define RF_SMOOTH_MAX_ITERATIONS 8
typedef struct {
    uint32_t abi;                     /* RF_ABI                                                  */
    int32_t  image_u8;                /* 0: f32 image planes; 1: uint8 image planes, in AND out  */
    int64_t  width, height;
    int32_t  n_planes;                /* 1..RF_MAX_PLANES image planes sharing the edges         */
    int32_t  n_guide;                 /* 0: the image guides itself; else 1..RF_MAX_PLANES       */
    int32_t  guide_u8;                /* type of the separate guide planes; 0 when n_guide == 0  */
    int32_t  iterations;              /* K, 1..RF_SMOOTH_MAX_ITERATIONS                          */
    double   sigma_s, sigma_r;        /* finite, > 0                                             */
    int32_t  device;                  /* HIP device ordinal, -1 = current, RF_DEVICE_HOST_ONLY   */
    uint32_t flags;                   /* 0                                                       */
} rf_smooth_desc;
typedef struct rf_smooth_plan rf_smooth_plan;
int    rf_smooth_plan_create(const rf_smooth_desc *desc, rf_smooth_plan **plan_out);
int    rf_smooth_plan_destroy(rf_smooth_plan *plan);
size_t rf_smooth_plan_workspace_bytes(const rf_smooth_plan *plan);
int    rf_smooth_plan_num_kernels(const rf_smooth_plan *plan);
/* a_0 .. a_{K-1}, the bases the plan runs with */
int    rf_smooth_plan_bases(const rf_smooth_plan *plan, float *out /* iterations */);
/* New sigmas for an existing plan: the scale of var_distances and a_0 .. a_{K-1} are recomputed exactly as create computes them, so
 * rf_smooth_plan_bases afterwards returns, bit for bit, what a fresh plan created with these sigmas returns, and every later
 * execute and backward runs with them.  Nothing is allocated and no HIP call is made: it works on host-only plans, and a caller who
 * tunes the sigmas keeps one plan and its workspace.  Refused as create refuses them, the plan left unchanged: a sigma that is not
 * finite and positive (RF_ERR_INVALID_ARG); sigma_s / sigma_r that is no f32, an a_k that rounds to 0 or 1 in f32
 * (RF_ERR_UNSUPPORTED).  The values are read by the host when a call is issued: order it against the plan's executes and backwards as
 * an execute is ordered (work already issued keeps the sigmas it was issued with). */
int    rf_smooth_plan_set_sigmas(rf_smooth_plan *plan, double sigma_s, double sigma_r);
/* image_planes / out_planes: n_planes device pointers each; guide_planes: n_guide device pointers, NULL iff n_guide == 0.
 * Asynchronous on `stream`. */
int    rf_smooth_plan_execute(rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes,
                              void *const *out_planes, void *stream);
/* per-kernel milliseconds and names (valid for the life of the plan); synchronises the stream */
int    rf_smooth_plan_execute_timed(rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes,
                                    void *const *out_planes, void *stream, float *ms_out, const char **names_out, int capacity);
/* The adjoint of rf_smooth_plan_execute for f32 images (a uint8-image plan: RF_ERR_UNSUPPORTED): grad_image = dL/d(image) from
 * grad_out = dL/d(out) and, with edges = 1, the gradient through the distances as well.
 * edges = 0 (distances held constant): "var_distances", then for k = K-1 .. 0 the adjoint stages of -y +y -x +x in the power form
 * with the bases {a_k, a_k} -- the launches of rf_var_plan_backward_power without exponent gradients, 1 + 12 K in all.  The first
 * stage reads grad_out, the rest run in place on grad_image; grad_out[pl] == grad_image[pl] is allowed; image_planes is needed only
 * where the image guides itself; a uint8 guide is allowed; grad_guide_planes must be NULL; no workspace beyond the plan's.  The
 * result is, bit for bit, that of K calls of rf_var_plan_backward_power in reverse order.
 * edges = 1: "var_distances"; the forward of iterations 0 .. K-2 (the six launches of an execute each), every output kept; for
 * k = K-1 .. 0 the launches of rf_var_plan_backward_power WITH both exponent gradients on iteration k's input (28), whose
 * var_grad launches store into two plan-owned planes the first time each is touched and add afterwards; one "var_distances_grad"
 * with the plan's scale.  34 K - 4 launches.  n_guide > 0: grad_guide_planes (n_guide planes) is required and stored, and
 * grad_image is bit for bit that of edges = 0.  n_guide = 0: grad_guide_planes must be NULL and the last launch ADDS the guide's
 * gradient into grad_image_planes.  A uint8 guide is refused (RF_ERR_UNSUPPORTED).  Workspace, allocated by the first call that
 * needs it and freed with the plan: 2 + (K - 1 + 5) * n_planes f32 planes = rf_smooth_plan_backward_workspace_bytes(plan, 1)
 * (0 for edges = 0; rf_smooth_plan_workspace_bytes does not count it).
 * No atomics: two runs of one call agree bit for bit.  A plan keeps no state across calls; order executes and backward calls of
 * one plan on one stream.  Checked in this order, before any HIP call: null plan / grad_out_planes / grad_image_planes; edges other
 * than 0 or 1 (RF_ERR_INVALID_ARG); a uint8-image plan (RF_ERR_UNSUPPORTED); guide_planes that does not match n_guide; image_planes
 * NULL where it is needed (RF_ERR_INVALID_ARG); edges = 1 with a uint8 guide (RF_ERR_UNSUPPORTED); grad_guide_planes NULL where it
 * is required or given where it must be NULL (RF_ERR_INVALID_ARG); a host-only plan (RF_ERR_HIP); null or misaligned planes; a
 * grad_image or guide-gradient plane that overlaps a guide plane, an image plane, another written plane, or a grad_out plane --
 * except grad_image[pl] being exactly grad_out[pl] (RF_ERR_INVALID_ARG; the message names the planes). */
int    rf_smooth_plan_backward(rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes,
                               const void *const *grad_out_planes, void *const *grad_image_planes, void *const *grad_guide_planes,
                               int32_t edges, void *stream);
int    rf_smooth_plan_backward_timed(rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes,
                                     const void *const *grad_out_planes, void *const *grad_image_planes,
                                     void *const *grad_guide_planes, int32_t edges, void *stream, float *ms_out,
                                     const char **names_out, int capacity);
int    rf_smooth_plan_backward_num_kernels(const rf_smooth_plan *plan, int edges);
/* rf_smooth_plan_backward with the gradients of the scalars that shape the filter.  grad_params is a DEVICE buffer of 3 + K doubles,
 * 8-byte aligned: dL/dsigma_s, dL/dsigma_r, dL/dspacing_z (0 on an image plan), then dL/da_0 .. dL/da_{K-1}, all summed over the
 * batch (the sigmas are shared).  With gd the exponent gradients the edges = 1 route accumulates, A_k = dL/da_k summed over the
 * dimensions (rf_var_plan_backward_power_bases' sum per iteration) and Q = sum over the dimensions and samples of gd (d - d0), d0 = 1
 * along x and y and spacing_z along z:
 *     dL/dsigma_s = (sum_k A_k a_k (-ln a_k) + Q) / sigma_s,   dL/dsigma_r = -Q / sigma_r,   dL/dspacing_z = sum gd_z.
 * A byte guide's 255 cancels; the roundings of a_k and of the scale to f32 are treated as the identity; the sigmas are those of
 * create or of the last rf_smooth_plan_set_sigmas.  The host forms the factors in double and the device multiplies: no call
 * synchronises, there are no atomics, and two runs agree bit for bit.
 * Launches: those of rf_smooth_plan_backward(edges = 1) with the base-reducing var_grad instances -- edges = 0 leaves out the final
 * var_distances[_volume]_grad -- then "var_dot" (one streaming launch over the (gd, d) pairs: f64 slabs of sum gd (d - d0), the term
 * 0 by a select where gd is 0, and of sum gd) and "var_param_sum": rf_smooth_plan_backward_sigmas_num_kernels(plan, edges) =
 * rf_smooth_plan_backward_num_kernels(plan, 1) + 2, one less at edges = 0.  grad_image and grad_guide are bit for bit what
 * rf_smooth_plan_backward gives with the same edges.  The workspace is that of edges = 1 plus plan-owned f64 slabs (8 bytes per
 * workgroup of every reducing launch and of var_dot), allocated by the first call.
 * image_planes is always needed (the forward is rerun); a uint8 guide is allowed with edges = 0.  Image plans, batched plans and
 * volume plans created with RF_SMOOTH_VOLUME_BACKWARD; unflagged volume plans and byte-image plans are refused as in
 * rf_smooth_plan_backward.  Checked in this order: null plan / grad_out_planes / grad_image_planes; null grad_params, then a
 * grad_params that is not 8-byte aligned (RF_ERR_INVALID_ARG); then the checks of rf_smooth_plan_backward in their order, the
 * host-only plan (RF_ERR_HIP) last before the per-plane checks. */
int    rf_smooth_plan_backward_sigmas(rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes,
                                      const void *const *grad_out_planes, void *const *grad_image_planes, void *const *grad_guide_planes,
                                      int32_t edges, double *grad_params /* device, 3 + iterations doubles */, void *stream);
int    rf_smooth_plan_backward_sigmas_timed(rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes,
                                            const void *const *grad_out_planes, void *const *grad_image_planes,
                                            void *const *grad_guide_planes, int32_t edges, double *grad_params, void *stream,
                                            float *ms_out, const char **names_out, int capacity);
int    rf_smooth_plan_backward_sigmas_num_kernels(const rf_smooth_plan *plan, int edges);
size_t rf_smooth_plan_backward_workspace_bytes(const rf_smooth_plan *plan, int edges);

/* A batch: `batch` images of the description per call, forward and backward, every launch taking all of them (the batch is a
 * grid dimension of every kernel, never a loop on the host).  The result is an ordinary rf_smooth_plan: execute, execute_timed,
 * backward, backward_timed, bases, the queries and destroy take it with their signatures above.
 * The pointer arrays of those calls name image 0's planes.  Plane pl of image b is  planes[pl] + b * image_stride  samples in
 * image_planes, out_planes, grad_out_planes and grad_image_planes, and  planes[ch] + b * guide_stride  in guide_planes and
 * grad_guide_planes.  A contiguous NCHW tensor: image_stride = C*H*W, guide_stride = G*H*W.
 * Every image is filtered with its own edges -- its own distance planes, from its own guide or from itself -- in its own tile
 * grid, with its own tails and carries: out[b] and the gradients of image b are, bit for bit, those of a single-image plan of the
 * same description on image b, whatever its position in the batch and whatever the other images hold (NaN included).
 * rf_smooth_plan_num_kernels and rf_smooth_plan_backward_num_kernels return what they return for one image (1 + 6 K, 1 + 12 K,
 * 34 K - 4; the same names in the same order): launches do not grow with the batch.  rf_smooth_plan_workspace_bytes and
 * rf_smooth_plan_backward_workspace_bytes(plan, 1) are exactly `batch` times the single-image plan's: 2 * batch distance planes,
 * batch * n_planes working planes for byte images, tails and carries per image in the single-image layout, and per image the
 * planes of the backward.  An allocation that fails: RF_ERR_NOMEM, the message carries the byte count, *plan_out stays NULL.
 * batch = 1 behaves as rf_smooth_plan_create in every respect, bit for bit.
 * Create refuses, before any HIP call and in this order: a null batch; a null desc or plan_out; batch outside
 * 1..RF_SMOOTH_MAX_BATCH; a stride that is not a multiple of 4 samples (every plane of every image stays 16-byte aligned for f32
 * and 4-byte aligned for bytes); image_stride < width * height; guide_stride != 0 with n_guide == 0; guide_stride < width * height
 * with n_guide > 0 -- a guide shared by the whole batch (stride 0) is not supported: its gradient would be a sum across images
 * (all RF_ERR_INVALID_ARG); then everything rf_smooth_plan_create refuses, with its status.
 * Execute and backward keep their checks and their order.  With batch > 1 the aliasing rules hold per (image, plane) extent
 * [planes[pl] + b * stride, + width * height samples): a written plane (out; grad_image, grad_guide) is disjoint from every other
 * extent of the call, read or written -- except that out[b][pl] may be exactly image[b][pl], and grad_image[b][pl] exactly
 * grad_out[b][pl] (in place).  Guide planes may still overlap the output planes of an execute.  A stride that makes planes of
 * different images overlap is refused by the same rule (RF_ERR_INVALID_ARG; the message names both planes and their images).  The
 * extents are sorted, not paired: E log E steps for the E = batch * (planes of the arrays involved) extents of a call.
 * Not supported: a guide shared across the batch, images of different sizes in one batch, 16-bit planes, widths that are not
 * multiples of 4, byte images in the backward. */
#define RF_SMOOTH_MAX_BATCH 1024
typedef struct {
    int32_t batch;          /* 1..RF_SMOOTH_MAX_BATCH images per call                                                   */
    int64_t image_stride;   /* samples from image b to image b+1 in image_planes, out_planes, grad_out_planes,
                               grad_image_planes: plane pl of image b is  planes[pl] + b * image_stride                 */
    int64_t guide_stride;   /* the same for guide_planes and grad_guide_planes; must be 0 when n_guide == 0             */
} rf_smooth_batch_desc;
int    rf_smooth_plan_create_batched(const rf_smooth_desc *desc, const rf_smooth_batch_desc *batch, rf_smooth_plan **plan_out);

/* A volume: the filter along x, y and z of n_planes dense volumes [z][y][x], f32 or uint8.  The result is an ordinary
 * rf_smooth_plan that owns THREE distance volumes: execute, execute_timed, bases, the queries and destroy take it with their
 * signatures above, a "plane" being a volume.  One "var_distances_volume" launch (rf_var_distances_volume with the plan's scale
 * and spacing_z), then for k = 0 .. K-1 the pair stages +x -x, +y -y, +z -z of the power form on d_x, d_y, d_z with the bases
 * {a_k, a_k, a_k}: 1 + 9 K launches, a_k as above.  f32 volumes: bit for bit rf_var_distances_volume followed by K calls of
 * rf_var_plan_execute_power on the volume plan.  uint8 volumes: the storage contract above -- the first x stage reads the
 * caller's bytes, the iterations run on n_planes plan-owned f32 volumes, the last z pass stores sat8; no conversion launch.
 * spacing_z: the sample distance along z in units of the x/y pitch, finite and > 0 (1 = isotropic).
 * Create refuses what rf_smooth_plan_create refuses, with the domain of rf_var_plan_create_volume in the place of the 2-D extent
 * checks and a spacing_z that is not finite and positive (RF_ERR_INVALID_ARG).  Without RF_SMOOTH_VOLUME_BACKWARD in flags,
 * rf_smooth_plan_backward and _backward_timed on a volume plan return RF_ERR_UNSUPPORTED, and rf_smooth_plan_backward_num_kernels
 * and _backward_workspace_bytes return 0.  There is no batch of volumes.
 * flags = RF_SMOOTH_VOLUME_BACKWARD (f32 volumes; with image_u8 = 1 create returns RF_ERR_UNSUPPORTED; any other bit is
 * RF_ERR_INVALID_ARG): the plan has a backward.  Its forward is the unflagged plan's -- the same launches, the same
 * rf_smooth_plan_workspace_bytes, the same bits -- and nothing more is allocated at create.  rf_smooth_plan_backward and
 * _backward_timed then run the sequence documented above one dimension up, with the same rules, refusals and order of refusals:
 *     edges = 0   "var_distances_volume", then for k = K-1 .. 0 the adjoint stages of -z +z -y +y -x +x in the power form with
 *                 {a_k, a_k, a_k}: 1 + 18 K launches; bit for bit K calls of rf_var_plan_backward_power on the volume plan in
 *                 reverse order.  grad_out[pl] == grad_image[pl] is allowed, a uint8 guide is allowed, no extra workspace.
 *     edges = 1   "var_distances_volume"; the forward of iterations 0 .. K-2 (nine launches each), every output kept; for
 *                 k = K-1 .. 0 the launches of rf_var_plan_backward_power with all three exponent gradients (7 * 6 = 42), the
 *                 first touch of gd_x / gd_y / gd_z storing and the later ones adding; one "var_distances_volume_grad"
 *                 (rf_var_distances_volume_backward) with the plan's scale: 51 K - 7 launches.  n_guide > 0: the gradient is
 *                 stored to grad_guide_planes and grad_image has the bits of edges = 0; n_guide = 0: the last launch adds into
 *                 grad_image_planes.  A uint8 guide is refused at the call (RF_ERR_UNSUPPORTED).
 * Workspace at edges = 1, allocated by the first call that needs it (RF_ERR_NOMEM with the byte count in the message if that
 * fails): 3 + (K - 1 + 7) * n_planes f32 volumes = rf_smooth_plan_backward_workspace_bytes(plan, 1) -- gd_x, gd_y, gd_z, K - 1
 * checkpoints per plane, and the inner plan's (6 + 1) * n_planes; 0 for edges = 0.  A plan keeps no state across calls.
 * Out of scope: byte and 16-bit volumes in the backward, byte-guide gradients, gradients of the sigmas, the bases or spacing_z,
 * batches of volumes, sharding, double backward; the flag is not the default. */
#define RF_SMOOTH_VOLUME_BACKWARD 1u   /* rf_smooth_volume_desc.flags: the plan has a backward (f32 volumes) */
typedef struct {
    uint32_t abi;                     /* RF_ABI                                                  */
    int32_t  image_u8;                /* 0: f32 volumes; 1: uint8 volumes, in AND out            */
    int64_t  width, height, depth;
    int32_t  n_planes;                /* 1..RF_MAX_PLANES volumes sharing the edges              */
    int32_t  n_guide;                 /* 0: the volume guides itself; else 1..RF_MAX_PLANES      */
    int32_t  guide_u8;                /* type of the separate guide volumes; 0 when n_guide == 0 */
    int32_t  iterations;              /* K, 1..RF_SMOOTH_MAX_ITERATIONS                          */
    double   sigma_s, sigma_r;        /* finite, > 0                                             */
    double   spacing_z;               /* finite, > 0; 1 = isotropic                              */
    int32_t  device;                  /* HIP device ordinal, -1 = current, RF_DEVICE_HOST_ONLY   */
    uint32_t flags;                   /* 0, or RF_SMOOTH_VOLUME_BACKWARD                         */
} rf_smooth_volume_desc;
int    rf_smooth_plan_create_volume(const rf_smooth_volume_desc *desc, rf_smooth_plan **plan_out);

/* ---- time-varying second-order all-pole scans on signals ("var2") ---------------------------
 * One scan per plan on n_lines dense f32 signals of `length` samples, line l beginning l * stride samples behind the pointer of
 * a call.  Every line has coefficient signals a1 and a2 of its own, laid out like the input:
 *     causal      y[n] = x[n] - a1~[n] y[n-1] - a2~[n] y[n-2]        y[-1] = y[-2] = 0
 *     anticausal  y[n] = x[n] - a1~[n] y[n+1] - a2~[n] y[n+2]        y[N] = y[N+1] = 0
 * The anticausal scan is the causal one on the three signals reversed.  a~ is a with every coefficient that would multiply a
 * sample outside the line replaced by 0 through a select: a1[0], a2[0], a2[1] of a causal scan, a1[N-1], a2[N-1], a2[N-2] of an
 * anticausal one -- a NaN stored there reaches no output.  Nothing restricts the coefficients: an unstable filter is the
 * caller's business, NaN propagates.  A resonator whose centre frequency and bandwidth move, an LPC synthesis filter, a swept
 * biquad's feedback half; zero-phase filtering is two plans, causal then anticausal, composed by the caller.
 * in == out is allowed; no other overlap of out with in, and none with a coefficient signal; all pointers 16-byte aligned.
 * Tiling (kernels_var2_signal.hip): the state is the 2-vector (y[n], y[n-1]); a lane owns 64 consecutive samples, a wave a group
 * of 64 such tiles (4096 samples).  Three launches: "var2_tails_1d" (per tile the state it leaves from zero entry and the 2 x 2
 * matrix that carries an entering state across it, then a scan of these across the wave: every lane stores the map from the
 * state that enters its group to the state that enters its tile, one lane the group's aggregate), "var2_carry_1d" (the
 * recurrence over groups, one workgroup per line sweeping 1024 groups at a time) and "var2_pass2_1d" (reruns the recurrence
 * from the entering state and stores: coefficients of exactly 0 give out == in bit for bit).  No kernel waits on another
 * workgroup, there are no atomics, and a result is reproducible bit for bit.  rf_var2_plan_num_kernels = 3.
 * rf_var2_plan_workspace_bytes is exact: 4 * n_lines * (6 * (tiles + groups) + 2 * groups) bytes, tiles = ceil(length / 64),
 * groups = ceil(tiles / 64).
 * The adjoint: rf_var2_plan_backward takes the coefficients, `out` = the forward's result and grad_out = dL/d(out), and stores
 * grad_in = dL/d(in) = lam, for a causal plan
 *     lam[n] = grad_out[n] - a1~[n+1] lam[n+1] - a2~[n+2] lam[n+2]
 * (the mirror image for an anticausal one), in three launches "var2_adj_tails_1d", "var2_carry_1d", "var2_adj_pass2_1d" on the
 * plan's workspace.  grad_a1 and grad_a2 both given: a fourth launch "var2_grad_1d" stores
 *     grad_a1[n] = -lam[n] y[n-1]    grad_a2[n] = -lam[n] y[n-2]          (anticausal: y[n+1], y[n+2])
 * with 0 at the masked entries.  Both null: no coefficient gradients, and `out` may be null.  One null and one not is refused.
 * grad_in == grad_out is allowed; a gradient that is written overlaps nothing else.  rf_var2_plan_backward_num_kernels = 3
 * without and 4 with coefficient gradients.  A plan keeps no state across calls; order the calls of one plan (one workspace).
 * Create refuses, in this order and before any HIP call: null arguments, abi != RF_ABI, nonzero flags, length < 1, n_lines
 * outside 1..65535, a stride below the length, not a multiple of 4 or above 2^40 (RF_ERR_INVALID_ARG); a length that is not a
 * multiple of 4, then one above 2^30 (RF_ERR_UNSUPPORTED).  A call refuses, in this order and before any HIP call: a null plan;
 * backward: exactly one of grad_a1, grad_a2 null; a null pointer; a pointer that is not 16-byte aligned; an overlap named above
 * (RF_ERR_INVALID_ARG); then a host-only plan (RF_ERR_HIP).  A *_timed call checks ms_out's capacity first.  A host-only plan
 * (device = RF_DEVICE_HOST_ONLY) answers the queries and checks the arguments of a call, which it never dereferences.
 * Out of scope: orders above 2; images and volumes; lists of scans inside one plan; 16-bit signals; second derivatives;
 * sharding; lengths that are not multiples of 4 (pad the signals with zeros behind the end of a causal scan, before the start
 * of an anticausal one: the real samples are what an unpadded scan gives).
 *
 * The whole section, direct form I (rf_var2_plan_execute_biquad), on the same plan: five coefficient signals laid out like in,
 *     causal      v[n] = b0[n] in[n] + b1~[n] in[n-1] + b2~[n] in[n-2]      y[n] = v[n] - a1~[n] y[n-1] - a2~[n] y[n-2]
 * (anticausal: the same on all six signals reversed).  The masked slots are b1[0], b2[0], b2[1], a1[0], a2[0], a2[1] of a causal
 * plan and their mirror images of an anticausal one; b0 has none.  The order of operations is fixed,
 * v = fma(b2~, in[n-2], fma(b1~, in[n-1], b0 * in[n])): b = (1, 0, 0) gives rf_var2_plan_execute's bits for finite input.
 * Three launches: "var2_biquad_tails_1d" forms v over a lane's tile in registers, STORES v to out and runs the tails stage on
 * it; "var2_carry_1d" and "var2_pass2_1d" then run on out in place.  rf_var2_plan_biquad_num_kernels = 3.  out overlaps none of
 * the six inputs: in == out is refused, because the first launch stores v while neighbouring groups still read in.
 * rf_var2_plan_backward_biquad takes the six inputs, out = the forward's result and grad_out, and stores, for a causal plan,
 *     grad_in[n] = b0[n] lam[n] + b1~[n+1] lam[n+1] + b2~[n+2] lam[n+2]       lam: the adjoint state above, from grad_out
 *     grad_b0[n] = lam[n] in[n]   grad_b1[n] = lam[n] in[n-1]   grad_b2[n] = lam[n] in[n-2]
 *     grad_a1[n] = -lam[n] y[n-1]   grad_a2[n] = -lam[n] y[n-2]
 * (the mirror image for an anticausal one; +0 at the masked slots) in four launches, "var2_adj_tails_1d", "var2_carry_1d",
 * "var2_adj_pass2_1d" and "var2_biquad_grad_1d", with or without coefficient gradients:
 * rf_var2_plan_backward_biquad_num_kernels = 4.  lam lives in one f32 signal of the plan's span that the plan allocates in its
 * first such call; rf_var2_plan_backward_biquad_bytes reports its size, 4 * ((n_lines - 1) * stride + length), and
 * rf_var2_plan_workspace_bytes is unchanged.  The five coefficient gradients are all given or all null; all null: out may be null.
 * grad_in == grad_out is allowed; a gradient that is written overlaps nothing else.  A call refuses, in this order and before
 * any HIP call: a null plan; backward: some but not all of the five coefficient gradients null; a null pointer; a pointer that
 * is not 16-byte aligned; execute: out overlapping a coefficient signal, then out overlapping in (in == out included); backward:
 * a written gradient overlapping a coefficient signal, in, out, another written gradient, or grad_out other than grad_in exactly
 * (RF_ERR_INVALID_ARG); then a host-only plan (RF_ERR_HIP).  A *_timed call checks ms_out's capacity first.
 * Out of scope for the section: orders above 2; the direct-form-II ordering; images and volumes; 16-bit signals; second
 * derivatives; sharding.
 *
 * A cascade of sections (rf_var2_plan_execute_cascade): n_sections direct-form-I sections, 1 .. RF_VAR2_MAX_SECTIONS, run one
 * behind the other in the plan's direction, section k + 1 on the result of section k; every section has five coefficient
 * signals of its own (rf_var2_section), masked and evaluated as above.  Launches: "var2_biquad_tails_1d", then, per boundary
 * between two sections, "var2_carry_1d" and "var2_link_1d" -- the final stage of section k, the feed-forward part of section
 * k + 1 on the tile in registers and the tails stage of section k + 1, v stored in place on out -- then "var2_carry_1d" and
 * "var2_pass2_1d": rf_var2_plan_cascade_num_kernels(plan, K) = 2 K + 1, and K = 1 is rf_var2_plan_execute_biquad's launches and
 * bits.  The two samples a link's feed-forward taps reach beyond a tile are the state that enters the tile in section k's final
 * stage (what its recurrence takes for y[t0-1], y[t0-2]), not a reload: equal to the stored samples up to the rounding of the
 * carry algebra, exactly where the feedback coefficients are 0.  in == out is refused as for one section; out overlaps no
 * coefficient signal of any section.
 * rf_var2_plan_backward_cascade keeps nothing from the forward: for K >= 2 it reruns sections 0 .. K-2 into K - 1 signals of the
 * plan's ("var2_biquad_tails_1d", K - 2 times "var2_carry_1d" and "var2_link_keep_1d", "var2_carry_1d", "var2_pass2_1d"), then
 * runs, from the last section to the first, the four launches of rf_var2_plan_backward_biquad, the gradient between two sections
 * in one more signal of the plan's: rf_var2_plan_backward_cascade_num_kernels(plan, K) = 4 at K = 1 and 6 K - 1 above.  The plan
 * owns 1 span (K = 1) or K + 1 spans (lam, the gradient between sections, K - 1 results) of 4 * ((n_lines - 1) * stride +
 * length) bytes, allocated by the first call and regrown when a later call asks for more sections:
 * rf_var2_plan_backward_cascade_bytes(plan, K); rf_var2_plan_workspace_bytes is unchanged.  grads is null (no coefficient
 * gradients; out may then be null) or an array of n_sections rf_var2_section_grad with every pointer given.  grad_in == grad_out
 * is allowed; a written gradient overlaps nothing else.  A call refuses, in this order and before any HIP call: a null plan;
 * n_sections outside 1 .. 16; null sections; backward: a section of grads with a null pointer ("section k: ..."); a null or
 * misaligned in, out, grad_out, grad_in ("signal 0: ..."); a null or misaligned coefficient pointer ("section k: ..."); backward: a
 * misaligned gradient pointer ("section k: ..."); execute: out overlapping a coefficient signal ("coefficient of section k plane
 * j", j = 0..4 for b0, b1, b2, a1, a2), then in; backward: a written gradient overlapping a coefficient signal, in, out, another
 * written gradient, or grad_out other than grad_in exactly (RF_ERR_INVALID_ARG); then a host-only plan (RF_ERR_HIP).  A *_timed
 * call checks ms_out's capacity after the plan and n_sections.
 *
 * The cascade for training (rf_var2_plan_execute_cascade_keep, rf_var2_plan_backward_cascade_kept): the forward keeps every
 * section's result, in signals the CALLER owns -- the plan still keeps no state between calls -- and the backward reruns nothing.
 * kept is an array of n_sections - 1 pointers to signals laid out like in (it may be null at K = 1); kept[k] receives section
 * k's result, out the last section's.  The launches are rf_var2_plan_execute_cascade's with "var2_link_keep_1d" for
 * "var2_link_1d" -- rf_var2_plan_cascade_num_kernels serves -- and out is that call's bit for bit; K = 1 is
 * rf_var2_plan_execute_biquad's launches and bits.  A kept signal overlaps nothing else in the call; in == out is refused.
 * rf_var2_plan_backward_cascade_kept takes them back.  Launches, from the last section down: "var2_adj_tails_1d" on grad_out;
 * per boundary between sections k and k - 1, "var2_carry_1d" and "var2_adj_link_1d" -- the final stage of section k's adjoint
 * scan, the gradient that enters section k - 1,
 *     g[n] = fma(b2~[n+2], lam[n+2], fma(b1~[n+1], lam[n+1], b0[n] lam[n]))          (causal; lam = section k's adjoint state)
 * formed on the tile in registers and stored to a signal of the plan's, and the adjoint tails stage of section k - 1 on it --
 * then "var2_carry_1d", "var2_adj_pass2_1d" and "var2_biquad_grad_1d" for section 0.  The two samples of lam the transposed taps
 * reach beyond a tile are the state that enters the tile in the adjoint scan's final stage, not a reload: with feedback the
 * gradients differ from rf_var2_plan_backward_cascade's in the last bits of a few samples, with all feedback coefficients 0 they
 * are its bits.  With coefficient gradients the link is "var2_adj_link_keep_1d" (lam stored too) and "var2_biquad_coef_1d"
 * follows it: the section's five gradients from lam, kept[k-1] and kept[k] (out for the last section).
 * rf_var2_plan_backward_cascade_kept_num_kernels(plan, K, with) = 2 K + 2 without coefficient gradients and 3 K + 1 with them;
 * both are 4 at K = 1, where launches and bits are rf_var2_plan_backward_biquad's.  The plan owns lam (K = 1) or lam and the
 * gradient between sections (K >= 2), whatever K: rf_var2_plan_backward_cascade_kept_bytes(plan, K) = 1 or 2 spans, shared with
 * rf_var2_plan_backward_cascade's allocation -- calls of both kinds mix on one plan in any order.  grads null: in, out and kept
 * may be null (nothing of the forward is read).  grads given: every pointer of every section, in, out and, for K >= 2, all of
 * kept are required.  grad_in == grad_out is allowed.  Refusals are those of the cascade calls above, in their order, with the
 * kept pointers checked behind in, out, grad_out, grad_in ("kept k: ...", null or misaligned) and before the coefficient
 * pointers; execute_cascade_keep: out, then a kept signal, overlapping a coefficient signal, in, or another written signal
 * ("kept plane k"); backward_cascade_kept: a written gradient overlapping a kept signal, beside the overlaps above.
 * Out of scope: mixed directions inside one cascade (zero-phase filtering stays two plans); concurrent calls on one plan. */
typedef struct rf_var2_plan rf_var2_plan;
typedef struct {
    uint32_t abi;                     /* RF_ABI                                                  */
    int64_t  length;                  /* samples per line: a multiple of 4, 4 .. 2^30            */
    int32_t  n_lines;                 /* 1..65535                                                */
    int64_t  stride;                  /* samples from line to line: a multiple of 4, >= length   */
    int32_t  causal;                  /* nonzero: causal; 0: anticausal                          */
    int32_t  device;                  /* HIP device ordinal, -1 = current, RF_DEVICE_HOST_ONLY   */
    uint32_t flags;                   /* 0                                                       */
} rf_var2_signal_desc;
int    rf_var2_plan_create_signal(const rf_var2_signal_desc *desc, rf_var2_plan **plan_out);
int    rf_var2_plan_destroy(rf_var2_plan *plan);
size_t rf_var2_plan_workspace_bytes(const rf_var2_plan *plan);
int    rf_var2_plan_num_kernels(const rf_var2_plan *plan);
int    rf_var2_plan_execute(rf_var2_plan *plan, const void *in, const void *a1, const void *a2, void *out, void *stream);
int    rf_var2_plan_execute_timed(rf_var2_plan *plan, const void *in, const void *a1, const void *a2, void *out, void *stream,
                                  float *ms_out, const char **names_out, int capacity);
int    rf_var2_plan_backward(rf_var2_plan *plan, const void *a1, const void *a2, const void *out, const void *grad_out, void *grad_in,
                             void *grad_a1, void *grad_a2, void *stream);
int    rf_var2_plan_backward_timed(rf_var2_plan *plan, const void *a1, const void *a2, const void *out, const void *grad_out,
                                   void *grad_in, void *grad_a1, void *grad_a2, void *stream, float *ms_out, const char **names_out,
                                   int capacity);
int    rf_var2_plan_backward_num_kernels(const rf_var2_plan *plan, int with_coefficient_gradients);
int    rf_var2_plan_execute_biquad(rf_var2_plan *plan, const void *in, const void *b0, const void *b1, const void *b2, const void *a1,
                                   const void *a2, void *out, void *stream);
int    rf_var2_plan_execute_biquad_timed(rf_var2_plan *plan, const void *in, const void *b0, const void *b1, const void *b2,
                                         const void *a1, const void *a2, void *out, void *stream, float *ms_out, const char **names_out,
                                         int capacity);
int    rf_var2_plan_backward_biquad(rf_var2_plan *plan, const void *in, const void *b0, const void *b1, const void *b2, const void *a1,
                                    const void *a2, const void *out, const void *grad_out, void *grad_in, void *grad_b0, void *grad_b1,
                                    void *grad_b2, void *grad_a1, void *grad_a2, void *stream);
int    rf_var2_plan_backward_biquad_timed(rf_var2_plan *plan, const void *in, const void *b0, const void *b1, const void *b2,
                                          const void *a1, const void *a2, const void *out, const void *grad_out, void *grad_in,
                                          void *grad_b0, void *grad_b1, void *grad_b2, void *grad_a1, void *grad_a2, void *stream,
                                          float *ms_out, const char **names_out, int capacity);
int    rf_var2_plan_biquad_num_kernels(const rf_var2_plan *plan);
int    rf_var2_plan_backward_biquad_num_kernels(const rf_var2_plan *plan);
size_t rf_var2_plan_backward_biquad_bytes(const rf_var2_plan *plan);
#define RF_VAR2_MAX_SECTIONS 16
typedef struct { const void *b0, *b1, *b2, *a1, *a2; } rf_var2_section;
typedef struct { void *b0, *b1, *b2, *a1, *a2; } rf_var2_section_grad;
int    rf_var2_plan_execute_cascade(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections, void *out,
                                    void *stream);
int    rf_var2_plan_execute_cascade_timed(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections,
                                          void *out, void *stream, float *ms_out, const char **names_out, int capacity);
int    rf_var2_plan_backward_cascade(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections,
                                     const void *out, const void *grad_out, void *grad_in, const rf_var2_section_grad *grads,
                                     void *stream);
int    rf_var2_plan_backward_cascade_timed(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections,
                                           const void *out, const void *grad_out, void *grad_in, const rf_var2_section_grad *grads,
                                           void *stream, float *ms_out, const char **names_out, int capacity);
int    rf_var2_plan_cascade_num_kernels(const rf_var2_plan *plan, int n_sections);             /* 0: n_sections out of range */
int    rf_var2_plan_backward_cascade_num_kernels(const rf_var2_plan *plan, int n_sections);
size_t rf_var2_plan_backward_cascade_bytes(const rf_var2_plan *plan, int n_sections);
/* kept: n_sections - 1 signals laid out like in (null at n_sections == 1) */
int    rf_var2_plan_execute_cascade_keep(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections,
                                         void *out, void *const *kept, void *stream);
int    rf_var2_plan_execute_cascade_keep_timed(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections,
                                               void *out, void *const *kept, void *stream, float *ms_out, const char **names_out,
                                               int capacity);
int    rf_var2_plan_backward_cascade_kept(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections,
                                          const void *const *kept, const void *out, const void *grad_out, void *grad_in,
                                          const rf_var2_section_grad *grads, void *stream);
int    rf_var2_plan_backward_cascade_kept_timed(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections,
                                                const void *const *kept, const void *out, const void *grad_out, void *grad_in,
                                                const rf_var2_section_grad *grads, void *stream, float *ms_out,
                                                const char **names_out, int capacity);
int    rf_var2_plan_backward_cascade_kept_num_kernels(const rf_var2_plan *plan, int n_sections, int with_coefficient_gradients);
size_t rf_var2_plan_backward_cascade_kept_bytes(const rf_var2_plan *plan, int n_sections);

/* The section with its coefficients at a control rate (rf_var2_plan_execute_biquad_frames): each of b0, b1, b2, a1, a2 is
 * n_frames = ceil(length / hop) + 1 f32 FRAMES per line, frame j at sample j * hop, line l frame_stride >= n_frames values
 * behind the pointer (4-byte aligned).  hop is a power of two, 64 .. 65536.  At n = j * hop + k, 0 <= k < hop, by absolute
 * position whatever the plan's direction,
 *     c[n] = fma(k / hop, c[j+1] - c[j], c[j])          (f32; the difference rounded once; c[j * hop] == c[j] exactly)
 * and on these c[n] the section is rf_var2_plan_execute_biquad's: the same masks by position, the same arithmetic, the same
 * bits as that call on the expanded signals (rf_var2_expand_frames writes them, one coefficient per call).  Frames have no
 * masked slots: all of them must be finite.  The kernels read the frames and interpolate in registers: the forward moves 16
 * bytes per sample for 44.  Launches: "var2_biquad_frames_tails_1d", "var2_carry_1d", "var2_frames_pass2_1d"
 * (rf_var2_plan_biquad_frames_num_kernels = 3); out overlaps neither in nor a frame array.
 * rf_var2_plan_backward_biquad_frames: "var2_adj_frames_tails_1d", "var2_carry_1d", "var2_adj_frames_pass2_1d" on grad_out into
 * the plan's lam, then "var2_biquad_frames_grad_1d": grad_in, rf_var2_plan_backward_biquad's bits on the expanded signals.
 * With frame gradients (frame_grads: five arrays laid out like the frames, all given; or all null, or frame_grads null, and
 * out may then be null) that launch also forms the five per-sample gradients of rf_var2_plan_backward_biquad, rounded to f32,
 * and contracts them with the interpolation's transpose in f64 -- per piece of min(hop, 1024) samples S0 = sum (1 - k / hop) g
 * and S1 = sum (k / hop) g, every product exact, a lane in the order of its samples, the lanes of a piece by a fixed tree --
 * into a slab of doubles the plan owns; "var2_frames_fold_1d" adds the pieces of interval j (S0) and of interval j - 1 (S1) in
 * order and rounds once: dL/dc_j.  No atomics; two calls give the same bits.
 * rf_var2_plan_backward_biquad_frames_num_kernels(plan, with) = 4 or 5.  rf_var2_plan_backward_biquad_frames_bytes(plan, hop):
 * lam, 4 * ((n_lines - 1) * stride + length), shared with the other backward calls, plus the slab, 80 * n_lines * ceil(length /
 * min(hop, 1024)); 0 for a refused hop.  Both are allocated by the first call that needs them (the slab regrown by a call with a
 * smaller hop); rf_var2_plan_workspace_bytes is unchanged and the plan keeps no state between calls.
 * Refusals, before any HIP call, in this order: a hop that is no power of two in 64 .. 65536 (RF_ERR_UNSUPPORTED); n_frames !=
 * rf_var2_frames_count(length, hop); frame_stride < n_frames; a null or misaligned pointer (frames, in, out, grad_out, grad_in);
 * in == out or out overlapping a frame array; frame gradients neither all given nor all null; a written gradient overlapping
 * anything else (grad_in == grad_out is allowed); last, a host-only plan (RF_ERR_HIP).
 * rf_var2_expand_frames: out[l * stride + n] = c[n] for one coefficient on `lines` lines of `length` samples (a multiple of 4;
 * out 16-byte aligned, apart from the frames), on the current device: "var2_expand_frames_1d".
 * Out of scope: hops below 64 or not powers of two (480, for example); hold or cubic interpolation; frames for
 * rf_var_plan; 16-bit signals, second derivatives, sharding.  (Cascades on frames: rf_var2_plan_execute_cascade_frames, below.) */
int    rf_var2_frames_count(int length, int hop);                        /* ceil(length / hop) + 1; 0: hop refused */
int    rf_var2_expand_frames(const void *frames, int hop, int n_frames, int64_t frame_stride, int length, int lines, int64_t stride,
                             void *out, void *stream);
int    rf_var2_plan_execute_biquad_frames(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int hop, int n_frames,
                                          int64_t frame_stride, void *out, void *stream);
int    rf_var2_plan_execute_biquad_frames_timed(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int hop,
                                                int n_frames, int64_t frame_stride, void *out, void *stream, float *ms_out,
                                                const char **names_out, int capacity);
int    rf_var2_plan_backward_biquad_frames(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int hop, int n_frames,
                                           int64_t frame_stride, const void *out, const void *grad_out, void *grad_in,
                                           const rf_var2_section_grad *frame_grads, void *stream);
int    rf_var2_plan_backward_biquad_frames_timed(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int hop,
                                                 int n_frames, int64_t frame_stride, const void *out, const void *grad_out,
                                                 void *grad_in, const rf_var2_section_grad *frame_grads, void *stream, float *ms_out,
                                                 const char **names_out, int capacity);
int    rf_var2_plan_biquad_frames_num_kernels(const rf_var2_plan *plan);
int    rf_var2_plan_backward_biquad_frames_num_kernels(const rf_var2_plan *plan, int with_frame_gradients);
size_t rf_var2_plan_backward_biquad_frames_bytes(const rf_var2_plan *plan, int hop);

/* A cascade of sections on control-rate frames (rf_var2_plan_execute_cascade_frames): n_sections sections, 1 ..
 * RF_VAR2_MAX_SECTIONS, all in the plan's direction, section k with its five coefficients as frames -- frames[k], an
 * rf_var2_section of frame pointers -- as rf_var2_plan_execute_biquad_frames defines them; one hop, one n_frames =
 * rf_var2_frames_count(length, hop) and one frame_stride serve all sections.  The result is rf_var2_plan_execute_cascade's on the
 * expanded signals bit for bit: c[n] by absolute position, the same masks, the same fma order of the feed-forward part, and the
 * two samples beyond a tile are the state that enters the tile.  No coefficient signal exists: 8 K + 8 bytes per sample move
 * where K calls of rf_var2_plan_execute_biquad_frames move 16 K and rf_var2_plan_execute_cascade 36 K + 8.
 * Launches: "var2_biquad_frames_tails_1d"; per boundary between two sections "var2_carry_1d" and "var2_frames_link_1d" -- the
 * final stage of section k, the feed-forward part and the tails stage of section k + 1 on the tile in registers, every
 * coefficient interpolated in the step that uses it -- then "var2_carry_1d" and "var2_frames_pass2_1d":
 * rf_var2_plan_cascade_frames_num_kernels(plan, K) = 2 K + 1.  kept null: v and the result in out, in place.  kept given (K - 1
 * signals laid out like in, the CALLER's): kept[k] receives section k's result ("var2_frames_link_keep_1d" for the link); out
 * has the same bits either way.  K = 1 is rf_var2_plan_execute_biquad_frames: its launches, names and bits; kept is not read.
 * rf_var2_plan_backward_cascade_frames runs on the kept signals and reruns nothing: "var2_adj_frames_tails_1d" on grad_out; per
 * boundary from the last one down "var2_carry_1d" and "var2_adj_frames_link_1d" -- rf_var2_plan_backward_cascade_kept's
 * "var2_adj_link_1d" on frames, grad_in that call's bits on the expanded signals -- then "var2_carry_1d",
 * "var2_adj_frames_pass2_1d" and "var2_biquad_frames_grad_1d" for section 0.  With frame gradients (frame_grads: n_sections
 * rf_var2_section_grad laid out like the frames, every pointer given) the link is "var2_adj_frames_link_keep_1d", lam to the
 * plan's signal, and "var2_frames_coef_1d" follows it: the per-sample gradients of section k from lam, kept[k-1] and kept[k]
 * (out for the last section), rounded to f32 and contracted in f64 as "var2_biquad_frames_grad_1d" contracts them -- the same
 * lane order, the same tree -- into section k's part of the slab; "var2_frames_fold_cascade_1d" is last and folds every
 * section in one launch, the additions per frame in rf_var2_plan_backward_biquad_frames' order.
 * rf_var2_plan_backward_cascade_frames_num_kernels(plan, K, with) = 2 K + 2 without frame gradients and 3 K + 2 with them; 4
 * and 5 at K = 1, where launches and bits are rf_var2_plan_backward_biquad_frames'.  The plan owns lam, the gradient between
 * sections (K >= 2) and a slab of K * 80 * n_lines * ceil(length / min(hop, 1024)) bytes, shared with the other backward calls
 * -- calls of every kind mix on one plan in any order, a call with a larger need regrows the slab:
 * rf_var2_plan_backward_cascade_frames_bytes(plan, K, hop), 0 for a refused K or hop.  rf_var2_plan_workspace_bytes is
 * unchanged and the plan keeps no state between calls.  Without frame gradients (frame_grads null, or every pointer null) in,
 * out and kept may be null; with them all are required.  grad_in == grad_out is allowed.
 * Refusals, before any HIP call, in this order: n_sections out of range (a *_timed call checks ms_out's capacity next); a hop
 * that is no power of two in 64 .. 65536 (RF_ERR_UNSUPPORTED); n_frames != rf_var2_frames_count(length, hop); frame_stride <
 * n_frames; a null or misaligned pointer (frames, then in, out, grad_out, grad_in, "kept k", "frames k", "frame gradients k");
 * execute: in == out, out overlapping a frame array, then a kept signal overlapping in, a frame array, out or another kept
 * signal; backward: the frame gradients of a section neither all given nor all null, or the sections not alike; a written
 * array (grad_in, a frame gradient) overlapping a frame array, in, out, a kept signal, another written array, or grad_out other
 * than grad_in exactly; last, a host-only plan (RF_ERR_HIP).
 * Out of scope: a backward that reruns instead of keeping; a hop or a direction per section; the contraction folded into the
 * adjoint link; and what is out of scope for one section on frames. */
int    rf_var2_plan_execute_cascade_frames(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int n_sections, int hop,
                                           int n_frames, int64_t frame_stride, void *out, void *const *kept, void *stream);
int    rf_var2_plan_execute_cascade_frames_timed(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int n_sections,
                                                 int hop, int n_frames, int64_t frame_stride, void *out, void *const *kept, void *stream,
                                                 float *ms_out, const char **names_out, int capacity);
int    rf_var2_plan_backward_cascade_frames(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int n_sections, int hop,
                                            int n_frames, int64_t frame_stride, const void *const *kept, const void *out,
                                            const void *grad_out, void *grad_in, const rf_var2_section_grad *frame_grads, void *stream);
int    rf_var2_plan_backward_cascade_frames_timed(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int n_sections,
                                                  int hop, int n_frames, int64_t frame_stride, const void *const *kept, const void *out,
                                                  const void *grad_out, void *grad_in, const rf_var2_section_grad *frame_grads,
                                                  void *stream, float *ms_out, const char **names_out, int capacity);
int    rf_var2_plan_cascade_frames_num_kernels(const rf_var2_plan *plan, int n_sections);      /* 0: n_sections out of range */
int    rf_var2_plan_backward_cascade_frames_num_kernels(const rf_var2_plan *plan, int n_sections, int with_frame_gradients);
size_t rf_var2_plan_backward_cascade_frames_bytes(const rf_var2_plan *plan, int n_sections, int hop);

/* The cascade on frames with a state that enters and leaves the call (rf_var2_plan_execute_cascade_frames_stream): a signal
 * filtered in chunks -- as audio arrives, or because it does not fit -- gives what one call on the whole signal gives up to
 * rounding, where every rf_var2_plan_execute_* call above starts from silence.  The arguments are
 * rf_var2_plan_execute_cascade_frames' and three more.  A line's state is n_sections + 1 PAIRS of f32, [line][K + 1][2],
 * state_stride >= 2 (K + 1) floats from line to line (4-byte aligned): pair 0 the history of the input, pair k + 1 the history
 * of section k's result, each pair (the sample one place before the line, the sample two places before it) in the direction of
 * the plan's recurrence -- (x[-1], x[-2]) for a causal plan; (x[n], x[n+1]) for an anticausal one, whose chunks are fed last
 * to first.  state_in null: zeros enter.  state_out null: not wanted.  Both null: the call IS
 * rf_var2_plan_execute_cascade_frames -- its launches, names, bits and refusals.  A chunk's frames are those of its own
 * samples: frame j of the call at sample j * hop of the chunk, so a chunk that starts at a multiple of hop of the whole signal
 * takes a slice of the whole signal's frames, frames + start / hop, n_frames = rf_var2_frames_count(length, hop).
 * Each section keeps its masks by position, and the entering state is folded into the two first samples of its v (src the
 * section's input, (hx1, hx2) pair k, (hy1, hy2) pair k + 1, every coefficient the interpolated, unmasked one; an anticausal
 * plan: the mirror image at samples n - 1 and n - 2), each line one rounding:
 *     v[0] = fma(b2[0], hx2, fma(b1[0], hx1, b0[0] * src[0]))          v[1] = fma(b2[1], hx1, fma(b1[1], src[0], b0[1] * src[1]))
 *     v[0] = fma(-a1[0], hy1, fma(-a2[0], hy2, v[0]))                  v[1] = fma(-a2[1], hy1, v[1])
 * The masked recurrence from zero on this v is, bit for bit, the unmasked one from the true state: the tile maps,
 * "var2_carry_1d" and the final stages run unchanged.  The six coefficient slots per section that no other call reads --
 * b1[0], b2[0], b2[1], a1[0], a2[0], a2[1] at the line's first samples in the recurrence's order -- are LIVE here whenever
 * state_in is given: they must be finite.  With state_in of zeros the result equals the call without a state (a zero's sign
 * apart).  The leaving state is stored by the lane that holds it in registers -- pair 0 by the first launch from x, pair k + 1
 * by the link that finishes section k, pair K by the last launch -- and is bit for bit the two last samples, in the
 * recurrence's order, of in, of every kept signal and of out: no further launch, no atomics, two calls give the same bits.
 * Launches, 2 K + 1 whatever K (rf_var2_plan_cascade_frames_stream_num_kernels): "var2_biquad_frames_tails_stream_1d"; per
 * boundary "var2_carry_1d" and "var2_frames_link_stream_1d" ("var2_frames_link_keep_stream_1d" where kept is given); then
 * "var2_carry_1d" and "var2_frames_pass2_stream_1d".  K = 1 runs the same instances (3 launches); kept is not read.  out and
 * kept have the same bits with and without keeping.  The plan keeps no state between calls: the state is the caller's,
 * rf_var2_plan_cascade_frames_stream_state_bytes(plan, K, state_stride) = 4 ((n_lines - 1) state_stride + 2 (K + 1)) bytes per
 * buffer, 0 for a refused K or stride.
 * Refusals: rf_var2_plan_execute_cascade_frames' in its order up to the overlaps of out and the kept signals; then
 * state_stride < 2 (K + 1); a state pointer that is not 4-byte aligned; state_out overlapping state_in, in, out, a kept signal
 * or a frame array; state_in overlapping out or a kept signal (they are stored while it is read); last, a host-only plan.
 * rf_var2_plan_backward_cascade_frames_stream is the adjoint of such a call on what it kept: the arguments of
 * rf_var2_plan_backward_cascade_frames, then state_in (what entered the forward; read for the frame gradients alone),
 * grad_state_out (the gradient of the state that left; null: zeros) and grad_state_in (the gradient of the state that entered;
 * null: not wanted), all laid out like the state.  The leaving state is made of samples of in, of the kept signals and of out,
 * so pair k of grad_state_out is ADDED, in f32, to the two last samples (in the recurrence's order) of the gradient that
 * signal receives: pair K to grad_out as the first two launches read it (grad_out is not written), pair k to g_{k-1} in the
 * registers of the adjoint link that forms it, pair 0 to grad_in.  The adjoint scans stay masked and start from zero.
 * grad_state_in comes from lam_k at the forward's two first samples, the coefficients interpolated and unmasked: pair k + 1
 * receives section k's feedback part (fma(-a1[0], lam[0], -(a2[1] * lam[1])), -(a2[0] * lam[0])) and pair k its feed-forward
 * part (fma(b1[0], lam[0], b2[1] * lam[1]), b2[0] * lam[0]); pair k + 1 is the f32 sum (feed-forward part of section k + 1) +
 * (feedback part of section k), formed by the launches that hold the two lam, by one lane, in stream order: no atomics.  With
 * frame gradients the per-sample gradients at the six boundary slots take the history in place of the selected +0
 * (grad_a1[0] = -lam[0] * hy1, ...) and enter the f64 contraction like any other sample; state_in null: zeros, the slots
 * masked as in the call without a state.  Launches, 2 K + 2 without frame gradients and 3 K + 2 with them, K = 1 included
 * (rf_var2_plan_backward_cascade_frames_stream_num_kernels): "var2_adj_frames_tails_stream_1d"; per boundary "var2_carry_1d",
 * "var2_adj_frames_link_stream_1d" ("var2_adj_frames_link_keep_stream_1d" and "var2_frames_coef_stream_1d" with frame
 * gradients); "var2_carry_1d", "var2_adj_frames_pass2_stream_1d", "var2_biquad_frames_grad_stream_1d"; with frame gradients
 * "var2_frames_fold_cascade_1d".  The plan owns what rf_var2_plan_backward_cascade_frames_bytes says.  All three state pointers
 * null: the call IS rf_var2_plan_backward_cascade_frames.  Refusals: that call's in its order; then state_stride < 2 (K + 1); a
 * state pointer that is not 4-byte aligned; grad_state_in overlapping state_in, grad_state_out, a signal, a frame array or a
 * frame gradient; grad_in or a frame gradient overlapping state_in or grad_state_out; last, a host-only plan.
 * Out of scope: a state for the audio-rate calls (execute, execute_biquad, execute_cascade) and for rf_var_plan; hops that are
 * no powers of two; chunk starts off the frame grid; graph capture; 16-bit signals; sharding. */
int    rf_var2_plan_execute_cascade_frames_stream(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int n_sections,
                                                  int hop, int n_frames, int64_t frame_stride, void *out, void *const *kept,
                                                  const void *state_in, void *state_out, int64_t state_stride, void *stream);
int    rf_var2_plan_execute_cascade_frames_stream_timed(rf_var2_plan *plan, const void *in, const rf_var2_section *frames,
                                                        int n_sections, int hop, int n_frames, int64_t frame_stride, void *out,
                                                        void *const *kept, const void *state_in, void *state_out,
                                                        int64_t state_stride, void *stream, float *ms_out, const char **names_out,
                                                        int capacity);
int    rf_var2_plan_cascade_frames_stream_num_kernels(const rf_var2_plan *plan, int n_sections);      /* 0: n_sections out of range */
size_t rf_var2_plan_cascade_frames_stream_state_bytes(const rf_var2_plan *plan, int n_sections, int64_t state_stride);
int    rf_var2_plan_backward_cascade_frames_stream(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int n_sections,
                                                   int hop, int n_frames, int64_t frame_stride, const void *const *kept, const void *out,
                                                   const void *grad_out, void *grad_in, const rf_var2_section_grad *frame_grads,
                                                   const void *state_in, const void *grad_state_out, void *grad_state_in,
                                                   int64_t state_stride, void *stream);
int    rf_var2_plan_backward_cascade_frames_stream_timed(rf_var2_plan *plan, const void *in, const rf_var2_section *frames,
                                                         int n_sections, int hop, int n_frames, int64_t frame_stride,
                                                         const void *const *kept, const void *out, const void *grad_out, void *grad_in,
                                                         const rf_var2_section_grad *frame_grads, const void *state_in,
                                                         const void *grad_state_out, void *grad_state_in, int64_t state_stride,
                                                         void *stream, float *ms_out, const char **names_out, int capacity);
int    rf_var2_plan_backward_cascade_frames_stream_num_kernels(const rf_var2_plan *plan, int n_sections, int with_frame_gradients);

/* ---- misc ------------------------------------------------------------------------------- */
const char *rf_last_error_string(void);
const char *rf_version(void);
/* number of visible HIP devices (0 when there is none); never fails */
int rf_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* RECFILTER_AMD_H */
