// kernels_var.hip -- first-order scans whose feedback changes from sample to sample (edge-aware smoothing by the
// domain-transform recursive filter, Gastal & Oliveira 2011).
//
//   causal (+d):      y[i] = (1 - w[i])   * x[i] + w[i]   * y[i-1]         w[0] and w[N] count as 0: a select, never a product
//   anticausal (-d):  y[i] = (1 - w[i+1]) * x[i] + w[i+1] * y[i+1]
//
// The three-stage tiling of the constant-coefficient paths with the carry operators read from the weight plane instead of a
// table.  A stage is one scan, or a causal scan directly followed by the anticausal scan on the same weights (VAR_PAIR).
// Tile [t0, t1) of a line, zero entry:  u = local causal scan of x,  p[i] = w[t0] * ... * w[i]  (so y = u + p * c_t),
// v_u / v_p = local anticausal scans of u / p,  q[t0] = w[t0+1] * ... * w[t1]:
//   var_tails_x / var_tails_y   E1 = u[t1-1], P1 = p[t1-1], E2 = v_u[t0], G = v_p[t0], P2 = q[t0]   (a single scan: its two)
//   var_carry                   c_0 = 0, c_{t+1} = E1_t + P1_t c_t;   d_{M-1} = 0, d_{t-1} = E2_t + G_t c_t + P2_t d_t
//   var_pass2_x / var_pass2_y   reloads the tile, reruns the recurrence(s) from c_t and d_t, stores
// The final pass RERUNS the recurrences (it does not superpose u + p c): weights of exactly 0 and 1 give exact results.
//
// One lane owns the 64 samples of a line's tile in registers, with the 65 weights that couple them (w[t1] belongs to the next
// tile: the anticausal scan enters through it).  Along y the lane is a column: every access of a wave is 256 contiguous bytes,
// no LDS.  Along x a workgroup of one wave takes 64 rows x 64 columns: 16-byte row loads, a transposition through LDS rows
// padded to 68 dwords (ds_write_b128 and ds_read_b128 both conflict-free), the scan, the way back, 16-byte stores.
// Samples a partial tile misses are loaded from a safe address inside the plane and selected away where they are consumed
// (image 0, weight 0); they are never stored.  A workgroup has loaded its whole tile before it stores: in == out is legal.
//
// Power form (POWER, rf_var_plan_execute_power): the weight plane holds exponents d >= 0 and a stage carries l = log2(base);
// the lane's 65 registers become w = exp2(d * l) in place, one multiply and one v_exp_f32 each, before mask_tile -- the scans
// and var_carry see weights as before.  d = 0 gives 1 and d = +inf gives 0, exactly.  A separate instantiation: the plane-form
// kernels hold no trace of it.
//
// Byte planes (rf_smooth_plan, plan_smooth.cpp; the pair mode in the power form only): a stage along x may read uint8 planes -- a
// 4-byte load per request where the f32 form loads 16, widened exactly, into the same transposition -- and a final pass along y
// may store them, sat8 (pixel.h) of the f32 result, one byte per lane and row.  A trailing template TYPE argument with a default:
// the f32 instances are what they were, register for register.
//
// var_distances: the two exponent planes of the domain-transform filter from a guide image, one streaming launch.
//
// Adjoint stages (ADJ, rf_var_plan_backward): the adjoint of a causal scan is the ANTICAUSAL recurrence with unit input gain
//   lam[i] = g[i] + w[i+1] * lam[i+1]        dL/dx[i] = (1 - w[i]) * lam[i]
// and the adjoint of an anticausal scan the causal one,  mu[i] = g[i] + w[i] * mu[i-1],  dL/dx[i] = (1 - w[i+1]) * mu[i].  The same
// tiling: the tails are E = the local scan's last value and the P the forward scan of that direction stores, var_carry is
// unchanged, the final pass reruns the recurrence from the carry and stores the scaled state -- and, where VarArgs names planes
// for it, the unscaled one.  Single scans, f32.  A trailing template argument with a default, as the byte planes'.  With POWER
// (rf_var_plan_backward_power) the exponents become weights where the forward instances convert them: the adjoint recurrences see
// weights as before.
//
// var_grad: the weight gradient of one scan from its adjoint state and its saved input and output, one streaming launch; the
// planes are summed in a register, in index order (no atomics: a backward call is reproducible bit for bit).  Its POWER instances
// give the gradient of an EXPONENT plane: d/dd exp2(d l) = w ln(base), so the register sum is multiplied by w * ln_base, w formed
// from d as the scans form it -- never by d itself (d = +inf: w = 0, a gradient of exactly 0).
//
// Its BASES instances (rf_var_plan_backward_power_bases) also reduce d * w * dL/dw -- base * dL/dbase -- in f64 to one slab entry
// per workgroup, and var_param_sum, one workgroup, sums the slabs in index order: no atomics there either.
//
// var_distances_grad (rf_var_distances_backward): the adjoint of var_distances, a gather -- a guide sample collects from the (at
// most) four differences it takes part in, with the sign of each; one streaming launch, no atomics.
//
// The batch (rf_smooth_plan_create_batched): every kernel takes `batch` images in one launch, the image index on gridDim.z (beside
// the plane in the pass kernels: z = b * n_planes + pl).  Image b's planes, weight plane, tails and carries are image 0's plus a
// wave-uniform 64-bit offset; an image keeps its own tile grid from its row 0 and column 0 and its own borders, so its result is
// what a launch of that image alone gives, bit for bit, and no sample of one image meets a sample of another.
//
// Volumes (rf_var_plan_create_volume, plan_var.cpp) run these kernels as they are: the slices of an x or y stage are the batch, and
// a z stage is var_y_kernel / var_grad_kernel<1, ...> on the (width * height) x depth view -- the launchers take dim = 2 for it and
// differ in the name they report.  var_distances_volume and its adjoint var_distances_volume_grad
// (rf_var_distances_volume_backward) are the two kernels volumes add.
#include "kernels_var.h"

#include "pixel.h"
#include "var_device.h"

#include <algorithm>
#include <string>

namespace rf {

namespace {

// (the tile-local recurrences, the masks, power_weight, request_tile and transpose_in: var_device.h, shared with kernels_var_signal.hip)
__device__ __forceinline__ int64_t tail_index(const VarArgs &a, int t, int comp, int pl, int line) {
    return (((int64_t)t * kVarComponents + comp) * a.n_planes + pl) * a.lines + line;
}
__device__ __forceinline__ int64_t carry_index(const VarArgs &a, int t, int which, int pl, int line) {
    return (((int64_t)t * 2 + which) * a.n_planes + pl) * a.lines + line;
}

// the batch (rf_smooth_plan_create_batched): gridDim.z = batch * n_planes, image b = z / n_planes.  Everything that depends on b
// is a wave-uniform 64-bit offset added to a base pointer once; behind that an image is tiled, and its tails and carries laid
// out, as the only image of a launch would be (batch 1: every offset is 0).
struct VarImage {
    int pl;
    int64_t b;
};
__device__ __forceinline__ VarImage image_of(const VarArgs &a, unsigned z) {
    const unsigned b = z / (unsigned)a.n_planes;
    return {(int)(z - b * (unsigned)a.n_planes), (int64_t)b};
}

template <int MODE>
__device__ __forceinline__ void store_tails(const VarArgs &a, float *tails, int t, int pl, int line, const float (&out)[kVarComponents]) {
    if constexpr (MODE != VAR_ANTICAUSAL) tails[tail_index(a, t, VAR_E1, pl, line)] = out[VAR_E1];
    if constexpr (MODE != VAR_CAUSAL) tails[tail_index(a, t, VAR_E2, pl, line)] = out[VAR_E2];
    if (pl != 0) return;
    if constexpr (MODE != VAR_ANTICAUSAL) tails[tail_index(a, t, VAR_P1, 0, line)] = out[VAR_P1];
    if constexpr (MODE == VAR_PAIR) tails[tail_index(a, t, VAR_G, 0, line)] = out[VAR_G];
    if constexpr (MODE != VAR_CAUSAL) tails[tail_index(a, t, VAR_P2, 0, line)] = out[VAR_P2];
}

// ---- along y: lane = column -------------------------------------------------------------------------------------------
// DST: the samples the final pass stores -- float, or uint8_t (the last pass of a byte image, rf_smooth_plan: sat8 of pixel.h, one
// byte per lane and row).  Instantiated for the pair mode in the power form only.
// The anticausal final pass sits just under the 168 registers of three waves per SIMD; with the batch offsets in its scalar
// registers the allocator, left alone, lands just above.  Asked for three waves it stays there (no scratch: profiles/r20).
template <int MODE, bool FINAL, bool ADJ>
constexpr int y_waves() { return MODE == VAR_ANTICAUSAL && FINAL && !ADJ ? 3 : 1; }

template <int MODE, bool FINAL, bool POWER, typename DST = float, bool ADJ = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(y_waves<MODE, FINAL, ADJ>()))) var_y_kernel(VarArgs a) {
    static_assert(!ADJ || MODE != VAR_PAIR, "adjoint stages: single scans");
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= a.width) return;                       // (no barrier below: lanes are independent)
    const int t = blockIdx.y, t0 = t * T;
    const VarImage im = image_of(a, blockIdx.z);
    const int pl = im.pl;
    const int64_t pitch = a.width;
    const float *src = static_cast<const float *>(a.src[pl]) + im.b * a.src_stride;
    const float *weights = a.weights + im.b * a.weights_stride;
    float *tails = a.tails + im.b * a.tails_stride;
    const float *carry = a.carry + im.b * a.carry_stride;
    float x[T], w[T + 1];
#pragma unroll
    for (int i = 0; i < T; i++) {
        const int r = min(t0 + i, a.height - 1);      // wave-uniform row: a scalar base and the lane's column
        x[i] = (src + r * pitch)[col];
        w[i] = (weights + r * pitch)[col];
    }
    w[T] = 0.0f;
    if constexpr (MODE != VAR_CAUSAL || (ADJ && FINAL)) w[T] = (weights + min(t0 + T, a.height - 1) * pitch)[col];
    if constexpr (POWER) {
#pragma unroll
        for (int i = 0; i < T; i++) w[i] = power_weight(w[i], a.log2_base);
        if constexpr (MODE != VAR_CAUSAL || (ADJ && FINAL)) w[T] = power_weight(w[T], a.log2_base);
    }
    float c = 0.0f, d = 0.0f;
    if constexpr (FINAL) {
        if constexpr (MODE != VAR_ANTICAUSAL) c = carry[carry_index(a, t, 0, pl, col)];
        if constexpr (MODE != VAR_CAUSAL) d = carry[carry_index(a, t, 1, pl, col)];
    }
    mask_tile(x, w, t0, a.height);
    if constexpr (ADJ) {
        if constexpr (FINAL) {
            tile_final_adjoint<MODE>(x, w, c, d);
            float *dst = static_cast<float *>(a.dst[pl]) + im.b * a.dst_stride;
            float *lam = a.lam[pl] ? static_cast<float *>(a.lam[pl]) + im.b * a.lam_stride : nullptr;
#pragma unroll
            for (int i = 0; i < T; i++)
                if (t0 + i < a.height) (dst + (t0 + i) * pitch)[col] = adjoint_result<MODE>(x, w, i);
            if (lam) {
#pragma unroll
                for (int i = 0; i < T; i++)
                    if (t0 + i < a.height) (lam + (t0 + i) * pitch)[col] = x[i];
            }
        } else {
            float out[kVarComponents];
            tile_tails_adjoint<MODE>(x, w, pl == 0, out);
            store_tails<MODE>(a, tails, t, pl, col, out);
        }
    } else if constexpr (FINAL) {
        tile_final<MODE>(x, w, c, d);
        DST *dst = static_cast<DST *>(a.dst[pl]) + im.b * a.dst_stride;
#pragma unroll
        for (int i = 0; i < T; i++)
            if (t0 + i < a.height) (dst + (t0 + i) * pitch)[col] = PixelTraits<DST>::store(x[i]);
    } else {
        float out[kVarComponents];
        tile_tails<MODE>(x, w, pl == 0, out);
        store_tails<MODE>(a, tails, t, pl, col, out);
    }
}

// ---- along x: workgroup = one wave = 64 rows x 64 columns, lane = row after the transposition -----------------------------
// (request_tile for f32 planes and transpose_in: var_device.h)
// a byte plane: the same rows and chunks as an f32 plane's request_tile, 4 bytes where the f32 form moves 16, widened exactly -- a wave instruction moves four
// rows of 64 contiguous bytes; everything behind the loads is the f32 kernel's
__device__ __forceinline__ void request_tile(const uint8_t *plane, const VarArgs &a, int r0, int c0, float (&v)[T]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < T / 4; k++) {
        const int flat = k * 64 + lane;
        const int r = min(r0 + (flat >> 4), a.height - 1);
        const int c = min(c0 + (flat & 15) * 4, a.width - 4);      // (the width is a multiple of 4: a 4-byte aligned address)
        const uint32_t q = *reinterpret_cast<const uint32_t *>(plane + (int64_t)r * a.width + c);
#pragma unroll
        for (int j = 0; j < 4; j++) v[4 * k + j] = (float)((q >> (8 * j)) & 255u);
    }
}

// SRC: the samples of the source planes -- float, or uint8_t (the first stage of a byte image, rf_smooth_plan; the destination
// stays f32).  Instantiated for the pair mode in the power form only.
template <int MODE, bool FINAL, bool POWER, typename SRC = float, bool ADJ = false>
__global__ void __launch_bounds__(64) var_x_kernel(VarArgs a) {
    static_assert(!ADJ || MODE != VAR_PAIR, "adjoint stages: single scans");
    __shared__ __attribute__((aligned(16))) float lds[T * LDS_PITCH];
    const int lane = threadIdx.x;
    const int t = blockIdx.x, t0 = t * T, r0 = blockIdx.y * 64;
    const VarImage im = image_of(a, blockIdx.z);
    const int pl = im.pl;
    const int row = r0 + lane;
    const SRC *src = static_cast<const SRC *>(a.src[pl]) + im.b * a.src_stride;
    const float *weights = a.weights + im.b * a.weights_stride;
    float *tails = a.tails + im.b * a.tails_stride;
    const float *carry = a.carry + im.b * a.carry_stride;
    float vx[T], vw[T];
    request_tile(src, a, r0, t0, vx);
    request_tile(weights, a, r0, t0, vw);
    float w_next = 0.0f;                             // w[t1], the next tile's first weight
    if constexpr (MODE != VAR_CAUSAL || (ADJ && FINAL)) w_next = weights[(int64_t)min(row, a.height - 1) * a.width + min(t0 + T, a.width - 1)];
    float c = 0.0f, d = 0.0f;
    if constexpr (FINAL) {
        const int line = min(row, a.height - 1);
        if constexpr (MODE != VAR_ANTICAUSAL) c = carry[carry_index(a, t, 0, pl, line)];
        if constexpr (MODE != VAR_CAUSAL) d = carry[carry_index(a, t, 1, pl, line)];
    }
    float x[T], wt[T], w[T + 1];
    transpose_in(vx, lds, x);
    transpose_in(vw, lds, wt);
#pragma unroll
    for (int i = 0; i < T; i++) w[i] = wt[i];
    w[T] = w_next;
    if constexpr (POWER) {
#pragma unroll
        for (int i = 0; i < T; i++) w[i] = power_weight(w[i], a.log2_base);
        if constexpr (MODE != VAR_CAUSAL || (ADJ && FINAL)) w[T] = power_weight(w[T], a.log2_base);
    }
    mask_tile(x, w, t0, a.width);
    __builtin_amdgcn_sched_barrier(0);      // (the scans stay behind the transposition: they would hold its registers)
    if constexpr (ADJ) {
        if constexpr (FINAL) {
            tile_final_adjoint<MODE>(x, w, c, d);
            // the way back twice: the scaled state to dst, then (where the plan wants it) the state itself to lam
            float *planes[2] = {static_cast<float *>(a.dst[pl]) + im.b * a.dst_stride,
                                a.lam[pl] ? static_cast<float *>(a.lam[pl]) + im.b * a.lam_stride : nullptr};
#pragma unroll
            for (int which = 0; which < 2; which++) {
                if (which == 1 && !planes[1]) break;      // (uniform)
                if (which == 1) __syncthreads();
#pragma unroll
                for (int k = 0; k < T / 4; k++) {
                    const float4 q = which == 0 ? make_float4(adjoint_result<MODE>(x, w, 4 * k), adjoint_result<MODE>(x, w, 4 * k + 1),
                                                              adjoint_result<MODE>(x, w, 4 * k + 2), adjoint_result<MODE>(x, w, 4 * k + 3))
                                                : make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
                    *reinterpret_cast<float4 *>(lds + lane * LDS_PITCH + k * 4) = q;
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < T / 4; k++) {
                    const int flat = k * 64 + lane;
                    const int r = r0 + (flat >> 4), col = t0 + (flat & 15) * 4;
                    const float4 q = *reinterpret_cast<const float4 *>(lds + (flat >> 4) * LDS_PITCH + (flat & 15) * 4);
                    if (r < a.height && col < a.width) *reinterpret_cast<float4 *>(planes[which] + (int64_t)r * a.width + col) = q;
                }
            }
        } else {
            float out[kVarComponents];
            tile_tails_adjoint<MODE>(x, w, pl == 0, out);
            if (row < a.height) store_tails<MODE>(a, tails, t, pl, row, out);
        }
    } else if constexpr (FINAL) {
        tile_final<MODE>(x, w, c, d);
#pragma unroll
        for (int k = 0; k < T / 4; k++)
            *reinterpret_cast<float4 *>(lds + lane * LDS_PITCH + k * 4) = make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
        __syncthreads();
        float *dst = static_cast<float *>(a.dst[pl]) + im.b * a.dst_stride;
#pragma unroll
        for (int k = 0; k < T / 4; k++) {
            const int flat = k * 64 + lane;
            const int r = r0 + (flat >> 4), col = t0 + (flat & 15) * 4;
            const float4 q = *reinterpret_cast<const float4 *>(lds + (flat >> 4) * LDS_PITCH + (flat & 15) * 4);
            if (r < a.height && col < a.width) *reinterpret_cast<float4 *>(dst + (int64_t)r * a.width + col) = q;
        }
    } else {
        float out[kVarComponents];
        tile_tails<MODE>(x, w, pl == 0, out);
        if (row < a.height) store_tails<MODE>(a, tails, t, pl, row, out);
    }
}

// ---- carries: one lane per line and plane -----------------------------------------------------------------------------------
// The tails of CHUNK tiles are requested together, ahead of the recurrence that consumes them (tiles past the end: the last
// tile's, not consumed).
template <int MODE>
__global__ void __launch_bounds__(256) var_carry_kernel(VarArgs a) {
    constexpr int CHUNK = 8;
    const int line = blockIdx.x * 256 + threadIdx.x;
    if (line >= a.lines) return;
    const int pl = blockIdx.y, M = a.tiles;
    const float *tails = a.tails + (int64_t)blockIdx.z * a.tails_stride;      // blockIdx.z: the image of the batch
    float *carry = a.carry + (int64_t)blockIdx.z * a.carry_stride;
    if constexpr (MODE != VAR_ANTICAUSAL) {
        float c = 0.0f;
        for (int tb = 0; tb < M; tb += CHUNK) {
            float e[CHUNK], p[CHUNK];
#pragma unroll
            for (int j = 0; j < CHUNK; j++) {
                const int t = min(tb + j, M - 1);
                e[j] = tails[tail_index(a, t, VAR_E1, pl, line)];
                p[j] = tails[tail_index(a, t, VAR_P1, 0, line)];
            }
#pragma unroll
            for (int j = 0; j < CHUNK; j++) {
                if (tb + j < M) {
                    carry[carry_index(a, tb + j, 0, pl, line)] = c;
                    c = __builtin_fmaf(p[j], c, e[j]);
                }
            }
        }
    }
    if constexpr (MODE != VAR_CAUSAL) {
        float d = 0.0f;
        for (int tb = M - 1; tb >= 0; tb -= CHUNK) {
            float e[CHUNK], p[CHUNK], g[CHUNK], c[CHUNK];
#pragma unroll
            for (int j = 0; j < CHUNK; j++) {
                const int t = max(tb - j, 0);
                e[j] = tails[tail_index(a, t, VAR_E2, pl, line)];
                p[j] = tails[tail_index(a, t, VAR_P2, 0, line)];
                g[j] = 0.0f; c[j] = 0.0f;
                if constexpr (MODE == VAR_PAIR) {
                    g[j] = tails[tail_index(a, t, VAR_G, 0, line)];
                    c[j] = carry[carry_index(a, t, 0, pl, line)];       // (this lane wrote it above)
                }
            }
#pragma unroll
            for (int j = 0; j < CHUNK; j++) {
                if (tb - j >= 0) {
                    carry[carry_index(a, tb - j, 1, pl, line)] = d;
                    d = __builtin_fmaf(p[j], d, e[j]);
                    if constexpr (MODE == VAR_PAIR) d = __builtin_fmaf(g[j], c[j], d);
                }
            }
        }
    }
}

// ---- var_distances: lane = 4 adjacent columns of one row -------------------------------------------------------------------
// a lane's chunk of one guide channel as four floats; bytes convert exactly
__device__ __forceinline__ void load_chunk(const float *g, int64_t at, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4 *>(g + at);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void load_chunk(const uint8_t *g, int64_t at, float (&v)[4]) {
    const uint32_t q = *reinterpret_cast<const uint32_t *>(g + at);
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = (float)((q >> (8 * j)) & 255u);
}

// The element to the left of the chunk and the chunk of the row above come from clamped addresses (column 0: the chunk's own
// first element; row 0: the row itself) and are selected away there.  Rows beyond gridDim.y are taken in a stride loop.
template <typename G>
__global__ void __launch_bounds__(256) var_distances_kernel(VarDistArgs a) {
    const int c = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (c >= a.width) return;
    const int64_t b = blockIdx.z;                    // the image of the batch: its own row 0 and column 0
    float *const out_dx = a.dx + b * ((int64_t)a.width * a.height), *const out_dy = a.dy + b * ((int64_t)a.width * a.height);
    for (int r = blockIdx.y; r < a.height; r += gridDim.y) {
        const int64_t own_at = (int64_t)r * a.width + c, up_at = (int64_t)max(r - 1, 0) * a.width + c;
        float sx[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int ch = 0; ch < a.n_guide; ch++) {
            const G *g = static_cast<const G *>(a.guide[ch]) + b * a.guide_stride;
            float own[4], up[4];
            load_chunk(g, own_at, own);
            load_chunk(g, up_at, up);
            const float left = (float)g[own_at - (c > 0 ? 1 : 0)];
            sx[0] += fabsf(own[0] - left);
#pragma unroll
            for (int j = 1; j < 4; j++) sx[j] += fabsf(own[j] - own[j - 1]);
#pragma unroll
            for (int j = 0; j < 4; j++) sy[j] += fabsf(own[j] - up[j]);
        }
        float dx[4], dy[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            dx[j] = (c + j == 0) ? 1.0f : 1.0f + a.scale * sx[j];
            dy[j] = (r == 0) ? 1.0f : 1.0f + a.scale * sy[j];
        }
        *reinterpret_cast<float4 *>(out_dx + own_at) = make_float4(dx[0], dx[1], dx[2], dx[3]);
        *reinterpret_cast<float4 *>(out_dy + own_at) = make_float4(dy[0], dy[1], dy[2], dy[3]);
    }
}

// ---- var_distances_volume: lane = 4 adjacent columns of one row, walking z ------------------------------------------------------
// d_x and d_y of a slice are var_distances' expressions on that slice, term for term.  The lanes are the (row, chunk) pairs of a
// slice, flat on gridDim.x (a narrow volume still fills its waves); gridDim.y takes segments of kVarDistSlices slices.  A lane
// keeps its chunk of the slice before, per channel, in registers: the guide is read once, plus one slice per segment.  NG: the
// channels the registers are laid out for (1, 4 or RF_MAX_PLANES; n_guide <= NG).
template <typename G, int NG>
__global__ void __launch_bounds__(256) var_distances_volume_kernel(VarDistVolumeArgs a) {
    const int chunks = a.width / 4;
    const int64_t flat = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (flat >= (int64_t)chunks * a.height) return;
    const int r = (int)(flat / chunks), c = (int)(flat - (int64_t)r * chunks) * 4;
    const int64_t slice = (int64_t)a.width * a.height;
    const int64_t own_row = (int64_t)r * a.width + c, up_row = (int64_t)max(r - 1, 0) * a.width + c;
    const int z0 = blockIdx.y * kVarDistSlices, z1 = min(z0 + kVarDistSlices, a.depth);
    float before[NG][4];
#pragma unroll
    for (int ch = 0; ch < NG; ch++)
        if (ch < a.n_guide) load_chunk(static_cast<const G *>(a.guide[ch]), (int64_t)max(z0 - 1, 0) * slice + own_row, before[ch]);
    for (int z = z0; z < z1; z++) {
        const int64_t own_at = z * slice + own_row, up_at = z * slice + up_row;
        float sx[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sy[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ch = 0; ch < NG; ch++) {
            if (ch >= a.n_guide) continue;
            const G *g = static_cast<const G *>(a.guide[ch]);
            float own[4], up[4];
            load_chunk(g, own_at, own);
            load_chunk(g, up_at, up);
            const float left = (float)g[own_at - (c > 0 ? 1 : 0)];
            sx[0] += fabsf(own[0] - left);
#pragma unroll
            for (int j = 1; j < 4; j++) sx[j] += fabsf(own[j] - own[j - 1]);
#pragma unroll
            for (int j = 0; j < 4; j++) sy[j] += fabsf(own[j] - up[j]);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                sz[j] += fabsf(own[j] - before[ch][j]);
                before[ch][j] = own[j];
            }
        }
        float dx[4], dy[4], dz[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            dx[j] = (c + j == 0) ? 1.0f : 1.0f + a.scale * sx[j];
            dy[j] = (r == 0) ? 1.0f : 1.0f + a.scale * sy[j];
            dz[j] = (z == 0) ? a.spacing_z : a.spacing_z + a.scale * sz[j];
        }
        *reinterpret_cast<float4 *>(a.dx + own_at) = make_float4(dx[0], dx[1], dx[2], dx[3]);
        *reinterpret_cast<float4 *>(a.dy + own_at) = make_float4(dy[0], dy[1], dy[2], dy[3]);
        *reinterpret_cast<float4 *>(a.dz + own_at) = make_float4(dz[0], dz[1], dz[2], dz[3]);
    }
}

// ---- var_grad: lane = 4 adjacent columns of one row, as var_distances ---------------------------------------------------------
// The sample before the chunk along the scanned dimension comes from a clamped address (dim 0: the element to the left of the
// chunk, column 0: the chunk's own first element; dim 1: the chunk of the row above, row 0: the row itself); element 0 of the
// gradient is 0 by a select, whatever was read for it.
template <int DIM>
__device__ __forceinline__ void load_previous(const float *p, int64_t own_at, int64_t before_at, const float (&own)[4], float (&prev)[4]) {
    if constexpr (DIM == 0) {
        prev[0] = p[before_at];
#pragma unroll
        for (int j = 1; j < 4; j++) prev[j] = own[j - 1];
    } else {
        load_chunk(p, before_at, prev);
    }
}

// BASES (rf_var_plan_backward_power_bases; POWER only): the launch also reduces t[i] = (w[i] == 0 ? 0 : d[i] * w[i] * dL/dw[i]), whose sum
// over the plane is base * dL/dbase.  A lane adds its t in f64, in the order it visits its rows; the workgroup folds its lanes by a
// fixed tree (shuffles down the wave, then the four waves in index order through LDS) and stores ONE slab entry at the index of
// its block: no atomics, and a second run gives the same bits.  Lanes past the width stay alive for the barrier and contribute 0;
// a null `grad` switches the plane's store off.  d is never a factor where w is 0 (d = +inf: exactly 0).
__device__ __forceinline__ double var_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <int DIM, bool CAUSAL, bool POWER = false, bool BASES = false>
__global__ void __launch_bounds__(256) var_grad_kernel(VarGradArgs a) {
    static_assert(!BASES || POWER, "the base gradient belongs to the power form");
    const int c = (blockIdx.x * 256 + threadIdx.x) * 4;
    if constexpr (!BASES) {
        if (c >= a.width) return;
    }
    const int64_t b = blockIdx.z;                    // the image of the batch
    [[maybe_unused]] double acc = 0.0;
    [[maybe_unused]] const bool store = !BASES || a.grad != nullptr;      // (uniform)
    float *const grad = store ? a.grad + b * a.grad_stride : nullptr;
    const int rows = BASES && c >= a.width ? 0 : a.height;      // (BASES: a lane past the width walks no row)
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const int64_t own_at = (int64_t)r * a.width + c;
        const int64_t before_at = DIM == 0 ? own_at - (c > 0 ? 1 : 0) : (int64_t)max(r - 1, 0) * a.width + c;
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int pl = 0; pl < a.n_planes; pl++) {
            const float *const p_lam = a.lam[pl] + b * a.lam_stride, *const p_x = a.x[pl] + b * a.x_stride, *const p_y = a.y[pl] + b * a.y_stride;
            float lam[4], x[4], y[4], before[4], term[4];
            if constexpr (CAUSAL) {              // lam[i] * (y[i-1] - x[i])
                load_chunk(p_lam, own_at, lam);
                load_chunk(p_x, own_at, x);
                if constexpr (DIM == 0) load_chunk(p_y, own_at, y);
                load_previous<DIM>(p_y, own_at, before_at, y, before);
#pragma unroll
                for (int j = 0; j < 4; j++) term[j] = lam[j] * (before[j] - x[j]);
            } else {                             // lam[i-1] * (y[i] - x[i-1])
                load_chunk(p_y, own_at, y);
                if constexpr (DIM == 0) { load_chunk(p_lam, own_at, lam); load_chunk(p_x, own_at, x); }
                load_previous<DIM>(p_lam, own_at, before_at, lam, before);
                float x_before[4];
                load_previous<DIM>(p_x, own_at, before_at, x, x_before);
#pragma unroll
                for (int j = 0; j < 4; j++) term[j] = before[j] * (y[j] - x_before[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) s[j] = pl == 0 ? term[j] : s[j] + term[j];
        }
        if constexpr (POWER) {                   // dL/dd = (w * ln base) * dL/dw, w as the scans form it
            float d[4];
            load_chunk(a.exponents + b * a.exponents_stride, own_at, d);
            if constexpr (BASES) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float w = power_weight(d[j], a.log2_base);
                    const double t = w == 0.0f ? 0.0 : ((double)d[j] * (double)w) * (double)s[j];
                    acc += (DIM == 0 ? c + j == 0 : r == 0) ? 0.0 : t;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) s[j] = (power_weight(d[j], a.log2_base) * a.ln_base) * s[j] + 0.0f;      // (w = 0: +0, not -0)
        }
        if constexpr (BASES) {
            if (!store) continue;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] = (DIM == 0 ? c + j == 0 : r == 0) ? 0.0f : s[j];
        if (a.accumulate) {
            float old[4];
            load_chunk(grad, own_at, old);
#pragma unroll
            for (int j = 0; j < 4; j++) s[j] = old[j] + s[j];
        }
        *reinterpret_cast<float4 *>(grad + own_at) = make_float4(s[0], s[1], s[2], s[3]);
    }
    if constexpr (BASES) {
        __shared__ double red[4];
        const double wave = var_wave_sum(acc);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wave;
        __syncthreads();
        if (threadIdx.x == 0)
            a.slabs[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// ---- var_param_sum: one workgroup, the f64 sibling of coeff_grad_sum (kernels_adjoint.hip) ------------------------------------------
// Every segment of slabs is summed lane-strided, folded down each wave and left in LDS, wave by wave; behind ONE barrier lane j sums
// the waves of the segments that name out[j], in index order, each times its host-formed factor.
constexpr int kParamSumThreads = 1024;
__global__ void __launch_bounds__(kParamSumThreads) var_param_sum_kernel(VarParamSumArgs a) {
    __shared__ double red[kVarParamSegments][kParamSumThreads / 64];
    const int tid = threadIdx.x;
    for (int s = 0; s < a.n_segments; s++) {
        const double *seg = a.slabs + a.offset[s];
        double v = 0.0;
        // eight loads in flight per lane, added in index order: the sum's bits do not depend on the unrolling
        int64_t i = tid;
        for (; i + 7 * kParamSumThreads < a.count[s]; i += 8 * kParamSumThreads) {
            double e[8];
#pragma unroll
            for (int j = 0; j < 8; j++) e[j] = seg[i + j * kParamSumThreads];
#pragma unroll
            for (int j = 0; j < 8; j++) v += e[j];
        }
        for (; i < a.count[s]; i += kParamSumThreads) v += seg[i];
        v = var_wave_sum(v);
        if ((tid & 63) == 0) red[s][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < a.n_out) {
        double total = 0.0;
        for (int s = 0; s < a.n_segments; s++) {
            if (a.target[s] != tid && a.target2[s] != tid) continue;
            double v = 0.0;
            for (int w = 0; w < kParamSumThreads / 64; w++) v += red[s][w];
            if (a.target[s] == tid) total += a.factor[s] * v;
            if (a.target2[s] == tid) total += a.factor2[s] * v;
        }
        a.out[tid] = total;
    }
}

// ---- var_dot: lane = 4 adjacent samples, a grid-stride walk -----------------------------------------------------------------------
constexpr int kDotMaxBlocks = 1024;
__global__ void __launch_bounds__(256) var_dot_kernel(VarDotArgs a) {
    __shared__ double red[6][4];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; e < a.n; e += (int64_t)gridDim.x * 1024) {
#pragma unroll
        for (int p = 0; p < 3; p++) {
            if (p >= a.n_pairs) continue;          // (uniform)
            float g[4], d[4];
            load_chunk(a.gd[p], e, g);
            load_chunk(a.d[p], e, d);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                acc[2 * p] += g[j] == 0.0f ? 0.0 : (double)g[j] * ((double)d[j] - (double)a.d0[p]);      // (d = +inf beside gd = 0: 0, not NaN)
                acc[2 * p + 1] += (double)g[j];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) {
        const double wave = var_wave_sum(acc[q]);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = wave;
    }
    __syncthreads();
    if (threadIdx.x < 2 * a.n_pairs) {
        const int q = threadIdx.x;
        a.slabs[(int64_t)q * gridDim.x + blockIdx.x] = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
    }
}

// ---- var_distances_grad: lane = 4 adjacent columns of one row, as var_distances ---------------------------------------------------
// the sign of a difference applied to the gradient that difference received: a select, sgn(0) = 0 (what the derivative of |.| is
// taken to be), so no product of a sign with a gradient is ever formed
__device__ __forceinline__ float signed_by(float difference, float g) { return difference > 0.0f ? g : (difference < 0.0f ? -g : 0.0f); }

// A guide sample takes part in the difference to its left (+), the one to its right (-), the one above (+) and the one below (-).
// The neighbours come from clamped addresses (column 0 / W-1: the chunk's own end element; row 0 / H-1: the row itself) and the
// terms they feed are selected away at the borders.  Rows beyond gridDim.y are taken in a stride loop.
__global__ void __launch_bounds__(256) var_distances_grad_kernel(VarDistGradArgs a) {
    const int c = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (c >= a.width) return;
    const bool has_right = c + 4 < a.width;
    const int64_t b = blockIdx.z;                    // the image of the batch: its own borders
    const float *const gdx = a.gdx + b * ((int64_t)a.width * a.height), *const gdy = a.gdy + b * ((int64_t)a.width * a.height);
    for (int r = blockIdx.y; r < a.height; r += gridDim.y) {
        const int64_t own_at = (int64_t)r * a.width + c, up_at = (int64_t)max(r - 1, 0) * a.width + c;
        const int64_t down_at = (int64_t)min(r + 1, a.height - 1) * a.width + c;
        const int64_t left_at = own_at - (c > 0 ? 1 : 0), right_at = own_at + (has_right ? 4 : 3);
        const bool has_down = r + 1 < a.height;
        float gx_own[4], gx[5], gy[4], gy_down[4];      // gx[4]: the gradient of the difference to the right of the chunk
        load_chunk(gdx, own_at, gx_own);
#pragma unroll
        for (int j = 0; j < 4; j++) gx[j] = gx_own[j];
        gx[4] = gdx[right_at];
        load_chunk(gdy, own_at, gy);
        load_chunk(gdy, down_at, gy_down);
        for (int ch = 0; ch < a.n_guide; ch++) {
            const float *g = a.guide[ch] + b * a.guide_stride;
            float chunk[4], own[6], up[4], down[4], out[4];      // own[0]: the element to the left, own[5]: the one to the right
            load_chunk(g, own_at, chunk);
#pragma unroll
            for (int j = 0; j < 4; j++) own[j + 1] = chunk[j];
            own[0] = g[left_at];
            own[5] = g[right_at];
            load_chunk(g, up_at, up);
            load_chunk(g, down_at, down);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float from_left = c + j > 0 ? signed_by(own[j + 1] - own[j], gx[j]) : 0.0f;
                const float from_right = (j < 3 || has_right) ? signed_by(own[j + 2] - own[j + 1], gx[j + 1]) : 0.0f;
                const float from_up = r > 0 ? signed_by(own[j + 1] - up[j], gy[j]) : 0.0f;
                const float from_down = has_down ? signed_by(down[j] - own[j + 1], gy_down[j]) : 0.0f;
                out[j] = a.scale * (((from_left - from_right) + from_up) - from_down);
            }
            float *dst = a.grad_guide[ch] + b * a.grad_guide_stride;
            if (a.accumulate) {
                float old[4];
                load_chunk(dst, own_at, old);
#pragma unroll
                for (int j = 0; j < 4; j++) out[j] = old[j] + out[j];
            }
            *reinterpret_cast<float4 *>(dst + own_at) = make_float4(out[0], out[1], out[2], out[3]);
        }
    }
}

// ---- var_distances_volume_grad: lane = 4 adjacent columns of one row, walking z, as var_distances_volume -------------------------
// A guide sample takes part in six differences: var_distances_grad's four in its slice, the one to the slice before (+) and the one
// to the slice after (-).  Neighbours come from clamped addresses (the slice before slice 0 and after slice D-1: the slice itself)
// and the terms they feed are selected away at the six faces.  The channels are independent and no array is indexed by the
// channel, so nothing goes to scratch whatever n_guide is.  Two forms of the walk, one arithmetic (guide_gradient_chunk):
//   ROLLING  the channel loop AROUND the walk: a lane keeps one channel's chunk of the slice before, its own and the slice after in
//            registers, so the guide is read once (plus one slice per segment and the row neighbours) -- and gdx, gdy, gdz once
//            PER CHANNEL.  One guide volume: every volume is read once.
//   else     the channel loop INSIDE the walk: gdx, gdy and gdz of a slice are loaded once for all channels (gdz rolls along z in
//            registers) and a channel's chunks of the slices before and after are read again from their clamped addresses, as
//            var_distances_grad reads the rows above and below -- the second and third touch of a slice follow the first by one
//            and two steps of the walk.  More than one guide volume.
struct VolumeLane {
    int r, c;
    bool has_right, has_down;
    int64_t slice, own_row, up_row, down_row, left_row, right_row;
};
__device__ __forceinline__ bool volume_lane(const VarDistVolumeGradArgs &a, VolumeLane &l) {
    const int chunks = a.width / 4;
    const int64_t flat = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (flat >= (int64_t)chunks * a.height) return false;
    l.r = (int)(flat / chunks);
    l.c = (int)(flat - (int64_t)l.r * chunks) * 4;
    l.has_right = l.c + 4 < a.width;
    l.has_down = l.r + 1 < a.height;
    l.slice = (int64_t)a.width * a.height;
    l.own_row = (int64_t)l.r * a.width + l.c;
    l.up_row = (int64_t)max(l.r - 1, 0) * a.width + l.c;
    l.down_row = (int64_t)min(l.r + 1, a.height - 1) * a.width + l.c;
    l.left_row = l.own_row - (l.c > 0 ? 1 : 0);
    l.right_row = l.own_row + (l.has_right ? 4 : 3);
    return true;
}

// the gradients a slice's differences received, of the lane's chunk: gx[4] belongs to the difference to the right of the chunk
struct SliceGradients {
    float gx[5], gy[4], gy_down[4];
};
__device__ __forceinline__ void load_slice_gradients(const VarDistVolumeGradArgs &a, const VolumeLane &l, int64_t at, SliceGradients &s) {
    float gx_own[4];
    load_chunk(a.gdx, at + l.own_row, gx_own);
#pragma unroll
    for (int j = 0; j < 4; j++) s.gx[j] = gx_own[j];
    s.gx[4] = a.gdx[at + l.right_row];
    load_chunk(a.gdy, at + l.own_row, s.gy);
    load_chunk(a.gdy, at + l.down_row, s.gy_down);
}

// one channel's chunk of slice z (at = z * slice): the six terms in the header's order, stored or added
__device__ __forceinline__ void guide_gradient_chunk(const VarDistVolumeGradArgs &a, const VolumeLane &l, const float *g, float *dst, int z, int64_t at,
                                                     const float (&before)[4], const float (&chunk)[4], const float (&after)[4],
                                                     const SliceGradients &s, const float (&gz)[4], const float (&gz_after)[4]) {
    const bool has_after = z + 1 < a.depth;
    float own[6], up[4], down[4], out[4];      // own[0]: the element to the left, own[5]: the one to the right
#pragma unroll
    for (int j = 0; j < 4; j++) own[j + 1] = chunk[j];
    own[0] = g[at + l.left_row];
    own[5] = g[at + l.right_row];
    load_chunk(g, at + l.up_row, up);
    load_chunk(g, at + l.down_row, down);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float from_left = l.c + j > 0 ? signed_by(own[j + 1] - own[j], s.gx[j]) : 0.0f;
        const float from_right = (j < 3 || l.has_right) ? signed_by(own[j + 2] - own[j + 1], s.gx[j + 1]) : 0.0f;
        const float from_up = l.r > 0 ? signed_by(own[j + 1] - up[j], s.gy[j]) : 0.0f;
        const float from_down = l.has_down ? signed_by(down[j] - own[j + 1], s.gy_down[j]) : 0.0f;
        const float from_before = z > 0 ? signed_by(chunk[j] - before[j], gz[j]) : 0.0f;
        const float from_after = has_after ? signed_by(after[j] - chunk[j], gz_after[j]) : 0.0f;
        out[j] = a.scale * (((((from_left - from_right) + from_up) - from_down) + from_before) - from_after);
    }
    if (a.accumulate) {
        float old[4];
        load_chunk(dst, at + l.own_row, old);
#pragma unroll
        for (int j = 0; j < 4; j++) out[j] = old[j] + out[j];
    }
    *reinterpret_cast<float4 *>(dst + at + l.own_row) = make_float4(out[0], out[1], out[2], out[3]);
}

template <bool ROLLING>
__global__ void __launch_bounds__(256) var_distances_volume_grad_kernel(VarDistVolumeGradArgs a) {
    VolumeLane l;
    if (!volume_lane(a, l)) return;
    const int z0 = blockIdx.y * kVarDistSlices, z1 = min(z0 + kVarDistSlices, a.depth);
    if constexpr (ROLLING) {
        for (int ch = 0; ch < a.n_guide; ch++) {
            const float *const g = a.guide[ch];
            float before[4], chunk[4], gz[4];
            load_chunk(g, (int64_t)max(z0 - 1, 0) * l.slice + l.own_row, before);
            load_chunk(g, (int64_t)z0 * l.slice + l.own_row, chunk);
            load_chunk(a.gdz, (int64_t)z0 * l.slice + l.own_row, gz);
            for (int z = z0; z < z1; z++) {
                const int64_t at = (int64_t)z * l.slice, after_at = (int64_t)min(z + 1, a.depth - 1) * l.slice;
                float after[4], gz_after[4];
                SliceGradients s;
                load_chunk(g, after_at + l.own_row, after);
                load_chunk(a.gdz, after_at + l.own_row, gz_after);
                load_slice_gradients(a, l, at, s);
                guide_gradient_chunk(a, l, g, a.grad_guide[ch], z, at, before, chunk, after, s, gz, gz_after);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    before[j] = chunk[j];
                    chunk[j] = after[j];
                    gz[j] = gz_after[j];
                }
            }
        }
    } else {
        float gz[4];
        load_chunk(a.gdz, (int64_t)z0 * l.slice + l.own_row, gz);
        for (int z = z0; z < z1; z++) {
            const int64_t at = (int64_t)z * l.slice, before_at = (int64_t)max(z - 1, 0) * l.slice, after_at = (int64_t)min(z + 1, a.depth - 1) * l.slice;
            float gz_after[4];
            SliceGradients s;
            load_chunk(a.gdz, after_at + l.own_row, gz_after);
            load_slice_gradients(a, l, at, s);
            for (int ch = 0; ch < a.n_guide; ch++) {
                const float *const g = a.guide[ch];
                float before[4], chunk[4], after[4];
                load_chunk(g, before_at + l.own_row, before);
                load_chunk(g, at + l.own_row, chunk);
                load_chunk(g, after_at + l.own_row, after);
                guide_gradient_chunk(a, l, g, a.grad_guide[ch], z, at, before, chunk, after, s, gz, gz_after);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) gz[j] = gz_after[j];
        }
    }
}

int launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("launch of %s failed: %s", what, hipGetErrorString(e)); return RF_ERR_HIP; }
    return RF_OK;
}

template <bool FINAL>
int launch_pass(const VarArgs &a, int dim, hipStream_t stream) {
    static const char *const kAxis[3] = {"x", "y", "z"};
    const char *const axis = kAxis[dim];
    // a z stage of a volume plan is the y kernels on the view plan_var.cpp describes: only its name differs
    if (dim == 2) dim = 1;
    const int cross = dim == 0 ? a.height : a.width;          // lines, 64 per workgroup
    const dim3 block(64);
    const dim3 grid = dim == 0 ? dim3((unsigned)a.tiles, (unsigned)((cross + 63) / 64), (unsigned)(a.batch * a.n_planes))
                               : dim3((unsigned)((cross + 63) / 64), (unsigned)a.tiles, (unsigned)(a.batch * a.n_planes));
    if (a.adjoint) {
        const std::string name = std::string(FINAL ? "var_adj_pass2_" : "var_adj_tails_") + axis;
        const char *what = name.c_str();
        if (a.src_u8 || a.dst_u8 || a.mode == VAR_PAIR) {
            set_error("%s: adjoint stages are single scans on f32 planes", what);
            return RF_ERR_UNSUPPORTED;
        }
#define RF_VAR_LAUNCH_ADJOINT_FORM(MODE, POWER)                                                                          \
        if (dim == 0) hipLaunchKernelGGL((var_x_kernel<MODE, FINAL, POWER, float, true>), grid, block, 0, stream, a);    \
        else hipLaunchKernelGGL((var_y_kernel<MODE, FINAL, POWER, float, true>), grid, block, 0, stream, a)
#define RF_VAR_LAUNCH_ADJOINT(MODE)                                                                                      \
        if (a.power) { RF_VAR_LAUNCH_ADJOINT_FORM(MODE, true); } else { RF_VAR_LAUNCH_ADJOINT_FORM(MODE, false); }
        if (a.mode == VAR_CAUSAL) { RF_VAR_LAUNCH_ADJOINT(VAR_CAUSAL); } else { RF_VAR_LAUNCH_ADJOINT(VAR_ANTICAUSAL); }
#undef RF_VAR_LAUNCH_ADJOINT
#undef RF_VAR_LAUNCH_ADJOINT_FORM
        return launched(what);
    }
    // byte planes (rf_smooth_plan): the instances that exist, and nothing else -- there is no conversion to fall back on
    if (a.src_u8 || a.dst_u8) {
        const std::string name = std::string(FINAL ? "var_pass2_" : "var_tails_") + axis;
        const char *what = name.c_str();
        const bool x_src = dim == 0 && a.src_u8 && !a.dst_u8, y_dst = dim == 1 && FINAL && a.dst_u8 && !a.src_u8;
        if (a.mode != VAR_PAIR || !a.power || !(x_src || y_dst)) {
            set_error("%s: no kernel for byte planes here (source %s, destination %s)", what, a.src_u8 ? "uint8" : "f32", a.dst_u8 ? "uint8" : "f32");
            return RF_ERR_UNSUPPORTED;
        }
        if (x_src) hipLaunchKernelGGL((var_x_kernel<VAR_PAIR, FINAL, true, uint8_t>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var_y_kernel<VAR_PAIR, true, true, uint8_t>), grid, block, 0, stream, a);
        return launched(what);
    }
#define RF_VAR_LAUNCH_FORM(MODE, POWER)                                                                   \
    if (dim == 0) hipLaunchKernelGGL((var_x_kernel<MODE, FINAL, POWER>), grid, block, 0, stream, a);      \
    else hipLaunchKernelGGL((var_y_kernel<MODE, FINAL, POWER>), grid, block, 0, stream, a)
#define RF_VAR_LAUNCH(MODE)                                                                               \
    if (a.power) { RF_VAR_LAUNCH_FORM(MODE, true); } else { RF_VAR_LAUNCH_FORM(MODE, false); }
    switch (a.mode) {
        case VAR_CAUSAL: RF_VAR_LAUNCH(VAR_CAUSAL); break;
        case VAR_ANTICAUSAL: RF_VAR_LAUNCH(VAR_ANTICAUSAL); break;
        default: RF_VAR_LAUNCH(VAR_PAIR); break;
    }
#undef RF_VAR_LAUNCH
#undef RF_VAR_LAUNCH_FORM
    return launched((std::string(FINAL ? "var_pass2_" : "var_tails_") + axis).c_str());
}

}  // namespace

int launch_var_tails(const VarArgs &a, int dim, hipStream_t stream) { return launch_pass<false>(a, dim, stream); }
int launch_var_pass2(const VarArgs &a, int dim, hipStream_t stream) { return launch_pass<true>(a, dim, stream); }

int launch_var_carry(const VarArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.lines + 255) / 256), (unsigned)a.n_planes, (unsigned)a.batch), block(256);
    switch (a.mode) {
        case VAR_CAUSAL: hipLaunchKernelGGL((var_carry_kernel<VAR_CAUSAL>), grid, block, 0, stream, a); break;
        case VAR_ANTICAUSAL: hipLaunchKernelGGL((var_carry_kernel<VAR_ANTICAUSAL>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((var_carry_kernel<VAR_PAIR>), grid, block, 0, stream, a); break;
    }
    return launched("var_carry");
}

int launch_var_distances(const VarDistArgs &a, bool guide_u8, hipStream_t stream) {
    const dim3 grid((unsigned)((a.width / 4 + 255) / 256), (unsigned)std::min(a.height, 65535), (unsigned)a.batch), block(256);
    if (guide_u8) hipLaunchKernelGGL((var_distances_kernel<uint8_t>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var_distances_kernel<float>), grid, block, 0, stream, a);
    return launched("var_distances");
}

int launch_var_distances_volume(const VarDistVolumeArgs &a, bool guide_u8, hipStream_t stream) {
    const int64_t lanes = (int64_t)(a.width / 4) * a.height;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)((a.depth + kVarDistSlices - 1) / kVarDistSlices)), block(256);
#define RF_VAR_LAUNCH_DISTANCES(NG)                                                                                    \
    if (guide_u8) hipLaunchKernelGGL((var_distances_volume_kernel<uint8_t, NG>), grid, block, 0, stream, a);            \
    else hipLaunchKernelGGL((var_distances_volume_kernel<float, NG>), grid, block, 0, stream, a)
    if (a.n_guide <= 1) { RF_VAR_LAUNCH_DISTANCES(1); }
    else if (a.n_guide <= 4) { RF_VAR_LAUNCH_DISTANCES(4); }
    else { RF_VAR_LAUNCH_DISTANCES(RF_MAX_PLANES); }
#undef RF_VAR_LAUNCH_DISTANCES
    return launched("var_distances_volume");
}

// dim 2 (a z stage of a volume plan): the dim 1 instances on the view the arguments describe
int launch_var_grad(const VarGradArgs &a, int dim, bool causal, hipStream_t stream) {
    const char *const what = dim == 0 ? "var_grad_x" : dim == 1 ? "var_grad_y" : "var_grad_z";
    if (dim == 2) dim = 1;
    // the base-reducing form walks at most kVarReduceRows rows at once: fewer, larger slabs for var_param_sum
    const dim3 grid((unsigned)((a.width / 4 + 255) / 256), (unsigned)std::min(a.height, a.slabs ? kVarReduceRows : 65535), (unsigned)a.batch), block(256);
#define RF_VAR_LAUNCH_GRAD(POWER, BASES)                                                                            \
    if (dim == 0) {                                                                                                 \
        if (causal) hipLaunchKernelGGL((var_grad_kernel<0, true, POWER, BASES>), grid, block, 0, stream, a);        \
        else hipLaunchKernelGGL((var_grad_kernel<0, false, POWER, BASES>), grid, block, 0, stream, a);              \
    } else {                                                                                                        \
        if (causal) hipLaunchKernelGGL((var_grad_kernel<1, true, POWER, BASES>), grid, block, 0, stream, a);        \
        else hipLaunchKernelGGL((var_grad_kernel<1, false, POWER, BASES>), grid, block, 0, stream, a);              \
    }
    if (a.slabs) {                                   // the base-reducing form: POWER instances only
        if (!a.exponents) { set_error("%s: the base gradient needs the exponent plane", what); return RF_ERR_INVALID_ARG; }
        RF_VAR_LAUNCH_GRAD(true, true)
    } else if (a.exponents) { RF_VAR_LAUNCH_GRAD(true, false) } else { RF_VAR_LAUNCH_GRAD(false, false) }
#undef RF_VAR_LAUNCH_GRAD
    return launched(what);
}

int64_t var_grad_blocks(int32_t width, int32_t height, int32_t batch) {
    return (int64_t)((width / 4 + 255) / 256) * std::min(height, kVarReduceRows) * batch;
}

int64_t var_dot_blocks(int64_t n) { return std::min<int64_t>((n / 4 + 255) / 256, kDotMaxBlocks); }

int launch_var_dot(const VarDotArgs &a, hipStream_t stream) {
    if (a.n_pairs < 1 || a.n_pairs > 3 || a.n < 4 || a.n % 4 != 0) { set_error("var_dot: bad arguments"); return RF_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(var_dot_kernel, dim3((unsigned)var_dot_blocks(a.n)), dim3(256), 0, stream, a);
    return launched("var_dot");
}

int launch_var_param_sum(const VarParamSumArgs &a, hipStream_t stream) {
    if (a.n_out < 1 || a.n_out > kVarParamOutputs || a.n_segments < 0 || a.n_segments > kVarParamSegments) {
        set_error("var_param_sum: bad argument counts");
        return RF_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(var_param_sum_kernel, dim3(1), dim3(kParamSumThreads), 0, stream, a);
    return launched("var_param_sum");
}

int launch_var_distances_grad(const VarDistGradArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.width / 4 + 255) / 256), (unsigned)std::min(a.height, 65535), (unsigned)a.batch), block(256);
    hipLaunchKernelGGL(var_distances_grad_kernel, grid, block, 0, stream, a);
    return launched("var_distances_grad");
}

int launch_var_distances_volume_grad(const VarDistVolumeGradArgs &a, hipStream_t stream) {
    const int64_t lanes = (int64_t)(a.width / 4) * a.height;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)((a.depth + kVarDistSlices - 1) / kVarDistSlices)), block(256);
    // one guide volume: the rolling window reads every volume once; more: gdx, gdy, gdz once for all channels (each form forced on
    // every case: profiles/r27/smooth_volume_grad.txt)
    if (a.n_guide == 1) hipLaunchKernelGGL(var_distances_volume_grad_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(var_distances_volume_grad_kernel<false>, grid, block, 0, stream, a);
    return launched("var_distances_volume_grad");
}

}  // namespace rf
