// kernels_var.h -- launchers of the spatially varying first-order scans (kernels_var.hip; plan_var.cpp drives them).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rf_internal.h"

namespace rf {

constexpr int kVarTile = 64;        // samples of a tile along the scanned dimension
constexpr int kVarComponents = 5;   // tail slots per tile and line: E1, P1, E2, G, P2
enum VarComponent { VAR_E1 = 0, VAR_P1 = 1, VAR_E2 = 2, VAR_G = 3, VAR_P2 = 4 };
// what a stage runs: one causal scan, one anticausal scan, or a causal scan directly followed by the anticausal one
enum VarMode { VAR_CAUSAL = 0, VAR_ANTICAUSAL = 1, VAR_PAIR = 2 };

// One stage on all planes of an image.  `lines` lines of `n` samples along the scanned dimension, `tiles` tiles of kVarTile.
//   tails [tile][component][plane][line]   E1 / E2 per image plane; P1 / G / P2 depend on the weights alone: plane 0 holds them
//   carry [tile][c, d][plane][line]        what enters tile `tile` from the left (c) and from the right (d)
struct VarArgs {
    const void *src[RF_MAX_PLANES];     // f32 planes, or bytes (src_u8)
    void *dst[RF_MAX_PLANES];           // what the final pass stores: f32 planes, or bytes (dst_u8)
    const float *weights;
    float *tails;
    float *carry;
    int32_t width, height;          // x fastest
    int32_t n_planes;
    int32_t tiles;
    int32_t lines;
    int32_t mode;                   // VarMode
    // power form (rf_var_plan_execute_power): `weights` holds exponents d, the kernels form w = exp2(d * log2_base) as they load
    int32_t power;
    float log2_base;
    // byte planes (rf_smooth_plan; the pair mode in the power form only): the source of a stage along x, the destination of a final
    // pass along y.  Separate kernel instances, chosen by the launchers; the f32 instances never look at these.
    int32_t src_u8, dst_u8;
    // adjoint stages (rf_var_plan_backward, rf_var_plan_backward_power; single scans, f32 only): `mode` is the direction of the ADJOINT recurrence
    // (VAR_ANTICAUSAL: the adjoint of a causal scan), which has unit input gain; the final pass stores (1 - w~) * lam to dst and,
    // where lam[pl] is not null, the unscaled lam to it.  The other instances never look at these.
    int32_t adjoint;
    void *lam[RF_MAX_PLANES];
    // the batch (rf_smooth_plan_create_batched): `batch` images per launch on gridDim.z = batch * n_planes.  The pointers above name
    // image 0's planes; image b's are `stride` SAMPLES further per b (0 with batch 1), its weight plane weights_stride floats, its
    // tails and carries -- one image's worth each, in the layout above -- tails_stride / carry_stride floats.
    int32_t batch;
    int64_t src_stride, dst_stride, lam_stride, weights_stride, tails_stride, carry_stride;
};

// The weight gradient of ONE scan (kernels_var.hip, var_grad): lam = that scan's adjoint state, x / y = its saved input and output.
//   causal      grad[i] = sum_planes lam[i]   * (y[i-1] - x[i])        anticausal  grad[i] = sum_planes lam[i-1] * (y[i] - x[i-1])
// along `dim`, planes summed in index order in f32; element 0 along the scanned dimension is 0.  accumulate: added to what `grad`
// holds (a later scan on the same weight plane), else stored.
struct VarGradArgs {
    const float *lam[RF_MAX_PLANES];
    const float *x[RF_MAX_PLANES];
    const float *y[RF_MAX_PLANES];
    float *grad;
    int32_t width, height;          // x fastest; the width is a multiple of 4
    int32_t n_planes;
    int32_t accumulate;
    // the gradient of an EXPONENT plane (rf_var_plan_backward_power): not null -> the sum above times w * ln_base,
    // w = exp2(exponents[i] * log2_base) as the scans form it
    const float *exponents;
    float log2_base, ln_base;
    // the batch, on gridDim.z: image b's planes are these strides (samples) behind image 0's
    int32_t batch;
    int64_t lam_stride, x_stride, y_stride, grad_stride, exponents_stride;
    // the base-reducing form (rf_var_plan_backward_power_bases; exponents != nullptr): not null -> every workgroup also stores
    //   slabs[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sum over its samples of (w == 0 ? 0 : d * w * dL/dw)
    // in f64, var_grad_blocks(a) entries in all; `grad` may then be null (nothing is stored to it).  Only these instances look at it.
    double *slabs;
};
// the workgroups of a base-reducing var_grad launch, whose grid walks at most kVarReduceRows rows at once (the rest in the stride
// loop): the slab entries it writes
constexpr int kVarReduceRows = 1024;
int64_t var_grad_blocks(int32_t width, int32_t height, int32_t batch);

// var_dot (rf_smooth_plan_backward_sigmas): one streaming launch over up to three pairs (gd, d) of dense f32 arrays of n samples (a
// multiple of 4; the images of a batch lie one behind the other).  Workgroup w of var_dot_blocks(n) stores, per pair p, in f64,
//   slabs[(2 * p) * blocks + w]     = its share of sum gd * (d - d0[p])      (gd == 0: the term is 0 by a select, whatever d holds)
//   slabs[(2 * p + 1) * blocks + w] = its share of sum gd
// lanes in the order of their grid-stride walk, the workgroup by var_grad's fixed tree.  No atomics.
struct VarDotArgs {
    const float *gd[3], *d[3];
    float d0[3];
    int32_t n_pairs;
    int64_t n;
    double *slabs;
};
int64_t var_dot_blocks(int64_t n);
int launch_var_dot(const VarDotArgs &a, hipStream_t stream);

// var_param_sum, one workgroup: with S_s = slabs[offset[s]] + ... + slabs[offset[s] + count[s] - 1], summed lane-strided and then by
// a fixed tree in f64,  out[j] = sum over the segments s, in index order, of (target[s] == j ? factor[s] * S_s : 0) +
// (target2[s] == j ? factor2[s] * S_s : 0);  target2 < 0: none.  An out entry no segment names is stored as 0.  No atomics: two runs
// agree bit for bit.
constexpr int kVarParamSegments = 64, kVarParamOutputs = 16;
struct VarParamSumArgs {
    const double *slabs;
    double *out;
    int32_t n_out;                  // at most kVarParamOutputs
    int32_t n_segments;             // at most kVarParamSegments
    int64_t offset[kVarParamSegments], count[kVarParamSegments];
    int32_t target[kVarParamSegments], target2[kVarParamSegments];
    double factor[kVarParamSegments], factor2[kVarParamSegments];
};
int launch_var_param_sum(const VarParamSumArgs &a, hipStream_t stream);

// d_x = 1 + scale * sum_ch |g - g one column to the left|, d_y the same with the row above (kernels_var.hip, var_distances)
struct VarDistArgs {
    const void *guide[RF_MAX_PLANES];
    float *dx, *dy;
    int32_t width, height;          // x fastest; the width is a multiple of 4
    int32_t n_guide;
    float scale;
    // the batch, on gridDim.z: image b's guide planes are guide_stride samples behind image 0's; dx and dy hold `batch` dense planes
    int32_t batch;
    int64_t guide_stride;
};

// The three exponent volumes of a guide volume [z][y][x] (kernels_var.hip, var_distances_volume): d_x and d_y slice by slice as
// var_distances forms them, d_z = spacing_z + scale * sum_ch |g - g one slice before| (slice 0: spacing_z).  One launch: a lane owns
// four adjacent columns of one row and walks kVarDistSlices slices with the slice before in registers.
constexpr int kVarDistSlices = 16;
struct VarDistVolumeArgs {
    const void *guide[RF_MAX_PLANES];
    float *dx, *dy, *dz;
    int32_t width, height, depth;   // x fastest; the width is a multiple of 4
    int32_t n_guide;
    float scale, spacing_z;
};

// The adjoint of var_distances (kernels_var.hip, var_distances_grad), f32 guides:
//   grad_guide[ch][r][c] = scale * (sx(r,c) gdx[r][c] - sx(r,c+1) gdx[r][c+1] + sy(r,c) gdy[r][c] - sy(r+1,c) gdy[r+1][c])
// sx / sy: the sign of the guide's difference to the left / above (0 for a difference of 0 and outside the plane).  accumulate:
// added to what the planes hold, else stored.
struct VarDistGradArgs {
    const float *guide[RF_MAX_PLANES];
    float *grad_guide[RF_MAX_PLANES];
    const float *gdx, *gdy;
    int32_t width, height;          // x fastest; the width is a multiple of 4
    int32_t n_guide;
    int32_t accumulate;
    float scale;
    // the batch, on gridDim.z: strides in samples per image; gdx and gdy hold `batch` dense planes
    int32_t batch;
    int64_t guide_stride, grad_guide_stride;
};

// The adjoint of var_distances_volume (kernels_var.hip, var_distances_volume_grad), f32 guides: per channel, the six terms in this
// order,
//   grad_guide[ch][z][r][c] = scale * (((((L - R) + U) - Dn) + B) - A)
//   L = sx(z,r,c) gdx[z][r][c]   R = sx(z,r,c+1) gdx[z][r][c+1]   U = sy(z,r,c) gdy[z][r][c]   Dn = sy(z,r+1,c) gdy[z][r+1][c]
//   B = sz(z,r,c) gdz[z][r][c]   A = sz(z+1,r,c) gdz[z+1][r][c]
// sx / sy / sz: the sign of the guide's difference to the left / above / one slice before (0 for a difference of 0 and outside
// the volume).  spacing_z is an additive constant of d_z and does not enter.  accumulate: added to what the volumes hold, else
// stored.  The grid is var_distances_volume's: a lane owns four adjacent columns of one row and walks kVarDistSlices slices.
struct VarDistVolumeGradArgs {
    const float *guide[RF_MAX_PLANES];
    float *grad_guide[RF_MAX_PLANES];
    const float *gdx, *gdy, *gdz;
    int32_t width, height, depth;   // x fastest; the width is a multiple of 4
    int32_t n_guide;
    int32_t accumulate;
    float scale;
};

// dim 2 (a z stage of a volume plan, plan_var.cpp): the y kernels on the view the arguments describe -- width = lines = the voxel
// columns, height = the depth -- under the names "var_*_z"
int launch_var_tails(const VarArgs &a, int dim, hipStream_t stream);
int launch_var_carry(const VarArgs &a, hipStream_t stream);
int launch_var_pass2(const VarArgs &a, int dim, hipStream_t stream);
// One long line (kernels_var_signal.hip; rf_var_plan_create_signal): width = the signal's length, height = lines = 1, tiles =
// ceil(width / kVarTile); 64 tiles are a group.  tails: 5 * n_planes * (tiles + groups) floats, carry: 2 * n_planes * groups (the
// layouts: kernels_var_signal.hip).  f32, batch 1; no byte planes.
constexpr int kVarGroupTiles = 64;
int launch_var_signal_tails(const VarArgs &a, hipStream_t stream);
int launch_var_signal_carry(const VarArgs &a, hipStream_t stream);
int launch_var_signal_pass2(const VarArgs &a, hipStream_t stream);
int launch_var_distances(const VarDistArgs &a, bool guide_u8, hipStream_t stream);
int launch_var_distances_volume(const VarDistVolumeArgs &a, bool guide_u8, hipStream_t stream);
int launch_var_grad(const VarGradArgs &a, int dim, bool causal, hipStream_t stream);
int launch_var_distances_grad(const VarDistGradArgs &a, hipStream_t stream);
int launch_var_distances_volume_grad(const VarDistVolumeGradArgs &a, hipStream_t stream);

}  // namespace rf
