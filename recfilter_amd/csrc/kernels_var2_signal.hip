// kernels_var2_signal.hip -- time-varying second-order all-pole scans on dense f32 signals (rf_var2_plan_*):
//   causal      y[n] = x[n] - a1~[n] y[n-1] - a2~[n] y[n-2]          anticausal: the same on the three signals reversed
// with a coefficient that would multiply a sample outside the line selected to 0 (a~).  N a multiple of 4 up to 2^30; every line
// has its own coefficient signals; lines ride on gridDim.y.
//
// The tiling is kernels_var_signal.hip's with a 2-vector where that file has a scalar.  The state behind sample n is
// s[n] = (y[n], y[n-1]),  s[n] = M[n] s[n-1] + (x[n], 0),  M[n] = [[-a1~[n], -a2~[n]], [1, 0]].  A lane owns a TILE of 64
// consecutive samples and forms six numbers: E, the state behind the tile from zero entry, and P = M[t1-1] ... M[t0], from two more
// recurrences started at (1, 0) and (0, 1) in the same sweep.  For a sub-line A followed by B
//   E = E_B + P_B E_A          P = P_B P_A                    identity (0, I)
// A workgroup of one wave owns a GROUP of 64 tiles, 4096 contiguous samples.
//
//   var2_tails_1d   tile tails per lane, then a Kogge-Stone scan of (E, P) across the 64 lanes with __shfl_up (an anticausal scan:
//                   __shfl_down, the lanes taken from the right).  A lane stores the map from the state that enters its group to the
//                   state that enters its tile, one lane the group's aggregate.
//   var2_carry_1d   the recurrence over GROUPS: one workgroup per line, up to 1024 lanes, sweeping the groups 1024 at a time in the
//                   order of the recurrence -- a wave scan, the waves' totals folded through LDS, the running 2-vector kept in
//                   registers between sweeps.
//   var2_pass2_1d   reloads the group, forms the state that enters each tile from the stored map and the group's carry, RERUNS the
//                   recurrence from it and stores.  Nothing is superposed: coefficients of exactly 0 give out == in.
// No kernel waits on another workgroup, there are no atomics, every sum has a fixed order: results are reproducible bit for bit.
//
// The loads are var_tails_1d's -- a wave instruction moves 1024 contiguous bytes, the chunks go through LDS to the lanes' tiles
// (transpose_in, var_device.h) -- for three signals.  request_tile of that header clamps rows and columns of a 2-D plane apart: on a
// line whose length is no multiple of 64 it would read past the end, so the request here clamps the flat address.  Samples past
// the end come from a clamped address inside the line and are selected away (input 0, coefficients 0): such a sample leaves the
// state (0, 0) behind it after two steps and passes nothing on.  A workgroup has loaded its whole group before it stores: in == out
// is legal.
//
// The adjoint of a causal scan is  lam[n] = g[n] - a1~[n+1] lam[n+1] - a2~[n+2] lam[n+2]:  an anticausal scan whose coefficients are
// read one (a1) and two (a2) samples further on.  The ADJ instances form them from the tile's own coefficients and the first three
// of the neighbouring tile (a1[t1], a2[t1], a2[t1+1]; the 65th weight of the first-order kernels), loaded from clamped addresses;
// the masks by position are those of the scan's own direction.  The adjoint of an anticausal scan is the mirror image.
//
// The direct-form-I section (rf_var2_plan_execute_biquad): v[n] = b0[n] x[n] + b1~[n] x[n-1] + b2~[n] x[n-2] in front of the scan.
//   var2_biquad_tails_1d   the FF instance of the tails stage: the lane forms v over its tile in registers (feed_forward: the
//                          six signals one at a time through the transposition), stores v to `out` and runs the tails on it;
//                          var2_carry_1d and var2_pass2_1d then run on out, in place.  Neighbouring groups read x while this one
//                          stores v: out overlaps no input.
//   var2_biquad_grad_1d    behind the adjoint scan (lam in a signal of the plan's): grad_in and, where asked for, the five
//                          coefficient gradients, pointwise in lam, x, y and the taps with neighbours from clamped addresses.
//
// A cascade of K sections in one plan (rf_var2_plan_execute_cascade): section k + 1 reads what section k stores, and the two
// samples its feed-forward taps reach beyond a tile are the state that enters the tile in section k's final stage.
//   var2_link_1d           one launch per boundary between sections: the final stage of section k as var2_pass2_1d runs it (y_k of
//                          the tile in registers), the feed-forward part of section k + 1 on y_k with the tile's entering state
//                          (y1, y2) for the near and the far sample beyond the tile, v_{k+1} stored -- in place: no workgroup reads
//                          another's samples -- and the tails of section k + 1 on it, into the slots the workgroup has just read.
//   var2_link_keep_1d      the same with y_k stored too (the backward's rerun of the forward keeps every section's output; so
//                          does rf_var2_plan_execute_cascade_keep, into signals of the caller's).
//
// The backward of a cascade whose forward kept every section's result (rf_var2_plan_backward_cascade_kept) mirrors the link: the
// gradient that enters section k - 1 is the transposed feed-forward part of section k on lam_k, and the two samples of lam_k its
// taps reach beyond a tile are the state that enters the tile in the adjoint scan's final stage.
//   var2_adj_link_1d       one launch per boundary: the final stage of section k's adjoint scan as var2_adj_pass2_1d runs it (lam_k
//                          of the tile in registers), g_{k-1} = fma(b2~ two along, lam_k two along, fma(b1~ one along, lam_k one
//                          along, b0 lam_k)) stored -- in place -- and the adjoint tails of section k - 1 on it.
//   var2_adj_link_keep_1d  the same with lam_k stored too, for
//   var2_biquad_coef_1d    the five coefficient gradients of a section from lam, x and y: the COEF half of var2_biquad_grad_1d.
//
// The section with its coefficients as control-rate frames (rf_var2_plan_execute_biquad_frames): frame j of a coefficient at sample
// j * hop, hop a power of two >= 64, linear interpolation in registers -- no coefficient signal is read.
//   var2_expand_frames_1d          c[n] of one coefficient at audio rate: what the kernels below form, bit for bit
//   var2_biquad_frames_tails_1d    var2_biquad_tails_1d reading x and the frames; var2_frames_pass2_1d, var2_adj_frames_tails_1d and
//                                  var2_adj_frames_pass2_1d are the other stages (var2_frames_kernel); var2_carry_1d serves unchanged
//   var2_biquad_frames_grad_1d     grad_in as var2_biquad_grad_1d forms it and, where asked for, that kernel's five per-sample
//                                  gradients contracted in f64 with the interpolation's transpose, per piece of min(hop, 1024)
//                                  samples, into a slab of the plan's
//   var2_frames_fold_1d            the pieces that meet at a frame added in order, rounded once: the five frame gradients
//
// A cascade on frames (rf_var2_plan_execute_cascade_frames): the link kernels with every coefficient formed as above.
//   var2_frames_link_1d            var2_link_1d reading x and seven frame pairs (var2_frames_link_keep_1d: y_k stored too)
//   var2_adj_frames_link_1d        var2_adj_link_1d likewise, the shifted coefficients as var2_adj_frames_tails_1d reads them
//                                  (var2_adj_frames_link_keep_1d: lam_k stored too), for
//   var2_frames_coef_1d            the sums of a section's five frame gradients from lam, x and y: var2_biquad_frames_grad_1d
//                                  without grad_in, into the section's part of the slab
//   var2_frames_fold_cascade_1d    var2_frames_fold_1d for all sections in one launch, the section on gridDim.z
//
// The cascade on frames with a state that enters and leaves the call (rf_var2_plan_execute_cascade_frames_stream): the STREAM
// instances of the forward stages -- var2_biquad_frames_tails_stream_1d, var2_frames_link_stream_1d,
// var2_frames_link_keep_stream_1d, var2_frames_pass2_stream_1d; var2_carry_1d serves unchanged.  The lane whose tile holds the
// line's two first samples in the order of the recurrence folds the entering state into them (fold_entering_state); the lane
// whose tile holds the two last stores the leaving pair from its registers (store_leaving_pair).  O(1) more work per line.
#include "kernels_var2.h"

#include "var_device.h"

#include <algorithm>

namespace rf {

namespace {

static_assert(kVar2Tile == T, "the tile of var_device.h");
constexpr int kGroupTiles = kVar2GroupTiles;       // tiles of a group: one per lane
constexpr int kGroupSamples = kGroupTiles * T;     // 4096
constexpr int kCarryLanes = 1024;                  // groups of a sweep of var2_carry_1d
constexpr int kGradLanes = 256;                    // lanes of a workgroup of var2_grad_1d, four samples each

__device__ __forceinline__ int64_t map_index(const Var2Args &a, int comp, int line, int t) { return ((int64_t)comp * a.n_lines + line) * a.tiles + t; }
__device__ __forceinline__ int64_t map_index_of(int n_lines, int tiles, int comp, int line, int t) { return ((int64_t)comp * n_lines + line) * tiles + t; }
__device__ __forceinline__ int64_t aggregate_index(const Var2Args &a, int comp, int line, int g) {
    return (int64_t)kVar2Components * a.n_lines * a.tiles + ((int64_t)comp * a.n_lines + line) * a.groups + g;
}
__device__ __forceinline__ int64_t group_carry_index(const Var2Args &a, int comp, int line, int g) { return ((int64_t)comp * a.n_lines + line) * a.groups + g; }

// one step of the recurrence: the new y from the two before it
__device__ __forceinline__ float step2(float c1, float c2, float x, float y1, float y2) { return __builtin_fmaf(-c1, y1, __builtin_fmaf(-c2, y2, x)); }

// sub-line A followed by B
__device__ __forceinline__ void compose(const float (&A)[kVar2Components], const float (&B)[kVar2Components], float (&r)[kVar2Components]) {
    r[VAR2_E0] = __builtin_fmaf(B[VAR2_P00], A[VAR2_E0], __builtin_fmaf(B[VAR2_P01], A[VAR2_E1], B[VAR2_E0]));
    r[VAR2_E1] = __builtin_fmaf(B[VAR2_P10], A[VAR2_E0], __builtin_fmaf(B[VAR2_P11], A[VAR2_E1], B[VAR2_E1]));
    r[VAR2_P00] = __builtin_fmaf(B[VAR2_P00], A[VAR2_P00], B[VAR2_P01] * A[VAR2_P10]);
    r[VAR2_P01] = __builtin_fmaf(B[VAR2_P00], A[VAR2_P01], B[VAR2_P01] * A[VAR2_P11]);
    r[VAR2_P10] = __builtin_fmaf(B[VAR2_P10], A[VAR2_P00], B[VAR2_P11] * A[VAR2_P10]);
    r[VAR2_P11] = __builtin_fmaf(B[VAR2_P10], A[VAR2_P01], B[VAR2_P11] * A[VAR2_P11]);
}

__device__ __forceinline__ void identity(float (&r)[kVar2Components]) {
    r[VAR2_E0] = 0.0f; r[VAR2_E1] = 0.0f; r[VAR2_P00] = 1.0f; r[VAR2_P01] = 0.0f; r[VAR2_P10] = 0.0f; r[VAR2_P11] = 1.0f;
}

// the map m applied to the state (s0, s1)
__device__ __forceinline__ void apply_map(const float (&m)[kVar2Components], float s0, float s1, float &r0, float &r1) {
    r0 = __builtin_fmaf(m[VAR2_P00], s0, __builtin_fmaf(m[VAR2_P01], s1, m[VAR2_E0]));
    r1 = __builtin_fmaf(m[VAR2_P10], s0, __builtin_fmaf(m[VAR2_P11], s1, m[VAR2_E1]));
}

// the value of the lane k places earlier in the order of the recurrence
template <bool REV>
__device__ __forceinline__ float from_before(float v, int k) { return REV ? __shfl_down(v, k) : __shfl_up(v, k); }

// From a lane's tile tails to its map and the group's aggregate.  pos: the lane's place in the order of the recurrence.
//   map: the inclusive scan of the lane before (the identity at place 0);   whole: valid at place 63
template <bool REV>
__device__ __forceinline__ void scan_group(const float (&own)[kVar2Components], float (&map)[kVar2Components], float (&whole)[kVar2Components]) {
    const int lane = threadIdx.x, pos = REV ? 63 - lane : lane;
    float other[kVar2Components], next[kVar2Components];
#pragma unroll
    for (int i = 0; i < kVar2Components; i++) whole[i] = own[i];
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) other[i] = from_before<REV>(whole[i], k);
        compose(other, whole, next);
        if (pos >= k) {
#pragma unroll
            for (int i = 0; i < kVar2Components; i++) whole[i] = next[i];
        }
    }
#pragma unroll
    for (int i = 0; i < kVar2Components; i++) other[i] = from_before<REV>(whole[i], 1);
    identity(map);
    if (pos > 0) {
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) map[i] = other[i];
    }
}

// request k of a lane: the 16-byte chunk k * 64 + lane of the group, from a flat address clamped into the line
__device__ __forceinline__ void request_group(const float *signal, int n, int s0, float (&v)[T]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < T / 4; k++) {
        const int at = min(s0 + (k * 64 + lane) * 4, n - 4);      // (n is a multiple of 4, at least 4)
        const float4 q = *reinterpret_cast<const float4 *>(signal + at);
        v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
    }
}

// the lanes' tiles back through LDS to the group's chunks; a chunk is inside the line or beyond it (n is a multiple of 4)
__device__ __forceinline__ void store_group(float *lds, float *signal, int n, int s0, const float (&y)[T]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < T / 4; k++)
        *reinterpret_cast<float4 *>(lds + lane * LDS_PITCH + k * 4) = make_float4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < T / 4; k++) {
        const int flat = k * 64 + lane;
        const int at = s0 + flat * 4;
        const float4 q = *reinterpret_cast<const float4 *>(lds + (flat >> 4) * LDS_PITCH + (flat & 15) * 4);
        if (at < n) *reinterpret_cast<float4 *>(signal + at) = q;
    }
}

// The feed-forward part of a direct-form-I section over the lane's tile (var2_biquad_tails_1d):
//   v[i] = fma(b2~, x two samples before, fma(b1~, x one sample before, b0 * x[i]))          (REV: the samples after)
// The signals come through the transposition one at a time -- x, then b0, b1, b2, each accumulated into v -- so three tiles are
// live at most.  The two samples of x beyond the tile come from clamped addresses and are selected to 0 outside the line; the
// taps are masked by position like the feedback coefficients, and everything from n on is 0: v is 0 there.
template <bool REV>
__device__ __forceinline__ void feed_forward(const Var2Args &a, float *lds, int64_t first, int n, int s0, int t0, float (&v)[T]) {
    const float *px = a.x + first;
    float raw[T], x[T], b[T];
    request_group(px, n, s0, raw);
    const int near = REV ? t0 + T : t0 - 1, far = REV ? t0 + T + 1 : t0 - 2;
    float x_near = px[max(min(near, n - 1), 0)], x_far = px[max(min(far, n - 1), 0)];
    x_near = (near < 0 || near >= n) ? 0.0f : x_near;
    x_far = (far < 0 || far >= n) ? 0.0f : x_far;
    transpose_in(raw, lds, x);
#pragma unroll
    for (int i = 0; i < T; i++) x[i] = t0 + i < n ? x[i] : 0.0f;
    request_group(a.b0 + first, n, s0, raw);
    transpose_in(raw, lds, b);
#pragma unroll
    for (int i = 0; i < T; i++) v[i] = (t0 + i < n ? b[i] : 0.0f) * x[i];
    request_group(a.b1 + first, n, s0, raw);
    transpose_in(raw, lds, b);
#pragma unroll
    for (int i = 0; i < T; i++) {
        const int at = t0 + i;
        const float one = REV ? (i + 1 < T ? x[i + 1 < T ? i + 1 : 0] : x_near) : (i >= 1 ? x[i >= 1 ? i - 1 : 0] : x_near);
        const bool masked = REV ? at >= n - 1 : (at < 1 || at >= n);
        v[i] = __builtin_fmaf(masked ? 0.0f : b[i], one, v[i]);
    }
    request_group(a.b2 + first, n, s0, raw);
    transpose_in(raw, lds, b);
#pragma unroll
    for (int i = 0; i < T; i++) {
        const int at = t0 + i;
        const float two = REV ? (i + 2 < T ? x[i + 2 < T ? i + 2 : 0] : (i + 2 == T ? x_near : x_far))
                              : (i >= 2 ? x[i >= 2 ? i - 2 : 0] : (i == 1 ? x_near : x_far));
        const bool masked = REV ? at >= n - 2 : (at < 2 || at >= n);
        v[i] = __builtin_fmaf(masked ? 0.0f : b[i], two, v[i]);
    }
}

// REV: the recurrence runs from the line's end to its start.  ADJ: the shifted coefficients of an adjoint stage.  FF: the tails
// stage of a direct-form-I section -- the recurrences run on v = the feed-forward part of x, which is stored to dst.
template <bool REV, bool ADJ, bool FINAL, bool FF = false>
__global__ void __launch_bounds__(64) var2_signal_kernel(Var2Args a) {
    static_assert(!FF || (!ADJ && !FINAL), "the feed-forward part stands in front of a forward tails stage");
    __shared__ __attribute__((aligned(16))) float lds[T * LDS_PITCH];
    const int lane = threadIdx.x;
    const int g = blockIdx.x, line = blockIdx.y;
    const int n = a.n;
    const int s0 = g * kGroupSamples;                 // below 2^30 + 4096
    const int t = g * kGroupTiles + lane, t0 = t * T;
    const int64_t first = (int64_t)line * a.stride;
    const float *px = a.x + first, *p1 = a.a1 + first, *p2 = a.a2 + first;
    float vx[T], v1[T], v2[T];
    float x[T], c1[T], c2[T];
    if constexpr (FF) {
        feed_forward<REV>(a, lds, first, n, s0, t0, x);
        request_group(p1, n, s0, v1);
        request_group(p2, n, s0, v2);
        store_group(lds, a.dst + first, n, s0, x);      // v: what var2_pass2_1d reads, in place
    } else {
        request_group(px, n, s0, vx);
        request_group(p1, n, s0, v1);
        request_group(p2, n, s0, v2);
    }
    // an adjoint stage: the three coefficients of the neighbouring tile its shifted reads reach (clamped; masked below by position)
    float nb1 = 0.0f, nb2_near = 0.0f, nb2_far = 0.0f;
    if constexpr (ADJ) {
        const int near = REV ? t0 + T : t0 - 1, far = REV ? t0 + T + 1 : t0 - 2;
        const int at_near = max(min(near, n - 1), 0), at_far = max(min(far, n - 1), 0);
        nb1 = p1[at_near];
        nb2_near = p2[at_near];
        nb2_far = p2[at_far];
    }
    float y1 = 0.0f, y2 = 0.0f;                       // the state that enters the tile
    if constexpr (FINAL) {
        const int tt = min(t, a.tiles - 1);
        float m[kVar2Components];
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) m[i] = a.tails[map_index(a, i, line, tt)];
        apply_map(m, a.carry[group_carry_index(a, 0, line, g)], a.carry[group_carry_index(a, 1, line, g)], y1, y2);
    }
    if constexpr (!FF) transpose_in(vx, lds, x);
    {
        float r1[T], r2[T];
        transpose_in(v1, lds, r1);
        transpose_in(v2, lds, r2);
        // the coefficients of step i: the tile's own, or (ADJ) those one and two samples further along the forward's direction
#pragma unroll
        for (int i = 0; i < T; i++) {
            if constexpr (!ADJ) {
                c1[i] = r1[i];
                c2[i] = r2[i];
            } else if constexpr (REV) {
                c1[i] = i + 1 < T ? r1[i + 1 < T ? i + 1 : 0] : nb1;
                c2[i] = i + 2 < T ? r2[i + 2 < T ? i + 2 : 0] : (i + 2 == T ? nb2_near : nb2_far);
            } else {
                c1[i] = i >= 1 ? r1[i >= 1 ? i - 1 : 0] : nb1;
                c2[i] = i >= 2 ? r2[i >= 2 ? i - 2 : 0] : (i == 1 ? nb2_near : nb2_far);
            }
        }
    }
    // the masks, by position in the line: everything from n on, and the coefficients that would reach outside the line
#pragma unroll
    for (int i = 0; i < T; i++) {
        const int at = t0 + i;
        x[i] = at < n ? x[i] : 0.0f;
        if constexpr (REV) {
            c1[i] = at >= n - 1 ? 0.0f : c1[i];
            c2[i] = at >= n - 2 ? 0.0f : c2[i];
        } else {
            c1[i] = (at < 1 || at >= n) ? 0.0f : c1[i];
            c2[i] = (at < 2 || at >= n) ? 0.0f : c2[i];
        }
    }
    __builtin_amdgcn_sched_barrier(0);      // (the recurrences stay behind the transposition: they would hold its registers)
    if constexpr (FINAL) {
#pragma unroll
        for (int j = 0; j < T; j++) {
            const int i = REV ? T - 1 - j : j;
            const float y = step2(c1[i], c2[i], x[i], y1, y2);
            x[i] = y; y2 = y1; y1 = y;
        }
        store_group(lds, a.dst + first, n, s0, x);
    } else {
        float u1 = 1.0f, u2 = 0.0f, w1 = 0.0f, w2 = 1.0f;
#pragma unroll
        for (int j = 0; j < T; j++) {
            const int i = REV ? T - 1 - j : j;
            const float y = step2(c1[i], c2[i], x[i], y1, y2);
            const float u = step2(c1[i], c2[i], 0.0f, u1, u2);
            const float w = step2(c1[i], c2[i], 0.0f, w1, w2);
            y2 = y1; y1 = y; u2 = u1; u1 = u; w2 = w1; w1 = w;
        }
        float own[kVar2Components], map[kVar2Components], whole[kVar2Components];
        own[VAR2_E0] = y1; own[VAR2_E1] = y2;
        own[VAR2_P00] = u1; own[VAR2_P10] = u2;       // the column the state (1, 0) becomes
        own[VAR2_P01] = w1; own[VAR2_P11] = w2;       // and the column of (0, 1)
        scan_group<REV>(own, map, whole);
        if (t < a.tiles) {
#pragma unroll
            for (int i = 0; i < kVar2Components; i++) a.tails[map_index(a, i, line, t)] = map[i];
        }
        if (lane == (REV ? 0 : 63)) {
#pragma unroll
            for (int i = 0; i < kVar2Components; i++) a.tails[aggregate_index(a, i, line, g)] = whole[i];
        }
    }
}

// ---- the boundary between two sections of a cascade ---------------------------------------------------------------------------------
// The feed-forward part of the next section on y, the finished tile of this one: feed_forward's arithmetic, order and masks, with
// the two samples beyond the tile handed in (the state that entered the tile: it is 0 where they lie outside the line).
template <bool REV>
__device__ __forceinline__ void link_feed_forward(const Var2LinkArgs &a, float *lds, int64_t first, int n, int s0, int t0, const float (&y)[T],
                                                  float y_near, float y_far, float (&v)[T]) {
    float raw[T], b[T];
    request_group(a.next_b0 + first, n, s0, raw);
    transpose_in(raw, lds, b);
#pragma unroll
    for (int i = 0; i < T; i++) v[i] = (t0 + i < n ? b[i] : 0.0f) * y[i];
    request_group(a.next_b1 + first, n, s0, raw);
    transpose_in(raw, lds, b);
#pragma unroll
    for (int i = 0; i < T; i++) {
        const int at = t0 + i;
        const float one = REV ? (i + 1 < T ? y[i + 1 < T ? i + 1 : 0] : y_near) : (i >= 1 ? y[i >= 1 ? i - 1 : 0] : y_near);
        const bool masked = REV ? at >= n - 1 : (at < 1 || at >= n);
        v[i] = __builtin_fmaf(masked ? 0.0f : b[i], one, v[i]);
    }
    request_group(a.next_b2 + first, n, s0, raw);
    transpose_in(raw, lds, b);
#pragma unroll
    for (int i = 0; i < T; i++) {
        const int at = t0 + i;
        const float two = REV ? (i + 2 < T ? y[i + 2 < T ? i + 2 : 0] : (i + 2 == T ? y_near : y_far))
                              : (i >= 2 ? y[i >= 2 ? i - 2 : 0] : (i == 1 ? y_near : y_far));
        const bool masked = REV ? at >= n - 2 : (at < 2 || at >= n);
        v[i] = __builtin_fmaf(masked ? 0.0f : b[i], two, v[i]);
    }
}

// the feedback coefficients of a forward stage over the lane's tile, masked by position
template <bool REV>
__device__ __forceinline__ void feedback_tiles(const float (&v1)[T], const float (&v2)[T], float *lds, int n, int t0, float (&c1)[T], float (&c2)[T]) {
    transpose_in(v1, lds, c1);
    transpose_in(v2, lds, c2);
#pragma unroll
    for (int i = 0; i < T; i++) {
        const int at = t0 + i;
        if constexpr (REV) {
            c1[i] = at >= n - 1 ? 0.0f : c1[i];
            c2[i] = at >= n - 2 ? 0.0f : c2[i];
        } else {
            c1[i] = (at < 1 || at >= n) ? 0.0f : c1[i];
            c2[i] = (at < 2 || at >= n) ? 0.0f : c2[i];
        }
    }
}

// KEEP: y of the finished section is stored to a.keep (it may be a.x: the group has loaded all of it)
template <bool REV, bool KEEP>
__global__ void __launch_bounds__(64) var2_link_kernel(Var2LinkArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[T * LDS_PITCH];
    const int lane = threadIdx.x;
    const int g = blockIdx.x, line = blockIdx.y;
    const int n = a.n;
    const int s0 = g * kGroupSamples;                 // below 2^30 + 4096
    const int t = g * kGroupTiles + lane, t0 = t * T;
    const int64_t first = (int64_t)line * a.stride;
    float y[T], v[T];
    float y_near, y_far;
    // the final stage of the section behind the boundary: var2_pass2_1d's, y kept in registers
    {
        float vx[T], v1[T], v2[T], c1[T], c2[T];
        request_group(a.x + first, n, s0, vx);
        request_group(a.a1 + first, n, s0, v1);
        request_group(a.a2 + first, n, s0, v2);
        const int tt = min(t, a.tiles - 1);
        float m[kVar2Components], y1, y2;
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) m[i] = a.tails[map_index_of(a.n_lines, a.tiles, i, line, tt)];
        apply_map(m, a.carry[((int64_t)0 * a.n_lines + line) * a.groups + g], a.carry[((int64_t)1 * a.n_lines + line) * a.groups + g], y1, y2);
        y_near = y1; y_far = y2;                      // y one and two samples before the tile, in the order of the recurrence
        transpose_in(vx, lds, y);
        feedback_tiles<REV>(v1, v2, lds, n, t0, c1, c2);
#pragma unroll
        for (int i = 0; i < T; i++) y[i] = t0 + i < n ? y[i] : 0.0f;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < T; j++) {
            const int i = REV ? T - 1 - j : j;
            const float r = step2(c1[i], c2[i], y[i], y1, y2);
            y[i] = r; y2 = y1; y1 = r;
        }
    }
    if constexpr (KEEP) {
        store_group(lds, a.keep + first, n, s0, y);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < T; i++) y[i] = t0 + i < n ? y[i] : 0.0f;
    __builtin_amdgcn_sched_barrier(0);
    // the section in front of the boundary: its feed-forward part on y, then its tails stage
    link_feed_forward<REV>(a, lds, first, n, s0, t0, y, y_near, y_far, v);
    float v1[T], v2[T], c1[T], c2[T];
    request_group(a.next_a1 + first, n, s0, v1);
    request_group(a.next_a2 + first, n, s0, v2);
    store_group(lds, a.dst + first, n, s0, v);
    __syncthreads();
    feedback_tiles<REV>(v1, v2, lds, n, t0, c1, c2);
    __builtin_amdgcn_sched_barrier(0);
    float y1 = 0.0f, y2 = 0.0f, u1 = 1.0f, u2 = 0.0f, w1 = 0.0f, w2 = 1.0f;
#pragma unroll
    for (int j = 0; j < T; j++) {
        const int i = REV ? T - 1 - j : j;
        const float r = step2(c1[i], c2[i], v[i], y1, y2);
        const float u = step2(c1[i], c2[i], 0.0f, u1, u2);
        const float w = step2(c1[i], c2[i], 0.0f, w1, w2);
        y2 = y1; y1 = r; u2 = u1; u1 = u; w2 = w1; w1 = w;
    }
    float own[kVar2Components], map[kVar2Components], whole[kVar2Components];
    own[VAR2_E0] = y1; own[VAR2_E1] = y2;
    own[VAR2_P00] = u1; own[VAR2_P10] = u2;
    own[VAR2_P01] = w1; own[VAR2_P11] = w2;
    scan_group<REV>(own, map, whole);
    if (t < a.tiles) {
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) a.tails[map_index_of(a.n_lines, a.tiles, i, line, t)] = map[i];
    }
    if (lane == (REV ? 0 : 63)) {
#pragma unroll
        for (int i = 0; i < kVar2Components; i++)
            a.tails[(int64_t)kVar2Components * a.n_lines * a.tiles + ((int64_t)i * a.n_lines + line) * a.groups + g] = whole[i];
    }
}

// ---- the boundary between two sections of a cascade, backward ------------------------------------------------------------------------
// One coefficient signal over the lane's tile as an adjoint stage reads it, from the tile as transposed: the values SHIFT samples
// further along the forward's direction (REV: toward the line's end) -- those beyond the tile handed in, read from clamped
// addresses -- then the mask by position of the scan's own direction.  The shifted feedback coefficients of var2_adj_tails_1d and
// the transposed taps of var2_biquad_grad_1d are both this: a tap that would multiply lam outside the line sits where the scan
// masks its coefficient.
template <bool REV, int SHIFT>
__device__ __forceinline__ void shift_and_mask(float (&c)[T], float beyond_near, float beyond_far, int n, int t0) {
#pragma unroll
    for (int j = 0; j < T; j++) {
        const int i = REV ? j : T - 1 - j;            // in place: a value is read before it is overwritten
        const int from = REV ? i + SHIFT : i - SHIFT;
        const bool inside = from >= 0 && from < T;
        const bool nearest = REV ? from == T : from == -1;
        c[i] = inside ? c[inside ? from : 0] : (nearest ? beyond_near : beyond_far);
    }
#pragma unroll
    for (int i = 0; i < T; i++) {
        const int at = t0 + i;
        c[i] = (REV ? at >= n - SHIFT : (at < SHIFT || at >= n)) ? 0.0f : c[i];
    }
}

// the two samples of a signal just beyond the lane's tile in the direction an adjoint stage looks, from clamped addresses
template <bool REV>
__device__ __forceinline__ void beyond_tile(const float *p, int n, int t0, float &near_value, float &far_value) {
    const int near = REV ? t0 + T : t0 - 1, far = REV ? t0 + T + 1 : t0 - 2;
    near_value = p[max(min(near, n - 1), 0)];
    far_value = p[max(min(far, n - 1), 0)];
}

// REV: the direction of the adjoint recurrence (the adjoint of a causal section runs REV).  KEEP: lam of the finished section is
// stored to a.keep.
template <bool REV, bool KEEP>
__global__ void __launch_bounds__(64) var2_adj_link_kernel(Var2AdjLinkArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[T * LDS_PITCH];
    const int lane = threadIdx.x;
    const int g = blockIdx.x, line = blockIdx.y;
    const int n = a.n;
    const int s0 = g * kGroupSamples;                 // below 2^30 + 4096
    const int t = g * kGroupTiles + lane, t0 = t * T;
    const int64_t first = (int64_t)line * a.stride;
    float lam[T], v[T];
    float lam_near, lam_far;
    // the final stage of section k's adjoint scan: var2_adj_pass2_1d's, lam kept in registers
    {
        float vx[T], v1[T], v2[T], c1[T], c2[T];
        request_group(a.x + first, n, s0, vx);
        request_group(a.a1 + first, n, s0, v1);
        request_group(a.a2 + first, n, s0, v2);
        float nb1, nb1_far, nb2_near, nb2_far;
        beyond_tile<REV>(a.a1 + first, n, t0, nb1, nb1_far);
        beyond_tile<REV>(a.a2 + first, n, t0, nb2_near, nb2_far);
        const int tt = min(t, a.tiles - 1);
        float m[kVar2Components], y1, y2;
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) m[i] = a.tails[map_index_of(a.n_lines, a.tiles, i, line, tt)];
        apply_map(m, a.carry[((int64_t)0 * a.n_lines + line) * a.groups + g], a.carry[((int64_t)1 * a.n_lines + line) * a.groups + g], y1, y2);
        lam_near = y1; lam_far = y2;                  // lam one and two samples before the tile, in the order of the recurrence
        transpose_in(vx, lds, lam);
        transpose_in(v1, lds, c1);
        transpose_in(v2, lds, c2);
        shift_and_mask<REV, 1>(c1, nb1, nb1_far, n, t0);
        shift_and_mask<REV, 2>(c2, nb2_near, nb2_far, n, t0);
#pragma unroll
        for (int i = 0; i < T; i++) lam[i] = t0 + i < n ? lam[i] : 0.0f;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < T; j++) {
            const int i = REV ? T - 1 - j : j;
            const float r = step2(c1[i], c2[i], lam[i], y1, y2);
            lam[i] = r; y2 = y1; y1 = r;
        }
    }
    if constexpr (KEEP) {
        store_group(lds, a.keep + first, n, s0, lam);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < T; i++) lam[i] = t0 + i < n ? lam[i] : 0.0f;
    __builtin_amdgcn_sched_barrier(0);
    // the transposed feed-forward part of section k on lam: var2_biquad_grad_1d's order, the taps one at a time
    {
        float raw[T], b[T], b_near, b_far;
        request_group(a.b0 + first, n, s0, raw);
        transpose_in(raw, lds, b);
#pragma unroll
        for (int i = 0; i < T; i++) v[i] = (t0 + i < n ? b[i] : 0.0f) * lam[i];
        request_group(a.b1 + first, n, s0, raw);
        beyond_tile<REV>(a.b1 + first, n, t0, b_near, b_far);
        transpose_in(raw, lds, b);
        shift_and_mask<REV, 1>(b, b_near, b_far, n, t0);
#pragma unroll
        for (int i = 0; i < T; i++) {
            const float one = REV ? (i + 1 < T ? lam[i + 1 < T ? i + 1 : 0] : lam_near) : (i >= 1 ? lam[i >= 1 ? i - 1 : 0] : lam_near);
            v[i] = __builtin_fmaf(b[i], one, v[i]);
        }
        request_group(a.b2 + first, n, s0, raw);
        beyond_tile<REV>(a.b2 + first, n, t0, b_near, b_far);
        transpose_in(raw, lds, b);
        shift_and_mask<REV, 2>(b, b_near, b_far, n, t0);
#pragma unroll
        for (int i = 0; i < T; i++) {
            const float two = REV ? (i + 2 < T ? lam[i + 2 < T ? i + 2 : 0] : (i + 2 == T ? lam_near : lam_far))
                                  : (i >= 2 ? lam[i >= 2 ? i - 2 : 0] : (i == 1 ? lam_near : lam_far));
            v[i] = __builtin_fmaf(b[i], two, v[i]);
        }
    }
    // the adjoint tails stage of section k - 1 on v, the gradient that enters it
    float v1[T], v2[T], c1[T], c2[T];
    request_group(a.prev_a1 + first, n, s0, v1);
    request_group(a.prev_a2 + first, n, s0, v2);
    float nb1, nb1_far, nb2_near, nb2_far;
    beyond_tile<REV>(a.prev_a1 + first, n, t0, nb1, nb1_far);
    beyond_tile<REV>(a.prev_a2 + first, n, t0, nb2_near, nb2_far);
    store_group(lds, a.dst + first, n, s0, v);
    __syncthreads();
    transpose_in(v1, lds, c1);
    transpose_in(v2, lds, c2);
    shift_and_mask<REV, 1>(c1, nb1, nb1_far, n, t0);
    shift_and_mask<REV, 2>(c2, nb2_near, nb2_far, n, t0);
#pragma unroll
    for (int i = 0; i < T; i++) v[i] = t0 + i < n ? v[i] : 0.0f;
    __builtin_amdgcn_sched_barrier(0);
    float y1 = 0.0f, y2 = 0.0f, u1 = 1.0f, u2 = 0.0f, w1 = 0.0f, w2 = 1.0f;
#pragma unroll
    for (int j = 0; j < T; j++) {
        const int i = REV ? T - 1 - j : j;
        const float r = step2(c1[i], c2[i], v[i], y1, y2);
        const float u = step2(c1[i], c2[i], 0.0f, u1, u2);
        const float w = step2(c1[i], c2[i], 0.0f, w1, w2);
        y2 = y1; y1 = r; u2 = u1; u1 = u; w2 = w1; w1 = w;
    }
    float own[kVar2Components], map[kVar2Components], whole[kVar2Components];
    own[VAR2_E0] = y1; own[VAR2_E1] = y2;
    own[VAR2_P00] = u1; own[VAR2_P10] = u2;
    own[VAR2_P01] = w1; own[VAR2_P11] = w2;
    scan_group<REV>(own, map, whole);
    if (t < a.tiles) {
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) a.tails[map_index_of(a.n_lines, a.tiles, i, line, t)] = map[i];
    }
    if (lane == (REV ? 0 : 63)) {
#pragma unroll
        for (int i = 0; i < kVar2Components; i++)
            a.tails[(int64_t)kVar2Components * a.n_lines * a.tiles + ((int64_t)i * a.n_lines + line) * a.groups + g] = whole[i];
    }
}

// ---- the recurrence over groups: one workgroup per line ---------------------------------------------------------------------------
// A sweep takes blockDim.x groups in the order of the recurrence (REV: from the last group down), lane i the i-th of them.  Within a
// sweep: an inclusive wave scan of the aggregates, the waves' totals through LDS, every lane folding the totals of the waves before
// it onto the running state -- at most 16 steps -- and all of them onto the next sweep's.  Lanes past the last group hold the identity.
template <bool REV>
__global__ void __launch_bounds__(kCarryLanes) var2_carry_kernel(Var2Args a) {
    __shared__ float totals[kCarryLanes / 64][kVar2Components];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6, span = blockDim.x;
    const int line = blockIdx.x, G = a.groups;
    float run0 = 0.0f, run1 = 0.0f;                   // the state that enters the sweep's first group
    for (int base = 0; base < G; base += span) {
        const int j = base + tid, jj = min(j, G - 1), g = REV ? G - 1 - jj : jj;
        float m[kVar2Components], other[kVar2Components], next[kVar2Components];
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) m[i] = a.tails[aggregate_index(a, i, line, g)];
        if (j >= G) identity(m);
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
#pragma unroll
            for (int i = 0; i < kVar2Components; i++) other[i] = __shfl_up(m[i], k);
            compose(other, m, next);
            if (lane >= k) {
#pragma unroll
                for (int i = 0; i < kVar2Components; i++) m[i] = next[i];
            }
        }
        if (lane == 63) {
#pragma unroll
            for (int i = 0; i < kVar2Components; i++) totals[wave][i] = m[i];
        }
        __syncthreads();
        float enter0 = run0, enter1 = run1, next0 = run0, next1 = run1;      // enter: what enters this wave's first group
        for (int w = 0; w < waves; w++) {
            float tw[kVar2Components], r0, r1;
#pragma unroll
            for (int i = 0; i < kVar2Components; i++) tw[i] = totals[w][i];
            apply_map(tw, next0, next1, r0, r1);
            next0 = r0; next1 = r1;
            if (w + 1 == wave) { enter0 = next0; enter1 = next1; }
        }
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) other[i] = __shfl_up(m[i], 1);
        if (lane == 0) identity(other);
        float c0, c1;
        apply_map(other, enter0, enter1, c0, c1);
        if (j < G) {
            a.carry[group_carry_index(a, 0, line, g)] = c0;
            a.carry[group_carry_index(a, 1, line, g)] = c1;
        }
        run0 = next0; run1 = next1;
        __syncthreads();
    }
}

// ---- the coefficient gradients: one streaming launch, four samples per lane -------------------------------------------------------
template <bool CAUSAL>
__global__ void __launch_bounds__(kGradLanes) var2_grad_kernel(Var2GradArgs a) {
    const int n = a.n;
    const int at = (blockIdx.x * kGradLanes + threadIdx.x) * 4;      // below 2^30 + 1024
    if (at >= n) return;
    const int64_t first = (int64_t)blockIdx.y * a.stride;
    const float *lam = a.lam + first, *y = a.y + first;
    const float4 l = *reinterpret_cast<const float4 *>(lam + at);
    const float4 v = *reinterpret_cast<const float4 *>(y + at);
    // the two neighbours beyond the lane's four samples, from clamped addresses; selected away at the line's end
    const int near = CAUSAL ? at - 1 : at + 4, far = CAUSAL ? at - 2 : at + 5;
    const float y_near = y[max(min(near, n - 1), 0)], y_far = y[max(min(far, n - 1), 0)];
    const float ls[4] = {l.x, l.y, l.z, l.w};
    // six consecutive samples: y[at - 2 .. at + 3] (causal: sample at + k is ys[k + 2]) or y[at .. at + 5] (sample at + k is ys[k])
    const float ys[6] = {CAUSAL ? y_far : v.x, CAUSAL ? y_near : v.y, CAUSAL ? v.x : v.z, CAUSAL ? v.y : v.w,
                         CAUSAL ? v.z : y_near, CAUSAL ? v.w : y_far};
    float g1[4], g2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float one = ys[k + 1], two = CAUSAL ? ys[k] : ys[k + 2];      // one and two samples against the forward's direction
        const bool no_one = CAUSAL ? at + k < 1 : at + k >= n - 1, no_two = CAUSAL ? at + k < 2 : at + k >= n - 2;
        g1[k] = no_one ? 0.0f : -ls[k] * one;
        g2[k] = no_two ? 0.0f : -ls[k] * two;
    }
    *reinterpret_cast<float4 *>(a.grad_a1 + first + at) = make_float4(g1[0], g1[1], g1[2], g1[3]);
    *reinterpret_cast<float4 *>(a.grad_a2 + first + at) = make_float4(g2[0], g2[1], g2[2], g2[3]);
}

// ---- the gradients of a direct-form-I section behind its adjoint scan: one streaming launch, four samples per lane ---------------
// Six consecutive samples of a signal around the lane's four, the two beyond them from clamped addresses and 0 outside the line.
//   AHEAD   p[at .. at + 5]:      sample at + k is w[k]
//   else    p[at - 2 .. at + 3]:  sample at + k is w[k + 2]
template <bool AHEAD>
__device__ __forceinline__ void load_six(const float *p, int at, int n, float (&w)[6]) {
    const float4 q = *reinterpret_cast<const float4 *>(p + at);
    const int near = AHEAD ? at + 4 : at - 1, far = AHEAD ? at + 5 : at - 2;
    float p_near = p[max(min(near, n - 1), 0)], p_far = p[max(min(far, n - 1), 0)];
    p_near = (near < 0 || near >= n) ? 0.0f : p_near;
    p_far = (far < 0 || far >= n) ? 0.0f : p_far;
    w[0] = AHEAD ? q.x : p_far; w[1] = AHEAD ? q.y : p_near; w[2] = AHEAD ? q.z : q.x; w[3] = AHEAD ? q.w : q.y;
    w[4] = AHEAD ? p_near : q.z; w[5] = AHEAD ? p_far : q.w;
}

// CAUSAL: the direction of the forward section -- its adjoint looks ahead (lam, b1, b2), its coefficient gradients look back (x, y)
template <bool CAUSAL, bool COEF>
__global__ void __launch_bounds__(kGradLanes) var2_biquad_grad_kernel(Var2BiquadGradArgs a) {
    const int n = a.n;
    const int at = (blockIdx.x * kGradLanes + threadIdx.x) * 4;      // below 2^30 + 1024
    if (at >= n) return;
    const int64_t first = (int64_t)blockIdx.y * a.stride;
    constexpr int L0 = CAUSAL ? 0 : 2;      // sample at + k in a window that looks where the adjoint looks
    constexpr int X0 = CAUSAL ? 2 : 0;      // and in one that looks where the forward looked
    float lam[6], t1[6], t2[6];
    load_six<CAUSAL>(a.lam + first, at, n, lam);
    load_six<CAUSAL>(a.b1 + first, at, n, t1);
    load_six<CAUSAL>(a.b2 + first, at, n, t2);
    const float4 q0 = *reinterpret_cast<const float4 *>(a.b0 + first + at);
    const float t0[4] = {q0.x, q0.y, q0.z, q0.w};
    float gx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        // the taps one and two samples along the forward's direction: inside the line they are never ones the forward masked
        const int one = CAUSAL ? at + k + 1 : at + k - 1, two = CAUSAL ? at + k + 2 : at + k - 2;
        const int i1 = CAUSAL ? L0 + k + 1 : L0 + k - 1, i2 = CAUSAL ? L0 + k + 2 : L0 + k - 2;
        const float c1 = (one < 0 || one >= n) ? 0.0f : t1[i1], c2 = (two < 0 || two >= n) ? 0.0f : t2[i2];
        gx[k] = __builtin_fmaf(c2, lam[i2], __builtin_fmaf(c1, lam[i1], t0[k] * lam[L0 + k]));
    }
    if constexpr (COEF) {
        float xs[6], ys[6];
        load_six<!CAUSAL>(a.x + first, at, n, xs);
        load_six<!CAUSAL>(a.y + first, at, n, ys);
        float g0[4], g1[4], g2[4], h1[4], h2[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i1 = CAUSAL ? X0 + k - 1 : X0 + k + 1, i2 = CAUSAL ? X0 + k - 2 : X0 + k + 2;
            const bool no_one = CAUSAL ? at + k < 1 : at + k >= n - 1, no_two = CAUSAL ? at + k < 2 : at + k >= n - 2;
            const float l = lam[L0 + k];
            g0[k] = l * xs[X0 + k];
            g1[k] = no_one ? 0.0f : l * xs[i1];
            g2[k] = no_two ? 0.0f : l * xs[i2];
            h1[k] = no_one ? 0.0f : -l * ys[i1];
            h2[k] = no_two ? 0.0f : -l * ys[i2];
        }
        *reinterpret_cast<float4 *>(a.grad_b0 + first + at) = make_float4(g0[0], g0[1], g0[2], g0[3]);
        *reinterpret_cast<float4 *>(a.grad_b1 + first + at) = make_float4(g1[0], g1[1], g1[2], g1[3]);
        *reinterpret_cast<float4 *>(a.grad_b2 + first + at) = make_float4(g2[0], g2[1], g2[2], g2[3]);
        *reinterpret_cast<float4 *>(a.grad_a1 + first + at) = make_float4(h1[0], h1[1], h1[2], h1[3]);
        *reinterpret_cast<float4 *>(a.grad_a2 + first + at) = make_float4(h2[0], h2[1], h2[2], h2[3]);
    }
    *reinterpret_cast<float4 *>(a.grad_in + first + at) = make_float4(gx[0], gx[1], gx[2], gx[3]);
}

// The five coefficient gradients alone (var2_biquad_coef_1d), for a section whose input gradient var2_adj_link_keep_1d has formed:
// the COEF half above -- the same products, selects and +0 at the masked slots -- from lam, x and y; no tap is read.
template <bool CAUSAL>
__global__ void __launch_bounds__(kGradLanes) var2_biquad_coef_kernel(Var2BiquadGradArgs a) {
    const int n = a.n;
    const int at = (blockIdx.x * kGradLanes + threadIdx.x) * 4;      // below 2^30 + 1024
    if (at >= n) return;
    const int64_t first = (int64_t)blockIdx.y * a.stride;
    constexpr int X0 = CAUSAL ? 2 : 0;
    const float4 q = *reinterpret_cast<const float4 *>(a.lam + first + at);
    const float lam[4] = {q.x, q.y, q.z, q.w};
    float xs[6], ys[6];
    load_six<!CAUSAL>(a.x + first, at, n, xs);
    load_six<!CAUSAL>(a.y + first, at, n, ys);
    float g0[4], g1[4], g2[4], h1[4], h2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i1 = CAUSAL ? X0 + k - 1 : X0 + k + 1, i2 = CAUSAL ? X0 + k - 2 : X0 + k + 2;
        const bool no_one = CAUSAL ? at + k < 1 : at + k >= n - 1, no_two = CAUSAL ? at + k < 2 : at + k >= n - 2;
        const float l = lam[k];
        g0[k] = l * xs[X0 + k];
        g1[k] = no_one ? 0.0f : l * xs[i1];
        g2[k] = no_two ? 0.0f : l * xs[i2];
        h1[k] = no_one ? 0.0f : -l * ys[i1];
        h2[k] = no_two ? 0.0f : -l * ys[i2];
    }
    *reinterpret_cast<float4 *>(a.grad_b0 + first + at) = make_float4(g0[0], g0[1], g0[2], g0[3]);
    *reinterpret_cast<float4 *>(a.grad_b1 + first + at) = make_float4(g1[0], g1[1], g1[2], g1[3]);
    *reinterpret_cast<float4 *>(a.grad_b2 + first + at) = make_float4(g2[0], g2[1], g2[2], g2[3]);
    *reinterpret_cast<float4 *>(a.grad_a1 + first + at) = make_float4(h1[0], h1[1], h1[2], h1[3]);
    *reinterpret_cast<float4 *>(a.grad_a2 + first + at) = make_float4(h2[0], h2[1], h2[2], h2[3]);
}

// ---- coefficients from control-rate frames ---------------------------------------------------------------------------------------
// Frame j of a coefficient sits at sample j * hop, hop = 1 << shift >= 64: a tile lies inside one interval.  At n = j * hop + k
//   c[n] = fma(k / hop, c[j+1] - c[j], c[j])          (k / hop exact; the difference rounded once; c[j * hop] == c[j])
// and every kernel below forms it with frame_lerp, so all of them see one value per sample.
struct FramePair {
    float c, d;      // c[j] and c[j+1] - c[j]
};
__device__ __forceinline__ FramePair frame_pair(const float *frames, int j) {
    const float c = frames[j];
    return {c, frames[j + 1] - c};
}
__device__ __forceinline__ float frame_lerp(const FramePair &p, int k, float inv_hop) { return __builtin_fmaf((float)k * inv_hop, p.d, p.c); }
// the coefficient at sample `at` of the line, 0 <= at < n: its interval has both frames (n_frames = ceil(n / hop) + 1)
__device__ __forceinline__ float frame_at(const float *frames, int at, int shift, float inv_hop) {
    return frame_lerp(frame_pair(frames, at >> shift), at & ((1 << shift) - 1), inv_hop);
}

// ---- a state that enters and leaves a call (rf_var2_plan_execute_cascade_frames_stream) ---------------------------------------------
// A line's state is K + 1 pairs (the sample one place before the line, the one two places before it) in the order of the
// recurrence: pair 0 of the input, pair k + 1 of section k's result.  The entering state is folded into the two first samples of a
// section's v, by the lane whose tile holds them (n is a multiple of 4: one tile holds both); the masked recurrence from zero on
// that v is the unmasked one from the true state, so the tails, the carry and the final stage run as they are.
//   v[0] = fma(b2[0], hx2, fma(b1[0], hx1, b0[0] * src[0]))          v[0] = fma(-a1[0], hy1, fma(-a2[0], hy2, v[0]))
//   v[1] = fma(b2[1], hx1, fma(b1[1], src[0], b0[1] * src[1]))       v[1] = fma(-a2[1], hy1, v[1])
// (REV: samples n - 1 and n - 2.)  pairs: (hx1, hx2, hy1, hy2), the section's input and result pairs, adjacent in the layout.
template <bool REV>
__device__ __forceinline__ void fold_entering_state(const float *pairs, const float (&src)[T], float (&v)[T], const FramePair &b0, const FramePair &b1,
                                                    const FramePair &b2, const FramePair &a1, const FramePair &a2, int k0, float inv_hop, int n, int t0) {
    const int i0 = REV ? n - 1 - t0 : 0, i1 = REV ? i0 - 1 : 1;      // the first and the second sample of the recurrence, in the tile
    const float hx1 = pairs[0], hx2 = pairs[1], hy1 = pairs[2], hy2 = pairs[3];
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int i = 0; i < T; i++) {
        s0 = i == i0 ? src[i] : s0;
        s1 = i == i1 ? src[i] : s1;
    }
    float v0 = frame_lerp(b0, k0 + i0, inv_hop) * s0;
    v0 = __builtin_fmaf(frame_lerp(b1, k0 + i0, inv_hop), hx1, v0);
    v0 = __builtin_fmaf(frame_lerp(b2, k0 + i0, inv_hop), hx2, v0);
    float v1 = frame_lerp(b0, k0 + i1, inv_hop) * s1;
    v1 = __builtin_fmaf(frame_lerp(b1, k0 + i1, inv_hop), s0, v1);
    v1 = __builtin_fmaf(frame_lerp(b2, k0 + i1, inv_hop), hx1, v1);
    v0 = step2(frame_lerp(a1, k0 + i0, inv_hop), frame_lerp(a2, k0 + i0, inv_hop), v0, hy1, hy2);
    v1 = __builtin_fmaf(-frame_lerp(a2, k0 + i1, inv_hop), hy1, v1);
#pragma unroll
    for (int i = 0; i < T; i++) v[i] = i == i0 ? v0 : (i == i1 ? v1 : v[i]);
}

// the leaving pair of a signal from the tile that holds the line's two last samples in the order of the recurrence
template <bool REV>
__device__ __forceinline__ void store_leaving_pair(float *pair, const float (&y)[T], int n, int t0) {
    const int i0 = REV ? 0 : n - 1 - t0, i1 = REV ? 1 : i0 - 1;
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int i = 0; i < T; i++) {
        s0 = i == i0 ? y[i] : s0;
        s1 = i == i1 ? y[i] : s1;
    }
    pair[0] = s0;
    pair[1] = s1;
}

// The backward of a call with a state.  The leaving state is made of samples of x, of the kept signals and of out, so its gradient
// is ADDED to the two last samples (the adjoint recurrence's two first) of the gradient each of them receives; the adjoint scans
// themselves stay masked and start from zero.  REV: the direction of the adjoint recurrence.
template <bool REV>
__device__ __forceinline__ void add_leaving_gradient(const float *pair, float (&g)[T], int n, int t0) {
    const int i0 = REV ? n - 1 - t0 : 0, i1 = REV ? i0 - 1 : 1;
    const float g0 = pair[0], g1 = pair[1];
#pragma unroll
    for (int i = 0; i < T; i++) g[i] = i == i0 ? g[i] + g0 : (i == i1 ? g[i] + g1 : g[i]);
}

// The gradient of the entering state from lam_j of the tile that holds the forward's two first samples (the adjoint's two last):
//   feedback part, to pair j + 1     (fma(-a1[0], lam[0], -(a2[1] * lam[1])), -(a2[0] * lam[0]))     added to what section j + 1 left there
//   feed-forward part, to pair j     (fma(b1[0], lam[0], b2[1] * lam[1]), b2[0] * lam[0])            stored
// by one lane, in stream order: no atomic.  first: nothing was left in pair j + 1 (the last section).
template <bool REV>
__device__ __forceinline__ void store_entering_gradient(float *pairs, bool first, const float (&lam)[T], const FramePair &b1, const FramePair &b2,
                                                        const FramePair &a1, const FramePair &a2, int k0, float inv_hop, int n, int t0) {
    const int i0 = REV ? 0 : n - 1 - t0, i1 = REV ? 1 : i0 - 1;      // the forward's first and second sample, in the tile
    float l0 = 0.0f, l1 = 0.0f;
#pragma unroll
    for (int i = 0; i < T; i++) {
        l0 = i == i0 ? lam[i] : l0;
        l1 = i == i1 ? lam[i] : l1;
    }
    const float fb0 = __builtin_fmaf(-frame_lerp(a1, k0 + i0, inv_hop), l0, -(frame_lerp(a2, k0 + i1, inv_hop) * l1));
    const float fb1 = -(frame_lerp(a2, k0 + i0, inv_hop) * l0);
    const float ff0 = __builtin_fmaf(frame_lerp(b1, k0 + i0, inv_hop), l0, frame_lerp(b2, k0 + i1, inv_hop) * l1);
    const float ff1 = frame_lerp(b2, k0 + i0, inv_hop) * l0;
    pairs[2] = first ? fb0 : pairs[2] + fb0;
    pairs[3] = first ? fb1 : pairs[3] + fb1;
    pairs[0] = ff0;
    pairs[1] = ff1;
}

// var2_signal_kernel with the coefficient signals formed in registers: the same masks by position, the same order of the
// feed-forward part, the same recurrences, scan and stores.  Nothing but x goes through the transposition, and a coefficient
// lives for one step.  ADJ: the three coefficients its shifted reads reach beyond the tile come from frame_at at a position
// clamped into the line -- the next interval's where the tile ends at a frame -- and are masked by position like the rest.
// STREAM (var2_biquad_frames_tails_stream_1d, var2_frames_pass2_stream_1d): a.state_in folded into v by the FF stage, the
// leaving pair a.pair of a.state_out from the tile in registers -- x by the FF stage, the result by the final one.
template <bool REV, bool ADJ, bool FINAL, bool FF = false, bool STREAM = false>
__global__ void __launch_bounds__(64) var2_frames_kernel(Var2FramesArgs a) {
    static_assert(!FF || (!ADJ && !FINAL), "the feed-forward part stands in front of a forward tails stage");
    static_assert(!STREAM || ADJ || FF || FINAL, "the state enters in the FF stage and leaves there and in the final one");
    __shared__ __attribute__((aligned(16))) float lds[T * LDS_PITCH];
    const int lane = threadIdx.x;
    const int g = blockIdx.x, line = blockIdx.y;
    const int n = a.n;
    const int s0 = g * kGroupSamples;                 // below 2^30 + 4096
    const int t = g * kGroupTiles + lane, t0 = t * T;
    const int64_t first = (int64_t)line * a.stride, frame0 = (int64_t)line * a.frame_stride;
    const int shift = a.hop_shift;
    const float inv_hop = a.inv_hop;
    // the tile's interval; a tile beyond the line takes the last one (everything in it is masked)
    const int j = min(t0 >> shift, a.n_frames - 2), k0 = t0 & ((1 << shift) - 1);
    const float *px = a.x + first;
    float raw[T], x[T];
    request_group(px, n, s0, raw);
    const FramePair f1 = frame_pair(a.a1 + frame0, j), f2 = frame_pair(a.a2 + frame0, j);
    const int near = REV ? t0 + T : t0 - 1, far = REV ? t0 + T + 1 : t0 - 2;      // beyond the tile, against the recurrence
    const int at_near = max(min(near, n - 1), 0), at_far = max(min(far, n - 1), 0);
    float nb1 = 0.0f, nb2_near = 0.0f, nb2_far = 0.0f;
    if constexpr (ADJ) {
        nb1 = frame_at(a.a1 + frame0, at_near, shift, inv_hop);
        nb2_near = frame_at(a.a2 + frame0, at_near, shift, inv_hop);
        nb2_far = frame_at(a.a2 + frame0, at_far, shift, inv_hop);
    }
    float y1 = 0.0f, y2 = 0.0f;                       // the state that enters the tile
    if constexpr (FINAL) {
        const int tt = min(t, a.tiles - 1);
        float m[kVar2Components];
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) m[i] = a.tails[map_index_of(a.n_lines, a.tiles, i, line, tt)];
        apply_map(m, a.carry[((int64_t)0 * a.n_lines + line) * a.groups + g], a.carry[((int64_t)1 * a.n_lines + line) * a.groups + g], y1, y2);
    }
    if constexpr (FF) {
        float x_near = px[at_near], x_far = px[at_far];
        x_near = (near < 0 || near >= n) ? 0.0f : x_near;
        x_far = (far < 0 || far >= n) ? 0.0f : x_far;
        const FramePair f0 = frame_pair(a.b0 + frame0, j), g1 = frame_pair(a.b1 + frame0, j), g2 = frame_pair(a.b2 + frame0, j);
        float u[T];
        transpose_in(raw, lds, u);
#pragma unroll
        for (int i = 0; i < T; i++) u[i] = t0 + i < n ? u[i] : 0.0f;
        // feed_forward's arithmetic: b0 x, then b1~ on the sample before, then b2~ on the one before that
#pragma unroll
        for (int i = 0; i < T; i++) {
            const int at = t0 + i;
            const float one = REV ? (i + 1 < T ? u[i + 1 < T ? i + 1 : 0] : x_near) : (i >= 1 ? u[i >= 1 ? i - 1 : 0] : x_near);
            const float two = REV ? (i + 2 < T ? u[i + 2 < T ? i + 2 : 0] : (i + 2 == T ? x_near : x_far))
                                  : (i >= 2 ? u[i >= 2 ? i - 2 : 0] : (i == 1 ? x_near : x_far));
            const bool no_one = REV ? at >= n - 1 : (at < 1 || at >= n), no_two = REV ? at >= n - 2 : (at < 2 || at >= n);
            float v = (at < n ? frame_lerp(f0, k0 + i, inv_hop) : 0.0f) * u[i];
            v = __builtin_fmaf(no_one ? 0.0f : frame_lerp(g1, k0 + i, inv_hop), one, v);
            x[i] = __builtin_fmaf(no_two ? 0.0f : frame_lerp(g2, k0 + i, inv_hop), two, v);
        }
        if constexpr (STREAM) {
            const int64_t state0 = (int64_t)line * a.state_stride + 2 * a.pair;
            if (a.state_in && t == (REV ? a.tiles - 1 : 0)) fold_entering_state<REV>(a.state_in + state0, u, x, f0, g1, g2, f1, f2, k0, inv_hop, n, t0);
            if (a.state_out && t == (REV ? 0 : a.tiles - 1)) store_leaving_pair<REV>(a.state_out + state0, u, n, t0);
        }
        store_group(lds, a.dst + first, n, s0, x);      // v: what var2_frames_pass2_1d reads, in place
#pragma unroll
        for (int i = 0; i < T; i++) x[i] = t0 + i < n ? x[i] : 0.0f;
    } else {
        transpose_in(raw, lds, x);
#pragma unroll
        for (int i = 0; i < T; i++) x[i] = t0 + i < n ? x[i] : 0.0f;
        if constexpr (STREAM && ADJ) {      // x is grad_out: the gradient of the result's leaving pair
            if (a.grad_state_out && a.add_pair >= 0 && t == (REV ? a.tiles - 1 : 0))
                add_leaving_gradient<REV>(a.grad_state_out + (int64_t)line * a.state_stride + 2 * a.add_pair, x, n, t0);
        }
    }
    // the coefficients of step i, masked by position: the tile's own, or (ADJ) those one and two samples further along the
    // forward's direction
    auto coefficients = [&](int i, float &c1, float &c2) {
        const int at = t0 + i;
        if constexpr (!ADJ) {
            c1 = frame_lerp(f1, k0 + i, inv_hop);
            c2 = frame_lerp(f2, k0 + i, inv_hop);
        } else if constexpr (REV) {
            c1 = i + 1 < T ? frame_lerp(f1, k0 + i + 1, inv_hop) : nb1;
            c2 = i + 2 < T ? frame_lerp(f2, k0 + i + 2, inv_hop) : (i + 2 == T ? nb2_near : nb2_far);
        } else {
            c1 = i >= 1 ? frame_lerp(f1, k0 + i - 1, inv_hop) : nb1;
            c2 = i >= 2 ? frame_lerp(f2, k0 + i - 2, inv_hop) : (i == 1 ? nb2_near : nb2_far);
        }
        if constexpr (REV) {
            c1 = at >= n - 1 ? 0.0f : c1;
            c2 = at >= n - 2 ? 0.0f : c2;
        } else {
            c1 = (at < 1 || at >= n) ? 0.0f : c1;
            c2 = (at < 2 || at >= n) ? 0.0f : c2;
        }
    };
    if constexpr (FINAL) {
#pragma unroll
        for (int s = 0; s < T; s++) {
            const int i = REV ? T - 1 - s : s;
            float c1, c2;
            coefficients(i, c1, c2);
            const float y = step2(c1, c2, x[i], y1, y2);
            x[i] = y; y2 = y1; y1 = y;
        }
        if constexpr (STREAM && !ADJ) {
            if (a.state_out && t == (REV ? 0 : a.tiles - 1)) store_leaving_pair<REV>(a.state_out + (int64_t)line * a.state_stride + 2 * a.pair, x, n, t0);
        }
        if constexpr (STREAM && ADJ) {      // x is lam of section a.pair
            if (a.grad_state_in && t == (REV ? 0 : a.tiles - 1))
                store_entering_gradient<REV>(a.grad_state_in + (int64_t)line * a.state_stride + 2 * a.pair, a.pair == a.last_section, x,
                                             frame_pair(a.b1 + frame0, j), frame_pair(a.b2 + frame0, j), f1, f2, k0, inv_hop, n, t0);
        }
        store_group(lds, a.dst + first, n, s0, x);
    } else {
        float u1 = 1.0f, u2 = 0.0f, w1 = 0.0f, w2 = 1.0f;
#pragma unroll
        for (int s = 0; s < T; s++) {
            const int i = REV ? T - 1 - s : s;
            float c1, c2;
            coefficients(i, c1, c2);
            const float y = step2(c1, c2, x[i], y1, y2);
            const float u = step2(c1, c2, 0.0f, u1, u2);
            const float w = step2(c1, c2, 0.0f, w1, w2);
            y2 = y1; y1 = y; u2 = u1; u1 = u; w2 = w1; w1 = w;
        }
        float own[kVar2Components], map[kVar2Components], whole[kVar2Components];
        own[VAR2_E0] = y1; own[VAR2_E1] = y2;
        own[VAR2_P00] = u1; own[VAR2_P10] = u2;
        own[VAR2_P01] = w1; own[VAR2_P11] = w2;
        scan_group<REV>(own, map, whole);
        if (t < a.tiles) {
#pragma unroll
            for (int i = 0; i < kVar2Components; i++) a.tails[map_index_of(a.n_lines, a.tiles, i, line, t)] = map[i];
        }
        if (lane == (REV ? 0 : 63)) {
#pragma unroll
            for (int i = 0; i < kVar2Components; i++)
                a.tails[(int64_t)kVar2Components * a.n_lines * a.tiles + ((int64_t)i * a.n_lines + line) * a.groups + g] = whole[i];
        }
    }
}

// ---- the boundary between two sections of a cascade on frames ------------------------------------------------------------------------
// The coefficient of step i of a forward stage from frames, masked by position where it would multiply a sample SHIFT places
// outside the line (SHIFT 0: b0, masked from n on alone).
template <bool REV, int SHIFT>
__device__ __forceinline__ float own_frame(const FramePair &p, int k0, int i, float inv_hop, int n, int t0) {
    const int at = t0 + i;
    return (REV ? at >= n - SHIFT : (at < SHIFT || at >= n)) ? 0.0f : frame_lerp(p, k0 + i, inv_hop);
}

// The coefficient of step i of an adjoint stage from frames: the value SHIFT samples further along the forward's direction (REV:
// toward the line's end) -- frame_lerp inside the tile, beyond it the values handed in (frame_at at a position clamped into the
// line) -- then the mask by position of the scan's own direction: shift_and_mask on a value that lives for one step.
template <bool REV, int SHIFT>
__device__ __forceinline__ float shifted_frame(const FramePair &p, int k0, int i, float inv_hop, float beyond_near, float beyond_far, int n, int t0) {
    const int from = REV ? i + SHIFT : i - SHIFT, at = t0 + i;
    const bool inside = from >= 0 && from < T;
    const bool nearest = REV ? from == T : from == -1;
    const float c = inside ? frame_lerp(p, k0 + (inside ? from : 0), inv_hop) : (nearest ? beyond_near : beyond_far);
    return (REV ? at >= n - SHIFT : (at < SHIFT || at >= n)) ? 0.0f : c;
}

// the tails of a tile from the state it leaves and the two columns of its matrix: the group scan and the stores every tails
// stage ends with
template <bool REV>
__device__ __forceinline__ void store_tails(float *tails, int n_lines, int tiles, int groups, int line, int g, int t, float y1, float y2, float u1,
                                            float u2, float w1, float w2) {
    float own[kVar2Components], map[kVar2Components], whole[kVar2Components];
    own[VAR2_E0] = y1; own[VAR2_E1] = y2;
    own[VAR2_P00] = u1; own[VAR2_P10] = u2;
    own[VAR2_P01] = w1; own[VAR2_P11] = w2;
    scan_group<REV>(own, map, whole);
    if (t < tiles) {
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) tails[map_index_of(n_lines, tiles, i, line, t)] = map[i];
    }
    if (threadIdx.x == (REV ? 0 : 63)) {
#pragma unroll
        for (int i = 0; i < kVar2Components; i++)
            tails[(int64_t)kVar2Components * n_lines * tiles + ((int64_t)i * n_lines + line) * groups + g] = whole[i];
    }
}

// var2_link_kernel with every coefficient formed as var2_frames_kernel forms it: x alone goes through the transposition, one
// FramePair per coefficient, a value per step.  KEEP: y of the finished section is stored to a.keep (it may be a.x).
// STREAM (var2_frames_link_stream_1d, var2_frames_link_keep_stream_1d): pair a.pair of the state is the finished section's -- its
// leaving pair from y in registers, and with the pair behind it what enters the next section, folded into v.
template <bool REV, bool KEEP, bool STREAM = false>
__global__ void __launch_bounds__(64) var2_frames_link_kernel(Var2FramesLinkArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[T * LDS_PITCH];
    const int lane = threadIdx.x;
    const int g = blockIdx.x, line = blockIdx.y;
    const int n = a.n;
    const int s0 = g * kGroupSamples;                 // below 2^30 + 4096
    const int t = g * kGroupTiles + lane, t0 = t * T;
    const int64_t first = (int64_t)line * a.stride, frame0 = (int64_t)line * a.frame_stride;
    const int shift = a.hop_shift;
    const float inv_hop = a.inv_hop;
    const int j = min(t0 >> shift, a.n_frames - 2), k0 = t0 & ((1 << shift) - 1);
    float y[T], v[T];
    float y_near, y_far;
    // the final stage of the section behind the boundary: var2_frames_pass2_1d's, y kept in registers
    {
        float raw[T];
        request_group(a.x + first, n, s0, raw);
        const FramePair f1 = frame_pair(a.a1 + frame0, j), f2 = frame_pair(a.a2 + frame0, j);
        const int tt = min(t, a.tiles - 1);
        float m[kVar2Components], y1, y2;
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) m[i] = a.tails[map_index_of(a.n_lines, a.tiles, i, line, tt)];
        apply_map(m, a.carry[((int64_t)0 * a.n_lines + line) * a.groups + g], a.carry[((int64_t)1 * a.n_lines + line) * a.groups + g], y1, y2);
        y_near = y1; y_far = y2;                      // y one and two samples before the tile, in the order of the recurrence
        transpose_in(raw, lds, y);
#pragma unroll
        for (int i = 0; i < T; i++) y[i] = t0 + i < n ? y[i] : 0.0f;
#pragma unroll
        for (int s = 0; s < T; s++) {
            const int i = REV ? T - 1 - s : s;
            const float r = step2(own_frame<REV, 1>(f1, k0, i, inv_hop, n, t0), own_frame<REV, 2>(f2, k0, i, inv_hop, n, t0), y[i], y1, y2);
            y[i] = r; y2 = y1; y1 = r;
        }
    }
    if constexpr (KEEP) {
        store_group(lds, a.keep + first, n, s0, y);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < T; i++) y[i] = t0 + i < n ? y[i] : 0.0f;
    // the section in front of the boundary: its feed-forward part on y in feed_forward's order, then its tails stage
    {
        const FramePair f0 = frame_pair(a.next_b0 + frame0, j), g1 = frame_pair(a.next_b1 + frame0, j), g2 = frame_pair(a.next_b2 + frame0, j);
#pragma unroll
        for (int i = 0; i < T; i++) {
            const float one = REV ? (i + 1 < T ? y[i + 1 < T ? i + 1 : 0] : y_near) : (i >= 1 ? y[i >= 1 ? i - 1 : 0] : y_near);
            const float two = REV ? (i + 2 < T ? y[i + 2 < T ? i + 2 : 0] : (i + 2 == T ? y_near : y_far))
                                  : (i >= 2 ? y[i >= 2 ? i - 2 : 0] : (i == 1 ? y_near : y_far));
            float w = own_frame<REV, 0>(f0, k0, i, inv_hop, n, t0) * y[i];
            w = __builtin_fmaf(own_frame<REV, 1>(g1, k0, i, inv_hop, n, t0), one, w);
            v[i] = __builtin_fmaf(own_frame<REV, 2>(g2, k0, i, inv_hop, n, t0), two, w);
        }
        if constexpr (STREAM) {
            const int64_t state0 = (int64_t)line * a.state_stride + 2 * a.pair;
            if (a.state_in && t == (REV ? a.tiles - 1 : 0))
                fold_entering_state<REV>(a.state_in + state0, y, v, f0, g1, g2, frame_pair(a.next_a1 + frame0, j), frame_pair(a.next_a2 + frame0, j), k0,
                                         inv_hop, n, t0);
            if (a.state_out && t == (REV ? 0 : a.tiles - 1)) store_leaving_pair<REV>(a.state_out + state0, y, n, t0);
        }
    }
    store_group(lds, a.dst + first, n, s0, v);
    const FramePair h1 = frame_pair(a.next_a1 + frame0, j), h2 = frame_pair(a.next_a2 + frame0, j);
    float y1 = 0.0f, y2 = 0.0f, u1 = 1.0f, u2 = 0.0f, w1 = 0.0f, w2 = 1.0f;
#pragma unroll
    for (int s = 0; s < T; s++) {
        const int i = REV ? T - 1 - s : s;
        const float c1 = own_frame<REV, 1>(h1, k0, i, inv_hop, n, t0), c2 = own_frame<REV, 2>(h2, k0, i, inv_hop, n, t0);
        const float r = step2(c1, c2, v[i], y1, y2);
        const float u = step2(c1, c2, 0.0f, u1, u2);
        const float w = step2(c1, c2, 0.0f, w1, w2);
        y2 = y1; y1 = r; u2 = u1; u1 = u; w2 = w1; w1 = w;
    }
    store_tails<REV>(a.tails, a.n_lines, a.tiles, a.groups, line, g, t, y1, y2, u1, u2, w1, w2);
}

// var2_adj_link_kernel on frames.  REV: the direction of the adjoint recurrence.  The shifted reads -- a1, b1 one sample and a2,
// b2 two samples along the forward's direction -- are frame_lerp inside the tile and frame_at at a clamped position beyond it
// (the ADJ branch of var2_frames_kernel).  KEEP: lam of the finished section is stored to a.keep.
// STREAM (var2_adj_frames_link_stream_1d, var2_adj_frames_link_keep_stream_1d): a.pair = k.  Where x is grad_out (a.add_pair >= 0) the
// gradient of the result's leaving pair is added to it in registers; lam_k gives its parts of grad_state_in; the gradient of pair k
// is added to g_{k-1} before it is stored and scanned.
template <bool REV, bool KEEP, bool STREAM = false>
__global__ void __launch_bounds__(64) var2_adj_frames_link_kernel(Var2AdjFramesLinkArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[T * LDS_PITCH];
    const int lane = threadIdx.x;
    const int g = blockIdx.x, line = blockIdx.y;
    const int n = a.n;
    const int s0 = g * kGroupSamples;                 // below 2^30 + 4096
    const int t = g * kGroupTiles + lane, t0 = t * T;
    const int64_t first = (int64_t)line * a.stride, frame0 = (int64_t)line * a.frame_stride;
    const int shift = a.hop_shift;
    const float inv_hop = a.inv_hop;
    const int j = min(t0 >> shift, a.n_frames - 2), k0 = t0 & ((1 << shift) - 1);
    const int near = REV ? t0 + T : t0 - 1, far = REV ? t0 + T + 1 : t0 - 2;      // beyond the tile, against the recurrence
    const int at_near = max(min(near, n - 1), 0), at_far = max(min(far, n - 1), 0);
    float lam[T], v[T];
    float lam_near, lam_far;
    // the final stage of section k's adjoint scan: var2_adj_frames_pass2_1d's, lam kept in registers
    {
        float raw[T];
        request_group(a.x + first, n, s0, raw);
        const FramePair f1 = frame_pair(a.a1 + frame0, j), f2 = frame_pair(a.a2 + frame0, j);
        const float nb1 = frame_at(a.a1 + frame0, at_near, shift, inv_hop);
        const float nb2_near = frame_at(a.a2 + frame0, at_near, shift, inv_hop), nb2_far = frame_at(a.a2 + frame0, at_far, shift, inv_hop);
        const int tt = min(t, a.tiles - 1);
        float m[kVar2Components], y1, y2;
#pragma unroll
        for (int i = 0; i < kVar2Components; i++) m[i] = a.tails[map_index_of(a.n_lines, a.tiles, i, line, tt)];
        apply_map(m, a.carry[((int64_t)0 * a.n_lines + line) * a.groups + g], a.carry[((int64_t)1 * a.n_lines + line) * a.groups + g], y1, y2);
        lam_near = y1; lam_far = y2;                  // lam one and two samples before the tile, in the order of the recurrence
        transpose_in(raw, lds, lam);
#pragma unroll
        for (int i = 0; i < T; i++) lam[i] = t0 + i < n ? lam[i] : 0.0f;
        if constexpr (STREAM) {
            if (a.grad_state_out && a.add_pair >= 0 && t == (REV ? a.tiles - 1 : 0))
                add_leaving_gradient<REV>(a.grad_state_out + (int64_t)line * a.state_stride + 2 * a.add_pair, lam, n, t0);
        }
#pragma unroll
        for (int s = 0; s < T; s++) {
            const int i = REV ? T - 1 - s : s;
            const float c1 = shifted_frame<REV, 1>(f1, k0, i, inv_hop, nb1, nb1, n, t0);
            const float c2 = shifted_frame<REV, 2>(f2, k0, i, inv_hop, nb2_near, nb2_far, n, t0);
            const float r = step2(c1, c2, lam[i], y1, y2);
            lam[i] = r; y2 = y1; y1 = r;
        }
    }
    if constexpr (KEEP) {
        store_group(lds, a.keep + first, n, s0, lam);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < T; i++) lam[i] = t0 + i < n ? lam[i] : 0.0f;
    // the transposed feed-forward part of section k on lam: var2_biquad_grad_1d's order
    {
        const FramePair f0 = frame_pair(a.b0 + frame0, j), g1 = frame_pair(a.b1 + frame0, j), g2 = frame_pair(a.b2 + frame0, j);
        const float b1_near = frame_at(a.b1 + frame0, at_near, shift, inv_hop);
        const float b2_near = frame_at(a.b2 + frame0, at_near, shift, inv_hop), b2_far = frame_at(a.b2 + frame0, at_far, shift, inv_hop);
#pragma unroll
        for (int i = 0; i < T; i++) {
            const float one = REV ? (i + 1 < T ? lam[i + 1 < T ? i + 1 : 0] : lam_near) : (i >= 1 ? lam[i >= 1 ? i - 1 : 0] : lam_near);
            const float two = REV ? (i + 2 < T ? lam[i + 2 < T ? i + 2 : 0] : (i + 2 == T ? lam_near : lam_far))
                                  : (i >= 2 ? lam[i >= 2 ? i - 2 : 0] : (i == 1 ? lam_near : lam_far));
            float w = own_frame<REV, 0>(f0, k0, i, inv_hop, n, t0) * lam[i];
            w = __builtin_fmaf(shifted_frame<REV, 1>(g1, k0, i, inv_hop, b1_near, b1_near, n, t0), one, w);
            v[i] = __builtin_fmaf(shifted_frame<REV, 2>(g2, k0, i, inv_hop, b2_near, b2_far, n, t0), two, w);
        }
        if constexpr (STREAM) {
            const int64_t state0 = (int64_t)line * a.state_stride + 2 * a.pair;
            if (a.grad_state_in && t == (REV ? 0 : a.tiles - 1))
                store_entering_gradient<REV>(a.grad_state_in + state0, a.pair == a.last_section, lam, g1, g2, frame_pair(a.a1 + frame0, j),
                                             frame_pair(a.a2 + frame0, j), k0, inv_hop, n, t0);
            if (a.grad_state_out && t == (REV ? a.tiles - 1 : 0)) add_leaving_gradient<REV>(a.grad_state_out + state0, v, n, t0);
        }
    }
    store_group(lds, a.dst + first, n, s0, v);
#pragma unroll
    for (int i = 0; i < T; i++) v[i] = t0 + i < n ? v[i] : 0.0f;
    // the adjoint tails stage of section k - 1 on v, the gradient that enters it
    const FramePair h1 = frame_pair(a.prev_a1 + frame0, j), h2 = frame_pair(a.prev_a2 + frame0, j);
    const float pb1 = frame_at(a.prev_a1 + frame0, at_near, shift, inv_hop);
    const float pb2_near = frame_at(a.prev_a2 + frame0, at_near, shift, inv_hop), pb2_far = frame_at(a.prev_a2 + frame0, at_far, shift, inv_hop);
    float y1 = 0.0f, y2 = 0.0f, u1 = 1.0f, u2 = 0.0f, w1 = 0.0f, w2 = 1.0f;
#pragma unroll
    for (int s = 0; s < T; s++) {
        const int i = REV ? T - 1 - s : s;
        const float c1 = shifted_frame<REV, 1>(h1, k0, i, inv_hop, pb1, pb1, n, t0);
        const float c2 = shifted_frame<REV, 2>(h2, k0, i, inv_hop, pb2_near, pb2_far, n, t0);
        const float r = step2(c1, c2, v[i], y1, y2);
        const float u = step2(c1, c2, 0.0f, u1, u2);
        const float w = step2(c1, c2, 0.0f, w1, w2);
        y2 = y1; y1 = r; u2 = u1; u1 = u; w2 = w1; w1 = w;
    }
    store_tails<REV>(a.tails, a.n_lines, a.tiles, a.groups, line, g, t, y1, y2, u1, u2, w1, w2);
}

// one coefficient at audio rate: four samples per lane, which share an interval (hop is a multiple of 4)
__global__ void __launch_bounds__(kGradLanes) var2_expand_frames_kernel(Var2ExpandArgs a) {
    const int at = (blockIdx.x * kGradLanes + threadIdx.x) * 4;      // below 2^30 + 1024
    if (at >= a.n) return;
    const FramePair p = frame_pair(a.frames + (int64_t)blockIdx.y * a.frame_stride, at >> a.hop_shift);
    const int k = at & ((1 << a.hop_shift) - 1);
    *reinterpret_cast<float4 *>(a.out + (int64_t)blockIdx.y * a.stride + at) =
        make_float4(frame_lerp(p, k, a.inv_hop), frame_lerp(p, k + 1, a.inv_hop), frame_lerp(p, k + 2, a.inv_hop), frame_lerp(p, k + 3, a.inv_hop));
}

// The gradients of the section behind its adjoint scan.  grad_in: var2_biquad_grad_kernel's expression, the taps one and two
// samples along the forward's direction from frame_at.  FRAMES: that kernel's five per-sample coefficient gradients -- the same
// products and selects, rounded to f32 -- weighted by 1 - k / hop (S0, to the interval's first frame) and k / hop (S1, to its
// second) and summed in f64, where every product is exact: a lane in the order of its four samples, the lanes of a piece of
// min(hop, 1024) samples by a fixed tree -- shuffles within a wave, then the piece's first lane over its waves' sums in order.
// COEF_ONLY (var2_frames_coef_1d): the FRAMES half alone, for a section whose input gradient var2_adj_frames_link_keep_1d has
// formed -- the same products, the same sums in the same order, from lam, x and y; no tap is read and grad_in is not written.
// STREAM: the section's history -- pairs a.pair (its input's) and a.pair + 1 (its result's) of a.state_in -- stands where the
// forward read it, in place of the 0 beyond the line, and the six slots masked elsewhere are live; the gradient of the input's
// leaving pair (pair 0 of a.grad_state_out) is added to the two last samples of grad_in.
template <bool CAUSAL, bool FRAMES, bool COEF_ONLY = false, bool STREAM = false>
__global__ void __launch_bounds__(kGradLanes) var2_frames_grad_kernel(Var2FramesGradArgs a) {
    static_assert(!COEF_ONLY || FRAMES, "the sums are what is left");
    static_assert(kGradLanes * 4 == kVar2GradBlock, "a workgroup's samples");
    __shared__ double sums[kGradLanes / 64][kVar2FrameSums];
    const int n = a.n;
    const int at = (blockIdx.x * kGradLanes + threadIdx.x) * 4;      // below 2^30 + 1024
    const bool inside = at < n;
    if (!FRAMES && !inside) return;
    const int64_t first = (int64_t)blockIdx.y * a.stride, frame0 = (int64_t)blockIdx.y * a.frame_stride;
    const int shift = a.hop_shift;
    const float inv_hop = a.inv_hop;
    constexpr int L0 = CAUSAL ? 0 : 2;      // sample at + k in a window that looks where the adjoint looks
    constexpr int X0 = CAUSAL ? 2 : 0;      // and in one that looks where the forward looked
    float lam[6] = {};
    double s[kVar2FrameSums] = {};
    if (inside) {
        if constexpr (COEF_ONLY) {
            const float4 q = *reinterpret_cast<const float4 *>(a.lam + first + at);
            lam[L0] = q.x; lam[L0 + 1] = q.y; lam[L0 + 2] = q.z; lam[L0 + 3] = q.w;
        } else {
            load_six<CAUSAL>(a.lam + first, at, n, lam);
            float gx[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int one = CAUSAL ? at + k + 1 : at + k - 1, two = CAUSAL ? at + k + 2 : at + k - 2;
                const int i1 = CAUSAL ? L0 + k + 1 : L0 + k - 1, i2 = CAUSAL ? L0 + k + 2 : L0 + k - 2;
                const float t0 = frame_at(a.b0 + frame0, at + k, shift, inv_hop);
                const float t1 = frame_at(a.b1 + frame0, max(min(one, n - 1), 0), shift, inv_hop);
                const float t2 = frame_at(a.b2 + frame0, max(min(two, n - 1), 0), shift, inv_hop);
                const float c1 = (one < 0 || one >= n) ? 0.0f : t1, c2 = (two < 0 || two >= n) ? 0.0f : t2;
                gx[k] = __builtin_fmaf(c2, lam[i2], __builtin_fmaf(c1, lam[i1], t0 * lam[L0 + k]));
            }
            if constexpr (STREAM) {
                if (a.grad_state_out && at == (CAUSAL ? n - 4 : 0)) {      // the forward's two last samples
                    const float *pair = a.grad_state_out + (int64_t)blockIdx.y * a.state_stride;
                    gx[CAUSAL ? 3 : 0] += pair[0];
                    gx[CAUSAL ? 2 : 1] += pair[1];
                }
            }
            *reinterpret_cast<float4 *>(a.grad_in + first + at) = make_float4(gx[0], gx[1], gx[2], gx[3]);
        }
        if constexpr (FRAMES) {
            float xs[6], ys[6];
            load_six<!CAUSAL>(a.x + first, at, n, xs);
            load_six<!CAUSAL>(a.y + first, at, n, ys);
            bool live = false;      // the history stands beyond the line: nothing is masked
            if constexpr (STREAM) {
                live = a.state_in != nullptr;
                if (live && at == (CAUSAL ? 0 : n - 4)) {      // the forward's two first samples
                    const float *pairs = a.state_in + (int64_t)blockIdx.y * a.state_stride + 2 * a.pair;
                    xs[CAUSAL ? 1 : 4] = pairs[0]; xs[CAUSAL ? 0 : 5] = pairs[1];
                    ys[CAUSAL ? 1 : 4] = pairs[2]; ys[CAUSAL ? 0 : 5] = pairs[3];
                }
            }
            const int k0 = at & ((1 << shift) - 1), hop = 1 << shift;
            const double scale = (double)inv_hop;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i1 = CAUSAL ? X0 + k - 1 : X0 + k + 1, i2 = CAUSAL ? X0 + k - 2 : X0 + k + 2;
                const bool no_one = !live && (CAUSAL ? at + k < 1 : at + k >= n - 1), no_two = !live && (CAUSAL ? at + k < 2 : at + k >= n - 2);
                const float l = lam[L0 + k];
                const float gc[5] = {l * xs[X0 + k], no_one ? 0.0f : l * xs[i1], no_two ? 0.0f : l * xs[i2],
                                     no_one ? 0.0f : -l * ys[i1], no_two ? 0.0f : -l * ys[i2]};
                const double w1 = (double)(k0 + k) * scale, w0 = (double)(hop - k0 - k) * scale;      // exact
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    s[2 * c] += w0 * (double)gc[c];
                    s[2 * c + 1] += w1 * (double)gc[c];
                }
            }
        }
    }
    if constexpr (FRAMES) {
        const int piece_lanes = min(1 << shift, kVar2GradBlock) / 4;      // 16 .. 256, a power of two
        const int wave_lanes = min(piece_lanes, 64);
        for (int off = wave_lanes >> 1; off >= 1; off >>= 1) {
#pragma unroll
            for (int q = 0; q < kVar2FrameSums; q++) s[q] += __shfl_down(s[q], off);
        }
        const int tid = threadIdx.x;
        if (piece_lanes > 64) {
            if ((tid & 63) == 0) {
#pragma unroll
                for (int q = 0; q < kVar2FrameSums; q++) sums[tid >> 6][q] = s[q];
            }
            __syncthreads();
        }
        if ((tid & (piece_lanes - 1)) == 0 && inside) {
            if (piece_lanes > 64) {
                for (int w = 1; w < piece_lanes / 64; w++) {
#pragma unroll
                    for (int q = 0; q < kVar2FrameSums; q++) s[q] += sums[(tid >> 6) + w][q];
                }
            }
            const int piece = at / (piece_lanes * 4);
            double *dst = a.slab + ((int64_t)blockIdx.y * a.pieces + piece) * kVar2FrameSums;
#pragma unroll
            for (int q = 0; q < kVar2FrameSums; q++) dst[q] = s[q];
        }
    }
}

// dL/dc_j = (the S0 of interval j's pieces, in order) + (the S1 of interval j - 1's pieces, in order), rounded once to f32.
// One lane per frame; a piece that begins beyond the line does not exist.  slab: the line's sums; grads: the line's five rows.
__device__ __forceinline__ void fold_frame(const double *slab, int j, int n_frames, int hop_shift, int pieces, float *const (&grads)[5]) {
    const int per_interval = max(1, (1 << hop_shift) / kVar2GradBlock);
    double own[5] = {}, before[5] = {};
    if (j + 1 < n_frames) {
        for (int p = j * per_interval; p < min((j + 1) * per_interval, pieces); p++) {
#pragma unroll
            for (int c = 0; c < 5; c++) own[c] += slab[(int64_t)p * kVar2FrameSums + 2 * c];
        }
    }
    if (j >= 1) {
        for (int p = (j - 1) * per_interval; p < min(j * per_interval, pieces); p++) {
#pragma unroll
            for (int c = 0; c < 5; c++) before[c] += slab[(int64_t)p * kVar2FrameSums + 2 * c + 1];
        }
    }
#pragma unroll
    for (int c = 0; c < 5; c++) grads[c][j] = (float)(own[c] + before[c]);
}

__global__ void __launch_bounds__(kGradLanes) var2_frames_fold_kernel(Var2FramesGradArgs a) {
    const int j = blockIdx.x * kGradLanes + threadIdx.x, line = blockIdx.y;
    if (j >= a.n_frames) return;
    const int64_t row = (int64_t)line * a.frame_stride;
    float *const grads[5] = {a.grad_b0 + row, a.grad_b1 + row, a.grad_b2 + row, a.grad_a1 + row, a.grad_a2 + row};
    fold_frame(a.slab + (int64_t)line * a.pieces * kVar2FrameSums, j, a.n_frames, a.hop_shift, a.pieces, grads);
}

// the fold of every section of a cascade: the section on gridDim.z, its sums and gradients from the argument struct
__global__ void __launch_bounds__(kGradLanes) var2_frames_fold_cascade_kernel(Var2FramesFoldCascadeArgs a) {
    const int j = blockIdx.x * kGradLanes + threadIdx.x, line = blockIdx.y, k = blockIdx.z;
    if (j >= a.n_frames) return;
    const int64_t row = (int64_t)line * a.frame_stride;
    float *const grads[5] = {a.grads[k][0] + row, a.grads[k][1] + row, a.grads[k][2] + row, a.grads[k][3] + row, a.grads[k][4] + row};
    fold_frame(a.slab + k * a.section_doubles + (int64_t)line * a.pieces * kVar2FrameSums, j, a.n_frames, a.hop_shift, a.pieces, grads);
}

int launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("launch of %s failed: %s", what, hipGetErrorString(e)); return RF_ERR_HIP; }
    return RF_OK;
}

template <bool FINAL>
int launch_pass(const Var2Args &a, hipStream_t stream) {
    const dim3 grid((unsigned)a.groups, (unsigned)a.n_lines), block(64);
    if (a.adjoint) {
        if (a.causal) hipLaunchKernelGGL((var2_signal_kernel<false, true, FINAL>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_signal_kernel<true, true, FINAL>), grid, block, 0, stream, a);
        return launched(FINAL ? "var2_adj_pass2_1d" : "var2_adj_tails_1d");
    }
    if (a.causal) hipLaunchKernelGGL((var2_signal_kernel<false, false, FINAL>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var2_signal_kernel<true, false, FINAL>), grid, block, 0, stream, a);
    return launched(FINAL ? "var2_pass2_1d" : "var2_tails_1d");
}

}  // namespace

int launch_var2_tails(const Var2Args &a, hipStream_t stream) { return launch_pass<false>(a, stream); }
int launch_var2_pass2(const Var2Args &a, hipStream_t stream) { return launch_pass<true>(a, stream); }

int launch_var2_carry(const Var2Args &a, hipStream_t stream) {
    const int lanes = std::min(kCarryLanes, (a.groups + 63) / 64 * 64);
    const dim3 grid((unsigned)a.n_lines), block((unsigned)lanes);
    if (a.causal) hipLaunchKernelGGL((var2_carry_kernel<false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var2_carry_kernel<true>), grid, block, 0, stream, a);
    return launched("var2_carry_1d");
}

int launch_var2_biquad_tails(const Var2Args &a, hipStream_t stream) {
    const dim3 grid((unsigned)a.groups, (unsigned)a.n_lines), block(64);
    if (a.causal) hipLaunchKernelGGL((var2_signal_kernel<false, false, false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var2_signal_kernel<true, false, false, true>), grid, block, 0, stream, a);
    return launched("var2_biquad_tails_1d");
}

int launch_var2_link(const Var2LinkArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)a.groups, (unsigned)a.n_lines), block(64);
    if (a.keep) {
        if (a.causal) hipLaunchKernelGGL((var2_link_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_link_kernel<true, true>), grid, block, 0, stream, a);
        return launched("var2_link_keep_1d");
    }
    if (a.causal) hipLaunchKernelGGL((var2_link_kernel<false, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var2_link_kernel<true, false>), grid, block, 0, stream, a);
    return launched("var2_link_1d");
}

int launch_var2_adj_link(const Var2AdjLinkArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)a.groups, (unsigned)a.n_lines), block(64);
    if (a.keep) {
        if (a.causal) hipLaunchKernelGGL((var2_adj_link_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_adj_link_kernel<true, true>), grid, block, 0, stream, a);
        return launched("var2_adj_link_keep_1d");
    }
    if (a.causal) hipLaunchKernelGGL((var2_adj_link_kernel<false, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var2_adj_link_kernel<true, false>), grid, block, 0, stream, a);
    return launched("var2_adj_link_1d");
}

int launch_var2_biquad_coef(const Var2BiquadGradArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n / 4 + kGradLanes - 1) / kGradLanes), (unsigned)a.n_lines), block(kGradLanes);
    if (a.causal) hipLaunchKernelGGL((var2_biquad_coef_kernel<true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var2_biquad_coef_kernel<false>), grid, block, 0, stream, a);
    return launched("var2_biquad_coef_1d");
}

int launch_var2_biquad_grad(const Var2BiquadGradArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n / 4 + kGradLanes - 1) / kGradLanes), (unsigned)a.n_lines), block(kGradLanes);
    if (a.causal) {
        if (a.with_coefficients) hipLaunchKernelGGL((var2_biquad_grad_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_biquad_grad_kernel<true, false>), grid, block, 0, stream, a);
    } else {
        if (a.with_coefficients) hipLaunchKernelGGL((var2_biquad_grad_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_biquad_grad_kernel<false, false>), grid, block, 0, stream, a);
    }
    return launched("var2_biquad_grad_1d");
}

int launch_var2_grad(const Var2GradArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n / 4 + kGradLanes - 1) / kGradLanes), (unsigned)a.n_lines), block(kGradLanes);
    if (a.causal) hipLaunchKernelGGL((var2_grad_kernel<true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var2_grad_kernel<false>), grid, block, 0, stream, a);
    return launched("var2_grad_1d");
}

int launch_var2_expand_frames(const Var2ExpandArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n / 4 + kGradLanes - 1) / kGradLanes), (unsigned)a.n_lines), block(kGradLanes);
    hipLaunchKernelGGL(var2_expand_frames_kernel, grid, block, 0, stream, a);
    return launched("var2_expand_frames_1d");
}

namespace {
template <bool FINAL>
int launch_frames_pass(const Var2FramesArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)a.groups, (unsigned)a.n_lines), block(64);
    if (a.adjoint && a.stream) {
        if (a.causal) hipLaunchKernelGGL((var2_frames_kernel<false, true, FINAL, false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_frames_kernel<true, true, FINAL, false, true>), grid, block, 0, stream, a);
        return launched(FINAL ? "var2_adj_frames_pass2_stream_1d" : "var2_adj_frames_tails_stream_1d");
    }
    if (a.adjoint) {
        if (a.causal) hipLaunchKernelGGL((var2_frames_kernel<false, true, FINAL>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_frames_kernel<true, true, FINAL>), grid, block, 0, stream, a);
        return launched(FINAL ? "var2_adj_frames_pass2_1d" : "var2_adj_frames_tails_1d");
    }
    if (a.state_in || a.state_out) {
        if constexpr (FINAL) {
            if (a.causal) hipLaunchKernelGGL((var2_frames_kernel<false, false, true, false, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((var2_frames_kernel<true, false, true, false, true>), grid, block, 0, stream, a);
            return launched("var2_frames_pass2_stream_1d");
        } else {
            if (a.causal) hipLaunchKernelGGL((var2_frames_kernel<false, false, false, true, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((var2_frames_kernel<true, false, false, true, true>), grid, block, 0, stream, a);
            return launched("var2_biquad_frames_tails_stream_1d");
        }
    }
    if constexpr (FINAL) {
        if (a.causal) hipLaunchKernelGGL((var2_frames_kernel<false, false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_frames_kernel<true, false, true>), grid, block, 0, stream, a);
        return launched("var2_frames_pass2_1d");
    } else {
        if (a.causal) hipLaunchKernelGGL((var2_frames_kernel<false, false, false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_frames_kernel<true, false, false, true>), grid, block, 0, stream, a);
        return launched("var2_biquad_frames_tails_1d");
    }
}
}  // namespace

int launch_var2_frames_tails(const Var2FramesArgs &a, hipStream_t stream) { return launch_frames_pass<false>(a, stream); }
int launch_var2_frames_pass2(const Var2FramesArgs &a, hipStream_t stream) { return launch_frames_pass<true>(a, stream); }

int launch_var2_frames_grad(const Var2FramesGradArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n / 4 + kGradLanes - 1) / kGradLanes), (unsigned)a.n_lines), block(kGradLanes);
    if (a.stream) {
        if (a.causal) {
            if (a.with_frames) hipLaunchKernelGGL((var2_frames_grad_kernel<true, true, false, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((var2_frames_grad_kernel<true, false, false, true>), grid, block, 0, stream, a);
        } else {
            if (a.with_frames) hipLaunchKernelGGL((var2_frames_grad_kernel<false, true, false, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((var2_frames_grad_kernel<false, false, false, true>), grid, block, 0, stream, a);
        }
        return launched("var2_biquad_frames_grad_stream_1d");
    }
    if (a.causal) {
        if (a.with_frames) hipLaunchKernelGGL((var2_frames_grad_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_frames_grad_kernel<true, false>), grid, block, 0, stream, a);
    } else {
        if (a.with_frames) hipLaunchKernelGGL((var2_frames_grad_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_frames_grad_kernel<false, false>), grid, block, 0, stream, a);
    }
    return launched("var2_biquad_frames_grad_1d");
}

int launch_var2_frames_fold(const Var2FramesGradArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n_frames + kGradLanes - 1) / kGradLanes), (unsigned)a.n_lines), block(kGradLanes);
    hipLaunchKernelGGL(var2_frames_fold_kernel, grid, block, 0, stream, a);
    return launched("var2_frames_fold_1d");
}

int launch_var2_frames_link(const Var2FramesLinkArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)a.groups, (unsigned)a.n_lines), block(64);
    if (a.state_in || a.state_out) {
        if (a.keep) {
            if (a.causal) hipLaunchKernelGGL((var2_frames_link_kernel<false, true, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((var2_frames_link_kernel<true, true, true>), grid, block, 0, stream, a);
            return launched("var2_frames_link_keep_stream_1d");
        }
        if (a.causal) hipLaunchKernelGGL((var2_frames_link_kernel<false, false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_frames_link_kernel<true, false, true>), grid, block, 0, stream, a);
        return launched("var2_frames_link_stream_1d");
    }
    if (a.keep) {
        if (a.causal) hipLaunchKernelGGL((var2_frames_link_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_frames_link_kernel<true, true>), grid, block, 0, stream, a);
        return launched("var2_frames_link_keep_1d");
    }
    if (a.causal) hipLaunchKernelGGL((var2_frames_link_kernel<false, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var2_frames_link_kernel<true, false>), grid, block, 0, stream, a);
    return launched("var2_frames_link_1d");
}

int launch_var2_adj_frames_link(const Var2AdjFramesLinkArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)a.groups, (unsigned)a.n_lines), block(64);
    if (a.stream) {
        if (a.keep) {
            if (a.causal) hipLaunchKernelGGL((var2_adj_frames_link_kernel<false, true, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((var2_adj_frames_link_kernel<true, true, true>), grid, block, 0, stream, a);
            return launched("var2_adj_frames_link_keep_stream_1d");
        }
        if (a.causal) hipLaunchKernelGGL((var2_adj_frames_link_kernel<false, false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_adj_frames_link_kernel<true, false, true>), grid, block, 0, stream, a);
        return launched("var2_adj_frames_link_stream_1d");
    }
    if (a.keep) {
        if (a.causal) hipLaunchKernelGGL((var2_adj_frames_link_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_adj_frames_link_kernel<true, true>), grid, block, 0, stream, a);
        return launched("var2_adj_frames_link_keep_1d");
    }
    if (a.causal) hipLaunchKernelGGL((var2_adj_frames_link_kernel<false, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var2_adj_frames_link_kernel<true, false>), grid, block, 0, stream, a);
    return launched("var2_adj_frames_link_1d");
}

int launch_var2_frames_coef(const Var2FramesGradArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n / 4 + kGradLanes - 1) / kGradLanes), (unsigned)a.n_lines), block(kGradLanes);
    if (a.stream) {
        if (a.causal) hipLaunchKernelGGL((var2_frames_grad_kernel<true, true, true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((var2_frames_grad_kernel<false, true, true, true>), grid, block, 0, stream, a);
        return launched("var2_frames_coef_stream_1d");
    }
    if (a.causal) hipLaunchKernelGGL((var2_frames_grad_kernel<true, true, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((var2_frames_grad_kernel<false, true, true>), grid, block, 0, stream, a);
    return launched("var2_frames_coef_1d");
}

int launch_var2_frames_fold_cascade(const Var2FramesFoldCascadeArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n_frames + kGradLanes - 1) / kGradLanes), (unsigned)a.n_lines, (unsigned)a.n_sections), block(kGradLanes);
    hipLaunchKernelGGL(var2_frames_fold_cascade_kernel, grid, block, 0, stream, a);
    return launched("var2_frames_fold_cascade_1d");
}

}  // namespace rf
