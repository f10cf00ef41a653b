// var_device.h -- the device functions the varying scans' kernels share (kernels_var.hip: images; kernels_var_signal.hip: long
// 1-D signals): the tile-local recurrences of a lane's 64 samples, forward and adjoint, the masks, the power form's weight, and
// the 16-byte loads with their transposition through LDS.  Everything is forced inline and lives in an anonymous namespace: each
// file that includes this holds its own copy and its kernels are what they were when the functions stood in that file.
#pragma once

#include "kernels_var.h"

namespace rf {

namespace {

constexpr int T = kVarTile;
constexpr int LDS_PITCH = T + 4;      // dwords: rows stay 16-byte aligned, lane l starts on bank 4 l

__device__ __forceinline__ float step(float w, float x, float prev) { return __builtin_fmaf(w, prev, (1.0f - w) * x); }

// The anticausal scan needs 1 - w[i+1], the causal one 1 - w[i]: left alone, the compiler keeps the 64 differences of one scan
// in registers for the next (and for the weight-only scans behind them) -- a wave less per SIMD.  Behind this fence it forms
// them again, one instruction per sample.  (An empty statement: it emits nothing and touches no memory.)
__device__ __forceinline__ void forget_differences(float (&w)[T + 1]) {
#pragma unroll
    for (int i = 0; i <= T; i++) asm volatile("" : "+v"(w[i]));
}

// tile-local tails; x: the tile's samples (destroyed), w: the masked weights w[t0 .. t1]
template <int MODE>
__device__ __forceinline__ void tile_tails(float (&x)[T], float (&w)[T + 1], bool weights_too, float (&out)[kVarComponents]) {
    // One sweep for the three that depend on the weights alone (plane 0 forms them; wave-uniform).  G = v_p[t0] is the
    // anticausal recurrence over p written out:  G = sum_i qq[i] * (1 - w[i+1]) * p[i],  qq[i] = w[t0+1] * ... * w[i]
    // (no array of p; exact for weights of 0 and 1).
    out[VAR_P1] = out[VAR_G] = out[VAR_P2] = 0.0f;
    if (weights_too) {
        float p = w[0], qq = 1.0f, g = 0.0f;
#pragma unroll
        for (int i = 0; i < T; i++) {
            if (i > 0) { p *= w[i]; qq *= w[i]; }
            if constexpr (MODE == VAR_PAIR) g = __builtin_fmaf(qq * (1.0f - w[i + 1]), p, g);
        }
        out[VAR_P1] = p;
        out[VAR_G] = g;
        out[VAR_P2] = qq * w[T];
        if constexpr (MODE != VAR_CAUSAL) forget_differences(w);
    }
    if constexpr (MODE != VAR_ANTICAUSAL) {
        float prev = 0.0f;
#pragma unroll
        for (int i = 0; i < T; i++) { x[i] = step(w[i], x[i], prev); prev = x[i]; }
        out[VAR_E1] = prev;
        if constexpr (MODE == VAR_PAIR) forget_differences(w);
    }
    if constexpr (MODE != VAR_CAUSAL) {
        float v = 0.0f;
#pragma unroll
        for (int i = T - 1; i >= 0; i--) v = step(w[i + 1], x[i], v);
        out[VAR_E2] = v;
    }
}

template <int MODE>
__device__ __forceinline__ void tile_final(float (&x)[T], float (&w)[T + 1], float c, float d) {
    if constexpr (MODE != VAR_ANTICAUSAL) {
        float prev = c;
#pragma unroll
        for (int i = 0; i < T; i++) { x[i] = step(w[i], x[i], prev); prev = x[i]; }
        if constexpr (MODE == VAR_PAIR) forget_differences(w);
    }
    if constexpr (MODE != VAR_CAUSAL) {
        float v = d;
#pragma unroll
        for (int i = T - 1; i >= 0; i--) { x[i] = step(w[i + 1], x[i], v); v = x[i]; }
    }
}

// ---- adjoint stages: MODE is the direction of the adjoint recurrence itself -----------------------------------------------------
__device__ __forceinline__ float adjoint_step(float w, float x, float prev) { return __builtin_fmaf(w, prev, x); }

// tile-local tails, zero entry: E and the product that carries the entry across the tile (the forward scans' P1 / P2, formed in
// their order of multiplication)
template <int MODE>
__device__ __forceinline__ void tile_tails_adjoint(const float (&x)[T], const float (&w)[T + 1], bool weights_too, float (&out)[kVarComponents]) {
    out[VAR_E1] = out[VAR_P1] = out[VAR_E2] = out[VAR_G] = out[VAR_P2] = 0.0f;
    if (weights_too) {
        float p = MODE == VAR_CAUSAL ? w[0] : 1.0f;
#pragma unroll
        for (int i = 1; i < T; i++) p *= w[i];
        if constexpr (MODE == VAR_CAUSAL) out[VAR_P1] = p;
        else out[VAR_P2] = p * w[T];
    }
    if constexpr (MODE == VAR_CAUSAL) {
        float prev = 0.0f;
#pragma unroll
        for (int i = 0; i < T; i++) prev = adjoint_step(w[i], x[i], prev);
        out[VAR_E1] = prev;
    } else {
        float v = 0.0f;
#pragma unroll
        for (int i = T - 1; i >= 0; i--) v = adjoint_step(w[i + 1], x[i], v);
        out[VAR_E2] = v;
    }
}

// x: the gradient that enters, replaced by the adjoint state (lam or mu)
template <int MODE>
__device__ __forceinline__ void tile_final_adjoint(float (&x)[T], const float (&w)[T + 1], float c, float d) {
    if constexpr (MODE == VAR_CAUSAL) {
        float prev = c;
#pragma unroll
        for (int i = 0; i < T; i++) { x[i] = adjoint_step(w[i], x[i], prev); prev = x[i]; }
    } else {
        float v = d;
#pragma unroll
        for (int i = T - 1; i >= 0; i--) { x[i] = adjoint_step(w[i + 1], x[i], v); v = x[i]; }
    }
}

// what the final pass stores for sample i: the state times the input gain of the FORWARD scan (the adjoint of a causal scan
// runs anticausally and scales by 1 - w[i]; the adjoint of an anticausal scan by 1 - w[i+1])
template <int MODE>
__device__ __forceinline__ float adjoint_result(const float (&x)[T], const float (&w)[T + 1], int i) {
    return (1.0f - w[MODE == VAR_ANTICAUSAL ? i : i + 1]) * x[i];
}

// samples and weights beyond the line's end, and the weight of element 0, selected away
__device__ __forceinline__ void mask_tile(float (&x)[T], float (&w)[T + 1], int t0, int n) {
#pragma unroll
    for (int i = 0; i < T; i++) x[i] = t0 + i < n ? x[i] : 0.0f;
#pragma unroll
    for (int i = 0; i <= T; i++) w[i] = (t0 + i == 0 || t0 + i >= n) ? 0.0f : w[i];
}

// exponents -> weights in place.  v_exp_f32: 1 ulp, exp2(-0) = 1, exp2(-inf) = 0; results below 2^-126 flush to 0 (such a
// weight couples nothing at f32 precision).  The product is a plain f32 multiply: what the tests' numpy yardstick forms.
__device__ __forceinline__ float power_weight(float d, float l) { return __builtin_amdgcn_exp2f(d * l); }

// request k of a lane: row (k * 64 + lane) / 16 of the tile, 16-byte chunk (k * 64 + lane) % 16 -- a wave instruction moves four
// rows of 256 contiguous bytes
__device__ __forceinline__ void request_tile(const float *plane, const VarArgs &a, int r0, int c0, float (&v)[T]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < T / 4; k++) {
        const int flat = k * 64 + lane;
        const int r = min(r0 + (flat >> 4), a.height - 1);
        const int c = min(c0 + (flat & 15) * 4, a.width - 4);      // (the width is a multiple of 4)
        const float4 q = *reinterpret_cast<const float4 *>(plane + (int64_t)r * a.width + c);
        v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
    }
}

// chunks as requested -> the lane's row of the tile
__device__ __forceinline__ void transpose_in(const float (&v)[T], float *lds, float (&row)[T]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < T / 4; k++) {
        const int flat = k * 64 + lane;
        *reinterpret_cast<float4 *>(lds + (flat >> 4) * LDS_PITCH + (flat & 15) * 4) = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < T / 4; k++) {
        const float4 q = *reinterpret_cast<const float4 *>(lds + lane * LDS_PITCH + k * 4);
        row[4 * k] = q.x; row[4 * k + 1] = q.y; row[4 * k + 2] = q.z; row[4 * k + 3] = q.w;
    }
    __syncthreads();
}

}  // namespace

}  // namespace rf
