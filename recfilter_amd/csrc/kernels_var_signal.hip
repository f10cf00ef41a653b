// kernels_var_signal.hip -- the varying first-order scans of kernels_var.hip on ONE long line (rf_var_plan_create_signal): a dense
// f32 signal of N samples, N a multiple of 4 up to 2^30, with a weight signal of the same length.
//
// Two levels.  A lane owns a TILE of 64 consecutive samples with the 65 weights that couple them, exactly as in var_x_kernel; a
// workgroup of one wave owns a GROUP of 64 consecutive tiles: 4096 contiguous samples, 16 KiB per plane.  The loads and the
// transposition through LDS are var_x_kernel's with a row pitch of 64 samples -- a wave instruction moves 1024 contiguous bytes --
// and the masks are by GLOBAL sample index (sample 0's weight, everything from N on), not at row starts.  blockIdx.x is the
// group (up to 2^18), blockIdx.y the plane.
//
// The five tails of a tile (E1, P1, E2, G, P2; kernels_var.hip) form a monoid: for a sub-line A followed on its right by B
//   E1 = E1_B + P1_B E1_A            P1 = P1_B P1_A
//   E2 = E2_A + P2_A (E2_B + G_B E1_A)
//   G  = G_A  + P2_A G_B P1_A        P2 = P2_A P2_B                                   identity (0, 1, 0, 0, 1)
// so the carries that enter a tile follow from those that enter its group, (c_g, d_g), by an affine map the wave can form itself.
//
//   var_tails_1d    tile-local tails per lane (tile_tails), then two Kogge-Stone scans across the 64 lanes with __shfl_up /
//                   __shfl_down (no LDS): the prefix of (E1, P1) and the suffix of the whole tuple.  A lane stores the five
//                   coefficients of ITS map,  c_l = a_l + b_l c_g,   d_l = A_l + B_l c_g + C_l d_g   (a, A per image plane; b, B, C
//                   depend on the weights alone: plane 0 stores them), and one lane stores the group's aggregate tuple (lane 0 from
//                   the suffix scan; a causal stage, which has no suffix scan, lane 63 from the prefix scan).
//   var_carry_1d    the recurrences of var_carry over GROUPS, c forward, then d backward with the G c term: ONE workgroup per
//                   plane, up to 1024 lanes, sweeping the groups 1024 at a time in index order -- a wave scan, the waves' totals
//                   folded through LDS, the running carry kept in a register between sweeps.
//   var_pass2_1d    reloads the group, forms (c_l, d_l) from the stored map and the group's carries, RERUNS the recurrences
//                   (tile_final) and stores: weights of exactly 0 and 1 stay exact.
// No kernel waits on another workgroup: the dependencies of a stage are its launch boundaries, every sum has a fixed order, and
// a result is reproducible bit for bit.
//
// Workspace (VarArgs::tails, ::carry; `tiles` = ceil(N / 64), groups = ceil(tiles / 64)):
//   tails   [component][plane][tile]    the lanes' maps: a, b, A, B, C in the slots of E1, P1, E2, G, P2
//           [component][plane][group]   behind them, the groups' aggregate tuples
//   carry   [c, d][plane][group]
// Samples a partial group misses are loaded from a clamped address inside the signal and selected away (image 0, weight 0); a
// tile past the end then has the tails (0, 0, 0, 0, 0), which pass d = 0 to the left as the border does.  A workgroup has loaded
// its whole group before it stores: in == out is legal.
//
// The power form and the adjoint stages are the instantiations kernels_var.hip has: exponents become weights in registers before
// the masks; adjoint stages are single scans with unit input gain whose final pass stores the scaled state and, where asked, the
// state itself.  The weight gradient is var_grad_kernel<0, ...> of kernels_var.hip on a 1 x N plane.
#include "kernels_var.h"

#include "var_device.h"

#include <algorithm>

namespace rf {

namespace {

constexpr int kGroupTiles = kVarGroupTiles;        // tiles of a group: one per lane
constexpr int kGroupSamples = kGroupTiles * T;     // 4096
constexpr int kCarryLanes = 1024;                  // groups of a sweep of var_carry_1d

__device__ __forceinline__ int groups_of(const VarArgs &a) { return (a.tiles + kGroupTiles - 1) / kGroupTiles; }
__device__ __forceinline__ int64_t map_index(const VarArgs &a, int comp, int pl, int t) { return ((int64_t)comp * a.n_planes + pl) * a.tiles + t; }
__device__ __forceinline__ int64_t aggregate_index(const VarArgs &a, int comp, int pl, int g) {
    return (int64_t)kVarComponents * a.n_planes * a.tiles + ((int64_t)comp * a.n_planes + pl) * groups_of(a) + g;
}
__device__ __forceinline__ int64_t group_carry_index(const VarArgs &a, int which, int pl, int g) {
    return ((int64_t)which * a.n_planes + pl) * groups_of(a) + g;
}

// sub-line A followed on its right by B; a stage forms only the components its mode needs (the others stay the identity's)
template <int MODE>
__device__ __forceinline__ void compose(const float (&A)[kVarComponents], const float (&B)[kVarComponents], float (&r)[kVarComponents]) {
    float e1 = 0.0f, p1 = 1.0f, e2 = 0.0f, g = 0.0f, p2 = 1.0f;
    if constexpr (MODE != VAR_ANTICAUSAL) {
        e1 = __builtin_fmaf(B[VAR_P1], A[VAR_E1], B[VAR_E1]);
        p1 = B[VAR_P1] * A[VAR_P1];
    }
    if constexpr (MODE != VAR_CAUSAL) {
        float inner = B[VAR_E2];
        if constexpr (MODE == VAR_PAIR) {
            inner = __builtin_fmaf(B[VAR_G], A[VAR_E1], inner);
            g = __builtin_fmaf(A[VAR_P2] * B[VAR_G], A[VAR_P1], A[VAR_G]);
        }
        e2 = __builtin_fmaf(A[VAR_P2], inner, A[VAR_E2]);
        p2 = A[VAR_P2] * B[VAR_P2];
    }
    r[VAR_E1] = e1; r[VAR_P1] = p1; r[VAR_E2] = e2; r[VAR_G] = g; r[VAR_P2] = p2;
}

__device__ __forceinline__ void identity(float (&r)[kVarComponents]) {
    r[VAR_E1] = 0.0f; r[VAR_P1] = 1.0f; r[VAR_E2] = 0.0f; r[VAR_G] = 0.0f; r[VAR_P2] = 1.0f;
}

// From a lane's tile tails to the coefficients of its map and the group's aggregate.  MODE: what the recurrences couple --
// VAR_CAUSAL: (E1, P1) only, VAR_ANTICAUSAL: (E2, P2) only, VAR_PAIR: everything.
//   map[E1] = a, map[P1] = b, map[E2] = A, map[G] = B, map[P2] = C;   whole: valid in lane 0 (VAR_CAUSAL: in lane 63)
template <int MODE>
__device__ __forceinline__ void scan_group(const float (&own)[kVarComponents], float (&map)[kVarComponents], float (&whole)[kVarComponents]) {
    const int lane = threadIdx.x;
    float pre[kVarComponents], suf[kVarComponents], other[kVarComponents], next[kVarComponents];
    identity(map);
    map[VAR_P1] = 0.0f; map[VAR_P2] = 0.0f;      // (a mode's unused coefficients: 0, never read)
#pragma unroll
    for (int i = 0; i < kVarComponents; i++) pre[i] = suf[i] = own[i];
    if constexpr (MODE != VAR_ANTICAUSAL) {
        // inclusive prefix of (E1, P1): tiles 0 .. lane
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            identity(other);
            other[VAR_E1] = __shfl_up(pre[VAR_E1], k);
            other[VAR_P1] = __shfl_up(pre[VAR_P1], k);
            compose<VAR_CAUSAL>(other, pre, next);
            if (lane >= k) { pre[VAR_E1] = next[VAR_E1]; pre[VAR_P1] = next[VAR_P1]; }
        }
        // what enters this tile: the prefix of the lane before
        const float a = __shfl_up(pre[VAR_E1], 1), b = __shfl_up(pre[VAR_P1], 1);
        map[VAR_E1] = lane == 0 ? 0.0f : a;
        map[VAR_P1] = lane == 0 ? 1.0f : b;
    }
    if constexpr (MODE != VAR_CAUSAL) {
        // inclusive suffix of the tuple: tiles lane .. 63
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
#pragma unroll
            for (int i = 0; i < kVarComponents; i++) other[i] = __shfl_down(suf[i], k);
            compose<MODE>(suf, other, next);
            if (lane + k < 64) {
#pragma unroll
                for (int i = 0; i < kVarComponents; i++) suf[i] = next[i];
            }
        }
        // S = tiles lane+1 .. 63:  d_l = E2_S + G_S c_{l+1} + P2_S d_g,  c_{l+1} = pre.E1 + pre.P1 c_g
        float S[kVarComponents];
#pragma unroll
        for (int i = 0; i < kVarComponents; i++) S[i] = __shfl_down(suf[i], 1);
        if (lane == 63) identity(S);
        map[VAR_E2] = S[VAR_E2];
        map[VAR_G] = 0.0f;
        if constexpr (MODE == VAR_PAIR) {
            map[VAR_E2] = __builtin_fmaf(S[VAR_G], pre[VAR_E1], S[VAR_E2]);
            map[VAR_G] = S[VAR_G] * pre[VAR_P1];
        }
        map[VAR_P2] = S[VAR_P2];
    }
#pragma unroll
    for (int i = 0; i < kVarComponents; i++) whole[i] = MODE == VAR_CAUSAL ? pre[i] : suf[i];
}

// request k of a lane: the 16-byte chunk k * 64 + lane of the group -- request_tile (var_device.h) with a row pitch of 64
__device__ __forceinline__ void request_group(const float *signal, int n, int s0, float (&v)[T]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < T / 4; k++) {
        const int at = min(s0 + (k * 64 + lane) * 4, n - 4);      // (n is a multiple of 4, at least 4)
        const float4 q = *reinterpret_cast<const float4 *>(signal + at);
        v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
    }
}

// the lanes' tiles back through LDS to the group's chunks; a chunk is inside the signal or beyond it (n is a multiple of 4)
template <typename F>
__device__ __forceinline__ void store_group(float *lds, float *signal, int n, int s0, F value) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < T / 4; k++)
        *reinterpret_cast<float4 *>(lds + lane * LDS_PITCH + k * 4) = make_float4(value(4 * k), value(4 * k + 1), value(4 * k + 2), value(4 * k + 3));
    __syncthreads();
#pragma unroll
    for (int k = 0; k < T / 4; k++) {
        const int flat = k * 64 + lane;
        const int at = s0 + flat * 4;
        const float4 q = *reinterpret_cast<const float4 *>(lds + (flat >> 4) * LDS_PITCH + (flat & 15) * 4);
        if (at < n) *reinterpret_cast<float4 *>(signal + at) = q;
    }
}

template <int MODE, bool FINAL, bool POWER, bool ADJ>
__global__ void __launch_bounds__(64) var_signal_kernel(VarArgs a) {
    static_assert(!ADJ || MODE != VAR_PAIR, "adjoint stages: single scans");
    __shared__ __attribute__((aligned(16))) float lds[T * LDS_PITCH];
    const int lane = threadIdx.x;
    const int g = blockIdx.x, pl = blockIdx.y;
    const int n = a.width;
    const int s0 = g * kGroupSamples;                 // below 2^30 + 4096
    const int t = g * kGroupTiles + lane, t0 = t * T;
    const float *src = static_cast<const float *>(a.src[pl]);
    float vx[T], vw[T];
    request_group(src, n, s0, vx);
    request_group(a.weights, n, s0, vw);
    float w_next = 0.0f;                              // w[t1], the next tile's first weight
    if constexpr (MODE != VAR_CAUSAL || (ADJ && FINAL)) w_next = a.weights[min(t0 + T, n - 1)];
    float c = 0.0f, d = 0.0f;
    if constexpr (FINAL) {
        // the group's carries (wave-uniform) through the lane's map
        const int tt = min(t, a.tiles - 1);
        float c_g = 0.0f, d_g = 0.0f;
        if constexpr (MODE != VAR_ANTICAUSAL) {
            c_g = a.carry[group_carry_index(a, 0, pl, g)];
            c = __builtin_fmaf(a.tails[map_index(a, VAR_P1, 0, tt)], c_g, a.tails[map_index(a, VAR_E1, pl, tt)]);
        }
        if constexpr (MODE != VAR_CAUSAL) {
            d_g = a.carry[group_carry_index(a, 1, pl, g)];
            d = a.tails[map_index(a, VAR_E2, pl, tt)];
            if constexpr (MODE == VAR_PAIR) d = __builtin_fmaf(a.tails[map_index(a, VAR_G, 0, tt)], c_g, d);
            d = __builtin_fmaf(a.tails[map_index(a, VAR_P2, 0, tt)], d_g, d);
        }
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
    mask_tile(x, w, t0, n);                           // by global index: t0 is the tile's first sample of the SIGNAL
    __builtin_amdgcn_sched_barrier(0);      // (the scans stay behind the transposition: they would hold its registers)
    if constexpr (FINAL) {
        float *dst = static_cast<float *>(a.dst[pl]);
        if constexpr (ADJ) {
            tile_final_adjoint<MODE>(x, w, c, d);
            store_group(lds, dst, n, s0, [&](int i) { return adjoint_result<MODE>(x, w, i); });
            float *lam = static_cast<float *>(a.lam[pl]);
            if (lam) {                                // (uniform)
                __syncthreads();
                store_group(lds, lam, n, s0, [&](int i) { return x[i]; });
            }
        } else {
            tile_final<MODE>(x, w, c, d);
            store_group(lds, dst, n, s0, [&](int i) { return x[i]; });
        }
    } else {
        float out[kVarComponents], map[kVarComponents], whole[kVarComponents];
        if constexpr (ADJ) tile_tails_adjoint<MODE>(x, w, true, out);
        else tile_tails<MODE>(x, w, true, out);
        // (what a mode leaves unset: the identity's; never read by that mode's scans)
        if constexpr (MODE == VAR_ANTICAUSAL) { out[VAR_E1] = 0.0f; out[VAR_P1] = 1.0f; }
        if constexpr (MODE == VAR_CAUSAL) { out[VAR_E2] = 0.0f; out[VAR_P2] = 1.0f; }
        if constexpr (MODE != VAR_PAIR) out[VAR_G] = 0.0f;
        scan_group<MODE>(out, map, whole);
        if (t < a.tiles) {
            if constexpr (MODE != VAR_ANTICAUSAL) a.tails[map_index(a, VAR_E1, pl, t)] = map[VAR_E1];
            if constexpr (MODE != VAR_CAUSAL) a.tails[map_index(a, VAR_E2, pl, t)] = map[VAR_E2];
            if (pl == 0) {
                if constexpr (MODE != VAR_ANTICAUSAL) a.tails[map_index(a, VAR_P1, 0, t)] = map[VAR_P1];
                if constexpr (MODE == VAR_PAIR) a.tails[map_index(a, VAR_G, 0, t)] = map[VAR_G];
                if constexpr (MODE != VAR_CAUSAL) a.tails[map_index(a, VAR_P2, 0, t)] = map[VAR_P2];
            }
        }
        if (lane == (MODE == VAR_CAUSAL ? 63 : 0)) {
            if constexpr (MODE != VAR_ANTICAUSAL) a.tails[aggregate_index(a, VAR_E1, pl, g)] = whole[VAR_E1];
            if constexpr (MODE != VAR_CAUSAL) a.tails[aggregate_index(a, VAR_E2, pl, g)] = whole[VAR_E2];
            if (pl == 0) {
                if constexpr (MODE != VAR_ANTICAUSAL) a.tails[aggregate_index(a, VAR_P1, 0, g)] = whole[VAR_P1];
                if constexpr (MODE == VAR_PAIR) a.tails[aggregate_index(a, VAR_G, 0, g)] = whole[VAR_G];
                if constexpr (MODE != VAR_CAUSAL) a.tails[aggregate_index(a, VAR_P2, 0, g)] = whole[VAR_P2];
            }
        }
    }
}

// ---- carries over groups: one workgroup per plane -----------------------------------------------------------------------------
// A sweep takes blockDim.x groups, lane i group base + i, in BOTH recurrences: the lane that stored c_g is the lane that reads it
// for the G c term.  Within a sweep: an inclusive wave scan of the affine maps (e, p): v -> e + p v, the waves' totals through LDS,
// every lane folding the totals of the waves before it (behind it, in the backward recurrence) onto the running carry -- at most
// 16 steps -- and all of them onto the next sweep's.  Lanes past the last group hold the identity.
template <int MODE>
__global__ void __launch_bounds__(kCarryLanes) var_carry_signal_kernel(VarArgs a) {
    __shared__ float lds_e[kCarryLanes / 64], lds_p[kCarryLanes / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6, span = blockDim.x;
    const int pl = blockIdx.x, G = groups_of(a);
    const float *tails = a.tails;
    float *carry = a.carry;
    if constexpr (MODE != VAR_ANTICAUSAL) {
        float run = 0.0f;                             // c entering the sweep's first group
        for (int base = 0; base < G; base += span) {
            const int g = base + tid, gg = min(g, G - 1);
            float e = tails[aggregate_index(a, VAR_E1, pl, gg)], p = tails[aggregate_index(a, VAR_P1, 0, gg)];
            if (g >= G) { e = 0.0f; p = 1.0f; }
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                const float eu = __shfl_up(e, k), pu = __shfl_up(p, k);
                if (lane >= k) { e = __builtin_fmaf(p, eu, e); p = p * pu; }
            }
            if (lane == 63) { lds_e[wave] = e; lds_p[wave] = p; }
            __syncthreads();
            float enter = run, next = run;            // enter: c entering this wave's first group
            for (int w = 0; w < waves; w++) {
                next = __builtin_fmaf(lds_p[w], next, lds_e[w]);
                if (w + 1 == wave) enter = next;
            }
            float ee = __shfl_up(e, 1), pe = __shfl_up(p, 1);
            if (lane == 0) { ee = 0.0f; pe = 1.0f; }
            if (g < G) carry[group_carry_index(a, 0, pl, g)] = __builtin_fmaf(pe, enter, ee);
            run = next;
            __syncthreads();
        }
    }
    if constexpr (MODE != VAR_CAUSAL) {
        float run = 0.0f;                             // d entering the sweep's last group from the right
        for (int base = (G - 1) / span * span; base >= 0; base -= span) {
            const int g = base + tid, gg = min(g, G - 1);
            float e = tails[aggregate_index(a, VAR_E2, pl, gg)], p = tails[aggregate_index(a, VAR_P2, 0, gg)];
            if constexpr (MODE == VAR_PAIR) e = __builtin_fmaf(tails[aggregate_index(a, VAR_G, 0, gg)], carry[group_carry_index(a, 0, pl, gg)], e);
            if (g >= G) { e = 0.0f; p = 1.0f; }
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                const float ed = __shfl_down(e, k), pd = __shfl_down(p, k);
                if (lane + k < 64) { e = __builtin_fmaf(p, ed, e); p = p * pd; }
            }
            if (lane == 0) { lds_e[wave] = e; lds_p[wave] = p; }
            __syncthreads();
            float enter = run, next = run;            // enter: d entering this wave's last group from the right
            for (int w = waves - 1; w >= 0; w--) {
                next = __builtin_fmaf(lds_p[w], next, lds_e[w]);
                if (w == wave + 1) enter = next;
            }
            float ee = __shfl_down(e, 1), pe = __shfl_down(p, 1);
            if (lane == 63) { ee = 0.0f; pe = 1.0f; }
            if (g < G) carry[group_carry_index(a, 1, pl, g)] = __builtin_fmaf(pe, enter, ee);
            run = next;
            __syncthreads();
        }
    }
}

int launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("launch of %s failed: %s", what, hipGetErrorString(e)); return RF_ERR_HIP; }
    return RF_OK;
}

int host_groups(const VarArgs &a) { return (a.tiles + kGroupTiles - 1) / kGroupTiles; }

template <bool FINAL>
int launch_pass(const VarArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)host_groups(a), (unsigned)a.n_planes), block(64);
    if (a.adjoint) {
        const char *what = FINAL ? "var_adj_pass2_1d" : "var_adj_tails_1d";
        if (a.mode == VAR_PAIR) { set_error("%s: adjoint stages are single scans", what); return RF_ERR_UNSUPPORTED; }
#define RF_VAR_SIGNAL_ADJOINT(MODE)                                                                               \
        if (a.power) hipLaunchKernelGGL((var_signal_kernel<MODE, FINAL, true, true>), grid, block, 0, stream, a);  \
        else hipLaunchKernelGGL((var_signal_kernel<MODE, FINAL, false, true>), grid, block, 0, stream, a)
        if (a.mode == VAR_CAUSAL) { RF_VAR_SIGNAL_ADJOINT(VAR_CAUSAL); } else { RF_VAR_SIGNAL_ADJOINT(VAR_ANTICAUSAL); }
#undef RF_VAR_SIGNAL_ADJOINT
        return launched(what);
    }
#define RF_VAR_SIGNAL(MODE)                                                                                        \
    if (a.power) hipLaunchKernelGGL((var_signal_kernel<MODE, FINAL, true, false>), grid, block, 0, stream, a);      \
    else hipLaunchKernelGGL((var_signal_kernel<MODE, FINAL, false, false>), grid, block, 0, stream, a)
    switch (a.mode) {
        case VAR_CAUSAL: RF_VAR_SIGNAL(VAR_CAUSAL); break;
        case VAR_ANTICAUSAL: RF_VAR_SIGNAL(VAR_ANTICAUSAL); break;
        default: RF_VAR_SIGNAL(VAR_PAIR); break;
    }
#undef RF_VAR_SIGNAL
    return launched(FINAL ? "var_pass2_1d" : "var_tails_1d");
}

}  // namespace

int launch_var_signal_tails(const VarArgs &a, hipStream_t stream) { return launch_pass<false>(a, stream); }
int launch_var_signal_pass2(const VarArgs &a, hipStream_t stream) { return launch_pass<true>(a, stream); }

int launch_var_signal_carry(const VarArgs &a, hipStream_t stream) {
    const int lanes = std::min(kCarryLanes, (host_groups(a) + 63) / 64 * 64);
    const dim3 grid((unsigned)a.n_planes), block((unsigned)lanes);
    switch (a.mode) {
        case VAR_CAUSAL: hipLaunchKernelGGL((var_carry_signal_kernel<VAR_CAUSAL>), grid, block, 0, stream, a); break;
        case VAR_ANTICAUSAL: hipLaunchKernelGGL((var_carry_signal_kernel<VAR_ANTICAUSAL>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((var_carry_signal_kernel<VAR_PAIR>), grid, block, 0, stream, a); break;
    }
    return launched("var_carry_1d");
}

}  // namespace rf
