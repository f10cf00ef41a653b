// kernels_adjoint.hip -- the kernels of rf_plan_backward that are not a forward plan: the coefficient-gradient
// reduction of one scan and the border term of a clamped scan's transpose.  gfx950; f32 planes, f64 sums, no atomics.
//
// coeff_grad      one streaming pass over mu (the unit-gain transposed scan of the incoming gradient), u (the scan's input) and
//                 y (its output): P[0] = sum mu u, P[j+1] = sum_{r > j} mu[r] y[r-j-1].  A workgroup takes chunks of 1024
//                 consecutive samples of a plane, 16 bytes per lane; the shifted y of a scan along x comes from an LDS copy of
//                 the chunk with RF_MAX_ORDER samples either side, the shifted y of a scan along y / z from the row / plane
//                 stride.  Sums are f64 per lane, reduced through the wave (shuffles) and LDS, stored as ONE slab per workgroup.
//                 Under a clamped border the lanes of the grid then add the clamp terms of the lines, one line per lane and round.
// coeff_grad_sum  one workgroup: the slabs in index order (lane-strided, then a fixed tree).
// adjoint_border  one lane per line: the first k samples of the line, one store.
#include <algorithm>

#include "kernels_adjoint.h"

namespace rf {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4 * kThreads;      // samples of a plane per workgroup and round
constexpr int kHalo = RF_MAX_ORDER;

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// per-lane sums -> the workgroup's slab: wave by wave in lane order, then the waves in index order
template <int KMAX>
__device__ __forceinline__ void store_slab(double (&acc)[KMAX + 1], int k, double (*red)[KMAX + 1], double *slab) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int j = 0; j <= KMAX; j++) {
        const double s = wave_sum(acc[j]);
        if (lane == 0) red[wave][j] = s;
    }
    __syncthreads();
    if (tid < kAdjSlabDoubles) {
        double s = 0.0;
        if (tid <= k && tid <= KMAX)
            for (int w = 0; w < kThreads / 64; w++) s += red[w][tid];
        slab[tid] = s;
    }
}

// element of position r of line L (over all planes); *pl = the plane
__device__ __forceinline__ int64_t line_base(const AdjGeom &g, int64_t L, int *pl) {
    const int64_t lines = g.total / g.N;
    *pl = (int)(L / lines);
    const int64_t l = L % lines;
    return (l / g.stride) * g.stride * g.N + (l % g.stride);
}
__device__ __forceinline__ int64_t line_at(const AdjGeom &g, int64_t base, int r) {
    return base + (g.causal ? (int64_t)r : g.N - 1 - r) * g.stride;
}

// The clamp terms of the coefficient sums (plan_adjoint.cpp): per line beta = u[0] sum_{1<=r<k} t_r mu[r] for every entry, and
// mu[0] u[0] + y[0] sum_{1<=r<=j} mu[r] for feedback tap j.  Lines are dealt to the lanes of the grid in a fixed order.
template <int KMAX>
__device__ __forceinline__ void add_clamp_terms(double (&acc)[KMAX + 1], const AdjPlanes &mu, const AdjPlanes &u, const AdjPlanes &y,
                                                const AdjGeom &g, const AdjClamp &cl) {
    const int k = g.k;
    const int64_t n_lines = (g.total / g.N) * g.n_planes;
    for (int64_t L = (int64_t)blockIdx.x * kThreads + threadIdx.x; L < n_lines; L += (int64_t)gridDim.x * kThreads) {
        int pl;
        const int64_t base = line_base(g, L, &pl);
        const int64_t first = line_at(g, base, 0);
        const double u0 = (double)u.p[pl][first], m0 = (double)mu.p[pl][first], y0 = (double)y.p[pl][first];
        double beta = 0.0;
        for (int r = 1; r < k; r++) beta += cl.t[r] * (double)mu.p[pl][line_at(g, base, r)];
        beta *= u0;
        acc[0] += beta;
        double run = 0.0;                                   // sum_{1 <= r <= j} mu[r]
#pragma unroll
        for (int j = 0; j < KMAX; j++)
            if (j < k) {
                if (j >= 1) run += (double)mu.p[pl][line_at(g, base, j)];
                acc[j + 1] += beta + m0 * u0 + y0 * run;
            }
    }
}

template <int KMAX, bool DIM0>
__global__ __launch_bounds__(kThreads) void coeff_grad_vec_kernel(AdjPlanes mu, AdjPlanes u, AdjPlanes y, AdjPlanesW gnext, float c0,
                                                                   AdjGeom g, AdjClamp cl, int clamped, double *slabs) {
    __shared__ __align__(16) float ys[DIM0 ? kChunk + 2 * kHalo : 4];
    __shared__ double red[kThreads / 64][KMAX + 1];
    const int tid = threadIdx.x, k = g.k;
    const int64_t per_plane = (g.total + kChunk - 1) / kChunk, n_chunks = per_plane * g.n_planes;
    const int64_t sgn = g.causal ? 1 : -1;
    double acc[KMAX + 1];
#pragma unroll
    for (int j = 0; j <= KMAX; j++) acc[j] = 0.0;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int pl = (int)(c / per_plane);
        const int64_t base = (c % per_plane) * kChunk, e0 = base + 4 * tid;
        const bool live = e0 < g.total;                    // total is a multiple of 4: four samples are live together
        const float *yp = y.p[pl];
        if (DIM0) {
            __syncthreads();                               // the previous round has read its copy
            const float4 v = live ? *reinterpret_cast<const float4 *>(yp + e0) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(&ys[kHalo + 4 * tid]) = v;
            if (tid < 2 * kHalo) {
                const bool left = tid < kHalo;
                const int64_t idx = left ? base - kHalo + tid : base + kChunk + (tid - kHalo);
                ys[left ? tid : kChunk + tid] = (idx >= 0 && idx < g.total) ? yp[idx] : 0.0f;
            }
            __syncthreads();
        }
        if (live) {
            const float4 m4 = *reinterpret_cast<const float4 *>(mu.p[pl] + e0);
            const float4 u4 = *reinterpret_cast<const float4 *>(u.p[pl] + e0);
            *reinterpret_cast<float4 *>(gnext.p[pl] + e0) = make_float4(c0 * m4.x, c0 * m4.y, c0 * m4.z, c0 * m4.w);
            const float m[4] = {m4.x, m4.y, m4.z, m4.w}, uu[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
            for (int q = 0; q < 4; q++) acc[0] += (double)m[q] * (double)uu[q];
            if (DIM0) {
                const int64_t x0 = e0 % g.N;               // the width is a multiple of 4: the four samples share a row
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int64_t r = g.causal ? x0 + q : g.N - 1 - (x0 + q);
#pragma unroll
                    for (int j = 0; j < KMAX; j++)
                        if (j < k && r > j) acc[j + 1] += (double)m[q] * (double)ys[kHalo + 4 * tid + q - (int)sgn * (j + 1)];
                }
            } else {
                const int64_t i = (e0 / g.stride) % g.N;   // the stride is a multiple of 4: one position for the four
                const int64_t r = g.causal ? i : g.N - 1 - i;
#pragma unroll
                for (int j = 0; j < KMAX; j++)
                    if (j < k && r > j) {
                        const float4 y4 = *reinterpret_cast<const float4 *>(yp + e0 - sgn * (j + 1) * g.stride);
                        acc[j + 1] += (double)m[0] * (double)y4.x + (double)m[1] * (double)y4.y + (double)m[2] * (double)y4.z +
                                      (double)m[3] * (double)y4.w;
                    }
            }
        }
    }
    if (clamped) add_clamp_terms<KMAX>(acc, mu, u, y, g, cl);
    store_slab<KMAX>(acc, k, red, slabs + (size_t)blockIdx.x * kAdjSlabDoubles);
}

// any extents, element-aligned planes: one sample per lane and load
template <int KMAX>
__global__ __launch_bounds__(kThreads) void coeff_grad_scalar_kernel(AdjPlanes mu, AdjPlanes u, AdjPlanes y, AdjPlanesW gnext, float c0,
                                                                      AdjGeom g, AdjClamp cl, int clamped, double *slabs) {
    __shared__ double red[kThreads / 64][KMAX + 1];
    const int tid = threadIdx.x, k = g.k;
    const int64_t per_plane = (g.total + kChunk - 1) / kChunk, n_chunks = per_plane * g.n_planes;
    const int64_t sgn = g.causal ? 1 : -1;
    double acc[KMAX + 1];
#pragma unroll
    for (int j = 0; j <= KMAX; j++) acc[j] = 0.0;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int pl = (int)(c / per_plane);
        const int64_t base = (c % per_plane) * kChunk;
        const float *yp = y.p[pl];
        for (int q = 0; q < 4; q++) {
            const int64_t e = base + q * kThreads + tid;
            if (e >= g.total) continue;
            const float m = mu.p[pl][e];
            gnext.p[pl][e] = c0 * m;
            acc[0] += (double)m * (double)u.p[pl][e];
            const int64_t i = (e / g.stride) % g.N;
            const int64_t r = g.causal ? i : g.N - 1 - i;
#pragma unroll
            for (int j = 0; j < KMAX; j++)
                if (j < k && r > j) acc[j + 1] += (double)m * (double)yp[e - sgn * (j + 1) * g.stride];
        }
    }
    if (clamped) add_clamp_terms<KMAX>(acc, mu, u, y, g, cl);
    store_slab<KMAX>(acc, k, red, slabs + (size_t)blockIdx.x * kAdjSlabDoubles);
}

__global__ __launch_bounds__(kThreads) void coeff_grad_sum_kernel(const double *slabs, int n_slabs, int k, double *row) {
    __shared__ double red[kThreads / 64];
    const int tid = threadIdx.x;
    for (int j = 0; j <= k; j++) {
        double s = 0.0;
        for (int i = tid; i < n_slabs; i += kThreads) s += slabs[(size_t)i * kAdjSlabDoubles + j];
        s = wave_sum(s);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int w = 0; w < kThreads / 64; w++) t += red[w];
            row[j] = t;
        }
        __syncthreads();
    }
    for (int j = k + 1 + tid; j < kAdjSlabDoubles; j += kThreads) row[j] = 0.0;
}

__global__ __launch_bounds__(kThreads) void adjoint_border_kernel(AdjPlanes mu, AdjPlanesW dst, double mu_scale, AdjGeom g, AdjClamp cl) {
    const int64_t n_lines = (g.total / g.N) * g.n_planes;
    const int64_t L = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (L >= n_lines) return;
    int pl;
    const int64_t base = line_base(g, L, &pl);
    double tail = 0.0;
    for (int r = 1; r < g.k; r++) tail += cl.t[r] * (double)mu.p[pl][line_at(g, base, r)];
    const int64_t first = line_at(g, base, 0);
    const double add = mu_scale * (cl.t[0] * (double)mu.p[pl][first] + cl.gamma * tail);
    dst.p[pl][first] = (float)((double)dst.p[pl][first] + add);
}

bool aligned16(const AdjPlanes &a, int n) {
    for (int i = 0; i < n; i++)
        if (((uintptr_t)a.p[i] & 15u) != 0) return false;
    return true;
}

template <int KMAX>
int launch_bucket(const AdjPlanes &mu, const AdjPlanes &u, const AdjPlanes &y, const AdjPlanesW &gnext, float c0, const AdjGeom &g,
                  const AdjClamp &cl, int clamped, double *slabs, int blocks, bool vec, hipStream_t stream) {
    if (!vec)
        hipLaunchKernelGGL((coeff_grad_scalar_kernel<KMAX>), dim3(blocks), dim3(kThreads), 0, stream, mu, u, y, gnext, c0, g, cl, clamped, slabs);
    else if (g.stride == 1)
        hipLaunchKernelGGL((coeff_grad_vec_kernel<KMAX, true>), dim3(blocks), dim3(kThreads), 0, stream, mu, u, y, gnext, c0, g, cl, clamped, slabs);
    else
        hipLaunchKernelGGL((coeff_grad_vec_kernel<KMAX, false>), dim3(blocks), dim3(kThreads), 0, stream, mu, u, y, gnext, c0, g, cl, clamped, slabs);
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}

int coeff_grad_slabs(const AdjGeom &g) {
    const int64_t n_chunks = ((g.total + kChunk - 1) / kChunk) * g.n_planes;
    return (int)std::min<int64_t>(n_chunks, kAdjMaxSlabs);
}

}  // namespace

int launch_coeff_grad(const AdjPlanes &mu, const AdjPlanes &u, const AdjPlanes &y, const AdjPlanesW &gnext, float c0,
                      const AdjGeom &g, const AdjClamp *clamp, double *slabs, int *n_slabs, hipStream_t stream) {
    if (g.k < 1 || g.k > RF_MAX_ORDER || g.total < 1 || g.n_planes < 1 || g.n_planes > RF_MAX_PLANES) {
        set_error("coeff_grad: bad geometry");
        return RF_ERR_INVALID_ARG;
    }
    const int blocks = coeff_grad_slabs(g);
    *n_slabs = blocks;
    AdjPlanes gn;
    for (int i = 0; i < g.n_planes; i++) gn.p[i] = gnext.p[i];
    AdjClamp cl{};
    if (clamp) cl = *clamp;
    const int clamped = clamp ? 1 : 0;
    const bool vec = g.total % 4 == 0 && g.width % 4 == 0 && aligned16(mu, g.n_planes) && aligned16(u, g.n_planes) &&
                     aligned16(y, g.n_planes) && aligned16(gn, g.n_planes);
    if (g.k <= 1) return launch_bucket<1>(mu, u, y, gnext, c0, g, cl, clamped, slabs, blocks, vec, stream);
    if (g.k <= 2) return launch_bucket<2>(mu, u, y, gnext, c0, g, cl, clamped, slabs, blocks, vec, stream);
    if (g.k <= 3) return launch_bucket<3>(mu, u, y, gnext, c0, g, cl, clamped, slabs, blocks, vec, stream);
    if (g.k <= 8) return launch_bucket<8>(mu, u, y, gnext, c0, g, cl, clamped, slabs, blocks, vec, stream);
    return launch_bucket<RF_MAX_ORDER>(mu, u, y, gnext, c0, g, cl, clamped, slabs, blocks, vec, stream);      // the generic instance
}

int launch_coeff_grad_sum(const double *slabs, int n_slabs, int k, double *row, hipStream_t stream) {
    hipLaunchKernelGGL(coeff_grad_sum_kernel, dim3(1), dim3(kThreads), 0, stream, slabs, n_slabs, k, row);
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}

int launch_adjoint_border(const AdjPlanes &mu, const AdjPlanesW &dst, double mu_scale, const AdjGeom &g, const AdjClamp &clamp,
                          hipStream_t stream) {
    const int64_t n_lines = (g.total / g.N) * g.n_planes;
    const int64_t blocks = (n_lines + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(adjoint_border_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, mu, dst, mu_scale, g, clamp);
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}

}  // namespace rf
