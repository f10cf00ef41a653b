// kernels_adjoint.h -- launchers of the backward of a plan of constant-coefficient scans (kernels_adjoint.hip, plan_adjoint.cpp).
#pragma once

#include "rf_internal.h"

namespace rf {

// One scan of the backward as the kernels see it.  A line has N samples `stride` elements apart; position r of the scan is
// element r of the line for a causal scan and element N-1-r for an anticausal one.
struct AdjGeom {
    int64_t total = 0;      // samples per plane
    int64_t N = 1;          // extent of the scanned dimension
    int64_t stride = 1;     // elements between neighbours along it
    int64_t width = 1;      // extent[0]
    int n_planes = 1;
    int causal = 1;
    int k = 1;              // feedback taps
};

struct AdjPlanes { const float *p[RF_MAX_PLANES]; };
struct AdjPlanesW { float *p[RF_MAX_PLANES]; };

// the clamp terms of a scan: t[r] = sum_{j >= r} a_j, gamma = c0 + t[0]
struct AdjClamp {
    double t[RF_MAX_ORDER];
    double gamma;
};

constexpr int kAdjMaxSlabs = 1024;                    // workgroups of coeff_grad: one slab of kAdjSlabDoubles each
constexpr int kAdjSlabDoubles = 1 + RF_MAX_ORDER;

// "coeff_grad": P[0] = sum mu[r] u[r], P[j+1] = sum_{r > j} mu[r] y[r-j-1] over every line of every plane, plus (clamp != null)
// the border terms of every line, in f64, one slab per workgroup; also stores gnext = c0 * mu (f32).  Returns the number of
// slabs written through n_slabs.
int launch_coeff_grad(const AdjPlanes &mu, const AdjPlanes &u, const AdjPlanes &y, const AdjPlanesW &gnext, float c0,
                      const AdjGeom &g, const AdjClamp *clamp, double *slabs, int *n_slabs, hipStream_t stream);
// "coeff_grad_sum": row[j] = the slabs' entries j summed in index order, j <= k; entries past the order are stored as 0.  One
// workgroup.
int launch_coeff_grad_sum(const double *slabs, int n_slabs, int k, double *row, hipStream_t stream);
// "adjoint_border": dst[first sample of the line] += t_0 m[0] + gamma sum_{1 <= r < k} t_r m[r],  m[r] = mu_scale * mu[r];
// touches the first k samples of every line of every plane.  mu == dst is allowed.
int launch_adjoint_border(const AdjPlanes &mu, const AdjPlanesW &dst, double mu_scale, const AdjGeom &g, const AdjClamp &clamp,
                          hipStream_t stream);

}  // namespace rf
