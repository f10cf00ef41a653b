// plan_adjoint.h -- the backward of a plan of constant-coefficient scans (rf_plan_backward).
#pragma once

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "kernels_adjoint.h"
#include "plan.h"

namespace rf {

// One launch (a child plan's step over all planes, or one of the adjoint kernels) of a backward call.
struct AdjLaunch {
    std::string name;
    std::function<int()> run;       // launches on Adjoint::stream
};

// What the backward of one plan owns.  The two launch lists are built lazily, each by the first call that needs it:
//   plain   no coefficient gradients -- route 1 (zero border: ONE adjoint plan) or route 2 (clamped: per scan in reverse order a
//           single-scan zero-border child plan and "adjoint_border")
//   coeff   route 3 -- the forward scan by scan into plan-owned planes, then per scan in reverse order a unit-gain child plan,
//           "coeff_grad", "coeff_grad_sum" and (clamped) "adjoint_border"
// A host-only plan builds host-only children: the lists answer rf_plan_backward_num_kernels, nothing runs.
struct Adjoint {
    std::vector<std::unique_ptr<rf_plan>> children;
    std::vector<AdjLaunch> plain, coeff;
    bool plain_built = false, coeff_built = false;
    // workspace of route 3: scan outputs Y[s][plane], the mu planes, the slabs of coeff_grad
    std::vector<void *> owned;
    std::vector<std::vector<float *>> Y;
    std::vector<float *> M;
    double *slabs = nullptr;
    int n_slabs = 0;                                  // of the coeff_grad launch that ran last (stream order)
    bool workspace_ready = false;
    // per-call context
    const void *in[RF_MAX_PLANES] = {nullptr};
    const void *gout[RF_MAX_PLANES] = {nullptr};
    void *gin[RF_MAX_PLANES] = {nullptr};
    double *gcoeff = nullptr;
    hipStream_t stream = nullptr;
    ~Adjoint();
};

int plan_backward(rf_plan *plan, const void *const *in_planes, const void *const *grad_out_planes, void *const *grad_in_planes,
                  double *grad_coeffs, void *stream, bool timed, float *ms_out, const char **names_out, int capacity);
int plan_backward_num_kernels(rf_plan *plan, int with_coeffs);
size_t plan_backward_workspace_bytes(const rf_plan *plan, int with_coeffs);

}  // namespace rf
