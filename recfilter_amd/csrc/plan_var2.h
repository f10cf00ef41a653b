// plan_var2.h -- the plan behind the rf_var2_plan_* entry points: one time-varying second-order all-pole scan on dense f32
// signals (plan_var2.cpp; kernels_var2_signal.hip).
#pragma once

#include <string>
#include <vector>

#include "kernels_var2.h"
#include "run_support.h"

struct rf_var2_plan {
    int64_t length = 0, stride = 0;
    int n_lines = 1;
    bool causal = true;
    int device = 0;
    bool host_only = false;
    int64_t tiles = 0, groups = 0;
    // the one workspace: the tails (maps and aggregates), then the carries; written before it is read
    float *workspace = nullptr;
    int64_t tails_floats() const { return (int64_t)rf::kVar2Components * n_lines * (tiles + groups); }
    int64_t carry_floats() const { return (int64_t)2 * n_lines * groups; }
    size_t workspace_bytes() const { return (size_t)(tails_floats() + carry_floats()) * sizeof(float); }
    // samples from the first one of line 0 to behind the last one of the last line
    size_t span_bytes() const { return (size_t)((int64_t)(n_lines - 1) * stride + length) * sizeof(float); }
    std::vector<std::string> names;                  // rf_var2_plan_execute_timed
    std::vector<std::string> backward_names[2];      // without ([0]) and with ([1]) coefficient gradients
    // the direct-form-I section (rf_var2_plan_execute_biquad, rf_var2_plan_backward_biquad): the adjoint state of its all-pole half
    // lives in one signal of the plan's span, allocated by the first backward call
    float *lam = nullptr;
    std::vector<std::string> biquad_names, biquad_backward_names;
    ~rf_var2_plan();
};

namespace rf {
int build_var2_signal_plan(const rf_var2_signal_desc *desc, rf_var2_plan **out);
// ms_out == nullptr: plain asynchronous run; else every launch bracketed by events (capacity checked by the caller)
int run_var2_plan(rf_var2_plan *plan, const void *in, const void *a1, const void *a2, void *out, hipStream_t stream, float *ms_out);
int run_var2_backward(rf_var2_plan *plan, const void *a1, const void *a2, const void *out, const void *grad_out, void *grad_in, void *grad_a1,
                      void *grad_a2, hipStream_t stream, float *ms_out);
int run_var2_biquad(rf_var2_plan *plan, const void *in, const void *b0, const void *b1, const void *b2, const void *a1, const void *a2, void *out,
                    hipStream_t stream, float *ms_out);
int run_var2_biquad_backward(rf_var2_plan *plan, const void *in, const void *b0, const void *b1, const void *b2, const void *a1, const void *a2,
                             const void *out, const void *grad_out, void *grad_in, void *grad_b0, void *grad_b1, void *grad_b2, void *grad_a1,
                             void *grad_a2, hipStream_t stream, float *ms_out);
}  // namespace rf
