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
    // a cascade's backward (rf_var2_plan_backward_cascade) with two sections or more: `cascade_spans` further signals of the
    // plan's span in one allocation -- the gradient between two sections, then the results of all sections but the last --
    // allocated by the first such call and regrown when a later one asks for more sections.  rf_var2_plan_backward_cascade_kept
    // uses the first span alone (the gradient between two sections) and allocates one span where there is none
    float *cascade = nullptr;
    int cascade_spans = 0;
    // the section on control-rate frames (rf_var2_plan_backward_biquad_frames): lam above, and the slab of f64 partial sums its
    // frame gradients are folded from -- 10 doubles per piece of min(hop, 1024) samples -- allocated by the first call that
    // asks for frame gradients and regrown when a later one has a smaller hop
    double *frames_slab = nullptr;
    size_t frames_slab_bytes = 0;
    size_t frames_slab_needed(int hop) const { return (size_t)n_lines * (size_t)rf::var2_frames_pieces(length, hop) * rf::kVar2FrameSums * sizeof(double); }
    std::vector<std::string> frames_names, frames_backward_names[2];      // [1]: with frame gradients
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
// the section with its five coefficients as control-rate frames: [line][n_frames] f32, frame j at sample j * hop
inline bool var2_hop_ok(int hop) { return hop >= 64 && hop <= 65536 && (hop & (hop - 1)) == 0; }
inline int var2_frames_count(int64_t length, int hop) { return var2_hop_ok(hop) && length >= 1 ? (int)((length + hop - 1) / hop) + 1 : 0; }
int run_var2_expand_frames(const void *frames, int hop, int n_frames, int64_t frame_stride, int64_t length, int lines, int64_t stride, void *out,
                           hipStream_t stream);
int run_var2_biquad_frames(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int hop, int n_frames, int64_t frame_stride, void *out,
                           hipStream_t stream, float *ms_out);
int run_var2_biquad_frames_backward(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int hop, int n_frames, int64_t frame_stride,
                                    const void *out, const void *grad_out, void *grad_in, const rf_var2_section_grad *frame_grads,
                                    hipStream_t stream, float *ms_out, bool in_required = true);
// a cascade of n_sections direct-form-I sections: the launches' names (string literals), counts and the backward's memory
const char *var2_cascade_name(int n_sections, size_t i);
const char *var2_cascade_backward_name(int n_sections, size_t i);
inline int var2_cascade_launches(int n_sections) { return 2 * n_sections + 1; }
inline int var2_cascade_backward_launches(int n_sections) { return n_sections == 1 ? 4 : 6 * n_sections - 1; }
inline size_t var2_cascade_backward_bytes(const rf_var2_plan *plan, int n_sections) {
    return plan->span_bytes() * (size_t)(n_sections == 1 ? 1 : n_sections + 1);
}
int run_var2_cascade(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections, void *out, hipStream_t stream,
                     float *ms_out, const char **names_out, int capacity, bool timed);
int run_var2_cascade_backward(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections, const void *out,
                              const void *grad_out, void *grad_in, const rf_var2_section_grad *grads, hipStream_t stream, float *ms_out,
                              const char **names_out, int capacity, bool timed);
// the cascade whose forward keeps every section's result in signals of the caller's (kept: n_sections - 1 of them), and the
// backward on them: no rerun, one adjoint link launch per boundary; the plan owns lam and, for two sections or more, the first
// span of `cascade` (the gradient between two sections)
const char *var2_cascade_keep_name(int n_sections, size_t i);
const char *var2_cascade_kept_backward_name(int n_sections, bool with_coefficients, size_t i);
inline int var2_cascade_kept_backward_launches(int n_sections, bool with_coefficients) {
    return with_coefficients ? 3 * n_sections + 1 : 2 * n_sections + 2;
}
inline size_t var2_cascade_kept_backward_bytes(const rf_var2_plan *plan, int n_sections) {
    return plan->span_bytes() * (size_t)(n_sections == 1 ? 1 : 2);
}
int run_var2_cascade_keep(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections, void *out, void *const *kept,
                          hipStream_t stream, float *ms_out, const char **names_out, int capacity, bool timed);
int run_var2_cascade_kept_backward(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections, const void *const *kept,
                                   const void *out, const void *grad_out, void *grad_in, const rf_var2_section_grad *grads, hipStream_t stream,
                                   float *ms_out, const char **names_out, int capacity, bool timed);
// the cascade on control-rate frames: frames[k] = section k's five frame arrays, one hop, n_frames and frame_stride for all;
// kept null: the plain link, else n_sections - 1 signals of the caller's.  The backward runs on the kept signals; the plan owns
// lam, the first span of `cascade` and, with frame gradients, n_sections slabs in frames_slab.  One section: the calls above.
const char *var2_cascade_frames_name(const rf_var2_plan *plan, int n_sections, bool keep, size_t i);
const char *var2_cascade_frames_backward_name(const rf_var2_plan *plan, int n_sections, bool with_frames, size_t i);
inline int var2_cascade_frames_launches(int n_sections) { return n_sections == 1 ? 3 : 2 * n_sections + 1; }
inline int var2_cascade_frames_backward_launches(int n_sections, bool with_frames) {
    return n_sections == 1 ? (with_frames ? 5 : 4) : with_frames ? 3 * n_sections + 2 : 2 * n_sections + 2;
}
inline size_t var2_cascade_frames_backward_bytes(const rf_var2_plan *plan, int n_sections, int hop) {
    return plan->span_bytes() * (size_t)(n_sections == 1 ? 1 : 2) + (size_t)n_sections * plan->frames_slab_needed(hop);
}
// state (rf_var2_plan_execute_cascade_frames_stream): [line][n_sections + 1][2] f32, `stride` floats from line to line; in null:
// zeros enter; out null: not wanted; state null or both pointers null: the call without a state, its launches, names and bits
struct Var2State {
    const void *in;
    void *out;
    int64_t stride;
};
const char *var2_cascade_frames_stream_name(int n_sections, bool keep, size_t i);
inline int var2_cascade_frames_stream_launches(int n_sections) { return 2 * n_sections + 1; }
int run_var2_cascade_frames(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int n_sections, int hop, int n_frames,
                            int64_t frame_stride, void *out, void *const *kept, hipStream_t stream, float *ms_out, const char **names_out,
                            int capacity, bool timed, const Var2State *state = nullptr);
// state (rf_var2_plan_backward_cascade_frames_stream): the state that entered the forward (read for the frame gradients alone),
// the gradient of the state that left it (null: zeros) and the gradient of the state that entered (null: not wanted), all laid
// out like the state; state null or every pointer null: the call without a state
struct Var2GradState {
    const void *in;
    const void *grad_out;
    void *grad_in;
    int64_t stride;
};
const char *var2_cascade_frames_stream_backward_name(int n_sections, bool with_frames, size_t i);
inline int var2_cascade_frames_stream_backward_launches(int n_sections, bool with_frames) { return with_frames ? 3 * n_sections + 2 : 2 * n_sections + 2; }
int run_var2_cascade_frames_backward(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int n_sections, int hop, int n_frames,
                                     int64_t frame_stride, const void *const *kept, const void *out, const void *grad_out, void *grad_in,
                                     const rf_var2_section_grad *frame_grads, hipStream_t stream, float *ms_out, const char **names_out,
                                     int capacity, bool timed, const Var2GradState *state = nullptr);
}  // namespace rf
