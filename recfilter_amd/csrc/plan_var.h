// plan_var.h -- the plan behind the rf_var_plan_* entry points: spatially varying first-order scans (plan_var.cpp).
#pragma once

#include <string>
#include <vector>

#include "kernels_var.h"
#include "run_support.h"

// One stage = one scan, or a causal scan directly followed by the anticausal scan of the same dimension and weight plane
// (where the two are all of a run along that dimension: plan_var.cpp).
struct rf_var_stage {
    int dim = 0;
    int mode = rf::VAR_CAUSAL;      // rf::VarMode
    int weights = 0;
};

struct rf_var_plan {
    int64_t width = 0, height = 0;
    int n_planes = 1, n_weights = 1;
    // images per launch (internal: rf_smooth_plan_create_batched; the public rf_var_plan_* entry points build 1).  Every workspace
    // below is `batch` times one image's, image after image, each in the single-image layout.
    int batch = 1;
    int device = 0;
    bool host_only = false;
    // one long 1-D signal (rf_var_plan_create_signal): width = its length, height = 1, every scan along dim 0; the stages run the
    // kernels of kernels_var_signal.hip and the workspace is sized for tiles plus groups of 64 tiles
    bool signal = false;
    // a volume (rf_var_plan_create_volume): planes are dense [z][y][x] volumes of width x height x depth samples and dim 2 scans
    // along z.  An x / y stage takes the `depth` slices as a batch (gridDim.z, slice strides of width * height samples, tails and
    // carries slice after slice in the single-image layout); a z stage runs the y kernels on the (width * height) x depth view,
    // one voxel column per lane.  `batch` stays 1: there is no batch of volumes.
    bool volume = false;
    int64_t depth = 1;
    int64_t plane_samples() const { return width * height * depth; }
    std::vector<rf_var_stage> stages;
    std::vector<std::string> names;          // three per stage: what rf_var_plan_execute_timed reports
    // the one workspace: every stage's tails and carries (sized for the larger dimension); written before it is read
    float *tails = nullptr, *carry = nullptr;
    size_t tails_bytes = 0, carry_bytes = 0;
    size_t workspace_bytes() const { return tails_bytes + carry_bytes; }
    int64_t image_tails_floats() const { return (int64_t)(tails_bytes / sizeof(float)) / batch; }
    int64_t image_carry_floats() const { return (int64_t)(carry_bytes / sizeof(float)) / batch; }
    // rf_var_plan_backward: the scans as described (adjoint stages are single scans), the launch names without ([0]) and with
    // ([1]) weight gradients, and the planes the weight gradients need -- every scan's output (n_scans * n_planes) and one
    // scan's adjoint state (n_planes) -- allocated by the first call that asks for a weight gradient.  [scan][image][plane]: the
    // planes of one scan are n_planes * width * height samples from image to image.
    std::vector<rf_var_scan_desc> scans;
    std::vector<std::string> backward_names[2];
    float *grad_planes = nullptr;
    size_t backward_workspace_bytes(bool with_weight_gradients) const {
        return with_weight_gradients ? (scans.size() + 1) * (size_t)batch * (size_t)n_planes * (size_t)plane_samples() * sizeof(float) : 0;
    }
    // rf_var_plan_backward_power_bases: backward_names[1] and "var_param_sum"; the f64 slabs of the base-reducing var_grad launches,
    // one entry per workgroup, scan q's at bases_slab_offset[q] (bases_slab_offset[n_scans]: their number) -- no two launches of a
    // call share an entry.  Allocated by the first call that needs them, freed with the plan.
    std::vector<std::string> backward_bases_names;
    std::vector<int64_t> bases_slab_offset;
    double *bases_slabs = nullptr;
    size_t bases_slab_bytes() const { return bases_slab_offset.empty() ? 0 : (size_t)bases_slab_offset.back() * sizeof(double); }
    ~rf_var_plan();
};

namespace rf {
// rf_var_plan_create, _create_signal (planes are dense f32 signals of desc->length samples) and _create_volume (dense f32 volumes): each
// description is lowered to an rf_var_desc and checked by the one validator as its kind
int build_var_plan(const rf_var_desc *desc, rf_var_plan **out, int batch = 1);
int build_var_signal_plan(const rf_var_signal_desc *desc, rf_var_plan **out);
int build_var_volume_plan(const rf_var_volume_desc *desc, rf_var_plan **out);
// what rf_var_plan_create_volume, the distances of a volume and rf_smooth_plan_create_volume refuse alike (the message names the limit):
// extents below 1 (RF_ERR_INVALID_ARG); a width that is no multiple of 4, an extent above 2^21, width * height above 2^30,
// depth * n_planes above 65535 (RF_ERR_UNSUPPORTED)
int check_volume_extents(int64_t width, int64_t height, int64_t depth, int32_t n_planes);

// The power form's constants: bases[k] inside (0, 1) for each of the n_weights planes, or a refusal; log2 and ln of each.
int power_constants(const float *bases, int n_weights, float *log2_base, float *ln_base);

// ms_out == nullptr: plain asynchronous execute; else every launch bracketed by events (capacity checked by the caller)
// bases == nullptr: `weight_planes` hold weights; else they hold exponents and bases[k] is the base of plane k (the power form)
int run_var_plan(rf_var_plan *plan, const void *const *in_planes, const void *const *weight_planes, const float *bases,
                 void *const *out_planes, hipStream_t stream, float *ms_out);
// The launches of one run of `plan`, nothing checked (run_var_plan and plan_smooth.cpp check first).  The first stage reads `in`
// (f32, or bytes: in_u8); the stages write `work` (f32) and later stages filter it in place; the final pass of the last stage
// stores to `out` (f32 -- then out is work -- or bytes: out_u8).  log2_base == nullptr: the plane form.  `timer` is marked behind
// every launch.  A batched plan: the arrays name image 0's planes and the strides are samples from image to image.
struct VarIo {
    const void *const *in = nullptr;
    void *const *work = nullptr, *const *out = nullptr;
    bool in_u8 = false, out_u8 = false;
    int64_t in_stride = 0, work_stride = 0, out_stride = 0, weights_stride = 0;
};
int launch_var_stages(rf_var_plan *plan, const VarIo &io, const void *const *weight_planes, const float *log2_base, hipStream_t stream,
                      LaunchTimer &timer);
// The adjoint of the plan (rf_var_plan_backward in recfilter_amd.h).  grad_weight_planes: nullptr, or n_weights entries, each nullptr
// (no gradient for that plane) or a plane.  ms_out as in run_var_plan, one slot per name of backward_names[with weight gradients].
// bases == nullptr: the plane form; else the power form (rf_var_plan_backward_power): `weight_planes` hold exponents and the
// gradient planes receive the gradient of the exponents.
// with_bases (rf_var_plan_backward_power_bases; the power form): the weight-gradient route whatever grad_weight_planes holds (it
// may be null), on the base-reducing var_grad instances, and one var_param_sum that stores dL/dbases[k] to grad_bases (device,
// n_weights doubles); ms_out then has one slot per name of backward_bases_names.
int run_var_backward(rf_var_plan *plan, const void *const *in_planes, const void *const *weight_planes, const float *bases,
                     const void *const *grad_out_planes, void *const *grad_in_planes, void *const *grad_weight_planes, hipStream_t stream,
                     float *ms_out, bool with_bases = false, double *grad_bases = nullptr);
// The launches of one backward run of `plan`, nothing checked (run_var_backward and plan_smooth.cpp check first, and call
// ensure_var_grad_planes where grad_weights is not null).  grad_weights: nullptr (3 launches per scan), or n_weights entries.
// log2_base / ln_base: nullptr for the plane form, else per weight plane.  holds_sum: nullptr, or per weight plane whether its
// gradient plane already holds a sum this run adds to (else the first var_grad launch that touches a plane stores).  `timer` is
// marked behind every launch and behind every var_grad slot that was not issued, which is skipped first.
struct VarBackwardIo {
    const void *const *in = nullptr, *const *weights = nullptr, *const *grad_out = nullptr;
    void *const *grad_in = nullptr, *const *grad_weights = nullptr;
    const float *log2_base = nullptr, *ln_base = nullptr;
    const bool *holds_sum = nullptr;
    // not null (the power form, grad_weights not null): the var_grad launches are the base-reducing ones, scan q's slabs at
    // slabs + plan->bases_slab_offset[q]; an entry of grad_weights may then be null (its launch still runs, nothing is stored)
    double *slabs = nullptr;
    int64_t in_stride = 0, weights_stride = 0, grad_out_stride = 0, grad_in_stride = 0, grad_weights_stride = 0;      // a batched plan
};
int ensure_var_grad_planes(rf_var_plan *plan);
int ensure_var_bases_slabs(rf_var_plan *plan);
int launch_var_backward(rf_var_plan *plan, const VarBackwardIo &io, hipStream_t stream, LaunchTimer &timer);
int64_t var_max_extent();      // extents above it are refused (RF_ERR_UNSUPPORTED)
// The distances and their adjoints, one launch each (plan_var.cpp: one argument record, one runner per direction).  The image forms
// take a batch (plan_smooth.cpp): image b's guide planes are guide_stride samples behind image 0's -- their gradients
// grad_guide_stride -- and dx, dy (grad_dx, grad_dy) hold `batch` dense planes.  The volume forms: d_x, d_y slice by slice as the image
// form gives them, d_z along z from spacing_z; no batch.  accumulate: added to what the gradient planes hold.
int run_var_distances(const void *const *guide_planes, int32_t n_guide, int32_t guide_u8, int64_t width, int64_t height, float scale,
                      void *dx, void *dy, int32_t device, hipStream_t stream, int32_t batch = 1, int64_t guide_stride = 0);
int run_var_distances_volume(const void *const *guide_volumes, int32_t n_guide, int32_t guide_u8, int64_t width, int64_t height, int64_t depth,
                             float scale, float spacing_z, void *dx, void *dy, void *dz, int32_t device, hipStream_t stream);
int run_var_distances_backward(const void *const *guide_planes, int32_t n_guide, int64_t width, int64_t height, float scale, const void *grad_dx,
                               const void *grad_dy, void *const *grad_guide_planes, int32_t accumulate, int32_t device, hipStream_t stream,
                               int32_t batch = 1, int64_t guide_stride = 0, int64_t grad_guide_stride = 0);
int run_var_distances_volume_backward(const void *const *guide_volumes, int32_t n_guide, int64_t width, int64_t height, int64_t depth, float scale,
                                      const void *grad_dx, const void *grad_dy, const void *grad_dz, void *const *grad_guide_volumes,
                                      int32_t accumulate, int32_t device, hipStream_t stream);
}  // namespace rf
