// plan_smooth.h -- the plan behind the rf_smooth_plan_* entry points: the domain-transform recursive filter as one object
// (plan_smooth.cpp).
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "plan_var.h"

struct rf_smooth_plan {
    int64_t width = 0, height = 0;
    int n_planes = 1, n_guide = 0, iterations = 1;
    // rf_smooth_plan_create_batched: `batch` images per call, every launch taking all of them (gridDim.z).  The callers' arrays name
    // image 0's planes; image b's are image_stride / guide_stride samples further per b.  rf_smooth_plan_create: 1, strides unused.
    int batch = 1;
    int64_t image_stride = 0, guide_stride = 0;
    bool image_u8 = false, guide_u8 = false;
    // rf_smooth_plan_create_volume: planes are [z][y][x] volumes of width x height x depth samples, the inner plan is a volume plan
    // (+x -x +y -y +z -z on three exponent volumes) and there is a third distance volume d_z, formed from spacing_z.  batch stays 1.
    bool volume = false;
    int64_t depth = 1;
    float spacing_z = 1.0f;
    // RF_SMOOTH_VOLUME_BACKWARD: a volume plan with a backward (f32 volumes).  An image plan always has one.
    bool volume_backward = false;
    bool has_backward() const { return !volume || volume_backward; }
    int n_distances() const { return volume ? 3 : 2; }
    int64_t samples() const { return width * height * depth; }      // of one plane
    int device = 0;
    bool host_only = false;
    double sigma_s = 0.0, sigma_r = 0.0;     // as given to create or to rf_smooth_plan_set_sigmas: the factors of the sigma gradients
    float scale = 0.0f;                      // of var_distances: sigma_s / sigma_r, over 255 where the planes that guide are bytes
    std::vector<float> bases;                // a_k
    std::vector<float> log2_bases;           // (float)log2((double)a_k): what rf_var_plan_execute_power forms from a_k
    std::vector<float> ln_bases;             // (float)log((double)a_k): what rf_var_plan_backward_power forms beside it
    std::unique_ptr<rf_var_plan> inner;      // +x -x +y -y on two exponent planes: two pair stages, the tails and the carries
    // one allocation: d_x (one plane per image), d_y (the same), (a volume: d_z,) then (byte images) n_planes f32 working planes per image
    float *planes = nullptr;
    size_t planes_bytes = 0;
    std::vector<std::string> names;          // "var_distances", then the inner plan's six per iteration
    size_t workspace_bytes() const { return planes_bytes + inner->workspace_bytes(); }
    // rf_smooth_plan_backward: the launch names with the distances held constant ([0]) and differentiated ([1]); [1] needs the
    // gradients of d_x and d_y and the outputs of iterations 0 .. K-2 -- 2 + (K - 1) * n_planes f32 planes, allocated by the first
    // call that needs them -- and the inner plan's (4 + 1) * n_planes; all of it per image: gd_x [image], gd_y [image], then
    // [iteration][image][plane].  A volume plan with a backward: the same one dimension up -- gd_x, gd_y, gd_z, then
    // [iteration][plane], 3 + (K - 1) * n_planes f32 volumes, and the inner plan's (6 + 1) * n_planes.  A volume plan without one has
    // no names and no workspace.
    std::vector<std::string> backward_names[2];
    float *grad_planes = nullptr;
    size_t own_backward_bytes() const { return (size_t)batch * (size_t)(n_distances() + (iterations - 1) * n_planes) * (size_t)samples() * sizeof(float); }
    size_t backward_workspace_bytes(bool edges) const { return edges && has_backward() ? own_backward_bytes() + inner->backward_workspace_bytes(true) : 0; }
    // rf_smooth_plan_backward_sigmas: the names of [1] (edges = 0: without the final distances' adjoint), "var_dot", "var_param_sum";
    // f64 slabs the plan owns -- per iteration the inner plan's bases slabs (iteration k's at k * inner->bases_slab_offset.back()),
    // then var_dot's 2 * n_distances * var_dot_blocks entries -- allocated by the first call that needs them.
    std::vector<std::string> sigma_names[2];
    double *sigma_slabs = nullptr;
    int64_t dot_blocks() const { return rf::var_dot_blocks(samples() * batch); }
    int64_t sigma_slab_count() const { return (int64_t)iterations * inner->bases_slab_offset.back() + 2 * n_distances() * dot_blocks(); }
    ~rf_smooth_plan();
};

namespace rf {
// batch == nullptr: rf_smooth_plan_create; else rf_smooth_plan_create_batched (which has refused a null one)
int build_smooth_plan(const rf_smooth_desc *desc, const rf_smooth_batch_desc *batch, rf_smooth_plan **out);
// rf_smooth_plan_create_volume
int build_smooth_volume_plan(const rf_smooth_volume_desc *desc, rf_smooth_plan **out);
// rf_smooth_plan_set_sigmas: the scale and the bases of new sigmas, formed as create forms them; a refusal leaves the plan as it was
int set_smooth_sigmas(rf_smooth_plan *plan, double sigma_s, double sigma_r);
// what the backward entry points answer for a volume plan without RF_SMOOTH_VOLUME_BACKWARD: RF_ERR_UNSUPPORTED
int refuse_volume_backward();
// ms_out == nullptr: plain asynchronous execute; else every launch bracketed by events (capacity checked by the caller)
int run_smooth_plan(rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes, void *const *out_planes,
                    hipStream_t stream, float *ms_out);
// The adjoint (rf_smooth_plan_backward in recfilter_amd.h); ms_out: one slot per name of backward_names[edges].
int run_smooth_backward(rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes,
                        const void *const *grad_out_planes, void *const *grad_image_planes, void *const *grad_guide_planes, int32_t edges,
                        hipStream_t stream, float *ms_out, bool sigmas = false, double *grad_params = nullptr);
}  // namespace rf
