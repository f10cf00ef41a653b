// plan_smooth.cpp -- edge-aware smoothing by the domain-transform recursive filter (Gastal & Oliveira 2011) as one plan.
//
// One var_distances launch forms the exponent planes d_x, d_y the plan owns; then K runs of an inner varying plan
// (+x -x +y -y: two pair stages, power form) with bases {a_k, a_k}.  Nothing here is a kernel of its own: the launches are those
// of rf_var_distances and rf_var_plan_execute_power, with the same arguments, so an f32 image gives their bits.
// Byte images (the storage contract of RF_IO_U8): the first stage reads the caller's bytes into f32 working planes the plan
// owns, everything between runs in place on those, and the final pass of the last stage stores sat8 (pixel.h) of its f32
// result to the caller's bytes.  No conversion launch, and nothing between two iterations is rounded.
//
// run_smooth_backward is the adjoint for f32 images.  With the distances held constant it is var_distances and, per iteration in
// reverse order, the inner plan's power-form adjoint without exponent gradients: the launches of rf_var_plan_backward_power.  To
// differentiate through the distances it first reruns iterations 0 .. K-2 into checkpoint planes (the fused pair stages), then
// per iteration in reverse order the inner plan's adjoint WITH both exponent gradients on that iteration's input -- the first
// stores into gd_x, gd_y, the later ones add -- and one var_distances_grad launch takes gd_x, gd_y to the guide.
//
// With the sigma gradients (rf_smooth_plan_backward_sigmas) it runs the list through the distances at either setting of `edges` (edges = 0
// leaves out the distances' adjoint), every inner backward on the base-reducing var_grad instances with its own segment of plan-owned
// f64 slabs, then one var_dot launch (sum gd (d - d0) and sum gd) and one var_param_sum launch that stores dL/dsigma_s, dL/dsigma_r,
// dL/dspacing_z and dL/da_k with factors the host formed in double.  rf_smooth_plan_set_sigmas recomputes the constants as create does.
//
// A batched plan (rf_smooth_plan_create_batched) is the same sequence: every launch takes all the images on gridDim.z, each image
// with its own distance planes, tails, carries and working planes, laid out image after image as a single-image plan lays out
// its one.  The launch count does not depend on the batch.  The caller's planes are checked per (image, plane) extent, sorted
// (check_extents); a single image's by the checks every plan family shares (run_support.h: check_plane, check_written_planes).
//
// Both run functions construct one LaunchTimer (run_support.h) and hand it to every launcher they call, so the slots of a timed run
// follow the plan's name lists; the constants of the power form, log2 and ln of every a_k, are the plan's from its construction.
// What the two share is here once: distance_planes (where d_x, d_y(, d_z) and their gradients lie), iteration_constants (the inner
// plan's triples of iteration k), form_distances and form_guide_gradient -- the one place per direction that chooses between the
// image's and the volume's distance runner, and between the guide and a self-guiding image.
//
// A volume plan (build_smooth_volume_plan, rf_smooth_plan_create_volume) is the same sequence one dimension up: three distance
// volumes from one var_distances_volume launch (d_z from spacing_z), an inner volume plan +x -x +y -y +z -z with {a_k, a_k, a_k},
// 1 + 9 K launches; bytes enter at the first x stage and leave at the last z pass.  No batch.  Created with
// RF_SMOOTH_VOLUME_BACKWARD (f32 volumes) it has the backward too, run_smooth_backward one dimension up: three exponent volumes and
// their gradients, the inner volume plan's adjoint with {a_k, a_k, a_k}, var_distances_volume_grad at the end -- 1 + 18 K launches
// with the distances held constant, 51 K - 7 through them.  Without the flag its backward is refused.
#include "plan_smooth.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

rf_smooth_plan::~rf_smooth_plan() {
    if (planes) (void)hipFree(planes);
    if (grad_planes) (void)hipFree(grad_planes);
    if (sigma_slabs) (void)hipFree(sigma_slabs);
}

namespace rf {

namespace {

int validate(const rf_smooth_desc *d) {
    if (d->abi != RF_ABI) {
        set_error("rf_smooth_desc.abi is %u, this library speaks revision %u of recfilter_amd.h", d->abi, RF_ABI);
        return RF_ERR_INVALID_ARG;
    }
    if (d->flags != 0) { set_error("rf_smooth_desc.flags must be 0 (got %#x)", d->flags); return RF_ERR_INVALID_ARG; }
    if (d->n_planes < 1 || d->n_planes > RF_MAX_PLANES) { set_error("n_planes must be 1..%d (got %d)", RF_MAX_PLANES, d->n_planes); return RF_ERR_INVALID_ARG; }
    if (d->n_guide < 0 || d->n_guide > RF_MAX_PLANES) { set_error("n_guide must be 0..%d (got %d)", RF_MAX_PLANES, d->n_guide); return RF_ERR_INVALID_ARG; }
    if (d->image_u8 != 0 && d->image_u8 != 1) { set_error("image_u8 must be 0 or 1 (got %d)", d->image_u8); return RF_ERR_INVALID_ARG; }
    if (d->guide_u8 != 0 && d->guide_u8 != 1) { set_error("guide_u8 must be 0 or 1 (got %d)", d->guide_u8); return RF_ERR_INVALID_ARG; }
    if (d->guide_u8 == 1 && d->n_guide == 0) { set_error("guide_u8 = 1 without guide planes (n_guide = 0: the image guides itself)"); return RF_ERR_INVALID_ARG; }
    if (d->iterations < 1 || d->iterations > RF_SMOOTH_MAX_ITERATIONS) {
        set_error("iterations must be 1..%d (got %d)", RF_SMOOTH_MAX_ITERATIONS, d->iterations);
        return RF_ERR_INVALID_ARG;
    }
    if (d->width < 1 || d->height < 1) { set_error("width and height must be positive (got %lld x %lld)", (long long)d->width, (long long)d->height); return RF_ERR_INVALID_ARG; }
    if (!std::isfinite(d->sigma_s) || !(d->sigma_s > 0.0)) { set_error("sigma_s must be finite and positive (got %g)", d->sigma_s); return RF_ERR_INVALID_ARG; }
    if (!std::isfinite(d->sigma_r) || !(d->sigma_r > 0.0)) { set_error("sigma_r must be finite and positive (got %g)", d->sigma_r); return RF_ERR_INVALID_ARG; }
    if (d->width % 4 != 0) {
        set_error("the varying scans move 16 bytes per lane along x: the width must be a multiple of 4 (got %lld)", (long long)d->width);
        return RF_ERR_UNSUPPORTED;
    }
    if (d->width > var_max_extent() || d->height > var_max_extent()) {
        set_error("extents %lld x %lld are above %lld", (long long)d->width, (long long)d->height, (long long)var_max_extent());
        return RF_ERR_UNSUPPORTED;
    }
    return RF_OK;
}

// the refusals of rf_smooth_plan_create_batched that concern the batch alone, in the order recfilter_amd.h documents
int validate_batch(const rf_smooth_desc *d, const rf_smooth_batch_desc *b) {
    if (b->batch < 1 || b->batch > RF_SMOOTH_MAX_BATCH) { set_error("batch must be 1..%d (got %d)", RF_SMOOTH_MAX_BATCH, b->batch); return RF_ERR_INVALID_ARG; }
    if (b->image_stride % 4 != 0 || b->guide_stride % 4 != 0) {
        set_error("image_stride = %lld and guide_stride = %lld must be multiples of 4 samples: every image's planes keep the alignment of image 0's",
                  (long long)b->image_stride, (long long)b->guide_stride);
        return RF_ERR_INVALID_ARG;
    }
    // (extents the plain validation refuses anyway form no product here)
    const bool sane = d->width >= 1 && d->height >= 1 && d->width <= var_max_extent() && d->height <= var_max_extent();
    const int64_t samples = sane ? d->width * d->height : 0;
    if (b->image_stride < samples || b->image_stride < 0) {
        set_error("image_stride = %lld is below one plane's %lld samples", (long long)b->image_stride, (long long)samples);
        return RF_ERR_INVALID_ARG;
    }
    if (d->n_guide == 0 && b->guide_stride != 0) {
        set_error("guide_stride must be 0 where the image guides itself (n_guide = 0; got %lld)", (long long)b->guide_stride);
        return RF_ERR_INVALID_ARG;
    }
    if (d->n_guide > 0 && b->guide_stride < std::max<int64_t>(samples, 1)) {
        set_error("guide_stride = %lld is below one plane's %lld samples (every image has its own guide: a guide shared by the batch is not supported)",
                  (long long)b->guide_stride, (long long)samples);
        return RF_ERR_INVALID_ARG;
    }
    return RF_OK;
}

// ---- the aliasing rules of a batched call, per (image, plane) extent ------------------------------------------------------------
// The planes of NCHW tensors interleave (image b's plane 1 lies between image b's plane 0 and image b+1's plane 0), so an array is
// not one span.  Every extent [planes[pl] + b * stride, + one plane) of every array goes into one list, sorted by its start;
// one sweep then holds, for the read and for the written extents seen so far, the two that end last.  An extent overlaps an
// earlier one of a class exactly when the one ending last does -- or, where that is the one extent it may be (in place: the same
// (image, plane) of the partner array, the same address), the second.  E extents: O(E log E), no pair is formed.
struct ExtentArray {
    const char *name;
    const void *const *planes;
    int n;
    int64_t stride_bytes;
    size_t bytes;            // of one plane
    bool written;
    int partner;             // the array whose extent of the same (image, plane) may be this one exactly, or -1
};
struct Extent {
    uintptr_t lo, hi;
    int32_t array, b, pl;
};

int check_extents(const ExtentArray *arrays, int n_arrays, int batch) {
    std::vector<Extent> ext;
    for (int k = 0; k < n_arrays; k++)
        for (int b = 0; b < batch; b++)
            for (int pl = 0; pl < arrays[k].n; pl++) {
                const uintptr_t lo = (uintptr_t)arrays[k].planes[pl] + (uintptr_t)((int64_t)b * arrays[k].stride_bytes);
                ext.push_back({lo, lo + arrays[k].bytes, k, b, pl});
            }
    std::sort(ext.begin(), ext.end(), [](const Extent &x, const Extent &y) { return x.lo < y.lo; });
    const Extent *last[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};      // [written][0: ends last, 1: the next]
    auto in_place = [&](const Extent &x, const Extent &y) {
        return arrays[x.array].partner == y.array && x.b == y.b && x.pl == y.pl && x.lo == y.lo && x.hi == y.hi;
    };
    for (const Extent &x : ext) {
        const bool w = arrays[x.array].written;
        for (int cls = 0; cls < 2; cls++) {
            if (!w && cls == 0) continue;                  // (two read extents may overlap)
            const Extent *y = last[cls][0];
            if (y && in_place(x, *y)) y = last[cls][1];
            if (y && y->hi > x.lo) {
                const Extent &rd = w ? *y : x, &wr = w ? x : *y;      // (both written: in the order met)
                set_error("%s plane %d of image %d overlaps %s plane %d of image %d: a plane that is written is disjoint from every other plane of the call, "
                          "or is exactly the same plane of the same image it is computed from",
                          arrays[wr.array].name, wr.pl, wr.b, arrays[rd.array].name, rd.pl, rd.b);
                return RF_ERR_INVALID_ARG;
            }
        }
        const Extent **slot = last[w ? 1 : 0];
        if (!slot[0] || x.hi > slot[0]->hi) { slot[1] = slot[0]; slot[0] = &x; }
        else if (!slot[1] || x.hi > slot[1]->hi) slot[1] = &x;
    }
    return RF_OK;
}

}  // namespace

namespace {
int build_checked(const rf_smooth_desc *desc, const rf_smooth_batch_desc *batch, int64_t depth, float spacing_z, bool volume_backward,
                  rf_smooth_plan **out);

// What the sigmas determine, for a plan whose guide kind and iteration count are set: the scale of var_distances and, per iteration,
// a_k with its log2 and ln -- or the refusal of a scale that is no f32 or of an a_k that rounds to 0 or 1.  The outputs are written
// only where nothing is refused.  Shared by create and rf_smooth_plan_set_sigmas: the two form the same bits.
int smooth_constants(const rf_smooth_plan *plan, double sigma_s, double sigma_r, float &scale_out, std::vector<float> &bases,
                     std::vector<float> &log2_bases, std::vector<float> &ln_bases) {
    // a byte guide means that guide divided by 255 (a separate uint8 guide, or a uint8 image guiding itself)
    const bool bytes_guide = plan->n_guide > 0 ? plan->guide_u8 : plan->image_u8;
    const float scale = (float)(sigma_s / sigma_r / (bytes_guide ? 255.0 : 1.0));
    if (!std::isfinite(scale)) { set_error("sigma_s / sigma_r = %g is not an f32", sigma_s / sigma_r); return RF_ERR_UNSUPPORTED; }
    const int K = plan->iterations;
    std::vector<float> a, l2, ln;
    for (int k = 0; k < K; k++) {
        const double sigma_k = sigma_s * std::sqrt(3.0) * std::ldexp(1.0, K - 1 - k) / std::sqrt(std::ldexp(1.0, 2 * K) - 1.0);
        const float a_k = (float)std::exp(-std::sqrt(2.0) / sigma_k);
        if (!(a_k > 0.0f && a_k < 1.0f)) {
            set_error("iteration k = %d: the base a_k = exp(-sqrt(2) / %g) rounds to %g in f32", k, sigma_k, (double)a_k);
            return RF_ERR_UNSUPPORTED;
        }
        a.push_back(a_k);
        l2.push_back((float)std::log2((double)a_k));
        ln.push_back((float)std::log((double)a_k));
    }
    scale_out = scale;
    bases.swap(a);
    log2_bases.swap(l2);
    ln_bases.swap(ln);
    return RF_OK;
}
}

int set_smooth_sigmas(rf_smooth_plan *plan, double sigma_s, double sigma_r) {
    if (!plan) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    if (!std::isfinite(sigma_s) || !(sigma_s > 0.0)) { set_error("sigma_s must be finite and positive (got %g)", sigma_s); return RF_ERR_INVALID_ARG; }
    if (!std::isfinite(sigma_r) || !(sigma_r > 0.0)) { set_error("sigma_r must be finite and positive (got %g)", sigma_r); return RF_ERR_INVALID_ARG; }
    const int rc = smooth_constants(plan, sigma_s, sigma_r, plan->scale, plan->bases, plan->log2_bases, plan->ln_bases);
    if (rc == RF_OK) { plan->sigma_s = sigma_s; plan->sigma_r = sigma_r; }
    return rc;
}

int build_smooth_plan(const rf_smooth_desc *desc, const rf_smooth_batch_desc *batch, rf_smooth_plan **out) {
    if (!desc || !out) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    *out = nullptr;
    int rc = batch ? validate_batch(desc, batch) : RF_OK;
    if (rc == RF_OK) rc = validate(desc);
    if (rc != RF_OK) return rc;
    return build_checked(desc, batch, 0, 1.0f, false, out);
}

int build_smooth_volume_plan(const rf_smooth_volume_desc *desc, rf_smooth_plan **out) {
    if (!desc || !out) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    *out = nullptr;
    // the description of a slice, checked as an image's; then the volume's own domain and spacing_z
    rf_smooth_desc d{};
    d.abi = desc->abi;
    d.image_u8 = desc->image_u8;
    d.width = desc->width;
    d.height = desc->height;
    d.n_planes = desc->n_planes;
    d.n_guide = desc->n_guide;
    d.guide_u8 = desc->guide_u8;
    d.iterations = desc->iterations;
    d.sigma_s = desc->sigma_s;
    d.sigma_r = desc->sigma_r;
    d.device = desc->device;
    d.flags = 0;
    // (any bit but the one flag a volume plan has: refused where an image's flags are, behind the revision check)
    if (desc->abi == RF_ABI && (desc->flags & ~(uint32_t)RF_SMOOTH_VOLUME_BACKWARD) != 0) {
        set_error("rf_smooth_volume_desc.flags must be 0 or RF_SMOOTH_VOLUME_BACKWARD (got %#x)", desc->flags);
        return RF_ERR_INVALID_ARG;
    }
    int rc = validate(&d);
    if (rc != RF_OK) return rc;
    const bool backward = (desc->flags & RF_SMOOTH_VOLUME_BACKWARD) != 0;
    if (backward && desc->image_u8) {
        set_error("RF_SMOOTH_VOLUME_BACKWARD: the backward of a smoothing plan takes f32 volumes (image_u8 = 1)");
        return RF_ERR_UNSUPPORTED;
    }
    const float spacing_z = (float)desc->spacing_z;
    if (!std::isfinite(desc->spacing_z) || !std::isfinite(spacing_z) || !(spacing_z > 0.0f)) {
        set_error("spacing_z must be finite and positive in f32 (got %g)", desc->spacing_z);
        return RF_ERR_INVALID_ARG;
    }
    rc = check_volume_extents(desc->width, desc->height, desc->depth, desc->n_planes);
    if (rc != RF_OK) return rc;
    return build_checked(&d, nullptr, desc->depth, spacing_z, backward, out);
}

int refuse_volume_backward() {
    set_error("this volume plan has no backward: create it with RF_SMOOTH_VOLUME_BACKWARD in rf_smooth_volume_desc.flags");
    return RF_ERR_UNSUPPORTED;
}

namespace {

// the plan of a description that has passed its checks; depth = 0: an image, else a volume
int build_checked(const rf_smooth_desc *desc, const rf_smooth_batch_desc *batch, int64_t depth, float spacing_z, bool volume_backward,
                  rf_smooth_plan **out) {
    int rc = RF_OK;
    std::unique_ptr<rf_smooth_plan> plan(new rf_smooth_plan);
    plan->volume = depth > 0;
    plan->volume_backward = plan->volume && volume_backward;
    plan->depth = plan->volume ? depth : 1;
    plan->spacing_z = spacing_z;
    plan->width = desc->width;
    plan->height = desc->height;
    plan->n_planes = desc->n_planes;
    plan->n_guide = desc->n_guide;
    plan->iterations = desc->iterations;
    plan->image_u8 = desc->image_u8 != 0;
    plan->guide_u8 = desc->guide_u8 != 0;
    plan->host_only = desc->device == RF_DEVICE_HOST_ONLY;
    if (batch) {
        plan->batch = batch->batch;
        plan->image_stride = batch->image_stride;
        plan->guide_stride = batch->guide_stride;
    }
    rc = smooth_constants(plan.get(), desc->sigma_s, desc->sigma_r, plan->scale, plan->bases, plan->log2_bases, plan->ln_bases);
    if (rc != RF_OK) return rc;
    plan->sigma_s = desc->sigma_s;
    plan->sigma_r = desc->sigma_r;
    const int K = desc->iterations;
    const rf_var_scan_desc scans[6] = {{0, 1, 0}, {0, 0, 0}, {1, 1, 1}, {1, 0, 1}, {2, 1, 2}, {2, 0, 2}};
    // the inner plan: +x -x +y -y(, +z -z), a weight plane per dimension (the device checks, and the tails and the carries)
    rf_var_plan *inner = nullptr;
    auto describe = [&](auto &d, int dims) {
        d.abi = RF_ABI;
        d.dtype = RF_F32;
        d.n_planes = desc->n_planes;
        d.n_weights = dims;
        d.n_scans = 2 * dims;
        d.scans = scans;
        d.device = desc->device;
    };
    if (plan->volume) {
        rf_var_volume_desc vv{};
        describe(vv, 3);
        vv.width = desc->width;
        vv.height = desc->height;
        vv.depth = depth;
        rc = build_var_volume_plan(&vv, &inner);
    } else {
        rf_var_desc vd{};
        describe(vd, 2);
        vd.ndim = 2;
        vd.extent[0] = desc->width;
        vd.extent[1] = desc->height;
        rc = build_var_plan(&vd, &inner, plan->batch);
    }
    if (rc != RF_OK) return rc;
    plan->inner.reset(inner);
    plan->device = inner->device;
    const size_t plane_bytes = (size_t)plan->samples() * sizeof(float);
    plan->planes_bytes = plane_bytes * (size_t)((plan->volume ? 3 : 2) + (plan->image_u8 ? desc->n_planes : 0)) * (size_t)plan->batch;
    if (!plan->host_only) {
        RF_HIP_CHECK(hipSetDevice(plan->device));
        if (hipMalloc((void **)&plan->planes, plan->planes_bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("hipMalloc of %zu bytes of distance and working planes failed", plan->planes_bytes);
            return RF_ERR_NOMEM;
        }
    }
    plan->names.push_back(plan->volume ? "var_distances_volume" : "var_distances");
    for (int k = 0; k < K; k++)
        for (const std::string &n : inner->names) plan->names.push_back(n);
    // the adjoint's launch lists (a volume plan without RF_SMOOTH_VOLUME_BACKWARD has none: its backward is refused)
    for (int edges = 0; edges < 2 && plan->has_backward(); edges++) {
        std::vector<std::string> &names = plan->backward_names[edges];
        names.push_back(plan->names[0]);
        if (edges)
            for (int k = 0; k + 1 < K; k++)
                for (const std::string &n : inner->names) names.push_back(n);
        for (int k = 0; k < K; k++)
            for (const std::string &n : inner->backward_names[edges]) names.push_back(n);
        if (edges) names.push_back(plan->volume ? "var_distances_volume_grad" : "var_distances_grad");
    }
    // the sigma gradients: the list through the distances with the reducing var_grad launches (same names), then the two sums
    for (int edges = 0; edges < 2 && plan->has_backward(); edges++) {
        std::vector<std::string> &names = plan->sigma_names[edges];
        names = plan->backward_names[1];
        if (!edges) names.pop_back();
        names.push_back("var_dot");
        names.push_back("var_param_sum");
    }
    *out = plan.release();
    return RF_OK;
}

}  // namespace

namespace {

// The plan's distance planes d_x, d_y(, d_z) at `base` -- or their gradients, laid out alike -- one plane per image each (a volume:
// the batch is 1), and what follows them: `own`.  base == nullptr (no gradient planes yet, or none needed): all null.
struct DistancePlanes {
    float *d[3] = {nullptr, nullptr, nullptr};
    float *own = nullptr;
};
DistancePlanes distance_planes(const rf_smooth_plan *plan, float *base) {
    DistancePlanes p;
    if (!base) return p;
    const size_t each = (size_t)plan->samples() * (size_t)plan->batch;
    for (int k = 0; k < plan->n_distances(); k++) p.d[k] = base + each * (size_t)k;
    p.own = base + each * (size_t)plan->n_distances();
    return p;
}

// The constants of iteration k for the inner plan, whose exponent planes all share the base a_k; holds_sum: the backward's
// exponent gradients already hold the sum of the iterations behind k.
struct IterationConstants {
    float log2_base[3], ln_base[3];
    bool holds_sum[3];
};
IterationConstants iteration_constants(const rf_smooth_plan *plan, int k) {
    IterationConstants c;
    for (int q = 0; q < 3; q++) {
        c.log2_base[q] = plan->log2_bases[(size_t)k];
        c.ln_base[q] = plan->ln_bases[(size_t)k];
        c.holds_sum[q] = k < plan->iterations - 1;
    }
    return c;
}

// The distances of a call, one launch: an image's or a volume's, from the guide planes or -- where the image guides itself -- from
// the image planes, with that array's stride from image to image.
int form_distances(const rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes, const DistancePlanes &p,
                   hipStream_t stream) {
    const bool self = plan->n_guide == 0;
    const void *const *guide = self ? image_planes : guide_planes;
    const int n_guide = self ? plan->n_planes : plan->n_guide, guide_u8 = self ? plan->image_u8 : plan->guide_u8;
    if (plan->volume)
        return run_var_distances_volume(guide, n_guide, guide_u8, plan->width, plan->height, plan->depth, plan->scale, plan->spacing_z, p.d[0], p.d[1],
                                        p.d[2], plan->device, stream);
    return run_var_distances(guide, n_guide, guide_u8, plan->width, plan->height, plan->scale, p.d[0], p.d[1], plan->device, stream, plan->batch,
                             self ? plan->image_stride : plan->guide_stride);
}

// The adjoint of form_distances, one launch, from the distance gradients `g`.  A separate guide: its gradient is stored; the image
// guiding itself: added to the image gradient the scans have just left there.
int form_guide_gradient(const rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes, const DistancePlanes &g,
                        void *const *grad_image_planes, void *const *grad_guide_planes, hipStream_t stream) {
    const bool self = plan->n_guide == 0;
    const void *const *guide = self ? image_planes : guide_planes;
    void *const *grad = self ? grad_image_planes : grad_guide_planes;
    const int n_guide = self ? plan->n_planes : plan->n_guide, accumulate = self ? 1 : 0;
    const int64_t stride = self ? plan->image_stride : plan->guide_stride;
    if (plan->volume)
        return run_var_distances_volume_backward(guide, n_guide, plan->width, plan->height, plan->depth, plan->scale, g.d[0], g.d[1], g.d[2], grad,
                                                 accumulate, plan->device, stream);
    return run_var_distances_backward(guide, n_guide, plan->width, plan->height, plan->scale, g.d[0], g.d[1], grad, accumulate, plan->device, stream,
                                      plan->batch, stride, stride);
}

}  // namespace

int run_smooth_plan(rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes, void *const *out_planes,
                    hipStream_t stream, float *ms_out) {
    if (!plan || !image_planes || !out_planes) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    if (plan->n_guide > 0 && !guide_planes) { set_error("this plan takes %d separate guide planes: guide_planes is null", plan->n_guide); return RF_ERR_INVALID_ARG; }
    if (plan->n_guide == 0 && guide_planes) { set_error("this plan's image guides itself (n_guide = 0): guide_planes must be null"); return RF_ERR_INVALID_ARG; }
    if (plan->host_only) { set_error("host-only plan (RF_DEVICE_HOST_ONLY) cannot execute"); return RF_ERR_HIP; }
    const size_t samples = (size_t)plan->samples();
    const size_t image_bytes = samples * (plan->image_u8 ? 1 : sizeof(float));
    int rc = RF_OK;
    for (int pl = 0; pl < plan->n_planes && rc == RF_OK; pl++)
        rc = check_plane("plane", pl, {{image_planes[pl]}, {out_planes[pl]}}, plan->image_u8 ? 3u : 15u, "null image pointer",
                         plan->image_u8 ? "uint8 image planes must be 4-byte aligned" : "f32 image planes must be 16-byte aligned");
    for (int ch = 0; ch < plan->n_guide && rc == RF_OK; ch++)
        rc = check_plane("guide plane", ch, {{guide_planes[ch]}}, plan->guide_u8 ? 3u : 15u, "null pointer",
                         plan->guide_u8 ? "uint8 guide planes must be 4-byte aligned" : "f32 guide planes must be 16-byte aligned");
    if (rc != RF_OK) return rc;
    // a stage has loaded its tile before it stores, so a plane may be filtered in place; any other overlap of an input with an output
    // is read after another workgroup's store
    const int B = plan->batch;
    const int64_t image_stride = plan->image_stride;
    if (B > 1) {
        const int64_t stride_bytes = image_stride * (int64_t)(plan->image_u8 ? 1 : sizeof(float));
        const ExtentArray arrays[2] = {{"input", image_planes, plan->n_planes, stride_bytes, image_bytes, false, 1},
                                       {"output", (const void *const *)out_planes, plan->n_planes, stride_bytes, image_bytes, true, 0}};
        rc = check_extents(arrays, 2, B);
        if (rc != RF_OK) return rc;
    }
    for (int pl = 0; pl < plan->n_planes && B == 1; pl++)
        for (int q = 0; q < plan->n_planes; q++) {
            if (pl == q && image_planes[pl] == out_planes[q]) continue;
            if (overlap(image_planes[pl], image_bytes, out_planes[q], image_bytes)) {
                set_error("input plane %d overlaps output plane %d: an input plane is its own output plane or disjoint from every output plane", pl, q);
                return RF_ERR_INVALID_ARG;
            }
        }
    RF_HIP_CHECK(hipSetDevice(plan->device));
    LaunchTimer timer(stream, ms_out, plan->names.size());
    if (timer.status() != RF_OK) return timer.status();
    // the distances first, on the same stream: guide planes may be output planes
    const DistancePlanes d = distance_planes(plan, plan->planes);
    rc = form_distances(plan, image_planes, guide_planes, d, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc != RF_OK) return rc;
    void *work[RF_MAX_PLANES] = {};
    // byte images: [image][plane] behind the distance planes
    for (int pl = 0; pl < plan->n_planes; pl++) work[pl] = plan->image_u8 ? (void *)(d.own + samples * (size_t)pl) : out_planes[pl];
    const int64_t work_stride = plan->image_u8 ? (int64_t)samples * plan->n_planes : image_stride;
    const void *const weights[3] = {d.d[0], d.d[1], d.d[2]};
    const int K = plan->iterations;
    for (int k = 0; k < K; k++) {
        VarIo io{};
        io.in = k == 0 ? image_planes : (const void *const *)work;
        io.in_u8 = k == 0 && plan->image_u8;
        io.work = work;
        io.out = k == K - 1 ? out_planes : work;
        io.out_u8 = k == K - 1 && plan->image_u8;
        io.in_stride = k == 0 ? image_stride : work_stride;
        io.work_stride = work_stride;
        io.out_stride = k == K - 1 ? image_stride : work_stride;
        io.weights_stride = (int64_t)samples;
        rc = launch_var_stages(plan->inner.get(), io, weights, iteration_constants(plan, k).log2_base, stream, timer);
        if (rc != RF_OK) return rc;
    }
    return timer.finish();
}

int run_smooth_backward(rf_smooth_plan *plan, const void *const *image_planes, const void *const *guide_planes,
                        const void *const *grad_out_planes, void *const *grad_image_planes, void *const *grad_guide_planes, int32_t edges,
                        hipStream_t stream, float *ms_out, bool sigmas, double *grad_params) {
    // refusals, in the order recfilter_amd.h documents; nothing of HIP is called before the last of them
    if (!plan || !grad_out_planes || !grad_image_planes) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    if (sigmas && !grad_params) { set_error("null grad_params"); return RF_ERR_INVALID_ARG; }
    if (sigmas && ((uintptr_t)grad_params & 7u) != 0) { set_error("grad_params must be 8-byte aligned: it receives 3 + iterations doubles"); return RF_ERR_INVALID_ARG; }
    if (edges != 0 && edges != 1) { set_error("edges must be 0 or 1 (got %d)", edges); return RF_ERR_INVALID_ARG; }
    if (!plan->has_backward()) return refuse_volume_backward();
    if (plan->image_u8) { set_error("the backward of a smoothing plan takes f32 images (this plan's are uint8)"); return RF_ERR_UNSUPPORTED; }
    const bool self = plan->n_guide == 0;
    if (!self && !guide_planes) { set_error("this plan takes %d separate guide planes: guide_planes is null", plan->n_guide); return RF_ERR_INVALID_ARG; }
    if (self && guide_planes) { set_error("this plan's image guides itself (n_guide = 0): guide_planes must be null"); return RF_ERR_INVALID_ARG; }
    const bool need_image = self || edges == 1 || sigmas;      // (the sigma gradients rerun the forward)
    if (need_image && !image_planes) {
        set_error(sigmas ? "the sigma gradients need the image planes (image_planes is null)" : self ? "this plan's image guides itself: the backward needs the image planes (image_planes is null)"
                       : "gradients through the distances need the image planes (image_planes is null)");
        return RF_ERR_INVALID_ARG;
    }
    if (edges == 1 && plan->guide_u8) { set_error("no gradient with respect to a uint8 guide: edges = 1 takes f32 guide planes"); return RF_ERR_UNSUPPORTED; }
    if (edges == 1 && !self && !grad_guide_planes) { set_error("edges = 1 with %d separate guide planes: grad_guide_planes is null", plan->n_guide); return RF_ERR_INVALID_ARG; }
    if ((edges == 0 || self) && grad_guide_planes) {
        set_error(edges == 0 ? "edges = 0 forms no guide gradient: grad_guide_planes must be null"
                             : "this plan's image guides itself (n_guide = 0): its guide gradient is added to grad_image_planes and grad_guide_planes must be null");
        return RF_ERR_INVALID_ARG;
    }
    if (plan->host_only) { set_error("host-only plan (RF_DEVICE_HOST_ONLY) cannot execute"); return RF_ERR_HIP; }
    const int P = plan->n_planes, G = plan->n_guide, K = plan->iterations;
    const bool with_guide_grad = edges == 1 && !self;
    const size_t samples = (size_t)plan->samples(), plane_bytes = samples * sizeof(float);
    const size_t guide_bytes = samples * (plan->guide_u8 ? 1 : sizeof(float));
    int rc = RF_OK;
    for (int pl = 0; pl < P && rc == RF_OK; pl++)
        rc = check_plane("plane", pl, {{grad_out_planes[pl]}, {grad_image_planes[pl]}, {need_image ? image_planes[pl] : nullptr, need_image}}, 15u,
                         "null image pointer", "the varying scans need 16-byte aligned image pointers");
    // (a guide with a gradient is f32: one mask for the plane and its gradient)
    for (int ch = 0; ch < G && rc == RF_OK; ch++)
        rc = check_plane("guide plane", ch, {{guide_planes[ch]}, {with_guide_grad ? grad_guide_planes[ch] : nullptr, with_guide_grad}},
                         plan->guide_u8 ? 3u : 15u, "null pointer",
                         plan->guide_u8 ? "uint8 guide planes must be 4-byte aligned (the plane and its gradient)"
                                        : "f32 guide planes must be 16-byte aligned (the plane and its gradient)");
    if (rc != RF_OK) return rc;
    // what is written (grad_image planes, guide-gradient planes) against everything that is read and everything else that is written
    const int B = plan->batch;
    const int64_t image_stride = plan->image_stride, guide_stride = plan->guide_stride;
    if (B > 1) {
        const int64_t image_stride_bytes = image_stride * (int64_t)sizeof(float), guide_stride_bytes = guide_stride * (int64_t)(plan->guide_u8 ? 1 : sizeof(float));
        ExtentArray arrays[5];
        int n = 0, grad_out_at, grad_image_at;
        if (G > 0) arrays[n++] = {"guide", guide_planes, G, guide_stride_bytes, guide_bytes, false, -1};
        if (need_image) arrays[n++] = {"image", image_planes, P, image_stride_bytes, plane_bytes, false, -1};
        grad_out_at = n;
        grad_image_at = n + 1;
        arrays[n++] = {"grad_out", grad_out_planes, P, image_stride_bytes, plane_bytes, false, grad_image_at};
        arrays[n++] = {"grad_image", (const void *const *)grad_image_planes, P, image_stride_bytes, plane_bytes, true, grad_out_at};
        if (with_guide_grad) arrays[n++] = {"gradient of guide", (const void *const *)grad_guide_planes, G, guide_stride_bytes, plane_bytes, true, -1};
        rc = check_extents(arrays, n, B);
    } else {
        const PlaneList written[2] = {{"grad_image", (const void *const *)grad_image_planes, P, plane_bytes},
                                      {"gradient of guide", (const void *const *)grad_guide_planes, with_guide_grad ? G : 0, plane_bytes}};
        const PlaneList read[2] = {{"guide", guide_planes, G, guide_bytes}, {"image", image_planes, need_image ? P : 0, plane_bytes}};
        rc = check_written_planes(written, 2, read, 2, {"grad_out", grad_out_planes, P, plane_bytes});
    }
    if (rc != RF_OK) return rc;
    RF_HIP_CHECK(hipSetDevice(plan->device));
    rf_var_plan *inner = plan->inner.get();
    const bool through = edges == 1 || sigmas;       // the launch list through the distances: checkpoints and exponent gradients
    if (sigmas && !plan->sigma_slabs && hipMalloc((void **)&plan->sigma_slabs, (size_t)plan->sigma_slab_count() * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        plan->sigma_slabs = nullptr;
        set_error("hipMalloc of %zu bytes for the sigma gradients' slabs failed", (size_t)plan->sigma_slab_count() * sizeof(double));
        return RF_ERR_NOMEM;
    }
    if (through) {
        rc = ensure_var_grad_planes(inner);
        if (rc != RF_OK) return rc;
        if (!plan->grad_planes && hipMalloc((void **)&plan->grad_planes, plan->own_backward_bytes()) != hipSuccess) {
            (void)hipGetLastError();
            plan->grad_planes = nullptr;
            set_error("hipMalloc of %zu bytes for the distance gradients and the checkpoint planes failed", plan->own_backward_bytes());
            return RF_ERR_NOMEM;
        }
    }
    LaunchTimer timer(stream, ms_out, sigmas ? plan->sigma_names[edges].size() : plan->backward_names[edges].size());
    if (timer.status() != RF_OK) return timer.status();
    const DistancePlanes d = distance_planes(plan, plan->planes), g = distance_planes(plan, plan->grad_planes);
    rc = form_distances(plan, image_planes, guide_planes, d, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc != RF_OK) return rc;
    const void *const exponents[3] = {d.d[0], d.d[1], d.d[2]};
    // the output of iteration k, k = 0 .. K-2: [iteration][image][plane]
    const int64_t checkpoint_stride = (int64_t)samples * P;
    void *checkpoints[RF_SMOOTH_MAX_ITERATIONS][RF_MAX_PLANES] = {};
    if (through) {
        for (int k = 0; k + 1 < K; k++) {
            for (int pl = 0; pl < P; pl++) checkpoints[k][pl] = g.own + samples * ((size_t)k * (size_t)B * P + pl);
            VarIo io{};
            io.in = k == 0 ? image_planes : (const void *const *)checkpoints[k - 1];
            io.work = io.out = checkpoints[k];
            io.in_stride = k == 0 ? image_stride : checkpoint_stride;
            io.work_stride = io.out_stride = checkpoint_stride;
            io.weights_stride = (int64_t)samples;
            rc = launch_var_stages(inner, io, exponents, iteration_constants(plan, k).log2_base, stream, timer);
            if (rc != RF_OK) return rc;
        }
    }
    void *const grad_exponents[3] = {g.d[0], g.d[1], g.d[2]};
    for (int k = K - 1; k >= 0; k--) {
        const IterationConstants c = iteration_constants(plan, k);
        VarBackwardIo io{};
        io.in = !through ? nullptr : k == 0 ? image_planes : (const void *const *)checkpoints[k - 1];
        io.weights = exponents;
        io.grad_out = k == K - 1 ? grad_out_planes : (const void *const *)grad_image_planes;
        io.grad_in = grad_image_planes;
        io.grad_weights = through ? grad_exponents : nullptr;
        io.slabs = sigmas ? plan->sigma_slabs + (int64_t)k * inner->bases_slab_offset.back() : nullptr;
        io.log2_base = c.log2_base;
        io.ln_base = c.ln_base;
        io.holds_sum = c.holds_sum;
        io.in_stride = k == 0 ? image_stride : checkpoint_stride;
        io.weights_stride = io.grad_weights_stride = (int64_t)samples;
        io.grad_out_stride = io.grad_in_stride = image_stride;
        rc = launch_var_backward(inner, io, stream, timer);      // (every exponent gradient is always formed: nothing is skipped)
        if (rc != RF_OK) return rc;
    }
    if (edges == 1) {
        rc = form_guide_gradient(plan, image_planes, guide_planes, g, grad_image_planes, grad_guide_planes, stream);
        if (rc == RF_OK) rc = timer.mark();
        if (rc != RF_OK) return rc;
    }
    if (sigmas) {
        // Q and the sum of gd_z from one var_dot launch, then every scalar from one var_param_sum launch: the host forms the factors
        // in double, the device multiplies -- nothing synchronises
        const int n_dist = plan->n_distances(), n_scans = (int)inner->scans.size();
        const int64_t per_iteration = inner->bases_slab_offset.back(), blocks = plan->dot_blocks();
        double *const dot_slabs = plan->sigma_slabs + (int64_t)K * per_iteration;
        VarDotArgs dot{};
        for (int q = 0; q < n_dist; q++) {
            dot.gd[q] = g.d[q];
            dot.d[q] = d.d[q];
            dot.d0[q] = q == 2 ? plan->spacing_z : 1.0f;
        }
        dot.n_pairs = n_dist;
        dot.n = plan->samples() * plan->batch;
        dot.slabs = dot_slabs;
        rc = launch_var_dot(dot, stream);
        if (rc == RF_OK) rc = timer.mark();
        if (rc != RF_OK) return rc;
        // out: dL/dsigma_s, dL/dsigma_r, dL/dspacing_z, dL/da_0 .. dL/da_{K-1}.  With T the slabs of iteration k (sum of d w dL/dw):
        // dL/da_k = T / a_k, and da_k/dsigma_s = a_k (-ln a_k) / sigma_s gives sigma_s its share T (-ln a_k) / sigma_s
        VarParamSumArgs p{};
        p.slabs = plan->sigma_slabs;
        p.out = grad_params;
        p.n_out = 3 + K;
        int n = 0;
        for (int k = 0; k < K; k++)
            for (int q = 0; q < n_scans; q++, n++) {
                const double a = (double)plan->bases[(size_t)k];
                p.offset[n] = (int64_t)k * per_iteration + inner->bases_slab_offset[(size_t)q];
                p.count[n] = inner->bases_slab_offset[(size_t)q + 1] - inner->bases_slab_offset[(size_t)q];
                p.target[n] = 3 + k;
                p.factor[n] = 1.0 / a;
                p.target2[n] = 0;
                p.factor2[n] = -std::log(a) / plan->sigma_s;
            }
        for (int q = 0; q < n_dist; q++) {
            // sum gd (d - d0) = Q's share of dimension q: Q / sigma_s to sigma_s, -Q / sigma_r to sigma_r (a byte guide's 255 cancels)
            p.offset[n] = (int64_t)K * per_iteration + (2 * q) * blocks;
            p.count[n] = blocks;
            p.target[n] = 0;
            p.factor[n] = 1.0 / plan->sigma_s;
            p.target2[n] = 1;
            p.factor2[n] = -1.0 / plan->sigma_r;
            n++;
            if (q == 2) {      // sum gd_z: dL/dspacing_z
                p.offset[n] = (int64_t)K * per_iteration + (2 * q + 1) * blocks;
                p.count[n] = blocks;
                p.target[n] = 2;
                p.factor[n] = 1.0;
                p.target2[n] = -1;
                n++;
            }
        }
        p.n_segments = n;
        rc = launch_var_param_sum(p, stream);
        if (rc == RF_OK) rc = timer.mark();
        if (rc != RF_OK) return rc;
    }
    return timer.finish();
}

}  // namespace rf
