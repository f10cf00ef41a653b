// plan_var.cpp -- plan builder and driver of the spatially varying first-order scans (kernels_var.hip).
//
// No tables: the carry operators are data.  The builder validates the description, groups the scans into stages (a causal scan
// directly followed by the anticausal scan of the same dimension and weight plane is one stage where the two are all the plan
// runs along that dimension at that point), and allocates one workspace:
// tails [tile][component][plane][line] and carries [tile][c, d][plane][line], sized for the dimension that needs more.  Every
// stage is three launches: tails, carry, final pass.  The first stage reads the input planes, later stages filter the output
// planes in place.  The power form (rf_var_plan_execute_power) runs the same stages on exponent planes: a stage carries
// log2 of its plane's base and launches the kernels' POWER instances.  run_var_plan checks the arguments and constructs the run's
// LaunchTimer; launch_var_stages issues the launches of one run, and is what the smoothing plan (plan_smooth.cpp) calls per
// iteration.
//
// What every run shares lives here once: scan_args (the fields of VarArgs a plan determines), launch_stage (tails, carry, final
// pass, a mark of the run's LaunchTimer behind each) and power_constants (the bases of the power form, log2 and ln of each).  The
// timer and the plane checks (check_plane, check_written_planes) are run_support.h's, shared with the other plan families.
//
// run_var_backward is the adjoint of a plan (rf_var_plan_backward): per scan in reverse order an adjoint stage -- a unit-gain scan
// in the opposite direction, tails / var_carry / final pass like a forward stage, always scan by scan.  The image gradient needs
// nothing else.  Weight gradients need every scan's input and output: the forward is rerun scan by scan into plan-owned planes
// (n_scans * n_planes, allocated by the first call that needs them), every adjoint stage also stores its unscaled state to
// n_planes more, and one var_grad launch per scan forms the gradient from the three -- stored by the first launch that touches a
// weight plane, added by the later ones; the host knows which is which, so there are no atomics and no zero-fill.
// The power form (rf_var_plan_backward_power) is the same list on the kernels' POWER instances: the stages carry log2 of their
// plane's base, var_grad also its natural logarithm and the exponent plane, and what it stores is the gradient of the exponents.
// run_var_backward checks and constructs the timer; launch_var_backward issues the launches, and is what the smoothing plan's
// backward (plan_smooth.cpp) calls per iteration -- with planes that already hold a sum after the first.
//
// run_var_distances_backward: the adjoint of run_var_distances, one launch; the two share their checks of counts, scale and extents.
// run_var_distances_volume_backward is the same for run_var_distances_volume (check_volume_distance_counts, check_distance_scale,
// check_volume_extents).
//
// A signal plan (build_var_signal_plan, rf_var_plan_create_signal) is the plan of a 1 x length image whose stages run the three
// kernels of kernels_var_signal.hip (launch_stage's `signal`): width = length, height = 1, every scan along dim 0, the workspace
// sized for tiles plus groups of 64 tiles.  Runs, the backward and var_grad are the code above, unchanged.
//
// A plan may hold a batch (build_var_plan's third argument; plan_smooth.cpp only, the public entry points build 1): tails,
// carries and the backward's planes are then `batch` images' worth, image after image, and the launchers above carry the batch
// and the strides from image to image (VarIo, VarBackwardIo) to the kernels, whose grids take all images at once.
//
// A volume plan (build_var_volume_plan, rf_var_plan_create_volume) runs the same kernels on dense [z][y][x] volumes: scan_args
// gives an x or y stage the `depth` slices as its batch (slice strides of width * height samples: stage_stride; tails and carries
// slice after slice in the single-image layout) and a z stage the (width * height) x depth view of the y kernels, a voxel column
// per lane.  plan->batch stays 1 and the backward's planes are volumes.  check_volume_extents is the accepted domain, shared with
// run_var_distances_volume (the three exponent volumes, one launch) and plan_smooth.cpp.
#include "plan_var.h"

#include <algorithm>
#include <cmath>
#include <memory>

rf_var_plan::~rf_var_plan() {
    if (tails) (void)hipFree(tails);
    if (grad_planes) (void)hipFree(grad_planes);
    if (carry) (void)hipFree(carry);
}

namespace rf {

namespace {

constexpr int64_t kVarMaxExtent = int64_t(1) << 21;      // 64 lines or samples per workgroup along grid.y (65535 workgroups)

int validate(const rf_var_desc *d) {
    if (d->abi != RF_ABI) {
        set_error("rf_var_desc.abi is %u, this library speaks revision %u of recfilter_amd.h", d->abi, RF_ABI);
        return RF_ERR_INVALID_ARG;
    }
    if (d->flags != 0) { set_error("rf_var_desc.flags must be 0 (got %#x)", d->flags); return RF_ERR_INVALID_ARG; }
    if (d->n_planes < 1 || d->n_planes > RF_MAX_PLANES) { set_error("n_planes must be 1..%d (got %d)", RF_MAX_PLANES, d->n_planes); return RF_ERR_INVALID_ARG; }
    if (d->n_weights < 1 || d->n_weights > RF_VAR_MAX_SCANS) { set_error("n_weights must be 1..%d (got %d)", RF_VAR_MAX_SCANS, d->n_weights); return RF_ERR_INVALID_ARG; }
    if (d->n_scans < 1 || d->n_scans > RF_VAR_MAX_SCANS) { set_error("n_scans must be 1..%d (got %d)", RF_VAR_MAX_SCANS, d->n_scans); return RF_ERR_INVALID_ARG; }
    if (!d->scans) { set_error("null scans"); return RF_ERR_INVALID_ARG; }
    if (d->ndim != 2) { set_error("varying scans take 2-D images (ndim = %d)", d->ndim); return RF_ERR_UNSUPPORTED; }
    if (d->dtype != RF_F32) { set_error("varying scans take f32 planes (dtype = %d)", d->dtype); return RF_ERR_UNSUPPORTED; }
    for (int s = 0; s < d->n_scans; s++) {
        const rf_var_scan_desc &sc = d->scans[s];
        if (sc.dim < 0 || sc.dim > 1) { set_error("scan %d: dim must be 0 or 1 (got %d)", s, sc.dim); return RF_ERR_INVALID_ARG; }
        if (sc.weights < 0 || sc.weights >= d->n_weights) {
            set_error("scan %d: weights must be 0..%d (got %d)", s, d->n_weights - 1, sc.weights);
            return RF_ERR_INVALID_ARG;
        }
    }
    for (int k = 0; k < 2; k++)
        if (d->extent[k] < 1) { set_error("extent[%d] must be positive", k); return RF_ERR_INVALID_ARG; }
    for (int k = 0; k < 2; k++)
        if (d->extent[k] > kVarMaxExtent) { set_error("extent[%d] = %lld is above %lld", k, (long long)d->extent[k], (long long)kVarMaxExtent); return RF_ERR_UNSUPPORTED; }
    if (d->extent[0] % 4 != 0) {
        set_error("varying scans move 16 bytes per lane along x: the width must be a multiple of 4 (got %lld)", (long long)d->extent[0]);
        return RF_ERR_UNSUPPORTED;
    }
    return RF_OK;
}

int64_t tiles_of(int64_t n) { return (n + kVarTile - 1) / kVarTile; }

// the three launches of a stage along `dim` (a signal plan: "1d"); prefix: "var_", or "var_adj_" for an adjoint stage
void push_stage_names(std::vector<std::string> &names, const char *prefix, int dim, bool signal) {
    const char *axis = signal ? "1d" : dim == 0 ? "x" : dim == 1 ? "y" : "z";
    names.push_back(std::string(prefix) + "tails_" + axis);
    names.push_back(signal ? "var_carry_1d" : "var_carry");
    names.push_back(std::string(prefix) + "pass2_" + axis);
}

constexpr int64_t kVarMaxSignal = int64_t(1) << 30;      // samples of a signal: indices and 4096-sample groups stay inside int32

int validate_signal(const rf_var_signal_desc *d) {
    if (d->abi != RF_ABI) {
        set_error("rf_var_signal_desc.abi is %u, this library speaks revision %u of recfilter_amd.h", d->abi, RF_ABI);
        return RF_ERR_INVALID_ARG;
    }
    if (d->flags != 0) { set_error("rf_var_signal_desc.flags must be 0 (got %#x)", d->flags); return RF_ERR_INVALID_ARG; }
    if (d->n_planes < 1 || d->n_planes > RF_MAX_PLANES) { set_error("n_planes must be 1..%d (got %d)", RF_MAX_PLANES, d->n_planes); return RF_ERR_INVALID_ARG; }
    if (d->n_weights < 1 || d->n_weights > RF_VAR_MAX_SCANS) { set_error("n_weights must be 1..%d (got %d)", RF_VAR_MAX_SCANS, d->n_weights); return RF_ERR_INVALID_ARG; }
    if (d->n_scans < 1 || d->n_scans > RF_VAR_MAX_SCANS) { set_error("n_scans must be 1..%d (got %d)", RF_VAR_MAX_SCANS, d->n_scans); return RF_ERR_INVALID_ARG; }
    if (!d->scans) { set_error("null scans"); return RF_ERR_INVALID_ARG; }
    if (d->dtype != RF_F32) { set_error("varying scans take f32 signals (dtype = %d)", d->dtype); return RF_ERR_UNSUPPORTED; }
    for (int s = 0; s < d->n_scans; s++) {
        const rf_var_scan_desc &sc = d->scans[s];
        if (sc.dim != 0) { set_error("scan %d: dim must be 0 on a signal (got %d)", s, sc.dim); return RF_ERR_INVALID_ARG; }
        if (sc.weights < 0 || sc.weights >= d->n_weights) {
            set_error("scan %d: weights must be 0..%d (got %d)", s, d->n_weights - 1, sc.weights);
            return RF_ERR_INVALID_ARG;
        }
    }
    if (d->length < 1) { set_error("length must be positive (got %lld)", (long long)d->length); return RF_ERR_INVALID_ARG; }
    if (d->length > kVarMaxSignal) { set_error("length = %lld is above %lld", (long long)d->length, (long long)kVarMaxSignal); return RF_ERR_UNSUPPORTED; }
    if (d->length % 4 != 0) {
        set_error("varying scans move 16 bytes per lane: length must be a multiple of 4 (got %lld)", (long long)d->length);
        return RF_ERR_UNSUPPORTED;
    }
    return RF_OK;
}

constexpr int64_t kVarMaxVolumeLines = int64_t(1) << 30;      // width * height: the z view's line index is an int32
constexpr int64_t kVarMaxGridZ = 65535;                        // depth * n_planes: the slices ride on gridDim.z beside the planes

int validate_volume(const rf_var_volume_desc *d) {
    if (d->abi != RF_ABI) {
        set_error("rf_var_volume_desc.abi is %u, this library speaks revision %u of recfilter_amd.h", d->abi, RF_ABI);
        return RF_ERR_INVALID_ARG;
    }
    if (d->flags != 0) { set_error("rf_var_volume_desc.flags must be 0 (got %#x)", d->flags); return RF_ERR_INVALID_ARG; }
    if (d->n_planes < 1 || d->n_planes > RF_MAX_PLANES) { set_error("n_planes must be 1..%d (got %d)", RF_MAX_PLANES, d->n_planes); return RF_ERR_INVALID_ARG; }
    if (d->n_weights < 1 || d->n_weights > RF_VAR_MAX_SCANS) { set_error("n_weights must be 1..%d (got %d)", RF_VAR_MAX_SCANS, d->n_weights); return RF_ERR_INVALID_ARG; }
    if (d->n_scans < 1 || d->n_scans > RF_VAR_MAX_SCANS) { set_error("n_scans must be 1..%d (got %d)", RF_VAR_MAX_SCANS, d->n_scans); return RF_ERR_INVALID_ARG; }
    if (!d->scans) { set_error("null scans"); return RF_ERR_INVALID_ARG; }
    if (d->dtype != RF_F32) { set_error("varying scans take f32 volumes (dtype = %d)", d->dtype); return RF_ERR_UNSUPPORTED; }
    for (int s = 0; s < d->n_scans; s++) {
        const rf_var_scan_desc &sc = d->scans[s];
        if (sc.dim < 0 || sc.dim > 2) { set_error("scan %d: dim must be 0, 1 or 2 on a volume (got %d)", s, sc.dim); return RF_ERR_INVALID_ARG; }
        if (sc.weights < 0 || sc.weights >= d->n_weights) {
            set_error("scan %d: weights must be 0..%d (got %d)", s, d->n_weights - 1, sc.weights);
            return RF_ERR_INVALID_ARG;
        }
    }
    return check_volume_extents(d->width, d->height, d->depth, d->n_planes);
}

int build_checked(const rf_var_desc *desc, rf_var_plan **out, int batch, bool signal);

}  // namespace

int check_volume_extents(int64_t width, int64_t height, int64_t depth, int32_t n_planes) {
    if (width < 1 || height < 1 || depth < 1) {
        set_error("width, height and depth must be positive (got %lld x %lld x %lld)", (long long)width, (long long)height, (long long)depth);
        return RF_ERR_INVALID_ARG;
    }
    if (width > kVarMaxExtent || height > kVarMaxExtent || depth > kVarMaxExtent) {
        set_error("extents %lld x %lld x %lld are above %lld", (long long)width, (long long)height, (long long)depth, (long long)kVarMaxExtent);
        return RF_ERR_UNSUPPORTED;
    }
    if (width % 4 != 0) {
        set_error("varying scans move 16 bytes per lane along x: the width must be a multiple of 4 (got %lld)", (long long)width);
        return RF_ERR_UNSUPPORTED;
    }
    if (width * height > kVarMaxVolumeLines) {
        set_error("width * height = %lld is above %lld: a z scan indexes its lines in 32 bits", (long long)(width * height), (long long)kVarMaxVolumeLines);
        return RF_ERR_UNSUPPORTED;
    }
    if (depth * n_planes > kVarMaxGridZ) {
        set_error("depth * n_planes = %lld is above %lld: the slices of an x or y stage ride on gridDim.z beside the planes",
                  (long long)(depth * n_planes), (long long)kVarMaxGridZ);
        return RF_ERR_UNSUPPORTED;
    }
    return RF_OK;
}

int64_t var_max_extent() { return kVarMaxExtent; }

int build_var_plan(const rf_var_desc *desc, rf_var_plan **out, int batch) {
    if (!desc || !out) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    *out = nullptr;
    int rc = validate(desc);
    if (rc != RF_OK) return rc;
    return build_checked(desc, out, batch, false);
}

int build_var_signal_plan(const rf_var_signal_desc *desc, rf_var_plan **out) {
    if (!desc || !out) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    *out = nullptr;
    int rc = validate_signal(desc);
    if (rc != RF_OK) return rc;
    // the plan of a 1 x length image, whose stages run the signal kernels
    rf_var_desc d{};
    d.ndim = 2;
    d.abi = desc->abi;
    d.extent[0] = desc->length;
    d.extent[1] = 1;
    d.dtype = desc->dtype;
    d.n_planes = desc->n_planes;
    d.n_weights = desc->n_weights;
    d.n_scans = desc->n_scans;
    d.scans = desc->scans;
    d.device = desc->device;
    return build_checked(&d, out, 1, true);
}

int build_var_volume_plan(const rf_var_volume_desc *desc, rf_var_plan **out) {
    if (!desc || !out) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    *out = nullptr;
    int rc = validate_volume(desc);
    if (rc != RF_OK) return rc;
    // (ndim = 3 reaches build_checked from here alone: rf_var_plan_create refuses it)
    rf_var_desc d{};
    d.ndim = 3;
    d.abi = desc->abi;
    d.extent[0] = desc->width;
    d.extent[1] = desc->height;
    d.extent[2] = desc->depth;
    d.dtype = desc->dtype;
    d.n_planes = desc->n_planes;
    d.n_weights = desc->n_weights;
    d.n_scans = desc->n_scans;
    d.scans = desc->scans;
    d.device = desc->device;
    return build_checked(&d, out, 1, false);
}

namespace {

// the plan of a description that has passed its checks
int build_checked(const rf_var_desc *desc, rf_var_plan **out, int batch, bool signal) {
    const bool host_only = desc->device == RF_DEVICE_HOST_ONLY;
    int device = desc->device;
    if (!host_only) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("no HIP device available (this library has no CPU fallback)"); return RF_ERR_HIP; }
        if (device < 0) RF_HIP_CHECK(hipGetDevice(&device));
        if (device >= ndev) { set_error("device %d out of range (%d visible)", device, ndev); return RF_ERR_INVALID_ARG; }
    }
    std::unique_ptr<rf_var_plan> plan(new rf_var_plan);
    plan->width = desc->extent[0];
    plan->height = desc->extent[1];
    plan->n_planes = desc->n_planes;
    plan->n_weights = desc->n_weights;
    plan->batch = batch;
    plan->device = host_only ? 0 : device;
    plan->host_only = host_only;
    plan->signal = signal;
    plan->volume = desc->ndim == 3;
    plan->depth = plan->volume ? desc->extent[2] : 1;
    // Stages: the scans are taken in runs along one dimension.  A run that is exactly {+d, -d} on one weight plane is ONE fused
    // stage; every other run -- a single scan, -d +d, a pair on two weight planes, three or more scans along the dimension --
    // goes scan by scan (longer runs are not searched for pairs).
    bool used[3] = {false, false, false};
    auto add_stage = [&](int dim, int mode, int weights) {
        rf_var_stage st;
        st.dim = dim; st.mode = mode; st.weights = weights;
        used[dim] = true;
        push_stage_names(plan->names, "var_", dim, signal);
        plan->stages.push_back(st);
    };
    for (int s = 0; s < desc->n_scans;) {
        int e = s + 1;
        while (e < desc->n_scans && desc->scans[e].dim == desc->scans[s].dim) e++;
        const rf_var_scan_desc *run = desc->scans + s;
        if (e - s == 2 && run[0].causal != 0 && run[1].causal == 0 && run[0].weights == run[1].weights) {
            add_stage(run[0].dim, VAR_PAIR, run[0].weights);
        } else {
            for (int q = s; q < e; q++) add_stage(desc->scans[q].dim, desc->scans[q].causal != 0 ? VAR_CAUSAL : VAR_ANTICAUSAL, desc->scans[q].weights);
        }
        s = e;
    }
    // the adjoint's launch lists: [1] reruns the forward scan by scan first, and has one var_grad behind every adjoint stage
    plan->scans.assign(desc->scans, desc->scans + desc->n_scans);
    for (const rf_var_scan_desc &sc : plan->scans) push_stage_names(plan->backward_names[1], "var_", sc.dim, signal);
    for (int with = 0; with < 2; with++)
        for (int q = desc->n_scans - 1; q >= 0; q--) {
            push_stage_names(plan->backward_names[with], "var_adj_", desc->scans[q].dim, signal);
            if (with) plan->backward_names[with].push_back(desc->scans[q].dim == 0 ? "var_grad_x" : desc->scans[q].dim == 1 ? "var_grad_y" : "var_grad_z");
        }
    // tiles x lines of the dimension that needs more: x scans have `height` lines (per slice of a volume), y scans `width`, z
    // scans width * height
    int64_t slots = 0;
    if (used[0]) slots = std::max(slots, tiles_of(plan->width) * plan->height * plan->depth);
    if (used[1]) slots = std::max(slots, tiles_of(plan->height) * plan->width * plan->depth);
    if (used[2]) slots = std::max(slots, tiles_of(plan->depth) * plan->width * plan->height);
    int64_t carry_slots = slots;
    if (signal) {
        // a lane's map per tile and an aggregate per group of 64 tiles; carries per group
        carry_slots = (tiles_of(plan->width) + kVarGroupTiles - 1) / kVarGroupTiles;
        slots = tiles_of(plan->width) + carry_slots;
    }
    plan->tails_bytes = (size_t)(slots * kVarComponents * plan->n_planes) * sizeof(float) * (size_t)batch;
    plan->carry_bytes = (size_t)(carry_slots * 2 * plan->n_planes) * sizeof(float) * (size_t)batch;
    if (!host_only) {
        RF_HIP_CHECK(hipSetDevice(device));
        if (hipMalloc((void **)&plan->tails, plan->tails_bytes) != hipSuccess || hipMalloc((void **)&plan->carry, plan->carry_bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("hipMalloc of %zu bytes of workspace failed", plan->workspace_bytes());
            return RF_ERR_NOMEM;
        }
    }
    *out = plan.release();
    return RF_OK;
}

}  // namespace

int power_constants(const float *bases, int n_weights, float *log2_base, float *ln_base) {
    for (int k = 0; k < n_weights; k++) {
        if (!std::isfinite(bases[k]) || !(bases[k] > 0.0f && bases[k] < 1.0f)) {
            set_error("exponent plane %d: the base must be inside (0, 1) (got %g)", k, (double)bases[k]);
            return RF_ERR_INVALID_ARG;
        }
        log2_base[k] = (float)std::log2((double)bases[k]);
        ln_base[k] = (float)std::log((double)bases[k]);
    }
    return RF_OK;
}

namespace {

// The fields of a stage's arguments that the plan determines -- the workspace, the batch, the extents, the tiling along `dim` --
// with the stage's weight plane and mode.  The planes, their strides and the power form are the caller's.
VarArgs scan_args(const rf_var_plan *plan, int dim, const void *weights, int mode) {
    VarArgs a{};
    a.weights = (const float *)weights;
    a.tails = plan->tails;
    a.carry = plan->carry;
    a.batch = plan->batch;
    a.tails_stride = plan->image_tails_floats();
    a.carry_stride = plan->image_carry_floats();
    a.width = (int32_t)plan->width;
    a.height = (int32_t)plan->height;
    a.n_planes = plan->n_planes;
    a.tiles = (int32_t)tiles_of(dim == 0 ? plan->width : plan->height);
    a.lines = (int32_t)(dim == 0 ? plan->height : plan->width);
    a.mode = mode;
    if (plan->volume && dim == 2) {
        // the (width * height) x depth view: a voxel column per lane, rows width * height samples apart
        a.width = a.lines = (int32_t)(plan->width * plan->height);
        a.height = (int32_t)plan->depth;
        a.tiles = (int32_t)tiles_of(plan->depth);
    } else if (plan->volume) {
        // the slices as a batch, each with a slice's tails and carries in the single-image layout
        a.batch = (int32_t)plan->depth;
        a.tails_stride = (int64_t)a.tiles * kVarComponents * a.n_planes * a.lines;
        a.carry_stride = (int64_t)a.tiles * 2 * a.n_planes * a.lines;
    }
    return a;
}

// Samples from image to image of a stage's planes: the caller's stride -- or, in a volume plan, the slice stride of an x / y stage
// and nothing for a z stage, whose one image is the whole view.
int64_t stage_stride(const rf_var_plan *plan, int dim, int64_t callers) {
    return plan->volume ? (dim == 2 ? 0 : plan->width * plan->height) : callers;
}

// The three launches of a stage, a mark behind each.  a.dst_u8 is held back until the final pass: the tails pass stores no sample.
// signal: the plan of one long line (rf_var_plan_create_signal), whose three launches are kernels_var_signal.hip's.
int launch_stage(VarArgs &a, int dim, bool signal, hipStream_t stream, LaunchTimer &timer) {
    const int32_t dst_u8 = a.dst_u8;
    a.dst_u8 = 0;
    int rc = signal ? launch_var_signal_tails(a, stream) : launch_var_tails(a, dim, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc == RF_OK) rc = signal ? launch_var_signal_carry(a, stream) : launch_var_carry(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    a.dst_u8 = dst_u8;
    if (rc == RF_OK) rc = signal ? launch_var_signal_pass2(a, stream) : launch_var_pass2(a, dim, stream);
    if (rc == RF_OK) rc = timer.mark();
    return rc;
}

}  // namespace

int run_var_plan(rf_var_plan *plan, const void *const *in_planes, const void *const *weight_planes, const float *bases,
                 void *const *out_planes, hipStream_t stream, float *ms_out) {
    if (!plan || !in_planes || !weight_planes || !out_planes) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    float log2_base[RF_VAR_MAX_SCANS] = {}, ln_base[RF_VAR_MAX_SCANS] = {};
    int rc = bases ? power_constants(bases, plan->n_weights, log2_base, ln_base) : RF_OK;
    if (rc != RF_OK) return rc;
    if (plan->host_only) { set_error("host-only plan (RF_DEVICE_HOST_ONLY) cannot execute"); return RF_ERR_HIP; }
    const size_t plane_bytes = (size_t)plan->plane_samples() * sizeof(float);
    for (int pl = 0; pl < plan->n_planes; pl++) {
        rc = check_plane("plane", pl, {{in_planes[pl]}, {out_planes[pl]}}, 15u, "null image pointer", "the varying scans need 16-byte aligned image pointers");
        if (rc != RF_OK) return rc;
    }
    for (int k = 0; k < plan->n_weights; k++) {
        rc = check_plane("weight plane", k, {{weight_planes[k]}}, 15u, "null pointer", "the varying scans need 16-byte aligned pointers");
        if (rc != RF_OK) return rc;
        for (int pl = 0; pl < plan->n_planes; pl++)
            if (overlap(weight_planes[k], plane_bytes, out_planes[pl], plane_bytes)) {
                set_error("weight plane %d overlaps output plane %d: every stage reads the weights after it has begun to store", k, pl);
                return RF_ERR_INVALID_ARG;
            }
    }
    RF_HIP_CHECK(hipSetDevice(plan->device));
    LaunchTimer timer(stream, ms_out, plan->names.size());
    if (timer.status() != RF_OK) return timer.status();
    VarIo io{};
    io.in = in_planes;
    io.work = io.out = out_planes;
    rc = launch_var_stages(plan, io, weight_planes, bases ? log2_base : nullptr, stream, timer);
    return rc == RF_OK ? timer.finish() : rc;
}

int launch_var_stages(rf_var_plan *plan, const VarIo &io, const void *const *weight_planes, const float *log2_base, hipStream_t stream,
                      LaunchTimer &timer) {
    const size_t last = plan->stages.size() - 1;
    for (size_t s = 0; s <= last; s++) {
        const rf_var_stage &st = plan->stages[s];
        VarArgs a = scan_args(plan, st.dim, weight_planes[st.weights], st.mode);
        for (int pl = 0; pl < plan->n_planes; pl++) {
            a.src[pl] = s == 0 ? io.in[pl] : io.work[pl];
            a.dst[pl] = s == last ? io.out[pl] : io.work[pl];
        }
        a.src_u8 = s == 0 && io.in_u8;
        a.dst_u8 = s == last && io.out_u8;
        a.src_stride = stage_stride(plan, st.dim, s == 0 ? io.in_stride : io.work_stride);
        a.dst_stride = stage_stride(plan, st.dim, s == last ? io.out_stride : io.work_stride);
        a.weights_stride = stage_stride(plan, st.dim, io.weights_stride);
        a.power = log2_base ? 1 : 0;
        a.log2_base = log2_base ? log2_base[st.weights] : 0.0f;
        int rc = launch_stage(a, st.dim, plan->signal, stream, timer);
        if (rc != RF_OK) return rc;
    }
    return RF_OK;
}

int run_var_backward(rf_var_plan *plan, const void *const *in_planes, const void *const *weight_planes, const float *bases,
                     const void *const *grad_out_planes, void *const *grad_in_planes, void *const *grad_weight_planes, hipStream_t stream,
                     float *ms_out) {
    // refusals, in the order recfilter_amd.h documents; nothing of HIP is called before the last of them
    if (!plan || !weight_planes || !grad_out_planes || !grad_in_planes) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    bool with_weights = false;
    if (grad_weight_planes)
        for (int k = 0; k < plan->n_weights; k++) with_weights = with_weights || grad_weight_planes[k] != nullptr;
    if (with_weights && !in_planes) { set_error("weight gradients need the input planes (in_planes is null)"); return RF_ERR_INVALID_ARG; }
    float log2_base[RF_VAR_MAX_SCANS] = {}, ln_base[RF_VAR_MAX_SCANS] = {};
    int rc = bases ? power_constants(bases, plan->n_weights, log2_base, ln_base) : RF_OK;
    if (rc != RF_OK) return rc;
    if (plan->host_only) { set_error("host-only plan (RF_DEVICE_HOST_ONLY) cannot execute"); return RF_ERR_HIP; }
    const int P = plan->n_planes, K = plan->n_weights;
    const size_t plane_bytes = (size_t)plan->plane_samples() * sizeof(float);
    for (int pl = 0; pl < P; pl++) {
        rc = check_plane("plane", pl, {{grad_out_planes[pl]}, {grad_in_planes[pl]}, {with_weights ? in_planes[pl] : nullptr, with_weights}}, 15u,
                         "null image pointer", "the varying scans need 16-byte aligned image pointers");
        if (rc != RF_OK) return rc;
    }
    for (int k = 0; k < K; k++) {
        rc = check_plane("weight plane", k, {{weight_planes[k]}, {with_weights ? grad_weight_planes[k] : nullptr, false}}, 15u, "null pointer",
                         "the varying scans need 16-byte aligned pointers (the plane and its gradient)");
        if (rc != RF_OK) return rc;
    }
    // what is written (grad_in planes, weight-gradient planes) against everything that is read and everything else that is written
    const PlaneList written[2] = {{"grad_in", (const void *const *)grad_in_planes, P, plane_bytes},
                                  {"gradient of weight", (const void *const *)grad_weight_planes, with_weights ? K : 0, plane_bytes}};
    const PlaneList read[2] = {{"weight", weight_planes, K, plane_bytes, ": every stage reads the weights after it has begun to store"},
                               {"input", in_planes, in_planes ? P : 0, plane_bytes}};
    rc = check_written_planes(written, 2, read, 2, {"grad_out", grad_out_planes, P, plane_bytes});
    if (rc != RF_OK) return rc;
    RF_HIP_CHECK(hipSetDevice(plan->device));
    if (with_weights) {
        rc = ensure_var_grad_planes(plan);
        if (rc != RF_OK) return rc;
    }
    LaunchTimer timer(stream, ms_out, plan->backward_names[with_weights ? 1 : 0].size());
    if (timer.status() != RF_OK) return timer.status();
    VarBackwardIo io{};
    io.in = in_planes;
    io.weights = weight_planes;
    io.grad_out = grad_out_planes;
    io.grad_in = grad_in_planes;
    io.grad_weights = with_weights ? grad_weight_planes : nullptr;
    io.log2_base = bases ? log2_base : nullptr;
    io.ln_base = bases ? ln_base : nullptr;
    rc = launch_var_backward(plan, io, stream, timer);
    return rc == RF_OK ? timer.finish() : rc;
}

int ensure_var_grad_planes(rf_var_plan *plan) {
    if (plan->grad_planes) return RF_OK;
    if (hipMalloc((void **)&plan->grad_planes, plan->backward_workspace_bytes(true)) != hipSuccess) {
        (void)hipGetLastError();
        plan->grad_planes = nullptr;
        set_error("hipMalloc of %zu bytes for the weight gradients' planes failed", plan->backward_workspace_bytes(true));
        return RF_ERR_NOMEM;
    }
    return RF_OK;
}

int launch_var_backward(rf_var_plan *plan, const VarBackwardIo &io, hipStream_t stream, LaunchTimer &timer) {
    const int P = plan->n_planes, S = (int)plan->scans.size();
    const bool with_weights = io.grad_weights != nullptr, power = io.log2_base != nullptr;
    const size_t plane_floats = (size_t)plan->plane_samples();
    // [scan][image][plane]; scan == S: the state
    auto saved = [&](int scan, int pl) { return plan->grad_planes + ((size_t)scan * (size_t)plan->batch * P + pl) * plane_floats; };
    const int64_t saved_stride = (int64_t)P * (int64_t)plane_floats;
    // one single-scan stage's arguments, planes aside
    auto stage_args = [&](const rf_var_scan_desc &sc, int mode) {
        VarArgs a = scan_args(plan, sc.dim, io.weights[sc.weights], mode);
        a.power = power ? 1 : 0;
        a.log2_base = power ? io.log2_base[sc.weights] : 0.0f;
        a.weights_stride = stage_stride(plan, sc.dim, io.weights_stride);
        return a;
    };
    int rc = RF_OK;
    if (with_weights) {
        // the forward again, scan by scan, every output kept: scan q reads scan q-1's planes
        for (int q = 0; q < S && rc == RF_OK; q++) {
            const rf_var_scan_desc &sc = plan->scans[q];
            VarArgs a = stage_args(sc, sc.causal != 0 ? VAR_CAUSAL : VAR_ANTICAUSAL);
            for (int pl = 0; pl < P; pl++) {
                a.src[pl] = q == 0 ? io.in[pl] : saved(q - 1, pl);
                a.dst[pl] = saved(q, pl);
            }
            a.src_stride = stage_stride(plan, sc.dim, q == 0 ? io.in_stride : saved_stride);
            a.dst_stride = stage_stride(plan, sc.dim, saved_stride);
            rc = launch_stage(a, sc.dim, plan->signal, stream, timer);
        }
    }
    bool touched[RF_VAR_MAX_SCANS] = {};
    if (io.holds_sum)
        for (int k = 0; k < plan->n_weights; k++) touched[k] = io.holds_sum[k];
    for (int q = S - 1; q >= 0 && rc == RF_OK; q--) {
        const rf_var_scan_desc &sc = plan->scans[q];
        float *const grad = with_weights ? (float *)io.grad_weights[sc.weights] : nullptr;
        // the adjoint of a causal scan runs anticausally, and the other way round
        VarArgs a = stage_args(sc, sc.causal != 0 ? VAR_ANTICAUSAL : VAR_CAUSAL);
        a.adjoint = 1;
        for (int pl = 0; pl < P; pl++) {
            a.src[pl] = q == S - 1 ? io.grad_out[pl] : io.grad_in[pl];
            a.dst[pl] = io.grad_in[pl];
            a.lam[pl] = grad ? saved(S, pl) : nullptr;
        }
        a.src_stride = stage_stride(plan, sc.dim, q == S - 1 ? io.grad_out_stride : io.grad_in_stride);
        a.dst_stride = stage_stride(plan, sc.dim, io.grad_in_stride);
        a.lam_stride = stage_stride(plan, sc.dim, saved_stride);
        rc = launch_stage(a, sc.dim, plan->signal, stream, timer);
        if (rc != RF_OK || !with_weights) continue;
        if (grad) {                                   // (a weight plane without a gradient: no launch, its slot reports 0 ms)
            VarGradArgs g{};
            for (int pl = 0; pl < P; pl++) {
                g.lam[pl] = saved(S, pl);
                g.x[pl] = q == 0 ? (const float *)io.in[pl] : saved(q - 1, pl);
                g.y[pl] = saved(q, pl);
            }
            g.grad = grad;
            g.width = a.width;                  // (a volume: the stage's view and its batch of slices)
            g.height = a.height;
            g.n_planes = P;
            g.batch = a.batch;
            g.lam_stride = g.y_stride = stage_stride(plan, sc.dim, saved_stride);
            g.x_stride = stage_stride(plan, sc.dim, q == 0 ? io.in_stride : saved_stride);
            g.grad_stride = stage_stride(plan, sc.dim, io.grad_weights_stride);
            g.exponents_stride = stage_stride(plan, sc.dim, io.weights_stride);
            g.accumulate = touched[sc.weights] ? 1 : 0;
            if (power) {
                g.exponents = (const float *)io.weights[sc.weights];
                g.log2_base = io.log2_base[sc.weights];
                g.ln_base = io.ln_base[sc.weights];
            }
            touched[sc.weights] = true;
            rc = launch_var_grad(g, sc.dim, sc.causal != 0, stream);
        } else {
            timer.skip();
        }
        if (rc == RF_OK) rc = timer.mark();
    }
    return rc;
}

namespace {

// What run_var_distances and run_var_distances_backward refuse alike, in three parts: each checks pointers of its own (and the
// backward `accumulate`) between them.  `kernel` names the launch in the message.
int check_distance_counts(int32_t n_guide, int64_t width, int64_t height) {
    if (n_guide < 1 || n_guide > RF_MAX_PLANES) { set_error("n_guide must be 1..%d (got %d)", RF_MAX_PLANES, n_guide); return RF_ERR_INVALID_ARG; }
    if (width < 1 || height < 1) { set_error("width and height must be positive"); return RF_ERR_INVALID_ARG; }
    return RF_OK;
}

int check_distance_scale(float scale) {
    if (!std::isfinite(scale) || scale < 0.0f) { set_error("scale must be finite and not negative (got %g)", (double)scale); return RF_ERR_INVALID_ARG; }
    return RF_OK;
}

int check_distance_extents(const char *kernel, int64_t width, int64_t height) {
    if (width % 4 != 0) {
        set_error("%s moves 16 bytes per lane along x: the width must be a multiple of 4 (got %lld)", kernel, (long long)width);
        return RF_ERR_UNSUPPORTED;
    }
    if (width > kVarMaxExtent || height > kVarMaxExtent) {
        set_error("extents %lld x %lld are above %lld", (long long)width, (long long)height, (long long)kVarMaxExtent);
        return RF_ERR_UNSUPPORTED;
    }
    return RF_OK;
}

// the first refusals of run_var_distances_volume and run_var_distances_volume_backward; both go on to check_distance_scale and
// check_volume_extents (n_planes = 1) behind pointer checks of their own
int check_volume_distance_counts(int32_t n_guide, int64_t width, int64_t height, int64_t depth) {
    if (n_guide < 1 || n_guide > RF_MAX_PLANES) { set_error("n_guide must be 1..%d (got %d)", RF_MAX_PLANES, n_guide); return RF_ERR_INVALID_ARG; }
    if (width < 1 || height < 1 || depth < 1) { set_error("width, height and depth must be positive"); return RF_ERR_INVALID_ARG; }
    return RF_OK;
}

}  // namespace

int run_var_distances(const void *const *guide_planes, int32_t n_guide, int32_t guide_u8, int64_t width, int64_t height, float scale,
                      void *dx, void *dy, int32_t device, hipStream_t stream, int32_t batch, int64_t guide_stride) {
    int rc = check_distance_counts(n_guide, width, height);
    if (rc != RF_OK) return rc;
    if (!guide_planes || !dx || !dy) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    for (int ch = 0; ch < n_guide; ch++)
        if (!guide_planes[ch]) { set_error("guide plane %d: null pointer", ch); return RF_ERR_INVALID_ARG; }
    rc = check_distance_scale(scale);
    if (rc == RF_OK) rc = check_distance_extents("var_distances", width, height);
    if (rc != RF_OK) return rc;
    if ((((uintptr_t)dx | (uintptr_t)dy) & 15u) != 0) { set_error("dx and dy must be 16-byte aligned"); return RF_ERR_INVALID_ARG; }
    const uintptr_t guide_align = guide_u8 ? 3u : 15u;
    for (int ch = 0; ch < n_guide; ch++)
        if (((uintptr_t)guide_planes[ch] & guide_align) != 0) {
            set_error("guide plane %d: %s guide planes must be %u-byte aligned", ch, guide_u8 ? "uint8" : "f32", (unsigned)guide_align + 1);
            return RF_ERR_INVALID_ARG;
        }
    const size_t samples = (size_t)(width * height), out_bytes = samples * sizeof(float), guide_bytes = samples * (guide_u8 ? 1 : sizeof(float));
    if (overlap(dx, out_bytes * (size_t)batch, dy, out_bytes * (size_t)batch)) { set_error("dx overlaps dy"); return RF_ERR_INVALID_ARG; }
    // (a batch comes from plan_smooth.cpp: dx and dy are the plan's own planes, which no plane of a caller overlaps)
    for (int ch = 0; ch < n_guide && batch == 1; ch++)
        if (overlap(dx, out_bytes, guide_planes[ch], guide_bytes) || overlap(dy, out_bytes, guide_planes[ch], guide_bytes)) {
            set_error("guide plane %d overlaps dx or dy: a lane reads its neighbours' samples", ch);
            return RF_ERR_INVALID_ARG;
        }
    if (device >= 0) RF_HIP_CHECK(hipSetDevice(device));
    VarDistArgs a{};
    for (int ch = 0; ch < n_guide; ch++) a.guide[ch] = guide_planes[ch];
    a.dx = (float *)dx;
    a.dy = (float *)dy;
    a.width = (int32_t)width;
    a.height = (int32_t)height;
    a.n_guide = n_guide;
    a.scale = scale;
    a.batch = batch;
    a.guide_stride = guide_stride;
    return launch_var_distances(a, guide_u8 != 0, stream);
}

int run_var_distances_volume(const void *const *guide_volumes, int32_t n_guide, int32_t guide_u8, int64_t width, int64_t height, int64_t depth,
                             float scale, float spacing_z, void *dx, void *dy, void *dz, int32_t device, hipStream_t stream) {
    int rc = check_volume_distance_counts(n_guide, width, height, depth);
    if (rc != RF_OK) return rc;
    if (!guide_volumes || !dx || !dy || !dz) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    for (int ch = 0; ch < n_guide; ch++)
        if (!guide_volumes[ch]) { set_error("guide volume %d: null pointer", ch); return RF_ERR_INVALID_ARG; }
    rc = check_distance_scale(scale);
    if (rc != RF_OK) return rc;
    if (!std::isfinite(spacing_z) || !(spacing_z > 0.0f)) { set_error("spacing_z must be finite and positive (got %g)", (double)spacing_z); return RF_ERR_INVALID_ARG; }
    rc = check_volume_extents(width, height, depth, 1);
    if (rc != RF_OK) return rc;
    if ((((uintptr_t)dx | (uintptr_t)dy | (uintptr_t)dz) & 15u) != 0) { set_error("dx, dy and dz must be 16-byte aligned"); return RF_ERR_INVALID_ARG; }
    const uintptr_t guide_align = guide_u8 ? 3u : 15u;
    for (int ch = 0; ch < n_guide; ch++)
        if (((uintptr_t)guide_volumes[ch] & guide_align) != 0) {
            set_error("guide volume %d: %s guide volumes must be %u-byte aligned", ch, guide_u8 ? "uint8" : "f32", (unsigned)guide_align + 1);
            return RF_ERR_INVALID_ARG;
        }
    const size_t samples = (size_t)(width * height * depth), out_bytes = samples * sizeof(float), guide_bytes = samples * (guide_u8 ? 1 : sizeof(float));
    if (overlap(dx, out_bytes, dy, out_bytes) || overlap(dx, out_bytes, dz, out_bytes) || overlap(dy, out_bytes, dz, out_bytes)) {
        set_error("dx, dy and dz overlap each other");
        return RF_ERR_INVALID_ARG;
    }
    for (int ch = 0; ch < n_guide; ch++)
        if (overlap(dx, out_bytes, guide_volumes[ch], guide_bytes) || overlap(dy, out_bytes, guide_volumes[ch], guide_bytes) ||
            overlap(dz, out_bytes, guide_volumes[ch], guide_bytes)) {
            set_error("guide volume %d overlaps dx, dy or dz: a lane reads its neighbours' samples", ch);
            return RF_ERR_INVALID_ARG;
        }
    if (device >= 0) RF_HIP_CHECK(hipSetDevice(device));
    VarDistVolumeArgs a{};
    for (int ch = 0; ch < n_guide; ch++) a.guide[ch] = guide_volumes[ch];
    a.dx = (float *)dx;
    a.dy = (float *)dy;
    a.dz = (float *)dz;
    a.width = (int32_t)width;
    a.height = (int32_t)height;
    a.depth = (int32_t)depth;
    a.n_guide = n_guide;
    a.scale = scale;
    a.spacing_z = spacing_z;
    return launch_var_distances_volume(a, guide_u8 != 0, stream);
}

int run_var_distances_backward(const void *const *guide_planes, int32_t n_guide, int64_t width, int64_t height, float scale, const void *grad_dx,
                               const void *grad_dy, void *const *grad_guide_planes, int32_t accumulate, int32_t device, hipStream_t stream,
                               int32_t batch, int64_t guide_stride, int64_t grad_guide_stride) {
    int rc = check_distance_counts(n_guide, width, height);
    if (rc != RF_OK) return rc;
    if (!guide_planes || !grad_dx || !grad_dy || !grad_guide_planes) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    for (int ch = 0; ch < n_guide; ch++)
        if (!guide_planes[ch] || !grad_guide_planes[ch]) { set_error("guide plane %d: null pointer (the plane or its gradient)", ch); return RF_ERR_INVALID_ARG; }
    rc = check_distance_scale(scale);
    if (rc != RF_OK) return rc;
    if (accumulate != 0 && accumulate != 1) { set_error("accumulate must be 0 or 1 (got %d)", accumulate); return RF_ERR_INVALID_ARG; }
    rc = check_distance_extents("var_distances_grad", width, height);
    if (rc != RF_OK) return rc;
    if ((((uintptr_t)grad_dx | (uintptr_t)grad_dy) & 15u) != 0) { set_error("grad_dx and grad_dy must be 16-byte aligned"); return RF_ERR_INVALID_ARG; }
    for (int ch = 0; ch < n_guide; ch++)
        if ((((uintptr_t)guide_planes[ch] | (uintptr_t)grad_guide_planes[ch]) & 15u) != 0) {
            set_error("guide plane %d: f32 guide planes and their gradients must be 16-byte aligned", ch);
            return RF_ERR_INVALID_ARG;
        }
    // a gradient plane is written while other lanes still read: it overlaps nothing that is read and no other gradient plane
    // (a batch comes from plan_smooth.cpp, which has checked every extent of the caller's against every other, sorted; grad_dx and
    // grad_dy are then the plan's own planes)
    const size_t bytes = (size_t)(width * height) * sizeof(float);
    for (int ch = 0; ch < n_guide && batch == 1; ch++) {
        const void *o = grad_guide_planes[ch];
        if (overlap(o, bytes, grad_dx, bytes) || overlap(o, bytes, grad_dy, bytes)) {
            set_error("gradient of guide plane %d overlaps grad_dx or grad_dy: a lane reads its neighbours' samples", ch);
            return RF_ERR_INVALID_ARG;
        }
        for (int q = 0; q < n_guide; q++) {
            if (overlap(o, bytes, guide_planes[q], bytes)) {
                set_error("gradient of guide plane %d overlaps guide plane %d: a lane reads its neighbours' samples", ch, q);
                return RF_ERR_INVALID_ARG;
            }
            if (q > ch && overlap(o, bytes, grad_guide_planes[q], bytes)) {
                set_error("gradient of guide plane %d overlaps gradient of guide plane %d", ch, q);
                return RF_ERR_INVALID_ARG;
            }
        }
    }
    if (device >= 0) RF_HIP_CHECK(hipSetDevice(device));
    VarDistGradArgs a{};
    for (int ch = 0; ch < n_guide; ch++) {
        a.guide[ch] = (const float *)guide_planes[ch];
        a.grad_guide[ch] = (float *)grad_guide_planes[ch];
    }
    a.gdx = (const float *)grad_dx;
    a.gdy = (const float *)grad_dy;
    a.width = (int32_t)width;
    a.height = (int32_t)height;
    a.n_guide = n_guide;
    a.accumulate = accumulate;
    a.scale = scale;
    a.batch = batch;
    a.guide_stride = guide_stride;
    a.grad_guide_stride = grad_guide_stride;
    return launch_var_distances_grad(a, stream);
}

int run_var_distances_volume_backward(const void *const *guide_volumes, int32_t n_guide, int64_t width, int64_t height, int64_t depth, float scale,
                                      const void *grad_dx, const void *grad_dy, const void *grad_dz, void *const *grad_guide_volumes,
                                      int32_t accumulate, int32_t device, hipStream_t stream) {
    int rc = check_volume_distance_counts(n_guide, width, height, depth);
    if (rc != RF_OK) return rc;
    if (!guide_volumes || !grad_dx || !grad_dy || !grad_dz || !grad_guide_volumes) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    for (int ch = 0; ch < n_guide; ch++)
        if (!guide_volumes[ch] || !grad_guide_volumes[ch]) { set_error("guide volume %d: null pointer (the volume or its gradient)", ch); return RF_ERR_INVALID_ARG; }
    rc = check_distance_scale(scale);
    if (rc == RF_OK) rc = check_volume_extents(width, height, depth, 1);
    if (rc != RF_OK) return rc;
    if (accumulate != 0 && accumulate != 1) { set_error("accumulate must be 0 or 1 (got %d)", accumulate); return RF_ERR_INVALID_ARG; }
    if ((((uintptr_t)grad_dx | (uintptr_t)grad_dy | (uintptr_t)grad_dz) & 15u) != 0) { set_error("grad_dx, grad_dy and grad_dz must be 16-byte aligned"); return RF_ERR_INVALID_ARG; }
    for (int ch = 0; ch < n_guide; ch++)
        if ((((uintptr_t)guide_volumes[ch] | (uintptr_t)grad_guide_volumes[ch]) & 15u) != 0) {
            set_error("guide volume %d: f32 guide volumes and their gradients must be 16-byte aligned", ch);
            return RF_ERR_INVALID_ARG;
        }
    // a gradient volume is written while other lanes still read: it overlaps nothing that is read and no other gradient volume
    const size_t bytes = (size_t)(width * height * depth) * sizeof(float);
    for (int ch = 0; ch < n_guide; ch++) {
        const void *o = grad_guide_volumes[ch];
        if (overlap(o, bytes, grad_dx, bytes) || overlap(o, bytes, grad_dy, bytes) || overlap(o, bytes, grad_dz, bytes)) {
            set_error("gradient of guide volume %d overlaps grad_dx, grad_dy or grad_dz: a lane reads its neighbours' samples", ch);
            return RF_ERR_INVALID_ARG;
        }
        for (int q = 0; q < n_guide; q++) {
            if (overlap(o, bytes, guide_volumes[q], bytes)) {
                set_error("gradient of guide volume %d overlaps guide volume %d: a lane reads its neighbours' samples", ch, q);
                return RF_ERR_INVALID_ARG;
            }
            if (q > ch && overlap(o, bytes, grad_guide_volumes[q], bytes)) {
                set_error("gradient of guide volume %d overlaps gradient of guide volume %d", ch, q);
                return RF_ERR_INVALID_ARG;
            }
        }
    }
    if (device >= 0) RF_HIP_CHECK(hipSetDevice(device));
    VarDistVolumeGradArgs a{};
    for (int ch = 0; ch < n_guide; ch++) {
        a.guide[ch] = (const float *)guide_volumes[ch];
        a.grad_guide[ch] = (float *)grad_guide_volumes[ch];
    }
    a.gdx = (const float *)grad_dx;
    a.gdy = (const float *)grad_dy;
    a.gdz = (const float *)grad_dz;
    a.width = (int32_t)width;
    a.height = (int32_t)height;
    a.depth = (int32_t)depth;
    a.n_guide = n_guide;
    a.accumulate = accumulate;
    a.scale = scale;
    return launch_var_distances_volume_grad(a, stream);
}

}  // namespace rf
