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
// With the gradient of the bases (rf_var_plan_backward_power_bases) the var_grad launches are the base-reducing ones, each on its own
// segment of plan-owned f64 slabs, and one var_param_sum launch behind them stores dL/dbases to the caller's device buffer.
// run_var_backward checks and constructs the timer; launch_var_backward issues the launches, and is what the smoothing plan's
// backward (plan_smooth.cpp) calls per iteration -- with planes that already hold a sum after the first.
//
// The three public descriptions (rf_var_desc, rf_var_signal_desc, rf_var_volume_desc) are lowered to one form, an rf_var_desc
// (`lowered`), and checked by one validator: what differs between the kinds -- the struct's name in the messages, the noun, the
// highest dim, the accepted domain -- is a VarKind record.  build_checked builds the plan of a lowered description.
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
// the distances of a volume and plan_smooth.cpp.
//
// The distances (rf_var_distances, rf_var_distances_volume) and their adjoints, one launch each, take one argument record,
// DistanceCall: two planes or three, written or read.  The refusals are small steps over that record; each of the four entry points
// lists its steps in its own documented order (run_distance_steps) and ends in run_distances_forward or run_distances_backward,
// which hold the alignment and overlap checks -- loops over the two or three planes -- and fill the kernels' argument structs.
#include "plan_var.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <memory>

rf_var_plan::~rf_var_plan() {
    if (tails) (void)hipFree(tails);
    if (grad_planes) (void)hipFree(grad_planes);
    if (bases_slabs) (void)hipFree(bases_slabs);
    if (carry) (void)hipFree(carry);
}

namespace rf {

namespace {

constexpr int64_t kVarMaxExtent = int64_t(1) << 21;      // 64 lines or samples per workgroup along grid.y (65535 workgroups)

constexpr int64_t kVarMaxSignal = int64_t(1) << 30;      // samples of a signal: indices and 4096-sample groups stay inside int32

// The accepted domain of each kind of description, on its lowered form (rf_var_desc: see lowered below).
int check_image_domain(const rf_var_desc *d) {
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

int check_signal_domain(const rf_var_desc *d) {
    const long long length = (long long)d->extent[0];
    if (length < 1) { set_error("length must be positive (got %lld)", length); return RF_ERR_INVALID_ARG; }
    if (length > kVarMaxSignal) { set_error("length = %lld is above %lld", length, (long long)kVarMaxSignal); return RF_ERR_UNSUPPORTED; }
    if (length % 4 != 0) { set_error("varying scans move 16 bytes per lane: length must be a multiple of 4 (got %lld)", length); return RF_ERR_UNSUPPORTED; }
    return RF_OK;
}

int check_volume_domain(const rf_var_desc *d) { return check_volume_extents(d->extent[0], d->extent[1], d->extent[2], d->n_planes); }

// What the three kinds of description differ in, to the one validator: the public struct's name (the abi and flags messages), the
// noun of the dtype message, the ndim of the lowered form, the highest dim of a scan with its message, and the domain.
struct VarKind {
    const char *struct_name, *noun;
    int ndim, max_dim;
    const char *dim_message;
    int (*check_domain)(const rf_var_desc *);
    bool signal;
};
const VarKind kImageKind = {"rf_var_desc", "planes", 2, 1, "scan %d: dim must be 0 or 1 (got %d)", check_image_domain, false};
const VarKind kSignalKind = {"rf_var_signal_desc", "signals", 2, 0, "scan %d: dim must be 0 on a signal (got %d)", check_signal_domain, true};
const VarKind kVolumeKind = {"rf_var_volume_desc", "volumes", 3, 2, "scan %d: dim must be 0, 1 or 2 on a volume (got %d)", check_volume_domain, false};

int validate(const rf_var_desc *d, const VarKind &kind) {
    if (d->abi != RF_ABI) {
        set_error("%s.abi is %u, this library speaks revision %u of recfilter_amd.h", kind.struct_name, d->abi, RF_ABI);
        return RF_ERR_INVALID_ARG;
    }
    if (d->flags != 0) { set_error("%s.flags must be 0 (got %#x)", kind.struct_name, d->flags); return RF_ERR_INVALID_ARG; }
    if (d->n_planes < 1 || d->n_planes > RF_MAX_PLANES) { set_error("n_planes must be 1..%d (got %d)", RF_MAX_PLANES, d->n_planes); return RF_ERR_INVALID_ARG; }
    if (d->n_weights < 1 || d->n_weights > RF_VAR_MAX_SCANS) { set_error("n_weights must be 1..%d (got %d)", RF_VAR_MAX_SCANS, d->n_weights); return RF_ERR_INVALID_ARG; }
    if (d->n_scans < 1 || d->n_scans > RF_VAR_MAX_SCANS) { set_error("n_scans must be 1..%d (got %d)", RF_VAR_MAX_SCANS, d->n_scans); return RF_ERR_INVALID_ARG; }
    if (!d->scans) { set_error("null scans"); return RF_ERR_INVALID_ARG; }
    // (only rf_var_desc has an ndim of its caller's: rf_var_plan_create takes images, and ndim = 3 comes from a volume description alone)
    if (d->ndim != kind.ndim) { set_error("varying scans take 2-D images (ndim = %d)", d->ndim); return RF_ERR_UNSUPPORTED; }
    if (d->dtype != RF_F32) { set_error("varying scans take f32 %s (dtype = %d)", kind.noun, d->dtype); return RF_ERR_UNSUPPORTED; }
    for (int s = 0; s < d->n_scans; s++) {
        const rf_var_scan_desc &sc = d->scans[s];
        if (sc.dim < 0 || sc.dim > kind.max_dim) { set_error(kind.dim_message, s, sc.dim); return RF_ERR_INVALID_ARG; }
        if (sc.weights < 0 || sc.weights >= d->n_weights) {
            set_error("scan %d: weights must be 0..%d (got %d)", s, d->n_weights - 1, sc.weights);
            return RF_ERR_INVALID_ARG;
        }
    }
    return kind.check_domain(d);
}

// The canonical form of a signal or volume description: an rf_var_desc of `ndim` dimensions with the fields all three share.
template <class Desc>
rf_var_desc lowered(const Desc &p, int ndim, int64_t width, int64_t height, int64_t depth) {
    rf_var_desc d{};
    d.ndim = ndim;
    d.abi = p.abi;
    d.extent[0] = width;
    d.extent[1] = height;
    d.extent[2] = depth;
    d.dtype = p.dtype;
    d.n_planes = p.n_planes;
    d.n_weights = p.n_weights;
    d.n_scans = p.n_scans;
    d.scans = p.scans;
    d.device = p.device;
    d.flags = p.flags;
    return d;
}

int64_t tiles_of(int64_t n) { return (n + kVarTile - 1) / kVarTile; }

// the three launches of a stage along `dim` (a signal plan: "1d"); prefix: "var_", or "var_adj_" for an adjoint stage
void push_stage_names(std::vector<std::string> &names, const char *prefix, int dim, bool signal) {
    const char *axis = signal ? "1d" : dim == 0 ? "x" : dim == 1 ? "y" : "z";
    names.push_back(std::string(prefix) + "tails_" + axis);
    names.push_back(signal ? "var_carry_1d" : "var_carry");
    names.push_back(std::string(prefix) + "pass2_" + axis);
}

constexpr int64_t kVarMaxVolumeLines = int64_t(1) << 30;      // width * height: the z view's line index is an int32
constexpr int64_t kVarMaxGridZ = 65535;                        // depth * n_planes: the slices ride on gridDim.z beside the planes

int build_checked(const rf_var_desc *desc, rf_var_plan **out, int batch, bool signal);
VarArgs scan_args(const rf_var_plan *plan, int dim, const void *weights, int mode);

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

namespace {
// every build_var_*_plan behind its null check: the lowered description validated as its kind, then built
int build_lowered(const rf_var_desc &d, const VarKind &kind, rf_var_plan **out, int batch) {
    *out = nullptr;
    const int rc = validate(&d, kind);
    return rc == RF_OK ? build_checked(&d, out, batch, kind.signal) : rc;
}
int refuse_null() { set_error("null argument"); return RF_ERR_INVALID_ARG; }
}  // namespace

int build_var_plan(const rf_var_desc *desc, rf_var_plan **out, int batch) {
    return desc && out ? build_lowered(*desc, kImageKind, out, batch) : refuse_null();
}

// the plan of a 1 x length image, whose stages run the signal kernels
int build_var_signal_plan(const rf_var_signal_desc *desc, rf_var_plan **out) {
    return desc && out ? build_lowered(lowered(*desc, 2, desc->length, 1, 0), kSignalKind, out, 1) : refuse_null();
}

int build_var_volume_plan(const rf_var_volume_desc *desc, rf_var_plan **out) {
    return desc && out ? build_lowered(lowered(*desc, 3, desc->width, desc->height, desc->depth), kVolumeKind, out, 1) : refuse_null();
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
    // the base-reducing route: the names above and the sum; a slab entry per workgroup of every scan's var_grad launch, whose
    // grid is that of the scan's stage (a volume: the view of a z stage, the slices of an x / y stage as its batch)
    plan->backward_bases_names = plan->backward_names[1];
    plan->backward_bases_names.push_back("var_param_sum");
    plan->bases_slab_offset.assign(1, 0);
    for (const rf_var_scan_desc &sc : plan->scans) {
        const VarArgs a = scan_args(plan.get(), sc.dim, nullptr, VAR_CAUSAL);
        plan->bases_slab_offset.push_back(plan->bases_slab_offset.back() + var_grad_blocks(a.width, a.height, a.batch));
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
                     float *ms_out, bool with_bases, double *grad_bases) {
    // refusals, in the order recfilter_amd.h documents; nothing of HIP is called before the last of them
    if (!plan || !weight_planes || !grad_out_planes || !grad_in_planes) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    if (with_bases && !bases) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    bool with_weights = with_bases;                   // (the base gradient takes the weight-gradient route, planes or none)
    void *const no_planes[RF_VAR_MAX_SCANS] = {};
    if (!grad_weight_planes && with_bases) grad_weight_planes = no_planes;
    if (grad_weight_planes)
        for (int k = 0; k < plan->n_weights; k++) with_weights = with_weights || grad_weight_planes[k] != nullptr;
    if (with_weights && !in_planes) { set_error("weight gradients need the input planes (in_planes is null)"); return RF_ERR_INVALID_ARG; }
    if (with_bases) {
        if (!grad_bases) { set_error("null grad_bases"); return RF_ERR_INVALID_ARG; }
        if (((uintptr_t)grad_bases & 7u) != 0) { set_error("grad_bases must be 8-byte aligned: it receives n_weights doubles"); return RF_ERR_INVALID_ARG; }
    }
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
    if (with_bases) {
        rc = ensure_var_bases_slabs(plan);
        if (rc != RF_OK) return rc;
    }
    LaunchTimer timer(stream, ms_out, with_bases ? plan->backward_bases_names.size() : plan->backward_names[with_weights ? 1 : 0].size());
    if (timer.status() != RF_OK) return timer.status();
    VarBackwardIo io{};
    io.in = in_planes;
    io.weights = weight_planes;
    io.grad_out = grad_out_planes;
    io.grad_in = grad_in_planes;
    io.grad_weights = with_weights ? grad_weight_planes : nullptr;
    io.log2_base = bases ? log2_base : nullptr;
    io.ln_base = bases ? ln_base : nullptr;
    io.slabs = with_bases ? plan->bases_slabs : nullptr;
    rc = launch_var_backward(plan, io, stream, timer);
    if (rc == RF_OK && with_bases) {
        // dL/dbase_k = (1 / base_k) * the slabs of the scans that read plane k, scan by scan in index order
        VarParamSumArgs p{};
        p.slabs = plan->bases_slabs;
        p.out = grad_bases;
        p.n_out = K;
        p.n_segments = (int32_t)plan->scans.size();
        for (int q = 0; q < p.n_segments; q++) {
            p.offset[q] = plan->bases_slab_offset[q];
            p.count[q] = plan->bases_slab_offset[q + 1] - plan->bases_slab_offset[q];
            p.target[q] = plan->scans[q].weights;
            p.target2[q] = -1;
            p.factor[q] = 1.0 / (double)bases[p.target[q]];
        }
        rc = launch_var_param_sum(p, stream);
        if (rc == RF_OK) rc = timer.mark();
    }
    return rc == RF_OK ? timer.finish() : rc;
}

int ensure_var_bases_slabs(rf_var_plan *plan) {
    if (plan->bases_slabs) return RF_OK;
    if (hipMalloc((void **)&plan->bases_slabs, plan->bases_slab_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        plan->bases_slabs = nullptr;
        set_error("hipMalloc of %zu bytes for the base gradients' slabs failed", plan->bases_slab_bytes());
        return RF_ERR_NOMEM;
    }
    return RF_OK;
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
            a.lam[pl] = grad || io.slabs ? saved(S, pl) : nullptr;
        }
        a.src_stride = stage_stride(plan, sc.dim, q == S - 1 ? io.grad_out_stride : io.grad_in_stride);
        a.dst_stride = stage_stride(plan, sc.dim, io.grad_in_stride);
        a.lam_stride = stage_stride(plan, sc.dim, saved_stride);
        rc = launch_stage(a, sc.dim, plan->signal, stream, timer);
        if (rc != RF_OK || !with_weights) continue;
        if (grad || io.slabs) {                       // (a weight plane without a gradient: no launch, its slot reports 0 ms)
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
            g.slabs = io.slabs ? io.slabs + plan->bases_slab_offset[q] : nullptr;
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

// One call of the distances or of their adjoint, on an image or on a volume: what the four entry points below hand to the shared
// steps.  Each entry point sequences the refusals in its own documented order (they differ: see the four functions) around
// check_distance_pointers and one of the two runners, which hold the alignment and overlap checks and the launch.
struct DistanceCall {
    bool volume, backward;
    const void *const *guide;
    int32_t n_guide, guide_u8;
    int64_t width, height, depth;      // depth: a volume's, else 1
    float scale, spacing_z;
    const void *planes[3];             // dx, dy(, dz): written by the forward; or their gradients, read by the backward
    void *const *grad_guide;           // the backward's
    int32_t accumulate, device;
    hipStream_t stream;
    int32_t batch;                     // an image's (plan_smooth.cpp); a volume has none
    int64_t guide_stride, grad_guide_stride;
    int n() const { return volume ? 3 : 2; }
    const char *noun() const { return volume ? "volume" : "plane"; }
    size_t bytes() const { return (size_t)(width * height * depth) * sizeof(float); }      // of one f32 plane
    // "dx and dy", "grad_dx, grad_dy or grad_dz", ...
    std::string list(const char *conjunction) const {
        const std::string p(backward ? "grad_" : "");
        return volume ? p + "dx, " + p + "dy " + conjunction + " " + p + "dz" : p + "dx " + conjunction + " " + p + "dy";
    }
};

int check_distance_counts(const DistanceCall &c) {
    if (c.n_guide < 1 || c.n_guide > RF_MAX_PLANES) { set_error("n_guide must be 1..%d (got %d)", RF_MAX_PLANES, c.n_guide); return RF_ERR_INVALID_ARG; }
    if (c.width < 1 || c.height < 1 || c.depth < 1) {
        set_error("%s must be positive", c.volume ? "width, height and depth" : "width and height");
        return RF_ERR_INVALID_ARG;
    }
    return RF_OK;
}

int check_distance_pointers(const DistanceCall &c) {
    bool null = !c.guide || (c.backward && !c.grad_guide);
    for (int k = 0; k < c.n(); k++) null = null || !c.planes[k];
    if (null) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    for (int ch = 0; ch < c.n_guide; ch++) {
        if (c.guide[ch] && (!c.backward || c.grad_guide[ch])) continue;
        if (c.backward) set_error("guide %s %d: null pointer (the %s or its gradient)", c.noun(), ch, c.noun());
        else set_error("guide %s %d: null pointer", c.noun(), ch);
        return RF_ERR_INVALID_ARG;
    }
    return RF_OK;
}

int check_distance_scale(const DistanceCall &c) {
    if (!std::isfinite(c.scale) || c.scale < 0.0f) { set_error("scale must be finite and not negative (got %g)", (double)c.scale); return RF_ERR_INVALID_ARG; }
    return RF_OK;
}

int check_distance_spacing(const DistanceCall &c) {
    if (!std::isfinite(c.spacing_z) || !(c.spacing_z > 0.0f)) { set_error("spacing_z must be finite and positive (got %g)", (double)c.spacing_z); return RF_ERR_INVALID_ARG; }
    return RF_OK;
}

int check_distance_accumulate(const DistanceCall &c) {
    if (c.accumulate != 0 && c.accumulate != 1) { set_error("accumulate must be 0 or 1 (got %d)", c.accumulate); return RF_ERR_INVALID_ARG; }
    return RF_OK;
}

// the accepted domain: a volume's is check_volume_extents with one plane
int check_distance_extents(const DistanceCall &c) {
    if (c.volume) return check_volume_extents(c.width, c.height, c.depth, 1);
    if (c.width % 4 != 0) {
        set_error("%s moves 16 bytes per lane along x: the width must be a multiple of 4 (got %lld)", c.backward ? "var_distances_grad" : "var_distances",
                  (long long)c.width);
        return RF_ERR_UNSUPPORTED;
    }
    if (c.width > kVarMaxExtent || c.height > kVarMaxExtent) {
        set_error("extents %lld x %lld are above %lld", (long long)c.width, (long long)c.height, (long long)kVarMaxExtent);
        return RF_ERR_UNSUPPORTED;
    }
    return RF_OK;
}

int check_distance_planes_aligned(const DistanceCall &c) {
    uintptr_t bits = 0;
    for (int k = 0; k < c.n(); k++) bits |= (uintptr_t)c.planes[k];
    if ((bits & 15u) != 0) { set_error("%s must be 16-byte aligned", c.list("and").c_str()); return RF_ERR_INVALID_ARG; }
    return RF_OK;
}

// The forward behind its entry point's refusals: alignment, overlaps, one launch.
int run_distances_forward(const DistanceCall &c) {
    int rc = check_distance_planes_aligned(c);
    if (rc != RF_OK) return rc;
    const uintptr_t guide_align = c.guide_u8 ? 3u : 15u;
    for (int ch = 0; ch < c.n_guide; ch++)
        if (((uintptr_t)c.guide[ch] & guide_align) != 0) {
            set_error("guide %s %d: %s guide %ss must be %u-byte aligned", c.noun(), ch, c.guide_u8 ? "uint8" : "f32", c.noun(), (unsigned)guide_align + 1);
            return RF_ERR_INVALID_ARG;
        }
    const size_t out_bytes = c.bytes(), guide_bytes = c.guide_u8 ? out_bytes / sizeof(float) : out_bytes;
    for (int k = 0; k < c.n(); k++)
        for (int q = k + 1; q < c.n(); q++)
            if (overlap(c.planes[k], out_bytes * (size_t)c.batch, c.planes[q], out_bytes * (size_t)c.batch)) {
                set_error("%s", c.volume ? "dx, dy and dz overlap each other" : "dx overlaps dy");
                return RF_ERR_INVALID_ARG;
            }
    // (a batch comes from plan_smooth.cpp: the distance planes are the plan's own, which no plane of a caller overlaps)
    for (int ch = 0; ch < c.n_guide && c.batch == 1; ch++)
        for (int k = 0; k < c.n(); k++)
            if (overlap(c.planes[k], out_bytes, c.guide[ch], guide_bytes)) {
                set_error("guide %s %d overlaps %s: a lane reads its neighbours' samples", c.noun(), ch, c.list("or").c_str());
                return RF_ERR_INVALID_ARG;
            }
    if (c.device >= 0) RF_HIP_CHECK(hipSetDevice(c.device));
    if (c.volume) {
        VarDistVolumeArgs a{};
        for (int ch = 0; ch < c.n_guide; ch++) a.guide[ch] = c.guide[ch];
        a.dx = (float *)c.planes[0];
        a.dy = (float *)c.planes[1];
        a.dz = (float *)c.planes[2];
        a.width = (int32_t)c.width;
        a.height = (int32_t)c.height;
        a.depth = (int32_t)c.depth;
        a.n_guide = c.n_guide;
        a.scale = c.scale;
        a.spacing_z = c.spacing_z;
        return launch_var_distances_volume(a, c.guide_u8 != 0, c.stream);
    }
    VarDistArgs a{};
    for (int ch = 0; ch < c.n_guide; ch++) a.guide[ch] = c.guide[ch];
    a.dx = (float *)c.planes[0];
    a.dy = (float *)c.planes[1];
    a.width = (int32_t)c.width;
    a.height = (int32_t)c.height;
    a.n_guide = c.n_guide;
    a.scale = c.scale;
    a.batch = c.batch;
    a.guide_stride = c.guide_stride;
    return launch_var_distances(a, c.guide_u8 != 0, c.stream);
}

// The adjoint behind its entry point's refusals: alignment, overlaps, one launch.
int run_distances_backward(const DistanceCall &c) {
    int rc = check_distance_planes_aligned(c);
    if (rc != RF_OK) return rc;
    for (int ch = 0; ch < c.n_guide; ch++)
        if ((((uintptr_t)c.guide[ch] | (uintptr_t)c.grad_guide[ch]) & 15u) != 0) {
            set_error("guide %s %d: f32 guide %ss and their gradients must be 16-byte aligned", c.noun(), ch, c.noun());
            return RF_ERR_INVALID_ARG;
        }
    // a gradient plane is written while other lanes still read: it overlaps nothing that is read and no other gradient plane
    // (a batch comes from plan_smooth.cpp, which has checked every extent of the caller's against every other, sorted; the distance
    // gradients are then the plan's own planes)
    const size_t bytes = c.bytes();
    for (int ch = 0; ch < c.n_guide && c.batch == 1; ch++) {
        const void *o = c.grad_guide[ch];
        for (int k = 0; k < c.n(); k++)
            if (overlap(o, bytes, c.planes[k], bytes)) {
                set_error("gradient of guide %s %d overlaps %s: a lane reads its neighbours' samples", c.noun(), ch, c.list("or").c_str());
                return RF_ERR_INVALID_ARG;
            }
        for (int q = 0; q < c.n_guide; q++) {
            if (overlap(o, bytes, c.guide[q], bytes)) {
                set_error("gradient of guide %s %d overlaps guide %s %d: a lane reads its neighbours' samples", c.noun(), ch, c.noun(), q);
                return RF_ERR_INVALID_ARG;
            }
            if (q > ch && overlap(o, bytes, c.grad_guide[q], bytes)) {
                set_error("gradient of guide %s %d overlaps gradient of guide %s %d", c.noun(), ch, c.noun(), q);
                return RF_ERR_INVALID_ARG;
            }
        }
    }
    if (c.device >= 0) RF_HIP_CHECK(hipSetDevice(c.device));
    if (c.volume) {
        VarDistVolumeGradArgs a{};
        for (int ch = 0; ch < c.n_guide; ch++) {
            a.guide[ch] = (const float *)c.guide[ch];
            a.grad_guide[ch] = (float *)c.grad_guide[ch];
        }
        a.gdx = (const float *)c.planes[0];
        a.gdy = (const float *)c.planes[1];
        a.gdz = (const float *)c.planes[2];
        a.width = (int32_t)c.width;
        a.height = (int32_t)c.height;
        a.depth = (int32_t)c.depth;
        a.n_guide = c.n_guide;
        a.accumulate = c.accumulate;
        a.scale = c.scale;
        return launch_var_distances_volume_grad(a, c.stream);
    }
    VarDistGradArgs a{};
    for (int ch = 0; ch < c.n_guide; ch++) {
        a.guide[ch] = (const float *)c.guide[ch];
        a.grad_guide[ch] = (float *)c.grad_guide[ch];
    }
    a.gdx = (const float *)c.planes[0];
    a.gdy = (const float *)c.planes[1];
    a.width = (int32_t)c.width;
    a.height = (int32_t)c.height;
    a.n_guide = c.n_guide;
    a.accumulate = c.accumulate;
    a.scale = c.scale;
    a.batch = c.batch;
    a.guide_stride = c.guide_stride;
    a.grad_guide_stride = c.grad_guide_stride;
    return launch_var_distances_grad(a, c.stream);
}

// the first refusal of `steps`, in their order; else what `run` answers
using DistanceStep = int (*)(const DistanceCall &);
int run_distance_steps(const DistanceCall &c, std::initializer_list<DistanceStep> steps, DistanceStep run) {
    for (DistanceStep step : steps)
        if (int rc = step(c); rc != RF_OK) return rc;
    return run(c);
}

}  // namespace

// The four entry points: each its own order of refusals, as recfilter_amd.h documents it.  The image backward decides `accumulate`
// before the extents, the volume backward the volume's domain before `accumulate`; the volume forward has spacing_z between the
// scale and the domain.
int run_var_distances(const void *const *guide_planes, int32_t n_guide, int32_t guide_u8, int64_t width, int64_t height, float scale,
                      void *dx, void *dy, int32_t device, hipStream_t stream, int32_t batch, int64_t guide_stride) {
    const DistanceCall c{false, false, guide_planes, n_guide, guide_u8, width, height, 1, scale, 1.0f, {dx, dy, nullptr}, nullptr, 0, device, stream,
                         batch, guide_stride, 0};
    return run_distance_steps(c, {check_distance_counts, check_distance_pointers, check_distance_scale, check_distance_extents}, run_distances_forward);
}

int run_var_distances_volume(const void *const *guide_volumes, int32_t n_guide, int32_t guide_u8, int64_t width, int64_t height, int64_t depth,
                             float scale, float spacing_z, void *dx, void *dy, void *dz, int32_t device, hipStream_t stream) {
    const DistanceCall c{true, false, guide_volumes, n_guide, guide_u8, width, height, depth, scale, spacing_z, {dx, dy, dz}, nullptr, 0, device, stream,
                         1, 0, 0};
    return run_distance_steps(c, {check_distance_counts, check_distance_pointers, check_distance_scale, check_distance_spacing, check_distance_extents},
                              run_distances_forward);
}

int run_var_distances_backward(const void *const *guide_planes, int32_t n_guide, int64_t width, int64_t height, float scale, const void *grad_dx,
                               const void *grad_dy, void *const *grad_guide_planes, int32_t accumulate, int32_t device, hipStream_t stream,
                               int32_t batch, int64_t guide_stride, int64_t grad_guide_stride) {
    const DistanceCall c{false, true, guide_planes, n_guide, 0, width, height, 1, scale, 1.0f, {grad_dx, grad_dy, nullptr}, grad_guide_planes, accumulate,
                         device, stream, batch, guide_stride, grad_guide_stride};
    return run_distance_steps(c, {check_distance_counts, check_distance_pointers, check_distance_scale, check_distance_accumulate, check_distance_extents},
                              run_distances_backward);
}

int run_var_distances_volume_backward(const void *const *guide_volumes, int32_t n_guide, int64_t width, int64_t height, int64_t depth, float scale,
                                      const void *grad_dx, const void *grad_dy, const void *grad_dz, void *const *grad_guide_volumes,
                                      int32_t accumulate, int32_t device, hipStream_t stream) {
    const DistanceCall c{true, true, guide_volumes, n_guide, 0, width, height, depth, scale, 1.0f, {grad_dx, grad_dy, grad_dz}, grad_guide_volumes,
                         accumulate, device, stream, 1, 0, 0};
    return run_distance_steps(c, {check_distance_counts, check_distance_pointers, check_distance_scale, check_distance_extents, check_distance_accumulate},
                              run_distances_backward);
}

}  // namespace rf
