// plan_var2.cpp -- rf_var2_plan_*: one time-varying second-order all-pole scan
//   y[n] = x[n] - a1~[n] y[n-1] - a2~[n] y[n-2]        (causal; the anticausal scan is this one on the three signals reversed)
// on n_lines dense f32 signals, each with coefficient signals of its own, and its adjoint.  The kernels and the tiling are
// kernels_var2_signal.hip's; this file holds the checks of a description and of a call -- in the order recfilter_amd.h documents,
// nothing of HIP called before the last of them -- and the launch sequences, on the run layer every plan family shares
// (run_support.h: the launch timer, the plane checks, the aliasing rules of a backward call).
//
//   forward    var2_tails_1d, var2_carry_1d, var2_pass2_1d
//   backward   var2_adj_tails_1d, var2_carry_1d, var2_adj_pass2_1d on grad_out, against the forward's direction, with the coefficients
//              read shifted: grad_in = lam.  With coefficient gradients, var2_grad_1d then reads lam from grad_in and y from `out`.
// The adjoint uses the forward's workspace and nothing else: the caller hands back the forward's result.
// The direct-form-I section (run_var2_biquad, run_var2_biquad_backward: the feed-forward taps in front of the scan) stands at the
// end of the file; its backward keeps the adjoint state in one signal the plan allocates in the first such call.  Behind it, the
// cascade of sections (run_var2_cascade, run_var2_cascade_backward): one link launch per boundary between two sections.
#include "plan_var2.h"

#include <memory>

rf_var2_plan::~rf_var2_plan() {
    if (workspace) (void)hipFree(workspace);
    if (lam) (void)hipFree(lam);
    if (cascade) (void)hipFree(cascade);
    if (frames_slab) (void)hipFree(frames_slab);
}

namespace rf {

namespace {

constexpr int64_t kVar2MaxLength = int64_t(1) << 30;      // indices and 4096-sample groups stay inside int32
constexpr int64_t kVar2MaxStride = int64_t(1) << 40;
constexpr int kVar2MaxLines = 65535;                      // the lines ride on gridDim.y

int refuse(int status, const char *fmt, long long a = 0, long long b = 0) {
    set_error(fmt, a, b);
    return status;
}

Var2Args scan_args(const rf_var2_plan *plan, bool causal, bool adjoint) {
    Var2Args a{};
    a.tails = plan->workspace;
    a.carry = plan->workspace + plan->tails_floats();
    a.n = (int32_t)plan->length;
    a.tiles = (int32_t)plan->tiles;
    a.groups = (int32_t)plan->groups;
    a.n_lines = plan->n_lines;
    a.causal = causal ? 1 : 0;
    a.adjoint = adjoint ? 1 : 0;
    a.stride = plan->stride;
    return a;
}

// the three launches of a scan, a mark behind each
int launch_scan(const Var2Args &a, hipStream_t stream, LaunchTimer &timer) {
    int rc = launch_var2_tails(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc == RF_OK) rc = launch_var2_carry(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc == RF_OK) rc = launch_var2_pass2(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    return rc;
}

int refuse_host_only() { set_error("host-only plan (RF_DEVICE_HOST_ONLY) cannot execute"); return RF_ERR_HIP; }

}  // namespace

int build_var2_signal_plan(const rf_var2_signal_desc *d, rf_var2_plan **out) {
    if (!d || !out) return refuse(RF_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (d->abi != RF_ABI) return refuse(RF_ERR_INVALID_ARG, "rf_var2_signal_desc.abi is %lld, this library implements abi %lld", d->abi, RF_ABI);
    if (d->flags != 0) return refuse(RF_ERR_INVALID_ARG, "rf_var2_signal_desc.flags must be 0 (got %lld)", d->flags);
    if (d->length < 1) return refuse(RF_ERR_INVALID_ARG, "length must be positive (got %lld)", d->length);
    if (d->n_lines < 1 || d->n_lines > kVar2MaxLines) return refuse(RF_ERR_INVALID_ARG, "n_lines must be 1..%lld (got %lld)", kVar2MaxLines, d->n_lines);
    if (d->stride < d->length || d->stride % 4 != 0 || d->stride > kVar2MaxStride)
        return refuse(RF_ERR_INVALID_ARG, "stride must be a multiple of 4, at least the length and at most 2^40 (got %lld for a length of %lld)", d->stride, d->length);
    if (d->length % 4 != 0) return refuse(RF_ERR_UNSUPPORTED, "length must be a multiple of 4 (got %lld): pad the signal and the coefficients with zeros", d->length);
    if (d->length > kVar2MaxLength) return refuse(RF_ERR_UNSUPPORTED, "length %lld is above the limit of 2^30 samples", d->length);
    const bool host_only = d->device == RF_DEVICE_HOST_ONLY;
    int device = d->device;
    if (!host_only) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("no HIP device available (this library has no CPU fallback)"); return RF_ERR_HIP; }
        if (device < 0) RF_HIP_CHECK(hipGetDevice(&device));
        if (device >= ndev) { set_error("device %d out of range (%d visible)", device, ndev); return RF_ERR_INVALID_ARG; }
    }
    std::unique_ptr<rf_var2_plan> plan(new rf_var2_plan);
    plan->length = d->length;
    plan->stride = d->stride;
    plan->n_lines = d->n_lines;
    plan->causal = d->causal != 0;
    plan->device = host_only ? 0 : device;
    plan->host_only = host_only;
    plan->tiles = (d->length + kVar2Tile - 1) / kVar2Tile;
    plan->groups = (plan->tiles + kVar2GroupTiles - 1) / kVar2GroupTiles;
    plan->names = {"var2_tails_1d", "var2_carry_1d", "var2_pass2_1d"};
    plan->backward_names[0] = {"var2_adj_tails_1d", "var2_carry_1d", "var2_adj_pass2_1d"};
    plan->backward_names[1] = {"var2_adj_tails_1d", "var2_carry_1d", "var2_adj_pass2_1d", "var2_grad_1d"};
    plan->biquad_names = {"var2_biquad_tails_1d", "var2_carry_1d", "var2_pass2_1d"};
    plan->biquad_backward_names = {"var2_adj_tails_1d", "var2_carry_1d", "var2_adj_pass2_1d", "var2_biquad_grad_1d"};
    plan->frames_names = {"var2_biquad_frames_tails_1d", "var2_carry_1d", "var2_frames_pass2_1d"};
    plan->frames_backward_names[0] = {"var2_adj_frames_tails_1d", "var2_carry_1d", "var2_adj_frames_pass2_1d", "var2_biquad_frames_grad_1d"};
    plan->frames_backward_names[1] = plan->frames_backward_names[0];
    plan->frames_backward_names[1].push_back("var2_frames_fold_1d");
    if (!host_only) {
        RF_HIP_CHECK(hipSetDevice(device));
        if (hipMalloc((void **)&plan->workspace, plan->workspace_bytes()) != hipSuccess) {
            (void)hipGetLastError();
            plan->workspace = nullptr;
            set_error("hipMalloc of %zu bytes of workspace failed", plan->workspace_bytes());
            return RF_ERR_NOMEM;
        }
    }
    *out = plan.release();
    return RF_OK;
}

int run_var2_plan(rf_var2_plan *plan, const void *in, const void *a1, const void *a2, void *out, hipStream_t stream, float *ms_out) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    int rc = check_plane("signal", 0, {{in}, {a1}, {a2}, {out}}, 15u, "null pointer (in, a1, a2, out)", "the var2 scans need 16-byte aligned pointers");
    if (rc != RF_OK) return rc;
    // out against the coefficients, and against in -- which alone it may be, and then exactly
    const size_t bytes = plan->span_bytes();
    const void *const written[1] = {out}, *const coefficients[2] = {a1, a2}, *const input[1] = {in};
    const PlaneList w = {"out", written, 1, bytes};
    const PlaneList r = {"coefficient", coefficients, 2, bytes, ": a coefficient signal is read while outputs are stored"};
    rc = check_written_planes(&w, 1, &r, 1, {"in", input, 1, bytes});
    if (rc != RF_OK) return rc;
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    LaunchTimer timer(stream, ms_out, plan->names.size());
    if (timer.status() != RF_OK) return timer.status();
    Var2Args a = scan_args(plan, plan->causal, false);
    a.x = (const float *)in;
    a.a1 = (const float *)a1;
    a.a2 = (const float *)a2;
    a.dst = (float *)out;
    rc = launch_scan(a, stream, timer);
    return rc == RF_OK ? timer.finish() : rc;
}

int run_var2_backward(rf_var2_plan *plan, const void *a1, const void *a2, const void *out, const void *grad_out, void *grad_in, void *grad_a1,
                      void *grad_a2, hipStream_t stream, float *ms_out) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    if ((grad_a1 == nullptr) != (grad_a2 == nullptr))
        return refuse(RF_ERR_INVALID_ARG, "grad_a1 and grad_a2 are both given or both null (one launch forms the two)");
    const bool with_coefficients = grad_a1 != nullptr;
    int rc = check_plane("signal", 0, {{a1}, {a2}, {grad_out}, {grad_in}, {out, with_coefficients}, {grad_a1, false}, {grad_a2, false}}, 15u,
                         "null pointer (a1, a2, grad_out, grad_in; out where coefficient gradients are asked for)",
                         "the var2 scans need 16-byte aligned pointers");
    if (rc != RF_OK) return rc;
    const size_t bytes = plan->span_bytes();
    const void *const gin[1] = {grad_in}, *const gcoef[2] = {grad_a1, grad_a2}, *const coefficients[2] = {a1, a2}, *const result[1] = {out},
                      *const gout[1] = {grad_out};
    const PlaneList written[2] = {{"grad_in", gin, 1, bytes}, {"gradient of coefficient", gcoef, with_coefficients ? 2 : 0, bytes}};
    const PlaneList read[2] = {{"coefficient", coefficients, 2, bytes, ": a coefficient signal is read while outputs are stored"},
                               {"out", result, with_coefficients ? 1 : 0, bytes}};
    rc = check_written_planes(written, 2, read, 2, {"grad_out", gout, 1, bytes});
    if (rc != RF_OK) return rc;
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    LaunchTimer timer(stream, ms_out, plan->backward_names[with_coefficients ? 1 : 0].size());
    if (timer.status() != RF_OK) return timer.status();
    Var2Args a = scan_args(plan, !plan->causal, true);
    a.x = (const float *)grad_out;
    a.a1 = (const float *)a1;
    a.a2 = (const float *)a2;
    a.dst = (float *)grad_in;
    rc = launch_scan(a, stream, timer);
    if (rc == RF_OK && with_coefficients) {
        Var2GradArgs g{};
        g.lam = (const float *)grad_in;
        g.y = (const float *)out;
        g.grad_a1 = (float *)grad_a1;
        g.grad_a2 = (float *)grad_a2;
        g.n = (int32_t)plan->length;
        g.n_lines = plan->n_lines;
        g.causal = plan->causal ? 1 : 0;
        g.stride = plan->stride;
        rc = launch_var2_grad(g, stream);
        if (rc == RF_OK) rc = timer.mark();
    }
    return rc == RF_OK ? timer.finish() : rc;
}

// ---- the direct-form-I section ------------------------------------------------------------------------------------------------------
//   forward    var2_biquad_tails_1d (stores v = the feed-forward part of `in` to out), then var2_carry_1d and var2_pass2_1d on out, in
//              place.  The first launch stores v while neighbouring groups still read `in`: in == out is refused.
//   backward   the three adjoint launches on grad_out, lam stored to the plan's own signal (allocated here, by the first call), then
//              var2_biquad_grad_1d: grad_in and, where asked for, the five coefficient gradients from lam, in, out and the taps.
int run_var2_biquad(rf_var2_plan *plan, const void *in, const void *b0, const void *b1, const void *b2, const void *a1, const void *a2, void *out,
                    hipStream_t stream, float *ms_out) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    int rc = check_plane("signal", 0, {{in}, {b0}, {b1}, {b2}, {a1}, {a2}, {out}}, 15u, "null pointer (in, b0, b1, b2, a1, a2, out)",
                         "the var2 scans need 16-byte aligned pointers");
    if (rc != RF_OK) return rc;
    const size_t bytes = plan->span_bytes();
    const void *const written[1] = {out}, *const coefficients[5] = {b0, b1, b2, a1, a2}, *const input[1] = {in};
    const PlaneList w = {"out", written, 1, bytes};
    const PlaneList r[2] = {{"coefficient", coefficients, 5, bytes, ": a coefficient signal is read while outputs are stored"},
                            {"in", input, 1, bytes,
                             ": in == out is not allowed for a biquad (the first launch stores the feed-forward part while neighbouring groups still read in)"}};
    rc = check_written_planes(&w, 1, r, 2, {"grad_out", nullptr, 0, bytes});
    if (rc != RF_OK) return rc;
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    LaunchTimer timer(stream, ms_out, plan->biquad_names.size());
    if (timer.status() != RF_OK) return timer.status();
    Var2Args a = scan_args(plan, plan->causal, false);
    a.x = (const float *)in;
    a.b0 = (const float *)b0;
    a.b1 = (const float *)b1;
    a.b2 = (const float *)b2;
    a.a1 = (const float *)a1;
    a.a2 = (const float *)a2;
    a.dst = (float *)out;
    rc = launch_var2_biquad_tails(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    a.x = (const float *)out;      // v; the scan finishes on it in place
    if (rc == RF_OK) rc = launch_var2_carry(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc == RF_OK) rc = launch_var2_pass2(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    return rc == RF_OK ? timer.finish() : rc;
}

int run_var2_biquad_backward(rf_var2_plan *plan, const void *in, const void *b0, const void *b1, const void *b2, const void *a1, const void *a2,
                             const void *out, const void *grad_out, void *grad_in, void *grad_b0, void *grad_b1, void *grad_b2, void *grad_a1,
                             void *grad_a2, hipStream_t stream, float *ms_out) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    const int given = (grad_b0 != nullptr) + (grad_b1 != nullptr) + (grad_b2 != nullptr) + (grad_a1 != nullptr) + (grad_a2 != nullptr);
    if (given != 0 && given != 5)
        return refuse(RF_ERR_INVALID_ARG, "grad_b0, grad_b1, grad_b2, grad_a1 and grad_a2 are all given or all null (one launch forms the five; %lld given)", given);
    const bool with_coefficients = given == 5;
    int rc = check_plane("signal", 0, {{in}, {b0}, {b1}, {b2}, {a1}, {a2}, {grad_out}, {grad_in}, {out, with_coefficients}, {grad_b0, false},
                                      {grad_b1, false}, {grad_b2, false}, {grad_a1, false}, {grad_a2, false}}, 15u,
                         "null pointer (in, b0, b1, b2, a1, a2, grad_out, grad_in; out where coefficient gradients are asked for)",
                         "the var2 scans need 16-byte aligned pointers");
    if (rc != RF_OK) return rc;
    const size_t bytes = plan->span_bytes();
    const void *const gin[1] = {grad_in}, *const gcoef[5] = {grad_b0, grad_b1, grad_b2, grad_a1, grad_a2},
                      *const coefficients[5] = {b0, b1, b2, a1, a2}, *const input[1] = {in}, *const result[1] = {out}, *const gout[1] = {grad_out};
    const PlaneList written[2] = {{"grad_in", gin, 1, bytes}, {"gradient of coefficient", gcoef, with_coefficients ? 5 : 0, bytes}};
    const PlaneList read[3] = {{"coefficient", coefficients, 5, bytes, ": a coefficient signal is read while outputs are stored"},
                               {"in", input, 1, bytes},
                               {"out", result, with_coefficients ? 1 : 0, bytes}};
    rc = check_written_planes(written, 2, read, 3, {"grad_out", gout, 1, bytes});
    if (rc != RF_OK) return rc;
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    if (!plan->lam && hipMalloc((void **)&plan->lam, bytes) != hipSuccess) {
        (void)hipGetLastError();
        plan->lam = nullptr;
        set_error("hipMalloc of %zu bytes for the adjoint state of the biquad's backward failed", bytes);
        return RF_ERR_NOMEM;
    }
    LaunchTimer timer(stream, ms_out, plan->biquad_backward_names.size());
    if (timer.status() != RF_OK) return timer.status();
    Var2Args a = scan_args(plan, !plan->causal, true);
    a.x = (const float *)grad_out;
    a.a1 = (const float *)a1;
    a.a2 = (const float *)a2;
    a.dst = plan->lam;
    rc = launch_scan(a, stream, timer);
    if (rc == RF_OK) {
        Var2BiquadGradArgs g{};
        g.lam = plan->lam;
        g.x = (const float *)in;
        g.y = (const float *)out;
        g.b0 = (const float *)b0;
        g.b1 = (const float *)b1;
        g.b2 = (const float *)b2;
        g.grad_in = (float *)grad_in;
        g.grad_b0 = (float *)grad_b0;
        g.grad_b1 = (float *)grad_b1;
        g.grad_b2 = (float *)grad_b2;
        g.grad_a1 = (float *)grad_a1;
        g.grad_a2 = (float *)grad_a2;
        g.n = (int32_t)plan->length;
        g.n_lines = plan->n_lines;
        g.causal = plan->causal ? 1 : 0;
        g.with_coefficients = with_coefficients ? 1 : 0;
        g.stride = plan->stride;
        rc = launch_var2_biquad_grad(g, stream);
        if (rc == RF_OK) rc = timer.mark();
    }
    return rc == RF_OK ? timer.finish() : rc;
}

// ---- a cascade of direct-form-I sections -------------------------------------------------------------------------------------------
//   forward    var2_biquad_tails_1d (v_0 to out), then per boundary var2_carry_1d and var2_link_1d (the final stage of section k,
//              the feed-forward part and the tails of section k + 1, v_{k+1} to out in place), then var2_carry_1d, var2_pass2_1d.
//   backward   keeps nothing from the forward.  K >= 2: sections 0 .. K-2 are rerun into the plan's signals I_0 .. I_{K-2} (the
//              link's KEEP instance stores y_k over v_k in I_k and v_{k+1} to I_{k+1}); then, from the last section to the first,
//              the three adjoint launches on g_k into lam and var2_biquad_grad_1d with x = y_{k-1}, y = y_k, the gradient
//              between two sections in one more signal of the plan's (the grad launch reads lam, never g_k: one buffer serves).
namespace {

constexpr const char *kSectionCount = "n_sections must be 1..%lld (got %lld)";

Var2LinkArgs link_args(const rf_var2_plan *plan, const float *x, const rf_var2_section &done, const rf_var2_section &next, float *dst, float *keep) {
    Var2LinkArgs l{};
    l.x = x;
    l.a1 = (const float *)done.a1;
    l.a2 = (const float *)done.a2;
    l.next_b0 = (const float *)next.b0;
    l.next_b1 = (const float *)next.b1;
    l.next_b2 = (const float *)next.b2;
    l.next_a1 = (const float *)next.a1;
    l.next_a2 = (const float *)next.a2;
    l.dst = dst;
    l.keep = keep;
    l.tails = plan->workspace;
    l.carry = plan->workspace + plan->tails_floats();
    l.n = (int32_t)plan->length;
    l.tiles = (int32_t)plan->tiles;
    l.groups = (int32_t)plan->groups;
    l.n_lines = plan->n_lines;
    l.causal = plan->causal ? 1 : 0;
    l.stride = plan->stride;
    return l;
}

// Sections 0 .. count-1 on `in`.  signals == nullptr: every v and the result in `out`, in place.  Else section k's v, then its
// result, in signals[k] (count of them).
int launch_sections(const rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int count, float *out, float *const *signals,
                    hipStream_t stream, LaunchTimer &timer) {
    Var2Args a = scan_args(plan, plan->causal, false);
    a.x = (const float *)in;
    a.b0 = (const float *)sections[0].b0;
    a.b1 = (const float *)sections[0].b1;
    a.b2 = (const float *)sections[0].b2;
    a.a1 = (const float *)sections[0].a1;
    a.a2 = (const float *)sections[0].a2;
    a.dst = signals ? signals[0] : out;
    int rc = launch_var2_biquad_tails(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    for (int k = 1; k < count && rc == RF_OK; k++) {
        rc = launch_var2_carry(a, stream);
        if (rc == RF_OK) rc = timer.mark();
        float *from = signals ? signals[k - 1] : out, *to = signals ? signals[k] : out;
        if (rc == RF_OK) rc = launch_var2_link(link_args(plan, from, sections[k - 1], sections[k], to, signals ? from : nullptr), stream);
        if (rc == RF_OK) rc = timer.mark();
    }
    a.x = a.dst = signals ? signals[count - 1] : out;
    a.a1 = (const float *)sections[count - 1].a1;
    a.a2 = (const float *)sections[count - 1].a2;
    if (rc == RF_OK) rc = launch_var2_carry(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc == RF_OK) rc = launch_var2_pass2(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    return rc;
}

int check_sections(const rf_var2_section *sections, int n_sections) {
    for (int k = 0; k < n_sections; k++) {
        const rf_var2_section &s = sections[k];
        int rc = check_plane("section", k, {{s.b0}, {s.b1}, {s.b2}, {s.a1}, {s.a2}}, 15u, "null pointer (b0, b1, b2, a1, a2)",
                             "the var2 scans need 16-byte aligned pointers");
        if (rc != RF_OK) return rc;
    }
    return RF_OK;
}

// the coefficient signals of every section as lists of read planes: "coefficient of section k plane j"
struct SectionLists {
    std::vector<std::string> nouns;
    std::vector<const void *> planes;
    SectionLists(const char *what, int n) {
        nouns.reserve(n);
        planes.reserve((size_t)5 * n);
        for (int k = 0; k < n; k++) nouns.push_back(std::string(what) + " of section " + std::to_string(k));
    }
    PlaneList list(int k, int count, size_t bytes, const char *why = "") const { return {nouns[k].c_str(), planes.data() + 5 * k, count, bytes, why}; }
};

}  // namespace

const char *var2_cascade_name(int n_sections, size_t i) {
    if (i == 0) return "var2_biquad_tails_1d";
    if (i + 1 == (size_t)var2_cascade_launches(n_sections)) return "var2_pass2_1d";
    return i % 2 == 1 ? "var2_carry_1d" : "var2_link_1d";
}

const char *var2_cascade_backward_name(int n_sections, size_t i) {
    static const char *const section[4] = {"var2_adj_tails_1d", "var2_carry_1d", "var2_adj_pass2_1d", "var2_biquad_grad_1d"};
    const size_t rerun = n_sections == 1 ? 0 : (size_t)var2_cascade_launches(n_sections - 1);
    if (i >= rerun) return section[(i - rerun) % 4];
    if (i == 0) return "var2_biquad_tails_1d";
    if (i + 1 == rerun) return "var2_pass2_1d";
    return i % 2 == 1 ? "var2_carry_1d" : "var2_link_keep_1d";
}

int run_var2_cascade(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections, void *out, hipStream_t stream,
                     float *ms_out, const char **names_out, int capacity, bool timed) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    if (n_sections < 1 || n_sections > RF_VAR2_MAX_SECTIONS) return refuse(RF_ERR_INVALID_ARG, kSectionCount, RF_VAR2_MAX_SECTIONS, n_sections);
    const size_t launches = (size_t)var2_cascade_launches(n_sections);
    if (timed) {
        int rc = timed_names(launches, [&](size_t i) { return var2_cascade_name(n_sections, i); }, ms_out, names_out, capacity);
        if (rc != RF_OK) return rc;
    }
    if (!sections) return refuse(RF_ERR_INVALID_ARG, "null sections");
    int rc = check_plane("signal", 0, {{in}, {out}}, 15u, "null pointer (in, out)", "the var2 scans need 16-byte aligned pointers");
    if (rc == RF_OK) rc = check_sections(sections, n_sections);
    if (rc != RF_OK) return rc;
    const size_t bytes = plan->span_bytes();
    SectionLists coefficients("coefficient", n_sections);
    for (int k = 0; k < n_sections; k++)
        coefficients.planes.insert(coefficients.planes.end(), {sections[k].b0, sections[k].b1, sections[k].b2, sections[k].a1, sections[k].a2});
    std::vector<PlaneList> read;
    for (int k = 0; k < n_sections; k++) read.push_back(coefficients.list(k, 5, bytes, ": a coefficient signal is read while outputs are stored"));
    const void *const written[1] = {out}, *const input[1] = {in};
    read.push_back({"in", input, 1, bytes,
                    ": in == out is not allowed for a biquad (the first launch stores the feed-forward part while neighbouring groups still read in)"});
    const PlaneList w = {"out", written, 1, bytes};
    rc = check_written_planes(&w, 1, read.data(), (int)read.size(), {"grad_out", nullptr, 0, bytes});
    if (rc != RF_OK) return rc;
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    LaunchTimer timer(stream, ms_out, launches);
    if (timer.status() != RF_OK) return timer.status();
    rc = launch_sections(plan, in, sections, n_sections, (float *)out, nullptr, stream, timer);
    return rc == RF_OK ? timer.finish() : rc;
}

int run_var2_cascade_backward(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections, const void *out,
                              const void *grad_out, void *grad_in, const rf_var2_section_grad *grads, hipStream_t stream, float *ms_out,
                              const char **names_out, int capacity, bool timed) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    if (n_sections < 1 || n_sections > RF_VAR2_MAX_SECTIONS) return refuse(RF_ERR_INVALID_ARG, kSectionCount, RF_VAR2_MAX_SECTIONS, n_sections);
    const int K = n_sections;
    const size_t launches = (size_t)var2_cascade_backward_launches(K);
    if (timed) {
        int rc = timed_names(launches, [&](size_t i) { return var2_cascade_backward_name(K, i); }, ms_out, names_out, capacity);
        if (rc != RF_OK) return rc;
    }
    if (!sections) return refuse(RF_ERR_INVALID_ARG, "null sections");
    const bool with_coefficients = grads != nullptr;
    for (int k = 0; with_coefficients && k < K; k++) {
        const rf_var2_section_grad &g = grads[k];
        const int given = (g.b0 != nullptr) + (g.b1 != nullptr) + (g.b2 != nullptr) + (g.a1 != nullptr) + (g.a2 != nullptr);
        if (given != 5)
            return refuse(RF_ERR_INVALID_ARG, "section %lld: the five coefficient gradients are all given, or grads is null (%lld given)", k, given);
    }
    int rc = check_plane("signal", 0, {{in}, {grad_out}, {grad_in}, {out, with_coefficients}}, 15u,
                         "null pointer (in, grad_out, grad_in; out where coefficient gradients are asked for)",
                         "the var2 scans need 16-byte aligned pointers");
    if (rc == RF_OK) rc = check_sections(sections, K);
    for (int k = 0; rc == RF_OK && with_coefficients && k < K; k++)
        rc = check_plane("section", k, {{grads[k].b0}, {grads[k].b1}, {grads[k].b2}, {grads[k].a1}, {grads[k].a2}}, 15u,
                         "null gradient pointer", "the var2 scans need 16-byte aligned pointers (a coefficient gradient)");
    if (rc != RF_OK) return rc;
    const size_t bytes = plan->span_bytes();
    SectionLists coefficients("coefficient", K), gradients("gradient", K);
    for (int k = 0; k < K; k++) {
        coefficients.planes.insert(coefficients.planes.end(), {sections[k].b0, sections[k].b1, sections[k].b2, sections[k].a1, sections[k].a2});
        if (with_coefficients) gradients.planes.insert(gradients.planes.end(), {grads[k].b0, grads[k].b1, grads[k].b2, grads[k].a1, grads[k].a2});
    }
    const void *const gin[1] = {grad_in}, *const input[1] = {in}, *const result[1] = {out}, *const gout[1] = {grad_out};
    std::vector<PlaneList> written, read;
    written.push_back({"grad_in", gin, 1, bytes});
    for (int k = 0; with_coefficients && k < K; k++) written.push_back(gradients.list(k, 5, bytes));
    for (int k = 0; k < K; k++) read.push_back(coefficients.list(k, 5, bytes, ": a coefficient signal is read while outputs are stored"));
    read.push_back({"in", input, 1, bytes});
    read.push_back({"out", result, with_coefficients ? 1 : 0, bytes});
    rc = check_written_planes(written.data(), (int)written.size(), read.data(), (int)read.size(), {"grad_out", gout, 1, bytes});
    if (rc != RF_OK) return rc;
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    if (!plan->lam && hipMalloc((void **)&plan->lam, bytes) != hipSuccess) {
        (void)hipGetLastError();
        plan->lam = nullptr;
        set_error("hipMalloc of %zu bytes for the adjoint state of the cascade's backward failed", bytes);
        return RF_ERR_NOMEM;
    }
    if (K >= 2 && plan->cascade_spans < K) {
        // (hipFree waits for the device: no earlier call on this plan still uses the signals)
        if (plan->cascade) (void)hipFree(plan->cascade);
        plan->cascade = nullptr;
        plan->cascade_spans = 0;
        if (hipMalloc((void **)&plan->cascade, bytes * (size_t)K) != hipSuccess) {
            (void)hipGetLastError();
            plan->cascade = nullptr;
            set_error("hipMalloc of %zu bytes for the signals of the cascade's backward failed", bytes * (size_t)K);
            return RF_ERR_NOMEM;
        }
        plan->cascade_spans = K;
    }
    LaunchTimer timer(stream, ms_out, launches);
    if (timer.status() != RF_OK) return timer.status();
    const size_t span_floats = bytes / sizeof(float);
    float *between = plan->cascade;                   // g_{k-1}, K >= 2
    float *results[RF_VAR2_MAX_SECTIONS] = {};        // y_0 .. y_{K-2}
    for (int k = 0; k + 1 < K; k++) results[k] = plan->cascade + (size_t)(k + 1) * span_floats;
    if (K >= 2) rc = launch_sections(plan, in, sections, K - 1, nullptr, results, stream, timer);
    for (int k = K - 1; k >= 0 && rc == RF_OK; k--) {
        Var2Args a = scan_args(plan, !plan->causal, true);
        a.x = k == K - 1 ? (const float *)grad_out : between;
        a.a1 = (const float *)sections[k].a1;
        a.a2 = (const float *)sections[k].a2;
        a.dst = plan->lam;
        rc = launch_scan(a, stream, timer);
        if (rc != RF_OK) break;
        Var2BiquadGradArgs g{};
        g.lam = plan->lam;
        g.x = k == 0 ? (const float *)in : results[k - 1];
        g.y = k == K - 1 ? (const float *)out : results[k];
        g.b0 = (const float *)sections[k].b0;
        g.b1 = (const float *)sections[k].b1;
        g.b2 = (const float *)sections[k].b2;
        g.grad_in = k == 0 ? (float *)grad_in : between;
        if (with_coefficients) {
            g.grad_b0 = (float *)grads[k].b0;
            g.grad_b1 = (float *)grads[k].b1;
            g.grad_b2 = (float *)grads[k].b2;
            g.grad_a1 = (float *)grads[k].a1;
            g.grad_a2 = (float *)grads[k].a2;
        }
        g.n = (int32_t)plan->length;
        g.n_lines = plan->n_lines;
        g.causal = plan->causal ? 1 : 0;
        g.with_coefficients = with_coefficients ? 1 : 0;
        g.stride = plan->stride;
        rc = launch_var2_biquad_grad(g, stream);
        if (rc == RF_OK) rc = timer.mark();
    }
    return rc == RF_OK ? timer.finish() : rc;
}

// ---- the cascade that keeps every section's result ---------------------------------------------------------------------------------
//   forward    run_var2_cascade's launches with the link's KEEP instance: section k's v, then its result, in kept[k] (the caller's;
//              K - 1 of them), the last section's in out.  The values of out are run_var2_cascade's.
//   backward   no rerun.  var2_adj_tails_1d on grad_out with the last section's coefficients; then, per boundary from the last one
//              down, var2_carry_1d and var2_adj_link_1d -- the final stage of section k's adjoint scan, the gradient that enters
//              section k - 1 formed on lam_k in registers and stored to the plan's signal G (plan->cascade, its first span), in
//              place from the second boundary on, and the adjoint tails of section k - 1 -- with, where coefficient gradients are
//              asked for, lam_k stored to the plan's lam (var2_adj_link_keep_1d) and var2_biquad_coef_1d on it; then
//              var2_carry_1d, var2_adj_pass2_1d into lam and var2_biquad_grad_1d for section 0.
const char *var2_cascade_keep_name(int n_sections, size_t i) {
    if (i == 0) return "var2_biquad_tails_1d";
    if (i + 1 == (size_t)var2_cascade_launches(n_sections)) return "var2_pass2_1d";
    return i % 2 == 1 ? "var2_carry_1d" : "var2_link_keep_1d";
}

const char *var2_cascade_kept_backward_name(int n_sections, bool with_coefficients, size_t i) {
    static const char *const last[3] = {"var2_carry_1d", "var2_adj_pass2_1d", "var2_biquad_grad_1d"};
    const size_t launches = (size_t)var2_cascade_kept_backward_launches(n_sections, with_coefficients);
    if (i == 0) return "var2_adj_tails_1d";
    if (i + 3 >= launches) return last[i + 3 - launches];
    const size_t at = (i - 1) % (with_coefficients ? 3 : 2);      // within the launches of one boundary
    return at == 0 ? "var2_carry_1d" : at == 2 ? "var2_biquad_coef_1d" : with_coefficients ? "var2_adj_link_keep_1d" : "var2_adj_link_1d";
}

namespace {

// the kept signals of a call, one "kept k" check each: required or, where not, aligned if given
int check_kept(const void *const *kept, int count, bool required) {
    for (int k = 0; k < count; k++) {
        int rc = check_plane("kept", k, {{kept ? kept[k] : nullptr, required}}, 15u, "null pointer (a kept signal)",
                             "the var2 scans need 16-byte aligned pointers");
        if (rc != RF_OK) return rc;
    }
    return RF_OK;
}

Var2BiquadGradArgs grad_args(const rf_var2_plan *plan, const rf_var2_section &s, const rf_var2_section_grad *g, const float *x, const float *y,
                             float *grad_in) {
    Var2BiquadGradArgs a{};
    a.lam = plan->lam;
    a.x = x;
    a.y = y;
    a.b0 = (const float *)s.b0;
    a.b1 = (const float *)s.b1;
    a.b2 = (const float *)s.b2;
    a.grad_in = grad_in;
    if (g) {
        a.grad_b0 = (float *)g->b0;
        a.grad_b1 = (float *)g->b1;
        a.grad_b2 = (float *)g->b2;
        a.grad_a1 = (float *)g->a1;
        a.grad_a2 = (float *)g->a2;
    }
    a.n = (int32_t)plan->length;
    a.n_lines = plan->n_lines;
    a.causal = plan->causal ? 1 : 0;
    a.with_coefficients = g ? 1 : 0;
    a.stride = plan->stride;
    return a;
}

}  // namespace

int run_var2_cascade_keep(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections, void *out, void *const *kept,
                          hipStream_t stream, float *ms_out, const char **names_out, int capacity, bool timed) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    if (n_sections < 1 || n_sections > RF_VAR2_MAX_SECTIONS) return refuse(RF_ERR_INVALID_ARG, kSectionCount, RF_VAR2_MAX_SECTIONS, n_sections);
    const int K = n_sections;
    const size_t launches = (size_t)var2_cascade_launches(K);
    if (timed) {
        int rc = timed_names(launches, [&](size_t i) { return var2_cascade_keep_name(K, i); }, ms_out, names_out, capacity);
        if (rc != RF_OK) return rc;
    }
    if (!sections) return refuse(RF_ERR_INVALID_ARG, "null sections");
    int rc = check_plane("signal", 0, {{in}, {out}}, 15u, "null pointer (in, out)", "the var2 scans need 16-byte aligned pointers");
    if (rc == RF_OK) rc = check_kept(kept, K - 1, true);
    if (rc == RF_OK) rc = check_sections(sections, K);
    if (rc != RF_OK) return rc;
    const size_t bytes = plan->span_bytes();
    SectionLists coefficients("coefficient", K);
    for (int k = 0; k < K; k++)
        coefficients.planes.insert(coefficients.planes.end(), {sections[k].b0, sections[k].b1, sections[k].b2, sections[k].a1, sections[k].a2});
    std::vector<PlaneList> read;
    for (int k = 0; k < K; k++) read.push_back(coefficients.list(k, 5, bytes, ": a coefficient signal is read while outputs are stored"));
    const void *const result[1] = {out}, *const input[1] = {in};
    read.push_back({"in", input, 1, bytes,
                    ": in == out is not allowed for a biquad (the first launch stores the feed-forward part while neighbouring groups still read in)"});
    const PlaneList written[2] = {{"out", result, 1, bytes}, {"kept", (const void *const *)kept, K - 1, bytes}};
    rc = check_written_planes(written, 1, read.data(), (int)read.size(), {"grad_out", nullptr, 0, bytes});      // out, as run_var2_cascade refuses it
    if (rc != RF_OK) return rc;
    read.back().why = ": a kept signal is stored while neighbouring groups still read in";
    rc = check_written_planes(written, 2, read.data(), (int)read.size(), {"grad_out", nullptr, 0, bytes});      // then the kept signals
    if (rc != RF_OK) return rc;
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    LaunchTimer timer(stream, ms_out, launches);
    if (timer.status() != RF_OK) return timer.status();
    float *signals[RF_VAR2_MAX_SECTIONS] = {};
    for (int k = 0; k + 1 < K; k++) signals[k] = (float *)kept[k];
    signals[K - 1] = (float *)out;
    rc = launch_sections(plan, in, sections, K, nullptr, signals, stream, timer);
    return rc == RF_OK ? timer.finish() : rc;
}

int run_var2_cascade_kept_backward(rf_var2_plan *plan, const void *in, const rf_var2_section *sections, int n_sections, const void *const *kept,
                                   const void *out, const void *grad_out, void *grad_in, const rf_var2_section_grad *grads, hipStream_t stream,
                                   float *ms_out, const char **names_out, int capacity, bool timed) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    if (n_sections < 1 || n_sections > RF_VAR2_MAX_SECTIONS) return refuse(RF_ERR_INVALID_ARG, kSectionCount, RF_VAR2_MAX_SECTIONS, n_sections);
    const int K = n_sections;
    const bool with_coefficients = grads != nullptr;
    const size_t launches = (size_t)var2_cascade_kept_backward_launches(K, with_coefficients);
    if (timed) {
        int rc = timed_names(launches, [&](size_t i) { return var2_cascade_kept_backward_name(K, with_coefficients, i); }, ms_out, names_out, capacity);
        if (rc != RF_OK) return rc;
    }
    if (!sections) return refuse(RF_ERR_INVALID_ARG, "null sections");
    for (int k = 0; with_coefficients && k < K; k++) {
        const rf_var2_section_grad &g = grads[k];
        const int given = (g.b0 != nullptr) + (g.b1 != nullptr) + (g.b2 != nullptr) + (g.a1 != nullptr) + (g.a2 != nullptr);
        if (given != 5)
            return refuse(RF_ERR_INVALID_ARG, "section %lld: the five coefficient gradients are all given, or grads is null (%lld given)", k, given);
    }
    // without coefficient gradients nothing of the forward is read: in, out and kept may be null
    int rc = check_plane("signal", 0, {{in, with_coefficients}, {grad_out}, {grad_in}, {out, with_coefficients}}, 15u,
                         "null pointer (grad_out, grad_in; in and out where coefficient gradients are asked for)",
                         "the var2 scans need 16-byte aligned pointers");
    if (rc == RF_OK) rc = check_kept(kept, K - 1, with_coefficients);
    if (rc == RF_OK) rc = check_sections(sections, K);
    for (int k = 0; rc == RF_OK && with_coefficients && k < K; k++)
        rc = check_plane("section", k, {{grads[k].b0}, {grads[k].b1}, {grads[k].b2}, {grads[k].a1}, {grads[k].a2}}, 15u,
                         "null gradient pointer", "the var2 scans need 16-byte aligned pointers (a coefficient gradient)");
    if (rc != RF_OK) return rc;
    const size_t bytes = plan->span_bytes();
    SectionLists coefficients("coefficient", K), gradients("gradient", K);
    for (int k = 0; k < K; k++) {
        coefficients.planes.insert(coefficients.planes.end(), {sections[k].b0, sections[k].b1, sections[k].b2, sections[k].a1, sections[k].a2});
        if (with_coefficients) gradients.planes.insert(gradients.planes.end(), {grads[k].b0, grads[k].b1, grads[k].b2, grads[k].a1, grads[k].a2});
    }
    const void *const gin[1] = {grad_in}, *const input[1] = {in}, *const result[1] = {out}, *const gout[1] = {grad_out};
    std::vector<PlaneList> written, read;
    written.push_back({"grad_in", gin, 1, bytes});
    for (int k = 0; with_coefficients && k < K; k++) written.push_back(gradients.list(k, 5, bytes));
    for (int k = 0; k < K; k++) read.push_back(coefficients.list(k, 5, bytes, ": a coefficient signal is read while outputs are stored"));
    read.push_back({"in", input, with_coefficients ? 1 : 0, bytes});
    read.push_back({"out", result, with_coefficients ? 1 : 0, bytes});
    read.push_back({"kept", kept, with_coefficients ? K - 1 : 0, bytes});
    rc = check_written_planes(written.data(), (int)written.size(), read.data(), (int)read.size(), {"grad_out", gout, 1, bytes});
    if (rc != RF_OK) return rc;
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    if (!plan->lam && hipMalloc((void **)&plan->lam, bytes) != hipSuccess) {
        (void)hipGetLastError();
        plan->lam = nullptr;
        set_error("hipMalloc of %zu bytes for the adjoint state of the cascade's backward failed", bytes);
        return RF_ERR_NOMEM;
    }
    if (K >= 2 && plan->cascade_spans < 1) {
        if (hipMalloc((void **)&plan->cascade, bytes) != hipSuccess) {
            (void)hipGetLastError();
            plan->cascade = nullptr;
            set_error("hipMalloc of %zu bytes for the gradient between the sections of the cascade's backward failed", bytes);
            return RF_ERR_NOMEM;
        }
        plan->cascade_spans = 1;
    }
    LaunchTimer timer(stream, ms_out, launches);
    if (timer.status() != RF_OK) return timer.status();
    float *between = plan->cascade;                   // G: g_{k-1}, K >= 2
    Var2Args a = scan_args(plan, !plan->causal, true);
    a.x = (const float *)grad_out;
    a.a1 = (const float *)sections[K - 1].a1;
    a.a2 = (const float *)sections[K - 1].a2;
    a.dst = plan->lam;
    rc = launch_var2_tails(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    for (int k = K - 1; k >= 1 && rc == RF_OK; k--) {
        rc = launch_var2_carry(a, stream);
        if (rc == RF_OK) rc = timer.mark();
        Var2AdjLinkArgs l{};
        l.x = k == K - 1 ? (const float *)grad_out : between;
        l.a1 = (const float *)sections[k].a1;
        l.a2 = (const float *)sections[k].a2;
        l.b0 = (const float *)sections[k].b0;
        l.b1 = (const float *)sections[k].b1;
        l.b2 = (const float *)sections[k].b2;
        l.prev_a1 = (const float *)sections[k - 1].a1;
        l.prev_a2 = (const float *)sections[k - 1].a2;
        l.dst = between;
        l.keep = with_coefficients ? plan->lam : nullptr;
        l.tails = a.tails;
        l.carry = a.carry;
        l.n = a.n;
        l.tiles = a.tiles;
        l.groups = a.groups;
        l.n_lines = a.n_lines;
        l.causal = a.causal;
        l.stride = a.stride;
        if (rc == RF_OK) rc = launch_var2_adj_link(l, stream);
        if (rc == RF_OK) rc = timer.mark();
        if (rc == RF_OK && with_coefficients) {
            rc = launch_var2_biquad_coef(grad_args(plan, sections[k], &grads[k], (const float *)kept[k - 1],
                                                   k == K - 1 ? (const float *)out : (const float *)kept[k], nullptr), stream);
            if (rc == RF_OK) rc = timer.mark();
        }
    }
    a.x = K == 1 ? (const float *)grad_out : between;
    a.a1 = (const float *)sections[0].a1;
    a.a2 = (const float *)sections[0].a2;
    if (rc == RF_OK) rc = launch_var2_carry(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc == RF_OK) rc = launch_var2_pass2(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc == RF_OK) {
        const float *y = !with_coefficients ? nullptr : K == 1 ? (const float *)out : (const float *)kept[0];
        rc = launch_var2_biquad_grad(grad_args(plan, sections[0], with_coefficients ? &grads[0] : nullptr, (const float *)in, y, (float *)grad_in), stream);
        if (rc == RF_OK) rc = timer.mark();
    }
    return rc == RF_OK ? timer.finish() : rc;
}

// ---- the section on control-rate frames -------------------------------------------------------------------------------------------
//   forward    var2_biquad_frames_tails_1d (reads in and the frames, stores v to out), var2_carry_1d, var2_frames_pass2_1d on out.
//   backward   var2_adj_frames_tails_1d, var2_carry_1d, var2_adj_frames_pass2_1d on grad_out into the plan's lam, then
//              var2_biquad_frames_grad_1d: grad_in and, where frame gradients are asked for, the f64 sums of every piece into the
//              plan's slab, which var2_frames_fold_1d folds into the five [line][frame] gradients.
// The checks common to the calls come first, in the header's order: the hop, the frame count, the frame stride.
namespace {

int hop_shift_of(int hop) {
    int shift = 0;
    while ((1 << shift) < hop) shift++;
    return shift;
}

int check_frames_layout(int64_t length, int hop, int n_frames, int64_t frame_stride) {
    if (!var2_hop_ok(hop)) return refuse(RF_ERR_UNSUPPORTED, "hop must be a power of two in 64..65536 (got %lld)", hop);
    if (n_frames != var2_frames_count(length, hop))
        return refuse(RF_ERR_INVALID_ARG, "n_frames must be ceil(length / hop) + 1 = %lld (got %lld)", var2_frames_count(length, hop), n_frames);
    if (frame_stride < n_frames) return refuse(RF_ERR_INVALID_ARG, "frame_stride must be at least n_frames = %lld (got %lld)", n_frames, frame_stride);
    return RF_OK;
}

constexpr const char *kFrameAlign = "signals need 16-byte aligned pointers, frame arrays 4-byte aligned ones";

Var2FramesArgs frames_args(const rf_var2_plan *plan, const rf_var2_section &f, int hop, int n_frames, int64_t frame_stride, bool causal, bool adjoint) {
    Var2FramesArgs a{};
    a.b0 = (const float *)f.b0;
    a.b1 = (const float *)f.b1;
    a.b2 = (const float *)f.b2;
    a.a1 = (const float *)f.a1;
    a.a2 = (const float *)f.a2;
    a.tails = plan->workspace;
    a.carry = plan->workspace + plan->tails_floats();
    a.n = (int32_t)plan->length;
    a.tiles = (int32_t)plan->tiles;
    a.groups = (int32_t)plan->groups;
    a.n_lines = plan->n_lines;
    a.causal = causal ? 1 : 0;
    a.adjoint = adjoint ? 1 : 0;
    a.hop_shift = hop_shift_of(hop);
    a.n_frames = n_frames;
    a.inv_hop = 1.0f / (float)hop;
    a.stride = plan->stride;
    a.frame_stride = frame_stride;
    return a;
}

// tails, carry, final stage: the three launches of a scan on frames, a mark behind each
int launch_frames_scan(const rf_var2_plan *plan, const Var2FramesArgs &a, hipStream_t stream, LaunchTimer &timer) {
    int rc = launch_var2_frames_tails(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc == RF_OK) rc = launch_var2_carry(scan_args(plan, a.causal != 0, a.adjoint != 0), stream);
    if (rc == RF_OK) rc = timer.mark();
    Var2FramesArgs last = a;
    if (!a.adjoint) last.x = a.dst;      // v; the scan finishes on it in place
    if (rc == RF_OK) rc = launch_var2_frames_pass2(last, stream);
    if (rc == RF_OK) rc = timer.mark();
    return rc;
}

size_t frames_span_bytes(int n_lines, int n_frames, int64_t frame_stride) { return (size_t)((int64_t)(n_lines - 1) * frame_stride + n_frames) * sizeof(float); }

}  // namespace

int run_var2_expand_frames(const void *frames, int hop, int n_frames, int64_t frame_stride, int64_t length, int lines, int64_t stride, void *out,
                           hipStream_t stream) {
    if (length < 1 || length % 4 != 0 || length > kVar2MaxLength)
        return refuse(RF_ERR_INVALID_ARG, "length must be a positive multiple of 4, at most 2^30 (got %lld)", length);
    if (lines < 1 || lines > kVar2MaxLines) return refuse(RF_ERR_INVALID_ARG, "lines must be 1..%lld (got %lld)", kVar2MaxLines, lines);
    if (stride < length || stride % 4 != 0 || stride > kVar2MaxStride)
        return refuse(RF_ERR_INVALID_ARG, "stride must be a multiple of 4, at least the length and at most 2^40 (got %lld for a length of %lld)", stride, length);
    int rc = check_frames_layout(length, hop, n_frames, frame_stride);
    if (rc != RF_OK) return rc;
    if (!frames || !out) return refuse(RF_ERR_INVALID_ARG, "null pointer (frames, out)");
    if (((uintptr_t)out & 15u) != 0 || ((uintptr_t)frames & 3u) != 0) { set_error("%s", kFrameAlign); return RF_ERR_INVALID_ARG; }
    if (overlap(out, (size_t)((int64_t)(lines - 1) * stride + length) * sizeof(float), frames, frames_span_bytes(lines, n_frames, frame_stride)))
        return refuse(RF_ERR_INVALID_ARG, "out overlaps the frames");
    Var2ExpandArgs a{};
    a.frames = (const float *)frames;
    a.out = (float *)out;
    a.n = (int32_t)length;
    a.n_lines = lines;
    a.hop_shift = hop_shift_of(hop);
    a.n_frames = n_frames;
    a.inv_hop = 1.0f / (float)hop;
    a.stride = stride;
    a.frame_stride = frame_stride;
    return launch_var2_expand_frames(a, stream);
}

int run_var2_biquad_frames(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int hop, int n_frames, int64_t frame_stride, void *out,
                           hipStream_t stream, float *ms_out) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    int rc = check_frames_layout(plan->length, hop, n_frames, frame_stride);
    if (rc != RF_OK) return rc;
    if (!frames) return refuse(RF_ERR_INVALID_ARG, "null frames");
    rc = check_plane("signal", 0, {{in}, {out}}, 15u, "null pointer (in, out)", kFrameAlign);
    if (rc == RF_OK) rc = check_plane("frames", 0, {{frames->b0}, {frames->b1}, {frames->b2}, {frames->a1}, {frames->a2}}, 3u,
                                      "null pointer (b0, b1, b2, a1, a2)", kFrameAlign);
    if (rc != RF_OK) return rc;
    const size_t bytes = plan->span_bytes(), frame_bytes = frames_span_bytes(plan->n_lines, n_frames, frame_stride);
    const void *const written[1] = {out}, *const coefficients[5] = {frames->b0, frames->b1, frames->b2, frames->a1, frames->a2}, *const input[1] = {in};
    const PlaneList w = {"out", written, 1, bytes};
    const PlaneList r[2] = {{"in", input, 1, bytes,
                             ": in == out is not allowed for a biquad (the first launch stores the feed-forward part while neighbouring groups still read in)"},
                            {"frames", coefficients, 5, frame_bytes, ": a frame array is read while outputs are stored"}};
    rc = check_written_planes(&w, 1, r, 2, {"grad_out", nullptr, 0, bytes});
    if (rc != RF_OK) return rc;
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    LaunchTimer timer(stream, ms_out, plan->frames_names.size());
    if (timer.status() != RF_OK) return timer.status();
    Var2FramesArgs a = frames_args(plan, *frames, hop, n_frames, frame_stride, plan->causal, false);
    a.x = (const float *)in;
    a.dst = (float *)out;
    rc = launch_frames_scan(plan, a, stream, timer);
    return rc == RF_OK ? timer.finish() : rc;
}

int run_var2_biquad_frames_backward(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int hop, int n_frames, int64_t frame_stride,
                                    const void *out, const void *grad_out, void *grad_in, const rf_var2_section_grad *frame_grads,
                                    hipStream_t stream, float *ms_out, bool in_required) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    int rc = check_frames_layout(plan->length, hop, n_frames, frame_stride);
    if (rc != RF_OK) return rc;
    if (!frames) return refuse(RF_ERR_INVALID_ARG, "null frames");
    const rf_var2_section_grad none{};
    const rf_var2_section_grad &fg = frame_grads ? *frame_grads : none;
    const int given = (fg.b0 != nullptr) + (fg.b1 != nullptr) + (fg.b2 != nullptr) + (fg.a1 != nullptr) + (fg.a2 != nullptr);
    const bool with_frames = given == 5;
    // (null pointers are refused first; the count of the frame gradients behind them, as the header orders the refusals)
    // (in_required == false: a cascade of one section, which reads nothing of the forward without frame gradients)
    rc = check_plane("signal", 0, {{in, in_required || with_frames}, {grad_out}, {grad_in}, {out, with_frames}}, 15u,
                     "null pointer (in, grad_out, grad_in; out where frame gradients are asked for)", kFrameAlign);
    if (rc == RF_OK) rc = check_plane("frames", 0, {{frames->b0}, {frames->b1}, {frames->b2}, {frames->a1}, {frames->a2}, {fg.b0, false}, {fg.b1, false},
                                                    {fg.b2, false}, {fg.a1, false}, {fg.a2, false}}, 3u, "null pointer (b0, b1, b2, a1, a2)", kFrameAlign);
    if (rc != RF_OK) return rc;
    if (given != 0 && given != 5)
        return refuse(RF_ERR_INVALID_ARG, "the five frame gradients are all given or all null (the fold forms the five; %lld given)", given);
    const size_t bytes = plan->span_bytes(), frame_bytes = frames_span_bytes(plan->n_lines, n_frames, frame_stride);
    const void *const gin[1] = {grad_in}, *const gframes[5] = {fg.b0, fg.b1, fg.b2, fg.a1, fg.a2},
                      *const coefficients[5] = {frames->b0, frames->b1, frames->b2, frames->a1, frames->a2}, *const input[1] = {in},
                      *const result[1] = {out}, *const gout[1] = {grad_out};
    const PlaneList written[2] = {{"grad_in", gin, 1, bytes}, {"gradient of frames", gframes, with_frames ? 5 : 0, frame_bytes}};
    const PlaneList read[3] = {{"frames", coefficients, 5, frame_bytes, ": a frame array is read while outputs are stored"},
                               {"in", input, 1, bytes},
                               {"out", result, with_frames ? 1 : 0, bytes}};
    rc = check_written_planes(written, 2, read, 3, {"grad_out", gout, 1, bytes});
    if (rc != RF_OK) return rc;
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    if (!plan->lam && hipMalloc((void **)&plan->lam, bytes) != hipSuccess) {
        (void)hipGetLastError();
        plan->lam = nullptr;
        set_error("hipMalloc of %zu bytes for the adjoint state of the biquad's backward failed", bytes);
        return RF_ERR_NOMEM;
    }
    const size_t slab_bytes = plan->frames_slab_needed(hop);
    if (with_frames && plan->frames_slab_bytes < slab_bytes) {
        // (hipFree waits for the device: no earlier call on this plan still uses the slab)
        if (plan->frames_slab) (void)hipFree(plan->frames_slab);
        plan->frames_slab = nullptr;
        plan->frames_slab_bytes = 0;
        if (hipMalloc((void **)&plan->frames_slab, slab_bytes) != hipSuccess) {
            (void)hipGetLastError();
            plan->frames_slab = nullptr;
            set_error("hipMalloc of %zu bytes for the partial sums of the frame gradients failed", slab_bytes);
            return RF_ERR_NOMEM;
        }
        plan->frames_slab_bytes = slab_bytes;
    }
    LaunchTimer timer(stream, ms_out, plan->frames_backward_names[with_frames ? 1 : 0].size());
    if (timer.status() != RF_OK) return timer.status();
    Var2FramesArgs a = frames_args(plan, *frames, hop, n_frames, frame_stride, !plan->causal, true);
    a.x = (const float *)grad_out;
    a.dst = plan->lam;
    rc = launch_frames_scan(plan, a, stream, timer);
    if (rc != RF_OK) return rc;
    Var2FramesGradArgs g{};
    g.lam = plan->lam;
    g.x = (const float *)in;
    g.y = (const float *)out;
    g.b0 = (const float *)frames->b0;
    g.b1 = (const float *)frames->b1;
    g.b2 = (const float *)frames->b2;
    g.grad_in = (float *)grad_in;
    g.slab = plan->frames_slab;
    g.grad_b0 = (float *)fg.b0;
    g.grad_b1 = (float *)fg.b1;
    g.grad_b2 = (float *)fg.b2;
    g.grad_a1 = (float *)fg.a1;
    g.grad_a2 = (float *)fg.a2;
    g.n = (int32_t)plan->length;
    g.n_lines = plan->n_lines;
    g.causal = plan->causal ? 1 : 0;
    g.with_frames = with_frames ? 1 : 0;
    g.hop_shift = a.hop_shift;
    g.n_frames = n_frames;
    g.pieces = (int32_t)var2_frames_pieces(plan->length, hop);
    g.inv_hop = a.inv_hop;
    g.stride = plan->stride;
    g.frame_stride = frame_stride;
    rc = launch_var2_frames_grad(g, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc == RF_OK && with_frames) {
        rc = launch_var2_frames_fold(g, stream);
        if (rc == RF_OK) rc = timer.mark();
    }
    return rc == RF_OK ? timer.finish() : rc;
}

// ---- a cascade of sections on control-rate frames ----------------------------------------------------------------------------------
//   forward    var2_biquad_frames_tails_1d (v_0 to out, or to kept[0]), then per boundary var2_carry_1d and var2_frames_link_1d
//              (var2_frames_link_keep_1d where the caller keeps: section k's v, then its result, in kept[k]), then var2_carry_1d and
//              var2_frames_pass2_1d.  No coefficient signal exists: 8 K + 8 bytes per sample, 4 more per kept signal.
//   backward   on the kept signals, nothing rerun: var2_adj_frames_tails_1d on grad_out; per boundary from the last one down
//              var2_carry_1d and var2_adj_frames_link_1d -- with frame gradients var2_adj_frames_link_keep_1d, lam_k to the plan's
//              lam, and var2_frames_coef_1d: section k's sums into its part of the slab -- then var2_carry_1d,
//              var2_adj_frames_pass2_1d and var2_biquad_frames_grad_1d for section 0, and var2_frames_fold_cascade_1d for all.
// One section: run_var2_biquad_frames and run_var2_biquad_frames_backward, their launches and bits.
//   with a state (rf_var2_plan_execute_cascade_frames_stream; `state` with either pointer given): the forward's launches on
//              their STREAM instances, one section included; the state's checks follow the call's own.
const char *var2_cascade_frames_name(const rf_var2_plan *plan, int n_sections, bool keep, size_t i) {
    if (n_sections == 1) return plan->frames_names[i].c_str();
    if (i == 0) return "var2_biquad_frames_tails_1d";
    if (i + 1 == (size_t)var2_cascade_frames_launches(n_sections)) return "var2_frames_pass2_1d";
    return i % 2 == 1 ? "var2_carry_1d" : keep ? "var2_frames_link_keep_1d" : "var2_frames_link_1d";
}

const char *var2_cascade_frames_stream_name(int n_sections, bool keep, size_t i) {
    if (i == 0) return "var2_biquad_frames_tails_stream_1d";
    if (i + 1 == (size_t)var2_cascade_frames_stream_launches(n_sections)) return "var2_frames_pass2_stream_1d";
    return i % 2 == 1 ? "var2_carry_1d" : keep ? "var2_frames_link_keep_stream_1d" : "var2_frames_link_stream_1d";
}

const char *var2_cascade_frames_stream_backward_name(int n_sections, bool with_frames, size_t i) {
    static const char *const last[4] = {"var2_carry_1d", "var2_adj_frames_pass2_stream_1d", "var2_biquad_frames_grad_stream_1d", "var2_frames_fold_cascade_1d"};
    const size_t launches = (size_t)var2_cascade_frames_stream_backward_launches(n_sections, with_frames), tail = with_frames ? 4 : 3;
    if (i == 0) return "var2_adj_frames_tails_stream_1d";
    if (i + tail >= launches) return last[i + tail - launches];
    const size_t at = (i - 1) % (with_frames ? 3 : 2);      // within the launches of one boundary
    return at == 0 ? "var2_carry_1d" : at == 2 ? "var2_frames_coef_stream_1d" : with_frames ? "var2_adj_frames_link_keep_stream_1d" : "var2_adj_frames_link_stream_1d";
}

const char *var2_cascade_frames_backward_name(const rf_var2_plan *plan, int n_sections, bool with_frames, size_t i) {
    if (n_sections == 1) return plan->frames_backward_names[with_frames ? 1 : 0][i].c_str();
    static const char *const last[4] = {"var2_carry_1d", "var2_adj_frames_pass2_1d", "var2_biquad_frames_grad_1d", "var2_frames_fold_cascade_1d"};
    const size_t launches = (size_t)var2_cascade_frames_backward_launches(n_sections, with_frames), tail = with_frames ? 4 : 3;
    if (i == 0) return "var2_adj_frames_tails_1d";
    if (i + tail >= launches) return last[i + tail - launches];
    const size_t at = (i - 1) % (with_frames ? 3 : 2);      // within the launches of one boundary
    return at == 0 ? "var2_carry_1d" : at == 2 ? "var2_frames_coef_1d" : with_frames ? "var2_adj_frames_link_keep_1d" : "var2_adj_frames_link_1d";
}

namespace {

// "frames k: ..." for every section: no pointer null, all 4-byte aligned
int check_section_frames(const rf_var2_section *frames, int n_sections) {
    for (int k = 0; k < n_sections; k++) {
        const rf_var2_section &s = frames[k];
        int rc = check_plane("frames", k, {{s.b0}, {s.b1}, {s.b2}, {s.a1}, {s.a2}}, 3u, "null pointer (b0, b1, b2, a1, a2)", kFrameAlign);
        if (rc != RF_OK) return rc;
    }
    return RF_OK;
}

int grow(float **signal, size_t bytes, const char *what) {
    if (*signal) return RF_OK;
    if (hipMalloc((void **)signal, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *signal = nullptr;
        set_error("hipMalloc of %zu bytes for %s failed", bytes, what);
        return RF_ERR_NOMEM;
    }
    return RF_OK;
}

}  // namespace

int run_var2_cascade_frames(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int n_sections, int hop, int n_frames,
                            int64_t frame_stride, void *out, void *const *kept, hipStream_t stream, float *ms_out, const char **names_out,
                            int capacity, bool timed, const Var2State *state) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    if (n_sections < 1 || n_sections > RF_VAR2_MAX_SECTIONS) return refuse(RF_ERR_INVALID_ARG, kSectionCount, RF_VAR2_MAX_SECTIONS, n_sections);
    const int K = n_sections;
    const bool keep = kept != nullptr && K >= 2;
    // a call with a state: the STREAM instances, one section included; both pointers null: the call without one
    const bool streamed = state && (state->in || state->out);
    const size_t launches = streamed ? (size_t)var2_cascade_frames_stream_launches(K) : (size_t)var2_cascade_frames_launches(K);
    if (timed) {
        int rc = timed_names(launches, [&](size_t i) { return streamed ? var2_cascade_frames_stream_name(K, keep, i) : var2_cascade_frames_name(plan, K, keep, i); },
                             ms_out, names_out, capacity);
        if (rc != RF_OK) return rc;
    }
    if (K == 1 && !streamed) return run_var2_biquad_frames(plan, in, frames, hop, n_frames, frame_stride, out, stream, ms_out);
    int rc = check_frames_layout(plan->length, hop, n_frames, frame_stride);
    if (rc != RF_OK) return rc;
    if (!frames) return refuse(RF_ERR_INVALID_ARG, "null frames");
    rc = check_plane("signal", 0, {{in}, {out}}, 15u, "null pointer (in, out)", kFrameAlign);
    if (rc == RF_OK && keep) rc = check_kept(kept, K - 1, true);
    if (rc == RF_OK) rc = check_section_frames(frames, K);
    if (rc != RF_OK) return rc;
    const size_t bytes = plan->span_bytes(), frame_bytes = frames_span_bytes(plan->n_lines, n_frames, frame_stride);
    SectionLists arrays("frames", K);
    for (int k = 0; k < K; k++) arrays.planes.insert(arrays.planes.end(), {frames[k].b0, frames[k].b1, frames[k].b2, frames[k].a1, frames[k].a2});
    std::vector<PlaneList> read;
    const void *const result[1] = {out}, *const input[1] = {in};
    read.push_back({"in", input, 1, bytes,
                    ": in == out is not allowed for a biquad (the first launch stores the feed-forward part while neighbouring groups still read in)"});
    for (int k = 0; k < K; k++) read.push_back(arrays.list(k, 5, frame_bytes, ": a frame array is read while outputs are stored"));
    const PlaneList written[2] = {{"out", result, 1, bytes}, {"kept", (const void *const *)kept, keep ? K - 1 : 0, bytes}};
    rc = check_written_planes(written, 1, read.data(), (int)read.size(), {"grad_out", nullptr, 0, bytes});      // out first
    if (rc != RF_OK) return rc;
    read.front().why = ": a kept signal is stored while neighbouring groups still read in";
    rc = check_written_planes(written, 2, read.data(), (int)read.size(), {"grad_out", nullptr, 0, bytes});      // then the kept signals
    if (rc != RF_OK) return rc;
    if (streamed) {
        // the state: K + 1 pairs per line; state_out is written while everything else may still be read
        const int64_t pairs = 2 * ((int64_t)K + 1);
        if (state->stride < pairs) return refuse(RF_ERR_INVALID_ARG, "state_stride must be at least 2 (n_sections + 1) = %lld (got %lld)", pairs, state->stride);
        if (((uintptr_t)state->in & 3u) != 0 || ((uintptr_t)state->out & 3u) != 0) return refuse(RF_ERR_INVALID_ARG, "state: state buffers need 4-byte aligned pointers");
        const size_t state_bytes = (size_t)((int64_t)(plan->n_lines - 1) * state->stride + pairs) * sizeof(float);
        if (state->out) {
            if (state->in && overlap(state->out, state_bytes, state->in, state_bytes)) return refuse(RF_ERR_INVALID_ARG, "state_out overlaps state_in");
            if (overlap(state->out, state_bytes, in, bytes)) return refuse(RF_ERR_INVALID_ARG, "state_out overlaps in");
            if (overlap(state->out, state_bytes, out, bytes)) return refuse(RF_ERR_INVALID_ARG, "state_out overlaps out");
            for (int k = 0; keep && k + 1 < K; k++)
                if (overlap(state->out, state_bytes, kept[k], bytes)) return refuse(RF_ERR_INVALID_ARG, "state_out overlaps kept plane %lld", k);
            for (int k = 0; k < K; k++)
                for (int i = 0; i < 5; i++)
                    if (overlap(state->out, state_bytes, arrays.planes[(size_t)(5 * k + i)], frame_bytes))
                        return refuse(RF_ERR_INVALID_ARG, "state_out overlaps frames of section %lld plane %lld", k, i);
        }
        if (state->in) {
            // (out and the kept signals are stored while the first tile's lane may still read state_in)
            if (overlap(state->in, state_bytes, out, bytes)) return refuse(RF_ERR_INVALID_ARG, "state_in overlaps out");
            for (int k = 0; keep && k + 1 < K; k++)
                if (overlap(state->in, state_bytes, kept[k], bytes)) return refuse(RF_ERR_INVALID_ARG, "state_in overlaps kept plane %lld", k);
        }
    }
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    LaunchTimer timer(stream, ms_out, launches);
    if (timer.status() != RF_OK) return timer.status();
    float *signals[RF_VAR2_MAX_SECTIONS];      // where section k's v, then its result, lies
    for (int k = 0; k < K; k++) signals[k] = keep && k + 1 < K ? (float *)kept[k] : (float *)out;
    Var2FramesArgs a = frames_args(plan, frames[0], hop, n_frames, frame_stride, plan->causal, false);
    a.x = (const float *)in;
    a.dst = signals[0];
    if (streamed) {
        a.state_in = (const float *)state->in;
        a.state_out = (float *)state->out;
        a.state_stride = state->stride;
        a.pair = 0;
    }
    rc = launch_var2_frames_tails(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    const Var2Args carry = scan_args(plan, plan->causal, false);
    for (int k = 1; k < K && rc == RF_OK; k++) {
        rc = launch_var2_carry(carry, stream);
        if (rc == RF_OK) rc = timer.mark();
        Var2FramesLinkArgs l{};
        l.x = signals[k - 1];
        l.a1 = (const float *)frames[k - 1].a1;
        l.a2 = (const float *)frames[k - 1].a2;
        l.next_b0 = (const float *)frames[k].b0;
        l.next_b1 = (const float *)frames[k].b1;
        l.next_b2 = (const float *)frames[k].b2;
        l.next_a1 = (const float *)frames[k].a1;
        l.next_a2 = (const float *)frames[k].a2;
        l.dst = signals[k];
        l.keep = keep ? signals[k - 1] : nullptr;
        l.tails = a.tails;
        l.carry = a.carry;
        l.n = a.n;
        l.tiles = a.tiles;
        l.groups = a.groups;
        l.n_lines = a.n_lines;
        l.causal = a.causal;
        l.hop_shift = a.hop_shift;
        l.n_frames = n_frames;
        l.inv_hop = a.inv_hop;
        l.stride = a.stride;
        l.frame_stride = frame_stride;
        if (streamed) {
            l.state_in = a.state_in;
            l.state_out = a.state_out;
            l.state_stride = a.state_stride;
            l.pair = k;      // section k - 1's
        }
        if (rc == RF_OK) rc = launch_var2_frames_link(l, stream);
        if (rc == RF_OK) rc = timer.mark();
    }
    if (rc == RF_OK) rc = launch_var2_carry(carry, stream);
    if (rc == RF_OK) rc = timer.mark();
    Var2FramesArgs last = frames_args(plan, frames[K - 1], hop, n_frames, frame_stride, plan->causal, false);
    last.x = last.dst = (float *)out;
    if (streamed) {
        last.state_in = a.state_in;        // (not read: the state has entered.  Given alone it still selects the STREAM instance)
        last.state_out = a.state_out;
        last.state_stride = a.state_stride;
        last.pair = K;
    }
    if (rc == RF_OK) rc = launch_var2_frames_pass2(last, stream);
    if (rc == RF_OK) rc = timer.mark();
    return rc == RF_OK ? timer.finish() : rc;
}

int run_var2_cascade_frames_backward(rf_var2_plan *plan, const void *in, const rf_var2_section *frames, int n_sections, int hop, int n_frames,
                                     int64_t frame_stride, const void *const *kept, const void *out, const void *grad_out, void *grad_in,
                                     const rf_var2_section_grad *frame_grads, hipStream_t stream, float *ms_out, const char **names_out,
                                     int capacity, bool timed, const Var2GradState *state) {
    if (!plan) return refuse(RF_ERR_INVALID_ARG, "null argument");
    if (n_sections < 1 || n_sections > RF_VAR2_MAX_SECTIONS) return refuse(RF_ERR_INVALID_ARG, kSectionCount, RF_VAR2_MAX_SECTIONS, n_sections);
    const int K = n_sections;
    // the backward of a call with a state: the STREAM instances, one section included; every pointer null: the call without one
    const bool streamed = state && (state->in || state->grad_out || state->grad_in);
    // with frame gradients: every pointer of every section given.  Anything between that and none at all is refused below
    int given = 0;
    bool partial = false;      // a section with one to four of its five
    for (int k = 0; frame_grads && k < K; k++) {
        const rf_var2_section_grad &g = frame_grads[k];
        const int own = (g.b0 != nullptr) + (g.b1 != nullptr) + (g.b2 != nullptr) + (g.a1 != nullptr) + (g.a2 != nullptr);
        partial = partial || (own != 0 && own != 5);
        given += own;
    }
    const bool with_frames = given == 5 * K;
    const size_t launches = streamed ? (size_t)var2_cascade_frames_stream_backward_launches(K, with_frames)
                                     : (size_t)var2_cascade_frames_backward_launches(K, with_frames);
    if (timed) {
        int rc = timed_names(launches, [&](size_t i) {
            return streamed ? var2_cascade_frames_stream_backward_name(K, with_frames, i) : var2_cascade_frames_backward_name(plan, K, with_frames, i);
        }, ms_out, names_out, capacity);
        if (rc != RF_OK) return rc;
    }
    if (K == 1 && !streamed)
        return run_var2_biquad_frames_backward(plan, in, frames, hop, n_frames, frame_stride, out, grad_out, grad_in, frame_grads, stream, ms_out,
                                               false);
    int rc = check_frames_layout(plan->length, hop, n_frames, frame_stride);
    if (rc != RF_OK) return rc;
    if (!frames) return refuse(RF_ERR_INVALID_ARG, "null frames");
    // without frame gradients nothing of the forward is read: in, out and kept may be null
    rc = check_plane("signal", 0, {{in, with_frames}, {grad_out}, {grad_in}, {out, with_frames}}, 15u,
                     "null pointer (grad_out, grad_in; in and out where frame gradients are asked for)", kFrameAlign);
    if (rc == RF_OK) rc = check_kept(kept, K - 1, with_frames);
    if (rc == RF_OK) rc = check_section_frames(frames, K);
    for (int k = 0; rc == RF_OK && frame_grads && k < K; k++) {
        const rf_var2_section_grad &g = frame_grads[k];
        rc = check_plane("frame gradients", k, {{g.b0, false}, {g.b1, false}, {g.b2, false}, {g.a1, false}, {g.a2, false}}, 3u, "", kFrameAlign);
    }
    if (rc != RF_OK) return rc;
    if (partial || (given != 0 && !with_frames))
        return refuse(RF_ERR_INVALID_ARG, "the five frame gradients of a section are all given or all null, and every section alike (the fold "
                                          "forms them all; %lld of %lld pointers given)", given, 5 * K);
    const size_t bytes = plan->span_bytes(), frame_bytes = frames_span_bytes(plan->n_lines, n_frames, frame_stride);
    SectionLists arrays("frames", K), gradients("gradient of frames", K);
    for (int k = 0; k < K; k++) {
        arrays.planes.insert(arrays.planes.end(), {frames[k].b0, frames[k].b1, frames[k].b2, frames[k].a1, frames[k].a2});
        if (with_frames)
            gradients.planes.insert(gradients.planes.end(), {frame_grads[k].b0, frame_grads[k].b1, frame_grads[k].b2, frame_grads[k].a1, frame_grads[k].a2});
    }
    const void *const gin[1] = {grad_in}, *const input[1] = {in}, *const result[1] = {out}, *const gout[1] = {grad_out};
    std::vector<PlaneList> written, read;
    written.push_back({"grad_in", gin, 1, bytes});
    for (int k = 0; with_frames && k < K; k++) written.push_back(gradients.list(k, 5, frame_bytes));
    for (int k = 0; k < K; k++) read.push_back(arrays.list(k, 5, frame_bytes, ": a frame array is read while outputs are stored"));
    read.push_back({"in", input, with_frames ? 1 : 0, bytes});
    read.push_back({"out", result, with_frames ? 1 : 0, bytes});
    read.push_back({"kept", kept, with_frames ? K - 1 : 0, bytes});
    rc = check_written_planes(written.data(), (int)written.size(), read.data(), (int)read.size(), {"grad_out", gout, 1, bytes});
    if (rc != RF_OK) return rc;
    if (streamed) {
        // the three state buffers: K + 1 pairs per line; grad_state_in is written while everything else may still be read
        const int64_t pairs = 2 * ((int64_t)K + 1);
        if (state->stride < pairs) return refuse(RF_ERR_INVALID_ARG, "state_stride must be at least 2 (n_sections + 1) = %lld (got %lld)", pairs, state->stride);
        if ((((uintptr_t)state->in | (uintptr_t)state->grad_out | (uintptr_t)state->grad_in) & 3u) != 0)
            return refuse(RF_ERR_INVALID_ARG, "state: state buffers need 4-byte aligned pointers");
        const size_t state_bytes = (size_t)((int64_t)(plan->n_lines - 1) * state->stride + pairs) * sizeof(float);
        if (state->grad_in) {
            if (state->in && overlap(state->grad_in, state_bytes, state->in, state_bytes)) return refuse(RF_ERR_INVALID_ARG, "grad_state_in overlaps state_in");
            if (state->grad_out && overlap(state->grad_in, state_bytes, state->grad_out, state_bytes))
                return refuse(RF_ERR_INVALID_ARG, "grad_state_in overlaps grad_state_out");
            const void *const signals[4] = {in, out, grad_out, grad_in};
            static const char *const nouns[4] = {"grad_state_in overlaps in", "grad_state_in overlaps out", "grad_state_in overlaps grad_out", "grad_state_in overlaps grad_in"};
            for (int i = 0; i < 4; i++)
                if (signals[i] && overlap(state->grad_in, state_bytes, signals[i], bytes)) return refuse(RF_ERR_INVALID_ARG, nouns[i]);
            for (int k = 0; kept && with_frames && k + 1 < K; k++)
                if (overlap(state->grad_in, state_bytes, kept[k], bytes)) return refuse(RF_ERR_INVALID_ARG, "grad_state_in overlaps kept plane %lld", k);
            for (int k = 0; k < K; k++)
                for (int i = 0; i < 5; i++) {
                    if (overlap(state->grad_in, state_bytes, arrays.planes[(size_t)(5 * k + i)], frame_bytes))
                        return refuse(RF_ERR_INVALID_ARG, "grad_state_in overlaps frames of section %lld plane %lld", k, i);
                    if (with_frames && overlap(state->grad_in, state_bytes, gradients.planes[(size_t)(5 * k + i)], frame_bytes))
                        return refuse(RF_ERR_INVALID_ARG, "grad_state_in overlaps gradient of frames of section %lld plane %lld", k, i);
                }
        }
        // (grad_in and the frame gradients are stored while state_in and grad_state_out may still be read)
        for (const void *read_state : {state->in, (const void *)state->grad_out}) {
            if (!read_state) continue;
            if (overlap(read_state, state_bytes, grad_in, bytes)) return refuse(RF_ERR_INVALID_ARG, "grad_in overlaps a state buffer that is read");
            for (int k = 0; with_frames && k < K; k++)
                for (int i = 0; i < 5; i++)
                    if (overlap(read_state, state_bytes, gradients.planes[(size_t)(5 * k + i)], frame_bytes))
                        return refuse(RF_ERR_INVALID_ARG, "gradient of frames of section %lld plane %lld overlaps a state buffer that is read", k, i);
        }
    }
    if (plan->host_only) return refuse_host_only();
    RF_HIP_CHECK(hipSetDevice(plan->device));
    rc = grow(&plan->lam, bytes, "the adjoint state of the cascade's backward");
    if (rc != RF_OK) return rc;
    if (K >= 2 && plan->cascade_spans < 1) {
        rc = grow(&plan->cascade, bytes, "the gradient between the sections of the cascade's backward");
        if (rc != RF_OK) return rc;
        plan->cascade_spans = 1;
    }
    const size_t section_bytes = plan->frames_slab_needed(hop), slab_bytes = section_bytes * (size_t)K;
    if (with_frames && plan->frames_slab_bytes < slab_bytes) {
        // (hipFree waits for the device: no earlier call on this plan still uses the slab)
        if (plan->frames_slab) (void)hipFree(plan->frames_slab);
        plan->frames_slab = nullptr;
        plan->frames_slab_bytes = 0;
        if (hipMalloc((void **)&plan->frames_slab, slab_bytes) != hipSuccess) {
            (void)hipGetLastError();
            plan->frames_slab = nullptr;
            set_error("hipMalloc of %zu bytes for the partial sums of the frame gradients failed", slab_bytes);
            return RF_ERR_NOMEM;
        }
        plan->frames_slab_bytes = slab_bytes;
    }
    LaunchTimer timer(stream, ms_out, launches);
    if (timer.status() != RF_OK) return timer.status();
    float *between = plan->cascade;                   // G: g_{k-1}
    const int64_t section_doubles = (int64_t)(section_bytes / sizeof(double));
    Var2FramesArgs a = frames_args(plan, frames[K - 1], hop, n_frames, frame_stride, !plan->causal, true);
    a.x = (const float *)grad_out;
    a.dst = plan->lam;
    if (streamed) {
        a.stream = 1;
        a.grad_state_out = (const float *)state->grad_out;
        a.grad_state_in = (float *)state->grad_in;
        a.state_stride = state->stride;
        a.add_pair = K;      // x is grad_out
        a.last_section = K - 1;
    }
    rc = launch_var2_frames_tails(a, stream);
    if (rc == RF_OK) rc = timer.mark();
    const Var2Args carry = scan_args(plan, !plan->causal, true);
    Var2FramesGradArgs g{};
    if (streamed) {
        g.stream = 1;
        g.state_in = (const float *)state->in;
        g.state_stride = state->stride;
    }
    g.lam = plan->lam;
    g.n = (int32_t)plan->length;
    g.n_lines = plan->n_lines;
    g.causal = plan->causal ? 1 : 0;
    g.with_frames = with_frames ? 1 : 0;
    g.hop_shift = a.hop_shift;
    g.n_frames = n_frames;
    g.pieces = (int32_t)var2_frames_pieces(plan->length, hop);
    g.inv_hop = a.inv_hop;
    g.stride = plan->stride;
    g.frame_stride = frame_stride;
    for (int k = K - 1; k >= 1 && rc == RF_OK; k--) {
        rc = launch_var2_carry(carry, stream);
        if (rc == RF_OK) rc = timer.mark();
        Var2AdjFramesLinkArgs l{};
        l.x = k == K - 1 ? (const float *)grad_out : between;
        l.a1 = (const float *)frames[k].a1;
        l.a2 = (const float *)frames[k].a2;
        l.b0 = (const float *)frames[k].b0;
        l.b1 = (const float *)frames[k].b1;
        l.b2 = (const float *)frames[k].b2;
        l.prev_a1 = (const float *)frames[k - 1].a1;
        l.prev_a2 = (const float *)frames[k - 1].a2;
        l.dst = between;
        l.keep = with_frames ? plan->lam : nullptr;
        l.tails = a.tails;
        l.carry = a.carry;
        l.n = a.n;
        l.tiles = a.tiles;
        l.groups = a.groups;
        l.n_lines = a.n_lines;
        l.causal = a.causal;
        l.hop_shift = a.hop_shift;
        l.n_frames = n_frames;
        l.inv_hop = a.inv_hop;
        l.stride = a.stride;
        l.frame_stride = frame_stride;
        if (streamed) {
            l.stream = 1;
            l.grad_state_out = a.grad_state_out;
            l.grad_state_in = a.grad_state_in;
            l.state_stride = a.state_stride;
            l.pair = k;
            l.add_pair = k == K - 1 ? K : -1;      // x is grad_out, or holds the addition already
            l.last_section = K - 1;
        }
        if (rc == RF_OK) rc = launch_var2_adj_frames_link(l, stream);
        if (rc == RF_OK) rc = timer.mark();
        if (rc == RF_OK && with_frames) {
            if (streamed) g.pair = k;
            g.x = (const float *)kept[k - 1];
            g.y = k == K - 1 ? (const float *)out : (const float *)kept[k];
            g.slab = plan->frames_slab + k * section_doubles;
            rc = launch_var2_frames_coef(g, stream);
            if (rc == RF_OK) rc = timer.mark();
        }
    }
    if (rc == RF_OK) rc = launch_var2_carry(carry, stream);
    if (rc == RF_OK) rc = timer.mark();
    Var2FramesArgs first = frames_args(plan, frames[0], hop, n_frames, frame_stride, !plan->causal, true);
    first.x = K == 1 ? (const float *)grad_out : between;
    first.dst = plan->lam;
    if (streamed) {
        first.stream = 1;
        first.grad_state_out = a.grad_state_out;
        first.grad_state_in = a.grad_state_in;
        first.state_stride = a.state_stride;
        first.pair = 0;
        first.add_pair = K == 1 ? K : -1;
        first.last_section = K - 1;
    }
    if (rc == RF_OK) rc = launch_var2_frames_pass2(first, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (streamed) {
        g.pair = 0;
        g.grad_state_out = (const float *)state->grad_out;
    }
    g.x = (const float *)in;
    g.y = !with_frames ? nullptr : K == 1 ? (const float *)out : (const float *)kept[0];
    g.b0 = (const float *)frames[0].b0;
    g.b1 = (const float *)frames[0].b1;
    g.b2 = (const float *)frames[0].b2;
    g.grad_in = (float *)grad_in;
    g.slab = plan->frames_slab;
    if (rc == RF_OK) rc = launch_var2_frames_grad(g, stream);
    if (rc == RF_OK) rc = timer.mark();
    if (rc == RF_OK && with_frames) {
        Var2FramesFoldCascadeArgs f{};
        f.slab = plan->frames_slab;
        f.section_doubles = section_doubles;
        for (int k = 0; k < K; k++) {
            f.grads[k][0] = (float *)frame_grads[k].b0;
            f.grads[k][1] = (float *)frame_grads[k].b1;
            f.grads[k][2] = (float *)frame_grads[k].b2;
            f.grads[k][3] = (float *)frame_grads[k].a1;
            f.grads[k][4] = (float *)frame_grads[k].a2;
        }
        f.n_sections = K;
        f.n_lines = plan->n_lines;
        f.hop_shift = a.hop_shift;
        f.n_frames = n_frames;
        f.pieces = g.pieces;
        f.frame_stride = frame_stride;
        rc = launch_var2_frames_fold_cascade(f, stream);
        if (rc == RF_OK) rc = timer.mark();
    }
    return rc == RF_OK ? timer.finish() : rc;
}

}  // namespace rf
