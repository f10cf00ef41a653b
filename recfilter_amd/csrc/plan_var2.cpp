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
// end of the file; its backward keeps the adjoint state in one signal the plan allocates in the first such call.
#include "plan_var2.h"

#include <memory>

rf_var2_plan::~rf_var2_plan() {
    if (workspace) (void)hipFree(workspace);
    if (lam) (void)hipFree(lam);
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

}  // namespace rf
