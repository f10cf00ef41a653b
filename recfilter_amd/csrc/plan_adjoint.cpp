// plan_adjoint.cpp -- rf_plan_backward: the transpose of a plan of constant-coefficient scans and the gradient with respect to
// its coefficients (include/recfilter_amd.h).
//
// Per line, in scan order r = 0 .. n-1 (an anticausal scan: the reversed line), a scan with input u, output y, feed-forward c0
// and feedback a_0 .. a_{k-1} is
//     y[r] = c0 u[r] + sum_{j < r} a_j y[r-j-1]                                  zero border
//          + t_r (r == 0 ? u[0] : y[0])   for r < k,   t_r = sum_{j >= r} a_j     clamped border
// With g = dL/dy and mu the unit-gain zero-border scan of g in the OPPOSITE direction (same feedback, feed-forward 1):
//     dL/du = c0 mu;   clamped: dL/du[0] += t_0 mu[0] + gamma sum_{1 <= r < k} t_r mu[r],   gamma = c0 + t_0
//     dL/da_j = sum_{r > j} mu[r] y[r-j-1];   clamped: + beta + mu[0] u[0] + y[0] sum_{1 <= r <= j} mu[r]
//     dL/dc0  = sum_r mu[r] u[r];             clamped: + beta,   beta = u[0] sum_{1 <= r < k} t_r mu[r]
// Every transposed scan is a forward plan (a child of this plan, built through build_plan and driven through child_steps /
// bind_child, plan.h); the border term and the coefficient sums are the kernels of kernels_adjoint.hip.
#include "plan_adjoint.h"

#include <algorithm>
#include <cstring>

#include "run_support.h"

namespace rf {

Adjoint::~Adjoint() {
    children.clear();
    for (void *p : owned)
        if (p) (void)hipFree(p);
}

namespace {

size_t dtype_bytes(int dtype) {
    switch (dtype) {
        case RF_F64: return 8;
        case RF_I16: case RF_F16: case RF_BF16: return 2;
        default: return 4;
    }
}

struct ChildDesc {
    rf_filter_desc d{};
    std::vector<rf_scan_desc> scans;
};

// the caller's description without its scans, shards and pointwise stages: what every child starts from
ChildDesc child_desc(const rf_plan *plan) {
    ChildDesc c;
    c.d = plan->saved.d;
    c.d.scans = nullptr;
    c.d.n_scans = 0;
    c.d.shard_extents = nullptr;
    c.d.shard_rank = 0;
    c.d.shard_world = 1;
    c.d.device = plan->host_only ? RF_DEVICE_HOST_ONLY : plan->device;
    std::memset(&c.d.pointwise, 0, sizeof(c.d.pointwise));
    return c;
}

int build_child(Adjoint *a, ChildDesc &c, bool may_fall_back, rf_plan **out) {
    c.d.scans = c.scans.data();
    c.d.n_scans = (int)c.scans.size();
    rf_plan *child = nullptr;
    int rc = build_plan(&c.d, &child);
    if (rc == RF_ERR_UNSUPPORTED && may_fall_back && c.d.path != RF_PATH_AUTO) {
        // the path (or the tiles) the caller asked for does not take a single scan of the filter: the automatic choice does
        c.d.path = RF_PATH_AUTO;
        for (int d = 0; d < RF_MAX_DIMS; d++) c.d.tile[d] = 0;
        rc = build_plan(&c.d, &child);
    }
    if (rc != RF_OK) return rc;
    a->children.emplace_back(child);
    *out = child;
    return RF_OK;
}

// the steps of `child` as launches of `list`; the first binds the child's planes and stream when it runs
int append_child(Adjoint *a, std::vector<AdjLaunch> &list, rf_plan *child, int n_planes, std::function<ChildPlanes(int)> planes) {
    std::vector<const Step *> steps;
    if (int rc = child_steps(child, steps)) return rc;
    for (auto &ex : child->exchanges) ex.send = ex.scratch;
    for (size_t i = 0; i < steps.size(); i++) {
        const Step *sp = steps[i];
        const bool first = i == 0;
        AdjLaunch l;
        l.name = sp->name;
        l.run = [a, child, sp, planes, n_planes, first]() {
            if (first) bind_child(child, n_planes, a->stream, planes);
            for (int pl = 0; pl < n_planes; pl++)
                if (int rc = sp->run(pl)) return rc;
            return (int)RF_OK;
        };
        list.push_back(std::move(l));
    }
    return RF_OK;
}

AdjGeom scan_geom(const rf_filter_desc &d, const rf_scan_desc &s) {
    AdjGeom g;
    g.total = 1;
    for (int i = 0; i < d.ndim; i++) g.total *= d.extent[i];
    g.N = d.extent[s.dim];
    g.stride = 1;
    for (int i = 0; i < s.dim; i++) g.stride *= d.extent[i];
    g.width = d.extent[0];
    g.n_planes = d.n_planes;
    g.causal = s.causal != 0;
    g.k = s.order;
    return g;
}

AdjClamp scan_clamp(const rf_scan_desc &s) {
    AdjClamp cl{};
    double t = 0.0;
    for (int r = s.order - 1; r >= 0; r--) {
        t += (double)s.feedback[r];
        cl.t[r] = t;
    }
    cl.gamma = (double)s.feedfwd + cl.t[0];
    return cl;
}

rf_scan_desc transposed(const rf_scan_desc &s) {
    rf_scan_desc t = s;
    t.causal = s.causal ? 0 : 1;
    return t;
}

template <typename P>
AdjPlanes read_planes(P *const *p, int n) {
    AdjPlanes a{};
    for (int i = 0; i < n; i++) a.p[i] = (const float *)p[i];
    return a;
}
AdjPlanesW write_planes(void *const *p, int n) {
    AdjPlanesW a{};
    for (int i = 0; i < n; i++) a.p[i] = (float *)p[i];
    return a;
}

// ---- route 1: ONE adjoint plan -- the scans reversed, every direction flipped, the affine stages composed:
// out = pf F(ps in + pb) + pi (ps in + pb) + po   =>   g_in = pf F^T(ps g) + pi ps g : prologue (ps, 0), epilogue (pf, pi, 0)
int build_route1(rf_plan *plan, Adjoint *a) {
    const rf_filter_desc &d = plan->saved.d;
    ChildDesc c = child_desc(plan);
    for (int s = d.n_scans - 1; s >= 0; s--) c.scans.push_back(transposed(plan->saved.scans[(size_t)s]));
    c.d.pointwise = d.pointwise;
    c.d.pointwise.pre_bias = 0.0f;
    c.d.pointwise.post_bias = 0.0f;
    rf_plan *child = nullptr;
    if (int rc = build_child(a, c, false, &child)) return rc;
    return append_child(a, a->plain, child, d.n_planes, [a](int q) { return ChildPlanes{a->gout[q], a->gin[q]}; });
}

// ---- route 2: per scan in reverse order, its transpose under a zero border (feed-forward c0) and the border term, in place
int build_route2(rf_plan *plan, Adjoint *a) {
    const rf_filter_desc &d = plan->saved.d;
    const int n = d.n_scans, P = d.n_planes;
    for (int s = n - 1; s >= 0; s--) {
        const rf_scan_desc &sc = plan->saved.scans[(size_t)s];
        ChildDesc c = child_desc(plan);
        c.d.border = RF_BORDER_ZERO;
        c.scans.push_back(transposed(sc));
        rf_plan *child = nullptr;
        if (int rc = build_child(a, c, true, &child)) return rc;
        const bool first = s == n - 1;
        if (int rc = append_child(a, a->plain, child, P, [a, first](int q) { return ChildPlanes{first ? a->gout[q] : a->gin[q], a->gin[q]}; }))
            return rc;
        const AdjGeom g = scan_geom(d, sc);
        const AdjClamp cl = scan_clamp(sc);
        const double inv_c0 = 1.0 / (double)sc.feedfwd;
        AdjLaunch l;
        l.name = "adjoint_border";
        l.run = [a, g, cl, inv_c0, P]() {
            return launch_adjoint_border(read_planes(a->gin, P), write_planes(a->gin, P), inv_c0, g, cl, a->stream);
        };
        a->plain.push_back(std::move(l));
    }
    return RF_OK;
}

// ---- route 3: the forward scan by scan with every output kept, then per scan in reverse order mu, the coefficient sums, and
// the next gradient c0 mu (+ the border term)
int build_route3(rf_plan *plan, Adjoint *a) {
    const rf_filter_desc &d = plan->saved.d;
    const int n = d.n_scans, P = d.n_planes;
    const bool clamped = d.border == RF_BORDER_CLAMP;
    a->Y.assign((size_t)n, std::vector<float *>((size_t)P, nullptr));
    a->M.assign((size_t)P, nullptr);
    for (int s = 0; s < n; s++) {
        ChildDesc c = child_desc(plan);
        c.scans.push_back(plan->saved.scans[(size_t)s]);
        rf_plan *child = nullptr;
        if (int rc = build_child(a, c, true, &child)) return rc;
        if (int rc = append_child(a, a->coeff, child, P, [a, s](int q) {
                return ChildPlanes{s == 0 ? a->in[q] : (const void *)a->Y[(size_t)s - 1][(size_t)q], a->Y[(size_t)s][(size_t)q]};
            }))
            return rc;
    }
    for (int s = n - 1; s >= 0; s--) {
        const rf_scan_desc &sc = plan->saved.scans[(size_t)s];
        ChildDesc c = child_desc(plan);
        c.d.border = RF_BORDER_ZERO;
        rf_scan_desc unit = transposed(sc);
        unit.feedfwd = 1.0f;
        c.scans.push_back(unit);
        rf_plan *child = nullptr;
        if (int rc = build_child(a, c, true, &child)) return rc;
        const bool first = s == n - 1;
        if (int rc = append_child(a, a->coeff, child, P, [a, first](int q) {
                return ChildPlanes{first ? a->gout[q] : (const void *)a->gin[q], a->M[(size_t)q]};
            }))
            return rc;
        const AdjGeom g = scan_geom(d, sc);
        const AdjClamp cl = scan_clamp(sc);
        const float c0 = sc.feedfwd;
        auto u_planes = [a, s, P]() { return s == 0 ? read_planes(a->in, P) : read_planes(a->Y[(size_t)s - 1].data(), P); };
        AdjLaunch grad;
        grad.name = "coeff_grad";
        grad.run = [a, g, cl, clamped, c0, s, P, u_planes]() {
            return launch_coeff_grad(read_planes(a->M.data(), P), u_planes(), read_planes(a->Y[(size_t)s].data(), P), write_planes(a->gin, P),
                                     c0, g, clamped ? &cl : nullptr, a->slabs, &a->n_slabs, a->stream);
        };
        a->coeff.push_back(std::move(grad));
        AdjLaunch sum;
        sum.name = "coeff_grad_sum";
        sum.run = [a, g, s]() { return launch_coeff_grad_sum(a->slabs, a->n_slabs, g.k, a->gcoeff + (size_t)s * kAdjSlabDoubles, a->stream); };
        a->coeff.push_back(std::move(sum));
        if (clamped) {
            AdjLaunch border;
            border.name = "adjoint_border";
            border.run = [a, g, cl, P]() {
                return launch_adjoint_border(read_planes(a->M.data(), P), write_planes(a->gin, P), 1.0, g, cl, a->stream);
            };
            a->coeff.push_back(std::move(border));
        }
    }
    return RF_OK;
}

size_t route3_bytes(const rf_filter_desc &d) {
    size_t total = 1;
    for (int i = 0; i < d.ndim; i++) total *= (size_t)d.extent[i];
    return ((size_t)d.n_scans + 1) * (size_t)d.n_planes * total * sizeof(float) + (size_t)kAdjMaxSlabs * kAdjSlabDoubles * sizeof(double);
}

int ensure_workspace(rf_plan *plan, Adjoint *a) {
    if (a->workspace_ready) return RF_OK;
    const rf_filter_desc &d = plan->saved.d;
    size_t total = 1;
    for (int i = 0; i < d.ndim; i++) total *= (size_t)d.extent[i];
    auto take = [&](size_t bytes, void **out) {
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("rf_plan_backward: the workspace of the coefficient gradients needs %zu bytes of device memory", route3_bytes(d));
            return (int)RF_ERR_NOMEM;
        }
        a->owned.push_back(p);
        *out = p;
        return (int)RF_OK;
    };
    for (auto &row : a->Y)
        for (auto &p : row)
            if (!p)
                if (int rc = take(total * sizeof(float), (void **)&p)) return rc;
    for (auto &p : a->M)
        if (!p)
            if (int rc = take(total * sizeof(float), (void **)&p)) return rc;
    if (!a->slabs)
        if (int rc = take((size_t)kAdjMaxSlabs * kAdjSlabDoubles * sizeof(double), (void **)&a->slabs)) return rc;
    a->workspace_ready = true;
    return RF_OK;
}

// what the description alone decides (the refusals of the header from the pixel type on)
int refuse_description(const rf_plan *plan, bool with_coeffs) {
    const rf_filter_desc &d = plan->saved.d;
    if (d.dtype != RF_F32) { set_error("rf_plan_backward: f32 pixels only (dtype %d)", d.dtype); return RF_ERR_UNSUPPORTED; }
    if (d.pointwise.in_dtype != RF_IN_PIXEL) { set_error("rf_plan_backward: unsigned-byte planes are not supported"); return RF_ERR_UNSUPPORTED; }
    if (d.shard_world > 1 || (d.flags & RF_PLAN_FORCE_EXCHANGE)) { set_error("rf_plan_backward: sharded plans are not supported"); return RF_ERR_UNSUPPORTED; }
    if (with_coeffs && d.pointwise.flags != 0) {
        set_error("rf_plan_backward: coefficient gradients of a plan with pointwise stages are not supported");
        return RF_ERR_UNSUPPORTED;
    }
    if (d.border == RF_BORDER_CLAMP) {
        for (int s = 0; s < d.n_scans; s++) {
            const rf_scan_desc &sc = plan->saved.scans[(size_t)s];
            if (d.extent[sc.dim] <= sc.order) {
                set_error("rf_plan_backward: clamped border: scan %d of order %d needs more than %d samples along dimension %d", s, sc.order,
                          sc.order, sc.dim);
                return RF_ERR_UNSUPPORTED;
            }
            if (sc.feedfwd == 0.0f) { set_error("rf_plan_backward: clamped border: scan %d has a zero feed-forward", s); return RF_ERR_UNSUPPORTED; }
        }
        if (d.n_scans > 0 && d.pointwise.flags != 0) {
            set_error("rf_plan_backward: a clamped plan with pointwise stages is not supported");
            return RF_ERR_UNSUPPORTED;
        }
    }
    if (with_coeffs && d.n_scans == 0) { set_error("rf_plan_backward: the plan has no scans, hence no coefficients"); return RF_ERR_UNSUPPORTED; }
    return RF_OK;
}

int ensure_built(rf_plan *plan, bool with_coeffs) {
    if (!plan->adjoint) plan->adjoint = std::make_shared<Adjoint>();
    Adjoint *a = plan->adjoint.get();
    const rf_filter_desc &d = plan->saved.d;
    if (with_coeffs) {
        if (a->coeff_built) return RF_OK;
        a->coeff.clear();
        const int rc = build_route3(plan, a);
        if (rc == RF_OK) a->coeff_built = true;
        else a->coeff.clear();
        return rc;
    }
    if (a->plain_built) return RF_OK;
    a->plain.clear();
    const int rc = (d.border == RF_BORDER_CLAMP && d.n_scans > 0) ? build_route2(plan, a) : build_route1(plan, a);
    if (rc == RF_OK) a->plain_built = true;
    else a->plain.clear();
    return rc;
}

}  // namespace

int plan_backward(rf_plan *plan, const void *const *in_planes, const void *const *grad_out_planes, void *const *grad_in_planes,
                  double *grad_coeffs, void *stream, bool timed, float *ms_out, const char **names_out, int capacity) {
    // ---- the refusals, in the order of the header, before any HIP call
    if (!plan || !grad_out_planes || !grad_in_planes) { set_error("rf_plan_backward: null argument"); return RF_ERR_INVALID_ARG; }
    const bool with_coeffs = grad_coeffs != nullptr;
    if (with_coeffs && !in_planes) { set_error("rf_plan_backward: coefficient gradients need in_planes"); return RF_ERR_INVALID_ARG; }
    if (!with_coeffs && in_planes) { set_error("rf_plan_backward: in_planes must be NULL without grad_coeffs"); return RF_ERR_INVALID_ARG; }
    const rf_filter_desc &d = plan->saved.d;
    const int P = d.n_planes;
    // null planes first, then (mask 15) every plane's alignment
    auto check_planes = [&](uintptr_t mask) {
        for (int pl = 0; pl < P; pl++)
            if (int rc = check_plane("rf_plan_backward: plane", pl, {{grad_out_planes[pl]}, {grad_in_planes[pl]}, {with_coeffs ? in_planes[pl] : nullptr, with_coeffs}},
                                     mask, "null image pointer", "this plan's kernels need 16-byte aligned image pointers"))
                return rc;
        return (int)RF_OK;
    };
    if (int rc = check_planes(0)) return rc;
    if (wants_aligned_planes(plan))
        if (int rc = check_planes(15u)) return rc;
    if (with_coeffs && ((uintptr_t)grad_coeffs & 7u)) { set_error("rf_plan_backward: grad_coeffs must be 8-byte aligned"); return RF_ERR_INVALID_ARG; }
    // what is written (grad_in planes, the rows of grad_coeffs) against everything that is read and everything else that is written
    size_t plane_bytes = dtype_bytes(d.dtype);
    for (int i = 0; i < d.ndim; i++) plane_bytes *= (size_t)d.extent[i];
    const void *const coeff_rows = grad_coeffs;
    const PlaneList written[2] = {{"grad_in", (const void *const *)grad_in_planes, P, plane_bytes},
                                  {"grad_coeffs", &coeff_rows, with_coeffs ? 1 : 0, (size_t)std::max(d.n_scans, 1) * kAdjSlabDoubles * sizeof(double)}};
    const PlaneList read = {"in", in_planes, with_coeffs ? P : 0, plane_bytes};
    if (int rc = check_written_planes(written, 2, &read, 1, {"grad_out", grad_out_planes, P, plane_bytes})) return rc;
    if ((d.pointwise.flags & RF_POINTWISE_POST) && d.pointwise.post_input != 0.0f)
        for (int pl = 0; pl < P; pl++)
            if (grad_in_planes[pl] == grad_out_planes[pl]) {
                set_error("rf_plan_backward: plane %d: an epilogue that reads the input needs grad_in != grad_out", pl);
                return RF_ERR_INVALID_ARG;
            }
    if (int rc = refuse_description(plan, with_coeffs)) return rc;
    if (plan->host_only) { set_error("host-only plan (RF_DEVICE_HOST_ONLY) cannot run a backward"); return RF_ERR_HIP; }

    // ---- build on first need, then run
    RF_HIP_CHECK(hipSetDevice(plan->device));
    if (int rc = ensure_built(plan, with_coeffs)) return rc;
    Adjoint *a = plan->adjoint.get();
    // (a single scan of a filter may run on a path that moves 16 bytes per lane where the whole filter's plan does not)
    for (const auto &child : a->children)
        if (wants_aligned_planes(child.get()))
            if (int rc = check_planes(15u)) return rc;
    if (with_coeffs)
        if (int rc = ensure_workspace(plan, a)) return rc;
    for (int pl = 0; pl < P; pl++) {
        a->in[pl] = with_coeffs ? in_planes[pl] : nullptr;
        a->gout[pl] = grad_out_planes[pl];
        a->gin[pl] = grad_in_planes[pl];
    }
    a->gcoeff = grad_coeffs;
    a->stream = (hipStream_t)stream;
    const std::vector<AdjLaunch> &list = with_coeffs ? a->coeff : a->plain;
    if (timed)
        if (int rc = timed_names(list.size(), [&](size_t i) { return list[i].name.c_str(); }, ms_out, names_out, capacity)) return rc;
    LaunchTimer timer(a->stream, timed ? ms_out : nullptr, list.size());
    if (timer.status() != RF_OK) return timer.status();
    for (const AdjLaunch &l : list) {
        if (int rc = l.run()) return rc;
        if (int rc = timer.mark()) return rc;
    }
    return timer.finish();
}

int plan_backward_num_kernels(rf_plan *plan, int with_coeffs) {
    if (!plan || refuse_description(plan, with_coeffs != 0) != RF_OK) return 0;
    if (!plan->host_only && hipSetDevice(plan->device) != hipSuccess) return 0;
    if (ensure_built(plan, with_coeffs != 0) != RF_OK) return 0;
    return (int)(with_coeffs ? plan->adjoint->coeff.size() : plan->adjoint->plain.size());
}

size_t plan_backward_workspace_bytes(const rf_plan *plan, int with_coeffs) {
    if (!plan || !with_coeffs || refuse_description(plan, true) != RF_OK) return 0;
    return route3_bytes(plan->saved.d);
}

}  // namespace rf
