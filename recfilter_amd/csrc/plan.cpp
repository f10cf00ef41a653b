// plan.cpp -- plan construction: validation, scan grouping, path choice, tables, step lists.
//
// build_plan, at the end of the rf namespace, runs these stages; their ORDER is behaviour:
//    1. validate_desc           2. plan_merged_runs: 1-D runs of same-direction scans as ONE scan each, if that plan is kept
//    3. describe: device, shard extents, dims, scans grouped by dimension
//    4. half_plan_is_native: 16-bit pixels run natively on the fused kernels, or as build_staged_half -- done
//    5. rewrite_into_sections: orders 4..8 as sections of order <= 3; fused_plan_applicable is then evaluated ONCE
//    6. try_clamped_1d -- done  7. try_cascade -- done            (wrappers: child plans driven through the helpers of plan.h)
//    8. choose_auto_path, check_path
//    9. build_on_path and its two fall-backs: 16-bit -> staged, RF_PATH_AUTO -> untiled
//   10. add_pointwise_steps, publish_scans_table                 11. finish: the one exit of every successful build
//
// Reference behaviour restated here (host side only):
//   * argument checks of RecFilter::add_filter      lib/recfilter.cpp:274-300
//   * group_scans_by_dimension                      lib/split.cpp:215-242  (with the
//     coefficient permutation the reference forgets)
//   * split() preconditions (tile divides extent)   lib/recfilter.h:311, lib/split.cpp:1879-1931
#include "plan.h"
#include "sections.h"
#include "plan_generic.h"
#include "plan_clamp1d.h"
#include "plan_strided.h"

#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstring>

namespace rf {

int build_fused_plan(rf_plan *plan, const rf_filter_desc *desc);  // plan_fused.cpp
bool fused_plan_applicable(const rf_plan *plan, const rf_filter_desc *desc, std::string *why);
int build_overlap_plan(rf_plan *plan, const rf_filter_desc *desc);  // plan_overlap.cpp
bool overlap_plan_applicable(const rf_plan *plan, const rf_filter_desc *desc, std::string *why);
int build_matrix_plan(rf_plan *plan, const rf_filter_desc *desc);   // plan_matrix.cpp
bool matrix_plan_applicable(const rf_plan *plan, const rf_filter_desc *desc, std::string *why);

// ---- a plan driven by another plan (plan.h) ------------------------------------------------------------------------------
std::vector<const Step *> single_device_steps(const rf_plan *plan, bool with_apply) {
    std::vector<const Step *> v;
    auto add = [&v](const std::vector<Step> &steps) { for (const Step &s : steps) v.push_back(&s); };
    add(plan->begin_steps);
    for (const auto &ex : plan->exchange_local_steps) add(ex);
    add(plan->interior_steps);
    if (with_apply)
        for (const auto &ex : plan->exchange_apply_steps) add(ex);
    add(plan->finish_steps);
    return v;
}

int child_steps(const rf_plan *child, std::vector<const Step *> &steps) {
    if (child->sharded() || !child->interior_steps.empty()) {
        set_error("a plan driven as steps of another plan must be unsharded");
        return RF_ERR_UNSUPPORTED;
    }
    // (the generic path keeps the exchange structure of an unsharded outermost dimension: those apply steps would propagate
    // the carry entering the slab -- zero, nobody gathers one here -- and a wrapper does not launch them)
    steps = single_device_steps(child, false);
    return RF_OK;
}

void append_child_steps(rf_plan *parent, rf_plan *child, const std::vector<const Step *> &steps, const std::string &prefix,
                        std::function<ChildPlanes(int plane)> planes) {
    for (size_t k = 0; k < steps.size(); k++) {
        const Step *sp = steps[k];
        Step w;
        w.name = prefix + sp->name;
        if (k == 0)
            w.run = [parent, child, sp, planes](int pl) {
                if (pl == 0) bind_child(child, parent->n_planes, parent->stream, planes);
                return sp->run(pl);
            };
        else w.run = [sp](int pl) { return sp->run(pl); };
        parent->begin_steps.push_back(w);
    }
}

void take_over_child(rf_plan *parent, rf_plan *child, bool shown) {
    parent->workspace_bytes += child->workspace_bytes;
    for (auto &ex : child->exchanges) ex.send = ex.scratch;
    if (!shown) return;
    for (int d = 0; d < RF_MAX_DIMS; d++) { parent->dims[d].T = child->dims[d].T; parent->dims[d].M = child->dims[d].M; }
    parent->tables = child->tables;
}

namespace {

double cast_coeff(double c, int dtype) {
    switch (dtype) {
        case RF_F32: return (double)(float)c;
        case RF_F16: case RF_BF16: return (double)(float)c;      // storage types: the coefficients are the f32 plan's (pixel.h)
        case RF_F64: return c;
        case RF_I32: return (double)(int32_t)c;   // Cast::make(Int(32), float): truncation
        case RF_I16: return (double)(int16_t)c;
    }
    return c;
}

// The untiled operator with the line-parallel kernels (kernels_lines.hip): pixel types of 2 / 4 bytes in the 32-bit
// arithmetic, orders <= 3, <= 4 scans per dimension, extents that are multiples of 16 (a lane owns 16 samples; the
// lines of a strided dimension are moved 16 at a time).
bool line_scans_applicable(const rf_plan *plan) {
    if (plan->sharded() || plan->scans.empty()) return false;
    if ((plan->flags & RF_PLAN_SERIAL_UNTILED) || RF_KNOB("RF_NO_LINE_SCANS") != nullptr) return false;     // the one-thread-per-line kernel
    bool strided = false;
    for (int d = 0; d < plan->ndim; d++) {
        const DimInfo &di = plan->dims[d];
        if (di.scan_ids.empty()) continue;
        if (di.k > kFusedMaxK || (int)di.scan_ids.size() > kFusedMaxScans || di.N % 16 != 0) return false;
        if (d > 0) strided = true;
    }
    if (strided && plan->dims[0].N % 16 != 0) return false;
    return true;
}

template <typename P, typename S>
int build_line_scans(rf_plan *plan) {
    using Acc = typename PixelTraits<P>::Acc;
    bool first = true;
    plan->vector_access = true;          // load16 / store16 / load_lines16 of kernels_lines.hip
    for (int d = 0; d < plan->ndim; d++) {
        const DimInfo &di = plan->dims[d];
        if (di.scan_ids.empty()) continue;
        LineScanArgs<Acc> a{};
        a.n = di.N; a.inner = di.stride; a.lines = di.lines;
        a.n_scans = (int)di.scan_ids.size();
        a.clamped = plan->clamped ? 1 : 0;
        for (int i = 0; i < a.n_scans; i++) a.scans[i] = make_fused_scan<S, Acc>(plan->scans[di.scan_ids[i]], di.k, true);
        const bool from_input = first, strided = d > 0;
        const int K = di.k;
        first = false;
        Step st;
        st.name = std::string("line_scans_") + "xyz"[d];
        st.run = [plan, a, K, strided, from_input](int pl) {
            const P *src = from_input ? (const P *)plan->in[pl] : (const P *)plan->out[pl];
            return launch_line_scans<P>(K, strided, src, (P *)plan->out[pl], a, plan->stream);
        };
        plan->begin_steps.push_back(st);
    }
    return RF_OK;
}

// ---------------------------------------------------------------------------------------
template <typename P>
int build_untiled(rf_plan *plan) {
    using Acc = typename PixelTraits<P>::Acc;
    if (plan->sharded()) {
        set_error("the untiled path cannot be sharded across devices");
        return RF_ERR_UNSUPPORTED;
    }
    {
        using S = typename std::conditional<PixelTraits<P>::is_integer, uint64_t, double>::type;
        if (line_scans_applicable(plan)) return build_line_scans<P, S>(plan);
    }
    bool first = true;
    for (size_t i = 0; i < plan->scans.size(); i++) {
        const Scan &s = plan->scans[i];
        const DimInfo &d = plan->dims[s.dim];
        LineGeom g{d.N, d.stride, d.lines};
        DevScan<Acc> sc = make_dev_scan<Acc>(s);
        bool from_input = first;
        bool clamped = plan->clamped;
        first = false;
        Step st;
        st.name = std::string("untiled_scan_") + "xyz"[s.dim] + (s.causal ? "+" : "-");
        st.run = [plan, g, sc, from_input, clamped](int pl) {
            const P *src = from_input ? (const P *)plan->in[pl] : (const P *)plan->out[pl];
            return launch_untiled_scan<P>(src, (P *)plan->out[pl], g, sc, clamped, plan->stream);
        };
        plan->begin_steps.push_back(st);
    }
    if (plan->scans.empty()) {
        Step st;
        st.name = "copy";
        st.run = [plan](int pl) -> int {
            if (plan->in[pl] != plan->out[pl])
                RF_HIP_CHECK(hipMemcpyAsync(plan->out[pl], plan->in[pl], plan->total * sizeof(P),
                                            hipMemcpyDeviceToDevice, plan->stream));
            return (int)RF_OK;
        };
        plan->begin_steps.push_back(st);
    }
    return RF_OK;
}

// ---------------------------------------------------------------------------------------
template <typename P, typename S>
int build_generic(rf_plan *plan, const rf_filter_desc *desc) {
    int status = RF_OK;
    bool first_dim = true;
    int last_scan_dim = -1;
    for (int d = 0; d < plan->ndim; d++)
        if (!plan->dims[d].scan_ids.empty()) last_scan_dim = d;
    if (last_scan_dim < 0) return build_untiled<P>(plan);
    if (plan->sharded() && plan->ndim < 2) {
        set_error("sharding needs at least two dimensions");
        return RF_ERR_UNSUPPORTED;
    }

    for (int d = 0; d < plan->ndim; d++) {
        if (plan->dims[d].scan_ids.empty()) continue;
        int rc = add_generic_dimension<P, S>(plan, desc->tile[d], d, first_dim);
        if (rc != RF_OK) return rc;
        first_dim = false;
    }
    // a filter whose outermost dimension has no scans but whose data still has to reach `out`
    // is covered: the last filtered dimension's pass 2 wrote `out`.
    return status;
}

// The pointwise stages the chosen path does not fuse run as stand-alone elementwise kernels around it:
// pointwise_pre writes x' into the output planes (every later stage then filters the output planes in
// place), pointwise_post combines the filtered output with the caller's input.
template <typename P>
void add_pointwise_steps_typed(rf_plan *plan) {
    const Pointwise pw = plan->pw;
    if (pw.pre && !pw.pre_fused) {
        Step st;
        st.name = "pointwise_pre";
        st.run = [plan, pw](int pl) {
            int rc = RF_OK;
            if constexpr (std::is_same<P, float>::value) {
                if (pw.in_u8) rc = launch_pointwise_from<P, uint8_t>(nullptr, (const uint8_t *)plan->orig_in[pl], (P *)plan->out[pl],
                                                                     plan->total, 0.0, pw.pre_s, pw.pre_b, plan->stream);
            }
            if (!pw.in_u8) rc = launch_pointwise<P>((const P *)plan->orig_in[pl], (const P *)nullptr, (P *)plan->out[pl], plan->total,
                                                    pw.pre_s, 0.0, pw.pre_b, plan->stream);
            plan->in[pl] = plan->out[pl];
            return rc;
        };
        plan->begin_steps.insert(plan->begin_steps.begin(), st);
    }
    if (pw.post && !pw.post_fused) {
        Step st;
        st.name = "pointwise_post";
        // out = post_f * F + post_i * (pre_s * in + pre_b) + post_b
        const double c1 = pw.post_i * (pw.pre ? pw.pre_s : 1.0);
        const double c2 = pw.post_b + pw.post_i * (pw.pre ? pw.pre_b : 0.0);
        st.run = [plan, pw, c1, c2](int pl) {
            if constexpr (std::is_same<P, float>::value) {
                if (pw.in_u8) return launch_pointwise_from<P, uint8_t>((const P *)plan->out[pl], (const uint8_t *)plan->orig_in[pl],
                                                                       (P *)plan->out[pl], plan->total, pw.post_f, c1, c2, plan->stream);
            }
            return launch_pointwise<P>((const P *)plan->out[pl], (const P *)plan->orig_in[pl], (P *)plan->out[pl], plan->total,
                                       pw.post_f, c1, c2, plan->stream);
        };
        plan->finish_steps.push_back(st);
    }
}

void add_pointwise_steps(rf_plan *plan) {
    if (plan->dtype == RF_F32) add_pointwise_steps_typed<float>(plan);
    else if (plan->dtype == RF_F64) add_pointwise_steps_typed<double>(plan);
}

template <typename P>
int build_for_pixel(rf_plan *plan, const rf_filter_desc *desc, int path) {
    using S = typename std::conditional<PixelTraits<P>::is_integer, uint64_t, double>::type;
    if (path == RF_PATH_UNTILED) return build_untiled<P>(plan);
    return build_generic<P, S>(plan, desc);
}

// ---- in-plan cascade ---------------------------------------------------------------------------------------------
// Scans of different dimensions commute and the scans of one dimension are successive in-place passes by definition
// (lib/recfilter.cpp:302-343), so any split of the scan list that keeps every dimension's order is the same filter
// (the reference's cascade(), lib/reorder.cpp:28-229, is this split done by the caller).  Stage of every scan of `desc`:
// at most kFusedMaxScans sections per dimension and stage (a scan of order n > 3 becomes up to ceil(n/2) sections,
// sections.h), and for a 1-D signal that gets zero-padded (length not a multiple of 8192) a new stage before an
// anticausal scan that follows a causal one -- every stage copies only the signal out of its padded buffer, so the
// ringing a causal scan leaves in the padding never reaches a later stage.
std::vector<int> cascade_stage_of_scans(const rf_filter_desc *desc) {
    const bool sections_ok = desc->border == RF_BORDER_ZERO && (desc->dtype == RF_F32 || desc->dtype == RF_F64) &&
                             !(desc->flags & RF_PLAN_NO_SECTIONS);
    const bool padded_1d = desc->ndim == 1 && desc->border == RF_BORDER_ZERO && desc->extent[0] % 8192 != 0;
    std::vector<int> stage((size_t)desc->n_scans, 0);
    for (int d = 0; d < desc->ndim; d++) {
        int cur = 0, used = 0;
        bool seen_causal = false;
        for (int i = 0; i < desc->n_scans; i++) {
            const rf_scan_desc &r = desc->scans[i];
            if (r.dim != d) continue;
            if (r.order > kFusedMaxK && (!sections_ok || r.order > kFusedMaxMod)) return {};
            const int w = r.order <= kFusedMaxK ? 1 : (r.order + 1) / 2;
            if (w > kFusedMaxScans) return {};
            if (used + w > kFusedMaxScans || (padded_1d && !r.causal && seen_causal)) { cur++; used = 0; seen_causal = false; }
            stage[(size_t)i] = cur;
            used += w;
            seen_causal = seen_causal || r.causal != 0;
        }
    }
    return stage;
}

int build_cascade(const rf_filter_desc *desc, const std::vector<int> &stage_of, int n_stages, rf_plan *parent) {
    std::vector<std::unique_ptr<rf_plan>> children;
    std::vector<std::vector<const Step *>> steps((size_t)n_stages);
    for (int st = 0; st < n_stages; st++) {
        std::vector<rf_scan_desc> sub;
        for (int i = 0; i < desc->n_scans; i++)
            if (stage_of[(size_t)i] == st) sub.push_back(desc->scans[i]);
        rf_filter_desc cd = *desc;
        cd.scans = sub.data();
        cd.n_scans = (int32_t)sub.size();
        if (st > 0) { cd.pointwise.flags &= ~RF_POINTWISE_PRE; cd.pointwise.in_dtype = RF_IN_PIXEL; }    // stage > 0 reads the output planes
        if (st + 1 < n_stages) cd.pointwise.flags &= ~RF_POINTWISE_POST;
        rf_plan *child = nullptr;
        int rc = build_plan(&cd, &child);
        if (rc != RF_OK) return rc;
        children.emplace_back(child);
        // the point of the split is the fused (or, for small images, the line-parallel) kernels: a stage that would still
        // run on the per-dimension generic passes means something else keeps this filter off them
        // (an untiled stage must be the line-parallel kind: the one-thread-per-line kernel is what the split is meant to avoid)
        if (child->path == RF_PATH_TILED_GENERIC || child->path == RF_PATH_TILED_OVERLAPPED ||
            (child->path == RF_PATH_UNTILED && !child->vector_access)) {
            set_error("cascade: stage %d would not run on the fused kernels", st);
            return RF_ERR_UNSUPPORTED;
        }
        if ((rc = child_steps(child, steps[(size_t)st])) != RF_OK) return rc;
    }
    // (the last refusal is behind us: from here on the parent changes)
    // rf_plan_tiles / rf_plan_table report the first FUSED stage (stage 0 may be an untiled line-kernel stage without tiles)
    const rf_plan *shown = children[0].get();
    for (auto &c : children)
        if (c->path == RF_PATH_TILED_FUSED) { shown = c.get(); break; }
    parent->path = shown->path;
    for (int st = 0; st < n_stages; st++) {
        rf_plan *child = children[(size_t)st].get();
        parent->vector_access = parent->vector_access || child->vector_access;
        take_over_child(parent, child, child == shown);
        // stage 0 reads the input, every later stage filters the output planes in place
        append_child_steps(parent, child, steps[(size_t)st], st == 0 ? "" : "stage" + std::to_string(st) + ".", [parent, st](int q) {
            return ChildPlanes{st == 0 ? parent->orig_in[q] : (const void *)parent->out[q], parent->out[q]};
        });
    }
    parent->stages = std::move(children);
    return RF_OK;
}

// ---- clamped 1-D signals (plan_clamp1d.h) ----------------------------------------------------------------------------
// The zero-border fused plan of the same scans as a child, a launch of n dot products in front of it and the corrections of
// the two ends of the output behind it.  RF_ERR_UNSUPPORTED (the caller goes on to the other paths) when the filter does not
// decay inside a quarter of the signal or its zero-border form does not run on the fused kernels.
int build_clamped_1d(const rf_filter_desc *desc, rf_plan *parent) {
    Clamp1DTables t;
    if (!build_clamp1d_tables(parent->scans, parent->dims[0].N, t)) {
        set_error("clamped 1-D: the filter does not decay inside a quarter of the signal");
        return RF_ERR_UNSUPPORTED;
    }
    rf_filter_desc cd = *desc;
    cd.border = RF_BORDER_ZERO;
    cd.path = RF_PATH_TILED_FUSED;
    rf_plan *child = nullptr;
    int rc = build_plan(&cd, &child);
    if (rc != RF_OK) return RF_ERR_UNSUPPORTED;
    std::unique_ptr<rf_plan> holder(child);
    std::vector<const Step *> steps;
    if (child->path != RF_PATH_TILED_FUSED || child_steps(child, steps) != RF_OK) return RF_ERR_UNSUPPORTED;
    // (the last refusal is behind us: from here on the parent changes, and a failure fails the build)
    int status = RF_OK;
    const int n = t.n, L = t.L;
    const int32_t *d_side = (const int32_t *)parent->upload(t.side.data(), t.side.size() * sizeof(int32_t), &status);
    const double *d_w = (const double *)parent->upload(t.w.data(), t.w.size() * sizeof(double), &status);
    const double *d_G = (const double *)parent->upload(t.G.data(), t.G.size() * sizeof(double), &status);
    const double *d_H = (const double *)parent->upload(t.H.data(), t.H.size() * sizeof(double), &status);
    double *d_dots = (double *)parent->alloc((size_t)n * parent->n_planes * sizeof(double), true, &status);
    if (status != RF_OK) return status;
    const int64_t N = parent->dims[0].N;
    Step dots;
    dots.name = "clamp1d_dots";
    dots.run = [parent, N, L, n, d_side, d_w, d_dots](int pl) {
        return launch_clamp1d_dots<float>((const float *)parent->orig_in[pl], N, L, n, d_side, d_w, d_dots + (size_t)pl * n, parent->stream);
    };
    parent->begin_steps.push_back(dots);
    append_child_steps(parent, child, steps, "", [parent](int q) { return ChildPlanes{parent->orig_in[q], parent->out[q]}; });
    Step fix;
    fix.name = "clamp1d_fix";
    fix.run = [parent, N, L, n, d_side, d_H, d_G, d_dots](int pl) {
        return launch_clamp1d_fix<float>((float *)parent->out[pl], N, L, n, d_side, d_H, d_G, d_dots + (size_t)pl * n, parent->stream);
    };
    parent->begin_steps.push_back(fix);
    parent->path = RF_PATH_TILED_FUSED;
    parent->vector_access = true;
    take_over_child(parent, child, true);
    parent->tables["clamp1d_w"] = t.w;
    parent->tables["clamp1d_G"] = t.G;
    parent->tables["clamp1d_H"] = t.H;
    parent->tables["clamp1d_L"] = {(double)L};
    parent->stages.push_back(std::move(holder));
    return RF_OK;
}

// ---- staged 16-bit plans ---------------------------------------------------------------------------------------------------
// RF_F16 / RF_BF16 are storage types: out = round16(F_f32(widen(in))), no intermediate is ever rounded (pixel.h).  The fused
// x/y kernels keep that contract by themselves (2-D images, 1-D signals: plan_fused.cpp).  Every other structure keeps an
// intermediate in the output planes -- the x stage in front of the y stage of the line-parallel, generic, overlapped and
// matrix paths, the x/y stage in front of a volume's z stage, the earlier stages of a cascade -- so such a plan owns one f32
// plane per image plane and runs
//     convert_in -> the f32 plan of the same description, in place in those planes -> convert_out
// (an epilogue with an input operand needs out != in: a second f32 plane per image plane).  The steps carry those two
// names, rf_plan_path reports the inner plan's path, rf_plan_workspace_bytes includes the planes.
// Volumes whose z stage runs on the strided kernels are native as well (plan_fused.cpp, "native 16-bit volumes"): the x/y
// stage's result waits in an f32 volume of the plan's own.  RF_PATH_TILED_FUSED asks for that form at any size; RF_PATH_AUTO
// takes it from kHalfVolumeNativeSamples samples per plane on and stays staged below.
// Measured, one MI355X, order-2 Gaussian along x, y and z, native / staged step (profiles/r9/half_volumes.txt): 64 x 96 x 128
// 1.73 and 128^3 (2^21) 1.27 -- there the staged form's f32 plan is three launches of the line kernels, 29 / 43 us a step against
// the native plan's seven launches, 51 / 55 us; 128 x 256 x 256 (2^23) 0.69, 256^3 0.71, 512^3 0.60, 2^28 0.54, 1024^3 0.52.
// 2^23 is the smallest size measured with the native form ahead; nothing between 2^21 and 2^23 has been measured.
constexpr int64_t kHalfVolumeNativeSamples = (int64_t)1 << 23;

// The threshold of native byte volumes (RF_IO_U8; u8_plan_is_native below) under RF_PATH_AUTO: the smallest measured size at which
// the native step is ahead of the staged one by more than the staged plan's spread against a copy of itself.
// Measured, one MI355X, order-2 Gaussian along x, y and z with the round trip in / 255, 255 F, native / staged step, two runs
// (profiles/r14/u8_volume_probe.txt): 128^3 (2^21) 0.81 / 0.83 (56 against 69 us; spread 0.1 us), 128 x 256 x 256 (2^23) 0.60 / 0.59,
// 256^3 0.60 / 0.60, 512^3 0.47 / 0.46, 1024^3 0.44 / 0.44 (3.54 against 8.08 ms; spread 0.3 ms).  The byte model says 15 / 23 = 0.65.
// Unlike the 16-bit volumes the staged form runs the same seven launches plus two, so the native form is ahead at 2^21 already;
// nothing below 2^21 has been measured.
constexpr int64_t kByteVolumeNativeSamples = (int64_t)1 << 21;

template <typename H>
int build_staged_half_typed(const rf_filter_desc *desc, rf_plan *parent) {
    rf_filter_desc fd = *desc;
    fd.dtype = RF_F32;
    rf_plan *child = nullptr;
    int rc = build_plan(&fd, &child);
    if (rc != RF_OK) return rc;
    std::unique_ptr<rf_plan> holder(child);
    std::vector<const Step *> steps;
    if ((rc = child_steps(child, steps)) != RF_OK) return rc;
    int status = RF_OK;
    const bool two = parent->pw.post && parent->pw.post_i != 0.0;
    const size_t plane_bytes = (size_t)parent->total * sizeof(float);
    std::vector<float *> pa((size_t)parent->n_planes, nullptr), pb((size_t)parent->n_planes, nullptr);
    for (int pl = 0; pl < parent->n_planes; pl++) {
        pa[(size_t)pl] = (float *)parent->alloc(plane_bytes, false, &status);
        pb[(size_t)pl] = two ? (float *)parent->alloc(plane_bytes, false, &status) : pa[(size_t)pl];
    }
    if (status != RF_OK) return status;
    const int64_t total = parent->total;
    Step ci;
    ci.name = "convert_in";
    ci.run = [parent, pa, total](int pl) {
        return launch_convert<float, H>((const H *)parent->orig_in[pl], pa[(size_t)pl], total, parent->stream);
    };
    parent->begin_steps.push_back(ci);
    append_child_steps(parent, child, steps, "", [pa, pb](int q) { return ChildPlanes{pa[(size_t)q], pb[(size_t)q]}; });
    Step co;
    co.name = "convert_out";
    co.run = [parent, pb, total](int pl) {
        return launch_convert<H, float>(pb[(size_t)pl], (H *)parent->out[pl], total, parent->stream);
    };
    parent->begin_steps.push_back(co);
    parent->path = child->path;
    parent->vector_access = false;           // (the conversions take any element-aligned plane)
    take_over_child(parent, child, true);
    parent->stages.push_back(std::move(holder));
    return RF_OK;
}

// (a staged plan is the whole plan: `parent` is a description nothing has been built on)
int build_staged_half(const rf_filter_desc *desc, rf_plan *parent) {
    if (parent->sharded()) {
        set_error("16-bit float pixels: only row-sharded 2-D images on the fused path can be sharded");
        return RF_ERR_UNSUPPORTED;
    }
    return desc->dtype == RF_F16 ? build_staged_half_typed<_Float16>(desc, parent) : build_staged_half_typed<__bf16>(desc, parent);
}

// ---- staged byte-output plans ---------------------------------------------------------------------------------------------
// RF_IO_U8 (pixel.h, sat8): out = sat8(F_f32(widen(in))), no intermediate ever passes through a byte plane.  The final pass of the
// fused x/y kernels keeps that contract for 2-D images (plan_fused.cpp, add_pass2), the final z pass for the volumes
// u8_plan_is_native admits (add_z_stage, "native byte volumes").  Every other plan owns one f32 plane per
// image plane and runs
//     the RF_IN_U8 f32 plan of the same description, from the caller's bytes into those planes -> convert_out
// (no convert_in: that plan reads the bytes itself; its epilogue's input operand is the caller's plane, never its output).
// Same wrapper as the staged 16-bit plans above.
int build_staged_u8(const rf_filter_desc *desc, rf_plan *parent) {
    rf_filter_desc fd = *desc;
    fd.pointwise.in_dtype = RF_IN_U8;
    rf_plan *child = nullptr;
    int rc = build_plan(&fd, &child);
    if (rc != RF_OK) return rc;
    std::unique_ptr<rf_plan> holder(child);
    std::vector<const Step *> steps;
    if ((rc = child_steps(child, steps)) != RF_OK) return rc;
    // (the launch list is the RF_IN_U8 plan's, name for name: the apply steps the generic path keeps for an unsharded outermost
    // dimension run here as rf_plan_execute runs them for that plan)
    steps = single_device_steps(child, true);
    int status = RF_OK;
    std::vector<float *> pa((size_t)parent->n_planes, nullptr);
    for (int pl = 0; pl < parent->n_planes; pl++) pa[(size_t)pl] = (float *)parent->alloc((size_t)parent->total * sizeof(float), false, &status);
    if (status != RF_OK) return status;
    const int64_t total = parent->total;
    append_child_steps(parent, child, steps, "", [parent, pa](int q) { return ChildPlanes{parent->orig_in[q], pa[(size_t)q]}; });
    Step co;
    co.name = "convert_out";
    co.run = [parent, pa, total](int pl) { return launch_convert_sat8(pa[(size_t)pl], (uint8_t *)parent->out[pl], total, parent->stream); };
    parent->begin_steps.push_back(co);
    parent->path = child->path;
    parent->vector_access = false;           // (rf_plan_execute checks the 4-byte alignment of byte planes by itself)
    take_over_child(parent, child, true);
    parent->stages.push_back(std::move(holder));
    return RF_OK;
}

// what a replica of this plan is built from (concurrent executions, capi.cpp)
void save_desc(rf_plan *plan, const rf_filter_desc *desc) {
    plan->saved.d = *desc;
    plan->saved.scans.assign(desc->scans, desc->scans + desc->n_scans);
    plan->saved.d.scans = nullptr;           // (re-pointed at the copies when a replica is built)
    plan->saved.extents.clear();
    if (desc->shard_extents != nullptr && desc->shard_world > 1)
        plan->saved.extents.assign(desc->shard_extents, desc->shard_extents + desc->shard_world);
    plan->saved.d.shard_extents = nullptr;
}

// A new plan with the description part of `plan` and nothing a builder added (no tiles, steps, tables or buffers): what a
// second builder starts from when the first one refused the shape.
std::unique_ptr<rf_plan> fresh_description(const rf_plan &plan) {
    std::unique_ptr<rf_plan> fresh(new rf_plan);
    fresh->ndim = plan.ndim; fresh->dtype = plan.dtype; fresh->n_planes = plan.n_planes;
    fresh->clamped = plan.clamped; fresh->device = plan.device; fresh->host_only = plan.host_only;
    fresh->shard_rank = plan.shard_rank; fresh->shard_world = plan.shard_world; fresh->flags = plan.flags;
    fresh->shard_extents = plan.shard_extents; fresh->shard_common = plan.shard_common;
    fresh->scans = plan.scans; fresh->total = plan.total; fresh->pw = plan.pw;
    for (int d = 0; d < RF_MAX_DIMS; d++) { fresh->dims[d] = plan.dims[d]; fresh->dims[d].T = 0; fresh->dims[d].M = 0; }
    return fresh;
}

// ---- the stages of build_plan, in the order it runs them (the head of this file) ----------------------------------------------
// A stage that may produce the whole plan returns kNextStage where it does not: the next stage then runs.
constexpr int kNextStage = -1;

bool is_half(int dtype) { return dtype == RF_F16 || dtype == RF_BF16; }      // storage types with f32 arithmetic (pixel.h)
bool auto_or_fused(const rf_filter_desc *desc) { return desc->path == RF_PATH_AUTO || desc->path == RF_PATH_TILED_FUSED; }

// a scan as the plan keeps it: the coefficients cast through the pixel type
Scan to_scan(const rf_scan_desc &r, int dtype) {
    Scan s;
    s.dim = r.dim;
    s.causal = r.causal != 0;
    s.order = r.order;
    s.b = cast_coeff(r.feedfwd, dtype);
    for (int j = 0; j < r.order; j++) s.a[j] = cast_coeff(r.feedback[j], dtype);
    return s;
}

int validate_desc(const rf_filter_desc *desc) {
    if (desc->abi != RF_ABI) {
        set_error("rf_filter_desc.abi is %u, this library speaks revision %u of include/recfilter_amd.h (set .abi = RF_ABI; a caller built "
                  "against another revision of the header must be rebuilt)", desc->abi, (unsigned)RF_ABI);
        return RF_ERR_INVALID_ARG;
    }
    if (desc->ndim < 1 || desc->ndim > RF_MAX_DIMS) { set_error("ndim must be 1..%d", RF_MAX_DIMS); return RF_ERR_INVALID_ARG; }
    if (desc->n_planes < 1 || desc->n_planes > RF_MAX_PLANES) { set_error("n_planes must be 1..%d", RF_MAX_PLANES); return RF_ERR_INVALID_ARG; }
    if (desc->dtype < RF_F32 || desc->dtype > RF_BF16) { set_error("unknown dtype %d", desc->dtype); return RF_ERR_INVALID_ARG; }
    if (desc->n_scans < 0 || desc->n_scans > RF_MAX_SCANS || (desc->n_scans > 0 && !desc->scans)) {
        set_error("n_scans must be 0..%d", RF_MAX_SCANS);
        return RF_ERR_INVALID_ARG;
    }
    if (desc->border != RF_BORDER_ZERO && desc->border != RF_BORDER_CLAMP) { set_error("unknown border mode"); return RF_ERR_INVALID_ARG; }
    for (int d = 0; d < desc->ndim; d++) {
        if (desc->extent[d] < 1) { set_error("extent[%d] must be positive", d); return RF_ERR_INVALID_ARG; }
        if (desc->tile[d] < 0) { set_error("tile[%d] must be >= 0", d); return RF_ERR_INVALID_ARG; }
        if (desc->tile[d] > 0 && desc->extent[d] % desc->tile[d] != 0) {
            // lib/recfilter.h:311: tile width must divide the image width
            set_error("tile %d does not divide extent %lld of dimension %d", desc->tile[d], (long long)desc->extent[d], d);
            return RF_ERR_INVALID_ARG;
        }
    }
    for (int i = 0; i < desc->n_scans; i++) {
        const rf_scan_desc &s = desc->scans[i];
        if (s.dim < 0 || s.dim >= desc->ndim) {   // lib/recfilter.cpp:296-300
            set_error("scan %d: dimension %d is not one of the filter's %d dimensions", i, s.dim, desc->ndim);
            return RF_ERR_INVALID_ARG;
        }
        if (s.order < 1 || s.order > RF_MAX_ORDER) {   // lib/recfilter.cpp:274-278
            set_error("scan %d: needs a feedforward and 1..%d feedback coefficients", i, RF_MAX_ORDER);
            return RF_ERR_INVALID_ARG;
        }
    }
    const rf_pointwise_desc &pwd = desc->pointwise;
    if (pwd.flags & ~(RF_POINTWISE_PRE | RF_POINTWISE_POST)) { set_error("unknown pointwise flags 0x%x", pwd.flags); return RF_ERR_INVALID_ARG; }
    if (pwd.in_dtype < RF_IN_PIXEL || pwd.in_dtype > RF_IO_U8) { set_error("unknown pointwise input type %d", pwd.in_dtype); return RF_ERR_INVALID_ARG; }
    if (pwd.in_dtype != RF_IN_PIXEL && desc->dtype != RF_F32) { set_error("unsigned-byte planes need f32 pixels"); return RF_ERR_UNSUPPORTED; }
    if (pwd.in_dtype == RF_IO_U8 && (desc->shard_world > 1 || (desc->flags & RF_PLAN_FORCE_EXCHANGE))) {
        set_error("unsigned-byte output planes cannot be sharded");
        return RF_ERR_UNSUPPORTED;
    }
    if (pwd.flags != 0 && desc->dtype != RF_F32 && desc->dtype != RF_F64 && !is_half(desc->dtype)) {
        set_error("pointwise stages need a floating-point pixel type");
        return RF_ERR_UNSUPPORTED;
    }
    if (desc->flags & ~(RF_PLAN_ALL_FLAGS | 0x00ffff00u)) { set_error("unknown plan flags 0x%x", desc->flags); return RF_ERR_INVALID_ARG; }
    for (int v : {(int)((desc->flags >> 8) & 0xffu), (int)((desc->flags >> 16) & 0xffu)})
        if (v != 0 && v != 32 && v != 64 && v != 128) { set_error("RF_PLAN_TILE_ROWS / RF_PLAN_TILE_PLANES take 32, 64 or 128"); return RF_ERR_INVALID_ARG; }
    if ((desc->flags & RF_PLAN_STREAM_PASS1) && (desc->flags & RF_PLAN_STAGED_PASS1)) { set_error("RF_PLAN_STREAM_PASS1 and RF_PLAN_STAGED_PASS1 exclude each other"); return RF_ERR_INVALID_ARG; }
    if (desc->shard_rank < 0 || desc->shard_rank >= std::max<int>(1, desc->shard_world)) { set_error("shard_rank out of range"); return RF_ERR_INVALID_ARG; }
    return RF_OK;
}

// ---- merged runs (1-D signals) -------------------------------------------------------------------------------------
// Consecutive scans of one direction with a zero border are ONE scan whose transfer function is the product of theirs --
// the reference's overlap_to_higher_order_filter (lib/reorder.cpp:231-381), which a caller applies by hand.  On a 1-D
// signal the fused kernels take four scans per stage (~50 us + 18 us per scan at 10,000,000 samples) while the matrix
// path takes a scan of ANY order up to 32 in four launches (~68 us): fifteen biquads (apps/audio/audio_filter_biquads.cpp)
// are four fused stages or one scan of order 30.  Done where it leaves fewer stages AND a probe finds the merged direct form,
// evaluated in f32, within 2e-5 of the cascade (sections.h); the plan then IS the plan of the merged scan list.
// Returns true where *out is that plan.
bool plan_merged_runs(const rf_filter_desc *desc, rf_plan **out) {
    if (!(desc->path == RF_PATH_AUTO && desc->ndim == 1 && desc->border == RF_BORDER_ZERO && desc->dtype == RF_F32 && desc->shard_world <= 1 &&
          !(desc->flags & (RF_PLAN_FORCE_EXCHANGE | RF_PLAN_NO_OVERLAP)) && desc->n_scans >= 2 && desc->extent[0] >= 8192 && desc->extent[0] % 4 == 0))
        return false;
    std::vector<rf_scan_desc> merged;
    bool ok = true, any = false;
    for (int i = 0; i < desc->n_scans && ok; ) {
        int j = i, order = 0;
        std::vector<Scan> run;
        while (j < desc->n_scans && (desc->scans[j].causal != 0) == (desc->scans[i].causal != 0) && order + desc->scans[j].order <= RF_MAX_ORDER) {
            order += desc->scans[j].order;
            run.push_back(to_scan(desc->scans[j], RF_F32));
            j++;
        }
        if (run.size() == 1) { merged.push_back(desc->scans[i]); i = j; continue; }
        std::vector<double> fb(run[0].a, run[0].a + run[0].order);
        double b = run[0].b;
        for (size_t q = 1; q < run.size(); q++) {
            fb = multiply_feedback(fb, std::vector<double>(run[q].a, run[q].a + run[q].order));
            b *= run[q].b;
        }
        rf_scan_desc m{};
        m.dim = 0; m.causal = desc->scans[i].causal; m.order = (int32_t)fb.size(); m.feedfwd = (float)b;
        for (size_t e = 0; e < fb.size(); e++) m.feedback[e] = (float)fb[e];
        ok = merged_well_conditioned(run, to_scan(m, RF_F32));
        merged.push_back(m);
        any = true;
        i = j;
    }
    // what each form costs, in the units above: a fused stage holds four scans (and a causal scan behind an anticausal one of a
    // padded signal starts a new stage, cascade_stage_of_scans); the matrix path runs every scan of order above 3 by itself
    const int fused_stages = (desc->n_scans + kFusedMaxScans - 1) / kFusedMaxScans;
    const double fused_cost = 50.0 * fused_stages + 18.0 * desc->n_scans, matrix_cost = 68.0 * (double)merged.size();
    if (!(ok && any && matrix_cost < fused_cost)) return false;
    rf_filter_desc md = *desc;
    md.scans = merged.data();
    md.n_scans = (int32_t)merged.size();
    md.flags |= RF_PLAN_NO_OVERLAP;
    // The merge is kept only if every merged run of order above 3 really runs in its DIRECT form, one matrix stage each
    // (ADVICE r5): a plan that sends the merged scans elsewhere -- back into sections of the f32-rounded product: a second
    // rounding of the poles -- is dropped and the scans are planned as given.
    rf_plan *mp = nullptr;
    const int rc = build_plan(&md, &mp);
    int max_order = 0;
    for (const rf_scan_desc &m : merged) max_order = std::max(max_order, (int)m.order);
    if (rc == RF_OK && mp != nullptr && (mp->path == RF_PATH_TILED_MATRIX || max_order <= kFusedMaxK)) { *out = mp; return true; }
    delete mp;
    *out = nullptr;
    return false;
}

// The description part of the plan: device, shard extents, dimensions, the scans grouped by dimension.
int describe(const rf_filter_desc *desc, rf_plan *plan) {
    const bool host_only = desc->device == RF_DEVICE_HOST_ONLY;
    const int world = std::max<int>(1, desc->shard_world);
    const rf_pointwise_desc &pwd = desc->pointwise;
    int device = desc->device;
    if (!host_only) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
            set_error("no HIP device available (this library has no CPU fallback)");
            return RF_ERR_HIP;
        }
        if (device < 0) RF_HIP_CHECK(hipGetDevice(&device));
        if (device >= ndev) { set_error("device %d out of range (%d visible)", device, ndev); return RF_ERR_INVALID_ARG; }
        RF_HIP_CHECK(hipSetDevice(device));
    }
    plan->host_only = host_only;
    plan->ndim = desc->ndim;
    plan->dtype = desc->dtype;
    plan->n_planes = desc->n_planes;
    plan->clamped = desc->border == RF_BORDER_CLAMP;
    plan->device = device;
    plan->shard_rank = desc->shard_rank;
    plan->shard_world = world;
    plan->flags = desc->flags;
    plan->pw.pre = (pwd.flags & RF_POINTWISE_PRE) != 0;
    plan->pw.post = (pwd.flags & RF_POINTWISE_POST) != 0;
    plan->pw.in_u8 = pwd.in_dtype == RF_IN_U8 || pwd.in_dtype == RF_IO_U8;
    plan->pw.out_u8 = pwd.in_dtype == RF_IO_U8;
    if (plan->pw.pre) { plan->pw.pre_s = pwd.pre_scale; plan->pw.pre_b = pwd.pre_bias; }
    if (plan->pw.in_u8) plan->pw.pre = true;        // the conversion is a prologue (scale 1, bias 0 unless given)
    if (plan->pw.post) { plan->pw.post_f = pwd.post_filtered; plan->pw.post_i = pwd.post_input; plan->pw.post_b = pwd.post_bias; }
    const int64_t own = desc->extent[desc->ndim - 1];
    plan->shard_extents.assign((size_t)world, own);
    if (desc->shard_extents != nullptr && world > 1) {
        for (int h = 0; h < world; h++) {
            if (desc->shard_extents[h] < 1) { set_error("shard_extents[%d] must be positive", h); return RF_ERR_INVALID_ARG; }
            plan->shard_extents[(size_t)h] = desc->shard_extents[h];
        }
        if (desc->shard_extents[desc->shard_rank] != own) {
            set_error("shard_extents[%d] = %lld is not this rank's extent %lld", desc->shard_rank,
                      (long long)desc->shard_extents[desc->shard_rank], (long long)own);
            return RF_ERR_INVALID_ARG;
        }
    }
    int64_t g = 0;
    for (int64_t e : plan->shard_extents) { int64_t a = e, b = g; while (b) { int64_t t = a % b; a = b; b = t; } g = a; }
    plan->shard_common = g;
    plan->total = 1;
    for (int d = 0; d < desc->ndim; d++) {
        plan->dims[d].N = desc->extent[d];
        plan->dims[d].stride = plan->total;
        plan->total *= desc->extent[d];
    }
    for (int d = 0; d < desc->ndim; d++) plan->dims[d].lines = plan->total / plan->dims[d].N;

    // group scans by dimension, stable (lib/split.cpp:215-242); coefficients travel with their scan
    for (int d = 0; d < desc->ndim; d++) {
        for (int i = 0; i < desc->n_scans; i++) {
            const rf_scan_desc &r = desc->scans[i];
            if (r.dim != d) continue;
            plan->dims[d].k = std::max(plan->dims[d].k, r.order);
            plan->dims[d].scan_ids.push_back((int)plan->scans.size());
            plan->scans.push_back(to_scan(r, desc->dtype));
        }
    }
    return RF_OK;
}

// 16-bit float pixels: native where the fused kernels take the filter in one piece (no intermediate then reaches a plane),
// staged through f32 planes everywhere else ("staged 16-bit plans" above).  A native plan goes on below; the rewrites and
// the cascade that follow apply to f32 / f64 plans or to filters the fused kernels refuse, i.e. not to it.
bool half_plan_is_native(const rf_filter_desc *desc, const rf_plan *plan) {
    std::string unused;
    // (volumes, RF_PATH_AUTO: native from kHalfVolumeNativeSamples samples per plane on -- above)
    const bool small_volume = desc->ndim > 2 && desc->path == RF_PATH_AUTO && plan->total < kHalfVolumeNativeSamples;
    return auto_or_fused(desc) && !(desc->flags & RF_PLAN_STAGE_HALF) && !small_volume && fused_plan_applicable(plan, desc, &unused);
}

// Byte planes on both sides: native where the fused kernels take the 2-D image as it is -- orders <= 3 (asked BEFORE the rewrite
// into sections: no byte instance carries border modifications), a width that is a multiple of 4 -- staged everywhere else
// ("staged byte-output plans" above).  RF_PLAN_STAGE_HALF forces the staged form.
// A volume is native where its x/y result can wait in an f32 volume of the plan's own in front of the strided z kernels, whose final
// pass then stores the bytes (plan_fused.cpp, "native byte volumes"): scans along z and along x and/or y, a depth the strided kernels
// tile, no epilogue with an input operand, none of RF_PLAN_INPLACE_Z / RF_PLAN_WALK_PASS1.  RF_PATH_TILED_FUSED asks for that form
// at any size, RF_PATH_AUTO takes it from kByteVolumeNativeSamples samples per plane on.
bool u8_plan_is_native(const rf_filter_desc *desc, const rf_plan *plan) {
    std::string unused;
    if (!auto_or_fused(desc) || (desc->flags & RF_PLAN_STAGE_HALF) || !fused_plan_applicable(plan, desc, &unused)) return false;
    if (desc->ndim == 2) return true;
    return byte_volume_form(plan) && (desc->path == RF_PATH_TILED_FUSED || plan->total >= kByteVolumeNativeSamples);
}

// Orders above 3 (lib/split.cpp:575-578 pads any order; the fused kernels stop at 3): with a zero border and float
// pixels a scan of order 4..RF_MAX_ORDER is the same filter as its first/second/third-order sections applied one after
// the other (sections.h), and those the fused kernels take -- as long as no dimension ends up with more than four scans.
// With a CLAMPED border (2-D / 3-D, f32) the same rewrite works on scans in "mod form": a clamped scan IS the zero-border
// scan of an input whose first k samples in scan direction are x_r + g_r x_0 (tables.h, scan_tile) --
//     y_r = b x_r + sum_{j<r} a_j y_{r-1-j} + (sum_{j>=r} a_j) c_r,   c_0 = x_0,  c_r = y_0 = (b + sum a) x_0
// (lib/recfilter.cpp:330-336), so  g_0 = (sum_j a_j) / b,  g_r = (sum_{j>=r} a_j)(b + sum a) / b -- and the zero-border
// scan factors into sections exactly.  The first section of every scan carries the modification of the ORIGINAL scan;
// every scan of the plan (the low-order ones too) is put into that form, and the kernels that run recurrences apply the
// modification on the tile where the scan enters the image (scan_device.h, border_mod_*).
// The rewrite is kept only if it makes the fused path applicable; every other path runs the scans as given.
void rewrite_into_sections(const rf_filter_desc *desc, rf_plan *plan) {
    if (!auto_or_fused(desc) || (plan->dtype != RF_F32 && plan->dtype != RF_F64) || (desc->flags & RF_PLAN_NO_SECTIONS)) return;
    // (orders above kFusedMaxMod = 8 are never sectioned: the direct form on the matrix path is well conditioned
    // where a long cascade of f32 resonators is not, and a border modification touches at most eight samples)
    bool high = false, too_high = false;
    for (const Scan &sc : plan->scans) { high = high || sc.order > kFusedMaxK; too_high = too_high || sc.order > kFusedMaxMod; }
    if (too_high) high = false;
    // ONE scan of a 1-D signal (apps/audio/audio_filter_high_order.cpp): its direct form on the matrix path is four
    // launches whatever the order (10,000,000 samples: 0.065 ms at orders 4..16), its two or three sections on the fused
    // kernels take 0.086-0.115 ms (profiles/r5/matrix_audio_sweep.txt)
    if (high && desc->path == RF_PATH_AUTO && desc->ndim == 1 && desc->n_scans == 1 && matrix_plan_applicable(plan, desc, nullptr)) high = false;
    const bool mod = plan->clamped;
    if (mod && (plan->dtype != RF_F32 || desc->ndim < 2 || plan->sharded())) high = false;
    if (!high) return;
    std::vector<Scan> rewritten;
    bool ok = true;
    const int dtype = plan->dtype;
    for (const Scan &sc : plan->scans) {
        std::vector<Scan> sec;
        if (sc.order <= kFusedMaxK) sec.push_back(sc);
        else ok = ok && split_into_sections(sc, kFusedMaxK, [dtype](double v) { return cast_coeff(v, dtype); }, sec) &&
                  (dtype != RF_F32 || sections_well_conditioned(sc, sec));
        if (!ok) break;
        if (mod) {
            // the modification of the scan as given, carried by its first section
            if (sc.b == 0.0) { ok = false; break; }
            double suffix[RF_MAX_ORDER + 1] = {0};
            for (int j = sc.order - 1; j >= 0; j--) suffix[j] = suffix[j + 1] + sc.a[j];
            const double total = sc.b + suffix[0];
            for (size_t i = 0; i < sec.size(); i++) {
                sec[i].mod_n = i == 0 ? sc.order : 0;
                for (int r = 0; r < RF_MAX_ORDER; r++)
                    sec[i].mod_g[r] = (i == 0 && r < sc.order) ? (r == 0 ? suffix[0] / sc.b : suffix[r] * total / sc.b) : 0.0;
            }
        }
        rewritten.insert(rewritten.end(), sec.begin(), sec.end());
    }
    if (!ok) return;
    std::vector<Scan> original = plan->scans;
    DimInfo saved[RF_MAX_DIMS];
    for (int d = 0; d < RF_MAX_DIMS; d++) saved[d] = plan->dims[d];
    plan->scans = rewritten;
    plan->mod_form = mod;
    for (int d = 0; d < desc->ndim; d++) { plan->dims[d].scan_ids.clear(); plan->dims[d].k = 0; }
    for (size_t i = 0; i < plan->scans.size(); i++) {
        DimInfo &di = plan->dims[plan->scans[i].dim];
        di.scan_ids.push_back((int)i);
        di.k = std::max(di.k, plan->scans[i].order);
    }
    std::string unused;
    if (!fused_plan_applicable(plan, desc, &unused)) {
        plan->scans = original;
        plan->mod_form = false;
        for (int d = 0; d < RF_MAX_DIMS; d++) plan->dims[d] = saved[d];
    }
}

// A clamped 1-D signal: the zero-border fused plan plus the border corrections (plan_clamp1d.h).
int try_clamped_1d(const rf_filter_desc *desc, rf_plan *plan) {
    if (!(auto_or_fused(desc) && desc->ndim == 1 && plan->clamped && plan->dtype == RF_F32 &&
          !plan->sharded() && !plan->pw.pre && !plan->pw.post && !plan->pw.in_u8 && desc->n_scans >= 1 &&
          // (one scan of order above 3: the matrix path, as for the zero border above)
          !(desc->path == RF_PATH_AUTO && desc->n_scans == 1 && plan->scans[0].order > kFusedMaxK && matrix_plan_applicable(plan, desc, nullptr))))
        return kNextStage;
    const int rc = build_clamped_1d(desc, plan);
    return rc == RF_ERR_UNSUPPORTED ? kNextStage : rc;         // (refused: nothing of the plan has been touched)
}

// What the fused kernels cannot take in one piece because of the NUMBER or the ORDER of its scans runs as a cascade of
// plans inside this one (build_cascade above) -- not on the generic path, whose carry scans are one thread per line
// (five biquads over 10,000,000 samples: 59.6 ms there, 0.26 ms as two stages).
int try_cascade(const rf_filter_desc *desc, rf_plan *plan, bool fused_ok) {
    if (fused_ok || !auto_or_fused(desc) || plan->sharded() || desc->n_scans <= 1 || (plan->pw.post && plan->pw.post_i != 0.0) ||
        (desc->flags & RF_PLAN_NO_CASCADE))
        return kNextStage;
    const std::vector<int> stage_of = cascade_stage_of_scans(desc);
    int n_stages = 0;
    for (int st : stage_of) n_stages = std::max(n_stages, st + 1);
    if (n_stages < 2) return kNextStage;        // (one stage, or a scan no stage takes)
    const int rc = build_cascade(desc, stage_of, n_stages, plan);
    // (refused under RF_PATH_AUTO: nothing of the plan has been touched, the paths below run the scans as given)
    return rc == RF_OK || desc->path == RF_PATH_TILED_FUSED ? rc : kNextStage;
}

// The path of RF_PATH_AUTO.
int choose_auto_path(const rf_filter_desc *desc, const rf_plan *plan, bool fused_ok) {
    std::string why;
    int filtered_dims = 0;
    for (int d = 0; d < desc->ndim; d++) filtered_dims += plan->dims[d].scan_ids.empty() ? 0 : 1;
    // small images are launch-bound on the five-kernel tiled pipeline (30-35 us, most of it host enqueue time): the
    // line-parallel untiled kernels need one launch per filtered dimension (kernels_lines.hip)
    int64_t max_extent = 0;
    for (int d = 0; d < desc->ndim; d++) max_extent = std::max<int64_t>(max_extent, plan->dims[d].N);
    // (RF_PLAN_TILED_ONLY: the automatic path never picks the line kernels; the limit itself is a developer knob)
    const int64_t small_limit = (desc->flags & RF_PLAN_TILED_ONLY) ? 0 : RF_KNOB("RF_SMALL_LIMIT") ? atoll(RF_KNOB("RF_SMALL_LIMIT")) : 1024;
    // ... up to 1984 for order-3 filters with four or more scans, whose tiled launches are the heaviest (C++ caller,
    // gaussian_3xy: 1152^2 47 -> 33 us, 1536^2 49 -> 45 us, 1920^2 56 -> 51 us, even at 2048^2; order 1 and 2 cross over
    // at 1024..1152)
    int max_order = 0;
    for (const Scan &sc : plan->scans) max_order = std::max(max_order, sc.order);
    const int64_t long_limit = (small_limit == 1024 && max_order >= 3 && plan->scans.size() >= 4) ? 1984 : small_limit;
    bool user_tiles = false;
    for (int d = 0; d < desc->ndim; d++) user_tiles = user_tiles || desc->tile[d] > 0;
    // (where the fused kernels apply, split() widths are hints -- the tile size never changes the result -- so a small
    // split() filter takes the line kernels too: the reference's own sweep, scripts/profile_app.sh, tiles at 32)
    // (scans in mod form -- clamped sections, above -- exist for the fused kernels only)
    if (fused_ok && !plan->mod_form && !plan->sharded() && max_extent <= long_limit && plan->total * plan->n_planes <= long_limit * long_limit * 4 &&
        plan->pw.pre == false && plan->pw.post == false && !is_half(plan->dtype) && line_scans_applicable(plan))
        return RF_PATH_UNTILED;     // (16-bit float pixels: a native plan stays on the fused kernels, which round once)
    if (fused_ok) return RF_PATH_TILED_FUSED;
    // a filter split() along two or more dimensions with small tiles: the fully overlapped tiling (two passes over
    // the image instead of two per dimension)
    if (filtered_dims >= 2 && overlap_plan_applicable(plan, desc, &why)) return RF_PATH_TILED_OVERLAPPED;
    // orders above 3 that did not become sections (orders above 8; cascades of f32 resonators the conditioning probe of
    // sections.h rejected; borders and shapes the section rewrite does not take): the direct form on the matrix cores
    if (max_order > kFusedMaxK && matrix_plan_applicable(plan, desc, &why)) return RF_PATH_TILED_MATRIX;
    // what the fused kernels do not take (f64 pixels): the line-parallel untiled kernels beat the per-dimension tiled
    // passes of the generic path at every size measured (profiles/r2/paths_4096.txt), unless the user tiled the filter
    if (!user_tiles && !plan->sharded() && small_limit > 0 && line_scans_applicable(plan)) return RF_PATH_UNTILED;
    return RF_PATH_TILED_GENERIC;
}

// What a path needs of the plan, the caller's choice or the automatic one (`fused_why`: why fused_plan_applicable said no).
int check_path(const rf_filter_desc *desc, const rf_plan *plan, int path, bool fused_ok, const std::string &fused_why) {
    std::string why;
    if (path == RF_PATH_TILED_OVERLAPPED && !overlap_plan_applicable(plan, desc, &why)) {
        set_error("overlapped tiled path not applicable: %s", why.c_str());
        return RF_ERR_UNSUPPORTED;
    }
    if (path == RF_PATH_TILED_MATRIX && !matrix_plan_applicable(plan, desc, &why)) {
        set_error("matrix path not applicable: %s", why.c_str());
        return RF_ERR_UNSUPPORTED;
    }
    if (path < RF_PATH_UNTILED || path > RF_PATH_TILED_MATRIX) { set_error("unknown path %d", path); return RF_ERR_INVALID_ARG; }
    if (path == RF_PATH_TILED_FUSED && !fused_ok) {
        set_error("fused tiled path not applicable: %s", fused_why.c_str());
        return RF_ERR_UNSUPPORTED;
    }
    return RF_OK;
}

int build_on_path(rf_plan *plan, const rf_filter_desc *desc, int p) {
    plan->path = p;
    if (p == RF_PATH_TILED_FUSED) return build_fused_plan(plan, desc);
    if (p == RF_PATH_TILED_OVERLAPPED) return build_overlap_plan(plan, desc);
    if (p == RF_PATH_TILED_MATRIX) return build_matrix_plan(plan, desc);
    switch (desc->dtype) {
        case RF_F32: return build_for_pixel<float>(plan, desc, p);
        case RF_F64: return build_for_pixel<double>(plan, desc, p);
        case RF_I32: return build_for_pixel<int32_t>(plan, desc, p);
        case RF_I16: return build_for_pixel<int16_t>(plan, desc, p);
    }
    return RF_ERR_INVALID_ARG;
}

// the scans as the plan runs them (after the rewrite into sections, grouped by dimension), for rf_plan_table("scans"):
// per scan [dim, causal, order, b, a[0..7], mod_n, mod_g[0..7]] -- what tests/fused_emulator.py replays
void publish_scans_table(rf_plan *plan) {
    std::vector<double> flat;
    for (const Scan &sc : plan->scans) {
        flat.push_back(sc.dim); flat.push_back(sc.causal ? 1.0 : 0.0); flat.push_back(sc.order); flat.push_back(sc.b);
        for (int j = 0; j < RF_MAX_ORDER; j++) flat.push_back(sc.a[j]);
        flat.push_back(sc.mod_n);
        for (int j = 0; j < RF_MAX_ORDER; j++) flat.push_back(sc.mod_g[j]);
    }
    plan->tables["scans"] = flat;
}

// The one exit of a build: `rc` is what the last builder returned; a plan that was built is handed to the caller.
// Table uploads and zero fills are work of a private NON-BLOCKING stream (build_stream below): waiting for it waits
// neither for the device nor -- as the legacy null stream would -- for every blocking stream of the process.  A replica
// is built while other streams are busy with executions of this very plan (capi.cpp, acquire_instance), and such a
// wait would serialise what the replica exists to overlap.
int finish(int rc, std::unique_ptr<rf_plan> &plan, const rf_filter_desc *desc, rf_plan **out) {
    if (rc != RF_OK) return rc;
    save_desc(plan.get(), desc);
    if (int fb = plan->finish_build()) return fb;
    *out = plan.release();
    return RF_OK;
}

}  // namespace

int build_plan(const rf_filter_desc *desc, rf_plan **out) {
    if (!desc || !out) { set_error("null argument"); return RF_ERR_INVALID_ARG; }
    *out = nullptr;
    if (int rc = validate_desc(desc)) return rc;
    const bool bytes_out = desc->pointwise.in_dtype == RF_IO_U8;       // (a staged plan: its RF_IN_U8 child merges its own runs)
    if (!bytes_out && plan_merged_runs(desc, out)) return RF_OK;
    std::unique_ptr<rf_plan> plan(new rf_plan);
    if (int rc = describe(desc, plan.get())) return rc;
    const bool half = is_half(desc->dtype);
    if (half && !half_plan_is_native(desc, plan.get())) return finish(build_staged_half(desc, plan.get()), plan, desc, out);
    if (bytes_out && !u8_plan_is_native(desc, plan.get())) return finish(build_staged_u8(desc, plan.get()), plan, desc, out);
    rewrite_into_sections(desc, plan.get());
    std::string fused_why;
    const bool fused_ok = fused_plan_applicable(plan.get(), desc, &fused_why);       // (of the final scan list: once)
    int rc = try_clamped_1d(desc, plan.get());
    if (rc == kNextStage) rc = try_cascade(desc, plan.get(), fused_ok);
    if (rc != kNextStage) return finish(rc, plan, desc, out);

    const int path = desc->path == RF_PATH_AUTO ? choose_auto_path(desc, plan.get(), fused_ok) : desc->path;
    if ((rc = check_path(desc, plan.get(), path, fused_ok, fused_why)) != RF_OK) return rc;
    // (a native byte-output plan is a fused plan: no other builder knows byte planes)
    rc = (bytes_out && path != RF_PATH_TILED_FUSED) ? (int)RF_ERR_UNSUPPORTED : build_on_path(plan.get(), desc, path);
    if (bytes_out && rc == RF_ERR_UNSUPPORTED) {                     // the fused builder refused the shape after all
        plan = fresh_description(*plan);
        return finish(build_staged_u8(desc, plan.get()), plan, desc, out);
    }
    if (half && rc == RF_ERR_UNSUPPORTED && !plan->sharded()) {      // the fused builder refused the shape after all
        plan = fresh_description(*plan);
        return finish(build_staged_half(desc, plan.get()), plan, desc, out);
    }
    if (rc == RF_ERR_UNSUPPORTED && desc->path == RF_PATH_AUTO && path != RF_PATH_UNTILED && !plan->sharded() && !plan->mod_form) {
        // auto mode: a shape no tile fits falls back to the untiled recurrence (still on the GPU)
        plan = fresh_description(*plan);
        plan->pw.pre_fused = plan->pw.post_fused = false;
        rc = build_on_path(plan.get(), desc, RF_PATH_UNTILED);
    }
    if (rc != RF_OK) return rc;
    add_pointwise_steps(plan.get());
    publish_scans_table(plan.get());
    return finish(RF_OK, plan, desc, out);
}

}  // namespace rf

rf_plan::~rf_plan() {
    replicas.clear();
    stages.clear();
    helpers.clear();
    if (done) (void)hipEventDestroy(done);
    for (auto &b : buffers)
        if (b.ptr) (void)hipFree(b.ptr);
}

namespace {
// One stream per device for everything a plan build puts on the GPU (zero fills, table uploads): created once with
// hipStreamNonBlocking, so that it neither waits for nor is waited for by the null stream, and kept for the life of the
// process.  HIP streams may be used from several host threads.
hipStream_t build_stream(int device, int *status) {
    static std::mutex mu;
    static std::map<int, hipStream_t> streams;
    std::lock_guard<std::mutex> lock(mu);
    auto it = streams.find(device);
    if (it != streams.end()) return it->second;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
        rf::set_error("hipStreamCreateWithFlags (plan build stream) failed");
        *status = RF_ERR_HIP;
        return nullptr;
    }
    streams[device] = s;
    return s;
}
}  // namespace

void rf_plan::all_buffers(std::vector<const rf::DeviceBuffer *> &into) const {
    for (const auto &b : buffers) into.push_back(&b);
    for (const auto &s : stages) s->all_buffers(into);
    for (const auto &h : helpers) h->all_buffers(into);
}

void *rf_plan::alloc(size_t bytes, bool zero, int *status) { return alloc_kind(bytes, zero ? RF_BUFFER_ZEROED : RF_BUFFER_SCRATCH, status); }

void *rf_plan::alloc_kind(size_t bytes, int kind, int *status) {
    const bool zero = kind == RF_BUFFER_ZEROED;
    if (*status != RF_OK) return nullptr;
    if (bytes == 0) bytes = 16;
    if (host_only) { buffers.push_back({nullptr, bytes, kind}); workspace_bytes += bytes; return nullptr; }
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        rf::set_error("hipMalloc of %zu bytes failed", bytes);
        *status = RF_ERR_NOMEM;
        return nullptr;
    }
    buffers.push_back({p, bytes, kind});
    workspace_bytes += bytes;
    if (zero) {
        hipStream_t bs = build_stream(device, status);
        if (*status == RF_OK && hipMemsetAsync(p, 0, bytes, bs) != hipSuccess) {
            rf::set_error("hipMemsetAsync failed");
            *status = RF_ERR_HIP;
        }
    }
    return p;
}

void *rf_plan::upload(const void *host, size_t bytes, int *status) {
    void *p = alloc_kind(bytes, RF_BUFFER_TABLE, status);
    if (!p) return nullptr;
    if (bytes) {
        // the host tables are temporaries of the build: the copy has left them when this returns
        hipStream_t bs = build_stream(device, status);
        if (*status == RF_OK && (hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, bs) != hipSuccess || hipStreamSynchronize(bs) != hipSuccess)) {
            rf::set_error("hipMemcpyAsync (table upload) failed");
            *status = RF_ERR_HIP;
        }
    }
    return p;
}

int rf_plan::finish_build() {
    if (host_only) return RF_OK;
    int status = RF_OK;
    hipStream_t bs = build_stream(device, &status);
    if (status != RF_OK) return status;
    RF_HIP_CHECK(hipStreamSynchronize(bs));
    if (done == nullptr) RF_HIP_CHECK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    return RF_OK;
}
