// plan_carry.h -- the carry stage of ONE tiled dimension, as every plan builder sets it up: the chaining tables W / A in
// the kernels' type (and as the doubles rf_plan_table reports), A^C for the blocked carry scan (kernels_carry.hip), the
// tails / entering-carry buffers, the GenericDimArgs of a plane, and the steps that run the carry recurrence -- one launch
// over all scans, or scan by scan around the exchanges of a sharded dimension.  Used by plan_fused.cpp (x and y),
// plan_generic.h, plan_strided.h and plan_overlap.cpp.
#pragma once

#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "kernels_fused.h"
#include "plan.h"

namespace rf {

template <typename Acc>
DevScan<Acc> make_dev_scan(const Scan &s) {
    DevScan<Acc> d;
    d.causal = s.causal ? 1 : 0;
    d.order = s.order;
    if constexpr (std::is_same<Acc, uint32_t>::value) {
        d.b = (uint32_t)(int64_t)s.b;
        for (int j = 0; j < RF_MAX_ORDER; j++) d.a[j] = (uint32_t)(int64_t)s.a[j];
    } else {
        d.b = (Acc)s.b;
        for (int j = 0; j < RF_MAX_ORDER; j++) d.a[j] = (Acc)s.a[j];
    }
    return d;
}

template <typename S>
ScanS<S> make_table_scan(const Scan &s) {
    ScanS<S> t;
    t.causal = s.causal;
    if constexpr (std::is_same<S, uint64_t>::value) {
        t.b = (uint64_t)(int64_t)s.b;
        for (int j = 0; j < RF_MAX_ORDER; j++) t.a[j] = (uint64_t)(int64_t)s.a[j];
    } else {
        t.b = (S)s.b;
        for (int j = 0; j < RF_MAX_ORDER; j++) t.a[j] = (S)s.a[j];
        t.mod_n = s.mod_n;
        for (int j = 0; j < RF_MAX_ORDER; j++) t.mod_g[j] = (S)s.mod_g[j];
    }
    return t;
}

template <typename S, typename Acc>
Acc table_to_acc(S v) {
    if constexpr (std::is_same<Acc, uint32_t>::value) return (uint32_t)v;
    else return (Acc)v;
}

template <typename S>
double table_to_double(S v) {
    if constexpr (std::is_same<S, uint64_t>::value) return (double)(int64_t)v;
    else return (double)v;
}

// A table in the kernels' arithmetic type; `name` non-empty: also published as the doubles rf_plan_table(name) reports
template <typename S, typename Acc>
std::vector<Acc> table_for_kernels(rf_plan *plan, const std::vector<S> &t, const std::string &name = std::string()) {
    std::vector<Acc> out(t.size());
    for (size_t e = 0; e < t.size(); e++) out[e] = table_to_acc<S, Acc>(t[e]);
    if (!name.empty()) {
        std::vector<double> d(t.size());
        for (size_t e = 0; e < t.size(); e++) d[e] = table_to_double<S>(t[e]);
        plan->tables[name] = d;
    }
    return out;
}

// (A[s])^(i+1) for i = 0..M-1, flattened [s][i][r][j] in the kernels' arithmetic type (GenericDimArgs::Apow)
template <typename S, typename Acc>
std::vector<Acc> carry_apply_powers(const std::vector<std::vector<S>> &A, int64_t M, int k) {
    std::vector<Acc> out((size_t)A.size() * M * k * k);
    for (size_t s = 0; s < A.size(); s++) {
        std::vector<S> pw = A[s];
        for (int64_t i = 0; i < M; i++) {
            for (int e = 0; e < k * k; e++) out[((size_t)s * M + i) * k * k + e] = table_to_acc<S, Acc>(pw[e]);
            pw = mat_mul<S>(pw, A[s], k);
        }
    }
    return out;
}

// A_s^(tiles of slab h) for every scan and every slab of the sharded dimension, [s][h][k x k]: what carries the state
// entering slab h to its exit (per-scan exchange; slabs may have different extents).
template <typename S, typename Acc>
std::vector<Acc> slab_powers(const rf_plan *plan, const std::vector<std::vector<S>> &A, int64_t T, int k) {
    const int n = (int)A.size(), world = plan->shard_world;
    std::vector<Acc> out((size_t)n * world * k * k, Acc(0));
    for (int s = 0; s < n; s++)
        for (int h = 0; h < world; h++) {
            std::vector<S> am = mat_pow<S>(A[s], plan->slab_tiles(h, T), k);
            for (int e = 0; e < k * k; e++) out[((size_t)s * world + h) * k * k + e] = table_to_acc<S, Acc>(am[e]);
        }
    return out;
}

// [s][k x k] of A[s]^p in the kernels' arithmetic type
template <typename S, typename Acc>
std::vector<Acc> scan_powers(const std::vector<std::vector<S>> &A, int64_t p, int k) {
    std::vector<Acc> out(A.size() * (size_t)k * k, Acc(0));
    for (size_t s = 0; s < A.size(); s++) {
        std::vector<S> ap = mat_pow<S>(A[s], p, k);
        for (int e = 0; e < k * k; e++) out[s * k * k + e] = table_to_acc<S, Acc>(ap[e]);
    }
    return out;
}

// The device side of a carry stage: what its steps capture.  Steps outlive the builder that made them, so they hold a COPY
// of this (pointers and integers only), never a reference to the CarryStage on the builder's stack.
template <typename Acc>
struct CarryDev {
    GenericDimArgs<Acc> base{};        // everything but a plane's tails / incoming; tile_major is the caller's to set
    uint32_t causal_mask = 0;          // bit s: scan s is causal
    const Acc *AC = nullptr;           // [s][k x k] = A[s]^C, the chunk transition of the blocked carry scan
    int C = 1;
    const Acc *AM = nullptr;           // [s][slab][k x k] (slab_powers); null unless the stage was built with them
    Acc *tails = nullptr, *incoming = nullptr;
    size_t tails_stride = 0, inc_stride = 0;      // elements between consecutive planes
    const Acc *tails_part2 = nullptr;  // GenericDimArgs::tails_part2 of plane 0 (same pitch as tails); null: one part

    GenericDimArgs<Acc> args(int pl) const {
        GenericDimArgs<Acc> a = base;
        a.tails = tails + (size_t)pl * tails_stride;
        a.incoming = incoming + (size_t)pl * inc_stride;
        if (tails_part2) a.tails_part2 = tails_part2 + (size_t)pl * tails_stride;
        return a;
    }
};

template <typename S, typename Acc>
struct CarryStage {
    struct Options {
        int T_last = -1;              // samples of the last tile where it is partial (tables.h); -1: whole tiles
        bool sharded = false;         // the dimension is cut into slabs: this rank may hold neither border
        bool slab_powers = false;     // A^(tiles of every slab), for the per-scan exchange (CarryDev::AM)
        bool apply_powers = false;    // A^1 .. A^M, for carry_apply (GenericDimArgs::Apow); otherwise Apow stays NULL
    };

    std::string dn;                   // "x" / "y" / "z": suffix of the table names
    int n = 0, k = 0, T = 0;
    int64_t M = 0, lines = 0;
    DimTables<S> tab;
    size_t tails_pp = 0, inc_pp = 0;  // elements of one plane's tails / entering carries
    CarryDev<Acc> dev;

    // Tables of the scans `ids` of `plan` at order k over M tiles of T samples; publishes W_<dn> / A_<dn> and uploads.
    int init(rf_plan *plan, const std::vector<int> &ids, const std::string &name, int order, int tile, int64_t tiles,
             const LineGeom &g, const Options &opt) {
        int status = RF_OK;
        dn = name; n = (int)ids.size(); k = order; T = tile; M = tiles; lines = g.lines;
        std::vector<ScanS<S>> ts;
        std::vector<DevScan<Acc>> ds;
        for (int i = 0; i < n; i++) {
            ts.push_back(make_table_scan<S>(plan->scans[ids[i]]));
            DevScan<Acc> dv = make_dev_scan<Acc>(plan->scans[ids[i]]);
            dv.order = k;             // shorter scans are zero padded to the dimension's order (lib/split.cpp:575-578)
            ds.push_back(dv);
            if (ts[i].causal) dev.causal_mask |= 1u << i;
        }
        tab = build_dim_tables<S>(ts, k, T, plan->clamped, opt.T_last);
        std::vector<Acc> hW((size_t)4 * n * n * k * k, Acc(0)), hA((size_t)n * k * k, Acc(0));
        std::vector<double> dW(hW.size(), 0.0), dA(hA.size(), 0.0);
        for (int v = 0; v < 4; v++)
            for (int q = 0; q < n; q++)
                for (int s = q + 1; s < n; s++)
                    for (int e = 0; e < k * k; e++) {
                        size_t idx = (((size_t)v * n + q) * n + s) * k * k + e;
                        hW[idx] = table_to_acc<S, Acc>(tab.Wm(v, q, s)[e]);
                        dW[idx] = table_to_double<S>(tab.Wm(v, q, s)[e]);
                    }
        for (int s = 0; s < n; s++)
            for (int e = 0; e < k * k; e++) {
                hA[(size_t)s * k * k + e] = table_to_acc<S, Acc>(tab.A[s][e]);
                dA[(size_t)s * k * k + e] = table_to_double<S>(tab.A[s][e]);
            }
        if (n > 0) {                  // (a dimension without scans has its placeholders uploaded, but no tables to show)
            plan->tables["W_" + dn] = dW;
            plan->tables["A_" + dn] = dA;
        }
        dev.C = carry_chunk_length(M, lines, k);
        const std::vector<Acc> hAC = scan_powers<S, Acc>(tab.A, dev.C, k);

        auto up = [&](const auto &vec) {
            using E = typename std::decay<decltype(vec)>::type::value_type;
            return (const E *)plan->upload(vec.data(), vec.size() * sizeof(E), &status);
        };
        GenericDimArgs<Acc> &b = dev.base;
        b.g = g;
        b.T = T; b.M = (int32_t)M; b.k = k; b.n_scans = n;
        b.clamped = plan->clamped ? 1 : 0;
        b.first_is_border = (!opt.sharded || plan->shard_rank == 0) ? 1 : 0;
        b.last_is_border = (!opt.sharded || plan->shard_rank == plan->shard_world - 1) ? 1 : 0;
        b.scans = up(ds); b.W = up(hW); b.A = up(hA);
        dev.AC = up(hAC);
        if (opt.slab_powers) dev.AM = up(slab_powers<S, Acc>(plan, tab.A, T, k));
        if (opt.apply_powers) b.Apow = up(carry_apply_powers<S, Acc>(tab.A, M, k));
        tails_pp = (size_t)n * M * k * lines;
        inc_pp = (size_t)n * k * lines;
        return status;
    }

    // the stage's own buffers, one run per plane ...
    int alloc_buffers(rf_plan *plan) {
        int status = RF_OK;
        Acc *t = (Acc *)plan->alloc(tails_pp * plan->n_planes * sizeof(Acc), false, &status);
        Acc *i = (Acc *)plan->alloc(inc_pp * plan->n_planes * sizeof(Acc), true, &status);     // zeros: image borders
        use_buffers(t, tails_pp, i, inc_pp);
        return status;
    }
    // ... or the caller's, with their own pitches
    void use_buffers(Acc *tails, size_t tails_stride, Acc *incoming, size_t inc_stride) {
        dev.tails = tails; dev.tails_stride = tails_stride;
        dev.incoming = incoming; dev.inc_stride = inc_stride;
    }

    // the carry recurrence of every scan in ONE launch (kernels_carry.hip), as a begin step
    void add_local_carry(rf_plan *plan, const std::string &name) const {
        const CarryDev<Acc> c = dev;
        Step cs;
        cs.name = name;
        cs.run = [plan, c](int pl) {
            return launch_carry_block<Acc>(c.base.k, c.args(pl), c.causal_mask, 0, c.base.n_scans, (Acc *)nullptr, c.AC, c.C, plan->stream);
        };
        plan->begin_steps.push_back(cs);
    }

    // The carry recurrence scan by scan: steps <local_name><s>.  `exchanged` (the outermost dimension, whose carry stage the
    // stepping API exposes): every scan is an exchange -- the local step publishes the slab's exit carries, form_incoming turns
    // the gathered exits into the carry entering this slab (needs Options::slab_powers), <apply_name><s> propagates it through
    // the tails.  Otherwise the scans are plain begin steps.
    int add_per_scan_carries(rf_plan *plan, const std::string &local_name, const std::string &apply_name, bool exchanged) const {
        int status = RF_OK;
        const CarryDev<Acc> c = dev;
        const int np = plan->n_planes;
        const int64_t plane_stride = (int64_t)k * lines, rank_stride = (int64_t)np * k * lines;
        for (int s = 0; s < n; s++) {
            int ex_index = -1;
            if (exchanged) {
                ex_index = (int)plan->exchanges.size();
                rf_plan::Exchange ex;
                ex.bytes = (size_t)np * k * lines * sizeof(Acc);
                ex.scratch = plan->alloc(ex.bytes, true, &status);
                if (status != RF_OK) return status;
                ex.send = ex.scratch;
                const Acc *AMs = c.AM + (size_t)s * plan->shard_world * k * k;      // [slab][k x k]
                ex.form_incoming = [plan, c, s, rank_stride, plane_stride, AMs](const void *gathered) {
                    for (int pl = 0; pl < plan->n_planes; pl++) {
                        int rc = launch_gather_incoming<Acc>(c.args(pl), s, (const Acc *)gathered, rank_stride, pl * plane_stride,
                                                             plan->shard_rank, plan->shard_world, AMs, plan->stream);
                        if (rc) return rc;
                    }
                    return (int)RF_OK;
                };
                plan->exchanges.push_back(ex);
            }
            Step cs;
            cs.name = local_name + std::to_string(s);
            // the blocked parallel scan of kernels_carry.hip: parallel over lines AND over chunks of tiles, so a 1-D
            // signal (one line) does not degenerate into one thread walking every tile
            cs.run = [plan, c, s, ex_index, plane_stride](int pl) {
                Acc *send = ex_index >= 0 ? (Acc *)plan->exchanges[ex_index].send : nullptr;
                if (send) send += pl * plane_stride;
                if (c.base.k > kCarryBlockMaxOrder)        // (orders 9..32: one thread per line, kernels_generic.hip)
                    return launch_generic_carry_serial<Acc>(c.args(pl), c.causal_mask, s, s + 1, send, plan->stream);
                return launch_carry_block<Acc>(c.base.k, c.args(pl), c.causal_mask, s, s + 1, send, c.AC, c.C, plan->stream);
            };
            if (!exchanged) {
                plan->begin_steps.push_back(cs);
                continue;
            }
            plan->exchange_local_steps.push_back({cs});
            Step ap;
            ap.name = apply_name + std::to_string(s);
            ap.run = [plan, c, s](int pl) { return launch_generic_carry_apply<Acc>(c.args(pl), s, plan->stream); };
            plan->exchange_apply_steps.push_back({ap});
        }
        return status;
    }
};

// The step "carry_planes_xy": a helper plan (the x/y filter F over carry planes, plan_strided.h) run on plane pl's carry
// planes, `tails + pl * stride`, in place, appended to `into`.  ONE step: the helper has one workspace, so its launches for a
// plane run back to back (the steps of an execute run plane by plane inside every step).  The plan takes the helper over
// (plan.h, "a plan driven by another plan").
template <typename Acc>
int adopt_carry_planes_plan(rf_plan *plan, std::unique_ptr<rf_plan> helper, Acc *tails, size_t stride, std::vector<Step> &into) {
    rf_plan *child = helper.get();
    std::vector<const Step *> steps;
    if (int rc = child_steps(child, steps)) return rc;
    plan->helpers.push_back(std::move(helper));
    take_over_child(plan, child, false);
    Step w;
    w.name = "carry_planes_xy";
    w.run = [plan, child, steps, tails, stride](int pl) {
        // the helper's context: this plane's run of carry planes, filtered in place
        Acc *planes = tails + (size_t)pl * stride;
        bind_child(child, 1, plan->stream, [planes](int) { return ChildPlanes{planes, planes}; });
        for (const Step *sp : steps) {
            const int rc = sp->run(0);
            if (rc != RF_OK) return rc;
        }
        return (int)RF_OK;
    };
    into.push_back(w);
    return RF_OK;
}

}  // namespace rf
