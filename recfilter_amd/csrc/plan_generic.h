// plan_generic.h -- builds the step list of ONE dimension on the generic tiled path
// (pass 1, per-scan carry stages, pass 2).  Shared by plan.cpp (every dimension) and
// plan_fused.cpp (the z dimension of 3-D filters).
#pragma once

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "kernels_fused.h"
#include "plan.h"
#include "plan_carry.h"

namespace rf {

// One scan as the fused / line kernels read it: coefficients plus, with_segment_tables, the tables of the 16-sample
// segment scan of the x phase (scan_device.h: R = effect of the entering state on the segment, in MEMORY order;
// P = segment exit-state transfer over 1, 2, 4, 8 segments) -- the tables of the causal twin at T = 16.
template <typename S, typename Acc>
FusedScan<Acc> make_fused_scan(const Scan &scan, int K, bool with_segment_tables) {
    FusedScan<Acc> f;
    std::memset(&f, 0, sizeof(f));
    ScanS<S> ts = make_table_scan<S>(scan);
    f.causal = ts.causal ? 1 : 0;
    f.b = table_to_acc<S, Acc>(ts.b);
    for (int j = 0; j < K && j < kFusedMaxK; j++) f.a[j] = table_to_acc<S, Acc>(ts.a[j]);
    f.mod_n = scan.mod_n;
    if constexpr (!std::is_same<S, uint64_t>::value) {
        for (int j = 0; j < kFusedMaxMod && j < RF_MAX_ORDER; j++) f.mod_g[j] = (Acc)ts.mod_g[j];
    }
    if (with_segment_tables) {
        ScanS<S> twin = ts;
        twin.causal = true;
        DimTables<S> seg = build_dim_tables<S>({twin}, K, kFusedSeg, false);
        const std::vector<S> &R = seg.P(0, 0, 0);
        for (int p = 0; p < kFusedSeg; p++)
            for (int j = 0; j < K; j++)     // direction position p -> memory position inside the segment
                f.R[j][ts.causal ? p : kFusedSeg - 1 - p] = table_to_acc<S, Acc>(R[(size_t)p * K + j]);
        std::vector<S> Pw = seg.A[0];
        for (int step = 0; step < 4; step++) {
            for (int r = 0; r < K; r++)
                for (int j = 0; j < K; j++) f.P[step][r][j] = table_to_acc<S, Acc>(Pw[r * K + j]);
            Pw = mat_mul<S>(Pw, Pw, K);
        }
    }
    return f;
}

// ---- merged exchange (one all-gather per sharded dimension) ------------------------------------------------
// With zero entering carries every slab completes ALL its scans locally; what the true entering carries in_q add
// afterwards is linear in them.  Y[q][s][t] (k x k, q <= s, t in memory order) is what a unit carry entering scan q
// adds to the completed tail of scan s at tile t: for q == s the plain propagation A_s^(i+1), for q < s the chaining
// terms W (create_tail_residual_term, lib/split.cpp:912-1004) followed by scan s's own recurrence.  The tables
// depend on which ends of the slab are image borders.  Flattened [q][s][t][r][o]; entries with q > s are zero.
template <typename S>
std::vector<S> cross_scan_transfer(const DimTables<S> &tab, int64_t M, bool first_is_border, bool last_is_border) {
    const int n = tab.n, k = tab.k, kk = k * k;
    std::vector<S> Y((size_t)n * n * M * kk, S(0));
    auto causal = [&](int s) { return tab.scans[s].causal; };
    auto variant = [&](int64_t t) { return ((t == 0 && first_is_border) ? 1 : 0) | ((t == M - 1 && last_is_border) ? 2 : 0); };
    std::vector<std::vector<S>> C(n, std::vector<S>((size_t)M * k));     // C[s][t*k + r]: effect on scan s, tile t
    for (int q = 0; q < n; q++)
        for (int o = 0; o < k; o++) {
            for (int s = q; s < n; s++) {
                std::vector<S> &Cs = C[s];
                std::fill(Cs.begin(), Cs.end(), S(0));
                if (s > q) {      // chaining on the scans q .. s-1 (their effects are already in C)
                    for (int64_t t = 0; t < M; t++) {
                        const int v = variant(t);
                        for (int qq = q; qq < s; qq++) {
                            const bool first = causal(qq) ? (t == 0) : (t == M - 1);
                            const std::vector<S> &Wm = tab.Wm(v, qq, s);
                            for (int r = 0; r < k; r++) {
                                S acc = S(0);
                                for (int j = 0; j < k; j++) {
                                    S c;
                                    if (first) c = (qq == q && j == o) ? S(1) : S(0);
                                    else c = C[qq][(size_t)(causal(qq) ? t - 1 : t + 1) * k + j];
                                    acc = acc + Wm[r * k + j] * c;
                                }
                                Cs[(size_t)t * k + r] = Cs[(size_t)t * k + r] + acc;
                            }
                        }
                    }
                }
                // scan s's own recurrence over the tiles; for s == q the entering state is the unit carry
                std::vector<S> x(k, S(0));
                if (s == q) x[o] = S(1);
                for (int64_t i = 0; i < M; i++) {
                    const int64_t t = causal(s) ? i : M - 1 - i;
                    for (int r = 0; r < k; r++) {
                        S acc = Cs[(size_t)t * k + r];
                        for (int j = 0; j < k; j++) acc = acc + tab.A[s][r * k + j] * x[j];
                        Cs[(size_t)t * k + r] = acc;
                    }
                    for (int r = 0; r < k; r++) x[r] = Cs[(size_t)t * k + r];
                }
                for (int64_t t = 0; t < M; t++)
                    for (int r = 0; r < k; r++)
                        Y[(((size_t)q * n + s) * M + t) * kk + r * k + o] = Cs[(size_t)t * k + r];
            }
        }
    return Y;
}

inline bool merged_exchange_applies(int n_scans, int k, int world) {
    return world >= 1 && n_scans >= 1 && n_scans <= 4 && k >= 1 && k <= 3 && n_scans * world * k <= 128;
}

// Exchange structure of a sharded dimension with ONE all-gather: the local step completes every scan with zero
// entering carries and publishes all exit carries ([plane][s][r][line]); the apply step derives every scan's true
// entering carry from the gathered exits and corrects all tails in one pass.
// (the stage's tile width is the same on every rank; slab h has plan->slab_tiles(h, T) tiles.)
template <typename S, typename Acc>
int add_merged_exchange(rf_plan *plan, const CarryStage<S, Acc> &stage, const std::string &carry_name,
                        const Acc **apply_in_final_pass = nullptr) {
    int status = RF_OK;
    const DimTables<S> &tab = stage.tab;
    const CarryDev<Acc> c = stage.dev;
    const std::string &dn = stage.dn;
    const int64_t T = stage.T, lines = stage.lines;
    const size_t inc_pp = stage.inc_pp;
    const int n = tab.n, K = tab.k, kk = K * K, np = plan->n_planes;
    const int world = plan->shard_world, rank = plan->shard_rank;
    // X[h]: the exit-tile rows of slab h's transfer (its own tile count and border type); Y: this slab's, every tile
    std::vector<Acc> hY, hX((size_t)world * n * n * kk, Acc(0));
    std::vector<double> dY, dX(hX.size(), 0.0);
    for (int h = 0; h < world; h++) {
        const int64_t Mh = plan->slab_tiles(h, T);
        std::vector<S> Y = cross_scan_transfer<S>(tab, Mh, h == 0, h == world - 1);
        for (int q = 0; q < n; q++)
            for (int s = q; s < n; s++) {
                const int64_t t_exit = tab.scans[s].causal ? Mh - 1 : 0;
                for (int e = 0; e < kk; e++) {
                    const S v = Y[(((size_t)q * n + s) * Mh + t_exit) * kk + e];
                    hX[(((size_t)h * n + q) * n + s) * kk + e] = table_to_acc<S, Acc>(v);
                    dX[(((size_t)h * n + q) * n + s) * kk + e] = table_to_double<S>(v);
                }
            }
        if (h == rank) {
            hY.resize(Y.size());
            dY.resize(Y.size());
            for (size_t e = 0; e < Y.size(); e++) { hY[e] = table_to_acc<S, Acc>(Y[e]); dY[e] = table_to_double<S>(Y[e]); }
        }
    }
    plan->tables["Y_" + dn] = dY;
    plan->tables["X_" + dn] = dX;
    const Acc *d_Y = (const Acc *)plan->upload(hY.data(), hY.size() * sizeof(Acc), &status);
    const Acc *d_X = (const Acc *)plan->upload(hX.data(), hX.size() * sizeof(Acc), &status);

    const int64_t plane_stride = (int64_t)n * K * lines, rank_stride = (int64_t)np * plane_stride;
    const int ex_index = (int)plan->exchanges.size();
    rf_plan::Exchange ex;
    ex.bytes = (size_t)rank_stride * sizeof(Acc);
    ex.scratch = plan->alloc(ex.bytes, true, &status);
    if (status != RF_OK) return status;
    ex.send = ex.scratch;
    ex.form_incoming = [plan, c, rank_stride, plane_stride, d_X](const void *gathered) {
        for (int pl = 0; pl < plan->n_planes; pl++) {
            int rc = launch_merged_gather<Acc>(c.args(pl), (const Acc *)gathered, rank_stride, pl * plane_stride,
                                               plan->shard_rank, plan->shard_world, d_X, plan->stream);
            if (rc) return rc;
        }
        return (int)RF_OK;
    };
    plan->exchanges.push_back(ex);

    // the local pass sees zero entering carries: a buffer of zeros of its own (the plan's `incoming` holds the true
    // carries of the previous execute until the gather overwrites them)
    const Acc *zeros = (const Acc *)plan->alloc(inc_pp * np * sizeof(Acc), true, &status);
    if (status != RF_OK) return status;
    Step cs;
    cs.name = carry_name;
    cs.run = [plan, c, K, n, ex_index, plane_stride, zeros, inc_pp](int pl) {
        Acc *send = (Acc *)plan->exchanges[ex_index].send;
        auto a = c.args(pl);
        a.incoming = const_cast<Acc *>(zeros) + (size_t)pl * inc_pp;
        return launch_carry_block<Acc>(K, a, c.causal_mask, 0, n, send ? send + pl * plane_stride : nullptr, c.AC, c.C,
                                       plan->stream);
    };
    plan->exchange_local_steps.push_back({cs});
    if (apply_in_final_pass != nullptr) {
        // the caller's final pass adds Y * in as it loads a carry (fused pass 2): the tails are not rewritten
        *apply_in_final_pass = d_Y;
        plan->exchange_apply_steps.push_back({});
        return status;
    }
    Step ap;
    ap.name = carry_name + "_apply";
    ap.run = [plan, c, d_Y](int pl) { return launch_merged_apply<Acc>(c.args(pl), d_Y, plan->stream); };
    plan->exchange_apply_steps.push_back({ap});
    return status;
}

inline int pick_generic_tile(int64_t N, int k, int hint) {
    if (hint > 0 && hint <= kGenericMaxTile && N % hint == 0 && hint >= k) return hint;
    int cap = hint > 0 ? kGenericMaxTile : 64;
    for (int T = (int)std::min<int64_t>(cap, N); T >= std::max(k, 1); T--)
        if (N % T == 0) return T;
    return 0;
}


// Appends the steps of dimension d.  from_input: this is the first filtered dimension, its
// passes read the caller's input planes; otherwise they read (and overwrite) the output planes.
template <typename P, typename S>
int add_generic_dimension(rf_plan *plan, int tile_hint, int d, bool from_input_flag) {
    using Acc = typename PixelTraits<P>::Acc;
    int status = RF_OK;
    const int outer = plan->ndim - 1;
    const bool first_dim = from_input_flag;
    {
        DimInfo &di = plan->dims[d];
        int T = pick_generic_tile(plan->tile_basis(d), di.k, tile_hint);       // (sharded: every slab must tile alike)
        if (T == 0) {
            set_error("no tile width <= %d divides extent %lld of dimension %d", kGenericMaxTile, (long long)di.N, d);
            return RF_ERR_UNSUPPORTED;
        }
        di.T = T;
        di.M = di.N / T;
        const int n = (int)di.scan_ids.size();
        const int k = di.k;

        const bool is_exchange_dim = (d == outer);   // its carry stage is exposed through the stepping API
        const bool sharded_dim = is_exchange_dim && plan->sharded();
        std::string dn(1, "xyz"[d]);
        CarryStage<S, Acc> stage;
        typename CarryStage<S, Acc>::Options opt;
        opt.sharded = sharded_dim;
        opt.slab_powers = true;          // A^M for the exchange (sharded outermost dimension)
        opt.apply_powers = sharded_dim;
        status = stage.init(plan, di.scan_ids, dn, k, T, di.M, LineGeom{di.N, di.stride, di.lines}, opt);
        const DimTables<S> &tab = stage.tab;
        {
            std::vector<double> dP;
            for (int v = 0; v < 4; v++)
                for (int q = 0; q < n; q++)
                    for (int s = 0; s < n; s++) {
                        if (s >= q) for (S x : tab.P(v, q, s)) dP.push_back(table_to_double<S>(x));
                        else dP.insert(dP.end(), (size_t)T * k, 0.0);
                    }
            plan->tables["prop_" + dn] = dP;
        }
        if (status == RF_OK) status = stage.alloc_buffers(plan);
        if (status != RF_OK) return status;
        const CarryDev<Acc> c = stage.dev;
        const bool from_input = first_dim;

        Step p1;
        p1.name = "generic_pass1_" + dn;
        p1.run = [plan, c, from_input](int pl) {
            const P *src = from_input ? (const P *)plan->in[pl] : (const P *)plan->out[pl];
            return launch_generic_pass1<P>(src, c.args(pl), plan->stream);
        };
        plan->begin_steps.push_back(p1);

        if (is_exchange_dim && merged_exchange_applies(n, k, plan->shard_world)) {
            int rc = add_merged_exchange<S, Acc>(plan, stage, "generic_carry_" + dn);
            if (rc != RF_OK) return rc;
        } else {
            int rc = stage.add_per_scan_carries(plan, "generic_carry_" + dn, "generic_carry_apply_" + dn, is_exchange_dim);
            if (rc != RF_OK) return rc;
        }

        Step p2;
        p2.name = "generic_pass2_" + dn;
        p2.run = [plan, c, from_input](int pl) {
            const P *src = from_input ? (const P *)plan->in[pl] : (const P *)plan->out[pl];
            return launch_generic_pass2<P>(src, (P *)plan->out[pl], c.args(pl), plan->stream);
        };
        if (is_exchange_dim) plan->finish_steps.push_back(p2);
        else plan->begin_steps.push_back(p2);
    }
    return status;
}

}  // namespace rf
