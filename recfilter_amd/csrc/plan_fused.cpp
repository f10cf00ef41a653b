// plan_fused.cpp -- plan for the LDS-staged fused x/y path (kernels_fused.hip).
//
// Stages of one execute (2-D; a 3-D filter runs this per z plane as a batch and then filters z
// with the generic dimension builder):
//   fused_tails      pass 1: tile-local tails of every x scan (per row) and the y tails' combined rows, by
//                    contraction with precomputed impulse responses
//   carry_x          x carry recurrence, all x scans (same-dimension chaining included); not run where the x carries
//                    take the neighbour form (neighbour_carry_bound below)
//   xscan_rows       finishes the y tails: tile-local x scans of the combined rows + the cross-dimension
//                    residual of the completed x carries (lib/split.cpp:1215-1633)
//   carry_y          y carry recurrence, all y scans (one launch per scan around the exchanges when sharded); not run
//                    where the y carries take the neighbour form
//   fused_pass2      final correction pass
// build_fused below is that list: geometry (fused_geometry) -> tables (fused_tables) -> buffers -> steps (FusedBuilder).
#include <cmath>
#include <cstring>
#include <memory>

#include "kernels_fused.h"
#include "plan.h"
#include "plan_carry.h"
#include "plan_generic.h"
#include "plan_strided.h"

namespace rf {

namespace {

int fused_order(const rf_plan *plan) {
    return std::max(plan->dims[0].k, plan->ndim > 1 ? plan->dims[1].k : 0);
}

// A long 1-D signal runs on the fused path folded into rows: N = NY rows of NX samples, every row tiled like an
// image row and the rows chained through their entering states ("chained rows").  Longest row first: fewer rows
// to chain, and the blocked carry scan still finds NY * MX/16 waves of work.
// A zero-border 1-D signal of any length is the same filter on the signal padded with zeros to the next multiple of 8192, as
// long as no anticausal scan follows a causal one: a causal scan never sees what follows it, and an anticausal scan that runs
// on untouched padding enters the signal with the zero state the padding leaves it in (fused_plan_applicable checks).
// The padded length is chosen so that the signal folds into LONG rows (few rows to chain): the longest row length whose
// 32-row granule costs at most 1/16 of padding.
int64_t chained_padded_length(int64_t N) {
    if (N % 8192 == 0) return N;
    for (int64_t nx = 16384; nx >= kFusedTX; nx /= 2) {
        const int64_t g = nx * 32, np = (N + g - 1) / g * g;
        if (np - N <= N / 16) return np;
    }
    return (N + 8191) / 8192 * 8192;
}

int64_t chained_row_length(int64_t N) {
    for (int64_t nx = 16384; nx >= kFusedTX; nx /= 2)
        if (N % nx == 0 && (N / nx) % 64 == 0) return nx;
    for (int64_t nx = 16384; nx >= kFusedTX; nx /= 2)
        if (N % nx == 0 && (N / nx) % 32 == 0) return nx;
    return 0;
}

// Neighbour-form carries.  The carry scans of a dimension compute, for scan s and tile t,
//   c_s(t) = tau_s(t) + sum_{q<s} W_v(t)[q->s] c_q(tile entering t) + A_s^L c_s(previous tile in s's direction)
// (tau: the tile-local tail with zero entering carries, W_v: the chaining table of t's border variant, A_s^L: the scan's
// transition across a tile).  For a filter that decays within a tile the last term is beyond what an f32 result can see,
// and without it a dimension of one scan, or of a causal scan s0 followed by an anticausal s1, needs no scan at all:
//   c_s0(t) = tau_s0(t),   c_s1(t) = tau_s1(t) + W_v(t)[0->1] tau_s0(t-1)
// -- the neighbour's own tail and, for s1, a k x k product with the tile's own causal tail.  What that form drops from a
// consumed carry, relative to the largest carry, is at most (infinity norms, in double)
//   one scan: |A^L|;   s0, s1: max(|A_s0^L|, max_v |W_v[0->1] A_s0^L| + |A_s1^L|)
// Every dropped transfer crosses a WHOLE tile: only the last tile may be partial, and the only carry that crosses it is the
// causal one leaving the image, which an unsharded plan never consumes (the caller checks that the plan is unsharded).
// Returns -1 for any other pattern of scans.
constexpr double kNeighbourCarryBound = 1.0 / 4294967296.0;      // 2^-32: 1/256 of the rounding the scan form applies to a tail

template <typename S>
double neighbour_carry_bound(const DimTables<S> &tab, const std::vector<int> &ids, const rf_plan *plan) {
    const int n = (int)ids.size(), k = tab.k;
    if (n < 1 || n > 2 || (n == 2 && !(plan->scans[ids[0]].causal && !plan->scans[ids[1]].causal))) return -1.0;
    auto norm = [k](const std::vector<double> &m) {
        double best = 0.0;
        for (int r = 0; r < k; r++) {
            double row = 0.0;
            for (int o = 0; o < k; o++) row += std::fabs(m[(size_t)r * k + o]);
            best = std::max(best, row);
        }
        return best;
    };
    auto to_double = [](const std::vector<S> &m) {
        std::vector<double> d(m.size());
        for (size_t e = 0; e < m.size(); e++) d[e] = table_to_double<S>(m[e]);
        return d;
    };
    const std::vector<double> A0 = to_double(tab.A[0]);
    double bound = norm(A0);
    if (n == 2) {
        double chained = 0.0;
        for (int v : {0, 2}) {       // the tiles whose entering causal carry is dropped: interior ones and the last one
            const std::vector<double> W = to_double(tab.Wm(v, 0, 1));
            std::vector<double> WA((size_t)k * k, 0.0);
            for (int r = 0; r < k; r++)
                for (int o = 0; o < k; o++)
                    for (int m = 0; m < k; m++) WA[(size_t)r * k + o] += W[(size_t)r * k + m] * A0[(size_t)m * k + o];
            chained = std::max(chained, norm(WA));
        }
        bound = std::max(bound, chained + norm(to_double(tab.A[1])));
    }
    return bound;
}

// ---- geometry ------------------------------------------------------------------------------------------------------
// How the fused kernels tile the plan's image: decided from the description alone.  fused_geometry allocates nothing and
// leaves the plan as it is.
struct FusedGeometry {
    const char *error = nullptr;         // non-null: a shape the kernels cannot tile (RF_ERR_UNSUPPORTED)
    int K = 0;                           // feedback order the kernels run both dimensions at
    bool chained = false;                // 1-D signal folded into chained rows
    int64_t N1 = 0;                      // chained: the length the kernels see
    bool in_place_tail = false, padded = false;
    bool batch = false;                  // Tuple planes ride in one launch per step
    int np = 1;                          // planes the steps run for (batched planes are inside Lx / Ly already, NZ)
    bool rows_sharded = false, y_is_exchange_dim = false, y_sharded = false;
    int64_t NX = 0, NY = 0, NZ = 1;
    int nx = 0, ny = 0;                  // scans along x / y
    int TY = 0, MX = 0, MY = 0;          // tile height, tiles per row / column
    int TVx = 0, TVy = 0;                // samples / rows of the last tile
    int64_t NXP = 0, NYP = 0;            // padded width / height
    int64_t Lx = 0, Ly = 0;              // lines of the x / y carry stage
};

template <typename P>
FusedGeometry fused_geometry(const rf_plan *plan) {
    using Acc = typename PixelTraits<P>::Acc;
    FusedGeometry g;
    const int K = fused_order(plan);
    const bool chained = plan->ndim == 1;        // 1-D signal folded into chained rows
    const DimInfo &dx = plan->dims[0];
    const DimInfo no_y;
    const DimInfo &dy = chained ? no_y : plan->dims[1];
    const int64_t N1 = chained ? chained_padded_length(dx.N) : dx.N;     // chained: the length the kernels see
    // ... and whether they run on zero-padded COPIES (an epilogue that re-reads the input, RF_PAD_COPIES=1 for A/B runs) or on
    // the caller's buffers with the samples behind the signal's end masked (FusedArgs::lin_limit: no copy in, no copy out --
    // 34 us of 98 for one biquad over 10,000,000 samples)
    static const bool pad_copies_env = RF_KNOB("RF_PAD_COPIES") != nullptr;
    const bool in_place_tail = chained && N1 != dx.N && !pad_copies_env && !(plan->pw.post && plan->pw.post_i != 0.0);
    const bool padded = chained && N1 != dx.N && !in_place_tail;
    const int64_t NX = chained ? chained_row_length(N1) : dx.N;
    // Tuple planes of a 2-D filter ride in ONE launch per step, as the z planes of a volume whose planes are separate
    // buffers (FusedArgs::plane_batch): 5 launches instead of 5 per plane, which is most of the time of a small RGB image.
    const bool batch = plan->ndim == 2 && plan->n_planes > 1 && plan->n_planes <= kFusedMaxPlanes && !plan->sharded() &&
                       !(plan->flags & RF_PLAN_NO_PLANE_BATCH) && RF_KNOB("RF_NO_PLANE_BATCH") == nullptr;
    const int64_t NY = chained ? N1 / NX : dy.N, NZ = batch ? plan->n_planes : (plan->ndim > 2 ? plan->dims[2].N : 1);
    // tile height: 64 rows unless only 32 divides the height; any other height runs 64-row tiles (32 below 33 rows)
    // with a partial last tile row
    // (row shards: decided on the slabs' common divisor, so that every rank tiles alike)
    const bool rows_sharded = plan->ndim == 2 && plan->sharded();
    const int64_t NYB = rows_sharded ? plan->shard_common : NY;
    int TY = (NYB % 64 == 0) ? 64 : (NYB % 32 == 0 || NYB < 32) ? 32 : 64;
    // a small image has too few 256 x 64 tiles to fill 256 CUs: half-height tiles double the workgroups
    // (2048^2: 43.5 -> 40.8 us, 1024^2: 38 -> 34.6 us; at 4096^2, 1024 tiles, the 64-row tiles win again)
    // (order 3 keeps 64 rows when 32-row tiles would be more than 64 per column: its carry scan along y then runs in two
    //  blocks -- 2112^2: 28 against 17 us, 80.7 against 75.1 us per filter, tools/mid_probe.py)
    if (TY == 64 && NY % 32 == 0 && !rows_sharded && ((NX + kFusedTX - 1) / kFusedTX) * (NY / 64) * NZ <= 384 &&
        !(K >= 3 && NY / 32 > 64))
        TY = 32;
    // ... and a mid-size image whose height is not a multiple of 64 runs the EDGE variants of its kernels either way: 32-row
    // tiles then waste less of the partial last tile row and cost the EDGE final pass less (tools/ty_probe.py, 64 -> 32 rows:
    // 5000^2 order 2 0.127 -> 0.123 ms, order 3 0.175 -> 0.156; 6000 x 8000 0.181 -> 0.172 / 0.234 -> 0.224; from ~4000 tiles
    // on the 64-row tiles are ahead again: 9000 x 12000 0.330 against 0.358)
    if (TY == 64 && NY % 64 != 0 && NY >= 32 && !rows_sharded && !chained &&
        ((NX + kFusedTX - 1) / kFusedTX) * ((NY + 63) / 64) * NZ <= 3200)
        TY = 32;
    // ... except at order 3 with 65..128 32-row tiles per column, where the y carry scan leaves its register-resident form
    // (kernels_carry.hip): 64-row tiles with a partial last row are ahead there (2160 x 3840: 74 against 85 us, 3000 x 4000:
    // 98 / 110, 4000^2: 112 / 123; above 128 tiles per column the 32-row tiles win again, 5000^2: 157 / 175 us)
    if (TY == 32 && K >= 3 && !rows_sharded && !chained && NY >= 64 && (NY + 31) / 32 > 64 && (NY + 31) / 32 <= 128)
        TY = 64;
    // Large images: 128-row tiles halve the y tails and the kernels that walk them between the passes; the final pass
    // takes such a tile through the LDS in two halves and keeps its columns in registers (kernels_fused_tall.hip).
    // Needs enough of them to fill the chip several times over (row shards: whole 128-row tiles per slab).  A height that is
    // not a multiple of 128 leaves a partial last tile row, which the final pass runs as a strip of its own on the EDGE
    // variant (kernels_fused_tall.hip): 16380 x 16384, 0.70 ms on 64-row tiles with the EDGE kernel everywhere.
    const int nx_early = (int)dx.scan_ids.size(), ny_early = (int)dy.scan_ids.size();
    // (end of round 2, same box, 64 against 128 rows: order 1, cfg4a 1.660 -> 1.636 ms, one bicubic plane 0.593 -> 0.575; order 2,
    // cfg3 0.624 -> 0.601; order 3, cfg4b 2.25 -> 1.87 ms; below ~4096 tiles -- cfg2, 8192^2 -- the 64-row tiles stay ahead)
    // (integer pixels keep 64 rows: their final pass needs more registers than the 128-sample column leaves)
    if ((TY == 64 || (TY == 32 && NY >= 4096)) && !chained && ny_early > 0 && nx_early > 0 && !PixelTraits<P>::is_integer &&
        (NYB % 128 == 0 || !rows_sharded) &&
        !(plan->pw.post && plan->pw.post_i != 0.0 && K <= 2) &&     // (orders 1, 2: an epilogue with an input operand keeps the input
                                                                    // column in registers, which a 128-sample column leaves no room for)
        RF_KNOB("RF_NO_TALL_TILES") == nullptr &&
        ((NX + kFusedTX - 1) / kFusedTX) * ((NY + 127) / 128) * NZ >= 4096)
        TY = 128;
    if (const int want = plan->fused_tile_rows() ? plan->fused_tile_rows() : RF_KNOB("RF_FUSED_TY") ? atoi(RF_KNOB("RF_FUSED_TY")) : 0) {
        // RF_PLAN_TILE_ROWS(n): the caller's tile height, where the shape admits it
        if (want == 32 || want == 64 || (want == 128 && !chained && (!rows_sharded || NYB % 128 == 0))) TY = want;
    }
    // scans in mod form (plan.cpp, "clamped sections"): whole tile rows, so that a modification sits at compile-time rows of
    // the column (fused_plan_applicable has checked that 32 divides the height)
    if (plan->mod_form && ny_early > 0)
        while (TY > 32 && NY % TY != 0) TY /= 2;
    // f64 pixels: a 256 x 32 tile is the 64 KiB of LDS a 256 x 64 tile of f32 takes (any height: partial last tile row)
    if (sizeof(Acc) == 8) {
        if (rows_sharded && NYB % 32 != 0) { g.error = "row-sharded f64 slabs must be multiples of 32 rows"; return g; }
        TY = 32;
    }
    const int nx = (int)dx.scan_ids.size(), ny = (int)dy.scan_ids.size();
    // The width only has to be a multiple of 4 (rows stay 16-byte aligned): the last tile of a row may be partial.  Its
    // missing samples are loaded as zeros and never stored; the tables of the "last tile" variants are built for the
    // samples that exist (tables.h, T_last), so a clamped anticausal scan enters at the true image border.
    // The height is arbitrary: the last tile row may be partial in the same way (rows loaded as zeros, never stored,
    // an anticausal y scan enters at the last existing row).
    const int MX = (int)((NX + kFusedTX - 1) / kFusedTX), MY = (int)((NY + TY - 1) / TY);
    const int TVx = (int)(NX - (int64_t)(MX - 1) * kFusedTX);      // samples of the last tile, (0, 256]
    const int TVy = (int)(NY - (int64_t)(MY - 1) * TY);            // rows of the last tile row, (0, TY]
    const int64_t NXP = (int64_t)MX * kFusedTX;                     // padded width: pitch of everything indexed by column
    const int64_t NYP = (int64_t)MY * TY;                           // padded height: pitch of everything indexed by row
    const int64_t Lx = NYP * NZ, Ly = NXP * NZ;
    const int outer = plan->ndim - 1;
    const bool y_is_exchange_dim = (outer == 1);
    const bool y_sharded = y_is_exchange_dim && plan->sharded();
    g.K = K; g.chained = chained; g.N1 = N1; g.in_place_tail = in_place_tail; g.padded = padded;
    g.batch = batch; g.np = batch ? 1 : plan->n_planes;
    g.rows_sharded = rows_sharded; g.y_is_exchange_dim = y_is_exchange_dim; g.y_sharded = y_sharded;
    g.NX = NX; g.NY = NY; g.NZ = NZ; g.nx = nx; g.ny = ny;
    g.TY = TY; g.MX = MX; g.MY = MY; g.TVx = TVx; g.TVy = TVy;
    g.NXP = NXP; g.NYP = NYP; g.Lx = Lx; g.Ly = Ly;
    return g;
}

// ---- tables --------------------------------------------------------------------------------------------------------
// Host tables of both dimensions, their uploads, and which dimensions take the neighbour form.
template <typename S, typename Acc>
struct FusedTables {
    CarryStage<S, Acc> x, y;                         // W / A / A^C and the GenericDimArgs of the two carry stages
    std::vector<FusedScan<Acc>> xs, ys;              // the scans as FusedArgs carries them
    const Acc *G = nullptr;                          // G_x (device)
    const Acc *Hx = nullptr, *Hy = nullptr;          // tail responses (device)
    const Acc *AMx = nullptr, *AMSx = nullptr;       // per x scan A^MX and (A^MX)^chain_S (device): the row chain of chained rows
    int chain_S = 1;                                 // rows per lane of the row-chain kernel
    bool nb_x = false, nb_y = false;                 // neighbour-form carries (neighbour_carry_bound)
    bool row_scans = false;                          // the row-scan form of the neighbour-form step (fused_tables)
    bool nb_x_pair() const { return nb_x && x.n == 2; }
    bool nb_y_pair() const { return nb_y && y.n == 2; }
};

template <typename P, typename S>
int fused_tables(rf_plan *plan, const FusedGeometry &g, FusedTables<S, typename PixelTraits<P>::Acc> &t) {
    using Acc = typename PixelTraits<P>::Acc;
    using Options = typename CarryStage<S, Acc>::Options;
    int status = RF_OK;
    const int K = g.K, nx = g.nx, ny = g.ny;
    const DimInfo &dx = plan->dims[0];
    const DimInfo no_y;
    const DimInfo &dy = g.chained ? no_y : plan->dims[1];
    auto up = [&](const auto &vec) {
        using T = typename std::decay<decltype(vec)>::type::value_type;
        return (const T *)plan->upload(vec.data(), vec.size() * sizeof(T), &status);
    };
    for (int id : dx.scan_ids) t.xs.push_back(make_fused_scan<S, Acc>(plan->scans[id], K, true));
    for (int id : dy.scan_ids) t.ys.push_back(make_fused_scan<S, Acc>(plan->scans[id], K, false));
    // neighbour-form carries (neighbour_carry_bound): f32 images and batched Tuple planes, unsharded, not chained rows, not in
    // mod form (a 3-D plan's x/y stage keeps its scans); the bound is reported whatever RF_PLAN_FULL_CARRY_SCAN says
    // (f32 arithmetic: 16-bit float storage types take the same decision as the f32 plan of the same description)
    const bool neighbour_plan = is_f32_arith<P>::value && plan->ndim == 2 && !plan->sharded() && !g.chained && !plan->mod_form;
    double nb_bound_x = -1.0, nb_bound_y = -1.0;
    t.chain_S = (int)((g.NY + 63) / 64);
    Options ox, oy;
    ox.T_last = g.TVx;
    ox.apply_powers = g.chained;                                     // (carry_apply runs for chained rows and row shards only)
    oy.T_last = g.TVy;
    oy.sharded = g.y_sharded;
    oy.slab_powers = oy.apply_powers = g.y_sharded;                  // [j][slab][K x K], for the per-scan exchange
    if (int rc = t.x.init(plan, dx.scan_ids, "x", K, kFusedTX, g.MX, LineGeom{g.NX, 1, g.Lx}, ox)) return rc;
    if (int rc = t.y.init(plan, dy.scan_ids, "y", K, g.TY, g.MY, LineGeom{g.NY, g.NXP, g.Ly}, oy)) return rc;
    std::vector<Acc> hHx, hHy, hG, hAMx, hAMSx;
    if (nx > 0) {
        const DimTables<S> &tx = t.x.tab;
        // segment tables as the x phase reads them (float pixels: exact values of the kernel constants)
        std::vector<double> sr, sp;
        for (const auto &f : t.xs) {
            for (int p = 0; p < kFusedSeg; p++)
                for (int j = 0; j < K; j++) sr.push_back((double)f.R[j][f.causal ? p : kFusedSeg - 1 - p]);
            for (int step = 0; step < 4; step++)
                for (int r = 0; r < K; r++)
                    for (int j = 0; j < K; j++) sp.push_back((double)f.P[step][r][j]);
        }
        plan->tables["seg_R_x"] = sr;
        plan->tables["seg_P_x"] = sp;
        if (neighbour_plan) nb_bound_x = neighbour_carry_bound<S>(tx, dx.scan_ids, plan);
        hHx = table_for_kernels<S, Acc>(plan, build_tail_responses<S>(tx.scans, K, kFusedTX, plan->clamped, g.TVx), "H_x");
        hAMx.assign((size_t)nx * K * K, Acc(0));
        hAMSx.assign((size_t)nx * K * K, Acc(0));
        for (int s = 0; s < nx; s++) {
            std::vector<S> am = mat_pow<S>(tx.A[s], g.MX, K);
            std::vector<S> ams = mat_pow<S>(am, t.chain_S, K);
            for (int e = 0; e < K * K; e++) {
                hAMx[(size_t)s * K * K + e] = table_to_acc<S, Acc>(am[e]);
                hAMSx[(size_t)s * K * K + e] = table_to_acc<S, Acc>(ams[e]);
            }
        }
        // G[v][q][o][xi]: what the carry entering x scan q adds to the tile after ALL x scans
        hG.assign((size_t)4 * nx * kFusedTX * K, Acc(0));
        std::vector<double> dG(hG.size());
        for (int v = 0; v < 4; v++)
            for (int q = 0; q < nx; q++) {
                const std::vector<S> &Pm = tx.P(v, q, nx - 1);          // [xi][o]
                for (int xi = 0; xi < kFusedTX; xi++)
                    for (int o = 0; o < K; o++) {
                        size_t idx = (((size_t)v * nx + q) * K + o) * kFusedTX + xi;
                        hG[idx] = table_to_acc<S, Acc>(Pm[(size_t)xi * K + o]);
                        dG[idx] = table_to_double<S>(Pm[(size_t)xi * K + o]);
                    }
            }
        plan->tables["G_x"] = dG;
    }
    if (ny > 0) {
        if (neighbour_plan) nb_bound_y = neighbour_carry_bound<S>(t.y.tab, dy.scan_ids, plan);
        hHy = table_for_kernels<S, Acc>(plan, build_tail_responses<S>(t.y.tab.scans, K, g.TY, plan->clamped, g.TVy), "H_y");
    }
    t.G = up(hG); t.Hx = up(hHx); t.Hy = up(hHy); t.AMx = up(hAMx); t.AMSx = up(hAMSx);

    // Which dimensions take the neighbour form.  x: one scan needs nothing but the tails pass 1 left; a pair is completed by
    // xscan_rows (kernels_tails.hip, NB), which runs only with y scans in the filter.  y: one scan likewise; a pair needs the
    // final pass to add W * (the tile's own causal tail) to the anticausal carry it loads (FusedArgs::y_nb_W), which the
    // 128-row final pass does (kernels_fused_tall.hip).
    const bool full_scan = (plan->flags & RF_PLAN_FULL_CARRY_SCAN) != 0;
    t.nb_x = !full_scan && nb_bound_x >= 0.0 && nb_bound_x <= kNeighbourCarryBound && (nx == 1 || ny > 0);
    t.nb_y = !full_scan && nb_bound_y >= 0.0 && nb_bound_y <= kNeighbourCarryBound && (ny == 1 || g.TY == 128);
    // (every dropped transfer crosses a whole tile: neighbour_plan admits unsharded plans only, which hold both borders of both
    // dimensions, so the only partial tile is a last one and the causal carry leaving it is never consumed)
    plan->tables["neighbour_carries"] = {nb_bound_x, t.nb_x ? 1.0 : 0.0, nb_bound_y, t.nb_y ? 1.0 : 0.0};

    // The row-scan form of the neighbour-form step.  With both dimensions in neighbour form nothing between the two passes runs a
    // recurrence across tiles, and what xscan_rows still does needs no launch that walks the y tails: the tile-local x scans of a
    // tile's combined rows depend on that tile alone -- pass 1 runs them while it holds the rows (kernels_tails_mfma.hip, RS) --
    // and the residual is a rank nx * K update per tile, which the final pass adds to the three tails it loads, as it completes
    // its x carries from the raw tails (kernels_fused_tall.hip, RS).  The middle launch shrinks to the contraction tau
    // (kernels_tails.hip, xtau_kernel): it reads the x tails once and writes 64 bytes per tile, into the allocation that is
    // xt_done otherwise.  Taken exactly where pass 1 is mfma_tails_kernel and the final pass the lean 128-row kernel on what the
    // headline workload runs: f32 planes on both sides, order 2, the pair in x and in y, whole 256 x 128 tiles, no pointwise
    // stage; RF_PLAN_SEPARATE_ROW_SCANS keeps the three kernels of the neighbour form.
    if constexpr (std::is_same<P, float>::value) {
        const int mfma_mode = (plan->flags & RF_PLAN_MFMA_PASS1) ? 1 : (plan->flags & RF_PLAN_STAGED_PASS1) ? -1 : 0;
        const int stream_mode = (plan->flags & RF_PLAN_STREAM_PASS1) ? 1 : (plan->flags & RF_PLAN_STAGED_PASS1) ? -1 : 0;
        t.row_scans = !(plan->flags & RF_PLAN_SEPARATE_ROW_SCANS) && t.nb_x_pair() && t.nb_y_pair() && K == 2 && g.TY == 128 &&
                      g.TVx == kFusedTX && g.TVy == 128 && !plan->pw.in_u8 && !plan->pw.out_u8 && !plan->pw.pre && !plan->pw.post &&
                      !g.padded && !g.in_place_tail && t.xs[0].causal != 0 && t.xs[1].causal == 0 && t.ys[0].causal != 0 && t.ys[1].causal == 0 &&
                      !stream_tails_applicable(K, g.TY, false, 0, g.TVx, g.TVy, (int64_t)g.MX * g.MY * g.NZ, g.MX, g.NZ, nx * K, ny * K, stream_mode) &&
                      mfma_tails_applicable(K, g.TY, false, 0, g.TVx, g.TVy, 0, nx, ny, mfma_mode);
    }
    plan->tables["row_scans"] = {t.row_scans ? 1.0 : 0.0};
    return status;
}

// ---- device memory -------------------------------------------------------------------------------------------------
template <typename Acc>
struct FusedBuffers {
    Acc *xt = nullptr, *yt = nullptr;                // tile-local tails, completed in place by the carry stages
    Acc *xt_done = nullptr;                          // the completed x tails where xscan_rows writes them (merged_cx, nb_x_pair)
    Acc *xin = nullptr, *yin = nullptr;              // entering carries
    Acc *row_exit = nullptr;                         // chained rows: the rows' exit states
    size_t xt_pp = 0, yt_pp = 0, xin_pp = 0, yin_pp = 0;     // elements per plane
    bool merged_cx = false;                          // xscan_rows completes the x tails itself (kernels_tails.hip, XC)
};

template <typename S, typename Acc>
int fused_buffers(rf_plan *plan, const FusedGeometry &g, FusedTables<S, Acc> &t, FusedBuffers<Acc> &b) {
    int status = RF_OK;
    const int K = g.K, np = g.np;
    b.xt_pp = (size_t)g.nx * g.MX * K * g.Lx; b.yt_pp = (size_t)g.ny * g.MY * K * g.Ly;
    b.xin_pp = (size_t)g.nx * K * g.Lx; b.yin_pp = (size_t)g.ny * K * g.Ly;
    // few tiles per row: xscan_rows completes the x tails itself, into a second array (kernels_tails.hip, XC)
    // (the neighbour form needs no recurrence at all: it takes such images too -- 2-4 µs per step ahead of XC on 1280^2 x 3 ...
    //  4096^2, orders 1-3, profiles/r7/xc_vs_nb.txt)
    b.merged_cx = !g.chained && !t.nb_x && xscan_completes_x_tails(K, g.TY, g.MX, g.nx, g.ny, sizeof(Acc), (int64_t)g.MY * g.NZ);
    b.xt = (Acc *)plan->alloc(b.xt_pp * np * sizeof(Acc), false, &status);
    b.xt_done = (b.merged_cx || t.nb_x_pair()) ? (Acc *)plan->alloc(b.xt_pp * np * sizeof(Acc), false, &status) : nullptr;
    b.yt = (Acc *)plan->alloc(b.yt_pp * np * sizeof(Acc), false, &status);
    b.xin = (Acc *)plan->alloc(b.xin_pp * np * sizeof(Acc), true, &status);
    b.yin = (Acc *)plan->alloc(b.yin_pp * np * sizeof(Acc), true, &status);
    // (two of them: with the chain of scan s folded into the carry launch of scan s + 1 that launch reads one and writes the other)
    b.row_exit = g.chained ? (Acc *)plan->alloc((size_t)2 * K * g.Lx * np * sizeof(Acc), true, &status) : nullptr;
    t.x.use_buffers(b.xt, b.xt_pp, b.xin, b.xin_pp);
    t.y.use_buffers(b.yt, b.yt_pp, b.yin, b.yin_pp);
    return status;
}

// ---- 3-D volumes: pass 1 in ONE read (kernels_tails_walk.hip) ------------------------------------
// The z tails are taken from the raw input by the pass that extracts the x/y tails (the z operators commute with the x/y
// filter: plan_strided.h); the z stage then has no first pass.  f32 volumes of whole tiles without a prologue (its bias is not
// linear) -- whole
// volumes, and z slabs that take the early exchange (the pass is then the slab's begin step) -- of at least one patch column (256 x 32 samples x one z tile: a workgroup of 1024 threads) per compute unit --
// measured, one read against two: 256^3 (32 patch columns) 0.214 against 0.124 ms, 512^3 (256) 0.645 against 0.680,
// 768^3 1.97 / 2.05, 1024^3 4.5 / 4.95, 2048^3 34.0 / 37.0 (profiles/r4/walk_tails_sizes.txt); RF_PLAN_WALK_PASS1: whatever
// the size; RF_PLAN_STAGED_PASS1 keeps the two first passes.
struct FusedWalk {
    WalkArgs args{};
    std::shared_ptr<WalkHook> hook;              // null: pass 1 does not walk
    std::unique_ptr<rf_plan> child;              // F over the z carry planes (plan_strided.h), handed to the z stage
};

template <typename P, typename S>
int plan_walk_pass1(rf_plan *plan, const rf_filter_desc *desc, const FusedGeometry &g,
                    const FusedBuffers<typename PixelTraits<P>::Acc> &b, FusedWalk &w) {
    using Acc = typename PixelTraits<P>::Acc;
    int status = RF_OK;
    if constexpr (std::is_same<P, float>::value) {
        const int K = g.K, TY = g.TY, nx = g.nx, ny = g.ny, np = g.np;
        static const char *walk_knob = RF_KNOB("RF_WALK");                        // A/B: 0 = never
        const bool wanted = !(plan->flags & RF_PLAN_STAGED_PASS1) && !(walk_knob && atoi(walk_knob) == 0);
        const bool z_slabs = plan->sharded();           // z slabs: with the early exchange (plan_strided.h), whose first step this pass then is
        if (!(wanted && plan->ndim == 3 && (!z_slabs || early_exchange_possible<P>(plan, 2, desc)) && !g.batch && !g.chained && !plan->mod_form &&
              !plan->pw.in_u8 && nx > 0 && ny > 0 && !plan->dims[2].scan_ids.empty() &&      // (a prologue x' = s x + b is applied as the samples arrive; an epilogue runs behind the z stage either way)
              plan->dims[2].lines == g.NX * g.NY))
            return status;
        const DimInfo &dz = plan->dims[2];
        const int TZ = strided_tile(plan, 2), nz = (int)dz.scan_ids.size(), KZ = dz.k;
        const int64_t patch_columns = TZ > 0 ? (int64_t)g.MX * ((g.NY + 31) / 32) * (dz.N / TZ) : 0;
        // (widths that are not multiples of four: the pass takes them since round 6 -- 4-byte loads, kernels_tails_walk.hip U4 --
        //  but loses to the two first passes there, 1024 x 1021 x 1021: walk 2.27 ms against 1.15 + 0.94, 1022 wide: 2.09 against
        //  1.13 + 1.04 (profiles/r6/walk_odd_widths.txt); only RF_PLAN_WALK_PASS1 selects it for such volumes)
        if (!(TZ > 0 && dz.N % TZ == 0 && walk_tails_applicable(K, TY, nx, ny, nz, KZ, TZ, g.TVx, g.TVy) &&
              ((patch_columns >= 256 && g.NX % 4 == 0) || (plan->flags & RF_PLAN_WALK_PASS1))))
            return status;
        const int MZ = (int)(dz.N / TZ);
        w.child.reset(build_carry_planes_plan(plan, desc, 2, (int64_t)nz * KZ * (MZ + (z_slabs ? 1 : 0))));
        if (!w.child) return status;
        // impulse responses of the z tails, transposed: [variant][z][4]
        std::vector<ScanS<S>> zs;
        for (int id : dz.scan_ids) zs.push_back(make_table_scan<S>(plan->scans[id]));
        const std::vector<Acc> H = table_for_kernels<S, Acc>(plan, build_tail_responses<S>(zs, KZ, TZ, plan->clamped), "H_z");
        std::vector<float> hHz((size_t)4 * TZ * 4, 0.0f);
        for (int v = 0; v < 4; v++)
            for (int j = 0; j < nz * KZ; j++)
                for (int z = 0; z < TZ; z++)
                    hHz[((size_t)v * TZ + z) * 4 + j] = H[((size_t)v * nz * KZ + j) * TZ + z];
        // tall patches (128 columns x 64 rows, round 6): 128-row y tiles, at most four x tails
        static const bool tall_off = RF_KNOB("RF_WALK_NO_TALL") != nullptr;       // A/B
        const bool tall = !tall_off && TY == 128 && K <= 2 && nx * K <= 4;
        const int parts = tall ? TY / 64 : TY / 32;
        w.args.tall = tall ? 1 : 0;
        w.args.xt2 = tall ? (float *)plan->alloc(b.xt_pp * np * sizeof(float), false, &status) : nullptr;      // (per Tuple plane)
        w.args.HzT = (const float *)plan->upload(hHz.data(), hHz.size() * sizeof(float), &status);
        w.args.TY = TY; w.args.TZ = TZ; w.args.MZ = MZ; w.args.nzk = nz * KZ; w.args.KZ = KZ;
        w.args.parts_log2 = parts == 4 ? 2 : parts == 2 ? 1 : 0;
        w.args.z_first_border = (!z_slabs || plan->shard_rank == 0) ? 1 : 0;
        w.args.z_last_border = (!z_slabs || plan->shard_rank == plan->shard_world - 1) ? 1 : 0;
        w.args.part_stride = (int64_t)b.yt_pp;
        w.args.ytp = parts > 1 ? (float *)plan->alloc(b.yt_pp * parts * np * sizeof(float), false, &status) : nullptr;      // (per Tuple plane)
        w.hook = std::make_shared<WalkHook>();
    }
    return status;
}

// ---- steps ---------------------------------------------------------------------------------------------------------
// The FusedArgs of a plane.  Steps keep a copy (they outlive the builder).
template <typename Acc>
struct FusedPlaneArgs {
    FusedArgs<Acc> base{};
    FusedBuffers<Acc> b;
    bool batch = false;
    FusedArgs<Acc> operator()(const rf_plan *plan, int pl) const {
        FusedArgs<Acc> a = base;
        a.xt = b.xt + (size_t)pl * b.xt_pp;
        a.yt = b.yt + (size_t)pl * b.yt_pp;
        if (a.ytp != nullptr) a.ytp = a.ytp + (size_t)pl * b.yt_pp * (size_t)a.yt_parts;       // (the parts of the one-read pass 1)
        a.y_incoming = b.yin + (size_t)pl * b.yin_pp;
        a.x_incoming = b.xin + (size_t)pl * b.xin_pp;
        a.plane_batch = batch ? 1 : 0;
        if (batch)
            for (int i = 0; i < plan->n_planes; i++) { a.in_planes[i] = plan->in[i]; a.out_planes[i] = plan->xy_result(i); }
        return a;
    }
};

// What pass 1 needs to choose its kernel
template <typename Acc>
struct Pass1Args {
    int K = 0, TY = 0;
    const Acc *Hx = nullptr, *Hy = nullptr;
    bool padded = false;
    int stream_mode = 0, mfma_mode = 0;
    WalkArgs walk{};
    std::shared_ptr<WalkHook> walk_hook;
    size_t xt_pp = 0;
    bool row_scans = false;      // FusedTables::row_scans: the instance that also scans the combined rows
};

// pass 1: tail extraction by contraction with the impulse responses (kernels_tails.hip)
template <typename P>
int launch_pass1(const rf_plan *plan, int pl, const FusedArgs<typename PixelTraits<P>::Acc> &a,
                 const Pass1Args<typename PixelTraits<P>::Acc> &p) {
    const int K = p.K, TY = p.TY;
    const void *in = p.padded ? plan->pad_in[pl] : plan->in[pl];
    if constexpr (std::is_same<P, float>::value) {
        if (p.row_scans) return launch_mfma_tails_row_scans((const float *)in, a, p.Hx, p.Hy, plan->stream);
        if (p.walk_hook) {
            WalkArgs wa = p.walk;
            wa.zt = p.walk_hook->zt + (size_t)pl * p.walk_hook->zt_stride;
            if (wa.xt2) wa.xt2 += (size_t)pl * p.xt_pp;
            if (wa.ytp) wa.ytp = const_cast<float *>(a.ytp);       // this plane's parts (FusedPlaneArgs)
            else wa.ytp = a.yt;                         // one patch per y tile: the combined rows go where they belong
            return launch_walk_tails(K, (const float *)plan->in[pl], a, wa, p.Hx, p.Hy, plan->stream);
        }
        // images of whole 256 x 64 tiles stream through the LDS-DMA ring (kernels_stream.hip)
        if (a.lin_limit == 0 && stream_tails_applicable(K, TY, plan->pw.in_u8, a.pw_flags, a.last_cols, a.last_rows, (int64_t)a.MX * a.MY * a.NZ, a.MX,
                                        a.NZ, a.nx * K, a.ny * K, p.stream_mode))
            return launch_stream_tails(K, (const float *)in, a, p.Hx, p.Hy, plan->stream);
        // ... other f32 images of whole tiles contract their x tails on the matrix cores (kernels_tails_mfma.hip)
        if (mfma_tails_applicable(K, TY, plan->pw.in_u8, a.pw_flags, a.last_cols, a.last_rows, a.lin_limit, a.nx, a.ny, p.mfma_mode))
            return launch_mfma_tails<float>(K, TY, (const float *)in, a, p.Hx, p.Hy, plan->stream);
    }
    // ... and so do images stored as 16-bit floats (the kernel widens the samples on their way into its f32 tile)
    if constexpr (is_half_pixel<P>::value) {
        if (mfma_tails_applicable(K, TY, false, a.pw_flags, a.last_cols, a.last_rows, a.lin_limit, a.nx, a.ny, p.mfma_mode, true))
            return launch_mfma_tails<P>(K, TY, (const P *)in, a, p.Hx, p.Hy, plan->stream);
    }
    return launch_fused_tails<P>(K, TY, in, plan->pw.in_u8, a, p.Hx, p.Hy, plan->stream);
}

// The step adders of one fused plan.  Every step captures COPIES of what it needs (plain structs of pointers and integers),
// never the builder: the steps run long after build_fused has returned.
template <typename P, typename S>
struct FusedBuilder {
    using Acc = typename PixelTraits<P>::Acc;
    rf_plan *plan = nullptr;
    const rf_filter_desc *desc = nullptr;
    FusedGeometry g;
    FusedTables<S, Acc> t;
    FusedBuffers<Acc> b;
    FusedWalk walk;
    FusedPlaneArgs<Acc> fargs;
    const Acc *d_Yapply = nullptr;       // row shards: the merged exchange's correction, applied by pass 2 (FusedArgs::y_apply)

    void set_plane_args() {
        const int K = g.K, nx = g.nx, ny = g.ny, TY = g.TY;
        const bool walks = (bool)walk.hook;
        FusedArgs<Acc> &fbase = fargs.base;
        fbase.NX = g.NX; fbase.NY = g.NY; fbase.NZ = g.NZ; fbase.MX = g.MX; fbase.MY = g.MY; fbase.nx = nx; fbase.ny = ny;
        fbase.NXP = g.NXP; fbase.last_lane = (g.TVx - 1) / kFusedSeg; fbase.last_cols = g.TVx;
        fbase.NYP = g.NYP; fbase.last_rows = g.TVy;
        fbase.row_bytes = (uint32_t)(g.NX * (int64_t)sizeof(P));
        fbase.clamped = plan->clamped ? 1 : 0;
        fbase.mod_form = plan->mod_form ? 1 : 0;
        fbase.y_first_border = (!g.y_sharded || plan->shard_rank == 0) ? 1 : 0;
        fbase.y_last_border = (!g.y_sharded || plan->shard_rank == plan->shard_world - 1) ? 1 : 0;
        if constexpr (!PixelTraits<P>::is_integer) {
            const bool z_follows = plan->ndim > 2 && !plan->dims[2].scan_ids.empty();
            plan->pw.pre_fused = plan->pw.pre;
            plan->pw.post_fused = plan->pw.post && !z_follows;     // with a z stage the epilogue runs after it
            fbase.pw_flags = (plan->pw.pre_fused ? 1 : 0) | (plan->pw.post_fused ? 2 : 0);
            fbase.pre_s = (Acc)plan->pw.pre_s; fbase.pre_b = (Acc)plan->pw.pre_b;
            fbase.post_f = (Acc)plan->pw.post_f; fbase.post_i = (Acc)plan->pw.post_i; fbase.post_b = (Acc)plan->pw.post_b;
        }
        // The y tails of an unsharded plan are tile-major, [tile row][tile column][scan][r][256]: the rows pass 1 stores for
        // one tile, and the ones pass 2 loads, are then one run of ny * K * 1 KiB instead of ny * K runs a whole image width
        // apart (FusedArgs::yt_index).  Slabs keep [scan][tile row][r][line], which the exchange kernels address, and so do
        // order-3 filters: measured on 16384^2, order 2 gains 0.005 ms of 0.62 ms and order 3 loses 0.01-0.03 ms of 1.98 ms
        // (its carry scan reads six rows per tile and line), order 1 is unchanged either way.
        static const bool yt_row_major = RF_KNOB("RF_YT_ROW_MAJOR") != nullptr;      // A/B runs
        static const bool yt_force_tile = RF_KNOB("RF_YT_TILE_MAJOR") != nullptr;    // A/B runs: order 3 too
        // (the one-read pass 1 of a volume stores a tile's combined rows as one run: tile-major for order 3 as well)
        const bool yt_tile_major = !yt_row_major && !g.y_sharded && ny > 0 && (K <= 2 || yt_force_tile || walks) && g.Ly % kFusedTX == 0 &&
                                   g.Ly == g.NXP * (int64_t)g.NZ;
        fbase.yt_tile_major = yt_tile_major ? 1 : 0;
        fbase.lin_limit = g.in_place_tail ? plan->dims[0].N : 0;
        if constexpr (std::is_same<P, float>::value) {
            // (pass 1 left the combined rows in parts: xscan_rows adds them up)
            if (walks && walk.args.ytp) { fbase.yt_parts = walk.args.tall ? TY / 64 : TY / 32; fbase.yt_part_stride = walk.args.part_stride; fbase.ytp = walk.args.ytp; }
            if (walk.args.xt2) t.x.dev.tails_part2 = walk.args.xt2;       // (tall patches: the x tails in two parts)
        }
        std::memset(fbase.xs, 0, sizeof(fbase.xs));
        std::memset(fbase.ys, 0, sizeof(fbase.ys));
        for (int s = 0; s < nx; s++) fbase.xs[s] = t.xs[s];
        for (int j = 0; j < ny; j++) {
            fbase.ys[j].causal = t.ys[j].causal;
            fbase.ys[j].b = t.ys[j].b;
            for (int e = 0; e < kFusedMaxK; e++) fbase.ys[j].a[e] = t.ys[j].a[e];
            fbase.ys[j].mod_n = t.ys[j].mod_n;
            for (int e = 0; e < kFusedMaxMod; e++) fbase.ys[j].mod_g[e] = t.ys[j].mod_g[e];
        }
        fargs.b = b;
        fargs.batch = g.batch;
        t.y.dev.base.tile_major = fbase.yt_tile_major;
    }

    int add_pass1() {
        int status = RF_OK;
        rf_plan *const plan = this->plan;
        Pass1Args<Acc> p1a;
        p1a.K = g.K; p1a.TY = g.TY; p1a.Hx = t.Hx; p1a.Hy = t.Hy; p1a.padded = g.padded;
        p1a.stream_mode = (plan->flags & RF_PLAN_STREAM_PASS1) ? 1 : (plan->flags & RF_PLAN_STAGED_PASS1) ? -1 : 0;
        p1a.mfma_mode = (plan->flags & RF_PLAN_MFMA_PASS1) ? 1 : (plan->flags & RF_PLAN_STAGED_PASS1) ? -1 : 0;
        p1a.walk = walk.args; p1a.walk_hook = walk.hook; p1a.xt_pp = b.xt_pp;
        p1a.row_scans = t.row_scans;
        Step p1;
        p1.name = walk.hook ? "walk_tails" : "fused_tails";
        p1.run = [plan, fargs = this->fargs, p1a](int pl) { return launch_pass1<P>(plan, pl, fargs(plan, pl), p1a); };
        if (g.padded) {
            // the zero-padded copies the kernels run on (the padding of the input copy is written once, here, and never again)
            plan->padded_len = g.N1;
            const size_t user_bytes = (size_t)plan->dims[0].N * sizeof(P);
            for (int pl = 0; pl < plan->n_planes; pl++) {
                plan->pad_in[pl] = plan->alloc((size_t)g.N1 * sizeof(P), true, &status);
                plan->pad_out[pl] = plan->alloc((size_t)g.N1 * sizeof(P), false, &status);
            }
            if (status != RF_OK) return status;
            Step ci;
            ci.name = "pad_copy_in";
            ci.run = [plan, user_bytes](int pl) -> int {
                RF_HIP_CHECK(hipMemcpyAsync(plan->pad_in[pl], plan->in[pl], user_bytes, hipMemcpyDeviceToDevice, plan->stream));
                return (int)RF_OK;
            };
            plan->begin_steps.push_back(ci);
        }
        plan->begin_steps.push_back(p1);
        return status;
    }

    void add_chained_row_carries() {
        // Chained rows: per scan, (1) the blocked carry scan of every row with a zero entering state, publishing the
        // rows' exit states, (2) the chain over the rows -> state entering every row, (3) that state propagated through
        // the row's tails.  The same three steps as a sharded dimension (exchange_local / gather / exchange_apply),
        // with rows in the role of slabs.  Scan s+1 chains on scan s's completed carries, hence scan by scan.
        // Where the rows' entering states fit the LDS the chain and its propagation are not launches of their own: scan s's
        // are done by the carry launch of scan s + 1 before its own scan (carry_block_kernel PRE), the last scan's by
        // chain_apply_kernel -- n + 1 launches for n scans.
        static const bool no_pre = RF_KNOB("RF_NO_CHAIN_PRE") != nullptr;        // A/B runs: chain_apply after every scan
        rf_plan *const plan = this->plan;
        const CarryDev<Acc> cx = t.x.dev;               // (built with Options::apply_powers: chain_apply / carry_apply have their A^i)
        const int K = g.K, nx = g.nx, MX = g.MX, chain_S = t.chain_S;
        const int64_t Lx = g.Lx;
        Acc *const row_exit = b.row_exit, *const xin = b.xin;
        const size_t xin_pp = b.xin_pp;
        const bool one_launch_chain = chain_apply_applies(K, Lx, sizeof(Acc));
        const size_t exit_pp = (size_t)K * Lx;            // one buffer of exit states (two per plane, by scan parity)
        for (int s = 0; s < nx; s++) {
            const bool causal = t.xs[s].causal != 0;
            const bool fold_prev = one_launch_chain && !no_pre && s > 0;
            Step cs;
            cs.name = "carry_x" + std::to_string(s);
            ChainPre<Acc> pre{};
            if (fold_prev) {
                pre.AM = t.AMx + (size_t)(s - 1) * K * K; pre.AMS = t.AMSx + (size_t)(s - 1) * K * K;
                pre.Apow = cx.base.Apow + (size_t)(s - 1) * MX * K * K;
                pre.S = chain_S; pre.causal_prev = t.xs[s - 1].causal != 0 ? 1 : 0;
            }
            cs.run = [plan, cx, K, s, row_exit, exit_pp, xin, xin_pp, Lx, pre, fold_prev](int pl) {
                Acc *mine = row_exit + ((size_t)pl * 2 + (s & 1)) * exit_pp;
                if (!fold_prev)
                    return launch_carry_block<Acc>(K, cx.args(pl), cx.causal_mask, s, s + 1, mine, cx.AC, cx.C, plan->stream);
                ChainPre<Acc> p = pre;
                p.exit_states = row_exit + ((size_t)pl * 2 + ((s - 1) & 1)) * exit_pp;
                p.incoming_prev = xin + (size_t)pl * xin_pp + (size_t)(s - 1) * K * Lx;
                return launch_carry_block<Acc>(K, cx.args(pl), cx.causal_mask, s, s + 1, mine, cx.AC, cx.C, plan->stream, &p);
            };
            plan->begin_steps.push_back(cs);
            const Acc *AMs = t.AMx + (size_t)s * K * K, *AMSs = t.AMSx + (size_t)s * K * K;
            if (one_launch_chain) {
                if (!no_pre && s + 1 < nx) continue;          // the next scan's carry launch finishes this one
                // the chain over the rows and the propagation through their tails in one launch (kernels_carry.hip)
                Step ca;
                ca.name = "chain_apply" + std::to_string(s);
                ca.run = [plan, cx, K, s, causal, row_exit, exit_pp, xin, xin_pp, Lx, AMs, AMSs, chain_S](int pl) {
                    Acc *inc = xin + (size_t)pl * xin_pp + (size_t)s * K * Lx;
                    return launch_chain_apply<Acc>(K, cx.args(pl), s, row_exit + ((size_t)pl * 2 + (s & 1)) * exit_pp, inc, causal, AMs,
                                                   AMSs, chain_S, plan->stream);
                };
                plan->begin_steps.push_back(ca);
                continue;
            }
            Step rc;
            rc.name = "row_chain" + std::to_string(s);
            rc.run = [plan, K, s, causal, row_exit, exit_pp, xin, xin_pp, Lx, AMs, AMSs, chain_S](int pl) {
                Acc *inc = xin + (size_t)pl * xin_pp + (size_t)s * K * Lx;
                return launch_row_chain<Acc>(K, row_exit + ((size_t)pl * 2 + (s & 1)) * exit_pp, inc, (int)Lx, causal, AMs, AMSs, chain_S,
                                             plan->stream);
            };
            plan->begin_steps.push_back(rc);
            Step ap;
            ap.name = "carry_x_apply" + std::to_string(s);
            ap.run = [plan, cx, s](int pl) { return launch_generic_carry_apply<Acc>(cx.args(pl), s, plan->stream); };
            plan->begin_steps.push_back(ap);
        }
    }

    void add_xscan_rows() {
        // finishes the y tails: tile-local x scans of the combined rows + the cross-dimension residual of the
        // completed x carries (lib/split.cpp:1215-1633)
        rf_plan *const plan = this->plan;
        const int K = g.K, TY = g.TY;
        const bool merged_cx = b.merged_cx, nb_x_pair = t.nb_x_pair();
        const Acc *d_Hy = t.Hy, *d_G = t.G, *d_Wx = t.x.dev.base.W, *d_Ax = t.x.dev.base.A;
        Acc *const xt_done = b.xt_done;
        const size_t xt_pp = b.xt_pp;
        Step xs;
        // (the step keeps its name in the row-scan form, where it launches xtau_kernel and scans no row: the step names of a plan
        //  are what its callers and the suite's launch lists know a neighbour-form step by)
        xs.name = "xscan_rows";
        if constexpr (std::is_same<Acc, float>::value) {
            if (t.row_scans) {
                xs.run = [plan, fargs = this->fargs, d_Hy, d_Wx, xt_done, xt_pp](int pl) {
                    return launch_xtau(fargs(plan, pl), d_Hy, d_Wx, xt_done + (size_t)pl * xt_pp, plan->stream);
                };
                plan->begin_steps.push_back(xs);
                return;
            }
        }
        xs.run = [plan, fargs = this->fargs, K, TY, d_Hy, d_G, merged_cx, nb_x_pair, d_Wx, d_Ax, xt_done, xt_pp](int pl) {
            if (merged_cx)
                return launch_xscan_rows<Acc>(K, TY, fargs(plan, pl), d_Hy, d_G, plan->stream, d_Wx, d_Ax, xt_done + (size_t)pl * xt_pp);
            if (nb_x_pair)      // neighbour form: the x tails completed from the neighbours' (NB)
                return launch_xscan_rows<Acc>(K, TY, fargs(plan, pl), d_Hy, d_G, plan->stream, d_Wx, nullptr, xt_done + (size_t)pl * xt_pp, true);
            return launch_xscan_rows<Acc>(K, TY, fargs(plan, pl), d_Hy, d_G, plan->stream);
        };
        plan->begin_steps.push_back(xs);
    }

    int add_y_carries() {
        if (!g.y_sharded) {   // one launch for every y scan; per-scan launches only around the exchanges
            if (g.ny > 0 && !t.nb_y) t.y.add_local_carry(plan, "carry_y");
            return RF_OK;
        }
        if (merged_exchange_applies(g.ny, g.K, plan->shard_world)) {
            // one all-gather for all y scans (plan_generic.h, "merged exchange")
            // ... whose correction of the tails is left to pass 2 (FusedArgs::y_apply): no launch between gather and pass 2
            static const bool separate_apply = RF_KNOB("RF_SHARD_SEPARATE_APPLY") != nullptr;     // A/B runs
            return add_merged_exchange<S, Acc>(plan, t.y, "carry_y", separate_apply ? nullptr : &d_Yapply);
        }
        return t.y.add_per_scan_carries(plan, "carry_y", "carry_y_apply", true);
    }

    void add_pass2() {
        rf_plan *const plan = this->plan;
        const int K = g.K, TY = g.TY;
        const bool padded = g.padded;
        const Acc *d_Yapply = this->d_Yapply, *d_Ynb = t.nb_y_pair() ? t.y.dev.base.W : nullptr;
        Acc *const xt_done = (b.merged_cx || t.nb_x_pair()) ? b.xt_done : nullptr;
        const size_t xt_pp = b.xt_pp;
        // the row-scan form: the allocation of xt_done holds tau, the x tails stay where pass 1 wrote them
        const bool row_scans = t.row_scans;
        const Acc *d_Xnb = row_scans ? t.x.dev.base.W : nullptr, *d_G = row_scans ? t.G : nullptr;
        Step p2;
        p2.name = "fused_pass2";
        p2.run = [plan, fargs = this->fargs, K, TY, d_Yapply, d_Ynb, padded, xt_done, xt_pp, row_scans, d_Xnb, d_G](int pl) {
            FusedArgs<Acc> a = fargs(plan, pl);
            a.y_apply = d_Yapply;
            a.y_nb_W = d_Ynb;
            if (row_scans) { a.x_nb_W = d_Xnb; a.rs_G = d_G; a.rs_tau = xt_done + (size_t)pl * xt_pp; }
            else if (xt_done) a.xt = xt_done + (size_t)pl * xt_pp;
            if constexpr (is_half_pixel<P>::value) {
                // native 16-bit volume (add_z_stage gave the plan its f32 volume, which only such a plan has): the f32 instances
                // with a 16-bit source, into the volume the z stage reads
                if (plan->mid[pl] != nullptr) {
                    const int kind = std::is_same<P, _Float16>::value ? kSrcF16 : kSrcBF16;
                    a.row_bytes = (uint32_t)(a.NX * (int64_t)sizeof(float));
                    if (TY == 128) return launch_fused_pass2_tall<float>(K, plan->in[pl], kind, (float *)plan->mid[pl], a, plan->stream);
                    return launch_fused_pass2<float>(K, TY, plan->in[pl], kind, (float *)plan->mid[pl], a, plan->stream);
                }
            }
            if constexpr (std::is_same<P, float>::value) {
                // byte planes on both sides (RF_IO_U8; plan.cpp, u8_plan_is_native: an unsharded 2-D image): everything up to
                // here was the RF_IN_U8 plan's, the final pass stores bytes
                // (a byte VOLUME's final x/y pass is the f32 one below, into the plan's f32 volume: add_z_stage)
                if (plan->pw.out_u8 && plan->ndim == 2) {
                    a.row_bytes = (uint32_t)a.NX;
                    if (TY == 128) return launch_fused_pass2_tall_u8(K, (const uint8_t *)plan->in[pl], (uint8_t *)plan->out[pl], a, plan->stream);
                    return launch_fused_pass2_u8(K, TY, (const uint8_t *)plan->in[pl], (uint8_t *)plan->out[pl], a, plan->stream);
                }
            }
            if constexpr (sizeof(Acc) == 4) {
                if (TY == 128) return launch_fused_pass2_tall<P>(K, plan->in[pl], plan->pw.in_u8, (P *)plan->xy_result(pl), a, plan->stream);
            }
            return launch_fused_pass2<P>(K, TY, padded ? plan->pad_in[pl] : plan->in[pl], plan->pw.in_u8, (P *)(padded ? plan->pad_out[pl] : plan->xy_result(pl)), a,
                                         plan->stream);
        };
        if (g.y_is_exchange_dim) plan->finish_steps.push_back(p2);
        else plan->begin_steps.push_back(p2);
        if (padded) {
            const size_t user_bytes = (size_t)plan->dims[0].N * sizeof(P);
            Step co;
            co.name = "pad_copy_out";
            co.run = [plan, user_bytes](int pl) -> int {
                RF_HIP_CHECK(hipMemcpyAsync(plan->out[pl], plan->pad_out[pl], user_bytes, hipMemcpyDeviceToDevice, plan->stream));
                return (int)RF_OK;
            };
            plan->begin_steps.push_back(co);
        }
    }

    // ---- z (3-D): filtered after the fused x/y stage, reading and writing the output planes ----
    int add_z_stage(size_t first_begin_step) {
        int status = RF_OK;
        const bool padded = g.padded;
        // Intermediate volume (RF_PLAN_INPLACE_Z forbids it): a final z pass that reads and writes the SAME addresses is 4 %
        // slower than one from one volume to another -- its write front follows its read front through the same DRAM banks
        // (tools/microbench/zpass_shape.hip: 2.95 against 2.82 ms per 512 planes of 2048^2; config 5 at 2048^3: 12.3 -> 11.8 ms).
        // Large volumes on the strided kernels therefore get a plan-owned volume between the two stages, as long as it is at
        // most a third of the memory the device has free now.  The x/y stage writes it, the z stage reads it and writes the
        // output planes; nothing else looks at the x/y stage's result.
        if constexpr (sizeof(Acc) == 4 && !is_half_pixel<P>::value) {
            const size_t mid_bytes = (size_t)plan->total * sizeof(P);
            if (!(plan->flags & RF_PLAN_INPLACE_Z) && !plan->host_only && !padded && strided_tile(plan, 2) > 0 &&
                plan->total >= ((int64_t)1 << 28)) {
                size_t free_b = 0, total_b = 0;
                if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && mid_bytes * (size_t)plan->n_planes <= free_b / 3) {
                    for (int pl = 0; pl < plan->n_planes && status == RF_OK; pl++) plan->mid[pl] = plan->alloc(mid_bytes, false, &status);
                    if (status != RF_OK) return status;
                }
            }
        }
        int rc;
        if constexpr (std::is_same<P, float>::value) {
            // Native byte volumes (RF_IO_U8; plan.cpp, u8_plan_is_native).  The contract is that of the 16-bit storage types below:
            // nothing may pass through a byte plane before the last store, so the x/y stage's result waits in the intermediate
            // volume, ALWAYS allocated (host-only plans count it; the free memory is not consulted: the staged form would own an
            // f32 plane of the same size).  Everything up to the final z pass is the RF_IN_U8 plan's -- the final x/y pass reads
            // the bytes and writes the volume, pass 1 of z and the carry scan read it -- and the final z pass stores
            // sat8(post_f * v + post_b) (strided_final_u8_kernel): the affine epilogue rides on the store, there is no
            // pointwise_post step.  Bytes per sample: 1 + (1 + 4) + 4 + (4 + 1) = 15, against 23 staged.
            // (build_fused has admitted byte planes for this form alone: plan_strided.h, byte_volume_form)
            if (plan->pw.out_u8) {
                for (int pl = 0; pl < plan->n_planes; pl++)
                    if (plan->mid[pl] == nullptr) plan->mid[pl] = plan->alloc((size_t)plan->total * sizeof(float), false, &status);
                if (status != RF_OK) return status;
                const bool post = plan->pw.post;
                rc = add_strided_dimension<float, S, uint8_t>(plan, 2, /*from_input=*/false, desc, first_begin_step, nullptr, nullptr,
                                                              post ? (float)plan->pw.post_f : 1.0f, post ? (float)plan->pw.post_b : 0.0f);
                plan->pw.post_fused = post;        // (no stand-alone step: plan.cpp, add_pointwise_steps)
                return rc;
            }
        }
        if constexpr (is_half_pixel<P>::value) {
            // Native 16-bit volumes.  RF_F16 / RF_BF16 are storage types (pixel.h): nothing may be rounded before the last store,
            // so the x/y stage's result cannot wait in the 16-bit output planes.  It waits in the intermediate volume above, here
            // ALWAYS allocated and ALWAYS f32 (host-only plans count it in their workspace; the free memory is not consulted: the
            // staged form would own an f32 plane of the same size): the final x/y pass reads the 16-bit input and writes it
            // (f32 instances with a 16-bit source), pass 1 of z and the carry scan are the f32 plan's, and the final z pass
            // rounds once as it stores (strided_final_narrow_kernel).  18 bytes per sample, against 32-36 staged.
            if (strided_tile(plan, 2) == 0 || padded) {
                set_error("fused path: a volume of 16-bit float pixels needs the strided z stage");
                return RF_ERR_UNSUPPORTED;
            }
            for (int pl = 0; pl < plan->n_planes; pl++) plan->mid[pl] = plan->alloc((size_t)plan->total * sizeof(float), false, &status);
            if (status != RF_OK) return status;
            return add_strided_dimension<float, S, P>(plan, 2, /*from_input=*/false, desc, first_begin_step);
        } else
        if constexpr (sizeof(Acc) == 4)
            rc = strided_tile(plan, 2) > 0 ? add_strided_dimension<P, S>(plan, 2, /*from_input=*/false, desc, first_begin_step,
                                                                         walk.hook.get(), walk.hook ? walk.child.release() : nullptr)
                                           : add_generic_dimension<P, S>(plan, desc->tile[2], 2, /*from_input=*/false);
        else rc = add_generic_dimension<P, S>(plan, desc->tile[2], 2, /*from_input=*/false);      // (f64: no strided kernels)
        return rc;
    }
};

template <typename P, typename S>
int build_fused(rf_plan *plan, const rf_filter_desc *desc) {
    plan->vector_access = true;                  // 16-byte chunks per lane in both passes
    FusedBuilder<P, S> fb;
    fb.plan = plan; fb.desc = desc;
    const FusedGeometry &g = fb.g = fused_geometry<P>(plan);
    if (g.error) { set_error("%s", g.error); return RF_ERR_UNSUPPORTED; }
    // (byte output planes: only the final pass of such an image stores bytes -- nothing else here may ever write them)
    // (... or the final z pass of a volume whose x/y result waits in an f32 volume of the plan's own: add_z_stage)
    const bool byte_volume = byte_volume_form(plan);
    if (plan->pw.out_u8 && (!std::is_same<P, float>::value || (plan->ndim != 2 && !byte_volume) || plan->sharded() || plan->mod_form || g.chained ||
                            g.padded || plan->dims[0].N % 4 != 0)) {
        set_error("fused path: byte output planes need an unsharded f32 plan of orders <= 3 whose width is a multiple of 4: a 2-D image, or a "
                  "volume with scans along z on the strided kernels");
        return RF_ERR_UNSUPPORTED;
    }
    plan->dims[0].T = kFusedTX; plan->dims[0].M = g.chained ? g.N1 / kFusedTX : g.MX;
    if (!g.chained) { plan->dims[1].T = g.TY; plan->dims[1].M = g.MY; }
    const size_t first_begin_step = plan->begin_steps.size(), first_finish_step = plan->finish_steps.size();

    if (int rc = fused_tables<P, S>(plan, g, fb.t)) return rc;
    if (int rc = fused_buffers<S>(plan, g, fb.t, fb.b)) return rc;
    if (int rc = plan_walk_pass1<P, S>(plan, desc, g, fb.b, fb.walk)) return rc;
    // The x tails of tall patches arrive in two parts (GenericDimArgs::tails_part2), which only the blocked carry scan carry_x
    // adds up: a plan whose x carries are completed by xscan_rows (merged_cx, the neighbour form) or by the row chain of chained
    // rows would drop the second part.  Unreachable today -- tall patches need a volume and 128-row tiles, merged_cx at most 64
    // rows, the neighbour form a 2-D image, chained rows a 1-D signal -- but those are heuristics of three functions.
    if (fb.walk.args.tall && (fb.b.merged_cx || fb.t.nb_x || g.chained)) {
        set_error("fused path: tall walk patches need the carry_x scan (not merged_cx / neighbour form / chained rows)");
        return RF_ERR_UNSUPPORTED;
    }
    fb.set_plane_args();

    if (int rc = fb.add_pass1()) return rc;
    if (g.nx > 0 && !g.chained && !fb.b.merged_cx && !fb.t.nb_x) fb.t.x.add_local_carry(plan, "carry_x");
    if (g.chained) fb.add_chained_row_carries();
    if (g.nx > 0 && g.ny > 0) fb.add_xscan_rows();
    if (int rc = fb.add_y_carries()) return rc;
    fb.add_pass2();
    if (plan->ndim > 2 && !plan->dims[2].scan_ids.empty())
        if (int rc = fb.add_z_stage(first_begin_step)) return rc;
    if (g.batch) {
        // every step above covers all planes in its one launch: it runs for plane 0 and is skipped for the others
        auto once = [](std::vector<Step> &steps, size_t first) {
            for (size_t i = first; i < steps.size(); i++) {
                auto inner = steps[i].run;
                steps[i].run = [inner](int pl) { return pl > 0 ? (int)RF_OK : inner(0); };
            }
        };
        once(plan->begin_steps, first_begin_step);
        once(plan->finish_steps, first_finish_step);
    }
    return RF_OK;
}

}  // namespace

bool fused_plan_applicable(const rf_plan *plan, const rf_filter_desc *, std::string *why) {
    auto no = [&](const char *msg) { if (why) *why = msg; return false; };
    const bool half = plan->dtype == RF_F16 || plan->dtype == RF_BF16;
    if (plan->dtype != RF_F32 && plan->dtype != RF_I32 && plan->dtype != RF_I16 && plan->dtype != RF_F64 && !half)
        return no("pixel type must be f32, f64, i32, i16, f16 or bf16");
    // 16-bit float storage types (pixel.h): 2-D images and 1-D signals run here natively -- no intermediate of theirs ever
    // reaches a plane.  A volume's z stage must not read the x/y stage's result back from the 16-bit output planes: a volume is
    // native where that result can wait in an f32 volume of the plan's own in front of the strided z kernels (add_z_stage,
    // "native 16-bit volumes") and staged through f32 planes everywhere else (plan.cpp, "staged 16-bit plans").
    if (half && plan->ndim > 2) {
        if (plan->dims[2].scan_ids.empty() || strided_tile(plan, 2) == 0) return no("16-bit float volumes: scans along z on the strided kernels");
        if (plan->sharded()) return no("16-bit float volumes cannot be sharded");
        // (a volume's epilogue is a stand-alone step over the output planes, i.e. behind the rounding)
        if (plan->pw.post) return no("16-bit float volumes: no epilogue");
        if (plan->flags & (RF_PLAN_INPLACE_Z | RF_PLAN_WALK_PASS1)) return no("16-bit float volumes: the z stage reads an f32 volume of the plan's own, after two first passes");
    }
    if (half && plan->pw.in_u8) return no("16-bit float pixels: no unsigned-byte input");
    if (plan->dtype == RF_F64 && (plan->ndim < 2 || plan->pw.in_u8)) return no("f64 pixels: 2-D / 3-D images of f64 samples");
    if (plan->ndim == 1) {
        // a long 1-D signal folded into chained rows (zero border only: the clamped prologue would differ per row)
        if (plan->clamped) return no("1-D: clamped border not supported on the fused path");
        if (plan->sharded()) return no("1-D: cannot be sharded");
        if (plan->dims[0].scan_ids.empty()) return no("no scans");
        if (plan->dims[0].N < 8192 || chained_row_length(chained_padded_length(plan->dims[0].N)) == 0)
            return no("1-D: at least 8192 samples");
        if (chained_padded_length(plan->dims[0].N) != plan->dims[0].N) {
            // zero padding behind the signal: a causal scan rings on into it, and an anticausal scan AFTER a causal one
            // would pick that ringing up -- such filters (and prologues, which turn the padding into their bias) run as given
            if (plan->pw.in_u8 || plan->pw.pre) return no("1-D: a length that is not a multiple of 8192 cannot take a prologue");
            bool seen_causal = false;
            for (int id : plan->dims[0].scan_ids) {
                if (plan->scans[id].causal) seen_causal = true;
                else if (seen_causal) return no("1-D: an anticausal scan behind a causal one needs a length that is a multiple of 8192");
            }
        }
        if (plan->dims[0].k > kFusedMaxK) return no("feedback order above 3");
        if ((int)plan->dims[0].scan_ids.size() > kFusedMaxScans) return no("more than 4 scans");
        return true;
    }
    if (plan->dims[0].scan_ids.empty() && plan->dims[1].scan_ids.empty()) return no("no scans along x or y");
    if (plan->mod_form) {
        // scans in zero-border form behind border modifications (plan.cpp, "clamped sections"): the kernels position a
        // modification at compile-time indices of the entry segment / the tile's first or last rows
        if (plan->dtype != RF_F32 || plan->sharded()) return no("clamped sections: unsharded f32 images");
        if (plan->pw.post && plan->pw.post_i != 0.0) return no("clamped sections: no epilogue with an input operand");
        if (plan->dims[0].N % 16 != 0) return no("clamped sections: width must be a multiple of 16");
        if (!plan->dims[1].scan_ids.empty() && plan->dims[1].N % 32 != 0) return no("clamped sections: height must be a multiple of 32");
        if (plan->ndim > 2 && !plan->dims[2].scan_ids.empty() && strided_tile(plan, 2) == 0) return no("clamped sections: the z stage needs the strided kernels");
        for (int d = 0; d < plan->ndim; d++)
            if ((int)plan->dims[d].scan_ids.size() > kFusedMaxScans) return no("clamped sections: more than 4 scans in a dimension");
    }
    // rows of 4- and 8-byte pixels only have to be element-aligned: a width that is not a multiple of 4 ends every row in a
    // partial chunk, loaded sample by sample (scan_device.h, load_chunk_cols); 2-byte pixels and unsigned-byte inputs are
    // moved in 8- and 4-byte pieces and keep the rule
    if (plan->dims[0].N % 4 != 0 && (plan->dtype == RF_I16 || half || plan->pw.in_u8))
        return no("2-byte pixels / uint8 inputs: width must be a multiple of 4");
    if (plan->ndim == 2 && plan->sharded() && plan->shard_common % 32 != 0)
        return no("row-sharded slabs must be whole tiles (height a multiple of 32)");
    const int K = fused_order(plan);
    if (K > kFusedMaxK) return no("feedback order above 3");
    if ((int)plan->dims[0].scan_ids.size() > kFusedMaxScans || (int)plan->dims[1].scan_ids.size() > kFusedMaxScans)
        return no("more than 4 scans along x or y");
    const int64_t NZ = plan->ndim > 2 ? plan->dims[2].N : 1;
    if (NZ > 65535 || (plan->dims[1].N + 31) / 32 > 65535) return no("grid too large");
    if (plan->ndim > 2 && !plan->dims[2].scan_ids.empty()) {
        // the z stage runs on the generic dimension builder
        if (strided_tile(plan, 2) == 0 && pick_generic_tile(plan->dims[2].N, plan->dims[2].k, 0) == 0)
            return no("no tile divides the z extent");
    }
    return true;
}

int build_fused_plan(rf_plan *plan, const rf_filter_desc *desc) {
    if (plan->dtype == RF_F32) return build_fused<float, double>(plan, desc);
    if (plan->dtype == RF_I32) return build_fused<int32_t, uint64_t>(plan, desc);
    if (plan->dtype == RF_I16) return build_fused<int16_t, uint64_t>(plan, desc);
    if (plan->dtype == RF_F64) return build_fused<double, double>(plan, desc);
    if (plan->dtype == RF_F16) return build_fused<_Float16, double>(plan, desc);
    if (plan->dtype == RF_BF16) return build_fused<__bf16, double>(plan, desc);
    set_error("fused path: unsupported pixel type");
    return RF_ERR_UNSUPPORTED;
}

}  // namespace rf
