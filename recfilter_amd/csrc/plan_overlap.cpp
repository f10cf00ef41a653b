// plan_overlap.cpp -- plan of RF_PATH_TILED_OVERLAPPED: every tiled dimension in ONE pass 1 and ONE pass 2, the
// carries dimension by dimension with the cross-dimension residuals of lib/split.cpp:1215-1633 between them
// (kernels_overlap.hip).  Steps of one execute:
//     overlap_pass1, { [overlap_residual_d,] carry_d }  for d = x, y, z,  overlap_pass2
#include <algorithm>
#include <cstring>

#include "kernels_fused.h"       // launch_carry_block / carry_chunk_length
#include "kernels_overlap.h"
#include "plan.h"
#include "plan_generic.h"

namespace rf {

bool overlap_plan_applicable(const rf_plan *plan, const rf_filter_desc *desc, std::string *why) {
    auto no = [&](const char *msg) { if (why) *why = msg; return false; };
    if (plan->sharded()) return no("the overlapped path runs on one device");
    int filtered = 0;
    int64_t vol = 1;
    for (int d = 0; d < plan->ndim; d++) {
        const DimInfo &di = plan->dims[d];
        if (di.scan_ids.empty()) continue;
        filtered++;
        const int T = desc->tile[d];
        if (T <= 0) return no("every filtered dimension needs an explicit tile width (RecFilter::split)");
        if (di.N % T != 0) return no("tile width does not divide the extent");
        if (T < di.k) return no("tile narrower than the filter order");
        if (di.k > kOvMaxOrder) return no("orders above 8 run on the matrix / generic paths");
        vol *= T;
    }
    if (filtered < 1) return no("no scans");
    if (vol > kOvMaxTile) return no("tile volume above 4096 samples");
    return true;
}

namespace {

template <typename P, typename S>
int build_overlap(rf_plan *plan, const rf_filter_desc *desc) {
    using Acc = typename PixelTraits<P>::Acc;
    int status = RF_OK;
    OvArgs<Acc> base{};
    base.ndim = plan->ndim;
    base.clamped = plan->clamped ? 1 : 0;
    CarryStage<S, Acc> carry[3];
    for (int d = 0; d < 3; d++) {
        OvDim<Acc> &od = base.d[d];
        od.N = d < plan->ndim ? plan->dims[d].N : 1;
        od.lines = d < plan->ndim ? plan->dims[d].lines : plan->total;
        od.T = 1; od.M = (int32_t)od.N; od.n = 0; od.k = 0;
        od.scans = nullptr; od.G = nullptr; od.tails = nullptr;
        if (d >= plan->ndim || plan->dims[d].scan_ids.empty()) {
            if (od.N >= (1ll << 31)) { set_error("overlapped path: extent too large"); return RF_ERR_UNSUPPORTED; }
            continue;
        }
        DimInfo &di = plan->dims[d];
        const int T = desc->tile[d], n = (int)di.scan_ids.size(), k = di.k;
        di.T = T; di.M = di.N / T;
        od.T = T; od.M = (int32_t)di.M; od.n = n; od.k = k;

        CarryStage<S, Acc> &c = carry[d];
        status = c.init(plan, di.scan_ids, std::string(1, "xyz"[d]), k, T, di.M, LineGeom{di.N, di.stride, di.lines}, {});
        // G[v][q][pos][o]: what the carry entering scan q adds to the tile after ALL scans of the dimension
        std::vector<S> G((size_t)4 * n * T * k, S(0));
        for (int v = 0; v < 4; v++)
            for (int q = 0; q < n; q++) {
                const std::vector<S> &Pm = c.tab.P(v, q, n - 1);
                std::copy(Pm.begin(), Pm.begin() + (std::ptrdiff_t)T * k, G.begin() + (std::ptrdiff_t)(((size_t)v * n + q) * T * k));
            }
        const std::vector<Acc> hG = table_for_kernels<S, Acc>(plan, G, "G_" + c.dn);
        od.G = (const Acc *)plan->upload(hG.data(), hG.size() * sizeof(Acc), &status);
        od.scans = c.dev.base.scans;
        if (status == RF_OK) status = c.alloc_buffers(plan);
        if (status != RF_OK) return status;
    }
    // (dimensions without scans are "tiled" one index at a time: check the tile count fits)
    CarryDev<Acc> dev[3];
    for (int d = 0; d < 3; d++) dev[d] = carry[d].dev;
    auto args_for = [base, dev](int pl) {
        OvArgs<Acc> a = base;
        for (int d = 0; d < 3; d++)
            if (a.d[d].n > 0) a.d[d].tails = dev[d].tails + (size_t)pl * dev[d].tails_stride;
        return a;
    };

    Step p1;
    p1.name = "overlap_pass1";
    p1.run = [plan, args_for](int pl) { return launch_overlap_pass1<P>((const P *)plan->in[pl], args_for(pl), plan->stream); };
    plan->begin_steps.push_back(p1);
    bool earlier = false;
    for (int d = 0; d < plan->ndim; d++) {
        if (base.d[d].n == 0) continue;
        const std::string dn(1, "xyz"[d]);
        if (earlier) {
            Step rs;
            rs.name = "overlap_residual_" + dn;
            rs.run = [plan, args_for, d](int pl) { return launch_overlap_residual<Acc>(args_for(pl), d, plan->stream); };
            plan->begin_steps.push_back(rs);
        }
        carry[d].add_local_carry(plan, "carry_" + dn);
        earlier = true;
    }
    Step p2;
    p2.name = "overlap_pass2";
    p2.run = [plan, args_for](int pl) {
        return launch_overlap_pass2<P>((const P *)plan->in[pl], (P *)plan->out[pl], args_for(pl), plan->stream);
    };
    plan->begin_steps.push_back(p2);
    return status;
}

}  // namespace

int build_overlap_plan(rf_plan *plan, const rf_filter_desc *desc) {
    switch (plan->dtype) {
        case RF_F32: return build_overlap<float, double>(plan, desc);
        case RF_F64: return build_overlap<double, double>(plan, desc);
        case RF_I32: return build_overlap<int32_t, uint64_t>(plan, desc);
        case RF_I16: return build_overlap<int16_t, uint64_t>(plan, desc);
    }
    set_error("overlapped path: unsupported pixel type");
    return RF_ERR_UNSUPPORTED;
}

}  // namespace rf
