// plan_strided.h -- step list of ONE strided dimension on the register-column path
// (kernels_strided.hip): pass 1, blocked carry scan, pass 2.  Used by plan_fused.cpp for the z
// dimension of 3-D filters.  Same exchange structure as plan_generic.h for the sharded dimension.
#pragma once

#include <cstring>
#include <memory>

#include "kernels_fused.h"
#include "plan.h"
#include "plan_generic.h"

namespace rf {

inline int strided_tile(const rf_plan *plan, int d) {
    const DimInfo &di = plan->dims[d];
    if (di.scan_ids.empty() || di.k > kFusedMaxK || (int)di.scan_ids.size() > kFusedMaxScans) return 0;
    // (RF_F16 / RF_BF16: the z stage of a native 16-bit volume, which reads an f32 volume -- plan_fused.cpp)
    if (plan->dtype != RF_F32 && plan->dtype != RF_I32 && plan->dtype != RF_I16 && plan->dtype != RF_F16 && plan->dtype != RF_BF16) return 0;
    const int64_t basis = plan->tile_basis(d);       // sharded dimension: every rank's slab must tile alike
    if (const int want = plan->strided_tile_planes() ? plan->strided_tile_planes() : RF_KNOB("RF_STRIDED_TZ") ? atoi(RF_KNOB("RF_STRIDED_TZ")) : 0) {
        // RF_PLAN_TILE_PLANES(n): the caller's tile width of the strided stage, where it divides the extent
        if ((want == 32 || want == 64 || want == 128) && basis % want == 0) return want;
    }
    // large volumes: 128 samples per thread halve the tails of this dimension and its carry scan (2048^3: carry_z 1.21 ->
    // 0.53 ms, the two passes unchanged within their run-to-run spread)
    if (basis % 128 == 0 && di.lines % 256 == 0 && di.stride % 256 == 0 && di.lines * di.N >= (int64_t)1 << 28) return 128;
    if (basis % 64 == 0) return 64;
    if (basis % 32 == 0) return 32;
    return 0;
}

// The form of a native byte volume (RF_IO_U8; plan.cpp, u8_plan_is_native; plan_fused.cpp, "native byte volumes"), beyond what the
// fused x/y stage asks of the RF_IN_U8 image: scans along z on the strided kernels behind an f32 volume of the plan's own, a width
// that is a multiple of 4, one device, no input operand in the epilogue.  The one statement of the rule: the plan stage that
// chooses the form and the builder that admits byte planes both ask here.
inline bool byte_volume_form(const rf_plan *plan) {
    return plan->ndim == 3 && !plan->dims[2].scan_ids.empty() && strided_tile(plan, 2) > 0 && plan->dims[0].N % 4 == 0 &&
           !plan->sharded() && !(plan->flags & (RF_PLAN_FORCE_EXCHANGE | RF_PLAN_STAGE_HALF | RF_PLAN_INPLACE_Z | RF_PLAN_WALK_PASS1)) &&
           !(plan->pw.post && plan->pw.post_i != 0.0);
}

// What pass 1 of the x/y stage needs to know when it also forms this dimension's tails (kernels_tails_walk.hip): the strided
// dimension then has no first pass of its own.  Filled by add_strided_dimension.
struct WalkHook {
    float *zt = nullptr;          // the dimension's tails, [s][t][r][line] (plane 0)
    size_t zt_stride = 0;         // elements between the tails of consecutive Tuple planes
};

// The x/y filter F over `planes` carry planes of dimension d, in place: a fused x/y plan of its own (null: cannot be built).
inline rf_plan *build_carry_planes_plan(const rf_plan *plan, const rf_filter_desc *desc, int d, int64_t planes) {
    std::vector<rf_scan_desc> xy;
    for (int i = 0; i < desc->n_scans; i++)
        if (desc->scans[i].dim != d) xy.push_back(desc->scans[i]);
    rf_filter_desc cd = *desc;
    cd.scans = xy.data();
    cd.n_scans = (int32_t)xy.size();
    cd.extent[2] = planes;
    cd.n_planes = 1;
    cd.tile[2] = 0;
    std::memset(&cd.pointwise, 0, sizeof(cd.pointwise));      // (F alone: an epilogue of the filter is not part of it)
    cd.path = RF_PATH_TILED_FUSED;
    cd.device = plan->host_only ? RF_DEVICE_HOST_ONLY : plan->device;
    cd.shard_rank = 0; cd.shard_world = 1; cd.shard_extents = nullptr;
    cd.flags = (desc->flags & (RF_PLAN_STREAM_PASS1 | RF_PLAN_STAGED_PASS1 | 0x0000ff00u)) | RF_PLAN_TILED_ONLY | RF_PLAN_NO_CASCADE;
    rf_plan *child = nullptr;
    if (build_plan(&cd, &child) != RF_OK) return nullptr;
    return child;
}

// Whether dimension d of a sharded plan takes the early exchange (below), before the helper plan has been tried.
template <typename P>
inline bool early_exchange_possible(const rf_plan *plan, int d, const rf_filter_desc *desc) {
    using Acc = typename PixelTraits<P>::Acc;
    const DimInfo &di = plan->dims[d];
    return d == plan->ndim - 1 && plan->sharded() && desc != nullptr && d == 2 &&
           merged_exchange_applies((int)di.scan_ids.size(), di.k, plan->shard_world) && !plan->pw.pre && !plan->pw.post &&
           !plan->pw.in_u8 && !(plan->flags & RF_PLAN_LATE_EXCHANGE) && di.lines == plan->dims[0].N * plan->dims[1].N &&
           sizeof(P) == sizeof(Acc);      // (the carry planes are filtered as pixels: f32 / i32)
}

// Early exchange (a z-sharded volume whose x/y stage precedes this dimension).  The operators of this dimension -- tail
// extraction, carry recurrence, the correction by the entering carries -- act along z alone and identically on every
// (x, y) line; the x/y filter F acts on every z plane alone and identically: they commute, borders included (everything
// is linear).  So the carries of the x/y-FILTERED volume are F applied to the carry planes of the RAW volume:
//     begin      pass 1 of this dimension on the raw input, slab-local carries, exit carries -> send
//     <all-gather>   ||   interior: the whole x/y stage (what rf_plan_interior runs beside the collective)
//     apply      entering carries from the gathered exits, correction of the (raw) tails, then F over the k * scans *
//                (tiles + 1) carry planes, in place -- a fused x/y plan of its own over those few planes
//     finish     pass 2 of this dimension on the x/y-filtered output with the filtered carries
// The exchange no longer waits for the x/y stage and the x/y stage no longer waits for the exchange: a rank's step is
// max(kernels, exchange) instead of their sum, for (tiles + 1) * scans * k / planes of extra x/y work (cfg5 on 8 GPUs:
// 12 carry planes beside 256).  `xy_begin` .. end of plan->begin_steps are the x/y stage's steps at the time of the call.
// Needs: the merged exchange, no pointwise stages (a prologue's bias is not linear), the x/y stage in front.
// `walk` (unsharded volumes, kernels_tails_walk.hip): the same commutation without an exchange -- pass 1 of the x/y stage has
// formed this dimension's tails from the raw input as it went, so the dimension is: carry scan, F over the scans * k * tiles
// carry planes (`walk_child`, built by the caller), pass 2 on the x/y-filtered output.
// PD (native 16-bit volumes, plan_fused.cpp): the type of the output planes where it is not P -- P = float is then the type of
// the plan-owned volume the x/y stage wrote (rf_plan::mid), which both passes read; only the final pass's store knows PD.
// PD = uint8_t (native byte volumes, RF_IO_U8): the same, and the affine part of the plan's epilogue rides on that store
// (`post_f`, `post_b`: out = sat8(post_f * v + post_b); no other destination type looks at them).
template <typename P, typename S, typename PD = P>
int add_strided_dimension(rf_plan *plan, int d, bool from_input, const rf_filter_desc *desc = nullptr, size_t xy_begin = (size_t)-1,
                          WalkHook *walk = nullptr, rf_plan *walk_child = nullptr, float post_f = 1.0f, float post_b = 0.0f) {
    using Acc = typename PixelTraits<P>::Acc;
    int status = RF_OK;
    DimInfo &di = plan->dims[d];
    const int TZ = strided_tile(plan, d);
    if (TZ == 0) { set_error("strided path not applicable to dimension %d", d); return RF_ERR_UNSUPPORTED; }
    if (!std::is_same<PD, P>::value && (from_input || walk != nullptr || plan->sharded() || (plan->mid[0] == nullptr && !plan->host_only))) {
        set_error("strided path: a destination type of its own needs the unsharded z stage behind an intermediate volume");
        return RF_ERR_INVALID_ARG;
    }
    di.T = TZ;
    di.M = di.N / TZ;
    const int n = (int)di.scan_ids.size(), K = di.k, M = (int)di.M;
    const int outer = plan->ndim - 1;
    const bool sharded = (d == outer) && plan->sharded();
    const int np = plan->n_planes;
    std::string dn(1, "xyz"[d]);

    CarryStage<S, Acc> stage;
    typename CarryStage<S, Acc>::Options opt;
    opt.sharded = sharded;
    opt.slab_powers = true;          // [s][slab][K x K], for the per-scan exchange
    opt.apply_powers = sharded;
    status = stage.init(plan, di.scan_ids, dn, K, TZ, M, LineGeom{di.N, di.stride, di.lines}, opt);
    StridedArgs<Acc> base{};
    std::memset(base.scans, 0, sizeof(base.scans));
    for (int i = 0; i < n; i++) {
        const ScanS<S> &t = stage.tab.scans[i];
        base.scans[i].causal = t.causal ? 1 : 0;
        base.scans[i].b = table_to_acc<S, Acc>(t.b);
        for (int j = 0; j < kFusedMaxK; j++) base.scans[i].a[j] = j < K ? table_to_acc<S, Acc>(t.a[j]) : Acc(0);
        base.scans[i].mod_n = plan->scans[di.scan_ids[i]].mod_n;
        if constexpr (!std::is_same<S, uint64_t>::value) {
            for (int j = 0; j < kFusedMaxMod && j < RF_MAX_ORDER; j++) base.scans[i].mod_g[j] = (Acc)t.mod_g[j];
        }
    }
    const size_t tails_pp = stage.tails_pp, inc_pp = stage.inc_pp;
    bool early = sharded && !from_input && xy_begin != (size_t)-1 && early_exchange_possible<P>(plan, d, desc);
    // The early exchange needs a helper plan: F over the carry planes = the x/y scans of this filter on a volume of
    // (tiles + 1) * scans * k planes, in place.  It is built BEFORE anything of the early layout is committed: a helper that
    // cannot be built (unsupported shape, out of memory) leaves the plan on the late exchange instead of failing it.
    // (a sharded plan whose pass 1 walks has had both checked by its builder: its helper is `walk_child`)
    std::unique_ptr<rf_plan> child(walk ? walk_child : nullptr);
    if (walk && sharded && !early) { set_error("one-read pass 1 of a sharded volume needs the early exchange"); return RF_ERR_UNSUPPORTED; }
    if (early && !walk) {
        child.reset(build_carry_planes_plan(plan, desc, d, (int64_t)n * K * (M + 1)));
        if (!child) early = false;
    }
    // early exchange: the tails and the entering carries of a plane are ONE run of (tiles + 1) * scans * k carry planes,
    // which the x/y filter then takes as a volume of that many z planes
    const size_t chunk_pp = early ? tails_pp + inc_pp : 0;
    if (early) {
        Acc *run = (Acc *)plan->alloc(chunk_pp * np * sizeof(Acc), true, &status);
        stage.use_buffers(run, chunk_pp, run ? run + tails_pp : nullptr, chunk_pp);
    } else if (status == RF_OK) {
        status = stage.alloc_buffers(plan);
    }
    if (status != RF_OK) return status;
    const CarryDev<Acc> c = stage.dev;

    base.n = di.N; base.inner = di.stride; base.lines = di.lines; base.M = M; base.n_scans = n;
    base.clamped = plan->clamped ? 1 : 0;
    base.mod_form = plan->mod_form ? 1 : 0;
    base.first_is_border = (!sharded || plan->shard_rank == 0) ? 1 : 0;
    base.last_is_border = (!sharded || plan->shard_rank == plan->shard_world - 1) ? 1 : 0;
    auto sargs = [base, c](int pl) {
        StridedArgs<Acc> a = base;
        a.tails = c.tails + (size_t)pl * c.tails_stride;
        a.incoming = c.incoming + (size_t)pl * c.inc_stride;
        return a;
    };

    Step p1;
    p1.name = "strided_pass1_" + dn;
    if (walk) { walk->zt = reinterpret_cast<float *>(c.tails); walk->zt_stride = c.tails_stride; }
    p1.run = [plan, sargs, K, TZ, from_input, early](int pl) {
        const P *src = (from_input || early) ? (const P *)plan->in[pl] : (const P *)plan->xy_result(pl);
        return launch_strided_pass<P>(false, K, TZ, src, (P *)plan->out[pl], sargs(pl), plan->stream);
    };
    if (early) {
        // the x/y stage leaves the begin phase: it is what runs beside the all-gather (all of it but a pass 1 that also forms
        // this dimension's tails, which the exchange waits for)
        const size_t keep = xy_begin + (walk ? 1 : 0);
        plan->interior_steps.assign(plan->begin_steps.begin() + (std::ptrdiff_t)keep, plan->begin_steps.end());
        plan->begin_steps.resize(keep);
    }
    if (!walk) plan->begin_steps.push_back(p1);

    if (!sharded) {
        stage.add_local_carry(plan, "carry_" + dn);
        if (walk)
            if (int rc = adopt_carry_planes_plan<Acc>(plan, std::move(child), c.tails, c.tails_stride, plan->begin_steps)) return rc;
    } else if (merged_exchange_applies(n, K, plan->shard_world)) {
        int rc = add_merged_exchange<S, Acc>(plan, stage, "carry_" + dn);
        if (rc == RF_OK && early) rc = adopt_carry_planes_plan<Acc>(plan, std::move(child), c.tails, c.tails_stride, plan->exchange_apply_steps.back());
        if (rc != RF_OK) return rc;
    } else {
        int rc = stage.add_per_scan_carries(plan, "carry_" + dn, "carry_apply_" + dn, true);
        if (rc != RF_OK) return rc;
    }

    Step p2;
    p2.name = "strided_pass2_" + dn;
    if constexpr (std::is_same<PD, uint8_t>::value) {
        p2.run = [plan, sargs, K, TZ, post_f, post_b](int pl) {
            return launch_strided_final_u8(K, TZ, (const float *)plan->xy_result(pl), (uint8_t *)plan->out[pl], sargs(pl), post_f, post_b, plan->stream);
        };
    } else {
        p2.run = [plan, sargs, K, TZ, from_input](int pl) {
            const P *src = from_input ? (const P *)plan->in[pl] : (const P *)plan->xy_result(pl);
            if constexpr (!std::is_same<PD, P>::value) return launch_strided_final_narrow<PD>(K, TZ, src, (PD *)plan->out[pl], sargs(pl), plan->stream);
            else return launch_strided_pass<P>(true, K, TZ, src, (P *)plan->out[pl], sargs(pl), plan->stream);
        };
    }
    if (d == outer) plan->finish_steps.push_back(p2);
    else plan->begin_steps.push_back(p2);
    return status;
}

}  // namespace rf
