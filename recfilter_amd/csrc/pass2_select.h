// pass2_select.h -- which instance of the final pass of the fused path runs, as one pure function (no HIP in here).
//
// fused_pass2_kernel (kernels_fused.hip, 32- and 64-row tiles) and fused_pass2_tall_kernel (kernels_fused_tall.hip, 128-row
// tiles) are templates of eight flags; every instance computes the same pixels, so only a timing shows a wrong pick.
// select_pass2 maps the facts of a launch (Pass2Query) to the launches to issue (Pass2Choice); tests/cpp/pass2_choice_table.cpp
// prints it over a lattice of queries and tests/test_pass2_choices_host.py pins that table.  The launchers in the two .hip files
// walk kPass2Instances, the flat list of the instances there are, under the `if constexpr` guard pass2_has.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/recfilter_amd.h"

namespace rf {

enum Pass2Pixel : int { kP2F32 = 0, kP2F16, kP2BF16, kP2I32, kP2I16, kP2F64, kP2U8, kP2Other };      // what a plane holds
constexpr int kPass2TileCols = 256, kPass2TallTY = 128, kPass2MaxScans = 4;      // kFusedTX, the tall kernel's rows, kFusedMaxScans

struct Pass2Query {
    bool tall;                    // fused_pass2_tall_kernel (its launchers have no TY: 128) or fused_pass2_kernel
    int dst, src;                 // Pass2Pixel; src == dst unless f32 planes are computed from bytes or from a 16-bit float type
    int K, TY, last_cols, last_rows, MX, MY;
    int64_t NX, NZ;
    uint32_t row_bytes;
    int nx, ny;
    bool x_causal[2], y_causal[2];     // FusedScan::causal of the first two scans of a dimension: all the rule reads
    bool mod_form, lin, plane_batch;   // lin: FusedArgs::lin_limit > 0
    int pw_flags;
    bool post_input;                   // FusedArgs::post_i != 0: the epilogue has an input operand
    bool y_apply, y_nb_W, x_nb_W, rs_tau, rs_G;      // the pointer is set
    bool edge_everywhere;              // the A/B knob RF_TALL_EDGE_EVERYWHERE (read by the launcher)
};

// One template instance.  YPAT: the y scans' pattern fixed at compile time -- 1: one causal scan, 2: causal then anticausal, 0:
// any; the short kernel folds EARLY (rows leave from inside the last scan) into it as YPAT 3 / 4 and has no RS, the tall kernel
// has EARLY of its own and no EPI, LIN or MOD.
struct Pass2Instance { bool EPI, EDGE; int YPAT; bool XFIX, EARLY, LIN, MOD, RS; };
constexpr bool operator==(const Pass2Instance &a, const Pass2Instance &b) {
    return a.EPI == b.EPI && a.EDGE == b.EDGE && a.YPAT == b.YPAT && a.XFIX == b.XFIX && a.EARLY == b.EARLY && a.LIN == b.LIN &&
           a.MOD == b.MOD && a.RS == b.RS;
}
struct Pass2Launch {
    Pass2Instance inst;
    int tx0, ty0, gx, gy;         // the strip of tiles, as FusedArgs::tx0 .. gy (gx / gy 0: MX / MY)
    int xcd_contig;               // FusedArgs::xcd_contig
    size_t lds;                   // dynamic LDS bytes
};
// The launches to issue, in order, then the refusal to return if there is one (a refusal that only a later strip of a split
// launch meets comes after the earlier strips' launches, as it always has).
struct Pass2Choice {
    int n;
    Pass2Launch launch[3];
    int refusal;                  // RF_OK: none
    char text[192];               // the refusal's message
};

// ---- the instances there are: one flat list for both kernels, pass2_has says which kernel and pixel types compile a row ----
constexpr Pass2Instance kPass2Instances[] = {
    // EPI  EDGE   YPAT XFIX   EARLY  LIN    MOD    RS
    {false, false, 0, false, false, false, false, false},      // the general-pattern code on whole tiles
    {false, false, 1, false, false, false, false, false}, {false, false, 2, false, false, false, false, false},      // the usual y scans, fixed at compile time
    {false, true, 0, false, false, false, false, false},       // partial tiles
    {false, true, 1, false, false, false, false, false}, {false, true, 2, false, false, false, false, false},
    // short kernel: rows leaving from inside the last scan ... and the x scans of the same pattern
    {false, false, 3, false, true, false, false, false}, {false, false, 4, false, true, false, false, false},
    {false, false, 3, true, true, false, false, false}, {false, false, 4, true, true, false, false, false},
    {true, false, 0, false, false, false, false, false}, {true, true, 0, false, false, false, false, false},      // ... the epilogue's input column in registers
    {true, false, 3, false, true, false, false, false}, {true, false, 4, false, true, false, false, false},
    {false, false, 0, false, false, true, false, false},       // ... a folded 1-D signal that ends inside the image
    {false, false, 0, false, false, false, true, false}, {false, true, 0, false, false, false, true, false},      // ... mod form
    // tall kernel: rows leaving from inside the last scan ... the x scans of the same pattern ... the row-scan form
    {false, false, 1, false, true, false, false, false}, {false, false, 2, false, true, false, false, false},
    {false, false, 1, true, true, false, false, false}, {false, false, 2, true, true, false, false, false},
    {false, false, 2, true, true, false, false, true},
};

// the routes with three instances per order and tile height: f32 planes from a 16-bit float type (the x/y stage of a 16-bit
// volume), bytes to bytes (rf_pointwise_desc.in_dtype == RF_IO_U8)
constexpr bool pass2_widens(int dst, int src) { return dst == kP2F32 && (src == kP2F16 || src == kP2BF16); }
constexpr bool pass2_bytes(int dst, int src) { return dst == kP2U8 && src == kP2U8; }
// a pixel type with instances of its own, or f32 from unsigned bytes (RF_IN_U8) on those of the f32 family that read no f32
constexpr bool pass2_typed(int dst, int src) { return (dst == src && dst >= kP2F32 && dst <= kP2F64) || (dst == kP2F32 && src == kP2U8); }

// Is instance `i` compiled for this kernel, these pixel types, this order (tall) / tile height (short)?
constexpr bool pass2_has(bool tall, int dst, int src, int K, int TY, const Pass2Instance &i) {
    const bool narrow = pass2_widens(dst, src) || pass2_bytes(dst, src), same = dst == src, plain_f32 = same && dst == kP2F32;
    if (!narrow && !pass2_typed(dst, src)) return false;
    if (tall) {
        if (i.EPI || i.LIN || i.MOD || i.YPAT > 2 || (i.XFIX && !i.EARLY) || (i.EARLY && (i.EDGE || i.YPAT == 0)) || (i.RS && !i.XFIX)) return false;
        if (i.RS) return K == 2 && plain_f32 && i.YPAT == 2;
        if (narrow) return i.EARLY ? (i.YPAT == 2 && i.XFIX) : (i.YPAT == 0 || (i.YPAT == 2 && (i.EDGE || pass2_bytes(dst, src))));
        return dst != kP2F64;
    }
    if (i.RS || i.EARLY != (i.YPAT > 2) || (i.XFIX && !i.EARLY) || (TY != 32 && TY != 64)) return false;
    if (narrow) return !i.EPI && !i.LIN && !i.MOD && (i.YPAT == 0 || (!i.EDGE && i.YPAT == 4 && i.XFIX));
    if (i.MOD) return plain_f32 && !i.EPI && !i.LIN && i.YPAT == 0;
    if (i.LIN) return same && !i.EPI && !i.EDGE && i.YPAT == 0;
    // (the epilogue variant that keeps the input column in registers exists for f32 and f64 pixels only; 16-bit float pixels have
    // no such instances -- their input operand comes back through the caches, as at order 3)
    if (i.EPI) return (dst == kP2F32 || dst == kP2F64) && (i.YPAT == 0 || (i.YPAT > 2 && !i.EDGE && TY == 64 && same && !i.XFIX));
    if (i.EDGE) return i.YPAT == 0 || (i.YPAT <= 2 && plain_f32);
    return i.YPAT == 0 || ((TY == 64 || dst == kP2F32) && same);
}

namespace pass2_detail {

inline int refuse(Pass2Choice &c, int code, const char *fmt, int v0 = 0, int v1 = 0) {
    c.refusal = code;
    snprintf(c.text, sizeof c.text, fmt, v0, v1);
    return code;
}
// the scans of a dimension when they are the usual ones -- 1: one causal scan, 2: causal then anticausal; 0: any other list
inline int scan_pattern(int n, const bool *causal) { return (n == 1 && causal[0]) ? 1 : (n == 2 && causal[0] && !causal[1]) ? 2 : 0; }

// The instance for one launch on the lean (edge = false) or the EDGE variant; anything but RF_OK: the refusal, filled into c.
inline int pick(const Pass2Query &q, bool edge, Pass2Choice &c, Pass2Instance &i) {
    i = Pass2Instance{};      // the general-pattern code ...
    i.EDGE = edge;
    const bool widens = pass2_widens(q.dst, q.src), bytes = pass2_bytes(q.dst, q.src), same = q.src == q.dst;
    const bool plain_f32 = same && q.dst == kP2F32, integer = q.dst == kP2I32 || q.dst == kP2I16;
    // (a plan in mod form -- FusedArgs::mod_form -- takes the general-pattern code, which applies its border modifications)
    const int ypat = q.mod_form ? 0 : scan_pattern(q.ny, q.y_causal), xpat = q.mod_form ? 0 : scan_pattern(q.nx, q.x_causal);
    const bool pair = ypat == 2 && xpat == 2, epilogue = (q.pw_flags & 2) != 0;
    // rows can leave from inside the last scan with an affine epilogue applied on the way out; one with an input operand only
    // where the column is in registers, i.e. the EPI variants
    const bool affine = integer || !epilogue || !q.post_input;
    if (q.tall && (q.K < 1 || q.K > 3)) return refuse(c, RF_ERR_UNSUPPORTED, "fused path: unsupported order %d", q.K);
    if (!bytes && !widens && !pass2_typed(q.dst, q.src))
        return refuse(c, RF_ERR_INVALID_ARG, "fused pass 2: only f32 pixels take a source of another type");
    if (widens && (q.mod_form || epilogue || q.plane_batch || (q.tall ? (q.y_nb_W || q.y_apply) : q.lin)))
        return refuse(c, RF_ERR_INVALID_ARG, q.tall ? "fused pass 2: a 16-bit source with an f32 destination is the x/y stage of an unsharded volume (no epilogue, no sections)"
                                                    : "fused pass 2: a 16-bit source with an f32 destination is the x/y stage of a volume (no epilogue, no sections)");
    const bool size_ok = q.tall || (q.K >= 1 && q.K <= 3 && (q.TY == 64 || q.TY == 32));
    const char *const size_text = "fused path: unsupported order %d / tile height %d";
    if (widens || bytes) {
        // three instances per order and tile height: partial tiles; whole tiles with the usual pair of scans in both dimensions
        // and rows leaving from inside the last scan (an affine epilogue is applied on the way out; an input operand comes back
        // through the caches, as for the 16-bit types); the general-pattern code for every other filter.  The tall kernel also
        // has the pair of y scans alone at compile time, on partial tiles and for bytes.
        if (!size_ok) return refuse(c, RF_ERR_UNSUPPORTED, size_text, q.K, q.TY);
        if (!edge && pair && affine) { i.YPAT = q.tall ? 2 : 4; i.EARLY = i.XFIX = true; }
        else if (q.tall && ypat == 2 && (edge || bytes)) i.YPAT = 2;
        return RF_OK;
    }
    if (q.tall) {
        // (no epilogue on the way out of the 128-row scan of the pixel types with instances of their own)
        const bool early = !edge && ypat > 0 && (integer || !epilogue);
        if (q.rs_tau) {      // the row-scan form (FusedArgs::rs_tau): one instance
            if (!(!edge && q.K == 2 && plain_f32 && early && pair && q.y_nb_W && q.x_nb_W && q.rs_G && !q.y_apply))
                return refuse(c, RF_ERR_INVALID_ARG, "fused pass 2: the row-scan form is misconfigured");
            i.RS = true;
        }
        i.YPAT = ypat; i.EARLY = early; i.XFIX = early && xpat == ypat;
        return RF_OK;
    }
    // the epilogue variant that keeps the input column in registers exists for f32 and f64 pixels only
    const bool epi = (q.dst == kP2F32 || q.dst == kP2F64) && epilogue && q.post_input && q.K <= 2;
    if (q.lin && (q.ny != 0 || q.NZ != 1 || q.plane_batch || epi || edge))
        return refuse(c, RF_ERR_INVALID_ARG, "fused pass 2: a signal that ends inside the image needs a 1-D plan of whole tiles without an input-operand epilogue");
    if (!size_ok) return refuse(c, RF_ERR_UNSUPPORTED, size_text, q.K, q.TY);
    if (plain_f32 && q.mod_form) {
        if (epi) return refuse(c, RF_ERR_UNSUPPORTED, "fused pass 2: clamped sections cannot take an epilogue with an input operand");
        i.MOD = true;
    } else if (same && q.lin) {
        i.LIN = true;
    } else if (epi) {
        // (three launches like the 128-row final pass's -- whole tiles lean, edge strips on the EDGE variant -- gain nothing here:
        // the 64-row EDGE variant costs 20-35 % per tile, what the two extra strips cost: 8192 x 8188, 0.134 / 0.135 ms)
        i.EPI = true;
        if (!edge && q.TY == 64 && same && ypat > 0) { i.YPAT = ypat + 2; i.EARLY = true; }
    } else if (edge) {
        if (plain_f32) i.YPAT = ypat;       // partial tiles, the usual y scans
    } else if ((q.TY == 64 || q.dst == kP2F32) && same && ypat > 0) {
        i.YPAT = affine ? ypat + 2 : ypat; i.EARLY = affine; i.XFIX = affine && xpat == ypat;
    }
    return RF_OK;
}

}  // namespace pass2_detail

// The launches of one call of a final-pass launcher (behind its grid guard), or its refusal.
inline Pass2Choice select_pass2(const Pass2Query &q) {
    using namespace pass2_detail;
    Pass2Choice c{};
    const bool bytes = pass2_bytes(q.dst, q.src);
    if (!q.tall && !bytes && q.y_nb_W)
        return refuse(c, RF_ERR_INVALID_ARG, "fused pass 2: neighbour-form y carries need the 128-row final pass"), c;
    if (bytes && (q.lin || q.mod_form || (!q.tall && q.y_nb_W) || q.y_apply || q.row_bytes != (uint32_t)q.NX))
        return refuse(c, RF_ERR_INVALID_ARG, "fused pass 2: byte planes on both sides are an unsharded 2-D image of orders <= 3 with a row pitch of NX bytes"), c;
    const bool edge = q.last_cols != kPass2TileCols || q.last_rows != (q.tall ? kPass2TallTY : q.TY);
    // the tile; the tall kernel: the half tile + the x carries of both halves ([2][4 scans][4 rows][K][16 slots]) + the y carries
    // of the columns ([ny * K][256])
    const size_t lds = q.tall ? ((size_t)64 * kPass2TileCols + 2 * kPass2MaxScans * 4 * q.K * 16 + (size_t)q.ny * q.K * kPass2TileCols) * (q.dst == kP2F64 ? 8 : 4)
                              : (size_t)q.TY * kPass2TileCols * (q.dst == kP2F64 ? 8 : 4);
    auto add = [&](bool e, int tx0, int ty0, int gx, int gy) {
        Pass2Launch &l = c.launch[c.n];
        if (pick(q, e, c, l.inst) != RF_OK) return false;
        l.tx0 = tx0; l.ty0 = ty0; l.gx = gx; l.gy = gy;
        const unsigned cells = (unsigned)(gx > 0 ? gx : q.MX) * (unsigned)(gy > 0 ? gy : q.MY);
        l.xcd_contig = (q.tall && q.row_bytes % 128u != 0 && cells % 8u == 0 && cells >= 2048u) ? 1 : 0;      // FusedArgs::xcd_contig
        l.lds = lds;
        c.n++;
        return true;
    };
    // Partial tiles on the 128-row kernel.  The EDGE variant costs the final pass almost twice its time per tile (no rows leave
    // from inside the last scan, a bound and a select per access, 24-144 bytes of scratch: 16384 x 16256, 0.662 ms against
    // 0.366 ms for 16384^2), and only the last tile column / row needs it: the whole tiles run on the lean kernel, the two strips
    // as launches of their own on the EDGE variant (FusedArgs::tx0 ..): 0.386 + 0.042 ms.  (One launch with a per-workgroup
    // branch between the two bodies was slower than the three launches: 0.531 ms.)  The byte route has no A/B knob.
    if (q.tall && edge && (bytes || !q.edge_everywhere)) {
        const int MXf = q.MX - (q.last_cols != kPass2TileCols ? 1 : 0), MYf = q.MY - (q.last_rows != kPass2TallTY ? 1 : 0);
        if (MXf > 0 && MYf > 0 && !add(false, 0, 0, MXf, MYf)) return c;
        if (MXf < q.MX && !add(true, q.MX - 1, 0, 1, q.MY)) return c;
        if (MYf < q.MY && MXf > 0) add(true, 0, q.MY - 1, MXf, 1);
        return c;
    }
    add(edge, 0, 0, 0, 0);
    return c;
}

}  // namespace rf
