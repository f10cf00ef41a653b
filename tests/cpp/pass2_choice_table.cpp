// The table that pins select_pass2 (recfilter_amd/csrc/pass2_select.h): one line per query of a fixed lattice, in a fixed
// nested order -- the refusal, or the ordered launches with every field of theirs.  Host only, no HIP:
//     c++ -O2 -std=c++17 -x c++ pass2_choice_table.cpp -o pass2_choice_table
//     ./pass2_choice_table             the table (tests/test_pass2_choices_host.py compares its SHA-256 and row count)
//     ./pass2_choice_table --summary   rows per instance, "unlisted" / "unreached" lines for the instance lists, no table
// Every instance computes the same pixels, so a changed line here is the only sign of a changed choice short of a timing.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../../recfilter_amd/csrc/pass2_select.h"

using namespace rf;

struct Family { const char *name; int dst, src, pixel_bytes; };
static const Family kFamilies[] = {
    {"f32", kP2F32, kP2F32, 4},       {"f16", kP2F16, kP2F16, 2},        {"bf16", kP2BF16, kP2BF16, 2}, {"i32", kP2I32, kP2I32, 4},
    {"i16", kP2I16, kP2I16, 2},       {"f64", kP2F64, kP2F64, 8},        {"u8>f32", kP2F32, kP2U8, 4},  {"f16>f32", kP2F32, kP2F16, 4},
    {"bf16>f32", kP2F32, kP2BF16, 4}, {"u8>u8", kP2U8, kP2U8, 1},
};
// scan lists of a dimension: none, one causal, causal + anticausal, anything else (anticausal first)
struct ScanList { int n; bool causal[2]; };
static const ScanList kScanLists[] = {{0, {false, false}}, {1, {true, false}}, {2, {true, false}}, {2, {false, true}}};
// 65 x 33 tiles (a grid of 64 x 32 whole ones is the smallest that takes the XCD-contiguous order): whole / last column partial /
// last row partial / both / a width that is not a multiple of 4
constexpr int kMX = 65, kMY = 33;
struct Tiles { int last_cols; bool rows_partial; };
static const Tiles kTiles[] = {{256, false}, {252, false}, {256, true}, {252, true}, {250, false}};

static std::string instance_label(const Pass2Query &q, const Family &f, const Pass2Instance &i) {
    char s[128];
    snprintf(s, sizeof s, "%s %s K%d TY%d EPI%d EDGE%d YPAT%d XFIX%d EARLY%d LIN%d MOD%d RS%d", q.tall ? "tall" : "short", f.name, q.K,
             q.tall ? kPass2TallTY : q.TY, i.EPI, i.EDGE, i.YPAT, i.XFIX, i.EARLY, i.LIN, i.MOD, i.RS);
    return s;
}

int main(int argc, char **argv) {
    const bool summary = argc > 1 && strcmp(argv[1], "--summary") == 0;
    static char buffer[1 << 20];
    setvbuf(stdout, buffer, _IOFBF, sizeof buffer);
    std::map<std::string, long> reached;
    long rows = 0, unlisted = 0;
    for (const Family &f : kFamilies)
    for (int K = 1; K <= 3; K++)
    for (int TY : {32, 64, 128})
    for (const Tiles &t : kTiles)
    for (int xi = 0; xi < 4; xi++)
    for (int yi = 0; yi < 4; yi++)
    for (int mod = 0; mod < 2; mod++)
    for (int lin = 0; lin < 2; lin++)
    for (int epi = 0; epi < 3; epi++)             // no epilogue, affine, with an input operand
    for (int y_apply = 0; y_apply < 2; y_apply++)
    for (int y_nb = 0; y_nb < 2; y_nb++)
    for (int rs = 0; rs < 2; rs++) {              // the row-scan form's pointers (x_nb_W, rs_tau, rs_G)
        Pass2Query q{};
        // (the plans send 128-row tiles to the tall kernel's launchers, which f64 pixels do not have)
        q.tall = TY == 128 && f.dst != kP2F64;
        q.dst = f.dst; q.src = f.src; q.K = K; q.TY = TY;
        q.MX = kMX; q.MY = kMY; q.NZ = 1;
        q.last_cols = t.last_cols; q.last_rows = t.rows_partial ? 5 : TY;
        q.NX = (int64_t)(kMX - 1) * kPass2TileCols + t.last_cols;
        q.row_bytes = (uint32_t)(q.NX * f.pixel_bytes);
        q.nx = kScanLists[xi].n; q.ny = kScanLists[yi].n;
        for (int s = 0; s < 2; s++) { q.x_causal[s] = kScanLists[xi].causal[s]; q.y_causal[s] = kScanLists[yi].causal[s]; }
        q.mod_form = mod; q.lin = lin;
        q.pw_flags = epi ? 2 : 0; q.post_input = epi == 2;
        q.y_apply = y_apply; q.y_nb_W = y_nb; q.x_nb_W = q.rs_tau = q.rs_G = rs;
        const Pass2Choice c = select_pass2(q);
        rows++;
        if (!summary)
            printf("%s K%d TY%d c%d r%d x%d y%d m%d l%d e%d a%d n%d s%d :", f.name, K, TY, q.last_cols, q.last_rows, xi, yi, mod, lin, epi, y_apply, y_nb, rs);
        for (int n = 0; n < c.n; n++) {
            const Pass2Launch &l = c.launch[n];
            const std::string label = instance_label(q, f, l.inst);
            reached[label]++;
            const bool listed = pass2_has(q.tall, q.dst, q.src, K, TY, l.inst);
            bool in_rows = false;
            for (const Pass2Instance &r : kPass2Instances) in_rows = in_rows || r == l.inst;
            if (!listed || !in_rows) {
                unlisted++;
                if (summary) printf("unlisted %s\n", label.c_str());
            }
            if (!summary)
                printf(" [%s] t%d,%d g%d,%d G%dx%dx%d X%d L%zu", label.c_str(), l.tx0, l.ty0, l.gx, l.gy, l.gx > 0 ? l.gx : q.MX, l.gy > 0 ? l.gy : q.MY,
                       (int)q.NZ, l.xcd_contig, l.lds);
        }
        if (!summary) {
            if (c.refusal != RF_OK) printf(" refuse %d %s", c.refusal, c.text);
            printf("\n");
        }
    }
    if (summary) {
        printf("rows %ld\n", rows);
        for (const auto &kv : reached) printf("reach %ld %s\n", kv.second, kv.first.c_str());
        // every instance the lists hold for a family the lattice walks, and no row reached it
        for (const Family &f : kFamilies)
        for (int K = 1; K <= 3; K++)
        for (int TY : {32, 64, 128}) {
            Pass2Query q{};
            q.tall = TY == 128; q.K = K; q.TY = TY;
            for (const Pass2Instance &r : kPass2Instances)
                if (pass2_has(q.tall, f.dst, f.src, K, TY, r) && !reached.count(instance_label(q, f, r))) printf("unreached %s\n", instance_label(q, f, r).c_str());
        }
    }
    return unlisted ? 1 : 0;
}
