// kernels_fused_tall.hip -- pass 2 on 256 x 128 tiles.
//
// The bytes the fused path moves besides the image are tails: k samples per tile border, scan and line.  Their volume is
// proportional to 1/256 + 1/TY, and every kernel between the two passes (the x residual of the y tails, the y carry scan)
// reads and writes the y tails once -- at TY = 64 that is 0.45 GB against the image's 1 GB on cfg3.  Doubling the tile height
// halves the y tails and with them those kernels.  A 256 x 128 tile is 128 KiB: it does not fit the LDS twice per CU, but
// the y phase never needed the tile in LDS -- it holds its column in registers.  So the tile goes through the SAME 64 KiB of
// LDS as two halves of 64 rows (load, x phase, columns out), the thread keeps its 128-sample column in registers, runs all
// y scans on it and stores.  Everything else is fused_pass2_kernel (kernels_fused.hip): same carries, same tables, same
// arithmetic per sample.
#include <iterator>
#include <type_traits>
#include <utility>

#include "kernels.h"
#include "kernels_fused.h"
#include "scan_device.h"

namespace rf {

namespace {

constexpr int kTallTY = 128;
constexpr int kHalfRows = 64;

// YPAT: the directions of the y scans when they are the usual ones -- 1: one causal scan, 2: causal then anticausal; 0: any
// (a run-time direction inside the loop over the scans makes every sample of the column a phi of two register
// assignments: a hundred and more register copies per scan and, on a 128-sample column, spills).
// EARLY (whole tiles, one of the fixed patterns, no epilogue -- byte planes: none with an input operand): the rows are stored from
// inside the last scan.
// XFIX: the x scans have the same pattern as the y scans (YPAT), fixed at compile time as well.
// RS (row-scan form, FusedArgs::rs_tau; f32 whole tiles, the pair in both dimensions, both in neighbour form): nothing between
// the passes has completed a carry.  x: FusedArgs::xt holds the raw tails, and the entry lane of the anticausal scan adds
// W_v(tx+1)[0->1] * (this tile's own causal tail) to the tail it loads from tile tx + 1 -- what xscan_rows_kernel<NB> wrote to
// xt_done.  y: the tails are tile-locally scanned along x (pass 1) but lack the cross-dimension residual, so each of the three
// the kernel loads -- the causal one of tile ty - 1, the anticausal one of tile ty + 1, its own causal one -- first gets
// sum_{q,o} G_vx[q][o][column] * tau(that tile)[j * K + r][q * K + o] (xtau_kernel).  Same terms in the same order as the
// three-kernel form: the results are the same to the bit.
template <typename P, int K, bool EDGE, typename PI, int YPAT, bool EARLY, bool XFIX, bool RS = false>
__global__ void __launch_bounds__(kFusedThreads, 2)
fused_pass2_tall_kernel(const PI *__restrict__ src, P *__restrict__ dst, FusedArgs<typename PixelTraits<P>::Acc> a) {
    using Acc = typename PixelTraits<P>::Acc;
    using A4 = typename Vec4<Acc>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Acc *tile = reinterpret_cast<Acc *>(lds_raw);
    A4 *tile4 = reinterpret_cast<A4 *>(lds_raw);
    constexpr int TY = kTallTY, TL = kHalfRows, NR = TL / 16;

    const int t = threadIdx.x;
    int bx = (int)blockIdx.x, by = (int)blockIdx.y;
    if (a.xcd_contig) {                                        // (uniform; FusedArgs::xcd_contig)
        const unsigned gxn = gridDim.x, total = gxn * gridDim.y;
        unsigned b = (unsigned)by * gxn + (unsigned)bx;
        b = (b & 7u) * (total >> 3) + (b >> 3);
        bx = (int)(b % gxn); by = (int)(b / gxn);
    }
    const int tx = bx + a.tx0, ty = by + a.ty0;
    const int64_t z = blockIdx.z;
    if (a.plane_batch) {
        src = reinterpret_cast<const PI *>(a.in_planes[z]);
        dst = reinterpret_cast<P *>(a.out_planes[z]);
    }
    const int64_t tile_off = (a.plane_batch ? 0 : z * a.NX * a.NY) + (int64_t)ty * TY * a.NX + (int64_t)tx * kFusedTX;
    const int l = t & 15, slot = t >> 4, sw = (l >> 2) & 3;    // x phase: segment lane, row slot
    const int cc = t & 63, rg = t >> 6;                        // load: 16-byte chunk, row group
    const int e = (swz_chunk(t >> 2) << 2) | (t & 3);          // y phase: swizzled column offset
    const int64_t Lx = a.NYP * a.NZ, Ly = a.NXP * a.NZ;
    const int64_t line = (int64_t)tx * kFusedTX + t + a.NXP * z;       // y phase: this thread's column
    const int last_lane = (EDGE && tx == a.MX - 1) ? a.last_lane : 15;
    const int last_cols = (EDGE && tx == a.MX - 1) ? a.last_cols : kFusedTX;
    const int entry_valid = last_cols - 16 * last_lane;
    const int rows_here = (EDGE && ty == a.MY - 1) ? a.last_rows : TY;

    const char *spb = reinterpret_cast<const char *>(src + tile_off);
    const uint32_t in_row_bytes = a.row_bytes / (uint32_t)sizeof(P) * (uint32_t)sizeof(PI);
    const uint32_t off0 = (uint32_t)rg * in_row_bytes + (uint32_t)cc * (uint32_t)(4 * sizeof(PI));
    const bool chunk_in = 4 * cc < last_cols;
    // ... and when the width is not a multiple of 4 the last of them is partial (tile-uniform flag; scan_device.h)
    const bool odd_cols = EDGE && (last_cols & 3) != 0;
    const int cols_valid = last_cols - 4 * cc;
    const A4 zero4 = A4{Acc(0), Acc(0), Acc(0), Acc(0)};

    Acc col[TY];              // this thread's column, all 128 rows
    A4 tmp[2][TL / 4];       // both halves are requested up front
    auto request_pixels = [&](int h) {
        // wave w streams rows w, w+4, ... of the half
#pragma unroll
        for (int i = 0; i < TL / 4; i++) {
            const int row = TL * h + rg + 4 * i;
            const bool in = chunk_in && (!EDGE || row < rows_here);
            if (odd_cols) tmp[h][i] = in ? load_chunk_cols<PI, Acc>(spb + (off0 + (uint32_t)(TL * h + 4 * i) * in_row_bytes), cols_valid) : zero4;
            else tmp[h][i] = in ? load_chunk<PI, Acc>(spb + (off0 + (uint32_t)(TL * h + 4 * i) * in_row_bytes)) : zero4;
        }
    };

    // Order of the requests: the first half's pixels, then every carry, then the second half's pixels.  (Carries first -- round
    // 1's order -- delays the first pixel request by ~90 load instructions per tile; the x phase of the first half waits for
    // "everything but the second half" either way.)
    request_pixels(0);
    // ---- y carries: requested first, used last ----
    Acc CY[kFusedMaxScans][K];
#pragma unroll
    for (int j = 0; j < kFusedMaxScans; j++) {
#pragma unroll
        for (int r = 0; r < K; r++) CY[j][r] = Acc(0);
        if (j < a.ny) {
            const bool causal = a.ys[j].causal != 0;
            const bool tile_first = causal ? (ty == 0) : (ty == a.MY - 1);
            if (tile_first) {
#pragma unroll
                for (int r = 0; r < K; r++) CY[j][r] = a.y_incoming[((int64_t)j * K + r) * Ly + line];
            } else {
                const int tp = causal ? ty - 1 : ty + 1;
#pragma unroll
                for (int r = 0; r < K; r++) CY[j][r] = a.yt[a.yt_index(j, tp, r, K, line)];
            }
        }
    }
    // row shard: tails completed with zero entering carries + Y * (true entering carries), as in fused_pass2_kernel.  The
    // entering carries are requested here, with the other carries; the correction itself waits until the pixels have been
    // requested (apply_entering_carries below) -- computed here it made every tile wait for its carry loads before it asked
    // for a single pixel.
    // Neighbour-form y carries (FusedArgs::y_nb_W): the anticausal carry from tile ty + 1 is that tile's own tail plus
    // W_v(ty+1)[0->1] * this tile's causal tail -- the same shape, a k-vector requested here and a k x k product applied
    // after the pixels, with the tile's own scan-0 tail in the place of the slab's entering carries.
    // RS: this column's G entries and the (workgroup-uniform) tau of the three tiles, requested with the carries
    Acc rs_g[RS ? 2 * K : 1];
    Acc rs_t[RS ? 3 : 1][K][RS ? 2 * K : 1];
    if constexpr (RS) {
        static_assert(!EDGE && YPAT == 2 && XFIX && std::is_same<Acc, float>::value, "row scans: whole tiles, the pair in x and in y");
        const int vx = (tx == 0 ? 1 : 0) | (tx == a.MX - 1 ? 2 : 0);
#pragma unroll
        for (int qo = 0; qo < 2 * K; qo++) rs_g[qo] = a.rs_G[((size_t)vx * 2 * K + qo) * kFusedTX + t];
        // [0]: tile ty - 1, scan 0; [1]: this tile, scan 0; [2]: tile ty + 1, scan 1
        const int64_t tile_id = (z * a.MY + ty) * a.MX + tx;
        const Acc *tp = a.rs_tau + tile_id * (4 * K * K);
#pragma unroll
        for (int r = 0; r < K; r++)
#pragma unroll
            for (int qo = 0; qo < 2 * K; qo++) {
                rs_t[0][r][qo] = ty > 0 ? tp[-(int64_t)a.MX * (4 * K * K) + r * 2 * K + qo] : Acc(0);
                rs_t[1][r][qo] = ty < a.MY - 1 ? tp[r * 2 * K + qo] : Acc(0);
                rs_t[2][r][qo] = ty < a.MY - 1 ? tp[(int64_t)a.MX * (4 * K * K) + (K + r) * 2 * K + qo] : Acc(0);
            }
    }
    Acc yin[kFusedMaxScans][K];
    if (a.y_apply != nullptr) {
#pragma unroll
        for (int q = 0; q < kFusedMaxScans; q++)
#pragma unroll
            for (int o = 0; o < K; o++) yin[q][o] = q < a.ny ? a.y_incoming[((int64_t)q * K + o) * Ly + line] : Acc(0);
    } else if (a.y_nb_W != nullptr && ty < a.MY - 1) {
#pragma unroll
        for (int o = 0; o < K; o++) yin[0][o] = a.yt[a.yt_index(0, ty, o, K, line)];
    }
    auto apply_entering_carries = [&]() {
        if constexpr (RS) {
            // the residual of the three loaded tails, q then o onto the tail as xscan_rows_kernel adds it to a row
#pragma unroll
            for (int r = 0; r < K; r++)
#pragma unroll
                for (int qo = 0; qo < 2 * K; qo++) {
                    if (ty > 0) CY[0][r] = CY[0][r] + rs_g[qo] * rs_t[0][r][qo];
                    if (ty < a.MY - 1) {
                        yin[0][r] = yin[0][r] + rs_g[qo] * rs_t[1][r][qo];
                        CY[1][r] = CY[1][r] + rs_g[qo] * rs_t[2][r][qo];
                    }
                }
        }
        if (a.y_nb_W != nullptr) {
            if (ty < a.MY - 1) {          // (the last tile row's anticausal carry enters at the border: nothing chains on it)
                const int v = (ty + 1 == a.MY - 1) ? 2 : 0;
                const Acc *Wm = a.y_nb_W + ((v * a.ny + 0) * a.ny + 1) * K * K;
                // (term by term onto the loaded tail, in the order the carry scan adds them: W has entries of either sign
                //  several times the sum of a row, so a partial sum formed first rounds differently)
#pragma unroll
                for (int r = 0; r < K; r++)
#pragma unroll
                    for (int o = 0; o < K; o++) CY[1][r] = CY[1][r] + Wm[r * K + o] * yin[0][o];
            }
            return;
        }
        if (a.y_apply == nullptr) return;
#pragma unroll
        for (int j = 0; j < kFusedMaxScans; j++) {
            if (j < a.ny) {
                const bool causal = a.ys[j].causal != 0;
                const bool tile_first = causal ? (ty == 0) : (ty == a.MY - 1);
                if (!tile_first) {
                    const int tp = causal ? ty - 1 : ty + 1;
#pragma unroll
                    for (int r = 0; r < K; r++) {
                        Acc add = Acc(0);
#pragma unroll
                        for (int q = 0; q <= j; q++) {
                            const Acc *Ym = a.y_apply + ((((int64_t)q * a.ny + j) * a.MY + tp) * K + r) * K;
#pragma unroll
                            for (int o = 0; o < K; o++) add = add + Ym[o] * yin[q][o];
                        }
                        CY[j][r] = CY[j][r] + add;
                    }
                }
            }
        }
    };

    // The x carries entering the rows of both halves: requested before the pixels, parked in LDS behind the tile once they
    // have arrived ([half][s][n][j][row slot]; read by every lane of a row, used by its entry lane) -- a 128-sample column,
    // a prefetched half tile and the x phase leave no registers for them.
    Acc *cx_lds = tile + TL * kFusedTX;
    Acc CX[2][kFusedMaxScans][NR][K];
    Acc XOWN[RS ? 2 : 1][RS ? NR : 1][K];      // RS: the tile's own causal tail, for the entry lane of the anticausal scan
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int64_t line0 = (int64_t)ty * TY + TL * h + slot + a.NYP * z;
#pragma unroll
        for (int s = 0; s < kFusedMaxScans; s++) {
#pragma unroll
            for (int n = 0; n < NR; n++)
#pragma unroll
                for (int j = 0; j < K; j++) CX[h][s][n][j] = Acc(0);
            if (s < a.nx) {
                const bool causal = a.xs[s].causal != 0;
                const bool tile_first = causal ? (tx == 0) : (tx == a.MX - 1);
                const bool first_lane = causal ? (l == 0) : (l == last_lane);
                if (first_lane) {
                    const int tp = causal ? tx - 1 : tx + 1;
                    const Acc *cp = tile_first ? a.x_incoming + (int64_t)s * K * Lx : a.xt + ((int64_t)s * a.MX + tp) * K * Lx;
#pragma unroll
                    for (int n = 0; n < NR; n++)
#pragma unroll
                        for (int j = 0; j < K; j++) CX[h][s][n][j] = cp[j * Lx + line0 + 16 * n];
                    if constexpr (RS) {
                        if (s == 1 && !tile_first) {
                            const Acc *op = a.xt + (int64_t)tx * K * Lx;
#pragma unroll
                            for (int n = 0; n < NR; n++)
#pragma unroll
                                for (int j = 0; j < K; j++) XOWN[h][n][j] = op[j * Lx + line0 + 16 * n];
                        }
                    }
                }
            }
        }
    }
    auto park_carries = [&]() {
        if constexpr (RS) {
            // c_1(tx+1) = tau_1(tx+1) + W_v(tx+1)[0->1] tau_0(tx), term by term onto the loaded tail (xscan_rows_kernel<NB>)
            if (l == last_lane && tx < a.MX - 1) {
                const int vt = (tx + 1 == a.MX - 1) ? 2 : 0;
                const Acc *Wm = a.x_nb_W + ((vt * 2 + 0) * 2 + 1) * K * K;
#pragma unroll
                for (int h = 0; h < 2; h++)
#pragma unroll
                    for (int n = 0; n < NR; n++)
#pragma unroll
                        for (int j = 0; j < K; j++)
#pragma unroll
                            for (int m = 0; m < K; m++) CX[h][1][n][j] = CX[h][1][n][j] + Wm[j * K + m] * XOWN[h][n][m];
            }
        }
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int s = 0; s < kFusedMaxScans; s++) {
                if (s < a.nx) {
                    const bool causal = a.xs[s].causal != 0;
                    const bool first_lane = causal ? (l == 0) : (l == last_lane);
                    if (first_lane) {
#pragma unroll
                        for (int n = 0; n < NR; n++)
#pragma unroll
                            for (int j = 0; j < K; j++) cx_lds[(((h * kFusedMaxScans + s) * NR + n) * K + j) * 16 + slot] = CX[h][s][n][j];
                    }
                }
            }
    };
    request_pixels(1);
    park_carries();
    apply_entering_carries();
    // ... and wait in LDS meanwhile, [j][r][column] behind the x carries (registers are the scarce resource here)
    Acc *cy_lds = tile + kHalfRows * kFusedTX + 2 * kFusedMaxScans * (kHalfRows / 16) * K * 16;
#pragma unroll
    for (int j = 0; j < kFusedMaxScans; j++)
        if (j < a.ny) {
#pragma unroll
            for (int r = 0; r < K; r++) cy_lds[(j * K + r) * kFusedTX + t] = CY[j][r];
        }

#pragma unroll
    for (int h = 0; h < TY / TL; h++) {
        if constexpr (!PixelTraits<P>::is_integer) {
            if (a.pw_flags & 1) {
#pragma unroll
                for (int i = 0; i < TL / 4; i++) {
                    const bool in = chunk_in && TL * h + rg + 4 * i < rows_here;      // samples beyond the image stay zero
                    const Acc s = in ? a.pre_s : Acc(0), b = in ? a.pre_b : Acc(0);
                    tmp[h][i].x = s * tmp[h][i].x + b; tmp[h][i].y = s * tmp[h][i].y + b;
                    tmp[h][i].z = s * tmp[h][i].z + b; tmp[h][i].w = s * tmp[h][i].w + b;
                    if (odd_cols) clear_dead_cols<A4, Acc>(tmp[h][i], cols_valid);
                }
            }
        }
        if (h > 0) __syncthreads();                             // the previous half's columns are out of LDS
#pragma unroll
        for (int i = 0; i < TL / 4; i++) tile4[(rg + 4 * i) * 64 + swz_chunk(cc)] = tmp[h][i];
        __syncthreads();
        // ---- x phase of this half ----
        if (a.nx > 0) {
            Acc v[NR][kFusedSeg];
#pragma unroll
            for (int n = 0; n < NR; n++) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    A4 q = tile4[(slot + 16 * n) * 64 + 4 * l + (j ^ sw)];
                    v[n][4 * j + 0] = q.x; v[n][4 * j + 1] = q.y; v[n][4 * j + 2] = q.z; v[n][4 * j + 3] = q.w;
                }
            }
            auto x_scan = [&](int s, auto causal_tag) __attribute__((always_inline)) {
                constexpr bool causal = decltype(causal_tag)::value;
                const FusedScan<Acc> &sc = a.xs[s];
                const bool tile_first = causal ? (tx == 0) : (tx == a.MX - 1);
                const bool first_lane = causal ? (l == 0) : (l == last_lane);
                const bool clamp_first = a.clamped && tile_first && first_lane;
                Acc cx[NR][K];
#pragma unroll
                for (int n = 0; n < NR; n++)
#pragma unroll
                    for (int j = 0; j < K; j++) cx[n][j] = cx_lds[(((h * kFusedMaxScans + s) * NR + n) * K + j) * 16 + slot];
                bool cf = clamp_first;
                if constexpr (!(XFIX && YPAT >= 1)) {              // (the general-pattern variants: what a mod-form plan launches)
                    if (a.mod_form) {
                        if (a.clamped && tile_first) border_mod_rows16<Acc, causal, NR>(v, sc, clamp_first);
                        cf = false;
                    }
                }
                if constexpr (causal) scan_rows16<Acc, true, K, NR>(v, sc, first_lane, cf, cx);
                else scan_rows16<Acc, false, K, NR>(v, sc, first_lane, cf, cx, l > last_lane, EDGE ? entry_valid : kFusedSeg);
            };
            // (the x scans' directions are compile-time too where they follow the y pattern: every row of the tile would
            // otherwise be a phi of two register assignments per scan, as the column is in the y phase)
            if constexpr (XFIX && YPAT == 1) {
                x_scan(0, std::true_type{});
            } else if constexpr (XFIX && YPAT == 2) {
                x_scan(0, std::true_type{});
                x_scan(1, std::false_type{});
            } else {
#pragma unroll 1
                for (int s = 0; s < a.nx; s++) {
                    if (a.xs[s].causal != 0) x_scan(s, std::true_type{});
                    else x_scan(s, std::false_type{});
                }
            }
#pragma unroll
            for (int n = 0; n < NR; n++) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    A4 q;
                    q.x = v[n][4 * j + 0]; q.y = v[n][4 * j + 1]; q.z = v[n][4 * j + 2]; q.w = v[n][4 * j + 3];
                    tile4[(slot + 16 * n) * 64 + 4 * l + (j ^ sw)] = q;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < TL; i++) col[TL * h + i] = tile[i * kFusedTX + e];
    }

    // ---- y phase: thread = column, 128 rows ----
    auto y_scan = [&](int j, auto causal_tag) __attribute__((always_inline)) {
        constexpr bool causal = decltype(causal_tag)::value;
        const FusedScanY<Acc> &sc = a.ys[j];
        const bool border = causal ? (ty == 0 && a.y_first_border) : (ty == a.MY - 1 && a.y_last_border);
        const bool clamp_first = a.clamped && border;
        Acc c[K];
#pragma unroll
        for (int r = 0; r < K; r++) c[r] = cy_lds[(j * K + r) * kFusedTX + t];      // (written by this thread)
        bool cf = clamp_first;
        if constexpr (YPAT == 0) {
            if (a.mod_form) {
                if (clamp_first) border_mod_col<Acc, causal, TY>(col, sc);
                cf = false;
            }
        }
        if constexpr (causal) scan_col<Acc, true, K, TY>(col, sc, cf, c);
        else {
            if (rows_here == TY) scan_col<Acc, false, K, TY>(col, sc, cf, c);
            else scan_col_partial_up<Acc, K, TY>(col, sc, cf, rows_here);
        }
    };
    // whole tiles without an epilogue: the rows are stored from inside the last scan, each as soon as it is final
    char *dpb_early = reinterpret_cast<char *>(dst + tile_off);
    static_assert(!EARLY || (!EDGE && YPAT > 0), "early stores: whole tiles, fixed scan pattern");
    Acc hq0 = Acc(0), hq1 = Acc(0), hq2 = Acc(0), hq3 = Acc(0);      // byte pixels, packed form: the rows of a block of four
    (void)hq0; (void)hq1; (void)hq2; (void)hq3;
    Acc held = Acc(0);
    (void)held;
    auto row_out = [&](int m, Acc v) __attribute__((always_inline)) {
        // (byte planes only: an affine epilogue is applied on the way out, so the usual x' = in / 255, out = 255 F round trip
        // of a byte image keeps the early stores; no other destination type launches EARLY with an epilogue)
        if constexpr (std::is_same<P, uint8_t>::value) {
            if (a.pw_flags & 2) v = a.post_f * v + a.post_b;
        }
        if constexpr (packed_bytes<P>::value) {
            // byte pixels, packed form: four rows at a time, one dword per lane (scan_device.h, store_row_quad)
            if ((m & 3) == 0) hq0 = v; else if ((m & 3) == 1) hq1 = v; else if ((m & 3) == 2) hq2 = v; else hq3 = v;
            if ((m & 3) == (YPAT == 2 ? 0 : 3))
                store_row_quad(dpb_early, (uint32_t)t, (uint32_t)(m & ~3), a.row_bytes, hq0, hq1, hq2, hq3, (uint32_t)TY);
        } else
        if constexpr (packed_stores<P>::value) {
            // 16-bit float pixels: two rows at a time, one dword per lane (scan_device.h, store_row_pair); the scan hands the
            // rows over in its own direction, so the first row of a pair waits for the second
            constexpr bool up = YPAT == 2;
            if (((m & 1) != 0) == up) held = v;
            else store_row_pair<P>(dpb_early, (uint32_t)t, (uint32_t)(m & ~1), a.row_bytes, up ? v : held, up ? held : v, (uint32_t)TY);
        } else
        __builtin_nontemporal_store(PixelTraits<P>::store(v),
                                    reinterpret_cast<P *>(dpb_early + ((uint32_t)t * (uint32_t)sizeof(P) + (uint32_t)m * a.row_bytes)));
    };
    if constexpr (YPAT == 1 || YPAT == 2) {
        if (YPAT == 2) y_scan(0, std::true_type{});
        if constexpr (EARLY) {
            constexpr int jl = YPAT - 1;
            const bool clamp_first = a.clamped && (YPAT == 1 ? (ty == 0 && a.y_first_border) : (ty == a.MY - 1 && a.y_last_border));
            Acc c[K];
#pragma unroll
            for (int r = 0; r < K; r++) c[r] = cy_lds[(jl * K + r) * kFusedTX + t];
            scan_col<Acc, YPAT == 1, K, TY>(col, a.ys[jl], clamp_first, c, row_out);
            return;
        } else {
            if (YPAT == 1) y_scan(0, std::true_type{});
            else y_scan(1, std::false_type{});
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < a.ny; j++) {
            if (a.ys[j].causal != 0) y_scan(j, std::true_type{});
            else y_scan(j, std::false_type{});
        }
    }
    if constexpr (!PixelTraits<P>::is_integer) {
        if (a.pw_flags & 2) {
            if (a.post_i != Acc(0)) {
                // the epilogue's input operand comes back through L2 / the Infinity Cache (no registers to spare here)
                const PI *xp = src + tile_off;
                const uint32_t nxu = (uint32_t)a.NX;
                const Acc c1 = a.post_i * ((a.pw_flags & 1) ? a.pre_s : Acc(1));
                const Acc c2 = a.post_b + a.post_i * ((a.pw_flags & 1) ? a.pre_b : Acc(0));
                if (t < last_cols) {
#pragma unroll
                    for (int i = 0; i < TY; i++)
                        if (i < rows_here) col[i] = a.post_f * col[i] + (c1 * (Acc)xp[(uint32_t)t + (uint32_t)i * nxu] + c2);
                }
            } else {
#pragma unroll
                for (int i = 0; i < TY; i++) col[i] = a.post_f * col[i] + a.post_b;
            }
        }
    }
    {
        char *dpb = reinterpret_cast<char *>(dst + tile_off);
        const uint32_t row_bytes = a.row_bytes;
        if (t < last_cols) {
            if constexpr (packed_bytes<P>::value) {
                // (byte pixels, packed form: last_cols is a multiple of 4, so a quad of columns is stored or not as one)
#pragma unroll
                for (int i = 0; i < TY; i += 4)
                    store_row_quad(dpb, (uint32_t)t, (uint32_t)i, row_bytes, col[i], col[i + 1], col[i + 2], col[i + 3], (uint32_t)(EDGE ? rows_here : TY));
            } else
            if constexpr (packed_stores<P>::value) {
                // (16-bit float pixels, scan_device.h: last_cols is a multiple of 4, so a column pair is stored or not as one)
#pragma unroll
                for (int i = 0; i < TY; i += 2)
                    store_row_pair<P>(dpb, (uint32_t)t, (uint32_t)i, row_bytes, col[i], col[i + 1], (uint32_t)(EDGE ? rows_here : TY));
            } else
#pragma unroll
            for (int i = 0; i < TY; i++)
                if (!EDGE || i < rows_here)
                    __builtin_nontemporal_store(PixelTraits<P>::store(col[i]),
                                                reinterpret_cast<P *>(dpb + ((uint32_t)t * (uint32_t)sizeof(P) + (uint32_t)i * row_bytes)));
        }
    }
}

// (pixel types, K, instance) -> the template instance, launched: the flat list kPass2Instances under its guard (pass2_select.h)
template <typename P, typename PI, int K>
int launch_instance(const Pass2Launch &l, const PI *src, P *dst, const FusedArgs<typename PixelTraits<P>::Acc> &a, hipStream_t stream) {
    using Acc = typename PixelTraits<P>::Acc;
    return pass2_walk(l, K, kTallTY, [&](auto row) -> int {
        constexpr Pass2Instance I = kPass2Instances[decltype(row)::value];
        if constexpr (pass2_has(true, pass2_pixel<P>(), pass2_pixel<PI>(), K, kTallTY, I)) {
            // (opted into for the most y scans a plan can have: Pass2Launch::lds counts the plan's)
            constexpr size_t lds_max = ((size_t)kHalfRows * kFusedTX + 2 * kFusedMaxScans * (kHalfRows / 16) * K * 16 + (size_t)kFusedMaxScans * K * kFusedTX) * sizeof(Acc);
            if (l.inst == I) return pass2_launch<&fused_pass2_tall_kernel<P, K, I.EDGE, PI, I.YPAT, I.EARLY, I.XFIX, I.RS>>(lds_max, l.lds, src, dst, a, stream);
        }
        return kPass2NotThisRow;
    }, std::make_index_sequence<std::size(kPass2Instances)>());
}

}  // namespace

template <typename P, typename PI>
static int run(int K, int src_pixel, const PI *src, P *dst, const FusedArgs<typename PixelTraits<P>::Acc> &a, hipStream_t stream) {
    using Args = FusedArgs<typename PixelTraits<P>::Acc>;
    static const bool edge_everywhere = RF_KNOB("RF_TALL_EDGE_EVERYWHERE") != nullptr;      // A/B runs
    // (partial tiles make up to three launches: pass2_select.h)
    return pass2_run(true, pass2_pixel<P>(), src_pixel, K, kTallTY, a, edge_everywhere, [&](const Pass2Launch &l, const Args &part) -> int {
        switch (K) {
        case 1: return launch_instance<P, PI, 1>(l, src, dst, part, stream);
        case 2: return launch_instance<P, PI, 2>(l, src, dst, part, stream);
        case 3: return launch_instance<P, PI, 3>(l, src, dst, part, stream);
        }
        set_error("fused pass 2: no 128-row instances of order %d", K);
        return RF_ERR_UNSUPPORTED;
    });
}

// unsigned bytes in, unsigned bytes out (kernels_fused.hip, launch_fused_pass2_u8)
int launch_fused_pass2_tall_u8(int K, const uint8_t *src, uint8_t *dst, const FusedArgs<float> &a, hipStream_t stream) {
    return run<uint8_t, uint8_t>(K, kP2U8, src, dst, a, stream);
}

template <typename P>
int launch_fused_pass2_tall(int K, const void *src, int src_kind, P *dst, const FusedArgs<typename PixelTraits<P>::Acc> &a,
                            hipStream_t stream) {
    const int src_pixel = pass2_source(pass2_pixel<P>(), src_kind);
    if constexpr (std::is_same<P, float>::value) {      // (as launch_fused_pass2, kernels_fused.hip)
        if (src_pixel == kP2U8) return run<P, uint8_t>(K, src_pixel, (const uint8_t *)src, dst, a, stream);
        if (src_pixel == kP2F16) return run<P, _Float16>(K, src_pixel, (const _Float16 *)src, dst, a, stream);
        if (src_pixel == kP2BF16) return run<P, __bf16>(K, src_pixel, (const __bf16 *)src, dst, a, stream);
    }
    return run<P, P>(K, src_pixel, (const P *)src, dst, a, stream);
}

template int launch_fused_pass2_tall<float>(int, const void *, int, float *, const FusedArgs<float> &, hipStream_t);
template int launch_fused_pass2_tall<_Float16>(int, const void *, int, _Float16 *, const FusedArgs<float> &, hipStream_t);
template int launch_fused_pass2_tall<__bf16>(int, const void *, int, __bf16 *, const FusedArgs<float> &, hipStream_t);
template int launch_fused_pass2_tall<int32_t>(int, const void *, int, int32_t *, const FusedArgs<uint32_t> &, hipStream_t);
template int launch_fused_pass2_tall<int16_t>(int, const void *, int, int16_t *, const FusedArgs<uint32_t> &, hipStream_t);

}  // namespace rf
