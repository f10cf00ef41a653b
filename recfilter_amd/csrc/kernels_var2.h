// kernels_var2.h -- launchers of the time-varying second-order all-pole scans on 1-D signals (kernels_var2_signal.hip;
// plan_var2.cpp drives them).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rf_internal.h"

namespace rf {

// tail slots per tile (and per group): E = (e0, e1), the state after the tile from zero entry, and the 2 x 2 matrix P that
// carries the entering state across it
constexpr int kVar2Components = 6;
enum Var2Component { VAR2_E0 = 0, VAR2_E1 = 1, VAR2_P00 = 2, VAR2_P01 = 3, VAR2_P10 = 4, VAR2_P11 = 5 };

// One scan on all lines.  Line l of every signal begins l * stride samples behind the pointer.  tiles = ceil(n / 64), groups =
// ceil(tiles / 64).
//   tails   [component][line][tile]     the lanes' maps: what enters tile t = E + P * (what enters its group)
//           [component][line][group]    behind them, the groups' aggregates
//   carry   [2][line][group]            the state that enters group g
// causal: the direction of THIS recurrence (an adjoint stage runs against its forward).  adjoint: the coefficients are read
// shifted by one (a1) and two (a2) samples against the direction of the recurrence -- lam[n] couples to lam[n+1] through a1[n+1].
struct Var2Args {
    const float *x;
    const float *a1, *a2;
    float *dst;
    float *tails;
    float *carry;
    int32_t n;                      // samples per line: a multiple of 4
    int32_t tiles, groups;
    int32_t n_lines;
    int32_t causal;
    int32_t adjoint;
    int64_t stride;
    const float *b0, *b1, *b2;      // var2_biquad_tails_1d alone: the feed-forward taps, laid out like x
};

// The coefficient gradients of one scan (var2_grad_1d): lam = its adjoint state, y = its output.
//   causal      grad_a1[n] = -lam[n] y[n-1]   grad_a2[n] = -lam[n] y[n-2]
//   anticausal  grad_a1[n] = -lam[n] y[n+1]   grad_a2[n] = -lam[n] y[n+2]
// and 0, by a select, where the neighbour lies outside the line.
struct Var2GradArgs {
    const float *lam, *y;
    float *grad_a1, *grad_a2;
    int32_t n;
    int32_t n_lines;
    int32_t causal;                 // the direction of the FORWARD scan
    int64_t stride;
};

// The gradients of one direct-form-I section behind its adjoint scan (var2_biquad_grad_1d): lam = the adjoint state of the
// all-pole half, x = the section's input, y = its output.  For a causal section
//   grad_in[n] = fma(b2~[n+2], lam[n+2], fma(b1~[n+1], lam[n+1], b0[n] * lam[n]))          (lam outside the line is 0)
//   grad_b0[n] = lam[n] x[n]   grad_b1[n] = lam[n] x[n-1]   grad_b2[n] = lam[n] x[n-2]   grad_a1[n] = -lam[n] y[n-1]   grad_a2[n] = -lam[n] y[n-2]
// the mirror image for an anticausal one; +0, by a select, where the neighbour lies outside the line.  with_coefficients == 0:
// grad_in alone; x, y and the five coefficient gradients are not touched.
struct Var2BiquadGradArgs {
    const float *lam, *x, *y;
    const float *b0, *b1, *b2;
    float *grad_in;
    float *grad_b0, *grad_b1, *grad_b2, *grad_a1, *grad_a2;
    int32_t n;
    int32_t n_lines;
    int32_t causal;                 // the direction of the FORWARD section
    int32_t with_coefficients;
    int64_t stride;
};

// The boundary between sections k and k + 1 of a cascade (var2_link_1d, var2_link_keep_1d): x = v_k, what section k's first launch
// or the link before this one stored; a1, a2 = section k's feedback coefficients; tails and carry hold section k's maps and
// carries on entry and section k + 1's maps and aggregates on return (a workgroup reads its own slots before it writes them).
// next_* = section k + 1's five coefficient signals.  dst receives v_{k+1} and may be x (no workgroup reads another's samples);
// keep, where not null, receives y_k and may be x too.  dst and keep are apart.
struct Var2LinkArgs {
    const float *x;
    const float *a1, *a2;
    const float *next_b0, *next_b1, *next_b2, *next_a1, *next_a2;
    float *dst;
    float *keep;
    float *tails;
    const float *carry;
    int32_t n;
    int32_t tiles, groups;
    int32_t n_lines;
    int32_t causal;
    int64_t stride;
};

// The boundary between sections k and k - 1 of a cascade, backward (var2_adj_link_1d, var2_adj_link_keep_1d): x = g_k, the
// gradient that enters section k's adjoint scan (grad_out, or what the link before this one stored); a1, a2, b0, b1, b2 = section
// k's coefficient signals; tails and carry hold that scan's maps and carries on entry and, on return, the maps and aggregates of
// section k - 1's adjoint scan (prev_a1, prev_a2: its feedback coefficients).  dst receives g_{k-1} and may be x; keep, where not
// null, receives lam_k and may be x too.  dst and keep are apart.  causal: the direction of the ADJOINT recurrence.
struct Var2AdjLinkArgs {
    const float *x;
    const float *a1, *a2;
    const float *b0, *b1, *b2;
    const float *prev_a1, *prev_a2;
    float *dst;
    float *keep;
    float *tails;
    const float *carry;
    int32_t n;
    int32_t tiles, groups;
    int32_t n_lines;
    int32_t causal;
    int64_t stride;
};

// ---- coefficients from control-rate frames (rf_var2_plan_execute_biquad_frames) -----------------------------------------------------
// A coefficient of line l is n_frames f32 values, frame j at sample j * hop, l * frame_stride values behind the pointer; hop =
// 1 << hop_shift, 64 .. 65536, inv_hop = 1 / hop.  At n = j * hop + k the coefficient is fma(k * inv_hop, c[j+1] - c[j], c[j]).
// One stage of the section on all lines: the FF tails stage (x = in, dst = v, all five coefficients), its final stage (x = dst = v;
// a1, a2) or a stage of the adjoint scan (adjoint = 1; a1, a2 read one and two samples along the forward's direction).
struct Var2FramesArgs {
    const float *x;
    const float *b0, *b1, *b2, *a1, *a2;      // frames
    float *dst;
    float *tails;
    float *carry;
    int32_t n;
    int32_t tiles, groups;
    int32_t n_lines;
    int32_t causal;                 // the direction of THIS recurrence
    int32_t adjoint;
    int32_t hop_shift, n_frames;
    float inv_hop;
    int64_t stride, frame_stride;
    // a call with a state (rf_var2_plan_execute_cascade_frames_stream), forward stages alone: [line][K + 1][2] f32, state_stride
    // floats from line to line; either pointer null: no state enters / none is wanted; both null: the instances without a state.
    // The FF stage (pair 0) folds pairs 0 and 1 of state_in into v and stores pair 0 of state_out from x; the final stage stores
    // pair `pair` = K from the result.  The names then end in "_stream_1d".
    const float *state_in;
    float *state_out;
    int64_t state_stride;
    int32_t pair;
    // the backward of such a call (stream != 0: the adjoint STREAM instances): grad_state_out and grad_state_in are laid out like
    // the state.  Pair add_pair of grad_state_out is added to x at the forward's two last samples where x is grad_out (-1: x
    // holds it already); the final stage, which holds lam of section `pair`, adds the feedback part of pair `pair` + 1 of
    // grad_state_in (stores it where pair == last_section) and stores the feed-forward part of pair `pair`.
    const float *grad_state_out;
    float *grad_state_in;
    int32_t add_pair, last_section;
    int32_t stream;
};

constexpr int kVar2FrameSums = 10;           // per piece of an interval: S0 and S1 of b0, b1, b2, a1, a2
constexpr int kVar2GradBlock = 1024;         // samples of a workgroup of var2_biquad_frames_grad_1d
// The gradients of the section behind its adjoint scan (var2_biquad_frames_grad_1d): grad_in as var2_biquad_grad_1d forms it, the
// taps interpolated; with_frames: the five per-sample coefficient gradients of that kernel, rounded to f32, contracted in f64 over
// pieces of min(hop, 1024) samples -- S0 = sum (1 - k / hop) g, S1 = sum (k / hop) g -- into
//   slab   [line][piece][10] doubles, pieces = ceil(n / min(hop, 1024)) per line
// var2_frames_fold_1d adds the pieces of the two intervals that meet at a frame, in order, and rounds once: grad[line][frame].
struct Var2FramesGradArgs {
    const float *lam, *x, *y;
    const float *b0, *b1, *b2;      // frames
    float *grad_in;
    double *slab;
    float *grad_b0, *grad_b1, *grad_b2, *grad_a1, *grad_a2;      // the fold's: [line][frame]
    int32_t n;
    int32_t n_lines;
    int32_t causal;                 // the direction of the FORWARD section
    int32_t with_frames;
    int32_t hop_shift, n_frames;
    int32_t pieces;                 // per line
    float inv_hop;
    int64_t stride, frame_stride;
    // stream != 0 (the backward of a call with a state): pairs `pair` and `pair` + 1 of state_in are the section's history, read
    // where the forward read it; pair 0 of grad_state_out is added to the two last samples of grad_in.  Either may be null.
    const float *state_in;
    const float *grad_state_out;
    int64_t state_stride;
    int32_t pair;
    int32_t stream;
};
inline int64_t var2_frames_pieces(int64_t n, int hop) { const int64_t piece = hop < kVar2GradBlock ? hop : kVar2GradBlock; return (n + piece - 1) / piece; }

// One coefficient expanded to audio rate on all lines (var2_expand_frames_1d): out[line * stride + n], n a multiple of 4.
struct Var2ExpandArgs {
    const float *frames;
    float *out;
    int32_t n;
    int32_t n_lines;
    int32_t hop_shift, n_frames;
    float inv_hop;
    int64_t stride, frame_stride;
};
int launch_var2_expand_frames(const Var2ExpandArgs &a, hipStream_t stream);      // "var2_expand_frames_1d"
// "var2_biquad_frames_tails_1d" (a.adjoint == 0), "var2_adj_frames_tails_1d"; with a state "var2_biquad_frames_tails_stream_1d" and
// "var2_frames_pass2_stream_1d"
int launch_var2_frames_tails(const Var2FramesArgs &a, hipStream_t stream);
int launch_var2_frames_pass2(const Var2FramesArgs &a, hipStream_t stream);       // "var2_frames_pass2_1d", "var2_adj_frames_pass2_1d"
int launch_var2_frames_grad(const Var2FramesGradArgs &a, hipStream_t stream);    // "var2_biquad_frames_grad_1d"
int launch_var2_frames_fold(const Var2FramesGradArgs &a, hipStream_t stream);    // "var2_frames_fold_1d"

// ---- a cascade of sections on control-rate frames (rf_var2_plan_execute_cascade_frames) ---------------------------------------------
// One hop, one n_frames and one frame_stride serve every section; a1 .. next_a2 (b0 .. prev_a2) are FRAMES.  Otherwise the two
// structs are Var2LinkArgs and Var2AdjLinkArgs: the same x, dst, keep, tails and carry, the same rules for what may be what.
struct Var2FramesLinkArgs {
    const float *x;
    const float *a1, *a2;
    const float *next_b0, *next_b1, *next_b2, *next_a1, *next_a2;
    float *dst;
    float *keep;
    float *tails;
    const float *carry;
    int32_t n;
    int32_t tiles, groups;
    int32_t n_lines;
    int32_t causal;
    int32_t hop_shift, n_frames;
    float inv_hop;
    int64_t stride, frame_stride;
    // as in Var2FramesArgs; pair = k + 1 for the link that finishes section k: that pair of state_out from y_k, that pair and the
    // next of state_in folded into v_{k+1}
    const float *state_in;
    float *state_out;
    int64_t state_stride;
    int32_t pair;
};
struct Var2AdjFramesLinkArgs {
    const float *x;
    const float *a1, *a2;
    const float *b0, *b1, *b2;
    const float *prev_a1, *prev_a2;
    float *dst;
    float *keep;
    float *tails;
    const float *carry;
    int32_t n;
    int32_t tiles, groups;
    int32_t n_lines;
    int32_t causal;                 // the direction of the ADJOINT recurrence
    int32_t hop_shift, n_frames;
    float inv_hop;
    int64_t stride, frame_stride;
    // as the adjoint fields of Var2FramesArgs; pair = k, and pair k of grad_state_out is added to g_{k-1} at the forward's two
    // last samples before it is stored
    const float *grad_state_out;
    float *grad_state_in;
    int64_t state_stride;
    int32_t pair, add_pair, last_section;
    int32_t stream;
};
// The fold of all sections in one launch (var2_frames_fold_cascade_1d): section k's sums lie k * section_doubles behind slab, laid
// out as Var2FramesGradArgs::slab; grads[k] = its five [line][frame] gradients (b0, b1, b2, a1, a2).  The sections ride on gridDim.z.
constexpr int kVar2MaxSections = 16;         // RF_VAR2_MAX_SECTIONS
struct Var2FramesFoldCascadeArgs {
    const double *slab;
    int64_t section_doubles;
    float *grads[kVar2MaxSections][5];
    int32_t n_sections;
    int32_t n_lines;
    int32_t hop_shift, n_frames;
    int32_t pieces;                 // per line
    int64_t frame_stride;
};
// "var2_frames_link_1d", "var2_frames_link_keep_1d" (a.keep != null); with a state "var2_frames_link_stream_1d", "var2_frames_link_keep_stream_1d"
int launch_var2_frames_link(const Var2FramesLinkArgs &a, hipStream_t stream);
int launch_var2_adj_frames_link(const Var2AdjFramesLinkArgs &a, hipStream_t stream);   // "var2_adj_frames_link_1d", "var2_adj_frames_link_keep_1d"
// the sums of the five frame gradients of a section without grad_in: a.b0, a.b1, a.b2, a.grad_in and a.with_frames are not looked at
int launch_var2_frames_coef(const Var2FramesGradArgs &a, hipStream_t stream);          // "var2_frames_coef_1d"
int launch_var2_frames_fold_cascade(const Var2FramesFoldCascadeArgs &a, hipStream_t stream);      // "var2_frames_fold_cascade_1d"

constexpr int kVar2Tile = 64;            // samples of a tile: one lane
constexpr int kVar2GroupTiles = 64;      // tiles of a group: one wave
int launch_var2_tails(const Var2Args &a, hipStream_t stream);      // "var2_tails_1d", "var2_adj_tails_1d"
int launch_var2_carry(const Var2Args &a, hipStream_t stream);      // "var2_carry_1d"
int launch_var2_pass2(const Var2Args &a, hipStream_t stream);      // "var2_pass2_1d", "var2_adj_pass2_1d"
int launch_var2_grad(const Var2GradArgs &a, hipStream_t stream);   // "var2_grad_1d"
// the tails launch of a direct-form-I section: v = b0 x + b1~ x[n-1] + b2~ x[n-2] formed in registers and STORED to a.dst, the
// tails of the all-pole scan on v stored as launch_var2_tails stores them (a.adjoint == 0; a.dst overlaps none of the inputs)
int launch_var2_biquad_tails(const Var2Args &a, hipStream_t stream);             // "var2_biquad_tails_1d"
int launch_var2_link(const Var2LinkArgs &a, hipStream_t stream);                 // "var2_link_1d", "var2_link_keep_1d" (a.keep != null)
int launch_var2_biquad_grad(const Var2BiquadGradArgs &a, hipStream_t stream);    // "var2_biquad_grad_1d"
int launch_var2_adj_link(const Var2AdjLinkArgs &a, hipStream_t stream);          // "var2_adj_link_1d", "var2_adj_link_keep_1d" (a.keep != null)
// the five coefficient gradients without grad_in: a.b0, a.b1, a.b2, a.grad_in and a.with_coefficients are not looked at
int launch_var2_biquad_coef(const Var2BiquadGradArgs &a, hipStream_t stream);    // "var2_biquad_coef_1d"

}  // namespace rf
