// RecFilterVarying2::realize_cascade_frames_stream (include/recfilter.hpp): a cascade of three direct-form-I sections on control-rate
// frames at hop 64, on ONE signal of 8384 samples filtered in two chunks -- 4160 samples (a group and a tile), then 4224 -- with the
// state handed from chunk to chunk, +x and -x (the chunks last to first), against the C calls on plans of their own BIT FOR BIT:
// out, both kept signals and the state that leaves every chunk, then gradient_cascade_frames_stream from the chunk fed last back to
// the first (grad_in, grad_state_in and the fifteen frame gradients of every chunk); the chain against realize_cascade_frames() on the whole signal to
// 1e-4 of the peak; the state that leaves against the two last samples of in, the kept signals and out.  What the C calls compute
// is pinned by tests/test_gpu_stream.py, which compiles and runs this.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int K = 3, HOP = 64, CHUNKS = 2;
constexpr int LENGTH[CHUNKS] = {4160, 4224}, START[CHUNKS] = {0, 4160}, N = 8384;
constexpr int PAIRS = 2 * (K + 1);
using Signal = std::vector<float>;

uint32_t rng_state = 20263u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)
#define RF_CALL(e) do { if ((e) != RF_OK) { std::printf("line %d: %s\n", __LINE__, rf_last_error_string()); return 1; } } while (0)

bool fetch(Signal &to, const float *from, size_t count) {
    to.resize(count);
    return hipMemcpy(to.data(), from, count * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
}

// count floats of two device arrays, bit for bit; NaN anywhere fails
bool same(const std::string &what, const float *a, const float *b, size_t count) {
    Signal x, y;
    if (!fetch(x, a, count) || !fetch(y, b, count)) { std::printf("%s: copy failed\n", what.c_str()); return false; }
    for (size_t i = 0; i < count; i++) {
        if (std::isnan(x[i]) || std::memcmp(&x[i], &y[i], sizeof(float)) != 0) {
            std::printf("%s: %a against %a at %zu\n", what.c_str(), x[i], y[i], i);
            return false;
        }
    }
    std::printf("%s: the same bits\n", what.c_str());
    return true;
}

}  // namespace

int main() {
    const size_t bytes = (size_t)N * sizeof(float);
    const int count = (N + HOP - 1) / HOP + 1;
    Signal in(N);
    for (int i = 0; i < N; i++) in[i] = 2.0f * uniform() - 1.0f;
    // for the front-end ([0]) and the C calls ([1]): out, two kept signals, two state buffers that swap roles; [2]: the whole signal at once
    float *d_in = nullptr, *d_out[3] = {}, *d_kept[2][K - 1] = {}, *d_state[2][2] = {}, *d_f[K][5] = {};
    HIP_OK(hipMalloc((void **)&d_in, bytes));
    for (float *&p : d_out) HIP_OK(hipMalloc((void **)&p, bytes));
    for (int s = 0; s < 2; s++) {
        for (float *&p : d_kept[s]) HIP_OK(hipMalloc((void **)&p, bytes));
        for (float *&p : d_state[s]) HIP_OK(hipMalloc((void **)&p, PAIRS * sizeof(float)));
    }
    HIP_OK(hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice));
    // three resonators whose pole radius and angle move from frame to frame, each behind a moving pair of zeros
    for (int k = 0; k < K; k++) {
        Signal f[5];
        for (Signal &s : f) s.resize((size_t)count);
        double theta = 1.0 + 0.3 * k, phi = 1.7 - 0.2 * k;
        for (int j = 0; j < count; j++) {
            theta = std::min(std::max(theta + 0.3 * (uniform() - 0.5), 0.2), 2.9);
            phi = std::min(std::max(phi + 0.3 * (uniform() - 0.5), 0.2), 2.9);
            const double r = 0.74 + 0.24 * std::sin(0.37 * j + k), q = 0.65 + 0.35 * std::sin(0.61 * j + 1.0 + k), gain = 1.0 + 0.5 * std::sin(0.23 * j + 2.0 + k);
            f[0][j] = (float)gain;
            f[1][j] = (float)(-2.0 * gain * q * std::cos(phi));
            f[2][j] = (float)(gain * q * q);
            f[3][j] = (float)(-2.0 * r * std::cos(theta));
            f[4][j] = (float)(r * r);
        }
        for (int c = 0; c < 5; c++) {
            HIP_OK(hipMalloc((void **)&d_f[k][c], (size_t)count * sizeof(float)));
            HIP_OK(hipMemcpy(d_f[k][c], f[c].data(), (size_t)count * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    // the frames of a chunk: the whole signal's arrays advanced to the chunk's first frame
    auto frames_at = [&](int start) {
        std::vector<rf_var2_section> frames;
        for (int k = 0; k < K; k++)
            frames.push_back({d_f[k][0] + start / HOP, d_f[k][1] + start / HOP, d_f[k][2] + start / HOP, d_f[k][3] + start / HOP, d_f[k][4] + start / HOP});
        return frames;
    };
    // the backward: grad_out, then per side grad_in, two gradient-state buffers that swap roles, and frame gradients per chunk
    Signal go(N);
    for (int i = 0; i < N; i++) go[i] = 2.0f * uniform() - 1.0f;
    float *d_go = nullptr, *d_gin[2] = {}, *d_gstate[2][2] = {}, *d_g[2][K][5] = {};
    HIP_OK(hipMalloc((void **)&d_go, bytes));
    HIP_OK(hipMemcpy(d_go, go.data(), bytes, hipMemcpyHostToDevice));
    for (int s = 0; s < 2; s++) {
        HIP_OK(hipMalloc((void **)&d_gin[s], bytes));
        for (float *&p : d_gstate[s]) HIP_OK(hipMalloc((void **)&p, PAIRS * sizeof(float)));
        for (int k = 0; k < K; k++)
            for (int c = 0; c < 5; c++) HIP_OK(hipMalloc((void **)&d_g[s][k][c], (size_t)count * sizeof(float)));
    }
    bool ok = true;
    for (bool causal : {true, false}) {
        const std::string d = causal ? "+x" : "-x";
        try {
            RecFilterDim whole("x", N);
            RecFilterVarying2 W(causal ? +whole : -whole);
            W.realize_cascade_frames(d_in, frames_at(0), HOP, d_out[2]);
            for (int step = 0; step < CHUNKS; step++) {
                const int c = causal ? step : CHUNKS - 1 - step, n = LENGTH[c], at = START[c], chunk_frames = (n + HOP - 1) / HOP + 1;
                const std::vector<rf_var2_section> frames = frames_at(at);
                const std::string what = d + " chunk " + std::to_string(c);
                // the C call, on a plan of its own
                rf_var2_signal_desc desc{};
                desc.abi = RF_ABI; desc.length = n; desc.n_lines = 1; desc.stride = n; desc.causal = causal ? 1 : 0; desc.device = -1;
                rf_var2_plan *plan = nullptr;
                RF_CALL(rf_var2_plan_create_signal(&desc, &plan));
                void *const kept_c[K - 1] = {d_kept[1][0] + at, d_kept[1][1] + at};
                RF_CALL(rf_var2_plan_execute_cascade_frames_stream(plan, d_in + at, frames.data(), K, HOP, chunk_frames, chunk_frames, d_out[1] + at, kept_c,
                                                                   step == 0 ? nullptr : d_state[1][(step + 1) % 2], d_state[1][step % 2], PAIRS, nullptr));
                RecFilterDim x("x", n);
                RecFilterVarying2 F(causal ? +x : -x);
                if (F.cascade_frames_stream_num_kernels(K) != 2 * K + 1 || F.cascade_frames_stream_num_kernels(1) != 3 ||
                    F.cascade_frames_stream_num_kernels(17) != 0 || F.cascade_frames_stream_state_bytes(K) != PAIRS * sizeof(float) ||
                    F.cascade_frames_stream_state_bytes(K, PAIRS - 1) != 0) {
                    std::printf("queries\n");
                    return 1;
                }
                F.realize_cascade_frames_stream(d_in + at, frames, HOP, d_out[0] + at, step == 0 ? nullptr : d_state[0][(step + 1) % 2], d_state[0][step % 2],
                                                {d_kept[0][0] + at, d_kept[0][1] + at});
                HIP_OK(hipDeviceSynchronize());
                ok = same(what + " out", d_out[0] + at, d_out[1] + at, (size_t)n) && ok;
                for (int k = 0; k + 1 < K; k++) ok = same(what + " kept " + std::to_string(k), d_kept[0][k] + at, d_kept[1][k] + at, (size_t)n) && ok;
                ok = same(what + " state", d_state[0][step % 2], d_state[1][step % 2], PAIRS) && ok;
                // the state that leaves: the two last samples, in the recurrence's order, of in, the kept signals and out
                Signal state, signal;
                if (!fetch(state, d_state[0][step % 2], PAIRS)) return 1;
                const float *signals[K + 1] = {d_in + at, d_kept[0][0] + at, d_kept[0][1] + at, d_out[0] + at};
                for (int k = 0; k <= K; k++) {
                    if (!fetch(signal, signals[k], (size_t)n)) return 1;
                    const float last = causal ? signal[n - 1] : signal[0], before = causal ? signal[n - 2] : signal[1];
                    if (std::memcmp(&state[2 * k], &last, 4) != 0 || std::memcmp(&state[2 * k + 1], &before, 4) != 0) {
                        std::printf("%s: pair %d is not the signal's two last samples\n", what.c_str(), k);
                        ok = false;
                    }
                }
                // refusals arrive as exceptions with the library's text
                bool threw = false;
                try { F.realize_cascade_frames_stream(d_in + at, frames, HOP, d_out[0] + at, d_state[0][0], d_state[0][0]); }
                catch (const RecFilterError &e) { threw = std::string(e.what()).find("state_out overlaps state_in") != std::string::npos; }
                if (!threw) { std::printf("state_out == state_in was not refused\n"); return 1; }
                threw = false;
                try { F.realize_cascade_frames_stream(d_in + at, frames, HOP, d_out[0] + at, nullptr, d_state[0][0], {}, 0, PAIRS - 1); }
                catch (const RecFilterError &e) { threw = std::string(e.what()).find("state_stride") != std::string::npos; }
                if (!threw) { std::printf("a short state stride was not refused\n"); return 1; }
                RF_CALL(rf_var2_plan_destroy(plan));
            }
            // the backward, from the chunk fed last back to the first: each chunk's grad_state_in is the grad_state_out of the chunk
            // before it; the state that entered a chunk is what the chunk fed before it left (the forward above left the last state in
            // d_state[.][(CHUNKS - 1) % 2] and the one before it in the other buffer)
            for (int step = CHUNKS - 1; step >= 0; step--) {
                const int c = causal ? step : CHUNKS - 1 - step, n = LENGTH[c], at = START[c], chunk_frames = (n + HOP - 1) / HOP + 1;
                const std::vector<rf_var2_section> frames = frames_at(at);
                const std::string what = d + " backward, chunk " + std::to_string(c);
                const int back = CHUNKS - 1 - step;      // 0 for the chunk fed last
                std::vector<rf_var2_section_grad> grads[2];
                for (int s = 0; s < 2; s++)
                    for (int k = 0; k < K; k++) grads[s].push_back({d_g[s][k][0], d_g[s][k][1], d_g[s][k][2], d_g[s][k][3], d_g[s][k][4]});
                rf_var2_signal_desc desc{};
                desc.abi = RF_ABI; desc.length = n; desc.n_lines = 1; desc.stride = n; desc.causal = causal ? 1 : 0; desc.device = -1;
                rf_var2_plan *plan = nullptr;
                RF_CALL(rf_var2_plan_create_signal(&desc, &plan));
                const void *const kept_c[K - 1] = {d_kept[1][0] + at, d_kept[1][1] + at};
                RF_CALL(rf_var2_plan_backward_cascade_frames_stream(plan, d_in + at, frames.data(), K, HOP, chunk_frames, chunk_frames, kept_c, d_out[1] + at,
                                                                    d_go + at, d_gin[1] + at, grads[1].data(), step == 0 ? nullptr : d_state[1][(step + 1) % 2],
                                                                    back == 0 ? nullptr : d_gstate[1][(back + 1) % 2], d_gstate[1][back % 2], PAIRS, nullptr));
                RecFilterDim x("x", n);
                RecFilterVarying2 F(causal ? +x : -x);
                if (F.cascade_frames_stream_gradient_num_kernels(K, false) != 2 * K + 2 || F.cascade_frames_stream_gradient_num_kernels(K, true) != 3 * K + 2 ||
                    F.cascade_frames_stream_gradient_num_kernels(1, true) != 5 || F.cascade_frames_stream_gradient_num_kernels(17, true) != 0) {
                    std::printf("gradient queries\n");
                    return 1;
                }
                F.gradient_cascade_frames_stream(d_in + at, frames, HOP, {d_kept[0][0] + at, d_kept[0][1] + at}, d_out[0] + at, d_go + at, d_gin[0] + at,
                                                 step == 0 ? nullptr : d_state[0][(step + 1) % 2], back == 0 ? nullptr : d_gstate[0][(back + 1) % 2],
                                                 d_gstate[0][back % 2], grads[0]);
                HIP_OK(hipDeviceSynchronize());
                ok = same(what + " grad_in", d_gin[0] + at, d_gin[1] + at, (size_t)n) && ok;
                ok = same(what + " grad_state_in", d_gstate[0][back % 2], d_gstate[1][back % 2], PAIRS) && ok;
                for (int k = 0; k < K; k++)
                    for (int cc = 0; cc < 5; cc++)
                        ok = same(what + " frame gradient " + std::to_string(cc) + " of section " + std::to_string(k), d_g[0][k][cc], d_g[1][k][cc],
                                  (size_t)chunk_frames) && ok;
                bool threw = false;
                try { F.gradient_cascade_frames_stream(nullptr, frames, HOP, {}, nullptr, d_go + at, d_gin[0] + at, nullptr, d_gstate[0][0], d_gstate[0][0]); }
                catch (const RecFilterError &e) { threw = std::string(e.what()).find("grad_state_in overlaps grad_state_out") != std::string::npos; }
                if (!threw) { std::printf("grad_state_in == grad_state_out was not refused\n"); return 1; }
                RF_CALL(rf_var2_plan_destroy(plan));
            }
            // the chain against the whole signal at once: the same filter to rounding (f32 rounding through poles of radius up to 0.98
            // stays far below 1e-4 of the peak; chunks stitched without the state miss by a share of the peak itself)
            Signal chained, at_once;
            if (!fetch(chained, d_out[0], N) || !fetch(at_once, d_out[2], N)) return 1;
            double peak = 0.0, worst = 0.0;
            for (int i = 0; i < N; i++) {
                peak = std::max(peak, (double)std::fabs(at_once[i]));
                worst = std::max(worst, std::fabs((double)chained[i] - (double)at_once[i]));
            }
            std::printf("%s: chunks against the whole signal, err/peak %.3e\n", d.c_str(), worst / peak);
            if (!(worst <= 1e-4 * peak)) { std::printf("%s: the chain is not the whole signal's filter\n", d.c_str()); ok = false; }
        } catch (const RecFilterError &e) {
            std::printf("RecFilterError: %s\n", e.what());
            return 1;
        }
    }
    (void)hipFree(d_in);
    (void)hipFree(d_go);
    for (int s = 0; s < 2; s++) {
        (void)hipFree(d_gin[s]);
        for (float *p : d_gstate[s]) (void)hipFree(p);
        for (int k = 0; k < K; k++)
            for (int c = 0; c < 5; c++) (void)hipFree(d_g[s][k][c]);
    }
    for (float *p : d_out) (void)hipFree(p);
    for (int s = 0; s < 2; s++) {
        for (float *p : d_kept[s]) (void)hipFree(p);
        for (float *p : d_state[s]) (void)hipFree(p);
    }
    for (int k = 0; k < K; k++)
        for (int c = 0; c < 5; c++) (void)hipFree(d_f[k][c]);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("cascade-frames-stream-frontend-ok\n");
    return 0;
}
