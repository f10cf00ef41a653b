// RecFilterVarying2::realize_cascade_frames / gradient_cascade_frames (include/recfilter.hpp): a cascade of three direct-form-I
// sections whose coefficients are control-rate frames, on ONE signal of 12356 samples (three groups of 4096 and a partial tile),
// hops 64 and 8192, +x and -x, against the C calls on a plan of its own BIT FOR BIT: the plain forward, the keeping forward (out
// and both kept signals), the backward without frame gradients (nothing of the forward handed in) and with them (grad_in and the
// fifteen frame gradients).  What the C calls compute is pinned by tests/test_gpu_cascade_frames.py, which compiles and runs this.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int N = 12356, K = 3;
using Signal = std::vector<float>;

uint32_t rng_state = 20262u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)
#define RF_CALL(e) do { if ((e) != RF_OK) { std::printf("line %d: %s\n", __LINE__, rf_last_error_string()); return 1; } } while (0)

// count floats of two device arrays, bit for bit; NaN anywhere fails
bool same(const std::string &what, const float *a, const float *b, size_t count) {
    Signal x(count), y(count);
    if (hipMemcpy(x.data(), a, count * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(y.data(), b, count * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { std::printf("%s: copy failed\n", what.c_str()); return false; }
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
    Signal in(N), go(N);
    for (int i = 0; i < N; i++) {
        in[i] = 2.0f * uniform() - 1.0f;
        go[i] = 2.0f * uniform() - 1.0f;
    }
    // signals: in, grad_out; then for the front-end ([0]) and the C calls ([1]): out, out of the keeping forward, two kept signals, grad_in
    float *d_in = nullptr, *d_go = nullptr, *d_out[2] = {}, *d_keep_out[2] = {}, *d_kept[2][K - 1] = {}, *d_gin[2] = {};
    for (float **p : {&d_in, &d_go}) HIP_OK(hipMalloc((void **)p, bytes));
    for (int s = 0; s < 2; s++)
        for (float **p : {&d_out[s], &d_keep_out[s], &d_kept[s][0], &d_kept[s][1], &d_gin[s]}) HIP_OK(hipMalloc((void **)p, bytes));
    HIP_OK(hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_go, go.data(), bytes, hipMemcpyHostToDevice));
    bool ok = true;
    for (int hop : {64, 8192}) {
        const int count = (N + hop - 1) / hop + 1;
        const size_t frame_bytes = (size_t)count * sizeof(float);
        // three resonators whose pole radius and angle move from frame to frame, each behind a moving pair of zeros
        float *d_f[K][5] = {}, *d_g[2][K][5] = {};
        std::vector<rf_var2_section> frames;
        std::vector<rf_var2_section_grad> grads[2];
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
                HIP_OK(hipMalloc((void **)&d_f[k][c], frame_bytes));
                HIP_OK(hipMemcpy(d_f[k][c], f[c].data(), frame_bytes, hipMemcpyHostToDevice));
                for (int s = 0; s < 2; s++) HIP_OK(hipMalloc((void **)&d_g[s][k][c], frame_bytes));
            }
            frames.push_back({d_f[k][0], d_f[k][1], d_f[k][2], d_f[k][3], d_f[k][4]});
            for (int s = 0; s < 2; s++) grads[s].push_back({d_g[s][k][0], d_g[s][k][1], d_g[s][k][2], d_g[s][k][3], d_g[s][k][4]});
        }
        for (bool causal : {true, false}) {
            const std::string d = std::string(causal ? "+x" : "-x") + " hop " + std::to_string(hop);
            // the C calls, on a plan of their own
            rf_var2_signal_desc desc{};
            desc.abi = RF_ABI; desc.length = N; desc.n_lines = 1; desc.stride = N; desc.causal = causal ? 1 : 0; desc.device = -1;
            rf_var2_plan *plan = nullptr;
            RF_CALL(rf_var2_plan_create_signal(&desc, &plan));
            void *const kept_c[K - 1] = {d_kept[1][0], d_kept[1][1]};
            const void *const kept_c_read[K - 1] = {d_kept[1][0], d_kept[1][1]};
            RF_CALL(rf_var2_plan_execute_cascade_frames(plan, d_in, frames.data(), K, hop, count, count, d_out[1], nullptr, nullptr));
            RF_CALL(rf_var2_plan_execute_cascade_frames(plan, d_in, frames.data(), K, hop, count, count, d_keep_out[1], kept_c, nullptr));
            RF_CALL(rf_var2_plan_backward_cascade_frames(plan, nullptr, frames.data(), K, hop, count, count, nullptr, nullptr, d_go, d_gin[1], nullptr, nullptr));
            try {
                RecFilterDim x("x", N);
                RecFilterVarying2 F(causal ? +x : -x);
                if (F.cascade_frames_num_kernels(K) != 2 * K + 1 || F.cascade_frames_num_kernels(1) != 3 || F.cascade_frames_num_kernels(17) != 0 ||
                    F.cascade_frames_gradient_num_kernels(K, false) != 2 * K + 2 || F.cascade_frames_gradient_num_kernels(K, true) != 3 * K + 2 ||
                    F.cascade_frames_gradient_bytes(K, hop) != 2 * bytes + (size_t)K * 80u * (size_t)((N + std::min(hop, 1024) - 1) / std::min(hop, 1024)) ||
                    F.cascade_frames_gradient_bytes(K, 480) != 0) {
                    std::printf("queries\n");
                    return 1;
                }
                F.realize_cascade_frames(d_in, frames, hop, d_out[0]);
                F.realize_cascade_frames(d_in, frames, hop, d_keep_out[0], {d_kept[0][0], d_kept[0][1]});
                F.gradient_cascade_frames(nullptr, frames, hop, {}, nullptr, d_go, d_gin[0]);
                HIP_OK(hipDeviceSynchronize());
                ok = same(d + " out", d_out[0], d_out[1], N) && ok;
                ok = same(d + " out, keeping", d_keep_out[0], d_keep_out[1], N) && ok;
                ok = same(d + " out, keeping or not", d_keep_out[0], d_out[0], N) && ok;
                for (int k = 0; k + 1 < K; k++) ok = same(d + " kept " + std::to_string(k), d_kept[0][k], d_kept[1][k], N) && ok;
                ok = same(d + " grad_in alone", d_gin[0], d_gin[1], N) && ok;
                F.gradient_cascade_frames(d_in, frames, hop, {d_kept[0][0], d_kept[0][1]}, d_keep_out[0], d_go, d_gin[0], grads[0]);
                RF_CALL(rf_var2_plan_backward_cascade_frames(plan, d_in, frames.data(), K, hop, count, count, kept_c_read, d_keep_out[1], d_go, d_gin[1],
                                                             grads[1].data(), nullptr));
                HIP_OK(hipDeviceSynchronize());
                ok = same(d + " grad_in", d_gin[0], d_gin[1], N) && ok;
                for (int k = 0; k < K; k++)
                    for (int c = 0; c < 5; c++)
                        ok = same(d + " frame gradient " + std::to_string(c) + " of section " + std::to_string(k), d_g[0][k][c], d_g[1][k][c], (size_t)count) && ok;
                // refusals arrive as exceptions with the library's text
                bool threw = false;
                try { F.realize_cascade_frames(d_in, frames, hop, d_in); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("in == out") != std::string::npos; }
                if (!threw) { std::printf("in == out was not refused\n"); return 1; }
                threw = false;
                try { F.realize_cascade_frames(d_in, frames, 480, d_out[0]); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("power of two") != std::string::npos; }
                if (!threw) { std::printf("hop 480 was not refused\n"); return 1; }
                threw = false;
                try { F.realize_cascade_frames(d_in, frames, hop, d_out[0], {d_kept[0][0]}); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("kept") != std::string::npos; }
                if (!threw) { std::printf("one kept signal for three sections was not refused\n"); return 1; }
                threw = false;
                std::vector<rf_var2_section_grad> mix = grads[0];
                mix[1].b1 = nullptr;
                try { F.gradient_cascade_frames(d_in, frames, hop, {d_kept[0][0], d_kept[0][1]}, d_keep_out[0], d_go, d_gin[0], mix); }
                catch (const RecFilterError &e) { threw = std::string(e.what()).find("all given or all null") != std::string::npos; }
                if (!threw) { std::printf("a mix of frame gradients was not refused\n"); return 1; }
            } catch (const RecFilterError &e) {
                std::printf("RecFilterError: %s\n", e.what());
                return 1;
            }
            RF_CALL(rf_var2_plan_destroy(plan));
        }
        for (int k = 0; k < K; k++)
            for (int c = 0; c < 5; c++) {
                (void)hipFree(d_f[k][c]);
                for (int s = 0; s < 2; s++) (void)hipFree(d_g[s][k][c]);
            }
    }
    for (float *p : {d_in, d_go}) (void)hipFree(p);
    for (int s = 0; s < 2; s++)
        for (float *p : {d_out[s], d_keep_out[s], d_kept[s][0], d_kept[s][1], d_gin[s]}) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("cascade-frames-frontend-ok\n");
    return 0;
}
