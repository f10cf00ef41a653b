// RecFilterVarying(x) (include/recfilter.hpp): +x -x with per-sample feedback on ONE signal of 12616 samples (three groups of 4096
// and a partial tile), against loops in this file: realize, realize_power, and gradient with the weight gradient.  The bar of
// tests/test_gpu_var_scans.py: max abs error over the peak <= max(4 x the f32 serial loop's, 1e-6).
// Compiled and run by tests/test_gpu_var_signal.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int N = 12616;

template <typename T>
struct Result {
    std::vector<T> out, grad_in, grad_w;
};

// +x then -x with the masked weights wt(i) (0 at i <= 0 and i >= N), and the adjoint of the two from g = dL/d(out)
template <typename T>
Result<T> loops(const std::vector<float> &in, const std::vector<T> &w, const std::vector<float> &g) {
    auto wt = [&](int i) { return (i <= 0 || i >= N) ? T(0) : w[(size_t)i]; };
    std::vector<T> x(in.begin(), in.end()), y1(N), y2(N), mu(N), g1(N), lam(N);
    Result<T> r;
    r.grad_in.resize(N); r.grad_w.assign(N, T(0));
    T acc = 0;
    for (int i = 0; i < N; i++) { acc = (T(1) - wt(i)) * x[i] + wt(i) * acc; y1[i] = acc; }
    acc = 0;
    for (int i = N - 1; i >= 0; i--) { acc = (T(1) - wt(i + 1)) * y1[i] + wt(i + 1) * acc; y2[i] = acc; }
    r.out = y2;
    // the adjoint of the anticausal scan: causal, unit gain
    acc = 0;
    for (int i = 0; i < N; i++) { acc = T(g[i]) + wt(i) * acc; mu[i] = acc; }
    for (int i = 0; i < N; i++) g1[i] = (T(1) - wt(i + 1)) * mu[i];
    for (int i = 1; i < N; i++) r.grad_w[i] = mu[i - 1] * (y2[i] - y1[i - 1]);
    // the adjoint of the causal scan: anticausal, unit gain
    acc = 0;
    for (int i = N - 1; i >= 0; i--) { acc = g1[i] + wt(i + 1) * acc; lam[i] = acc; }
    for (int i = 0; i < N; i++) r.grad_in[i] = (T(1) - wt(i)) * lam[i];
    for (int i = 1; i < N; i++) r.grad_w[i] = r.grad_w[i] + lam[i] * (y1[i - 1] - x[i]);
    return r;
}

uint32_t rng_state = 20251u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

bool under_bar(const char *what, const std::vector<float> &got, const std::vector<double> &want, const std::vector<float> &serial) {
    double peak = 0, err = 0, err32 = 0;
    for (int i = 0; i < N; i++) {
        if (std::isnan(got[i])) { std::printf("%s: NaN at sample %d\n", what, i); return false; }
        peak = std::max(peak, std::fabs(want[i]));
        err = std::max(err, std::fabs((double)got[i] - want[i]));
        err32 = std::max(err32, std::fabs((double)serial[i] - want[i]));
    }
    err /= peak; err32 /= peak;
    const double bar = std::max(4.0 * err32, 1e-6);
    std::printf("%s: err/peak %.3e, f32 serial loop %.3e, bar %.3e\n", what, err, err32, bar);
    return err <= bar;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

}  // namespace

int main() {
    const size_t bytes = (size_t)N * sizeof(float);
    const float base = 0.9f, l = (float)std::log2((double)base);
    std::vector<float> in(N), w(N), d(N), g(N);
    for (auto &v : in) v = 2.0f * uniform() - 1.0f;
    for (auto &v : w) v = std::sqrt(std::sqrt(uniform()));
    for (auto &v : d) { const float u = uniform(); v = 1.0f + 30.0f * u * u * u * u; }
    for (auto &v : g) v = 2.0f * uniform() - 1.0f;
    w[0] = d[0] = std::numeric_limits<float>::quiet_NaN();      // element 0 is never used
    float *d_in = nullptr, *d_w = nullptr, *d_d = nullptr, *d_g = nullptr, *d_out = nullptr, *d_gin = nullptr, *d_gw = nullptr;
    for (float **p : {&d_in, &d_w, &d_d, &d_g, &d_out, &d_gin, &d_gw}) HIP_OK(hipMalloc((void **)p, bytes));
    HIP_OK(hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_w, w.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_d, d.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_g, g.data(), bytes, hipMemcpyHostToDevice));
    std::vector<float> out(N), out_power(N), gin(N), gw(N);
    try {
        RecFilterDim x("x", N);
        RecFilterVarying F(x);
        F.add_scan(+x, 0); F.add_scan(-x, 0);
        F.realize({d_in}, {d_w}, {d_out});
        HIP_OK(hipDeviceSynchronize());
        if (F.num_kernels() != 3) { std::printf("expected 3 launches, the plan has %d\n", F.num_kernels()); return 1; }
        if (F.gradient_num_kernels(false) != 6 || F.gradient_num_kernels(true) != 14) { std::printf("gradient launch counts\n"); return 1; }
        HIP_OK(hipMemcpy(out.data(), d_out, bytes, hipMemcpyDeviceToHost));
        F.realize_power({d_in}, {d_d}, {base}, {d_out});
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out_power.data(), d_out, bytes, hipMemcpyDeviceToHost));
        F.gradient({d_in}, {d_w}, {d_g}, {d_gin}, {d_gw});
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(gin.data(), d_gin, bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(gw.data(), d_gw, bytes, hipMemcpyDeviceToHost));
        // refusals arrive as exceptions with the library's text
        bool threw = false;
        try {
            RecFilterDim x3("x", N + 2);
            RecFilterVarying G(x3);
            G.add_scan(+x3, 0);
            G.realize({d_in}, {d_w}, {d_out});
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("multiple of 4") != std::string::npos; }
        if (!threw) { std::printf("a length of %d was not refused\n", N + 2); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    std::vector<double> w64(w.begin(), w.end()), p64(N);
    std::vector<float> p32(N);
    for (int i = 0; i < N; i++) { p64[i] = std::exp2((double)d[i] * (double)l); p32[i] = std::exp2(d[i] * l); }
    const Result<double> want = loops<double>(in, w64, g), want_power = loops<double>(in, p64, g);
    const Result<float> serial = loops<float>(in, w, g), serial_power = loops<float>(in, p32, g);
    bool ok = under_bar("signal", out, want.out, serial.out);
    ok = under_bar("signal, power form", out_power, want_power.out, serial_power.out) && ok;
    ok = under_bar("signal, grad_in", gin, want.grad_in, serial.grad_in) && ok;
    ok = under_bar("signal, grad_w", gw, want.grad_w, serial.grad_w) && ok;
    if (gw[0] != 0.0f) { std::printf("element 0 of the weight gradient is %g\n", gw[0]); ok = false; }
    for (float *p : {d_in, d_w, d_d, d_g, d_out, d_gin, d_gw}) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("varying-signal-frontend-ok\n");
    return 0;
}
