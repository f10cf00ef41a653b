// RecFilterVarying2 (include/recfilter.hpp): one time-varying second-order all-pole scan on ONE signal of 12356 samples (three
// groups of 4096 and a partial tile), +x and -x, against loops in this file: realize, and gradient with the coefficient gradients.
// The bar of tests/var2_cases.py: max abs error over the peak <= max(4 x the f32 serial loop's, 1e-6).
// Compiled and run by tests/test_gpu_var2_signal.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int N = 12356;

template <typename T>
struct Result {
    std::vector<T> out, grad_in, grad_a1, grad_a2;
};

// the causal scan and its adjoint from g = dL/d(out); a1[0], a2[0], a2[1] are never used
template <typename T>
Result<T> causal_loops(const std::vector<float> &in, const std::vector<float> &a1, const std::vector<float> &a2, const std::vector<float> &g) {
    auto c1 = [&](int i) { return (i < 1 || i >= N) ? T(0) : T(a1[(size_t)i]); };
    auto c2 = [&](int i) { return (i < 2 || i >= N) ? T(0) : T(a2[(size_t)i]); };
    Result<T> r;
    r.out.assign(N, T(0)); r.grad_in.assign(N, T(0)); r.grad_a1.assign(N, T(0)); r.grad_a2.assign(N, T(0));
    for (int i = 0; i < N; i++) r.out[i] = T(in[i]) - c1(i) * (i >= 1 ? r.out[i - 1] : T(0)) - c2(i) * (i >= 2 ? r.out[i - 2] : T(0));
    for (int i = N - 1; i >= 0; i--)
        r.grad_in[i] = T(g[i]) - c1(i + 1) * (i + 1 < N ? r.grad_in[i + 1] : T(0)) - c2(i + 2) * (i + 2 < N ? r.grad_in[i + 2] : T(0));
    for (int i = 1; i < N; i++) r.grad_a1[i] = -r.grad_in[i] * r.out[i - 1];
    for (int i = 2; i < N; i++) r.grad_a2[i] = -r.grad_in[i] * r.out[i - 2];
    return r;
}

template <typename V>
V reversed(V v) { std::reverse(v.begin(), v.end()); return v; }

// the anticausal scan: the causal one on the signals reversed
template <typename T>
Result<T> loops(bool causal, const std::vector<float> &in, const std::vector<float> &a1, const std::vector<float> &a2, const std::vector<float> &g) {
    if (causal) return causal_loops<T>(in, a1, a2, g);
    Result<T> r = causal_loops<T>(reversed(in), reversed(a1), reversed(a2), reversed(g));
    return {reversed(r.out), reversed(r.grad_in), reversed(r.grad_a1), reversed(r.grad_a2)};
}

uint32_t rng_state = 20252u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

bool under_bar(const std::string &what, const std::vector<float> &got, const std::vector<double> &want, const std::vector<float> &serial, double peak) {
    double err = 0, err32 = 0;
    for (int i = 0; i < N; i++) {
        if (std::isnan(got[i])) { std::printf("%s: NaN at sample %d\n", what.c_str(), i); return false; }
        if (peak <= 0) continue;
        err = std::max(err, std::fabs((double)got[i] - want[i]));
        err32 = std::max(err32, std::fabs((double)serial[i] - want[i]));
    }
    err /= peak; err32 /= peak;
    const double bar = std::max(4.0 * err32, 1e-6);
    std::printf("%s: err/peak %.3e, f32 serial loop %.3e, bar %.3e\n", what.c_str(), err, err32, bar);
    return err <= bar;
}

double peak_of(const std::vector<double> &v) {
    double p = 0;
    for (double x : v) p = std::max(p, std::fabs(x));
    return p;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

}  // namespace

int main() {
    const size_t bytes = (size_t)N * sizeof(float);
    std::vector<float> in(N), a1(N), a2(N), g(N);
    // a resonator whose pole radius and angle move slowly
    double theta = 1.0, phase = 0.0;
    for (int i = 0; i < N; i++) {
        in[i] = 2.0f * uniform() - 1.0f;
        g[i] = 2.0f * uniform() - 1.0f;
        theta = std::min(std::max(theta + 0.02 * (uniform() - 0.5), 0.2), 2.9);
        phase += 0.002;
        const double r = 0.74 + 0.24 * std::sin(phase);
        a1[i] = (float)(-2.0 * r * std::cos(theta));
        a2[i] = (float)(r * r);
    }
    float *d_in = nullptr, *d_a1 = nullptr, *d_a2 = nullptr, *d_g = nullptr, *d_out = nullptr, *d_gin = nullptr, *d_g1 = nullptr, *d_g2 = nullptr;
    for (float **p : {&d_in, &d_a1, &d_a2, &d_g, &d_out, &d_gin, &d_g1, &d_g2}) HIP_OK(hipMalloc((void **)p, bytes));
    HIP_OK(hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_g, g.data(), bytes, hipMemcpyHostToDevice));
    bool ok = true;
    for (bool causal : {true, false}) {
        // the coefficients the scan masks hold NaN
        std::vector<float> m1 = a1, m2 = a2;
        const float nan = std::numeric_limits<float>::quiet_NaN();
        if (causal) { m1[0] = m2[0] = m2[1] = nan; } else { m1[N - 1] = m2[N - 1] = m2[N - 2] = nan; }
        HIP_OK(hipMemcpy(d_a1, m1.data(), bytes, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_a2, m2.data(), bytes, hipMemcpyHostToDevice));
        std::vector<float> out(N), gin(N), g1(N), g2(N), gin_only(N);
        try {
            RecFilterDim x("x", N);
            RecFilterVarying2 F(causal ? +x : -x);
            F.realize(d_in, d_a1, d_a2, d_out);
            if (F.num_kernels() != 3 || F.gradient_num_kernels(false) != 3 || F.gradient_num_kernels(true) != 4) { std::printf("launch counts\n"); return 1; }
            F.gradient(d_a1, d_a2, nullptr, d_g, d_gin);
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(gin_only.data(), d_gin, bytes, hipMemcpyDeviceToHost));
            F.gradient(d_a1, d_a2, d_out, d_g, d_gin, d_g1, d_g2);
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(out.data(), d_out, bytes, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(gin.data(), d_gin, bytes, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(g1.data(), d_g1, bytes, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(g2.data(), d_g2, bytes, hipMemcpyDeviceToHost));
            // refusals arrive as exceptions with the library's text
            bool threw = false;
            try {
                RecFilterDim x3("x", N + 2);
                RecFilterVarying2 G(+x3);
                G.realize(d_in, d_a1, d_a2, d_out);
            } catch (const RecFilterError &e) { threw = std::string(e.what()).find("multiple of 4") != std::string::npos; }
            if (!threw) { std::printf("a length of %d was not refused\n", N + 2); return 1; }
            threw = false;
            try { F.gradient(d_a1, d_a2, d_out, d_g, d_gin, d_g1, nullptr); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("grad_a1") != std::string::npos; }
            if (!threw) { std::printf("one coefficient gradient without the other was not refused\n"); return 1; }
        } catch (const RecFilterError &e) {
            std::printf("RecFilterError: %s\n", e.what());
            return 1;
        }
        const Result<double> want = loops<double>(causal, in, a1, a2, g);
        const Result<float> serial = loops<float>(causal, in, a1, a2, g);
        const std::string d = causal ? "+x" : "-x";
        ok = under_bar(d + " out", out, want.out, serial.out, 1.0) && ok;
        ok = under_bar(d + " grad_in", gin, want.grad_in, serial.grad_in, peak_of(want.grad_in)) && ok;
        ok = under_bar(d + " grad_a1", g1, want.grad_a1, serial.grad_a1, peak_of(want.grad_a1)) && ok;
        ok = under_bar(d + " grad_a2", g2, want.grad_a2, serial.grad_a2, peak_of(want.grad_a2)) && ok;
        for (int i = 0; i < N; i++)
            if (gin[i] != gin_only[i]) { std::printf("%s: grad_in differs with the coefficient gradients at %d\n", d.c_str(), i); ok = false; break; }
        const int e1 = causal ? 0 : N - 1, e2 = causal ? 1 : N - 2;
        if (g1[e1] != 0.0f || g2[e1] != 0.0f || g2[e2] != 0.0f) { std::printf("%s: a masked coefficient has a gradient\n", d.c_str()); ok = false; }
    }
    for (float *p : {d_in, d_a1, d_a2, d_g, d_out, d_gin, d_g1, d_g2}) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("varying2-frontend-ok\n");
    return 0;
}
