// RecFilterVarying2::realize_biquad / gradient_biquad (include/recfilter.hpp): one time-varying direct-form-I section on ONE signal
// of 12356 samples (three groups of 4096 and a partial tile), +x and -x, against loops in this file: the forward and all six
// gradients.  The bar of tests/biquad_cases.py: max abs error over the peak <= max(4 x the f32 serial loop's, 1e-6); the forward's
// peak is that of the f64 feed-forward part.  Compiled and run by tests/test_gpu_biquad_signal.py.
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
using Signal = std::vector<float>;

template <typename T>
struct Result {
    std::vector<T> v, out, g[6];      // g: grad_in, grad_b0, grad_b1, grad_b2, grad_a1, grad_a2
};

// the causal section and its adjoint from go = dL/d(out); c: b0, b1, b2, a1, a2 -- b1[0], b2[0], b2[1], a1[0], a2[0], a2[1] are never used
template <typename T>
Result<T> causal_loops(const Signal &in, const Signal (&c)[5], const Signal &go) {
    auto one = [&](int k, int i) { return (i < 1 || i >= N) ? T(0) : T(c[k][(size_t)i]); };
    auto two = [&](int k, int i) { return (i < 2 || i >= N) ? T(0) : T(c[k][(size_t)i]); };
    auto at = [&](const std::vector<T> &s, int i) { return (i < 0 || i >= N) ? T(0) : s[(size_t)i]; };
    Result<T> r;
    std::vector<T> x(in.begin(), in.end()), lam(N, T(0));
    r.v.assign(N, T(0)); r.out.assign(N, T(0));
    for (auto &g : r.g) g.assign(N, T(0));
    for (int i = 0; i < N; i++) {
        r.v[i] = T(c[0][i]) * x[i] + one(1, i) * at(x, i - 1) + two(2, i) * at(x, i - 2);
        r.out[i] = r.v[i] - one(3, i) * at(r.out, i - 1) - two(4, i) * at(r.out, i - 2);
    }
    for (int i = N - 1; i >= 0; i--) lam[i] = T(go[i]) - one(3, i + 1) * at(lam, i + 1) - two(4, i + 2) * at(lam, i + 2);
    for (int i = 0; i < N; i++) {
        r.g[0][i] = T(c[0][i]) * lam[i] + one(1, i + 1) * at(lam, i + 1) + two(2, i + 2) * at(lam, i + 2);
        r.g[1][i] = lam[i] * x[i];
        if (i >= 1) { r.g[2][i] = lam[i] * x[i - 1]; r.g[4][i] = -lam[i] * r.out[i - 1]; }
        if (i >= 2) { r.g[3][i] = lam[i] * x[i - 2]; r.g[5][i] = -lam[i] * r.out[i - 2]; }
    }
    return r;
}

template <typename V>
V reversed(V v) { std::reverse(v.begin(), v.end()); return v; }

// the anticausal section: the causal one on the signals reversed
template <typename T>
Result<T> loops(bool causal, const Signal &in, const Signal (&c)[5], const Signal &go) {
    if (causal) return causal_loops<T>(in, c, go);
    const Signal rc[5] = {reversed(c[0]), reversed(c[1]), reversed(c[2]), reversed(c[3]), reversed(c[4])};
    Result<T> r = causal_loops<T>(reversed(in), rc, reversed(go));
    r.v = reversed(r.v); r.out = reversed(r.out);
    for (auto &g : r.g) g = reversed(g);
    return r;
}

uint32_t rng_state = 20253u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

bool under_bar(const std::string &what, const Signal &got, const std::vector<double> &want, const Signal &serial, double peak) {
    double err = 0, err32 = 0;
    for (int i = 0; i < N; i++) {
        if (std::isnan(got[i])) { std::printf("%s: NaN at sample %d\n", what.c_str(), i); return false; }
        err = std::max(err, std::fabs((double)got[i] - want[i]));
        err32 = std::max(err32, std::fabs((double)serial[i] - want[i]));
    }
    if (peak <= 0) { std::printf("%s: the reference is all zero\n", what.c_str()); return false; }
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
    Signal in(N), go(N), c[5];
    for (Signal &s : c) s.resize(N);
    // a resonator whose pole radius and angle move slowly, behind a moving pair of zeros with a moving gain
    double theta = 1.0, phi = 1.7, phase = 0.0;
    for (int i = 0; i < N; i++) {
        in[i] = 2.0f * uniform() - 1.0f;
        go[i] = 2.0f * uniform() - 1.0f;
        theta = std::min(std::max(theta + 0.02 * (uniform() - 0.5), 0.2), 2.9);
        phi = std::min(std::max(phi + 0.02 * (uniform() - 0.5), 0.2), 2.9);
        phase += 0.002;
        const double r = 0.74 + 0.24 * std::sin(phase), q = 0.65 + 0.35 * std::sin(1.7 * phase + 1.0), k = 1.0 + 0.5 * std::sin(0.6 * phase + 2.0);
        c[0][i] = (float)k;
        c[1][i] = (float)(-2.0 * k * q * std::cos(phi));
        c[2][i] = (float)(k * q * q);
        c[3][i] = (float)(-2.0 * r * std::cos(theta));
        c[4][i] = (float)(r * r);
    }
    float *d_in = nullptr, *d_go = nullptr, *d_out = nullptr, *d_c[5] = {}, *d_g[6] = {};
    for (float **p : {&d_in, &d_go, &d_out}) HIP_OK(hipMalloc((void **)p, bytes));
    for (float *&p : d_c) HIP_OK(hipMalloc((void **)&p, bytes));
    for (float *&p : d_g) HIP_OK(hipMalloc((void **)&p, bytes));
    HIP_OK(hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_go, go.data(), bytes, hipMemcpyHostToDevice));
    bool ok = true;
    const char *names[6] = {"grad_in", "grad_b0", "grad_b1", "grad_b2", "grad_a1", "grad_a2"};
    for (bool causal : {true, false}) {
        // the coefficients the section masks hold NaN
        Signal m[5] = {c[0], c[1], c[2], c[3], c[4]};
        const float nan = std::numeric_limits<float>::quiet_NaN();
        const int e1 = causal ? 0 : N - 1, e2 = causal ? 1 : N - 2;
        m[1][e1] = m[3][e1] = m[2][e1] = m[2][e2] = m[4][e1] = m[4][e2] = nan;
        for (int k = 0; k < 5; k++) HIP_OK(hipMemcpy(d_c[k], m[k].data(), bytes, hipMemcpyHostToDevice));
        Signal out(N), gin_only(N), g[6];
        for (Signal &s : g) s.resize(N);
        try {
            RecFilterDim x("x", N);
            RecFilterVarying2 F(causal ? +x : -x);
            if (F.biquad_num_kernels() != 3 || F.biquad_gradient_num_kernels() != 4 || F.biquad_gradient_bytes() != bytes) { std::printf("queries\n"); return 1; }
            F.realize_biquad(d_in, d_c[0], d_c[1], d_c[2], d_c[3], d_c[4], d_out);
            F.gradient_biquad(d_in, d_c[0], d_c[1], d_c[2], d_c[3], d_c[4], nullptr, d_go, d_g[0]);
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(gin_only.data(), d_g[0], bytes, hipMemcpyDeviceToHost));
            F.gradient_biquad(d_in, d_c[0], d_c[1], d_c[2], d_c[3], d_c[4], d_out, d_go, d_g[0], d_g[1], d_g[2], d_g[3], d_g[4], d_g[5]);
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(out.data(), d_out, bytes, hipMemcpyDeviceToHost));
            for (int k = 0; k < 6; k++) HIP_OK(hipMemcpy(g[k].data(), d_g[k], bytes, hipMemcpyDeviceToHost));
            // refusals arrive as exceptions with the library's text
            bool threw = false;
            try { F.realize_biquad(d_in, d_c[0], d_c[1], d_c[2], d_c[3], d_c[4], d_in); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("in == out") != std::string::npos; }
            if (!threw) { std::printf("in == out was not refused\n"); return 1; }
            threw = false;
            try {
                F.gradient_biquad(d_in, d_c[0], d_c[1], d_c[2], d_c[3], d_c[4], d_out, d_go, d_g[0], d_g[1], nullptr, d_g[3], d_g[4], d_g[5]);
            } catch (const RecFilterError &e) { threw = std::string(e.what()).find("all given or all null") != std::string::npos; }
            if (!threw) { std::printf("a mix of coefficient gradients was not refused\n"); return 1; }
        } catch (const RecFilterError &e) {
            std::printf("RecFilterError: %s\n", e.what());
            return 1;
        }
        const Result<double> want = loops<double>(causal, in, c, go);
        const Result<float> serial = loops<float>(causal, in, c, go);
        const std::string d = causal ? "+x" : "-x";
        ok = under_bar(d + " out", out, want.out, serial.out, peak_of(want.v)) && ok;
        for (int k = 0; k < 6; k++) ok = under_bar(d + " " + names[k], g[k], want.g[k], serial.g[k], peak_of(want.g[k])) && ok;
        for (int i = 0; i < N; i++)
            if (g[0][i] != gin_only[i]) { std::printf("%s: grad_in differs with the coefficient gradients at %d\n", d.c_str(), i); ok = false; break; }
        if (g[2][e1] != 0.0f || g[4][e1] != 0.0f || g[3][e1] != 0.0f || g[3][e2] != 0.0f || g[5][e1] != 0.0f || g[5][e2] != 0.0f) {
            std::printf("%s: a masked coefficient has a gradient\n", d.c_str());
            ok = false;
        }
    }
    for (float *p : {d_in, d_go, d_out}) (void)hipFree(p);
    for (float *p : d_c) (void)hipFree(p);
    for (float *p : d_g) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("biquad-frontend-ok\n");
    return 0;
}
