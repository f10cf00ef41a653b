// RecFilterVarying2::realize_cascade_keep / gradient_cascade_kept (include/recfilter.hpp): a cascade of three time-varying
// direct-form-I sections on ONE signal of 12356 samples (three groups of 4096 and a partial tile), +x and -x, against loops in
// this file: the forward, the two kept signals and all 1 + 15 gradients, the forward keeping every section's result and the
// backward rerunning nothing.  The bar of tests/cascade_cases.py: max abs error over the peak <= max(4 x the f32 serial
// cascade's, 1e-6); the forward's peak is the f64 result's.  Compiled and run by tests/test_gpu_cascade_kept.py.
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
constexpr int K = 3;
using Signal = std::vector<float>;
struct Section { Signal c[5]; };      // b0, b1, b2, a1, a2

template <typename T>
struct Result {
    std::vector<T> out, gin, g[K][5], y[K];      // y[k]: section k's result
};

// the causal cascade and its adjoint from go = dL/d(out); b1[0], b2[0], b2[1], a1[0], a2[0], a2[1] of a section are never used
template <typename T>
Result<T> causal_loops(const Signal &in, const Section (&s)[K], const Signal &go) {
    auto at = [&](const std::vector<T> &v, int i) { return (i < 0 || i >= N) ? T(0) : v[(size_t)i]; };
    std::vector<T> y[K + 1];
    y[0].assign(in.begin(), in.end());
    for (int k = 0; k < K; k++) {
        auto one = [&](int j, int i) { return (i < 1 || i >= N) ? T(0) : T(s[k].c[j][(size_t)i]); };
        auto two = [&](int j, int i) { return (i < 2 || i >= N) ? T(0) : T(s[k].c[j][(size_t)i]); };
        const std::vector<T> &x = y[k];
        std::vector<T> &o = y[k + 1];
        o.assign(N, T(0));
        for (int i = 0; i < N; i++) {
            const T v = T(s[k].c[0][i]) * x[i] + one(1, i) * at(x, i - 1) + two(2, i) * at(x, i - 2);
            o[i] = v - one(3, i) * at(o, i - 1) - two(4, i) * at(o, i - 2);
        }
    }
    Result<T> r;
    r.out = y[K];
    for (int k = 0; k < K; k++) r.y[k] = y[k + 1];
    std::vector<T> g(go.begin(), go.end()), lam(N, T(0));
    for (int k = K - 1; k >= 0; k--) {
        auto one = [&](int j, int i) { return (i < 1 || i >= N) ? T(0) : T(s[k].c[j][(size_t)i]); };
        auto two = [&](int j, int i) { return (i < 2 || i >= N) ? T(0) : T(s[k].c[j][(size_t)i]); };
        const std::vector<T> &x = y[k], &o = y[k + 1];
        for (auto &q : r.g[k]) q.assign(N, T(0));
        for (int i = N - 1; i >= 0; i--) lam[i] = g[i] - one(3, i + 1) * at(lam, i + 1) - two(4, i + 2) * at(lam, i + 2);
        for (int i = 0; i < N; i++) {
            g[i] = T(s[k].c[0][i]) * lam[i] + one(1, i + 1) * at(lam, i + 1) + two(2, i + 2) * at(lam, i + 2);
            r.g[k][0][i] = lam[i] * x[i];
            if (i >= 1) { r.g[k][1][i] = lam[i] * x[i - 1]; r.g[k][3][i] = -lam[i] * o[i - 1]; }
            if (i >= 2) { r.g[k][2][i] = lam[i] * x[i - 2]; r.g[k][4][i] = -lam[i] * o[i - 2]; }
        }
    }
    r.gin = g;
    return r;
}

template <typename V>
V reversed(V v) { std::reverse(v.begin(), v.end()); return v; }

// the anticausal cascade: the causal one on the signals reversed
template <typename T>
Result<T> loops(bool causal, const Signal &in, const Section (&s)[K], const Signal &go) {
    if (causal) return causal_loops<T>(in, s, go);
    Section rs[K];
    for (int k = 0; k < K; k++)
        for (int j = 0; j < 5; j++) rs[k].c[j] = reversed(s[k].c[j]);
    Result<T> r = causal_loops<T>(reversed(in), rs, reversed(go));
    r.out = reversed(r.out); r.gin = reversed(r.gin);
    for (auto &y : r.y) y = reversed(y);
    for (auto &section : r.g)
        for (auto &g : section) g = reversed(g);
    return r;
}

uint32_t rng_state = 20311u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

template <typename T>
bool under_bar(const std::string &what, const Signal &got, const std::vector<double> &want, const std::vector<T> &serial) {
    double err = 0, err32 = 0, peak = 0;
    for (int i = 0; i < N; i++) {
        if (std::isnan(got[i])) { std::printf("%s: NaN at sample %d\n", what.c_str(), i); return false; }
        err = std::max(err, std::fabs((double)got[i] - want[i]));
        err32 = std::max(err32, std::fabs((double)serial[i] - want[i]));
        peak = std::max(peak, std::fabs(want[i]));
    }
    if (peak <= 0) { std::printf("%s: the reference is all zero\n", what.c_str()); return false; }
    err /= peak; err32 /= peak;
    const double bar = std::max(4.0 * err32, 1e-6);
    std::printf("%s: err/peak %.3e, f32 serial cascade %.3e, bar %.3e\n", what.c_str(), err, err32, bar);
    return err <= bar;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

}  // namespace

int main() {
    const size_t bytes = (size_t)N * sizeof(float);
    Signal in(N), go(N);
    Section s[K];
    for (Section &q : s)
        for (Signal &c : q.c) c.resize(N);
    // per section: a resonator whose pole radius and angle move slowly, behind a moving pair of zeros with a moving gain
    for (int i = 0; i < N; i++) { in[i] = 2.0f * uniform() - 1.0f; go[i] = 2.0f * uniform() - 1.0f; }
    for (int k = 0; k < K; k++) {
        double theta = 1.0 + 0.4 * k, phi = 1.7 - 0.3 * k, phase = 0.9 * k;
        for (int i = 0; i < N; i++) {
            theta = std::min(std::max(theta + 0.02 * (uniform() - 0.5), 0.2), 2.9);
            phi = std::min(std::max(phi + 0.02 * (uniform() - 0.5), 0.2), 2.9);
            phase += 0.002;
            const double r = 0.74 + 0.24 * std::sin(phase), q = 0.65 + 0.35 * std::sin(1.7 * phase + 1.0), g = 1.0 + 0.5 * std::sin(0.6 * phase + 2.0);
            s[k].c[0][i] = (float)g;
            s[k].c[1][i] = (float)(-2.0 * g * q * std::cos(phi));
            s[k].c[2][i] = (float)(g * q * q);
            s[k].c[3][i] = (float)(-2.0 * r * std::cos(theta));
            s[k].c[4][i] = (float)(r * r);
        }
    }
    float *d_in = nullptr, *d_go = nullptr, *d_out = nullptr, *d_gin = nullptr, *d_c[K][5] = {}, *d_g[K][5] = {}, *d_kept[K - 1] = {};
    for (float **p : {&d_in, &d_go, &d_out, &d_gin}) HIP_OK(hipMalloc((void **)p, bytes));
    for (float *&p : d_kept) HIP_OK(hipMalloc((void **)&p, bytes));
    const std::vector<void *> kept(d_kept, d_kept + K - 1);
    const std::vector<const void *> kept_read(d_kept, d_kept + K - 1);
    for (auto &section : d_c)
        for (float *&p : section) HIP_OK(hipMalloc((void **)&p, bytes));
    for (auto &section : d_g)
        for (float *&p : section) HIP_OK(hipMalloc((void **)&p, bytes));
    HIP_OK(hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_go, go.data(), bytes, hipMemcpyHostToDevice));
    std::vector<rf_var2_section> sections(K);
    std::vector<rf_var2_section_grad> grads(K);
    for (int k = 0; k < K; k++) {
        sections[k] = {d_c[k][0], d_c[k][1], d_c[k][2], d_c[k][3], d_c[k][4]};
        grads[k] = {d_g[k][0], d_g[k][1], d_g[k][2], d_g[k][3], d_g[k][4]};
    }
    bool ok = true;
    const char *names[5] = {"grad_b0", "grad_b1", "grad_b2", "grad_a1", "grad_a2"};
    for (bool causal : {true, false}) {
        // the coefficients a section masks hold NaN
        const float nan = std::numeric_limits<float>::quiet_NaN();
        const int e1 = causal ? 0 : N - 1, e2 = causal ? 1 : N - 2;
        for (int k = 0; k < K; k++) {
            Section m = s[k];
            m.c[1][e1] = m.c[3][e1] = m.c[2][e1] = m.c[2][e2] = m.c[4][e1] = m.c[4][e2] = nan;
            for (int j = 0; j < 5; j++) HIP_OK(hipMemcpy(d_c[k][j], m.c[j].data(), bytes, hipMemcpyHostToDevice));
        }
        Signal out(N), gin_only(N), gin(N), g[K][5], y[K - 1];
        for (Signal &q : y) q.resize(N);
        for (auto &section : g)
            for (Signal &q : section) q.resize(N);
        try {
            RecFilterDim x("x", N);
            RecFilterVarying2 F(causal ? +x : -x);
            if (F.cascade_num_kernels(K) != 2 * K + 1 || F.cascade_kept_gradient_num_kernels(K, false) != 2 * K + 2 ||
                F.cascade_kept_gradient_num_kernels(K, true) != 3 * K + 1 || F.cascade_kept_gradient_num_kernels(1, true) != 4 ||
                F.cascade_kept_gradient_bytes(K) != 2 * bytes || F.cascade_kept_gradient_bytes(1) != bytes ||
                F.cascade_gradient_bytes(K) != (K + 1) * bytes) { std::printf("queries\n"); return 1; }
            F.realize_cascade_keep(d_in, sections, d_out, kept);
            F.gradient_cascade_kept(nullptr, sections, {}, nullptr, d_go, d_gin);      // nothing of the forward is read
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(gin_only.data(), d_gin, bytes, hipMemcpyDeviceToHost));
            F.gradient_cascade_kept(d_in, sections, kept_read, d_out, d_go, d_gin, grads);
            HIP_OK(hipDeviceSynchronize());
            for (int k = 0; k + 1 < K; k++) HIP_OK(hipMemcpy(y[k].data(), d_kept[k], bytes, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(out.data(), d_out, bytes, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(gin.data(), d_gin, bytes, hipMemcpyDeviceToHost));
            for (int k = 0; k < K; k++)
                for (int j = 0; j < 5; j++) HIP_OK(hipMemcpy(g[k][j].data(), d_g[k][j], bytes, hipMemcpyDeviceToHost));
            // refusals arrive as exceptions with the library's text
            bool threw = false;
            try { F.realize_cascade_keep(d_in, sections, d_in, kept); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("in == out") != std::string::npos; }
            if (!threw) { std::printf("in == out was not refused\n"); return 1; }
            threw = false;
            try { F.realize_cascade_keep(d_in, sections, d_out, {d_kept[0], d_out}); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("kept plane 1") != std::string::npos; }
            if (!threw) { std::printf("a kept signal that is the output was not refused\n"); return 1; }
            threw = false;
            try { F.gradient_cascade_kept(d_in, sections, {}, d_out, d_go, d_gin, grads); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("kept 0") != std::string::npos; }
            if (!threw) { std::printf("coefficient gradients without the kept signals were not refused\n"); return 1; }
            threw = false;
            std::vector<rf_var2_section_grad> partial = grads;
            partial[1].b2 = nullptr;
            try { F.gradient_cascade_kept(d_in, sections, kept_read, d_out, d_go, d_gin, partial); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("section 1") != std::string::npos; }
            if (!threw) { std::printf("a partial set of coefficient gradients was not refused by its section\n"); return 1; }
            threw = false;
        } catch (const RecFilterError &e) {
            std::printf("RecFilterError: %s\n", e.what());
            return 1;
        }
        const Result<double> want = loops<double>(causal, in, s, go);
        const Result<float> serial = loops<float>(causal, in, s, go);
        const std::string d = causal ? "+x" : "-x";
        ok = under_bar(d + " out", out, want.out, serial.out) && ok;
        ok = under_bar(d + " grad_in", gin, want.gin, serial.gin) && ok;
        for (int k = 0; k + 1 < K; k++) ok = under_bar(d + " kept " + std::to_string(k), y[k], want.y[k], serial.y[k]) && ok;
        for (int k = 0; k < K; k++)
            for (int j = 0; j < 5; j++) ok = under_bar(d + " section " + std::to_string(k) + " " + names[j], g[k][j], want.g[k][j], serial.g[k][j]) && ok;
        for (int i = 0; i < N; i++)
            if (gin[i] != gin_only[i]) { std::printf("%s: grad_in differs with the coefficient gradients at %d\n", d.c_str(), i); ok = false; break; }
        for (int k = 0; k < K; k++)
            if (g[k][1][e1] != 0.0f || g[k][3][e1] != 0.0f || g[k][2][e1] != 0.0f || g[k][2][e2] != 0.0f || g[k][4][e1] != 0.0f || g[k][4][e2] != 0.0f) {
                std::printf("%s: a masked coefficient of section %d has a gradient\n", d.c_str(), k);
                ok = false;
            }
    }
    for (float *p : {d_in, d_go, d_out, d_gin}) (void)hipFree(p);
    for (float *p : d_kept) (void)hipFree(p);
    for (auto &section : d_c)
        for (float *p : section) (void)hipFree(p);
    for (auto &section : d_g)
        for (float *p : section) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("cascade-kept-frontend-ok\n");
    return 0;
}
