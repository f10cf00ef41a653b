// RecFilterVarying2::realize_biquad_frames / gradient_biquad_frames (include/recfilter.hpp): one direct-form-I section whose five
// coefficients are control-rate frames, on ONE signal of 12356 samples (three groups of 4096 and a partial tile), hops 64 and 8192,
// +x and -x, against loops in this file on the interpolated coefficients: the forward, grad_in and the five frame gradients (the
// per-sample gradients contracted with the interpolation's transpose in double).  The bar of tests/frames_cases.py: max abs error
// over the peak <= max(4 x the f32 serial loop's, 1e-6); the forward's peak is that of the f64 feed-forward part.  Compiled and run
// by tests/test_gpu_biquad_frames.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int N = 12356;
using Signal = std::vector<float>;

template <typename T>
struct Result {
    std::vector<T> v, out, g[6];      // g: grad_in, then the per-sample grad_b0, grad_b1, grad_b2, grad_a1, grad_a2
};

// c[n] = fma(k / hop, c[j+1] - c[j], c[j]) at n = j * hop + k, in T (float: the difference rounded once, then one fma)
template <typename T>
std::vector<T> expand(const Signal &frames, int hop) {
    std::vector<T> c(N);
    for (int n = 0; n < N; n++) {
        const int j = n / hop, k = n % hop;
        const T c0 = T(frames[(size_t)j]), d = T(frames[(size_t)j + 1]) - c0;
        c[n] = std::fma(T(k) / T(hop), d, c0);
    }
    return c;
}

// the transpose of expand, in double
std::vector<double> contract(const std::vector<double> &g, int hop, int count) {
    std::vector<double> out((size_t)count, 0.0);
    for (int n = 0; n < N; n++) {
        const int j = n / hop, k = n % hop;
        out[(size_t)j] += (1.0 - (double)k / hop) * g[n];
        out[(size_t)j + 1] += ((double)k / hop) * g[n];
    }
    return out;
}

// the causal section and its adjoint from go = dL/d(out); c: b0, b1, b2, a1, a2 at audio rate
template <typename T>
Result<T> causal_loops(const Signal &in, const std::vector<T> (&c)[5], const Signal &go) {
    auto one = [&](int k, int i) { return (i < 1 || i >= N) ? T(0) : c[k][(size_t)i]; };
    auto two = [&](int k, int i) { return (i < 2 || i >= N) ? T(0) : c[k][(size_t)i]; };
    auto at = [&](const std::vector<T> &s, int i) { return (i < 0 || i >= N) ? T(0) : s[(size_t)i]; };
    Result<T> r;
    std::vector<T> x(in.begin(), in.end()), lam(N, T(0));
    r.v.assign(N, T(0)); r.out.assign(N, T(0));
    for (auto &g : r.g) g.assign(N, T(0));
    for (int i = 0; i < N; i++) {
        r.v[i] = c[0][i] * x[i] + one(1, i) * at(x, i - 1) + two(2, i) * at(x, i - 2);
        r.out[i] = r.v[i] - one(3, i) * at(r.out, i - 1) - two(4, i) * at(r.out, i - 2);
    }
    for (int i = N - 1; i >= 0; i--) lam[i] = T(go[i]) - one(3, i + 1) * at(lam, i + 1) - two(4, i + 2) * at(lam, i + 2);
    for (int i = 0; i < N; i++) {
        r.g[0][i] = c[0][i] * lam[i] + one(1, i + 1) * at(lam, i + 1) + two(2, i + 2) * at(lam, i + 2);
        r.g[1][i] = lam[i] * x[i];
        if (i >= 1) { r.g[2][i] = lam[i] * x[i - 1]; r.g[4][i] = -lam[i] * r.out[i - 1]; }
        if (i >= 2) { r.g[3][i] = lam[i] * x[i - 2]; r.g[5][i] = -lam[i] * r.out[i - 2]; }
    }
    return r;
}

template <typename V>
V reversed(V v) { std::reverse(v.begin(), v.end()); return v; }

// the anticausal section: the causal one on the signals reversed -- the coefficients expanded by absolute position first
template <typename T>
Result<T> loops(bool causal, const Signal &in, const Signal (&frames)[5], int hop, const Signal &go) {
    std::vector<T> c[5];
    for (int k = 0; k < 5; k++) c[k] = causal ? expand<T>(frames[k], hop) : reversed(expand<T>(frames[k], hop));
    if (causal) return causal_loops<T>(in, c, go);
    Result<T> r = causal_loops<T>(reversed(in), c, reversed(go));
    r.v = reversed(r.v); r.out = reversed(r.out);
    for (auto &g : r.g) g = reversed(g);
    return r;
}

uint32_t rng_state = 20261u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

bool under_bar(const std::string &what, const Signal &got, const std::vector<double> &want, const std::vector<double> &serial, double peak) {
    double err = 0, err32 = 0;
    for (size_t i = 0; i < want.size(); i++) {
        if (std::isnan(got[i])) { std::printf("%s: NaN at %zu\n", what.c_str(), i); return false; }
        err = std::max(err, std::fabs((double)got[i] - want[i]));
        err32 = std::max(err32, std::fabs(serial[i] - want[i]));
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

template <typename T>
std::vector<double> widened(const std::vector<T> &v) { return std::vector<double>(v.begin(), v.end()); }

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

}  // namespace

int main() {
    const size_t bytes = (size_t)N * sizeof(float);
    Signal in(N), go(N);
    for (int i = 0; i < N; i++) {
        in[i] = 2.0f * uniform() - 1.0f;
        go[i] = 2.0f * uniform() - 1.0f;
    }
    float *d_in = nullptr, *d_go = nullptr, *d_out = nullptr, *d_gin = nullptr;
    for (float **p : {&d_in, &d_go, &d_out, &d_gin}) HIP_OK(hipMalloc((void **)p, bytes));
    HIP_OK(hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_go, go.data(), bytes, hipMemcpyHostToDevice));
    bool ok = true;
    const char *names[6] = {"grad_in", "grad_b0", "grad_b1", "grad_b2", "grad_a1", "grad_a2"};
    for (int hop : {64, 8192}) {
        const int count = (N + hop - 1) / hop + 1;
        const size_t frame_bytes = (size_t)count * sizeof(float);
        // a resonator whose pole radius and angle move from frame to frame, behind a moving pair of zeros with a moving gain
        Signal frames[5];
        double theta = 1.0, phi = 1.7;
        for (Signal &s : frames) s.resize((size_t)count);
        for (int j = 0; j < count; j++) {
            theta = std::min(std::max(theta + 0.3 * (uniform() - 0.5), 0.2), 2.9);
            phi = std::min(std::max(phi + 0.3 * (uniform() - 0.5), 0.2), 2.9);
            const double r = 0.74 + 0.24 * std::sin(0.37 * j), q = 0.65 + 0.35 * std::sin(0.61 * j + 1.0), k = 1.0 + 0.5 * std::sin(0.23 * j + 2.0);
            frames[0][j] = (float)k;
            frames[1][j] = (float)(-2.0 * k * q * std::cos(phi));
            frames[2][j] = (float)(k * q * q);
            frames[3][j] = (float)(-2.0 * r * std::cos(theta));
            frames[4][j] = (float)(r * r);
        }
        float *d_f[5] = {}, *d_g[5] = {};
        for (int k = 0; k < 5; k++) {
            HIP_OK(hipMalloc((void **)&d_f[k], frame_bytes));
            HIP_OK(hipMalloc((void **)&d_g[k], frame_bytes));
            HIP_OK(hipMemcpy(d_f[k], frames[k].data(), frame_bytes, hipMemcpyHostToDevice));
        }
        const rf_var2_section section = {d_f[0], d_f[1], d_f[2], d_f[3], d_f[4]};
        const rf_var2_section_grad grads = {d_g[0], d_g[1], d_g[2], d_g[3], d_g[4]};
        for (bool causal : {true, false}) {
            Signal out(N), gin_only(N), gin(N), g[5];
            for (Signal &s : g) s.resize((size_t)count);
            try {
                RecFilterDim x("x", N);
                RecFilterVarying2 F(causal ? +x : -x);
                if (F.frames_count(hop) != count || F.frames_count(480) != 0 || F.biquad_frames_num_kernels() != 3 ||
                    F.biquad_frames_gradient_num_kernels(false) != 4 || F.biquad_frames_gradient_num_kernels(true) != 5 ||
                    F.biquad_frames_gradient_bytes(hop) != bytes + 80u * (size_t)((N + std::min(hop, 1024) - 1) / std::min(hop, 1024))) {
                    std::printf("queries\n");
                    return 1;
                }
                F.realize_biquad_frames(d_in, section, hop, d_out);
                F.gradient_biquad_frames(d_in, section, hop, nullptr, d_go, d_gin);
                HIP_OK(hipDeviceSynchronize());
                HIP_OK(hipMemcpy(gin_only.data(), d_gin, bytes, hipMemcpyDeviceToHost));
                F.gradient_biquad_frames(d_in, section, hop, d_out, d_go, d_gin, &grads);
                HIP_OK(hipDeviceSynchronize());
                HIP_OK(hipMemcpy(out.data(), d_out, bytes, hipMemcpyDeviceToHost));
                HIP_OK(hipMemcpy(gin.data(), d_gin, bytes, hipMemcpyDeviceToHost));
                for (int k = 0; k < 5; k++) HIP_OK(hipMemcpy(g[k].data(), d_g[k], frame_bytes, hipMemcpyDeviceToHost));
                // refusals arrive as exceptions with the library's text
                bool threw = false;
                try { F.realize_biquad_frames(d_in, section, hop, d_in); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("in == out") != std::string::npos; }
                if (!threw) { std::printf("in == out was not refused\n"); return 1; }
                threw = false;
                try { F.realize_biquad_frames(d_in, section, 480, d_out); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("power of two") != std::string::npos; }
                if (!threw) { std::printf("hop 480 was not refused\n"); return 1; }
                threw = false;
                const rf_var2_section_grad mix = {d_g[0], nullptr, d_g[2], d_g[3], d_g[4]};
                try { F.gradient_biquad_frames(d_in, section, hop, d_out, d_go, d_gin, &mix); } catch (const RecFilterError &e) { threw = std::string(e.what()).find("all given or all null") != std::string::npos; }
                if (!threw) { std::printf("a mix of frame gradients was not refused\n"); return 1; }
            } catch (const RecFilterError &e) {
                std::printf("RecFilterError: %s\n", e.what());
                return 1;
            }
            const Result<double> want = loops<double>(causal, in, frames, hop, go);
            const Result<float> serial = loops<float>(causal, in, frames, hop, go);
            const std::string d = std::string(causal ? "+x" : "-x") + " hop " + std::to_string(hop);
            ok = under_bar(d + " out", out, want.out, widened(serial.out), peak_of(want.v)) && ok;
            ok = under_bar(d + " grad_in", gin, want.g[0], widened(serial.g[0]), peak_of(want.g[0])) && ok;
            for (int k = 0; k < 5; k++) {
                const std::vector<double> w = contract(want.g[k + 1], hop, count), s = contract(widened(serial.g[k + 1]), hop, count);
                ok = under_bar(d + " " + names[k + 1], g[k], w, s, peak_of(w)) && ok;
            }
            for (int i = 0; i < N; i++)
                if (gin[i] != gin_only[i]) { std::printf("%s: grad_in differs with the frame gradients at %d\n", d.c_str(), i); ok = false; break; }
        }
        for (float *p : d_f) (void)hipFree(p);
        for (float *p : d_g) (void)hipFree(p);
    }
    for (float *p : {d_in, d_go, d_out, d_gin}) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("biquad-frames-frontend-ok\n");
    return 0;
}
