// RecFilterVarying(x, y, z) and RecFilterSmooth on a volume (include/recfilter.hpp), against loops in this file: +x -x +y -y +z -z
// with per-sample feedback on ONE volume of 24 x 22 x 70 samples (two z tiles, the second partial) -- realize, realize_power,
// gradient and gradient_power with the three weight (exponent) gradients -- then domain_transform_distances_volume and the f32
// smoothing filter with K = 3 on the distance volumes the library forms.  The bar of tests/test_gpu_var_scans.py: max abs error
// over the peak <= max(4 x the f32 serial loops', 1e-6).
// Compiled and run by tests/test_gpu_var_volume.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int W = 24, H = 22, D = 70, N = W * H * D;
constexpr int EXTENT[3] = {W, H, D}, STRIDE[3] = {1, W, W * H};

// calls f(base) for the first sample of every line along `axis`
template <typename F>
void for_lines(int axis, F f) {
    for (int z = 0; z < (axis == 2 ? 1 : D); z++)
        for (int y = 0; y < (axis == 1 ? 1 : H); y++)
            for (int x = 0; x < (axis == 0 ? 1 : W); x++) f((z * H + y) * W + x);
}

// one scan along `axis` with the masked weights wt(i) (0 at i <= 0 and i >= n)
template <typename T>
std::vector<T> scan(const std::vector<T> &x, const std::vector<T> &w, int axis, bool causal) {
    const int n = EXTENT[axis], s = STRIDE[axis];
    std::vector<T> y(N);
    for_lines(axis, [&](int base) {
        auto wt = [&](int i) { return (i <= 0 || i >= n) ? T(0) : w[(size_t)(base + i * s)]; };
        T acc = 0;
        if (causal) for (int i = 0; i < n; i++) { acc = (T(1) - wt(i)) * x[base + i * s] + wt(i) * acc; y[base + i * s] = acc; }
        else for (int i = n - 1; i >= 0; i--) { acc = (T(1) - wt(i + 1)) * x[base + i * s] + wt(i + 1) * acc; y[base + i * s] = acc; }
    });
    return y;
}

// the adjoint of one scan: g = dL/dy in, dL/dx out; the weight gradient is added to gw (element 0 of a line: nothing)
template <typename T>
void scan_adjoint(std::vector<T> &g, const std::vector<T> &x, const std::vector<T> &y, const std::vector<T> &w, int axis, bool causal,
                  std::vector<T> &gw) {
    const int n = EXTENT[axis], s = STRIDE[axis];
    std::vector<T> state(n);
    for_lines(axis, [&](int base) {
        auto wt = [&](int i) { return (i <= 0 || i >= n) ? T(0) : w[(size_t)(base + i * s)]; };
        auto at = [&](int i) { return (size_t)(base + i * s); };
        T acc = 0;
        if (causal) {
            for (int i = n - 1; i >= 0; i--) { acc = g[at(i)] + wt(i + 1) * acc; state[i] = acc; }
            for (int i = 0; i < n; i++) g[at(i)] = (T(1) - wt(i)) * state[i];
            for (int i = 1; i < n; i++) gw[at(i)] += state[i] * (y[at(i - 1)] - x[at(i)]);
        } else {
            for (int i = 0; i < n; i++) { acc = g[at(i)] + wt(i) * acc; state[i] = acc; }
            for (int i = 0; i < n; i++) g[at(i)] = (T(1) - wt(i + 1)) * state[i];
            for (int i = 1; i < n; i++) gw[at(i)] += state[i - 1] * (y[at(i)] - x[at(i - 1)]);
        }
    });
}

template <typename T>
struct Result {
    std::vector<T> out, grad_in, grad_w[3];
};

// +x -x +y -y +z -z on the weight volumes w[0..2], and the adjoint of the six from g = dL/d(out)
template <typename T>
Result<T> loops(const std::vector<float> &in, const std::vector<T> (&w)[3], const std::vector<float> &g) {
    std::vector<T> saved[7];
    saved[0].assign(in.begin(), in.end());
    for (int q = 0; q < 6; q++) saved[q + 1] = scan(saved[q], w[q / 2], q / 2, q % 2 == 0);
    Result<T> r;
    r.out = saved[6];
    r.grad_in.assign(g.begin(), g.end());
    for (auto &v : r.grad_w) v.assign(N, T(0));
    for (int q = 5; q >= 0; q--) scan_adjoint(r.grad_in, saved[q], saved[q + 1], w[q / 2], q / 2, q % 2 == 0, r.grad_w[q / 2]);
    return r;
}

uint32_t rng_state = 20261u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

template <typename G, typename T, typename S>
bool under_bar(const char *what, const std::vector<G> &got, const std::vector<T> &want, const std::vector<S> &serial) {
    double peak = 0, err = 0, err32 = 0;
    for (int i = 0; i < N; i++) {
        if (std::isnan(got[i])) { std::printf("%s: NaN at sample %d\n", what, i); return false; }
        peak = std::max(peak, std::fabs((double)want[i]));
        err = std::max(err, std::fabs((double)got[i] - (double)want[i]));
        err32 = std::max(err32, std::fabs((double)serial[i] - (double)want[i]));
    }
    err /= peak; err32 /= peak;
    const double bar = std::max(4.0 * err32, 1e-6);
    std::printf("%s: err/peak %.3e, f32 serial loops %.3e, bar %.3e\n", what, err, err32, bar);
    return err <= bar;
}

// element 0 of a weight gradient along its axis: exactly +0
bool first_is_zero(const char *what, const std::vector<float> &gw, int axis) {
    bool ok = true;
    for_lines(axis, [&](int base) {
        uint32_t u;
        std::memcpy(&u, &gw[(size_t)base], 4);
        ok = ok && u == 0u;
    });
    if (!ok) std::printf("%s: element 0 along axis %d is not exactly +0\n", what, axis);
    return ok;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

}  // namespace

int main() {
    const size_t bytes = (size_t)N * sizeof(float);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const std::vector<float> bases = {0.9f, 0.98f, 0.8f};
    std::vector<float> in(N), g(N), w[3], d[3];
    for (auto &v : in) v = 2.0f * uniform() - 1.0f;
    for (auto &v : g) v = 2.0f * uniform() - 1.0f;
    for (int k = 0; k < 3; k++) {
        w[k].resize(N); d[k].resize(N);
        for (auto &v : w[k]) v = std::sqrt(std::sqrt(uniform()));
        for (auto &v : d[k]) { const float u = uniform(); v = 1.0f + 30.0f * u * u * u * u; }
        for_lines(k, [&](int base) { w[k][(size_t)base] = d[k][(size_t)base] = nan; });      // element 0 along the axis is never used
    }
    // device volumes: in, g, out, gin; w, d, gw per axis; three distance volumes
    float *d_in = nullptr, *d_g = nullptr, *d_out = nullptr, *d_gin = nullptr, *d_w[3] = {}, *d_d[3] = {}, *d_gw[3] = {}, *d_dist[3] = {};
    for (float **p : {&d_in, &d_g, &d_out, &d_gin}) HIP_OK(hipMalloc((void **)p, bytes));
    for (int k = 0; k < 3; k++)
        for (float **p : {&d_w[k], &d_d[k], &d_gw[k], &d_dist[k]}) HIP_OK(hipMalloc((void **)p, bytes));
    HIP_OK(hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_g, g.data(), bytes, hipMemcpyHostToDevice));
    for (int k = 0; k < 3; k++) {
        HIP_OK(hipMemcpy(d_w[k], w[k].data(), bytes, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_d[k], d[k].data(), bytes, hipMemcpyHostToDevice));
    }
    std::vector<float> out(N), out_power(N), gin(N), gin_power(N), gw[3], gd[3], dist[3], smooth(N);
    std::vector<float> smooth_bases;
    const float scale = 40.0f / 0.5f, spacing_z = 2.5f;
    try {
        RecFilterDim x("x", W), y("y", H), z("z", D);
        RecFilterVarying F(x, y, z);
        F.add_scan(+x, 0); F.add_scan(-x, 0); F.add_scan(+y, 1); F.add_scan(-y, 1); F.add_scan(+z, 2); F.add_scan(-z, 2);
        F.realize({d_in}, {d_w[0], d_w[1], d_w[2]}, {d_out});
        HIP_OK(hipDeviceSynchronize());
        if (F.num_kernels() != 9) { std::printf("expected 9 launches, the plan has %d\n", F.num_kernels()); return 1; }
        if (F.gradient_num_kernels(false) != 18 || F.gradient_num_kernels(true) != 42) { std::printf("gradient launch counts\n"); return 1; }
        HIP_OK(hipMemcpy(out.data(), d_out, bytes, hipMemcpyDeviceToHost));
        F.realize_power({d_in}, {d_d[0], d_d[1], d_d[2]}, bases, {d_out});
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out_power.data(), d_out, bytes, hipMemcpyDeviceToHost));
        F.gradient({d_in}, {d_w[0], d_w[1], d_w[2]}, {d_g}, {d_gin}, {d_gw[0], d_gw[1], d_gw[2]});
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(gin.data(), d_gin, bytes, hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; k++) { gw[k].resize(N); HIP_OK(hipMemcpy(gw[k].data(), d_gw[k], bytes, hipMemcpyDeviceToHost)); }
        F.gradient_power({d_in}, {d_d[0], d_d[1], d_d[2]}, bases, {d_g}, {d_gin}, {d_gw[0], d_gw[1], d_gw[2]});
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(gin_power.data(), d_gin, bytes, hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; k++) { gd[k].resize(N); HIP_OK(hipMemcpy(gd[k].data(), d_gw[k], bytes, hipMemcpyDeviceToHost)); }
        // the smoothing filter on the volume, guiding itself, and the distances it runs on
        domain_transform_distances_volume({d_in}, false, W, H, D, scale, spacing_z, d_dist[0], d_dist[1], d_dist[2]);
        RecFilterSmooth S(W, H, D, 1, 0, false, false, 3, 40.0, 0.5, (double)spacing_z);
        S.realize({d_in}, {}, {d_out});
        HIP_OK(hipDeviceSynchronize());
        if (S.num_kernels() != 28) { std::printf("expected 28 launches, the smoothing plan has %d\n", S.num_kernels()); return 1; }
        smooth_bases = S.bases();
        HIP_OK(hipMemcpy(smooth.data(), d_out, bytes, hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; k++) { dist[k].resize(N); HIP_OK(hipMemcpy(dist[k].data(), d_dist[k], bytes, hipMemcpyDeviceToHost)); }
        // refusals arrive as exceptions with the library's text
        bool threw = false;
        try {
            RecFilterDim x3("x", W + 2);
            RecFilterVarying G(x3, y, z);
            G.add_scan(+z, 0);
            G.realize({d_in}, {d_w[0]}, {d_out});
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("multiple of 4") != std::string::npos; }
        if (!threw) { std::printf("a width of %d was not refused\n", W + 2); return 1; }
        threw = false;
        try { S.gradient({d_in}, {}, {d_g}, {d_gin}); } catch (const RecFilterError &) { threw = true; }
        if (!threw) { std::printf("the gradient of a volume filter was not refused\n"); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    bool ok = true;
    {
        std::vector<double> w64[3];
        for (int k = 0; k < 3; k++) w64[k].assign(w[k].begin(), w[k].end());
        const Result<double> want = loops<double>(in, w64, g);
        const Result<float> serial = loops<float>(in, w, g);
        ok = under_bar("volume", out, want.out, serial.out) && ok;
        ok = under_bar("volume, grad_in", gin, want.grad_in, serial.grad_in) && ok;
        for (int k = 0; k < 3; k++) {
            const std::string what = "volume, grad_w[" + std::to_string(k) + "]";
            ok = under_bar(what.c_str(), gw[k], want.grad_w[k], serial.grad_w[k]) && ok;
            ok = first_is_zero(what.c_str(), gw[k], k) && ok;
        }
    }
    {
        std::vector<double> p64[3];
        std::vector<float> p32[3];
        double c64[3];
        float c32[3];
        for (int k = 0; k < 3; k++) {
            const float l = (float)std::log2((double)bases[k]);
            c64[k] = std::log((double)bases[k]);
            c32[k] = (float)c64[k];
            p64[k].resize(N); p32[k].resize(N);
            for (int i = 0; i < N; i++) { p64[k][i] = std::exp2((double)d[k][i] * std::log2((double)bases[k])); p32[k][i] = std::exp2(d[k][i] * l); }
        }
        Result<double> want = loops<double>(in, p64, g);
        Result<float> serial = loops<float>(in, p32, g);
        for (int k = 0; k < 3; k++)
            for (int i = 0; i < N; i++) {      // dL/dd = (w ln a) dL/dw, exactly 0 where dL/dw is
                want.grad_w[k][i] = want.grad_w[k][i] == 0 ? 0 : (p64[k][i] * c64[k]) * want.grad_w[k][i];
                serial.grad_w[k][i] = serial.grad_w[k][i] == 0 ? 0 : (p32[k][i] * c32[k]) * serial.grad_w[k][i];
            }
        ok = under_bar("volume, power form", out_power, want.out, serial.out) && ok;
        ok = under_bar("volume, power form, grad_in", gin_power, want.grad_in, serial.grad_in) && ok;
        for (int k = 0; k < 3; k++) {
            const std::string what = "volume, power form, grad_d[" + std::to_string(k) + "]";
            ok = under_bar(what.c_str(), gd[k], want.grad_w[k], serial.grad_w[k]) && ok;
            ok = first_is_zero(what.c_str(), gd[k], k) && ok;
        }
    }
    {
        // the distances: per element within 4 * 2^-23 of the f64 formula (one channel: tests/test_gpu_var_power.py's bound)
        for (int k = 0; k < 3; k++) {
            double worst = 0;
            for (int i = 0; i < N; i++) {
                const int at = (i / STRIDE[k]) % EXTENT[k];
                const double first = k == 2 ? (double)spacing_z : 1.0;
                const double want = at == 0 ? first : first + (double)scale * std::fabs((double)in[i] - (double)in[i - STRIDE[k]]);
                worst = std::max(worst, std::fabs((double)dist[k][i] - want) / want);
            }
            std::printf("distances, axis %d: max relative error %.3e\n", k, worst);
            ok = worst <= 4.0 * std::ldexp(1.0, -23) && ok;
        }
        // K = 3 iterations of the six scans with the bases {a_k, a_k, a_k} on those distances
        std::vector<double> v64(in.begin(), in.end());
        std::vector<float> v32 = in;
        for (float a : smooth_bases) {
            const float l = (float)std::log2((double)a);
            std::vector<double> p64[3];
            std::vector<float> p32[3];
            for (int k = 0; k < 3; k++) {
                p64[k].resize(N); p32[k].resize(N);
                for (int i = 0; i < N; i++) { p64[k][i] = std::exp2((double)dist[k][i] * std::log2((double)a)); p32[k][i] = std::exp2(dist[k][i] * l); }
            }
            for (int q = 0; q < 6; q++) { v64 = scan(v64, p64[q / 2], q / 2, q % 2 == 0); v32 = scan(v32, p32[q / 2], q / 2, q % 2 == 0); }
        }
        ok = smooth_bases.size() == 3 && under_bar("smoothing filter on the volume", smooth, v64, v32) && ok;
    }
    for (float *p : {d_in, d_g, d_out, d_gin}) (void)hipFree(p);
    for (int k = 0; k < 3; k++)
        for (float *p : {d_w[k], d_d[k], d_gw[k], d_dist[k]}) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("varying-volume-frontend-ok\n");
    return 0;
}
