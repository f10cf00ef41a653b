// RecFilterVarying::gradient_power_bases (include/recfilter.hpp on rf_var_plan_backward_power_bases): +x -x +y -y in the power form on
// 70 x 132, two planes, against f64 loops in this file.  Held to 1e-6 of sum |terms|, the floor of the bar of
// tests/test_gpu_sigma_grad.py; grad_in and the exponent gradients bit for bit those of gradient_power.  Then RecFilterSmooth:
// set_sigmas against a fresh filter and gradient_sigmas against gradient(), bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "recfilter.hpp"

#define HIP_OK(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) { std::printf("%s: %s\n", #call, hipGetErrorString(e_)); return 1; } \
    } while (0)

namespace {

constexpr int H = 70, W = 132, P = 2, N = H * W;

struct Scan { int dim; bool causal; int k; };
const Scan kScans[4] = {{0, true, 0}, {0, false, 0}, {1, true, 1}, {1, false, 1}};

// element i of line l along dim
inline int at(int dim, int l, int i) { return dim == 0 ? l * W + i : i * W + l; }
inline int lines(int dim) { return dim == 0 ? H : W; }
inline int length(int dim) { return dim == 0 ? W : H; }

// w~[0] = w~[n] = 0
inline double wt(const std::vector<double> &w, int dim, int l, int i) { return i <= 0 || i >= length(dim) ? 0.0 : w[at(dim, l, i)]; }

void scan(const std::vector<double> &x, const std::vector<double> &w, const Scan &s, std::vector<double> &y) {
    const int n = length(s.dim);
    for (int l = 0; l < lines(s.dim); l++) {
        double acc = 0.0;
        for (int q = 0; q < n; q++) {
            const int i = s.causal ? q : n - 1 - q;
            const double wi = wt(w, s.dim, l, s.causal ? i : i + 1);
            acc = (1.0 - wi) * x[at(s.dim, l, i)] + wi * acc;
            y[at(s.dim, l, i)] = acc;
        }
    }
}

// g -> dL/dx in place; dw += this plane's dL/dw
void adjoint(std::vector<double> &g, const std::vector<double> &x, const std::vector<double> &y, const std::vector<double> &w, const Scan &s,
             std::vector<double> &dw) {
    const int n = length(s.dim);
    std::vector<double> state(n);
    for (int l = 0; l < lines(s.dim); l++) {
        double acc = 0.0;
        for (int q = 0; q < n; q++) {
            const int i = s.causal ? n - 1 - q : q;
            acc = g[at(s.dim, l, i)] + wt(w, s.dim, l, s.causal ? i + 1 : i) * acc;
            state[i] = acc;
        }
        for (int i = 0; i < n; i++) g[at(s.dim, l, i)] = (1.0 - wt(w, s.dim, l, s.causal ? i : i + 1)) * state[i];
        for (int i = 1; i < n; i++)
            dw[at(s.dim, l, i)] += s.causal ? state[i] * (y[at(s.dim, l, i - 1)] - x[at(s.dim, l, i)])
                                            : state[i - 1] * (y[at(s.dim, l, i)] - x[at(s.dim, l, i - 1)]);
    }
}

}  // namespace

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { std::printf("no device\n"); return 1; }
    std::mt19937 rng(2811);
    std::uniform_real_distribution<float> signed_unit(-1.0f, 1.0f), spread(1.0f, 4.0f);
    std::vector<std::vector<float>> in(P, std::vector<float>(N)), gout(P, std::vector<float>(N)), d(2, std::vector<float>(N));
    for (auto &p : in) for (float &v : p) v = signed_unit(rng);
    for (auto &p : gout) for (float &v : p) v = signed_unit(rng);
    for (auto &p : d) for (float &v : p) v = spread(rng);
    d[0][5 * W + 7] = INFINITY;                        // w = 0: exactly no contribution
    d[1][9 * W + 3] = 0.0f;                            // w = 1
    for (int r = 0; r < H; r++) d[0][r * W] = NAN;     // element 0 along the scanned dimension is never read
    for (int c = 0; c < W; c++) d[1][c] = NAN;
    const std::vector<float> bases = {0.9f, 0.8f};

    // ---- f64 loops ----
    std::vector<std::vector<double>> w(2, std::vector<double>(N));
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < N; i++) w[k][i] = std::exp2((double)d[k][i] * std::log2((double)bases[k]));
    std::vector<std::vector<std::vector<double>>> saved(5, std::vector<std::vector<double>>(P, std::vector<double>(N)));
    for (int pl = 0; pl < P; pl++) saved[0][pl].assign(in[pl].begin(), in[pl].end());
    for (int q = 0; q < 4; q++)
        for (int pl = 0; pl < P; pl++) scan(saved[q][pl], w[kScans[q].k], kScans[q], saved[q + 1][pl]);
    std::vector<std::vector<double>> g(P, std::vector<double>(N));
    for (int pl = 0; pl < P; pl++) g[pl].assign(gout[pl].begin(), gout[pl].end());
    double want[2] = {0.0, 0.0}, norm[2] = {0.0, 0.0};
    for (int q = 3; q >= 0; q--) {
        const Scan &s = kScans[q];
        std::vector<double> dw(N, 0.0);
        for (int pl = 0; pl < P; pl++) adjoint(g[pl], saved[q][pl], saved[q + 1][pl], w[s.k], s, dw);
        for (int l = 0; l < lines(s.dim); l++)
            for (int i = 1; i < length(s.dim); i++) {
                const int e = at(s.dim, l, i);
                const double t = w[s.k][e] == 0.0 ? 0.0 : (double)d[s.k][e] * w[s.k][e] * dw[e];
                want[s.k] += t;
                norm[s.k] += std::fabs(t);
            }
    }
    for (int k = 0; k < 2; k++) { want[k] /= (double)bases[k]; norm[k] /= (double)bases[k]; }

    // ---- the device ----
    auto upload = [](const std::vector<float> &v, float **p) {
        if (hipMalloc((void **)p, v.size() * sizeof(float)) != hipSuccess) return false;
        return hipMemcpy(*p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    };
    float *d_in[P], *d_gout[P], *d_d[2], *d_gin[2][P], *d_gd[2][2];
    for (int pl = 0; pl < P; pl++)
        if (!upload(in[pl], &d_in[pl]) || !upload(gout[pl], &d_gout[pl])) return 1;
    for (int k = 0; k < 2; k++)
        if (!upload(d[k], &d_d[k])) return 1;
    for (int v = 0; v < 2; v++) {
        for (int pl = 0; pl < P; pl++) HIP_OK(hipMalloc((void **)&d_gin[v][pl], N * sizeof(float)));
        for (int k = 0; k < 2; k++) HIP_OK(hipMalloc((void **)&d_gd[v][k], N * sizeof(float)));
    }
    double *d_gb = nullptr;
    HIP_OK(hipMalloc((void **)&d_gb, 2 * sizeof(double)));
    HIP_OK(hipMemset(d_gb, 0xff, 2 * sizeof(double)));

    double got[2] = {0.0, 0.0}, alone[2] = {0.0, 0.0};
    std::vector<float> a(N), b(N);
    try {
        RecFilterDim x("x", W), y("y", H);
        RecFilterVarying F(x, y);
        F.add_scan(+x, 0);
        F.add_scan(-x, 0);
        F.add_scan(+y, 1);
        F.add_scan(-y, 1);
        const std::vector<const void *> ins = {d_in[0], d_in[1]}, exps = {d_d[0], d_d[1]}, gouts = {d_gout[0], d_gout[1]};
        F.gradient_power(ins, exps, bases, gouts, {d_gin[0][0], d_gin[0][1]}, {d_gd[0][0], d_gd[0][1]});
        F.gradient_power_bases(ins, exps, bases, gouts, {d_gin[1][0], d_gin[1][1]}, {d_gd[1][0], d_gd[1][1]}, d_gb);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got, d_gb, sizeof(got), hipMemcpyDeviceToHost));
        if (F.gradient_bases_num_kernels() != 29) { std::printf("gradient_bases_num_kernels = %d, expected 29\n", F.gradient_bases_num_kernels()); return 1; }
        // without exponent gradients: the same scalars, bit for bit
        F.gradient_power_bases(ins, exps, bases, gouts, {d_gin[1][0], d_gin[1][1]}, {}, d_gb);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(alone, d_gb, sizeof(alone), hipMemcpyDeviceToHost));
        // a misaligned result buffer is refused
        bool refused = false;
        try {
            F.gradient_power_bases(ins, exps, bases, gouts, {d_gin[1][0], d_gin[1][1]}, {}, (double *)((char *)d_gb + 4));
        } catch (const RecFilterError &e) {
            refused = std::strstr(e.what(), "8-byte") != nullptr;
        }
        if (!refused) { std::printf("a misaligned grad_bases was not refused\n"); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    for (int pl = 0; pl < P + 2; pl++) {
        const float *p0 = pl < P ? d_gin[0][pl] : d_gd[0][pl - P], *p1 = pl < P ? d_gin[1][pl] : d_gd[1][pl - P];
        HIP_OK(hipMemcpy(a.data(), p0, N * sizeof(float), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(b.data(), p1, N * sizeof(float), hipMemcpyDeviceToHost));
        if (std::memcmp(a.data(), b.data(), N * sizeof(float)) != 0) { std::printf("plane %d differs from gradient_power's\n", pl); return 1; }
    }
    bool ok = true;
    for (int k = 0; k < 2; k++) {
        const double fig = std::fabs(got[k] - want[k]) / norm[k];
        std::printf("sigma-grad-frontend base %d: got %.9e want %.9e figure %.3e (bar 1e-6)\n", k, got[k], want[k], fig);
        ok = ok && std::isfinite(got[k]) && fig <= 1e-6 && std::memcmp(&got[k], &alone[k], sizeof(double)) == 0;
    }
    // ---- RecFilterSmooth: set_sigmas gives a fresh filter's bases and gradients, gradient_sigmas gradient()'s planes, bit for bit ----
    try {
        RecFilterSmooth S(W, H, P, 0, false, false, 2, 9.5, 0.3), T(W, H, P, 0, false, false, 2, 3.0, 0.8);
        T.set_sigmas(9.5, 0.3);
        const std::vector<float> bs = S.bases(), bt = T.bases();
        if (bs.size() != 2 || std::memcmp(bs.data(), bt.data(), 2 * sizeof(float)) != 0) { std::printf("set_sigmas: other bases than a fresh filter\n"); return 1; }
        bool refused = false;
        try { T.set_sigmas(0.0, 0.3); } catch (const RecFilterError &) { refused = true; }
        const std::vector<float> kept = T.bases();
        if (!refused || std::memcmp(kept.data(), bt.data(), 2 * sizeof(float)) != 0) { std::printf("a refused set_sigmas changed the filter\n"); return 1; }
        double *d_gp = nullptr;
        HIP_OK(hipMalloc((void **)&d_gp, 2 * 5 * sizeof(double)));
        const std::vector<const void *> ins = {d_in[0], d_in[1]}, gouts = {d_gout[0], d_gout[1]};
        S.gradient(ins, {}, gouts, {d_gin[0][0], d_gin[0][1]}, {}, true);
        S.gradient_sigmas(ins, {}, gouts, {d_gin[1][0], d_gin[1][1]}, {}, true, d_gp);
        T.gradient_sigmas(ins, {}, gouts, {d_gd[1][0], d_gd[1][1]}, {}, true, d_gp + 5);
        HIP_OK(hipDeviceSynchronize());
        if (S.gradient_sigmas_num_kernels(true) != S.gradient_num_kernels(true) + 2) { std::printf("gradient_sigmas_num_kernels\n"); return 1; }
        double gp[10];
        HIP_OK(hipMemcpy(gp, d_gp, sizeof(gp), hipMemcpyDeviceToHost));
        for (int j = 0; j < 5; j++) {
            std::printf("sigma-grad-frontend smooth param %d: %.9e\n", j, gp[j]);
            if (!std::isfinite(gp[j]) || std::memcmp(&gp[j], &gp[5 + j], sizeof(double)) != 0 || (j != 2 && gp[j] == 0.0)) { std::printf("smooth params differ\n"); return 1; }
        }
        for (int pl = 0; pl < P; pl++)
            for (int v = 0; v < 2; v++) {
                HIP_OK(hipMemcpy(a.data(), d_gin[0][pl], N * sizeof(float), hipMemcpyDeviceToHost));
                HIP_OK(hipMemcpy(b.data(), v == 0 ? d_gin[1][pl] : d_gd[1][pl], N * sizeof(float), hipMemcpyDeviceToHost));
                if (std::memcmp(a.data(), b.data(), N * sizeof(float)) != 0) { std::printf("gradient_sigmas: plane %d differs from gradient()'s\n", pl); return 1; }
            }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    if (!ok) { std::printf("sigma-grad-frontend FAILED\n"); return 1; }
    std::printf("sigma-grad-frontend-ok\n");
    return 0;
}
