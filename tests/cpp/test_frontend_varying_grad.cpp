// RecFilterVarying::gradient (include/recfilter.hpp): the adjoint of +x -x +y -y with per-sample feedback on a 70 x 260 image --
// the image gradient and both weight gradients against loops in this file.  The bar of tests/test_gpu_var_grad.py, for each
// gradient separately: max abs error over that gradient's f64 peak <= max(4 x the f32 serial loops', 1e-6).
// Compiled and run by tests/test_gpu_var_grad.py.
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

constexpr int W = 260, H = 70;

struct Line {      // a line of n samples with stride `step` in a W x H plane
    size_t first;
    int n, step;
    size_t at(int i) const { return first + (size_t)i * step; }
};

// masked weight of element i of a line
template <typename T>
T wt(const std::vector<float> &w, const Line &l, int i) { return (i <= 0 || i >= l.n) ? T(0) : T(w[l.at(i)]); }

template <typename T>
void scan_line(const std::vector<T> &x, std::vector<T> &y, const std::vector<float> &w, const Line &l, bool causal) {
    T acc = 0;
    if (causal) for (int i = 0; i < l.n; i++) { acc = (T(1) - wt<T>(w, l, i)) * x[l.at(i)] + wt<T>(w, l, i) * acc; y[l.at(i)] = acc; }
    else for (int i = l.n - 1; i >= 0; i--) { acc = (T(1) - wt<T>(w, l, i + 1)) * x[l.at(i)] + wt<T>(w, l, i + 1) * acc; y[l.at(i)] = acc; }
}

// g: dL/dy on entry, dL/dx on return; dw accumulates the weight gradient (element 0 of a line gets nothing)
template <typename T>
void adjoint_line(std::vector<T> &g, const std::vector<T> &x, const std::vector<T> &y, const std::vector<float> &w, std::vector<T> &dw,
                  const Line &l, bool causal) {
    std::vector<T> s(l.n);
    T acc = 0;
    if (causal) {
        for (int i = l.n - 1; i >= 0; i--) { acc = g[l.at(i)] + wt<T>(w, l, i + 1) * acc; s[i] = acc; }
        for (int i = 0; i < l.n; i++) g[l.at(i)] = (T(1) - wt<T>(w, l, i)) * s[i];
        for (int i = 1; i < l.n; i++) dw[l.at(i)] += s[i] * (y[l.at(i - 1)] - x[l.at(i)]);
    } else {
        for (int i = 0; i < l.n; i++) { acc = g[l.at(i)] + wt<T>(w, l, i) * acc; s[i] = acc; }
        for (int i = 0; i < l.n; i++) g[l.at(i)] = (T(1) - wt<T>(w, l, i + 1)) * s[i];
        for (int i = 1; i < l.n; i++) dw[l.at(i)] += s[i - 1] * (y[l.at(i)] - x[l.at(i - 1)]);
    }
}

std::vector<Line> lines_of(int dim) {
    std::vector<Line> out;
    if (dim == 0) for (int y = 0; y < H; y++) out.push_back(Line{(size_t)y * W, W, 1});
    else for (int x = 0; x < W; x++) out.push_back(Line{(size_t)x, H, W});
    return out;
}

template <typename T>
struct Gradients { std::vector<T> in, wx, wy; };

// +x -x on wx, +y -y on wy, then the adjoints in reverse order
template <typename T>
Gradients<T> reference(const std::vector<float> &in, const std::vector<float> &wx, const std::vector<float> &wy, const std::vector<float> &grad_out) {
    const int dims[4] = {0, 0, 1, 1};
    const bool causal[4] = {true, false, true, false};
    std::vector<std::vector<T>> saved(5, std::vector<T>(in.size()));
    saved[0].assign(in.begin(), in.end());
    for (int q = 0; q < 4; q++)
        for (const Line &l : lines_of(dims[q])) scan_line<T>(saved[q], saved[q + 1], dims[q] == 0 ? wx : wy, l, causal[q]);
    Gradients<T> g;
    g.in.assign(grad_out.begin(), grad_out.end());
    g.wx.assign(in.size(), T(0));
    g.wy.assign(in.size(), T(0));
    for (int q = 3; q >= 0; q--)
        for (const Line &l : lines_of(dims[q]))
            adjoint_line<T>(g.in, saved[q], saved[q + 1], dims[q] == 0 ? wx : wy, dims[q] == 0 ? g.wx : g.wy, l, causal[q]);
    return g;
}

uint32_t rng_state = 20118u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

bool under_bar(const char *what, const std::vector<float> &got, const std::vector<double> &want, const std::vector<float> &serial) {
    double peak = 0, err = 0, err32 = 0;
    for (size_t i = 0; i < got.size(); i++) {
        if (std::isnan(got[i])) { std::printf("%s: NaN at sample %zu\n", what, i); return false; }
        peak = std::max(peak, std::fabs(want[i]));
        err = std::max(err, std::fabs((double)got[i] - want[i]));
        err32 = std::max(err32, std::fabs((double)serial[i] - want[i]));
    }
    err /= peak; err32 /= peak;
    const double bar = std::max(4.0 * err32, 1e-6);
    std::printf("%s: err/peak %.3e, f32 serial loops %.3e, bar %.3e\n", what, err, err32, bar);
    return err <= bar;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

}  // namespace

int main() {
    const size_t n = (size_t)W * H, bytes = n * sizeof(float);
    std::vector<float> in(n), wx(n), wy(n), grad_out(n);
    for (auto &v : in) v = 2.0f * uniform() - 1.0f;
    for (auto &v : wx) v = std::sqrt(std::sqrt(uniform()));
    for (auto &v : wy) v = std::sqrt(std::sqrt(uniform()));
    for (auto &v : grad_out) v = 2.0f * uniform() - 1.0f;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int y = 0; y < H; y++) wx[(size_t)y * W] = nan;      // element 0 of the scanned dimension is never used
    for (int x = 0; x < W; x++) wy[x] = nan;
    float *d[7] = {};      // in, wx, wy, grad_out, grad_in, grad_wx, grad_wy
    for (auto &p : d) HIP_OK(hipMalloc((void **)&p, bytes));
    HIP_OK(hipMemcpy(d[0], in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d[1], wx.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d[2], wy.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d[3], grad_out.data(), bytes, hipMemcpyHostToDevice));
    std::vector<float> got_in(n), got_wx(n), got_wy(n), image_only(n);
    try {
        RecFilterDim x("x", W), y("y", H);
        RecFilterVarying F(x, y);
        F.add_scan(+x, 0); F.add_scan(-x, 0); F.add_scan(+y, 1); F.add_scan(-y, 1);
        F.gradient({}, {d[1], d[2]}, {d[3]}, {d[4]});      // the image gradient alone: no input planes needed
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(image_only.data(), d[4], bytes, hipMemcpyDeviceToHost));
        F.gradient({d[0]}, {d[1], d[2]}, {d[3]}, {d[4]}, {d[5], d[6]});
        HIP_OK(hipDeviceSynchronize());
        if (F.gradient_num_kernels(false) != 12 || F.gradient_num_kernels(true) != 28) {
            std::printf("expected 12 and 28 launches, the plan has %d and %d\n", F.gradient_num_kernels(false), F.gradient_num_kernels(true));
            return 1;
        }
        HIP_OK(hipMemcpy(got_in.data(), d[4], bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_wx.data(), d[5], bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_wy.data(), d[6], bytes, hipMemcpyDeviceToHost));
        // a refusal arrives as an exception with the library's text
        bool threw = false;
        try {
            F.gradient({d[0]}, {d[1], d[2]}, {d[3]}, {d[4]}, {d[1], nullptr});      // a gradient plane that is a weight plane
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("overlaps weight plane 0") != std::string::npos; }
        if (!threw) { std::printf("a gradient plane on top of a weight plane was not refused\n"); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    for (size_t i = 0; i < n; i++)
        if (std::memcmp(&image_only[i], &got_in[i], sizeof(float)) != 0) { std::printf("the image gradient differs with weight gradients at sample %zu\n", i); return 1; }
    for (int y = 0; y < H; y++) if (got_wx[(size_t)y * W] != 0.0f) { std::printf("grad_wx: column 0 is not 0\n"); return 1; }
    for (int x = 0; x < W; x++) if (got_wy[x] != 0.0f) { std::printf("grad_wy: row 0 is not 0\n"); return 1; }
    const Gradients<double> want = reference<double>(in, wx, wy, grad_out);
    const Gradients<float> serial = reference<float>(in, wx, wy, grad_out);
    bool ok = under_bar("grad_in", got_in, want.in, serial.in);
    ok = under_bar("grad_wx", got_wx, want.wx, serial.wx) && ok;
    ok = under_bar("grad_wy", got_wy, want.wy, serial.wy) && ok;
    for (auto &p : d) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("varying-grad-frontend-ok\n");
    return 0;
}
