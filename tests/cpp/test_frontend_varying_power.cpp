// The power form of RecFilterVarying (include/recfilter.hpp): domain_transform_distances of a one-plane guide, then
// realize_power with +x -x +y -y on a 70 x 260 image, against loops in this file.  The distances: the f64 formula, per element
// within (C + 3) * 2^-23 of it (C = 1).  The scans: truth is the f64 loop fed 2^(d * log2(base)) in f64 on the library's own
// distance planes, the yardstick the f32 loop fed exp2f(d * (float)log2(base)); the bar of tests/test_gpu_var_scans.py,
// max abs error over the input peak <= max(4 x the yardstick's, 1e-6).  Compiled and run by tests/test_gpu_var_power.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int W = 260, H = 70;

// one scan along a line of n samples with stride `step`; wt(i) = masked weight of element i
template <typename T>
void scan_line(T *v, const T *w, int n, int step, bool causal) {
    auto wt = [&](int i) { return (i <= 0 || i >= n) ? T(0) : w[(size_t)i * step]; };
    if (causal) {
        T prev = 0;
        for (int i = 0; i < n; i++) { prev = (T(1) - wt(i)) * v[(size_t)i * step] + wt(i) * prev; v[(size_t)i * step] = prev; }
    } else {
        T next = 0;
        for (int i = n - 1; i >= 0; i--) { next = (T(1) - wt(i + 1)) * v[(size_t)i * step] + wt(i + 1) * next; v[(size_t)i * step] = next; }
    }
}

double power_weight(double d, float base) { return std::exp2(d * std::log2((double)base)); }
float power_weight(float d, float base) { return exp2f(d * (float)std::log2((double)base)); }

template <typename T>
std::vector<T> reference(const std::vector<float> &in, const std::vector<float> &dx, const std::vector<float> &dy, float bx, float by) {
    std::vector<T> v(in.begin(), in.end()), wx(in.size()), wy(in.size());
    for (size_t i = 0; i < in.size(); i++) { wx[i] = power_weight((T)dx[i], bx); wy[i] = power_weight((T)dy[i], by); }
    for (int y = 0; y < H; y++) scan_line<T>(&v[(size_t)y * W], &wx[(size_t)y * W], W, 1, true);
    for (int y = 0; y < H; y++) scan_line<T>(&v[(size_t)y * W], &wx[(size_t)y * W], W, 1, false);
    for (int x = 0; x < W; x++) scan_line<T>(&v[x], &wy[x], H, W, true);
    for (int x = 0; x < W; x++) scan_line<T>(&v[x], &wy[x], H, W, false);
    return v;
}

uint32_t rng_state = 20112u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

}  // namespace

int main() {
    const size_t n = (size_t)W * H, bytes = n * sizeof(float);
    const float scale = 8.0f, bx = 0.9f, by = 0.75f;
    std::vector<float> in(n), guide(n);
    for (auto &v : in) v = 2.0f * uniform() - 1.0f;
    for (size_t i = 0; i < n; i++) guide[i] = ((int)(i % W) < W / 2 ? 0.2f : 0.8f) + 0.1f * uniform();      // a noisy step
    float *d_in = nullptr, *d_guide = nullptr, *d_dx = nullptr, *d_dy = nullptr, *d_out = nullptr;
    HIP_OK(hipMalloc((void **)&d_in, bytes)); HIP_OK(hipMalloc((void **)&d_guide, bytes));
    HIP_OK(hipMalloc((void **)&d_dx, bytes)); HIP_OK(hipMalloc((void **)&d_dy, bytes)); HIP_OK(hipMalloc((void **)&d_out, bytes));
    HIP_OK(hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_guide, guide.data(), bytes, hipMemcpyHostToDevice));
    std::vector<float> got(n), dx(n), dy(n);
    try {
        domain_transform_distances({d_guide}, false, W, H, scale, d_dx, d_dy);
        RecFilterDim x("x", W), y("y", H);
        RecFilterVarying F(x, y);
        F.add_scan(+x, 0); F.add_scan(-x, 0); F.add_scan(+y, 1); F.add_scan(-y, 1);
        F.realize_power({d_in}, {d_dx, d_dy}, {bx, by}, {d_out});
        HIP_OK(hipDeviceSynchronize());
        if (F.num_kernels() != 6) { std::printf("expected 6 launches, the plan has %d\n", F.num_kernels()); return 1; }
        HIP_OK(hipMemcpy(got.data(), d_out, bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(dx.data(), d_dx, bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(dy.data(), d_dy, bytes, hipMemcpyDeviceToHost));
        // refusals arrive as exceptions with the library's text
        bool threw = false;
        try { F.realize_power({d_in}, {d_dx, d_dy}, {bx, 1.0f}, {d_out}); }
        catch (const RecFilterError &e) { threw = std::string(e.what()).find("plane 1") != std::string::npos; }
        if (!threw) { std::printf("a base of 1 was not refused\n"); return 1; }
        threw = false;
        try { domain_transform_distances({d_guide}, false, W, H, scale, d_dx, d_dx); }
        catch (const RecFilterError &e) { threw = std::string(e.what()).find("overlaps") != std::string::npos; }
        if (!threw) { std::printf("dx == dy was not refused\n"); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    // the distances against the f64 formula
    double worst = 0;
    for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++) {
            const size_t i = (size_t)r * W + c;
            const double wx = c > 0 ? 1.0 + (double)scale * std::fabs((double)guide[i] - (double)guide[i - 1]) : 1.0;
            const double wy = r > 0 ? 1.0 + (double)scale * std::fabs((double)guide[i] - (double)guide[i - W]) : 1.0;
            worst = std::max(worst, std::max(std::fabs(dx[i] - wx) / wx, std::fabs(dy[i] - wy) / wy));
            if ((c == 0 && dx[i] != 1.0f) || (r == 0 && dy[i] != 1.0f)) { std::printf("element 0 of a distance line is not 1\n"); return 1; }
        }
    const double dist_bound = 4.0 * std::ldexp(1.0, -23);
    std::printf("distances: max relative error %.3e, bound %.3e\n", worst, dist_bound);
    if (!(worst <= dist_bound)) { std::printf("FAILED\n"); return 1; }
    const std::vector<double> want = reference<double>(in, dx, dy, bx, by);
    const std::vector<float> serial = reference<float>(in, dx, dy, bx, by);
    double peak = 0, err = 0, err32 = 0;
    for (size_t i = 0; i < n; i++) {
        peak = std::max(peak, (double)std::fabs(in[i]));
        if (std::isnan(got[i])) { std::printf("NaN at sample %zu\n", i); return 1; }
        err = std::max(err, std::fabs((double)got[i] - want[i]));
        err32 = std::max(err32, std::fabs((double)serial[i] - want[i]));
    }
    err /= peak; err32 /= peak;
    const double bar = std::max(4.0 * err32, 1e-6);
    std::printf("varying, power form: err/peak %.3e, f32 serial loop %.3e, bar %.3e\n", err, err32, bar);
    (void)hipFree(d_in); (void)hipFree(d_guide); (void)hipFree(d_dx); (void)hipFree(d_dy); (void)hipFree(d_out);
    if (!(err <= bar)) { std::printf("FAILED\n"); return 1; }
    std::printf("varying-power-frontend-ok\n");
    return 0;
}
