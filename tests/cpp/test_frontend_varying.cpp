// RecFilterVarying (include/recfilter.hpp): +x -x +y -y with per-sample feedback on a 70 x 260 image, against loops in this
// file.  The bar of tests/test_gpu_var_scans.py: max abs error over the input peak <= max(4 x the f32 serial loop's, 1e-6).
// Compiled and run by tests/test_gpu_var_scans.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int W = 260, H = 70;

// one scan along a line of n samples with stride `step`; wt(i) = masked weight of element i
template <typename T>
void scan_line(T *v, const float *w, int n, int step, bool causal) {
    auto wt = [&](int i) { return (i <= 0 || i >= n) ? T(0) : T(w[(size_t)i * step]); };
    if (causal) {
        T prev = 0;
        for (int i = 0; i < n; i++) { prev = (T(1) - wt(i)) * v[(size_t)i * step] + wt(i) * prev; v[(size_t)i * step] = prev; }
    } else {
        T next = 0;
        for (int i = n - 1; i >= 0; i--) { next = (T(1) - wt(i + 1)) * v[(size_t)i * step] + wt(i + 1) * next; v[(size_t)i * step] = next; }
    }
}

template <typename T>
std::vector<T> reference(const std::vector<float> &in, const std::vector<float> &wx, const std::vector<float> &wy) {
    std::vector<T> v(in.begin(), in.end());
    for (int y = 0; y < H; y++) scan_line<T>(&v[(size_t)y * W], &wx[(size_t)y * W], W, 1, true);
    for (int y = 0; y < H; y++) scan_line<T>(&v[(size_t)y * W], &wx[(size_t)y * W], W, 1, false);
    for (int x = 0; x < W; x++) scan_line<T>(&v[x], &wy[x], H, W, true);
    for (int x = 0; x < W; x++) scan_line<T>(&v[x], &wy[x], H, W, false);
    return v;
}

uint32_t rng_state = 20111u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

}  // namespace

int main() {
    const size_t n = (size_t)W * H, bytes = n * sizeof(float);
    std::vector<float> in(n), wx(n), wy(n);
    for (auto &v : in) v = 2.0f * uniform() - 1.0f;
    for (auto &v : wx) v = std::sqrt(std::sqrt(uniform()));
    for (auto &v : wy) v = std::sqrt(std::sqrt(uniform()));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int y = 0; y < H; y++) wx[(size_t)y * W] = nan;      // element 0 of the scanned dimension is never used
    for (int x = 0; x < W; x++) wy[x] = nan;
    float *d_in = nullptr, *d_wx = nullptr, *d_wy = nullptr, *d_out = nullptr;
    HIP_OK(hipMalloc((void **)&d_in, bytes)); HIP_OK(hipMalloc((void **)&d_wx, bytes));
    HIP_OK(hipMalloc((void **)&d_wy, bytes)); HIP_OK(hipMalloc((void **)&d_out, bytes));
    HIP_OK(hipMemcpy(d_in, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_wx, wx.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_wy, wy.data(), bytes, hipMemcpyHostToDevice));
    std::vector<float> got(n);
    try {
        RecFilterDim x("x", W), y("y", H);
        RecFilterVarying F(x, y);
        F.add_scan(+x, 0); F.add_scan(-x, 0); F.add_scan(+y, 1); F.add_scan(-y, 1);
        F.realize({d_in}, {d_wx, d_wy}, {d_out});
        HIP_OK(hipDeviceSynchronize());
        if (F.num_kernels() != 6) { std::printf("expected 6 launches, the plan has %d\n", F.num_kernels()); return 1; }
        HIP_OK(hipMemcpy(got.data(), d_out, bytes, hipMemcpyDeviceToHost));
        // a refusal arrives as an exception with the library's text
        bool threw = false;
        try {
            RecFilterDim x3("x", 262);
            RecFilterVarying G(x3, y);
            G.add_scan(+x3, 0);
            G.realize({d_in}, {d_wx}, {d_out});
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("multiple of 4") != std::string::npos; }
        if (!threw) { std::printf("a width of 262 was not refused\n"); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    const std::vector<double> want = reference<double>(in, wx, wy);
    const std::vector<float> serial = reference<float>(in, wx, wy);
    double peak = 0, err = 0, err32 = 0;
    for (size_t i = 0; i < n; i++) {
        peak = std::max(peak, (double)std::fabs(in[i]));
        if (std::isnan(got[i])) { std::printf("NaN at sample %zu\n", i); return 1; }
        err = std::max(err, std::fabs((double)got[i] - want[i]));
        err32 = std::max(err32, std::fabs((double)serial[i] - want[i]));
    }
    err /= peak; err32 /= peak;
    const double bar = std::max(4.0 * err32, 1e-6);
    std::printf("varying: err/peak %.3e, f32 serial loop %.3e, bar %.3e\n", err, err32, bar);
    (void)hipFree(d_in); (void)hipFree(d_wx); (void)hipFree(d_wy); (void)hipFree(d_out);
    if (!(err <= bar)) { std::printf("FAILED\n"); return 1; }
    std::printf("varying-frontend-ok\n");
    return 0;
}
