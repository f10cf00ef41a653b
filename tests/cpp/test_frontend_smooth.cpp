// RecFilterSmooth (include/recfilter.hpp) on a 70 x 260 byte image that guides itself, K = 3, against loops in this file.
// Truth: the f64 loops on the widened bytes, fed 2^(d * log2(a_k)) in f64 on the distance planes the library forms from the same
// bytes (domain_transform_distances) and the bases the filter reports.  Yardstick: the f32 loops fed exp2f(d * (float)log2(a_k)).
// The one-rounding rule, per sample:  |got - want| <= 0.5 + 255 * max(4 * err32, 1e-6),  err32 = the yardstick's max abs error
// over 255.  Compiled and run by tests/test_gpu_smooth.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int W = 260, H = 70, K = 3;
constexpr double SIGMA_S = 40.0, SIGMA_R = 0.5;

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
std::vector<T> reference(const std::vector<uint8_t> &in, const std::vector<float> &dx, const std::vector<float> &dy, const std::vector<float> &bases) {
    std::vector<T> v(in.begin(), in.end()), wx(in.size()), wy(in.size());
    for (float a : bases) {
        for (size_t i = 0; i < in.size(); i++) { wx[i] = power_weight((T)dx[i], a); wy[i] = power_weight((T)dy[i], a); }
        for (int y = 0; y < H; y++) scan_line<T>(&v[(size_t)y * W], &wx[(size_t)y * W], W, 1, true);
        for (int y = 0; y < H; y++) scan_line<T>(&v[(size_t)y * W], &wx[(size_t)y * W], W, 1, false);
        for (int x = 0; x < W; x++) scan_line<T>(&v[x], &wy[x], H, W, true);
        for (int x = 0; x < W; x++) scan_line<T>(&v[x], &wy[x], H, W, false);
    }
    return v;
}

uint32_t rng_state = 20113u;
uint32_t next_u32() {      // xorshift32
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

}  // namespace

int main() {
    const size_t n = (size_t)W * H;
    std::vector<uint8_t> in(n), got(n);
    for (size_t i = 0; i < n; i++) {      // a noisy step: an edge to keep, noise to smooth
        const int v = ((int)(i % W) < W / 2 ? 60 : 190) + (int)(next_u32() % 41u) - 20;
        in[i] = (uint8_t)std::min(std::max(v, 0), 255);
    }
    uint8_t *d_in = nullptr, *d_out = nullptr;
    float *d_dx = nullptr, *d_dy = nullptr;
    HIP_OK(hipMalloc((void **)&d_in, n)); HIP_OK(hipMalloc((void **)&d_out, n));
    HIP_OK(hipMalloc((void **)&d_dx, n * sizeof(float))); HIP_OK(hipMalloc((void **)&d_dy, n * sizeof(float)));
    HIP_OK(hipMemcpy(d_in, in.data(), n, hipMemcpyHostToDevice));
    std::vector<float> dx(n), dy(n), bases;
    try {
        RecFilterSmooth F(W, H, 1, 0, false, true, K, SIGMA_S, SIGMA_R);
        bases = F.bases();
        if ((int)bases.size() != K) { std::printf("expected %d bases, got %zu\n", K, bases.size()); return 1; }
        F.realize({d_in}, {}, {d_out});
        HIP_OK(hipDeviceSynchronize());
        if (F.num_kernels() != 1 + 6 * K) { std::printf("expected %d launches, the plan has %d\n", 1 + 6 * K, F.num_kernels()); return 1; }
        HIP_OK(hipMemcpy(got.data(), d_out, n, hipMemcpyDeviceToHost));
        // the distance planes the plan formed, formed again: a byte guide means that guide divided by 255
        domain_transform_distances({d_in}, true, W, H, (float)(SIGMA_S / SIGMA_R / 255.0), d_dx, d_dy);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(dx.data(), d_dx, n * sizeof(float), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(dy.data(), d_dy, n * sizeof(float), hipMemcpyDeviceToHost));
        // refusals arrive as exceptions with the library's text
        bool threw = false;
        try { F.realize({d_in}, {d_in}, {d_out}); }
        catch (const RecFilterError &) { threw = true; }
        if (!threw) { std::printf("a guide plane for a self-guided filter was not refused\n"); return 1; }
        threw = false;
        try { RecFilterSmooth G(W + 1, H, 1, 0, false, true, K, SIGMA_S, SIGMA_R); G.bases(); }
        catch (const RecFilterError &e) { threw = std::string(e.what()).find("multiple of 4") != std::string::npos; }
        if (!threw) { std::printf("a width of %d was not refused\n", W + 1); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    for (int k = 0; k < K; k++) {
        const double sigma_k = SIGMA_S * std::sqrt(3.0) * std::pow(2.0, K - 1 - k) / std::sqrt(std::pow(4.0, K) - 1.0);
        const float a_k = (float)std::exp(-std::sqrt(2.0) / sigma_k);
        if (std::fabs(bases[k] - a_k) > std::ldexp(1.0, -24)) { std::printf("base %d is %.9g, expected %.9g\n", k, bases[k], a_k); return 1; }
    }
    const std::vector<double> want = reference<double>(in, dx, dy, bases);
    const std::vector<float> serial = reference<float>(in, dx, dy, bases);
    double err32 = 0, worst = 0;
    for (size_t i = 0; i < n; i++) err32 = std::max(err32, std::fabs((double)serial[i] - want[i]));
    err32 /= 255.0;
    const double bound = 0.5 + 255.0 * std::max(4.0 * err32, 1e-6);
    size_t changed = 0;
    for (size_t i = 0; i < n; i++) {
        worst = std::max(worst, std::fabs((double)got[i] - want[i]));
        changed += got[i] != in[i];
    }
    std::printf("smooth, byte image: max |got - want| %.6f, bound %.6f (f32 serial loop over 255: %.3e), %zu of %zu samples changed\n",
                worst, bound, err32, changed, n);
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_dx); (void)hipFree(d_dy);
    if (!(worst <= bound)) { std::printf("FAILED\n"); return 1; }
    if (changed < n / 2) { std::printf("FAILED: the filter left the image\n"); return 1; }
    std::printf("smooth-frontend-ok\n");
    return 0;
}
