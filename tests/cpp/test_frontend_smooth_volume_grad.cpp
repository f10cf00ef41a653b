// RecFilterSmooth::differentiable() / gradient() on a volume and domain_transform_distances_volume_gradient (include/recfilter.hpp)
// on ONE volume of 24 x 22 x 70 samples (two z tiles, the second partial; five z segments of the distance kernels) with a separate
// f32 guide: the adjoint of the distances alone (stored and accumulated), and the whole filter's backward (K = 2, spacing_z = 2.5)
// with the distances held constant and through them, against loops in this file.  The bar of tests/test_gpu_smooth_volume_grad.py,
// for each gradient separately: max abs error over that gradient's f64 peak <= max(4 x the f32 serial loops', 1e-6).
// Compiled and run by tests/test_gpu_smooth_volume_grad.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int W = 24, H = 22, D = 70, N = W * H * D, K = 2;
constexpr int EXTENT[3] = {W, H, D}, STRIDE[3] = {1, W, W * H};
constexpr double SIGMA_S = 40.0, SIGMA_R = 0.5, SPACING_Z = 2.5;
const int AXES[6] = {0, 0, 1, 1, 2, 2};
const bool CAUSAL[6] = {true, false, true, false, true, false};

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

// w = exp2(d * l), l = log2 of the f32 base: in f32 what the library forms, (float)log2((double)a) and one f32 product
template <typename T>
std::vector<T> weights_of(const std::vector<T> &d, float base) {
    const T l = (T)std::log2((double)base);
    std::vector<T> w(d.size());
    for (size_t i = 0; i < d.size(); i++) w[i] = std::exp2(d[i] * l);
    return w;
}

// one iteration with the base a on the three distance volumes; saved: every scan's input and the result
template <typename T>
std::vector<T> iteration(const std::vector<T> &in, const std::vector<T> (&ds)[3], float a, std::vector<std::vector<T>> *saved = nullptr) {
    std::vector<std::vector<T>> s{in};
    for (int q = 0; q < 6; q++) s.push_back(scan<T>(s.back(), weights_of(ds[AXES[q]], a), AXES[q], CAUSAL[q]));
    std::vector<T> out = s.back();
    if (saved) *saved = std::move(s);
    return out;
}

// the adjoint of one iteration: g becomes dL/d(in); gd[k] receive (or, `add`, are added) the exponent gradients (w ln a) dL/dw
template <typename T>
void iteration_backward(const std::vector<T> &in, const std::vector<T> (&ds)[3], float a, std::vector<T> &g, std::vector<T> (&gd)[3], bool add) {
    std::vector<std::vector<T>> saved;
    iteration<T>(in, ds, a, &saved);
    std::vector<T> w[3] = {weights_of(ds[0], a), weights_of(ds[1], a), weights_of(ds[2], a)};
    std::vector<T> dw[3] = {std::vector<T>(N, T(0)), std::vector<T>(N, T(0)), std::vector<T>(N, T(0))};
    for (int q = 5; q >= 0; q--) scan_adjoint<T>(g, saved[q], saved[q + 1], w[AXES[q]], AXES[q], CAUSAL[q], dw[AXES[q]]);
    const T c = (T)std::log((double)a);
    for (int k = 0; k < 3; k++)
        for (int i = 0; i < N; i++) {
            const T e = dw[k][i] == T(0) ? T(0) : (w[k][i] * c) * dw[k][i];
            gd[k][i] = add ? gd[k][i] + e : e;
        }
}

template <typename T>
void distances(const std::vector<T> &g, T scale, T spacing, std::vector<T> (&ds)[3]) {
    for (int k = 0; k < 3; k++) ds[k].assign(N, T(0));
    for (int z = 0; z < D; z++)
        for (int r = 0; r < H; r++)
            for (int c = 0; c < W; c++) {
                const size_t i = ((size_t)z * H + r) * W + c;
                ds[0][i] = c == 0 ? T(1) : T(1) + scale * std::fabs(g[i] - g[i - 1]);
                ds[1][i] = r == 0 ? T(1) : T(1) + scale * std::fabs(g[i] - g[i - W]);
                ds[2][i] = z == 0 ? spacing : spacing + scale * std::fabs(g[i] - g[i - W * H]);
            }
}

template <typename T>
T sgn(T v) { return v > T(0) ? T(1) : (v < T(0) ? T(-1) : T(0)); }

template <typename T>
std::vector<T> distances_backward(const std::vector<T> &g, T scale, const std::vector<T> (&gd)[3]) {
    std::vector<T> out(N);
    const int S = W * H;
    for (int z = 0; z < D; z++)
        for (int r = 0; r < H; r++)
            for (int c = 0; c < W; c++) {
                const size_t i = ((size_t)z * H + r) * W + c;
                const T left = c > 0 ? sgn(g[i] - g[i - 1]) * gd[0][i] : T(0), right = c + 1 < W ? sgn(g[i + 1] - g[i]) * gd[0][i + 1] : T(0);
                const T up = r > 0 ? sgn(g[i] - g[i - W]) * gd[1][i] : T(0), down = r + 1 < H ? sgn(g[i + W] - g[i]) * gd[1][i + W] : T(0);
                const T before = z > 0 ? sgn(g[i] - g[i - S]) * gd[2][i] : T(0), after = z + 1 < D ? sgn(g[i + S] - g[i]) * gd[2][i + S] : T(0);
                out[i] = scale * (((((left - right) + up) - down) + before) - after);
            }
    return out;
}

template <typename T>
struct Gradients { std::vector<T> image, guide, distances_alone; };

template <typename T>
Gradients<T> reference(const std::vector<float> &image_f, const std::vector<float> &guide_f, const std::vector<float> &grad_out_f,
                       const std::vector<float> (&probe_f)[3], const std::vector<float> &bases, float scale) {
    const std::vector<T> image(image_f.begin(), image_f.end()), guide(guide_f.begin(), guide_f.end());
    std::vector<T> ds[3];
    distances<T>(guide, (T)scale, (T)SPACING_Z, ds);
    Gradients<T> out;
    std::vector<T> probe[3];
    for (int k = 0; k < 3; k++) probe[k].assign(probe_f[k].begin(), probe_f[k].end());
    out.distances_alone = distances_backward<T>(guide, (T)scale, probe);
    // the whole filter: iteration k's input kept, the adjoint with k = K-1 first
    std::vector<std::vector<T>> inputs{image};
    for (int k = 0; k + 1 < K; k++) inputs.push_back(iteration<T>(inputs.back(), ds, bases[k]));
    out.image.assign(grad_out_f.begin(), grad_out_f.end());
    std::vector<T> gd[3] = {std::vector<T>(N, T(0)), std::vector<T>(N, T(0)), std::vector<T>(N, T(0))};
    for (int k = K - 1; k >= 0; k--) iteration_backward<T>(inputs[k], ds, bases[k], out.image, gd, k < K - 1);
    out.guide = distances_backward<T>(guide, (T)scale, gd);
    return out;
}

uint32_t rng_state = 20127u;
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
    const size_t n = (size_t)N, bytes = n * sizeof(float);
    std::vector<float> image(n), guide(n), grad_out(n), old(n), probe[3];
    for (auto &v : image) v = uniform();
    for (int z = 0; z < D; z++)      // a ramp along the three axes under noise: no two neighbours equal
        for (int r = 0; r < H; r++)
            for (int c = 0; c < W; c++)
                guide[((size_t)z * H + r) * W + c] = 0.5f * uniform() + (float)c / (W - 1) + (float)r / (H - 1) + (float)z / (D - 1);
    for (int z = 0; z < D; z++)
        for (int r = 0; r < H; r++)
            for (int c = 0; c < W; c++) {
                const size_t i = ((size_t)z * H + r) * W + c;
                if ((c > 0 && guide[i] == guide[i - 1]) || (r > 0 && guide[i] == guide[i - W]) || (z > 0 && guide[i] == guide[i - W * H])) {
                    std::printf("ties in the guide\n");
                    return 1;
                }
            }
    for (auto &v : grad_out) v = 2.0f * uniform() - 1.0f;
    for (auto &v : old) v = 2.0f * uniform() - 1.0f;
    for (auto &p : probe) { p.resize(n); for (auto &v : p) v = 2.0f * uniform() - 1.0f; }
    const float scale = (float)(SIGMA_S / SIGMA_R);
    enum { IMAGE, GUIDE, GRAD_OUT, GDX, GDY, GDZ, GRAD_IMAGE, GRAD_GUIDE, HELD, ALONE, ADDED, N_BUFFERS };
    float *d[N_BUFFERS] = {};
    for (auto &p : d) HIP_OK(hipMalloc((void **)&p, bytes));
    HIP_OK(hipMemcpy(d[IMAGE], image.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d[GUIDE], guide.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d[GRAD_OUT], grad_out.data(), bytes, hipMemcpyHostToDevice));
    for (int k = 0; k < 3; k++) HIP_OK(hipMemcpy(d[GDX + k], probe[k].data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d[ADDED], old.data(), bytes, hipMemcpyHostToDevice));
    std::vector<float> got_image(n), got_guide(n), got_held(n), got_alone(n), got_added(n), bases;
    try {
        // a volume filter without differentiable(): no launches to report, and gradient() is refused with the library's text
        RecFilterSmooth plain(W, H, D, 1, 1, false, false, K, SIGMA_S, SIGMA_R, SPACING_Z);
        if (plain.gradient_num_kernels(false) != 0 || plain.gradient_num_kernels(true) != 0) { std::printf("a plain volume filter reports backward launches\n"); return 1; }
        bool threw = false;
        try {
            plain.gradient({}, {d[GUIDE]}, {d[GRAD_OUT]}, {d[HELD]});
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("RF_SMOOTH_VOLUME_BACKWARD") != std::string::npos; }
        if (!threw) { std::printf("gradient() on a volume filter without differentiable() was not refused\n"); return 1; }
        threw = false;
        try { plain.differentiable(); } catch (const RecFilterError &) { threw = true; }
        if (!threw) { std::printf("differentiable() after first use was not refused\n"); return 1; }

        RecFilterSmooth F(W, H, D, 1, 1, false, false, K, SIGMA_S, SIGMA_R, SPACING_Z);
        F.differentiable();
        bases = F.bases();
        if (F.num_kernels() != 1 + 9 * K || F.gradient_num_kernels(false) != 1 + 18 * K || F.gradient_num_kernels(true) != 51 * K - 7) {
            std::printf("expected %d, %d and %d launches, the plan has %d, %d and %d\n", 1 + 9 * K, 1 + 18 * K, 51 * K - 7, F.num_kernels(),
                        F.gradient_num_kernels(false), F.gradient_num_kernels(true));
            return 1;
        }
        F.gradient({}, {d[GUIDE]}, {d[GRAD_OUT]}, {d[HELD]});      // the distances held constant: no image volumes needed
        F.gradient({d[IMAGE]}, {d[GUIDE]}, {d[GRAD_OUT]}, {d[GRAD_IMAGE]}, {d[GRAD_GUIDE]}, true);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got_held.data(), d[HELD], bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_image.data(), d[GRAD_IMAGE], bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_guide.data(), d[GRAD_GUIDE], bytes, hipMemcpyDeviceToHost));
        threw = false;
        try {
            F.gradient({d[IMAGE]}, {d[GUIDE]}, {d[GRAD_OUT]}, {d[GRAD_IMAGE]}, {d[IMAGE]}, true);      // a gradient volume that is the image
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("overlaps image plane 0") != std::string::npos; }
        if (!threw) { std::printf("a gradient volume on top of the image was not refused\n"); return 1; }
        // the adjoint of the distances alone, stored and accumulated
        domain_transform_distances_volume_gradient({d[GUIDE]}, W, H, D, scale, d[GDX], d[GDY], d[GDZ], {d[ALONE]});
        domain_transform_distances_volume_gradient({d[GUIDE]}, W, H, D, scale, d[GDX], d[GDY], d[GDZ], {d[ADDED]}, true);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got_alone.data(), d[ALONE], bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_added.data(), d[ADDED], bytes, hipMemcpyDeviceToHost));
        threw = false;
        try {
            domain_transform_distances_volume_gradient({d[GUIDE]}, W, H, D, scale, d[GDX], d[GDY], d[GDZ], {d[GDZ]});
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("overlaps grad_dx, grad_dy or grad_dz") != std::string::npos; }
        if (!threw) { std::printf("a gradient volume on top of grad_dz was not refused\n"); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    for (size_t i = 0; i < n; i++)
        if (std::memcmp(&got_held[i], &got_image[i], sizeof(float)) != 0) { std::printf("the image gradient differs with edges at sample %zu\n", i); return 1; }
    const Gradients<double> want = reference<double>(image, guide, grad_out, probe, bases, scale);
    const Gradients<float> serial = reference<float>(image, guide, grad_out, probe, bases, scale);
    std::vector<double> want_added(n);
    std::vector<float> serial_added(n);
    for (size_t i = 0; i < n; i++) { want_added[i] = (double)old[i] + want.distances_alone[i]; serial_added[i] = old[i] + serial.distances_alone[i]; }
    bool ok = under_bar("volume smooth grad_image", got_image, want.image, serial.image);
    ok = under_bar("volume smooth grad_guide", got_guide, want.guide, serial.guide) && ok;
    ok = under_bar("volume distances gradient", got_alone, want.distances_alone, serial.distances_alone) && ok;
    ok = under_bar("volume distances gradient, accumulated", got_added, want_added, serial_added) && ok;
    for (auto &p : d) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("smooth-volume-grad-frontend-ok\n");
    return 0;
}
