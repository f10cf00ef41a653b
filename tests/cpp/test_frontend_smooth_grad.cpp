// RecFilterSmooth::gradient and RecFilterVarying::gradient_power (include/recfilter.hpp) on a 70 x 260 image with a separate guide:
// the adjoint of +x -x +y -y in the power form with both exponent gradients, and the whole filter's backward (K = 2) with the
// distances held constant and through them, against loops in this file.  The bar of tests/test_gpu_smooth_grad.py, for each
// gradient separately: max abs error over that gradient's f64 peak <= max(4 x the f32 serial loops', 1e-6).
// Compiled and run by tests/test_gpu_smooth_grad.py.
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

constexpr int W = 260, H = 70, K = 2;
constexpr double SIGMA_S = 40.0, SIGMA_R = 0.5;

struct Line {      // a line of n samples with stride `step` in a W x H plane
    size_t first;
    int n, step;
    size_t at(int i) const { return first + (size_t)i * step; }
};

std::vector<Line> lines_of(int dim) {
    std::vector<Line> out;
    if (dim == 0) for (int y = 0; y < H; y++) out.push_back(Line{(size_t)y * W, W, 1});
    else for (int x = 0; x < W; x++) out.push_back(Line{(size_t)x, H, W});
    return out;
}

// masked weight of element i of a line
template <typename T>
T wt(const std::vector<T> &w, const Line &l, int i) { return (i <= 0 || i >= l.n) ? T(0) : w[l.at(i)]; }

template <typename T>
void scan_line(const std::vector<T> &x, std::vector<T> &y, const std::vector<T> &w, const Line &l, bool causal) {
    T acc = 0;
    if (causal) for (int i = 0; i < l.n; i++) { acc = (T(1) - wt(w, l, i)) * x[l.at(i)] + wt(w, l, i) * acc; y[l.at(i)] = acc; }
    else for (int i = l.n - 1; i >= 0; i--) { acc = (T(1) - wt(w, l, i + 1)) * x[l.at(i)] + wt(w, l, i + 1) * acc; y[l.at(i)] = acc; }
}

// g: dL/dy on entry, dL/dx on return; dw accumulates the weight gradient (element 0 of a line gets nothing)
template <typename T>
void adjoint_line(std::vector<T> &g, const std::vector<T> &x, const std::vector<T> &y, const std::vector<T> &w, std::vector<T> &dw,
                  const Line &l, bool causal) {
    std::vector<T> s(l.n);
    T acc = 0;
    if (causal) {
        for (int i = l.n - 1; i >= 0; i--) { acc = g[l.at(i)] + wt(w, l, i + 1) * acc; s[i] = acc; }
        for (int i = 0; i < l.n; i++) g[l.at(i)] = (T(1) - wt(w, l, i)) * s[i];
        for (int i = 1; i < l.n; i++) dw[l.at(i)] += s[i] * (y[l.at(i - 1)] - x[l.at(i)]);
    } else {
        for (int i = 0; i < l.n; i++) { acc = g[l.at(i)] + wt(w, l, i) * acc; s[i] = acc; }
        for (int i = 0; i < l.n; i++) g[l.at(i)] = (T(1) - wt(w, l, i + 1)) * s[i];
        for (int i = 1; i < l.n; i++) dw[l.at(i)] += s[i - 1] * (y[l.at(i)] - x[l.at(i - 1)]);
    }
}

const int DIMS[4] = {0, 0, 1, 1};
const bool CAUSAL[4] = {true, false, true, false};

// w = exp2(d * l), l = log2 of the f32 base: in f32 what the library forms, (float)log2((double)a) and one f32 product
template <typename T>
std::vector<T> weights_of(const std::vector<T> &d, float base) {
    const T l = (T)std::log2((double)base);
    std::vector<T> w(d.size());
    for (size_t i = 0; i < d.size(); i++) w[i] = std::exp2(d[i] * l);
    return w;
}

template <typename T>
std::vector<T> forward(const std::vector<T> &in, const std::vector<T> &wx, const std::vector<T> &wy, std::vector<std::vector<T>> *saved = nullptr) {
    std::vector<std::vector<T>> s(5, std::vector<T>(in.size()));
    s[0] = in;
    for (int q = 0; q < 4; q++)
        for (const Line &l : lines_of(DIMS[q])) scan_line<T>(s[q], s[q + 1], DIMS[q] == 0 ? wx : wy, l, CAUSAL[q]);
    std::vector<T> out = s[4];
    if (saved) *saved = std::move(s);
    return out;
}

// +x -x on d_x, +y -y on d_y in the power form, then the adjoints in reverse order: g becomes dL/d(in); gdx / gdy receive (or, `add`,
// are added) the exponent gradients (w ln a) dL/dw
template <typename T>
void power_backward(const std::vector<T> &in, const std::vector<T> &dx, const std::vector<T> &dy, float ax, float ay, std::vector<T> &g,
                    std::vector<T> &gdx, std::vector<T> &gdy, bool add) {
    const std::vector<T> wx = weights_of(dx, ax), wy = weights_of(dy, ay);
    std::vector<std::vector<T>> saved;
    forward(in, wx, wy, &saved);
    std::vector<T> dwx(in.size(), T(0)), dwy(in.size(), T(0));
    for (int q = 3; q >= 0; q--)
        for (const Line &l : lines_of(DIMS[q]))
            adjoint_line<T>(g, saved[q], saved[q + 1], DIMS[q] == 0 ? wx : wy, DIMS[q] == 0 ? dwx : dwy, l, CAUSAL[q]);
    const T cx = (T)std::log((double)ax), cy = (T)std::log((double)ay);
    for (size_t i = 0; i < in.size(); i++) {
        const T ex = dwx[i] == T(0) ? T(0) : (wx[i] * cx) * dwx[i], ey = dwy[i] == T(0) ? T(0) : (wy[i] * cy) * dwy[i];
        gdx[i] = add ? gdx[i] + ex : ex;
        gdy[i] = add ? gdy[i] + ey : ey;
    }
}

template <typename T>
void distances(const std::vector<T> &g, T scale, std::vector<T> &dx, std::vector<T> &dy) {
    for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++) {
            const size_t i = (size_t)r * W + c;
            dx[i] = c == 0 ? T(1) : T(1) + scale * std::fabs(g[i] - g[i - 1]);
            dy[i] = r == 0 ? T(1) : T(1) + scale * std::fabs(g[i] - g[i - W]);
        }
}

template <typename T>
T sgn(T v) { return v > T(0) ? T(1) : (v < T(0) ? T(-1) : T(0)); }

template <typename T>
std::vector<T> distances_backward(const std::vector<T> &g, T scale, const std::vector<T> &gdx, const std::vector<T> &gdy) {
    std::vector<T> out(g.size());
    for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++) {
            const size_t i = (size_t)r * W + c;
            const T left = c > 0 ? sgn(g[i] - g[i - 1]) * gdx[i] : T(0), right = c + 1 < W ? sgn(g[i + 1] - g[i]) * gdx[i + 1] : T(0);
            const T up = r > 0 ? sgn(g[i] - g[i - W]) * gdy[i] : T(0), down = r + 1 < H ? sgn(g[i + W] - g[i]) * gdy[i + W] : T(0);
            out[i] = scale * (((left - right) + up) - down);
        }
    return out;
}

template <typename T>
struct Gradients { std::vector<T> image, guide, power_in, power_dx, power_dy; };

template <typename T>
Gradients<T> reference(const std::vector<float> &image_f, const std::vector<float> &guide_f, const std::vector<float> &grad_out_f,
                       const std::vector<float> &bases, float scale) {
    const std::vector<T> image(image_f.begin(), image_f.end()), guide(guide_f.begin(), guide_f.end());
    const size_t n = image.size();
    std::vector<T> dx(n), dy(n);
    distances<T>(guide, (T)scale, dx, dy);
    Gradients<T> out;
    // one power-form plan: the bases of iteration 0 and 1 on the two planes
    out.power_in.assign(grad_out_f.begin(), grad_out_f.end());
    out.power_dx.assign(n, T(0));
    out.power_dy.assign(n, T(0));
    power_backward<T>(image, dx, dy, bases[0], bases[1], out.power_in, out.power_dx, out.power_dy, false);
    // the whole filter: iteration k's input kept, the adjoint with k = K-1 first
    std::vector<std::vector<T>> inputs{image};
    for (int k = 0; k + 1 < K; k++) inputs.push_back(forward(inputs.back(), weights_of(dx, bases[k]), weights_of(dy, bases[k])));
    out.image.assign(grad_out_f.begin(), grad_out_f.end());
    std::vector<T> gdx(n, T(0)), gdy(n, T(0));
    for (int k = K - 1; k >= 0; k--) power_backward<T>(inputs[k], dx, dy, bases[k], bases[k], out.image, gdx, gdy, k < K - 1);
    out.guide = distances_backward<T>(guide, (T)scale, gdx, gdy);
    return out;
}

uint32_t rng_state = 20119u;
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
    std::vector<float> image(n), guide(n), grad_out(n);
    for (auto &v : image) v = uniform();
    for (int r = 0; r < H; r++)      // a ramp both ways under noise: no two neighbours equal
        for (int c = 0; c < W; c++) guide[(size_t)r * W + c] = 0.5f * uniform() + (float)c / (W - 1) + (float)r / (H - 1);
    for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++) {
            const size_t i = (size_t)r * W + c;
            if ((c > 0 && guide[i] == guide[i - 1]) || (r > 0 && guide[i] == guide[i - W])) { std::printf("ties in the guide\n"); return 1; }
        }
    for (auto &v : grad_out) v = 2.0f * uniform() - 1.0f;
    const float scale = (float)(SIGMA_S / SIGMA_R);
    enum { IMAGE, GUIDE, GRAD_OUT, DX, DY, GRAD_IMAGE, GRAD_GUIDE, GRAD_DX, GRAD_DY, HELD, N_BUFFERS };
    float *d[N_BUFFERS] = {};
    for (auto &p : d) HIP_OK(hipMalloc((void **)&p, bytes));
    HIP_OK(hipMemcpy(d[IMAGE], image.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d[GUIDE], guide.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d[GRAD_OUT], grad_out.data(), bytes, hipMemcpyHostToDevice));
    std::vector<float> got_image(n), got_guide(n), got_held(n), got_power_in(n), got_dx(n), got_dy(n), bases;
    try {
        RecFilterSmooth F(W, H, 1, 1, false, false, K, SIGMA_S, SIGMA_R);
        bases = F.bases();
        if (F.gradient_num_kernels(false) != 1 + 12 * K || F.gradient_num_kernels(true) != 34 * K - 4) {
            std::printf("expected %d and %d launches, the plan has %d and %d\n", 1 + 12 * K, 34 * K - 4, F.gradient_num_kernels(false), F.gradient_num_kernels(true));
            return 1;
        }
        F.gradient({}, {d[GUIDE]}, {d[GRAD_OUT]}, {d[HELD]});      // the distances held constant: no image planes needed
        F.gradient({d[IMAGE]}, {d[GUIDE]}, {d[GRAD_OUT]}, {d[GRAD_IMAGE]}, {d[GRAD_GUIDE]}, true);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got_held.data(), d[HELD], bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_image.data(), d[GRAD_IMAGE], bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_guide.data(), d[GRAD_GUIDE], bytes, hipMemcpyDeviceToHost));
        // a refusal arrives as an exception with the library's text
        bool threw = false;
        try {
            F.gradient({d[IMAGE]}, {d[GUIDE]}, {d[GRAD_OUT]}, {d[GRAD_IMAGE]}, {d[IMAGE]}, true);      // a gradient plane that is the image
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("overlaps image plane 0") != std::string::npos; }
        if (!threw) { std::printf("a gradient plane on top of the image was not refused\n"); return 1; }
        // the power form by hand: the library's distance planes, one base per plane
        RecFilterDim x("x", W), y("y", H);
        RecFilterVarying V(x, y);
        V.add_scan(+x, 0); V.add_scan(-x, 0); V.add_scan(+y, 1); V.add_scan(-y, 1);
        domain_transform_distances({d[GUIDE]}, false, W, H, scale, d[DX], d[DY]);
        V.gradient_power({d[IMAGE]}, {d[DX], d[DY]}, {bases[0], bases[1]}, {d[GRAD_OUT]}, {d[GRAD_IMAGE]}, {d[GRAD_DX], d[GRAD_DY]});
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got_power_in.data(), d[GRAD_IMAGE], bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_dx.data(), d[GRAD_DX], bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_dy.data(), d[GRAD_DY], bytes, hipMemcpyDeviceToHost));
        threw = false;
        try {
            V.gradient_power({d[IMAGE]}, {d[DX], d[DY]}, {bases[0], 1.0f}, {d[GRAD_OUT]}, {d[GRAD_IMAGE]});
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("(0, 1)") != std::string::npos; }
        if (!threw) { std::printf("a base of 1 was not refused\n"); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    for (size_t i = 0; i < n; i++)
        if (std::memcmp(&got_held[i], &got_image[i], sizeof(float)) != 0) { std::printf("the image gradient differs with edges at sample %zu\n", i); return 1; }
    for (int r = 0; r < H; r++) if (got_dx[(size_t)r * W] != 0.0f) { std::printf("grad_dx: column 0 is not 0\n"); return 1; }
    for (int c = 0; c < W; c++) if (got_dy[c] != 0.0f) { std::printf("grad_dy: row 0 is not 0\n"); return 1; }
    const Gradients<double> want = reference<double>(image, guide, grad_out, bases, scale);
    const Gradients<float> serial = reference<float>(image, guide, grad_out, bases, scale);
    bool ok = under_bar("smooth grad_image", got_image, want.image, serial.image);
    ok = under_bar("smooth grad_guide", got_guide, want.guide, serial.guide) && ok;
    ok = under_bar("power grad_in", got_power_in, want.power_in, serial.power_in) && ok;
    ok = under_bar("power grad_dx", got_dx, want.power_dx, serial.power_dx) && ok;
    ok = under_bar("power grad_dy", got_dy, want.power_dy, serial.power_dy) && ok;
    for (auto &p : d) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("smooth-grad-frontend-ok\n");
    return 0;
}
