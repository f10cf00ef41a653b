// test_frontend_u8.cpp -- byte images end to end through include/recfilter.hpp with a plain host compiler.
//
// RecFilterImage(const uint8_t *) / 255 binds a plane of unsigned bytes that the passes widen on load; the consumer
// RecFilterPointwise{255, 0, 0, to_bytes} is the reference's cast<uint8_t>(255 * blur) computed at the filter
// (rf_pointwise_desc.in_dtype = RF_IO_U8): realize() returns a plane of bytes, each min(max(rint(v), 0), 255) of the f32 value
// v, converted once at the final store.  A 512 x 512 Gaussian of order 2 (+x -x +y -y, clamped) is compared with the raster
// loops tests/cpp/test_frontend_half.cpp uses, in double, under the one-rounding rule of tests/u8_cases.py:
//     |got - clip(want, 0, 255)| <= 0.5 + 1e-4 * |want|
// Compiled and run by tests/test_gpu_u8_output.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "recfilter.hpp"

// one clamped scan along `dim` over a w x h image, in place: samples before the border read as the border sample's input
// for the feed-forward history and as the scan's first output afterwards (the reference's clamped prologue)
static void loop_scan_clamped(std::vector<double> &img, int w, int h, int dim, bool causal, const std::vector<float> &W) {
    const int n = dim == 0 ? w : h, lines = dim == 0 ? h : w;
    const long stride = dim == 0 ? 1 : w, line_stride = dim == 0 ? w : 1;
    const int k = (int)W.size() - 1;
    for (int line = 0; line < lines; line++) {
        const long base = line * line_stride;
        std::vector<double> y((size_t)n);
        for (int r = 0; r < n; r++) {
            const int i = causal ? r : n - 1 - r;
            const double x = img[base + i * stride];
            double acc = (double)W[0] * x;
            for (int j = 0; j < k; j++) {
                const int rr = r - 1 - j;
                double prev;
                if (rr >= 0) prev = y[(size_t)rr];
                else prev = r == 0 ? x : y[0];           // before the border: the border sample, then the first output
                acc += (double)W[j + 1] * prev;
            }
            y[(size_t)r] = acc;
        }
        for (int r = 0; r < n; r++) img[base + (causal ? r : n - 1 - r) * stride] = y[(size_t)r];
    }
}

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { std::fprintf(stderr, "no GPU\n"); return 2; }
    const int width = 512, height = 512;
    std::vector<uint8_t> image((size_t)width * height);
    std::vector<double> ref(image.size());
    const float scale = 1.0f / 255.0f;
    unsigned long long s = 0x9E3779B97F4A7C15ull * 21;
    for (size_t i = 0; i < image.size(); i++) {      // SplitMix64 -> a byte
        s += 0x9E3779B97F4A7C15ull;
        unsigned long long z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        image[i] = (uint8_t)(z >> 56);
        ref[i] = (double)(scale * (float)image[i]);         // x' as the passes form it, in f32
    }
    uint8_t *d = nullptr;
    if (hipMalloc(&d, image.size()) != hipSuccess) return 2;
    if (hipMemcpy(d, image.data(), image.size(), hipMemcpyHostToDevice) != hipSuccess) return 2;

    const std::vector<float> W = gaussian_weights(5.0f, 2);
    RecFilterDim x("x", width), y("y", height);
    RecFilter filter;
    filter.set_clamped_image_border();
    filter(x, y) = RecFilterImage(d) / 255.0f;
    filter.add_filter(+x, W);
    filter.add_filter(-x, W);
    filter.add_filter(+y, W);
    filter.add_filter(-y, W);
    filter.split(x, 32, y, 32);
    RecFilterPointwise to_bytes;
    to_bytes.w_filtered = 255.0f;
    to_bytes.to_bytes = true;
    filter.compute_at(to_bytes);
    RecFilterRealization r = filter.realize();
    if (!r.bytes || r.bytes_per_plane != image.size()) { std::printf("unexpected plane: bytes %d, %zu bytes per plane\n", (int)r.bytes, r.bytes_per_plane); return 1; }
    std::vector<uint8_t> out = r.to_host<uint8_t>();
    (void)hipFree(d);
    if (out.size() != image.size()) { std::printf("unexpected result size %zu\n", out.size()); return 1; }

    loop_scan_clamped(ref, width, height, 0, true, W);
    loop_scan_clamped(ref, width, height, 0, false, W);
    loop_scan_clamped(ref, width, height, 1, true, W);
    loop_scan_clamped(ref, width, height, 1, false, W);
    double worst = -1.0;
    int lo = 255, hi = 0;
    for (size_t i = 0; i < ref.size(); i++) {
        const double want = 255.0 * ref[i], clipped = std::fmin(std::fmax(want, 0.0), 255.0);
        worst = std::fmax(worst, std::fabs((double)out[i] - clipped) - (0.5 + 1e-4 * std::fabs(want)));
        lo = out[i] < lo ? out[i] : lo; hi = out[i] > hi ? out[i] : hi;
    }
    std::printf("u8 frontend: bytes %d..%d, worst |got - clip(want)| - (0.5 + 1e-4 |want|) = %.4e\n", lo, hi, worst);
    if (!(worst <= 0.0) || hi - lo < 16) { std::printf("FAILED\n"); return 1; }
    std::printf("u8-frontend-ok\n");
    return 0;
}
