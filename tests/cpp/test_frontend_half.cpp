// test_frontend_half.cpp -- 16-bit float pixels through include/recfilter.hpp with a plain host compiler.
//
// RecFilterImage(const rf_half *) binds planes of IEEE binary16 bit patterns (RF_F16: storage in 16 bits, arithmetic in f32,
// one rounding at the final store).  A 512 x 512 Gaussian of order 2 (+x -x +y -y, clamped) is realized on the GPU, widened
// on the host and compared with raster loops over the widened input -- the loops tests/cpp/test_frontend.cpp uses for its
// f32 cases, here with the clamped border -- at 1e-4 + 2^-11: the suite's f32 bar plus half an ulp of the final rounding.
// Compiled and run by tests/test_gpu_half_pixels.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "recfilter.hpp"

// binary16 <-> f32 on the host, round to nearest even (normal and subnormal results; the test's values are in (0, 2))
static float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 31u, man = h & 1023u;
    float v;
    if (exp == 0) v = std::ldexp((float)man, -24);
    else if (exp == 31) v = man ? NAN : INFINITY;
    else v = std::ldexp((float)(man | 1024u), (int)exp - 25);
    return sign ? -v : v;
}

static uint16_t float_to_half(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);                     // overflow (the test has no NaN)
    if (x < 0x38800000u) {                                                       // subnormal half
        const float scaled = std::fabs(f) * 16777216.0f;                         // units of 2^-24
        return (uint16_t)(sign | (uint32_t)std::nearbyint(scaled));
    }
    const uint32_t rounded = x + 0xfffu + ((x >> 13) & 1u);                      // to nearest even at bit 13
    return (uint16_t)(sign | ((rounded - 0x38000000u) >> 13));
}

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
    std::vector<rf_half> image((size_t)width * height);
    std::vector<double> ref(image.size());
    unsigned long long s = 0x9E3779B97F4A7C15ull * 12;
    for (size_t i = 0; i < image.size(); i++) {      // SplitMix64 -> [0.25, 1.25), rounded to binary16
        s += 0x9E3779B97F4A7C15ull;
        unsigned long long z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        image[i].bits = float_to_half(0.25f + (float)(z >> 40) / 16777216.0f);
        ref[i] = (double)half_to_float(image[i].bits);
    }
    rf_half *d = nullptr;
    if (hipMalloc(&d, image.size() * sizeof(rf_half)) != hipSuccess) return 2;
    if (hipMemcpy(d, image.data(), image.size() * sizeof(rf_half), hipMemcpyHostToDevice) != hipSuccess) return 2;

    const std::vector<float> W = gaussian_weights(5.0f, 2);
    RecFilterDim x("x", width), y("y", height);
    RecFilter filter;
    filter.set_clamped_image_border();
    filter(x, y) = RecFilterImage(d);
    filter.add_filter(+x, W);
    filter.add_filter(-x, W);
    filter.add_filter(+y, W);
    filter.add_filter(-y, W);
    filter.split(x, 32, y, 32);
    std::vector<rf_half> out = filter.realize().to_host<rf_half>();
    (void)hipFree(d);
    if (out.size() != image.size()) { std::printf("unexpected result size %zu\n", out.size()); return 1; }

    loop_scan_clamped(ref, width, height, 0, true, W);
    loop_scan_clamped(ref, width, height, 0, false, W);
    loop_scan_clamped(ref, width, height, 1, true, W);
    loop_scan_clamped(ref, width, height, 1, false, W);
    double worst = 0.0;
    for (size_t i = 0; i < ref.size(); i++)
        worst = std::fmax(worst, std::fabs(ref[i] - (double)half_to_float(out[i].bits)) / std::fmax(std::fabs(ref[i]), 1e-6));
    const double bar = 1e-4 + 1.0 / 2048.0;
    std::printf("half frontend: max rel err %.4e against %.4e\n", worst, bar);
    if (!(worst < bar)) { std::printf("FAILED\n"); return 1; }
    std::printf("half-frontend-ok\n");
    return 0;
}
