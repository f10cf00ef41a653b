// RecFilterSmooth::batch (include/recfilter.hpp): a batch of 3 images of 2 planes, 70 x 260, with a separate one-plane guide per
// image, against three realizes and three gradients of a filter without a batch -- bit for bit, forward and backward (through the
// distances).  No tolerance: the single-image filter is held to loops by test_frontend_smooth.cpp and test_frontend_smooth_grad.cpp.
// Compiled and run by tests/test_gpu_smooth_batch.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int W = 260, H = 70, C = 2, N = 3, K = 2;
constexpr double SIGMA_S = 40.0, SIGMA_R = 0.5;

uint32_t rng_state = 40213u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)

bool same_bits(const char *what, const std::vector<float> &a, const std::vector<float> &b) {
    if (a.size() != b.size() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) != 0) {
        size_t i = 0;
        while (i < a.size() && i < b.size() && std::memcmp(&a[i], &b[i], sizeof(float)) == 0) i++;
        std::printf("%s: the batch differs from the single filters at sample %zu\n", what, i);
        return false;
    }
    std::printf("%s: %zu samples, the same bits\n", what, a.size());
    return true;
}

}  // namespace

int main() {
    const size_t plane = (size_t)W * H, image = plane * C;      // NCHW: image_stride = C*H*W, guide_stride = H*W
    std::vector<float> h_image(image * N), h_guide(plane * N), h_grad_out(image * N);
    for (auto &v : h_image) v = uniform();
    for (auto &v : h_guide) v = uniform();
    for (auto &v : h_grad_out) v = 2.0f * uniform() - 1.0f;
    enum { IMAGE, GUIDE, GRAD_OUT, OUT, GRAD_IMAGE, GRAD_GUIDE, OUT_1, GRAD_IMAGE_1, GRAD_GUIDE_1, N_BUFFERS };
    const size_t floats[N_BUFFERS] = {image * N, plane * N, image * N, image * N, image * N, plane * N, image * N, image * N, plane * N};
    float *d[N_BUFFERS] = {};
    for (int i = 0; i < N_BUFFERS; i++) HIP_OK(hipMalloc((void **)&d[i], floats[i] * sizeof(float)));
    HIP_OK(hipMemcpy(d[IMAGE], h_image.data(), floats[IMAGE] * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d[GUIDE], h_guide.data(), floats[GUIDE] * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d[GRAD_OUT], h_grad_out.data(), floats[GRAD_OUT] * sizeof(float), hipMemcpyHostToDevice));
    auto planes_of = [&](int buffer, int b, int count, size_t stride) {
        std::vector<void *> p;
        for (int pl = 0; pl < count; pl++) p.push_back(d[buffer] + (size_t)b * stride + (size_t)pl * plane);
        return p;
    };
    auto constant = [](const std::vector<void *> &p) { return std::vector<const void *>(p.begin(), p.end()); };
    try {
        RecFilterSmooth batched(W, H, C, 1, false, false, K, SIGMA_S, SIGMA_R);
        batched.batch(N, (int64_t)image, (int64_t)plane);
        RecFilterSmooth one(W, H, C, 1, false, false, K, SIGMA_S, SIGMA_R);
        if (batched.num_kernels() != one.num_kernels() || batched.gradient_num_kernels(true) != one.gradient_num_kernels(true) ||
            batched.num_kernels() != 1 + 6 * K || batched.gradient_num_kernels(true) != 34 * K - 4) {
            std::printf("the batch changed the launch counts: %d and %d\n", batched.num_kernels(), batched.gradient_num_kernels(true));
            return 1;
        }
        // the batch: the planes of image 0, one call each way
        batched.realize(constant(planes_of(IMAGE, 0, C, image)), constant(planes_of(GUIDE, 0, 1, plane)), planes_of(OUT, 0, C, image));
        batched.gradient(constant(planes_of(IMAGE, 0, C, image)), constant(planes_of(GUIDE, 0, 1, plane)), constant(planes_of(GRAD_OUT, 0, C, image)),
                         planes_of(GRAD_IMAGE, 0, C, image), planes_of(GRAD_GUIDE, 0, 1, plane), true);
        // three single filters' worth
        for (int b = 0; b < N; b++) {
            one.realize(constant(planes_of(IMAGE, b, C, image)), constant(planes_of(GUIDE, b, 1, plane)), planes_of(OUT_1, b, C, image));
            one.gradient(constant(planes_of(IMAGE, b, C, image)), constant(planes_of(GUIDE, b, 1, plane)), constant(planes_of(GRAD_OUT, b, C, image)),
                         planes_of(GRAD_IMAGE_1, b, C, image), planes_of(GRAD_GUIDE_1, b, 1, plane), true);
        }
        HIP_OK(hipDeviceSynchronize());
        // refusals arrive as exceptions with the library's text
        bool threw = false;
        try {
            batched.batch(2, (int64_t)image, (int64_t)plane);
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("before the first") != std::string::npos; }
        if (!threw) { std::printf("batch() after first use was not refused\n"); return 1; }
        threw = false;
        try {
            RecFilterSmooth bad(W, H, C, 1, false, false, K, SIGMA_S, SIGMA_R);
            bad.batch(N, (int64_t)image + 2, (int64_t)plane);
            bad.num_kernels();
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("multiples of 4") != std::string::npos; }
        if (!threw) { std::printf("a stride of 4k + 2 samples was not refused\n"); return 1; }
        threw = false;
        try {      // image 1's output planes on image 0's input planes
            batched.realize(constant(planes_of(IMAGE, 0, C, image)), constant(planes_of(GUIDE, 0, 1, plane)), planes_of(IMAGE, 1, C, image));
        } catch (const RecFilterError &e) { threw = std::string(e.what()).find("overlaps input plane") != std::string::npos; }
        if (!threw) { std::printf("output planes on another image's input planes were not refused\n"); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    bool ok = true;
    const int pairs[3][2] = {{OUT, OUT_1}, {GRAD_IMAGE, GRAD_IMAGE_1}, {GRAD_GUIDE, GRAD_GUIDE_1}};
    const char *names[3] = {"realize", "gradient, image", "gradient, guide"};
    for (int i = 0; i < 3; i++) {
        std::vector<float> a(floats[pairs[i][0]]), b(floats[pairs[i][1]]);
        HIP_OK(hipMemcpy(a.data(), d[pairs[i][0]], a.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(b.data(), d[pairs[i][1]], b.size() * sizeof(float), hipMemcpyDeviceToHost));
        ok = same_bits(names[i], a, b) && ok;
    }
    for (auto &p : d) (void)hipFree(p);
    if (!ok) { std::printf("FAILED\n"); return 1; }
    std::printf("smooth-batch-frontend-ok\n");
    return 0;
}
