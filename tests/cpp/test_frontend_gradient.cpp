// RecFilter::gradient (include/recfilter.hpp) against rf_plan_backward on the same plan and the same buffers, bit for bit: a
// clamped order-2 Gaussian +x -x +y -y on a 96 x 512 image, the input gradient alone and with the coefficient gradients, and
// the same filter with a zero border (one adjoint plan).  Compiled and run by tests/test_gpu_plan_grad.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "recfilter.hpp"

namespace {

constexpr int W = 512, H = 96, N_SCANS = 4;
constexpr size_t ROW = 1 + RF_MAX_ORDER;

uint32_t rng_state = 90210u;
float uniform() {      // xorshift32, [0, 1)
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) / 16777216.0f;
}

#define HIP_OK(e) do { if ((e) != hipSuccess) { std::printf("HIP error at line %d\n", __LINE__); return 1; } } while (0)
#define RF_CALL(e) do { if ((e) != RF_OK) { std::printf("line %d: %s\n", __LINE__, rf_last_error_string()); return 1; } } while (0)

int run(bool clamped) {
    const size_t n = (size_t)W * H, bytes = n * sizeof(float), row_bytes = N_SCANS * ROW * sizeof(double);
    std::vector<float> image(n), grad_out(n);
    for (auto &v : image) v = uniform();
    for (auto &v : grad_out) v = uniform() - 0.5f;
    float *d_image, *d_gout, *d_a, *d_b;
    double *d_ca, *d_cb;
    HIP_OK(hipMalloc((void **)&d_image, bytes));
    HIP_OK(hipMalloc((void **)&d_gout, bytes));
    HIP_OK(hipMalloc((void **)&d_a, bytes));
    HIP_OK(hipMalloc((void **)&d_b, bytes));
    HIP_OK(hipMalloc((void **)&d_ca, row_bytes));
    HIP_OK(hipMalloc((void **)&d_cb, row_bytes));
    HIP_OK(hipMemcpy(d_image, image.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_gout, grad_out.data(), bytes, hipMemcpyHostToDevice));
    std::vector<float> got_a(n), got_b(n);
    std::vector<double> rows_a(N_SCANS * ROW), rows_b(N_SCANS * ROW);
    try {
        const std::vector<float> w = {0.0975842401f, 1.5283848f, -0.625968993f};
        RecFilterDim x("x", W), y("y", H);
        RecFilter F("G");
        if (clamped) F.set_clamped_image_border();
        F(x, y) = RecFilterImage(d_image);
        F.add_filter(+x, w); F.add_filter(-x, w); F.add_filter(+y, w); F.add_filter(-y, w);
        F.split(x, 32, y, 32);
        for (int with_coeffs = 0; with_coeffs < 2; with_coeffs++) {
            HIP_OK(hipMemset(d_a, 0xff, bytes));
            HIP_OK(hipMemset(d_b, 0xff, bytes));
            if (with_coeffs) F.gradient({d_image}, {d_gout}, {d_a}, d_ca);
            else F.gradient({d_gout}, {d_a});
            rf_plan *plan = const_cast<rf_plan *>(F.plan());
            const void *in[1] = {d_image}, *gout[1] = {d_gout};
            void *gin[1] = {d_b};
            RF_CALL(rf_plan_backward(plan, with_coeffs ? in : nullptr, gout, gin, with_coeffs ? d_cb : nullptr, nullptr));
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(got_a.data(), d_a, bytes, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(got_b.data(), d_b, bytes, hipMemcpyDeviceToHost));
            if (std::memcmp(got_a.data(), got_b.data(), bytes) != 0) { std::printf("grad_in differs from the C ABI's (coeffs %d)\n", with_coeffs); return 1; }
            for (float v : got_a) if (v != v) { std::printf("NaN in grad_in (coeffs %d)\n", with_coeffs); return 1; }
            if (with_coeffs) {
                HIP_OK(hipMemcpy(rows_a.data(), d_ca, row_bytes, hipMemcpyDeviceToHost));
                HIP_OK(hipMemcpy(rows_b.data(), d_cb, row_bytes, hipMemcpyDeviceToHost));
                if (std::memcmp(rows_a.data(), rows_b.data(), row_bytes) != 0) { std::printf("coefficient gradients differ from the C ABI's\n"); return 1; }
                for (int s = 0; s < N_SCANS; s++) {
                    if (rows_a[s * ROW] == 0.0 || rows_a[s * ROW + 2] == 0.0) { std::printf("scan %d: a gradient is exactly 0\n", s); return 1; }
                    for (size_t j = 3; j < ROW; j++) if (rows_a[s * ROW + j] != 0.0) { std::printf("scan %d: entry %zu past the order is not 0\n", s, j); return 1; }
                }
            }
        }
        const int n1 = rf_plan_backward_num_kernels(const_cast<rf_plan *>(F.plan()), 0), n3 = rf_plan_backward_num_kernels(const_cast<rf_plan *>(F.plan()), 1);
        std::printf("%s border: %d launches, %d with coefficient gradients\n", clamped ? "clamped" : "zero", n1, n3);
        if (n1 <= 0 || n3 <= n1) return 1;
        // a refusal arrives as an exception with the library's text
        bool threw = false;
        try { F.gradient({d_image}, {d_gout}, {d_image}, d_ca); }
        catch (const RecFilterError &e) { threw = std::string(e.what()).find("overlaps") != std::string::npos; }
        if (!threw) { std::printf("grad_in on top of the input was not refused\n"); return 1; }
    } catch (const RecFilterError &e) {
        std::printf("RecFilterError: %s\n", e.what());
        return 1;
    }
    for (void *p : {(void *)d_image, (void *)d_gout, (void *)d_a, (void *)d_b, (void *)d_ca, (void *)d_cb}) (void)hipFree(p);
    return 0;
}

}  // namespace

int main() {
    if (run(true) != 0 || run(false) != 0) { std::printf("FAILED\n"); return 1; }
    std::printf("gradient-frontend-ok\n");
    return 0;
}
