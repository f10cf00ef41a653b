// test_frontend_u8_volume.cpp -- byte VOLUMES end to end through include/recfilter.hpp with a plain host compiler.
//
// RecFilterImage(const uint8_t *) / 255 binds a volume of unsigned bytes that the passes widen on load; the consumer
// RecFilterPointwise{255, 0, 0, to_bytes} is cast<uint8_t>(255 * blur) computed at the filter (rf_pointwise_desc.in_dtype =
// RF_IO_U8): realize() returns a volume of bytes, each min(max(rint(v), 0), 255) of the f32 value v, converted once.
// A Gaussian of order 2 (+x -x +y -y +z -z, clamped) is compared with raster loops in double under the one-rounding rule of
// tests/u8_cases.py,   |got - clip(want, 0, 255)| <= 0.5 + 1e-4 * |want|,   on two volumes (z, y, x):
//   64 x 128 x 256 = 2^21 samples: the NATIVE plan.  The front end always plans with RF_PATH_AUTO, which takes the native form
//       from 2^21 samples per plane on (plan.cpp, kByteVolumeNativeSamples), so this is the smallest volume of this width and
//       depth with which RecFilterPointwise::to_bytes reaches strided_final_u8_kernel.  Checked through RecFilter::plan():
//       one launch fewer than the RF_IN_U8 plan of the same description (no pointwise_post, no convert_out) and one f32 volume
//       more workspace.
//   64 x 96 x 256 = 2^20.6 samples: below the threshold, so the STAGED plan (one launch more than the RF_IN_U8 plan); the front
//       end has no path option that would ask for the native form at this size.  The same contract either way.
// Compiled and run by tests/test_gpu_u8_volumes.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "recfilter.hpp"

// one clamped scan along `dim` over a w x h x d volume, in place: samples before the border read as the border sample's input
// for the feed-forward history and as the scan's first output afterwards (the reference's clamped prologue)
static void loop_scan_clamped(std::vector<double> &img, int w, int h, int d, int dim, bool causal, const std::vector<float> &W) {
    const long ext[3] = {w, h, d}, strides[3] = {1, w, (long)w * h};
    const int n = (int)ext[dim];
    const int o1 = (dim + 1) % 3, o2 = (dim + 2) % 3;
    const long stride = strides[dim];
    const int k = (int)W.size() - 1;
    std::vector<double> y((size_t)n);
    for (long u = 0; u < ext[o1]; u++)
        for (long v = 0; v < ext[o2]; v++) {
            const long base = u * strides[o1] + v * strides[o2];
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

// launches and workspace of the RF_IN_U8 plan of the same description (f32 output), as the front end would describe it
static bool in_u8_plan_figures(int width, int height, int depth, const std::vector<float> &W, int *kernels, size_t *workspace) {
    rf_scan_desc sd[6] = {};
    for (int i = 0; i < 6; i++) {
        sd[i].dim = i / 2; sd[i].causal = i % 2 == 0; sd[i].order = (int)W.size() - 1; sd[i].feedfwd = W[0];
        for (size_t j = 1; j < W.size(); j++) sd[i].feedback[j - 1] = W[j];
    }
    rf_filter_desc d{};
    d.abi = RF_ABI; d.ndim = 3; d.extent[0] = width; d.extent[1] = height; d.extent[2] = depth;
    d.tile[0] = d.tile[1] = d.tile[2] = 32;
    d.dtype = RF_F32; d.n_planes = 1; d.border = RF_BORDER_CLAMP; d.n_scans = 6; d.scans = sd;
    d.path = RF_PATH_AUTO; d.device = -1; d.shard_rank = 0; d.shard_world = 1;
    d.pointwise.in_dtype = RF_IN_U8;
    d.pointwise.flags = RF_POINTWISE_PRE | RF_POINTWISE_POST;
    d.pointwise.pre_scale = 1.0f / 255.0f; d.pointwise.post_filtered = 255.0f;
    rf_plan *p = nullptr;
    if (rf_plan_create(&d, &p) != RF_OK) { std::printf("RF_IN_U8 plan: %s\n", rf_last_error_string()); return false; }
    *kernels = rf_plan_num_kernels(p);
    *workspace = (size_t)rf_plan_workspace_bytes(p);
    rf_plan_destroy(p);
    return true;
}

static int run_volume(int width, int height, int depth, bool expect_native) {
    std::vector<uint8_t> image((size_t)width * height * depth);
    std::vector<double> ref(image.size());
    const float scale = 1.0f / 255.0f;
    unsigned long long s = 0x9E3779B97F4A7C15ull * 23;
    for (size_t i = 0; i < image.size(); i++) {      // SplitMix64 -> seven bits
        s += 0x9E3779B97F4A7C15ull;
        unsigned long long z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        image[i] = (uint8_t)((z >> 57) + (i % (size_t)width) / 2);      // noise on a ramp along x: the blur keeps the ramp
        ref[i] = (double)(scale * (float)image[i]);         // x' as the passes form it, in f32
    }
    uint8_t *d = nullptr;
    if (hipMalloc(&d, image.size()) != hipSuccess) return 2;
    if (hipMemcpy(d, image.data(), image.size(), hipMemcpyHostToDevice) != hipSuccess) return 2;

    const std::vector<float> W = gaussian_weights(5.0f, 2);
    RecFilterDim x("x", width), y("y", height), z("z", depth);
    RecFilter filter;
    filter.set_clamped_image_border();
    filter(x, y, z) = RecFilterImage(d) / 255.0f;
    filter.add_filter(+x, W);
    filter.add_filter(-x, W);
    filter.add_filter(+y, W);
    filter.add_filter(-y, W);
    filter.add_filter(+z, W);
    filter.add_filter(-z, W);
    filter.split(x, 32, y, 32, z, 32);
    RecFilterPointwise to_bytes;
    to_bytes.w_filtered = 255.0f;
    to_bytes.to_bytes = true;
    filter.compute_at(to_bytes);
    RecFilterRealization r = filter.realize();
    if (!r.bytes || r.bytes_per_plane != image.size()) { std::printf("unexpected plane: bytes %d, %zu bytes per plane\n", (int)r.bytes, r.bytes_per_plane); return 1; }
    std::vector<uint8_t> out = r.to_host<uint8_t>();
    (void)hipFree(d);
    if (out.size() != image.size()) { std::printf("unexpected result size %zu\n", out.size()); return 1; }

    // which plan ran: against the RF_IN_U8 plan of the same description
    int in_kernels = 0;
    size_t in_workspace = 0;
    if (filter.plan() == nullptr || !in_u8_plan_figures(width, height, depth, W, &in_kernels, &in_workspace)) return 1;
    const int kernels = rf_plan_num_kernels(filter.plan());
    const size_t workspace = (size_t)rf_plan_workspace_bytes(filter.plan()), volume = image.size() * sizeof(float);
    const bool native = rf_plan_path(filter.plan()) == RF_PATH_TILED_FUSED && kernels == in_kernels - 1 && workspace >= in_workspace + volume;
    const bool staged = kernels == in_kernels + 1 && workspace >= in_workspace + volume;
    std::printf("%d x %d x %d: %d launches (the RF_IN_U8 plan: %d), workspace %zu (%zu): %s\n", depth, height, width, kernels, in_kernels,
                workspace, in_workspace, native ? "native" : staged ? "staged" : "neither form");
    if (expect_native ? !native : !staged) { std::printf("FAILED: expected the %s plan\n", expect_native ? "native" : "staged"); return 1; }

    for (int dim = 0; dim < 3; dim++) {
        loop_scan_clamped(ref, width, height, depth, dim, true, W);
        loop_scan_clamped(ref, width, height, depth, dim, false, W);
    }
    double worst = -1.0;
    int lo = 255, hi = 0;
    for (size_t i = 0; i < ref.size(); i++) {
        const double want = 255.0 * ref[i], clipped = std::fmin(std::fmax(want, 0.0), 255.0);
        worst = std::fmax(worst, std::fabs((double)out[i] - clipped) - (0.5 + 1e-4 * std::fabs(want)));
        lo = out[i] < lo ? out[i] : lo; hi = out[i] > hi ? out[i] : hi;
    }
    std::printf("u8 volume frontend: bytes %d..%d, worst |got - clip(want)| - (0.5 + 1e-4 |want|) = %.4e\n", lo, hi, worst);
    if (!(worst <= 0.0) || hi - lo < 16) { std::printf("FAILED\n"); return 1; }
    return 0;
}

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { std::fprintf(stderr, "no GPU\n"); return 2; }
    if (int rc = run_volume(256, 128, 64, /*expect_native=*/true)) return rc;
    if (int rc = run_volume(256, 96, 64, /*expect_native=*/false)) return rc;
    std::printf("u8-volume-frontend-ok\n");
    return 0;
}
