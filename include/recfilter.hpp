// recfilter.hpp -- Halide-free C++ front-end with the surface of the reference's RecFilter
// (/root/reference lib/recfilter.h:68-566), implemented on top of the C ABI in recfilter_amd.h.
//
// Same class and method names, argument meaning and misuse behaviour as the reference.  The two
// unavoidable differences of a runtime without Halide:
//   * the defining right-hand side is a bound device image instead of a Halide::Expr:
//         R(x, y) = RecFilterImage<float>(device_ptr)            // one per Tuple element via {...}
//     (the reference: R(x,y) = image(x,y), lib/recfilter.cpp:150-162, 192-248)
//   * realize() returns RecFilterRealization (device pointers owned by the filter) instead of
//     Halide::Realization (lib/recfilter.cpp:984-989).
// Where the reference prints to cerr and assert(false)s this throws RecFilterError, which carries
// the same message.  Header-only; link against librecfilter_amd.so and the HIP runtime.
#pragma once

#include <hip/hip_runtime_api.h>

#include <chrono>
#include <functional>
#include <algorithm>
#include <cmath>
#include <ostream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "recfilter_amd.h"

class RecFilterError : public std::runtime_error {
public:
    explicit RecFilterError(const std::string &m) : std::runtime_error(m) {}
};

/** Filter dimension: a name and the image extent along it (lib/recfilter.h:68-95). */
class RecFilterDim {
    std::string v;
    int e = 0;
public:
    RecFilterDim() {}
    RecFilterDim(std::string var_name, int var_extent) : v(std::move(var_name)), e(var_extent) {}
    const std::string &var() const { return v; }
    int num_pixels() const { return e; }
};

/** Filter dimension augmented with causality (lib/recfilter.h:98-128). */
class RecFilterDimAndCausality {
    RecFilterDim r;
    bool c = true;
public:
    RecFilterDimAndCausality() {}
    RecFilterDimAndCausality(RecFilterDim rec_var, bool causal) : r(std::move(rec_var)), c(causal) {}
    const std::string &var() const { return r.var(); }
    int num_pixels() const { return r.num_pixels(); }
    bool causal() const { return c; }
};

/** +x: causal scan, -x: anticausal scan (lib/recfilter.h:135-139). */
inline RecFilterDimAndCausality operator+(RecFilterDim x) { return RecFilterDimAndCausality(std::move(x), true); }
inline RecFilterDimAndCausality operator-(RecFilterDim x) { return RecFilterDimAndCausality(std::move(x), false); }

template <typename T> struct RecFilterPixel;
template <> struct RecFilterPixel<float>   { static constexpr int dtype = RF_F32; };
template <> struct RecFilterPixel<double>  { static constexpr int dtype = RF_F64; };
template <> struct RecFilterPixel<int32_t> { static constexpr int dtype = RF_I32; };
template <> struct RecFilterPixel<int16_t> { static constexpr int dtype = RF_I16; };
/** 16-bit floating-point pixels: STORAGE types -- the planes hold IEEE binary16 / bfloat16 bit patterns, the filter runs in
 *  f32 and rounds once at the final store (recfilter_amd.h, rf_dtype).  Tag types any host compiler accepts; a compiler that
 *  has the native types may bind `const _Float16 *` / `const __bf16 *` planes as well. */
struct rf_half { uint16_t bits; };
struct rf_bfloat16 { uint16_t bits; };
template <> struct RecFilterPixel<rf_half>     { static constexpr int dtype = RF_F16; };
template <> struct RecFilterPixel<rf_bfloat16> { static constexpr int dtype = RF_BF16; };
#if defined(__HIP__)      /* hipcc: both native types exist on host and device */
template <> struct RecFilterPixel<_Float16>    { static constexpr int dtype = RF_F16; };
template <> struct RecFilterPixel<__bf16>      { static constexpr int dtype = RF_BF16; };
#endif

/** A dense x-fastest DEVICE image bound as (one Tuple element of) the filter's definition. */
struct RecFilterImageRef {
    const void *ptr = nullptr;
    int dtype = RF_F32;
    /** affine defining expression, e.g. `cast<float>(in)/255` (demo/demo_gaussian_filter.cpp:51-53): the filter
     *  runs on scale*image + bias, applied when the passes load pixels.  Shared by all Tuple elements. */
    float scale = 1.0f, bias = 0.0f;
    /** the buffer holds unsigned bytes that are converted to float on load (rf_pointwise_desc.in_dtype = RF_IN_U8);
     *  the filter itself is a float filter */
    bool bytes = false;
    RecFilterImageRef operator*(float s) const { RecFilterImageRef r = *this; r.scale *= s; r.bias *= s; return r; }
    RecFilterImageRef operator/(float s) const { return *this * (1.0f / s); }
    RecFilterImageRef operator+(float b) const { RecFilterImageRef r = *this; r.bias += b; return r; }
};

/** A pointwise consumer of a filter for RecFilter::compute_at: `w_filtered * F + w_input * I + bias`, I = the filter's
 *  own (scaled) input -- the unsharp mask `(1+w)*I - w*Blur` of apps/usm/unsharp_mask_optimized.cpp:57. */
struct RecFilterPointwise {
    float w_filtered = 1.0f, w_input = 0.0f, bias = 0.0f;
    /** the consumer is `cast<uint8_t>(...)` of that expression (a filter defined on a uint8 image only): realize() returns
     *  planes of unsigned bytes, each min(max(rint(v), 0), 255) of the float value v, converted once as the final pass stores
     *  it (rf_pointwise_desc.in_dtype = RF_IO_U8) */
    bool to_bytes = false;
};
template <typename T>
RecFilterImageRef RecFilterImage(const T *device_ptr) { return RecFilterImageRef{device_ptr, RecFilterPixel<T>::dtype}; }
/** `cast<float>(input(x,y))` of a uint8 image (demo/demo_gaussian_filter.cpp:51-53): the bytes are read directly by
 *  the passes; combine with `/ 255.0f`. */
inline RecFilterImageRef RecFilterImage(const uint8_t *device_ptr) {
    RecFilterImageRef r{device_ptr, RF_F32};
    r.bytes = true;
    return r;
}

/** Result of realize(): one device buffer per Tuple element, owned by the filter. */
struct RecFilterRealization {
    std::vector<void *> planes;
    std::vector<int64_t> extent;   // x first
    int dtype = RF_F32;
    size_t bytes_per_plane = 0;
    /** the planes hold unsigned bytes (a RecFilterPointwise::to_bytes consumer): read them with to_host<uint8_t>() */
    bool bytes = false;
    /** copy plane i to host memory */
    template <typename T> std::vector<T> to_host(size_t i = 0) const {
        std::vector<T> h(bytes_per_plane / sizeof(T));
        if (hipMemcpy(h.data(), planes.at(i), bytes_per_plane, hipMemcpyDeviceToHost) != hipSuccess)
            throw RecFilterError("hipMemcpy to host failed");
        return h;
    }
};

/** Error summary of a result against a reference, in the reference's terms (lib/recfilter.h:792-823): per-sample
 *  relative error in percent, 100 * |ref - out| / (ref + 1e-9), its maximum and its mean.  Streams like the
 *  reference's CheckResult ("Max relative error = ... %"). */
template <typename T>
struct CheckResult {
    float max_diff = 0.0f, mean_diff = 0.0f;
    CheckResult(const std::vector<T> &ref, const std::vector<T> &out) {
        if (ref.size() != out.size()) throw RecFilterError("CheckResult: images differ in size");
        double sum = 0.0;
        for (size_t i = 0; i < ref.size(); i++) {
            const float re = 100.0f * std::abs((float)ref[i] - (float)out[i]) / ((float)ref[i] + 1e-9f);
            sum += re;
            max_diff = std::max(max_diff, re);
        }
        mean_diff = ref.empty() ? 0.0f : (float)(sum / (double)ref.size());
    }
};
template <typename T>
std::ostream &operator<<(std::ostream &s, const CheckResult<T> &v) {
    return s << "Max  relative error = " << v.max_diff << " % \n" << "Mean relative error = " << v.mean_diff << " % \n\n";
}

class RecFilter;

/** Handle returned by intra_/inter_/full_schedule (lib/recfilter.h:516-566).  The reference's
 *  directives steer Halide's code generator; the kernels here are hand written, so every directive
 *  is accepted and recorded only. */
class RecFilterSchedule {
    std::shared_ptr<std::vector<std::string>> log;
    std::string what;
    RecFilterSchedule &note(const std::string &n) { log->push_back(what + "." + n); return *this; }
public:
    RecFilterSchedule(std::shared_ptr<std::vector<std::string>> l, std::string w) : log(std::move(l)), what(std::move(w)) {}
    template <typename... A> RecFilterSchedule &compute_globally(A...) { return note("compute_globally"); }
    template <typename... A> RecFilterSchedule &compute_locally(A...) { return note("compute_locally"); }
    template <typename... A> RecFilterSchedule &parallel(A...) { return note("parallel"); }
    template <typename... A> RecFilterSchedule &unroll(A...) { return note("unroll"); }
    template <typename... A> RecFilterSchedule &vectorize(A...) { return note("vectorize"); }
    template <typename... A> RecFilterSchedule &gpu_blocks(A...) { return note("gpu_blocks"); }
    template <typename... A> RecFilterSchedule &gpu_threads(A...) { return note("gpu_threads"); }
    template <typename... A> RecFilterSchedule &fuse(A...) { return note("fuse"); }
    template <typename... A> RecFilterSchedule &split(A...) { return note("split"); }
    template <typename... A> RecFilterSchedule &reorder(A...) { return note("reorder"); }
    template <typename... A> RecFilterSchedule &storage_layout(A...) { return note("storage_layout"); }
    template <typename... A> RecFilterSchedule &reorder_storage(A...) { return note("reorder_storage"); }
};

class RecFilterRefVar;

/** Recursive filter (lib/recfilter.h:146-510).  Copies alias the same contents
 *  (lib/recfilter.cpp:141-144). */
class RecFilter {
    struct Scan { int dim; bool causal; std::vector<float> coeff; };
    struct Contents {
        std::string name;
        std::vector<RecFilterDim> dims;
        std::vector<RecFilterImageRef> inputs;
        std::shared_ptr<Contents> source;       // cascaded stage: reads the previous stage's result
        std::vector<Scan> scans;
        std::map<std::string, int> tile;
        bool clamped = false, tiled = false, compiled = false, has_consumer = false;
        bool out_bytes = false;        // the planes realize() returns hold unsigned bytes (RecFilterPointwise::to_bytes)
        bool merged = false;                     // the plan holds the scans of the whole cascade this stage ends (compile_jit)
        bool merge_at_compile = true;            // merge_cascades() when the plan was built (toggled since: execute_chain plans again)
        RecFilterPointwise consumer;
        rf_plan *plan = nullptr;
        void *stream = nullptr;                  // HIP stream of enqueue() / realize() (set_stream); null = default stream
        std::vector<void *> out;                 // device buffers of the last realization
        int shard_rank = 0, shard_world = 1;     // shard(): this object describes ONE rank's slab of a larger image
        uint32_t plan_flags = 0;                 // plan_options(): rf_filter_desc.flags (RF_PLAN_*)
        std::vector<int64_t> shard_extents;      // ... the slab extents of all ranks (empty: all equal)
        std::vector<void *> xsend, xgathered;    // exchange buffers of realize_sharded(), one pair per exchange
        hipStream_t xstream = nullptr;           // side stream of the collective when the plan has exchange-independent work
        hipEvent_t xev_sent = nullptr, xev_got = nullptr;
        std::shared_ptr<std::vector<std::string>> schedule_log = std::make_shared<std::vector<std::string>>();
        ~Contents() {
            if (plan) rf_plan_destroy(plan);
            for (void *p : out) if (p) (void)hipFree(p);
            for (void *p : xsend) if (p) (void)hipFree(p);
            for (void *p : xgathered) if (p) (void)hipFree(p);
            if (xev_sent) (void)hipEventDestroy(xev_sent);
            if (xev_got) (void)hipEventDestroy(xev_got);
            if (xstream) (void)hipStreamDestroy(xstream);
        }
    };
    std::shared_ptr<Contents> c;
    static int &counter() { static int n = 0; return n; }
    static int &max_threads() { static int v = 128; return v; }
    static int &vec_width() { static int v = 8; return v; }
    [[noreturn]] static void fail(const std::string &m) { throw RecFilterError(m); }

    int dim_index(const std::string &var) const {
        for (size_t i = 0; i < c->dims.size(); i++) if (c->dims[i].var() == var) return (int)i;
        return -1;
    }
    size_t plane_elems() const { size_t n = 1; for (auto &d : c->dims) n *= (size_t)d.num_pixels(); return n; }
    int dtype() const { return c->source ? RecFilter(c->source).dtype() : c->inputs.at(0).dtype; }
    size_t n_planes() const { return c->source ? RecFilter(c->source).n_planes() : c->inputs.size(); }
    static size_t dtype_size(int dt) { return dt == RF_F64 ? 8 : ((dt == RF_I16 || dt == RF_F16 || dt == RF_BF16) ? 2 : 4); }
    explicit RecFilter(std::shared_ptr<Contents> p) : c(std::move(p)) {}

public:
    explicit RecFilter(std::string name = "") : c(std::make_shared<Contents>()) {
        c->name = (name.empty() ? std::string("R") : name) + "_" + std::to_string(counter()++);
    }
    std::string name() const { return c->name; }

    /** R(x), R(x,y), R(x,y,z) = image   (lib/recfilter.h:207-210) */
    RecFilterRefVar operator()(RecFilterDim x);
    RecFilterRefVar operator()(RecFilterDim x, RecFilterDim y);
    RecFilterRefVar operator()(RecFilterDim x, RecFilterDim y, RecFilterDim z);
    RecFilterRefVar operator()(std::vector<RecFilterDim> x);

    /** lib/recfilter.cpp:192-248 */
    void define(std::vector<RecFilterDim> pure_args, std::vector<RecFilterImageRef> pure_def) {
        if (pure_args.empty() || pure_def.empty()) fail("empty filter definition");
        for (auto &i : pure_def)
            if (i.dtype != pure_def[0].dtype) fail("Type of all Tuple elements in filter definition must be same");
        if (!c->dims.empty()) fail("Recursive filter " + c->name + " already defined");
        if (pure_args.size() > RF_MAX_DIMS) fail("at most 3 dimensions are supported");
        c->dims = std::move(pure_args);
        c->inputs = std::move(pure_def);
    }
    /** definition that reads another filter's result: f2(x,y) = f1.as_func()(x,y) in the reference */
    void define(std::vector<RecFilterDim> pure_args, const RecFilter &source) {
        if (!c->dims.empty()) fail("Recursive filter " + c->name + " already defined");
        c->dims = std::move(pure_args);
        c->source = source.c;
    }

    /** lib/recfilter.cpp:252-258 */
    void set_clamped_image_border() {
        if (!c->dims.empty()) fail("Recursive filter " + c->name + " already defined");
        c->clamped = true;
    }

    /** lib/recfilter.cpp:260-392; coeff = {feedforward, feedback_1 .. feedback_k} */
    void add_filter(RecFilterDim x, std::vector<float> coeff) { add_filter(RecFilterDimAndCausality(x, true), std::move(coeff)); }
    void add_filter(RecFilterDimAndCausality x, std::vector<float> coeff) {
        if (c->dims.empty())
            fail("Cannot add scans to recursive filter " + c->name + " before specifying an initial definition using RecFilter::define()");
        if (coeff.size() < 2)
            fail("Cannot add scan to recursive filter " + c->name + " without feed forward and feedback coefficients");
        int d = dim_index(x.var());
        if (d < 0) fail("Variable " + x.var() + " is not one of the dimensions of the recursive filter " + c->name);
        if (c->compiled) fail("cannot add scans after the filter is compiled");
        c->scans.push_back({d, x.causal(), std::move(coeff)});
    }

    /** lib/split.cpp:1850-2080 */
    void split(std::map<std::string, int> dims) {
        if (c->tiled) fail("Recursive filter cannot be tiled twice");
        for (auto &kv : dims) {
            int d = dim_index(kv.first);
            if (d < 0) fail("Variable " + kv.first + " is not a dimension of " + c->name);
            bool has = false;
            for (auto &s : c->scans) has = has || s.dim == d;
            if (!has) fail("Cannot tile dimension " + kv.first + " without any scans in it");
            if (kv.second <= 0 || c->dims[d].num_pixels() % kv.second) fail("tile does not divide the extent of " + kv.first);
        }
        c->tile = std::move(dims);
        c->tiled = true;
    }
    void split(RecFilterDim x, int tx) { split({{x.var(), tx}}); }
    void split(RecFilterDim x, int tx, RecFilterDim y, int ty) { split({{x.var(), tx}, {y.var(), ty}}); }
    void split(RecFilterDim x, int tx, RecFilterDim y, int ty, RecFilterDim z, int tz) {
        split({{x.var(), tx}, {y.var(), ty}, {z.var(), tz}});
    }
    void split_all_dimensions(int tx) {
        std::map<std::string, int> m;
        for (size_t d = 0; d < c->dims.size(); d++)
            for (auto &s : c->scans) if (s.dim == (int)d) { m[c->dims[d].var()] = tx; break; }
        split(m);
    }

    /** lib/reorder.cpp:28-229 */
    std::vector<RecFilter> cascade(std::vector<std::vector<int>> lists) {
        if (c->tiled || c->compiled)
            fail("Cascading directive cascade() cannot be used after the filter is already tiled, compiled or realized");
        std::vector<int> flat;
        for (auto &g : lists) for (int s : g) flat.push_back(s);
        const int n = (int)c->scans.size();
        for (int s : flat) if (s < 0 || s >= n) fail("Scan " + std::to_string(s) + " not found in recursive filter");
        for (size_t u = 0; u < flat.size(); u++)
            for (size_t v = u + 1; v < flat.size(); v++) {
                const Scan &a = c->scans[flat[u]], &b = c->scans[flat[v]];
                if (a.dim == b.dim && a.causal != b.causal && flat[v] < flat[u])
                    fail("Scans " + std::to_string(flat[u]) + " " + std::to_string(flat[v]) +
                         " cannot be reordered during cascading because they have opposite causality");
            }
        for (int s = 0; s < n; s++) {
            int count = 0;
            for (int f : flat) count += (f == s);
            if (count == 0) fail("Scan " + std::to_string(s) + " does not appear in the list of scans for cascading");
            if (count > 1) fail("Scan " + std::to_string(s) + " appears multiple times in the list of scans for cascading");
        }
        std::vector<RecFilter> out;
        for (size_t i = 0; i < lists.size(); i++) {
            RecFilter rf(c->name + "_" + std::to_string(i));
            if (c->clamped) rf.set_clamped_image_border();
            if (i == 0) { rf.c->dims = c->dims; rf.c->inputs = c->inputs; rf.c->source = c->source; }
            else rf.define(c->dims, out[i - 1]);
            for (int s : lists[i]) rf.c->scans.push_back(c->scans[s]);
            out.push_back(rf);
        }
        return out;
    }
    std::vector<RecFilter> cascade(std::vector<int> a, std::vector<int> b) { return cascade({std::move(a), std::move(b)}); }
    std::vector<RecFilter> cascade_by_causality() {
        std::vector<int> causal, anti;
        for (size_t d = 0; d < c->dims.size(); d++)
            for (size_t i = 0; i < c->scans.size(); i++)
                if (c->scans[i].dim == (int)d) (c->scans[i].causal ? causal : anti).push_back((int)i);
        return cascade({causal, anti});
    }
    std::vector<RecFilter> cascade_by_dimension() {
        std::vector<std::vector<int>> groups;
        for (size_t d = 0; d < c->dims.size(); d++) {
            std::vector<int> g;
            for (size_t i = 0; i < c->scans.size(); i++) if (c->scans[i].dim == (int)d) g.push_back((int)i);
            if (!g.empty()) groups.push_back(g);
        }
        return cascade(groups);
    }

    /** lib/reorder.cpp:231-381: `this` reads fA's result; merge both into one higher-order filter */
    RecFilter overlap_to_higher_order_filter(RecFilter fA, std::string name = "O") {
        if (c->tiled || fA.c->tiled) fail("overlap_to_higher_order_filter cannot be used on tiled filters");
        if (c->dims.size() != fA.c->dims.size()) fail("filters must have the same dimensions");
        RecFilter rf(std::move(name));
        if (fA.c->clamped) rf.set_clamped_image_border();
        rf.c->dims = fA.c->dims; rf.c->inputs = fA.c->inputs; rf.c->source = fA.c->source;
        for (size_t d = 0; d < c->dims.size(); d++) {
            std::vector<Scan> sa, sb;
            for (auto &s : fA.c->scans) if (s.dim == (int)d) sa.push_back(s);
            for (auto &s : c->scans) if (s.dim == (int)d) sb.push_back(s);
            if (sa.size() != sb.size()) fail("each dimension must have the same number of scans in both filters");
            for (size_t i = 0; i < sa.size(); i++) {
                if (sa[i].causal != sb[i].causal) fail("each scan of each dimension must have the same causality in both filters");
                std::vector<float> a(sa[i].coeff.begin() + 1, sa[i].coeff.end()), b(sb[i].coeff.begin() + 1, sb[i].coeff.end());
                std::vector<float> fb(a.size() + b.size());
                if (rf_overlap_feedback_coeff(a.data(), (int)a.size(), b.data(), (int)b.size(), fb.data()) != RF_OK)
                    fail(rf_last_error_string());
                fb.insert(fb.begin(), sa[i].coeff[0] * sb[i].coeff[0]);
                rf.c->scans.push_back({(int)d, sa[i].causal, fb});
            }
        }
        return rf;
    }

    /** schedule handles and auto-schedules: accepted, not needed (lib/recfilter.cpp:396-870) */
    RecFilterSchedule intra_schedule(int id = 0) { return RecFilterSchedule(c->schedule_log, "intra" + std::to_string(id)); }
    RecFilterSchedule inter_schedule() { return RecFilterSchedule(c->schedule_log, "inter"); }
    RecFilterSchedule full_schedule() {
        if (c->tiled) fail("Filter is tiled, use RecFilter::intra_schedule() and RecFilter::inter_schedule()");
        return RecFilterSchedule(c->schedule_log, "full");
    }
    /** lib/recfilter.cpp:473-573: compute the result inside a consumer's tiles.  With a pointwise consumer the final
     *  pass applies it to every sample before its only store; a RecFilter consumer needs nothing here (cascaded stages
     *  already read their producer's device buffer). */
    void compute_at(RecFilterPointwise consumer) {
        if (c->has_consumer) fail("Cannot compute " + c->name + " at another consumer because it already has a consumer");
        if (c->compiled) fail("compute_at must be called before the filter is compiled or realized");
        c->consumer = consumer;
        c->has_consumer = true;
    }
    /** lib/recfilter.cpp:473-573, compute_at(RecFilter external): a SCHEDULE directive there -- this filter's result is
     *  computed inside the tiles of the RecFilter that consumes it instead of going through memory; the result is the same
     *  with or without it.  Here a filter defined on another filter's output (cascade stages, R2(x,y) = R1) is realized as
     *  ONE plan over the head's input (cascade_chain below): the producer's result never exists in memory, which is what the
     *  directive asks for, so it is recorded and needs nothing else (no app or test of the reference uses it). */
    void compute_at(RecFilter external) { c->schedule_log->push_back("compute_at(" + external.c->name + "): the consumer's plan holds this filter's scans"); }
    void gpu_auto_schedule(int = 32) {}
    void gpu_auto_full_schedule(int = 32) {}
    void gpu_auto_inter_schedule() {}
    void gpu_auto_intra_schedule(int = 0) {}
    void cpu_auto_schedule() {}
    void cpu_auto_full_schedule() {}
    void cpu_auto_inter_schedule() {}
    void cpu_auto_intra_schedule() {}
    static void set_max_threads_per_cuda_warp(int v) {
        if (v % 32) fail("max threads per warp must be a multiple of 32");
        max_threads() = v;
    }
    static void set_vectorization_width(int v) {
        if (v < 2 || v > 64 || (v & (v - 1))) fail("vectorization width must be a power of two <= 64");
        vec_width() = v;
    }

    /** The stages of the cascade this filter ends, head first, when the whole chain IS one filter: the scans of a cascade
     *  are the scans of the filter it was made from (lib/reorder.cpp:100-176 distributes them over Funcs that read one
     *  another), scans of different dimensions commute and the scans of a dimension stay in order -- so the last stage's
     *  result is the result of ONE plan on the head's input with all the scans in stage order, which moves every sample once
     *  per pass instead of once per pass and stage (gaussian_1xy_2xy, apps/gaussian/gaussian_filter_1xy_2xy.cpp:44-54: four
     *  scans per dimension of order <= 2 = one fused stage).  Empty when a stage boundary carries something the merged plan
     *  cannot express (a consumer fused into an upstream stage, stages of different borders or extents) or merge_cascades()
     *  is off. */
    static bool &merge_cascades() { static bool on = true; return on; }
    std::vector<const Contents *> cascade_chain() const {
        std::vector<const Contents *> chain;
        if (!merge_cascades() || !c->source || c->shard_world > 1) return chain;
        for (const Contents *p = c.get(); p; p = p->source.get()) chain.insert(chain.begin(), p);
        for (const Contents *p : chain) {
            bool same = p->dims.size() == c->dims.size() && p->clamped == c->clamped && (p == c.get() || !p->has_consumer);
            for (size_t i = 0; same && i < p->dims.size(); i++)
                same = p->dims[i].var() == c->dims[i].var() && p->dims[i].num_pixels() == c->dims[i].num_pixels();
            if (!same) return {};
        }
        return chain;
    }

    /** lib/recfilter.cpp:918-930: builds the plan (tiling tables + kernels), replaces Func::compile_jit */
    void compile_jit(std::string = "") {
        if (c->dims.empty()) fail("filter has no definition");
        if (c->plan) { rf_plan_destroy(c->plan); c->plan = nullptr; }
        // The merged plan of a cascade may not exist where every stage's own plan does (more than RF_MAX_SCANS scans in all, a
        // combination no path accepts): then this stage is planned by itself and reads its source's result, as before the
        // merge existed.
        if (!cascade_chain().empty() && build_plan_for(cascade_chain())) return;
        if (!build_plan_for({})) fail(rf_last_error_string());
    }

    /** one attempt of compile_jit: the whole cascade `chain` as one plan, or (empty chain) this stage alone */
    bool build_plan_for(const std::vector<const Contents *> &chain) {
        c->merged = !chain.empty();
        std::vector<Scan> all;                              // the stage's scans, or those of the whole cascade in stage order
        if (c->merged) { for (const Contents *p : chain) all.insert(all.end(), p->scans.begin(), p->scans.end()); }
        else all = c->scans;
        const Contents *head = c->merged ? chain.front() : c.get();
        bool tiled = c->tiled;
        for (const Contents *p : chain) tiled = tiled || p->tiled;
        std::vector<rf_scan_desc> sd(all.size());
        for (size_t i = 0; i < sd.size(); i++) {
            const Scan &s = all[i];
            if ((int)s.coeff.size() - 1 > RF_MAX_ORDER) fail("filter order above RF_MAX_ORDER");
            sd[i].dim = s.dim; sd[i].causal = s.causal; sd[i].order = (int)s.coeff.size() - 1; sd[i].feedfwd = s.coeff[0];
            for (size_t j = 1; j < s.coeff.size(); j++) sd[i].feedback[j - 1] = s.coeff[j];
        }
        rf_filter_desc d{};
        d.abi = RF_ABI;
        d.ndim = (int)c->dims.size();
        for (int i = 0; i < d.ndim; i++) {
            d.extent[i] = c->dims[i].num_pixels();
            auto it = c->tile.find(c->dims[i].var());
            d.tile[i] = it == c->tile.end() ? 0 : it->second;
        }
        d.dtype = dtype(); d.n_planes = (int)n_planes();
        d.border = c->clamped ? RF_BORDER_CLAMP : RF_BORDER_ZERO;
        d.n_scans = (int)sd.size(); d.scans = sd.data();
        d.path = tiled ? RF_PATH_AUTO : RF_PATH_UNTILED;
        d.device = -1; d.shard_rank = c->shard_rank; d.shard_world = c->shard_world;
        d.shard_extents = c->shard_extents.empty() ? nullptr : c->shard_extents.data();
        d.flags = c->plan_flags;
        // (the defining expression belongs to the stage that reads the image: this one, or the head of the merged cascade)
        const bool head_bytes = !head->source && !head->inputs.empty() && head->inputs[0].bytes;
        c->out_bytes = c->has_consumer && c->consumer.to_bytes;
        if (c->out_bytes && !head_bytes) fail("a consumer that stores bytes needs a filter defined on a uint8 image, run as one plan");
        if (head_bytes) d.pointwise.in_dtype = c->out_bytes ? RF_IO_U8 : RF_IN_U8;
        if (!head->source && !head->inputs.empty() && (head->inputs[0].scale != 1.0f || head->inputs[0].bias != 0.0f)) {
            d.pointwise.flags |= RF_POINTWISE_PRE;
            d.pointwise.pre_scale = head->inputs[0].scale; d.pointwise.pre_bias = head->inputs[0].bias;
        }
        if (c->has_consumer) {
            d.pointwise.flags |= RF_POINTWISE_POST;
            d.pointwise.post_filtered = c->consumer.w_filtered; d.pointwise.post_input = c->consumer.w_input;
            d.pointwise.post_bias = c->consumer.bias;
        }
        if (rf_plan_create(&d, &c->plan) != RF_OK) { c->plan = nullptr; c->merged = false; return false; }
        c->compiled = true;
        c->merge_at_compile = merge_cascades();
        return true;
    }

    /** launches every upstream cascade stage, then this one, without synchronising: Func::realize on the last stage of
     *  a cascade recomputes all of its producers (they are compute_root Funcs) */
    void execute_chain() {
        if (c->compiled && c->merge_at_compile != merge_cascades()) c->compiled = false;      // toggled since: plan again
        if (!c->compiled) compile_jit();
        std::vector<const void *> in;
        if (c->merged) {                          // the whole cascade is this one plan: it reads the head's image
            const Contents *head = c.get();
            while (head->source) head = head->source.get();
            for (auto &i : head->inputs) in.push_back(i.ptr);
        } else if (c->source) { RecFilter up(c->source); up.execute_chain(); for (void *p : up.c->out) in.push_back(p); }
        else for (auto &i : c->inputs) in.push_back(i.ptr);
        const size_t bytes = out_plane_bytes();
        if (c->out.size() != in.size()) {
            for (void *p : c->out) (void)hipFree(p);
            c->out.assign(in.size(), nullptr);
            for (auto &p : c->out) if (hipMalloc(&p, bytes) != hipSuccess) fail("hipMalloc failed");
        }
        if (rf_plan_execute(c->plan, in.data(), c->out.data(), c->stream) != RF_OK) fail(rf_last_error_string());
    }
    /** bytes of one output plane: the pixel type's, or one per sample behind a to_bytes consumer */
    size_t out_plane_bytes() const { return plane_elems() * (c->out_bytes ? 1 : dtype_size(dtype())); }

    /** Not in the reference (it has no multi-device path): this object filters ONE rank's slab of an image that is
     *  partitioned along its outermost dimension over `world` GPUs, one process (or thread) per GPU.  The extents of the
     *  RecFilterDims are the LOCAL slab's; `extents` lists every rank's extent along the outermost dimension when they
     *  differ (whole tiles; the same list on every rank). */
    void shard(int rank, int world, std::vector<int64_t> extents = {}) {
        if (world < 1 || rank < 0 || rank >= world) fail("shard: rank out of range");
        if (!extents.empty() && (int)extents.size() != world) fail("shard: one extent per rank");
        c->shard_rank = rank; c->shard_world = world; c->shard_extents = std::move(extents);
        c->compiled = false;
    }

    /** Not in the reference: options of the plan behind realize() (rf_filter_desc.flags, RF_PLAN_* of recfilter_amd.h) --
     *  e.g. RF_PLAN_TILED_ONLY, or RF_PLAN_FORCE_EXCHANGE to drive a one-rank shard through enqueue_sharded(). */
    void plan_options(uint32_t flags) { c->plan_flags = flags; c->compiled = false; }

    /** `all_gather(send, gathered, bytes_per_rank, stream)`: every rank contributes `bytes_per_rank` device bytes and
     *  receives all ranks' contributions rank-major, ordered on `stream` (ncclAllGather(send, gathered, bytes, ncclChar,
     *  comm, (hipStream_t)stream) is exactly that). */
    using AllGather = std::function<void(const void *send, void *gathered, size_t bytes_per_rank, void *stream)>;

    /** enqueue() for a sharded filter: pass 1 and the slab-local carries, then per exchange (ONE for all scans of the
     *  sharded dimension up to order 3) the slab's exit carries, the caller's all-gather and the entering carries, then
     *  the final pass -- rf_plan_begin / exchange_local / exchange_apply / finish (include/recfilter_amd.h).  No
     *  synchronisation; the output planes are valid once the stream has drained. */
    RecFilterRealization enqueue_sharded(const AllGather &all_gather) {
        if (c->source) fail("a cascade cannot be sharded stage by stage: shard the merged filter");
        if (!c->compiled) compile_jit();
        std::vector<const void *> in;
        for (auto &i : c->inputs) in.push_back(i.ptr);
        const size_t bytes = plane_elems() * dtype_size(dtype());
        if (c->out.size() != in.size()) {
            for (void *p : c->out) (void)hipFree(p);
            c->out.assign(in.size(), nullptr);
            for (auto &p : c->out) if (hipMalloc(&p, bytes) != hipSuccess) fail("hipMalloc failed");
        }
        if (c->shard_world <= 1 && !(c->plan_flags & RF_PLAN_FORCE_EXCHANGE)) {
            if (rf_plan_execute(c->plan, in.data(), c->out.data(), c->stream) != RF_OK) fail(rf_last_error_string());
        } else {
            if (rf_plan_begin(c->plan, in.data(), c->out.data(), c->stream) != RF_OK) fail(rf_last_error_string());
            // whatever throws between here and rf_plan_finish (fail(), the caller's collective) hands the execution instance
            // back to the plan, so that the next realize starts afresh
            struct AbortUnlessFinished {
                rf_plan *plan; bool finished = false;
                ~AbortUnlessFinished() { if (!finished) (void)rf_plan_abort(plan); }
            } stepping_guard{c->plan};
            const int nex = rf_plan_num_exchanges(c->plan);
            if ((int)c->xsend.size() != nex) {
                for (void *p : c->xsend) (void)hipFree(p);
                for (void *p : c->xgathered) (void)hipFree(p);
                c->xsend.assign((size_t)nex, nullptr); c->xgathered.assign((size_t)nex, nullptr);
                for (int e = 0; e < nex; e++) {
                    const size_t xb = rf_plan_exchange_bytes(c->plan, e);
                    if (hipMalloc(&c->xsend[(size_t)e], xb) != hipSuccess ||
                        hipMalloc(&c->xgathered[(size_t)e], xb * (size_t)c->shard_world) != hipSuccess)
                        fail("hipMalloc failed");
                }
            }
            for (int e = 0; e < nex; e++) {
                if (rf_plan_exchange_local(c->plan, e, c->xsend[(size_t)e]) != RF_OK) fail(rf_last_error_string());
                if (e == nex - 1 && rf_plan_has_interior(c->plan)) {
                    // exchange-independent work (the x/y stage of a z-sharded volume): the collective goes to a side stream
                    // behind the exit carries, rf_plan_interior runs beside it, the apply step waits for it
                    if (!c->xstream) {
                        if (hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking) != hipSuccess ||
                            hipEventCreateWithFlags(&c->xev_sent, hipEventDisableTiming) != hipSuccess ||
                            hipEventCreateWithFlags(&c->xev_got, hipEventDisableTiming) != hipSuccess)
                            fail("hipStreamCreate failed");
                    }
                    if (hipEventRecord(c->xev_sent, (hipStream_t)c->stream) != hipSuccess || hipStreamWaitEvent(c->xstream, c->xev_sent, 0) != hipSuccess)
                        fail("hipEventRecord failed");
                    all_gather(c->xsend[(size_t)e], c->xgathered[(size_t)e], rf_plan_exchange_bytes(c->plan, e), c->xstream);
                    if (hipEventRecord(c->xev_got, c->xstream) != hipSuccess) fail("hipEventRecord failed");
                    if (rf_plan_interior(c->plan) != RF_OK) fail(rf_last_error_string());
                    if (hipStreamWaitEvent((hipStream_t)c->stream, c->xev_got, 0) != hipSuccess) fail("hipStreamWaitEvent failed");
                } else {
                    all_gather(c->xsend[(size_t)e], c->xgathered[(size_t)e], rf_plan_exchange_bytes(c->plan, e), c->stream);
                }
                if (rf_plan_exchange_apply(c->plan, e, c->xgathered[(size_t)e]) != RF_OK) fail(rf_last_error_string());
            }
            stepping_guard.finished = true;      // (rf_plan_finish ends the execute whether it succeeds or not)
            if (rf_plan_finish(c->plan) != RF_OK) fail(rf_last_error_string());
        }
        RecFilterRealization r;
        r.planes = c->out; r.dtype = dtype(); r.bytes_per_plane = bytes;
        for (auto &dm : c->dims) r.extent.push_back(dm.num_pixels());
        return r;
    }

    /** realize() for a sharded filter: enqueue_sharded, then this rank's stream is drained */
    RecFilterRealization realize_sharded(const AllGather &all_gather) {
        RecFilterRealization r = enqueue_sharded(all_gather);
        if (hipStreamSynchronize((hipStream_t)c->stream) != hipSuccess) fail("stream synchronisation failed");
        return r;
    }

    /** Not in the reference (Halide owns its streams): the HIP stream this filter's kernels run on (a hipStream_t).  Every
     *  stage of a cascade launches on its own setting: give all stages the same stream. */
    void set_stream(void *hip_stream) { c->stream = hip_stream; }

    /** realize() without the device synchronisation: launches the filter (and its upstream cascade stages) on its stream
     *  and returns the output planes, valid once the stream has drained.  Several RecFilter objects enqueued on
     *  different streams run beside each other -- the carry kernels of one under the passes of another. */
    RecFilterRealization enqueue() {
        execute_chain();
        RecFilterRealization r;
        r.planes = c->out; r.dtype = dtype(); r.bytes_per_plane = out_plane_bytes(); r.bytes = c->out_bytes;
        for (auto &dm : c->dims) r.extent.push_back(dm.num_pixels());
        return r;
    }

    /** lib/recfilter.cpp:984-989 */
    RecFilterRealization realize() {
        execute_chain();
        if (hipDeviceSynchronize() != hipSuccess) fail("device synchronisation failed");
        RecFilterRealization r;
        r.planes = c->out; r.dtype = dtype(); r.bytes_per_plane = out_plane_bytes(); r.bytes = c->out_bytes;
        for (auto &dm : c->dims) r.extent.push_back(dm.num_pixels());
        return r;
    }

    /** Not in the reference: the gradient of a loss through the filter (rf_plan_backward).  grad_out / grad_in: one device plane
     *  per Tuple element, f32; grad_in[p] may be grad_out[p].  The filter must run as ONE plan (a single stage, or a cascade
     *  compile_jit merged); it is compiled if it has not been.  Asynchronous on the filter's stream. */
    void gradient(const std::vector<const void *> &grad_out, const std::vector<void *> &grad_in) {
        backward_call(nullptr, grad_out, grad_in, nullptr);
    }
    /** ... and with respect to every coefficient: `input` = the planes the realization read, `grad_coeffs` = a DEVICE buffer of
     *  n_scans * (1 + RF_MAX_ORDER) doubles, row s = dL/dfeedfwd, dL/dfeedback[0..] of the s-th add_filter call */
    void gradient(const std::vector<const void *> &input, const std::vector<const void *> &grad_out, const std::vector<void *> &grad_in,
                  double *grad_coeffs) {
        if (!grad_coeffs) fail("gradient: null coefficient-gradient buffer");
        backward_call(&input, grad_out, grad_in, grad_coeffs);
    }

private:
    void backward_call(const std::vector<const void *> *input, const std::vector<const void *> &grad_out, const std::vector<void *> &grad_in,
                       double *grad_coeffs) {
        if (c->compiled && c->merge_at_compile != merge_cascades()) c->compiled = false;
        if (!c->compiled) compile_jit();
        if (c->source && !c->merged) fail("gradient: a cascade that is not merged into one plan has no single backward");
        const size_t n = n_planes();
        if (grad_out.size() != n || grad_in.size() != n || (input && input->size() != n)) fail("gradient: one plane per Tuple element is needed");
        if (rf_plan_backward(c->plan, input ? input->data() : nullptr, grad_out.data(), grad_in.data(), grad_coeffs, c->stream) != RF_OK)
            fail(rf_last_error_string());
    }

public:
    /** lib/recfilter.cpp:991-1016: one warm-up, then the mean time of `iterations` runs in ms, every run including the
     *  upstream stages of a cascade (unlike the reference the device is synchronised before the clock is read) */
    float profile(int iterations) {
        realize();
        auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < iterations; i++) execute_chain();
        if (hipDeviceSynchronize() != hipSuccess) fail("device synchronisation failed");
        std::chrono::duration<double, std::milli> dt = std::chrono::steady_clock::now() - t0;
        return (float)(dt.count() / (iterations > 0 ? iterations : 1));
    }

    std::string print_synopsis() const {
        std::ostringstream s;
        s << "RecFilter " << c->name << ":";
        for (auto &d : c->dims) s << " " << d.var() << "=" << d.num_pixels();
        s << "\n";
        for (size_t i = 0; i < c->scans.size(); i++) {
            s << "  scan " << i << ": " << (c->scans[i].causal ? "+" : "-") << c->dims[c->scans[i].dim].var() << " {";
            for (float v : c->scans[i].coeff) s << " " << v;
            s << " }\n";
        }
        if (c->plan) {
            int32_t t[RF_MAX_DIMS];
            rf_plan_tiles(c->plan, t);
            s << "  plan: path " << rf_plan_path(c->plan) << " tiles " << t[0] << " " << t[1] << " " << t[2] << "\n";
        }
        return s.str();
    }
    const std::vector<std::string> &schedule_log() const { return *c->schedule_log; }
    /** Not in the reference: the plan behind realize(), for the rf_plan_* queries of recfilter_amd.h (path, launches,
     *  workspace); null before compile_jit() / realize(), owned by the filter */
    const rf_plan *plan() const { return c->plan; }

    friend class RecFilterRefVar;
};

/** R(x,y) = image  (lib/recfilter.h:580-600) */
class RecFilterRefVar {
    RecFilter rf;
    std::vector<RecFilterDim> args;
public:
    RecFilterRefVar(RecFilter r, std::vector<RecFilterDim> a) : rf(std::move(r)), args(std::move(a)) {}
    void operator=(RecFilterImageRef image) { rf.define(args, std::vector<RecFilterImageRef>{image}); }
    void operator=(std::vector<RecFilterImageRef> tuple) { rf.define(args, std::move(tuple)); }
    void operator=(const RecFilter &source) { rf.define(args, source); }
};

inline RecFilterRefVar RecFilter::operator()(RecFilterDim x) { return RecFilterRefVar(*this, {x}); }
inline RecFilterRefVar RecFilter::operator()(RecFilterDim x, RecFilterDim y) { return RecFilterRefVar(*this, {x, y}); }
inline RecFilterRefVar RecFilter::operator()(RecFilterDim x, RecFilterDim y, RecFilterDim z) { return RecFilterRefVar(*this, {x, y, z}); }
inline RecFilterRefVar RecFilter::operator()(std::vector<RecFilterDim> x) { return RecFilterRefVar(*this, std::move(x)); }

inline std::ostream &operator<<(std::ostream &s, const RecFilter &r) { return s << r.print_synopsis(); }

/** coefficient helpers of lib/iir_coeff.h */
inline std::vector<float> gaussian_weights(float sigma, int order) {
    std::vector<float> c(order + 1);
    if (rf_gaussian_weights(sigma, order, c.data()) != RF_OK) throw RecFilterError(rf_last_error_string());
    return c;
}
inline std::vector<float> integral_image_coeff(int n) {
    std::vector<float> c(n + 1);
    if (rf_integral_image_coeff(n, c.data()) != RF_OK) throw RecFilterError(rf_last_error_string());
    return c;
}
inline std::vector<float> overlap_feedback_coeff(std::vector<float> a, std::vector<float> b) {
    std::vector<float> c(a.size() + b.size());
    if (rf_overlap_feedback_coeff(a.data(), (int)a.size(), b.data(), (int)b.size(), c.data()) != RF_OK)
        throw RecFilterError(rf_last_error_string());
    return c;
}
inline int gaussian_box_filter(int k, float sigma) {
    int w = 0;
    if (rf_gaussian_box_filter(k, sigma, &w) != RF_OK) throw RecFilterError(rf_last_error_string());
    return w;
}

/** The pointwise-with-offsets Funcs the reference's apps define on top of a filter's result (Halide expressions there):
 *  box_difference -- apps/box/box_filter.h:36-39, 128-139; tap_filter -- any clamped tap combination, e.g. diff_op_x /
 *  diff_op_y / diff_op_xy of apps/DoG/diff_gauss.cpp:176-197.  Device planes in, device plane out, on `stream`. */
inline void box_difference(const RecFilterRealization &table, int plane, void *out, int radius, std::vector<int32_t> order,
                           void *stream = nullptr) {
    order.resize(table.extent.size(), 0);
    if (rf_box_difference(table.planes.at((size_t)plane), out, (int)table.extent.size(), table.extent.data(), table.dtype, radius,
                          order.data(), stream) != RF_OK) throw RecFilterError(rf_last_error_string());
}
inline void tap_filter(const std::vector<const void *> &in_planes, void *out, const std::vector<int64_t> &extent, int dtype,
                       const std::vector<rf_tap> &taps, void *stream = nullptr) {
    if (rf_tap_filter(in_planes.data(), (int)in_planes.size(), out, (int)extent.size(), extent.data(), dtype, taps.data(),
                      (int)taps.size(), stream) != RF_OK) throw RecFilterError(rf_last_error_string());
}

/** Spatially varying first-order scans over 2-D f32 device planes (recfilter_amd.h, rf_var_plan_*): the edge-aware
 *  counterpart of a recursive Gaussian -- the domain-transform recursive filter runs `+x, -x, +y, -y` with a per-pixel
 *  feedback.  y[i] = (1 - w[i]) x[i] + w[i] y[i-1] along +dim; -dim couples sample i to i+1 through w[i+1]; element 0 of a weight
 *  plane along the scanned dimension is never used.
 *      RecFilterDim x("x", width), y("y", height);
 *      RecFilterVarying F(x, y);            // extents; the first dimension is the fastest
 *      F.add_scan(+x, 0); F.add_scan(-x, 0); F.add_scan(+y, 1); F.add_scan(-y, 1);
 *      F.realize({in}, {wx, wy}, {out});    // device pointers; in == out is allowed
 *      F.gradient({in}, {wx, wy}, {grad_out}, {grad_in}, {grad_wx, grad_wy});      // the adjoint, weight gradients optional
 *  The plan is built on the first realize() and kept; it owns one workspace: order the realizations of one object.
 *  A long 1-D signal (rf_var_plan_create_signal; a multiple of 4 samples, up to 2^30):
 *      RecFilterDim x("x", length);
 *      RecFilterVarying F(x);               // a "plane" is a dense f32 signal; scans are +x and -x
 *      F.add_scan(+x, 0); F.add_scan(-x, 0);
 *      F.realize({in}, {w}, {out});         // realize_power, gradient and gradient_power likewise */
class RecFilterVarying {
    std::vector<RecFilterDim> dims;
    std::vector<rf_var_scan_desc> scans;
    int n_weights = 0;
    rf_var_plan *plan = nullptr;
    int plan_planes = 0;
    void drop() { if (plan) { rf_var_plan_destroy(plan); plan = nullptr; } }
public:
    RecFilterVarying(RecFilterDim x, RecFilterDim y) : dims{std::move(x), std::move(y)} {}
    /** one long 1-D signal of x.num_pixels() samples (rf_var_plan_create_signal) */
    explicit RecFilterVarying(RecFilterDim x) : dims{std::move(x)} {}
    /** volumes [z][y][x] of x.num_pixels() x y.num_pixels() x z.num_pixels() samples (rf_var_plan_create_volume): a "plane" of
     *  realize() and gradient() is a dense f32 volume, a weight plane a volume of the same size, and scans run along x, y or z */
    RecFilterVarying(RecFilterDim x, RecFilterDim y, RecFilterDim z) : dims{std::move(x), std::move(y), std::move(z)} {}
    RecFilterVarying(const RecFilterVarying &) = delete;
    RecFilterVarying &operator=(const RecFilterVarying &) = delete;
    ~RecFilterVarying() { drop(); }
    /** one scan along +dim or -dim with the weight plane `weight_index` of realize() */
    void add_scan(const RecFilterDimAndCausality &d, int weight_index) {
        int dim = -1;
        for (size_t i = 0; i < dims.size(); i++) if (dims[i].var() == d.var()) dim = (int)i;
        if (dim < 0) throw RecFilterError("add_scan: '" + d.var() + "' is not a dimension of this filter");
        if (weight_index < 0) throw RecFilterError("add_scan: negative weight index");
        scans.push_back(rf_var_scan_desc{dim, d.causal() ? 1 : 0, weight_index});
        n_weights = std::max(n_weights, weight_index + 1);
        drop();
    }
    int num_kernels() const { return plan ? rf_var_plan_num_kernels(plan) : 0; }
    /** in / out: one device plane per channel; weights: the planes add_scan indexed.  Asynchronous on `stream`. */
    void realize(const std::vector<const void *> &in, const std::vector<const void *> &weights, const std::vector<void *> &out,
                 void *stream = nullptr) {
        prepare(in, weights.size(), out);
        if (rf_var_plan_execute(plan, in.data(), weights.data(), out.data(), stream) != RF_OK) throw RecFilterError(rf_last_error_string());
    }
    /** The power form (rf_var_plan_execute_power): plane k of `exponents` holds d >= 0 and the scans that index it use
     *  w = bases[k] ^ d, formed in the kernels; 0 < bases[k] < 1, one base per exponent plane.  The same plan as realize(). */
    void realize_power(const std::vector<const void *> &in, const std::vector<const void *> &exponents, const std::vector<float> &bases,
                       const std::vector<void *> &out, void *stream = nullptr) {
        prepare(in, exponents.size(), out);
        if ((int)bases.size() < n_weights) throw RecFilterError("realize_power: one base per exponent plane");
        if (rf_var_plan_execute_power(plan, in.data(), exponents.data(), bases.data(), out.data(), stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** The adjoint of realize() (rf_var_plan_backward): grad_in = dL/d(in) from grad_out = dL/d(out), and dL/d(weights[k]) into
     *  grad_weights[k] where that entry is not null.  grad_weights empty: the image gradient alone, and `in` may be empty too.
     *  grad_in[pl] == grad_out[pl] is allowed.  The same plan as realize(), on its workspace: order the calls. */
    void gradient(const std::vector<const void *> &in, const std::vector<const void *> &weights, const std::vector<const void *> &grad_out,
                  const std::vector<void *> &grad_in, const std::vector<void *> &grad_weights = {}, void *stream = nullptr) {
        if (!in.empty() && in.size() != grad_out.size()) throw RecFilterError("gradient: as many input planes as grad_out planes, or none");
        if (!grad_weights.empty() && grad_weights.size() != weights.size()) throw RecFilterError("gradient: one grad_weights entry per weight plane (null: no gradient), or none");
        prepare(grad_out, weights.size(), grad_in);
        if (rf_var_plan_backward(plan, in.empty() ? nullptr : in.data(), weights.data(), grad_out.data(), grad_in.data(),
                                 grad_weights.empty() ? nullptr : grad_weights.data(), stream) != RF_OK) throw RecFilterError(rf_last_error_string());
    }
    /** The adjoint of realize_power() (rf_var_plan_backward_power): as gradient(), with the exponent planes and their bases in the
     *  place of the weights; grad_exponents[k], where not null, receives dL/d(exponents[k]) = (w ln bases[k]) dL/dw. */
    void gradient_power(const std::vector<const void *> &in, const std::vector<const void *> &exponents, const std::vector<float> &bases,
                        const std::vector<const void *> &grad_out, const std::vector<void *> &grad_in,
                        const std::vector<void *> &grad_exponents = {}, void *stream = nullptr) {
        if (!in.empty() && in.size() != grad_out.size()) throw RecFilterError("gradient_power: as many input planes as grad_out planes, or none");
        if (!grad_exponents.empty() && grad_exponents.size() != exponents.size())
            throw RecFilterError("gradient_power: one grad_exponents entry per exponent plane (null: no gradient), or none");
        prepare(grad_out, exponents.size(), grad_in);
        if ((int)bases.size() < n_weights) throw RecFilterError("gradient_power: one base per exponent plane");
        if (rf_var_plan_backward_power(plan, in.empty() ? nullptr : in.data(), exponents.data(), bases.data(), grad_out.data(), grad_in.data(),
                                       grad_exponents.empty() ? nullptr : grad_exponents.data(), stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** gradient_power() with the gradient of the bases (rf_var_plan_backward_power_bases): grad_bases, a DEVICE buffer of one
     *  double per exponent plane (8-byte aligned), receives dL/d(bases[k]); grad_exponents may be empty or hold null entries. */
    void gradient_power_bases(const std::vector<const void *> &in, const std::vector<const void *> &exponents, const std::vector<float> &bases,
                              const std::vector<const void *> &grad_out, const std::vector<void *> &grad_in,
                              const std::vector<void *> &grad_exponents, double *grad_bases, void *stream = nullptr) {
        if (in.size() != grad_out.size()) throw RecFilterError("gradient_power_bases: as many input planes as grad_out planes");
        if (!grad_exponents.empty() && grad_exponents.size() != exponents.size())
            throw RecFilterError("gradient_power_bases: one grad_exponents entry per exponent plane (null: no gradient), or none");
        prepare(grad_out, exponents.size(), grad_in);
        if ((int)bases.size() < n_weights) throw RecFilterError("gradient_power_bases: one base per exponent plane");
        if (rf_var_plan_backward_power_bases(plan, in.data(), exponents.data(), bases.data(), grad_out.data(), grad_in.data(),
                                             grad_exponents.empty() ? nullptr : grad_exponents.data(), grad_bases, stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** launches of gradient_power_bases(): 7 per scan and one */
    int gradient_bases_num_kernels() const { return plan ? rf_var_plan_backward_bases_num_kernels(plan) : 0; }
    /** launches of gradient() and gradient_power(): 3 per scan, 7 with weight gradients */
    int gradient_num_kernels(bool with_weight_gradients) const { return plan ? rf_var_plan_backward_num_kernels(plan, with_weight_gradients ? 1 : 0) : 0; }
private:
    void prepare(const std::vector<const void *> &in, size_t weight_planes, const std::vector<void *> &out) {
        if (in.empty() || in.size() != out.size()) throw RecFilterError("realize: as many output planes as input planes, at least one");
        if ((int)weight_planes < n_weights) throw RecFilterError("realize: a scan indexes a weight plane that was not passed");
        if (!plan || plan_planes != (int)in.size()) {
            drop();
            if (dims.size() == 1) {
                rf_var_signal_desc sd{};
                sd.abi = RF_ABI;
                sd.length = dims[0].num_pixels();
                sd.dtype = RF_F32;
                sd.n_planes = (int)in.size();
                sd.n_weights = std::max(n_weights, 1);
                sd.n_scans = (int)scans.size();
                sd.scans = scans.data();
                sd.device = -1;
                if (rf_var_plan_create_signal(&sd, &plan) != RF_OK) throw RecFilterError(rf_last_error_string());
                plan_planes = (int)in.size();
                return;
            }
            if (dims.size() == 3) {
                rf_var_volume_desc vd{};
                vd.abi = RF_ABI;
                vd.width = dims[0].num_pixels();
                vd.height = dims[1].num_pixels();
                vd.depth = dims[2].num_pixels();
                vd.dtype = RF_F32;
                vd.n_planes = (int)in.size();
                vd.n_weights = std::max(n_weights, 1);
                vd.n_scans = (int)scans.size();
                vd.scans = scans.data();
                vd.device = -1;
                if (rf_var_plan_create_volume(&vd, &plan) != RF_OK) throw RecFilterError(rf_last_error_string());
                plan_planes = (int)in.size();
                return;
            }
            rf_var_desc d{};
            d.ndim = 2;
            d.abi = RF_ABI;
            d.extent[0] = dims[0].num_pixels();
            d.extent[1] = dims[1].num_pixels();
            d.dtype = RF_F32;
            d.n_planes = (int)in.size();
            d.n_weights = std::max(n_weights, 1);
            d.n_scans = (int)scans.size();
            d.scans = scans.data();
            d.device = -1;
            if (rf_var_plan_create(&d, &plan) != RF_OK) throw RecFilterError(rf_last_error_string());
            plan_planes = (int)in.size();
        }
    }
};

/** The exponent planes of the domain-transform filter from a guide image (rf_var_distances): d_x = 1 + scale * sum over the
 *  guide planes of |g - g one column to the left|, d_y the same with the row above; scale = sigma_s / sigma_r (over 255 for a
 *  uint8 guide that stands for guide / 255).  One launch on `stream`, on the current device.  With
 *  RecFilterVarying::realize_power and bases {a_k, a_k} per iteration this is the whole filter. */
inline void domain_transform_distances(const std::vector<const void *> &guide_planes, bool guide_u8, int64_t width, int64_t height,
                                       float scale, void *dx, void *dy, void *stream = nullptr) {
    if (rf_var_distances(guide_planes.data(), (int32_t)guide_planes.size(), guide_u8 ? 1 : 0, width, height, scale, dx, dy, -1,
                         stream) != RF_OK) throw RecFilterError(rf_last_error_string());
}

/** The exponent volumes of the filter on volumes [z][y][x] (rf_var_distances_volume): d_x and d_y slice by slice as
 *  domain_transform_distances forms them, d_z = spacing_z + scale * sum over the guide volumes of |g - g one slice before| (slice
 *  0: spacing_z).  spacing_z > 0 is the sample distance along z in units of the x/y pitch.  One launch on `stream`. */
inline void domain_transform_distances_volume(const std::vector<const void *> &guide_volumes, bool guide_u8, int64_t width, int64_t height,
                                              int64_t depth, float scale, float spacing_z, void *dx, void *dy, void *dz, void *stream = nullptr) {
    if (rf_var_distances_volume(guide_volumes.data(), (int32_t)guide_volumes.size(), guide_u8 ? 1 : 0, width, height, depth, scale, spacing_z,
                                dx, dy, dz, -1, stream) != RF_OK) throw RecFilterError(rf_last_error_string());
}

/** The adjoint of domain_transform_distances for f32 guide planes (rf_var_distances_backward): the guide's gradient from those of
 *  d_x and d_y, stored to grad_guide_planes or (accumulate) added to what they hold.  One launch on `stream`. */
inline void domain_transform_distances_gradient(const std::vector<const void *> &guide_planes, int64_t width, int64_t height, float scale,
                                                const void *grad_dx, const void *grad_dy, const std::vector<void *> &grad_guide_planes,
                                                bool accumulate = false, void *stream = nullptr) {
    if (guide_planes.size() != grad_guide_planes.size()) throw RecFilterError("domain_transform_distances_gradient: one gradient plane per guide plane");
    if (rf_var_distances_backward(guide_planes.data(), (int32_t)guide_planes.size(), width, height, scale, grad_dx, grad_dy,
                                  grad_guide_planes.data(), accumulate ? 1 : 0, -1, stream) != RF_OK) throw RecFilterError(rf_last_error_string());
}

/** The adjoint of domain_transform_distances_volume for f32 guide volumes (rf_var_distances_volume_backward): the guide's gradient
 *  from those of d_x, d_y and d_z (spacing_z does not enter), stored to grad_guide_volumes or (accumulate) added to what they hold.
 *  One launch on `stream`. */
inline void domain_transform_distances_volume_gradient(const std::vector<const void *> &guide_volumes, int64_t width, int64_t height, int64_t depth,
                                                       float scale, const void *grad_dx, const void *grad_dy, const void *grad_dz,
                                                       const std::vector<void *> &grad_guide_volumes, bool accumulate = false,
                                                       void *stream = nullptr) {
    if (guide_volumes.size() != grad_guide_volumes.size())
        throw RecFilterError("domain_transform_distances_volume_gradient: one gradient volume per guide volume");
    if (rf_var_distances_volume_backward(guide_volumes.data(), (int32_t)guide_volumes.size(), width, height, depth, scale, grad_dx, grad_dy, grad_dz,
                                         grad_guide_volumes.data(), accumulate ? 1 : 0, -1, stream) != RF_OK)
        throw RecFilterError(rf_last_error_string());
}

/** Edge-aware smoothing as one object (recfilter_amd.h, rf_smooth_plan_*): the domain-transform recursive filter of `planes`
 *  dense device planes of width x height, f32 or uint8 (bytes in AND out: sat8 of the f32 filter on the widened bytes, rounded
 *  once, at the final store).  guide_planes = 0: the image guides itself; else that many separate guide planes, f32 or uint8 (a
 *  byte guide means that guide divided by 255).  The library owns the distance planes and sequences 1 + 6 K launches.
 *      RecFilterSmooth F(width, height, 3, 0, false, true, 3, 60.0, 0.4);      // an RGB byte image guiding itself
 *      F.realize({r, g, b}, {}, {r, g, b});                                      // device pointers; in == out is allowed
 *  f32 images are differentiable: F.gradient(image, guide, grad_out, grad_image, grad_guide, edges) (rf_smooth_plan_backward);
 *  f32 volumes are where differentiable() was called before first use.
 *  The plan is built on first use and kept; it owns one workspace: order the realizations of one object. */
class RecFilterSmooth {
    rf_smooth_desc desc{};
    rf_smooth_plan *plan = nullptr;
    rf_smooth_batch_desc batch_desc{};
    bool batched = false;
    int64_t depth = 0;             // > 0: a volume (rf_smooth_plan_create_volume)
    double spacing_z = 1.0;
    bool volume_backward = false;  // differentiable(): RF_SMOOTH_VOLUME_BACKWARD
    void prepare() {
        if (plan) return;
        int rc;
        if (depth > 0) {
            if (batched) throw RecFilterError("a volume filter takes no batch");
            rf_smooth_volume_desc vd{};
            vd.abi = desc.abi;
            vd.image_u8 = desc.image_u8;
            vd.width = desc.width;
            vd.height = desc.height;
            vd.depth = depth;
            vd.n_planes = desc.n_planes;
            vd.n_guide = desc.n_guide;
            vd.guide_u8 = desc.guide_u8;
            vd.iterations = desc.iterations;
            vd.sigma_s = desc.sigma_s;
            vd.sigma_r = desc.sigma_r;
            vd.spacing_z = spacing_z;
            vd.device = desc.device;
            vd.flags = volume_backward ? RF_SMOOTH_VOLUME_BACKWARD : 0;
            rc = rf_smooth_plan_create_volume(&vd, &plan);
        } else {
            rc = batched ? rf_smooth_plan_create_batched(&desc, &batch_desc, &plan) : rf_smooth_plan_create(&desc, &plan);
        }
        if (rc != RF_OK) throw RecFilterError(rf_last_error_string());
    }
public:
    /** The filter along x, y and z of volumes [z][y][x] (rf_smooth_plan_create_volume): a "plane" of realize() is a dense volume,
     *  f32 or uint8; spacing_z > 0 is the sample distance along z in units of the x/y pitch.  1 + 9 K launches; no batch.
     *  gradient() is refused by the library unless differentiable() was called before first use. */
    RecFilterSmooth(int64_t width, int64_t height, int64_t depth_, int planes, int guide_planes, bool guide_u8, bool image_u8, int iterations,
                    double sigma_s, double sigma_r, double spacing_z_)
        : RecFilterSmooth(width, height, planes, guide_planes, guide_u8, image_u8, iterations, sigma_s, sigma_r) {
        if (depth_ < 1) throw RecFilterError("RecFilterSmooth: the depth of a volume must be positive");
        depth = depth_;
        spacing_z = spacing_z_;
    }
    RecFilterSmooth(int64_t width, int64_t height, int planes, int guide_planes, bool guide_u8, bool image_u8, int iterations,
                    double sigma_s, double sigma_r) {
        desc.abi = RF_ABI;
        desc.image_u8 = image_u8 ? 1 : 0;
        desc.width = width;
        desc.height = height;
        desc.n_planes = planes;
        desc.n_guide = guide_planes;
        desc.guide_u8 = guide_u8 ? 1 : 0;
        desc.iterations = iterations;
        desc.sigma_s = sigma_s;
        desc.sigma_r = sigma_r;
        desc.device = -1;
        desc.flags = 0;
    }
    RecFilterSmooth(const RecFilterSmooth &) = delete;
    RecFilterSmooth &operator=(const RecFilterSmooth &) = delete;
    ~RecFilterSmooth() { if (plan) rf_smooth_plan_destroy(plan); }
    /** Before first use: `n` images per realize() / gradient() call, every launch taking all of them (rf_smooth_plan_create_batched).
     *  The plane vectors then name image 0's planes; image b's are image_stride samples further per b (guide planes and their
     *  gradients: guide_stride; 0 where the image guides itself).  Contiguous NCHW: image_stride = C*H*W, guide_stride = G*H*W.
     *  Each image is filtered with its own edges, bit for bit as a filter without a batch filters it. */
    RecFilterSmooth &batch(int n, int64_t image_stride, int64_t guide_stride = 0) {
        if (plan) throw RecFilterError("batch: set before the first realize, gradient or query");
        batch_desc.batch = n;
        batch_desc.image_stride = image_stride;
        batch_desc.guide_stride = guide_stride;
        batched = true;
        return *this;
    }
    /** Before first use, on a volume filter of f32 volumes: the plan is created with RF_SMOOTH_VOLUME_BACKWARD, so gradient() and
     *  gradient_num_kernels() work on it (1 + 18 K launches, 51 K - 7 with edges; the workspace of edges is allocated by the first
     *  such call).  realize() is unchanged, bit for bit.  The library refuses the flag for uint8 volumes. */
    RecFilterSmooth &differentiable() {
        if (plan) throw RecFilterError("differentiable: set before the first realize, gradient or query");
        if (depth < 1) throw RecFilterError("differentiable: an image filter has its gradient already; this is for the volume constructor");
        volume_backward = true;
        return *this;
    }
    /** image / out: one device plane per channel; guide: the separate guide planes, empty when the image guides itself.
     *  Asynchronous on `stream`. */
    void realize(const std::vector<const void *> &image, const std::vector<const void *> &guide, const std::vector<void *> &out,
                 void *stream = nullptr) {
        prepare();
        if ((int)image.size() != desc.n_planes || (int)out.size() != desc.n_planes || (int)guide.size() != desc.n_guide)
            throw RecFilterError("realize: as many image, output and guide planes as the filter was built for");
        if (rf_smooth_plan_execute(plan, image.data(), guide.empty() ? nullptr : guide.data(), out.data(), stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** a_0 .. a_{K-1}: the f32 bases of the iterations */
    std::vector<float> bases() {
        prepare();
        std::vector<float> b((size_t)desc.iterations);
        if (rf_smooth_plan_bases(plan, b.data()) != RF_OK) throw RecFilterError(rf_last_error_string());
        return b;
    }
    /** New sigmas for the same plan (rf_smooth_plan_set_sigmas): the scale and the bases are recomputed as create computes them,
     *  nothing is allocated, and every later realize() and gradient() runs with them.  A refusal leaves the filter as it was. */
    void set_sigmas(double sigma_s, double sigma_r) {
        prepare();
        if (rf_smooth_plan_set_sigmas(plan, sigma_s, sigma_r) != RF_OK) throw RecFilterError(rf_last_error_string());
        desc.sigma_s = sigma_s;
        desc.sigma_r = sigma_r;
    }
    /** gradient() with the gradients of the scalars (rf_smooth_plan_backward_sigmas): grad_params, a DEVICE buffer of
     *  3 + iterations doubles (8-byte aligned), receives dL/dsigma_s, dL/dsigma_r, dL/dspacing_z, dL/da_0 .. dL/da_{K-1}, summed over
     *  the batch.  `image` is always needed; grad_image and grad_guide are bit for bit gradient()'s with the same `edges`. */
    void gradient_sigmas(const std::vector<const void *> &image, const std::vector<const void *> &guide, const std::vector<const void *> &grad_out,
                         const std::vector<void *> &grad_image, const std::vector<void *> &grad_guide, bool edges, double *grad_params,
                         void *stream = nullptr) {
        prepare();
        if ((int)image.size() != desc.n_planes || (int)grad_out.size() != desc.n_planes || (int)grad_image.size() != desc.n_planes ||
            (int)guide.size() != desc.n_guide || (!grad_guide.empty() && grad_guide.size() != guide.size()))
            throw RecFilterError("gradient_sigmas: as many image, gradient and guide planes as the filter was built for");
        if (rf_smooth_plan_backward_sigmas(plan, image.data(), guide.empty() ? nullptr : guide.data(), grad_out.data(), grad_image.data(),
                                           grad_guide.empty() ? nullptr : grad_guide.data(), edges ? 1 : 0, grad_params, stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    int gradient_sigmas_num_kernels(bool edges) { prepare(); return rf_smooth_plan_backward_sigmas_num_kernels(plan, edges ? 1 : 0); }
    int num_kernels() { prepare(); return rf_smooth_plan_num_kernels(plan); }
    /** The adjoint of realize() for f32 images (rf_smooth_plan_backward): grad_image = dL/d(image) from grad_out = dL/d(out).
     *  edges = false holds the distances constant (grad_guide empty; `image` may be empty unless the image guides itself).
     *  edges = true differentiates through them: with separate f32 guide planes grad_guide receives the guide's gradient; where
     *  the image guides itself grad_guide stays empty and that gradient is added into grad_image.  grad_image[pl] == grad_out[pl]
     *  is allowed.  On the plan's workspace: order the calls. */
    void gradient(const std::vector<const void *> &image, const std::vector<const void *> &guide, const std::vector<const void *> &grad_out,
                  const std::vector<void *> &grad_image, const std::vector<void *> &grad_guide = {}, bool edges = false, void *stream = nullptr) {
        prepare();
        if ((!image.empty() && (int)image.size() != desc.n_planes) || (int)grad_out.size() != desc.n_planes ||
            (int)grad_image.size() != desc.n_planes || (int)guide.size() != desc.n_guide || (!grad_guide.empty() && grad_guide.size() != guide.size()))
            throw RecFilterError("gradient: as many image, gradient and guide planes as the filter was built for");
        if (rf_smooth_plan_backward(plan, image.empty() ? nullptr : image.data(), guide.empty() ? nullptr : guide.data(), grad_out.data(),
                                    grad_image.data(), grad_guide.empty() ? nullptr : grad_guide.data(), edges ? 1 : 0, stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** launches of gradient(): 1 + 12 K, or 34 K - 4 with edges; a differentiable() volume filter: 1 + 18 K, or 51 K - 7; a volume
     *  filter without it: 0 */
    int gradient_num_kernels(bool edges) { prepare(); return rf_smooth_plan_backward_num_kernels(plan, edges ? 1 : 0); }
};

/** One time-varying second-order all-pole scan on dense f32 device signals (recfilter_amd.h, rf_var2_plan_*):
 *      y[n] = x[n] - a1[n] y[n-1] - a2[n] y[n-2]            (-x: y[n+1], y[n+2])
 *  with coefficient signals as long as the input; a coefficient that would multiply a sample outside the line is never used.
 *      RecFilterDim x("x", length);             // a multiple of 4, up to 2^30
 *      RecFilterVarying2 F(+x);                 // or -x; F(+x, lines, stride): `lines` signals `stride` samples apart
 *      F.realize(in, a1, a2, out);              // device pointers; in == out is allowed
 *      F.gradient(a1, a2, out, grad_out, grad_in, grad_a1, grad_a2);      // the adjoint; grad_a1 = grad_a2 = nullptr: grad_in only
 *  The plan is built on the first call and kept; it owns one workspace: order the calls of one object.  Zero-phase filtering is
 *  two objects, +x then -x.  Refusals arrive as RecFilterError with the library's text. */
class RecFilterVarying2 {
    rf_var2_signal_desc desc{};
    rf_var2_plan *plan = nullptr;
    void prepare() {
        if (!plan && rf_var2_plan_create_signal(&desc, &plan) != RF_OK) throw RecFilterError(rf_last_error_string());
    }
public:
    explicit RecFilterVarying2(const RecFilterDimAndCausality &x, int lines = 1, int64_t stride = 0) {
        desc.abi = RF_ABI;
        desc.length = x.num_pixels();
        desc.n_lines = lines;
        desc.stride = stride > 0 ? stride : desc.length;
        desc.causal = x.causal() ? 1 : 0;
        desc.device = -1;
        desc.flags = 0;
    }
    RecFilterVarying2(const RecFilterVarying2 &) = delete;
    RecFilterVarying2 &operator=(const RecFilterVarying2 &) = delete;
    ~RecFilterVarying2() { if (plan) rf_var2_plan_destroy(plan); }
    /** 3 */
    int num_kernels() { prepare(); return rf_var2_plan_num_kernels(plan); }
    /** 3, or 4 with coefficient gradients */
    int gradient_num_kernels(bool with_coefficients) { prepare(); return rf_var2_plan_backward_num_kernels(plan, with_coefficients ? 1 : 0); }
    size_t workspace_bytes() { prepare(); return rf_var2_plan_workspace_bytes(plan); }
    /** Asynchronous on `stream`. */
    void realize(const void *in, const void *a1, const void *a2, void *out, void *stream = nullptr) {
        prepare();
        if (rf_var2_plan_execute(plan, in, a1, a2, out, stream) != RF_OK) throw RecFilterError(rf_last_error_string());
    }
    /** The adjoint of realize() (rf_var2_plan_backward): grad_in = dL/d(in) from grad_out = dL/d(out); `out` is realize()'s result.
     *  grad_a1 and grad_a2: both null (no coefficient gradients; `out` may then be null) or both signals to be written.
     *  grad_in == grad_out is allowed. */
    void gradient(const void *a1, const void *a2, const void *out, const void *grad_out, void *grad_in, void *grad_a1 = nullptr,
                  void *grad_a2 = nullptr, void *stream = nullptr) {
        prepare();
        if (rf_var2_plan_backward(plan, a1, a2, out, grad_out, grad_in, grad_a1, grad_a2, stream) != RF_OK) throw RecFilterError(rf_last_error_string());
    }
    /** The whole section in direct form I (rf_var2_plan_execute_biquad), five coefficient signals as long as the input:
     *      v[n] = b0[n] in[n] + b1[n] in[n-1] + b2[n] in[n-2]        out[n] = v[n] - a1[n] out[n-1] - a2[n] out[n-2]
     *  (-x: the samples after n).  3 launches.  out overlaps none of the six inputs: in == out is refused. */
    void realize_biquad(const void *in, const void *b0, const void *b1, const void *b2, const void *a1, const void *a2, void *out,
                        void *stream = nullptr) {
        prepare();
        if (rf_var2_plan_execute_biquad(plan, in, b0, b1, b2, a1, a2, out, stream) != RF_OK) throw RecFilterError(rf_last_error_string());
    }
    /** The adjoint of realize_biquad() (rf_var2_plan_backward_biquad), 4 launches: grad_in from grad_out; `out` is realize_biquad()'s
     *  result.  The five coefficient gradients: all null (`out` may then be null) or all signals to be written.  grad_in == grad_out
     *  is allowed.  The plan allocates one signal for the adjoint state in the first call (biquad_gradient_bytes()). */
    void gradient_biquad(const void *in, const void *b0, const void *b1, const void *b2, const void *a1, const void *a2, const void *out,
                         const void *grad_out, void *grad_in, void *grad_b0 = nullptr, void *grad_b1 = nullptr, void *grad_b2 = nullptr,
                         void *grad_a1 = nullptr, void *grad_a2 = nullptr, void *stream = nullptr) {
        prepare();
        if (rf_var2_plan_backward_biquad(plan, in, b0, b1, b2, a1, a2, out, grad_out, grad_in, grad_b0, grad_b1, grad_b2, grad_a1, grad_a2,
                                         stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** 3 */
    int biquad_num_kernels() { prepare(); return rf_var2_plan_biquad_num_kernels(plan); }
    /** 4 */
    int biquad_gradient_num_kernels() { prepare(); return rf_var2_plan_backward_biquad_num_kernels(plan); }
    size_t biquad_gradient_bytes() { prepare(); return rf_var2_plan_backward_biquad_bytes(plan); }
    /** The section with its coefficients at a control rate (rf_var2_plan_execute_biquad_frames): every member of `frames` is
     *  frames_count(hop) f32 values per line, frame j at sample j * hop, lines frame_stride values apart (0: dense); between two
     *  frames the kernels interpolate linearly in registers -- bit for bit realize_biquad() on the expanded signals.  hop: a
     *  power of two, 64 .. 65536.  3 launches.  out overlaps neither in nor a frame array. */
    void realize_biquad_frames(const void *in, const rf_var2_section &frames, int hop, void *out, int64_t frame_stride = 0,
                               void *stream = nullptr) {
        prepare();
        const int count = frames_count(hop);
        if (rf_var2_plan_execute_biquad_frames(plan, in, &frames, hop, count, frame_stride > 0 ? frame_stride : count, out, stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** The adjoint of realize_biquad_frames() (rf_var2_plan_backward_biquad_frames), 4 launches, or 5 with frame gradients:
     *  frame_grads null (`out` may then be null) or five arrays laid out like the frames, to be written -- the per-sample
     *  gradients contracted in f64 and rounded once.  grad_in == grad_out is allowed. */
    void gradient_biquad_frames(const void *in, const rf_var2_section &frames, int hop, const void *out, const void *grad_out, void *grad_in,
                                const rf_var2_section_grad *frame_grads = nullptr, int64_t frame_stride = 0, void *stream = nullptr) {
        prepare();
        const int count = frames_count(hop);
        if (rf_var2_plan_backward_biquad_frames(plan, in, &frames, hop, count, frame_stride > 0 ? frame_stride : count, out, grad_out, grad_in,
                                                frame_grads, stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** ceil(length / hop) + 1; 0 for a hop the library refuses */
    int frames_count(int hop) const { return rf_var2_frames_count((int)desc.length, hop); }
    /** 3 */
    int biquad_frames_num_kernels() { prepare(); return rf_var2_plan_biquad_frames_num_kernels(plan); }
    /** 4, or 5 with frame gradients */
    int biquad_frames_gradient_num_kernels(bool with_frames) { prepare(); return rf_var2_plan_backward_biquad_frames_num_kernels(plan, with_frames ? 1 : 0); }
    size_t biquad_frames_gradient_bytes(int hop) { prepare(); return rf_var2_plan_backward_biquad_frames_bytes(plan, hop); }
    /** A cascade of 1 .. RF_VAR2_MAX_SECTIONS such sections in this object's direction (rf_var2_plan_execute_cascade), section
     *  k + 1 on the result of section k, each with five coefficient signals of its own: 2 K + 1 launches, one link launch per
     *  boundary between two sections.  out overlaps neither in nor any coefficient signal. */
    void realize_cascade(const void *in, const std::vector<rf_var2_section> &sections, void *out, void *stream = nullptr) {
        prepare();
        if (rf_var2_plan_execute_cascade(plan, in, sections.data(), (int)sections.size(), out, stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** The adjoint of realize_cascade() (rf_var2_plan_backward_cascade): grad_in from grad_out; `out` is realize_cascade()'s result.
     *  grads: empty (no coefficient gradients; `out` may then be null) or one rf_var2_section_grad per section, every pointer a
     *  signal to be written.  grad_in == grad_out is allowed.  Nothing is kept from the forward: the call reruns all sections but
     *  the last into signals the plan owns (cascade_gradient_bytes()). */
    void gradient_cascade(const void *in, const std::vector<rf_var2_section> &sections, const void *out, const void *grad_out, void *grad_in,
                          const std::vector<rf_var2_section_grad> &grads = {}, void *stream = nullptr) {
        prepare();
        if (!grads.empty() && grads.size() != sections.size())
            throw RecFilterError("gradient_cascade: grads is empty or holds one rf_var2_section_grad per section");
        if (rf_var2_plan_backward_cascade(plan, in, sections.data(), (int)sections.size(), out, grad_out, grad_in,
                                          grads.empty() ? nullptr : grads.data(), stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** 2 K + 1 */
    int cascade_num_kernels(int sections) { prepare(); return rf_var2_plan_cascade_num_kernels(plan, sections); }
    /** 4 at K = 1, 6 K - 1 above */
    int cascade_gradient_num_kernels(int sections) { prepare(); return rf_var2_plan_backward_cascade_num_kernels(plan, sections); }
    size_t cascade_gradient_bytes(int sections) { prepare(); return rf_var2_plan_backward_cascade_bytes(plan, sections); }
    /** realize_cascade() with every section's result kept, for training (rf_var2_plan_execute_cascade_keep): kept holds one
     *  signal per section but the last, laid out like in, and receives section k's result in kept[k]; out is realize_cascade()'s
     *  bit for bit.  The signals are the caller's; a kept signal overlaps nothing else in the call. */
    void realize_cascade_keep(const void *in, const std::vector<rf_var2_section> &sections, void *out, const std::vector<void *> &kept,
                              void *stream = nullptr) {
        prepare();
        if (kept.size() + 1 != sections.size())
            throw RecFilterError("realize_cascade_keep: kept holds one signal per section but the last");
        if (rf_var2_plan_execute_cascade_keep(plan, in, sections.data(), (int)sections.size(), out, kept.empty() ? nullptr : kept.data(),
                                              stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** The adjoint of realize_cascade_keep() on what it kept (rf_var2_plan_backward_cascade_kept): nothing is rerun, one adjoint
     *  link launch per boundary between two sections.  grads: empty (no coefficient gradients: in, out and kept may then be null
     *  and empty, nothing of the forward is read) or one rf_var2_section_grad per section.  grad_in == grad_out is allowed.  The
     *  plan owns one signal, two for two sections or more (cascade_kept_gradient_bytes()). */
    void gradient_cascade_kept(const void *in, const std::vector<rf_var2_section> &sections, const std::vector<const void *> &kept,
                               const void *out, const void *grad_out, void *grad_in, const std::vector<rf_var2_section_grad> &grads = {},
                               void *stream = nullptr) {
        prepare();
        if (!grads.empty() && grads.size() != sections.size())
            throw RecFilterError("gradient_cascade_kept: grads is empty or holds one rf_var2_section_grad per section");
        if (!kept.empty() && kept.size() + 1 != sections.size())
            throw RecFilterError("gradient_cascade_kept: kept is empty or holds one signal per section but the last");
        if (rf_var2_plan_backward_cascade_kept(plan, in, sections.data(), (int)sections.size(), kept.empty() ? nullptr : kept.data(), out,
                                               grad_out, grad_in, grads.empty() ? nullptr : grads.data(), stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** 2 K + 2 without coefficient gradients, 3 K + 1 with them */
    int cascade_kept_gradient_num_kernels(int sections, bool with_coefficients) {
        prepare();
        return rf_var2_plan_backward_cascade_kept_num_kernels(plan, sections, with_coefficients ? 1 : 0);
    }
    size_t cascade_kept_gradient_bytes(int sections) { prepare(); return rf_var2_plan_backward_cascade_kept_bytes(plan, sections); }
    /** realize_cascade() with every section's coefficients at a control rate (rf_var2_plan_execute_cascade_frames): frames[k]
     *  holds section k's five frame arrays as realize_biquad_frames() takes them, one hop and one frame_stride (0: dense) for all
     *  sections.  2 K + 1 launches that read no coefficient signal; bit for bit realize_cascade() on the expanded signals.  kept:
     *  empty (v and the result in out, in place) or one signal per section but the last, which receives section k's result in
     *  kept[k] -- out has the same bits either way. */
    void realize_cascade_frames(const void *in, const std::vector<rf_var2_section> &frames, int hop, void *out,
                                const std::vector<void *> &kept = {}, int64_t frame_stride = 0, void *stream = nullptr) {
        prepare();
        if (!kept.empty() && kept.size() + 1 != frames.size())
            throw RecFilterError("realize_cascade_frames: kept is empty or holds one signal per section but the last");
        const int count = frames_count(hop);
        if (rf_var2_plan_execute_cascade_frames(plan, in, frames.data(), (int)frames.size(), hop, count, frame_stride > 0 ? frame_stride : count,
                                                out, kept.empty() ? nullptr : kept.data(), stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** The adjoint of realize_cascade_frames() on what it kept (rf_var2_plan_backward_cascade_frames): nothing is rerun.
     *  frame_grads: empty (no frame gradients: in, out and kept may then be null and empty) or one rf_var2_section_grad per
     *  section, five arrays laid out like the frames, to be written -- the per-sample gradients contracted in f64 and rounded
     *  once.  grad_in == grad_out is allowed.  The plan owns two signals and the slab (cascade_frames_gradient_bytes()). */
    void gradient_cascade_frames(const void *in, const std::vector<rf_var2_section> &frames, int hop, const std::vector<const void *> &kept,
                                 const void *out, const void *grad_out, void *grad_in, const std::vector<rf_var2_section_grad> &frame_grads = {},
                                 int64_t frame_stride = 0, void *stream = nullptr) {
        prepare();
        if (!frame_grads.empty() && frame_grads.size() != frames.size())
            throw RecFilterError("gradient_cascade_frames: frame_grads is empty or holds one rf_var2_section_grad per section");
        if (!kept.empty() && kept.size() + 1 != frames.size())
            throw RecFilterError("gradient_cascade_frames: kept is empty or holds one signal per section but the last");
        const int count = frames_count(hop);
        if (rf_var2_plan_backward_cascade_frames(plan, in, frames.data(), (int)frames.size(), hop, count, frame_stride > 0 ? frame_stride : count,
                                                 kept.empty() ? nullptr : kept.data(), out, grad_out, grad_in,
                                                 frame_grads.empty() ? nullptr : frame_grads.data(), stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** 2 K + 1 (3 at K = 1) */
    int cascade_frames_num_kernels(int sections) { prepare(); return rf_var2_plan_cascade_frames_num_kernels(plan, sections); }
    /** 2 K + 2 without frame gradients, 3 K + 2 with them; 4 and 5 at K = 1 */
    int cascade_frames_gradient_num_kernels(int sections, bool with_frames) {
        prepare();
        return rf_var2_plan_backward_cascade_frames_num_kernels(plan, sections, with_frames ? 1 : 0);
    }
    size_t cascade_frames_gradient_bytes(int sections, int hop) { prepare(); return rf_var2_plan_backward_cascade_frames_bytes(plan, sections, hop); }
    /** realize_cascade_frames() on one CHUNK of a longer signal (rf_var2_plan_execute_cascade_frames_stream): state_in enters
     *  (null: silence), state_out receives the state that leaves (null: not wanted) -- K + 1 pairs of f32 per line, pair 0 the
     *  two last samples of the input, pair k + 1 those of section k's result, the nearest first, state_stride floats from line to
     *  line (0: dense, 2 (K + 1)).  frames: the chunk's own -- for a chunk that starts at a multiple of hop, the whole signal's
     *  frame arrays advanced by start / hop.  A filter over -x takes its chunks last to first.  2 K + 1 launches; both state
     *  pointers null: realize_cascade_frames() itself. */
    void realize_cascade_frames_stream(const void *in, const std::vector<rf_var2_section> &frames, int hop, void *out, const void *state_in,
                                       void *state_out, const std::vector<void *> &kept = {}, int64_t frame_stride = 0, int64_t state_stride = 0,
                                       void *stream = nullptr) {
        prepare();
        if (!kept.empty() && kept.size() + 1 != frames.size())
            throw RecFilterError("realize_cascade_frames_stream: kept is empty or holds one signal per section but the last");
        const int count = frames_count(hop);
        if (rf_var2_plan_execute_cascade_frames_stream(plan, in, frames.data(), (int)frames.size(), hop, count, frame_stride > 0 ? frame_stride : count,
                                                       out, kept.empty() ? nullptr : kept.data(), state_in, state_out,
                                                       state_stride > 0 ? state_stride : 2 * ((int64_t)frames.size() + 1), stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** The adjoint of realize_cascade_frames_stream() on what it kept (rf_var2_plan_backward_cascade_frames_stream):
     *  gradient_cascade_frames()'s arguments, then state_in (what entered the forward; read for the frame gradients alone),
     *  grad_state_out (the gradient of the state that left, e.g. the next chunk's grad_state_in; null: zeros) and grad_state_in
     *  (written; null: not wanted), laid out like the state.  All three null: gradient_cascade_frames() itself. */
    void gradient_cascade_frames_stream(const void *in, const std::vector<rf_var2_section> &frames, int hop, const std::vector<const void *> &kept,
                                        const void *out, const void *grad_out, void *grad_in, const void *state_in, const void *grad_state_out,
                                        void *grad_state_in, const std::vector<rf_var2_section_grad> &frame_grads = {}, int64_t frame_stride = 0,
                                        int64_t state_stride = 0, void *stream = nullptr) {
        prepare();
        if (!frame_grads.empty() && frame_grads.size() != frames.size())
            throw RecFilterError("gradient_cascade_frames_stream: frame_grads is empty or holds one rf_var2_section_grad per section");
        if (!kept.empty() && kept.size() + 1 != frames.size())
            throw RecFilterError("gradient_cascade_frames_stream: kept is empty or holds one signal per section but the last");
        const int count = frames_count(hop);
        if (rf_var2_plan_backward_cascade_frames_stream(plan, in, frames.data(), (int)frames.size(), hop, count, frame_stride > 0 ? frame_stride : count,
                                                        kept.empty() ? nullptr : kept.data(), out, grad_out, grad_in,
                                                        frame_grads.empty() ? nullptr : frame_grads.data(), state_in, grad_state_out, grad_state_in,
                                                        state_stride > 0 ? state_stride : 2 * ((int64_t)frames.size() + 1), stream) != RF_OK)
            throw RecFilterError(rf_last_error_string());
    }
    /** 2 K + 2 without frame gradients, 3 K + 2 with them, K = 1 included */
    int cascade_frames_stream_gradient_num_kernels(int sections, bool with_frames) {
        prepare();
        return rf_var2_plan_backward_cascade_frames_stream_num_kernels(plan, sections, with_frames ? 1 : 0);
    }
    /** 2 K + 1, K = 1 included */
    int cascade_frames_stream_num_kernels(int sections) { prepare(); return rf_var2_plan_cascade_frames_stream_num_kernels(plan, sections); }
    /** the bytes of one state buffer; state_stride 0: dense */
    size_t cascade_frames_stream_state_bytes(int sections, int64_t state_stride = 0) {
        prepare();
        return rf_var2_plan_cascade_frames_stream_state_bytes(plan, sections, state_stride > 0 ? state_stride : 2 * ((int64_t)sections + 1));
    }
};
