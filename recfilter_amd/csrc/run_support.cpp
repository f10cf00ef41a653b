// run_support.cpp -- the launch timer and the plane checks every plan family's run function uses (run_support.h).
#include "run_support.h"

namespace rf {

// ---- the launch timer -----------------------------------------------------------------------------------------------------------
LaunchTimer::LaunchTimer(hipStream_t stream, float *ms_out, size_t n_slots) : stream_(stream), ms_out_(ms_out), n_slots_(n_slots) {
    if (ms_out_) status_ = create();
}

LaunchTimer::~LaunchTimer() {
    for (hipEvent_t e : events_) (void)hipEventDestroy(e);
}

int LaunchTimer::create() {
    for (size_t i = 0; i < n_slots_; i++) ms_out_[i] = 0.0f;
    for (size_t i = 0; i < n_slots_ + 1; i++) {
        hipEvent_t e;
        RF_HIP_CHECK(hipEventCreate(&e));
        events_.push_back(e);
    }
    RF_HIP_CHECK(hipEventRecord(events_[0], stream_));
    return RF_OK;
}

int LaunchTimer::mark() {
    if (!ms_out_) return RF_OK;
    marks_++;
    RF_HIP_CHECK(hipEventRecord(events_[marks_], stream_));
    return RF_OK;
}

void LaunchTimer::skip() {
    if (ms_out_) skipped_.push_back(marks_);
}

int LaunchTimer::finish() {
    if (!ms_out_) return RF_OK;
    RF_HIP_CHECK(hipEventSynchronize(events_.back()));
    for (size_t i = 0; i < n_slots_; i++) RF_HIP_CHECK(hipEventElapsedTime(&ms_out_[i], events_[i], events_[i + 1]));
    for (size_t i : skipped_) ms_out_[i] = 0.0f;
    return RF_OK;
}

// ---- the shared checks ------------------------------------------------------------------------------------------------------------
int check_plane(const char *what, int index, std::initializer_list<PlanePointer> pointers, uintptr_t mask, const char *null_text, const char *align_text) {
    uintptr_t bits = 0;
    for (const PlanePointer &q : pointers) {
        if (q.required && !q.p) { set_error("%s %d: %s", what, index, null_text); return RF_ERR_INVALID_ARG; }
        bits |= (uintptr_t)q.p;
    }
    if ((bits & mask) != 0) { set_error("%s %d: %s", what, index, align_text); return RF_ERR_INVALID_ARG; }
    return RF_OK;
}

int check_written_planes(const PlaneList *written, int n_written, const PlaneList *read, int n_read, const PlaneList &grad_out) {
    for (int w = 0; w < n_written; w++)
        for (int i = 0; i < written[w].n; i++) {
            const void *o = written[w].planes[i];
            if (!o) continue;
            const size_t bytes = written[w].bytes;
            char name[64];
            std::snprintf(name, sizeof name, "%s plane %d", written[w].noun, i);
            for (int r = 0; r < n_read; r++)
                for (int q = 0; q < read[r].n; q++)
                    if (read[r].planes[q] && overlap(o, bytes, read[r].planes[q], read[r].bytes)) {
                        set_error("%s overlaps %s plane %d%s", name, read[r].noun, q, read[r].why);
                        return RF_ERR_INVALID_ARG;
                    }
            for (int v = w; v < n_written; v++)      // every written plane behind this one
                for (int j = v == w ? i + 1 : 0; j < written[v].n; j++)
                    if (written[v].planes[j] && overlap(o, bytes, written[v].planes[j], written[v].bytes)) {
                        set_error("%s overlaps %s plane %d", name, written[v].noun, j);
                        return RF_ERR_INVALID_ARG;
                    }
            for (int pl = 0; pl < grad_out.n; pl++) {
                if (w == 0 && i == pl && o == grad_out.planes[pl]) continue;      // in place: a plane and its own gradient, exactly
                if (overlap(o, bytes, grad_out.planes[pl], grad_out.bytes)) {
                    set_error("%s overlaps %s plane %d (only %s plane %d may, and then exactly)", name, grad_out.noun, pl, written[0].noun, pl);
                    return RF_ERR_INVALID_ARG;
                }
            }
        }
    return RF_OK;
}

}  // namespace rf
