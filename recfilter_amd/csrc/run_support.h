// run_support.h -- what the run functions of every plan family share (run_support.cpp): the events of a timed run and the checks
// of a call's planes.  rf_plan_execute (capi.cpp), rf_plan_backward (plan_adjoint.cpp), the varying scans (plan_var.cpp) and the
// smoothing plan (plan_smooth.cpp) all run through it: a run function takes a LaunchTimer & (or constructs the run's one) and marks
// it behind every launch, so one function serves the plain and the *_timed entry point.
#pragma once

#include <initializer_list>
#include <string>
#include <vector>

#include "rf_internal.h"

namespace rf {

// What a *_timed entry point does before it runs: ms_out has a slot per launch, and names_out (where given) receives the launches'
// names, name_of(i) for launch i (pointers that live as long as the plan).
template <typename NameOf>
int timed_names(size_t n, NameOf &&name_of, float *ms_out, const char **names_out, int capacity) {
    if (!ms_out || capacity < (int)n) { set_error("ms_out too small: need %zu", n); return RF_ERR_INVALID_ARG; }
    if (names_out)
        for (size_t i = 0; i < n; i++) names_out[i] = name_of(i);
    return RF_OK;
}
inline int timed_names(const std::vector<std::string> &names, float *ms_out, const char **names_out, int capacity) {
    return timed_names(names.size(), [&](size_t i) { return names[i].c_str(); }, ms_out, names_out, capacity);
}

// The events of one timed run: slot i of ms_out receives the time from the i-th mark (the construction is mark 0) to the next.
// ms_out == nullptr: a plain asynchronous run -- no event is created and every method returns RF_OK.  The events are destroyed
// on every path.  n_slots: the launches of the run, one name each (the caller of the run function has checked the capacity).
class LaunchTimer {
public:
    LaunchTimer(hipStream_t stream, float *ms_out, size_t n_slots);      // zero-fills ms_out; look at status() before launching
    ~LaunchTimer();
    LaunchTimer(const LaunchTimer &) = delete;
    LaunchTimer &operator=(const LaunchTimer &) = delete;
    int status() const { return status_; }
    int mark();         // behind every launch, and behind every slot whose launch was not issued
    void skip();        // just before mark(), for a slot whose launch was not issued: it reports 0 ms
    int finish();       // synchronises with the last mark and fills ms_out
private:
    int create();
    hipStream_t stream_;
    float *ms_out_;
    size_t n_slots_, marks_ = 0;
    int status_ = RF_OK;
    std::vector<hipEvent_t> events_;
    std::vector<size_t> skipped_;
};

// ---- the checks of a call's planes ------------------------------------------------------------------------------------------------
inline bool overlap(const void *a, size_t na, const void *b, size_t nb) { return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na; }

// Plane `index` of one or more arrays of a call: no pointer that is `required` is null, and every pointer (a null one passes) is
// aligned to mask + 1 bytes.  The refusals read "<what> <index>: <null_text>" and "<what> <index>: <align_text>".
struct PlanePointer {
    const void *p;
    bool required = true;
};
int check_plane(const char *what, int index, std::initializer_list<PlanePointer> pointers, uintptr_t mask, const char *null_text, const char *align_text);

// The aliasing rules of a single-image backward call: every plane that is written against every plane that is read, every other
// plane that is written, and the gradient it is computed from -- which alone it may be, plane for plane and exactly, and only
// written[0] (the image gradient: in place).  `noun` is how the messages name a plane of the array ("<noun> plane <index>"),
// `why` what follows where a written plane overlaps one of a read array.  Null planes are passed over.
struct PlaneList {
    const char *noun;
    const void *const *planes;
    int n;
    size_t bytes;            // of one plane
    const char *why = "";
};
int check_written_planes(const PlaneList *written, int n_written, const PlaneList *read, int n_read, const PlaneList &grad_out);

}  // namespace rf
