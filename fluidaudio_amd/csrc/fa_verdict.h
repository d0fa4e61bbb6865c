// fa_verdict.h — how a plain-C++ argument pass or plan (der_geom.h, timeline_launch.h, paraformer_launch.h, tdt_merge_launch.h, vad_launch.h,
// kws_plan.h, speaker_db_core.h) reports a refusal
// without a context: the status and the text, which the host unit hands to fa::set_error — unchanged, or behind the entry's name.  No HIP
// call; the stand-alone programs under tests/cpu include it too.
#pragma once
#include <cstdarg>
#include <cstdio>

#include "../../include/fluidaudio_hip.h"

namespace fa {

struct Verdict {
    fa_status status = FA_SUCCESS;
    char text[192] = "";
};

#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline Verdict refuse(const fa_status status, const char *fmt, ...) {
    Verdict v;
    v.status = status;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(v.text, sizeof(v.text), fmt, ap);
    va_end(ap);
    return v;
}

}  // namespace fa
