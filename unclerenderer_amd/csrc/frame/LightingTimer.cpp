// LightingTimer.cpp — see LightingTimer.h.

#include "LightingTimer.h"

#include <hip/hip_runtime.h>

#include "../../../include/ur_hotpath.h"

bool FLightingTimer::Grow()
{
    constexpr size_t kRing = 1024;
    if (Events.size() < kRing && Count == Events.size()) {
        hipEvent_t a = nullptr, b = nullptr, c = nullptr;
        if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventCreate(&c) == hipSuccess) Events.push_back({a, b, c, false, false});
    }
    return !Events.empty();
}

void FLightingTimer::StartOnCull(ur_ctx* Ctx)
{
    bStartOnCull = Grow() && ur_time_next_cull(Ctx, Events[Count % Events.size()].first) == UR_OK;
}

void FLightingTimer::Mark(ur_ctx* Ctx, hipStream_t s, bool bBegin)
{
    if (!(bBegin ? Grow() : !Events.empty())) return;
    if (bKernelEvents) {
        if (bBegin) {
            Head = Count % Events.size();
            // stop = bound to the Lighting kernel's own dispatch (its completion signal's end stamp). start = the end stamp of the
            // dispatch directly in front of it when that is this frame's cull launch (StartOnCull handed it the event: NOTHING
            // enters the queue for the measurement), else a marker the runtime puts in front of the kernel (~8 us of queue time).
            // (One event alone measures nothing on this runtime: hipEventElapsedTime(e, e) is 0.)
            // (a cull call that launched nothing took no event: the marker form then, never a stamp left over from an earlier use of the slot)
            if (bStartOnCull && !ur_time_cull_carried(Ctx)) bStartOnCull = false;
            (void)ur_time_next_lighting(Ctx, bStartOnCull ? nullptr : Events[Head].first, Events[Head].second);
        } else {
            (void)ur_time_next_lighting(Ctx, nullptr, nullptr); // (a launch that failed validation consumed nothing)
            Events[Head].has_after = false;
            Events[Head].on_dispatch = true;
            ++Count;
        }
        return;
    }
    if (bBegin) {
        Head = Count % Events.size();
        (void)hipEventRecord(Events[Head].first, s);
    } else {
        (void)hipEventRecord(Events[Head].second, s);
        // a third record with nothing in front of it: second -> after is what one event record adds to the bracket
        Events[Head].has_after = bRecordAfter;
        Events[Head].on_dispatch = false;
        if (bRecordAfter) (void)hipEventRecord(Events[Head].after, s);
        ++Count;
    }
}

uint32_t FLightingTimer::Read(float* OutMs, float* OutRecordMs, uint32_t Cap)
{
    const size_t n = Count < Events.size() ? Count : Events.size();
    uint32_t k = 0;
    for (size_t i = 0; i < n && k < Cap; ++i) {
        float ms = 0.0f, rec = 0.0f;
        if (hipEventElapsedTime(&ms, Events[i].first, Events[i].second) != hipSuccess) continue;
        if (OutRecordMs) {
            rec = -1.0f; // no third event on this sample
            if (Events[i].has_after && hipEventElapsedTime(&rec, Events[i].second, Events[i].after) != hipSuccess) rec = -1.0f;
            OutRecordMs[k] = rec;
        }
        OutMs[k++] = ms;
    }
    Count = 0;
    return k;
}

void FLightingTimer::Destroy()
{
    for (auto& e : Events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); (void)hipEventDestroy(e.after); }
    Events.clear();
}
