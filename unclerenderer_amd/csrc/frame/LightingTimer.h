// LightingTimer — the frame's ring of HIP events around the Lighting pass (UR_FRAME_TIME_LIGHTING, _RECORD_COST, _KERNEL): an event pair
// around the pass, or carried on the Lighting dispatch itself, plus one more event right behind the pair (what a record costs).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

struct ur_ctx;

class FLightingTimer
{
public:
    bool bRecordAfter = false;  // this frame's bracket gets the third event (UR_FRAME_TIME_LIGHTING_RECORD_COST)
    bool bKernelEvents = false; // UR_FRAME_TIME_LIGHTING_KERNEL: the pair rides on the Lighting dispatch itself, nothing is recorded around it
    bool bStartOnCull = false;  // ... and this frame's START event was handed to the cull launch directly in front of the Lighting launch

    // Two launches in this frame, the cull and the Lighting launch that carries Build HZB: the cull's own completion stamp is the
    // start of the Lighting measurement.
    void StartOnCull(ur_ctx* Ctx);
    // FHotPathRenderer's hook: right before (bBegin) and after the Lighting pass launches, on the pass's context and stream
    void Mark(ur_ctx* Ctx, hipStream_t Stream, bool bBegin);
    // ur_frame_lighting_times_ex: the samples since the last call
    uint32_t Read(float* OutMs, float* OutRecordMs, uint32_t Cap);
    void Destroy();

private:
    // The slot of the next sample, with its events created if this is the ring's first use of it; false while the ring has none
    bool Grow();

    struct FEvents { hipEvent_t first, second, after; bool has_after; bool on_dispatch; };
    std::vector<FEvents> Events; // ring: an event pair around the Lighting pass + one more right behind it
    size_t Head = 0, Count = 0;
};
