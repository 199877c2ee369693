// The targets of the multi-target loss heads (lpips.hip, idloss.hip, fploss.hip, pixloss.hip): one reconstruction read against k <= E4S_MAX_TARGETS targets, target j
// weighted by w[j].  Target j of sample b starts at y[j] + frame * fstride + b * (per-sample size), frame = *frame_idx when frame_idx is given (a device
// int32: a captured step selects the frame of a clip-wide cache by writing it before the replay; clamped to [0, nframes) so that a bad index cannot
// read past the cache) and 0 otherwise.
#pragma once
#include "common.h"

namespace e4s {

constexpr int MAX_TARGETS = E4S_MAX_TARGETS;

struct Targets {
    const float* y[MAX_TARGETS];
    float w[MAX_TARGETS];
    const int* frame;
    int64_t fstride;
    int nframes;
    int k;
};

// host: the kernel argument from the C ABI's (ys [k] device pointers, tw [k] weights, both host arrays); 0 or E4S_ERR_ARG with the error set
inline int make_targets(Targets& t, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes, const char* who) {
    E4S_REQUIRE(ys && tw && k >= 1 && k <= MAX_TARGETS, "%s: 1 .. %d targets with their weights, got %d", who, MAX_TARGETS, k);
    E4S_REQUIRE(fstride >= 0 && (frame == nullptr || (fstride > 0 && nframes >= 1)), "%s: a frame index needs a positive frame stride and frame count",
                who);
    for (int j = 0; j < MAX_TARGETS; ++j) {
        t.y[j] = j < k ? ys[j] : nullptr;
        t.w[j] = j < k ? tw[j] : 0.f;
        E4S_REQUIRE(j >= k || ys[j], "%s: target %d is null", who, j);
    }
    t.frame = frame;
    t.fstride = fstride;
    t.nframes = frame ? nframes : 1;
    t.k = k;
    return 0;
}

// device: where target j of the selected frame starts
__device__ __forceinline__ const float* target_base(const Targets& t, int j) {
    return t.y[j] + (t.frame ? (int64_t)min(max(t.frame[0], 0), t.nframes - 1) * t.fstride : (int64_t)0);
}

}  // namespace e4s
