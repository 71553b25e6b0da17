// Workgroup-wide integer scan of the metric kernels (det_eval.hip, coco_eval.hip): kThreads threads, exact, in thread order.
#pragma once
#include "common.h"

static_assert(kThreads == 256 && kThreads % MTP_WAVE == 0, "block_scan_add: four full waves per workgroup");

// inclusive sum over the workgroup's 256 threads, in thread order; total = the sum of all.  wsum: kThreads / MTP_WAVE words of LDS.
__device__ __forceinline__ unsigned long long block_scan_add(unsigned long long v, unsigned long long* wsum, int tid, unsigned long long& total) {
    const int lane = tid & (MTP_WAVE - 1), w = tid / MTP_WAVE;
    for (int off = 1; off < MTP_WAVE; off <<= 1) {
        const unsigned long long o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    __syncthreads();      // the readers of the previous call are done with wsum
    if (lane == MTP_WAVE - 1) wsum[w] = v;
    __syncthreads();
    unsigned long long before = 0ull, all = 0ull;
    for (int i = 0; i < kThreads / MTP_WAVE; ++i) {
        if (i < w) before += wsum[i];
        all += wsum[i];
    }
    total = all;
    return v + before;
}
