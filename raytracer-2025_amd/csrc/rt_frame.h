// rt_frame.h -- the launch parameters of the path kernel: the frame and its
// work queue's shape (Frame), and the block the kernel reads them from (KParams).
#pragma once
#include <stdint.h>

#include "rt_kernel.h"
#include "rt_math.h"

namespace rtk {

struct Frame {
    uint32_t W, rows, row_offset, row_stride;
    uint32_t S;  // sqrt_spp
    uint32_t max_depth;
    uint32_t key0, key1;
    uint32_t total_items;
    // Work queue (item = launch pixel * S + s_i, a stratum row): the shard's
    // first whole_items items -- the pixels of its rows above the frame's
    // tail rows (rtk_tail_rows) -- are one entry each, a whole row of S
    // samples; every later item is `parts` entries of part_len consecutive
    // samples s_j (the last part the rest), so that the last entries of a
    // launch are short: a whole row of a pixel whose paths bounce 40 times
    // inside a glass sphere is ~10 ms of one wave (scripts/lane_trace.py).
    // The frame's last `fine` rows (rtk_tail_split) go out in finer parts
    // still -- parts2 entries of part_len2 samples, from queue entry fine_q0
    // and item fine_item0 on -- so that what is in flight when the queue
    // runs dry is about one sample a lane: a 1/8 row shard of C4 drained for
    // ~3 ms after its last 4-sample part was handed out (lane_trace_c4.json).
    // Entry q writes its f64 sum to partial slot q (queue order: the lanes
    // of a wave take consecutive entries, so their 24-B sums fill whole L2
    // lines), and the reduce adds a tail row's parts in part order.
    uint32_t parts, part_len, queue_total, whole_items;
    uint32_t parts2, part_len2, fine_q0, fine_item0;
    uint32_t static_entries;  // 64 per wave of the grid: their first pools, taken without the counter
    uint32_t chunk_min;  // smallest guided chunk (queue entries per atomic)
    uint32_t chunk_cap;  // largest guided chunk
    uint32_t chunk_min_whole;  // smallest guided chunk while whole-row entries are left
    // 1/parts, 1/S, 1/W rounded up (udiv_inv), and 1/(waves of the grid x
    // RT_QUEUE_GUIDE): the queue-entry decode without integer divisions
    double inv_parts, inv_parts2, inv_S, inv_W;
    float inv_guide;
    // samples per entry of each region and their reciprocals: the guided
    // chunk is the work left in samples / (waves x guide), in the entries of
    // the region the pool starts in
    float S_f, part_len_f, part_len2_f, inv_S_f, inv_part_len_f, inv_part_len2_f;
    uint32_t defocus;
    double recip_sqrt_spp, pixel_sample_scale;
    D3 center, pixel00, du, dv, disk_u, disk_v;
};

// Launch parameters live in device memory and are read where they are used
// (scalar loads), not pinned in SGPRs for the life of the kernel.
struct KParams {
    SceneView S;
    Frame F;
    uint32_t* queue;
    double* partial;  // [queue_total][3]: the f64 sum of each queue entry's samples
    unsigned long long* stats;
    RT_GLOBAL uint2* stack_ovf;  // mesh / full tiers: [stack_need - LDS entries][grid * RT_BLOCK]
    // Basic tier, batch variant: the launch's primary-ray candidates
    // (rt_primary.h: PRIMARY_CAP sphere indices per launch pixel, filled by
    // rt_primary_kernel ahead of the path kernel), and 1 / row_stride rounded
    // up (udiv_inv: image row -> shard row).  Appended, so that every other
    // field keeps its offset and the other kernels their code.
    const RT_GLOBAL uint4* cand;
    double inv_stride;
};

}  // namespace rtk
