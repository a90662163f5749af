// Pieces the persistent inference renderers share (csrc/render.hip for the
// grid backbone, csrc/voxelrender.hip for the DVGO backbone): the batch
// constants, a ray's pending-slot list, the per-wave LDS stage, the queue's
// chunk-to-ray map and the f16 colour packing.  The queue order itself
// (dfhip_render_ray_order*) lives in render.hip and serves both.
#pragma once

#include "common.h"

namespace dfhip {
namespace rd {

#ifndef DFHIP_RENDER_K
#define DFHIP_RENDER_K 8
#endif
#ifndef DFHIP_RENDER_BATCH
#define DFHIP_RENDER_BATCH 64
#endif
constexpr int kK = DFHIP_RENDER_K;          // samples a ray may have pending per batch
constexpr int kBatch = DFHIP_RENDER_BATCH;  // a batch closes at >= kBatch staged samples
// empty cells a lane checks per march iteration (rm::march_step_ahead): their
// occupancy bytes load together.  K = 2: 1.830 -> 1.776 ms per frame (R0),
// 2.005 -> 1.963 (R1); K = 3 / 4 lose to the discarded candidates' work in
// occupied space (profiles/r06/c4_march_ahead_ab.txt)
#ifndef DFHIP_RENDER_AHEAD
#define DFHIP_RENDER_AHEAD 2
#endif
constexpr int kAhead = DFHIP_RENDER_AHEAD;
// pending slots, 8 bits each: one u64 holds 8, a second one up to 16
static_assert(kK >= 1 && kK <= 16, "kK: 1..16 pending samples");
struct PendSlots {
    uint64_t lo = 0, hi = 0;
    __device__ __forceinline__ void put(uint32_t i, uint32_t slot) {
        if (kK <= 8 || i < 8) lo |= (uint64_t)slot << (8 * (i & 7));
        else hi |= (uint64_t)slot << (8 * (i & 7));
    }
    __device__ __forceinline__ uint32_t get(uint32_t i) const {
        const uint64_t w = (kK <= 8 || i < 8) ? lo : hi;
        return (uint32_t)(w >> (8 * (i & 7))) & 0xFFu;
    }
};
constexpr int kSlots = kBatch + 64; // per-wave staged samples (< 64 added after the last check)
static_assert(kSlots <= 256, "PendSlots keeps LDS slot numbers in 8 bits: DFHIP_RENDER_BATCH <= 192");

// Per-wave LDS staging of one batch of samples, in the order the lanes found
// them.  pos holds the sample position until the field has read it, then
// (sigma, rgb as f16).
struct Stage {
    float pos[kSlots * 3];
    float dt[kSlots];
    float tc[kSlots];  // rays_t after the sample (the depth weight's t)
};

// Shading of the composited colour (the dfhip_shading codes; 0 = albedo).
constexpr int kAlbedo = 0, kTextureless = DFHIP_SHADING_TEXTURELESS,
              kLambertian = DFHIP_SHADING_LAMBERTIAN, kNormal = DFHIP_SHADING_NORMAL;
// The normal view composites f32 colours (sigma and two channels in the slot's
// pos words, the third here); the other modes pack f16 colours into pos.
template <int MODE> struct StageT : Stage {};
template <> struct StageT<kNormal> : Stage {
    float cz[kSlots];
};

// Ray j of queue chunk ch: 2^cl consecutive ray ids, or with tile_w (the
// width of a row-major image; cl = 6) pixel (j / 8, j % 8) of the image's
// 8 x 8 tile ch (tiles row-major).  A tile's rays stay closer in 3-D than a
// 64-pixel row strip's, so a wave's field gathers share more cache lines.
__device__ __forceinline__ uint32_t chunk_ray(uint32_t ch, uint32_t j, uint32_t cl,
                                              uint32_t tile_w) {
    if (!tile_w) return (ch << cl) + j;
    const uint32_t tw = tile_w >> 3, ty = ch / tw, tx = ch - ty * tw;
    return ((ty << 3) + (j >> 3)) * tile_w + (tx << 3) + (j & 7u);
}

__device__ __forceinline__ uint32_t pack_h2(half_t a, half_t b) {
    uint16_t ua, ub;
    __builtin_memcpy(&ua, &a, 2);
    __builtin_memcpy(&ub, &b, 2);
    return (uint32_t)ua | ((uint32_t)ub << 16);
}
__device__ __forceinline__ float lo_h(uint32_t v) {
    const uint16_t u = (uint16_t)(v & 0xFFFFu);
    half_t h;
    __builtin_memcpy(&h, &u, 2);
    return (float)h;
}
__device__ __forceinline__ float hi_h(uint32_t v) {
    const uint16_t u = (uint16_t)(v >> 16);
    half_t h;
    __builtin_memcpy(&h, &u, 2);
    return (float)h;
}

}  // namespace rd
}  // namespace dfhip
