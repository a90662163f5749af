// Device building blocks of the non-albedo shadings (finite-difference
// normal, the autocast light product, the lambertian term), shared by the
// train-step kernels (shade.hip) and the shaded fused inference renderer
// (render.hip).  Both users are built with -ffp-contract=off, so they round
// identically.  See shade.hip for the reference lines and the rounding points.
#pragma once

#include "common.h"

namespace dfhip {
namespace shd {

// round to the autocast element type E (f16 or bf16), through an f32 value
template <typename E>
__device__ __forceinline__ float rnd(float x) { return (float)(E)f32_rounded(x); }

struct Normal {
    float v[3], n[3], r, ss;
    bool nan[3];
};

// network_grid.py:90-121 (f32): v = -(0.5 * (s+ - s-) / eps), n = v / sqrt(clamp(|v|^2, 1e-20))
__device__ __forceinline__ Normal fd_normal(const float *__restrict__ sigma7, uint32_t i,
                                            float eps) {
    Normal o;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float sp = sigma7[7 * (size_t)i + 1 + 2 * a];
        const float sn = sigma7[7 * (size_t)i + 2 + 2 * a];
        o.v[a] = -((0.5f * (sp - sn)) / eps);
    }
    o.ss = (o.v[0] * o.v[0] + o.v[1] * o.v[1]) + o.v[2] * o.v[2];
    // torch.clamp(min=1e-20) propagates a NaN |v|^2 (fmaxf alone would return
    // 1e-20): r is NaN, every component of v / r is NaN and the normal is 0
    o.r = sqrtf(o.ss != o.ss ? o.ss : fmaxf(o.ss, 1e-20f));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = o.v[a] / o.r;
        o.nan[a] = q != q;
        o.n[a] = o.nan[a] ? 0.0f : q;
    }
    return o;
}

// (normal @ l) under autocast: E operands, f32 accumulation, E result
template <typename E>
__device__ __forceinline__ float dot16(const float n[3], const float l16[3]) {
    const float p0 = rnd<E>(n[0]) * l16[0], p1 = rnd<E>(n[1]) * l16[1],
                p2 = rnd<E>(n[2]) * l16[2];
    return rnd<E>((p0 + p1) + p2);
}

struct Shade {
    float d16, lam16;
};

template <typename E>
__device__ __forceinline__ Shade lambert(const float n[3], const float l16[3], float ratio,
                                         float omr) {
    Shade s;
    s.d16 = dot16<E>(n, l16);
    const float c16 = s.d16 > 0.0f ? s.d16 : 0.0f;     // clamp(min=0)
    s.lam16 = rnd<E>(ratio + rnd<E>(c16 * omr));       // ratio + (1 - ratio) * c
    return s;
}

}  // namespace shd
}  // namespace dfhip
