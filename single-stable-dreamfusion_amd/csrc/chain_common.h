// The row-per-ray compositing chains (one ray per 16-lane row of a wave),
// shared by the compositing kernels (raymarching.hip) and the fused per-ray
// chain (head.hip: k_ray_chain), so both run the same code.
//
// Each lane loads one sample of the ray's 16-sample window (coalesced),
// computes its alpha, and the row then runs the reference's serial chain (T,
// the colour / weight / depth sums) over the window, each step reading sample
// j's values with a DPP row broadcast (row_newbcast:j) that the compiler folds
// into the consuming VALU instruction.  One VALU instruction thus advances
// four rays, where a whole-wave chain (readlane per value) spends it on one.
// Bit-identical to the one-thread-per-ray loop (same f32 operations, same
// order, same break).
//
// The chain is branch-free inside a window: the reference's
// `if (T < T_thresh) break` becomes a row-uniform `alive` flag that zeroes the
// weight of every later sample (fmaf(0, c, x) == x and x + 0 == x, so the sums
// are unchanged), and lanes past the window's count hold alpha 0, 1 - alpha 1,
// zero colour and delta (no-ops).  Only the window loop branches (per row).
#pragma once

#include "common.h"

namespace dfhip {
namespace rm {

// Colour-gradient store.  f32 compositing of f16 colours: the f32 product is
// rounded to f16 once, as the reference's autograd cast of its f32 gradient
// does.  f32_rounded keeps the backend from fusing product and conversion into
// one v_fma_mix, which rounds the exact product once and can differ in the
// last f16 bit.
template <typename scalar_t, typename rgb_t, typename acc_t>
__device__ __forceinline__ rgb_t grad_cast(acc_t v) { return (rgb_t)v; }
template <>
__device__ __forceinline__ half_t grad_cast<float, half_t, float>(float v) {
    return (half_t)f32_rounded(v);
}
template <>
__device__ __forceinline__ bf16_t grad_cast<float, bf16_t, float>(float v) {
    return (bf16_t)f32_rounded(v);
}

template <int J>
__device__ __forceinline__ float row_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x150 + J, 0xF, 0xF, true));
}

template <typename rgb_t>
__device__ __forceinline__ void load_rgb3(const rgb_t *c, float &r, float &g, float &b) {
    r = to_f(c[0]);
    g = to_f(c[1]);
    b = to_f(c[2]);
}

struct FwdChain {
    float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f, ws = 0.0f, t = 0.0f, d = 0.0f;
    bool alive = true;
    template <int J>
    __device__ __forceinline__ void step(float a, float om, float cr, float cg, float cb,
                                         float dl, float T_thresh) {
        // the product outside the select: a broadcast (a convergent operation)
        // in one arm would make the select a branch per step
        const float aT = row_bcast<J>(a) * T;
        const float w = alive ? aT : 0.0f;
        r = fmaf(w, row_bcast<J>(cr), r);
        g = fmaf(w, row_bcast<J>(cg), g);
        b = fmaf(w, row_bcast<J>(cb), b);
        t += row_bcast<J>(dl);
        d = fmaf(w, t, d);
        ws += w;
        T *= row_bcast<J>(om);
        alive = alive && !(T < T_thresh);
    }
};

// Backward chain: lane l of the row captures the state after sample l of the
// window (weight, T, colour sums) and whether the reference loop reached it.
struct BwdChain {
    float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f;
    bool alive = true;
    float wl, Tl, rl, gl, bl;
    bool taken;
    template <int J>
    __device__ __forceinline__ void step(int lane, float a, float om, float cr, float cg,
                                         float cb, float T_thresh) {
        const float w = row_bcast<J>(a) * T;
        r = fmaf(w, row_bcast<J>(cr), r);
        g = fmaf(w, row_bcast<J>(cg), g);
        b = fmaf(w, row_bcast<J>(cb), b);
        T *= row_bcast<J>(om);
        const bool mine = lane == J;
        wl = mine ? w : wl;
        Tl = mine ? T : Tl;
        rl = mine ? r : rl;
        gl = mine ? g : gl;
        bl = mine ? b : bl;
        taken = mine ? alive : taken;
        alive = alive && !(T < T_thresh);
    }
};

}  // namespace rm
}  // namespace dfhip
