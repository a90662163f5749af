// Device building blocks of the fused voxel field (csrc/voxelfield.hip): the
// DVGO backbone's coordinate map and trilinear sample in f32, its feature row
// (k0 sample, position encoding, constant view encoding) and the colour MLP
// dim0 -> 128 -> 128 -> 3 (BasicMLP, ReLU) on v_mfma_f32_16x16x32_f16.
// Operand maps and LDS strides are those of field_common.h / resmlp_common.h:
// the sample sits on the lane column c = lane & 15, accumulator tile t,
// register r of lane group h = lane >> 4 is neuron 16 t + 4 h + r, and a
// layer's f16 tiles are the next layer's B operand in the permuted k order
// a_perm reads the weights in.  The first Linear takes its B operand in
// natural k order (a_nat): lane group h, element j of k-step s is feature
// 32 s + 8 h + j of the row.
#pragma once

#include "field_common.h"

#include <math.h>

namespace dfhip {
namespace vx {

using fm::a_nat;
using fm::a_perm;
using fm::bias4;
using fm::f4;
using fm::half4;
using fm::half8;
using fm::mfma;

constexpr int kInPad = 96, kHid = 128, kOut = 3;
constexpr int kSteps0 = kInPad / 32;  // k-steps of the first Linear
constexpr int kTiles = kHid / 16;     // accumulator tiles of a hidden layer
// LDS row strides (halves), 4 * odd dwords (field_common.h)
constexpr int kLdI = 104;  // rows of 96 halves (+8): 52 dwords = 4 * 13
constexpr int kLdH = 136;  // rows of 128 halves (+8): 68 dwords = 4 * 17

// Packed parameter order = rgbnet.state_dict() order (BasicMLP, depth 3):
//   0 net.0.weight [128, dim0]  1 net.0.bias  2 net.2.0.weight [128, 128]
//   3 net.2.0.bias  4 net.3.weight [3, 128]  5 net.3.bias
constexpr int kTensors = 6;
struct Ptrs { const float *p[kTensors]; };
struct GPtrs { float *p[kTensors]; };

__host__ __device__ inline uint32_t t_size(int t, uint32_t dim0) {
    return t == 0 ? kHid * dim0 : t == 2 ? kHid * kHid : t == 4 ? kOut * kHid
           : t == 5 ? kOut : kHid;
}
__host__ __device__ inline uint32_t t_offset(int t, uint32_t dim0) {
    uint32_t o = 0;
    for (int i = 0; i < t; ++i) o += t_size(i, dim0);
    return o;
}

// The volume's geometry and the feature row's layout (by value to kernels).
struct Geom {
    float bound, inv2b, act_shift;
    float mn[3], mx[3], ext[3];  // box_min, box_max, box_max - box_min (f32)
    uint32_t n[3];               // Nx, Ny, Nz
    uint32_t C, P, vdim, dim0;   // k0 channels, position frequencies, view features
};

// ---------------------------------------------------------------- sampling
// Where a position falls in the volume.  hi / lo: the weights of the lower /
// upper corner per grid axis ((floor + 1) - g and g - floor, not clamped);
// i0 / i1: their indices clamped to [0, N - 1]; u: the position normalised to
// the box (the position encoding's input).
struct Cell {
    bool inside;
    float u[3], hi[3], lo[3];
    uint32_t i0[3], i1[3];
};

__device__ __forceinline__ Cell locate(const Geom &G, const float (&x)[3]) {
    float s[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) s[d] = (x[d] + G.bound) * G.inv2b;
    const float sw[3] = {s[0], s[2], s[1]};  // grid y is world z
    Cell c;
    c.inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float sc = (sw[a] - 0.5f) * 1.25f + 0.5f;
        const float p = sc * G.ext[a] + G.mn[a];
        if (!(p <= G.mx[a] && G.mn[a] <= p)) c.inside = false;
        const float u = (p - G.mn[a]) / G.ext[a];
        c.u[a] = u;
        float g = ((u * 2.0f - 1.0f) + 1.0f) * 0.5f * (float)(G.n[a] - 1u);
        // inside rows have 0 <= g <= N - 1; the others are never sampled
        if (!(g >= 0.0f && g <= (float)(G.n[a] - 1u))) g = 0.0f;
        const float f = floorf(g);
        c.hi[a] = (f + 1.0f) - g;
        c.lo[a] = g - f;
        const uint32_t i = (uint32_t)f, last = G.n[a] - 1u;
        c.i0[a] = i < last ? i : last;
        c.i1[a] = i + 1u < last ? i + 1u : last;
    }
    return c;
}

// The eight corners in the reference's summation order (grid z fastest, then
// y, then x: tnw, tne, tsw, tse, bnw, bne, bsw, bse), weights as its products
// (z * y) * x, voxel indices ((ix Ny) + iy) Nz + iz.
struct Corners {
    float w[8];
    uint32_t v[8];
};

__device__ __forceinline__ Corners corners(const Geom &G, const Cell &c) {
    Corners q;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool z1 = k & 1, y1 = k & 2, x1 = k & 4;
        q.w[k] = (z1 ? c.lo[2] : c.hi[2]) * (y1 ? c.lo[1] : c.hi[1]) * (x1 ? c.lo[0] : c.hi[0]);
        q.v[k] = ((x1 ? c.i1[0] : c.i0[0]) * G.n[1] + (y1 ? c.i1[1] : c.i0[1])) * G.n[2] +
                 (z1 ? c.i1[2] : c.i0[2]);
    }
    return q;
}

// Channel ch of a channel-last volume with `stride` channels, f32.
__device__ __forceinline__ float trilinear(const Corners &q, const float *__restrict__ vol,
                                           uint32_t stride, uint32_t ch) {
    const float *p = vol + ch;
    float out = p[(size_t)q.v[0] * stride] * q.w[0];
    out = out + p[(size_t)q.v[1] * stride] * q.w[1];
    out = out + p[(size_t)q.v[2] * stride] * q.w[2];
    out = out + p[(size_t)q.v[3] * stride] * q.w[3];
    out = out + p[(size_t)q.v[4] * stride] * q.w[4];
    out = out + p[(size_t)q.v[5] * stride] * q.w[5];
    out = out + p[(size_t)q.v[6] * stride] * q.w[6];
    out = out + p[(size_t)q.v[7] * stride] * q.w[7];
    return out;
}

__device__ __forceinline__ float sigmoidf(float z) { return 1.0f / (1.0f + expf(-z)); }

// 10 * softplus(raw + act_shift) (softplus with beta 1, threshold 20), f32.
__device__ __forceinline__ float activate(float raw, float act_shift) {
    const float y = raw + act_shift;
    return (y > 20.0f ? y : log1pf(expf(y))) * 10.0f;
}

// raw (the trilinear density sample, trilinear()'s sum) and n = -d sigma / d x
// in world axes, not normalised, of a position inside the box: the closed
// form of k_voxel_normal, from the cell's eight corner values.
__device__ __forceinline__ void density_normal(const Geom &G, const Cell &c, const Corners &q,
                                               const float *__restrict__ density, float &raw,
                                               float (&n)[3]) {
    float v[8];  // corner k: bit 0 = z + 1, bit 1 = y + 1, bit 2 = x + 1
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = density[q.v[k]];
    raw = v[0] * q.w[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) raw = raw + v[k] * q.w[k];
    // d raw / d g per grid axis: the weights' derivatives are -1 / +1 on
    // the lower / upper corner (equal clamped corners cancel exactly)
    float dg[3];
    dg[2] = c.hi[1] * c.hi[0] * (v[1] - v[0]) + c.lo[1] * c.hi[0] * (v[3] - v[2]) +
            c.hi[1] * c.lo[0] * (v[5] - v[4]) + c.lo[1] * c.lo[0] * (v[7] - v[6]);
    dg[1] = c.hi[2] * c.hi[0] * (v[2] - v[0]) + c.lo[2] * c.hi[0] * (v[3] - v[1]) +
            c.hi[2] * c.lo[0] * (v[6] - v[4]) + c.lo[2] * c.lo[0] * (v[7] - v[5]);
    dg[0] = c.hi[2] * c.hi[1] * (v[4] - v[0]) + c.lo[2] * c.hi[1] * (v[5] - v[1]) +
            c.hi[2] * c.lo[1] * (v[6] - v[2]) + c.lo[2] * c.lo[1] * (v[7] - v[3]);
    // softplus backward (beta 1, threshold 20) of the gradient 10
    const float y = raw + G.act_shift, z = expf(y);
    const float ds = y > 20.0f ? 10.0f : 10.0f * z / (z + 1.0f);
    float dp[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float g = ds * dg[a];
        g = g * (float)(G.n[a] - 1u) * 0.5f * 2.0f;
        g = g / G.ext[a] * G.ext[a];
        dp[a] = g * 1.25f * G.inv2b;
    }
    n[0] = -dp[0], n[1] = -dp[2], n[2] = -dp[1];  // grid y is world z
}

// NeRFNetwork._unit: n / sqrt(clamp(|n|^2, 1e-20)), NaN -> 0 (f32).
__device__ __forceinline__ void unit_normal(float (&n)[3]) {
    const float ss = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const float r = sqrtf(fmaxf(ss, 1e-20f));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = n[a] / r;
        n[a] = q != q ? 0.0f : q;
    }
}

// Feature f of PE(u) = [u, sin(u_d 2^i), cos(u_d 2^i)] (d major), f32.
__device__ __forceinline__ float pos_feature(const Geom &G, float u0, float u1, float u2,
                                             uint32_t f) {
    if (f < 3u) return f == 0 ? u0 : (f == 1 ? u1 : u2);
    f -= 3u;
    const bool is_cos = f >= 3u * G.P;
    if (is_cos) f -= 3u * G.P;
    const uint32_t d = f / G.P, i = f - d * G.P;
    const float arg = scalbnf(d == 0 ? u0 : (d == 1 ? u1 : u2), (int)i);
    return is_cos ? cosf(arg) : sinf(arg);
}

// The first Linear's B operand of the lane's sample: the row cat(k0 sample,
// PE(u), view) rounded to f16 (autocast's cast of the f32 row), zeros past
// dim0 and for rows that are not `live`.  The four lane groups of a sample
// write every fourth feature of its row into the wave's LDS image `buf`
// ([16][kLdI] halves), then each reads its 8 features per k-step.
__device__ __forceinline__ void feature_operands(const Geom &G, const Cell &c, bool live,
                                                 const float *__restrict__ k0,
                                                 const float *__restrict__ view, int col, int h,
                                                 half_t *buf, half8 (&xb)[kSteps0]) {
    half_t *row = buf + col * kLdI;
    const uint32_t pdim = G.P ? 3u + 6u * G.P : 0u;
    uint32_t pad = h;  // first feature this lane zero-fills
    if (live) {
        const Corners q = corners(G, c);
        // as registers: a select among c.u[] by a runtime index would turn
        // the whole Cell into an indexed private array
        const float u0 = f32_rounded(c.u[0]), u1 = f32_rounded(c.u[1]), u2 = f32_rounded(c.u[2]);
#pragma unroll 1
        for (uint32_t ch = h; ch < G.C; ch += 4u) row[ch] = (half_t)trilinear(q, k0, G.C, ch);
#pragma unroll 1
        for (uint32_t f = h; f < pdim; f += 4u) row[G.C + f] = (half_t)pos_feature(G, u0, u1, u2, f);
#pragma unroll 1
        for (uint32_t f = h; f < G.vdim; f += 4u) row[G.C + pdim + f] = (half_t)view[f];
        pad += G.dim0;
    }
#pragma unroll 1
    for (uint32_t f = pad; f < (uint32_t)kInPad; f += 4u) row[f] = (half_t)0.0f;
    fm::wave_lds_sync();
#pragma unroll
    for (int s = 0; s < kSteps0; ++s)
        xb[s] = *reinterpret_cast<const half8 *>(row + 32 * s + 8 * h);
    fm::wave_lds_sync();  // the next tile overwrites the image
}

// ---------------------------------------------------------------- LDS images
// Weights as f16 (autocast's cast of the f32 parameters), biases as f32 of
// their f16 rounding.
struct alignas(16) FwdW {
    half_t w0[kHid * kLdI];  // [n][f], columns dim0..95 zero
    half_t w1[kHid * kLdH];  // [n_out][n_in]
    half_t w2[16 * kLdH];    // row i = output i & 3 (row 3 of every four zero): every lane
                             // group's accumulator registers r = 0..2 are outputs 0..2
    float b0[kHid], b1[kHid], b2[16];
};

__device__ inline void load_fwd_weights(FwdW &W, const Ptrs &P, uint32_t dim0) {
    for (int i = threadIdx.x; i < kHid * kInPad; i += blockDim.x) {
        const uint32_t n = i / kInPad, f = i % kInPad;
        W.w0[n * kLdI + f] = f < dim0 ? (half_t)P.p[0][n * dim0 + f] : (half_t)0.0f;
    }
    for (int i = threadIdx.x; i < kHid * kHid; i += blockDim.x)
        W.w1[(i / kHid) * kLdH + i % kHid] = (half_t)P.p[2][i];
    for (int i = threadIdx.x; i < 16 * kHid; i += blockDim.x) {
        const int o = (i / kHid) & 3;
        W.w2[(i / kHid) * kLdH + i % kHid] =
            o < kOut ? (half_t)P.p[4][o * kHid + i % kHid] : (half_t)0.0f;
    }
    for (int i = threadIdx.x; i < kHid; i += blockDim.x) {
        W.b0[i] = (float)(half_t)P.p[1][i];
        W.b1[i] = (float)(half_t)P.p[3][i];
    }
    for (int i = threadIdx.x; i < 16; i += blockDim.x)
        W.b2[i] = (i & 3) < kOut ? (float)(half_t)P.p[5][i & 3] : 0.0f;
}

// B operand of k-step s from eight f16 accumulator tiles (tiles 2 s, 2 s + 1).
__device__ __forceinline__ half8 b_tiles(const half4 (&v)[kTiles], int s) {
    return __builtin_shufflevector(v[2 * s], v[2 * s + 1], 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ half4 relu_half4(f4 a) {
    // ReLU and round-to-nearest commute: this is ReLU of the f16 output
    const f4 r = {fmaxf(a[0], 0.0f), fmaxf(a[1], 0.0f), fmaxf(a[2], 0.0f), fmaxf(a[3], 0.0f)};
    return __builtin_convertvector(r, half4);
}

// One 16-sample tile through the MLP.  a1, a2: the post-ReLU f16 activations
// (neuron 16 t + 4 h + r of the lane's sample); out: f32 of the f16 outputs
// 0..2 of the lane's sample (every lane group holds all three).
template <typename WT>
__device__ __forceinline__ void mlp_tile(const WT &W, const half8 (&xb)[kSteps0], int c, int h,
                                         half4 (&a1)[kTiles], half4 (&a2)[kTiles],
                                         float (&out)[kOut]) {
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
        f4 acc = bias4(W.b0, 16 * t + 4 * h);
#pragma unroll
        for (int s = 0; s < kSteps0; ++s)
            acc = mfma(a_nat(W.w0, kLdI, 16 * t + c, 32 * s, h), xb[s], acc);
        a1[t] = relu_half4(acc);
    }
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
        f4 acc = bias4(W.b1, 16 * t + 4 * h);
#pragma unroll
        for (int s = 0; s < 4; ++s)
            acc = mfma(a_perm(W.w1, kLdH, 16 * t + c, s, h), b_tiles(a1, s), acc);
        a2[t] = relu_half4(acc);
    }
    f4 o = bias4(W.b2, 4 * h);
#pragma unroll
    for (int s = 0; s < 4; ++s) o = mfma(a_perm(W.w2, kLdH, c, s, h), b_tiles(a2, s), o);
    const half4 oh = __builtin_convertvector(o, half4);
#pragma unroll
    for (int r = 0; r < kOut; ++r) out[r] = (float)oh[r];
}

// ---------------------------------------------------------------- host side
// Argument checks shared by the entries of voxelfield.hip and voxelrender.hip.
inline bool geometry(const char *name, uint32_t Nx, uint32_t Ny, uint32_t Nz, uint32_t C,
                     uint32_t pos_freqs, uint32_t view_dim, const float *box, float bound,
                     float act_shift, bool colour, Geom &G) {
    if (!box) {
        set_error("%s: box is null", name);
        return false;
    }
    if (!Nx || !Ny || !Nz || (uint64_t)Nx * Ny * Nz > 0x7fffffffull) {
        set_error("%s: the volume must have 1 .. 2^31 - 1 voxels, got %u x %u x %u", name, Nx, Ny,
                  Nz);
        return false;
    }
    if (!(bound > 0.0f)) {
        set_error("%s: bound must be positive", name);
        return false;
    }
    G.bound = bound, G.inv2b = 1.0f / (2.0f * bound), G.act_shift = act_shift;
    for (int a = 0; a < 3; ++a) {
        G.mn[a] = box[a], G.mx[a] = box[3 + a], G.ext[a] = box[3 + a] - box[a];
        if (!(G.ext[a] > 0.0f)) {
            set_error("%s: box_max must exceed box_min on every axis", name);
            return false;
        }
    }
    G.n[0] = Nx, G.n[1] = Ny, G.n[2] = Nz;
    G.C = C, G.P = pos_freqs, G.vdim = view_dim;
    G.dim0 = C + (pos_freqs ? 3u + 6u * pos_freqs : 0u) + view_dim;
    if (colour && (C == 0 || pos_freqs > 15u || view_dim > (uint32_t)kInPad ||
                   G.dim0 > (uint32_t)kInPad)) {
        set_error("%s: the feature row must have 1 .. %d entries with C >= 1 (C %u, pos_freqs %u, "
                  "view_dim %u)", name, kInPad, C, pos_freqs, view_dim);
        return false;
    }
    return true;
}

inline bool gather(const char *name, const float *const *params, Ptrs &P) {
    if (!params) {
        set_error("%s: null parameter list", name);
        return false;
    }
    for (int t = 0; t < kTensors; ++t) {
        if (!params[t]) {
            set_error("%s: parameter %d is null", name, t);
            return false;
        }
        P.p[t] = params[t];
    }
    return true;
}

}  // namespace vx
}  // namespace dfhip
