// Device building blocks of the fused vanilla field (csrc/resmlp.hip): the
// degree-6 frequency encoding, the residual MLP 39 -> 128 x4 -> 4 of
// nerf/network.py (four ResBlocks: Linear -> LayerNorm -> + skip -> SiLU, then
// Linear(128, 4)) on v_mfma_f32_16x16x32_f16, and its LDS weight images.
// Operand maps, the transposed-layer scheme and the LDS stride reasoning are
// those of field_common.h / fieldmlp.hip: the sample sits on the lane column
// c = lane & 15, accumulator tile t, register r of lane group h = lane >> 4
// is neuron 16 t + 4 h + r, and a layer's f16 tiles are the next layer's B
// operand in the permuted k order a_perm reads the weights in.
#pragma once

#include "field_common.h"

#include <math.h>

namespace dfhip {
namespace rs {

using fm::a_nat;
using fm::a_perm;
using fm::f4;
using fm::half4;
using fm::half8;
using fm::mfma;
using fm::u32x4;

constexpr int kEnc = 39, kEncPad = 64, kHid = 128, kOut = 4, kBlocks = 4;
constexpr int kTiles = kHid / 16;  // accumulator tiles of a hidden layer
// LDS row strides (halves), 4 * odd dwords as field_common.h's kLd64
constexpr int kLdE = 72;   // rows of 64 halves (+8)
constexpr int kLdH = 136;  // rows of 128 halves (+8): 68 dwords = 4 * 17

// Packed parameter order = sigma_net.state_dict() order (network.py ResBlock /
// MLP creation order):
//   0 net.0.dense.weight [128,39]  1 net.0.dense.bias  2 net.0.norm.weight
//   3 net.0.norm.bias  4 net.0.skip.weight [128,39]
//   5 + 4 (l - 1) + {0, 1, 2, 3}: net.l.{dense.weight [128,128], dense.bias,
//   norm.weight, norm.bias}, l = 1..3;  17 net.4.weight [4,128]  18 net.4.bias
constexpr int kTensors = 19;
__host__ __device__ constexpr int t_dense_w(int l) { return l == 0 ? 0 : 5 + 4 * (l - 1); }
__host__ __device__ constexpr int t_dense_b(int l) { return t_dense_w(l) + 1; }
__host__ __device__ constexpr int t_gamma(int l) { return t_dense_w(l) + 2; }
__host__ __device__ constexpr int t_beta(int l) { return t_dense_w(l) + 3; }
constexpr int kTSkip = 4, kTOutW = 17, kTOutB = 18;
__host__ __device__ constexpr int t_size(int t) {
    return (t == 0 || t == kTSkip) ? kHid * kEnc
           : t == kTOutW           ? kOut * kHid
           : t == kTOutB           ? kOut
           : (t >= 5 && (t - 5) % 4 == 0) ? kHid * kHid
                                          : kHid;
}
__host__ __device__ constexpr int t_offset(int t) {
    int o = 0;
    for (int i = 0; i < t; ++i) o += t_size(i);
    return o;
}
constexpr int kParams = t_offset(kTensors);  // 61188
static_assert(kParams == 61188, "sigma_net of network.py has 61,188 parameters");

struct Ptrs { const float *p[kTensors]; };
struct GPtrs { float *p[kTensors]; };

constexpr float kHalfPi = 3.141592653589793f / 2.0f;  // as csrc/freqencoder.hip

// ---------------------------------------------------------------- LDS images
// Forward weights as f16 (autocast's cast of the f32 parameters), biases as
// f32 of their f16 rounding, LayerNorm parameters in f32 (autocast runs
// layer_norm in f32 with the f32 parameters).
struct alignas(16) FwdW {
    half_t w0d[kHid * kLdE];        // [n][f], columns 39..63 zero
    half_t w0s[kHid * kLdE];        // skip projection, same layout
    half_t w[3][kHid * kLdH];       // layers 1..3 [n_out][n_in]
    half_t w4[16 * kLdH];           // row i = output i & 3: every lane group's
                                    // accumulator registers r = 0..3 are outputs 0..3
    float b[kBlocks][kHid], gamma[kBlocks][kHid], beta[kBlocks][kHid], b4[16];
};

__device__ inline void load_fwd_weights(FwdW &W, const Ptrs &P) {
    for (int i = threadIdx.x; i < kHid * kEncPad; i += blockDim.x) {
        const int n = i / kEncPad, f = i % kEncPad;
        W.w0d[n * kLdE + f] = f < kEnc ? (half_t)P.p[0][n * kEnc + f] : (half_t)0.0f;
        W.w0s[n * kLdE + f] = f < kEnc ? (half_t)P.p[kTSkip][n * kEnc + f] : (half_t)0.0f;
    }
    for (int l = 1; l < kBlocks; ++l) {
        const float *w = P.p[t_dense_w(l)];
        for (int i = threadIdx.x; i < kHid * kHid; i += blockDim.x)
            W.w[l - 1][(i / kHid) * kLdH + i % kHid] = (half_t)w[i];
    }
    for (int i = threadIdx.x; i < 16 * kHid; i += blockDim.x)
        W.w4[(i / kHid) * kLdH + i % kHid] = (half_t)P.p[kTOutW][((i / kHid) & 3) * kHid + i % kHid];
    for (int l = 0; l < kBlocks; ++l)
        for (int i = threadIdx.x; i < kHid; i += blockDim.x) {
            W.b[l][i] = (float)(half_t)P.p[t_dense_b(l)][i];
            W.gamma[l][i] = P.p[t_gamma(l)][i];
            W.beta[l][i] = P.p[t_beta(l)][i];
        }
    for (int i = threadIdx.x; i < 16; i += blockDim.x) W.b4[i] = (float)(half_t)P.p[kTOutB][i & 3];
}

// ---------------------------------------------------------------- pieces
// B operand of k-step s from eight f16 accumulator tiles (tiles 2 s, 2 s + 1).
__device__ __forceinline__ half8 b_tiles(const half4 (&v)[kTiles], int s) {
    return __builtin_shufflevector(v[2 * s], v[2 * s + 1], 0, 1, 2, 3, 4, 5, 6, 7);
}

// Encoding features 32 s + 8 h + j (j = 0..7) of position x as the first
// Linear's B operand: freqencoder.hip's k_freq_fwd in f32 (layout
// [x, sin(2^k x), cos(2^k x)], cos as sin(. + pi/2), full-precision sinf),
// rounded to f16; features 39..63 are the zero padding of K.
// pick(d): coordinate d of the position.
template <typename Pick>
__device__ __forceinline__ half8 enc_operand_of(Pick pick, int s, int h) {
    half8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int f = 32 * s + 8 * h + j;
        const int d = f % 3;
        const float xd = pick(d);
        float v = 0.0f;
        if (f < 3) {
            v = xd;
        } else if (f < kEnc) {
            const int col = f / 3 - 1;
            v = sinf(scalbnf(xd, col >> 1) + (float)(col & 1) * kHalfPi);
        }
        out[j] = (half_t)v;
    }
    return out;
}
__device__ __forceinline__ half8 enc_operand(const float (&x)[3], int s, int h) {
    return enc_operand_of(
        [&](int d) __attribute__((always_inline)) {
            return d == 0 ? x[0] : (d == 1 ? x[1] : x[2]);
        },
        s, h);
}
// The same of a position held in registers (no addressable array: the
// coordinate picks stay selects where the array form may turn into an indexed
// stack slot).
__device__ __forceinline__ half8 enc_operand(float x0, float x1, float x2, int s, int h) {
    return enc_operand_of(
        [=](int d) __attribute__((always_inline)) { return d == 0 ? x0 : (d == 1 ? x1 : x2); }, s,
        h);
}

// Sum over the 128 neurons of the lane's sample: the lane's own 32 values
// are summed by the caller; this adds the other three lane groups'.
__device__ __forceinline__ float groups_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// LayerNorm(128) statistics of a row in f32 (biased variance, eps 1e-5).
__device__ __forceinline__ void ln_stats(const float (&v)[kTiles][4], float &mean, float &rstd) {
    float s = 0.0f;
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += v[t][r];
    mean = groups_sum(s) * (1.0f / kHid);
    float q = 0.0f;
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) q += (v[t][r] - mean) * (v[t][r] - mean);
    const float var = groups_sum(q) * (1.0f / kHid);
    rstd = 1.0f / sqrtf(var + 1e-5f);
}

__device__ __forceinline__ float sigmoidf(float z) { return 1.0f / (1.0f + expf(-z)); }

// Per-tile state the backward's recompute hands to its gradient pass, as
// 16-byte vectors indexed [vector][lane] (each lane reads back what it
// wrote): per block the f16 dense output (4 vectors: tiles 2 v, 2 v + 1), the
// f32 pre-activation z (8 vectors: tile v) and {mean, rstd}; then the four
// f16 outputs.
constexpr int kStBlock = 13, kStOut = kBlocks * kStBlock, kStTile = kStOut + 1;

// NT 16-sample tiles through the MLP from their encodings xb[n] (the first
// Linear's B operands, enc_operand), every weight operand and LayerNorm
// parameter read from LDS once and used for all NT.  Each tile's arithmetic
// and rounding points are those of NT = 1: MFMA columns are independent.
// hout[n]: f32 of the f16-rounded outputs h[0..3] of the lane's sample of tile
// n (every lane group holds all four).  The backward's hooks serve tile 0
// (their caller runs NT = 1).  st != nullptr: store the state above (st
// already points at the tile's vector 0 of this lane).  arows != nullptr:
// store the f16 inputs of layers 1..4 (4 x 128 rows) neuron-major ([row][Mp],
// column `sample`) for the weight gradients.
template <int NT>
__device__ __forceinline__ void mlp_tiles(const FwdW &W, const half8 (&xb)[NT][2], int c, int h,
                                          float (&hout)[NT][4], u32x4 *st, half_t *arows,
                                          size_t Mp, size_t sample) {
    float a[NT][kTiles][4];  // the block's f32 output (the next block's identity)
    half4 ah[NT][kTiles];    // its f16 rounding (the next Linear's operand)
#pragma unroll
    for (int l = 0; l < kBlocks; ++l) {
        float v[NT][kTiles][4];
        half4 dh[NT][kTiles], sk[NT][kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
            // NT > 1: the operands of one accumulator tile at a time (hoisted,
            // a layer's 128 operand registers spill beside two tiles' state)
            if constexpr (NT > 1) asm volatile("" ::: "memory");
            f4 acc[NT], sacc[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                acc[n] = fm::bias4(W.b[l], 16 * t + 4 * h);
                sacc[n] = f4{0, 0, 0, 0};
            }
            if (l == 0) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const half8 wd = a_nat(W.w0d, kLdE, 16 * t + c, 32 * s, h);
                    const half8 ws = a_nat(W.w0s, kLdE, 16 * t + c, 32 * s, h);
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        acc[n] = mfma(wd, xb[n][s], acc[n]);
                        sacc[n] = mfma(ws, xb[n][s], sacc[n]);
                    }
                }
#pragma unroll
                for (int n = 0; n < NT; ++n) sk[n][t] = __builtin_convertvector(sacc[n], half4);
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const half8 w = a_perm(W.w[l - 1], kLdH, 16 * t + c, s, h);
#pragma unroll
                    for (int n = 0; n < NT; ++n) acc[n] = mfma(w, b_tiles(ah[n], s), acc[n]);
                }
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                dh[n][t] = __builtin_convertvector(acc[n], half4);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[n][t][r] = (float)dh[n][t][r];
            }
        }
        float mean[NT], rstd[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) ln_stats(v[n], mean[n], rstd[n]);
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
            if constexpr (NT > 1) asm volatile("" ::: "memory");
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                f4 z;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int nn = 16 * t + 4 * h + r;
                    const float nrm =
                        (v[n][t][r] - mean[n]) * rstd[n] * W.gamma[l][nn] + W.beta[l][nn];
                    z[r] = nrm + (l == 0 ? (float)sk[n][t][r] : a[n][t][r]);
                    a[n][t][r] = z[r] * sigmoidf(z[r]);
                }
                ah[n][t] = half4{(half_t)a[n][t][0], (half_t)a[n][t][1], (half_t)a[n][t][2],
                                 (half_t)a[n][t][3]};
                if (n == 0 && st) {
                    u32x4 zz;
                    __builtin_memcpy(&zz, &z, 16);
                    st[(size_t)(kStBlock * l + 4 + t) * 64] = zz;
                }
                if (n == 0 && arows)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        arows[(size_t)(kHid * l + 16 * t + 4 * h + r) * Mp + sample] = ah[n][t][r];
            }
        }
        if (st) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const half8 two = __builtin_shufflevector(dh[0][2 * q], dh[0][2 * q + 1], 0, 1, 2, 3,
                                                          4, 5, 6, 7);
                u32x4 dd;
                __builtin_memcpy(&dd, &two, 16);
                st[(size_t)(kStBlock * l + q) * 64] = dd;
            }
            st[(size_t)(kStBlock * l + 12) * 64] =
                u32x4{__float_as_uint(mean[0]), __float_as_uint(rstd[0]), 0u, 0u};
        }
    }
    if constexpr (NT > 1) asm volatile("" ::: "memory");
    f4 o[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) o[n] = fm::bias4(W.b4, 4 * h);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const half8 w = a_perm(W.w4, kLdH, c, s, h);
#pragma unroll
        for (int n = 0; n < NT; ++n) o[n] = mfma(w, b_tiles(ah[n], s), o[n]);
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const half4 oh = __builtin_convertvector(o[n], half4);
#pragma unroll
        for (int r = 0; r < 4; ++r) hout[n][r] = (float)oh[r];
        if (n == 0 && st) {
            uint32_t w[2];
            __builtin_memcpy(w, &oh, 8);
            st[(size_t)kStOut * 64] = u32x4{w[0], w[1], 0u, 0u};
        }
    }
}

// One 16-sample tile through the field: the encoding of x, then the MLP.
// xrows != nullptr: store the f16 encoding (64 rows) neuron-major as arows.
__device__ __forceinline__ void forward_tile(const FwdW &W, const float (&x)[3], int c, int h,
                                             float (&hout)[4], u32x4 *st, half_t *xrows,
                                             half_t *arows, size_t Mp, size_t sample) {
    half8 xb[1][2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        xb[0][s] = enc_operand(x, s, h);
        if (xrows)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                xrows[(size_t)(32 * s + 8 * h + j) * Mp + sample] = xb[0][s][j];
    }
    mlp_tiles<1>(W, xb, c, h, reinterpret_cast<float (&)[1][4]>(hout), st, arows, Mp, sample);
}

// Sum over the 16 lanes of a row (the 16 samples of a tile), every lane
// receiving it: xor butterflies on DPP (quad_perm [1,0,3,2], [2,3,0,1],
// row_half_mirror, row_mirror), no LDS traffic.  Float addition commutes, so
// all 16 lanes hold the same bits.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), CTRL,
                                                                 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    v += dpp_f<0x140>(v);
    return v;
}

}  // namespace rs
}  // namespace dfhip
