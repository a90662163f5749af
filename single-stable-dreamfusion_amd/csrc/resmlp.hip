// Fused vanilla field on MFMA (gfx950): frequency encoding (degree 6) ->
// residual MLP 39 -> 128 x4 -> 4 (Linear -> LayerNorm -> + skip -> SiLU four
// times, then Linear) -> trunc_exp density with the Gaussian blob and sigmoid
// albedo; forward, and backward with the f32 parameter gradients and the
// input gradient.
//
// Behavioural spec: nerf/network.py:13-67 (ResBlock, MLP), :96-115 (gaussian,
// common_forward), :135-146 (normal), activation.py (trunc_exp), run under
// torch.autocast(fp16): every Linear is an f16 GEMM with f32 accumulation and
// an f16 output, layer_norm runs in f32 on the f16 dense output, the residual
// add and SiLU are f32, sigma is f32 and albedo f16.
//
// Forward: one launch.  A workgroup of 8 waves keeps all f16 weights in LDS
// (142 KiB of padded rows + 6 KiB of f32 biases and LayerNorm parameters, one
// workgroup per CU); a wave takes 16 samples through every layer in registers
// (resmlp_common.h forward_tile).  The LayerNorm reductions are 32 in-lane
// adds and two cross-lane-group exchanges.
//
// Backward: the weights and their transposed copies do not fit LDS together,
// so the one C call runs four launches per chunk of up to 65536 samples:
//   1. the forward again, storing per tile what the gradient pass needs (the
//      f16 dense outputs, the f32 pre-activations, the LayerNorm statistics)
//      and, neuron-major, the f16 inputs of every Linear;
//   2. the gradient pass with the transposed weights in LDS: heads, then per
//      block SiLU', LayerNorm backward, W^T products; it stores the f16 output
//      gradients of every Linear neuron-major, accumulates the LayerNorm
//      parameter gradients per wave (DPP row sums, single-writer LDS adds) and
//      runs the encoder's chain rule for the input gradient;
//   3. the weight gradients as MFMA products over the sample axis, split over
//      the samples into per-split partials;
//   4. a fixed-order sum of the partials into the f32 gradients.
// No float atomics anywhere: two runs give the same bits.
#include "resmlp_common.h"

namespace dfhip {
namespace rs {

constexpr int kFwdWaves = 8;
constexpr uint32_t kChunk = 65536;  // samples per backward chunk
constexpr uint32_t kSplits = 64;    // sample-axis splits of the weight-gradient products
constexpr uint32_t kLnParts = 256;  // upper bound of the gradient pass's workgroups

// rows of the neuron-major f16 operands of the weight gradients
constexpr int kXRows = kEncPad, kARows = kBlocks * kHid;
// gradient side: GD_l at rows 128 l (l = 0..3), the skip's at 512, the
// outputs' (4 rows) at 640
constexpr int kGSkip = kBlocks * kHid, kGOut = kGSkip + kHid, kGRows = kGOut + 16;

// ------------------------------------------------------------------ forward
template <bool SAVE>
__global__ __launch_bounds__(64 * kFwdWaves) void k_resmlp_fwd(
    const float *__restrict__ xyz, Ptrs P, float *__restrict__ sigma,
    half_t *__restrict__ albedo, uint32_t M, uint32_t tiles, u32x4 *__restrict__ state,
    half_t *__restrict__ xrows, half_t *__restrict__ arows, uint32_t Mp) {
    __shared__ FwdW W;
    load_fwd_weights(W, P);
    __syncthreads();
    const int lane = threadIdx.x & 63, c = lane & 15, h = lane >> 4;
    const uint32_t waves = gridDim.x * kFwdWaves;
    for (uint32_t tile = blockIdx.x * kFwdWaves + (threadIdx.x >> 6); tile < tiles;
         tile += waves) {
        // weights and LayerNorm parameters are re-read from LDS every tile
        // (hoisted out of the loop they spill; fieldmlp.hip's idiom)
        asm volatile("" ::: "memory");
        const uint32_t sample = tile * 16 + c;
        const bool valid = sample < M;
        float x[3] = {0.0f, 0.0f, 0.0f};
        if (valid)
#pragma unroll
            for (int d = 0; d < 3; ++d) x[d] = xyz[(size_t)sample * 3 + d];
        float ho[4];
        forward_tile(W, x, c, h, ho, SAVE ? state + (size_t)tile * kStTile * 64 + lane : nullptr,
                     SAVE ? xrows : nullptr, SAVE ? arows : nullptr, Mp, sample);
        if (SAVE || !valid) continue;
        // lane group 0 writes the density, groups 1..3 albedo channel h - 1
        if (h == 0) {
            sigma[sample] = expf(ho[0] + fm::gaussian(x));
        } else {
            const float v = h == 1 ? ho[1] : (h == 2 ? ho[2] : ho[3]);
            albedo[(size_t)sample * 3 + h - 1] = (half_t)sigmoidf(v);
        }
    }
}

// ------------------------------------------------------------------ device counts
// The device-count entries take their row count from the device: buffers hold
// `cap` rows, *m_dev is the live count, so the launch shapes depend on the
// capacity only and the launches capture into a graph (voxelfield.hip's
// scheme).  Rows at or past the live count are neither read nor written.
__device__ __forceinline__ uint32_t live_rows(const int32_t *m_dev, uint32_t cap) {
    const int32_t m = *m_dev;
    return m < 0 ? 0u : ((uint32_t)m < cap ? (uint32_t)m : cap);
}

// Rows the backward sums over: the live count rounded up to `align` (the
// march's slice), at most the capacity.
__device__ __forceinline__ uint32_t effective_rows(uint32_t m, uint32_t cap, uint32_t align) {
    const uint64_t a = ((uint64_t)m + align - 1u) / align * align;
    return a < (uint64_t)cap ? (uint32_t)a : cap;
}

__host__ __device__ inline uint32_t padded(uint32_t m) { return ceil_div(m, 32u) * 32u; }

// Workgroups the host-count backward gives the gradient pass of a chunk of
// `tiles` tiles (persistent_blocks(tiles, 8, kLnParts) on a device of `cus`
// compute units): the number of LayerNorm-parameter partials of that chunk.
__host__ __device__ inline uint32_t act_blocks(uint32_t tiles, uint32_t cus) {
    const uint32_t want = ceil_div(tiles, 8u);
    uint32_t n = want < cus ? want : cus;
    if (n > kLnParts) n = kLnParts;
    return n ? n : 1u;
}

// Chunk `chunk` of Me effective rows of a capacity of cap rows: the padded row
// count, splits and gradient-pass workgroups the host loop gives it, and the
// row stride of its neuron-major images (the capacity's share of the chunk).
struct Chunk {
    uint32_t mp, splits, nblk, ld;
};
__device__ __forceinline__ Chunk chunk_of(uint32_t chunk, uint32_t Me, uint32_t cap,
                                          uint32_t cus) {
    const uint32_t m0 = chunk * kChunk, left = cap - m0;
    Chunk k;
    k.mp = padded(Me - m0 < kChunk ? Me - m0 : kChunk);
    k.splits = k.mp / 32u < kSplits ? k.mp / 32u : kSplits;
    k.nblk = act_blocks(k.mp / 16u, cus);
    k.ld = padded(left < kChunk ? left : kChunk);
    return k;
}

// The neuron-major images of the device-count backward: chunk c's three images
// (xrows, arows, grows, each of row stride Chunk::ld) start at rows + c *
// kChunk * kRowsAll halves.
constexpr int kRowsAll = kXRows + kARows + kGRows;

// Forward with the device count.  SAVE false: sigma / albedo of rows [0, m).
// SAVE true: the backward's saving forward over the tiles of the effective
// rows (tile t of the capacity is tile t % 4096 of chunk t / 4096; rows at or
// past the live count run as position 0, the host-count entry's padding).
template <bool SAVE>
__global__ __launch_bounds__(64 * kFwdWaves) void k_resmlp_fwd_dev(
    const float *__restrict__ xyz, Ptrs P, float *__restrict__ sigma,
    half_t *__restrict__ albedo, uint32_t cap, const int32_t *__restrict__ m_dev,
    uint32_t align, u32x4 *__restrict__ state, half_t *__restrict__ rows) {
    __shared__ FwdW W;
    load_fwd_weights(W, P);
    __syncthreads();
    const int lane = threadIdx.x & 63, c = lane & 15, h = lane >> 4;
    const uint32_t M = live_rows(m_dev, cap);
    const uint32_t Me = SAVE ? effective_rows(M, cap, align) : M;
    const uint32_t tiles = SAVE ? padded(Me) / 16u : ceil_div(M, 16u);
    const uint32_t waves = gridDim.x * kFwdWaves;
    for (uint32_t tile = blockIdx.x * kFwdWaves + (threadIdx.x >> 6); tile < tiles;
         tile += waves) {
        asm volatile("" ::: "memory");  // as k_resmlp_fwd
        const uint32_t sample = tile * 16 + c;
        const bool valid = sample < M;
        float x[3] = {0.0f, 0.0f, 0.0f};
        if (valid)
#pragma unroll
            for (int d = 0; d < 3; ++d) x[d] = xyz[(size_t)sample * 3 + d];
        float ho[4];
        if constexpr (SAVE) {
            const uint32_t chunk = tile / (kChunk / 16u);
            const uint32_t left = cap - chunk * kChunk;
            const size_t ld = padded(left < kChunk ? left : kChunk);
            half_t *img = rows + (size_t)chunk * kChunk * kRowsAll;
            forward_tile(W, x, c, h, ho, state + (size_t)tile * kStTile * 64 + lane, img,
                         img + (size_t)kXRows * ld, ld, sample - chunk * kChunk);
        } else {
            forward_tile(W, x, c, h, ho, nullptr, nullptr, nullptr, 0, sample);
            if (!valid) continue;
            if (h == 0) {
                sigma[sample] = expf(ho[0] + fm::gaussian(x));
            } else {
                const float v = h == 1 ? ho[1] : (h == 2 ? ho[2] : ho[3]);
                albedo[(size_t)sample * 3 + h - 1] = (half_t)sigmoidf(v);
            }
        }
    }
}

// ------------------------------------------------------------------ gradient pass
// Transposed weights [n_in][n_out] of layers 1..3, and with DX of layer 0's
// dense and skip projections ([64][128], rows 39..63 zero); the output layer
// as f32 of its f16 weights (4 x 128: its product is four FMAs per neuron).
template <bool DX>
struct alignas(16) BwdW {
    half_t wt[3][kHid * kLdH];
    half_t w0t[DX ? 2 * kEncPad * kLdH : 8];
    float w4[kOut][kHid], gamma[kBlocks][kHid];
};

template <bool DX>
__device__ inline void load_bwd_weights(BwdW<DX> &W, const Ptrs &P) {
    for (int l = 1; l < kBlocks; ++l) {
        const float *w = P.p[t_dense_w(l)];
        for (int i = threadIdx.x; i < kHid * kHid; i += blockDim.x)
            W.wt[l - 1][(i % kHid) * kLdH + i / kHid] = (half_t)w[i];  // w[n_out][n_in]
    }
    if constexpr (DX)
        for (int i = threadIdx.x; i < kEncPad * kHid; i += blockDim.x) {
            const int f = i / kHid, n = i % kHid;
            W.w0t[f * kLdH + n] = f < kEnc ? (half_t)P.p[0][n * kEnc + f] : (half_t)0.0f;
            W.w0t[(kEncPad + f) * kLdH + n] =
                f < kEnc ? (half_t)P.p[kTSkip][n * kEnc + f] : (half_t)0.0f;
        }
    for (int i = threadIdx.x; i < kOut * kHid; i += blockDim.x)
        W.w4[i / kHid][i % kHid] = (float)(half_t)P.p[kTOutW][i];
    for (int l = 0; l < kBlocks; ++l)
        for (int i = threadIdx.x; i < kHid; i += blockDim.x) W.gamma[l][i] = P.p[t_gamma(l)][i];
}

// DX: write the input gradient dx [M, 3].  WG: store the Linear output
// gradients for the weight-gradient products (grows, neuron-major [row][Mp])
// and this workgroup's LayerNorm parameter gradients (lnpart [gridDim.x]
// [block][gamma | beta][128]).  ga_t: grad_albedo's type.
// Device count (DEV; parameter gradients only, DX false): the host-count entry
// gives chunk k of the effective rows Chunk::nblk workgroups, workgroup b's
// wave w the tiles 8 b + w, + 8 nblk, ... of the chunk, and one LayerNorm
// partial per workgroup.  A workgroup of the DEV launch plays workgroup b =
// blockIdx.x (+ gridDim.x, ...) of every live chunk in turn: the same tiles in
// the same order into freshly zeroed sums, the same wave-ordered partial, at
// lnpart [chunk][kLnParts][block][gamma | beta][128].  The grid is the
// capacity's (a full chunk's workgroups from 32768 rows on), so a workgroup
// takes at most one role per chunk, as the host-count launch gives it.  The
// per-chunk arguments (xyz .. Mp) are then unused: they come from `dev`.
template <bool DEV>
struct DevCount {};
template <>
struct DevCount<true> {
    const float *xyz, *grad_sigma;
    const void *grad_albedo;
    const u32x4 *state;
    half_t *rows;
    const int32_t *m_dev;
    uint32_t cap, align, cus;
};
template <bool DEV>
struct DevRole {};
template <>
struct DevRole<true> {
    uint32_t live, Me, chunk, b;
    bool started;
    Chunk k;
    __device__ __forceinline__ void begin(const DevCount<true> &d) {
        live = live_rows(d.m_dev, d.cap), Me = effective_rows(live, d.cap, d.align);
        chunk = 0, b = 0, started = false;
    }
    // workgroup-uniform: the roles b = block, block + grid, ... of chunk 0, then chunk 1, ...
    __device__ __forceinline__ bool next(const DevCount<true> &d, uint32_t block, uint32_t grid) {
        b = started ? b + grid : block;
        started = true;
        for (; chunk * kChunk < Me; ++chunk, b = block) {
            k = chunk_of(chunk, Me, d.cap, d.cus);
            if (b < k.nblk) return true;
        }
        return false;
    }
};

template <bool DX, bool WG, int WAVES, typename ga_t, bool DEV = false>
__global__ __launch_bounds__(64 * WAVES) void k_resmlp_bwd_act(
    const float *__restrict__ xyz, Ptrs P, const float *__restrict__ grad_sigma,
    const ga_t *__restrict__ grad_albedo, uint32_t M, uint32_t tiles,
    const u32x4 *__restrict__ state, half_t *__restrict__ grows, uint32_t Mp,
    float *__restrict__ lnpart, float *__restrict__ dx, DevCount<DEV> dev) {
    __shared__ BwdW<DX> W;
    __shared__ __attribute__((aligned(16))) float lnacc[WG ? WAVES : 1][kBlocks][2][kHid];
    load_bwd_weights(W, P);
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63, c = lane & 15, h = lane >> 4;
    // the role of this workgroup: its first tile, the tile stride, its partial
    uint32_t first = blockIdx.x * WAVES + wave, waves = gridDim.x * WAVES;
    float *lnout = lnpart + (size_t)blockIdx.x * (kBlocks * 2 * kHid);
    DevRole<DEV> role;
    if constexpr (DEV) role.begin(dev);
    do {  // once (host count), or once per role (DEV); the body keeps its indentation
    if constexpr (DEV) {
        // the next (chunk, workgroup) role of the host-count launches
        if (!role.next(dev, blockIdx.x, gridDim.x)) break;
        const uint32_t m0 = role.chunk * kChunk;
        xyz = dev.xyz + (size_t)m0 * 3, grad_sigma = dev.grad_sigma + m0;
        grad_albedo = (const ga_t *)dev.grad_albedo + (size_t)m0 * 3;
        M = role.live > m0 ? (role.live - m0 < kChunk ? role.live - m0 : kChunk) : 0u;
        tiles = role.k.mp / 16u, Mp = role.k.ld;
        state = dev.state + (size_t)(m0 / 16u) * kStTile * 64;
        grows = dev.rows + (size_t)role.chunk * kChunk * kRowsAll +
                (size_t)(kXRows + kARows) * role.k.ld;
        first = role.b * WAVES + wave, waves = role.k.nblk * WAVES;
        lnout = lnpart + ((size_t)role.chunk * kLnParts + role.b) * (kBlocks * 2 * kHid);
        __syncthreads();  // the last role's partial is read (first: nothing to wait for)
    }
    if (WG)
        for (int i = threadIdx.x; i < WAVES * kBlocks * 2 * kHid; i += blockDim.x)
            (&lnacc[0][0][0][0])[i] = 0.0f;
    __syncthreads();
    for (uint32_t tile = first; tile < tiles; tile += waves) {
        asm volatile("" ::: "memory");  // no hoisting of the LDS operands (see k_resmlp_fwd)
        const uint32_t sample = tile * 16 + c;
        const bool valid = sample < M;
        const u32x4 *st = state + (size_t)tile * kStTile * 64 + lane;
        float x[3] = {0.0f, 0.0f, 0.0f}, gs = 0.0f, gal[3] = {0.0f, 0.0f, 0.0f};
        if (valid) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                x[d] = xyz[(size_t)sample * 3 + d];
                // the gradient of the f16 albedo arrives in f16
                gal[d] = (float)(half_t)(float)grad_albedo[(size_t)sample * 3 + d];
            }
            gs = grad_sigma[sample];
        }
        // ---- heads (network.py:112-113, activation.py): every lane group
        // computes all four output gradients of its sample
        const u32x4 ov = st[(size_t)kStOut * 64];
        half4 oh;
        {
            const uint32_t w[2] = {ov[0], ov[1]};
            __builtin_memcpy(&oh, w, 8);
        }
        const float gauss = fm::gaussian(x);
        const float y = (float)oh[0] + gauss;
        // trunc_exp backward: g * exp(clamp(y, -15, 15)), f32
        const float gpre = gs * expf(fminf(fmaxf(y, -15.0f), 15.0f));
        half_t go[4];
        go[0] = (half_t)gpre;  // back through the f16 -> f32 promotion of h[..., 0]
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float av = (float)(half_t)sigmoidf((float)oh[k]);
            go[k] = (half_t)(gal[k - 1] * (1.0f - av) * av);  // sigmoid_backward in f16
        }
        if (WG && h == 0)
#pragma unroll
            for (int k = 0; k < 4; ++k) grows[(size_t)(kGOut + k) * Mp + sample] = go[k];
        // ---- dL/d(a_3) = go @ W4 as an f16 GEMM output, then f32
        float ga[kTiles][4];
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = 16 * t + 4 * h + r;
                float s = (float)go[0] * W.w4[0][n];
                s = fmaf((float)go[1], W.w4[1][n], s);
                s = fmaf((float)go[2], W.w4[2][n], s);
                s = fmaf((float)go[3], W.w4[3][n], s);
                ga[t][r] = (float)(half_t)s;
            }
        half4 gsk[kTiles];  // block 0: the skip projection's output gradient
#pragma unroll
        for (int l = kBlocks - 1; l >= 0; --l) {
            const u32x4 sv = st[(size_t)(kStBlock * l + 12) * 64];
            const float mean = __uint_as_float(sv[0]), rstd = __uint_as_float(sv[1]);
            float gy[kTiles][4], xh[kTiles][4];
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4 dv = st[(size_t)(kStBlock * l + q) * 64];
                half8 dd;
                __builtin_memcpy(&dd, &dv, 16);
#pragma unroll
                for (int e = 0; e < 8; ++e) xh[2 * q + (e >> 2)][e & 3] = ((float)dd[e] - mean) * rstd;
            }
#pragma unroll
            for (int t = 0; t < kTiles; ++t) {
                const u32x4 zv = st[(size_t)(kStBlock * l + 4 + t) * 64];
                f4 z;
                __builtin_memcpy(&z, &zv, 16);
                f4 gz;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sg = sigmoidf(z[r]);
                    // SiLU' = sig (1 + z (1 - sig)), f32
                    gz[r] = ga[t][r] * (sg * (1.0f + z[r] * (1.0f - sg)));
                    ga[t][r] = gz[r];  // the residual branch's share (blocks 1..3)
                }
                if (l == 0) gsk[t] = __builtin_convertvector(gz, half4);
                if (WG) {
                    // LayerNorm parameter gradients of this tile's 16 samples
                    f4 pg, pb;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pg[r] = row16_sum(gz[r] * xh[t][r]);
                        pb[r] = row16_sum(gz[r]);
                    }
                    if (c == 0) {  // neurons 16 t + 4 h .. + 3: one writer per wave
                        f4 *ag = reinterpret_cast<f4 *>(&lnacc[wave][l][0][16 * t + 4 * h]);
                        f4 *ab = reinterpret_cast<f4 *>(&lnacc[wave][l][1][16 * t + 4 * h]);
                        *ag = *ag + pg;
                        *ab = *ab + pb;
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gy[t][r] = gz[r] * W.gamma[l][16 * t + 4 * h + r];
                    s1 += gy[t][r];
                    s2 += gy[t][r] * xh[t][r];
                }
            }
            // LayerNorm backward, f32: rstd (gy - mean(gy) - xhat mean(gy xhat))
            const float m1 = groups_sum(s1) * (1.0f / kHid), m2 = groups_sum(s2) * (1.0f / kHid);
            half4 gd[kTiles];
#pragma unroll
            for (int t = 0; t < kTiles; ++t) {
                f4 g;
#pragma unroll
                for (int r = 0; r < 4; ++r) g[r] = rstd * (gy[t][r] - m1 - xh[t][r] * m2);
                gd[t] = __builtin_convertvector(g, half4);
                if (WG)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const size_t row = 16 * t + 4 * h + r;
                        grows[((size_t)kHid * l + row) * Mp + sample] = gd[t][r];
                        if (l == 0) grows[((size_t)kGSkip + row) * Mp + sample] = gsk[t][r];
                    }
            }
            if (l > 0) {
                // dL/d(a_{l-1}) = f32 of the f16 product gd @ W_l, plus the residual's
#pragma unroll
                for (int t = 0; t < kTiles; ++t) {
                    f4 acc = f4{0, 0, 0, 0};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc = mfma(a_perm(W.wt[l - 1], kLdH, 16 * t + c, s, h), b_tiles(gd, s), acc);
                    const half4 dh = __builtin_convertvector(acc, half4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) ga[t][r] = (float)dh[r] + ga[t][r];
                }
            } else if constexpr (DX) {
                // encoding gradient (f16: the dense and the skip product, added in
                // f16), then the encoder's chain rule (freqencoder.hip k_freq_bwd)
                // and the Gaussian blob's term
                float part[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    f4 ad = f4{0, 0, 0, 0}, as = f4{0, 0, 0, 0};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        ad = mfma(a_perm(W.w0t, kLdH, 16 * t + c, s, h), b_tiles(gd, s), ad);
                        as = mfma(a_perm(W.w0t + kEncPad * kLdH, kLdH, 16 * t + c, s, h),
                                  b_tiles(gsk, s), as);
                    }
                    const half4 hd = __builtin_convertvector(ad, half4);
                    const half4 hs = __builtin_convertvector(as, half4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * t + 4 * h + r;
                        const float g = (float)(half_t)((float)hd[r] + (float)hs[r]);
                        const int d = f % 3;
                        const float xd = d == 0 ? x[0] : (d == 1 ? x[1] : x[2]);
                        float contrib = 0.0f;
                        if (f < 3) {
                            contrib = g;
                        } else if (f < kEnc) {
                            const int col = f / 3 - 1, k = col >> 1;
                            const float arg = scalbnf(xd, k);
                            // d sin = cos, d cos = -sin, with the saved outputs' own
                            // form of cos: sin(. + pi/2)
                            const float o = (col & 1) ? -sinf(arg) : sinf(arg + kHalfPi);
                            contrib = scalbnf(1.0f, k) * (g * o);
                        }
                        part[0] += d == 0 ? contrib : 0.0f;
                        part[1] += d == 1 ? contrib : 0.0f;
                        part[2] += d == 2 ? contrib : 0.0f;
                    }
                }
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const float e = groups_sum(part[d]);
                    // gaussian = 5 exp(-|x|^2 / 0.08): d/dx = gaussian * (-2 x / 0.08)
                    const float gg = gpre * (gauss * (-2.0f * x[d] / 0.08f));
                    if (valid && h == 0) dx[(size_t)sample * 3 + d] = e + gg;
                }
            }
        }
    }
    if (WG) {
        __syncthreads();
        // the workgroup's LayerNorm partial: waves added in order
        for (int i = threadIdx.x; i < kBlocks * 2 * kHid; i += blockDim.x) {
            float s = 0.0f;
            for (int w = 0; w < WAVES; ++w) s += (&lnacc[w][0][0][0])[i];
            lnout[i] = s;
        }
    }
    } while (DEV);
}

// ------------------------------------------------------------------ weight gradients
// One wave per (job, split): job = 16 output rows of one Linear against all of
// its input columns, split = a range of 32-sample k-steps.  Both operands are
// 16-byte loads from the neuron-major images: A[i = c][k = 8 h + j] is the
// output gradient of row row0 + c at samples 32 ks + 8 h + j, B[k][col = c]
// the input of column 16 tm + c at the same samples; the bias is the product
// with a ones operand.  Jobs: 0..7 layer 0 dense, 8..15 layer 0 skip, 16..39
// layers 1..3, 40 the output layer.
constexpr int kJobs = 41;

// wgrad_chunk: one chunk's product of wave (job, split) out of `splits`:
// images of row stride Mp, mp / 32 k-steps.
__device__ __forceinline__ void wgrad_chunk(const half_t *__restrict__ xrows,
                                            const half_t *__restrict__ arows,
                                            const half_t *__restrict__ grows, uint32_t Mp,
                                            uint32_t mp, uint32_t split, uint32_t splits,
                                            float *__restrict__ partial) {
    const int job = blockIdx.x, lane = threadIdx.x, c = lane & 15, h = lane >> 4;
    const uint32_t ksteps = mp / 32u;
    const uint32_t per = ceil_div(ksteps, splits);
    const uint32_t k0 = split * per < ksteps ? split * per : ksteps;
    const uint32_t k1 = k0 + per < ksteps ? k0 + per : ksteps;
    const half_t *G, *B;
    int ntile, nrow, ld, ncol, tw, tb;  // column tiles, live rows, out stride, out columns
    int row0;
    if (job < 16) {
        row0 = 16 * (job & 7);
        G = grows + (size_t)(job < 8 ? 0 : kGSkip) * Mp;
        B = xrows;
        ntile = 3, nrow = 16, ld = kEnc, ncol = kEnc;
        tw = job < 8 ? 0 : kTSkip, tb = job < 8 ? 1 : -1;
    } else if (job < 40) {
        const int l = 1 + (job - 16) / 8;
        row0 = 16 * ((job - 16) & 7);
        G = grows + (size_t)(kHid * l) * Mp;
        B = arows + (size_t)(kHid * (l - 1)) * Mp;
        ntile = 8, nrow = 16, ld = kHid, ncol = kHid;
        tw = t_dense_w(l), tb = t_dense_b(l);
    } else {
        row0 = 0;
        G = grows + (size_t)kGOut * Mp;
        B = arows + (size_t)(kHid * 3) * Mp;
        ntile = 8, nrow = kOut, ld = kHid, ncol = kHid;
        tw = kTOutW, tb = kTOutB;
    }
    f4 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = f4{0, 0, 0, 0};
    const half_t one = (half_t)1.0f;
    const half8 ones8 = half8{one, one, one, one, one, one, one, one};
    for (uint32_t ks = k0; ks < k1; ++ks) {
        const size_t col = (size_t)32 * ks + 8 * h;
        half8 a = half8{};
        if (c < nrow) a = *reinterpret_cast<const half8 *>(G + (size_t)(row0 + c) * Mp + col);
#pragma unroll
        for (int tm = 0; tm < 8; ++tm)
            if (tm < ntile)
                acc[tm] = mfma(a, *reinterpret_cast<const half8 *>(B + (size_t)(16 * tm + c) * Mp + col),
                               acc[tm]);
        acc[8] = mfma(a, ones8, acc[8]);
    }
    // accumulator element r of lane (c, h): row 4 h + r, column c of the tile;
    // every partial entry is written by exactly one lane of one job
    float *out = partial + (size_t)split * kParams;
    int offw = 0, offb = 0;
#pragma unroll
    for (int t = 0; t < kTensors; ++t) {
        if (t == tw) offw = t_offset(t);
        if (t == tb) offb = t_offset(t);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * h + r;
        if (row >= nrow) continue;
#pragma unroll
        for (int tm = 0; tm < 8; ++tm)
            if (tm < ntile && 16 * tm + c < ncol)
                out[offw + (row0 + row) * ld + 16 * tm + c] = acc[tm][r];
        if (tb >= 0 && c == 0) out[offb + row0 + row] = acc[8][r];
    }
}

__global__ __launch_bounds__(64) void k_resmlp_wgrad(const half_t *__restrict__ xrows,
                                                     const half_t *__restrict__ arows,
                                                     const half_t *__restrict__ grows,
                                                     uint32_t Mp, float *__restrict__ partial) {
    wgrad_chunk(xrows, arows, grows, Mp, Mp, blockIdx.y, gridDim.y, partial);
}

// Device count: wave (job, split) takes its share of every live chunk in turn;
// chunk c has kSplits partial images at partial + c * kSplits * kParams.
__global__ __launch_bounds__(64) void k_resmlp_wgrad_dev(const half_t *__restrict__ rows,
                                                         uint32_t cap,
                                                         const int32_t *__restrict__ m_dev,
                                                         uint32_t align,
                                                         float *__restrict__ partial) {
    const uint32_t Me = effective_rows(live_rows(m_dev, cap), cap, align);
    for (uint32_t chunk = 0; chunk * kChunk < Me; ++chunk) {
        const Chunk k = chunk_of(chunk, Me, cap, 1u);  // (nblk unused)
        if (blockIdx.y >= k.splits) continue;
        const half_t *img = rows + (size_t)chunk * kChunk * kRowsAll;
        wgrad_chunk(img, img + (size_t)kXRows * k.ld, img + (size_t)(kXRows + kARows) * k.ld, k.ld,
                    k.mp, blockIdx.y, k.splits, partial + (size_t)chunk * kSplits * kParams);
    }
}

// Fixed-order sums into the f32 gradients: a block takes 64 parameters; its
// 16 part-lanes add the parts p = j, j + 16, ... in that order, then lane
// j = 0 adds the 16 lane sums in order (as fieldmlp.hip's k_field_wgrad_sum).
// Linear parameters come from the weight-gradient splits, LayerNorm
// parameters from the gradient pass's workgroups.
__global__ __launch_bounds__(1024) void k_resmlp_reduce(const float *__restrict__ partial,
                                                        uint32_t splits,
                                                        const float *__restrict__ lnpart,
                                                        uint32_t lnparts, GPtrs G,
                                                        int accumulate) {
    __shared__ float lane_sum[16][64];
    const int col = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + col;
    int ti = 0, k = 0;
    float s = 0.0f;
    if (i < kParams) {
        int off = 0;
        for (int t = 0; t < kTensors; ++t) {
            const int sz = t_size(t);
            if (i >= off && i < off + sz) ti = t, k = i - off;
            off += sz;
        }
        // LayerNorm tensors: index 2, 3 of block 0's five, of the later blocks' four
        const int l = ti < 5 ? 0 : (ti < kTOutW ? 1 + (ti - 5) / 4 : -1);
        const int w = ti < 5 ? ti : (ti < kTOutW ? (ti - 5) % 4 : -1);
        const float *src = partial + i;
        size_t stride = kParams;
        uint32_t parts = splits;
        if (l >= 0 && (w == 2 || w == 3)) {
            src = lnpart + (size_t)(l * 2 + (w - 2)) * kHid + k;
            stride = kBlocks * 2 * kHid;
            parts = lnparts;
        }
        for (uint32_t p = j; p < parts; p += 16) s += src[(size_t)p * stride];
    }
    lane_sum[j][col] = s;
    __syncthreads();
    if (j != 0 || i >= kParams) return;
    s = 0.0f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += lane_sum[q][col];
    float *dst = G.p[ti];
    dst[k] = accumulate ? dst[k] + s : s;
}

// Device count: the chunks' sums in chunk order, each formed as above (the
// chunk's own split and workgroup counts) and added to the running f32 value
// as the host loop's launches add it in memory.  No live chunk: zeros, or
// nothing with accumulate.
__global__ __launch_bounds__(1024) void k_resmlp_reduce_dev(const float *__restrict__ partial,
                                                            const float *__restrict__ lnpart,
                                                            uint32_t cap,
                                                            const int32_t *__restrict__ m_dev,
                                                            uint32_t align, uint32_t cus, GPtrs G,
                                                            int accumulate) {
    __shared__ float lane_sum[16][64];
    const uint32_t Me = effective_rows(live_rows(m_dev, cap), cap, align);
    const int col = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + col;
    int ti = 0, k = 0;
    bool ln = false;
    size_t src0 = 0;
    if (i < kParams) {
        int off = 0;
        for (int t = 0; t < kTensors; ++t) {
            const int sz = t_size(t);
            if (i >= off && i < off + sz) ti = t, k = i - off;
            off += sz;
        }
        const int l = ti < 5 ? 0 : (ti < kTOutW ? 1 + (ti - 5) / 4 : -1);
        const int w = ti < 5 ? ti : (ti < kTOutW ? (ti - 5) % 4 : -1);
        ln = l >= 0 && (w == 2 || w == 3);
        src0 = ln ? (size_t)(l * 2 + (w - 2)) * kHid + k : (size_t)i;
    }
    const bool writer = j == 0 && i < kParams;
    float *dst = G.p[ti];
    float v = 0.0f;
    if (writer && accumulate) v = dst[k];
    for (uint32_t chunk = 0; chunk * kChunk < Me; ++chunk) {  // block-uniform
        const Chunk ck = chunk_of(chunk, Me, cap, cus);
        const float *src = ln ? lnpart + (size_t)chunk * kLnParts * (kBlocks * 2 * kHid) + src0
                              : partial + (size_t)chunk * kSplits * kParams + src0;
        const size_t stride = ln ? kBlocks * 2 * kHid : kParams;
        const uint32_t parts = ln ? ck.nblk : ck.splits;
        float s = 0.0f;
        if (i < kParams)
            for (uint32_t p = j; p < parts; p += 16) s += src[(size_t)p * stride];
        lane_sum[j][col] = s;
        __syncthreads();
        if (writer) {
            s = 0.0f;
#pragma unroll
            for (int q = 0; q < 16; ++q) s += lane_sum[q][col];
            v = (accumulate || chunk > 0) ? v + s : s;
        }
        __syncthreads();  // lane_sum is rewritten next
    }
    if (writer && !(accumulate && Me == 0)) dst[k] = v;
}

// ------------------------------------------------------------------ host side
// scratch layout for a chunk of mp (padded) samples; all sizes are multiples
// of 16 bytes
struct Scratch {
    size_t state, xrows, arows, grows, partial, lnpart, total;
};
static Scratch scratch_layout(uint32_t mp) {
    Scratch s;
    size_t o = 0;
    s.state = o, o += (size_t)(mp / 16u) * kStTile * 64 * sizeof(u32x4);
    s.xrows = o, o += (size_t)kXRows * mp * sizeof(half_t);
    s.arows = o, o += (size_t)kARows * mp * sizeof(half_t);
    s.grows = o, o += (size_t)kGRows * mp * sizeof(half_t);
    s.partial = o, o += (size_t)kSplits * kParams * sizeof(float);
    s.lnpart = o, o += (size_t)kLnParts * kBlocks * 2 * kHid * sizeof(float);
    s.total = o;
    return s;
}

// Device count: the tile state and the three neuron-major images of every
// chunk of the capacity (cap rounded up to 32), then per 65536-row chunk
// kSplits partial images of the gradients and kLnParts LayerNorm partials.
struct ScratchDev {
    size_t state, rows, partial, lnpart, total;
};
static ScratchDev scratch_layout_dev(uint32_t cap) {
    ScratchDev s;
    const size_t capp = ceil_div((size_t)cap, (size_t)32) * 32, chunks = ceil_div(cap, kChunk);
    size_t o = 0;
    s.state = o, o += capp / 16 * kStTile * 64 * sizeof(u32x4);
    s.rows = o, o += (size_t)kRowsAll * capp * sizeof(half_t);
    s.partial = o, o += chunks * kSplits * kParams * sizeof(float);
    s.lnpart = o, o += chunks * kLnParts * kBlocks * 2 * kHid * sizeof(float);
    s.total = o ? o : 16;
    return s;
}

static uint32_t persistent_blocks(uint32_t tiles, int waves, uint32_t cap) {
    const uint32_t want = ceil_div(tiles, (uint32_t)waves), cus = device_cus();
    uint32_t n = want < cus ? want : cus;
    if (n > cap) n = cap;
    return n ? n : 1u;
}

template <bool DX, bool WG, int WAVES>
static void launch_bwd_act(hipStream_t s, uint32_t nblk, const float *xyz, const Ptrs &P,
                           const float *gs, const void *ga, int ga_dtype, uint32_t m,
                           uint32_t tiles, const u32x4 *state, half_t *grows, uint32_t mp,
                           float *lnpart, float *dx) {
    if (ga_dtype == DFHIP_F16)
        k_resmlp_bwd_act<DX, WG, WAVES, half_t><<<nblk, 64 * WAVES, 0, s>>>(
            xyz, P, gs, (const half_t *)ga, m, tiles, state, grows, mp, lnpart, dx, DevCount<false>{});
    else
        k_resmlp_bwd_act<DX, WG, WAVES, float><<<nblk, 64 * WAVES, 0, s>>>(
            xyz, P, gs, (const float *)ga, m, tiles, state, grows, mp, lnpart, dx, DevCount<false>{});
}

}  // namespace rs
}  // namespace dfhip

using namespace dfhip;
using namespace dfhip::rs;

extern "C" uint32_t dfhip_resmlp_params(void) { return (uint32_t)kParams; }

extern "C" uint64_t dfhip_resmlp_field_backward_scratch(uint32_t M) {
    return (uint64_t)scratch_layout(padded(M < kChunk ? M : kChunk)).total;
}

static bool gather(const char *name, const float *const *params, Ptrs &P) {
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

extern "C" int dfhip_resmlp_field_forward(const float *xyz, const float *const *params,
                                          float *sigma, void *albedo, uint32_t M,
                                          dfhip_stream_t stream) {
    const char *name = "resmlp_field_forward";
    Ptrs P;
    if (!gather(name, params, P)) return DFHIP_EINVAL;
    if (M == 0) return DFHIP_OK;
    if (!xyz || !sigma || !albedo) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    const uint32_t tiles = ceil_div(M, 16u);
    k_resmlp_fwd<false><<<persistent_blocks(tiles, kFwdWaves, 65535u), 64 * kFwdWaves, 0,
                          as_stream(stream)>>>(xyz, P, sigma, (half_t *)albedo, M, tiles, nullptr,
                                               nullptr, nullptr, 0u);
    return check_launch(name);
}

extern "C" int dfhip_resmlp_field_backward(const float *xyz, const float *const *params,
                                           const float *grad_sigma, const void *grad_albedo,
                                           int grad_albedo_dtype, uint32_t M, float *dx,
                                           void *scratch, float *const *grads, int accumulate,
                                           dfhip_stream_t stream) {
    const char *name = "resmlp_field_backward";
    Ptrs P;
    if (!gather(name, params, P)) return DFHIP_EINVAL;
    GPtrs G;
    if (grads)
        for (int t = 0; t < kTensors; ++t) {
            if (!grads[t]) {
                set_error("%s: gradient %d is null", name, t);
                return DFHIP_EINVAL;
            }
            G.p[t] = grads[t];
        }
    if (!grads && !dx) {
        set_error("%s: neither grads nor dx requested", name);
        return DFHIP_EINVAL;
    }
    if (grad_albedo_dtype != DFHIP_F16 && grad_albedo_dtype != DFHIP_F32) {
        set_error("%s: grad_albedo dtype must be f16 or f32", name);
        return DFHIP_EDTYPE;
    }
    if (!scratch || ((uintptr_t)scratch & 15u)) {
        set_error("%s: scratch must be a 16-byte aligned buffer of "
                  "dfhip_resmlp_field_backward_scratch(M) bytes", name);
        return DFHIP_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    if (M == 0) {
        if (grads && !accumulate)
            for (int t = 0; t < kTensors; ++t)
                (void)hipMemsetAsync(G.p[t], 0, t_size(t) * sizeof(float), s);
        return check_launch(name);
    }
    if (!xyz || !grad_sigma || !grad_albedo) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    char *base = (char *)scratch;
    const size_t ga_size = grad_albedo_dtype == DFHIP_F16 ? 2 : 4;
    for (uint32_t m0 = 0; m0 < M; m0 += kChunk) {
        const uint32_t m = M - m0 < kChunk ? M - m0 : kChunk;
        const uint32_t mp = padded(m), tiles = mp / 16u;
        const Scratch L = scratch_layout(mp);
        u32x4 *state = (u32x4 *)(base + L.state);
        half_t *xrows = (half_t *)(base + L.xrows), *arows = (half_t *)(base + L.arows);
        half_t *grows = (half_t *)(base + L.grows);
        float *partial = (float *)(base + L.partial), *lnpart = (float *)(base + L.lnpart);
        const float *x = xyz + (size_t)m0 * 3, *gs = grad_sigma + m0;
        const void *ga = (const char *)grad_albedo + (size_t)m0 * 3 * ga_size;
        float *dxc = dx ? dx + (size_t)m0 * 3 : nullptr;
        k_resmlp_fwd<true><<<persistent_blocks(tiles, kFwdWaves, 65535u), 64 * kFwdWaves, 0, s>>>(
            x, P, nullptr, nullptr, m, tiles, state, grads ? xrows : nullptr,
            grads ? arows : nullptr, mp);
        if (!grads) {
            launch_bwd_act<true, false, 8>(s, persistent_blocks(tiles, 8, kLnParts), x, P, gs, ga,
                                           grad_albedo_dtype, m, tiles, state, nullptr, mp,
                                           nullptr, dxc);
            continue;
        }
        uint32_t nblk;
        if (dx) {
            // both: the layer-0 transposes and the LayerNorm accumulators fit
            // LDS together with 4 waves
            nblk = persistent_blocks(tiles, 4, kLnParts);
            launch_bwd_act<true, true, 4>(s, nblk, x, P, gs, ga, grad_albedo_dtype, m, tiles,
                                          state, grows, mp, lnpart, dxc);
        } else {
            nblk = persistent_blocks(tiles, 8, kLnParts);
            launch_bwd_act<false, true, 8>(s, nblk, x, P, gs, ga, grad_albedo_dtype, m, tiles,
                                           state, grows, mp, lnpart, nullptr);
        }
        const uint32_t splits = mp / 32u < kSplits ? mp / 32u : kSplits;
        k_resmlp_wgrad<<<dim3(kJobs, splits), 64, 0, s>>>(xrows, arows, grows, mp, partial);
        k_resmlp_reduce<<<ceil_div((uint32_t)kParams, 64u), 1024, 0, s>>>(
            partial, splits, lnpart, nblk, G, (accumulate || m0 > 0) ? 1 : 0);
    }
    return check_launch(name);
}

// ------------------------------------------------------------------ device-count entries
// The checks of the device-count forms' own arguments.
static bool device_count(const char *name, uint32_t cap, const int32_t *m_dev, uint32_t align) {
    if (cap > 0x7fffffffu) {
        set_error("%s: the capacity must be below 2^31 rows, got %u", name, cap);
        return false;
    }
    if (!m_dev) {
        set_error("%s: m_dev is null", name);
        return false;
    }
    if (align == 0) {
        set_error("%s: align must be at least 1", name);
        return false;
    }
    return true;
}

extern "C" int dfhip_resmlp_field_forward_dev(const float *xyz, const float *const *params,
                                              float *sigma, void *albedo, uint32_t cap,
                                              const int32_t *m_dev, uint32_t align,
                                              dfhip_stream_t stream) {
    const char *name = "resmlp_field_forward_dev";
    Ptrs P;
    if (!gather(name, params, P)) return DFHIP_EINVAL;
    if (!device_count(name, cap, m_dev, align)) return DFHIP_EINVAL;
    if (cap == 0) return DFHIP_OK;
    if (!xyz || !sigma || !albedo) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    // the launch shape of the capacity; the kernel stops at the live tiles
    const uint32_t tiles = ceil_div(cap, 16u);
    k_resmlp_fwd_dev<false><<<persistent_blocks(tiles, kFwdWaves, 65535u), 64 * kFwdWaves, 0,
                              as_stream(stream)>>>(xyz, P, sigma, (half_t *)albedo, cap, m_dev,
                                                   align, nullptr, nullptr);
    return check_launch(name);
}

extern "C" uint64_t dfhip_resmlp_field_backward_dev_scratch(uint32_t cap) {
    return (uint64_t)scratch_layout_dev(cap).total;
}

extern "C" int dfhip_resmlp_field_backward_dev(const float *xyz, const float *const *params,
                                               const float *grad_sigma, const void *grad_albedo,
                                               int grad_albedo_dtype, uint32_t cap,
                                               const int32_t *m_dev, uint32_t align,
                                               void *scratch, float *const *grads,
                                               int accumulate, dfhip_stream_t stream) {
    const char *name = "resmlp_field_backward_dev";
    Ptrs P;
    if (!gather(name, params, P)) return DFHIP_EINVAL;
    GPtrs G;
    if (!grads) {
        set_error("%s: null gradient list", name);
        return DFHIP_EINVAL;
    }
    for (int t = 0; t < kTensors; ++t) {
        if (!grads[t]) {
            set_error("%s: gradient %d is null", name, t);
            return DFHIP_EINVAL;
        }
        G.p[t] = grads[t];
    }
    if (grad_albedo_dtype != DFHIP_F16 && grad_albedo_dtype != DFHIP_F32) {
        set_error("%s: grad_albedo dtype must be f16 or f32", name);
        return DFHIP_EDTYPE;
    }
    if (!device_count(name, cap, m_dev, align)) return DFHIP_EINVAL;
    if (!scratch || ((uintptr_t)scratch & 15u)) {
        set_error("%s: scratch must be a 16-byte aligned buffer of "
                  "dfhip_resmlp_field_backward_dev_scratch(cap) bytes", name);
        return DFHIP_EINVAL;
    }
    if (cap && (!xyz || !grad_sigma || !grad_albedo)) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    const ScratchDev L = scratch_layout_dev(cap);
    char *base = (char *)scratch;
    u32x4 *state = (u32x4 *)(base + L.state);
    half_t *rows = (half_t *)(base + L.rows);
    float *partial = (float *)(base + L.partial), *lnpart = (float *)(base + L.lnpart);
    const uint32_t cus = device_cus();
    if (cap) {
        // launch shapes of the capacity; the kernels stop at the live chunks
        const uint32_t tiles = ceil_div(cap, 32u) * 2u;
        k_resmlp_fwd_dev<true><<<persistent_blocks(tiles, kFwdWaves, 65535u), 64 * kFwdWaves, 0,
                                 s>>>(xyz, P, nullptr, nullptr, cap, m_dev, align, state, rows);
        const uint32_t nblk = persistent_blocks(tiles, 8, kLnParts);
        const DevCount<true> dev{xyz, grad_sigma, grad_albedo, state, rows, m_dev, cap, align, cus};
        if (grad_albedo_dtype == DFHIP_F16)
            k_resmlp_bwd_act<false, true, 8, half_t, true><<<nblk, 64 * 8, 0, s>>>(
                nullptr, P, nullptr, nullptr, 0u, 0u, nullptr, nullptr, 0u, lnpart, nullptr, dev);
        else
            k_resmlp_bwd_act<false, true, 8, float, true><<<nblk, 64 * 8, 0, s>>>(
                nullptr, P, nullptr, nullptr, 0u, 0u, nullptr, nullptr, 0u, lnpart, nullptr, dev);
        const uint32_t first = padded(cap < kChunk ? cap : kChunk);
        const uint32_t splits = first / 32u < kSplits ? first / 32u : kSplits;
        k_resmlp_wgrad_dev<<<dim3(kJobs, splits), 64, 0, s>>>(rows, cap, m_dev, align, partial);
    }
    k_resmlp_reduce_dev<<<ceil_div((uint32_t)kParams, 64u), 1024, 0, s>>>(
        partial, lnpart, cap, m_dev, align, cus, G, accumulate ? 1 : 0);
    return check_launch(name);
}
