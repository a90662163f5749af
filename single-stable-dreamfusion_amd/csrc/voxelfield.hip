// Fused voxel field on MFMA (gfx950): the DVGO backbone of
// nerf/network_dvgo.py.  Frozen dense volumes (density [Nx, Ny, Nz], k0
// [Nx, Ny, Nz, C] channel last, both f32), a trainable colour MLP
// dim0 -> 128 -> 128 -> 3 (BasicMLP, ReLU).
//
// Behavioural spec: nerf/network.py:245-268 (to_our_coor, common_forward with
// weight = None), frameworks/nerf/modules/osr_fine.py:559-673 (the trilinear
// sample), dvgo_fine.py:45-54 (query_rgb), modules/utils.py:129-131
// (position_encoding), decoders/mlps.py:59-73 (BasicMLP), run under
// torch.autocast(fp16): map, sample, activation and encodings are f32, the
// feature row is cast to f16 at the first Linear, every Linear is an f16
// GEMM with f32 accumulation and an f16 output, ReLU and sigmoid act on f16.
//
// Forward: one launch.  A workgroup of 8 waves keeps the f16 weights in LDS
// (65 KiB); a wave takes 16 samples through map, gathers, encodings and the
// three layers in registers (voxel_common.h).  The four lane groups of a
// sample fill its 96-feature row, every fourth feature each, into a per-wave
// LDS image (26 KiB per workgroup) and read their operands back from it.  A
// tile with no row inside the box skips the MLP.
//
// Backward (parameter gradients only: the volumes are frozen and the
// positions are leaves), three launches per chunk of up to 65536 samples:
//   1. the forward again with the transposed second layer also in LDS
//      (101 KiB), then the output gradients of the three Linears (sigmoid' and
//      the two W^T products as f16 GEMM outputs, ReLU masks); every Linear's
//      f16 input and output gradient is stored neuron-major;
//   2. the weight gradients as MFMA products over the sample axis, split over
//      the samples into per-split partials;
//   3. a fixed-order sum of the partials into the f32 gradients.
// No float atomics anywhere: two runs give the same bits.
//
// Normal: -d sigma / d x in closed form, one thread per sample.
#include "voxel_common.h"

namespace dfhip {
namespace vx {

constexpr int kWaves = 8;     // forward
constexpr int kBwdWaves = 4;  // gradient pass: twice the forward's register budget per wave
constexpr uint32_t kChunk = 65536;  // samples per backward chunk
constexpr uint32_t kSplits = 64;    // sample-axis splits of the weight-gradient products

// ------------------------------------------------------------------ device counts
// The kDev instances of the kernels below take their row count from the
// device: M is then the capacity of the buffers and *m_dev the live count, so
// the launch shape depends on the capacity only and the launches capture into
// a graph.  Rows at or past the live count are neither read nor written.
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

// ------------------------------------------------------------------ density only
template <bool kDev>
__global__ __launch_bounds__(256) void k_voxel_sigma(const float *__restrict__ xyz,
                                                     const float *__restrict__ density, Geom G,
                                                     float *__restrict__ sigma, uint32_t M,
                                                     const int32_t *__restrict__ m_dev) {
    if constexpr (kDev) M = live_rows(m_dev, M);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= M) return;
    const float x[3] = {xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2]};
    const Cell c = locate(G, x);
    float raw = 0.0f;
    if (c.inside) raw = trilinear(corners(G, c), density, 1u, 0u);
    sigma[i] = activate(raw, G.act_shift);
}

// ------------------------------------------------------------------ forward
// (the body of both kernels below: the host-count one keeps its argument list)
__device__ __forceinline__ void voxel_fwd(
    const float *__restrict__ xyz, const float *__restrict__ density,
    const float *__restrict__ k0, const float *__restrict__ view, const Geom &G, const Ptrs &P,
    float *__restrict__ sigma, half_t *__restrict__ albedo, uint32_t M, uint32_t tiles) {
    __shared__ FwdW W;
    __shared__ __attribute__((aligned(16))) half_t xbuf[kWaves][16 * kLdI];
    load_fwd_weights(W, P, G.dim0);
    __syncthreads();
    const int lane = threadIdx.x & 63, c = lane & 15, h = lane >> 4;
    const uint32_t waves = gridDim.x * kWaves;
    for (uint32_t tile = blockIdx.x * kWaves + (threadIdx.x >> 6); tile < tiles; tile += waves) {
        // weights are re-read from LDS every tile (hoisted out of the loop
        // they spill; fieldmlp.hip's idiom)
        asm volatile("" ::: "memory");
        const uint32_t sample = tile * 16 + c;
        const bool valid = sample < M;
        float x[3] = {0.0f, 0.0f, 0.0f};
        if (valid)
#pragma unroll
            for (int d = 0; d < 3; ++d) x[d] = xyz[(size_t)sample * 3 + d];
        const Cell cell = locate(G, x);
        const bool inside = valid && cell.inside;
        if (valid && h == 0) {
            float raw = 0.0f;
            if (inside) raw = trilinear(corners(G, cell), density, 1u, 0u);
            sigma[sample] = activate(raw, G.act_shift);
        }
        float out[kOut] = {0.0f, 0.0f, 0.0f};
        if (__ballot(inside) != 0ull) {  // wave-uniform
            half8 xb[kSteps0];
            feature_operands(G, cell, inside, k0, view, c, h, xbuf[threadIdx.x >> 6], xb);
            half4 a1[kTiles], a2[kTiles];
            mlp_tile(W, xb, c, h, a1, a2, out);
        }
        if (valid && h == 0)
#pragma unroll
            for (int k = 0; k < kOut; ++k)
                albedo[(size_t)sample * 3 + k] = inside ? (half_t)sigmoidf(out[k]) : (half_t)0.5f;
    }
}

__global__ __launch_bounds__(64 * kWaves) void k_voxel_fwd(
    const float *__restrict__ xyz, const float *__restrict__ density,
    const float *__restrict__ k0, const float *__restrict__ view, Geom G, Ptrs P,
    float *__restrict__ sigma, half_t *__restrict__ albedo, uint32_t M, uint32_t tiles) {
    voxel_fwd(xyz, density, k0, view, G, P, sigma, albedo, M, tiles);
}

// Device count: `cap` rows of buffers, the tiles of the live rows.
__global__ __launch_bounds__(64 * kWaves) void k_voxel_fwd_dev(
    const float *__restrict__ xyz, const float *__restrict__ density,
    const float *__restrict__ k0, const float *__restrict__ view, Geom G, Ptrs P,
    float *__restrict__ sigma, half_t *__restrict__ albedo, uint32_t cap,
    const int32_t *__restrict__ m_dev) {
    const uint32_t M = live_rows(m_dev, cap);
    voxel_fwd(xyz, density, k0, view, G, P, sigma, albedo, M, ceil_div(M, 16u));
}

// ------------------------------------------------------------------ gradient pass
// The forward's images, the second layer transposed ([n_in][n_out]) and the
// output layer as f32 of its f16 weights (its transposed product is three
// FMAs per neuron).
struct alignas(16) BwdW {
    half_t w0[kHid * kLdI], w1[kHid * kLdH], w2[16 * kLdH];
    float b0[kHid], b1[kHid], b2[16];
    half_t w1t[kHid * kLdH];
    float w2f[kOut][kHid];
};

__device__ inline void load_bwd_weights(BwdW &W, const Ptrs &P, uint32_t dim0) {
    load_fwd_weights(*reinterpret_cast<FwdW *>(&W), P, dim0);
    for (int i = threadIdx.x; i < kHid * kHid; i += blockDim.x)
        W.w1t[(i % kHid) * kLdH + i / kHid] = (half_t)P.p[2][i];  // w[n_out][n_in]
    for (int i = threadIdx.x; i < kOut * kHid; i += blockDim.x)
        W.w2f[i / kHid][i % kHid] = (float)(half_t)P.p[4][i];
}
static_assert(offsetof(BwdW, w1t) == sizeof(FwdW), "BwdW starts with FwdW's members");

// Rows of the neuron-major f16 images ([row][Mp], column = sample) the weight
// gradients read: the feature row, both hidden activations, and the output
// gradients of the three Linears.
constexpr int kRowX = 0, kRowA1 = kRowX + kInPad, kRowA2 = kRowA1 + kHid, kRowG1 = kRowA2 + kHid,
              kRowG2 = kRowG1 + kHid, kRowGo = kRowG2 + kHid, kRows = kRowGo + 8;

// kDev: M is the capacity.  Rows [0, live) are read; the tiles up to the
// padded effective count are written, rows from the live count on as padding
// rows (zero output gradients).  Chunk c of 65536 samples has its images at
// rows + kRows * kChunk * c with the row stride of the capacity's chunk c, so
// the layout depends on the capacity only.
template <typename ga_t, bool kDev>
__global__ __launch_bounds__(64 * kBwdWaves) void k_voxel_bwd_act(
    const float *__restrict__ xyz, const float *__restrict__ k0, const float *__restrict__ view,
    Geom G, Ptrs P, const ga_t *__restrict__ grad_albedo, uint32_t M, uint32_t tiles, uint32_t Mp,
    half_t *__restrict__ rows, const int32_t *__restrict__ m_dev, uint32_t align) {
    const uint32_t cap = M;
    if constexpr (kDev) {
        M = live_rows(m_dev, cap);
        tiles = padded(effective_rows(M, cap, align)) / 16u;
    }
    __shared__ BwdW W;
    __shared__ __attribute__((aligned(16))) half_t xbuf[kBwdWaves][16 * kLdI];
    load_bwd_weights(W, P, G.dim0);
    __syncthreads();
    const int lane = threadIdx.x & 63, c = lane & 15, h = lane >> 4;
    const uint32_t waves = gridDim.x * kBwdWaves;
    // tiles = Mp / 16: the padding rows of the last tile are written as zeros
    for (uint32_t tile = blockIdx.x * kBwdWaves + (threadIdx.x >> 6); tile < tiles; tile += waves) {
        asm volatile("" ::: "memory");  // no hoisting of the LDS operands (see k_voxel_fwd)
        const uint32_t sample = tile * 16 + c;
        const bool valid = sample < M;
        // the images of this tile: [row][ld], column col
        half_t *rw = rows;
        uint32_t ld = Mp, col = sample;
        if constexpr (kDev) {
            const uint32_t chunk = (tile * 16u) / kChunk, left = cap - chunk * kChunk;
            rw = rows + (size_t)kRows * kChunk * chunk;
            ld = padded(left < kChunk ? left : kChunk);
            col = sample - chunk * kChunk;
        }
        float x[3] = {0.0f, 0.0f, 0.0f};
        if (valid)
#pragma unroll
            for (int d = 0; d < 3; ++d) x[d] = xyz[(size_t)sample * 3 + d];
        const Cell cell = locate(G, x);
        const bool inside = valid && cell.inside;
        half8 xb[kSteps0];
        feature_operands(G, cell, inside, k0, view, c, h, xbuf[threadIdx.x >> 6], xb);
#pragma unroll
        for (int s = 0; s < kSteps0; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                rw[(size_t)(kRowX + 32 * s + 8 * h + j) * ld + col] = xb[s][j];
        half4 a1[kTiles], a2[kTiles];
        float out[kOut];
        mlp_tile(W, xb, c, h, a1, a2, out);
        // ---- sigmoid backward in f16 on the f16 albedo; rows outside the box
        // never reached the MLP: no gradient
        half_t go[kOut];
#pragma unroll
        for (int k = 0; k < kOut; ++k) {
            float g = 0.0f;
            if (inside) {
                // the gradient of the f16 albedo arrives in f16
                const float ga = (float)(half_t)(float)grad_albedo[(size_t)sample * 3 + k];
                const float av = (float)(half_t)sigmoidf(out[k]);
                g = ga * (1.0f - av) * av;
            }
            go[k] = (half_t)g;
            if (h == 0) rw[(size_t)(kRowGo + k) * ld + col] = go[k];
        }
        // ---- dL/d(a2) = go @ W2 as an f16 GEMM output, ReLU mask
        half4 g2[kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = 16 * t + 4 * h + r;
                float s = (float)go[0] * W.w2f[0][n];
                s = fmaf((float)go[1], W.w2f[1][n], s);
                s = fmaf((float)go[2], W.w2f[2][n], s);
                g2[t][r] = (float)a2[t][r] > 0.0f ? (half_t)s : (half_t)0.0f;
                rw[(size_t)(kRowA2 + n) * ld + col] = a2[t][r];
                rw[(size_t)(kRowG2 + n) * ld + col] = g2[t][r];
            }
        }
        // ---- dL/d(a1) = g2 @ W1 as an f16 GEMM output, ReLU mask
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
            f4 acc = f4{0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc = mfma(a_perm(W.w1t, kLdH, 16 * t + c, s, h), b_tiles(g2, s), acc);
            const half4 gh = __builtin_convertvector(acc, half4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = 16 * t + 4 * h + r;
                rw[(size_t)(kRowA1 + n) * ld + col] = a1[t][r];
                rw[(size_t)(kRowG1 + n) * ld + col] =
                    (float)a1[t][r] > 0.0f ? gh[r] : (half_t)0.0f;
            }
        }
    }
}

// ------------------------------------------------------------------ weight gradients
// One wave per (job, split): job = 16 output rows of one Linear against all of
// its input columns, split = a range of 32-sample k-steps (resmlp.hip's
// k_resmlp_wgrad).  A[i = c][k = 8 h + j] is the output gradient of row
// row0 + c at samples 32 ks + 8 h + j, B[k][col = c] the input of column
// 16 tm + c at the same samples; the bias is the product with a ones operand.
// Jobs: 0..7 the first Linear, 8..15 the second, 16 the output layer.
constexpr int kJobs = 17;

// One chunk's product of wave (job, split) out of `splits`: images of row
// stride Mp, mp / 32 k-steps.
__device__ __forceinline__ void wgrad_chunk(const half_t *__restrict__ rows, uint32_t Mp,
                                            uint32_t mp, uint32_t split, uint32_t splits,
                                            uint32_t dim0, float *__restrict__ partial) {
    const int job = blockIdx.x, lane = threadIdx.x, c = lane & 15, h = lane >> 4;
    const uint32_t ksteps = mp / 32u;
    const uint32_t per = ceil_div(ksteps, splits);
    const uint32_t k0 = split * per < ksteps ? split * per : ksteps;
    const uint32_t k1 = k0 + per < ksteps ? k0 + per : ksteps;
    const half_t *Gr, *B;
    int ntile, nrow, ld, tw, row0;  // column tiles, live rows, out stride (= columns), tensor
    if (job < 8) {
        row0 = 16 * job, Gr = rows + (size_t)kRowG1 * Mp, B = rows + (size_t)kRowX * Mp;
        ntile = (int)ceil_div(dim0, 16u), nrow = 16, ld = (int)dim0, tw = 0;
    } else if (job < 16) {
        row0 = 16 * (job - 8), Gr = rows + (size_t)kRowG2 * Mp, B = rows + (size_t)kRowA1 * Mp;
        ntile = kTiles, nrow = 16, ld = kHid, tw = 2;
    } else {
        row0 = 0, Gr = rows + (size_t)kRowGo * Mp, B = rows + (size_t)kRowA2 * Mp;
        ntile = kTiles, nrow = kOut, ld = kHid, tw = 4;
    }
    f4 acc[kTiles + 1];
#pragma unroll
    for (int i = 0; i < kTiles + 1; ++i) acc[i] = f4{0, 0, 0, 0};
    const half_t one = (half_t)1.0f;
    const half8 ones8 = half8{one, one, one, one, one, one, one, one};
    for (uint32_t ks = k0; ks < k1; ++ks) {
        const size_t col = (size_t)32 * ks + 8 * h;
        half8 a = half8{};
        if (c < nrow) a = *reinterpret_cast<const half8 *>(Gr + (size_t)(row0 + c) * Mp + col);
#pragma unroll
        for (int tm = 0; tm < kTiles; ++tm)
            if (tm < ntile)
                acc[tm] = mfma(a, *reinterpret_cast<const half8 *>(B + (size_t)(16 * tm + c) * Mp + col),
                               acc[tm]);
        acc[kTiles] = mfma(a, ones8, acc[kTiles]);
    }
    // accumulator element r of lane (c, h): row 4 h + r, column c of the tile;
    // every partial entry is written by exactly one lane of one job
    float *out = partial + (size_t)split * t_offset(kTensors, dim0);
    const uint32_t offw = t_offset(tw, dim0), offb = t_offset(tw + 1, dim0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * h + r;
        if (row >= nrow) continue;
#pragma unroll
        for (int tm = 0; tm < kTiles; ++tm)
            if (tm < ntile && 16 * tm + c < ld)
                out[offw + (row0 + row) * ld + 16 * tm + c] = acc[tm][r];
        if (c == 0) out[offb + row0 + row] = acc[kTiles][r];
    }
}

__global__ __launch_bounds__(64) void k_voxel_wgrad(const half_t *__restrict__ rows, uint32_t Mp,
                                                    uint32_t dim0, float *__restrict__ partial) {
    wgrad_chunk(rows, Mp, Mp, blockIdx.y, gridDim.y, dim0, partial);
}

// The chunks of the device-count backward: m0, the padded row count and the
// splits of chunk `chunk` of Me effective rows (the host loop's values), the
// row stride of its images (the capacity's).
struct Chunk {
    uint32_t mp, splits, ld;
};
__device__ __forceinline__ Chunk chunk_of(uint32_t chunk, uint32_t Me, uint32_t cap) {
    const uint32_t m0 = chunk * kChunk, left = cap - m0;
    Chunk k;
    k.mp = padded(Me - m0 < kChunk ? Me - m0 : kChunk);
    k.splits = k.mp / 32u < kSplits ? k.mp / 32u : kSplits;
    k.ld = padded(left < kChunk ? left : kChunk);
    return k;
}

// Device count: wave (job, split) takes its share of every live chunk in turn;
// chunk c has kSplits partial images at partial + c * kSplits * total.
__global__ __launch_bounds__(64) void k_voxel_wgrad_dev(const half_t *__restrict__ rows,
                                                        uint32_t cap,
                                                        const int32_t *__restrict__ m_dev,
                                                        uint32_t align, uint32_t dim0,
                                                        float *__restrict__ partial) {
    const uint32_t Me = effective_rows(live_rows(m_dev, cap), cap, align);
    const size_t total = t_offset(kTensors, dim0);
    for (uint32_t chunk = 0; chunk * kChunk < Me; ++chunk) {
        const Chunk k = chunk_of(chunk, Me, cap);
        if (blockIdx.y >= k.splits) continue;
        wgrad_chunk(rows + (size_t)kRows * kChunk * chunk, k.ld, k.mp, blockIdx.y, k.splits, dim0,
                    partial + (size_t)chunk * kSplits * total);
    }
}

// Fixed-order sums into the f32 gradients: a block takes 64 parameters; its
// 16 part-lanes add the parts p = j, j + 16, ... in that order, then lane
// j = 0 adds the 16 lane sums in order (as resmlp.hip's k_resmlp_reduce).
__global__ __launch_bounds__(1024) void k_voxel_reduce(const float *__restrict__ partial,
                                                       uint32_t splits, uint32_t dim0, GPtrs Gp,
                                                       int accumulate) {
    __shared__ float lane_sum[16][64];
    const int col = threadIdx.x & 63, j = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 64u + col, total = t_offset(kTensors, dim0);
    int ti = 0;
    uint32_t k = 0;
    float s = 0.0f;
    if (i < total) {
        uint32_t off = 0;
        for (int t = 0; t < kTensors; ++t) {
            const uint32_t sz = t_size(t, dim0);
            if (i >= off && i < off + sz) ti = t, k = i - off;
            off += sz;
        }
        for (uint32_t p = j; p < splits; p += 16) s += partial[(size_t)p * total + i];
    }
    lane_sum[j][col] = s;
    __syncthreads();
    if (j != 0 || i >= total) return;
    s = 0.0f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += lane_sum[q][col];
    float *dst = Gp.p[ti];
    dst[k] = accumulate ? dst[k] + s : s;
}

// Device count: the chunks' sums in chunk order, each formed as above and
// added to the running f32 value as the host loop's launches add it in memory.
// No live chunk: zeros, or nothing with accumulate.
__global__ __launch_bounds__(1024) void k_voxel_reduce_dev(const float *__restrict__ partial,
                                                           uint32_t cap,
                                                           const int32_t *__restrict__ m_dev,
                                                           uint32_t align, uint32_t dim0, GPtrs Gp,
                                                           int accumulate) {
    __shared__ float lane_sum[16][64];
    const uint32_t Me = effective_rows(live_rows(m_dev, cap), cap, align);
    const int col = threadIdx.x & 63, j = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 64u + col, total = t_offset(kTensors, dim0);
    int ti = 0;
    uint32_t k = 0;
    if (i < total) {
        uint32_t off = 0;
        for (int t = 0; t < kTensors; ++t) {
            const uint32_t sz = t_size(t, dim0);
            if (i >= off && i < off + sz) ti = t, k = i - off;
            off += sz;
        }
    }
    const bool writer = j == 0 && i < total;
    float *dst = Gp.p[ti];
    float v = 0.0f;
    if (writer && accumulate) v = dst[k];
    for (uint32_t chunk = 0; chunk * kChunk < Me; ++chunk) {  // block-uniform
        const uint32_t splits = chunk_of(chunk, Me, cap).splits;
        const float *part = partial + (size_t)chunk * kSplits * total;
        float s = 0.0f;
        if (i < total)
            for (uint32_t p = j; p < splits; p += 16) s += part[(size_t)p * total + i];
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

// ------------------------------------------------------------------ normal
template <bool kDev>
__global__ __launch_bounds__(256) void k_voxel_normal(const float *__restrict__ xyz,
                                                      const float *__restrict__ density, Geom G,
                                                      float *__restrict__ normal, uint32_t M,
                                                      const int32_t *__restrict__ m_dev) {
    if constexpr (kDev) M = live_rows(m_dev, M);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= M) return;
    const float x[3] = {xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2]};
    const Cell c = locate(G, x);
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (c.inside) {
        float raw;
        density_normal(G, c, corners(G, c), density, raw, n);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) normal[(size_t)i * 3 + d] = n[d];
}

// ------------------------------------------------------------------ host side
// scratch layout for a chunk of mp (padded) samples; both sizes are multiples
// of 16 bytes
struct Scratch {
    size_t rows, partial, total;
};
static Scratch scratch_layout(uint32_t mp, uint32_t dim0) {
    Scratch s;
    size_t o = 0;
    s.rows = o, o += (size_t)kRows * mp * sizeof(half_t);
    s.partial = o, o += ceil_div((size_t)kSplits * t_offset(kTensors, dim0) * sizeof(float),
                                 (size_t)16) * 16;
    s.total = o;
    return s;
}

static uint32_t persistent_blocks(uint32_t tiles, int waves) {
    const uint32_t want = ceil_div(tiles, (uint32_t)waves), cus = device_cus();
    const uint32_t n = want < cus ? want : cus;
    return n ? n : 1u;
}

}  // namespace vx
}  // namespace dfhip

using namespace dfhip;
using namespace dfhip::vx;

// m_dev NULL: M rows; else M is the capacity and *m_dev the live count
static int field_forward(const char *name, const float *xyz, const float *density,
                         const float *k0, uint32_t Nx, uint32_t Ny, uint32_t Nz, uint32_t C,
                         uint32_t pos_freqs, const float *view, uint32_t view_dim,
                         const float *box, float bound, float act_shift,
                         const float *const *params, float *sigma, void *albedo, uint32_t M,
                         const int32_t *m_dev, dfhip_stream_t stream) {
    Geom G;
    if (!geometry(name, Nx, Ny, Nz, C, pos_freqs, view_dim, box, bound, act_shift,
                  albedo != nullptr, G))
        return DFHIP_EINVAL;
    Ptrs P = {};
    if (albedo && !gather(name, params, P)) return DFHIP_EINVAL;
    if (M == 0) return DFHIP_OK;
    if (!xyz || !density || !sigma || (albedo && (!k0 || (view_dim && !view)))) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    if (!albedo) {
        if (m_dev)
            k_voxel_sigma<true><<<ceil_div(M, 256u), 256, 0, s>>>(xyz, density, G, sigma, M, m_dev);
        else
            k_voxel_sigma<false><<<ceil_div(M, 256u), 256, 0, s>>>(xyz, density, G, sigma, M,
                                                                   nullptr);
        return check_launch(name);
    }
    const uint32_t tiles = ceil_div(M, 16u);
    if (m_dev)
        k_voxel_fwd_dev<<<persistent_blocks(tiles, kWaves), 64 * kWaves, 0, s>>>(
            xyz, density, k0, view, G, P, sigma, (half_t *)albedo, M, m_dev);
    else
        k_voxel_fwd<<<persistent_blocks(tiles, kWaves), 64 * kWaves, 0, s>>>(
            xyz, density, k0, view, G, P, sigma, (half_t *)albedo, M, tiles);
    return check_launch(name);
}

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

extern "C" int dfhip_voxel_field_forward(const float *xyz, const float *density, const float *k0,
                                         uint32_t Nx, uint32_t Ny, uint32_t Nz, uint32_t C,
                                         uint32_t pos_freqs, const float *view, uint32_t view_dim,
                                         const float *box, float bound, float act_shift,
                                         const float *const *params, float *sigma, void *albedo,
                                         uint32_t M, dfhip_stream_t stream) {
    return field_forward("voxel_field_forward", xyz, density, k0, Nx, Ny, Nz, C, pos_freqs, view,
                         view_dim, box, bound, act_shift, params, sigma, albedo, M, nullptr,
                         stream);
}

extern "C" int dfhip_voxel_field_forward_dev(const float *xyz, const float *density,
                                             const float *k0, uint32_t Nx, uint32_t Ny,
                                             uint32_t Nz, uint32_t C, uint32_t pos_freqs,
                                             const float *view, uint32_t view_dim,
                                             const float *box, float bound, float act_shift,
                                             const float *const *params, float *sigma,
                                             void *albedo, uint32_t cap, const int32_t *m_dev,
                                             uint32_t align, dfhip_stream_t stream) {
    const char *name = "voxel_field_forward_dev";
    if (!device_count(name, cap, m_dev, align)) return DFHIP_EINVAL;
    return field_forward(name, xyz, density, k0, Nx, Ny, Nz, C, pos_freqs, view, view_dim, box,
                         bound, act_shift, params, sigma, albedo, cap, m_dev, stream);
}

extern "C" uint64_t dfhip_voxel_field_backward_scratch(uint32_t M, uint32_t dim0) {
    if (dim0 > (uint32_t)kInPad) dim0 = kInPad;
    return (uint64_t)scratch_layout(padded(M < kChunk ? M : kChunk), dim0).total;
}

// Device count: the images of every chunk of the capacity (616 rows x 2 bytes
// per padded sample), then kSplits partial images per chunk.
static Scratch scratch_layout_dev(uint32_t cap, uint32_t dim0) {
    Scratch s;
    size_t o = 0;
    s.rows = o, o += (size_t)kRows * ceil_div((size_t)cap, (size_t)32) * 32 * sizeof(half_t);
    s.partial = o, o += ceil_div((size_t)ceil_div(cap, kChunk) * kSplits *
                                     t_offset(kTensors, dim0) * sizeof(float), (size_t)16) * 16;
    s.total = o ? o : 16;
    return s;
}

extern "C" uint64_t dfhip_voxel_field_backward_dev_scratch(uint32_t cap, uint32_t dim0) {
    if (dim0 > (uint32_t)kInPad) dim0 = kInPad;
    return (uint64_t)scratch_layout_dev(cap, dim0).total;
}

// The checks both backward entries share; fills G, P, Gp.
static int backward_args(const char *name, uint32_t Nx, uint32_t Ny, uint32_t Nz, uint32_t C,
                         uint32_t pos_freqs, uint32_t view_dim, const float *box, float bound,
                         const float *const *params, int grad_albedo_dtype, float *const *grads,
                         Geom &G, Ptrs &P, GPtrs &Gp) {
    if (!geometry(name, Nx, Ny, Nz, C, pos_freqs, view_dim, box, bound, 0.0f, true, G))
        return DFHIP_EINVAL;
    if (!gather(name, params, P)) return DFHIP_EINVAL;
    if (!grads) {
        set_error("%s: null gradient list", name);
        return DFHIP_EINVAL;
    }
    for (int t = 0; t < kTensors; ++t) {
        if (!grads[t]) {
            set_error("%s: gradient %d is null", name, t);
            return DFHIP_EINVAL;
        }
        Gp.p[t] = grads[t];
    }
    if (grad_albedo_dtype != DFHIP_F16 && grad_albedo_dtype != DFHIP_F32) {
        set_error("%s: grad_albedo dtype must be f16 or f32", name);
        return DFHIP_EDTYPE;
    }
    return DFHIP_OK;
}

extern "C" int dfhip_voxel_field_backward(const float *xyz, const float *k0, uint32_t Nx,
                                          uint32_t Ny, uint32_t Nz, uint32_t C,
                                          uint32_t pos_freqs, const float *view,
                                          uint32_t view_dim, const float *box, float bound,
                                          const float *const *params, const void *grad_albedo,
                                          int grad_albedo_dtype, uint32_t M, void *scratch,
                                          float *const *grads, int accumulate,
                                          dfhip_stream_t stream) {
    const char *name = "voxel_field_backward";
    Geom G;
    Ptrs P;
    GPtrs Gp;
    if (int rc = backward_args(name, Nx, Ny, Nz, C, pos_freqs, view_dim, box, bound, params,
                               grad_albedo_dtype, grads, G, P, Gp))
        return rc;
    hipStream_t s = as_stream(stream);
    if (M == 0) {
        if (!accumulate)
            for (int t = 0; t < kTensors; ++t)
                (void)hipMemsetAsync(Gp.p[t], 0, t_size(t, G.dim0) * sizeof(float), s);
        return check_launch(name);
    }
    if (!scratch || ((uintptr_t)scratch & 15u)) {
        set_error("%s: scratch must be a 16-byte aligned buffer of "
                  "dfhip_voxel_field_backward_scratch(M, dim0) bytes", name);
        return DFHIP_EINVAL;
    }
    if (!xyz || !k0 || !grad_albedo || (view_dim && !view)) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    char *base = (char *)scratch;
    const size_t ga_size = grad_albedo_dtype == DFHIP_F16 ? 2 : 4;
    const uint32_t total = t_offset(kTensors, G.dim0);
    for (uint32_t m0 = 0; m0 < M; m0 += kChunk) {
        const uint32_t m = M - m0 < kChunk ? M - m0 : kChunk;
        const uint32_t mp = padded(m), tiles = mp / 16u;
        const Scratch L = scratch_layout(mp, G.dim0);
        half_t *rows = (half_t *)(base + L.rows);
        float *partial = (float *)(base + L.partial);
        const float *x = xyz + (size_t)m0 * 3;
        const void *ga = (const char *)grad_albedo + (size_t)m0 * 3 * ga_size;
        const uint32_t nblk = persistent_blocks(tiles, kBwdWaves);
        if (grad_albedo_dtype == DFHIP_F16)
            k_voxel_bwd_act<half_t, false><<<nblk, 64 * kBwdWaves, 0, s>>>(
                x, k0, view, G, P, (const half_t *)ga, m, tiles, mp, rows, nullptr, 1u);
        else
            k_voxel_bwd_act<float, false><<<nblk, 64 * kBwdWaves, 0, s>>>(
                x, k0, view, G, P, (const float *)ga, m, tiles, mp, rows, nullptr, 1u);
        const uint32_t splits = mp / 32u < kSplits ? mp / 32u : kSplits;
        k_voxel_wgrad<<<dim3(kJobs, splits), 64, 0, s>>>(rows, mp, G.dim0, partial);
        k_voxel_reduce<<<ceil_div(total, 64u), 1024, 0, s>>>(partial, splits, G.dim0, Gp,
                                                            (accumulate || m0 > 0) ? 1 : 0);
    }
    return check_launch(name);
}

extern "C" int dfhip_voxel_field_backward_dev(const float *xyz, const float *k0, uint32_t Nx,
                                              uint32_t Ny, uint32_t Nz, uint32_t C,
                                              uint32_t pos_freqs, const float *view,
                                              uint32_t view_dim, const float *box, float bound,
                                              const float *const *params,
                                              const void *grad_albedo, int grad_albedo_dtype,
                                              uint32_t cap, const int32_t *m_dev, uint32_t align,
                                              void *scratch, float *const *grads, int accumulate,
                                              dfhip_stream_t stream) {
    const char *name = "voxel_field_backward_dev";
    Geom G;
    Ptrs P;
    GPtrs Gp;
    if (int rc = backward_args(name, Nx, Ny, Nz, C, pos_freqs, view_dim, box, bound, params,
                               grad_albedo_dtype, grads, G, P, Gp))
        return rc;
    if (!device_count(name, cap, m_dev, align)) return DFHIP_EINVAL;
    if (!scratch || ((uintptr_t)scratch & 15u)) {
        set_error("%s: scratch must be a 16-byte aligned buffer of "
                  "dfhip_voxel_field_backward_dev_scratch(cap, dim0) bytes", name);
        return DFHIP_EINVAL;
    }
    if (cap && (!xyz || !k0 || !grad_albedo || (view_dim && !view))) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    const Scratch L = scratch_layout_dev(cap, G.dim0);
    half_t *rows = (half_t *)((char *)scratch + L.rows);
    float *partial = (float *)((char *)scratch + L.partial);
    const uint32_t total = t_offset(kTensors, G.dim0);
    if (cap) {
        // launch shapes of the capacity; the kernels stop at the live chunks
        const uint32_t tiles = ceil_div(cap, 32u) * 2u;
        const uint32_t nblk = persistent_blocks(tiles, kBwdWaves);
        if (grad_albedo_dtype == DFHIP_F16)
            k_voxel_bwd_act<half_t, true><<<nblk, 64 * kBwdWaves, 0, s>>>(
                xyz, k0, view, G, P, (const half_t *)grad_albedo, cap, tiles, 0u, rows, m_dev,
                align);
        else
            k_voxel_bwd_act<float, true><<<nblk, 64 * kBwdWaves, 0, s>>>(
                xyz, k0, view, G, P, (const float *)grad_albedo, cap, tiles, 0u, rows, m_dev,
                align);
        const uint32_t first = padded(cap < kChunk ? cap : kChunk);
        const uint32_t splits = first / 32u < kSplits ? first / 32u : kSplits;
        k_voxel_wgrad_dev<<<dim3(kJobs, splits), 64, 0, s>>>(rows, cap, m_dev, align, G.dim0,
                                                             partial);
    }
    k_voxel_reduce_dev<<<ceil_div(total, 64u), 1024, 0, s>>>(partial, cap, m_dev, align, G.dim0,
                                                             Gp, accumulate ? 1 : 0);
    return check_launch(name);
}

// m_dev NULL: M rows; else M is the capacity and *m_dev the live count
static int field_normal(const char *name, const float *xyz, const float *density, uint32_t Nx,
                        uint32_t Ny, uint32_t Nz, const float *box, float bound, float act_shift,
                        float *normal, uint32_t M, const int32_t *m_dev, dfhip_stream_t stream) {
    Geom G;
    if (!geometry(name, Nx, Ny, Nz, 0u, 0u, 0u, box, bound, act_shift, false, G))
        return DFHIP_EINVAL;
    if (M == 0) return DFHIP_OK;
    if (!xyz || !density || !normal) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    if (m_dev)
        k_voxel_normal<true><<<ceil_div(M, 256u), 256, 0, as_stream(stream)>>>(xyz, density, G,
                                                                               normal, M, m_dev);
    else
        k_voxel_normal<false><<<ceil_div(M, 256u), 256, 0, as_stream(stream)>>>(xyz, density, G,
                                                                                normal, M, nullptr);
    return check_launch(name);
}

extern "C" int dfhip_voxel_normal(const float *xyz, const float *density, uint32_t Nx,
                                  uint32_t Ny, uint32_t Nz, const float *box, float bound,
                                  float act_shift, float *normal, uint32_t M,
                                  dfhip_stream_t stream) {
    return field_normal("voxel_normal", xyz, density, Nx, Ny, Nz, box, bound, act_shift, normal,
                        M, nullptr, stream);
}

extern "C" int dfhip_voxel_normal_dev(const float *xyz, const float *density, uint32_t Nx,
                                      uint32_t Ny, uint32_t Nz, const float *box, float bound,
                                      float act_shift, float *normal, uint32_t cap,
                                      const int32_t *m_dev, uint32_t align,
                                      dfhip_stream_t stream) {
    const char *name = "voxel_normal_dev";
    if (!device_count(name, cap, m_dev, align)) return DFHIP_EINVAL;
    return field_normal(name, xyz, density, Nx, Ny, Nz, box, bound, act_shift, normal, cap, m_dev,
                        stream);
}
