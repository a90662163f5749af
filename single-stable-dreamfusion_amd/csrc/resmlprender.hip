// Fused persistent inference renderer of the vanilla backbone for gfx950:
// occupancy-grid march + frequency-encoded residual MLP field + front-to-back
// compositing in ONE launch with a device work queue of rays
// (csrc/voxelrender.hip's design, with the field of csrc/resmlp.hip in place of
// the voxel field).  Albedo frames only: the shaded views' normal is the MLP's
// input gradient, whose transposed weights do not fit LDS beside the forward
// weights (resmlp.hip splits the two for the same reason).
//
// Behavioural spec: the reference's inference branch of run_cuda
// (nerf/renderer.py:496-532) with nerf/network.py:104-115 under fp16 autocast
// as the field: a host loop of march_rays -> field -> composite_rays ->
// compaction, one host sync per iteration.  As voxelrender.hip, this kernel is
// that loop at n_step = 1 with the same device functions in the same order:
//   * queue, refill, rm::march_step_ahead, the per-wave LDS stage with up to
//     kK pending samples per ray and the in-order compositing are
//     voxelrender.hip's k_render_voxel<kAlbedo> (render_common.h holds what the
//     files share);
//   * the field phase is k_resmlp_fwd<false>'s forward_tile, taken as its two
//     halves rs::enc_operand and rs::mlp_tiles on the staged positions, then
//     sigma = expf(h0 + gaussian(x)) in f32 and albedo = f16(sigmoid(h1..3));
//     lanes of a partial tile carry x = 0 and store nothing; a pass with no
//     staged sample runs no MLP.
//
// LDS: the f16 weights (rs::FwdW, 151,872 B) once per workgroup and the stage
// (2,560 B) per wave: four waves, 162,112 B of the CU's 163,840.  At one wave
// per SIMD a wave may hold 512 registers, so DFHIP_RESMLP_RENDER_TILES = 2
// takes two 16-sample tiles through every layer per weight operand and
// LayerNorm parameter read from LDS: half the LDS traffic per sample and a
// second, independent MFMA chain (DESIGN.md "Vanilla renderer" has the builds
// measured: 256 VGPRs + 211 AGPRs, no scratch).
#include "march_common.h"
#include "resmlp_common.h"
#include "render_common.h"

namespace dfhip {
namespace rr {

using rd::kAhead;
using rd::kAlbedo;
using rd::kBatch;
using rd::kK;

// waves per workgroup (they share one weight copy): the stages the weights
// leave room for, one wave per SIMD
constexpr int kWaves = 4;
// 16-sample tiles per weight operand read (1: the A/B build of DESIGN.md)
#ifndef DFHIP_RESMLP_RENDER_TILES
#define DFHIP_RESMLP_RENDER_TILES 2
#endif
constexpr int kNT = DFHIP_RESMLP_RENDER_TILES;
static_assert(kNT == 1 || kNT == 2, "one or two tiles per weight read");
static_assert(sizeof(rs::FwdW) + kWaves * sizeof(rd::StageT<kAlbedo>) <= 160 * 1024,
              "weights and stages must fit the CU's 160 KiB of LDS");

// NT tiles of staged samples [s0, s0 + 16 NT) through the field; the slot's
// words become (sigma, rg, b) as k_render_voxel<kAlbedo> leaves them.
template <int NT>
__device__ __forceinline__ void field_tiles(const rs::FwdW &W, rd::StageT<kAlbedo> &S,
                                            uint32_t s0, uint32_t total, int c, int h) {
    float x0[NT], x1[NT], x2[NT];
    bool valid[NT];
    rs::half8 xb[NT][2];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const uint32_t s = s0 + 16 * n + c;
        valid[n] = s < total;
        x0[n] = valid[n] ? S.pos[3 * s] : 0.0f;
        x1[n] = valid[n] ? S.pos[3 * s + 1] : 0.0f;
        x2[n] = valid[n] ? S.pos[3 * s + 2] : 0.0f;
#pragma unroll
        for (int q = 0; q < 2; ++q) xb[n][q] = rs::enc_operand(x0[n], x1[n], x2[n], q, h);
    }
    float ho[NT][4];
    rs::mlp_tiles<NT>(W, xb, c, h, ho, nullptr, nullptr, 0, 0);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        if (!valid[n] || h != 0) continue;
        // k_resmlp_fwd's heads (every lane group holds all four outputs)
        const uint32_t s = s0 + 16 * n + c;
        const float xs[3] = {x0[n], x1[n], x2[n]};
        const float sigma = expf(ho[n][0] + fm::gaussian(xs));
        const half_t a0 = (half_t)rs::sigmoidf(ho[n][1]), a1 = (half_t)rs::sigmoidf(ho[n][2]),
                     a2 = (half_t)rs::sigmoidf(ho[n][3]);
        S.pos[3 * s] = sigma;
        S.pos[3 * s + 1] = __uint_as_float(rd::pack_h2(a0, a1));
        S.pos[3 * s + 2] = __uint_as_float(rd::pack_h2(a2, (half_t)0.0f));
    }
}

__global__ __launch_bounds__(64 * kWaves) void k_render_resmlp(
    uint32_t N, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
    const float *__restrict__ nears, const float *__restrict__ fars,
    const float *__restrict__ noises, rm::MarchConsts k, const uint8_t *__restrict__ grid,
    uint32_t max_samples, float T_thresh, rs::Ptrs P, float *__restrict__ weights_sum,
    float *__restrict__ depth, float *__restrict__ image, uint32_t *__restrict__ work,
    const int32_t *__restrict__ order, uint32_t chunk_log2, uint32_t tile_w) {
    __shared__ rs::FwdW W;
    __shared__ rd::StageT<kAlbedo> stages[kWaves];
    rs::load_fwd_weights(W, P);
    __syncthreads();
    rd::StageT<kAlbedo> &S = stages[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    // queue positions: N, or whole chunks of the order
    const uint32_t nchunks = ceil_div(N, 1u << chunk_log2);
    const uint32_t Nq = order ? nchunks << chunk_log2 : N;
    // mirrored halves: in blocks of G chunk positions (G = the grid's waves),
    // grab g takes the first half of chunk g and the second half of chunk
    // G-1-g (none for single-ray chunks); render.hip's
    const uint32_t G = order && chunk_log2 ? gridDim.x * kWaves : 0u;

    int ray = -1;
    bool exhausted = false;
    rm::Ray r{};
    // march state: t, last_t (the march loop's), tc (rays_t: near + the f32
    // sum of deltas[1], where the loop restarts after every sample), whether
    // the march reached far, and the samples marched for this ray
    float t = 0.0f, far = 0.0f, last_t = 0.0f, tc = 0.0f;
    bool at_far = false;
    uint32_t marched = 0;
    // compositing state
    float ws = 0.0f, dp = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    uint32_t taken = 0;
    bool finished = false;  // T < T_thresh or max_samples: later samples are dropped
    uint32_t samples = 0;   // per-lane count of evaluated samples (stats)

    while (true) {
        // ---- refill lanes without a ray from the global queue
        const bool need = ray < 0 && !exhausted;
        const uint64_t needm = __ballot(need);
        if (needm) {
            const int leader = __ffsll((unsigned long long)needm) - 1;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&work[0], (uint32_t)__popcll(needm));
            base = __shfl(base, leader);
            if (need) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
                    (uint32_t)(needm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)needm, 0u));
                const uint32_t q = base + rank;
                // the queue's q-th ray: ray q, or ray j of chunk order[q >> cl];
                // an id >= N (the partial last chunk, or an order entry that
                // is not a chunk index: checked before the shift) is skipped,
                // never read or written
                uint32_t id = N;
                if (q < Nq) {
                    if (order) {
                        const uint32_t j = q & ((1u << chunk_log2) - 1u);
                        uint32_t pos = q >> chunk_log2;
                        if (G && (j >> (chunk_log2 - 1))) {
                            const uint32_t b0 = pos / G * G;
                            pos = b0 + min(G, nchunks - b0) - 1u - (pos - b0);
                        }
                        const uint32_t ch = (uint32_t)order[pos];
                        if (ch < nchunks) id = rd::chunk_ray(ch, j, chunk_log2, tile_w);
                    } else {
                        id = q;
                    }
                }
                if (q >= Nq) {
                    exhausted = true;
                } else if (id < N) {
                    ray = (int)id;
                    r = rm::load_ray(rays_o + 3 * (size_t)id, rays_d + 3 * (size_t)id);
                    // rays_t starts at the near plane (renderer.py:509); the
                    // perturbation applies to the first march only (:522)
                    tc = nears[id];
                    far = fars[id];
                    t = tc;
                    if (noises)
                        t = fmaf(rm::clampf(t * k.dt_gamma, k.dt_min, k.dt_max), noises[id], t);
                    last_t = t;
                    at_far = false;
                    marched = 0;
                    ws = dp = cr = cg = cb = 0.0f;
                    taken = 0;
                    finished = false;
                }
            }
        }
        // done when no lane holds a ray and the queue is dry for all (a lane
        // whose queue entry was skipped refills next round)
        if (__ballot(ray >= 0 || !exhausted) == 0) break;

        // ---- march ahead: every lane takes one march step per iteration and
        // stages each sample it finds, until the wave has a batch of kBatch
        // samples or no lane may march (at far, kK samples pending, or
        // max_samples marched); samples past a ray's termination are dropped
        // by the compositing
        uint32_t count = 0, npend = 0;
        rd::PendSlots pslots;  // slots of the pending samples
        while (true) {
            const bool can = ray >= 0 && !at_far && !finished && npend < (uint32_t)kK &&
                             marched < max_samples;
            if (__ballot(can) == 0) break;
            bool emit = false;
            float px[3], pdt = 0.0f, dl = 0.0f;
            if (can) {
                const int st =
                    rm::march_step_ahead<kAhead>(k, r, grid, t, last_t, far, px, pdt, dl);
                if (st == 2) {
                    at_far = true;
                } else if (st == 1) {
                    emit = true;
                    tc += dl;
                    t = tc;
                    last_t = tc;
                    ++marched;
                }
            }
            const uint64_t em = __ballot(emit);
            if (emit) {
                const uint32_t slot =
                    count + __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u));
                S.pos[3 * slot] = px[0];
                S.pos[3 * slot + 1] = px[1];
                S.pos[3 * slot + 2] = px[2];
                S.dt[slot] = pdt;
                S.tc[slot] = tc;
                pslots.put(npend, slot);
                ++npend;
            }
            count += (uint32_t)__popcll(em);
            if (count >= (uint32_t)kBatch) break;
        }
        fm::wave_lds_sync();

        // ---- field over the staged samples: sample c = lane & 15 of a tile,
        // lane group h.  total is wave-uniform; a pass whose second tile would
        // be empty takes one tile, an empty batch none
        const uint32_t total = count;
        {
            const int c = lane & 15, h = lane >> 4;
            uint32_t s0 = 0;
            if constexpr (kNT == 2) {
                for (; s0 + 16u < total; s0 += 32u) {
                    // weights are re-read from LDS every pass (k_resmlp_fwd's idiom)
                    asm volatile("" ::: "memory");
                    field_tiles<2>(W, S, s0, total, c, h);
                }
            }
            for (; s0 < total; s0 += 16u) {
                asm volatile("" ::: "memory");
                field_tiles<1>(W, S, s0, total, c, h);
            }
        }
        fm::wave_lds_sync();

        // ---- composite each ray's staged samples in order (k_composite_infer,
        // raymarching.cu:848-873); a ray retires on T < T_thresh or
        // max_samples, or when its march reached far with nothing pending
        if (ray >= 0) {
            for (uint32_t q = 0; q < npend && !finished; ++q) {
                const uint32_t slot = pslots.get(q);
                const float sigma = S.pos[3 * slot];
                const uint32_t rg = __float_as_uint(S.pos[3 * slot + 1]);
                const uint32_t bz = __float_as_uint(S.pos[3 * slot + 2]);
                const float alpha = 1.0f - __expf(-sigma * S.dt[slot]);
                const float T = 1.0f - ws;
                const float w = alpha * T;
                ws += w;
                dp = fmaf(w, S.tc[slot], dp);
                cr = fmaf(w, rd::lo_h(rg), cr);
                cg = fmaf(w, rd::hi_h(rg), cg);
                cb = fmaf(w, rd::lo_h(bz), cb);
                ++taken;
                ++samples;
                if (T < T_thresh || taken >= max_samples) finished = true;
            }
            if (finished || at_far || marched >= max_samples) {
                weights_sum[ray] = ws;
                depth[ray] = dp;
                image[3 * (size_t)ray] = cr;
                image[3 * (size_t)ray + 1] = cg;
                image[3 * (size_t)ray + 2] = cb;
                ray = -1;
            }
        }
        fm::wave_lds_sync();
    }
    uint32_t tot = samples;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
    // stats: composited samples (64-bit, low / high words)
    if (lane == 0 && tot) {
        const uint32_t old = atomicAdd(&work[1], tot);
        if (old + tot < old) atomicAdd(&work[2], 1u);
    }
}

}  // namespace rr
}  // namespace dfhip

using namespace dfhip;

extern "C" int dfhip_resmlp_render_rays_infer(
    uint32_t N, const float *rays_o, const float *rays_d, const float *nears, const float *fars,
    const float *noises, float bound, float dt_gamma, uint32_t max_steps, uint32_t C,
    uint32_t H, const uint8_t *grid, float T_thresh, const float *const *params,
    float *weights_sum, float *depth, float *image, uint32_t *work, const int32_t *order,
    uint32_t chunk_log2, uint32_t tile_w, dfhip_stream_t stream) {
    const char *name = "resmlp_render_rays_infer";
    if (order && tile_w && (chunk_log2 != 6 || tile_w % 8 || N % (8 * tile_w))) {
        set_error("%s: tile chunks need chunk_log2 6, tile_w a multiple of 8 and N of 8 tile_w "
                  "(got chunk_log2 %u, tile_w %u, N %u)", name, chunk_log2, tile_w, N);
        return DFHIP_EINVAL;
    }
    if (order && (chunk_log2 > 16 || N > 0xFFFFFFFFu - (1u << chunk_log2))) {
        set_error("%s: chunk_log2 must be <= 16 and N + 2^chunk_log2 < 2^32 (got %u, N=%u)",
                  name, chunk_log2, N);
        return DFHIP_EINVAL;
    }
    if (C < 1 || C > 16 || H < 2 || H > 1024 || max_steps == 0) {
        set_error("%s: invalid C=%u H=%u max_steps=%u", name, C, H, max_steps);
        return DFHIP_EINVAL;
    }
    if (!params) {
        set_error("%s: null parameter list", name);
        return DFHIP_EINVAL;
    }
    rs::Ptrs P;
    for (int t = 0; t < rs::kTensors; ++t) {
        if (!params[t]) {
            set_error("%s: parameter %d is null", name, t);
            return DFHIP_EINVAL;
        }
        P.p[t] = params[t];
    }
    if (!work) {
        set_error("%s: work is null", name);
        return DFHIP_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(work, 0, 4 * sizeof(uint32_t), s) != hipSuccess) return check_launch(name);
    if (N == 0) return DFHIP_OK;  // no launch; the sample count reads 0
    if (!rays_o || !rays_d || !nears || !fars || !grid || !weights_sum || !depth || !image) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    const rm::MarchConsts k = rm::make_consts(bound, dt_gamma, max_steps, C, H);
    // persistent waves: as many workgroups as are co-resident on the chip (one
    // per CU: the weights fill its LDS); the queue balances the rays
    const uint32_t resident =
        resident_blocks((const void *)rr::k_render_resmlp, 64 * rr::kWaves, 1);
    const uint32_t want = ceil_div(N, 64u * (uint32_t)rr::kWaves);
    const uint32_t blocks = want < resident ? want : resident;
    rr::k_render_resmlp<<<blocks, 64 * rr::kWaves, 0, s>>>(
        N, rays_o, rays_d, nears, fars, noises, k, grid, max_steps, T_thresh, P, weights_sum,
        depth, image, work, order, chunk_log2, tile_w);
    return check_launch(name);
}
