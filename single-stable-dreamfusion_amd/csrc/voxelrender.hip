// Fused persistent inference renderer of the DVGO backbone for gfx950:
// occupancy-grid march + voxel field + front-to-back compositing in ONE
// launch with a device work queue of rays (csrc/render.hip's design, with the
// field of csrc/voxelfield.hip in place of the grid field).
//
// Behavioural spec: the reference's inference branch of run_cuda
// (nerf/renderer.py:496-532) with nerf/network.py:245-312 (NeRFNetwork_Kailu
// under fp16 autocast) as the field: a host loop of march_rays -> field
// (-> normal and the shading ops) -> composite_rays -> compaction, one host
// sync per iteration.  As render.hip, this kernel is that loop at n_step = 1
// (every sample restarts the march from the composited rays_t), with the same
// device functions in the same order:
//   * queue, refill, rm::march_step_ahead, the per-wave LDS stage with up to
//     kK pending samples per ray and the in-order compositing are render.hip's
//     (render_common.h holds what the two files share; the skeleton itself is
//     written out here, see DESIGN.md "Voxel renderer" for why);
//   * the field phase uses only what k_voxel_fwd / k_voxel_normal use from
//     voxel_common.h, so sigma, the f16 albedo and the normal carry their
//     bits: f32 map and interpolation, the feature row rounded to f16 in a
//     per-wave LDS image, v_mfma_f32_16x16x32_f16 with f32 accumulation, f16
//     between layers, raw = 0 and albedo 0.5 outside the box, no MLP for a
//     tile with no row inside it.
//
// Modes (template instances, no run-time branch):
//   albedo       16-sample tiles: lane group 0 takes the density, all four
//                fill the feature row, the MLP runs on MFMA;
//   lambertian   the same, and lane group 0 forms the closed-form normal from
//                the density's eight corners (vx::density_normal, the cell
//                and corners of the sample), normalises it as
//                NeRFNetwork._unit and takes shd::lambert<half_t> against the
//                light rounded to f16 once; colour = f16(albedo16 * lam16);
//   textureless  (lam16 on three channels) and
//   normal       ((n + 1) * 0.5 in f32, third channel in StageT<kNormal>::cz):
//                no k0 gathers, no feature row, no MLP and no weights in LDS;
//                one lane per staged sample, 64 samples per pass.
//
// LDS: the f16 weights (vx::FwdW, 66,880 B) once per workgroup, plus per wave
// the stage (2,560 B) and the feature-row image (3,328 B).  kColourWaves
// waves share one weight copy (DFHIP_VOXEL_RENDER_WAVES: 8 -> 113,984 B,
// 12 -> 137,536 B, 16 -> 161,088 B of the CU's 160 KiB).
#include "march_common.h"
#include "voxel_common.h"
#include "shade_common.h"
#include "render_common.h"

namespace dfhip {
namespace vr {

using rd::kAlbedo;
using rd::kAhead;
using rd::kBatch;
using rd::kK;
using rd::kLambertian;
using rd::kNormal;
using rd::kTextureless;

// waves per workgroup of the modes that keep the MLP's weights in LDS
#ifndef DFHIP_VOXEL_RENDER_WAVES
#define DFHIP_VOXEL_RENDER_WAVES 12
#endif
constexpr int kColourWaves = DFHIP_VOXEL_RENDER_WAVES;
constexpr int kPlainWaves = 4;  // textureless / normal: no weights to share
static_assert(kColourWaves >= 1 && kColourWaves <= 16, "1..16 waves per workgroup");

constexpr bool has_colour(int mode) { return mode == kAlbedo || mode == kLambertian; }
constexpr int waves_of(int mode) { return has_colour(mode) ? kColourWaves : kPlainWaves; }

// light: DEVICE f32 [3]; omr = 1 - ratio (rounded as dfhip_shading_forward's).
// Unused by the albedo mode.
struct ShadeArgs {
    const float *light;
    float ratio, omr;
};

// The MLP's LDS of the colour modes: weights and one feature-row image per wave.
template <bool COLOUR, int WAVES> struct FieldLds {
    vx::FwdW W;
    __attribute__((aligned(16))) half_t xbuf[WAVES][16 * vx::kLdI];
};
template <int WAVES> struct FieldLds<false, WAVES> {};

template <int MODE>
__global__ __launch_bounds__(64 * waves_of(MODE)) void k_render_voxel(
    uint32_t N, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
    const float *__restrict__ nears, const float *__restrict__ fars,
    const float *__restrict__ noises, rm::MarchConsts k, const uint8_t *__restrict__ grid,
    uint32_t max_samples, float T_thresh, const float *__restrict__ density,
    const float *__restrict__ k0, const float *__restrict__ view, vx::Geom Gm, vx::Ptrs P,
    float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image,
    uint32_t *__restrict__ work, const int32_t *__restrict__ order, uint32_t chunk_log2,
    uint32_t tile_w, ShadeArgs sh) {
    constexpr int kWaves = waves_of(MODE);
    constexpr bool kColour = has_colour(MODE);
    __shared__ FieldLds<kColour, kWaves> F;
    __shared__ rd::StageT<MODE> stages[kWaves];
    if constexpr (kColour) {
        vx::load_fwd_weights(F.W, P, Gm.dim0);
        __syncthreads();
    }
    rd::StageT<MODE> &S = stages[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    // the light as autocast holds it, rounded once per kernel
    float l16[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (MODE != kAlbedo && MODE != kNormal) {
#pragma unroll
        for (int d = 0; d < 3; ++d) l16[d] = shd::rnd<half_t>(sh.light[d]);
    }
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

        // ---- field over the staged samples
        const uint32_t total = count;
        if constexpr (kColour) {
            // 16 samples per MFMA tile: sample c = lane & 15, lane group h
            const int c = lane & 15, h = lane >> 4;
            half_t *xbuf = F.xbuf[threadIdx.x >> 6];
            const uint32_t tiles = ceil_div(total, 16u);
            for (uint32_t tile = 0; tile < tiles; ++tile) {
                // weights are re-read from LDS every tile (k_voxel_fwd's idiom)
                asm volatile("" ::: "memory");
                const uint32_t s = tile * 16 + c;
                const bool valid = s < total;
                float x[3] = {0.0f, 0.0f, 0.0f};
                if (valid)
#pragma unroll
                    for (int d = 0; d < 3; ++d) x[d] = S.pos[3 * s + d];
                const vx::Cell cell = vx::locate(Gm, x);
                const bool inside = valid && cell.inside;
                float sigma = 0.0f, lam = 0.0f;
                if (valid && h == 0) {
                    float raw = 0.0f;
                    if constexpr (MODE == kLambertian) {
                        float n[3] = {0.0f, 0.0f, 0.0f};
                        if (inside)
                            vx::density_normal(Gm, cell, vx::corners(Gm, cell), density, raw, n);
                        vx::unit_normal(n);
                        lam = shd::lambert<half_t>(n, l16, sh.ratio, sh.omr).lam16;
                    } else {
                        if (inside) raw = vx::trilinear(vx::corners(Gm, cell), density, 1u, 0u);
                    }
                    sigma = vx::activate(raw, Gm.act_shift);
                }
                float out[vx::kOut] = {0.0f, 0.0f, 0.0f};
                if (__ballot(inside) != 0ull) {  // wave-uniform
                    vx::half8 xb[vx::kSteps0];
                    vx::feature_operands(Gm, cell, inside, k0, view, c, h, xbuf, xb);
                    vx::half4 a1[vx::kTiles], a2[vx::kTiles];
                    vx::mlp_tile(F.W, xb, c, h, a1, a2, out);
                }
                if (valid && h == 0) {
                    // k_voxel_fwd's head; the slot's words become (sigma, rg, b)
                    half_t a[vx::kOut];
#pragma unroll
                    for (int q = 0; q < vx::kOut; ++q) {
                        a[q] = inside ? (half_t)vx::sigmoidf(out[q]) : (half_t)0.5f;
                        if constexpr (MODE == kLambertian)  // albedo * lambertian as f16 values
                            a[q] = (half_t)shd::rnd<half_t>((float)a[q] * lam);
                    }
                    S.pos[3 * s] = sigma;
                    S.pos[3 * s + 1] = __uint_as_float(rd::pack_h2(a[0], a[1]));
                    S.pos[3 * s + 2] = __uint_as_float(rd::pack_h2(a[2], (half_t)0.0f));
                }
            }
        } else {
            // density and normal only: one lane per staged sample
            for (uint32_t s = lane; s < total; s += 64u) {
                const float x[3] = {S.pos[3 * s], S.pos[3 * s + 1], S.pos[3 * s + 2]};
                const vx::Cell cell = vx::locate(Gm, x);
                float raw = 0.0f, n[3] = {0.0f, 0.0f, 0.0f};
                if (cell.inside)
                    vx::density_normal(Gm, cell, vx::corners(Gm, cell), density, raw, n);
                vx::unit_normal(n);
                S.pos[3 * s] = vx::activate(raw, Gm.act_shift);
                if constexpr (MODE == kNormal) {
                    // (normal + 1) / 2 in f32 (nerf/network_dvgo.py forward)
                    S.pos[3 * s + 1] = (n[0] + 1.0f) * 0.5f;
                    S.pos[3 * s + 2] = (n[1] + 1.0f) * 0.5f;
                    S.cz[s] = (n[2] + 1.0f) * 0.5f;
                } else {
                    const half_t l = (half_t)shd::lambert<half_t>(n, l16, sh.ratio, sh.omr).lam16;
                    S.pos[3 * s + 1] = __uint_as_float(rd::pack_h2(l, l));
                    S.pos[3 * s + 2] = __uint_as_float(rd::pack_h2(l, (half_t)0.0f));
                }
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
                if constexpr (MODE == kNormal) {  // f32 colours
                    cr = fmaf(w, __uint_as_float(rg), cr);
                    cg = fmaf(w, __uint_as_float(bz), cg);
                    cb = fmaf(w, S.cz[slot], cb);
                } else {
                    cr = fmaf(w, rd::lo_h(rg), cr);
                    cg = fmaf(w, rd::hi_h(rg), cg);
                    cb = fmaf(w, rd::lo_h(bz), cb);
                }
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

}  // namespace vr
}  // namespace dfhip

using namespace dfhip;

// shading: a dfhip_shading code; sh is read by the non-albedo ones
static int voxel_render(const char *name, uint32_t N, const float *rays_o, const float *rays_d,
                        const float *nears, const float *fars, const float *noises, float bound,
                        float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                        const uint8_t *grid, float T_thresh, const float *density,
                        const float *k0, uint32_t Nx, uint32_t Ny, uint32_t Nz,
                        uint32_t k0_channels, uint32_t pos_freqs, const float *view,
                        uint32_t view_dim, const float *box, float act_shift,
                        const float *const *params, float *weights_sum, float *depth,
                        float *image, uint32_t *work, const int32_t *order, uint32_t chunk_log2,
                        uint32_t tile_w, int shading, const vr::ShadeArgs &sh,
                        dfhip_stream_t stream) {
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
    const bool colour = vr::has_colour(shading);
    vx::Geom G;
    if (!vx::geometry(name, Nx, Ny, Nz, k0_channels, pos_freqs, view_dim, box, bound, act_shift,
                      colour, G))
        return DFHIP_EINVAL;
    vx::Ptrs P = {};
    if (colour && !vx::gather(name, params, P)) return DFHIP_EINVAL;
    if (!work) {
        set_error("%s: work is null", name);
        return DFHIP_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(work, 0, 4 * sizeof(uint32_t), s) != hipSuccess) return check_launch(name);
    if (N == 0) return DFHIP_OK;  // no launch; the sample count reads 0
    if (!rays_o || !rays_d || !nears || !fars || !grid || !density || !weights_sum || !depth ||
        !image || (colour && (!k0 || (view_dim && !view)))) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    const rm::MarchConsts k = rm::make_consts(bound, dt_gamma, max_steps, C, H);
    // persistent waves: as many workgroups as are co-resident on the chip
    // (occupancy query, cached per device); the queue balances the rays
    auto launch = [&](auto kernel, int waves) {
        const uint32_t resident = resident_blocks((const void *)kernel, 64 * waves, 1);
        const uint32_t want = ceil_div(N, 64u * (uint32_t)waves);
        const uint32_t blocks = want < resident ? want : resident;
        kernel<<<blocks, 64 * waves, 0, s>>>(N, rays_o, rays_d, nears, fars, noises, k, grid,
                                             max_steps, T_thresh, density, k0, view, G, P,
                                             weights_sum, depth, image, work, order, chunk_log2,
                                             tile_w, sh);
    };
    if (shading == rd::kTextureless)
        launch(vr::k_render_voxel<rd::kTextureless>, vr::waves_of(rd::kTextureless));
    else if (shading == rd::kLambertian)
        launch(vr::k_render_voxel<rd::kLambertian>, vr::waves_of(rd::kLambertian));
    else if (shading == rd::kNormal)
        launch(vr::k_render_voxel<rd::kNormal>, vr::waves_of(rd::kNormal));
    else
        launch(vr::k_render_voxel<rd::kAlbedo>, vr::waves_of(rd::kAlbedo));
    return check_launch(name);
}

extern "C" int dfhip_voxel_render_rays_infer(
    uint32_t N, const float *rays_o, const float *rays_d, const float *nears, const float *fars,
    const float *noises, float bound, float dt_gamma, uint32_t max_steps, uint32_t C,
    uint32_t H, const uint8_t *grid, float T_thresh, const float *density, const float *k0,
    uint32_t Nx, uint32_t Ny, uint32_t Nz, uint32_t k0_channels, uint32_t pos_freqs,
    const float *view, uint32_t view_dim, const float *box, float act_shift,
    const float *const *params, float *weights_sum, float *depth, float *image, uint32_t *work,
    const int32_t *order, uint32_t chunk_log2, uint32_t tile_w, dfhip_stream_t stream) {
    return voxel_render("voxel_render_rays_infer", N, rays_o, rays_d, nears, fars, noises, bound,
                        dt_gamma, max_steps, C, H, grid, T_thresh, density, k0, Nx, Ny, Nz,
                        k0_channels, pos_freqs, view, view_dim, box, act_shift, params,
                        weights_sum, depth, image, work, order, chunk_log2, tile_w, rd::kAlbedo,
                        vr::ShadeArgs{}, stream);
}

// The shaded frames: argument checks of the shading, then the launcher above.
extern "C" int dfhip_voxel_render_rays_infer_shaded(
    uint32_t N, const float *rays_o, const float *rays_d, const float *nears, const float *fars,
    const float *noises, float bound, float dt_gamma, uint32_t max_steps, uint32_t C,
    uint32_t H, const uint8_t *grid, float T_thresh, const float *density, const float *k0,
    uint32_t Nx, uint32_t Ny, uint32_t Nz, uint32_t k0_channels, uint32_t pos_freqs,
    const float *view, uint32_t view_dim, const float *box, float act_shift,
    const float *const *params, float *weights_sum, float *depth, float *image, uint32_t *work,
    const int32_t *order, uint32_t chunk_log2, uint32_t tile_w, int shading, const float *light,
    float ratio, dfhip_stream_t stream) {
    const char *name = "voxel_render_rays_infer_shaded";
    if (shading == DFHIP_SHADING_ALBEDO) {
        set_error("%s: the albedo shading is dfhip_voxel_render_rays_infer's", name);
        return DFHIP_EINVAL;
    }
    if (shading != DFHIP_SHADING_TEXTURELESS && shading != DFHIP_SHADING_LAMBERTIAN &&
        shading != DFHIP_SHADING_NORMAL) {
        set_error("%s: shading must be DFHIP_SHADING_TEXTURELESS, _LAMBERTIAN or _NORMAL "
                  "(got %d)", name, shading);
        return DFHIP_EINVAL;
    }
    if (!light) {
        set_error("%s: light is NULL (a DEVICE f32 [3] direction is required)", name);
        return DFHIP_EINVAL;
    }
    // 1 - ratio as dfhip_shading_forward rounds it
    const vr::ShadeArgs sh{light, ratio, (float)(1.0 - (double)ratio)};
    return voxel_render(name, N, rays_o, rays_d, nears, fars, noises, bound, dt_gamma, max_steps,
                        C, H, grid, T_thresh, density, k0, Nx, Ny, Nz, k0_channels, pos_freqs,
                        view, view_dim, box, act_shift, params, weights_sum, depth, image, work,
                        order, chunk_log2, tile_w, shading, sh, stream);
}
