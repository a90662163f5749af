// Training shadings of the DVGO backbone's native train step
// (nerf/native_voxel_step.py): the `textureless` and `lambertian` colours of
// nerf/network_dvgo.py's forward and the orientation term of
// nerf/renderer.py's run_cuda, on capacity-sized buffers with the live sample
// count read on the device.
//
//   normal = NeRFNetwork._unit(-d sigma / d x): the closed form of
//            dfhip_voxel_normal (vx::density_normal) from the sample's own
//            cell, then vx::unit_normal                               (f32)
//   lam    = shd::lambert<half_t>: the rounding points of fp16 autocast  (f16)
//   colour = lam on three channels | f16(albedo * lam)                  (f16)
//   orient = mean(w * clamp(normal . dir, 0)^2), w = 1 - exp(-sigma), over the
//            Me = min(cap, align_up(live, align)) rows of the march's slice,
//            whose tail rows contribute 0; f64 partials as in shade.hip
//
// The density is frozen, so nothing flows back through the normal: the
// backward of a lambertian step is grad_albedo = f16(grad_colour * lam), and a
// textureless step has none.
#include "shade_common.h"
#include "voxel_common.h"

namespace dfhip {
namespace vs {

constexpr uint32_t kThreads = 256;

__device__ __forceinline__ uint32_t live_rows(const int32_t *m_dev, uint32_t cap) {
    const int32_t m = *m_dev;
    return m < 0 ? 0u : ((uint32_t)m < cap ? (uint32_t)m : cap);
}

__device__ __forceinline__ uint32_t effective_rows(uint32_t m, uint32_t cap, uint32_t align) {
    const uint64_t a = ((uint64_t)m + align - 1u) / align * align;
    return a < (uint64_t)cap ? (uint32_t)a : cap;
}

__global__ __launch_bounds__(kThreads) void k_shade_fwd(
    const float *__restrict__ xyz, const float *__restrict__ dirs,
    const float *__restrict__ density, vx::Geom G, const half_t *__restrict__ albedo,
    const float *__restrict__ light, float ratio, float omr, int lambertian,
    const int32_t *__restrict__ m_dev, uint32_t cap, float *__restrict__ normal,
    half_t *__restrict__ lam, half_t *__restrict__ color, double *__restrict__ part) {
    __shared__ double red[kThreads / 64];
    const uint32_t M = live_rows(m_dev, cap);
    float l16[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) l16[d] = shd::rnd<half_t>(light[d]);
    double acc = 0.0;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < M; i += gridDim.x * kThreads) {
        const float x[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
        const vx::Cell cell = vx::locate(G, x);
        float raw = 0.0f, n[3] = {0.0f, 0.0f, 0.0f};
        if (cell.inside) vx::density_normal(G, cell, vx::corners(G, cell), density, raw, n);
        vx::unit_normal(n);
        const float l = shd::lambert<half_t>(n, l16, ratio, omr).lam16;
        lam[i] = (half_t)l;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            normal[3 * (size_t)i + d] = n[d];
            const float c = lambertian ? shd::rnd<half_t>((float)albedo[3 * (size_t)i + d] * l) : l;
            color[3 * (size_t)i + d] = (half_t)c;
        }
        const float w = 1.0f - expf(-vx::activate(raw, G.act_shift));
        const float nd = (n[0] * dirs[3 * (size_t)i] + n[1] * dirs[3 * (size_t)i + 1]) +
                         n[2] * dirs[3 * (size_t)i + 2];
        const float c = nd > 0.0f ? nd : 0.0f;
        acc += (double)(w * (c * c));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < (int)(kThreads / 64); ++w) s += red[w];
        part[blockIdx.x] = s;
    }
}

// orient = sum / Me in a fixed order (0 when no row is live)
__global__ __launch_bounds__(64) void k_orient_finish(const double *__restrict__ part,
                                                      uint32_t parts, const int32_t *m_dev,
                                                      uint32_t cap, uint32_t align,
                                                      float *__restrict__ orient) {
    double s = 0.0;
    for (uint32_t p = threadIdx.x; p < parts; p += 64) s += part[p];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) {
        const uint32_t Me = effective_rows(live_rows(m_dev, cap), cap, align);
        *orient = Me ? (float)(s / (double)Me) : 0.0f;
    }
}

// grad_albedo = f16(grad_colour * lam): torch's half product (f32, rounded once)
__global__ __launch_bounds__(kThreads) void k_shade_bwd(const half_t *__restrict__ grad_color,
                                                        const half_t *__restrict__ lam,
                                                        const int32_t *__restrict__ m_dev,
                                                        uint32_t cap,
                                                        half_t *__restrict__ grad_albedo) {
    const size_t n = 3 * (size_t)live_rows(m_dev, cap);
    for (size_t j = blockIdx.x * (size_t)kThreads + threadIdx.x; j < n;
         j += (size_t)gridDim.x * kThreads)
        grad_albedo[j] = (half_t)shd::rnd<half_t>((float)grad_color[j] * (float)lam[j / 3]);
}

// grid-stride launches: dfhip_shading_partial_doubles' rule
static uint32_t blocks(uint32_t cap) {
    const uint32_t b = ceil_div(cap, kThreads);
    return b < 1024u ? (b ? b : 1u) : 1024u;
}

static bool arguments(const char *name, int shading, uint32_t cap, const int32_t *m_dev,
                      uint32_t align, int &lambertian) {
    if (shading == DFHIP_SHADING_TEXTURELESS) lambertian = 0;
    else if (shading == DFHIP_SHADING_LAMBERTIAN) lambertian = 1;
    else {
        set_error("%s: shading must be DFHIP_SHADING_TEXTURELESS or _LAMBERTIAN", name);
        return false;
    }
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

}  // namespace vs
}  // namespace dfhip

using namespace dfhip;

extern "C" int dfhip_voxel_shade_train_forward(const float *xyz, const float *dirs,
                                               const float *density, uint32_t Nx, uint32_t Ny,
                                               uint32_t Nz, const float *box, float bound,
                                               float act_shift, const void *albedo,
                                               const float *light, float ratio, int shading,
                                               uint32_t cap, const int32_t *m_dev, uint32_t align,
                                               float *normal, void *lam, void *color,
                                               double *partial, float *orient,
                                               dfhip_stream_t stream) {
    const char *name = "voxel_shade_train_forward";
    int lambertian = 0;
    if (!vs::arguments(name, shading, cap, m_dev, align, lambertian)) return DFHIP_EINVAL;
    vx::Geom G;
    if (!vx::geometry(name, Nx, Ny, Nz, 0u, 0u, 0u, box, bound, act_shift, false, G))
        return DFHIP_EINVAL;
    if (!xyz || !dirs || !density || !light || !normal || !lam || !color || !partial || !orient ||
        (lambertian && !albedo)) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    const uint32_t nblk = vs::blocks(cap);
    const float omr = (float)(1.0 - (double)ratio);
    vs::k_shade_fwd<<<nblk, vs::kThreads, 0, s>>>(xyz, dirs, density, G, (const half_t *)albedo,
                                                  light, ratio, omr, lambertian, m_dev, cap,
                                                  normal, (half_t *)lam, (half_t *)color, partial);
    vs::k_orient_finish<<<1, 64, 0, s>>>(partial, nblk, m_dev, cap, align, orient);
    return check_launch(name);
}

extern "C" int dfhip_voxel_shade_train_backward(const void *grad_color, const void *lam,
                                                int shading, uint32_t cap, const int32_t *m_dev,
                                                uint32_t align, void *grad_albedo,
                                                dfhip_stream_t stream) {
    const char *name = "voxel_shade_train_backward";
    int lambertian = 0;
    if (!vs::arguments(name, shading, cap, m_dev, align, lambertian)) return DFHIP_EINVAL;
    if (!lambertian) return DFHIP_OK;  // a constant colour: no gradient leaves it
    if (!grad_color || !lam || !grad_albedo) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    vs::k_shade_bwd<<<vs::blocks(cap), vs::kThreads, 0, as_stream(stream)>>>(
        (const half_t *)grad_color, (const half_t *)lam, m_dev, cap, (half_t *)grad_albedo);
    return check_launch(name);
}
