// Hierarchical sampling and compositing of NeRFRenderer.run() (the renderer of
// every run without --cuda_ray; reference nerf/renderer.py:15-49, 301-443):
// coarse uniform samples, sample_pdf importance samples, the sort of their
// union and the cumulative-product compositing with its closed-form backward.
//
// One wave of 64 lanes serves one ray, HS_RAYS rays per workgroup.  In the
// sampling and compositing kernels lane l holds the K = ceil(M / 64)
// consecutive samples l K .. l K + K - 1 of its ray in registers; prefix
// products, prefix sums and suffix sums are a serial pass over the lane's own
// samples around a wave scan of the 64 lane totals.  The inverse-CDF search
// and the sort read a per-ray table in LDS (cdf and bin edges, sort keys).
// No atomics, no host synchronisation, all arithmetic f32 with no contraction.
#include "common.h"

namespace dfhip {
namespace {

constexpr int HS_RAYS = 4;  // rays (waves) per workgroup
constexpr int HS_THREADS = 64 * HS_RAYS;
constexpr uint32_t HS_MAX_T = 256, HS_MAX_M = 512;

// torch.max / torch.min of a value against a bound: NaN propagates.
__device__ __forceinline__ float nan_max(float x, float b) { return x != x ? x : fmaxf(x, b); }
__device__ __forceinline__ float nan_min(float x, float b) { return x != x ? x : fminf(x, b); }

// rays_o + rays_d * z clamped into the box (renderer.py:342-343, 369-370).
__device__ __forceinline__ void store_position(float *xyz, const float o[3], const float d[3],
                                               float z, const float box[6]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float p = o[c] + d[c] * z;
        xyz[c] = nan_min(nan_max(p, box[c]), box[3 + c]);
    }
}

// Inclusive product / sum of the lanes below and this one.
__device__ __forceinline__ float wave_prefix_mul(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_up(v, o, 64);
        if (lane >= o) v = u * v;
    }
    return v;
}
__device__ __forceinline__ float wave_prefix_add(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_up(v, o, 64);
        if (lane >= o) v = u + v;
    }
    return v;
}
// Inclusive sum of this lane and the lanes above.
__device__ __forceinline__ float wave_suffix_add(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_down(v, o, 64);
        if (lane + o < 64) v = v + u;
    }
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------ coarse samples
// renderer.py:331-343 in torch's operation order: z = near + (far - near) lin,
// sample_dist = (far - near) (1 / T) (torch divides by a host scalar as a
// product with its f32 reciprocal), z += (noise - 0.5) sample_dist.
__global__ void __launch_bounds__(HS_THREADS)
k_uniform_samples(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                  const float *__restrict__ aabb, const float *__restrict__ nears,
                  const float *__restrict__ fars, const float *__restrict__ lin,
                  const float *__restrict__ noise, uint32_t N, uint32_t T, float inv_T,
                  float *__restrict__ z_out, float *__restrict__ xyzs) {
    const int lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * HS_RAYS + (threadIdx.x >> 6);
    if (r >= N) return;
    float o[3], d[3], box[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = rays_o[3 * (size_t)r + c];
        d[c] = rays_d[3 * (size_t)r + c];
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) box[c] = aabb[c];
    const float near = nears[r], range = fars[r] - near;
    const float sample_dist = range * inv_T;
    const size_t row = (size_t)r * T;
    for (uint32_t j = lane; j < T; j += 64) {
        float z = near + range * lin[j];
        if (noise) z = z + (noise[row + j] - 0.5f) * sample_dist;
        z_out[row + j] = z;
        store_position(xyzs + 3 * (row + j), o, d, z, box);
    }
}

// -------------------------------------------------------- importance samples
// renderer.py:358-370 and sample_pdf (renderer.py:15-49) for one ray per wave.
// Sample i = lane K + k.  The cdf (T - 1 entries, cdf[0] = 0) and the bin
// edges z_mid (T - 1 entries) go to LDS, then lane l inverts u_l, u_{l+64}, ...
template <int K>
__global__ void __launch_bounds__(HS_THREADS)
k_importance_samples(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                     const float *__restrict__ aabb, const float *__restrict__ nears,
                     const float *__restrict__ fars, const float *__restrict__ z_in,
                     const float *__restrict__ sigma, const float *__restrict__ u_in, uint32_t N,
                     uint32_t T, uint32_t t, float inv_T, float *__restrict__ new_z,
                     float *__restrict__ new_xyzs) {
    __shared__ float s_cdf[HS_RAYS][HS_MAX_T];
    __shared__ float s_bin[HS_RAYS][HS_MAX_T];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ray = blockIdx.x * HS_RAYS + wave;
    const bool live = ray < N;
    const uint32_t r = live ? ray : N - 1;  // a spare wave repeats the last ray, stores nothing
    const float near = nears[r];
    const float sample_dist = (fars[r] - near) * inv_T;
    const size_t row = (size_t)r * T;

    float z[K], s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t i = lane * K + k;
        z[k] = i < T ? z_in[row + i] : 0.f;
        s[k] = i < T ? sigma[row + i] : 0.f;
    }
    const float z_above = __shfl_down(z[0], 1, 64);  // first sample of the next lane

    float alpha[K], dz[K], q_lane = 1.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t i = lane * K + k;
        const float zn = k + 1 < K ? z[k + 1 < K ? k + 1 : k] : z_above;
        dz[k] = i + 1 == T ? sample_dist : zn - z[k];
        alpha[k] = i < T ? 1.f - expf(-dz[k] * s[k]) : 0.f;
        q_lane *= i < T ? (1.f - alpha[k]) + 1e-15f : 1.f;
    }
    // transmittance before the lane's first sample
    const float q_incl = wave_prefix_mul(q_lane, lane);
    float trans = __shfl_up(q_incl, 1, 64);
    if (lane == 0) trans = 1.f;

    // pdf weights of samples 1 .. T - 2 (weights[1:-1] + 1e-5)
    float w[K], w_lane = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t i = lane * K + k;
        const bool in_pdf = i >= 1 && i + 1 < T;
        w[k] = in_pdf ? alpha[k] * trans + 1e-5f : 0.f;
        w_lane += w[k];
        trans *= i < T ? (1.f - alpha[k]) + 1e-15f : 1.f;
    }
    const float w_total = wave_sum(w_lane);
    float pdf_lane = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t i = lane * K + k;
        w[k] = (i >= 1 && i + 1 < T) ? w[k] / w_total : 0.f;
        pdf_lane += w[k];
    }
    float cdf = __shfl_up(wave_prefix_add(pdf_lane, lane), 1, 64);  // the lanes below
    if (lane == 0) cdf = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t i = lane * K + k;
        cdf += w[k];
        if (i + 1 < T) {  // entries 0 .. T - 2; w of sample 0 is 0, so cdf[0] = 0
            s_cdf[wave][i] = cdf;
            s_bin[wave][i] = z[k] + 0.5f * dz[k];
        }
    }
    __syncthreads();

    float o[3], d[3], box[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = rays_o[3 * (size_t)r + c];
        d[c] = rays_d[3 * (size_t)r + c];
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) box[c] = aabb[c];
    const int L = (int)T - 1;  // cdf / bin entries
    const float *cdfs = s_cdf[wave], *bins = s_bin[wave];
    for (uint32_t j = lane; j < t; j += 64) {
        const float u = u_in ? u_in[(size_t)r * t + j] : ((float)j + 0.5f) / (float)t;
        // searchsorted(cdf, u, right=True): the number of entries <= u
        int lo_n = 0, hi_n = L;
        while (lo_n < hi_n) {
            const int mid = (lo_n + hi_n) >> 1;
            if (cdfs[mid] <= u) lo_n = mid + 1; else hi_n = mid;
        }
        const int lo = lo_n - 1 < 0 ? 0 : lo_n - 1;
        const int hi = lo_n > L - 1 ? L - 1 : lo_n;
        float span = cdfs[hi] - cdfs[lo];
        if (span < 1e-5f) span = 1.f;
        const float frac = (u - cdfs[lo]) / span;
        const float zj = bins[lo] + frac * (bins[hi] - bins[lo]);
        if (live) {
            new_z[(size_t)r * t + j] = zj;
            store_position(new_xyzs + 3 * ((size_t)r * t + j), o, d, zj, box);
        }
    }
}

// --------------------------------------------------------------------- merge
// The union of the coarse and the new samples in ascending depth, ties by
// their index in the concatenation [coarse, new].  Each sample's place is the
// number of samples ordered before it, counted against the ray's keys in LDS
// (every lane reads the same key: a broadcast).  The key is the depth's bit
// pattern mapped to an unsigned integer of the same order, -0 counted as +0.
__device__ __forceinline__ uint32_t depth_key(float z) {
    const uint32_t b = __float_as_uint(z + 0.f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ void __launch_bounds__(HS_THREADS)
k_merge_samples(const float *__restrict__ z_in, const float *__restrict__ new_z,
                const float *__restrict__ xyzs, const float *__restrict__ new_xyzs, uint32_t N,
                uint32_t T, uint32_t t, float *__restrict__ z_all, int32_t *__restrict__ order,
                float *__restrict__ xyzs_all) {
    __shared__ uint32_t s_key[HS_RAYS][HS_MAX_M];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ray = blockIdx.x * HS_RAYS + wave;
    const bool live = ray < N;
    const uint32_t r = live ? ray : N - 1;
    const uint32_t M = T + t;
    uint32_t *keys = s_key[wave];
    for (uint32_t i = lane; i < M; i += 64) {
        const float z = i < T ? z_in[(size_t)r * T + i] : new_z[(size_t)r * t + (i - T)];
        keys[i] = depth_key(z);
    }
    __syncthreads();
    if (!live) return;
    for (uint32_t i = lane; i < M; i += 64) {
        const uint32_t key = keys[i];
        uint32_t place = 0;
        for (uint32_t k = 0; k < M; ++k) {
            const uint32_t other = keys[k];
            place += (other < key || (other == key && k < i)) ? 1u : 0u;
        }
        const float *src = i < T ? xyzs + 3 * ((size_t)r * T + i)
                                 : new_xyzs + 3 * ((size_t)r * t + (i - T));
        const size_t dst = (size_t)r * M + place;  // place < M: a permutation
        z_all[dst] = i < T ? z_in[(size_t)r * T + i] : new_z[(size_t)r * t + (i - T)];
        order[dst] = (int32_t)i;
        xyzs_all[3 * dst + 0] = src[0];
        xyzs_all[3 * dst + 1] = src[1];
        xyzs_all[3 * dst + 2] = src[2];
    }
}

// ----------------------------------------------------------------- composite
// One ray's samples in the lanes' registers: depth, sigma through `order`,
// dz (sample_dist after the last sample), e = exp(-dz sigma), alpha = 1 - e,
// q = (1 - alpha) + 1e-15 and the transmittance before each sample
// (renderer.py:389-393).
template <int K>
struct RaySamples {
    float z[K], dz[K], e[K], alpha[K], q[K], trans[K];
    int32_t idx[K];

    __device__ __forceinline__ void load(const float *sigma_c, const float *sigma_n,
                                         const int32_t *order, const float *z_all, uint32_t r,
                                         uint32_t T, uint32_t t, float sample_dist, int lane) {
        const uint32_t M = T + t;
        const size_t row = (size_t)r * M;
        float s[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t i = lane * K + k;
            const bool valid = i < M;
            // an index outside the ray's samples would read outside the arrays
            uint32_t j = valid && order ? (uint32_t)order[row + i] : i;
            j = j < M ? j : M - 1;
            idx[k] = (int32_t)j;
            z[k] = valid ? z_all[row + i] : 0.f;
            s[k] = !valid ? 0.f : j < T ? sigma_c[(size_t)r * T + j] : sigma_n[(size_t)r * t + (j - T)];
        }
        const float z_above = __shfl_down(z[0], 1, 64);
        float q_lane = 1.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t i = lane * K + k;
            const bool valid = i < M;
            const float zn = k + 1 < K ? z[k + 1 < K ? k + 1 : k] : z_above;
            dz[k] = i + 1 == M ? sample_dist : zn - z[k];
            e[k] = valid ? expf(-dz[k] * s[k]) : 1.f;
            alpha[k] = valid ? 1.f - e[k] : 0.f;
            q[k] = valid ? (1.f - alpha[k]) + 1e-15f : 1.f;
            q_lane *= q[k];
        }
        const float q_incl = wave_prefix_mul(q_lane, lane);
        float tr = __shfl_up(q_incl, 1, 64);
        if (lane == 0) tr = 1.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            trans[k] = tr;
            tr *= q[k];
        }
    }
};

// clamp((z - near) / (far - near), 0, 1) as torch.clamp: NaN (a ray that
// misses the box has near = far) stays NaN.
__device__ __forceinline__ float unit_depth(float z, float near, float far) {
    return nan_min(nan_max((z - near) / (far - near), 0.f), 1.f);
}

template <int K, typename C>
__global__ void __launch_bounds__(HS_THREADS)
k_composite_uniform_forward(const float *__restrict__ sigma_c, const float *__restrict__ sigma_n,
                            const int32_t *__restrict__ order, const float *__restrict__ z_all,
                            const float *__restrict__ nears, const float *__restrict__ fars,
                            const float *__restrict__ sample_dist, const C *__restrict__ rgbs,
                            uint32_t N, uint32_t T, uint32_t t, float *__restrict__ weights_sum,
                            float *__restrict__ depth, float *__restrict__ image,
                            float *__restrict__ weights) {
    const int lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * HS_RAYS + (threadIdx.x >> 6);
    if (r >= N) return;  // whole waves leave; no workgroup barrier below
    const uint32_t M = T + t;
    const size_t row = (size_t)r * M;
    RaySamples<K> smp;
    smp.load(sigma_c, sigma_n, order, z_all, r, T, t, sample_dist[r], lane);
    const float near = nears[r], far = fars[r];
    float ws = 0.f, dep = 0.f, img[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t i = lane * K + k;
        if (i < M) {
            const float w = smp.alpha[k] * smp.trans[k];
            weights[row + i] = w;
            ws += w;
            dep += w * unit_depth(smp.z[k], near, far);
#pragma unroll
            for (int c = 0; c < 3; ++c) img[c] += w * to_f(rgbs[3 * (row + i) + c]);
        }
    }
    ws = wave_sum(ws);
    dep = wave_sum(dep);
#pragma unroll
    for (int c = 0; c < 3; ++c) img[c] = wave_sum(img[c]);
    if (lane == 0) {
        weights_sum[r] = ws;
        depth[r] = dep;
#pragma unroll
        for (int c = 0; c < 3; ++c) image[3 * (size_t)r + c] = img[c];
    }
}

// Closed-form backward.  With G_i = g_image . c_i + g_ws + g_depth zeta_i and
// S_i = sum_{k > i} w_k G_k:
//   dL/dsigma_i = dz_i e_i (T_i G_i - S_i / q_i),  dL/dc_i = w_i g_image,
// e_i = exp(-dz_i sigma_i) being d alpha_i / d(dz_i sigma_i).  A null upstream
// gradient leaves its term out (its output took no part in the loss).
template <int K, typename C>
__global__ void __launch_bounds__(HS_THREADS)
k_composite_uniform_backward(const float *__restrict__ g_ws, const float *__restrict__ g_depth,
                             const float *__restrict__ g_image, const float *__restrict__ sigma_c,
                             const float *__restrict__ sigma_n, const int32_t *__restrict__ order,
                             const float *__restrict__ z_all, const float *__restrict__ nears,
                             const float *__restrict__ fars, const float *__restrict__ sample_dist,
                             const C *__restrict__ rgbs, uint32_t N, uint32_t T, uint32_t t,
                             float *__restrict__ g_sigma_c, float *__restrict__ g_sigma_n,
                             C *__restrict__ g_rgbs) {
    const int lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * HS_RAYS + (threadIdx.x >> 6);
    if (r >= N) return;
    const uint32_t M = T + t;
    const size_t row = (size_t)r * M;
    RaySamples<K> smp;
    smp.load(sigma_c, sigma_n, order, z_all, r, T, t, sample_dist[r], lane);
    const float near = nears[r], far = fars[r];
    const float gw = g_ws ? g_ws[r] : 0.f, gd = g_depth ? g_depth[r] : 0.f;
    float gi[3] = {0.f, 0.f, 0.f};
    if (g_image) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gi[c] = g_image[3 * (size_t)r + c];
    }
    float G[K], wG[K], wG_lane = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t i = lane * K + k;
        G[k] = 0.f;
        wG[k] = 0.f;
        if (i < M) {
            const float w = smp.alpha[k] * smp.trans[k];
            float g = 0.f;
            if (g_image) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    g += gi[c] * to_f(rgbs[3 * (row + i) + c]);
                    if (g_rgbs) g_rgbs[3 * (row + i) + c] = from_f<C>(f32_rounded(w * gi[c]));
                }
            } else if (g_rgbs) {
#pragma unroll
                for (int c = 0; c < 3; ++c) g_rgbs[3 * (row + i) + c] = from_f<C>(0.f);
            }
            if (g_ws) g += gw;
            if (g_depth) g += gd * unit_depth(smp.z[k], near, far);
            G[k] = g;
            wG[k] = w * g;
            wG_lane += wG[k];
        }
    }
    // sum of w G over the samples after the lane's last one
    float S = __shfl_down(wave_suffix_add(wG_lane, lane), 1, 64);
    if (lane == 63) S = 0.f;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
        const uint32_t i = lane * K + k;
        if (i < M) {
            const float g = smp.dz[k] * smp.e[k] * (smp.trans[k] * G[k] - S / smp.q[k]);
            const uint32_t j = (uint32_t)smp.idx[k];
            if (j < T) g_sigma_c[(size_t)r * T + j] = g;
            else g_sigma_n[(size_t)r * t + (j - T)] = g;
        }
        S += wG[k];
    }
}

bool sizes_ok(const char *what, uint32_t T, uint32_t t) {
    if (T < 3 || T > HS_MAX_T || t > HS_MAX_T || T + t > HS_MAX_M) {
        set_error("%s: 3 <= T <= 256, t <= 256 and T + t <= 512 expected, got T = %u, t = %u",
                  what, T, t);
        return false;
    }
    return true;
}

#define HS_REQUIRE(what, p)                                          \
    if (!(p)) {                                                      \
        dfhip::set_error("%s: " #p " must not be NULL", what);       \
        return DFHIP_EINVAL;                                         \
    }

#define HS_DISPATCH_K(Kv, ...)                                       \
    switch (Kv) {                                                    \
    case 1: { constexpr int K = 1; __VA_ARGS__; break; }             \
    case 2: { constexpr int K = 2; __VA_ARGS__; break; }             \
    case 3: { constexpr int K = 3; __VA_ARGS__; break; }             \
    case 4: { constexpr int K = 4; __VA_ARGS__; break; }             \
    case 5: { constexpr int K = 5; __VA_ARGS__; break; }             \
    case 6: { constexpr int K = 6; __VA_ARGS__; break; }             \
    case 7: { constexpr int K = 7; __VA_ARGS__; break; }             \
    default: { constexpr int K = 8; __VA_ARGS__; break; }            \
    }

}  // namespace
}  // namespace dfhip

using namespace dfhip;

extern "C" int dfhip_uniform_samples(const float *rays_o, const float *rays_d, const float *aabb,
                                     const float *nears, const float *fars, const float *lin,
                                     const float *noise, uint32_t N, uint32_t T, float *z,
                                     float *xyzs, dfhip_stream_t stream) {
    const char *what = "uniform_samples";
    if (!sizes_ok(what, T, 0)) return DFHIP_EINVAL;
    if (N == 0) return DFHIP_OK;
    HS_REQUIRE(what, rays_o) HS_REQUIRE(what, rays_d) HS_REQUIRE(what, aabb)
    HS_REQUIRE(what, nears) HS_REQUIRE(what, fars) HS_REQUIRE(what, lin)
    HS_REQUIRE(what, z) HS_REQUIRE(what, xyzs)
    k_uniform_samples<<<ceil_div(N, (uint32_t)HS_RAYS), HS_THREADS, 0, as_stream(stream)>>>(
        rays_o, rays_d, aabb, nears, fars, lin, noise, N, T, 1.0f / (float)T, z, xyzs);
    return check_launch(what);
}

extern "C" int dfhip_importance_samples(const float *rays_o, const float *rays_d,
                                        const float *aabb, const float *nears, const float *fars,
                                        const float *z, const float *sigma, const float *u,
                                        uint32_t N, uint32_t T, uint32_t t, float *new_z,
                                        float *new_xyzs, dfhip_stream_t stream) {
    const char *what = "importance_samples";
    if (!sizes_ok(what, T, t)) return DFHIP_EINVAL;
    if (N == 0 || t == 0) return DFHIP_OK;
    HS_REQUIRE(what, rays_o) HS_REQUIRE(what, rays_d) HS_REQUIRE(what, aabb)
    HS_REQUIRE(what, nears) HS_REQUIRE(what, fars) HS_REQUIRE(what, z) HS_REQUIRE(what, sigma)
    HS_REQUIRE(what, new_z) HS_REQUIRE(what, new_xyzs)
    const dim3 grid(ceil_div(N, (uint32_t)HS_RAYS));
    HS_DISPATCH_K((int)ceil_div(T, 64u),
        if constexpr (K <= 4)
            k_importance_samples<K><<<grid, HS_THREADS, 0, as_stream(stream)>>>(
                rays_o, rays_d, aabb, nears, fars, z, sigma, u, N, T, t, 1.0f / (float)T, new_z,
                new_xyzs));
    return check_launch(what);
}

extern "C" int dfhip_merge_samples(const float *z, const float *new_z, const float *xyzs,
                                   const float *new_xyzs, uint32_t N, uint32_t T, uint32_t t,
                                   float *z_all, int32_t *order, float *xyzs_all,
                                   dfhip_stream_t stream) {
    const char *what = "merge_samples";
    if (!sizes_ok(what, T, t)) return DFHIP_EINVAL;
    if (N == 0) return DFHIP_OK;
    HS_REQUIRE(what, z) HS_REQUIRE(what, xyzs)
    if (t > 0) { HS_REQUIRE(what, new_z) HS_REQUIRE(what, new_xyzs) }
    HS_REQUIRE(what, z_all) HS_REQUIRE(what, order) HS_REQUIRE(what, xyzs_all)
    k_merge_samples<<<ceil_div(N, (uint32_t)HS_RAYS), HS_THREADS, 0, as_stream(stream)>>>(
        z, new_z, xyzs, new_xyzs, N, T, t, z_all, order, xyzs_all);
    return check_launch(what);
}

extern "C" int dfhip_composite_uniform_forward(int dtype, const float *sigma_coarse,
                                               const float *sigma_new, const int32_t *order,
                                               const float *z_all, const float *nears,
                                               const float *fars, const float *sample_dist,
                                               const void *rgbs, uint32_t N, uint32_t T,
                                               uint32_t t, float *weights_sum, float *depth,
                                               float *image, float *weights,
                                               dfhip_stream_t stream) {
    const char *what = "composite_uniform_forward";
    if (!sizes_ok(what, T, t)) return DFHIP_EINVAL;
    if (dtype != DFHIP_F32 && dtype != DFHIP_F16) {
        set_error("%s: rgbs must be f32 or f16, got dtype %d", what, dtype);
        return DFHIP_EDTYPE;
    }
    if (N == 0) return DFHIP_OK;
    HS_REQUIRE(what, sigma_coarse) HS_REQUIRE(what, z_all) HS_REQUIRE(what, nears)
    HS_REQUIRE(what, fars) HS_REQUIRE(what, sample_dist) HS_REQUIRE(what, rgbs)
    HS_REQUIRE(what, weights_sum) HS_REQUIRE(what, depth) HS_REQUIRE(what, image)
    HS_REQUIRE(what, weights)
    if (t > 0) { HS_REQUIRE(what, sigma_new) HS_REQUIRE(what, order) }
    const dim3 grid(ceil_div(N, (uint32_t)HS_RAYS));
    hipStream_t s = as_stream(stream);
    HS_DISPATCH_K((int)ceil_div(T + t, 64u),
        if (dtype == DFHIP_F16)
            k_composite_uniform_forward<K, half_t><<<grid, HS_THREADS, 0, s>>>(
                sigma_coarse, sigma_new, order, z_all, nears, fars, sample_dist,
                (const half_t *)rgbs, N, T, t, weights_sum, depth, image, weights);
        else
            k_composite_uniform_forward<K, float><<<grid, HS_THREADS, 0, s>>>(
                sigma_coarse, sigma_new, order, z_all, nears, fars, sample_dist,
                (const float *)rgbs, N, T, t, weights_sum, depth, image, weights));
    return check_launch(what);
}

extern "C" int dfhip_composite_uniform_backward(int dtype, const float *grad_weights_sum,
                                                const float *grad_depth, const float *grad_image,
                                                const float *sigma_coarse, const float *sigma_new,
                                                const int32_t *order, const float *z_all,
                                                const float *nears, const float *fars,
                                                const float *sample_dist, const void *rgbs,
                                                uint32_t N, uint32_t T, uint32_t t,
                                                float *grad_sigma_coarse, float *grad_sigma_new,
                                                void *grad_rgbs, dfhip_stream_t stream) {
    const char *what = "composite_uniform_backward";
    if (!sizes_ok(what, T, t)) return DFHIP_EINVAL;
    if (dtype != DFHIP_F32 && dtype != DFHIP_F16) {
        set_error("%s: rgbs must be f32 or f16, got dtype %d", what, dtype);
        return DFHIP_EDTYPE;
    }
    if (N == 0) return DFHIP_OK;
    HS_REQUIRE(what, sigma_coarse) HS_REQUIRE(what, z_all) HS_REQUIRE(what, nears)
    HS_REQUIRE(what, fars) HS_REQUIRE(what, sample_dist) HS_REQUIRE(what, rgbs)
    HS_REQUIRE(what, grad_sigma_coarse)
    if (t > 0) { HS_REQUIRE(what, sigma_new) HS_REQUIRE(what, order) HS_REQUIRE(what, grad_sigma_new) }
    const dim3 grid(ceil_div(N, (uint32_t)HS_RAYS));
    hipStream_t s = as_stream(stream);
    HS_DISPATCH_K((int)ceil_div(T + t, 64u),
        if (dtype == DFHIP_F16)
            k_composite_uniform_backward<K, half_t><<<grid, HS_THREADS, 0, s>>>(
                grad_weights_sum, grad_depth, grad_image, sigma_coarse, sigma_new, order, z_all,
                nears, fars, sample_dist, (const half_t *)rgbs, N, T, t, grad_sigma_coarse,
                grad_sigma_new, (half_t *)grad_rgbs);
        else
            k_composite_uniform_backward<K, float><<<grid, HS_THREADS, 0, s>>>(
                grad_weights_sum, grad_depth, grad_image, sigma_coarse, sigma_new, order, z_all,
                nears, fars, sample_dist, (const float *)rgbs, N, T, t, grad_sigma_coarse,
                grad_sigma_new, (float *)grad_rgbs));
    return check_launch(what);
}
