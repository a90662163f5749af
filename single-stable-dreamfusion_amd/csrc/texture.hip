// Texture bake of export_mesh: UV-space rasteriser, attribute interpolation
// and seam dilation (dfhip.h "texture bake").  The three kernels are
// bandwidth-trivial next to the field query between them; they are written
// to be deterministic (integer atomicMin only) and exact at texel centres.
#include "common.h"

namespace dfhip {
namespace tex {

// A face in texel space, relative to its first vertex p0: d1 = p1 - p0,
// d2 = p2 - p0, area = d1 x d2 (twice the signed area).  The edge functions
// of a point q = centre - p0 are
//   e2 = d1 x q              (edge p0 p1, weight of p2)
//   e1 = q x d2              (edge p2 p0, weight of p1)
//   e0 = (d2 - d1) x (q - d1) (edge p1 p2, weight of p0)
// and the centre is covered when all three have one sign or are zero.
struct Face {
    float p0x, p0y, d1x, d1y, d2x, d2y, area;
    bool valid;  // indices in range and area != 0
};

__device__ __forceinline__ Face load_face(const float *__restrict__ vt,
                                          const int32_t *__restrict__ ft, uint32_t face,
                                          uint32_t T, uint32_t H, uint32_t W) {
    Face fc;
    const uint32_t i0 = (uint32_t)ft[3 * (size_t)face + 0];
    const uint32_t i1 = (uint32_t)ft[3 * (size_t)face + 1];
    const uint32_t i2 = (uint32_t)ft[3 * (size_t)face + 2];
    fc.valid = i0 < T && i1 < T && i2 < T;  // negative indices wrap above T
    fc.p0x = fc.p0y = fc.d1x = fc.d1y = fc.d2x = fc.d2y = fc.area = 0.0f;
    if (!fc.valid) return fc;
    const float fw = (float)W, fh = (float)H;
    fc.p0x = vt[2 * (size_t)i0] * fw;
    fc.p0y = vt[2 * (size_t)i0 + 1] * fh;
    fc.d1x = vt[2 * (size_t)i1] * fw - fc.p0x;
    fc.d1y = vt[2 * (size_t)i1 + 1] * fh - fc.p0y;
    fc.d2x = vt[2 * (size_t)i2] * fw - fc.p0x;
    fc.d2y = vt[2 * (size_t)i2 + 1] * fh - fc.p0y;
    fc.area = fc.d1x * fc.d2y - fc.d1y * fc.d2x;
    fc.valid = fc.area != 0.0f && fc.area == fc.area;
    return fc;
}

// Edge functions of texel centre (col, row).
__device__ __forceinline__ void edge_functions(const Face &fc, uint32_t col, uint32_t row,
                                               float &e0, float &e1, float &e2) {
    const float qx = ((float)col + 0.5f) - fc.p0x;
    const float qy = ((float)row + 0.5f) - fc.p0y;
    e2 = fc.d1x * qy - fc.d1y * qx;
    e1 = qx * fc.d2y - qy * fc.d2x;
    e0 = (fc.d2x - fc.d1x) * (qy - fc.d1y) - (fc.d2y - fc.d1y) * (qx - fc.d1x);
}

__device__ __forceinline__ bool covered(float e0, float e1, float e2) {
    return (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) || (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
}

// The texels whose centres can lie in the face: [x0, x0 + bw) x [y0, y0 + bh),
// clipped to the image (bw = 0 when nothing is left).
struct Box {
    uint32_t x0, y0, bw, bh;
};

// First texel whose centre is >= lo and one past the last whose centre is
// <= hi, clamped to [0, n] in float before the conversion (no overflow, NaN
// clamps to an end).
__device__ __forceinline__ void span(float lo, float hi, uint32_t n, uint32_t &first,
                                     uint32_t &count) {
    const float fn = (float)n;
    const float a = fminf(fmaxf(ceilf(lo - 0.5f), 0.0f), fn);
    const float b = fminf(fmaxf(floorf(hi - 0.5f) + 1.0f, 0.0f), fn);
    first = (uint32_t)a;
    count = b > a ? (uint32_t)b - (uint32_t)a : 0u;
}

__device__ __forceinline__ Box face_box(const Face &fc, uint32_t H, uint32_t W) {
    Box b;
    const float p1x = fc.p0x + fc.d1x, p2x = fc.p0x + fc.d2x;
    const float p1y = fc.p0y + fc.d1y, p2y = fc.p0y + fc.d2y;
    // one texel of slack on each side: p0 + d is rounded, the edge test decides
    span(fminf(fc.p0x, fminf(p1x, p2x)) - 1.0f, fmaxf(fc.p0x, fmaxf(p1x, p2x)) + 1.0f, W, b.x0,
         b.bw);
    span(fminf(fc.p0y, fminf(p1y, p2y)) - 1.0f, fmaxf(fc.p0y, fmaxf(p1y, p2y)) + 1.0f, H, b.y0,
         b.bh);
    if (b.bh == 0) b.bw = 0;
    return b;
}

// Lanes first, first + stride, ... of the box's texels in row-major order.
__device__ __forceinline__ void walk(const Face &fc, const Box &b, uint32_t face, uint32_t first,
                                     uint32_t stride, uint32_t W,
                                     uint32_t *__restrict__ face_id) {
    const uint32_t n = b.bw * b.bh;  // <= H W < 2^31
    for (uint32_t t = first; t < n; t += stride) {
        const uint32_t dy = t / b.bw;
        const uint32_t col = b.x0 + (t - dy * b.bw), row = b.y0 + dy;
        float e0, e1, e2;
        edge_functions(fc, col, row, e0, e1, e2);
        if (covered(e0, e1, e2)) atomicMin(&face_id[(size_t)row * W + col], face);
    }
}

constexpr uint32_t kGroup = 16;                // lanes per face for small boxes
constexpr uint32_t kFacesPerWave = 64 / kGroup;
constexpr uint32_t kSmallBox = 1024;           // texels; larger boxes get the whole wave
constexpr uint32_t kRasterThreads = 256;
constexpr uint32_t kFacesPerBlock = kRasterThreads / kGroup;

// One 16-lane group per face for boxes of up to kSmallBox texels; the wave
// then walks each larger box of its four faces with all 64 lanes.  face_id
// is compared as unsigned, so the -1 fill is the largest value and the
// lowest face id wins whatever the order.
__global__ void __launch_bounds__(kRasterThreads)
k_raster_faces(const float *__restrict__ vt, const int32_t *__restrict__ ft, uint32_t F,
               uint32_t T, uint32_t H, uint32_t W, uint32_t *__restrict__ face_id) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_face0 =
        (blockIdx.x * (kRasterThreads / 64u) + (threadIdx.x >> 6)) * kFacesPerWave;
    {
        const uint32_t face = wave_face0 + lane / kGroup;
        if (face < F) {
            const Face fc = load_face(vt, ft, face, T, H, W);
            if (fc.valid) {
                const Box b = face_box(fc, H, W);
                if (b.bw && b.bw * b.bh <= kSmallBox)
                    walk(fc, b, face, lane % kGroup, kGroup, W, face_id);
            }
        }
    }
    for (uint32_t g = 0; g < kFacesPerWave; ++g) {
        const uint32_t face = wave_face0 + g;  // wave-uniform
        if (face >= F) break;
        const Face fc = load_face(vt, ft, face, T, H, W);
        if (!fc.valid) continue;
        const Box b = face_box(fc, H, W);
        if (b.bw && b.bw * b.bh > kSmallBox) walk(fc, b, face, lane, 64u, W, face_id);
    }
}

// One lane per texel: barycentric weights of the centre in its face and the
// interpolated position.
__global__ void __launch_bounds__(256)
k_raster_interp(const float *__restrict__ vt, const int32_t *__restrict__ ft,
                const float *__restrict__ v, const int32_t *__restrict__ f,
                const int32_t *__restrict__ face_id, uint32_t F, uint32_t T, uint32_t V,
                uint32_t H, uint32_t W, float *__restrict__ xyz, float *__restrict__ bary) {
    const uint32_t n = H * W;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    float x = 0.0f, y = 0.0f, z = 0.0f, w1 = 0.0f, w2 = 0.0f;
    const uint32_t face = (uint32_t)face_id[t];
    if (face < F) {
        const Face fc = load_face(vt, ft, face, T, H, W);
        const uint32_t j0 = (uint32_t)f[3 * (size_t)face + 0];
        const uint32_t j1 = (uint32_t)f[3 * (size_t)face + 1];
        const uint32_t j2 = (uint32_t)f[3 * (size_t)face + 2];
        if (fc.valid && j0 < V && j1 < V && j2 < V) {
            const uint32_t row = t / W, col = t - row * W;
            float e0, e1, e2;
            edge_functions(fc, col, row, e0, e1, e2);
            w1 = e1 / fc.area;
            w2 = e2 / fc.area;
            const float w0 = (1.0f - w1) - w2;
            const float *a = v + 3 * (size_t)j0, *b = v + 3 * (size_t)j1, *c = v + 3 * (size_t)j2;
            x = (w0 * a[0] + w1 * b[0]) + w2 * c[0];
            y = (w0 * a[1] + w1 * b[1]) + w2 * c[1];
            z = (w0 * a[2] + w1 * b[2]) + w2 * c[2];
        }
    }
    xyz[3 * (size_t)t + 0] = x;
    xyz[3 * (size_t)t + 1] = y;
    xyz[3 * (size_t)t + 2] = z;
    if (bary) {
        bary[2 * (size_t)t + 0] = w1;
        bary[2 * (size_t)t + 1] = w2;
    }
}

// One lane per texel, one dilation step (dfhip.h for the neighbour order).
__global__ void __launch_bounds__(256)
k_texture_dilate(const uint8_t *__restrict__ src_rgb, const uint8_t *__restrict__ src_mask,
                 uint32_t H, uint32_t W, uint8_t *__restrict__ dst_rgb,
                 uint8_t *__restrict__ dst_mask) {
    const uint32_t n = H * W;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const int row = (int)(t / W), col = (int)(t - (t / W) * W);
    uint32_t from = t;
    uint8_t m = src_mask[t];
    if (!m) {
        // N, W, E, S, NW, NE, SW, SE
        const int dr[8] = {-1, 0, 0, 1, -1, -1, 1, 1};
        const int dc[8] = {0, -1, 1, 0, -1, 1, -1, 1};
#pragma unroll
        for (int k = 7; k >= 0; --k) {  // backwards: the first in order is kept last
            const int r = row + dr[k], c = col + dc[k];
            if (r >= 0 && r < (int)H && c >= 0 && c < (int)W) {
                const uint32_t u = (uint32_t)r * W + (uint32_t)c;
                if (src_mask[u]) {
                    from = u;
                    m = 1;
                }
            }
        }
    }
    dst_rgb[3 * (size_t)t + 0] = src_rgb[3 * (size_t)from + 0];
    dst_rgb[3 * (size_t)t + 1] = src_rgb[3 * (size_t)from + 1];
    dst_rgb[3 * (size_t)t + 2] = src_rgb[3 * (size_t)from + 2];
    dst_mask[t] = m;
}

// H W < 2^31 (texel indices are int32 / uint32 products) and non-zero.
inline bool texels_ok(const char *name, uint32_t H, uint32_t W) {
    const uint64_t n = (uint64_t)H * W;
    if (n == 0 || n >= (1ull << 31)) {
        set_error("%s: H*W must be in [1, 2^31), got %u x %u", name, H, W);
        return false;
    }
    return true;
}

}  // namespace tex
}  // namespace dfhip

using namespace dfhip;

extern "C" int dfhip_raster_uv_faces(const float *vt, const int32_t *ft, uint32_t F, uint32_t T,
                                     uint32_t H, uint32_t W, int32_t *face_id,
                                     dfhip_stream_t stream) {
    const char *name = "raster_uv_faces";
    if (!tex::texels_ok(name, H, W)) return DFHIP_EINVAL;
    if (F >= (1u << 31)) {
        set_error("%s: F must be below 2^31, got %u", name, F);
        return DFHIP_EINVAL;
    }
    if (!face_id || (F && (!vt || !ft || !T))) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    const size_t n = (size_t)H * W;
    if (hipMemsetAsync(face_id, 0xff, n * sizeof(int32_t), as_stream(stream)) != hipSuccess)
        return check_launch(name);
    if (F == 0) return check_launch(name);
    tex::k_raster_faces<<<ceil_div(F, tex::kFacesPerBlock), tex::kRasterThreads, 0,
                          as_stream(stream)>>>(vt, ft, F, T, H, W,
                                               reinterpret_cast<uint32_t *>(face_id));
    return check_launch(name);
}

extern "C" int dfhip_raster_uv_interp(const float *vt, const int32_t *ft, const float *v,
                                      const int32_t *f, const int32_t *face_id, uint32_t F,
                                      uint32_t T, uint32_t V, uint32_t H, uint32_t W, float *xyz,
                                      float *bary, dfhip_stream_t stream) {
    const char *name = "raster_uv_interp";
    if (!tex::texels_ok(name, H, W)) return DFHIP_EINVAL;
    if (F >= (1u << 31)) {
        set_error("%s: F must be below 2^31, got %u", name, F);
        return DFHIP_EINVAL;
    }
    if (!face_id || !xyz || (F && (!vt || !ft || !v || !f))) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    const uint32_t n = H * W;
    tex::k_raster_interp<<<ceil_div(n, 256u), 256, 0, as_stream(stream)>>>(
        vt, ft, v, f, face_id, F, T, V, H, W, xyz, bary);
    return check_launch(name);
}

extern "C" int dfhip_texture_dilate(const uint8_t *src_rgb, const uint8_t *src_mask, uint32_t H,
                                    uint32_t W, uint8_t *dst_rgb, uint8_t *dst_mask,
                                    dfhip_stream_t stream) {
    const char *name = "texture_dilate";
    if (!tex::texels_ok(name, H, W)) return DFHIP_EINVAL;
    if (!src_rgb || !src_mask || !dst_rgb || !dst_mask) {
        set_error("%s: null pointer", name);
        return DFHIP_EINVAL;
    }
    if (src_rgb == dst_rgb || src_mask == dst_mask) {
        set_error("%s: source and destination must be different buffers", name);
        return DFHIP_EINVAL;
    }
    const uint32_t n = H * W;
    tex::k_texture_dilate<<<ceil_div(n, 256u), 256, 0, as_stream(stream)>>>(
        src_rgb, src_mask, H, W, dst_rgb, dst_mask);
    return check_launch(name);
}
