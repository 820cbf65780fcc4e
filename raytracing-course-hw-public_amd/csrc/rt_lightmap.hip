// rt_lightmap.hip — the rasteriser of rt_lightmap_points (rt_abi.h): which texel centres of a light-map atlas lie in which triangle, and the bake
// point (position, normal) of every covered texel, in texel order.
//
//   lm_cover   : one wave per triangle walks the triangle's bounding texels, 64 at a time, evaluates the rule's three weights at each centre
//                and claims covered texels with an integer atomicMin on the triangle index: the lowest covering triangle owns the texel
//                whatever order the waves run in.
//   scan       : exclusive prefix count of the owned texels (rocPRIM), the deterministic compaction the accumulators' round lists use.
//   lm_scatter : one lane per owned texel evaluates the weights of its owner again and writes point and texel index at its prefix position.
//
// Everything is integer-ordered or single-owner: no float atomics, and the output does not depend on scheduling.
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "rt_dev_math.h"
#include "rt_kernels.h"

namespace {

struct LmTri {
    float ax, ay, bx, by, cx, cy;
};
DEV LmTri lm_tri(const float *lm_uv, uint32_t t) {
    const float *u = lm_uv + 6ull * t;
    return LmTri{u[0], u[1], u[2], u[3], u[4], u[5]};
}
DEV float lm_area(const LmTri &T) { return (T.bx - T.ax) * (T.cy - T.ay) - (T.by - T.ay) * (T.cx - T.ax); }
DEV bool lm_area_ok(float area) { return area != 0.0f && fabsf(area) <= 3.402823466e38f; } // not 0, not inf, not NaN
// the rule's weights of texel (x, y): true iff the centre is covered
DEV bool lm_weights(const LmTri &T, float area, uint32_t x, uint32_t y, uint32_t W, uint32_t H, float &w0, float &w1, float &w2) {
    const float cx = ((float)x + 0.5f) / (float)W;
    const float cy = ((float)y + 0.5f) / (float)H;
    w1 = ((cx - T.ax) * (T.cy - T.ay) - (cy - T.ay) * (T.cx - T.ax)) / area;
    w2 = ((T.bx - T.ax) * (cy - T.ay) - (T.by - T.ay) * (cx - T.ax)) / area;
    w0 = 1.0f - w1 - w2;
    return w0 >= 0 && w1 >= 0 && w2 >= 0;
}

__global__ __launch_bounds__(256) void lm_fill(uint32_t *owner, uint32_t n) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x)
        owner[q] = RT_NONE;
}

// The texels a triangle's wave visits must hold every texel the rule says it covers, and the rule is evaluated in rounded arithmetic: a
// centre outside the exact triangle can still get three weights >= 0. How far outside, per triangle (everything below in double):
//   ex, ey = the triangle's extents; Mx, My = the largest |difference| along an axis between a point of the atlas [0, 1]^2 or a vertex
//          and a vertex. A float difference of two floats is within 2^-24 relative, so is a product and the final subtraction: either
//          numerator and `area` are of the form D1*E1 - D2*E2 with |D1| <= Mx, |E1| <= ey, |D2| <= My, |E2| <= ex, off by at most
//          ((1 + 2^-24)^4 - 1) (|D1 E1| + |D2 E2|);
//   errN = 8 * 2^-24 * (Mx * ey + My * ex) + 2^-120 bounds that with a factor 2 to spare (the constant: products that underflow);
//   if |area| <= 64 * errN the signs of the weights are not to be trusted anywhere: the wave visits the whole atlas (a triangle far
//          smaller than a texel of a large atlas, or a sliver: slow, and the same answer);
//   else a division keeps the sign of its numerator, and w0 >= 0 says w1 + w2 <= 1 + 2^-24: computed weights that are all >= 0 put every
//          exact barycentric coordinate above -eta, eta = 8 * errN / |area| + 8 * 2^-24 < 1/4. A centre that is delta beyond the triangle's
//          extent `ext` along an axis has an exact coordinate <= -delta / (2 * (ext + delta)) (the coordinates sum to 1 and reproduce the
//          centre), which that contradicts once delta >= 4 * eta * ext.
//   So the box is the triangle's bounds grown by 4 * eta * ext + 4 * 2^-24 (the rounding of the centre itself), in texels rounded outwards and
//   grown by one more texel. For a triangle of a few texels eta is of the order 2^-24 * (texels across the atlas): the box is its bounds
//   and a texel around them.
struct LmBox {
    uint32_t x0, y0, w, h; // w == 0: visits nothing
};
DEV void lm_axis(double lo, double hi, double eta, uint32_t n, uint32_t &first, uint32_t &count) {
    const double grow = 4.0 * eta * (hi - lo) + 4.0 * 5.9604644775390625e-8;
    const double f = floor((lo - grow) * (double)n - 0.5) - 1.0, l = ceil((hi + grow) * (double)n - 0.5) + 1.0;
    const double fc = f < 0.0 ? 0.0 : f, lc = l > (double)n - 1.0 ? (double)n - 1.0 : l;
    if (!(fc <= lc)) { // wholly outside the atlas
        first = 0, count = 0;
        return;
    }
    first = (uint32_t)fc;
    count = (uint32_t)lc - first + 1u;
}
DEV LmBox lm_box(const LmTri &T, float area, uint32_t W, uint32_t H) {
    const double lox = fmin(fmin((double)T.ax, (double)T.bx), (double)T.cx), hix = fmax(fmax((double)T.ax, (double)T.bx), (double)T.cx);
    const double loy = fmin(fmin((double)T.ay, (double)T.by), (double)T.cy), hiy = fmax(fmax((double)T.ay, (double)T.by), (double)T.cy);
    const double ex = hix - lox, ey = hiy - loy;
    const double Mx = fmax(ex, fmax(fmax(fabs(lox), fabs(hix)), fmax(fabs(1.0 - lox), fabs(1.0 - hix))));
    const double My = fmax(ey, fmax(fmax(fabs(loy), fabs(hiy)), fmax(fabs(1.0 - loy), fabs(1.0 - hiy))));
    const double errN = 8.0 * 5.9604644775390625e-8 * (Mx * ey + My * ex) + 7.52316384526264e-37;
    const double a = fabs((double)area);
    LmBox B{0u, 0u, W, H};
    if (!(a > 64.0 * errN)) // (coordinates are finite here: a non-finite one makes `area` non-finite, which covers nothing)
        return B;
    const double eta = 8.0 * errN / a + 8.0 * 5.9604644775390625e-8;
    lm_axis(lox, hix, eta, W, B.x0, B.w);
    lm_axis(loy, hiy, eta, H, B.y0, B.h);
    if (B.h == 0u)
        B.w = 0u;
    return B;
}

__global__ __launch_bounds__(256) void lm_cover(const float *lm_uv, uint32_t n_tris, uint32_t W, uint32_t H, uint32_t *owner) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t t = wave; t < n_tris; t += n_waves) {
        const LmTri T = lm_tri(lm_uv, t);
        const float area = lm_area(T);
        if (!lm_area_ok(area))
            continue;
        const LmBox B = lm_box(T, area, W, H);
        const uint64_t n = (uint64_t)B.w * B.h;
        for (uint64_t i = lane; i < n; i += 64u) {
            const uint32_t by = (uint32_t)(i / B.w), x = B.x0 + (uint32_t)(i - (uint64_t)by * B.w), y = B.y0 + by;
            float w0, w1, w2;
            if (lm_weights(T, area, x, y, W, H, w0, w1, w2))
                atomicMin(owner + ((size_t)y * W + x), t);
        }
    }
}

struct LmOwned {
    __device__ uint32_t operator()(uint32_t o) const { return o != RT_NONE ? 1u : 0u; }
};

__global__ __launch_bounds__(256) void lm_scatter(const float *positions, const float *normals, const float *lm_uv, uint32_t W, uint32_t H, const uint32_t *owner,
                                                  const uint32_t *offs, uint4 *points_out, uint32_t *texels_out, uint32_t capacity, uint32_t *count) {
    const uint32_t n = W * H;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        const uint32_t t = owner[q], at = offs[q];
        if (q == n - 1u)
            *count = at + (t != RT_NONE ? 1u : 0u);
        if (t == RT_NONE || at >= capacity)
            continue;
        const LmTri T = lm_tri(lm_uv, t);
        float w0, w1, w2;
        (void)lm_weights(T, lm_area(T), q % W, q / W, W, H, w0, w1, w2);
        const float *P = positions + 9ull * t, *N = normals + 9ull * t;
        const V3 pos = w0 * ld3(P) + w1 * ld3(P + 3) + w2 * ld3(P + 6);
        const V3 nrm = norm(w0 * ld3(N) + w1 * ld3(N + 3) + w2 * ld3(N + 6));
        points_out[2ull * at] = make_uint4(__float_as_uint(pos.x), __float_as_uint(pos.y), __float_as_uint(pos.z), __float_as_uint(nrm.x));
        points_out[2ull * at + 1] = make_uint4(__float_as_uint(nrm.y), __float_as_uint(nrm.z), q, 0u);
        texels_out[at] = q;
    }
}

} // namespace

namespace rt {

size_t lightmap_scan_temp_bytes(size_t texels) {
    size_t bytes = 0;
    uint32_t *p = nullptr;
    (void)rocprim::exclusive_scan(nullptr, bytes, rocprim::make_transform_iterator(p, LmOwned{}), p, 0u, texels, rocprim::plus<uint32_t>(), (hipStream_t) nullptr);
    return bytes;
}

hipError_t launch_lightmap_points(const float *positions, const float *normals, const float *lm_uv, uint32_t n_tris, uint32_t width, uint32_t height, uint32_t *owner,
                                  uint32_t *offs, void *scan_temp, size_t scan_temp_bytes, void *points_out, uint32_t *texels_out, uint32_t capacity, uint32_t *count,
                                  int num_cus, hipStream_t stream) {
    const uint32_t n = width * height;
    const uint32_t cap_blocks = (uint32_t)num_cus * 16u;
    const uint32_t texel_blocks = std::max(1u, std::min<uint32_t>((n + 255u) / 256u, cap_blocks));
    hipError_t e;
    if ((e = RT_LAUNCH_CHECKED(lm_fill, dim3(texel_blocks), dim3(256), 0, stream, owner, n)) != hipSuccess)
        return e;
    const uint32_t tri_blocks = std::max(1u, std::min<uint32_t>((n_tris + 3u) / 4u, cap_blocks)); // four waves, four triangles per block
    if ((e = RT_LAUNCH_CHECKED(lm_cover, dim3(tri_blocks), dim3(256), 0, stream, lm_uv, n_tris, width, height, owner)) != hipSuccess)
        return e;
    if ((e = rocprim::exclusive_scan(scan_temp, scan_temp_bytes, rocprim::make_transform_iterator(owner, LmOwned{}), offs, 0u, (size_t)n, rocprim::plus<uint32_t>(),
                                     stream)) != hipSuccess)
        return e;
    return RT_LAUNCH_CHECKED(lm_scatter, dim3(texel_blocks), dim3(256), 0, stream, positions, normals, lm_uv, width, height, owner, offs, static_cast<uint4 *>(points_out),
                             texels_out, capacity, count);
}

} // namespace rt
