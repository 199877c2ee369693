// f7 (the two-image caller, step 2): the skin colour transfer of Face_swap_with_two_imgs.py:537-572 for ct_mode 'lct' / 'mkl' on the device.
//   e4s_grey_morph : the flat (2r+1)^2 dilation / erosion of utils/morphology.py:23-198 ('geodesic' border) on float planes.  Separable: a 64 x 32 output tile
//                    with its halo lies in LDS, a row pass writes the horizontal extrema of every tile row into a second LDS plane, a column pass reads it with
//                    8 vertically adjacent outputs per thread (one LDS read feeds up to 8 comparisons).  Every LDS access of a wave covers consecutive dwords.
//                    2 (2r+1) comparisons per pixel where the window has (2r+1)^2; 4 bytes in and 4 out per pixel, the halo from L2.
//   e4s_ct_moments : the nine raw moments of v = (u8 * mask) / 255 per image in float64: per thread, wave shuffle, LDS, one partial row per workgroup.
//   e4s_ct_solve   : partial rows summed in a fixed order, means / covariances, cyclic Jacobi on the symmetric 3 x 3 matrices, the 3 x 3 map and the two offsets.
//   e4s_ct_apply   : the map per pixel, quantised like np.uint8(y * 255), and the composition D (1 - m) + q m in numpy's float32 arithmetic.
// No atomics anywhere: the same inputs give the same bits.
#include <float.h>
#include <math.h>

#include "common.h"

using namespace e4s;

namespace {

// ------------------------------------------------------------------------------------------------ grey morphology
constexpr int GM_TW = 64;                  // tile width = the wave
constexpr int GM_R = 8;                    // outputs per thread (vertical)
constexpr int GM_TH = 4 * GM_R;            // tile height = 4 waves x GM_R rows
constexpr int GM_MAXR = 16;

template <bool MIN>
__device__ __forceinline__ float gm_op(float a, float b) { return MIN ? fminf(a, b) : fmaxf(a, b); }

// LDS: tile [LH][LW] (LH = GM_TH + 2 r, LW = GM_TW + 2 ra, ra = r rounded up to 4 so that the tile's first column is a multiple of 4), then rows [LH][GM_TW].
// VEC: w % 4 == 0 and 16-byte aligned planes — a float4 of the tile lies wholly inside or wholly outside the image.
template <bool MIN, bool VEC>
__global__ __launch_bounds__(256) void grey_morph_kernel(float* __restrict__ out, const float* __restrict__ x, int h, int w, int r) {
    extern __shared__ float gm_lds[];
    const float ident = MIN ? INFINITY : -INFINITY;
    const int ra = (r + 3) & ~3;
    const int LW = GM_TW + 2 * ra, LH = GM_TH + 2 * r;
    float* __restrict__ tile = gm_lds;
    float* __restrict__ rows = gm_lds + LH * LW;
    const int plane = blockIdx.z;
    const int x0 = blockIdx.x * GM_TW, y0 = blockIdx.y * GM_TH;
    const float* __restrict__ src = x + (size_t)plane * h * w;
    if (VEC) {
        const int lw4 = LW >> 2;
        for (int e = threadIdx.x; e < LH * lw4; e += 256) {
            const int py = e / lw4, p4 = e - py * lw4;
            const int gy = y0 - r + py, gx = x0 - ra + 4 * p4;
            float4 v = make_float4(ident, ident, ident, ident);
            if (gy >= 0 && gy < h && gx >= 0 && gx + 3 < w) v = *reinterpret_cast<const float4*>(src + (size_t)gy * w + gx);
            *reinterpret_cast<float4*>(tile + py * LW + 4 * p4) = v;
        }
    } else {
        for (int e = threadIdx.x; e < LH * LW; e += 256) {
            const int py = e / LW, px = e - py * LW;
            const int gy = y0 - r + py, gx = x0 - ra + px;
            tile[e] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? src[(size_t)gy * w + gx] : ident;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < LH * GM_TW; e += 256) {          // row pass: rows[py][px] = op over tile[py][ra + px - r .. ra + px + r]
        const int py = e >> 6, px = e & 63;
        const float* __restrict__ p = tile + py * LW + ra - r + px;
        float m = ident;
        for (int j = 0; j <= 2 * r; ++j) m = gm_op<MIN>(m, p[j]);
        rows[e] = m;
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = (threadIdx.x >> 6) * GM_R;
    float acc[GM_R];
#pragma unroll
    for (int k = 0; k < GM_R; ++k) acc[k] = ident;
    const float* __restrict__ col = rows + ty * GM_TW + tx;
    for (int j = 0; j < 2 * r + GM_R; ++j) {                       // column pass: output row ty + k takes rows ty + k .. ty + k + 2 r
        const float v = col[j * GM_TW];
#pragma unroll
        for (int k = 0; k < GM_R; ++k)
            if (j >= k && j - k <= 2 * r) acc[k] = gm_op<MIN>(acc[k], v);
    }
    const int gx = x0 + tx;
#pragma unroll
    for (int k = 0; k < GM_R; ++k) {
        const int gy = y0 + ty + k;
        if (gx < w && gy < h) out[((size_t)plane * h + gy) * w + gx] = acc[k];
    }
}

// ------------------------------------------------------------------------------------------------ colour statistics
constexpr int CT_CHUNK = 4096;             // pixels per workgroup: 256 threads x 4 groups of 4 pixels
constexpr int CT_NMOM = 9;
constexpr int CT_NCOEF = 15;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// v = (float(u8) * m) / 255.0f exactly as numpy forms it: a rounded product, then a true division (no reciprocal, no contraction)
__device__ __forceinline__ float ct_value(uint8_t u, float m) {
#pragma clang fp contract(off)
    const float p = (float)u * m;
    return __fdiv_rn(p, 255.0f);
}

__device__ __forceinline__ void ct_accumulate(double (&s)[CT_NMOM], uint8_t r, uint8_t g, uint8_t b, float m) {
    const double v0 = (double)ct_value(r, m), v1 = (double)ct_value(g, m), v2 = (double)ct_value(b, m);
    s[0] += v0; s[1] += v1; s[2] += v2;
    s[3] += v0 * v0; s[4] += v0 * v1; s[5] += v0 * v2;
    s[6] += v1 * v1; s[7] += v1 * v2; s[8] += v2 * v2;
}

// 12 bytes = 4 RGB pixels as three dwords
struct Px4 { uint32_t a, b, c; };
__device__ __forceinline__ uint8_t px4_byte(const Px4& p, int i) {
    const uint32_t wd = i < 4 ? p.a : (i < 8 ? p.b : p.c);
    return (uint8_t)(wd >> (8 * (i & 3)));
}

template <bool VEC>
__global__ __launch_bounds__(256) void ct_moments_kernel(double* __restrict__ partial, const uint8_t* __restrict__ frame, const float* __restrict__ mask, int hw) {
    __shared__ double wave_part[4][CT_NMOM];
    const int b = blockIdx.y;
    const uint8_t* __restrict__ fr = frame + (size_t)b * hw * 3;
    const float* __restrict__ mk = mask + (size_t)b * hw;
    const int base = blockIdx.x * CT_CHUNK;
    double s[CT_NMOM];
#pragma unroll
    for (int k = 0; k < CT_NMOM; ++k) s[k] = 0.0;
    if (VEC) {                                                     // hw % 4 == 0: every group of 4 pixels is 12 + 16 aligned bytes
#pragma unroll
        for (int it = 0; it < CT_CHUNK / 1024; ++it) {
            const int p = base + (it * 256 + threadIdx.x) * 4;
            if (p < hw) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(fr + (size_t)p * 3);
                const Px4 px = {q[0], q[1], q[2]};
                const float4 m = *reinterpret_cast<const float4*>(mk + p);
                ct_accumulate(s, px4_byte(px, 0), px4_byte(px, 1), px4_byte(px, 2), m.x);
                ct_accumulate(s, px4_byte(px, 3), px4_byte(px, 4), px4_byte(px, 5), m.y);
                ct_accumulate(s, px4_byte(px, 6), px4_byte(px, 7), px4_byte(px, 8), m.z);
                ct_accumulate(s, px4_byte(px, 9), px4_byte(px, 10), px4_byte(px, 11), m.w);
            }
        }
    } else {
        for (int it = 0; it < CT_CHUNK / 256; ++it) {
            const int p = base + it * 256 + threadIdx.x;
            if (p < hw) ct_accumulate(s, fr[(size_t)p * 3], fr[(size_t)p * 3 + 1], fr[(size_t)p * 3 + 2], mk[p]);
        }
    }
#pragma unroll
    for (int k = 0; k < CT_NMOM; ++k) s[k] = wave_sum_f64(s[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < CT_NMOM; ++k) wave_part[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < CT_NMOM)
        partial[((size_t)b * gridDim.x + blockIdx.x) * CT_NMOM + threadIdx.x] =
            ((wave_part[0][threadIdx.x] + wave_part[1][threadIdx.x]) + wave_part[2][threadIdx.x]) + wave_part[3][threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ the 3 x 3 map
struct M3 { double m[3][3]; };

__device__ __forceinline__ M3 m3_mul(const M3& a, const M3& b) {
    M3 c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return c;
}
__device__ __forceinline__ M3 m3_t(const M3& a) {
    M3 c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[j][i];
    return c;
}

// one Jacobi rotation in the (P, Q) plane: a <- J^T a J, v <- v J
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(M3& a, M3& v) {
    const double apq = a.m[P][Q];
    if (apq == 0.0) return;
    const double theta = (a.m[Q][Q] - a.m[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    constexpr int K = 3 - P - Q;                                    // the third index
    const double akp = a.m[K][P], akq = a.m[K][Q];
    a.m[P][P] -= t * apq;
    a.m[Q][Q] += t * apq;
    a.m[P][Q] = a.m[Q][P] = 0.0;
    a.m[K][P] = a.m[P][K] = c * akp - s * akq;
    a.m[K][Q] = a.m[Q][K] = s * akp + c * akq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = v.m[k][P], vkq = v.m[k][Q];
        v.m[k][P] = c * vkp - s * vkq;
        v.m[k][Q] = s * vkp + c * vkq;
    }
}

// eigen-decomposition of a symmetric 3 x 3 matrix by cyclic Jacobi sweeps: a = v diag(lam) v^T.  Converges quadratically; 3 x 3 needs 5 - 7 sweeps.
__device__ __forceinline__ void jacobi_eigh(M3 a, M3& v, double (&lam)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v.m[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = a.m[0][1] * a.m[0][1] + a.m[0][2] * a.m[0][2] + a.m[1][2] * a.m[1][2];
        const double diag = a.m[0][0] * a.m[0][0] + a.m[1][1] * a.m[1][1] + a.m[2][2] * a.m[2][2];
        if (off <= 1e-36 * diag || off == 0.0) break;
        jacobi_rotate<0, 1>(a, v);
        jacobi_rotate<0, 2>(a, v);
        jacobi_rotate<1, 2>(a, v);
    }
    lam[0] = a.m[0][0]; lam[1] = a.m[1][1]; lam[2] = a.m[2][2];
}

// v diag(d) v^T
__device__ __forceinline__ M3 m3_vdvt(const M3& v, const double (&d)[3]) {
    M3 c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.m[i][j] = v.m[i][0] * d[0] * v.m[j][0] + v.m[i][1] * d[1] * v.m[j][1] + v.m[i][2] * d[2] * v.m[j][2];
    return c;
}

// raw moments (sums) -> mean and the centred second moment divided by `denom`
__device__ __forceinline__ void ct_mean_cov(const double (&s)[CT_NMOM], double n, double denom, double (&mu)[3], M3& cov) {
#pragma unroll
    for (int c = 0; c < 3; ++c) mu[c] = s[c] / n;
    const double raw[3][3] = {{s[3], s[4], s[5]}, {s[4], s[6], s[7]}, {s[5], s[7], s[8]}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) cov.m[i][j] = (raw[i][j] - n * mu[i] * mu[j]) / denom;
}

__global__ __launch_bounds__(64) void ct_solve_kernel(double* __restrict__ coef, const double* __restrict__ part_src, const double* __restrict__ part_trg,
                                                      int nchunk, double n, int mode) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double ss[CT_NMOM], st[CT_NMOM];
#pragma unroll
    for (int k = 0; k < CT_NMOM; ++k) ss[k] = st[k] = 0.0;
    for (int i = lane; i < nchunk; i += 64) {                      // lane l adds chunks l, l + 64, ... in that order; then the butterfly: a fixed order
        const double* ps = part_src + ((size_t)b * nchunk + i) * CT_NMOM;
        const double* pt = part_trg + ((size_t)b * nchunk + i) * CT_NMOM;
#pragma unroll
        for (int k = 0; k < CT_NMOM; ++k) { ss[k] += ps[k]; st[k] += pt[k]; }
    }
#pragma unroll
    for (int k = 0; k < CT_NMOM; ++k) { ss[k] = wave_sum_f64(ss[k]); st[k] = wave_sum_f64(st[k]); }
    if (lane != 0) return;
    double mus[3], mut[3], lam[3], d[3];
    M3 cs, ct, v, A;
    if (mode == 0) {
        // linear_color_transfer(src, trg, 'pca'): C = cov / N + 1e-5 I;  A = sqrtm(C_trg) inv(sqrtm(C_src))
        ct_mean_cov(ss, n, n, mus, cs);
        ct_mean_cov(st, n, n, mut, ct);
#pragma unroll
        for (int i = 0; i < 3; ++i) { cs.m[i][i] += 1e-5; ct.m[i][i] += 1e-5; }
        jacobi_eigh(cs, v, lam);
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = 1.0 / sqrt(fmax(lam[i], DBL_MIN));
        const M3 qs_inv = m3_vdvt(v, d);
        jacobi_eigh(ct, v, lam);
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = sqrt(fmax(lam[i], 0.0));
        A = m3_mul(m3_vdvt(v, d), qs_inv);
    } else {
        // color_transfer_mkl(src, trg): a, b = np.cov;  t = Ua Da^-1 Uc Dc Uc^T Da^-1 Ua^T with C = Da Ua^T b Ua Da;  y = (x - mu) t + mu_trg, so A = t^T
        const double denom = n > 1.0 ? n - 1.0 : 1.0;
        ct_mean_cov(ss, n, denom, mus, cs);
        ct_mean_cov(st, n, denom, mut, ct);
        M3 ua;
        double da[3], dai[3];
        jacobi_eigh(cs, ua, lam);
#pragma unroll
        for (int i = 0; i < 3; ++i) { da[i] = sqrt(fmax(lam[i], DBL_EPSILON)); dai[i] = 1.0 / da[i]; }
        M3 c = m3_mul(m3_mul(m3_t(ua), ct), ua);
        M3 csym;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) csym.m[i][j] = 0.5 * (da[i] * c.m[i][j] * da[j] + da[j] * c.m[j][i] * da[i]);
        jacobi_eigh(csym, v, lam);
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = sqrt(fmax(lam[i], DBL_EPSILON));
        const M3 s = m3_vdvt(v, d);
        M3 left;                                                    // Ua Da^-1
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) left.m[i][j] = ua.m[i][j] * dai[j];
        const M3 t = m3_mul(m3_mul(left, s), m3_t(left));
        A = m3_t(t);
    }
    double* __restrict__ o = coef + (size_t)b * CT_NCOEF;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = A.m[i][j];
#pragma unroll
    for (int i = 0; i < 3; ++i) { o[9 + i] = mus[i]; o[12 + i] = mut[i]; }
}

// ------------------------------------------------------------------------------------------------ apply + compose
struct CtCoef { double a[3][3], mus[3], mut[3]; };

// one pixel: q[c] = np.uint8(clip(float32(A (v - mu_src) + mu_trg), 0, 1) * 255), comp[c] = D (1 - m) + q m in float32, every operation rounded on its own
__device__ __forceinline__ void ct_pixel(const CtCoef& k, const uint8_t (&u)[3], float m, uint8_t (&q)[3], float (&comp)[3]) {
#pragma clang fp contract(off)
    double dv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dv[c] = (double)ct_value(u[c], m) - k.mus[c];
    const float om = 1.f - m;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double y = ((k.a[c][0] * dv[0] + k.a[c][1] * dv[1]) + k.a[c][2] * dv[2]) + k.mut[c];
        float yf = (float)y;
        yf = yf > 1.f ? 1.f : yf;
        yf = yf < 0.f ? 0.f : yf;                                    // (NaN cannot occur: the coefficients are finite)
        const float scaled = yf * 255.0f;
        q[c] = (uint8_t)scaled;
        const float lo = (float)u[c] * om, hi = (float)q[c] * m;
        comp[c] = lo + hi;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void ct_apply_kernel(float* __restrict__ composed, uint8_t* __restrict__ q_u8, const uint8_t* __restrict__ frame,
                                                       const float* __restrict__ mask, const double* __restrict__ coef, int hw) {
    const int b = blockIdx.y;
    CtCoef k;
    const double* __restrict__ cf = coef + (size_t)b * CT_NCOEF;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) k.a[i][j] = cf[i * 3 + j];
        k.mus[i] = cf[9 + i];
        k.mut[i] = cf[12 + i];
    }
    const uint8_t* __restrict__ fr = frame + (size_t)b * hw * 3;
    const float* __restrict__ mk = mask + (size_t)b * hw;
    float* __restrict__ co = composed + (size_t)b * 3 * hw;
    uint8_t* __restrict__ qo = q_u8 ? q_u8 + (size_t)b * hw * 3 : nullptr;
    if (VEC) {
        const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
        if (p >= hw) return;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(fr + (size_t)p * 3);
        const Px4 px = {src[0], src[1], src[2]};
        const float4 m4 = *reinterpret_cast<const float4*>(mk + p);
        const float m[4] = {m4.x, m4.y, m4.z, m4.w};
        float comp[4][3];
        uint8_t q[4][3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint8_t u[3] = {px4_byte(px, 3 * i), px4_byte(px, 3 * i + 1), px4_byte(px, 3 * i + 2)};
            ct_pixel(k, u, m[i], q[i], comp[i]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(co + (size_t)c * hw + p) = make_float4(comp[0][c], comp[1][c], comp[2][c], comp[3][c]);
        if (qo) {
            uint32_t wd[3] = {0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 12; ++i) wd[i >> 2] |= (uint32_t)q[i / 3][i % 3] << (8 * (i & 3));
            uint32_t* dst = reinterpret_cast<uint32_t*>(qo + (size_t)p * 3);
            dst[0] = wd[0]; dst[1] = wd[1]; dst[2] = wd[2];
        }
    } else {
        const int p = blockIdx.x * 256 + threadIdx.x;
        if (p >= hw) return;
        const uint8_t u[3] = {fr[(size_t)p * 3], fr[(size_t)p * 3 + 1], fr[(size_t)p * 3 + 2]};
        float comp[3];
        uint8_t q[3];
        ct_pixel(k, u, mk[p], q, comp);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            co[(size_t)c * hw + p] = comp[c];
            if (qo) qo[(size_t)p * 3 + c] = q[c];
        }
    }
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int e4s_grey_morph(float* out, const float* x, int planes, int h, int w, int radius, int op, void* stream) {
    E4S_REQUIRE(planes >= 0 && planes <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= (1 << 28), "grey_morph: bad size (planes 0..65535, h * w <= 2^28)");
    E4S_REQUIRE(radius >= 0 && radius <= GM_MAXR, "grey_morph: radius %d is not in 0..%d", radius, GM_MAXR);
    E4S_REQUIRE(op == 0 || op == 1, "grey_morph: op %d is not 0 (max) or 1 (min)", op);
    if (planes == 0) return 0;
    E4S_REQUIRE(out && x && out != x, "grey_morph: null or aliased tensor");
    E4S_REQUIRE(cdiv(h, GM_TH) <= 65535, "grey_morph: h too large");
    const int ra = (radius + 3) & ~3;
    const int LW = GM_TW + 2 * ra, LH = GM_TH + 2 * radius;
    const size_t lds = (size_t)(LH * LW + LH * GM_TW) * sizeof(float);          // <= 40 KiB at radius 16
    const dim3 grid(cdiv(w, GM_TW), cdiv(h, GM_TH), planes);
    const bool vec = (w % 4 == 0) && aligned(x, 16);
    hipStream_t st = (hipStream_t)stream;
    if (op == 0) {
        if (vec) hipLaunchKernelGGL((grey_morph_kernel<false, true>), grid, dim3(256), lds, st, out, x, h, w, radius);
        else hipLaunchKernelGGL((grey_morph_kernel<false, false>), grid, dim3(256), lds, st, out, x, h, w, radius);
    } else {
        if (vec) hipLaunchKernelGGL((grey_morph_kernel<true, true>), grid, dim3(256), lds, st, out, x, h, w, radius);
        else hipLaunchKernelGGL((grey_morph_kernel<true, false>), grid, dim3(256), lds, st, out, x, h, w, radius);
    }
    return check_launch("grey_morph");
}

extern "C" int e4s_ct_moments_scratch_bytes(int bs, int h, int w, int64_t* bytes) {
    E4S_REQUIRE(bytes, "ct_moments_scratch_bytes: null result");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= (1 << 28), "ct_moments_scratch_bytes: bad size (bs 0..65535, h * w <= 2^28)");
    *bytes = (int64_t)sizeof(double) * CT_NMOM * bs * cdiv(h * w, CT_CHUNK);
    return 0;
}

extern "C" int e4s_ct_moments(void* partial, const uint8_t* frame, const float* mask, int bs, int h, int w, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= (1 << 28), "ct_moments: bad size (bs 0..65535, h * w <= 2^28)");
    if (bs == 0) return 0;
    E4S_REQUIRE(partial && frame && mask && aligned(partial, 8), "ct_moments: null or misaligned tensor");
    const int hw = h * w;
    const dim3 grid(cdiv(hw, CT_CHUNK), bs);
    if (hw % 4 == 0 && aligned(frame, 4) && aligned(mask, 16))
        hipLaunchKernelGGL((ct_moments_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, (double*)partial, frame, mask, hw);
    else
        hipLaunchKernelGGL((ct_moments_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, (double*)partial, frame, mask, hw);
    return check_launch("ct_moments");
}

extern "C" int e4s_ct_solve(void* coef, const void* partial_src, const void* partial_trg, int bs, int h, int w, int mode, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= (1 << 28), "ct_solve: bad size (bs 0..65535, h * w <= 2^28)");
    E4S_REQUIRE(mode == 0 || mode == 1, "ct_solve: mode %d is not 0 (lct) or 1 (mkl)", mode);
    if (bs == 0) return 0;
    E4S_REQUIRE(coef && partial_src && partial_trg && aligned(coef, 8) && aligned(partial_src, 8) && aligned(partial_trg, 8), "ct_solve: null or misaligned tensor");
    const int hw = h * w;
    hipLaunchKernelGGL(ct_solve_kernel, dim3(bs), dim3(64), 0, (hipStream_t)stream, (double*)coef, (const double*)partial_src, (const double*)partial_trg, cdiv(hw, CT_CHUNK), (double)hw, mode);
    return check_launch("ct_solve");
}

extern "C" int e4s_ct_apply(float* composed, uint8_t* q_u8, const uint8_t* frame, const float* mask, const void* coef, int bs, int h, int w, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= (1 << 28), "ct_apply: bad size (bs 0..65535, h * w <= 2^28)");
    if (bs == 0) return 0;
    E4S_REQUIRE(composed && frame && mask && coef && aligned(coef, 8), "ct_apply: null or misaligned tensor");
    const int hw = h * w;
    hipStream_t st = (hipStream_t)stream;
    if (hw % 4 == 0 && aligned(frame, 4) && aligned(mask, 16) && aligned(composed, 16) && (!q_u8 || aligned(q_u8, 4)))
        hipLaunchKernelGGL((ct_apply_kernel<true>), dim3(cdiv(hw, 1024), bs), dim3(256), 0, st, composed, q_u8, frame, mask, (const double*)coef, hw);
    else
        hipLaunchKernelGGL((ct_apply_kernel<false>), dim3(cdiv(hw, 256), bs), dim3(256), 0, st, composed, q_u8, frame, mask, (const double*)coef, hw);
    return check_launch("ct_apply");
}
