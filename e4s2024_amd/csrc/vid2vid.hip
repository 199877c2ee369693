// f17: face-vid2vid reenactment, stage 1 — the glue of KPDetector and of keypoint_transformation (swap_face_fine/face_vid2vid/modules/keypoint_detector.py:44-82,
// modules/util.py:55-71, 196-213, 372-418, drive_demo.py:67-180).  Everything here is small against the convolutions: one lane per output, or one workgroup per
// (sample, keypoint); float32 with every sum in a fixed order.
#include "common.h"
#include "spade_value.h"
#include "v2v_sample.h"

using namespace e4s;

// ------------------------------------------------------------------------------------ AntiAliasInterpolation2d: pad, depthwise k x k, [::s, ::s] in one pass
__global__ __launch_bounds__(256) void v2v_antialias_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ taps, int planes, int h,
                                                            int w, int ho, int wo, int k, int s) {
    const int64_t total = (int64_t)planes * ho * wo;
    const int r = k / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % wo);
        const int64_t q = i / wo;
        const int oy = (int)(q % ho);
        const float* xp = x + (size_t)(q / ho) * h * w;
        float acc = 0.f;
        for (int ky = 0; ky < k; ++ky) {
            const int iy = oy * s - r + ky;
            const bool row_ok = iy >= 0 && iy < h;
            for (int kx = 0; kx < k; ++kx) {
                const int ix = ox * s - r + kx;
                const bool ok = row_ok && ix >= 0 && ix < w;
                const float v = xp[ok ? (size_t)iy * w + ix : 0];
                acc = fmaf(taps[ky * k + kx], ok ? v : 0.f, acc);
            }
        }
        out[i] = acc;
    }
}

extern "C" int e4s_v2v_antialias_down(float* out, const float* x, const float* taps, int planes, int h, int w, int k, int s, void* stream) {
    E4S_REQUIRE(planes >= 0 && h >= 1 && w >= 1, "v2v_antialias_down: bad size");
    E4S_REQUIRE(k >= 1 && k <= 33 && (k & 1) && s >= 1, "v2v_antialias_down: k odd, 1 .. 33, and s >= 1, got k = %d, s = %d", k, s);
    if (planes == 0) return 0;
    E4S_REQUIRE(out && x && taps, "v2v_antialias_down: null tensor");
    const int ho = cdiv(h, s), wo = cdiv(w, s);
    hipLaunchKernelGGL(v2v_antialias_kernel, dim3(grid_1d((int64_t)planes * ho * wo)), dim3(256), 0, (hipStream_t)stream, out, x, taps, planes, h, w, ho, wo, k, s);
    return check_launch("v2v_antialias_down");
}

// ------------------------------------------------------------------------------------ nn.AvgPool2d(2)
__global__ __launch_bounds__(256) void avgpool2x2_kernel(float* __restrict__ out, const float* __restrict__ x, int planes, int h, int w, int ho, int wo) {
#pragma clang fp contract(off)
    const int64_t total = (int64_t)planes * ho * wo;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % wo);
        const int64_t q = i / wo;
        const int oy = (int)(q % ho);
        const float* xp = x + (size_t)(q / ho) * h * w + (size_t)(2 * oy) * w + 2 * ox;
        out[i] = (((xp[0] + xp[1]) + xp[w]) + xp[w + 1]) * 0.25f;
    }
}

extern "C" int e4s_avgpool2x2(float* out, const float* x, int planes, int h, int w, void* stream) {
    E4S_REQUIRE(planes >= 0 && h >= 2 && w >= 2, "avgpool2x2: the planes must be at least 2 x 2, got %d x %d", h, w);
    if (planes == 0) return 0;
    E4S_REQUIRE(out && x, "avgpool2x2: null tensor");
    const int ho = h / 2, wo = w / 2;
    hipLaunchKernelGGL(avgpool2x2_kernel, dim3(grid_1d((int64_t)planes * ho * wo)), dim3(256), 0, (hipStream_t)stream, out, x, planes, h, w, ho, wo);
    return check_launch("avgpool2x2");
}

// ------------------------------------------------------------------------------------ softmax expectation over the volume
// the four waves' values combined in wave order: every lane returns the same sum / max
template <class Op>
__device__ __forceinline__ float block4(float v, float* red, Op op) {
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                   // (red may still be read from the previous reduction)
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return op(op(op(red[0], red[1]), red[2]), red[3]);
}

template <bool JAC>
__global__ __launch_bounds__(256) void v2v_heatmap_kp_kernel(float* __restrict__ value, float* __restrict__ jacobian, float* __restrict__ heatmap,
                                                             const float* __restrict__ logits, const float* __restrict__ jac_planes, float temperature, int K,
                                                             int D, int H, int W) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int bk = blockIdx.x;                         // sample * K + keypoint
    const int n = D * H * W, hw = H * W;
    const float* lg = logits + (size_t)bk * n;
    const int tid = threadIdx.x;
    auto fmax2 = [](float a, float b) { return fmaxf(a, b); };
    auto add2 = [](float a, float b) { return a + b; };

    float m = -INFINITY;
    for (int i = tid; i < n; i += 256) m = fmaxf(m, lg[i] / temperature);
    m = block4(wave_max(m), red, fmax2);

    const float fx = (float)(W - 1), fy = (float)(H - 1), fz = (float)(D - 1);
    float se = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
    float sj[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) sj[j] = 0.f;
    const float* jp = JAC ? jac_planes + (size_t)bk * 9 * n : nullptr;
    for (int i = tid; i < n; i += 256) {
        const float e = expf(lg[i] / temperature - m);
        const int z = i / hw, r = i - z * hw;
        const int y = r / W, x = r - y * W;
        // make_coordinate_grid: 2 * (i / (n - 1)) - 1 in float32
        const float gx = 2.f * ((float)x / fx) - 1.f, gy = 2.f * ((float)y / fy) - 1.f, gz = 2.f * ((float)z / fz) - 1.f;
        se += e;
        sx += e * gx;
        sy += e * gy;
        sz += e * gz;
        if (JAC) {
#pragma unroll
            for (int j = 0; j < 9; ++j) sj[j] += e * jp[(size_t)j * n + i];
        }
    }
    se = block4(wave_sum(se), red, add2);
    sx = block4(wave_sum(sx), red, add2);
    sy = block4(wave_sum(sy), red, add2);
    sz = block4(wave_sum(sz), red, add2);
    if (JAC) {
#pragma unroll
        for (int j = 0; j < 9; ++j) sj[j] = block4(wave_sum(sj[j]), red, add2);
    }
    if (tid == 0) {
        value[(size_t)bk * 3 + 0] = sx / se;
        value[(size_t)bk * 3 + 1] = sy / se;
        value[(size_t)bk * 3 + 2] = sz / se;
        if (JAC) {
#pragma unroll
            for (int j = 0; j < 9; ++j) jacobian[(size_t)bk * 9 + j] = sj[j] / se;
        }
    }
    if (heatmap) {
        float* hp = heatmap + (size_t)bk * n;
        for (int i = tid; i < n; i += 256) hp[i] = expf(lg[i] / temperature - m) / se;
    }
}

extern "C" int e4s_v2v_heatmap_kp(float* value, float* jacobian, float* heatmap, const float* logits, const float* jac_planes, float temperature, int bs, int K,
                                  int D, int H, int W, void* stream) {
    E4S_REQUIRE(bs >= 0 && K >= 1 && D >= 2 && H >= 2 && W >= 2, "v2v_heatmap_kp: every extent of the volume must be at least 2 (the grid divides by n - 1), got %d x %d x %d",
                D, H, W);
    E4S_REQUIRE((int64_t)D * H * W <= 0x7fffffff && (int64_t)bs * K <= 0x7fffffff, "v2v_heatmap_kp: volume too large");
    E4S_REQUIRE(temperature > 0.f, "v2v_heatmap_kp: the temperature must be positive");
    E4S_REQUIRE((jacobian == nullptr) == (jac_planes == nullptr), "v2v_heatmap_kp: jacobian and jac_planes go together");
    if (bs == 0) return 0;
    E4S_REQUIRE(value && logits, "v2v_heatmap_kp: null tensor");
    if (jac_planes)
        hipLaunchKernelGGL(v2v_heatmap_kp_kernel<true>, dim3(bs * K), dim3(256), 0, (hipStream_t)stream, value, jacobian, heatmap, logits, jac_planes, temperature, K, D, H, W);
    else
        hipLaunchKernelGGL(v2v_heatmap_kp_kernel<false>, dim3(bs * K), dim3(256), 0, (hipStream_t)stream, value, jacobian, heatmap, logits, jac_planes, temperature, K, D, H, W);
    return check_launch("v2v_heatmap_kp");
}

// ------------------------------------------------------------------------------------ keypoint_transformation
constexpr int V2V_MAX_BINS = 1024;

// headpose_pred_to_degree: sum(softmax(row) * idx) * 3 - 99, one lane, in index order.  The 66 terms are summed in float64 and the result rounded once: the
// expectation is near 30 and ends as a difference against 99, so a float32 running sum would cost several of the few ulps the result has.
__device__ float v2v_degree(const float* __restrict__ row, int nbins) {
    float m = row[0];
    for (int i = 1; i < nbins; ++i) m = fmaxf(m, row[i]);
    double s = 0.0, d = 0.0;
    for (int i = 0; i < nbins; ++i) {
        const double e = exp((double)row[i] - (double)m);
        s += e;
        d += e * (double)i;
    }
    return (float)(d / s * 3.0 - 99.0);
}

__device__ __forceinline__ void v2v_mat3(const float (&a)[9], const float (&b)[9], float (&c)[9]) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}

__global__ __launch_bounds__(64) void v2v_kp_transform_kernel(float* __restrict__ value_out, float* __restrict__ jac_out, float* __restrict__ deg_out,
                                                              float* __restrict__ rot_out, const float* __restrict__ yaw, const float* __restrict__ pitch,
                                                              const float* __restrict__ roll, const float* __restrict__ deg_in, const float* __restrict__ t,
                                                              const float* __restrict__ exp, const float* __restrict__ kp, const float* __restrict__ jac, int kp_bs,
                                                              int K, int nbins) {
#pragma clang fp contract(off)
    __shared__ float deg[3];
    __shared__ float rot[9];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 3) {
        const float* rows = tid == 0 ? yaw : (tid == 1 ? pitch : roll);
        deg[tid] = rows ? v2v_degree(rows + (size_t)b * nbins, nbins) : deg_in[(size_t)b * 3 + tid];
    }
    __syncthreads();
    if (tid == 0) {
        // get_rotation_matrix: radians with 3.14, rot = pitch_mat yaw_mat roll_mat
        const float y = deg[0] / 180.f * 3.14f, p = deg[1] / 180.f * 3.14f, r = deg[2] / 180.f * 3.14f;
        const float cy = cosf(y), sy = sinf(y), cp = cosf(p), sp = sinf(p), cr = cosf(r), sr = sinf(r);
        const float pm[9] = {1.f, 0.f, 0.f, 0.f, cp, -sp, 0.f, sp, cp};
        const float ym[9] = {cy, 0.f, sy, 0.f, 1.f, 0.f, -sy, 0.f, cy};
        const float rm[9] = {cr, -sr, 0.f, sr, cr, 0.f, 0.f, 0.f, 1.f};
        float py[9], out[9];
        v2v_mat3(pm, ym, py);
        v2v_mat3(py, rm, out);
        for (int i = 0; i < 9; ++i) rot[i] = out[i];
    }
    __syncthreads();
    if (tid < 3 && deg_out) deg_out[(size_t)b * 3 + tid] = deg[tid];
    if (tid < 9 && rot_out) rot_out[(size_t)b * 9 + tid] = rot[tid];
    const size_t kb = kp_bs == 1 ? 0 : (size_t)b;
    for (int i = tid; i < K * 3; i += 64) {
        const int k = i / 3, m = i - k * 3;
        const float* q = kp + (kb * K + k) * 3;
        const float rv = (rot[m * 3] * q[0] + rot[m * 3 + 1] * q[1]) + rot[m * 3 + 2] * q[2];
        value_out[((size_t)b * K + k) * 3 + m] = (rv + t[(size_t)b * 3 + m]) + exp[((size_t)b * K + k) * 3 + m];
    }
    if (jac) {
        for (int i = tid; i < K * 9; i += 64) {
            const int k = i / 9, ms = i - k * 9, m = ms / 3, s = ms - m * 3;
            const float* q = jac + (kb * K + k) * 9;
            jac_out[((size_t)b * K + k) * 9 + ms] = (rot[m * 3] * q[s] + rot[m * 3 + 1] * q[3 + s]) + rot[m * 3 + 2] * q[6 + s];
        }
    }
}

extern "C" int e4s_v2v_kp_transform(float* value_out, float* jac_out, float* deg_out, float* rot_out, const float* yaw, const float* pitch, const float* roll,
                                    const float* deg_in, const float* t, const float* exp, const float* kp, const float* jac, int bs, int kp_bs, int K, int nbins,
                                    void* stream) {
    E4S_REQUIRE(bs >= 0 && K >= 1 && nbins >= 1 && nbins <= V2V_MAX_BINS, "v2v_kp_transform: bad size");
    E4S_REQUIRE(kp_bs == bs || kp_bs == 1, "v2v_kp_transform: the canonical keypoints have %d samples, expected %d or 1", kp_bs, bs);
    E4S_REQUIRE((jac == nullptr) == (jac_out == nullptr), "v2v_kp_transform: jac and jac_out go together");
    if (bs == 0) return 0;
    E4S_REQUIRE(value_out && t && exp && kp, "v2v_kp_transform: null tensor");
    E4S_REQUIRE((yaw && pitch && roll) || deg_in, "v2v_kp_transform: an angle without logits needs deg_in");
    hipLaunchKernelGGL(v2v_kp_transform_kernel, dim3(bs), dim3(64), 0, (hipStream_t)stream, value_out, jac_out, deg_out, rot_out, yaw, pitch, roll, deg_in, t, exp, kp,
                       jac, kp_bs, K, nbins);
    return check_launch("v2v_kp_transform");
}

// ==================================================================================== f18: the glue of DenseMotionNetwork (modules/dense_motion.py:34-128)
// nn.AvgPool3d((1, 2, 2)) of an encoder block, written through a batch stride into the last channels of the decoder buffer that concatenates it
__global__ __launch_bounds__(256) void avgpool2x2_strided_kernel(float* __restrict__ out, const float* __restrict__ x, int planes, int h, int w, int ho, int wo,
                                                                 size_t out_bs) {
#pragma clang fp contract(off)
    const int64_t per = (int64_t)planes * ho * wo;
    const int b = blockIdx.y;
    const float* xb = x + (size_t)b * planes * h * w;
    float* ob = out + (size_t)b * out_bs;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % wo);
        const int64_t q = i / wo;
        const int oy = (int)(q % ho);
        const float* xp = xb + (size_t)(q / ho) * h * w + (size_t)(2 * oy) * w + 2 * ox;
        ob[i] = (((xp[0] + xp[1]) + xp[w]) + xp[w + 1]) * 0.25f;
    }
}

extern "C" int e4s_avgpool2x2_strided(float* out, const float* x, int bs, int planes, int h, int w, int64_t out_bstride, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && planes >= 0 && h >= 2 && w >= 2, "avgpool2x2_strided: the planes must be at least 2 x 2, got %d x %d", h, w);
    E4S_REQUIRE(out_bstride >= (int64_t)planes * (h / 2) * (w / 2), "avgpool2x2_strided: the batch stride is smaller than a sample");
    if (bs == 0 || planes == 0) return 0;
    E4S_REQUIRE(out && x, "avgpool2x2_strided: null tensor");
    const int ho = h / 2, wo = w / 2;
    hipLaunchKernelGGL(avgpool2x2_strided_kernel, dim3(grid_1d((int64_t)planes * ho * wo), bs), dim3(256), 0, (hipStream_t)stream, out, x, planes, h, w, ho, wo,
                       (size_t)out_bstride);
    return check_launch("avgpool2x2_strided");
}

constexpr int V2V_MAX_MOTIONS = 32;          // K + 1, the background included

// make_coordinate_grid at a position, (x, y, z) order: 2 * (i / (n - 1)) - 1 in float32
__device__ __forceinline__ void v2v_grid(float (&g)[3], int pos, int H, int W, float fx, float fy, float fz) {
#pragma clang fp contract(off)
    const int hw = H * W;
    const int z = pos / hw, r = pos - z * hw;
    const int y = r / W, x = r - y * W;
    g[0] = 2.f * ((float)x / fx) - 1.f;
    g[1] = 2.f * ((float)y / fy) - 1.f;
    g[2] = 2.f * ((float)z / fz) - 1.f;
}

// J = jac_s inv(jac_d) of one keypoint: the inverse from the adjugate and the product in float64, rounded once
__device__ void v2v_motion_jac(float* __restrict__ out9, const float* __restrict__ js, const float* __restrict__ jd) {
    const double a = jd[0], b = jd[1], c = jd[2], d = jd[3], e = jd[4], f = jd[5], g = jd[6], h = jd[7], i = jd[8];
    const double A = e * i - f * h, B = c * h - b * i, C = b * f - c * e;
    const double Dd = f * g - d * i, E = a * i - c * g, F = c * d - a * f;
    const double G = d * h - e * g, Hh = b * g - a * h, I = a * e - b * d;
    const double det = a * A + b * Dd + c * G;
    const double inv[9] = {A / det, B / det, C / det, Dd / det, E / det, F / det, G / det, Hh / det, I / det};
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q)
            out9[r * 3 + q] = (float)(((double)js[r * 3] * inv[q] + (double)js[r * 3 + 1] * inv[3 + q]) + (double)js[r * 3 + 2] * inv[6 + q]);
}

// the sparse motion of a keypoint at grid point g: J (g - kp_d) + kp_s (J null: the identity), the one function both kernels call: the same bits
__device__ __forceinline__ void v2v_sparse_motion(float (&m)[3], const float (&g)[3], const float* kd, const float* ks, const float* J) {
#pragma clang fp contract(off)
    const float c0 = g[0] - kd[0], c1 = g[1] - kd[1], c2 = g[2] - kd[2];
    if (J) {
        m[0] = ((J[0] * c0 + J[1] * c1) + J[2] * c2) + ks[0];
        m[1] = ((J[3] * c0 + J[4] * c1) + J[5] * c2) + ks[1];
        m[2] = ((J[6] * c0 + J[7] * c1) + J[8] * c2) + ks[2];
    } else {
        m[0] = c0 + ks[0];
        m[1] = c1 + ks[1];
        m[2] = c2 + ks[2];
    }
}

__global__ __launch_bounds__(256) void v2v_motion_input_kernel(float* __restrict__ out, const float* __restrict__ feature, const float* __restrict__ kp_d,
                                                               const float* __restrict__ kp_s, const float* __restrict__ jac_d,
                                                               const float* __restrict__ jac_s, int K, int c, int D, int H, int W, size_t out_bs) {
#pragma clang fp contract(off)
    __shared__ float sJ[9];
    __shared__ float skp[6];
    const int k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int n = D * H * W;
    if (k > 0) {
        const size_t bk = (size_t)b * K + (k - 1);
        if (tid == 0 && jac_d) v2v_motion_jac(sJ, jac_s + bk * 9, jac_d + bk * 9);
        if (tid >= 64 && tid < 67) skp[tid - 64] = kp_d[bk * 3 + (tid - 64)];
        if (tid >= 128 && tid < 131) skp[3 + tid - 128] = kp_s[bk * 3 + (tid - 128)];
    }
    __syncthreads();
    const int pos = blockIdx.x * 256 + tid;
    if (pos >= n) return;
    float g[3], m[3];
    v2v_grid(g, pos, H, W, (float)(W - 1), (float)(H - 1), (float)(D - 1));
    float heat = 0.f;
    if (k == 0) {
        m[0] = g[0]; m[1] = g[1]; m[2] = g[2];
    } else {
        v2v_sparse_motion(m, g, skp, skp + 3, jac_d ? sJ : nullptr);
        // kp2gaussian(kp_driving) - kp2gaussian(kp_source), kp_variance 0.01
        const float d0 = g[0] - skp[0], d1 = g[1] - skp[1], d2 = g[2] - skp[2];
        const float s0 = g[0] - skp[3], s1 = g[1] - skp[4], s2 = g[2] - skp[5];
        const float gd = expf(-0.5f * ((d0 * d0 + d1 * d1) + d2 * d2) / 0.01f);
        const float gs = expf(-0.5f * ((s0 * s0 + s1 * s1) + s2 * s2) / 0.01f);
        heat = gd - gs;
    }
    float* ob = out + (size_t)b * out_bs + (size_t)k * (c + 1) * n + pos;
    ob[0] = heat;
    float wgt[8];
    int off[8];
    const unsigned okm = v2v_trilinear_taps(wgt, off, m[0], m[1], m[2], D, H, W);
    const float* fb = feature + (size_t)b * c * n;
    for (int j = 0; j < c; ++j) {
        const float* fp = fb + (size_t)j * n;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float v = fp[off[t]];
            if ((okm >> t) & 1u) acc = acc + v * wgt[t];
        }
        ob[(size_t)(1 + j) * n] = acc;
    }
}

static int v2v_motion_checked(const char* what, const void* kp_d, const void* kp_s, const void* jac_d, const void* jac_s, int bs, int K, int D, int H, int W) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && K >= 1 && K + 1 <= V2V_MAX_MOTIONS, "%s: num_kp + 1 = %d motions: 2 .. %d are supported", what, K + 1, V2V_MAX_MOTIONS);
    E4S_REQUIRE(D >= 2 && H >= 2 && W >= 2, "%s: every extent of the volume must be at least 2 (the grid divides by n - 1), got %d x %d x %d", what, D, H, W);
    E4S_REQUIRE((int64_t)D * H * W <= 0x7fffffff - 256, "%s: volume too large", what);
    E4S_REQUIRE((jac_d == nullptr) == (jac_s == nullptr), "%s: jac_d and jac_s go together", what);
    E4S_REQUIRE(bs == 0 || (kp_d && kp_s), "%s: null tensor", what);
    return 0;
}

extern "C" int e4s_v2v_motion_input(float* out, const float* feature, const float* kp_d, const float* kp_s, const float* jac_d, const float* jac_s, int bs, int K,
                                    int c, int D, int H, int W, int64_t out_bstride, void* stream) {
    if (int st = v2v_motion_checked("v2v_motion_input", kp_d, kp_s, jac_d, jac_s, bs, K, D, H, W)) return st;
    E4S_REQUIRE(c >= 1 && (int64_t)c * D * H * W <= 0x7fffffff, "v2v_motion_input: bad channel count");
    E4S_REQUIRE(out_bstride >= (int64_t)(K + 1) * (c + 1) * D * H * W, "v2v_motion_input: the batch stride is smaller than a sample");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && feature, "v2v_motion_input: null tensor");
    const int n = D * H * W;
    hipLaunchKernelGGL(v2v_motion_input_kernel, dim3(cdiv(n, 256), K + 1, bs), dim3(256), 0, (hipStream_t)stream, out, feature, kp_d, kp_s, jac_d, jac_s, K, c, D,
                       H, W, (size_t)out_bstride);
    return check_launch("v2v_motion_input");
}

__global__ __launch_bounds__(256) void v2v_motion_combine_kernel(float* __restrict__ mask, float* __restrict__ deformation, const float* __restrict__ logits,
                                                                 const float* __restrict__ kp_d, const float* __restrict__ kp_s,
                                                                 const float* __restrict__ jac_d, const float* __restrict__ jac_s, int K, int D, int H, int W) {
#pragma clang fp contract(off)
    __shared__ float sJ[(V2V_MAX_MOTIONS - 1) * 9];
    __shared__ float skd[(V2V_MAX_MOTIONS - 1) * 3];
    __shared__ float sks[(V2V_MAX_MOTIONS - 1) * 3];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = D * H * W;
    if (tid < K && jac_d) v2v_motion_jac(sJ + tid * 9, jac_s + ((size_t)b * K + tid) * 9, jac_d + ((size_t)b * K + tid) * 9);
    if (tid >= 64 && tid < 64 + K * 3) {
        skd[tid - 64] = kp_d[(size_t)b * K * 3 + (tid - 64)];
        sks[tid - 64] = kp_s[(size_t)b * K * 3 + (tid - 64)];
    }
    __syncthreads();
    const int pos = blockIdx.x * 256 + tid;
    if (pos >= n) return;
    const float* lg = logits + (size_t)b * (K + 1) * n + pos;
    float* mk = mask + (size_t)b * (K + 1) * n + pos;
    float mx = lg[0];
    for (int k = 1; k <= K; ++k) mx = fmaxf(mx, lg[(size_t)k * n]);
    float sum = 0.f;
    for (int k = 0; k <= K; ++k) sum = sum + expf(lg[(size_t)k * n] - mx);
    float g[3];
    v2v_grid(g, pos, H, W, (float)(W - 1), (float)(H - 1), (float)(D - 1));
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int k = 0; k <= K; ++k) {
        const float w = expf(lg[(size_t)k * n] - mx) / sum;
        mk[(size_t)k * n] = w;
        float m[3];
        if (k == 0) {
            m[0] = g[0]; m[1] = g[1]; m[2] = g[2];
        } else {
            v2v_sparse_motion(m, g, skd + (k - 1) * 3, sks + (k - 1) * 3, jac_d ? sJ + (k - 1) * 9 : nullptr);
        }
        a0 = a0 + m[0] * w;
        a1 = a1 + m[1] * w;
        a2 = a2 + m[2] * w;
    }
    float* dp = deformation + ((size_t)b * n + pos) * 3;
    dp[0] = a0; dp[1] = a1; dp[2] = a2;
}

extern "C" int e4s_v2v_motion_combine(float* mask, float* deformation, const float* logits, const float* kp_d, const float* kp_s, const float* jac_d,
                                      const float* jac_s, int bs, int K, int D, int H, int W, void* stream) {
    if (int st = v2v_motion_checked("v2v_motion_combine", kp_d, kp_s, jac_d, jac_s, bs, K, D, H, W)) return st;
    E4S_REQUIRE((int64_t)(K + 1) * D * H * W <= 0x7fffffff, "v2v_motion_combine: volume too large");
    if (bs == 0) return 0;
    E4S_REQUIRE(mask && deformation && logits, "v2v_motion_combine: null tensor");
    const int n = D * H * W;
    hipLaunchKernelGGL(v2v_motion_combine_kernel, dim3(cdiv(n, 256), bs), dim3(256), 0, (hipStream_t)stream, mask, deformation, logits, kp_d, kp_s, jac_d, jac_s, K, D,
                       H, W);
    return check_launch("v2v_motion_combine");
}

// ==================================================================================== f19: the glue of the generator's feature warp (modules/generator.py:201-244)
constexpr int V2V_DEFORM_CG = 4;             // channels per workgroup row of e4s_v2v_deform: a position's taps are computed once per that many channels

// deform_input: F.grid_sample(feature [bs][C][D][H][W], deformation [bs][D][H][W][3]) at its defaults, written as [bs][C D][H][W] (the same element order: the
// reference's view costs nothing).  One position per lane: the 64 lanes of a wave gather from neighbouring addresses (a deformation is smooth) and store 256
// contiguous bytes.  A form with four positions per lane and 16-byte stores was measured 1.7x slower at [32][16][64][64] (tools/probes/deform_forms_probe.hip, profiles/f19_deform_forms_probe.txt): a lane that owns four neighbouring
// positions spreads every gather instruction of its wave over four times the cache lines.
__global__ __launch_bounds__(256) void v2v_deform_kernel(float* __restrict__ out, const float* __restrict__ feature, const float* __restrict__ deformation, int C,
                                                         int D, int H, int W, size_t feat_bs, size_t out_bs) {
#pragma clang fp contract(off)
    const int b = blockIdx.z;
    const int n = D * H * W;
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= n) return;
    const int c0 = blockIdx.y * V2V_DEFORM_CG;
    const int c1 = min(c0 + V2V_DEFORM_CG, C);
    float wgt[8];
    int off[8];
    const float* dp = deformation + ((size_t)b * n + pos) * 3;
    const unsigned okm = v2v_trilinear_taps(wgt, off, dp[0], dp[1], dp[2], D, H, W);
    const float* fb = feature + (size_t)b * feat_bs;
    float* ob = out + (size_t)b * out_bs + pos;
    for (int j = c0; j < c1; ++j) {
        const float* fp = fb + (size_t)j * n;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float v = fp[off[t]];
            if ((okm >> t) & 1u) acc = acc + v * wgt[t];
        }
        ob[(size_t)j * n] = acc;
    }
}

static inline bool v2v_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int e4s_v2v_deform(float* out, const float* feature, const float* deformation, int bs, int C, int D, int H, int W, int64_t feat_bstride,
                              int64_t out_bstride, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && C >= 1 && D >= 1 && H >= 1 && W >= 1, "v2v_deform: bad size");
    E4S_REQUIRE((int64_t)C * D * H * W <= 0x7fffffff - 1024 && cdiv(C, V2V_DEFORM_CG) <= 65535, "v2v_deform: volume too large");
    E4S_REQUIRE(feat_bstride == 0 || feat_bstride >= (int64_t)C * D * H * W, "v2v_deform: the feature's batch stride is 0 (one feature for every sample) or at least a sample");
    E4S_REQUIRE(out_bstride >= (int64_t)C * D * H * W, "v2v_deform: the output's batch stride is smaller than a sample");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && feature && deformation, "v2v_deform: null tensor");
    hipLaunchKernelGGL(v2v_deform_kernel, dim3(cdiv(D * H * W, 256), cdiv(C, V2V_DEFORM_CG), bs), dim3(256), 0, (hipStream_t)stream, out, feature, deformation, C, D, H,
                       W, (size_t)feat_bstride, (size_t)out_bstride);
    return check_launch("v2v_deform");
}

// ResBlock3d's norm1 + ReLU in front of conv1: relu(x scale[c] + shift[c]) over [bs][C][n], the product and the sum as one fused multiply-add
template <int V>
__global__ __launch_bounds__(256) void v2v_bn_relu_kernel(float* out, const float* x, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, int64_t total, int C, int n) {
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (int64_t)gridDim.x * 256 * V) {
        const int c = (int)((i / n) % C);              // V = 4 only with n % 4 == 0: the four elements share a channel
        const float s = scale[c], t = shift[c];
        if constexpr (V == 4) {
            const float4 v = *reinterpret_cast<const float4*>(x + i);
            *reinterpret_cast<float4*>(out + i) = make_float4(fmaxf(fmaf(v.x, s, t), 0.f), fmaxf(fmaf(v.y, s, t), 0.f), fmaxf(fmaf(v.z, s, t), 0.f),
                                                              fmaxf(fmaf(v.w, s, t), 0.f));
        } else {
            out[i] = fmaxf(fmaf(x[i], s, t), 0.f);
        }
    }
}

extern "C" int e4s_v2v_bn_relu(float* out, const float* x, const float* scale, const float* shift, int bs, int C, int n, void* stream) {
    E4S_REQUIRE(bs >= 0 && C >= 1 && n >= 1, "v2v_bn_relu: bad size");
    const int64_t total = (int64_t)bs * C * n;
    if (total == 0) return 0;
    E4S_REQUIRE(out && x && scale && shift, "v2v_bn_relu: null tensor");
    if (n % 4 == 0 && v2v_aligned16(out) && v2v_aligned16(x))
        hipLaunchKernelGGL(v2v_bn_relu_kernel<4>, dim3(grid_1d(total / 4)), dim3(256), 0, (hipStream_t)stream, out, x, scale, shift, total, C, n);
    else
        hipLaunchKernelGGL(v2v_bn_relu_kernel<1>, dim3(grid_1d(total)), dim3(256), 0, (hipStream_t)stream, out, x, scale, shift, total, C, n);
    return check_launch("v2v_bn_relu");
}

// out = x [bs][C][hw] * occ [bs][1][hw]; out may be x (every element is read once, by the lane that writes it)
template <int V>
__global__ __launch_bounds__(256) void v2v_occlude_kernel(float* out, const float* x, const float* __restrict__ occ, int64_t total, int C, int hw) {
    const int64_t chw = (int64_t)C * hw;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (int64_t)gridDim.x * 256 * V) {
        const int64_t b = i / chw;
        const int p = (int)(i % hw);                   // V = 4 only with hw % 4 == 0: the four elements lie in one plane
        const float* op = occ + b * hw + p;
        if constexpr (V == 4) {
            const float4 v = *reinterpret_cast<const float4*>(x + i), o = *reinterpret_cast<const float4*>(op);
            *reinterpret_cast<float4*>(out + i) = make_float4(v.x * o.x, v.y * o.y, v.z * o.z, v.w * o.w);
        } else {
            out[i] = x[i] * op[0];
        }
    }
}

extern "C" int e4s_v2v_occlude(float* out, const float* x, const float* occ, int bs, int C, int hw, void* stream) {
    E4S_REQUIRE(bs >= 0 && C >= 1 && hw >= 1, "v2v_occlude: bad size");
    const int64_t total = (int64_t)bs * C * hw;
    if (total == 0) return 0;
    E4S_REQUIRE(out && x && occ, "v2v_occlude: null tensor");
    if (hw % 4 == 0 && v2v_aligned16(out) && v2v_aligned16(x) && v2v_aligned16(occ))
        hipLaunchKernelGGL(v2v_occlude_kernel<4>, dim3(grid_1d(total / 4)), dim3(256), 0, (hipStream_t)stream, out, x, occ, total, C, hw);
    else
        hipLaunchKernelGGL(v2v_occlude_kernel<1>, dim3(grid_1d(total)), dim3(256), 0, (hipStream_t)stream, out, x, occ, total, C, hw);
    return check_launch("v2v_occlude");
}

// ==================================================================================== f20: the glue of the SPADEDecoder (modules/generator.py:120-158, modules/util.py:421-481)
// spade_norm: the modulation of one or two SPADE norms that normalise the same x (norm_0, and norm_s of a learned shortcut), x read once, the decoder's nearest x2
// folded into the read: x [bs][C][h / UP][w / UP] at (y / UP, x / UP).  The statistics are those of the low-resolution plane: a nearest x2 plane repeats every value
// four times, its mean and biased variance are the same.  Every element is spade_value (spade_value.h), e4s_spade_modulate's function: the same bits.
// A group is V consecutive OUTPUT elements of one row (V = 4: w % 4 == 0, hence w / UP even: the two x values of a group are one 8-byte read).  n: groups in all.
template <int V, int UP>
__global__ __launch_bounds__(256) void v2v_spade_norm_kernel(float* __restrict__ out_a, float* __restrict__ out_s, const float* __restrict__ x,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gb_a,
                                                             const float* __restrict__ gb_s, int64_t n, int C, int h, int w) {
    const int hw = h * w, gpp = hw / V, ws = w / UP;
    const int64_t xhw = (int64_t)(h / UP) * ws;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t plane = g / gpp;
        const int i0 = (int)(g - plane * gpp) * V;
        const int y = i0 / w, x0 = i0 - y * w;
        const float m = mean[plane], r = rstd[plane];
        const float* xp = x + plane * xhw + (int64_t)(y / UP) * ws + x0 / UP;
        const int64_t b = plane / C, c = plane - b * C;
        const int64_t go = (b * 2 * C + c) * hw + i0, oo = plane * hw + i0;
        float xv[V];
        if constexpr (V == 4) {
            if constexpr (UP == 1) {
                const float4 q = *reinterpret_cast<const float4*>(xp);
                xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
            } else {
                const float2 q = *reinterpret_cast<const float2*>(xp);
                xv[0] = q.x; xv[1] = q.x; xv[2] = q.y; xv[3] = q.y;
            }
        } else {
            xv[0] = xp[0];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {                                           // k = 0: norm_0 with the leaky activation; k = 1: norm_s without
            const float* gb = k ? gb_s : gb_a;
            float* out = k ? out_s : out_a;
            if (!gb) continue;
            const float slope = k ? 1.f : 0.2f;
            const float *gp = gb + go, *bp = gp + (int64_t)C * hw;
            if constexpr (V == 4) {
                const float4 ga = *reinterpret_cast<const float4*>(gp), be = *reinterpret_cast<const float4*>(bp);
                *reinterpret_cast<float4*>(out + oo) =
                    make_float4(spade_value(xv[0], m, r, ga.x, be.x, true, slope), spade_value(xv[1], m, r, ga.y, be.y, true, slope),
                                spade_value(xv[2], m, r, ga.z, be.z, true, slope), spade_value(xv[3], m, r, ga.w, be.w, true, slope));
            } else {
                out[oo] = spade_value(xv[0], m, r, gp[0], bp[0], true, slope);
            }
        }
    }
}

extern "C" int e4s_v2v_spade_norm(float* out_a, float* out_s, const float* x, const float* mean, const float* rstd, const float* gb_a, const float* gb_s, int bs,
                                  int C, int h, int w, int up, void* stream) {
    E4S_REQUIRE(bs >= 0 && C >= 1 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "v2v_spade_norm: bad size");
    E4S_REQUIRE((up == 1 || up == 2) && h % up == 0 && w % up == 0, "v2v_spade_norm: up is 1 or 2 and divides h = %d and w = %d", h, w);
    E4S_REQUIRE((out_s == nullptr) == (gb_s == nullptr), "v2v_spade_norm: out_s and gb_s go together");
    if (bs == 0) return 0;
    E4S_REQUIRE(out_a && x && mean && rstd && gb_a, "v2v_spade_norm: null tensor");
    const int64_t n = (int64_t)bs * C * h * w;
    const bool vec = w % 4 == 0 && v2v_aligned16(out_a) && v2v_aligned16(out_s) && v2v_aligned16(x) && v2v_aligned16(gb_a) && v2v_aligned16(gb_s);
    hipStream_t st = (hipStream_t)stream;
    if (vec && up == 1)
        hipLaunchKernelGGL((v2v_spade_norm_kernel<4, 1>), dim3(grid_1d(n / 4)), dim3(256), 0, st, out_a, out_s, x, mean, rstd, gb_a, gb_s, n / 4, C, h, w);
    else if (vec)
        hipLaunchKernelGGL((v2v_spade_norm_kernel<4, 2>), dim3(grid_1d(n / 4)), dim3(256), 0, st, out_a, out_s, x, mean, rstd, gb_a, gb_s, n / 4, C, h, w);
    else if (up == 1)
        hipLaunchKernelGGL((v2v_spade_norm_kernel<1, 1>), dim3(grid_1d(n)), dim3(256), 0, st, out_a, out_s, x, mean, rstd, gb_a, gb_s, n, C, h, w);
    else
        hipLaunchKernelGGL((v2v_spade_norm_kernel<1, 2>), dim3(grid_1d(n)), dim3(256), 0, st, out_a, out_s, x, mean, rstd, gb_a, gb_s, n, C, h, w);
    return check_launch("v2v_spade_norm");
}

// image_head: out [bs][3][H][W] = sigmoid(conv3x3(leaky_0.2(x), weight [3][cin][3][3], zero pad 1) + bias): the decoder's last three lines.  Three output channels
// would waste an output-channel tile of the MFMA kernel; this is the form of the RRDB tail (csrc/rrdb.hip): a workgroup owns a 64 x 16 tile, a lane four pixels of
// a row and all three outputs; eight input channels at a time are staged in LDS with their halo, the activation applied once per staged value (0 stays 0: the
// padding), their 27 weights per channel beside them.  Exact float32: every sum starts at the bias and takes 9 cin fused multiply-adds in (input channel, row,
// column) order; the sigmoid is 1 / (1 + expf(-v)).
constexpr int HEAD_TW = 64, HEAD_TH = 16;        // the tile of a workgroup: 16 lanes x 4 pixels across, 16 rows
constexpr int HEAD_CH = 8;                       // input channels per LDS chunk
constexpr int HEAD_LW = 72;                      // LDS row: the left halo at column 3, the tile at 4 .. 67 (16-byte aligned), the right halo at 68
constexpr int HEAD_LH = HEAD_TH + 2;
constexpr int HEAD_WROW = 28;                    // 27 weights of an input channel, [row][column][output], padded to seven 16-byte reads

__device__ __forceinline__ float v2v_leaky02(float v) { return v > 0.f ? v : v * 0.2f; }

// grid (ceil(W / 64), ceil(H / 16), bs).  VEC: W % 4 == 0, x and out 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void v2v_image_head_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ wgt,
                                                             const float* __restrict__ bias, int C, int H, int W) {
    __shared__ __attribute__((aligned(16))) float tile[HEAD_CH * HEAD_LH * HEAD_LW];
    __shared__ __attribute__((aligned(16))) float wl[HEAD_CH * HEAD_WROW];
    const int tid = threadIdx.x;
    const int lx = tid & 15, ly = tid >> 4;
    const int tx0 = blockIdx.x * HEAD_TW, ty0 = blockIdx.y * HEAD_TH;
    const int64_t b = blockIdx.z;
    const int64_t hw = (int64_t)H * W;
    const float* xb = x + b * C * hw;

    float acc[3][4];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[o][j] = bias[o];

    for (int c0 = 0; c0 < C; c0 += HEAD_CH) {
        const int nc = min(HEAD_CH, C - c0);                                    // the last chunk may be short: its missing channels are neither staged nor read
        __syncthreads();                                                        // the previous chunk has been read (first pass: nothing yet)
        if (tid < HEAD_CH * HEAD_WROW) {
            const int ci = tid / HEAD_WROW, r = tid - ci * HEAD_WROW;
            const int tap = r / 3, o = r - tap * 3;
            wl[tid] = (ci < nc && r < 27) ? wgt[((int64_t)o * C + c0 + ci) * 9 + tap] : 0.f;
        }
        if constexpr (VEC) {
            for (int i = tid; i < nc * HEAD_LH * (HEAD_TW / 4); i += 256) {
                const int rr = i / (HEAD_TW / 4), q = i - rr * (HEAD_TW / 4);   // rr = c * LH + r
                const int c = rr / HEAD_LH, r = rr - c * HEAD_LH;
                const int gy = ty0 - 1 + r, gx = tx0 + 4 * q;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gy >= 0 && gy < H && gx < W) {
                    v = *reinterpret_cast<const float4*>(xb + (c0 + c) * hw + (int64_t)gy * W + gx);
                    v = make_float4(v2v_leaky02(v.x), v2v_leaky02(v.y), v2v_leaky02(v.z), v2v_leaky02(v.w));
                }
                *reinterpret_cast<float4*>(tile + rr * HEAD_LW + 4 + 4 * q) = v;
            }
            for (int i = tid; i < nc * HEAD_LH * 2; i += 256) {
                const int rr = i >> 1, side = i & 1;
                const int c = rr / HEAD_LH, r = rr - c * HEAD_LH;
                const int gy = ty0 - 1 + r, gx = side ? tx0 + HEAD_TW : tx0 - 1;
                float v = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = v2v_leaky02(xb[(c0 + c) * hw + (int64_t)gy * W + gx]);
                tile[rr * HEAD_LW + (side ? 4 + HEAD_TW : 3)] = v;
            }
        } else {
            for (int i = tid; i < nc * HEAD_LH * (HEAD_TW + 2); i += 256) {
                const int rr = i / (HEAD_TW + 2), cx = i - rr * (HEAD_TW + 2);
                const int c = rr / HEAD_LH, r = rr - c * HEAD_LH;
                const int gy = ty0 - 1 + r, gx = tx0 - 1 + cx;
                float v = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = v2v_leaky02(xb[(c0 + c) * hw + (int64_t)gy * W + gx]);
                tile[rr * HEAD_LW + 3 + cx] = v;
            }
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            float wv[HEAD_WROW];
            const float4* wp = reinterpret_cast<const float4*>(wl + c * HEAD_WROW);             // the same address in every lane
#pragma unroll
            for (int k = 0; k < HEAD_WROW / 4; ++k) {
                const float4 q = wp[k];
                wv[4 * k] = q.x; wv[4 * k + 1] = q.y; wv[4 * k + 2] = q.z; wv[4 * k + 3] = q.w;
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float* rp = tile + (c * HEAD_LH + ly + ky) * HEAD_LW + 4 * lx + 3;
                const float4 mid = *reinterpret_cast<const float4*>(rp + 1);
                const float v[6] = {rp[0], mid.x, mid.y, mid.z, mid.w, rp[5]};
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int o = 0; o < 3; ++o)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[o][j] = fmaf(wv[(ky * 3 + kx) * 3 + o], v[j + kx], acc[o][j]);
            }
        }
    }

    const int y = ty0 + ly, x0 = tx0 + 4 * lx;
    if (y >= H || x0 >= W) return;
    const int64_t pix = (int64_t)y * W + x0;
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[o][j] = 1.0f / (1.0f + expf(-acc[o][j]));
    if constexpr (VEC) {
#pragma unroll
        for (int o = 0; o < 3; ++o) *reinterpret_cast<float4*>(out + (b * 3 + o) * hw + pix) = make_float4(acc[o][0], acc[o][1], acc[o][2], acc[o][3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j >= W) break;
#pragma unroll
            for (int o = 0; o < 3; ++o) out[(b * 3 + o) * hw + pix + j] = acc[o][j];
        }
    }
}

extern "C" int e4s_v2v_image_head(float* out, const float* x, const float* weight, const float* bias, int bs, int cin, int H, int W, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && cin >= 1 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "v2v_image_head: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && x && weight && bias, "v2v_image_head: null tensor");
    const dim3 grid(cdiv(W, HEAD_TW), cdiv(H, HEAD_TH), bs);
    if (W % 4 == 0 && v2v_aligned16(x) && v2v_aligned16(out))
        hipLaunchKernelGGL(v2v_image_head_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, out, x, weight, bias, cin, H, W);
    else
        hipLaunchKernelGGL(v2v_image_head_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, out, x, weight, bias, cin, H, W);
    return check_launch("v2v_image_head");
}
