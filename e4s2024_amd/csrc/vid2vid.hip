// f17: face-vid2vid reenactment, stage 1 — the glue of KPDetector and of keypoint_transformation (swap_face_fine/face_vid2vid/modules/keypoint_detector.py:44-82,
// modules/util.py:55-71, 196-213, 372-418, drive_demo.py:67-180).  Everything here is small against the convolutions: one lane per output, or one workgroup per
// (sample, keypoint); float32 with every sum in a fixed order.
#include "common.h"

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
