// Row f19: the two forms of the feature gather (e4s_v2v_deform) that were weighed against each other, and the channels per workgroup row, at the upstream shape
// [32][16][64][64] with one feature shared by bs deformations.  V = 1: one position per lane (the form csrc/vid2vid.hip keeps).  V = 4: four neighbouring
// positions per lane, 16-byte loads of the deformation and one 16-byte store per channel (the form that was taken out).  Both call v2v_trilinear_taps and join
// the taps in the same order; the program checks that they give the same bits and prints the median device time of five rounds of 20 launches for cg = 1 .. 32
// channels per row, on a smooth deformation (the identity grid plus a slow sine: what a dense-motion network returns) and on a uniformly random one.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/probes/deform_forms_probe.hip -o tools/probes/deform_forms_probe && tools/probes/deform_forms_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../e4s2024_amd/csrc/v2v_sample.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int V>
__global__ __launch_bounds__(256) void deform_form(float* __restrict__ out, const float* __restrict__ feature, const float* __restrict__ deformation, int C, int D,
                                                   int H, int W, size_t feat_bs, size_t out_bs, int cg) {
#pragma clang fp contract(off)
    const int b = blockIdx.z;
    const int n = D * H * W;
    const int pos = (blockIdx.x * 256 + threadIdx.x) * V;
    if (pos >= n) return;                              // V = 4 only with n % 4 == 0
    const int c0 = blockIdx.y * cg;
    const int c1 = min(c0 + cg, C);
    float wgt[V][8];
    int off[V][8];
    unsigned okm[V];
    const float* dp = deformation + ((size_t)b * n + pos) * 3;
    if constexpr (V == 4) {
        const float4 q0 = reinterpret_cast<const float4*>(dp)[0], q1 = reinterpret_cast<const float4*>(dp)[1], q2 = reinterpret_cast<const float4*>(dp)[2];
        okm[0] = v2v_trilinear_taps(wgt[0], off[0], q0.x, q0.y, q0.z, D, H, W);
        okm[1] = v2v_trilinear_taps(wgt[1], off[1], q0.w, q1.x, q1.y, D, H, W);
        okm[2] = v2v_trilinear_taps(wgt[2], off[2], q1.z, q1.w, q2.x, D, H, W);
        okm[3] = v2v_trilinear_taps(wgt[3], off[3], q2.y, q2.z, q2.w, D, H, W);
    } else {
        okm[0] = v2v_trilinear_taps(wgt[0], off[0], dp[0], dp[1], dp[2], D, H, W);
    }
    const float* fb = feature + (size_t)b * feat_bs;
    float* ob = out + (size_t)b * out_bs + pos;
    for (int j = c0; j < c1; ++j) {
        const float* fp = fb + (size_t)j * n;
        float acc[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            acc[i] = 0.f;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float v = fp[off[i][t]];
                if ((okm[i] >> t) & 1u) acc[i] = acc[i] + v * wgt[i][t];
            }
        }
        if constexpr (V == 4)
            *reinterpret_cast<float4*>(ob + (size_t)j * n) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else
            ob[(size_t)j * n] = acc[0];
    }
}

template <int V>
static void launch(float* out, const float* f, const float* g, int bs, int C, int D, int H, int W, int cg) {
    const int n = D * H * W;
    hipLaunchKernelGGL(deform_form<V>, dim3((n / V + 255) / 256, (C + cg - 1) / cg, bs), dim3(256), 0, 0, out, f, g, C, D, H, W, (size_t)0, (size_t)C * n, cg);
}

template <int V>
static float median_us(float* out, const float* f, const float* g, int bs, int C, int D, int H, int W, int cg) {
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    for (int i = 0; i < 5; ++i) launch<V>(out, f, g, bs, C, D, H, W, cg);
    std::vector<float> rounds;
    for (int r = 0; r < 5; ++r) {
        hipEventRecord(a, 0);
        for (int i = 0; i < 20; ++i) launch<V>(out, f, g, bs, C, D, H, W, cg);
        hipEventRecord(b, 0);
        hipEventSynchronize(b);
        float ms = 0.f;
        hipEventElapsedTime(&ms, a, b);
        rounds.push_back(ms * 1000.f / 20.f);
    }
    hipEventDestroy(a);
    hipEventDestroy(b);
    std::sort(rounds.begin(), rounds.end());
    return rounds[2];
}

int main() {
    const int C = 32, D = 16, H = 64, W = 64, n = D * H * W, maxbs = 4;
    std::vector<float> hf((size_t)C * n), hg[2];
    srand(19);
    for (auto& v : hf) v = (float)rand() / RAND_MAX * 2.f - 1.f;
    for (int kind = 0; kind < 2; ++kind) {
        hg[kind].resize((size_t)maxbs * n * 3);
        for (int b = 0; b < maxbs; ++b)
            for (int z = 0; z < D; ++z)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        float* p = &hg[kind][(((size_t)b * D + z) * H * W + (size_t)y * W + x) * 3];
                        const float gx = 2.f * x / (W - 1) - 1.f, gy = 2.f * y / (H - 1) - 1.f, gz = 2.f * z / (D - 1) - 1.f;
                        if (kind == 0) {
                            p[0] = gx + 0.1f * sinf(3.f * gz + b), p[1] = gy + 0.1f * sinf(3.f * gy), p[2] = gz + 0.1f * sinf(3.f * gx);
                        } else {
                            for (int k = 0; k < 3; ++k) p[k] = ((float)rand() / RAND_MAX * 2.f - 1.f) * 1.15f;
                        }
                    }
    }
    float *f, *g, *o1, *o4;
    CHECK(hipMalloc(&f, hf.size() * 4));
    CHECK(hipMalloc(&g, hg[0].size() * 4));
    CHECK(hipMalloc(&o1, (size_t)maxbs * C * n * 4));
    CHECK(hipMalloc(&o4, (size_t)maxbs * C * n * 4));
    CHECK(hipMemcpy(f, hf.data(), hf.size() * 4, hipMemcpyHostToDevice));
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    printf("e4s_v2v_deform forms on %s: feature [32][16][64][64] shared by bs deformations, median of 5 rounds x 20 launches, microseconds\n", prop.gcnArchName);
    std::vector<float> h1((size_t)maxbs * C * n), h4(h1.size());
    for (int kind = 0; kind < 2; ++kind) {
        CHECK(hipMemcpy(g, hg[kind].data(), hg[kind].size() * 4, hipMemcpyHostToDevice));
        launch<1>(o1, f, g, maxbs, C, D, H, W, 4);
        launch<4>(o4, f, g, maxbs, C, D, H, W, 8);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(h1.data(), o1, h1.size() * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(h4.data(), o4, h4.size() * 4, hipMemcpyDeviceToHost));
        const bool same = memcmp(h1.data(), h4.data(), h1.size() * 4) == 0;
        printf("%s deformation: the two forms give the same bits: %s\n", kind == 0 ? "smooth" : "random", same ? "yes" : "NO");
        if (!same) return 1;
        for (int bs : {1, 4})
            for (int cg : {1, 2, 4, 8, 16, 32})
                printf("  %s bs %d cg %2d: one position per lane %7.1f   four positions per lane, 16-byte stores %7.1f\n", kind == 0 ? "smooth" : "random", bs, cg,
                       median_us<1>(o1, f, g, bs, C, D, H, W, cg), median_us<4>(o4, f, g, bs, C, D, H, W, cg));
    }
    CHECK(hipDeviceSynchronize());
    printf("ok\n");
    return 0;
}
