// Row f21: CodeFormer face restoration, stage 1 (e4s2024_amd/ops_codeformer.py) — the arithmetic the VQGAN encoder, the code transformer and the code head need
// between their convolutions, which run on conv.hip (e4s_conv2d_sb3; conv_in and the logits head on the exact e4s_conv2d): GroupNorm (its statistics and) + swish, softmax attention
// and LayerNorm on channel-major operands, GELU, the right / bottom pad of Downsample, the top-1 code per token, the codebook gather with its AdaIN.
// fp32, no atomics, no host synchronisation, no scratch memory, grids from shapes alone; every reduction adds in a fixed order: the same inputs give the same
// bits, and a sample of a batch gets the bits it gets alone.
#include <math.h>

#include "common.h"

using namespace e4s;

// ------------------------------------------------------------------------------------ GroupNorm (+ swish)
// In NCHW a group of one sample is one contiguous run of C / groups * hw floats.  Statistics: the run is cut into `chunks` pieces of equal length, one block
// each (a run of 2 * 512 * 512 floats on one block per group left 224 of 256 CUs idle at batch 1); a block writes its piece's mean and its sum of squares
// about THAT mean (two passes; the second comes from the cache), so a run whose mean is a hundred times its deviation loses nothing.  A second small kernel
// merges the pieces of a run in piece order in float64 (done inside every block of the consumer instead, the merge's 64 float64 divisions per thread made the
// normalisation 2.6 times slower at batch 8).
__device__ __forceinline__ float cf_block_sum(float v, float* sh) {       // 256 threads; the result is valid in every thread
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void cf_group_stats_kernel(float* __restrict__ part, const float* __restrict__ x, int run, int len) {
    __shared__ float sh[4];
    const int lo = blockIdx.x * len, n = (run - lo < len ? run - lo : len);
    const float* xp = x + (size_t)blockIdx.y * run + lo;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += xp[i];
    const float m = cf_block_sum(s, sh) / (float)n;
    float q = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float a = xp[i] - m;
        q = fmaf(a, a, q);
    }
    q = cf_block_sum(q, sh);
    if (threadIdx.x == 0) {
        float* o = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        o[0] = m;
        o[1] = q;
    }
}

// stats[g] = (mean_g, corr_g, rstd_g): the pieces of run g merged in piece order in float64 (Chan's update), mean_g the float32 rounding of the merged mean,
// corr_g what that rounding left, rstd_g = 1 / sqrt(var + eps) with the biased variance.  One thread per run.
__global__ __launch_bounds__(256) void cf_group_merge_kernel(float* __restrict__ stats, const float* __restrict__ part, int runs, int run, int chunks, float eps) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= runs) return;
    const int len = (run + chunks - 1) / chunks;
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    for (int k = 0; k < chunks; ++k) {
        const int lo = k * len;
        const double nk = (double)(run - lo < len ? run - lo : len);
        const double mk = (double)part[((size_t)g * chunks + k) * 2], qk = (double)part[((size_t)g * chunks + k) * 2 + 1];
        const double delta = mk - mean, tot = cnt + nk;
        mean += delta * nk / tot;
        m2 += qk + delta * delta * cnt * nk / tot;
        cnt = tot;
    }
    const float m = (float)mean;
    stats[(size_t)g * 3] = m;
    stats[(size_t)g * 3 + 1] = (float)(mean - (double)m);
    stats[(size_t)g * 3 + 2] = (float)(1.0 / sqrt(m2 / cnt + (double)eps));
}

extern "C" int e4s_cf_group_stats(float* stats, float* part, const float* x, int runs, int run, int chunks, float eps, void* stream) {
    E4S_REQUIRE(runs >= 0 && runs <= 65535 && run >= 1 && chunks >= 1 && chunks <= 64 && chunks <= run, "cf_group_stats: bad size (1 .. 64 chunks)");
    E4S_REQUIRE((int64_t)(chunks - 1) * cdiv(run, chunks) < run, "cf_group_stats: %d chunks leave the last piece of a run of %d empty", chunks, run);
    E4S_REQUIRE(runs == 0 || (stats && part && x), "cf_group_stats: null tensor");
    if (runs == 0) return 0;
    hipLaunchKernelGGL(cf_group_stats_kernel, dim3(chunks, runs), dim3(256), 0, (hipStream_t)stream, part, x, run, cdiv(run, chunks));
    hipLaunchKernelGGL(cf_group_merge_kernel, dim3(cdiv(runs, 256)), dim3(256), 0, (hipStream_t)stream, stats, part, runs, run, chunks, eps);
    return check_launch("cf_group_stats");
}

// y = s * sigmoid(s) (swish) or s, s = ((x - mean_g) - corr_g) * rstd_g * gamma_c + beta_c with stats [bs groups][3] = (mean, corr, rstd) of e4s_cf_group_stats.
// One (b, c) plane per blockIdx.y.
__global__ __launch_bounds__(256) void cf_group_norm_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ stats,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, int C, int cpg, int hw, int swish, int vec) {
#pragma clang fp contract(off)
    const int plane = blockIdx.y, c = plane % C, g = (plane / C) * (C / cpg) + c / cpg;
    const float m = stats[(size_t)g * 3], corr = stats[(size_t)g * 3 + 1], r = stats[(size_t)g * 3 + 2];
    const float ga = gamma[c], be = beta[c];
    const float* xp = x + (size_t)plane * hw;
    float* op = out + (size_t)plane * hw;
    auto f = [&](float v) {
        const float s = ((v - m) - corr) * r * ga + be;
        return swish ? s * (1.0f / (1.0f + expf(-s))) : s;
    };
    if (vec) {
        for (int i = (blockIdx.x * 256 + threadIdx.x) * 4; i < hw; i += gridDim.x * 1024) {
            const float4 t = *reinterpret_cast<const float4*>(xp + i);
            *reinterpret_cast<float4*>(op + i) = make_float4(f(t.x), f(t.y), f(t.z), f(t.w));
        }
    } else {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) op[i] = f(xp[i]);
    }
}

extern "C" int e4s_cf_group_norm(float* out, const float* x, const float* stats, const float* gamma, const float* beta, int bs, int C, int groups, int hw,
                                 int swish, void* stream) {
    E4S_REQUIRE(out && x && stats && gamma && beta, "cf_group_norm: null tensor");
    E4S_REQUIRE(bs >= 0 && C >= 1 && groups >= 1 && C % groups == 0 && hw >= 1 && (int64_t)bs * C <= 65535, "cf_group_norm: bad size (C a multiple of groups, bs C <= 65535)");
    if (bs == 0) return 0;
    const int vec = (hw & 3) == 0 && (((uintptr_t)out | (uintptr_t)x) & 15) == 0;
    const int per = vec ? 1024 : 256;
    const int gx = cdiv(hw, per) < 64 ? cdiv(hw, per) : 64;
    hipLaunchKernelGGL(cf_group_norm_kernel, dim3(gx, bs * C), dim3(256), 0, (hipStream_t)stream, out, x, stats, gamma, beta, C, C / groups, hw, swish ? 1 : 0, vec);
    return check_launch("cf_group_norm");
}

// ------------------------------------------------------------------------------------ softmax attention, channel-major
// out[b][h d + c][i] = sum_j softmax_j(scale q_i . k_j) v[c][j] for q, k, v, out [.][heads d][T] (sample b of q at q + b q_bstride, ...).  One wave per QW
// queries: the scores of a query are NJ = ceil(T / 64) registers per lane (key j = 64 jj + lane), every product an fmaf over the d channels in channel order;
// the maximum and the sum are wave butterflies (a fixed order), p = expf(s - max); the output sums p_j v[c][j] per lane in jj order and then over the lanes
// with wave_sum_x32, 32 channels at a time.  Exact float32 products throughout.
template <int NJ, int QW>
__global__ __launch_bounds__(256) void cf_attention_kernel(float* __restrict__ out, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                           int64_t qb, int64_t kb, int64_t vb, int64_t ob, int d, int T, float scale) {
    extern __shared__ float qs[];                     // [4 waves][QW][d]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.y, b = blockIdx.z;
    const int i0 = (blockIdx.x * 4 + wave) * QW;
    const float* qp = q + (size_t)b * qb + (size_t)h * d * T;
    const float* kp = k + (size_t)b * kb + (size_t)h * d * T;
    const float* vp = v + (size_t)b * vb + (size_t)h * d * T;
    float* op = out + (size_t)b * ob + (size_t)h * d * T;
    float* myq = qs + (size_t)wave * QW * d;
    for (int e = lane; e < QW * d; e += 64) {
        const int qi = e / d, c = e - qi * d;
        const int i = i0 + qi < T ? i0 + qi : T - 1;
        myq[e] = qp[(size_t)c * T + i];
    }
    __syncthreads();
    if (i0 >= T) return;                              // (wave-uniform; no barrier below)
    int jc[NJ];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) jc[jj] = jj * 64 + lane < T ? jj * 64 + lane : T - 1;
    float s[QW][NJ];
#pragma unroll
    for (int qi = 0; qi < QW; ++qi)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) s[qi][jj] = 0.f;
    for (int c = 0; c < d; ++c) {
        float kv[NJ];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) kv[jj] = kp[(size_t)c * T + jc[jj]];
#pragma unroll
        for (int qi = 0; qi < QW; ++qi) {
            const float qv = myq[qi * d + c];
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) s[qi][jj] = fmaf(qv, kv[jj], s[qi][jj]);
        }
    }
    float inv[QW];
#pragma unroll
    for (int qi = 0; qi < QW; ++qi) {
        float mx = -INFINITY;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            s[qi][jj] = jj * 64 + lane < T ? s[qi][jj] * scale : -INFINITY;
            mx = fmaxf(mx, s[qi][jj]);
        }
        mx = wave_max(mx);
        float l = 0.f;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            s[qi][jj] = expf(s[qi][jj] - mx);          // exp(-inf) = 0 for the keys past T
            l += s[qi][jj];
        }
        inv[qi] = 1.0f / wave_sum(l);
    }
    const int myc = wave_sum_x32_index(lane);
    for (int c0 = 0; c0 < d; c0 += 32) {
        float acc[QW][32];
#pragma unroll
        for (int cc = 0; cc < 32; ++cc) {
            const int c = c0 + cc < d ? c0 + cc : d - 1;
            float vv[NJ];
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) vv[jj] = vp[(size_t)c * T + jc[jj]];
#pragma unroll
            for (int qi = 0; qi < QW; ++qi) {
                float a = 0.f;
#pragma unroll
                for (int jj = 0; jj < NJ; ++jj) a = fmaf(s[qi][jj], vv[jj], a);
                acc[qi][cc] = a;
            }
        }
#pragma unroll
        for (int qi = 0; qi < QW; ++qi) {
            const float r = wave_sum_x32(acc[qi]) * inv[qi];
            if ((lane & 1) == 0 && c0 + myc < d && i0 + qi < T) op[(size_t)(c0 + myc) * T + i0 + qi] = r;
        }
    }
}

template <int NJ, int QW>
static int launch_attention(float* out, const float* q, const float* k, const float* v, int64_t qb, int64_t kb, int64_t vb, int64_t ob, int bs, int heads, int d,
                            int T, float scale, hipStream_t st) {
    hipLaunchKernelGGL((cf_attention_kernel<NJ, QW>), dim3(cdiv(T, 4 * QW), heads, bs), dim3(256), (size_t)4 * QW * d * sizeof(float), st, out, q, k, v, qb, kb, vb,
                       ob, d, T, scale);
    return check_launch("cf_attention");
}

extern "C" int e4s_cf_attention(float* out, const float* q, const float* k, const float* v, int64_t q_bstride, int64_t k_bstride, int64_t v_bstride,
                                int64_t out_bstride, int bs, int heads, int d, int T, float scale, void* stream) {
    E4S_REQUIRE(out && q && k && v, "cf_attention: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && heads >= 1 && heads <= 65535, "cf_attention: bad size");
    E4S_REQUIRE(d >= 16 && d <= 512 && d % 16 == 0, "cf_attention: head width %d (a multiple of 16 up to 512)", d);
    E4S_REQUIRE(T >= 1 && T <= 1024, "cf_attention: %d tokens (1 .. 1024)", T);
    const int64_t need = (int64_t)heads * d * T;
    E4S_REQUIRE(q_bstride >= need && k_bstride >= need && v_bstride >= need && out_bstride >= need, "cf_attention: a batch stride below heads d T");
    if (bs == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (T <= 64) return launch_attention<1, 4>(out, q, k, v, q_bstride, k_bstride, v_bstride, out_bstride, bs, heads, d, T, scale, st);
    if (T <= 128) return launch_attention<2, 4>(out, q, k, v, q_bstride, k_bstride, v_bstride, out_bstride, bs, heads, d, T, scale, st);
    if (T <= 256) return launch_attention<4, 2>(out, q, k, v, q_bstride, k_bstride, v_bstride, out_bstride, bs, heads, d, T, scale, st);
    if (T <= 512) return launch_attention<8, 1>(out, q, k, v, q_bstride, k_bstride, v_bstride, out_bstride, bs, heads, d, T, scale, st);
    return launch_attention<16, 1>(out, q, k, v, q_bstride, k_bstride, v_bstride, out_bstride, bs, heads, d, T, scale, st);
}

// ------------------------------------------------------------------------------------ LayerNorm over channels, channel-major
// y[b][c][t] = (x[b][c][t] - mean_t) * rstd_t * gamma[c] + beta[c] over the C channels of token t (biased variance, two passes on registers), and, with pos,
// y_pos = y + pos[c][t] as a second output.  16 tokens x 16 channel groups per block: thread (g, tl) holds channels g, g + 16, ... of token t0 + tl; the 16
// partial sums of a token meet in LDS and are added in group order.
__global__ __launch_bounds__(256) void cf_layer_norm_kernel(float* __restrict__ y, float* __restrict__ ypos, const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ pos, int C, int T, float eps) {
#pragma clang fp contract(off)
    __shared__ float sh[16][17];
    const int tl = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int t = blockIdx.x * 16 + tl, b = blockIdx.y;
    const bool ok = t < T;
    const float* xp = x + (size_t)b * C * T + (ok ? t : T - 1);
    float v[32];
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const int c = g + 16 * e;
        v[e] = c < C ? xp[(size_t)c * T] : 0.f;
        s += v[e];
    }
    sh[g][tl] = s;
    __syncthreads();
    float m = 0.f;
#pragma unroll
    for (int gg = 0; gg < 16; ++gg) m += sh[gg][tl];
    m /= (float)C;
    float qq = 0.f;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const float a = g + 16 * e < C ? v[e] - m : 0.f;
        qq += a * a;
    }
    __syncthreads();
    sh[g][tl] = qq;
    __syncthreads();
    float var = 0.f;
#pragma unroll
    for (int gg = 0; gg < 16; ++gg) var += sh[gg][tl];
    const float r = 1.0f / sqrtf(var / (float)C + eps);
    if (!ok) return;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const int c = g + 16 * e;
        if (c < C) {
            const float o = (v[e] - m) * r * gamma[c] + beta[c];
            const size_t at = ((size_t)b * C + c) * T + t;
            y[at] = o;
            if (ypos) ypos[at] = o + pos[(size_t)c * T + t];
        }
    }
}

extern "C" int e4s_cf_layer_norm(float* y, float* y_pos, const float* x, const float* gamma, const float* beta, const float* pos, int bs, int C, int T, float eps,
                                 void* stream) {
    E4S_REQUIRE(y && x && gamma && beta, "cf_layer_norm: null tensor");
    E4S_REQUIRE((y_pos == nullptr) == (pos == nullptr), "cf_layer_norm: y_pos and pos go together");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && C >= 1 && C <= 512 && T >= 1, "cf_layer_norm: bad size (1 .. 512 channels)");
    if (bs == 0) return 0;
    hipLaunchKernelGGL(cf_layer_norm_kernel, dim3(cdiv(T, 16), bs), dim3(256), 0, (hipStream_t)stream, y, y_pos, x, gamma, beta, pos, C, T, eps);
    return check_launch("cf_layer_norm");
}

// ------------------------------------------------------------------------------------ GELU (exact erf form), in place or not
__global__ __launch_bounds__(256) void cf_gelu_kernel(float* out, const float* x, int64_t n) {     // (out may be x)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = x[i];
        out[i] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    }
}

extern "C" int e4s_cf_gelu(float* out, const float* x, int64_t n, void* stream) {
    E4S_REQUIRE(n >= 0 && (n == 0 || (out && x)), "cf_gelu: null tensor");
    if (n == 0) return 0;
    hipLaunchKernelGGL(cf_gelu_kernel, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, out, x, n);
    return check_launch("cf_gelu");
}

// ------------------------------------------------------------------------------------ Downsample's pad (0, 1, 0, 1)
// out [planes][h + 1][w + 1] = x [planes][h][w] with a zero column on the right and a zero row at the bottom.
__global__ __launch_bounds__(256) void cf_pad_rb_kernel(float* __restrict__ out, const float* __restrict__ x, int h, int w) {
    const int wp = w + 1, n = (h + 1) * wp;
    const float* xp = x + (size_t)blockIdx.y * h * w;
    float* op = out + (size_t)blockIdx.y * n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int yy = i / wp, xx = i - yy * wp;
        op[i] = (yy < h && xx < w) ? xp[(size_t)yy * w + xx] : 0.f;
    }
}

extern "C" int e4s_cf_pad_rb(float* out, const float* x, int planes, int h, int w, void* stream) {
    E4S_REQUIRE(planes >= 0 && planes <= 65535 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "cf_pad_rb: bad size");
    E4S_REQUIRE(planes == 0 || (out && x), "cf_pad_rb: null tensor");
    if (planes == 0) return 0;
    const int n = (h + 1) * (w + 1);
    hipLaunchKernelGGL(cf_pad_rb_kernel, dim3(cdiv(n, 256) < 256 ? cdiv(n, 256) : 256, planes), dim3(256), 0, (hipStream_t)stream, out, x, h, w);
    return check_launch("cf_pad_rb");
}

// ------------------------------------------------------------------------------------ top-1 code per token
// idx[b][t] = the smallest n with logits[b][t][n] = max_n (the element at b sb + t st + n sn): one thread per token walks the codebook upwards and moves on
// a strictly larger value only.
__global__ __launch_bounds__(256) void cf_argmax_kernel(int64_t* __restrict__ idx, const float* __restrict__ logits, int T, int K, int64_t sb, int64_t st_, int64_t sn) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (t >= T) return;
    const float* p = logits + (size_t)b * sb + (size_t)t * st_;
    float best = p[0];
    int at = 0;
    for (int n = 1; n < K; ++n) {
        const float v = p[(size_t)n * sn];
        if (v > best) { best = v; at = n; }
    }
    idx[(size_t)b * T + t] = at;
}

extern "C" int e4s_cf_argmax(int64_t* idx, const float* logits, int bs, int T, int K, int64_t b_stride, int64_t t_stride, int64_t n_stride, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && T >= 1 && K >= 1 && b_stride >= 0 && t_stride >= 0 && n_stride >= 0, "cf_argmax: bad size");
    E4S_REQUIRE(bs == 0 || (idx && logits), "cf_argmax: null tensor");
    if (bs == 0) return 0;
    hipLaunchKernelGGL(cf_argmax_kernel, dim3(cdiv(T, 256), bs), dim3(256), 0, (hipStream_t)stream, idx, logits, T, K, b_stride, t_stride, n_stride);
    return check_launch("cf_argmax");
}

// ------------------------------------------------------------------------------------ codebook gather (+ AdaIN)
// quant[b][c][t] = emb[idx[b][t]][c]; with adain, out = (quant - mean_q) / sqrt(var_q + eps) * sqrt(var_s + eps) + mean_s per (b, c) plane, var the UNBIASED
// variance over the T tokens and (mean_s, var_s) those of style[b][c][:]: adaptive_instance_normalization's expression, operation by operation.  One wave per
// plane, T <= 1024: 16 values per lane, two passes on registers.  An index outside the codebook is clamped (never read past it).
__global__ __launch_bounds__(256) void cf_quant_kernel(float* __restrict__ out, const int64_t* __restrict__ idx, const float* __restrict__ emb, const float* __restrict__ style,
                                                       int planes, int C, int T, int K, int adain, float eps) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, plane = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const int b = plane / C, c = plane - b * C;
    float qv[16], sv[16];
    float sq = 0.f, ss = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int t = e * 64 + lane;
        qv[e] = sv[e] = 0.f;
        if (t < T) {
            int64_t n = idx[(size_t)b * T + t];
            n = n < 0 ? 0 : (n < K ? n : K - 1);
            qv[e] = emb[(size_t)n * C + c];
            if (adain) sv[e] = style[(size_t)plane * T + t];
            sq += qv[e];
            ss += sv[e];
        }
    }
    float mq = 0.f, ms = 0.f, dq = 1.f, ds = 1.f;
    if (adain) {
        mq = wave_sum(sq) / (float)T;
        ms = wave_sum(ss) / (float)T;
        float vq = 0.f, vs = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            if (e * 64 + lane < T) {
                const float a = qv[e] - mq, s2 = sv[e] - ms;
                vq += a * a;
                vs += s2 * s2;
            }
        }
        dq = sqrtf(wave_sum(vq) / (float)(T - 1) + eps);
        ds = sqrtf(wave_sum(vs) / (float)(T - 1) + eps);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int t = e * 64 + lane;
        if (t < T) out[(size_t)plane * T + t] = adain ? (qv[e] - mq) / dq * ds + ms : qv[e];
    }
}

extern "C" int e4s_cf_quant(float* out, const void* idx, const float* emb, const float* style, int bs, int C, int T, int K, int adain, float eps, void* stream) {
    E4S_REQUIRE(bs >= 0 && C >= 1 && K >= 1 && (int64_t)bs * C <= 0x7fffffff, "cf_quant: bad size");
    E4S_REQUIRE(T >= (adain ? 2 : 1) && T <= 1024, "cf_quant: %d tokens (1 .. 1024; at least 2 with the AdaIN, whose variance is unbiased)", T);
    E4S_REQUIRE(bs == 0 || (out && idx && emb && (!adain || style)), "cf_quant: null tensor");
    if (bs == 0) return 0;
    hipLaunchKernelGGL(cf_quant_kernel, dim3(cdiv(bs * C, 4)), dim3(256), 0, (hipStream_t)stream, out, static_cast<const int64_t*>(idx), emb, style, bs * C, C, T, K, adain ? 1 : 0, eps);
    return check_launch("cf_quant");
}
