// gsr_ssim.h -- the 11x11 Gaussian window of SSIM (utils/loss_utils.py:23-58) as the LDS-tiled
// separable passes share it: loss.hip (the loss) and eval.hip (the evaluation metrics).  A 64x16
// output tile per 256-thread workgroup; the horizontal pass writes the five windowed moments of a
// staged halo, the vertical pass finishes them for four rows per thread.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

#include "gsr_device.h"

namespace gsr {
namespace {

constexpr int kR = 5;  // window radius: 11 taps
constexpr int kTW = 64;
constexpr int kTH = 16;
constexpr int kLossThreads = 256;
constexpr float kC1 = 0.01f * 0.01f;  // utils/loss_utils.py:54-55 (C1 = 0.01^2, C2 = 0.03^2)
constexpr float kC2 = 0.03f * 0.03f;

struct Window {
    float w[2 * kR + 1];
};

// utils/loss_utils.py:24-26: exp(-(x - 5)^2 / (2 sigma^2)) as fp32, normalised by its fp32 sum.
[[maybe_unused]] Window ssim_window() {
    Window win;
    float sum = 0.f;
    for (int i = 0; i < 2 * kR + 1; i++) {
        win.w[i] = (float)std::exp(-(double)((i - kR) * (i - kR)) / (2.0 * 1.5 * 1.5));
        sum += win.w[i];
    }
    for (int i = 0; i < 2 * kR + 1; i++) win.w[i] /= sum;
    return win;
}

struct Moments {
    float m1, m2, a11, a22, a12;
};

// Numerator and denominator of the SSIM map value at one pixel from its windowed moments
// (utils/loss_utils.py:44-58 op order).
__device__ __forceinline__ void ssim_terms(const Moments &s, float &num, float &den) {
    const float mu1_sq = s.m1 * s.m1, mu2_sq = s.m2 * s.m2, mu12 = s.m1 * s.m2;
    const float s1 = s.a11 - mu1_sq, s2 = s.a22 - mu2_sq, s12 = s.a12 - mu12;
    num = (2.f * mu12 + kC1) * (2.f * s12 + kC2);
    den = (mu1_sq + mu2_sq + kC1) * (s1 + s2 + kC2);
}

// SSIM map value at one pixel from its windowed moments.
__device__ __forceinline__ float ssim_value(const Moments &s) {
    float num, den;
    ssim_terms(s, num, den);
    return num / den;
}

// LDS layout: every staged map is row-major with an odd row pitch (an odd number of floats), so
// the passes below, whose 32-lane halves walk down consecutive rows of a map, touch 32
// different banks.
constexpr int odd_pitch(int cols) { return cols | 1; }

// Horizontal pass of the five moments: out[q][r][c] = sum_j w_j f_q(in[r][c + j]).  A task is a
// kS-column segment of one row: kS + 10 inputs are loaded once into registers, so LDS reads drop
// from 22 per output to (2 kS + 20) / kS.  Consecutive tasks (lanes) take consecutive rows.
template <int kS>
__device__ __forceinline__ void hpass5(const float *sx, const float *sy, int rows, int in_cols, int in_pitch,
                                       int out_cols, int out_pitch, int plane, const Window &win, float *hs) {
    const int segs = (out_cols + kS - 1) / kS;
    for (int task = threadIdx.x; task < rows * segs; task += kLossThreads) {
        const int s = task / rows, r = task - s * rows, c0 = s * kS;
        const float *px = sx + r * in_pitch + c0, *py = sy + r * in_pitch + c0;
        float u[kS + 2 * kR], v[kS + 2 * kR];
#pragma unroll
        for (int k = 0; k < kS + 2 * kR; k++) {
            const bool ok = c0 + k < in_cols;
            u[k] = ok ? px[k] : 0.f;
            v[k] = ok ? py[k] : 0.f;
        }
#pragma unroll
        for (int o = 0; o < kS; o++) {
            float m1 = 0.f, m2 = 0.f, a11 = 0.f, a22 = 0.f, a12 = 0.f;
#pragma unroll
            for (int j = 0; j < 2 * kR + 1; j++) {
                const float w = win.w[j];
                m1 = fmaf(w, u[o + j], m1);
                m2 = fmaf(w, v[o + j], m2);
                a11 = fmaf(w, u[o + j] * u[o + j], a11);
                a22 = fmaf(w, v[o + j] * v[o + j], a22);
                a12 = fmaf(w, u[o + j] * v[o + j], a12);
            }
            if (c0 + o < out_cols) {
                const int i = r * out_pitch + c0 + o;
                hs[i] = m1;
                hs[plane + i] = m2;
                hs[2 * plane + i] = a11;
                hs[3 * plane + i] = a22;
                hs[4 * plane + i] = a12;
            }
        }
    }
}

// Vertical pass for the 64 x 16 output tile: lane column c = tid & 63 and four consecutive rows
// r0..r0+3 per thread, a 14-row sliding window per quantity.
template <int NQ>
__device__ __forceinline__ void vpass_tile(const float *hs, int pitch, int plane, const Window &win,
                                           float (&acc)[NQ][4]) {
    const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
#pragma unroll
        for (int k = 0; k < 4; k++) acc[q][k] = 0.f;
        const float *h = hs + q * plane + r0 * pitch + c;
#pragma unroll
        for (int t = 0; t < 2 * kR + 4; t++) {
            const float v = h[t * pitch];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = t - k;
                if (j >= 0 && j <= 2 * kR) acc[q][k] = fmaf(win.w[j], v, acc[q][k]);
            }
        }
    }
}

template <int kThreads = kLossThreads>
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum(v);
    const int wv = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wv] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kThreads / 64; k++) s += red[k];
    return s;
}

}  // namespace
}  // namespace gsr
