// The kernels every training family launches as they are (train.hip: the ConvNets, tcn_train.hip: the TCN): the ascending
// reduction of a weight gradient's partial tiles, the cross-entropy of two-class logits, and Adam over a flat parameter vector.
// In an anonymous namespace: each file's code is what it was with the definitions in its own text.
#pragma once
#include "../common.hpp"

namespace rs {
namespace {

// grad[i] = partial[0][i] + partial[1][i] + ..., ascending
__global__ __launch_bounds__(256) void train_reduce_kernel(const float* __restrict__ partial, int n_slices, int64_t n,
                                                           float* __restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = partial[i];
#pragma unroll 8
    for (int k = 1; k < n_slices; ++k) s += partial[(int64_t)k * n + i];
    grad[i] = s;
}

// out[0] = mean loss, out[1] = reads whose argmax is their label, out[2 ..] = logits (already there); dlogits; flag[0] = 1
// where a label is outside {0, 1}.  One thread: B terms in read order.
__global__ void train_loss_kernel(float* __restrict__ out, const int32_t* __restrict__ labels, int B,
                                  float* __restrict__ dlogits, int32_t* __restrict__ flag) {
    if (threadIdx.x || blockIdx.x) return;
    double loss = 0.0;
    int correct = 0, bad = 0;
    for (int b = 0; b < B; ++b) {
        const double l0 = out[2 + 2 * b], l1 = out[3 + 2 * b];
        int y = labels[b];
        if (y < 0 || y > 1) {
            bad = 1;
            y = 0;
        }
        const double mx = fmax(l0, l1);
        const double lse = mx + log(exp(l0 - mx) + exp(l1 - mx));
        loss += lse - (y ? l1 : l0);
        correct += ((l1 > l0) ? 1 : 0) == y;                // argmax takes the first of equal logits
        dlogits[2 * b] = (float)((exp(l0 - lse) - (y == 0 ? 1.0 : 0.0)) / B);
        dlogits[2 * b + 1] = (float)((exp(l1 - lse) - (y == 1 ? 1.0 : 0.0)) / B);
    }
    out[0] = (float)(loss / B);
    out[1] = (float)correct;
    flag[0] = bad;
}

// torch.optim.Adam (no weight decay, no amsgrad): step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), both from the host
__global__ __launch_bounds__(256) void train_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, int64_t n, float beta1,
                                                         float beta2, float step_size, float bc2_sqrt, float eps) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
}

}  // namespace
}  // namespace rs
