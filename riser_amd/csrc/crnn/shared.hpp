// What the CNN-RNN's fp32 kernels (crnn.hip) and its f16x3 kernels (crnn/x3.hpp) share: a read's lengths through the conv
// front, and the sigmoid.
#pragma once
#include "../common.hpp"

namespace rs {
namespace {

constexpr int kMaxConv = 16;

struct Lens {
    int n;                      // conv layers
    int k[kMaxConv];
};

// samples of read b after `upto` conv layers; 0 where the reference's conv or max_pool would raise
__device__ __forceinline__ int crnn_len(const int32_t* len, int b, int ld, const Lens& ls, int upto) {
    int L = as_const_len(len)[b];
    L = L < 0 ? 0 : (L > ld ? ld : L);
    for (int i = 0; i < upto; ++i) L = L >= ls.k[i] + 1 ? (L - ls.k[i] + 1) >> 1 : 0;
    return L;
}

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

}  // namespace
}  // namespace rs
