// TCN / TCNBot temporal blocks in split precision on the bf16 MFMA (rs_tcn_set_mode(m, RS_BF16X3)): the interface between
// the host program of csrc/tcn.hip and the kernel of csrc/tcn_x3.hip.
#pragma once
#include "common.hpp"

namespace rs {

constexpr int kTcnX3MaxConvs = 4;

inline int tcn_cp8(int c) { return (c + 7) & ~7; }

// Weights of one conv, split and packed on the host: two planes [hi | lo], each [steps][4][np][8] bf16 bit patterns.  K index
// 32 s + 8 kq + e is (tap, ci) = divmod(K, cp8(c_in)) (tap t reads the row m + t, i.e. w_ref[co][ci][k - 1 - t]); zero where
// tap >= k, ci >= c_in or co >= c_out.  steps = ceil(k cp8(c_in) / 32), np = c_out rounded up to 16.
std::vector<unsigned short> tcn_x3_pack(const float* w /* [c_out][c_in][k] */, int c_out, int c_in, int k, int* steps, int* np);

struct TcnX3Args {
    const float* x;             // block input: [B][in_rows][cp_in] fp32 (block 0: the signal, [B][ld])
    const int32_t* len;
    float* y;                   // block output: [B][out_rows][cp_out] fp32
    int B, ld, first;
    int64_t dil;
    int r;                      // base: output m' is input m = r * m'
    int in_rows, out_rows;
    int cp_in, cp_out;          // global row pitches (floats, channels padded to 4)
    int T, nb, tiles_pos, rows_in;
    int nconv;
    const unsigned short* w[kTcnX3MaxConvs];   // tcn_x3_pack planes
    const float* b[kTcnX3MaxConvs];            // [np]
    int k[kTcnX3MaxConvs], cpi[kTcnX3MaxConvs], cpo[kTcnX3MaxConvs], np[kTcnX3MaxConvs], steps[kTcnX3MaxConvs];
    int rows[kTcnX3MaxConvs], step[kTcnX3MaxConvs], ostride[kTcnX3MaxConvs];
    int src[kTcnX3MaxConvs], dst[kTcnX3MaxConvs];   // LDS buffers: 0 = X, 1 = P, 2 = Q; dst -1 = global
    // the same resolved per conv (halfwords): source offset, pitch, plane and rows per read; destination offset, pitch, plane
    int s_off[kTcnX3MaxConvs], s_pitch[kTcnX3MaxConvs], s_plane[kTcnX3MaxConvs], s_rows[kTcnX3MaxConvs];
    int d_off[kTcnX3MaxConvs], d_pitch[kTcnX3MaxConvs], d_plane[kTcnX3MaxConvs];
    const unsigned short* sw;   // shortcut planes (k = 1) or null (identity)
    const float* sb;
    int sw_steps;
    int off[3], pitch[3], plane[3];   // LDS buffers in halfwords: hi plane at off, lo plane at off + plane; row pitch
};

struct TcnX3Plan {
    int rows[kTcnX3MaxConvs], rows_in;
    int off[3], pitch[3], plane[3];
    size_t lds_bytes;
};

// rows of every conv's output per read for a tile of T outputs of nb reads, the X rows, and the LDS layout.  cpi / cpo: the
// convs' channels padded to 8.
TcnX3Plan tcn_x3_plan(int nconv, const int* k, const int* cpi, const int* cpo, int jk, int base, int T, int nb);

hipError_t tcn_x3_launch(const TcnX3Args& a, unsigned grid, size_t lds_bytes, hipStream_t st);

}  // namespace rs
