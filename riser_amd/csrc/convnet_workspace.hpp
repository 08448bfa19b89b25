// The workspace of a call: where the block tables, the normalised signals and the activation buffers lie in it (WsLayout),
// and what one call runs on (Batch).
#pragma once
#include <algorithm>

#include "common.hpp"
#include "convnet_model.hpp"

namespace rs {
namespace {

constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// Workspace: [coarse block table][fine block table][16 zero bytes | normalised signals, fine blocks of Uf floats][activation
// buffer A][B].  Laid out for the upper bounds NB = B * (Lmax / U + 1) blocks of either size, so the offsets depend on
// (B, Lmax) only; a batch of mixed lengths uses a prefix of every region.  With one level the fine table IS the coarse one.
struct WsLayout {
    size_t rbase_off, blen_off, bread_off;          // coarse table
    size_t rbase_f_off, blen_f_off, bread_f_off;    // fine table (== coarse when the model has one level)
    size_t xnorm_off, bufa_off, bufb_off, fc_part_off, total;
    int U, Uf;              // block sizes in samples (1 << pad_shift, 1 << fine_shift)
    int nblk_max, nblk_f_max;   // blocks of a read of Lmax samples
    int64_t nb_max, nb_f_max;   // B * nblk_max
};

WsLayout ws_layout(const rs_model* m, int B, int Lmax) {
    WsLayout w{};
    const bool two = two_level(m);
    w.U = 1 << m->pad_shift;
    w.Uf = two ? 1 << m->fine_shift : w.U;
    w.nblk_max = (Lmax >> m->pad_shift) + 1;
    w.nb_max = (int64_t)B * w.nblk_max;
    w.nblk_f_max = two ? (Lmax >> m->fine_shift) + 1 : w.nblk_max;
    w.nb_f_max = (int64_t)B * w.nblk_f_max;
    size_t buf = 0;
    for (int i = 0; i < m->n_layers; ++i) {                       // layer i's output buffer
        const bool fine = two && i < m->split;
        const size_t rows = fine ? (size_t)w.nb_f_max * (w.Uf >> (i + 1)) : (size_t)w.nb_max * (w.U >> (i + 1));
        // F8 rows carry their scale plane behind them (conv_ring_f8.hip)
        const bool f8 = i + 1 < m->n_layers && m->layers[i + 1].f8_in;
        auto bytes_of = [&](size_t r) { return f8 ? f8_scale_offset((int64_t)r, m->cp[i]) + f8_scale_bytes((int64_t)r, m->cp[i]) : r * m->cp[i] * esize(m); };
        buf = std::max(buf, bytes_of(rows));
        if (two && i == m->split - 1)                             // ... and its re-packed copy in the coarse layout
            buf = std::max(buf, bytes_of((size_t)w.nb_max * (w.U >> (i + 1))));
    }
    buf = align_up(buf + kAlign);
    w.rbase_off = 0;
    w.blen_off = align_up((size_t)(B + 1) * 4);
    w.bread_off = w.blen_off + align_up((size_t)w.nb_max * 4);
    size_t at = w.bread_off + align_up((size_t)w.nb_max * 4);
    if (two) {
        w.rbase_f_off = at;
        w.blen_f_off = w.rbase_f_off + align_up((size_t)(B + 1) * 4);
        w.bread_f_off = w.blen_f_off + align_up((size_t)w.nb_f_max * 4);
        at = w.bread_f_off + align_up((size_t)w.nb_f_max * 4);
    } else {
        w.rbase_f_off = w.rbase_off;
        w.blen_f_off = w.blen_off;
        w.bread_f_off = w.bread_off;
    }
    w.xnorm_off = at + kAlign;                                    // the last 16 bytes before the rows are a zero prefix
    w.bufa_off = align_up(w.xnorm_off + (size_t)w.nb_f_max * w.Uf * sizeof(float));
    w.bufb_off = w.bufa_off + buf;
    w.fc_part_off = w.bufb_off + buf;
    w.total = w.fc_part_off + (m->fc.H ? align_up(fc_head_workspace_bytes(B, m->fc.H)) : 0);
    return w;
}

// What one call runs on: the block table(s) in the workspace and the number of blocks in use (host-known: from the host's
// copy of the lengths, or nblk_max blocks for every read when it has none)
struct Batch {
    BlockPlan plan;         // coarse: late layers, head
    BlockPlan fine;         // early layers, normalised rows (a copy of `plan` when the model has one level)
    int NB = 0, NBf = 0;    // blocks in use
    int Lmin_blk = 0, Lmin_blk_f = 0;   // lower bound of blen over the reads' last blocks (dead-tile hint), 0 = unknown
};

// h_len may be NULL.  Returns RS_OK or RS_ERR_LENGTH (a host length outside [2^n_layers, Lmax]).
int make_batch(const rs_model* m, const WsLayout& w, void* d_ws, const int32_t* h_len, int B, int Lmin, int Lmax, Batch* out) {
    char* ws = static_cast<char*>(d_ws);
    const bool two = two_level(m);
    Batch bt;
    bt.plan.rbase = reinterpret_cast<int32_t*>(ws + w.rbase_off);
    bt.plan.blen = reinterpret_cast<int32_t*>(ws + w.blen_off);
    bt.plan.bread = reinterpret_cast<int32_t*>(ws + w.bread_off);
    bt.plan.shift = m->pad_shift;
    bt.fine.rbase = reinterpret_cast<int32_t*>(ws + w.rbase_f_off);
    bt.fine.blen = reinterpret_cast<int32_t*>(ws + w.blen_f_off);
    bt.fine.bread = reinterpret_cast<int32_t*>(ws + w.bread_f_off);
    bt.fine.shift = two ? m->fine_shift : m->pad_shift;
    if (h_len) {
        int64_t nb = 0, nbf = 0;
        int lmin_blk = w.U, lmin_blk_f = w.Uf;
        for (int b = 0; b < B; ++b) {
            const int n = h_len[b];
            if (n < (1 << m->n_layers) || n > Lmax) {
                set_error("read %d has %d samples, outside [%d, Lmax = %d]", b, n, 1 << m->n_layers, Lmax);
                return RS_ERR_LENGTH;
            }
            nb += (n >> m->pad_shift) + 1;
            nbf += (n >> bt.fine.shift) + 1;
            lmin_blk = std::min(lmin_blk, n & (w.U - 1));            // the read's last block holds len mod U samples
            lmin_blk_f = std::min(lmin_blk_f, n & (w.Uf - 1));
        }
        bt.plan.uniform_nblk = bt.fine.uniform_nblk = 0;
        bt.NB = (int)nb;
        bt.NBf = (int)nbf;
        bt.Lmin_blk = lmin_blk;
        bt.Lmin_blk_f = lmin_blk_f;
    } else {
        bt.plan.uniform_nblk = w.nblk_max;
        bt.fine.uniform_nblk = w.nblk_f_max;
        bt.NB = (int)w.nb_max;
        bt.NBf = (int)w.nb_f_max;
        // every read has nblk_max blocks: the last one of the shortest read holds max(Lmin - (nblk_max - 1) U, 0) samples
        bt.Lmin_blk = Lmin > 0 ? std::max(0, std::min(w.U, Lmin - (w.nblk_max - 1) * w.U)) : 0;
        bt.Lmin_blk_f = Lmin > 0 ? std::max(0, std::min(w.Uf, Lmin - (w.nblk_f_max - 1) * w.Uf)) : 0;
    }
    bt.plan.nb_total = bt.NB;
    bt.fine.nb_total = bt.NBf;
    *out = bt;
    return RS_OK;
}

int check_call(const char* who, const rs_model* m, int B, int Lmax, const WsLayout& w, size_t ws_bytes) {
    if (ws_bytes < w.total) {
        set_error("%s: workspace %zu < required %zu", who, ws_bytes, w.total);
        return RS_ERR_WORKSPACE;
    }
    if (w.nb_max * (w.U / 2) > 0x7fffffffLL || w.nb_f_max * (w.Uf / 2) > 0x7fffffffLL) {
        set_error("%s: batch too large, split it (%d reads of up to %d samples)", who, B, Lmax);
        return RS_ERR_ARG;
    }
    return RS_OK;
}

}  // namespace
}  // namespace rs
