// The per-chunk, per-block and per-pixel functions of the JPEG decoder (include/yolo355_jpeg.h), written once for the GPU
// kernels (y3_jpeg.hip) and for the host build tests/test_jpeg_cpu.py runs against Pillow (tests/jpeg_emul.cpp).  Integer
// arithmetic only.  Each step restates libjpeg-turbo's default decompression path, the one Pillow takes:
//   entropy   jdhuff.c decode_mcu: Huffman symbol, extra bits, HUFF_EXTEND, runs, EOB, DC prediction per component
//   IDCT      jidctint.c jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2, columns then rows, the masked range limit
//   upsample  jdsample.c h2v1 / h2v2 fancy upsampling (triangle filter, alternating rounding biases, edge replication)
//   colour    jdcolor.c ycc_rgb_convert with its 16-bit fixed-point tables
// Everything that reads the blob is bounded by the record's extents, which the host checks (rec_check) before a launch.
#pragma once
#include <stdint.h>
#include "../../include/yolo355_jpeg.h"

#ifdef __HIPCC__
#define Y3J_HD __host__ __device__ __forceinline__
#else
#define Y3J_HD inline
#endif

namespace y3jpx {

// status bits of an image
constexpr int kBadCode = 1, kOverrun = 2, kBlockCount = 4, kNoSync = 8;

struct Chunk {
    uint32_t first, end, seg;
};

// the state of the decoder at a codeword boundary: bit position, next coefficient z of the block, block b of the MCU
struct State {
    uint32_t pos;
    int z, b;
};

Y3J_HD uint32_t pack(int z, int b) { return (uint32_t)z | ((uint32_t)b << 8); }

// natural-order index of zig-zag position z; positions past 63 (a run that overflows the block) land on 63, as
// jpeg_natural_order's 16 guard entries make them in libjpeg
constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
Y3J_HD int natural(int z) { return z < 64 ? kNatural[z] : 63; }

// 16 bits of the data starting at bit `pos`, zeros past the end
Y3J_HD uint32_t peek16(const uint8_t* d, uint64_t nbytes, uint32_t pos) {
    const uint64_t byte = pos >> 3;
    uint32_t w = 0;
    for (int i = 0; i < 3; ++i) w = (w << 8) | (byte + i < nbytes ? d[byte + i] : 0u);
    return (w >> (8 - (pos & 7))) & 0xFFFFu;
}

// jdhuff's look-ahead then maxcode / valoffset walk; -1: no code of <= 16 bits
Y3J_HD int huff_decode(const y3j_huff& t, uint32_t bits16, int* len) {
    const uint32_t e = t.look[bits16 >> (16 - Y3J_LOOKAHEAD)];
    if (e >> 8) {
        *len = (int)(e >> 8);
        return (int)(e & 255);
    }
    for (int l = Y3J_LOOKAHEAD + 1; l <= 16; ++l) {
        const int code = (int)(bits16 >> (16 - l));
        if (code <= t.maxcode[l]) {
            *len = l;
            return t.huffval[(code + t.valoffset[l]) & 255];
        }
    }
    return -1;
}

Y3J_HD int extend(uint32_t v, int s) { return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// decode-order block g -> block index in the coefficient array (plane of its component, row-major)
Y3J_HD int block_addr(const y3j_rec& r, int g) {
    const int mcu = g / r.blocks_per_mcu, b = g - mcu * r.blocks_per_mcu;
    const int c = r.blk_comp[b];
    const int hc = r.comp_bw[c] / r.mcus_x, vc = r.comp_bh[c] / r.mcus_y;
    const int bx = (mcu % r.mcus_x) * hc + r.blk_dx[b], by = (mcu / r.mcus_x) * vc + r.blk_dy[b];
    return r.comp_block0[c] + by * r.comp_bw[c] + bx;
}

Y3J_HD Chunk chunk_of(const y3j_rec& r, const uint8_t* blob, int c) {
    const uint32_t* t = reinterpret_cast<const uint32_t*>(blob + r.chunk_off) + 3 * (size_t)c;
    return Chunk{t[0], t[1], t[2]};
}

Y3J_HD uint32_t seg_bit(const y3j_rec& r, const uint8_t* blob, uint32_t s) {
    const uint32_t limit = (uint32_t)(r.data_bytes * 8);
    const uint32_t v = reinterpret_cast<const uint32_t*>(blob + r.seg_off)[s <= (uint32_t)r.n_seg ? s : r.n_seg];
    return v < limit ? v : limit;
}

// Decodes codewords from `st` while a codeword starts before `end` and fewer than `limit` blocks have been completed.
// WRITE: block `g` (decode order) is the one in progress; coefficients (DC differences in [0]) go to coef.  Returns 0 or a
// status bit; `done` counts the blocks completed.
template <bool WRITE>
Y3J_HD int decode_run(const y3j_rec& r, const y3j_huff* tabs, const uint8_t* data, uint32_t seg_end, uint32_t end, State& st,
                      int& done, int limit, int g, int16_t* coef) {
    const int ntab = r.n_tables;
    while (st.pos < end && done < limit) {
        const int c = r.blk_comp[st.b];
        int ti = st.z == 0 ? r.comp_dc[c] : r.comp_ac[c];
        ti = ti < ntab ? ti : 0;
        int len = 0;
        const int sym = huff_decode(tabs[ti], peek16(data, r.data_bytes, st.pos), &len);
        if (sym < 0) return kBadCode;
        uint32_t p = st.pos + (uint32_t)len;
        int s, v = 0;
        if (st.z == 0) {
            s = sym & 15;
            if (s) {
                if (p + s > seg_end) return kOverrun;
                v = extend(peek16(data, r.data_bytes, p) >> (16 - s), s);
                p += s;
            }
            if (WRITE) {
                if (g >= r.total_blocks) return kBlockCount;
                coef[(size_t)block_addr(r, g) * 64] = (int16_t)v;
            }
            st.z = 1;
        } else {
            const int run = sym >> 4;
            s = sym & 15;
            if (s) {
                st.z += run;
                if (p + s > seg_end) return kOverrun;
                v = extend(peek16(data, r.data_bytes, p) >> (16 - s), s);
                p += s;
                if (WRITE) {
                    if (g >= r.total_blocks) return kBlockCount;
                    coef[(size_t)block_addr(r, g) * 64 + natural(st.z)] = (int16_t)v;
                }
                st.z += 1;
            } else if (run == 15) {
                st.z += 16;
            } else {
                st.z = 64;
            }
        }
        if (p > seg_end) return kOverrun;
        st.pos = p;
        if (st.z >= 64) {
            st.z = 0;
            st.b = st.b + 1 == r.blocks_per_mcu ? 0 : st.b + 1;
            ++done;
            ++g;
        }
    }
    return 0;
}

// state rows in the scratch: [0] start position, [1] start (z | b << 8 | dirty << 16), [2] exit position, [3] exit state,
// [4] blocks completed (then: first block of the chunk)
Y3J_HD int32_t* state_row(const y3j_rec& r, uint8_t* scratch, int row) {
    return reinterpret_cast<int32_t*>(scratch + r.state_off) + (size_t)row * r.n_chunk;
}

// every chunk starts from the guess (its first bit, z = 0, first block): exact for the first chunk of each interval
Y3J_HD void chunk_init(const y3j_rec& r, const uint8_t* blob, uint8_t* scratch, int c) {
    const Chunk k = chunk_of(r, blob, c);
    state_row(r, scratch, 0)[c] = (int32_t)k.first;
    state_row(r, scratch, 1)[c] = (int32_t)(pack(0, 0) | (1u << 16));
}

// one chunk of a synchronisation round, if its start state changed since it was last decoded
Y3J_HD void chunk_sync(const y3j_rec& r, const uint8_t* blob, uint8_t* scratch, const y3j_huff* tabs, int c) {
    int32_t* s1 = state_row(r, scratch, 1);
    const uint32_t zb = (uint32_t)s1[c];
    if (!(zb >> 16)) return;
    const Chunk k = chunk_of(r, blob, c);
    State st{(uint32_t)state_row(r, scratch, 0)[c], (int)(zb & 255), (int)((zb >> 8) & 255)};
    int done = 0;
    decode_run<false>(r, tabs, blob + r.data_off, seg_bit(r, blob, k.seg + 1), k.end, st, done, 0x7fffffff, 0, nullptr);
    state_row(r, scratch, 2)[c] = (int32_t)st.pos;
    state_row(r, scratch, 3)[c] = (int32_t)pack(st.z, st.b);
    state_row(r, scratch, 4)[c] = done;
    s1[c] = (int32_t)(zb & 0xFFFF);
}

// after a round: a chunk whose left neighbour (same interval) exits in another state than it started from adopts that
// state and is decoded again.  Returns whether it changed.
Y3J_HD bool chunk_adopt(const y3j_rec& r, const uint8_t* blob, uint8_t* scratch, int c) {
    if (c == 0 || chunk_of(r, blob, c).seg != chunk_of(r, blob, c - 1).seg) return false;
    const int32_t pos = state_row(r, scratch, 2)[c - 1], zb = state_row(r, scratch, 3)[c - 1];
    int32_t* s0 = state_row(r, scratch, 0);
    int32_t* s1 = state_row(r, scratch, 1);
    if (s0[c] == pos && (s1[c] & 0xFFFF) == zb) return false;
    s0[c] = pos;
    s1[c] = (int32_t)((uint32_t)zb | (1u << 16));
    return true;
}

// the first block (decode order) of interval s and the block after its last
Y3J_HD int seg_block0(const y3j_rec& r, uint32_t s) {
    return r.restart_interval ? (int)((long long)s * r.restart_interval * r.blocks_per_mcu < r.total_blocks
                                          ? (long long)s * r.restart_interval * r.blocks_per_mcu : r.total_blocks)
                              : 0;
}
Y3J_HD int seg_block_end(const y3j_rec& r, uint32_t s) {
    return r.restart_interval ? seg_block0(r, s + 1) : r.total_blocks;
}

// the final pass: chunk c from its true start state, its first block `first` (decode order, from the segmented prefix
// sum of the completed-block counts) writes its coefficients.  Returns status bits.
Y3J_HD int chunk_write(const y3j_rec& r, const uint8_t* blob, uint8_t* scratch, const y3j_huff* tabs, int c, int first) {
    const Chunk k = chunk_of(r, blob, c);
    if (k.seg >= (uint32_t)r.n_seg) return kBlockCount;
    const uint32_t zb = (uint32_t)state_row(r, scratch, 1)[c];
    State st{(uint32_t)state_row(r, scratch, 0)[c], (int)(zb & 255), (int)((zb >> 8) & 255)};
    const int block_end = seg_block_end(r, k.seg);
    int done = 0;
    int16_t* coef = reinterpret_cast<int16_t*>(scratch + r.coef_off);
    int status = decode_run<true>(r, tabs, blob + r.data_off, seg_bit(r, blob, k.seg + 1), k.end, st, done, block_end - first,
                                  first, coef);
    const bool last = c + 1 == r.n_chunk || chunk_of(r, blob, c + 1).seg != k.seg;
    if (last && !status && (first + done != block_end || st.z != 0)) status = kBlockCount;
    return status;
}

// ---- dequantisation + jpeg_idct_islow of coefficient block k (plane order) into the component's plane -----------------
constexpr int kConstBits = 13, kPass1Bits = 2;
constexpr int32_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
                  F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;

Y3J_HD int32_t descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// jdmaster's post-IDCT range limit: the index is masked to 10 bits, i.e. wraps as a signed 10-bit value, then clamps
Y3J_HD uint8_t range_limit(int32_t x) {
    const int v = ((x + 512) & 1023) - 512 + 128;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

Y3J_HD void idct_block(const y3j_rec& r, const uint8_t* blob, uint8_t* scratch, int k) {
    int c = 0;
    while (c + 1 < r.components && k >= r.comp_block0[c + 1]) ++c;
    const int kb = k - r.comp_block0[c];
    const int bx = kb % r.comp_bw[c], by = kb / r.comp_bw[c];
    const int16_t* in = reinterpret_cast<const int16_t*>(scratch + r.coef_off) + (size_t)k * 64;
    const uint16_t* q = reinterpret_cast<const uint16_t*>(blob + r.quant_off) + 64 * c;
    const int stride = r.comp_bw[c] * 8;
    uint8_t* out = scratch + r.plane_off + r.comp_plane0[c] + (size_t)by * 8 * stride + bx * 8;
    int32_t ws[64];
    for (int col = 0; col < 8; ++col) {
        int32_t z1, z2, z3, z4, z5, tmp0, tmp1, tmp2, tmp3, tmp10, tmp11, tmp12, tmp13;
        z2 = in[16 + col] * (int32_t)q[16 + col];
        z3 = in[48 + col] * (int32_t)q[48 + col];
        z1 = (z2 + z3) * F0541;
        tmp2 = z1 + z3 * -F1847;
        tmp3 = z1 + z2 * F0765;
        z2 = in[col] * (int32_t)q[col];
        z3 = in[32 + col] * (int32_t)q[32 + col];
        tmp0 = (int32_t)((uint32_t)(z2 + z3) << kConstBits);
        tmp1 = (int32_t)((uint32_t)(z2 - z3) << kConstBits);
        tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = in[56 + col] * (int32_t)q[56 + col];
        tmp1 = in[40 + col] * (int32_t)q[40 + col];
        tmp2 = in[24 + col] * (int32_t)q[24 + col];
        tmp3 = in[8 + col] * (int32_t)q[8 + col];
        z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
        z5 = (z3 + z4) * F1175;
        tmp0 *= F0298, tmp1 *= F2053, tmp2 *= F3072, tmp3 *= F1501;
        z1 *= -F0899, z2 *= -F2562, z3 *= -F1961, z4 *= -F0390;
        z3 += z5, z4 += z5;
        tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
        const int n = kConstBits - kPass1Bits;
        ws[col] = descale(tmp10 + tmp3, n), ws[56 + col] = descale(tmp10 - tmp3, n);
        ws[8 + col] = descale(tmp11 + tmp2, n), ws[48 + col] = descale(tmp11 - tmp2, n);
        ws[16 + col] = descale(tmp12 + tmp1, n), ws[40 + col] = descale(tmp12 - tmp1, n);
        ws[24 + col] = descale(tmp13 + tmp0, n), ws[32 + col] = descale(tmp13 - tmp0, n);
    }
    for (int row = 0; row < 8; ++row) {
        const int32_t* w = ws + 8 * row;
        int32_t z1, z2, z3, z4, z5, tmp0, tmp1, tmp2, tmp3, tmp10, tmp11, tmp12, tmp13;
        z2 = w[2], z3 = w[6];
        z1 = (z2 + z3) * F0541;
        tmp2 = z1 + z3 * -F1847;
        tmp3 = z1 + z2 * F0765;
        tmp0 = (int32_t)((uint32_t)(w[0] + w[4]) << kConstBits);
        tmp1 = (int32_t)((uint32_t)(w[0] - w[4]) << kConstBits);
        tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = w[7], tmp1 = w[5], tmp2 = w[3], tmp3 = w[1];
        z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
        z5 = (z3 + z4) * F1175;
        tmp0 *= F0298, tmp1 *= F2053, tmp2 *= F3072, tmp3 *= F1501;
        z1 *= -F0899, z2 *= -F2562, z3 *= -F1961, z4 *= -F0390;
        z3 += z5, z4 += z5;
        tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
        const int n = kConstBits + kPass1Bits + 3;
        uint8_t* o = out + (size_t)row * stride;
        o[0] = range_limit(descale(tmp10 + tmp3, n)), o[7] = range_limit(descale(tmp10 - tmp3, n));
        o[1] = range_limit(descale(tmp11 + tmp2, n)), o[6] = range_limit(descale(tmp11 - tmp2, n));
        o[2] = range_limit(descale(tmp12 + tmp1, n)), o[5] = range_limit(descale(tmp12 - tmp1, n));
        o[3] = range_limit(descale(tmp13 + tmp0, n)), o[4] = range_limit(descale(tmp13 - tmp0, n));
    }
}

// ---- fancy upsampling + YCbCr -> RGB of output pixel (x, y) ------------------------------------------------------------
Y3J_HD int sample(const y3j_rec& r, const uint8_t* planes, int c, int x, int y) {
    x = x < 0 ? 0 : (x >= r.comp_dw[c] ? r.comp_dw[c] - 1 : x);      // edges: the last real column / row, replicated
    y = y < 0 ? 0 : (y >= r.comp_dh[c] ? r.comp_dh[c] - 1 : y);
    return planes[r.comp_plane0[c] + (size_t)y * r.comp_bw[c] * 8 + x];
}

Y3J_HD int chroma(const y3j_rec& r, const uint8_t* planes, int c, int x, int y) {
    if (r.hmax == 1) return sample(r, planes, c, x, y);
    const int k = x >> 1, odd = x & 1;
    // jdsample.c jinit_upsampler takes the fancy (triangle) filters only when downsampled_width > 2; a narrower plane is
    // replicated (h2v1_upsample / h2v2_upsample), in both directions
    if (r.comp_dw[c] <= 2) return sample(r, planes, c, k, r.vmax == 1 ? y : y >> 1);
    if (r.vmax == 1) {          // h2v1: 3/4 nearer + 1/4 further, biases 1 (even) and 2 (odd)
        const int a = 3 * sample(r, planes, c, k, y);
        return odd ? (a + sample(r, planes, c, k + 1, y) + 2) >> 2 : (a + sample(r, planes, c, k - 1, y) + 1) >> 2;
    }
    const int row = y >> 1, near = (y & 1) ? row + 1 : row - 1;     // h2v2: column sums of 3/4 this row + 1/4 the next
    const int cs = 3 * sample(r, planes, c, k, row) + sample(r, planes, c, k, near);
    const int k2 = odd ? k + 1 : k - 1;
    const int cs2 = 3 * sample(r, planes, c, k2, row) + sample(r, planes, c, k2, near);
    return odd ? (3 * cs + cs2 + 7) >> 4 : (3 * cs + cs2 + 8) >> 4;
}

Y3J_HD uint8_t clamp_u8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

Y3J_HD void rgb_pixel(const y3j_rec& r, const uint8_t* planes, int x, int y, uint8_t out[3]) {
    const int Y = sample(r, planes, 0, x, y);
    if (r.components == 1) {
        out[0] = out[1] = out[2] = (uint8_t)Y;
        return;
    }
    const int cb = chroma(r, planes, 1, x, y) - 128, cr = chroma(r, planes, 2, x, y) - 128;
    const int32_t half = 1 << 15;
    out[0] = clamp_u8(Y + ((91881 * cr + half) >> 16));
    out[1] = clamp_u8(Y + ((-22554 * cb + half + -46802 * cr) >> 16));
    out[2] = clamp_u8(Y + ((116130 * cb + half) >> 16));
}

// ---- the host's check of one record against the buffers it will be launched on ----------------------------------------
// `scratch_head`: the bytes at the start of the scratch that hold the device copy of the records (nothing else may lie there)
inline bool rec_check(const y3j_rec& r, size_t blob_bytes, size_t scratch_bytes, size_t out_bytes, size_t scratch_head = 0) {
    auto fits = [](uint64_t off, uint64_t bytes, uint64_t total) { return off <= total && bytes <= total - off; };
    if (r.coef_off < scratch_head || r.plane_off < scratch_head || r.state_off < scratch_head) return false;
    if (r.components != 1 && r.components != 3) return false;
    if (r.width <= 0 || r.height <= 0 || r.width > 65535 || r.height > 65535) return false;
    if (r.n_tables < 1 || r.n_tables > 8 || r.blocks_per_mcu < 1 || r.blocks_per_mcu > 10) return false;
    if (r.hmax < 1 || r.hmax > 2 || r.vmax < 1 || r.vmax > r.hmax || r.mcus_x < 1 || r.mcus_y < 1) return false;
    if (r.restart_interval < 0 || r.n_seg < 1 || r.n_chunk < r.n_seg || r.data_bytes > 0x1FFFFFFFull) return false;
    const long long mcus = (long long)r.mcus_x * r.mcus_y;
    if (mcus * r.blocks_per_mcu != r.total_blocks || mcus * r.blocks_per_mcu > (1 << 24)) return false;
    if (r.restart_interval ? r.n_seg != (mcus + r.restart_interval - 1) / r.restart_interval : r.n_seg != 1) return false;
    long long blocks = 0, plane_end = 0;
    for (int c = 0; c < r.components; ++c) {
        if (r.comp_dc[c] < 0 || r.comp_dc[c] >= r.n_tables || r.comp_ac[c] < 0 || r.comp_ac[c] >= r.n_tables) return false;
        if (r.comp_bw[c] < 1 || r.comp_bh[c] < 1 || r.comp_bw[c] % r.mcus_x || r.comp_bh[c] % r.mcus_y) return false;
        if (r.comp_dw[c] < 1 || r.comp_dh[c] < 1 || r.comp_dw[c] > 8 * r.comp_bw[c] || r.comp_dh[c] > 8 * r.comp_bh[c])
            return false;
        if (r.comp_block0[c] != blocks || r.comp_plane0[c] < plane_end) return false;
        blocks += (long long)r.comp_bw[c] * r.comp_bh[c];
        plane_end = r.comp_plane0[c] + 64LL * r.comp_bw[c] * r.comp_bh[c];
    }
    // the luma plane covers the image; chroma index (x >> 1) stays inside comp_dw by construction of sample()
    if (blocks != r.total_blocks || r.comp_dw[0] < r.width || r.comp_dh[0] < r.height) return false;
    if (r.components == 3 && ((r.width + r.hmax - 1) / r.hmax > 8 * r.comp_bw[1] || (r.height + r.vmax - 1) / r.vmax >
                              8 * r.comp_bh[1]))
        return false;
    int in_mcu[3] = {0, 0, 0};
    for (int b = 0; b < r.blocks_per_mcu; ++b) {
        const int c = r.blk_comp[b];
        if (c < 0 || c >= r.components) return false;
        const int hc = r.comp_bw[c] / r.mcus_x, vc = r.comp_bh[c] / r.mcus_y;
        if (r.blk_dx[b] < 0 || r.blk_dx[b] >= hc || r.blk_dy[b] < 0 || r.blk_dy[b] >= vc) return false;
        ++in_mcu[c];
    }
    for (int c = 0; c < r.components; ++c)
        if (in_mcu[c] != (r.comp_bw[c] / r.mcus_x) * (r.comp_bh[c] / r.mcus_y)) return false;
    const uint64_t offs[] = {r.tables_off, r.quant_off, r.seg_off, r.chunk_off, r.coef_off, r.state_off};
    for (uint64_t o : offs)
        if (o % 16) return false;
    return fits(r.tables_off, (uint64_t)r.n_tables * sizeof(y3j_huff), blob_bytes) &&
           fits(r.quant_off, 128ull * r.components, blob_bytes) && fits(r.data_off, r.data_bytes, blob_bytes) &&
           fits(r.seg_off, 4ull * (r.n_seg + 1), blob_bytes) && fits(r.chunk_off, 12ull * r.n_chunk, blob_bytes) &&
           fits(r.coef_off, 128ull * r.total_blocks, scratch_bytes) && fits(r.plane_off, (uint64_t)plane_end, scratch_bytes) &&
           fits(r.state_off, 20ull * r.n_chunk, scratch_bytes) && fits(r.out_off, 3ull * r.width * r.height, out_bytes);
}

}  // namespace y3jpx
