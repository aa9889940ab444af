// liby3feed.so: the host half of the feeder's JPEG decoder (include/yolo355_jpeg.h).  What is O(file bytes) and nothing
// more: the marker walk, jdhuff's derived Huffman tables, the quantisation tables in natural order, the entropy-coded data
// with its FF00 stuffing and RST markers removed, and the cut of every restart interval into chunks for the device's
// self-synchronising decoder (csrc/y3_jpeg.hip).  Every read is bounded by the file's length.
#include "../../include/yolo355_feed.h"
#include "../../include/yolo355_jpeg.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

int y3f_fail(int code, const char* fmt, ...);       // y3_feed.cpp: sets y3f_last_error()

static_assert(sizeof(y3j_huff) == 1424, "the device copies y3j_huff in 4-byte words");
static_assert(sizeof(y3j_rec) == 272 && sizeof(y3j_rec) % 16 == 0, "jpeg.py and the device kernels assume this layout");

namespace {

constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr int kTargetChunks = 512;      // y3_jpeg.hip's workgroup: about one chunk per thread
constexpr uint32_t kMinChunkBits = 256;
constexpr long long kMaxBlocks = 1 << 24;   // rec_check's limit (y3_jpeg_px.h)
constexpr int kMaxThreads = 8;              // the default (threads = 0) pool: the hardware's threads, at most this many

struct Huff {
    bool defined = false;
    uint8_t bits[17] = {};
    uint8_t vals[256] = {};
};

struct Comp {
    int id, h, v, tq, td, ta;
};

struct Parsed {
    y3f_jpeg_info info{};
    int ncomp = 0;
    Comp comp[4]{};
    Huff huff[2][4];            // [class: 0 DC, 1 AC][id], as they stood at the SOS
    uint16_t quant[4][64]{};    // natural order, as they stood at the SOS
    size_t scan_begin = 0, scan_end = 0;
    int n_rst = 0;
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// jdhuff.c jpeg_make_d_derived_tbl, with the 9-bit look-ahead the device uses
int derive(const Huff& h, bool dc, y3j_huff& t) {
    memset(&t, 0, sizeof(t));
    int huffsize[257], huffcode[257], p = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < h.bits[l]; ++i) {
            if (p >= 256) return y3f_fail(Y3F_EINVAL, "jpeg: Huffman table with more than 256 symbols");
            huffsize[p++] = l;
        }
    huffsize[p] = 0;
    const int nsym = p;
    int code = 0, si = nsym ? huffsize[0] : 0;
    p = 0;
    while (huffsize[p]) {
        while (huffsize[p] == si) huffcode[p++] = code++;
        if (code >= (1 << si)) return y3f_fail(Y3F_EINVAL, "jpeg: bad Huffman table");
        code <<= 1;
        ++si;
    }
    p = 0;
    for (int l = 1; l <= 16; ++l) {
        if (h.bits[l]) {
            t.valoffset[l] = p - huffcode[p];
            p += h.bits[l];
            t.maxcode[l] = huffcode[p - 1];
        } else {
            t.maxcode[l] = -1;
        }
    }
    t.maxcode[17] = 0xFFFFF;
    memcpy(t.huffval, h.vals, 256);
    for (int i = 0; i < nsym; ++i) {
        if (dc && h.vals[i] > 15) return y3f_fail(Y3F_EINVAL, "jpeg: DC Huffman symbol %d > 15", h.vals[i]);
        const int l = huffsize[i];
        if (l > Y3J_LOOKAHEAD) continue;
        const int first = huffcode[i] << (Y3J_LOOKAHEAD - l);
        for (int k = 0; k < (1 << (Y3J_LOOKAHEAD - l)); ++k) t.look[first + k] = (uint16_t)((l << 8) | h.vals[i]);
    }
    return Y3F_OK;
}

int unsupported(Parsed& p, int reason) {
    if (p.info.supported) p.info.supported = 0, p.info.reason = reason;
    return Y3F_OK;
}

// the whole marker walk; Y3F_EINVAL for a malformed or truncated stream, else info.supported / reason
int parse(const uint8_t* d, size_t len, Parsed& p) {
    if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) return y3f_fail(Y3F_EINVAL, "jpeg: not a JPEG stream (no SOI)");
    bool sof = false, eoi = false, jfif = false, adobe = false;
    int sof_type = -1, adobe_transform = -1, n_sos = 0, scan_ok = 1, ri = 0;
    Huff huff[2][4];
    bool qdef[4] = {false, false, false, false};
    uint16_t quant[4][64] = {};
    p.info.supported = 1;
    size_t pos = 2;
    while (!eoi) {
        if (pos >= len) return y3f_fail(Y3F_EINVAL, "jpeg: truncated stream (no EOI)");
        if (d[pos] != 0xFF) return y3f_fail(Y3F_EINVAL, "jpeg: expected a marker at byte %zu", pos);
        while (pos < len && d[pos] == 0xFF) ++pos;
        if (pos >= len) return y3f_fail(Y3F_EINVAL, "jpeg: truncated stream (no EOI)");
        const int m = d[pos++];
        if (m == 0xD9) {
            eoi = true;
            break;
        }
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD8) return y3f_fail(Y3F_EINVAL, "jpeg: a second SOI");
        if (pos + 2 > len) return y3f_fail(Y3F_EINVAL, "jpeg: truncated marker segment");
        const size_t L = (size_t)be16(d + pos);
        if (L < 2 || pos + L > len) return y3f_fail(Y3F_EINVAL, "jpeg: truncated marker segment 0x%02X", m);
        const uint8_t* s = d + pos + 2;
        const size_t n = L - 2;
        size_t next = pos + L;
        if ((m >= 0xC0 && m <= 0xC3) || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF)) {
            if (sof) return y3f_fail(Y3F_EINVAL, "jpeg: a second frame header");
            if (n < 6) return y3f_fail(Y3F_EINVAL, "jpeg: short frame header");
            sof = true;
            sof_type = m;
            const int prec = s[0], nf = s[5];
            p.info.height = be16(s + 1);
            p.info.width = be16(s + 3);
            if (nf < 1 || nf > 4 || n < 6 + 3 * (size_t)nf) return y3f_fail(Y3F_EINVAL, "jpeg: bad frame header");
            if (p.info.width == 0) return y3f_fail(Y3F_EINVAL, "jpeg: width 0");
            p.ncomp = p.info.components = nf;
            for (int c = 0; c < nf; ++c) {
                Comp& k = p.comp[c];
                k.id = s[6 + 3 * c];
                k.h = s[7 + 3 * c] >> 4;
                k.v = s[7 + 3 * c] & 15;
                k.tq = s[8 + 3 * c];
                if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3)
                    return y3f_fail(Y3F_EINVAL, "jpeg: bad component %d in the frame header", c);
            }
            p.info.h_samp = p.comp[0].h, p.info.v_samp = p.comp[0].v;
            if (m == 0xC2 || m == 0xC6) unsupported(p, Y3J_PROGRESSIVE);
            else if (m == 0xC3 || m == 0xC7 || m == 0xC5) unsupported(p, Y3J_LOSSLESS);
            else if (m >= 0xC9) unsupported(p, Y3J_ARITHMETIC);
            if (prec != 8) unsupported(p, Y3J_PRECISION);
            if (p.info.height == 0) unsupported(p, Y3J_SIZE);
        } else if (m == 0xC4) {                         // DHT: one or more tables
            size_t i = 0;
            while (i < n) {
                if (i + 17 > n) return y3f_fail(Y3F_EINVAL, "jpeg: short DHT");
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) return y3f_fail(Y3F_EINVAL, "jpeg: bad DHT class / id");
                Huff& h = huff[tc][th];
                int total = 0;
                h.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) total += (h.bits[l] = s[i + l]);
                if (total > 256 || i + 17 + total > n) return y3f_fail(Y3F_EINVAL, "jpeg: bad DHT counts");
                memset(h.vals, 0, sizeof(h.vals));
                memcpy(h.vals, s + i + 17, total);
                h.defined = true;
                i += 17 + total;
            }
        } else if (m == 0xDB) {                         // DQT: one or more tables, zig-zag order
            size_t i = 0;
            while (i < n) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (pq > 1 || tq > 3 || i + 1 + 64 * (pq + 1) > n) return y3f_fail(Y3F_EINVAL, "jpeg: bad DQT");
                for (int k = 0; k < 64; ++k) quant[tq][kNatural[k]] = pq ? (uint16_t)be16(s + i + 1 + 2 * k) : s[i + 1 + k];
                qdef[tq] = true;
                i += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) {
            if (n < 2) return y3f_fail(Y3F_EINVAL, "jpeg: short DRI");
            ri = be16(s);
        } else if (m == 0xDC) {
            unsupported(p, Y3J_SIZE);                   // DNL
        } else if (m == 0xE0) {
            if (n >= 5 && !memcmp(s, "JFIF\0", 5)) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && !memcmp(s, "Adobe", 5)) adobe = true, adobe_transform = s[11];
        } else if (m == 0xDA) {                         // SOS, then the entropy-coded data up to the next marker
            if (!sof) return y3f_fail(Y3F_EINVAL, "jpeg: SOS before the frame header");
            if (n < 1 || n < 4 + 2 * (size_t)s[0]) return y3f_fail(Y3F_EINVAL, "jpeg: short SOS");
            const int ns = s[0];
            if (++n_sos == 1) {
                if (ns != p.ncomp) scan_ok = 0;
                for (int i = 0; i < ns && scan_ok; ++i) {
                    if (s[1 + 2 * i] != p.comp[i].id) {
                        scan_ok = 0;
                        break;
                    }
                    Comp& k = p.comp[i];
                    k.td = s[2 + 2 * i] >> 4, k.ta = s[2 + 2 * i] & 15;
                    if (k.td > 3 || k.ta > 3) return y3f_fail(Y3F_EINVAL, "jpeg: bad table selector in the SOS");
                    if (sof_type != 0xC0 && sof_type != 0xC1) continue;     // (other kinds use other tables)
                    if (!huff[0][k.td].defined || !huff[1][k.ta].defined)
                        return y3f_fail(Y3F_EINVAL, "jpeg: component %d uses a Huffman table that is not defined", i);
                    if (!qdef[k.tq]) return y3f_fail(Y3F_EINVAL, "jpeg: component %d uses a quantisation table that is not defined", i);
                }
                const uint8_t* t = s + 1 + 2 * ns;
                if (t[0] != 0 || t[1] != 63 || t[2] != 0) scan_ok = 0;
                memcpy(p.huff, huff, sizeof(huff));
                memcpy(p.quant, quant, sizeof(quant));
                p.info.restart_interval = ri;
            }
            size_t e = next;
            int expect = 0;
            for (;;) {
                const uint8_t* f = static_cast<const uint8_t*>(memchr(d + e, 0xFF, len - e));
                if (!f || (size_t)(f - d) + 1 >= len) return y3f_fail(Y3F_EINVAL, "jpeg: truncated entropy-coded data (no EOI)");
                e = (size_t)(f - d);
                const int b = d[e + 1];
                if (b == 0x00) {
                    e += 2;
                } else if (b >= 0xD0 && b <= 0xD7) {
                    if (n_sos == 1) {
                        if (b - 0xD0 != (expect & 7)) scan_ok = 2;
                        ++expect, ++p.n_rst;
                    }
                    e += 2;
                } else if (b == 0xFF) {
                    e += 1;                             // fill byte before a marker
                } else {
                    break;
                }
            }
            if (n_sos == 1) p.scan_begin = next, p.scan_end = e;
            next = e;
        }
        pos = next;
    }
    if (!sof) return y3f_fail(Y3F_EINVAL, "jpeg: no frame header");
    if (!n_sos) return y3f_fail(Y3F_EINVAL, "jpeg: no SOS");
    if (sof_type == 0xC0 || sof_type == 0xC1) {     // the checks that only matter for a stream the device might take
        if (n_sos > 1 || scan_ok == 0) unsupported(p, Y3J_SCANS);
        if (p.ncomp == 3) {
            if ((adobe && adobe_transform != 1) ||
                (!jfif && !adobe && p.comp[0].id == 'R' && p.comp[1].id == 'G' && p.comp[2].id == 'B'))
                unsupported(p, Y3J_COLOUR);
            const int h = p.comp[0].h, v = p.comp[0].v;
            const bool ok = (h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2);
            for (int c = 1; c < 3; ++c)
                if (p.comp[c].h != 1 || p.comp[c].v != 1) unsupported(p, Y3J_SAMPLING);
            if (!ok) unsupported(p, Y3J_SAMPLING);
        } else if (p.ncomp != 1) {
            unsupported(p, Y3J_COLOUR);
        }
        if (p.info.supported) {
            const int hm = p.ncomp == 3 ? p.comp[0].h : 1, vm = p.ncomp == 3 ? p.comp[0].v : 1;
            const long long mcus = (long long)((p.info.width + 8 * hm - 1) / (8 * hm)) * ((p.info.height + 8 * vm - 1) / (8 * vm));
            if (scan_ok == 2 || (ri ? (mcus + ri - 1) / ri - 1 != p.n_rst : p.n_rst != 0)) unsupported(p, Y3J_RESTART);
        }
        if (p.info.supported)                        // a corrupt table is an error even where libjpeg would only warn
            for (int c = 0; c < p.ncomp; ++c) {
                y3j_huff t;
                if (derive(p.huff[0][p.comp[c].td], true, t) || derive(p.huff[1][p.comp[c].ta], false, t)) return Y3F_EINVAL;
            }
    }
    return Y3F_OK;
}

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// one planned image: its record (offsets relative to the image's own sections until the layout pass) and its payloads
struct Plan {
    y3j_rec rec{};
    std::vector<y3j_huff> tables;
    uint16_t quant[3][64];
    std::vector<uint8_t> data;
    std::vector<uint32_t> seg, chunks;
    size_t blob_bytes = 0, scratch_bytes = 0;
};

int plan_one(const uint8_t* d, size_t len, Plan& pl) {
    Parsed p;
    const int rc = parse(d, len, p);
    if (rc) return rc;
    if (!p.info.supported) return y3f_fail(Y3F_EINVAL, "jpeg: stream not supported by the device decoder (reason %d)", p.info.reason);
    y3j_rec& r = pl.rec;
    const int W = p.info.width, H = p.info.height, nc = p.ncomp;
    r.width = W, r.height = H, r.components = nc;
    r.hmax = nc == 3 ? p.comp[0].h : 1, r.vmax = nc == 3 ? p.comp[0].v : 1;
    r.mcus_x = (W + 8 * r.hmax - 1) / (8 * r.hmax), r.mcus_y = (H + 8 * r.vmax - 1) / (8 * r.vmax);
    r.restart_interval = p.info.restart_interval;
    // every block count and byte offset below stays far inside int32 (plane bytes = 64 x blocks <= 2^30)
    const long long bpm_hint = nc == 3 ? (long long)r.hmax * r.vmax + 2 : 1;
    if ((long long)r.mcus_x * r.mcus_y * bpm_hint > kMaxBlocks) return y3f_fail(Y3F_EINVAL, "jpeg: image too large");
    int bpm = 0, blocks = 0, plane = 0;
    for (int c = 0; c < nc; ++c) {
        const int hc = nc == 3 ? p.comp[c].h : 1, vc = nc == 3 ? p.comp[c].v : 1;
        r.comp_bw[c] = r.mcus_x * hc, r.comp_bh[c] = r.mcus_y * vc;
        r.comp_dw[c] = (W * hc + r.hmax - 1) / r.hmax, r.comp_dh[c] = (H * vc + r.vmax - 1) / r.vmax;
        r.comp_block0[c] = blocks, r.comp_plane0[c] = plane;
        blocks += r.comp_bw[c] * r.comp_bh[c];
        plane += 64 * r.comp_bw[c] * r.comp_bh[c];
        for (int dy = 0; dy < vc; ++dy)
            for (int dx = 0; dx < hc; ++dx) r.blk_comp[bpm] = (int8_t)c, r.blk_dx[bpm] = (int8_t)dx, r.blk_dy[bpm++] = (int8_t)dy;
        // the tables this component uses, each once
        for (int cls = 0; cls < 2; ++cls) {
            const int id = cls ? p.comp[c].ta : p.comp[c].td;
            int found = -1;
            for (int o = 0; o < c && found < 0; ++o) {
                const int oid = cls ? p.comp[o].ta : p.comp[o].td;
                if (oid == id) found = cls ? r.comp_ac[o] : r.comp_dc[o];
            }
            if (found < 0) {
                found = (int)pl.tables.size();
                pl.tables.emplace_back();
                if (derive(p.huff[cls][id], cls == 0, pl.tables.back())) return Y3F_EINVAL;
            }
            (cls ? r.comp_ac : r.comp_dc)[c] = found;
        }
        memcpy(pl.quant[c], p.quant[p.comp[c].tq], 128);
    }
    r.blocks_per_mcu = bpm, r.total_blocks = blocks, r.n_tables = (int)pl.tables.size();
    // the entropy-coded data without stuffing; a new interval at every RST marker
    const uint8_t* s = d + p.scan_begin;
    const size_t n = p.scan_end - p.scan_begin;
    pl.data.resize(n);
    size_t o = 0;
    pl.seg.push_back(0);
    for (size_t i = 0; i < n;) {
        const uint8_t* f = static_cast<const uint8_t*>(memchr(s + i, 0xFF, n - i));
        const size_t j = f ? (size_t)(f - s) : n;
        memcpy(pl.data.data() + o, s + i, j - i);
        o += j - i;
        if (j >= n) break;
        const int b = j + 1 < n ? s[j + 1] : -1;
        if (b == 0x00) pl.data[o++] = 0xFF, i = j + 2;
        else if (b >= 0xD0 && b <= 0xD7) pl.seg.push_back((uint32_t)(o * 8)), i = j + 2;
        else i = j + 1;
    }
    pl.data.resize(o);
    if (o > 0x1FFFFFFF) return y3f_fail(Y3F_EINVAL, "jpeg: entropy-coded data too large");
    pl.seg.push_back((uint32_t)(o * 8));
    r.n_seg = (int)pl.seg.size() - 1;
    r.data_bytes = o;
    const uint32_t S = std::max(kMinChunkBits, (uint32_t)((o * 8 + kTargetChunks - 1) / kTargetChunks + 31) & ~31u);
    for (int k = 0; k < r.n_seg; ++k) {
        const uint32_t a = pl.seg[k], b = pl.seg[k + 1];
        const uint32_t nch = std::max(1u, (b - a + S - 1) / S);
        for (uint32_t j = 0; j < nch; ++j)
            pl.chunks.insert(pl.chunks.end(), {a + j * S, j + 1 == nch ? b : a + (j + 1) * S, (uint32_t)k});
    }
    r.n_chunk = (int)(pl.chunks.size() / 3);
    // offsets within the image's own sections (the layout pass adds the bases)
    size_t at = 0;
    r.tables_off = at, at = align16(at + pl.tables.size() * sizeof(y3j_huff));
    r.quant_off = at, at = align16(at + 128 * (size_t)nc);
    r.seg_off = at, at = align16(at + 4 * pl.seg.size());
    r.chunk_off = at, at = align16(at + 4 * pl.chunks.size());
    r.data_off = at, at = align16(at + o);
    pl.blob_bytes = at;
    at = 0;
    r.coef_off = at, at = align256(at + 128 * (size_t)blocks);
    r.plane_off = at, at = align256(at + (size_t)plane);
    r.state_off = at, at = align256(at + 20 * (size_t)r.n_chunk);
    pl.scratch_bytes = at;
    return Y3F_OK;
}

template <typename F>
void parallel_jobs(int n, int threads, F work) {
    int workers = threads > 0 ? threads : std::min(kMaxThreads, (int)std::thread::hardware_concurrency());
    workers = std::max(1, std::min(workers, n));
    std::atomic<int> next(0);
    auto loop = [&]() {
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) work(i);
    };
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < workers; ++t) pool.emplace_back(loop);
    } catch (...) {      // fewer threads than asked for: the caller's thread takes what is left
    }
    loop();
    for (auto& t : pool) t.join();
}

}  // namespace

extern "C" {

int y3f_jpeg_inspect(const uint8_t* data, size_t len, y3f_jpeg_info* info) {
    if (!info) return y3f_fail(Y3F_EINVAL, "jpeg_inspect: null info");
    try {
        Parsed p;
        const int rc = parse(data, len, p);
        *info = p.info;
        return rc;
    } catch (const std::bad_alloc&) {
        return y3f_fail(Y3F_ENOMEM, "jpeg_inspect: out of memory");
    }
}

int y3f_jpeg_plan(const uint8_t* const* data, const size_t* lens, int n, uint8_t* blob, size_t capacity, size_t* blob_bytes,
                  size_t* scratch_bytes, size_t* out_bytes, int threads) {
    if (n < 0 || (n && (!data || !lens)) || !blob_bytes || !scratch_bytes || !out_bytes)
        return y3f_fail(Y3F_EINVAL, "jpeg_plan: bad arguments");
    try {
        std::vector<Plan> plans((size_t)n);
        std::vector<int> rcs((size_t)n, 0);
        std::vector<std::string> errors((size_t)n);
        parallel_jobs(n, threads, [&](int i) {
            rcs[i] = plan_one(data[i], lens[i], plans[i]);
            if (rcs[i]) errors[i] = y3f_last_error();
        });
        for (int i = 0; i < n; ++i)
            if (rcs[i]) return y3f_fail(rcs[i], "image %d: %s", i, errors[i].c_str());
        // the scratch starts with the device copy of the records, which y3_jpeg_decode uploads from the ones it checked
        size_t b = align16((size_t)n * sizeof(y3j_rec)), sc = align256((size_t)n * sizeof(y3j_rec)), out = 0;
        for (auto& pl : plans) {
            y3j_rec& r = pl.rec;
            r.tables_off += b, r.quant_off += b, r.seg_off += b, r.chunk_off += b, r.data_off += b;
            b += pl.blob_bytes;
            r.coef_off += sc, r.plane_off += sc, r.state_off += sc;
            sc += pl.scratch_bytes;
            r.out_off = out;
            out = align256(out + 3 * (size_t)r.width * r.height);
        }
        *blob_bytes = b, *scratch_bytes = sc, *out_bytes = out;
        if (!blob || capacity < b) return Y3F_OK;
        parallel_jobs(n, threads, [&](int i) {
            const Plan& pl = plans[i];
            const y3j_rec& r = pl.rec;
            memcpy(blob + (size_t)i * sizeof(y3j_rec), &r, sizeof(r));
            memcpy(blob + r.tables_off, pl.tables.data(), pl.tables.size() * sizeof(y3j_huff));
            memcpy(blob + r.quant_off, pl.quant, 128 * (size_t)r.components);
            memcpy(blob + r.seg_off, pl.seg.data(), 4 * pl.seg.size());
            memcpy(blob + r.chunk_off, pl.chunks.data(), 4 * pl.chunks.size());
            memcpy(blob + r.data_off, pl.data.data(), pl.data.size());
        });
        return Y3F_OK;
    } catch (const std::bad_alloc&) {
        return y3f_fail(Y3F_ENOMEM, "jpeg_plan: out of memory");
    }
}

}  // extern "C"
