// Test infrastructure: the device functions of the JPEG decoder (yolov3_tensorflow_amd/csrc/y3_jpeg_px.h) run on the HOST
// in the order y3_jpeg_decode's kernels run them - the same chunks, the same guessed start states, the same synchronisation
// rounds - so that the planner (y3f_jpeg_plan) and the arithmetic can be compared with Pillow without a GPU
// (tests/test_jpeg_cpu.py builds this file with g++, once more under -fsanitize=address).  The workgroup's prefix sums are
// plain serial sums here: they give the same numbers.  Never part of the product.
#include <cstring>
#include <vector>
#include "../yolov3_tensorflow_amd/csrc/y3_jpeg_px.h"

// status: n x 2 int32 (status bits, synchronisation rounds), as y3_jpeg_decode writes it.  Returns -1 if a record does not
// pass the host check the device entry point makes.
extern "C" int y3j_emulate(const uint8_t* blob, size_t blob_bytes, int n, uint8_t* scratch, size_t scratch_bytes, uint8_t* out,
                           size_t out_bytes, int32_t* status) {
    // as y3_jpeg_decode: the records are copied to the head of the scratch, checked there, and read from there
    const size_t head = ((size_t)n * sizeof(y3j_rec) + 255) & ~(size_t)255;
    if ((size_t)n * sizeof(y3j_rec) > blob_bytes || head > scratch_bytes) return -1;
    memcpy(scratch, blob, (size_t)n * sizeof(y3j_rec));
    const y3j_rec* recs = reinterpret_cast<const y3j_rec*>(scratch);
    for (int i = 0; i < n; ++i)
        if (!y3jpx::rec_check(recs[i], blob_bytes, scratch_bytes, out_bytes, head)) return -1;
    for (int i = 0; i < n; ++i) {
        const y3j_rec& r = recs[i];
        std::vector<y3j_huff> tabs((size_t)r.n_tables);
        memcpy(tabs.data(), blob + r.tables_off, tabs.size() * sizeof(y3j_huff));
        memset(scratch + r.coef_off, 0, 128 * (size_t)r.total_blocks);
        for (int c = 0; c < r.n_chunk; ++c) y3jpx::chunk_init(r, blob, scratch, c);
        int bad = 0, rounds = 0;
        for (;;) {
            for (int c = 0; c < r.n_chunk; ++c) y3jpx::chunk_sync(r, blob, scratch, tabs.data(), c);
            bool changed = false;
            for (int c = 0; c < r.n_chunk; ++c) changed |= y3jpx::chunk_adopt(r, blob, scratch, c);
            ++rounds;
            if (!changed) break;
            if (rounds > r.n_chunk + 1) {
                bad |= y3jpx::kNoSync;
                break;
            }
        }
        int32_t* count = y3jpx::state_row(r, scratch, 4);
        int carry = 0;
        for (int c = 0; c < r.n_chunk; ++c) {
            const uint32_t seg = y3jpx::chunk_of(r, blob, c).seg;
            if (c == 0 || seg != y3jpx::chunk_of(r, blob, c - 1).seg) carry = 0;
            const int k = count[c];
            count[c] = y3jpx::seg_block0(r, seg) + carry;
            carry += k;
        }
        for (int c = 0; c < r.n_chunk; ++c) bad |= y3jpx::chunk_write(r, blob, scratch, tabs.data(), c, count[c]);
        int16_t* coef = reinterpret_cast<int16_t*>(scratch + r.coef_off);
        const int seg_blocks = r.restart_interval ? r.restart_interval * r.blocks_per_mcu : r.total_blocks;
        int s[3] = {0, 0, 0};
        for (int g = 0; g < r.total_blocks; ++g) {
            if (g % seg_blocks == 0) s[0] = s[1] = s[2] = 0;
            const int c = r.blk_comp[g % r.blocks_per_mcu];
            int16_t& dc = coef[(size_t)y3jpx::block_addr(r, g) * 64];
            s[c] = (int)((unsigned)s[c] + (unsigned)dc);
            dc = (int16_t)s[c];
        }
        status[2 * i] = bad, status[2 * i + 1] = rounds;
        for (int k = 0; k < r.total_blocks; ++k) y3jpx::idct_block(r, blob, scratch, k);
        for (long long p = 0; p < (long long)r.width * r.height; ++p)
            y3jpx::rgb_pixel(r, scratch + r.plane_off, (int)(p % r.width), (int)(p / r.width), out + r.out_off + 3 * p);
    }
    return 0;
}

#ifdef Y3J_EMUL_MAIN
// the sanitizer build: jpeg_emul <blob file> <n> <scratch bytes> <out bytes>; every buffer exactly as large as the plan says,
// so that a read or write past an extent is reported.  Prints the n status words.
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    if (argc != 5) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + k);
    fclose(f);
    const int n = atoi(argv[2]);
    const size_t sb = strtoull(argv[3], nullptr, 10), ob = strtoull(argv[4], nullptr, 10);
    uint8_t* blob = new uint8_t[file.size()];
    memcpy(blob, file.data(), file.size());
    uint8_t* scratch = new uint8_t[sb];
    uint8_t* out = new uint8_t[ob];
    memset(scratch, 0xA5, sb);
    std::vector<int32_t> status(2 * (size_t)n, 0);
    const int rc = y3j_emulate(blob, file.size(), n, scratch, sb, out, ob, status.data());
    for (int i = 0; i < n; ++i) printf("%d\n", status[2 * i]);
    delete[] blob;
    delete[] scratch;
    delete[] out;
    return rc ? 3 : 0;
}
#endif
