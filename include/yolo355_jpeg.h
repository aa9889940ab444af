/* yolo355_jpeg.h - the feeder's JPEG decoder: host half in liby3feed.so, device half (y3_jpeg_decode) in libyolo355.so.
 *
 * The host does what is O(file bytes): it parses the markers, builds the Huffman decode tables, removes the byte stuffing
 * and the restart markers, and lays n files out as ONE relocatable blob (y3f_jpeg_plan), the way y3f_plan_batch does for
 * the pixel work.  The device does the rest (csrc/y3_jpeg.hip, arithmetic in csrc/y3_jpeg_px.h): self-synchronising
 * parallel Huffman decoding, the DC prediction, libjpeg's islow IDCT, its fancy upsampling and its YCbCr -> RGB tables.
 * The result is byte-identical to Pillow's `np.asarray(Image.open(f).convert('RGB'))` (tests/test_jpeg_cpu.py,
 * tests/test_jpeg_gpu.py).
 *
 * Supported: baseline and extended-sequential Huffman (SOF0, SOF1), 8-bit, one scan holding every component; one
 * component (grayscale, replicated to RGB) or three (YCbCr) sampled 4:4:4, 4:2:2 (h2v1) or 4:2:0 (h2v2); any restart
 * interval.  Everything else is reported unsupported by y3f_jpeg_inspect, and the caller decodes it as before.
 * Functions return Y3F_OK or a negative Y3F_E* code (include/yolo355_feed.h); y3f_last_error() has the message.
 */
#ifndef YOLO355_JPEG_H
#define YOLO355_JPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* y3f_jpeg_info.reason when supported == 0 */
#define Y3J_OK 0
#define Y3J_PROGRESSIVE 1       /* SOF2 / SOF6 */
#define Y3J_ARITHMETIC 2        /* SOF9..SOF15 */
#define Y3J_LOSSLESS 3          /* SOF3 / SOF7 / hierarchical (DHP, SOF5) */
#define Y3J_PRECISION 4         /* not 8-bit samples */
#define Y3J_COLOUR 5            /* not 1 or 3 components, an Adobe transform other than YCbCr, or RGB component ids */
#define Y3J_SAMPLING 6          /* three components, not 4:4:4, 4:2:2 (h2v1) or 4:2:0 (h2v2) */
#define Y3J_SCANS 7             /* more than one scan, or a scan without every component */
#define Y3J_RESTART 8           /* restart markers that do not follow the interval */
#define Y3J_SIZE 9              /* height 0 (DNL) or an image too large for the device records */

typedef struct y3f_jpeg_info {
    int32_t width, height, components;
    int32_t h_samp, v_samp;     /* the luma sampling factors: 1,1 (4:4:4 or grayscale), 2,1 (4:2:2), 2,2 (4:2:0) */
    int32_t supported;          /* 1: y3f_jpeg_plan takes it */
    int32_t reason;             /* Y3J_* when supported == 0 */
    int32_t restart_interval;   /* MCUs, 0: none */
} y3f_jpeg_info;

/* Parses the headers of one file (and walks its entropy-coded data to the EOI).  Never reads past len.  A stream that is
 * not a JPEG, or is truncated, lacks a table, an SOS or the EOI, returns Y3F_EINVAL; a well-formed stream of a kind the
 * device does not decode returns Y3F_OK with supported = 0 and a reason. */
int y3f_jpeg_inspect(const uint8_t* data, size_t len, y3f_jpeg_info* info);

/* One Huffman table as the device reads it (jdhuff's derived table with a 9-bit look-ahead). */
#define Y3J_LOOKAHEAD 9
typedef struct y3j_huff {
    uint16_t look[1 << Y3J_LOOKAHEAD];  /* (code length << 8) | symbol for codes of <= 9 bits, 0: longer */
    int32_t maxcode[18];                /* largest code of each length, -1: none; [17] sentinel */
    int32_t valoffset[18];              /* symbol index = code + valoffset[length] */
    uint8_t huffval[256];
} y3j_huff;                             /* 1424 bytes */

/* One planned image.  Offsets: bytes from the start of the blob (tables, quant, data, seg, chunk), of the device scratch
 * (coef, plane, state) or of the output buffer (out).  Blocks of a component are stored plane by plane, row-major in
 * block units (comp_bw x comp_bh blocks); "decode order" is the order of the blocks in the scan. */
typedef struct y3j_rec {
    uint64_t tables_off;        /* n_tables y3j_huff */
    uint64_t quant_off;         /* components x 64 uint16, natural order */
    uint64_t data_off;          /* entropy-coded bytes, stuffing and restart markers removed */
    uint64_t seg_off;           /* n_seg + 1 uint32: bit offset at which each restart interval starts, then the end */
    uint64_t chunk_off;         /* n_chunk x uint32[3]: first bit, end bit, segment */
    uint64_t coef_off;          /* int16 [blocks][64] */
    uint64_t plane_off;         /* uint8 sample planes, comp_bw * 8 wide, comp_bh * 8 high */
    uint64_t state_off;         /* int32 [5][n_chunk]: start position, start (z | block << 8), exit position, exit state,
                                   blocks completed */
    uint64_t out_off;           /* uint8 [height][width][3] */
    uint64_t data_bytes;
    int32_t width, height, components, n_tables;
    int32_t hmax, vmax, mcus_x, mcus_y;
    int32_t blocks_per_mcu, restart_interval, n_seg, n_chunk;
    int32_t total_blocks;       /* mcus_x * mcus_y * blocks_per_mcu */
    int32_t comp_bw[3], comp_bh[3];         /* plane size in blocks */
    int32_t comp_dw[3], comp_dh[3];         /* downsampled size in samples (libjpeg's downsampled_width / _height) */
    int32_t comp_block0[3];                 /* first block of the component in coef */
    int32_t comp_plane0[3];                 /* byte offset of the component's plane from plane_off */
    int32_t comp_dc[3], comp_ac[3];         /* index into the image's tables */
    int8_t blk_comp[10], blk_dx[10], blk_dy[10];    /* per block of an MCU: component, block column / row in the MCU */
    int8_t pad[2];
    int32_t reserved[3];
} y3j_rec;                      /* 272 bytes */

/* Plans n supported files (data[i], lens[i]) into one blob: the n y3j_rec first, then each image's tables and data.
 * Always sets *blob_bytes, *scratch_bytes (device scratch) and *out_bytes (the packed RGB outputs); writes the blob only
 * when `blob` is not NULL and `capacity` suffices, on up to `threads` threads of the library's own (0: the hardware's, at
 * most 8).  The scratch begins with room for the n records (n * 272 bytes, rounded up to 256): y3_jpeg_decode copies the
 * records it has checked there, and the kernels read them from that copy.
 * A file that y3f_jpeg_inspect rejects or reports unsupported fails the call with the index of the file. */
int y3f_jpeg_plan(const uint8_t* const* data, const size_t* lens, int n, uint8_t* blob, size_t capacity,
                  size_t* blob_bytes, size_t* scratch_bytes, size_t* out_bytes, int threads);

#ifdef __cplusplus
}
#endif
#endif
