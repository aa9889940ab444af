// Host half shared by the two implicit-GEMM fp32 conv kernels (the exact kernel of y3_conv.hip, the split-plane kernel of
// y3_conv_split.hip): the descriptor check, the ConvArgs builder, the image-range walker and the launch ladder.  A kernel
// family describes itself with a traits type F:
//     F::KDIV                 Cin (and c_up) must divide by it: the kernel's K-step
//     F::FORMS                whether the STATS / BSTATS / TMODE instantiations exist
//     F::TILE_64              whether the 64x64 tile is instantiated
//     F::tile(ks, tmode, cout)  the family's tile table: THE place that says which tile a shape runs on.  The launch below
//                             switches on it, and the row-block counts of the statistics outputs derive from it.
//     F::grid(tile, tiles)    workgroups of a data-parallel launch over `tiles` tiles
//     F::launch<BM, BN, WGM, WGN, KS, UPCAT, STREAMK, TMODE, STATS, BSTATS>(stream, grid, args)
#pragma once
#include "y3_conv_common.h"

namespace y3conv {

// Every check of a forward conv's descriptor that does not depend on the kernel's tile.  (The Cin = 3 stem has no K-step: the
// exact kernel's launcher checks its one shape.)
inline int check_conv_desc(const y3_conv_desc* d, const void* x_up, const char* who, int kdiv) {
    Y3_CHECK_ARG(d->k == 1 || d->k == 3, "%s: kernel_size must be 1 or 3 (got %d)", who, d->k);
    Y3_CHECK_ARG(d->stride == 1 || d->stride == 2, "%s: stride must be 1 or 2 (got %d)", who, d->stride);
    Y3_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->cin > 0 && d->cout > 0, "%s: non-positive dimension", who);
    Y3_CHECK_ARG(!(d->stride == 2 && (d->h % 2 || d->w % 2)), "%s: stride-2 conv needs even H,W (got %dx%d)", who,
                 d->h, d->w);
    Y3_CHECK_ARG((x_up != nullptr) == (d->c_up > 0), "%s: x_up and c_up must agree", who);
    if (d->cin == 3) return Y3_OK;
    Y3_CHECK_ARG(d->cin % kdiv == 0, "%s: Cin must be 3 or a multiple of %d (got %d)", who, kdiv, d->cin);
    if (x_up) {
        Y3_CHECK_ARG(d->k == 1 && d->stride == 1, "%s: fused upsample+concat needs a 1x1 s1 conv", who);
        Y3_CHECK_ARG(d->c_up % kdiv == 0 && d->c_up < d->cin && d->h % 2 == 0 && d->w % 2 == 0,
                     "%s: bad c_up=%d for cin=%d", who, d->c_up, d->cin);
    }
    Y3_CHECK_ARG(!(d->k == 1 && d->stride != 1), "%s: 1x1 conv must have stride 1", who);
    return Y3_OK;      // (the element limit: the image ranges)
}

// The argument block of conv `d` over the whole batch: value-initialised, then what the descriptor and the tensors say.  The
// rows (N, M) are set per image range by walk_image_ranges; what a form adds (stats, bz / bvec, wrev, tmode) by its entry point.
inline ConvArgs conv_args(const y3_conv_desc* d, const float* x, const float* x_up, const void* w, const float* scale,
                          const float* shift, const float* resid, float* y) {
    ConvArgs a{};
    a.x = x; a.xu = x_up; a.w = static_cast<const float*>(w); a.scale = scale; a.shift = shift; a.resid = resid; a.y = y;
    a.N = d->n; a.H = d->h; a.W = d->w; a.Cin = d->cin; a.Cu = d->c_up; a.Cx = d->cin - d->c_up;
    a.Cout = d->cout; a.stride = d->stride; a.pad = d->k / 2; a.act = d->act;
    a.Ho = d->h / d->stride; a.Wo = d->w / d->stride;
    return a;
}

// Row blocks of `bm` rows over the image ranges of a launch with `rows_img` GEMM rows per image: every range starts a row
// block of its own, its blocks behind the previous range's.  (rg.n < 0, one image over the limit: 0, no such launch.)
inline int range_row_blocks(const y3_image_ranges& rg, long long rows_img, int bm) {
    long long nb = 0;
    for (int i = 0; i < rg.n; ++i) nb += (rg.count[i] * rows_img + bm - 1) / bm;
    return (int)nb;
}

// A launch over its image ranges (a tensor of 2^29 elements or more runs as the same launch per range of whole
// images).  `a` describes the whole batch; launch(r, whole) gets the block of one range:
//   * every tensor pointer advanced by whole images - x, the fused upsample input, the residual, y and (BSTATS) z;
//   * the statistics rows of a range behind the previous range's, in row blocks of `stats_bm` rows (range_row_blocks);
//   * whole = the launch is not cut.  Only then may it take the workspace, and with it the stream-K schedule: one set of flag
//     words and accumulator slots serves one launch, so no range takes stream-K and none reads y3_sk_opts::flags.
template <class Launch>
int walk_image_ranges(const y3_image_ranges& rg, const ConvArgs& a, int stats_bm, Launch&& launch) {
    if (rg.n < 0) return rg.n;
    // GEMM rows and output pixels of one image (tmode: rows = the coarse grid, one parity class of the 2x finer output)
    const size_t rows = a.tmode ? (size_t)a.H * a.W : (size_t)a.Ho * a.Wo, out = (a.tmode ? 4 * rows : rows) * a.Cout;
    float* stats = a.stats;
    for (int i = 0; i < rg.n; ++i) {
        const size_t b = (size_t)rg.begin[i];
        ConvArgs r = a;
        r.N = rg.count[i];
        r.M = (int)(rg.count[i] * rows);
        r.x += b * a.H * a.W * a.Cx;
        if (a.xu) r.xu += b * (a.H / 2) * (a.W / 2) * a.Cu;
        if (a.resid) r.resid += b * out;
        r.y += b * out;
        if (a.bz) r.bz += b * out;
        r.stats = stats;
        if (int rc = launch(r, rg.n == 1)) return rc;
        if (stats) stats += (size_t)((r.M + stats_bm - 1) / stats_bm) * 2 * a.Cout;
    }
    return Y3_OK;
}

// One workgroup per tile of the family's table (or F::grid's walk of them)
template <class F, int KS, bool UPCAT, bool TMODE = false, bool STATS = false, bool BSTATS = false>
int launch_tiles(hipStream_t stream, const ConvArgs& a) {
    static_assert(!BSTATS || KS == 1, "the fused BN backward reduction exists on the tiles of the 1x1 data gradient only");
    const Tile t = F::tile(KS, TMODE, a.Cout);
    const int grid = F::grid(t, tile_count(t, a.M, a.Cout));
    if (t.bm == 128 && t.bn == 32) return F::template launch<128, 32, 4, 1, KS, UPCAT, false, TMODE, STATS, BSTATS>(stream, grid, a);
    if (t.bm == 128 && t.bn == 64) return F::template launch<128, 64, 4, 1, KS, UPCAT, false, TMODE, STATS, BSTATS>(stream, grid, a);
    if constexpr (F::TILE_64) {
        if (t.bm == 64 && t.bn == 64) return F::template launch<64, 64, 2, 2, KS, UPCAT, false, TMODE, STATS, BSTATS>(stream, grid, a);
    }
    Y3_CHECK_ARG(t.bm == 128 && t.bn == 128, "conv launch: the tile table names a %dx%d tile that is not instantiated", t.bm, t.bn);
    return F::template launch<128, 128, 2, 2, KS, UPCAT, false, TMODE, STATS, BSTATS>(stream, grid, a);
}

template <class F, bool TMODE = false, bool STATS = false>
int launch_streamk(hipStream_t stream, const ConvArgs& a) {
    return F::template launch<SK_TILE.bm, SK_TILE.bn, SK_TILE.wgm, SK_TILE.wgn, 3, false, true, TMODE, STATS, false>(stream, a.workers, a);
}

// One launch (not cut, or one image range) of a k x k conv on family F: the fused upsample input and the 1x1 convs on the tile
// ladder, a 3x3 conv on stream-K where use_streamk says so (it needs the workspace) and on the ladder otherwise.
template <class F>
int launch_conv_family(hipStream_t stream, ConvArgs& a, int k, void* workspace, size_t workspace_bytes, const y3_sk_opts* sk) {
    if (a.xu) return launch_tiles<F, 1, true>(stream, a);
    if (k == 1) {
        if constexpr (F::FORMS) {
            // (a data gradient whose output is the dy of a BN layer: its backward reduction rides in the epilogue)
            if (a.bz) return launch_tiles<F, 1, false, false, false, true>(stream, a);
            if (a.stats) return launch_tiles<F, 1, false, false, true>(stream, a);
        }
        return launch_tiles<F, 1, false>(stream, a);
    }
    const bool has_ws = workspace != nullptr && workspace_bytes >= SK_WORKSPACE_BYTES && ((uintptr_t)workspace & 15) == 0;
    if constexpr (F::FORMS) {
        if (a.tmode) {
            // four output parity classes, each a dense conv over the coarse grid's rows with 1/2/2/4 taps
            for (int cls = 0; cls < 4; ++cls) {
                a.cy = cls >> 1; a.cx = cls & 1;
                a.ntaps = (a.cy ? 2 : 1) * (a.cx ? 2 : 1);
                a.partial = nullptr; a.workers = 0;
                int rc;
                if (use_streamk(a.M, a.Cin, a.Cout, a.ntaps, has_ws)) {
                    // (the four parity-class launches share the workspace's own flag words: zeroed ahead of each)
                    y3_sk_opts o;
                    o.err = sk ? sk->err : nullptr;
                    rc = sk_prepare(stream, a, workspace, &o);
                    if (rc == Y3_OK) rc = launch_streamk<F, true>(stream, a);
                } else {
                    rc = launch_tiles<F, 3, false, true>(stream, a);
                }
                if (rc != Y3_OK) return rc;
            }
            return Y3_OK;
        }
    }
    if (use_streamk(a.M, a.Cin, a.Cout, 9, has_ws)) {
        if (int rc = sk_prepare(stream, a, workspace, sk)) return rc;
        if constexpr (F::FORMS) {
            if (a.stats) return launch_streamk<F, false, true>(stream, a);
        }
        return launch_streamk<F>(stream, a);
    }
    if constexpr (F::FORMS) {
        if (a.stats) return launch_tiles<F, 3, false, false, true>(stream, a);
    }
    return launch_tiles<F, 3, false>(stream, a);
}

}  // namespace y3conv
