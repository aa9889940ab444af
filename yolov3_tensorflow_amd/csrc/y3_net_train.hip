// The train step of train.py:72-115 behind ONE C entry (SURVEY.md §8b asks for whole-graph entries; VERDICT r2 missing #4):
//   y3_net_train_forward   yolov3.forward(inputs, is_training=True)        model.py:30-80 with batch-statistics BN
//   y3_net_train_loss      yolov3.compute_loss(y_pred, y_true)             model.py:192-365
//   y3_net_train_backward  optimizer.compute_gradients(loss[0] + l2_loss)  train.py:112 (the L2 term, the clip and the
//                                                                          update are y3_clip_update_multi's)
//   y3_net_train_step      the three in one call
// Host code only: it sequences the per-op entry points of include/yolo355.h over a caller-owned workspace, exactly the
// calls yolov3_tensorflow_amd/training.py used to make from Python (with torch.empty as the allocator).  Every buffer lives
// in the workspace: the forward's saved tensors are bump-allocated and stay until the next forward; everything else
// (packed kernels, the materialised concat's parts, gradients of activations) comes from a first-fit free list and is
// recycled as soon as its last consumer has been LAUNCHED - all launches go to the context's one stream, so launch order is
// execution order.  y3_net_train_workspace_bytes runs the same allocation sequence without launching anything.
// Each pass is one object (Forward, Backward): its per-layer body is a list of named steps over that pass's context.
#include <cstring>
#include <vector>
#include <algorithm>
#include "y3_net.h"

namespace {

constexpr float BN_EPS = 1e-5f;      // model.py:37
// (the ones / zeros vectors and the per-channel scratch take the graph's own widest channel count, y3_net::max_channels)
constexpr int BN_MAXC = 1024;        // widest batch-norm layer of either architecture (the exchange buffer of y3_net_train_set_bn_sync)
// Rows of y3_bias_grad's partial sums as `bias_sc` is sized; the [det_pad] result sits behind them.  The reduction itself
// uses at most RED_BLOCKS = 512 rows (y3_train.hip): a kept over-allocation, the workspace size is pinned
// (tests/golden/conv_routes.json).
constexpr int BIAS_SC_ROWS = 1024;

__global__ void loss_total_kernel(const float* __restrict__ loss4, float* __restrict__ loss5) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        // model.py:364: total = xy + wh + conf + class, summed in this order
        loss5[0] = loss4[0] + loss4[1] + loss4[2] + loss4[3];
        loss5[1] = loss4[0]; loss5[2] = loss4[1]; loss5[3] = loss4[2]; loss5[4] = loss4[3];
    }
}

}  // namespace

struct y3_train_state {
    Arena arena;
    int n = 0, h = 0, w = 0;
    const float* x = nullptr;
    bool have_fwd = false, have_loss = false;
    size_t saved_top = 0;                    // arena top after forward (+ loss): backward's temporaries start here
    // persistent scratch (allocated first)
    Buf ones, zeros, sk_ws, reduce_sc, bnbwd_sc, loss_sc, bias_sc, wgrad_sc, loss4;
    std::vector<Buf> tens;                   // activation of every tensor id (0: the caller's x)
    std::vector<Buf> xin;                    // per layer: the materialised concat input (fused-upsample layers), else empty
    std::vector<Buf> z, stats;               // per BN layer: raw conv output, [4][cout] mean / inv_std / scale / shift
    struct Routes { ConvRoute fwd, dgrad, wgrad; };
    std::vector<Routes> routes;              // per layer, at the shape of the last forward (y3_route_*: what is sized is what runs)
    Buf fm_grad[3];                          // d loss / d feature_map_i, [n,g,g,det_pad]
    int fm_tensor[3] = {-1, -1, -1};         // tensor ids of feature maps 1..3 (13-, 26-, 52-grid)
    // what the second stream of backward keeps from pass to pass (WgradLane): its context and the events that order it against
    // the context's stream - "dz of this layer is ready" (main -> side), "this layer's weight gradient is done" (side -> main)
    y3_ctx* side_ctx = nullptr;
    void* side_stream = nullptr;
    static constexpr int NEV = 8;
    hipEvent_t ev_dz[NEV] = {}, ev_done[NEV] = {};
};

void y3_train_state_free(y3_train_state* s) {
    if (!s) return;
    for (int i = 0; i < y3_train_state::NEV; ++i) {
        if (s->ev_dz[i]) (void)hipEventDestroy(s->ev_dz[i]);
        if (s->ev_done[i]) (void)hipEventDestroy(s->ev_done[i]);
    }
    if (s->side_ctx) (void)y3_ctx_destroy(s->side_ctx);
    delete s;
}

namespace {

// a launch or pass call: skipped in the dry run, its failure ends the pass
#define Y3_TRY(expr)                    \
    do {                                \
        if (!dry) {                     \
            const int rc_ = (expr);     \
            if (rc_ != Y3_OK) return rc_; \
        }                               \
    } while (0)
// a step of a pass: runs in the dry run too (it allocates and releases), its failure ends the pass
#define Y3_STEP(expr)                   \
    do {                                \
        const int rc_ = (expr);         \
        if (rc_ != Y3_OK) return rc_;   \
    } while (0)

// synchronised batch norm (y3_net_train_set_bn_sync): the host hook between the two halves of a BN layer's finalize
int bn_sync_call(const y3_net* net, int layer, int phase, int cout) {
    if (net->bn_sync_fn(net->bn_sync_user, layer, phase, 2 * cout + 1) != 0) {
        y3_set_error("y3_net_train: the batch-norm exchange hook failed (layer %d, %s)", layer, phase ? "backward" : "forward");
        return Y3_ESTATE;
    }
    return Y3_OK;
}

// the channel stride of the loss gradients (the last layer is a detection conv)
int det_pad_of(const y3_net* net) { return net->dz_stride((int)net->layers.size() - 1); }

// What every pass works on: the net, its train state and arena, the caller's variable table, and whether it only sizes.
struct Pass {
    y3_net* net;
    y3_train_state& S;
    Arena& A;
    y3_ctx* ctx;                     // (the dry run of a size query may have none)
    const y3_train_var* vars;
    const bool dry;
    const int n, h, w;               // the input of the last forward
    Pass(y3_net* net_, const y3_train_var* vars_, bool dry_)
        : net(net_), S(*net_->train), A(S.arena), ctx(net_->ctx), vars(vars_), dry(dry_), n(S.n), h(S.h), w(S.w) {}
    const float* tptr(int id) const { return id == 0 ? S.x : A.p(S.tens[id]); }
    hipStream_t stream() const { return dry ? nullptr : ctx->stream; }
    template <class T> static T* at(T* p, long long k) { return p ? p + k : nullptr; }      // (the dry run's pointers are null)
    y3_sk_opts sk_opts(const ConvRoute& r) const {
        y3_sk_opts so;
        so.err = dry ? nullptr : ctx->err_host;
        so.wino44_form = r.two_pass;
        return so;
    }
};

// ---- forward ------------------------------------------------------------------------------------------------------------

// The persistent scratch, first in the arena, sized for the routes every layer takes at this shape.
void alloc_scratch(const y3_net* net, y3_train_state& S, int n, int h, int w) {
    Arena& A = S.arena;
    const size_t nl = net->layers.size();
    const int det_pad = det_pad_of(net);
    const int MAXC = net->max_channels();
    S.ones = A.alloc((size_t)MAXC * 4);
    S.zeros = A.alloc((size_t)MAXC * 4);
    size_t sk = 0, wg = 0;
    S.routes.resize(nl);
    for (size_t i = 0; i < nl; ++i) {
        S.routes[i] = {y3_route_train_fwd(*net, (int)i, n, h, w), y3_route_dgrad(*net, (int)i, n, h, w),
                       y3_route_wgrad(*net, (int)i, n, h, w)};
        sk = std::max({sk, S.routes[i].fwd.scratch, S.routes[i].dgrad.scratch});
        wg = std::max(wg, S.routes[i].wgrad.scratch);
    }
    S.sk_ws = A.alloc(std::max<size_t>(sk, 256));
    S.reduce_sc = A.alloc(y3_reduce_scratch_bytes(MAXC));
    S.bnbwd_sc = A.alloc(y3_bn_bwd_scratch_bytes(MAXC));
    size_t ls = 0;
    for (int s : {32, 16, 8}) ls = std::max(ls, y3_loss_scratch_bytes(n, h / s, w / s));
    S.loss_sc = A.alloc(ls);
    S.bias_sc = A.alloc((size_t)BIAS_SC_ROWS * det_pad * 4 + (size_t)det_pad * 4);
    S.wgrad_sc = A.alloc(std::max<size_t>(wg, 256));
    S.loss4 = A.alloc(64);
}

struct Forward : Pass {
    const y3_train_opts* o;
    Forward(y3_net* net_, const y3_train_var* vars_, const y3_train_opts* o_, bool dry_) : Pass(net_, vars_, dry_), o(o_) {}

    struct Step {                    // one layer of the pass
        int i; const Layer& l; const y3_train_var& v; y3_conv_desc d;
        bool b16, half;              // dtype 1: the bf16 kernels (every layer but the stem) / bf16 activations (all layers)
        const float* xin;            // the conv's input
        long long rows;              // of the conv's output
        int nblk = 0; Buf part;      // BN layers: rows of the column sums the conv kernel leaves in `part` (0: none)
        float* y = nullptr;          // the conv's output: z of a BN layer, a feature map
    };

    int fill_constants() {           // the ones / zeros vectors (not in the dry run)
        if (A.overflow) { y3_set_error("y3_net_train_forward: workspace too small"); return Y3_EINVAL; }
        void* stage = nullptr;
        const size_t MAXC = (size_t)net->max_channels();
        if (int rc = y3_ctx_stage_acquire(ctx, MAXC * 4, &stage)) return rc;
        for (size_t i = 0; i < MAXC; ++i) static_cast<float*>(stage)[i] = 1.f;
        Y3_CHECK_HIP(hipMemcpyAsync(A.p(S.ones), stage, MAXC * 4, hipMemcpyHostToDevice, ctx->stream));
        if (int rc = y3_ctx_stage_release(ctx)) return rc;
        Y3_CHECK_HIP(hipMemsetAsync(A.p(S.zeros), 0, MAXC * 4, ctx->stream));
        return Y3_OK;
    }

    // training materialises concat([upsample(up), route]) (model.py:61-62,71-72)
    int concat_input(Step& s) {
        const Layer& l = s.l;
        if (l.up < 0) return Y3_OK;
        const long long in_rows = (long long)n * s.d.h * s.d.w;
        const int cu = net->tensors[l.up].c, cx = net->tensors[l.src].c;
        Buf upt = s.half ? Buf() : A.alloc((size_t)in_rows * cu * 4);      // (bf16: one kernel upsamples and concatenates)
        S.xin[s.i] = A.alloc((size_t)in_rows * (cu + cx) * (s.half ? 2 : 4));
        if (s.half) {
            Y3_TRY(y3_upsample_concat_bf16(ctx, tptr(l.up), cu, s.xin, cx, n, s.d.h, s.d.w, A.p(S.xin[s.i])));
        } else {
            Y3_TRY(y3_upsample_nearest(ctx, tptr(l.up), n, s.d.h / 2, s.d.w / 2, cu, s.d.h, s.d.w, A.p(upt)));
            Y3_TRY(y3_concat_channels(ctx, A.p(upt), cu, s.xin, cx, in_rows, A.p(S.xin[s.i])));
        }
        A.release(upt);
        s.xin = A.p(S.xin[s.i]);
        return Y3_OK;
    }

    // a pool layer's input spp(src), materialised in the element type of src: the conv and its weight gradient read it as a
    // plain [rows, 4c] input, backward reads x back out of its last slot
    int pool_input(Step& s) {
        const Layer& l = s.l;
        if (!l.pool) return Y3_OK;
        const long long in_rows = (long long)n * s.d.h * s.d.w;
        S.xin[s.i] = A.alloc((size_t)in_rows * l.cin * (s.half ? 2 : 4));
        Y3_TRY(y3_spp_fwd(ctx, s.xin, s.half, n, s.d.h, s.d.w, net->tensors[l.src].c, A.p(S.xin[s.i])));
        s.xin = A.p(S.xin[s.i]);
        return Y3_OK;
    }

    // BN layers: the raw conv output z (with its column sums where the kernel has them); detection convs: bias, linear
    // (model.py:55-57)
    int conv(Step& s) {
        const Layer& l = s.l;
        const y3_conv_desc& d = s.d;
        const ConvRoute& r = S.routes[s.i].fwd;
        s.nblk = !l.bn || r.kind == RouteKind::Split ? 0
                 : s.b16 ? y3_conv_bf16_train_stats_blocks(&d)
                         : y3_conv_stats_blocks(&d, r.kind == RouteKind::Wino44 ? 2 : r.kind == RouteKind::Wino ? 1 : 0);
        s.part = s.nblk ? A.alloc((size_t)s.nblk * 2 * l.cout * 4) : Buf();
        // the kernel in this step's packing (the variable changes every step)
        const ConvPack pk = y3_conv_pack(*net, s.i, r);
        Buf wp = pk.bytes() ? A.alloc(pk.bytes()) : Buf();
        const float* wdev = s.v.weights;                    // (Hwio: the variable as it is)
        if (wp.ok()) {
            Y3_TRY(pk.launch(ctx, s.v.weights, A.p(wp)));
            wdev = A.p(wp);
        }
        Buf& out = l.bn ? S.z[s.i] : S.tens[l.dst];
        out = A.alloc((size_t)s.rows * l.cout * (s.b16 && l.bn ? 2 : 4));      // (dtype 1: z in bf16; the feature maps fp32)
        float* y = s.y = A.p(out);
        const float *xin = s.xin, *ones = A.p(S.ones), *shift = l.bn ? A.p(S.zeros) : s.v.biases;
        void* skp = A.p(S.sk_ws);
        const size_t skb = S.sk_ws.bytes;
        y3_sk_opts so = sk_opts(r);
        so.stats = s.nblk ? A.p(s.part) : nullptr;
        hipStream_t st = stream();
        switch (r.kind) {
        case RouteKind::Bf16Train:
            if (l.bn) Y3_TRY(y3_launch_conv_bf16_train(st, &d, xin, wdev, y, A.p(s.part)));
            else Y3_TRY(y3_launch_conv_bf16_reg(st, &d, xin, wdev, ones, shift, y, 1));
            break;
        case RouteKind::Wino44: Y3_TRY(y3_launch_conv_wino44(st, &d, xin, wdev, ones, shift, nullptr, y, skp, skb, &so)); break;
        case RouteKind::Wino: Y3_TRY(y3_launch_conv_wino(st, &d, xin, wdev, ones, shift, nullptr, y, skp, skb, &so)); break;
        case RouteKind::Split:
            Y3_TRY(y3_launch_conv_split(st, &d, r.planes, xin, nullptr, wdev, ones, shift, nullptr, y, skp, skb, &so)); break;
        default: Y3_TRY(y3_launch_conv(st, &d, xin, nullptr, wdev, ones, shift, nullptr, y, skp, skb, &so));
        }
        A.release(wp);
        return Y3_OK;
    }

    // the batch statistics of z (and the moving ones), in one of three forms, into the layer's saved [4][cout]; then BN applied
    int batch_norm(Step& s) {
        const int cout = s.l.cout, nblk = s.nblk;
        const y3_train_var& v = s.v;
        S.stats[s.i] = A.alloc((size_t)4 * cout * 4);
        float* st = A.p(S.stats[s.i]);
        if (net->bn_sync_fn) {      // the same statistics as sums | exchange | finish (the dry run launches and calls nothing)
            Y3_TRY(y3_bn_sync_stats_sums(ctx, s.y, 0, nblk ? A.p(s.part) : nullptr, nblk, s.rows, cout, net->bn_sync_buf,
                                         A.p(S.reduce_sc)));
            Y3_TRY(bn_sync_call(net, s.i, 0, cout));
            Y3_TRY(y3_bn_sync_stats_finish(ctx, net->bn_sync_buf, cout, v.gamma, v.beta, BN_EPS, o->bn_decay, st, st + cout,
                                           st + 2 * cout, st + 3 * cout, v.moving_mean, v.moving_variance));
        } else if (nblk)
            Y3_TRY(y3_bn_train_stats_partials(ctx, A.p(s.part), nblk, s.rows, cout, v.gamma, v.beta, BN_EPS, o->bn_decay, st,
                                              st + cout, st + 2 * cout, st + 3 * cout, v.moving_mean, v.moving_variance));
        else
            Y3_TRY(y3_bn_train_stats(ctx, s.y, s.rows, cout, v.gamma, v.beta, BN_EPS, o->bn_decay, st, st + cout, st + 2 * cout,
                                     st + 3 * cout, v.moving_mean, v.moving_variance, A.p(S.reduce_sc)));
        A.release(s.part);
        const Layer& l = s.l;       // the layer's activation: folded scale / shift, LeakyReLU, the shortcut added
        S.tens[l.dst] = A.alloc((size_t)s.rows * cout * (s.half ? 2 : 4));
        const float* res = l.resid >= 0 ? tptr(l.resid) : nullptr;
        if (s.half)      // (the stem's z is fp32)
            Y3_TRY(y3_bn_apply_fwd_bf16(ctx, s.y, !s.b16, st + 2 * cout, st + 3 * cout, res, s.rows, cout, A.p(S.tens[l.dst])));
        else
            Y3_TRY(y3_bn_apply_fwd(ctx, s.y, st + 2 * cout, st + 3 * cout, res, s.rows, cout, 1, A.p(S.tens[l.dst])));
        return Y3_OK;
    }

    int run() {
        if (!dry) Y3_STEP(fill_constants());
        for (int i = 0; i < (int)net->layers.size(); ++i) {
            const Layer& l = net->layers[i];
            const y3_conv_desc d = net->desc(i, n, h, w, true);
            Step s{i, l, vars[i], d, S.routes[i].fwd.kind == RouteKind::Bf16Train, net->dtype == NetDtype::BF16, tptr(l.src),
                   (long long)n * (d.h / l.stride) * (d.w / l.stride)};
            Y3_TRY(ctx_pending_error(ctx));     // (the conv launches below go to the launchers: refuse after a stream-K time-out)
            Y3_STEP(concat_input(s));
            Y3_STEP(pool_input(s));
            Y3_STEP(conv(s));
            if (l.bn) Y3_STEP(batch_norm(s));
            const int e = net->tensors[l.dst].ext;
            if (e >= 0) S.fm_tensor[e] = l.dst;
        }
        // the loss gradients live with the saved tensors (backward may be re-run from them)
        for (int i = 0; i < 3; ++i) {
            const int s = 32 >> i;
            S.fm_grad[i] = A.alloc((size_t)n * (h / s) * (w / s) * det_pad_of(net) * 4);
        }
        S.saved_top = A.top;
        if (!dry && A.overflow) { y3_set_error("y3_net_train_forward: workspace too small"); return Y3_EINVAL; }
        S.have_fwd = !dry;
        return Y3_OK;
    }
};

// sizes the persistent scratch and runs (or, dry, only sizes) the training forward
int forward_impl(y3_net* net, const y3_train_var* vars, const float* x, int n, int h, int w, const y3_train_opts* o,
                 void* ws, size_t ws_bytes, bool dry) {
    if (!net->train) net->train = new y3_train_state;
    y3_train_state& S = *net->train;
    S.arena.reset(ws, ws_bytes, dry);
    S.n = n; S.h = h; S.w = w; S.x = x;
    S.have_fwd = S.have_loss = false;
    const size_t nl = net->layers.size();
    S.tens.assign(net->tensors.size(), Buf());
    S.xin.assign(nl, Buf());
    S.z.assign(nl, Buf());
    S.stats.assign(nl, Buf());
    alloc_scratch(net, S, n, h, w);
    return Forward(net, vars, o, dry).run();
}

int loss_impl(y3_net* net, const float* const y_true[3], const y3_train_opts* o, float* loss5, bool dry) {
    y3_train_state& S = *net->train;
    Arena& A = S.arena;
    y3_ctx* ctx = net->ctx;
    const int C = net->class_num, det_pad = det_pad_of(net);
    if (!dry) Y3_CHECK_HIP(hipMemsetAsync(A.p(S.loss4), 0, 16, ctx->stream));
    for (int i = 0; i < 3; ++i) {
        const int s = 32 >> i, gh = S.h / s, gw = S.w / s;
        if (dry) continue;
        Y3_CHECK_HIP(hipMemsetAsync(A.p(S.fm_grad[i]), 0, (size_t)S.n * gh * gw * det_pad * 4, ctx->stream));   // pad lanes stay 0
        // model.py:352-355: anchors [6:9], [3:6], [0:3] for the 13-, 26-, 52-grid maps
        const float* anc = o->anchors + 2 * 3 * (2 - i);
        const int rc = y3_loss_layer_conf(ctx, A.p(S.tens[S.fm_tensor[i]]), y_true[i], S.n, gh, gw, C, S.h, S.w, anc,
                                          o->use_label_smooth, o->use_focal_loss, net->box_loss, net->ignore_thresh,
                                          net->obj_iou_ratio, i > 0, A.p(S.loss4), A.p(S.fm_grad[i]), det_pad,
                                          A.p(S.loss_sc), S.loss_sc.bytes);
        if (rc != Y3_OK) return rc;
    }
    if (!dry && loss5) {
        hipLaunchKernelGGL(loss_total_kernel, dim3(1), dim3(64), 0, ctx->stream, A.p(S.loss4), loss5);
        Y3_CHECK_HIP(hipGetLastError());
    }
    S.have_loss = !dry;
    return Y3_OK;
}

// ---- backward -----------------------------------------------------------------------------------------------------------

// The gradient of every tensor (activation) while backward walks the layers: its buffer, whether a contribution is in it,
// and whether the buffer is this pass's (an arena buffer) or the forward's (a loss gradient: never released here).
struct GradTable {
    struct Entry { Buf buf; bool have = false, own = false; };
    std::vector<Entry> e;
    Arena& A;
    explicit GradTable(Arena& A_) : A(A_) {}
    void reset(size_t tensors) { e.assign(tensors, Entry()); }
    void set_loss_gradient(int t, Buf b) { e[t].buf = b; e[t].have = true; }
    bool have(int t) const { return e[t].have; }
    Buf buf(int t) const { return e[t].buf; }
    // The buffer the next contribution to tensor t's gradient goes to, allocated on first use (`bytes`) and from now on
    // present.  *accumulate: something is in it already, the caller's launch must add.
    Buf contribute(int t, size_t bytes, int* accumulate) {
        Entry& x = e[t];
        if (!x.have) { x.buf = A.alloc(bytes); x.own = true; }
        *accumulate = x.have ? 1 : 0;
        x.have = true;
        return x.buf;
    }
    // dy of `from` is also the first contribution to `to` (res_block: net + shortcut, utils/layer_utils.py:30): the buffer
    // itself becomes that gradient (no copy)
    void hand_off(int from, int to) { e[to].buf = e[from].buf; e[to].own = e[from].own; e[to].have = true; }
    // The consumed gradient of tensor t leaves the table.  What goes back to the free list: owned buffers only, never the
    // loss gradients, and not one that was handed off.
    Buf consume(int t, bool handed_off) {
        const Buf b = (!handed_off && e[t].own) ? e[t].buf : Buf();
        e[t].buf = Buf();
        return b;
    }
};

// Two streams (y3_net_train_set_wgrad_stream).  A layer's weight gradient is off the critical path - nothing of this pass
// reads it - while its data gradient and the BN backward of the layer below are on it: the weight gradient goes to the
// side stream behind "dz ready", and the context's stream waits for it only one layer later, just before the buffers it
// read go back to the arena (their release, and the layer's `ready` call, are deferred by that one layer; the dry run
// defers alike, so the workspace is sized for it).  What overlaps: a matrix-pipe-bound weight gradient with the HBM-bound
// BN passes of the next layer.  One weight gradient is in flight at most: deeper lanes were measured and lost
// (profiles/r06_wgrad_stream_ab.txt).  The lane of one pass: the side context, the event pair in use and the one pending
// entry.  It also makes the pass's `ready` calls, so that they come in order with the entry's.
struct WgradLane {
    y3_train_state& S; Arena& A; y3_ctx* const main_ctx;
    y3_ctx* side;                       // where a layer "on the side" launches (the dry run: nowhere)
    const bool dry, two;
    const y3_grad_ready_fn ready; void* const user;
    struct Pending {
        Buf a, b;                       // buffers the weight gradient read: released once the main stream waits for it
        hipEvent_t done = nullptr;
        long long g_end = -1;
        bool set = false;
    } pend;
    int flip = 0;                       // the event pair of the layer at hand (an event comes round again NEV layers later)

    WgradLane(y3_net* net, bool dry_, y3_grad_ready_fn ready_, void* user_)
        : S(*net->train), A(S.arena), main_ctx(net->ctx), side(net->ctx), dry(dry_), two(net->wgrad_stream != nullptr),
          ready(ready_), user(user_) {}
    // Every exit joins the side stream, the early error returns included: the caller may free the workspace or flat_grad as
    // soon as the pass returns, and a weight gradient still pending reads the one and writes the other.  (On the normal path
    // the final drain has retired it; no `ready` call here.)
    ~WgradLane() {
        if (!dry && pend.set && pend.done) (void)hipStreamWaitEvent(main_ctx->stream, pend.done, 0);
    }
    // for this pass: the side context on the net's second stream (made anew when that stream changed) and the events
    int open(const y3_net* net) {
        if (!two || dry) return Y3_OK;
        if (S.side_ctx && S.side_stream != net->wgrad_stream) { (void)y3_ctx_destroy(S.side_ctx); S.side_ctx = nullptr; }
        if (!S.side_ctx) {
            if (int rc = y3_ctx_create(main_ctx->device, net->wgrad_stream, &S.side_ctx)) return rc;
            S.side_stream = net->wgrad_stream;
        }
        for (int e = 0; e < y3_train_state::NEV; ++e) {
            if (!S.ev_dz[e]) Y3_CHECK_HIP(hipEventCreateWithFlags(&S.ev_dz[e], hipEventDisableTiming));
            if (!S.ev_done[e]) Y3_CHECK_HIP(hipEventCreateWithFlags(&S.ev_done[e], hipEventDisableTiming));
        }
        side = S.side_ctx;
        return Y3_OK;
    }
    int fork_behind_dz() {              // the side stream goes on behind what the main stream has enqueued: dz is ready
        if (dry) return Y3_OK;
        Y3_CHECK_HIP(hipEventRecord(S.ev_dz[flip], main_ctx->stream));
        Y3_CHECK_HIP(hipStreamWaitEvent(side->stream, S.ev_dz[flip], 0));
        return Y3_OK;
    }
    int mark_wgrad_done() {
        if (!dry) Y3_CHECK_HIP(hipEventRecord(S.ev_done[flip], side->stream));
        return Y3_OK;
    }
    // a and b are read by the weight gradient just marked: theirs release, and ready(g_end), wait for retire()
    void defer(Buf a, Buf b, long long g_end) {
        pend.a = a; pend.b = b; pend.g_end = g_end; pend.set = true;
        pend.done = dry ? nullptr : S.ev_done[flip];
        flip = (flip + 1) % y3_train_state::NEV;
    }
    // the pending entry, if any: the main stream waits for its weight gradient, its buffers go back, its `ready` is called
    int retire() {
        if (!pend.set) return Y3_OK;
        Pending q = pend;
        pend = Pending();
        if (!dry && q.done) Y3_CHECK_HIP(hipStreamWaitEvent(main_ctx->stream, q.done, 0));
        A.release(q.a);
        A.release(q.b);
        signal(q.g_end);
        return Y3_OK;
    }
    int drain() { return retire(); }    // (one entry deep)
    void signal(long long g_end) const {
        if (ready && g_end >= 0 && !dry) ready(user, g_end);
    }
};

struct Backward : Pass {
    float* const flat_grad;
    GradTable grads;
    WgradLane lane;
    // the BN backward reduction of a layer whose dy the data gradient of its reader writes (y3_route_dgrad: bn_blocks)
    struct Fused { Buf part; int nb = 0; };
    std::vector<Fused> fused;
    int first = -1;                  // earliest layer holding a trainable variable: gradients need not flow below it

    Backward(y3_net* net_, const y3_train_var* vars_, float* flat_grad_, y3_grad_ready_fn ready, void* user, bool dry_)
        : Pass(net_, vars_, dry_), flat_grad(flat_grad_), grads(A), lane(net_, dry_, ready, user) {}

    struct Step {                    // one layer of the pass
        int i; const Layer& l; const y3_train_var& v; y3_conv_desc d;
        bool b16;                    // dtype 1 (all but the stem): dz in bf16, rounded once from the fp32 BN backward (or loss gradient); dy stays fp32
        bool on_side;                // the weight gradient runs on the lane's side stream
        int dz_stride;
        long long rows;              // of dy and dz
        Buf dy;                      // the gradient of the layer's output
        Buf dz_buf;                  // where dz lives (dy itself, or a fresh buffer)
        bool dy_given_away = false;  // dy became the shortcut's gradient
        const float* w_d = nullptr;  // the kernel as the data gradient reads it: [k*k][cin][dz_stride]
        Buf w_d_buf;
    };
    // (asked of the offsets, not the pointers: the dry run's flat_grad is null, and an offset of 0 must not look untrainable)
    static bool trainable(long long g) { return g >= 0; }
    float* gptr(long long g) const { return g >= 0 && flat_grad ? flat_grad + g : nullptr; }
    bool needs(int t) const { return t > 0 && (t - 1) >= first; }       // tensor t is produced by layer t-1
    size_t tbytes(int id) const {
        const Tensor& t = net->tensors[id];
        return (size_t)n * (h / t.sdiv) * (w / t.sdiv) * t.c * 4;
    }
    const float* xin(const Step& s) const { return S.xin[s.i].ok() ? A.p(S.xin[s.i]) : tptr(s.l.src); }

    // dy -> the shortcut's gradient and dz = the BN backward of dy, with d gamma / d beta, in one of its four forms
    int bn_layer(Step& s) {
        const Layer& l = s.l;
        const y3_train_var& v = s.v;
        const int i = s.i, cout = l.cout;
        const long long rows = s.rows;
        if (l.resid >= 0 && needs(l.resid)) {
            if (grads.have(l.resid)) {
                int acc;
                const Buf g = grads.contribute(l.resid, tbytes(l.resid), &acc);
                Y3_TRY(y3_slice_accumulate(ctx, A.p(s.dy), cout, 0, rows, cout, acc, A.p(g)));
            } else {
                grads.hand_off(l.dst, l.resid);
                s.dy_given_away = true;
            }
        }
        // fp32: BN backward runs in place unless dy was given away; bf16: dz is always a buffer of its own, half the size
        s.dz_buf = s.b16 ? A.alloc((size_t)rows * cout * 2) : s.dy_given_away ? A.alloc((size_t)rows * cout * 4) : s.dy;
        Buf tmp;
        if (!trainable(v.g_gamma) || !trainable(v.g_beta)) tmp = A.alloc((size_t)2 * cout * 4);
        float* dgam = trainable(v.g_gamma) ? gptr(v.g_gamma) : A.p(tmp);
        float* dbet = trainable(v.g_beta) ? gptr(v.g_beta) : at(A.p(tmp), cout);
        const float *st = A.p(S.stats[i]), *z = A.p(S.z[i]), *dy = A.p(s.dy);
        const float *sc = at(st, 2 * cout), *sh = at(st, 3 * cout), *mean = st, *istd = at(st, cout);
        float *dz = A.p(s.dz_buf), *bsc = A.p(S.bnbwd_sc);
        Fused& f = fused[i];
        if (net->bn_sync_fn) {      // sums (d gamma, d beta from this rank's) | exchange | coefficients and apply pass
            const float* fp = f.nb > 0 ? A.p(f.part) : nullptr;
            Y3_TRY(y3_bn_sync_bwd_sums(ctx, z, s.b16, dy, sc, sh, mean, istd, rows, cout, fp, f.nb, dgam, dbet, net->bn_sync_buf, bsc));
            if (f.nb > 0) A.release(f.part);
            Y3_TRY(bn_sync_call(net, i, 1, cout));
            Y3_TRY(y3_bn_sync_bwd_finish(ctx, z, s.b16, dy, v.gamma, sc, sh, mean, istd, rows, cout, net->bn_sync_buf, dz, bsc));
        } else if (s.b16) {
            Y3_TRY(y3_bn_train_bwd_bf16(ctx, z, dy, v.gamma, sc, sh, mean, istd, rows, cout, dgam, dbet, dz, bsc));
        } else if (f.nb > 0) {
            Y3_TRY(y3_bn_train_bwd_partials(ctx, z, dy, v.gamma, sc, sh, mean, istd, rows, cout, A.p(f.part), f.nb, dgam, dbet, dz, bsc));
            A.release(f.part);
        } else {
            Y3_TRY(y3_bn_train_bwd(ctx, z, dy, v.gamma, sc, sh, mean, istd, rows, cout, dgam, dbet, dz, bsc));
        }
        A.release(tmp);
        return Y3_OK;
    }

    // dz = the loss gradient: the bias gradient, then dz rounded to bf16 or the kernel's channels padded to dz's
    int detection_layer(Step& s) {
        const Layer& l = s.l;
        if (trainable(s.v.g_biases)) {
            float* tmp = at(A.p(S.bias_sc), (long long)BIAS_SC_ROWS * s.dz_stride);      // [det_pad] behind the kernel's own scratch
            Y3_TRY(y3_bias_grad(ctx, A.p(s.dy), s.rows, s.dz_stride, tmp, A.p(S.bias_sc)));
            if (!dry) Y3_CHECK_HIP(hipMemcpyAsync(gptr(s.v.g_biases), tmp, (size_t)l.cout * 4, hipMemcpyDeviceToDevice, ctx->stream));
        }
        if (s.b16) {           // d loss / d fm, rounded once to bf16 (the bias gradient above read it in fp32)
            s.dz_buf = A.alloc((size_t)s.rows * s.dz_stride * 2);
            Y3_TRY(y3_f32_to_bf16(ctx, A.p(s.dy), s.rows * s.dz_stride, A.p(s.dz_buf)));
        } else {
            s.dz_buf = s.dy;
            // the data gradient reads the kernel as [k*k][cin][dz_stride]: zero-extend its last axis
            s.w_d_buf = A.alloc((size_t)l.k * l.k * l.cin * s.dz_stride * 4);
            Y3_TRY(y3_pad_channels(ctx, s.v.weights, l.cout, (long long)l.k * l.k * l.cin, s.dz_stride, A.p(s.w_d_buf)));
            s.w_d = A.p(s.w_d_buf);
        }
        return Y3_OK;
    }

    // on the context's stream, or on the lane's behind "dz ready"
    int weight_gradient(Step& s) {
        if (!trainable(s.v.g_weights)) return Y3_OK;
        if (s.on_side) Y3_STEP(lane.fork_behind_dz());
        y3_ctx* wctx = s.on_side ? lane.side : ctx;
        const float* dz = A.p(s.dz_buf);
        float* dw = gptr(s.v.g_weights);
        if (s.b16)
            Y3_TRY(y3_launch_conv_wgrad_bf16(wctx->stream, &s.d, xin(s), dz, s.dz_stride, dw, A.p(S.wgrad_sc), S.wgrad_sc.bytes));
        else if (S.routes[s.i].wgrad.kind == RouteKind::Wino)
            Y3_TRY(y3_conv_wgrad_wino(wctx, &s.d, xin(s), dz, s.dz_stride, dw, A.p(S.wgrad_sc), S.wgrad_sc.bytes));
        else
            Y3_TRY(y3_conv_wgrad(wctx, &s.d, xin(s), dz, s.dz_stride, dw, A.p(S.wgrad_sc), S.wgrad_sc.bytes));
        if (s.on_side) Y3_STEP(lane.mark_wgrad_done());
        return Y3_OK;
    }

    // This layer's gradients are complete (enqueued) - on the lane: once the main stream waits for it (retire).
    // ready(g_end) promises all of flat[0:g_end), which holds the gradients of the layers above this one (gradient_layout):
    // a layer that is not on the side stream (a trainable gamma / beta / bias under an untrainable kernel) first joins
    // the weight gradient still pending, so the calls come in increasing g_end order, each behind the waits for all
    // it covers.  (The dry run drains alike: the releases move with it.)
    int ready_edge(const Step& s) {
        if (s.on_side || s.v.g_end < 0) return Y3_OK;
        Y3_STEP(lane.drain());
        lane.signal(s.v.g_end);
        return Y3_OK;
    }

    // the launch of the layer's data gradient by its route: dx (+)= it  (acc: the Winograd forms read dx as the residual, same thread)
    int launch_dgrad(const Step& s, const float* wk, const y3_sk_opts& so, int acc, float* dx) {
        const ConvRoute& r = S.routes[s.i].dgrad;
        const y3_conv_desc& d = s.d;
        const y3_conv_desc g = y3_dgrad_desc(&d, s.dz_stride);      // (the Winograd forms run it as a forward conv)
        const float *dz = A.p(s.dz_buf), *ones = A.p(S.ones), *zeros = A.p(S.zeros);
        void* skp = A.p(S.sk_ws);
        const size_t skb = S.sk_ws.bytes;
        hipStream_t st = stream();
        switch (r.kind) {
        case RouteKind::Bf16Train: Y3_TRY(y3_launch_conv_bf16_dgrad(st, &d, dz, s.dz_stride, wk, acc, dx)); break;
        case RouteKind::Wino44: Y3_TRY(y3_launch_conv_wino44(st, &g, dz, wk, ones, zeros, acc ? dx : nullptr, dx, skp, skb, &so)); break;
        case RouteKind::Wino: Y3_TRY(y3_launch_conv_wino(st, &g, dz, wk, ones, zeros, acc ? dx : nullptr, dx, skp, skb, &so)); break;
        case RouteKind::Split:
            Y3_TRY(y3_launch_conv_dgrad_split(st, &d, r.planes, dz, s.dz_stride, wk, ones, zeros, acc, dx, skp, skb, &so)); break;
        default: Y3_TRY(y3_launch_conv_dgrad(st, &d, dz, s.dz_stride, s.w_d, ones, zeros, acc, dx, skp, skb, &so));
        }
        return Y3_OK;
    }

    // a pool layer: the data gradient into a [rows, 4c] buffer; y3_spp_bwd takes the argmax from x, the last slot of the
    // spp(x) the forward kept (S.xin), and writes the gradient of src - so the BN backward reduction of the layer below is
    // never fused here (y3_route_dgrad)
    int pool_gradient(const Step& s, const float* wk, const y3_sk_opts& so) {
        const Layer& l = s.l;
        const int c = net->tensors[l.src].c;
        const bool half = net->dtype == NetDtype::BF16;
        const long long in_rows = (long long)n * s.d.h * s.d.w;
        Buf dpool = A.alloc((size_t)in_rows * l.cin * 4);
        Y3_STEP(launch_dgrad(s, wk, so, 0, A.p(dpool)));
        int acc;
        const Buf g = grads.contribute(l.src, tbytes(l.src), &acc);
        const char* x = at(reinterpret_cast<const char*>(A.p(S.xin[s.i])), (long long)3 * c * (half ? 2 : 4));
        Y3_TRY(y3_spp_bwd(ctx, x, l.cin, half, A.p(dpool), n, s.d.h, s.d.w, c, acc, A.p(g)));
        A.release(dpool);
        return Y3_OK;
    }

    // the gradient of the layer's input, where a layer below trains: into the gradients of src (and, a concat input, of up)
    int data_gradient(Step& s) {
        const Layer& l = s.l;
        const int src = l.src, up = l.up, cin = l.cin;
        const bool need_src = needs(src), need_up = up >= 0 && needs(up);
        if (!need_src && !need_up) return Y3_OK;
        const ConvRoute& r = S.routes[s.i].dgrad;
        const ConvPack pk = y3_conv_pack(*net, s.i, r, true);
        Buf wk = pk.bytes() ? A.alloc(pk.bytes()) : Buf();      // the kernel in the data gradient's packing
        if (wk.ok()) Y3_TRY(pk.launch(ctx, s.w_d, A.p(wk)));     // (the direct kernel reads w_d)
        y3_sk_opts so = sk_opts(r);
        int acc;
        if (up >= 0) {               // the gradient of the concat, then its two slices: upsample backward | copy
            const long long in_rows = (long long)n * s.d.h * s.d.w;
            Buf dcat = A.alloc((size_t)in_rows * cin * 4);
            Y3_STEP(launch_dgrad(s, A.p(wk), so, 0, A.p(dcat)));
            const int cu = net->tensors[up].c;
            if (need_up) {
                const Buf g = grads.contribute(up, tbytes(up), &acc);
                Y3_TRY(y3_upsample2x_bwd(ctx, A.p(dcat), cin, n, s.d.h / 2, s.d.w / 2, cu, acc, A.p(g)));
            }
            if (need_src) {
                const Buf g = grads.contribute(src, tbytes(src), &acc);
                Y3_TRY(y3_slice_accumulate(ctx, A.p(dcat), cin, cu, in_rows, cin - cu, acc, A.p(g)));
            }
            A.release(dcat);
        } else if (l.pool) {         // the gradient of spp(src), then the pool's backward into the gradient of src
            Y3_STEP(pool_gradient(s, A.p(wk), so));
        } else {
            const Buf g = grads.contribute(src, tbytes(src), &acc);
            // src is the output of layer src - 1: fuse its BN backward reduction where this is the last contribution
            const int pj = src - 1;
            const int nbf = pj >= first ? r.bn_blocks : 0;
            if (nbf > 0) {                // (a Direct route: the launch takes them through `so`)
                fused[pj].part = A.alloc((size_t)nbf * 2 * cin * 4);
                fused[pj].nb = nbf;
                so.stats = A.p(fused[pj].part); so.bwd_z = A.p(S.z[pj]); so.bwd_vec = A.p(S.stats[pj]);
            }
            Y3_STEP(launch_dgrad(s, A.p(wk), so, acc, A.p(g)));
        }
        A.release(wk);
        return Y3_OK;
    }

    // The consumed gradient goes back to the free list - at once, or, when the side stream may still be reading it, behind
    // the wait of the NEXT layer's end: first the layer before this one is retired, then this one takes its place.
    int retire(Step& s) {
        A.release(s.w_d_buf);
        Y3_STEP(lane.retire());
        Buf rel_a = (s.dz_buf.off != s.dy.off) ? s.dz_buf : Buf();
        Buf rel_b = grads.consume(s.l.dst, s.dy_given_away);
        if (s.on_side) {
            lane.defer(rel_a, rel_b, s.v.g_end);
        } else {
            A.release(rel_a);
            A.release(rel_b);
        }
        return Y3_OK;
    }

    int run() {
        A.rewind(S.saved_top);
        const int nl = (int)net->layers.size();
        for (int i = 0; i < nl && first < 0; ++i) {
            const y3_train_var& v = vars[i];
            if (trainable(v.g_weights) || trainable(v.g_gamma) || trainable(v.g_beta) || trainable(v.g_biases)) first = i;
        }
        if (first < 0) return Y3_OK;
        grads.reset(net->tensors.size());
        for (int i = 0; i < 3; ++i) grads.set_loss_gradient(S.fm_tensor[i], S.fm_grad[i]);
        fused.assign(nl, Fused());
        Y3_STEP(lane.open(net));
        for (int i = nl - 1; i >= first; --i) {
            const Layer& l = net->layers[i];
            if (!grads.have(l.dst)) continue;
            const y3_conv_desc d = net->desc(i, n, h, w, true);
            Step s{i, l, vars[i], d, S.routes[i].wgrad.kind == RouteKind::Bf16Train, lane.two && trainable(vars[i].g_weights),
                   net->dz_stride(i), (long long)n * (d.h / l.stride) * (d.w / l.stride), grads.buf(l.dst)};
            s.w_d = s.v.weights;
            Y3_TRY(ctx_pending_error(ctx));
            Y3_STEP(l.bn ? bn_layer(s) : detection_layer(s));
            Y3_STEP(weight_gradient(s));
            Y3_STEP(ready_edge(s));
            Y3_STEP(data_gradient(s));
            Y3_STEP(retire(s));
        }
        Y3_STEP(lane.drain());
        if (!dry && A.overflow) { y3_set_error("y3_net_train_backward: workspace too small"); return Y3_EINVAL; }
        return Y3_OK;
    }
};

int backward_impl(y3_net* net, const y3_train_var* vars, float* flat_grad, y3_grad_ready_fn ready, void* user, bool dry) {
    return Backward(net, vars, flat_grad, ready, user, dry).run();
}

int check_common(const char* who, y3_net* net, int n, int h, int w) {
    Y3_CHECK_ARG(net, "%s: null net", who);
    Y3_CHECK_ARG(n > 0 && h > 0 && w > 0 && h % 32 == 0 && w % 32 == 0,
                 "%s: the batch must be positive and the input size a positive multiple of 32 (got %d x %dx%d)", who, n, h, w);
    return Y3_OK;
}

int check_vars(const char* who, const y3_net* net, const y3_train_var* vars) {
    Y3_CHECK_ARG(vars, "%s: null variable table", who);
    for (size_t i = 0; i < net->layers.size(); ++i) {
        const Layer& l = net->layers[i];
        const y3_train_var& v = vars[i];
        Y3_CHECK_ARG(v.weights, "%s: layer %zu has no kernel", who, i);
        if (l.bn) Y3_CHECK_ARG(v.gamma && v.beta && v.moving_mean && v.moving_variance, "%s: layer %zu: batch-norm variables missing", who, i);
        else Y3_CHECK_ARG(v.biases, "%s: layer %zu: bias missing", who, i);
    }
    return Y3_OK;
}

}  // namespace

extern "C" int y3_net_train_set_wgrad_stream(y3_net* net, void* stream) {
    Y3_CHECK_ARG(net, "y3_net_train_set_wgrad_stream: null net");
    if (stream == Y3_OWN_STREAM) {
        // A stream of the LOWEST priority, created here: (1) the weight gradient is the work that can wait - where the two
        // streams compete, the critical path should win; (2) a stream of another priority gets a hardware queue of its own.
        // Measured why (2) matters: a caller's ordinary stream can land on the hardware queue of the context's stream once
        // enough streams are alive in the process (bench.py's default line: c2, detect and c5 each leave two behind) - the
        // event waits between the two then serialise INSIDE one queue: 96 ms per step instead of 79.6
        // (profiles/r06_wgrad_stream_ab.txt).
        if (!net->own_stream) {
            if (!net->ctx) { y3_set_error("y3_net_train_set_wgrad_stream: the net was created without a context"); return Y3_ESTATE; }
            int prev = -1;
            Y3_CHECK_HIP(hipGetDevice(&prev));
            Y3_CHECK_HIP(hipSetDevice(net->ctx->device));
            int least = 0, greatest = 0;
            hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
            hipStream_t s = nullptr;
            if (e == hipSuccess) e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least);
            (void)hipSetDevice(prev);
            if (e != hipSuccess) { y3_set_error("y3_net_train_set_wgrad_stream: %s", hipGetErrorString(e)); return Y3_EHIP; }
            net->own_stream = s;
        }
        stream = net->own_stream;
    }
    net->wgrad_stream = stream;
    return Y3_OK;
}

extern "C" int y3_net_train_set_box_loss(y3_net* net, int box_loss) {
    Y3_CHECK_ARG(net, "y3_net_train_set_box_loss: null net");
    Y3_CHECK_ARG(box_loss >= Y3_BOX_MSE && box_loss <= Y3_BOX_CIOU, "y3_net_train_set_box_loss: unknown box_loss kind %d", box_loss);
    net->box_loss = box_loss;
    return Y3_OK;
}

extern "C" int y3_net_train_set_conf_rule(y3_net* net, float ignore_thresh, float obj_iou_ratio) {
    Y3_CHECK_ARG(net, "y3_net_train_set_conf_rule: null net");
    Y3_CHECK_ARG(ignore_thresh >= 0.f && ignore_thresh <= 1.f, "y3_net_train_set_conf_rule: ignore_thresh %g outside [0, 1]",
                 (double)ignore_thresh);
    Y3_CHECK_ARG(obj_iou_ratio >= 0.f && obj_iou_ratio <= 1.f, "y3_net_train_set_conf_rule: obj_iou_ratio %g outside [0, 1]",
                 (double)obj_iou_ratio);
    net->ignore_thresh = ignore_thresh;
    net->obj_iou_ratio = obj_iou_ratio;
    return Y3_OK;
}

extern "C" int y3_net_train_set_bn_sync(y3_net* net, y3_bn_sync_fn fn, void* user, double* exchange_dev, size_t exchange_bytes) {
    Y3_CHECK_ARG(net, "y3_net_train_set_bn_sync: null net");
    if (fn)
        Y3_CHECK_ARG(exchange_dev && exchange_bytes >= (size_t)(2 * BN_MAXC + 1) * sizeof(double),
                     "y3_net_train_set_bn_sync: the exchange buffer must hold %d doubles", 2 * BN_MAXC + 1);
    net->bn_sync_fn = fn;
    net->bn_sync_user = fn ? user : nullptr;
    net->bn_sync_buf = fn ? exchange_dev : nullptr;
    return Y3_OK;
}

extern "C" size_t y3_net_train_workspace_bytes(y3_net* net, const y3_train_var* vars, int n, int h, int w) {
    if (check_common("y3_net_train_workspace_bytes", net, n, h, w) != Y3_OK || !vars) return 0;
    // the same allocation sequence as a real step, nothing launched; the state is rebuilt by the next forward anyway
    y3_train_opts o;
    std::memset(&o, 0, sizeof(o));
    if (forward_impl(net, vars, nullptr, n, h, w, &o, nullptr, 0, true) != Y3_OK) return 0;
    const float* yt[3] = {nullptr, nullptr, nullptr};
    if (loss_impl(net, yt, &o, nullptr, true) != Y3_OK) return 0;
    std::vector<y3_train_var> all(vars, vars + net->layers.size());
    if (backward_impl(net, all.data(), nullptr, nullptr, nullptr, true) != Y3_OK) return 0;
    const size_t peak = net->train->arena.peak;
    net->train->have_fwd = net->train->have_loss = false;
    return (peak + 255) & ~(size_t)255;
}

extern "C" int y3_net_train_forward(y3_net* net, const y3_train_var* vars, const float* x, int n, int h, int w,
                                    const y3_train_opts* opts, void* workspace, size_t workspace_bytes, float** fm1,
                                    float** fm2, float** fm3) {
    if (int rc = check_common("y3_net_train_forward", net, n, h, w)) return rc;
    if (int rc = check_vars("y3_net_train_forward", net, vars)) return rc;
    Y3_CHECK_ARG(x && opts && workspace, "y3_net_train_forward: null argument");
    Y3_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "y3_net_train_forward: workspace must be 256-byte aligned");
    if (!net->ctx) { y3_set_error("y3_net_train_forward: the net was created without a context"); return Y3_ESTATE; }
    // Refuse a workspace that is too small BEFORE anything is launched: the dry run (host only, a few microseconds per layer)
    // replays the allocation sequence of forward + loss + backward for THIS dtype, shape and variable table.  (The arena's
    // own overflow flag is only read after a pass has been enqueued - too late to keep the device from writing past the end.)
    {
        const size_t need = y3_net_train_workspace_bytes(net, vars, n, h, w);
        if (need == 0 || workspace_bytes < need) {
            y3_set_error("y3_net_train_forward: workspace too small (%zu bytes given, %zu needed for this dtype / shape / variable table)",
                         workspace_bytes, need);
            return Y3_EINVAL;
        }
    }
    if (int rc = forward_impl(net, vars, x, n, h, w, opts, workspace, workspace_bytes, false)) return rc;
    y3_train_state& S = *net->train;
    float** out[3] = {fm1, fm2, fm3};
    for (int i = 0; i < 3; ++i)
        if (out[i]) *out[i] = S.arena.p(S.tens[S.fm_tensor[i]]);
    return Y3_OK;
}

extern "C" int y3_net_train_loss(y3_net* net, const float* y_true_1, const float* y_true_2, const float* y_true_3,
                                 const y3_train_opts* opts, float* loss5) {
    Y3_CHECK_ARG(net && y_true_1 && y_true_2 && y_true_3 && opts && opts->anchors, "y3_net_train_loss: null argument");
    if (!net->train || !net->train->have_fwd) { y3_set_error("y3_net_train_loss: call y3_net_train_forward first"); return Y3_ESTATE; }
    const float* yt[3] = {y_true_1, y_true_2, y_true_3};
    return loss_impl(net, yt, opts, loss5, false);
}

extern "C" int y3_net_train_backward(y3_net* net, const y3_train_var* vars, float* flat_grad, y3_grad_ready_fn ready,
                                     void* user) {
    Y3_CHECK_ARG(net && flat_grad, "y3_net_train_backward: null argument");
    if (int rc = check_vars("y3_net_train_backward", net, vars)) return rc;
    if (!net->train || !net->train->have_fwd || !net->train->have_loss) {
        y3_set_error("y3_net_train_backward: call y3_net_train_forward and y3_net_train_loss first");
        return Y3_ESTATE;
    }
    return backward_impl(net, vars, flat_grad, ready, user, false);
}

extern "C" int y3_net_train_step(y3_net* net, const y3_train_var* vars, const float* x, int n, int h, int w,
                                 const float* y_true_1, const float* y_true_2, const float* y_true_3,
                                 const y3_train_opts* opts, float* flat_grad, void* workspace, size_t workspace_bytes,
                                 float* loss5, y3_grad_ready_fn ready, void* user) {
    if (int rc = y3_net_train_forward(net, vars, x, n, h, w, opts, workspace, workspace_bytes, nullptr, nullptr, nullptr)) return rc;
    if (int rc = y3_net_train_loss(net, y_true_1, y_true_2, y_true_3, opts, loss5)) return rc;
    return y3_net_train_backward(net, vars, flat_grad, ready, user);
}

// offsets (bytes into the workspace of the last forward) of the tensors that fix layer i's LeakyReLU branches: the raw conv
// output z [n,ho,wo,cout] and the [4][cout] mean / inv_std / folded scale / folded shift (test hook of tests/test_train_gpu.py)
extern "C" int y3_net_train_saved(const y3_net* net, int layer, size_t* z_offset, size_t* stats_offset) {
    Y3_CHECK_ARG(net && net->train && net->train->have_fwd && layer >= 0 && layer < (int)net->layers.size(),
                 "y3_net_train_saved: no forward state for layer %d", layer);
    const y3_train_state& S = *net->train;
    if (z_offset) *z_offset = S.z[layer].off;
    if (stats_offset) *stats_offset = S.stats[layer].off;
    return Y3_OK;
}

// offset (bytes into the workspace of the last forward) of a pool layer's materialised spp(x), in the element type of x (bf16 in
// net dtype 1); SIZE_MAX for every other layer (test hook of tests/test_spp_gpu.py)
extern "C" int y3_net_train_saved_pool(const y3_net* net, int layer, size_t* offset) {
    Y3_CHECK_ARG(net && net->train && net->train->have_fwd && layer >= 0 && layer < (int)net->layers.size() && offset,
                 "y3_net_train_saved_pool: no forward state for layer %d", layer);
    *offset = net->layers[layer].pool ? net->train->xin[layer].off : SIZE_MAX;
    return Y3_OK;
}

// 1: layer i's saved z (y3_net_train_saved) is bf16 (net dtype 1, every BN layer but the stem); 0: fp32
extern "C" int y3_net_train_saved_type(const y3_net* net, int layer) {
    if (!net || layer < 0 || layer >= (int)net->layers.size()) return 0;
    const Layer& l = net->layers[layer];
    return net->dtype == NetDtype::BF16 && l.bn && l.cin != 3 ? 1 : 0;
}
