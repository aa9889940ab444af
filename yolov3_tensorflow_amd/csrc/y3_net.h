// The conv graph object (75 convs; YOLOv3-SPP: 76 and one pooling block) shared by the inference plan (y3_abi.hip: y3_net_forward) and the train step
// (y3_net_train.hip).  Tensor ids: 0 = network input; 1.. = conv outputs in creation order.
#pragma once
#include <vector>
#include <algorithm>
#include "y3_internal.h"

// y3_net_set_dtype: exact fp32 MFMA | bf16 storage | fp32 from 3 / 2 bf16 planes (y3_conv_split.hip) | fp32 + Winograd kernels
enum class NetDtype { F32 = 0, BF16 = 1, F32_BF16X6 = 2, F32_BF16X3 = 3, F32_WINO = 4 };

// How a conv layer runs in one role, decided only by y3_route_* (y3_abi.hip).  InNext: inside the next layer's launch; the
// three after it: this launch also runs the layer before it.  Bf16Train: the bf16 train step's kernels (net dtype 1: the
// register-staged bf16 kernel's training forms, y3_conv_bf16.hip; the weight gradient of y3_wgrad_bf16.hip).
enum class RouteKind { Direct, Split, Wino, Wino44, Bf16, InNext, StemS2F32, StemS2Bf16, ResBlock64Bf16, Bf16Train };
struct ConvRoute {
    RouteKind kind = RouteKind::Direct;
    int planes = 0;          // Split: 3 or 2
    bool two_pass = false;   // Wino44: the two-kernel form (V = B^T d B in the scratch)
    bool streamk = false;    // Direct / Split: y3_conv_schedule_impl
    size_t scratch = 0;      // bytes of the conv scratch the launch needs (weight gradient: of its own scratch)
    int bn_blocks = 0;       // data gradient: rows of the fused BN-backward partial sums of the layer below (0: none)
};
struct y3_net;
ConvRoute y3_route_infer(const y3_net& net, int i, int n, int h, int w);
ConvRoute y3_route_train_fwd(const y3_net& net, int i, int n, int h, int w);
ConvRoute y3_route_dgrad(const y3_net& net, int i, int n, int h, int w);
ConvRoute y3_route_wgrad(const y3_net& net, int i, int n, int h, int w);

// The layout a launch reads a conv kernel in, implied by its route (y3_conv_pack, y3_abi.hip).  Hwio: the variable as it is
// (the Cin = 3 stem in every dtype; the direct data gradient, which reads the kernel as [k*k][cin][dz_stride]).  Bf16Reg: the
// register-staged bf16 kernel's [tap][Cin/32][Cout][32] at every shape (Bf16Train; as the data gradient's: flipped, the channel
// axes swapped, Cin' = dz_stride zero-extended).
enum class Packing { Hwio, Direct, Bf16, Split, Wino, Wino44, Bf16Reg, Count };
struct ConvPack {
    Packing kind = Packing::Hwio;
    int planes = 0;                  // Split: 3 or 2
    bool dgrad = false;              // the data gradient's packing: the kernel read as [k*k][cin][cout = dz_stride], axes swapped
    int k = 0, cin = 0, cout = 0;
    int wcout = 0;                   // the variable's Cout (a data gradient's packing zero-extends it to cout)
    size_t bytes() const;            // of the packing (0 for Hwio: the launch reads the variable)
    int launch(y3_ctx* ctx, const float* w, void* out) const;   // writes the packing of w (nothing for Hwio)
};
ConvPack y3_conv_pack(const y3_net& net, int i, const ConvRoute& r, bool dgrad = false);   // dgrad: r is y3_route_dgrad's

struct Buf {
    size_t off = SIZE_MAX, bytes = 0;
    bool ok() const { return off != SIZE_MAX; }
};

// Best-fit free list over one buffer: a released block merges with its neighbours, and a free block at the top goes back to
// the bump pointer.  dry: hand out offsets, touch nothing (sizing).
struct Arena {
    char* base = nullptr;
    size_t cap = 0, top = 0, peak = 0;
    bool dry = false;
    bool overflow = false;
    struct Free { size_t off, size; };
    std::vector<Free> fl;
    static size_t round(size_t b) { return (b + 255) & ~(size_t)255; }
    void reset(void* ws, size_t bytes, bool dry_) { base = static_cast<char*>(ws); cap = bytes; top = peak = 0; dry = dry_; overflow = false; fl.clear(); }
    void rewind(size_t to) { top = to; fl.clear(); }
    Buf alloc(size_t bytes) {
        bytes = round(bytes ? bytes : 1);
        size_t best = SIZE_MAX, best_size = SIZE_MAX;
        for (size_t f = 0; f < fl.size(); ++f)
            if (fl[f].size >= bytes && fl[f].size < best_size) { best = f; best_size = fl[f].size; }
        Buf b;
        b.bytes = bytes;
        if (best != SIZE_MAX) {
            b.off = fl[best].off;
            fl[best].off += bytes;
            fl[best].size -= bytes;
            if (fl[best].size == 0) fl.erase(fl.begin() + best);
        } else {
            b.off = top;
            top += bytes;
            peak = std::max(peak, top);
            if (!dry && top > cap) overflow = true;
        }
        return b;
    }
    void release(Buf& b) {
        if (!b.ok()) return;
        fl.push_back({b.off, b.bytes});
        std::sort(fl.begin(), fl.end(), [](const Free& x, const Free& y) { return x.off < y.off; });
        std::vector<Free> merged;
        for (const Free& f : fl) {
            if (!merged.empty() && merged.back().off + merged.back().size == f.off) merged.back().size += f.size;
            else merged.push_back(f);
        }
        if (!merged.empty() && merged.back().off + merged.back().size == top) {
            top = merged.back().off;
            merged.pop_back();
        }
        fl.swap(merged);
        b = Buf();
    }
    float* p(const Buf& b) const { return b.ok() && base ? reinterpret_cast<float*>(base + b.off) : nullptr; }   // (dry: null)
};

struct Tensor {
    int c;        // channels
    int sdiv;     // spatial divisor relative to the input (1,2,4,8,16,32)
    int last_use; // index of the last layer reading it (-1: never read)
    int ext;      // >=0: external output slot (fm1..fm3), storage provided by the caller
};

struct Layer {
    int k, stride, cin, cout, bn, act;
    int src, up, resid, dst;  // tensor ids (-1 = none)
    int c_up;
    int pool;                 // 1: the layer reads spp(src) (y3_spp_fwd), cin = 4 * channels(src); conv outputs stay the only tensors
    const float *scale, *shift;     // folded BN (detection convs: ones, bias), bound by y3_net_set_params
    const void* w[(int)Packing::Count];     // the kernel in every packing the inference routes may read (y3_net_set_params)
};

struct y3_train_state;                       // y3_net_train.hip: what a training forward leaves for loss / backward
void y3_train_state_free(y3_train_state* s);

struct y3_net {
    y3_ctx* ctx;
    int class_num;
    int arch = Y3_ARCH_YOLOV3;
    y3_train_state* train = nullptr;
    void* wgrad_stream = nullptr;   // y3_net_train_set_wgrad_stream: the weight gradients of backward run on this stream (nullptr: on the context's)
    int box_loss = Y3_BOX_MSE;      // y3_net_train_set_box_loss: the box term of the train step's loss, all three scales
    float ignore_thresh = 0.5f;     // y3_net_train_set_conf_rule: the ignore mask's threshold ...
    float obj_iou_ratio = 0.f;      // ... and r of the objectness target (1 - r) + r * IoU, all three scales
    void* own_stream = nullptr;     // the low-priority stream y3_net_train_set_wgrad_stream(net, Y3_OWN_STREAM) created (destroyed with the net)
    // y3_net_train_set_bn_sync: the host hook between the two halves of every BN finalize, and the caller's exchange buffer
    y3_bn_sync_fn bn_sync_fn = nullptr;
    void* bn_sync_user = nullptr;
    double* bn_sync_buf = nullptr;
    NetDtype dtype = NetDtype::F32;
    std::vector<Tensor> tensors;
    std::vector<Layer> layers;
    // cached plan
    int pn = 0, ph = 0, pw = 0;
    std::vector<size_t> offsets;  // byte offset of each tensor in the workspace (SIZE_MAX if external)
    std::vector<size_t> pool_offsets;   // per layer: its pooled input spp(src), alive for that layer only (SIZE_MAX: none)
    size_t plan_bytes = 0;    // arena + conv scratch + flag regions
    size_t arena_bytes = 0;   // activations only; the conv (stream-K) scratch follows at this offset
    size_t scratch_bytes = 0; // the largest scratch of the routes (shared by all layers: launches on one stream are ordered)
    std::vector<ConvRoute> routes;   // per layer, y3_route_infer
    size_t flags_bytes = 0;   // one region of FLAG_WORDS "partial published" words per layer, after the scratch:
                              // all regions are zeroed by ONE memset at the start of a forward
    static constexpr size_t FLAG_WORDS = 512;   // >= the largest stream-K grid (512 direct / 256 Winograd workers)
    // profiling: one set of (layers+1) events per profiled forward, averaged by y3_net_get_layer_ms
    bool profiling = false;
    std::vector<std::vector<hipEvent_t>> event_sets;
    size_t sets_used = 0;

    int add_conv(int src, int cout, int k, int stride = 1, bool bn = true, bool act = true, int resid = -1,
                 int up = -1, bool pool = false) {
        Layer l;
        l.k = k; l.stride = stride; l.cout = cout; l.bn = bn; l.act = act;
        l.src = src; l.up = up; l.resid = resid;
        l.c_up = up >= 0 ? tensors[up].c : 0;
        l.pool = pool ? 1 : 0;
        l.cin = pool ? 4 * tensors[src].c : tensors[src].c + l.c_up;
        l.scale = l.shift = nullptr;
        std::fill(std::begin(l.w), std::end(l.w), nullptr);
        Tensor t;
        t.c = cout; t.sdiv = tensors[src].sdiv * stride; t.last_use = -1; t.ext = -1;
        tensors.push_back(t);
        l.dst = (int)tensors.size() - 1;
        const int li = (int)layers.size();
        tensors[src].last_use = li;
        if (up >= 0) tensors[up].last_use = li;
        if (resid >= 0) tensors[resid].last_use = li;
        layers.push_back(l);
        return l.dst;
    }
    // utils/layer_utils.py:25-32
    int res_block(int x, int f) {
        const int a = add_conv(x, f, 1);
        return add_conv(a, 2 * f, 3, 1, true, true, /*resid=*/x);
    }
    // utils/layer_utils.py:71-79 ; `up` >= 0 means the input is concat([upsample(up), x]).  spp: the pooling block and one
    // more 1x1 conv, which reads it, behind the third conv (darknet's yolov3-spp.cfg)
    void yolo_block(int x, int f, int up, int* route, int* net, bool spp = false) {
        int t = add_conv(x, f, 1, 1, true, true, -1, up);
        t = add_conv(t, 2 * f, 3);
        t = add_conv(t, f, 1);
        if (spp) t = add_conv(t, f, 1, 1, true, true, -1, -1, /*pool=*/true);
        t = add_conv(t, 2 * f, 3);
        t = add_conv(t, f, 1);
        *route = t;
        *net = add_conv(t, 2 * f, 3);
    }
    void build() {
        tensors.clear(); layers.clear();
        tensors.push_back(Tensor{3, 1, -1, -1});
        // utils/layer_utils.py:34-68 darknet53_body
        int t = add_conv(0, 32, 3);
        t = add_conv(t, 64, 3, 2);
        t = res_block(t, 32);
        t = add_conv(t, 128, 3, 2);
        for (int i = 0; i < 2; ++i) t = res_block(t, 64);
        t = add_conv(t, 256, 3, 2);
        for (int i = 0; i < 8; ++i) t = res_block(t, 128);
        const int route1 = t;
        t = add_conv(t, 512, 3, 2);
        for (int i = 0; i < 8; ++i) t = res_block(t, 256);
        const int route2 = t;
        t = add_conv(t, 1024, 3, 2);
        for (int i = 0; i < 4; ++i) t = res_block(t, 512);
        const int route3 = t;
        // model.py:53-78 yolov3_head
        const int det = 3 * (5 + class_num);
        int inter1, net1, inter2, net2, inter3, net3;
        yolo_block(route3, 512, -1, &inter1, &net1, arch == Y3_ARCH_YOLOV3_SPP);
        const int fm1 = add_conv(net1, det, 1, 1, false, false);
        tensors[fm1].ext = 0;
        const int i1 = add_conv(inter1, 256, 1);
        yolo_block(route2, 256, i1, &inter2, &net2);
        const int fm2 = add_conv(net2, det, 1, 1, false, false);
        tensors[fm2].ext = 1;
        const int i2 = add_conv(inter2, 128, 1);
        yolo_block(route1, 128, i2, &inter3, &net3);
        const int fm3 = add_conv(net3, det, 1, 1, false, false);
        tensors[fm3].ext = 2;
    }

    // layer i at input n x h x w; train: as the train step runs it (the concat materialised, BN and activation applied apart)
    y3_conv_desc desc(int i, int n, int h, int w, bool train = false) const {
        const Layer& l = layers[i];
        const int sd = tensors[l.src].sdiv;
        return {n, h / sd, w / sd, l.cin, train ? 0 : l.c_up, l.cout, l.k, l.stride, train ? 0 : l.act};
    }

    // the channel stride of layer i's output gradient in the train step: Cout, the detection convs' padded to a multiple of 32
    int dz_stride(int i) const { return layers[i].bn ? layers[i].cout : ((3 * (5 + class_num) + 31) / 32) * 32; }

    // the widest channel count a layer reads or writes (the default graph: 1024; SPP: the pooled 2048)
    int max_channels() const {
        int m = 0;
        for (const Layer& l : layers) m = std::max({m, l.cin, l.cout});
        return m;
    }

    // spp(src) of a pool layer, in the element type of src
    size_t pool_bytes(int li, int n, int h, int w) const { return layers[li].pool ? 4 * tensor_bytes(layers[li].src, n, h, w) : 0; }

    size_t tensor_bytes(int id, int n, int h, int w) const {
        const Tensor& t = tensors[id];
        const size_t esize = (dtype == NetDtype::BF16 && t.ext < 0 && id != 0) ? 2 : sizeof(float);
        return (size_t)n * (h / t.sdiv) * (w / t.sdiv) * t.c * esize;
    }

    // Liveness-based arena: a tensor's bytes are recycled after its last reader has been launched
    // (same stream => ordered), keeping the working set small enough to sit in the 256 MB Infinity Cache
    // for the deeper layers.
    void plan(int n, int h, int w) {
        if (n == pn && h == ph && w == pw) return;
        Arena A;
        A.reset(nullptr, 0, true);
        std::vector<Buf> live(tensors.size());
        offsets.assign(tensors.size(), SIZE_MAX);
        pool_offsets.assign(layers.size(), SIZE_MAX);
        for (size_t li = 0; li < layers.size(); ++li) {
            const Layer& l = layers[li];
            for (size_t t = 1; t < tensors.size(); ++t)
                if (live[t].ok() && tensors[t].last_use < (int)li) A.release(live[t]);
            Buf pooled = l.pool ? A.alloc(pool_bytes((int)li, n, h, w)) : Buf();
            pool_offsets[li] = pooled.off;
            if (tensors[l.dst].ext < 0) {
                live[l.dst] = A.alloc(tensor_bytes(l.dst, n, h, w));
                offsets[l.dst] = live[l.dst].off;
            }
            A.release(pooled);
        }
        arena_bytes = Arena::round(A.peak);
        scratch_bytes = 0;
        routes.clear();
        for (size_t li = 0; li < layers.size(); ++li) {
            routes.push_back(y3_route_infer(*this, (int)li, n, h, w));
            scratch_bytes = std::max(scratch_bytes, routes.back().scratch);
        }
        scratch_bytes = (scratch_bytes + 255) & ~(size_t)255;
        flags_bytes = scratch_bytes ? layers.size() * FLAG_WORDS * sizeof(unsigned) : 0;
        plan_bytes = arena_bytes + scratch_bytes + flags_bytes;
        pn = n; ph = h; pw = w;
    }
};

